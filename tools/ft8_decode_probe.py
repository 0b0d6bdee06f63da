#!/usr/bin/env python3
"""Cost of the FT8 decode of a finished slot (t41rx_ft8_decode_device: ft8_sync_kernel + ft8_ldpc_kernel) at 4096 channels,
beside the receive time of the slot it decodes.

Three waterfalls, every channel its own:
  quiet   all zero: no entry reaches kMin_score, no candidates
  noise   uniform bytes: about 12 700 qualifying entries per channel, the heap full, 20 failed bp_decode() runs of 10
          iterations each
  signal  three transmissions of different levels over byte noise 0..19 (the tests' encoder, tests/ft8_codec.py), each
          channel at its own offsets
hipEvents around each decode call, after warm-up; median, min and max in us per call.  Beside them the receive path of the
same context with the FT8 stage on (tools/ft8_probe.py's arm `on`), timed at --frames frames per launch and scaled to
the 1380 frames of a slot.  No threshold: the figures go into README.md and DESIGN.md.

  python tools/ft8_decode_probe.py [--channels 4096] [--frames 128] [--rounds 10] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    import ft8_codec as Cd
    import ft8_decode_model as D
    if not torch.cuda.is_available():
        raise SystemExit("ft8_decode_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    rx = T.RxChain(nch, T.default_params(mode=0))
    t = D.tables()
    rx.set_ft8_decode_tables(t.costas, t.gray, t.nm, t.mn, t.nrw)
    rx.set_ft8_tables()
    rx.set_ft8(1, nfr)
    rx.ft8_sync()
    g = torch.Generator(device="cuda").manual_seed(2)
    falls = {"quiet": torch.zeros(nch, D.SLOT_BYTES, dtype=torch.uint8, device="cuda"),
             "noise": torch.randint(0, 256, (nch, D.SLOT_BYTES), dtype=torch.uint8, device="cuda", generator=g)}
    # three transmissions per channel over weak noise: painted on the host for 64 patterns, repeated over the channels
    msgs = [Cd.encode(Cd.pack_standard(*m))[0] for m in (("CQ", "K1ABC", "FN42"), ("W9XYZ", "K1ABC", "-12"), ("K1ABC", "W9XYZ", "RR73"))]
    rng = np.random.default_rng(3)
    pat = []
    for _ in range(min(nch, 64)):
        w = rng.integers(0, 20, (D.NUM_BLOCKS, 4, D.NUM_BINS)).astype(np.uint8)
        for tones, level, f0 in zip(msgs, (150, 110, 90), (60, 160, 260)):
            Cd.paint(w, tones, int(rng.integers(-7, 20)), f0 + int(rng.integers(0, 80)), int(rng.integers(0, 4)), level, 40)
        pat.append(w.reshape(-1))
    pat = torch.from_numpy(np.array(pat)).cuda()
    falls["signal"] = pat[torch.arange(nch, device="cuda") % pat.shape[0]].contiguous()
    # the receive path of the same context, FT8 stage on (as tools/ft8_probe.py)
    n = torch.arange(nfr * 2048, device="cuda", dtype=torch.float32)
    ph = 2 * torch.pi * (47000.0 / 192000.0) * n
    I = (0.1 * torch.cos(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    Q = (0.1 * torch.sin(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    out = torch.empty_like(I)
    import ctypes as C
    res = torch.zeros(nch, T.ft8.RESULT.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    times = {k: [] for k in list(falls) + ["receive"]}
    found = {}
    for r in range(a.warmup + a.rounds):
        for k in times:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if k == "receive":
                rx.ProcessIQData(I, Q, out=out)
            else:
                T._lib.check(rx._lib.t41rx_ft8_decode_device(rx._ctx, C.c_void_p(falls[k].data_ptr()), D.SLOT_BYTES, None, nch,
                                                             C.c_void_p(res.data_ptr()), C.c_void_p(stream)))
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
            if k != "receive" and r == 0:
                rec = res.cpu().numpy().view(T.ft8.RESULT).reshape(nch)
                found[k] = {"candidates_per_channel": round(float(rec["num_candidates"].mean()), 2),
                            "valid_per_channel": round(float(rec["num_valid"].mean()), 2),
                            "messages_per_channel": round(float(np.mean([len(m) for m in T.ft8.messages(rec[:64])])), 2)}
    out_d = {"channels": nch, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per call", "found": found}
    for k, v in times.items():
        out_d[k] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    out_d["receive"]["frames"] = nfr
    out_d["receive_1380_frames"] = round(out_d["receive"]["median"] * 1380.0 / nfr, 1)
    line = json.dumps(out_d)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
