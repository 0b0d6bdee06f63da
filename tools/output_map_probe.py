#!/usr/bin/env python3
"""Cost of the output map (t41rx_set_output_map): one launch of the receive path through the device entry point on 4096
channels x 128 frames of SSB reading ONE shared input stream (every channel reads row 0: a receiver group), all arms of
a series interleaved in one process on one device (as tools/input_map_probe.py and tools/audio_rate_probe.py do).
hipEvents around each launch, after warm-up; median, min and max in us per launch, and the bytes of audio buffer the
arm's caller allocates (computed from the shapes).

One series per sample format (f32, q15) and AGC setting (off; AGCMode 1, the pipelined kernel).  The arms of a series:
  a_nomap        no output map
  b_identity     the identity output map (the fused twin, every channel listened)
  c_2_listened   2 of the channels listened (rows 0 and 1), the rest muted
  d_none         nobody listens, n_rows == 0, no audio buffer
  e_24k_2        arm c at 24 kS/s              e0_24k_nomap   its own arm without a map
  f_cw_2         arm c with the CW detector on f0_cw_nomap    its own arm without a map (the tap kernel hands over)
  g_ft8_2        arm c with FT8 receive on     g0_ft8_nomap   its own arm without a map
The order of the arms rotates from round to round, so that no arm always runs behind the same neighbour.

  python tools/output_map_probe.py [--channels 4096] [--frames 128] [--rounds 5] [--series REGEX] [--out FILE.json]
"""
import argparse
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def decode_fir():
    """a 64-tap low-pass for the detector: the probe times the stage, any finite table does"""
    import numpy as np
    n = np.arange(64) - 31.5
    return (np.sinc(n / 8.0) / 8.0 * np.hanning(64)).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--series", default=None, help="regular expression: run only the series it matches, e.g. 'f32/agc_off'")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("output_map_probe needs a HIP device")
    nch, nfr, L, D = a.channels, a.frames, 2048, 256
    nco = (np.random.default_rng(1000).integers(-860, 801, nch) * 50).astype(np.int32)  # config 2's tunings
    g = torch.Generator(device="cuda").manual_seed(0)
    I = (0.2 * torch.randn(1, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    Q = (0.2 * torch.randn(1, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    stream = torch.cuda.current_stream().cuda_stream
    two = np.full(nch, -1, np.int32)
    two[[nch // 3, (2 * nch) // 3]] = [0, 1]
    maps = {"a_nomap": None, "b_identity": (np.arange(nch, dtype=np.int32), nch), "c_2_listened": (two, 2),
            "d_none": (np.full(nch, -1, np.int32), 0), "e_24k_2": (two, 2), "e0_24k_nomap": None, "f_cw_2": (two, 2),
            "f0_cw_nomap": None, "g_ft8_2": (two, 2), "g0_ft8_nomap": None}
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch"}
    for fmt in ("f32", "q15"):
        dt, size = (torch.float32, 4) if fmt == "f32" else (torch.int16, 2)
        x, y = (I, Q) if fmt == "f32" else ((Q * 32768).to(torch.int16), (I * 32768).to(torch.int16))  # (the L queue carries Q)
        out = torch.empty(nch * nfr * L, dtype=dt, device="cuda")  # one buffer, the largest any arm needs
        for agc in (0, 1):
            series = "%s/agc_%s" % (fmt, "on" if agc else "off")
            if a.series and not re.search(a.series, series):
                continue
            arms = {}
            for name, m in maps.items():
                kw = dict(mode=0, FLoCut=200, FHiCut=3000, AGCMode=agc)
                if name.startswith("f"):
                    kw["xmtMode"] = 1
                rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
                rx.set_input_map(np.zeros(nch, np.int32), 1)
                if name.startswith("e"):
                    rx.set_audio_rate(24000)
                if name.startswith("f"):
                    rx.set_cw_tables(None, decode_fir())
                    rx.set_cw_detector(1, nfr)
                if name.startswith("g"):
                    rx.set_ft8_tables()
                    rx.set_ft8(1, nfr)
                    rx.ft8_sync()
                if m is not None:
                    rx.set_output_map(*m)
                arms[name] = rx
            entry = arms["a_nomap"]._lib.t41rx_process_device_q15 if fmt == "q15" else arms["a_nomap"]._lib.t41rx_process_device
            times = {k: [] for k in arms}
            order = list(arms)
            for r in range(a.warmup + a.rounds):
                for k in order[r % len(order):] + order[:r % len(order)]:
                    rx = arms[k]
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rc = entry(rx._ctx, x.data_ptr(), y.data_ptr(), out.data_ptr() if rx.audio_rows else None, nfr, stream)
                    e1.record()
                    e1.synchronize()
                    if rc != 0:
                        raise RuntimeError("libt41rx: %d %s" % (rc, rx._lib.t41rx_last_error().decode()))
                    if r >= a.warmup:
                        times[k].append(e0.elapsed_time(e1) * 1e3)
            for k, t in times.items():
                rx = arms[k]
                res["%s/%s" % (series, k)] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1),
                                              "audio_bytes": rx.audio_rows * nfr * rx.audio_frame_len * size}
            torch.cuda.synchronize()
            for rx in arms.values():
                rx.close()
    line = json.dumps(res)
    print(line)
    for k in sorted(res):
        if isinstance(res[k], dict):
            print("%-32s median %9.1f  min %9.1f  max %9.1f  us per launch   audio buffer %13d bytes"
                  % (k, res[k]["median"], res[k]["min"], res[k]["max"], res[k]["audio_bytes"]))
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
