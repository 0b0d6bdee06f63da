#!/usr/bin/env python3
"""Cost of the CW exciter: one launch of CW_ExciterIQData() through the device entry point (key = NULL and with a random
key) and one launch of the SSB exciter (equaliser off) on the same shape, interleaved in one process on one device.
hipEvents around each launch, after warm-up; median, min and max, and the store bandwidth the median stands for (both
kernels write 8 KiB per channel and frame; the SSB exciter also reads 4 KiB).

  python tools/cw_tx_probe.py [--channels 4096] [--frames 32] [--rounds 25] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd._lib import check
    if not torch.cuda.is_available():
        raise SystemExit("cw_tx_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    # the SSB arm's microphone: speech-band tones + noise at about half scale, made on the device
    g = torch.Generator(device="cuda").manual_seed(1)
    n = torch.arange(nfr * 2048, device="cuda", dtype=torch.float32)
    f = torch.rand(nch, 1, device="cuda", generator=g) * 2500.0 + 300.0
    x = 0.4 * torch.sin(2 * torch.pi * f / 192000.0 * n) + 0.05 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)
    x = (x * 32768.0).clamp(-32768, 32767).to(torch.int16).contiguous()
    key = (torch.rand(nch, nfr * 16, device="cuda", generator=g) < 0.5).to(torch.uint8).contiguous()
    ssb, cw, cwk = T.TxChain(nch), T.TxChain(nch), T.TxChain(nch)
    for tx in (cw, cwk):
        tx.set_cw_tone(*T.sine_tone(8))
    oL, oR = torch.empty_like(x), torch.empty_like(x)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lib = ssb._lib
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    arms = {"ssb_eq_off": lambda: lib.t41tx_process_device_q15(ssb._ctx, vp(x), None, vp(oL), vp(oR), nfr, stream),
            "cw": lambda: lib.t41tx_process_cw_device_q15(cw._ctx, None, vp(oL), vp(oR), nfr, stream),
            "cw_keyed": lambda: lib.t41tx_process_cw_device_q15(cwk._ctx, vp(key), vp(oL), vp(oR), nfr, stream)}
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.rounds):
        for k, launch in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(launch())
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch"}
    stored = 2 * 2 * 2048 * nfr * nch  # bytes
    for k, t in times.items():
        med = statistics.median(t)
        res[k] = {"median": round(med, 1), "min": round(min(t), 1), "max": round(max(t), 1), "per_frame": round(med / nfr, 2),
                  "store_GB_per_s": round(stored / med / 1e3, 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
