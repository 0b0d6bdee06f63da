#!/usr/bin/env python3
"""Cost of the display FFT side output: one ProcessIQData() call of the SSB chain with the side output off, at spectrumZoom 0
and at spectrumZoom 2 on the same shape, interleaved in one process on one device.  hipEvents around each call, after
warm-up; median, min and max in microseconds per call; the side output's own cost is an arm's median minus the off arm's.

  python tools/display_probe.py [--channels 4096] [--frames 8] [--rounds 15] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("display_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    g = torch.Generator(device="cuda").manual_seed(1)
    I = (0.1 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    Q = (0.1 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    out = torch.empty_like(I)
    arms, keep = {}, []
    for name, zoom in (("off", None), ("zoom0", 0), ("zoom2", 2)):
        rx = T.RxChain(nch, T.default_params(mode=0, FLoCut=200, FHiCut=3000))
        if zoom is not None:
            spec = torch.zeros(nch, nfr, 512, device="cuda")
            old = torch.zeros_like(spec)
            rx.set_display_spectrum(spec, old, zoom)
            keep.append((spec, old))
        arms[name] = rx
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.rounds):
        for k, rx in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rx.ProcessIQData(I, Q, out=out)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per call"}
    for k, t in times.items():
        res[k] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
