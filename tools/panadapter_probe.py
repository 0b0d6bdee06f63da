#!/usr/bin/env python3
"""Cost of the panadapter stage next to the two side outputs it replaces: one launch of the receive path (USB, fixed gain,
f32) on `channels` x `frames`, with

  a        no side output
  b        t41rx_set_display_spectrum + t41rx_set_audio_spectrum: every frame a display frame (the way to a display before)
  c        the stage at update_period 1
  d        the stage at update_period 16
  e        the stage at update_period = frames: one row per launch
  f        the stage at a period that flags no frame

The arms are interleaved in one process on one device, `rounds` times after warm-up; hipEvents around each launch.
Printed: every round's times, the medians and the spread (max - min) of the rounds, and the device memory each arm's
context and buffers took (hipMemGetInfo around their creation).  --arms picks a subset: a library without the stage
(T41RX_LIB=...) can run a and b.

  python tools/panadapter_probe.py [--channels 4096] [--frames 128] [--rounds 5] [--zoom 0] [--arms a,b,c,...] [--out FILE.json]
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
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--zoom", type=int, default=0)
    ap.add_argument("--arms", default="a,b,c,d,e,f")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("panadapter_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    g = torch.Generator(device="cuda").manual_seed(1)
    n = torch.arange(nfr * 2048, device="cuda", dtype=torch.float32)
    ph = 2 * torch.pi * (47000.0 / 192000.0) * n
    I = (0.1 * torch.cos(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    Q = (0.1 * torch.sin(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    out = torch.empty_like(I)
    gradient = np.load(os.path.join(ROOT, "tests", "golden", "display", "gradient.npz"))["gradient"]
    keep, held, arms = [], {}, {}

    def stage(period, phase, rows):
        rx = T.RxChain(nch, T.default_params(mode=0))
        rx.set_panadapter_tables(gradient)
        keep.append(rx.set_panadapter(True, spectrumZoom=a.zoom, update_period=period, update_phase=phase, max_rows=rows))
        return rx

    def make(name):
        if name == "a":
            return T.RxChain(nch, T.default_params(mode=0))
        if name == "b":
            rx = T.RxChain(nch, T.default_params(mode=0))
            bufs = (torch.zeros(nch, nfr, 512, device="cuda"), torch.zeros(nch, nfr, 512, device="cuda"),
                    torch.zeros(nch, nfr, 1024, device="cuda"), torch.zeros(nch, nfr, 3, device="cuda"))
            rx.set_display_spectrum(bufs[0], bufs[1], a.zoom)
            rx.set_audio_spectrum(bufs[2], bufs[3])
            keep.append(bufs)
            return rx
        if name == "c":
            return stage(1, 0, nfr)
        if name == "d":
            return stage(16, 0, (nfr + 15) // 16)
        if name == "e":
            return stage(nfr, 0, 1)
        if name == "f":
            return stage(1 << 30, 1 << 29, 1)
        raise SystemExit("unknown arm %r" % name)

    for name in a.arms.split(","):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        rx = make(name)
        torch.cuda.synchronize()
        held[name] = round((free0 - torch.cuda.mem_get_info()[0]) / 2.0**20, 1)

        arms[name] = lambda rx=rx: rx.ProcessIQData(I, Q, out=out)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    rounds = []
    for r in range(a.warmup + a.rounds):
        t = {k: round(timed(fn), 1) for k, fn in arms.items()}
        if r >= a.warmup:
            rounds.append(t)
    res = {"channels": nch, "frames": nfr, "zoom": a.zoom, "rounds": rounds, "device": torch.cuda.get_device_name(0),
           "library": T.LIB_PATH, "unit": "us per launch; held_MiB = device memory the arm's context and buffers took", "held_MiB": held}
    for k in arms:
        v = [x[k] for x in rounds]
        res[k] = {"median": round(statistics.median(v), 1), "min": min(v), "max": max(v), "spread": round(max(v) - min(v), 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
