#!/usr/bin/env python3
"""Cost of the beacon monitor stage behind the panadapter: one launch of the receive path (USB, fixed gain, f32) on
`channels` x `frames` with the panadapter at update_period `period` (smeter rows only), and

  pan      the panadapter alone
  mode0    with the beacon stage in mode 0 (the firmware's cycle)
  mode1    with the beacon stage in mode 1 (continuous)
  norow    the beacon stage on and the panadapter at a period that flags no frame of the launch

The arms are interleaved in one process on one device, `rounds` times after warm-up; hipEvents around each launch.
Printed: every round's times, and per arm the median and the spread (max - min) of the rounds.  --arms picks a subset:
copied into the tools/ of a checkout without the stage, `--arms pan` gives that tree's figure on the same box (the
package binds every declared symbol at load, so an older library does not load under this tree's Python).

The structural condition -- a call without an update frame launches no beacon kernel -- is checked, not timed: the events
and the status words of arm `norow` must be the ones the switch left after every launch.

  python tools/beacon_probe.py [--channels 4096] [--frames 128] [--period 16] [--rounds 5] [--arms pan,mode0,...] [--out FILE.json]
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
    ap.add_argument("--period", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arms", default="pan,mode0,mode1,norow")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("beacon_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    g = torch.Generator(device="cuda").manual_seed(1)
    n = torch.arange(nfr * 2048, device="cuda", dtype=torch.float32)
    ph = 2 * torch.pi * (47000.0 / 192000.0) * n
    I = (0.1 * torch.cos(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    Q = (0.1 * torch.sin(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    out = torch.empty_like(I)
    gradient = np.load(os.path.join(ROOT, "tests", "golden", "display", "gradient.npz"))["gradient"]
    rows = (nfr + a.period - 1) // a.period
    keep, arms, norow = [], {}, None

    def make(name):
        rx = T.RxChain(nch, T.default_params(mode=0))
        rx.set_panadapter_tables(gradient)
        if name == "norow":
            keep.append(rx.set_panadapter(True, update_period=1 << 30, update_phase=1 << 29, max_rows=1, outputs=["smeter"]))
        else:
            keep.append(rx.set_panadapter(True, update_period=a.period, max_rows=rows, outputs=["smeter"]))
        if name != "pan":
            rx.set_beacon_clock(0, 1000, 1)  # a slot change every ten frames: records in every launch
            keep.append(rx.set_beacon(True, 1 if name == "mode1" else 0, np.arange(nch) % 5))
        return rx

    for name in a.arms.split(","):
        if name not in ("pan", "mode0", "mode1", "norow"):
            raise SystemExit("unknown arm %r" % name)
        rx = make(name)
        if name == "norow":
            norow = (rx, rx.beacon_status().copy(), keep[-1][1].clone())
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
    res = {"channels": nch, "frames": nfr, "period": a.period, "rows_per_launch": rows, "rounds": rounds,
           "device": torch.cuda.get_device_name(0), "library": T.LIB_PATH, "unit": "us per launch"}
    for k in arms:
        v = [x[k] for x in rounds]
        res[k] = {"median": round(statistics.median(v), 1), "min": min(v), "max": max(v), "spread": round(max(v) - min(v), 1)}
    if norow is not None:
        rx, status, events = norow
        same = bool((rx.beacon_status() == status).all()) and bool((rx._beacon[1] == events).all()) and not rx.beacon_snr().any()
        res["norow_launched_no_beacon_kernel"] = same
        if not same:
            raise SystemExit("a call without an update frame changed the beacon stage's words: " + json.dumps(res))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
