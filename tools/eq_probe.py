#!/usr/bin/env python3
"""Cost of the receive equalizer: the path at 4096 channels x 128 frames, USB, timed interleaved in one process --
EQ off, EQ on, EQ + noise reduction (Kim) + noise blanker -- in us per launch and per frame (launch time / frames).

usage: python tools/eq_probe.py [--channels 4096] [--frames 128] [--reps 10]
The equalizer kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/eq_probe.py ...`
run.  The band table is the test fixture tests/golden/eq/rx_eq_bands.npz (the firmware's EQ_Band1Coeffs .. EQ_Band14Coeffs).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch
    import t41_sdr_amd as T
    nch, nfr = a.channels, a.frames
    table = np.load(os.path.join(ROOT, "tests", "golden", "eq", "rx_eq_bands.npz"))["coeffs_f32"]
    levels = [0, 15, 30, 0, 61, 77, 92, 108, 0, 138, 154, 169, 185, 200]
    g = torch.Generator(device="cuda").manual_seed(1)
    I = 0.05 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)
    Q = 0.05 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)
    out = torch.empty_like(I)
    nco = [(-20000 + 37 * c) % 40000 - 20000 for c in range(nch)]
    cfg = {"eq_off": (dict(), 0, 0), "eq_on": (dict(), 1, 0), "eq_kim_nb": (dict(nrOptionSelect=1), 1, 1)}
    chains = {}
    for k, (kw, eq, nb) in cfg.items():
        rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
        rx.set_receive_eq_bands(table)
        rx.set_receive_eq(eq, levels)
        rx.set_noise_blanker(nb)
        rx.ProcessIQData(I, Q, out=out)  # warm-up (allocations, first launch)
        chains[k] = rx
    torch.cuda.synchronize()
    times = {k: [] for k in cfg}
    for _ in range(a.reps):
        for k, rx in chains.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            rx.ProcessIQData(I, Q, out=out)
            e.record()
            torch.cuda.synchronize()
            times[k].append(s.elapsed_time(e) * 1e3)  # us per launch
    res = {k: dict(us_per_launch_median=sorted(v)[len(v) // 2], us_per_frame_median=sorted(v)[len(v) // 2] / nfr,
                   us_per_launch_min=min(v)) for k, v in times.items()}
    res["eq_stage_us_per_launch_median"] = res["eq_on"]["us_per_launch_median"] - res["eq_off"]["us_per_launch_median"]
    res["shape"] = dict(channels=nch, frames=nfr, reps=a.reps, mode="USB")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
