#!/usr/bin/env python3
"""Cost of the receive noise blanker: the path at 4096 channels x 128 frames, USB, timed interleaved in one process --
NB off, NB on, noise reduction (Kim) + NB -- in us per frame (per channel-frame of the batch: launch time / frames).

usage: python tools/nb_probe.py [--channels 4096] [--frames 128] [--reps 10]
The blanker kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats -- python tools/nb_probe.py ...` run.
Algorithmic bytes of the stage: 256 f32 read + 256 f32 written per channel-frame (2 KiB).
"""
import argparse
import json
import os
import sys

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
    g = torch.Generator(device="cuda").manual_seed(1)
    I = 0.05 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)
    Q = 0.05 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)
    out = torch.empty_like(I)
    nco = [(-20000 + 37 * c) % 40000 - 20000 for c in range(nch)]
    cfg = {"nb_off": (dict(), 0), "nb_on": (dict(), 1), "kim_nb": (dict(nrOptionSelect=1), 1)}
    chains = {}
    for k, (kw, nb) in cfg.items():
        rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
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
    res["nb_stage_us_per_launch_median"] = res["nb_on"]["us_per_launch_median"] - res["nb_off"]["us_per_launch_median"]
    stage_bytes = nch * nfr * 256 * 4 * 2
    res["nb_stage_algorithmic_bytes"] = stage_bytes
    res["nb_stage_bytes_per_us_at_that_cost"] = stage_bytes / max(res["nb_stage_us_per_launch_median"], 1e-9)
    res["shape"] = dict(channels=nch, frames=nfr, reps=a.reps, mode="USB")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
