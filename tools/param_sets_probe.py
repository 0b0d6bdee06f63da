#!/usr/bin/env python3
"""Cost of parameter sets (t41rx_set_param_sets): one launch of the receive path through the device entry point on
4096 channels x 128 frames of SSB, all arms interleaved in one process on one device (as tools/input_map_probe.py
does).  hipEvents around each launch, after warm-up; median, min and max in us per launch.  Arms: no sets twice (`none`,
`none_b`: their distance is the spread an arm has to exceed before it says anything), the identity input map alone
(what the set kernels are twins of: the arms with sets are to be compared with THIS arm), one extra set equal to set 0,
and 2, 8 and 64 distinct pass bands.  The same with AGCMode 1 (the pipelined kernel, whose duty wave reads the
constants of the channel it serves per lane).

k pass bands: set j is USB FLoCut 200, FHiCut 3000 - 30 j (distinct masks, levels and resampler taps), channel c runs set
c % k -- the 16 waves of a workgroup run 16 different sets where there are that many.

  python tools/param_sets_probe.py [--channels 4096] [--frames 128] [--rounds 5] [--sets 2,8,64] [--arms REGEX] [--out FILE.json]
"""
import argparse
import json
import os
import re
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
    ap.add_argument("--sets", default="2,8,64")
    ap.add_argument("--arms", default=None, help="regular expression: run only the arms it matches, e.g. 'usb/(identity|sets_64)$' "
                                                 "(a counter run under rocprofv3 --pmc takes one arm per process)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("param_sets_probe needs a HIP device")
    nch, nfr, L = a.channels, a.frames, 2048
    counts = [int(s) for s in a.sets.split(",")]
    nco = (np.random.default_rng(1000).integers(-860, 801, nch) * 50).astype(np.int32)  # config 2's tunings
    g = torch.Generator(device="cuda").manual_seed(0)
    I = (0.2 * torch.randn(nch, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    Q = (0.2 * torch.randn(nch, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    out = torch.empty_like(I)
    chan = np.arange(nch, dtype=np.int64)

    def bands(k):  # k pass bands in all: set 0 and k - 1 extra ones
        return [dict(FHiCut=3000 - 30 * j) for j in range(1, k)], (chan % k).astype(np.int32)

    arms = {}
    for shape, kw in (("usb", dict(mode=0, FLoCut=200, FHiCut=3000)), ("usb_agc", dict(mode=0, FLoCut=200, FHiCut=3000, AGCMode=1))):
        plan = [("none", None), ("none_b", None), ("identity", "map"), ("same_1", ([{}], (chan % 2).astype(np.int32)))]
        plan += [("sets_%d" % k, bands(k)) for k in counts]
        for name, what in plan:
            if a.arms and not re.search(a.arms, "%s/%s" % (shape, name)):
                continue
            rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
            if what == "map":
                rx.set_input_map(np.arange(nch, dtype=np.int32))
            elif what is not None:
                rx.set_param_sets(*what)
            arms["%s/%s" % (shape, name)] = rx
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
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch",
           "sets": "k pass bands: USB 200 .. 3000 - 30 j Hz, channel c -> set c % k"}
    for k, t in times.items():
        res[k] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1),
                  "per_frame": round(statistics.median(t) / nfr, 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
