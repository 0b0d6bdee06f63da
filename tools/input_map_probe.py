#!/usr/bin/env python3
"""Cost of receiver groups (t41rx_set_input_map): one launch of the receive path through the device entry point on
4096 channels x 128 frames, with no map, the identity map, and 1, 8 and 64 shared streams, all arms interleaved in one
process on one device (as tools/ab_probe.py interleaves builds).  hipEvents around each launch, after warm-up; median,
min and max in us per launch.  Two arms run without a map (`none`, `none_b`): the distance between them is the spread a
mapped arm has to exceed before it says anything.  Shapes: USB with the AGC off on f32 samples, the same with AGCMode 1
(the pipelined kernel), and on q15 samples.

A map with n_streams rows puts channels c * n_streams // n_channels on one row: the 16 waves of a workgroup read the
same row (`--scatter` maps channel c to row c % n_streams instead).  The mapped arms read the first n_streams rows of
the unmapped arms' buffers.

  python tools/input_map_probe.py [--channels 4096] [--frames 128] [--rounds 10] [--streams 1,8,64] [--scatter] [--arms REGEX] [--out FILE.json]
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
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", default="1,8,64")
    ap.add_argument("--scatter", action="store_true", help="channel c reads row c %% n_streams")
    ap.add_argument("--arms", default=None, help="regular expression: run only the arms it matches, e.g. 'usb_agc/(none|streams_8)$' "
                                                 "(a counter run under rocprofv3 --pmc takes one arm per process)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("input_map_probe needs a HIP device")
    nch, nfr, L = a.channels, a.frames, 2048
    counts = [int(s) for s in a.streams.split(",")]
    nco = (np.random.default_rng(1000).integers(-860, 801, nch) * 50).astype(np.int32)  # config 2's tunings
    g = torch.Generator(device="cuda").manual_seed(0)
    I = (0.2 * torch.randn(nch, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    Q = (0.2 * torch.randn(nch, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    Iq, Qq = (I * 32768.0).to(torch.int16), (Q * 32768.0).to(torch.int16)
    out, outq = torch.empty_like(I), torch.empty_like(Iq)

    def smap(ns):
        c = np.arange(nch, dtype=np.int64)
        return (c % ns if a.scatter else c * ns // nch).astype(np.int32)

    arms = {}
    for shape, kw, q15 in (("usb", dict(mode=0), False), ("usb_agc", dict(mode=0, AGCMode=1), False), ("usb_q15", dict(mode=0), True)):
        for name, m in [("none", None), ("none_b", None), ("identity", np.arange(nch, dtype=np.int32))] + [("streams_%d" % n, smap(n)) for n in counts]:
            if a.arms and not re.search(a.arms, "%s/%s" % (shape, name)):
                continue
            rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
            rows = nch
            if m is not None:
                rx.set_input_map(m)
                rows = rx.n_streams
            x, y = (Qq, Iq) if q15 else (I, Q)  # (q15: I comes from the R queue)
            arms["%s/%s" % (shape, name)] = (rx, x[:rows], y[:rows], outq if q15 else out, q15)
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.rounds):
        for k, (rx, x, y, o, q15) in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            if q15:
                rx.ProcessIQData_q15(x, y, out=o)
            else:
                rx.ProcessIQData(x, y, out=o)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch",
           "map": "channel c -> row c % n_streams" if a.scatter else "channel c -> row c * n_streams // n_channels"}
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
