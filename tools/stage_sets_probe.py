#!/usr/bin/env python3
"""Cost of parameter sets loaded next to the chain-splitting stages (t41rx_set_param_sets_ex with T41RX_SETS_STAGES):
one launch of the receive path through the device entry point on 4096 channels x 128 frames of SSB reading ONE shared input
stream (every channel reads row 0: a receiver group), in the manner of tools/nr_map_probe.py; the helpers are
tools/stage_map_probe.py's.  hipEvents around each launch, after warm-up; median, min and max in us per launch.

For each of three stages -- the noise blanker, the spectral noise reduction, the CW detector + decoder -- the arms:
  a  the stage on, no sets: every channel runs set 0
  b  staged sets, 3 sets, the channels dealt round-robin
  c  what a caller has without the feature: three contexts of a third of the channels each, one per set, with the stage
     on; the three launches' times summed
b against a is the surcharge of the sets; b against c is what the feature buys.  Under staged sets the noise reduction
always runs through the map's two launches (nrspec_sets_kernel / anr_map_kernel), so the spectral series' b against a
includes what the noise-reduction map's identity-like arm measures against the context-wide kernel.
The arms of a series rotate from round to round inside one process; every series runs in a child process of its own under
a time limit, one behind the other, and the first that fails ends the run.

  python tools/stage_sets_probe.py [--channels 4096] [--frames 128] [--rounds 5] [--out FILE.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from stage_map_probe import decode_fir, inputs, timed_launch, tunings  # noqa: E402

SERIES = ("blanker", "spectral", "cw")
BASE = dict(mode=0, FLoCut=200, FHiCut=3000)
EXTRA = [dict(mode=1, FLoCut=-3000, FHiCut=-200), dict(FLoCut=300, FHiCut=2400, audioVolume=40)]


def context(T, series, kw, nco, nfr):
    """a context of the series with the stage on, on one shared stream"""
    import numpy as np
    kw = dict(kw, xmtMode=1) if series == "cw" else dict(kw, nrOptionSelect=2) if series == "spectral" else kw
    rx = T.RxChain(len(nco), T.default_params(**kw), NCOFreq=nco)
    rx.set_input_map(np.zeros(len(nco), np.int32), 1)
    if series == "blanker":
        rx.set_noise_blanker(1)
    if series == "cw":
        rx.set_cw_tables(None, decode_fir())
        rx.set_cw_decode_tree(b"-" * 129)
        rx.set_cw_detector(1, nfr)
        rx.set_cw_decoder(1, nfr)
    return rx


def run_series(a):
    """the child: one series, its arms interleaved; prints one JSON line"""
    import numpy as np
    import torch
    import t41_sdr_amd as T
    series, nch, nfr = a.series, a.channels, a.frames
    nco = tunings(nch)
    setof = (np.arange(nch) % 3).astype(np.int32)
    sets = [dict(BASE, **e) for e in [{}] + EXTRA]
    arm_a = context(T, series, BASE, nco, nfr)
    arm_b = context(T, series, BASE, nco, nfr)
    extra = [dict(e, nrOptionSelect=2) for e in EXTRA] if series == "spectral" else EXTRA
    arm_b.set_param_sets(extra, setof, stages=True)
    assert arm_b.param_sets_stages
    arm_c = [context(T, series, sets[k], nco[setof == k], nfr) for k in range(3)]
    I, Q = inputs(nfr)
    out = torch.empty(nch * nfr * 2048, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    launch = {"a": lambda: timed_launch(arm_a, I, Q, out, nfr, stream), "b": lambda: timed_launch(arm_b, I, Q, out, nfr, stream),
              "c": lambda: sum(timed_launch(rx, I, Q, out, nfr, stream) for rx in arm_c)}
    arms = list(launch)
    for _ in range(a.warmup):
        for arm in arms:
            launch[arm]()
    us = {arm: [] for arm in arms}
    for r in range(a.rounds):
        for arm in arms[r % 3:] + arms[:r % 3]:
            us[arm].append(launch[arm]())
    print(json.dumps({"series": series, "us": us}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a series' child process may take")
    ap.add_argument("--series", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.series:
        return run_series(a)
    lines = ["# tools/stage_sets_probe.py: %d channels x %d frames of SSB on one shared stream, %d interleaved rounds, us per launch" % (a.channels, a.frames, a.rounds),
             "# a: the stage on, no sets; b: staged sets, 3 sets; c: three contexts of a third of the channels, summed",
             "series arm median min max"]
    for series in SERIES:
        cmd = [sys.executable, os.path.abspath(__file__), "--series", series, "--channels", str(a.channels), "--frames", str(a.frames),
               "--rounds", str(a.rounds), "--warmup", str(a.warmup)]
        child = subprocess.run(["timeout", "-k", "10", str(a.limit)] + cmd, capture_output=True, text=True)
        if child.returncode != 0:  # a failure ends the run: nothing more is started on the device
            sys.stderr.write(child.stdout + child.stderr)
            sys.exit("series %s: exit status %d; stopping" % (series, child.returncode))
        us = json.loads(child.stdout.strip().splitlines()[-1])["us"]
        med = {arm: statistics.median(v) for arm, v in us.items()}
        for arm, v in us.items():
            lines.append("%s %s %.1f %.1f %.1f" % (series, arm, med[arm], min(v), max(v)))
        lines.append("%s b/a %.3f b/c %.3f" % (series, med["b"] / med["a"], med["b"] / med["c"]))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
