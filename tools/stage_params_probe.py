#!/usr/bin/env python3
"""Cost of the stage parameters per channel (t41rx_set_cw_filter_map, t41rx_set_receive_eq_map): one launch of the receive
path through the device entry point on 4096 channels x 128 frames reading ONE shared input stream (every channel reads
row 0: a receiver group), all arms of a series interleaved in one process on one device, in the manner of
tools/stage_map_probe.py, whose helpers this uses.  hipEvents around each launch, after warm-up; median, min and max in us
per launch.

Series `filter`, a CW context (xmtMode CW_MODE, no detector):
  a_off          the narrow filter off (context-wide index 5)
  b_ctx2         context-wide CWFilterIndex 2: cw_filter_kernel + cw_back_kernel
  b_parent       the same on the parent commit's build (--parent-lib), where given: a child process that loads that
                 library, holds its context and runs one launch whenever this process tells it to, inside the rotation
  c_map2         a uniform map of 2: the map form of the filter over all channels + cw_back_kernel
  d_half         every other channel 2, the others 5: the map form over half + both back kernels
  e_2_filtered   2 of the channels filtered
  f_all5         a map of 5s: plans as the filter off
Series `eq`, an SSB context with the receive equalizer on:
  a_ctx          context-wide levels: eq_kernel
  a_parent       the same on the parent commit's build
  b_map1         a level map with one vector for every channel: eq_levels_kernel
  c_map64        a level map with 64 distinct vectors
The order of the arms rotates from round to round, so that no arm always runs behind the same neighbour.

  python tools/stage_params_probe.py [--channels 4096] [--frames 128] [--rounds 5] [--series REGEX] [--parent-lib LIB] [--out FILE.json]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from stage_map_probe import eq_bands, inputs, timed_launch, tunings  # noqa: E402

SERIES = ("filter", "eq")
NEW = ("t41rx_set_cw_filter_map", "t41rx_get_cw_filter_map", "t41rx_set_receive_eq_map", "t41rx_get_receive_eq_map")


def cw_filters():
    """5 x 6 stable low-pass sections {b0, b1, b2, -a1, -a2}: the probe times the stage, any finite stable table does"""
    import numpy as np
    t = np.zeros((5, 6, 5), np.float32)
    for f in range(5):
        for s in range(6):
            w = 2 * np.pi * (800.0 + 250.0 * f) / 24000.0
            r = 0.90 + 0.015 * s
            t[f, s] = [0.05, 0.1, 0.05, 2 * r * np.cos(w), -r * r]
    return t


def make_chain(T, series, nch, nco, index=5):
    """a context of the series on one shared stream: the CW context with this context-wide index, or the equalizer on"""
    import numpy as np
    kw = dict(mode=0, FLoCut=200, FHiCut=3000)
    if series == "filter":
        kw["xmtMode"] = 1
    rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
    rx.set_input_map(np.zeros(nch, np.int32), 1)
    if series == "filter":
        rx.set_cw_tables(cw_filters(), None)
        rx.set_cw_filter(index)
    else:
        rx.set_receive_eq_bands(eq_bands())
        rx.set_receive_eq(1)
    return rx


def serve(a):
    """the child: the library T41RX_LIB names (the parent commit's), one context per series -- context-wide filter 2, or
    the equalizer with its context-wide levels; a line `series` on stdin runs one launch and answers its microseconds"""
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd import _lib
    for name in NEW:  # (the parent's library has no such entry to bind)
        _lib.SYMBOLS.pop(name, None)
    nch, nfr = a.channels, a.frames
    I, Q = inputs(nfr)
    out = torch.empty(nch * nfr * 2048, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    chains = {}
    print("ready %s" % T.LIB_PATH, flush=True)
    for line in sys.stdin:
        series = line.strip()
        if series == "quit":
            break
        if series not in chains:
            for rx in chains.values():  # one series at a time, as in the parent process
                rx.close()
            chains = {series: make_chain(T, series, nch, tunings(nch), 2)}
        print("%.1f" % timed_launch(chains[series], I, Q, out, nfr, stream), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--series", default=None, help="regular expression: run only the series it matches, e.g. 'eq'")
    ap.add_argument("--parent-lib", default=None, help="libt41rx.so built from the parent commit: adds the parent's arm")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.serve:
        return serve(a)
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("stage_params_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    nco = tunings(nch)
    I, Q = inputs(nfr)
    out = torch.empty(nch * nfr * 2048, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    child = None
    if a.parent_lib:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", "--channels", str(nch), "--frames", str(nfr)],
                                 env=dict(os.environ, T41RX_LIB=os.path.abspath(a.parent_lib)), stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        hello = child.stdout.readline().split()
        if hello[:1] != ["ready"] or os.path.abspath(hello[1]) != os.path.abspath(a.parent_lib):
            raise SystemExit("the child did not load %s: %r" % (a.parent_lib, hello))

    def filter_arms():
        half = np.where(np.arange(nch) % 2 == 0, 2, 5).astype(np.int32)
        two = np.full(nch, 5, np.int32)
        two[[nch // 3, nch - 1 - nch // 7]] = 2
        arms = {"a_off": make_chain(T, "filter", nch, nco, 5), "b_ctx2": make_chain(T, "filter", nch, nco, 2)}
        for name, m in (("c_map2", np.full(nch, 2, np.int32)), ("d_half", half), ("e_2_filtered", two), ("f_all5", np.full(nch, 5, np.int32))):
            arms[name] = make_chain(T, "filter", nch, nco, 5)
            arms[name].set_cw_filter_map(m)
        return arms, "b_parent"

    def eq_arms():
        rng = np.random.default_rng(7)
        vectors = rng.integers(0, 201, (64, 14)).astype(np.int32)
        arms = {"a_ctx": make_chain(T, "eq", nch, nco)}
        for name, lv in (("b_map1", np.full((nch, 14), 100, np.int32)), ("c_map64", vectors[np.arange(nch) % 64])):
            arms[name] = make_chain(T, "eq", nch, nco)
            arms[name].set_receive_eq_map(lv)
        return arms, "a_parent"

    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch",
           "parent_lib": bool(child)}
    try:
        for series, make in (("filter", filter_arms), ("eq", eq_arms)):
            if a.series and not re.search(a.series, series):
                continue
            arms, parent_arm = make()
            order = list(arms) + ([parent_arm] if child else [])
            times = {k: [] for k in order}
            for r in range(a.warmup + a.rounds):
                for k in order[r % len(order):] + order[:r % len(order)]:
                    if k == parent_arm:
                        child.stdin.write(series + "\n")
                        child.stdin.flush()
                        t = float(child.stdout.readline())
                    else:
                        t = timed_launch(arms[k], I, Q, out, nfr, stream)
                    if r >= a.warmup:
                        times[k].append(t)
            for k, t in times.items():
                res["%s/%s" % (series, k)] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
            torch.cuda.synchronize()
            for rx in arms.values():
                rx.close()
    finally:
        if child:
            try:
                child.stdin.write("quit\n")
                child.stdin.flush()
            except OSError:
                pass
            child.wait(timeout=60)
    line = json.dumps(res)
    print(line)
    for k in sorted(res):
        if isinstance(res[k], dict):
            print("%-24s median %9.1f  min %9.1f  max %9.1f  us per launch" % (k, res[k]["median"], res[k]["min"], res[k]["max"]))
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
