#!/usr/bin/env python3
"""Cost of the noise-reduction map (t41rx_set_nr_map): one launch of the receive path through the device entry point on
4096 channels x 128 frames of SSB reading ONE shared input stream (every channel reads row 0: a receiver group), all arms
interleaved in one process on one device, in the manner of tools/stage_params_probe.py; the helpers are
tools/stage_map_probe.py's.  hipEvents around each launch, after warm-up; median, min and max in us per launch.

The arms without a noise-reduction map run on the parent commit's build where --parent-lib names it (a child process that
loads that library through T41RX_LIB, holds its contexts and runs one launch whenever this process tells it to, inside the
rotation), else on this build:
  a_off            noise reduction off
  b_kim2           context-wide Kim1_NR() with a stage map listing 2 channels: the parent's way to run one kind on a few
  b_spectral2      the same with SpectralNoiseReduction()
  b_lms2           the same with Xanr() as LMS noise reduction
  b_notch2         the same with Xanr() as the automatic notch
  e_ctx_spectral   context-wide SpectralNoiseReduction() on every channel, no map of any kind
The arms with the map, on this build:
  c_mixed2         2 channels of each of the four at once: (1, 0), (2, 0), (3, 0) and (0, 1), everyone else 0 / 0
  d_mixed256       256 channels of each
  f_map_spectral   the identity-like map: every channel (2, 0), against e_ctx_spectral
The mixed arms are to be read against the SUM and the MAXIMUM of the four b_ arms: four separate launches per kind would
cost about the sum of their chains, one launch per kernel form about the longest.  Both are printed.
The order of the arms rotates from round to round, so that no arm always runs behind the same neighbour.

  python tools/nr_map_probe.py [--channels 4096] [--frames 128] [--rounds 5] [--parent-lib LIB] [--out FILE.json]
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
from stage_map_probe import inputs, timed_launch, tunings  # noqa: E402

NEW = ("t41rx_set_nr_map", "t41rx_get_nr_map")
KINDS = {"kim": (1, 0), "spectral": (2, 0), "lms": (3, 0), "notch": (0, 1)}
PLAIN = ("a_off", "b_kim2", "b_spectral2", "b_lms2", "b_notch2", "e_ctx_spectral")


def listed(nch, count, shift=0):
    """`count` channels spread over the batch, another set per shift"""
    import numpy as np
    c = np.unique(np.round(np.linspace(nch // 3, nch - 1 - nch // 7, count)).astype(int)) - shift
    assert c.size == count and c.min() >= 0
    return c


def plain_chain(T, arm, nch, nco):
    """a context of an arm without a noise-reduction map, on one shared stream"""
    import numpy as np
    kind, notch = {"a_off": (0, 0), "e_ctx_spectral": (2, 0)}.get(arm) or KINDS[arm[2:-1]]
    rx = T.RxChain(nch, T.default_params(mode=0, FLoCut=200, FHiCut=3000, nrOptionSelect=kind, ANR_notchOn=notch), NCOFreq=nco)
    rx.set_input_map(np.zeros(nch, np.int32), 1)
    if arm.startswith("b_"):
        m = np.full(nch, T.STAGE_ALL & ~T.STAGE_NR, np.uint32)
        m[listed(nch, 2)] = T.STAGE_ALL
        rx.set_stage_map(m)
    return rx


def mapped_chain(T, arm, nch, nco):
    import numpy as np
    rx = T.RxChain(nch, T.default_params(mode=0, FLoCut=200, FHiCut=3000), NCOFreq=nco)
    rx.set_input_map(np.zeros(nch, np.int32), 1)
    kind, notch = np.zeros(nch, np.int32), np.zeros(nch, np.int32)
    if arm == "f_map_spectral":
        kind[:] = 2
    else:
        count = 2 if arm == "c_mixed2" else 256
        for i, (k, t) in enumerate(KINDS.values()):  # interleaved: the four sets one channel apart
            kind[listed(nch, count, i)], notch[listed(nch, count, i)] = k, t
        assert all(int(((kind == k) & (notch == t)).sum()) == count for k, t in KINDS.values())
    rx.set_nr_map(kind, notch)
    return rx


def serve(a):
    """the child: the library T41RX_LIB names (the parent commit's), one context per arm without a map; a line `arm` on
    stdin runs one launch and answers its microseconds"""
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
        arm = line.strip()
        if arm == "quit":
            break
        if arm not in chains:
            chains[arm] = plain_chain(T, arm, nch, tunings(nch))
        print("%.1f" % timed_launch(chains[arm], I, Q, out, nfr, stream), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libt41rx.so built from the parent commit: the arms without a map run on it")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.serve:
        return serve(a)
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("nr_map_probe needs a HIP device")
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
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch",
           "parent_lib": bool(child)}
    try:
        arms = {} if child else {k: plain_chain(T, k, nch, nco) for k in PLAIN}
        arms.update({k: mapped_chain(T, k, nch, nco) for k in ("c_mixed2", "d_mixed256", "f_map_spectral")})
        order = sorted(set(PLAIN) | set(arms))
        times = {k: [] for k in order}
        for r in range(a.warmup + a.rounds):
            for k in order[r % len(order):] + order[:r % len(order)]:
                if k in arms:
                    t = timed_launch(arms[k], I, Q, out, nfr, stream)
                else:
                    child.stdin.write(k + "\n")
                    child.stdin.flush()
                    t = float(child.stdout.readline())
                if r >= a.warmup:
                    times[k].append(t)
        for k, t in times.items():
            res[k] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
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
    # the stages' share of an arm: what it costs over the call with noise reduction off
    off = res["a_off"]["median"]
    four = [res["b_%s2" % k]["median"] - off for k in KINDS]
    res["four_kinds_2_over_off"] = {"sum": round(sum(four), 1), "max": round(max(four), 1)}
    res["mixed_over_off"] = {"c_mixed2": round(res["c_mixed2"]["median"] - off, 1), "d_mixed256": round(res["d_mixed256"]["median"] - off, 1)}
    line = json.dumps(res)
    print(line)
    for k in sorted(res):
        if isinstance(res[k], dict) and "median" in res[k]:
            print("%-24s median %9.1f  min %9.1f  max %9.1f  us per launch" % (k, res[k]["median"], res[k]["min"], res[k]["max"]))
    print("over a_off: the four kinds on 2 channels each, separately: sum %.1f  max %.1f;  c_mixed2 %.1f;  d_mixed256 %.1f  us per launch"
          % (res["four_kinds_2_over_off"]["sum"], res["four_kinds_2_over_off"]["max"], res["mixed_over_off"]["c_mixed2"], res["mixed_over_off"]["d_mixed256"]))
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
