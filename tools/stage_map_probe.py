#!/usr/bin/env python3
"""Cost of the stage map (t41rx_set_stage_map): one launch of the receive path through the device entry point on 4096
channels x 128 frames of SSB reading ONE shared input stream (every channel reads row 0: a receiver group), all arms of
a series interleaved in one process on one device (as tools/output_map_probe.py does).  hipEvents around each launch,
after warm-up; median, min and max in us per launch.

One series per stage: the receive equalizer, the spectral noise reduction (nrOptionSelect 2), the automatic notch, and
the CW detector with the Morse decoder.  The arms of a series:
  a_off          the stage switched off
  b_nomap        the stage on, no stage map
  b_parent       the same on the parent commit's build (--parent-lib), where given: a child process that loads that
                 library, holds its context and runs one launch whenever this process tells it to, inside the rotation
  c_identity     every mask STAGE_ALL: the list forms of the stage kernels over all channels
  d_2_listed     2 of the channels listed
  e_256_listed   256 of the channels listed, spread evenly
  f_nobody       nobody listed: the stage launches nothing, the call still hands over
The order of the arms rotates from round to round, so that no arm always runs behind the same neighbour.

  python tools/stage_map_probe.py [--channels 4096] [--frames 128] [--rounds 5] [--series REGEX] [--parent-lib LIB] [--out FILE.json]
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
SERIES = ("eq", "spectral", "notch", "cw")


def decode_fir():
    """a 64-tap low-pass for the detector: the probe times the stage, any finite table does"""
    import numpy as np
    n = np.arange(64) - 31.5
    return (np.sinc(n / 8.0) / 8.0 * np.hanning(64)).astype(np.float32)


def eq_bands():
    """14 x 4 stable band-pass sections {b0, b1, b2, -a1, -a2}: the probe times the stage, any finite stable table does"""
    import numpy as np
    t = np.zeros((14, 4, 5), np.float32)
    for b in range(14):
        w = 2 * np.pi * (100.0 * 1.45 ** b) / 24000.0
        r = 0.98
        t[b, :] = [0.02, 0.0, -0.02, 2 * r * np.cos(w), -r * r]
    return t


def make_chain(T, series, nch, nfr, nco, on):
    """a context of the series on one shared stream, the stage switched on or off"""
    import numpy as np
    kw = dict(mode=0, FLoCut=200, FHiCut=3000)
    if series == "cw":
        kw["xmtMode"] = 1
    if on and series == "spectral":
        kw["nrOptionSelect"] = 2
    if on and series == "notch":
        kw["ANR_notchOn"] = 1
    rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
    rx.set_input_map(np.zeros(nch, np.int32), 1)
    if on and series == "eq":
        rx.set_receive_eq_bands(eq_bands())
        rx.set_receive_eq(1)
    if on and series == "cw":
        rx.set_cw_tables(None, decode_fir())
        rx.set_cw_decode_tree(b"-" * 129)
        rx.set_cw_detector(1, nfr)
        rx.set_cw_decoder(1, nfr)
    return rx


def inputs(nfr):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    I = (0.2 * torch.randn(1, nfr * 2048, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    Q = (0.2 * torch.randn(1, nfr * 2048, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    return I, Q


def timed_launch(rx, I, Q, out, nfr, stream):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = rx._lib.t41rx_process_device(rx._ctx, I.data_ptr(), Q.data_ptr(), out.data_ptr(), nfr, stream)
    e1.record()
    e1.synchronize()
    if rc != 0:
        raise RuntimeError("libt41rx: %d %s" % (rc, rx._lib.t41rx_last_error().decode()))
    return e0.elapsed_time(e1) * 1e3


def tunings(nch):
    import numpy as np
    return (np.random.default_rng(1000).integers(-860, 801, nch) * 50).astype(np.int32)  # config 2's tunings


def serve(a):
    """the child: the library T41RX_LIB names (the parent commit's), one context per series with the stage on and no
    map; a line `series` on stdin runs one launch and answers its microseconds"""
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd import _lib
    for name in ("t41rx_set_stage_map", "t41rx_get_stage_map"):  # (the parent's library has no such entry to bind)
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
            chains = {series: make_chain(T, series, nch, nfr, tunings(nch), True)}
        print("%.1f" % timed_launch(chains[series], I, Q, out, nfr, stream), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--series", default=None, help="regular expression: run only the series it matches, e.g. 'notch|cw'")
    ap.add_argument("--parent-lib", default=None, help="libt41rx.so built from the parent commit: adds the arm b_parent")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.serve:
        return serve(a)
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("stage_map_probe needs a HIP device")
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

    def listed(count):
        m = np.zeros(nch, np.uint32)
        m[np.unique(np.round(np.linspace(nch // 3, nch - 1 - nch // 7, count)).astype(int))] = T.STAGE_ALL
        assert int((m != 0).sum()) == count
        return m

    maps = {"b_nomap": None, "c_identity": np.full(nch, T.STAGE_ALL, np.uint32), "d_2_listed": listed(2),
            "e_256_listed": listed(min(256, nch)), "f_nobody": np.zeros(nch, np.uint32)}
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch",
           "parent_lib": bool(child)}
    try:
        for series in SERIES:
            if a.series and not re.search(a.series, series):
                continue
            arms = {"a_off": make_chain(T, series, nch, nfr, nco, False)}
            for name, m in maps.items():
                arms[name] = make_chain(T, series, nch, nfr, nco, True)
                if m is not None:
                    arms[name].set_stage_map(m)
            order = list(arms) + (["b_parent"] if child else [])
            times = {k: [] for k in order}
            for r in range(a.warmup + a.rounds):
                for k in order[r % len(order):] + order[:r % len(order)]:
                    if k == "b_parent":
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
