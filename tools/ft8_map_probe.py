#!/usr/bin/env python3
"""Cost of the FT8 map (t41rx_set_ft8_map): one launch of the receive path through the device entry point on 4096 channels
x 128 frames of SSB reading ONE shared input stream (every channel reads row 0: a receiver group), every channel synced,
all arms interleaved in one process on one device (as tools/stage_map_probe.py does).  hipEvents around each launch, after
warm-up; median, min and max in us per launch, and next to each arm the bytes of d_power + d_status it was given.

The arms:
  a_off          FT8 receive off
  b_tap_only     FT8 off, the caller's demod tap set: what the stage's audio costs without the stage
  c_nomap        FT8 on, no FT8 map
  c_parent       the same on the parent commit's build (--parent-lib), where given: a child process that loads that
                 library, holds its context and runs one launch whenever this process tells it to, inside the rotation
  d_identity     the identity map: the list form of ft8_kernel over all channels
  e_256_listed   256 of the channels listed, spread evenly, 256 rows
  f_2_listed     2 of the channels listed, 2 rows
  g_nobody       nobody listed, 1 row: the stage launches nothing, the call still writes the demod tap
The order of the arms rotates from round to round, so that no arm always runs behind the same neighbour.

  python tools/ft8_map_probe.py [--channels 4096] [--frames 128] [--rounds 5] [--parent-lib LIB] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("t41rx_set_ft8_map", "t41rx_get_ft8_map", "t41rx_ft8_rows")


def make_chain(T, nch, nfr, nco, arm, rows=None):
    """a USB context on one shared stream: FT8 off, off with the caller's demod tap, or on and synced (rows: the FT8 map)"""
    import numpy as np
    import torch
    rx = T.RxChain(nch, T.default_params(mode=0, FLoCut=200, FHiCut=3000), NCOFreq=nco)
    rx.set_input_map(np.zeros(nch, np.int32), 1)
    keep, nbytes = None, 0
    if arm == "tap":
        keep = torch.zeros(nch, nfr * 256, dtype=torch.float32, device="cuda")
        rx.set_debug_taps(demod=keep)
    elif arm == "on":
        if rows is not None:
            rx.set_ft8_map(*rows)
        rx.set_ft8_tables()
        keep = rx.set_ft8(1, nfr)
        rx.ft8_sync()
        nbytes = sum(t.numel() * t.element_size() for t in keep)
    return rx, keep, nbytes


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
    """the child: the library T41RX_LIB names (the parent commit's), one context with FT8 on and no map; a line on stdin
    runs one launch and answers its microseconds"""
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd import _lib
    for name in NEW:  # (the parent's library has no such entry to bind)
        _lib.SYMBOLS.pop(name, None)
    nch, nfr = a.channels, a.frames
    I, Q = inputs(nfr)
    out = torch.empty(nch * nfr * 2048, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rx, keep, nbytes = make_chain(T, nch, nfr, tunings(nch), "on")
    print("ready %s %d" % (T.LIB_PATH, nbytes), flush=True)
    for line in sys.stdin:
        if line.strip() == "quit":
            break
        print("%.1f" % timed_launch(rx, I, Q, out, nfr, stream), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libt41rx.so built from the parent commit: adds the arm c_parent")
    ap.add_argument("--serve", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.serve:
        return serve(a)
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("ft8_map_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    nco = tunings(nch)
    I, Q = inputs(nfr)
    out = torch.empty(nch * nfr * 2048, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    child, parent_bytes = None, 0
    if a.parent_lib:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", "--channels", str(nch), "--frames", str(nfr)],
                                 env=dict(os.environ, T41RX_LIB=os.path.abspath(a.parent_lib)), stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        hello = child.stdout.readline().split()
        if hello[:1] != ["ready"] or os.path.abspath(hello[1]) != os.path.abspath(a.parent_lib):
            raise SystemExit("the child did not load %s: %r" % (a.parent_lib, hello))
        parent_bytes = int(hello[2])

    def listed(count):
        """`count` channels spread over the group, rows in descending order: a permutation, not the identity's prefix"""
        m = np.full(nch, -1, np.int32)
        at = np.unique(np.round(np.linspace(nch // 3, nch - 1 - nch // 7, count)).astype(int))
        assert at.size == count
        m[at] = np.arange(count - 1, -1, -1)
        return m, count

    arms = {"a_off": make_chain(T, nch, nfr, nco, "off"),
            "b_tap_only": make_chain(T, nch, nfr, nco, "tap"),
            "c_nomap": make_chain(T, nch, nfr, nco, "on"),
            "d_identity": make_chain(T, nch, nfr, nco, "on", (np.arange(nch, dtype=np.int32), nch)),
            "e_256_listed": make_chain(T, nch, nfr, nco, "on", listed(min(256, nch))),
            "f_2_listed": make_chain(T, nch, nfr, nco, "on", listed(min(2, nch))),
            "g_nobody": make_chain(T, nch, nfr, nco, "on", (np.full(nch, -1, np.int32), 1))}
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch",
           "parent_lib": bool(child)}
    order = list(arms) + (["c_parent"] if child else [])
    times = {k: [] for k in order}
    try:
        for r in range(a.warmup + a.rounds):
            for k in order[r % len(order):] + order[:r % len(order)]:
                if k == "c_parent":
                    child.stdin.write("go\n")
                    child.stdin.flush()
                    t = float(child.stdout.readline())
                else:
                    t = timed_launch(arms[k][0], I, Q, out, nfr, stream)
                if r >= a.warmup:
                    times[k].append(t)
        torch.cuda.synchronize()
    finally:
        if child:
            try:
                child.stdin.write("quit\n")
                child.stdin.flush()
            except OSError:
                pass
            child.wait(timeout=60)
    for k, t in times.items():
        res[k] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1),
                  "power_status_bytes": parent_bytes if k == "c_parent" else arms[k][2]}
    for rx, _, _ in arms.values():
        rx.close()
    line = json.dumps(res)
    print(line)
    for k in sorted(times):
        print("%-14s median %9.1f  min %9.1f  max %9.1f  us per launch   d_power + d_status %12d bytes" % (
            k, res[k]["median"], res[k]["min"], res[k]["max"], res[k]["power_status_bytes"]))
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
