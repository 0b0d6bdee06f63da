#!/usr/bin/env python3
"""Cost of the panadapter map (t41rx_set_panadapter_map): one launch of the receive path through the device entry point on
4096 channels x 128 frames of SSB reading ONE shared input stream (every channel reads row 0: a receiver group), the
panadapter at update_period 16 (8 rows per launch) with the beacon monitor behind it, all arms interleaved in one process
on one device (as tools/ft8_map_probe.py does).  hipEvents around each launch, after warm-up; median, min and max in us per
launch, and next to each arm the device memory its context took (hipMemGetInfo around its creation: the context's taps
and memories and the row buffers together) and the bytes of the row buffers alone.

The arms:
  a_off          the panadapter off
  c_nomap        the panadapter and the beacon monitor on, no panadapter map
  c_parent       the same on the parent commit's build (--parent-lib), where given: a child process that loads that
                 library, holds its context and runs one launch whenever this process tells it to, inside the rotation
  d_identity     the identity map: the list forms of the two kernels over all channels, the taps by row
  e_256_listed   256 of the channels listed, spread evenly, 256 rows
  f_5_listed     5 of the channels listed, 5 rows: the beacon monitor's five bands
  g_nobody       nobody listed, 1 row: the call is one without the stage
The order of the arms rotates from round to round, so that no arm always runs behind the same neighbour.

  python tools/pan_map_probe.py [--channels 4096] [--frames 128] [--rounds 5] [--parent-lib LIB] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NEW = ("t41rx_set_panadapter_map", "t41rx_get_panadapter_map", "t41rx_panadapter_rows")
PERIOD = 16


def make_chain(T, nch, nfr, nco, arm, rows=None):
    """a USB context on one shared stream: the panadapter off, or on at PERIOD with the beacon monitor behind it (rows: the
    panadapter map).  Returns (context, what keeps its buffers alive, device bytes taken, bytes of the row buffers)"""
    import numpy as np
    import torch
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    rx = T.RxChain(nch, T.default_params(mode=0, FLoCut=200, FHiCut=3000), NCOFreq=nco)
    rx.set_input_map(np.zeros(nch, np.int32), 1)
    keep, nbytes = None, 0
    if arm == "on":
        if rows is not None:
            rx.set_panadapter_map(*rows)
        max_rows = (nfr + PERIOD - 1) // PERIOD
        rx.set_panadapter_tables(np.load(os.path.join(ROOT, "tests", "golden", "display", "gradient.npz"))["gradient"])
        bufs = rx.set_panadapter(True, spectrumZoom=0, currentScale=1, update_period=PERIOD, update_phase=0, max_rows=max_rows)
        rx.set_beacon_clock(0, 32, 3)
        keep = (bufs, rx.set_beacon(True, 1, np.arange(nch) % 5, max_rows=max_rows))
        nbytes = sum(t.numel() * t.element_size() for t in bufs.values())
    torch.cuda.synchronize()
    return rx, keep, free0 - torch.cuda.mem_get_info()[0], nbytes


def inputs(nfr):
    import torch
    g = torch.Generator(device="cuda").manual_seed(0)
    I = (0.2 * torch.randn(1, nfr * 2048, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    Q = (0.2 * torch.randn(1, nfr * 2048, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    return I, Q


def timed_launch(rx, I, Q, out, nfr, stream):
    import torch
    if rx.panadapter_status()[0]:
        rx.set_panadapter_counter(0)  # every launch has the same update frames: 0, 16, ..
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
    """the child: the library T41RX_LIB names (the parent commit's), one context with the stage on and no map; a line on
    stdin runs one launch and answers its microseconds"""
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd import _lib
    for name in NEW:  # (the parent's library has no such entry to bind)
        _lib.SYMBOLS.pop(name, None)
    T.RxChain.panadapter_rows = property(lambda self: self.n_channels)  # (... and no map: a row per channel)
    nch, nfr = a.channels, a.frames
    I, Q = inputs(nfr)
    out = torch.empty(nch * nfr * 2048, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    rx, keep, held, nbytes = make_chain(T, nch, nfr, tunings(nch), "on")
    print("ready %s %d %d" % (T.LIB_PATH, held, nbytes), flush=True)
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
        raise SystemExit("pan_map_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    nco = tunings(nch)
    I, Q = inputs(nfr)
    out = torch.empty(nch * nfr * 2048, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    child, parent_bytes = None, (0, 0)
    if a.parent_lib:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve", "--channels", str(nch), "--frames", str(nfr)],
                                 env=dict(os.environ, T41RX_LIB=os.path.abspath(a.parent_lib)), stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        hello = child.stdout.readline().split()
        if hello[:1] != ["ready"] or os.path.abspath(hello[1]) != os.path.abspath(a.parent_lib):
            raise SystemExit("the child did not load %s: %r" % (a.parent_lib, hello))
        parent_bytes = (int(hello[2]), int(hello[3]))

    def listed(count):
        """`count` channels spread over the group, rows in descending order: a permutation, not the identity's prefix"""
        m = np.full(nch, -1, np.int32)
        at = np.unique(np.round(np.linspace(nch // 3, nch - 1 - nch // 7, count)).astype(int))
        assert at.size == count
        m[at] = np.arange(count - 1, -1, -1)
        return m, count

    arms = {"a_off": make_chain(T, nch, nfr, nco, "off"),
            "c_nomap": make_chain(T, nch, nfr, nco, "on"),
            "d_identity": make_chain(T, nch, nfr, nco, "on", (np.arange(nch, dtype=np.int32), nch)),
            "e_256_listed": make_chain(T, nch, nfr, nco, "on", listed(min(256, nch))),
            "f_5_listed": make_chain(T, nch, nfr, nco, "on", listed(min(5, nch))),
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
        held, rows_bytes = parent_bytes if k == "c_parent" else arms[k][2:]
        res[k] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1),
                  "device_bytes": held, "row_buffer_bytes": rows_bytes}
    for rx, _, _, _ in arms.values():
        rx.close()
    line = json.dumps(res)
    print(line)
    for k in sorted(times):
        print("%-14s median %9.1f  min %9.1f  max %9.1f  us per launch   context + rows %12d bytes   rows alone %12d bytes" % (
            k, res[k]["median"], res[k]["min"], res[k]["max"], res[k]["device_bytes"], res[k]["row_buffer_bytes"]))
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
