#!/usr/bin/env python3
"""Cost of the audio rate (t41rx_set_audio_rate): one launch of the receive path through the device entry point on
4096 channels x 128 frames of SSB, all arms interleaved in one process on one device (as tools/param_sets_probe.py
does).  hipEvents around each launch, after warm-up; median, min and max in us per launch.

Arms: AGC off and on (AGCMode 1, the pipelined kernel) x f32 and q15 samples x no input map and one shared stream (every
channel reads row 0) x three libraries' worth of back end:
  192k         this library at T41RX_AUDIO_RATE_192K
  24k          this library at T41RX_AUDIO_RATE_24K (the fused form: no taps, no stage)
  parent_192k  the library --parent names (default: $T41RX_PARENT_LIB), loaded next to this one in the same process: the
               baseline the 192k arms must stay within the spread of.  Left out when no such file is given.
  parent_192k_b  the same again, a second context of the parent's library: the distance between these two arms is the
               spread an arm has to exceed before it says anything (two contexts differ in where their buffers lie)
  192k_b       this library at 192 kS/s again, the context created behind the parent's two: with parent_192k_b it
               tells a difference between the libraries from one between a context's place in the allocation order
The order of the arms rotates from round to round, so that no arm always runs behind the same neighbour.
Both libraries are driven through the same ctypes calls (create, set_nco_freq, set_input_map, process_device[_q15]), so an
arm differs from its neighbour in the library and the rate alone.

  python tools/audio_rate_probe.py [--parent LIB] [--channels 4096] [--frames 128] [--rounds 5] [--arms REGEX] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bind(path):
    """the library at `path` with the argument types of every entry point of t41_sdr_amd._lib.SYMBOLS it exports"""
    from t41_sdr_amd import _lib
    lib = C.CDLL(path)
    for name, (res, args) in _lib.SYMBOLS.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


class Chain:
    """a context of `lib` and its launch, raw: the probe times the library, not the Python layer"""

    def __init__(self, lib, nch, params, nco, shared, rate24):
        import numpy as np
        self.lib, self.ctx = lib, C.c_void_p()
        self.check(lib.t41rx_create(C.byref(self.ctx), 0, nch, C.byref(params)))
        self.check(lib.t41rx_set_nco_freq(self.ctx, nco.ctypes.data_as(C.POINTER(C.c_int32)), nch))
        if shared:
            m = np.zeros(nch, np.int32)
            self.check(lib.t41rx_set_input_map(self.ctx, m.ctypes.data_as(C.POINTER(C.c_int32)), nch, 1))
        if rate24:
            self.check(lib.t41rx_set_audio_rate(self.ctx, 1))

    def check(self, rc):
        if rc != 0:
            raise RuntimeError("libt41rx: %d %s" % (rc, self.lib.t41rx_last_error().decode()))

    def launch(self, a, b, out, nfr, q15, stream):
        entry = self.lib.t41rx_process_device_q15 if q15 else self.lib.t41rx_process_device
        self.check(entry(self.ctx, a.data_ptr(), b.data_ptr(), out.data_ptr(), nfr, stream))

    def close(self):
        self.lib.t41rx_destroy(self.ctx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=os.environ.get("T41RX_PARENT_LIB"), help="the parent commit's libt41rx.so (the 192 kS/s baseline)")
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--arms", default=None, help="regular expression: run only the arms it matches, e.g. 'agc_off/f32/.*/24k$'")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("audio_rate_probe needs a HIP device")
    nch, nfr, L = a.channels, a.frames, 2048
    libs = {"this": bind(_lib.LIB_PATH)}
    if a.parent and os.path.exists(a.parent):
        libs["parent"] = bind(a.parent)
    nco = (np.random.default_rng(1000).integers(-860, 801, nch) * 50).astype(np.int32)  # config 2's tunings
    g = torch.Generator(device="cuda").manual_seed(0)
    I = (0.2 * torch.randn(nch, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    Q = (0.2 * torch.randn(nch, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
    data = {"f32": (I, Q, torch.empty_like(I)),
            "q15": ((I * 32768).to(torch.int16), (Q * 32768).to(torch.int16), torch.empty(nch, nfr * L, dtype=torch.int16, device="cuda"))}
    stream = torch.cuda.current_stream().cuda_stream
    arms = {}
    for agc in (0, 1):
        p = T.default_params(mode=0, FLoCut=200, FHiCut=3000, AGCMode=agc)
        for fmt in ("f32", "q15"):
            for rows in ("own", "shared"):
                for what, lib, r24 in (("192k", "this", False), ("24k", "this", True), ("parent_192k", "parent", False),
                                       ("parent_192k_b", "parent", False), ("192k_b", "this", False)):
                    name = "agc_%s/%s/%s/%s" % ("on" if agc else "off", fmt, rows, what)
                    if lib not in libs or (a.arms and not re.search(a.arms, name)):
                        continue
                    arms[name] = (Chain(libs[lib], nch, p, nco, rows == "shared", r24), fmt, rows)
    times = {k: [] for k in arms}
    order = list(arms)
    for r in range(a.warmup + a.rounds):
        for k in order[r % len(order):] + order[:r % len(order)]:
            ch, fmt, rows = arms[k]
            x, y, out = data[fmt]
            if fmt == "q15":
                x, y = y, x  # the L queue carries Q, the R queue I (Process.cpp:107-108)
            if rows == "shared":
                x, y = x[:1], y[:1]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ch.launch(x, y, out, nfr, fmt == "q15", stream)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    for ch, _, _ in arms.values():
        ch.close()
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch",
           "parent": bool("parent" in libs)}
    for k, t in times.items():
        res[k] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1),
                  "per_frame": round(statistics.median(t) / nfr, 2)}
    line = json.dumps(res)
    print(line)
    for k in sorted(res):
        if isinstance(res[k], dict):
            print("%-34s median %9.1f  min %9.1f  max %9.1f  us per launch  (%6.2f us per frame)"
                  % (k, res[k]["median"], res[k]["min"], res[k]["max"], res[k]["per_frame"]))
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
