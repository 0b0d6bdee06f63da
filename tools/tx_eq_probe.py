#!/usr/bin/env python3
"""Cost of the transmit equaliser: one launch of the exciter through the device entry point, equaliser off and on, and
-- with --parent LIB, a libt41rx.so built from the commit before the equaliser -- the off case on that library too,
all interleaved in one process on one device.  hipEvents around each launch, after warm-up; median, min and max.

  python tools/tx_eq_probe.py [--parent LIB] [--channels 4096] [--frames 32] [--rounds 25] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Exciter:
    """a raw binding of one library's t41tx_* entry points (two libraries live side by side in this process)"""

    def __init__(self, path, nch):
        import t41_sdr_amd as T
        self.lib = C.CDLL(path)
        self.lib.t41rx_last_error.restype = C.c_char_p
        self.ctx = C.c_void_p()
        p = T.default_tx_params()
        self.check(self.lib.t41tx_create(C.byref(self.ctx), 0, nch, C.byref(p)))

    def check(self, rc):
        if rc != 0:
            raise RuntimeError("t41tx status %d: %s" % (rc, self.lib.t41rx_last_error().decode()))

    def equaliser(self, on, bands):
        self.check(self.lib.t41tx_set_transmit_eq_bands(self.ctx, bands.ctypes.data_as(C.c_void_p)))
        self.check(self.lib.t41tx_set_transmit_eq(self.ctx, int(on), None))

    def launch(self, x, oL, oR, nfr, stream):
        self.check(self.lib.t41tx_process_device_q15(self.ctx, C.c_void_p(x.data_ptr()), None, C.c_void_p(oL.data_ptr()),
                                                     C.c_void_p(oR.data_ptr()), nfr, C.c_void_p(stream)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None)
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("tx_eq_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    bands = np.ascontiguousarray(np.load(os.path.join(ROOT, "tests", "golden", "eq", "rx_eq_bands.npz"))["coeffs_f32"], np.float32)
    # speech-band tones + noise at about half scale, made on the device
    g = torch.Generator(device="cuda").manual_seed(1)
    n = torch.arange(nfr * 2048, device="cuda", dtype=torch.float32)
    f = torch.rand(nch, 1, device="cuda", generator=g) * 2500.0 + 300.0
    x = 0.4 * torch.sin(2 * torch.pi * f / 192000.0 * n) + 0.05 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)
    x = (x * 32768.0).clamp(-32768, 32767).to(torch.int16).contiguous()
    oL, oR = torch.empty_like(x), torch.empty_like(x)
    arms = {}
    if a.parent:
        arms["parent_eq_off"] = Exciter(a.parent, nch)
    arms["eq_off"] = Exciter(T.LIB_PATH, nch)
    arms["eq_on"] = Exciter(T.LIB_PATH, nch)
    arms["eq_on"].equaliser(1, bands)
    stream = torch.cuda.current_stream().cuda_stream
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.rounds):
        for k, ex in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ex.launch(x, oL, oR, nfr, stream)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch"}
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
