#!/usr/bin/env python3
"""Cost of the IQ calibration: one receive sweep (t41rx_calibrate_device, every channel a candidate on one shared
recording) at spectrumZoom 0 with 40 frames and at spectrumZoom 2 with 64 frames, each with the first frame flagged only
(a sweep as the firmware runs it) and with every frame flagged; and one launch of the calibration exciter beside one of
the CW exciter on the same shape.  All arms interleaved in one process on one device, hipEvents around each launch, after
warm-up; median, min and max in microseconds per launch.

  python tools/cal_probe.py [--channels 4096] [--tx-frames 32] [--rounds 15] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--channels", type=int, default=4096)
    ap.add_argument("--tx-frames", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd._lib import check
    if not torch.cuda.is_available():
        raise SystemExit("cal_probe needs a HIP device")
    nch, tfr = a.channels, a.tx_frames
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    amps = (1.0 + 0.0001 * (np.arange(nch) % 101 - 50)).astype(np.float32)
    phases = (0.0001 * (np.arange(nch) % 97 - 48)).astype(np.float32)
    arms, keep = {}, []
    g = torch.Generator(device="cuda").manual_seed(1)
    for zoom, frames, bins in ((0, 40, (65, 192)), (2, 64, (209, 273))):
        n = torch.arange(frames * 2048, device="cuda", dtype=torch.float32)
        w = 2 * torch.pi * 3000.0 / 192000.0 * n
        I = (0.25 * torch.cos(w) + 0.001 * torch.randn(frames * 2048, device="cuda", generator=g)).contiguous()
        Q = (0.24 * torch.sin(w + 0.02) + 0.001 * torch.randn(frames * 2048, device="cuda", generator=g)).contiguous()
        res = torch.zeros(nch, frames, 3, device="cuda")
        first = torch.zeros(frames, dtype=torch.uint8, device="cuda")
        first[0] = 1
        for name, upd in (("first_frame", first), ("every_frame", None)):
            rx = T.RxChain(nch, T.default_params(mode=T.DEMOD_USB))
            rx.set_calibration(True, zoom, 1, 0, bins[0], bins[1], 10)
            rx.set_cal_corrections(amps, phases)
            keep.append((rx, I, Q, res, upd))
            arms["rx_zoom%d_%dfr_%s" % (zoom, frames, name)] = (
                lambda rx=rx, I=I, Q=Q, res=res, upd=upd, frames=frames: rx._lib.t41rx_calibrate_device(
                    rx._ctx, vp(I), vp(Q), 1, None if upd is None else vp(upd), vp(res), None, None, frames, stream))
    cal, cw = T.TxChain(nch), T.TxChain(nch)
    cal.set_cal_tone(*T.cal_tone(), 0.5)
    cal.set_cal_corrections(amps, phases)
    cw.set_cw_tone(*T.sine_tone(8))
    oL = torch.empty((nch, tfr * 2048), dtype=torch.int16, device="cuda")
    oR = torch.empty_like(oL)
    lib = cal._lib
    arms["tx_cal_%dfr" % tfr] = lambda: lib.t41tx_process_cal_device_q15(cal._ctx, vp(oL), vp(oR), tfr, stream)
    arms["tx_cw_%dfr" % tfr] = lambda: lib.t41tx_process_cw_device_q15(cw._ctx, None, vp(oL), vp(oR), tfr, stream)
    times = {k: [] for k in arms}
    for r in range(a.warmup + a.rounds):
        for k, launch in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            check(launch())
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
    out = {"channels": nch, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch"}
    for k, t in times.items():
        out[k] = {"median": round(statistics.median(t), 1), "min": round(min(t), 1), "max": round(max(t), 1)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
