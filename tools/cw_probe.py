#!/usr/bin/env python3
"""Cost of the CW receive stages: one launch of the receive path through the device entry point, USB with xmtMode = CW,
with the narrow filter and the tone detector off and on, all arms interleaved in one process on one device.  hipEvents
around each launch, after warm-up; median, min and max.  The arm without either stage runs the fused kernel alone; the
others add the stage path's split of it, the stage kernels and the back kernel.

The Morse decoder behind the detector (t41rx_set_cw_decoder) is timed on two streams, each against the detector alone in
the same interleave: the quiet one -- the carrier stays keyed, no histogram call -- and the worst case, in which every
channel runs DoGapHistogram() with its scaling pass in the same frame: before each launch of the `_worst` arms the context
is set to a prepared checkpoint (oldTime = -6000, the last signal 100 ms back, the gap histogram filled with counts of 12).

  python tools/cw_probe.py [--channels 4096] [--frames 128] [--rounds 10] [--index 0] [--out FILE.json]
"""
import argparse
import json
import os
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
    ap.add_argument("--index", type=int, default=0, help="CWFilterIndex of the filter arms")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("cw_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    z = np.load(os.path.join(ROOT, "tests", "golden", "cw", "cw_tables.npz"))
    tree = np.load(os.path.join(ROOT, "tests", "golden", "cw", "morse_tree.npz"))["tree"]
    # a carrier at the dial (heard at the 750 Hz side tone) + noise, made on the device
    g = torch.Generator(device="cuda").manual_seed(1)
    n = torch.arange(nfr * 2048, device="cuda", dtype=torch.float32)
    ph = 2 * torch.pi * (48000.0 / 192000.0) * n
    I = (0.3 * torch.cos(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    Q = (0.3 * torch.sin(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    out = torch.empty_like(I)
    arms = {}
    for name, index, det, dec in (("off", 5, 0, 0), ("filter", a.index, 0, 0), ("detector", 5, 1, 0), ("filter_detector", a.index, 1, 0),
                                  ("detector_decoder", 5, 1, 1), ("detector_worst", 5, 1, 0), ("detector_decoder_worst", 5, 1, 1)):
        rx = T.RxChain(nch, T.default_params(mode=0, xmtMode=1))
        rx.set_cw_tables(z["filters_f32"], z["fir_f32"])
        rx.set_cw_filter(index)
        if det:
            rx.set_cw_detector(1, nfr)
        if dec:
            rx.set_cw_decode_tree(tree)
            rx.set_cw_decoder(1, nfr)
        arms[name] = rx
    # the worst case's checkpoint: the decoder's section (include/t41rx.h, section bit 5: 3104 int32 words per channel)
    # at power-on, then n = 3, oldTime = -6000, signalEnd = -100 and every gap-histogram word 12
    rx = arms["detector_decoder_worst"]
    rx.ProcessIQData(I[:, :2048].contiguous(), Q[:, :2048].contiguous())
    rx.reset()
    worst = rx.get_state()
    assert worst[:32].view(np.int32)[5] == 16 | 32
    sec = worst[-4 * 3104 * nch:].view(np.int32).reshape(nch, 3104)
    sec[:, 1], sec[:, 2], sec[:, 4] = 3, -6000, -100
    sec[:, 32 + 768:] = 12
    plain = arms["detector_worst"].get_state()
    times = {k: [] for k in arms}
    calls = 0
    for r in range(a.warmup + a.rounds):
        for k, rx in arms.items():
            if k.endswith("_worst"):
                rx.set_state(worst if k == "detector_decoder_worst" else plain)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rx.ProcessIQData(I, Q, out=out)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
            if k == "detector_decoder_worst":  # every channel's histogram ran: its gap word went from 12 to 9 and back up
                after = rx.get_state()[-4 * 3104 * nch:].view(np.int32).reshape(nch, 3104)
                calls = int((after[:, 32 + 768] == 9).sum())
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "CWFilterIndex": a.index,
           "device": torch.cuda.get_device_name(0), "unit": "us per launch",
           "worst_case_channels_with_a_histogram_call": calls}
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
