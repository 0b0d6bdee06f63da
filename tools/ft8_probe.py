#!/usr/bin/env python3
"""Cost of the FT8 receive stage: one launch of the receive path through the device entry point on USB, with the stage
off and on, every channel synced (at 128 frames per launch each channel then runs 8 or 9 blocks of two 2048-point q15
transforms), all arms interleaved in one process on one device.  hipEvents around each launch, after warm-up; median, min
and max.

`off` is the fused kernel alone; `tap` adds the demod tap the stage reads (the tap kernels), without the stage; `on` adds
the stage behind it (a workgroup of 256 threads per channel; the wave-per-channel layout once timed beside it is recorded
in DESIGN.md, "FT8 receive", and gone from the library).

  python tools/ft8_probe.py [--channels 4096] [--frames 128] [--rounds 10] [--out FILE.json]
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("ft8_probe needs a HIP device")
    nch, nfr = a.channels, a.frames
    # a tone in the USB passband (1 kHz of audio) + noise, made on the device
    g = torch.Generator(device="cuda").manual_seed(1)
    n = torch.arange(nfr * 2048, device="cuda", dtype=torch.float32)
    ph = 2 * torch.pi * (47000.0 / 192000.0) * n  # (tests/siggen.py: 48000 - NCOFreq - audio)
    I = (0.1 * torch.cos(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    Q = (0.1 * torch.sin(ph) + 0.02 * torch.randn(nch, nfr * 2048, device="cuda", generator=g)).contiguous()
    out = torch.empty_like(I)
    arms = {}
    for name in ("off", "tap", "on"):
        rx = T.RxChain(nch, T.default_params(mode=0))
        if name == "tap":
            tap = torch.zeros(nch, nfr * 256, dtype=torch.float32, device="cuda")
            rx.set_debug_taps(demod=tap)
        if name == "on":
            rx.set_ft8_tables()
            rx.set_ft8(1, nfr)
            rx.ft8_sync()
        arms[name] = rx
    times = {k: [] for k in arms}
    blocks = {}
    for r in range(a.warmup + a.rounds):
        for k, rx in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rx.ProcessIQData(I, Q, out=out)
            e1.record()
            e1.synchronize()
            if r >= a.warmup:
                times[k].append(e0.elapsed_time(e1) * 1e3)
            if k == "on":  # blocks per channel in this launch: FT_8_counter moves by 8 or 9 (mod 92 across a slot's end)
                blocks[k] = int(rx.ft8_status(nfr)[0, -1, 0])
    res = {"channels": nch, "frames": nfr, "rounds": a.rounds, "device": torch.cuda.get_device_name(0), "unit": "us per launch",
           "FT_8_counter_after": blocks}
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
