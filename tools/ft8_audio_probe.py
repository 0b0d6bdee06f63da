#!/usr/bin/env python3
"""Cost of FT8 from 12 kS/s audio: one call of RxChain.ft8_audio() on int16 samples, a whole slot of 1380 frames per channel
(92 blocks of two 2048-point q15 transforms), next to what the same 92 blocks cost behind the live stage.

The live stage cannot be timed alone (it runs behind the receive path), so its cost is the increment tools/ft8_probe.py
measures: a launch of the receive path with the stage on minus one with the demod tap only, here at --live-frames frames
per launch and scaled to 1380 frames.  The three arms are interleaved in one process on one device, `rounds` times;
hipEvents around each launch, after warm-up.  Printed: every round's three times, the medians, and the spread (max - min)
of the rounds.

  python tools/ft8_audio_probe.py [--channels 4096] [--frames 1380] [--live-frames 128] [--rounds 5] [--out FILE.json]
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
    ap.add_argument("--frames", type=int, default=1380)
    ap.add_argument("--live-frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import t41_sdr_amd as T
    if not torch.cuda.is_available():
        raise SystemExit("ft8_audio_probe needs a HIP device")
    nch, nfr, lfr = a.channels, a.frames, a.live_frames
    g = torch.Generator(device="cuda").manual_seed(1)
    # the audio arm: a 1 kHz tone + noise as int16 at 12 kS/s
    n = torch.arange(nfr * 128, device="cuda", dtype=torch.float32)
    pcm = ((0.1 * torch.sin(2 * torch.pi * (1000.0 / 12000.0) * n) + 0.02 * torch.randn(nch, nfr * 128, device="cuda", generator=g))
           * 32768.0).to(torch.int16).contiguous()
    audio = T.RxChain(nch, T.default_params(mode=0))
    audio.set_ft8_tables()
    audio.set_ft8(1, nfr)
    audio.ft8_audio_begin()
    # the live arms (tools/ft8_probe.py's `tap` and `on`): the same tone in the USB passband
    n = torch.arange(lfr * 2048, device="cuda", dtype=torch.float32)
    ph = 2 * torch.pi * (47000.0 / 192000.0) * n
    I = (0.1 * torch.cos(ph) + 0.02 * torch.randn(nch, lfr * 2048, device="cuda", generator=g)).contiguous()
    Q = (0.1 * torch.sin(ph) + 0.02 * torch.randn(nch, lfr * 2048, device="cuda", generator=g)).contiguous()
    out = torch.empty_like(I)
    tap = T.RxChain(nch, T.default_params(mode=0))
    tap_buf = torch.zeros(nch, lfr * 256, dtype=torch.float32, device="cuda")
    tap.set_debug_taps(demod=tap_buf)
    on = T.RxChain(nch, T.default_params(mode=0))
    on.set_ft8_tables()
    on.set_ft8(1, lfr)
    on.ft8_sync()

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    arms = {"audio": lambda: audio.ft8_audio(pcm), "tap": lambda: tap.ProcessIQData(I, Q, out=out), "on": lambda: on.ProcessIQData(I, Q, out=out)}
    rounds = []
    for r in range(a.warmup + a.rounds):
        t = {k: round(timed(fn), 1) for k, fn in arms.items()}
        if r >= a.warmup:
            t["live_increment_scaled"] = round((t["on"] - t["tap"]) * nfr / lfr, 1)
            rounds.append(t)
    last = audio.ft8_status(nfr)[0, -1].tolist()  # FT_8_counter, ft8_flag, 0 or 1 + the half completed, dataLoop behind the call
    res = {"channels": nch, "frames": nfr, "live_frames": lfr, "rounds": rounds, "device": torch.cuda.get_device_name(0),
           "unit": "us per call; live_increment_scaled = (on - tap) * frames / live_frames", "audio_status_behind_the_call": last}
    for k in ("audio", "live_increment_scaled"):
        v = [x[k] for x in rounds]
        res[k] = {"median": round(statistics.median(v), 1), "min": min(v), "max": max(v), "spread": round(max(v) - min(v), 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fo:
            fo.write(line + "\n")


if __name__ == "__main__":
    main()
