#!/usr/bin/env python3
"""A/B timing of kernel builds on config 2's shape: interleaved rounds, one process per cell (GPU box).

  python tools/ab_probe.py product uncond other ... [--rounds 3] [--frames 32] [--reps 60] [--layout channel]
    NAME = "product" (t41_sdr_amd/libt41rx.so) or a build of tools/build_variant.sh NAME (t41_sdr_amd/abl/libt41rx_NAME.so)
Prints the median / minimum us per 4096-channel frame per build and the spread, as JSON lines.

  python tools/ab_probe.py one NAME [--frames 32] [--reps 60] [--layout channel] [--mode M] [--agc A]
    one timing of the library this process binds (T41RX_LIB): what the rounds above start per cell
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def one(frames, reps, layout="channel"):
    """HIP-event time per frame of the library this process bound (T41RX_LIB), config 2's shape"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import t41_sdr_amd as T
    nch, L = 4096, 2048
    rng = np.random.default_rng(1000)
    nco = (rng.integers(-860, 801, nch) * 50).astype(np.int32)
    a = sys.argv[1:]
    kw = {}
    if "--mode" in a:
        kw["mode"] = int(a[a.index("--mode") + 1])
    if "--agc" in a:
        kw["AGCMode"] = int(a[a.index("--agc") + 1])
    rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
    rx.set_buffer_layout(layout)
    shape = (nch, frames * L) if layout == "channel" else (frames, nch, L)
    ring = max(2, -(-(768 << 20) // (3 * nch * frames * L * 4)))
    g = torch.Generator(device="cuda").manual_seed(0)
    Is = [(0.2 * torch.randn(*shape, generator=g, device="cuda")).clamp_(-0.999, 0.999) for _ in range(ring)]
    Qs = [(0.2 * torch.randn(*shape, generator=g, device="cuda")).clamp_(-0.999, 0.999) for _ in range(ring)]
    out = [torch.empty(*shape, device="cuda") for _ in range(ring)]
    for k in range(max(6, reps // 4)):
        rx.ProcessIQData(Is[k % ring], Qs[k % ring], out=out[k % ring])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(reps):
        rx.ProcessIQData(Is[k % ring], Qs[k % ring], out=out[k % ring])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3 / frames


def main():
    args = sys.argv[1:]
    if args and args[0] == "one":
        def val(flag, default):
            return type(default)(args[args.index(flag) + 1]) if flag in args else default
        us = one(val("--frames", 32), val("--reps", 60), val("--layout", "channel"))
        print(json.dumps({"variant": args[1] if len(args) > 1 else "product", "us_per_frame": round(us, 3)}), flush=True)
        return

    def opt(flag, default):
        if flag in args:
            i = args.index(flag)
            v = type(default)(args[i + 1])
            del args[i:i + 2]
            return v
        return default
    rounds, frames, reps, layout = opt("--rounds", 3), opt("--frames", 32), opt("--reps", 60), opt("--layout", "channel")
    extra = []
    for f in ("--mode", "--agc"):
        if f in args:
            i = args.index(f)
            extra += args[i:i + 2]
            del args[i:i + 2]
    names = args
    res = {n: [] for n in names}
    for r in range(rounds):
        for n in names:
            env = dict(os.environ)
            env.pop("T41RX_LIB", None)
            if n != "product":
                env["T41RX_LIB"] = os.path.join(ROOT, "t41_sdr_amd", "abl", "libt41rx_%s.so" % n)
                env["T41RX_ALLOW_EXPERIMENT"] = "1"  # (a diagnostic build refuses t41rx_create() without it)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "one", n, "--frames", str(frames),
                                "--reps", str(reps), "--layout", layout] + extra, env=env, capture_output=True, text=True, timeout=600)
            cells = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
            if p.returncode != 0 or not cells:
                print("build %s failed: %s" % (n, p.stderr[-300:]), flush=True)
                continue
            res[n].append(cells[0]["us_per_frame"])
    for n in names:
        v = res[n]
        if v:
            print(json.dumps({"build": n, "median_us": round(statistics.median(v), 3), "min_us": round(min(v), 3), "all": v,
                              "frac_of_8TBs": round(12 * 4096 * 2048 / statistics.median(v) / 1e3 / 8000, 4)}), flush=True)


if __name__ == "__main__":
    main()
