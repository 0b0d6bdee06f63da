"""GPU box: soak of the pipelined AGC / SAM kernels (rx_chains.hpp: agc_prep_pipe) against the barrier form, bit for
bit, on random shapes -- the hand-over between waves rests on the CU's in-order vector memory path and LDS flags; a
race would show as a mismatch in some run.  One call of n frames (pipelined) against the same stream in calls of at
most three frames (barrier form), outputs and checkpoints compared; now and then the full 4096 x 32 shape.
usage: python tools/pipe_soak.py [seconds]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
L = 2048


def main():
    import torch
    import t41_sdr_amd as T
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 300.0
    rng = np.random.default_rng(int(time.time()))
    g = torch.Generator(device="cuda").manual_seed(int(rng.integers(1 << 30)))
    t0, runs, frames, bad, nonfinite, nan_payload, changed = time.time(), 0, 0, [], 0, 0, 0
    while time.time() - t0 < budget:
        big = runs % 25 == 24
        nch = 4096 if big else int(rng.choice([1, 2, 3, 5, 15, 16, 17, 31, 33, 64, 100, 255, 256, 300, 1000]))
        nfr = 32 if big else int(rng.integers(4, 41))
        mode = int(rng.choice([0, 1, 2, 3, 8]))
        agc = int(rng.integers(0, 5)) if mode == 8 else int(rng.integers(1, 5))  # (SAM: PLL alone, or behind the AGC -- two chains)
        flo, fhi = {0: (200, 3000), 1: (-3000, -200), 2: (-3000, 3000), 3: (200, 3000), 8: (-3000, 3000)}[mode]
        kw = dict(mode=mode, AGCMode=agc, FLoCut=flo, FHiCut=fhi)
        nco = (rng.integers(-860, 801, nch) * 50).astype(np.int32)
        # noise with a slow random envelope: the gain law keeps changing state
        env = torch.rand(nch, nfr * 8, generator=g, device="cuda").repeat_interleave(L // 8, dim=1) ** 3
        I = (0.3 * env * torch.randn(nch, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
        Q = (0.3 * env * torch.randn(nch, nfr * L, generator=g, device="cuda")).clamp_(-0.999, 0.999)
        q15 = runs % 3 == 2  # every third run on the firmware's wire format (q15 queues in, q15 samples out)
        if q15:
            I = (I * 32768.0).round_().clamp_(-32768, 32767).to(torch.int16)
            Q = (Q * 32768.0).round_().clamp_(-32768, 32767).to(torch.int16)
        # round 5: in a third of the runs with the AGC on, AGC_thresh changes mid-stream (a live CalcFilters(): min_volts
        # jumps up or down under lanes in their decay states -- the case ADVICE r04 found the per-block short-cut unsound for)
        cutf, thr0, thr1 = None, 20, 20
        if agc and nfr >= 8 and rng.random() < 0.34:
            cutf = int(rng.integers(4, nfr - 3))
            thr0, thr1 = int(rng.integers(-20, 91)), int(rng.integers(-20, 91))
            kw["AGC_thresh"] = thr0
        rx1 = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
        run = (lambda rx, a, b: rx.ProcessIQData_q15(b, a)) if q15 else (lambda rx, a, b: rx.ProcessIQData(a, b))
        if cutf is None:
            whole = run(rx1, I, Q)
        else:  # two pipelined calls (>= 4 frames each) around the change
            w1 = run(rx1, I[:, :cutf * L].contiguous(), Q[:, :cutf * L].contiguous())
            rx1.CalcFilters(AGC_thresh=thr1)
            whole = torch.cat([w1, run(rx1, I[:, cutf * L:].contiguous(), Q[:, cutf * L:].contiguous())], dim=1)
        rx2 = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
        parts, pos = [], 0
        while pos < nfr:
            n = min(int(rng.integers(1, 4)), nfr - pos)
            if cutf is not None and pos < cutf:
                n = min(n, cutf - pos)
            if cutf is not None and pos == cutf:
                rx2.CalcFilters(AGC_thresh=thr1)
            parts.append(run(rx2, I[:, pos * L:(pos + n) * L].contiguous(), Q[:, pos * L:(pos + n) * L].contiguous()))
            pos += n
        short = torch.cat(parts, dim=1)
        # (bitwise: NFM divides by |z|^2, and an envelope this deep underflows it to 0 now and then -- NaNs, in both forms alike)
        bits = torch.int16 if q15 else torch.int32
        s1, s2 = np.asarray(rx1.get_state()), np.asarray(rx2.get_state())
        same_state = bool(np.array_equal(s1, s2))
        if not same_state and s1.shape == s2.shape:
            # A stream that went NaN (NFM's discriminator divides by |z|^2: exact zeros on the q15 format give 0 / 0) leaves NaNs in
            # the AGC's back-averages in BOTH forms; which payload / sign a NaN carries through a product or a sum depends on
            # the operand order the compiler chose per kernel variant.  Not a difference of values: counted apart.
            w1 = np.frombuffer(s1.tobytes()[32:32 + (s1.nbytes - 32) // 4 * 4], np.uint32)
            w2 = np.frombuffer(s2.tobytes()[32:32 + (s2.nbytes - 32) // 4 * 4], np.uint32)
            d = w1 != w2
            if s1.tobytes()[:32] == s2.tobytes()[:32] and bool((np.isnan(w1.view(np.float32)[d]) & np.isnan(w2.view(np.float32)[d])).all()):
                same_state = True
                nan_payload += 1
        same = bool(torch.equal(whole.view(bits), short.view(bits))) and same_state
        finite = True if q15 else bool(torch.isfinite(whole).all())
        nonfinite += 0 if finite else 1
        if not same:
            bad.append(dict(run=runs, nch=nch, nfr=nfr, kw=kw, same=same, finite=finite))
            print("MISMATCH", bad[-1], flush=True)
        runs += 1
        changed += 0 if cutf is None else 1
        frames += nch * nfr
        del rx1, rx2, I, Q, env, whole, short, parts
        if runs % 20 == 0:
            print("%d runs, %.1f M channel-frames, %d mismatches, %.0f s" % (runs, frames / 1e6, len(bad), time.time() - t0), flush=True)
    print(json.dumps({"runs": runs, "channel_frames": frames, "runs_with_AGC_thresh_changed_mid_stream": changed, "mismatches": len(bad), "runs_with_nonfinite_samples": nonfinite, "runs_whose_checkpoints_differ_in_nan_payloads_only": nan_payload,
                      "seconds": round(time.time() - t0, 1)}), flush=True)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
