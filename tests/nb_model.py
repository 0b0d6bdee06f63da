"""CPU models of the receive noise blanker (NoiseBlanker() / AltNoiseBlanking(), DSP_Fn.cpp:105-362; call site
Process.cpp:873-876), per 256-sample block of 24 kS/s audio.

* ``block_f32`` -- the f32 restatement: numpy float32, every sum in CMSIS-DSP's order (one f32 accumulator that starts
  at 0 and adds the terms in index order: ``acc0``; np.cumsum in float32 is such a sequential accumulator), no
  contraction.  arm_var_f32 is the two-pass form (mean, then squared deviations, / (N - 1)); ``var="onepass"`` selects
  the one-pass form of older CMSIS releases (sum and sum of squares).
* ``block_f64`` -- an independent float64 model: the same algorithm written from its definitions (Toeplitz solve for
  the predictor, lfilter, np.var), for the tolerances.

Both keep the reference's quirks: the forward seed below the block reads last_frame_end[pos + k], one sample earlier
than the x[pos - 13 + k] it stands for (``carry_fix=True`` reads the intended sample, for the tests only); the carry is
the block's input x[242 .. 254].
"""
import numpy as np

N, ORDER, PL, IMP, BOUND, MAXIMP, THRESH = 256, 10, 3, 7, 14, 20, 2.5
NCARRY = ORDER + PL
F = np.float32


def acc0(p):
    """a CMSIS single-accumulator sum: 0.0f + p[0] + p[1] + ... in float32"""
    p = np.asarray(p, F)
    return np.cumsum(np.concatenate([np.zeros(1, F), p]), dtype=F)[-1]


def _windows():
    wbw = np.array([np.float64(i) / 6.0 for i in range(IMP)]).astype(F)  # (float)(1.0 * i / (impulse_length - 1))
    return wbw[::-1].copy(), wbw


def scan(t, thr):
    """the do-while loop: search_pos = 13, hit = |t| > thr (as t > thr || t < -thr), skip PL, while < 242 and < 20 hits"""
    pos, sp = [], ORDER + PL
    while True:
        if t[sp] > thr or t[sp] < -thr:
            pos.append(sp - ORDER)
            sp += PL
        sp += 1
        if not (sp < N - BOUND and len(pos) < MAXIMP):
            return pos


def margin(t, thr):
    """smallest | |t| - thr | / thr over the scanned positions (inf where the threshold is not a positive finite number)"""
    thr = float(thr)
    if not np.isfinite(thr) or thr <= 0:
        return np.inf
    a = np.abs(t[ORDER + PL:N - BOUND].astype(np.float64))
    a = a[np.isfinite(a)]
    return float(np.min(np.abs(a - thr)) / thr) if a.size else np.inf


def block_f32(x, carry, var="twopass", carry_fix=False):
    """one block: returns (output, impulse positions, smallest threshold margin, threshold)"""
    with np.errstate(all="ignore"):
        x = np.asarray(x, F).copy()
        carry = np.asarray(carry, F)
        R = np.array([acc0(x[:N - i] * x[i:]) for i in range(ORDER + 1)], F)
        R[0] = F(np.float64(R[0]) * (1.0 + 1.0e-9))
        lp = np.zeros(ORDER + 1, F)
        lp[0] = 1
        alfa = R[0]
        for m in range(1, ORDER + 1):
            s = F(0)
            for u in range(1, m):
                s = F(s + F(lp[u] * R[m - u]))
            k = F(-F(R[m] + s) / alfa)
            anyv = lp.copy()
            for v in range(1, m):
                anyv[v] = F(lp[v] + F(k * lp[m - v]))
            lp[1:m] = anyv[1:m]
            lp[m] = k
            alfa = F(alfa * F(F(1) - F(k * k)))
        rl = lp[::-1].copy()

        def fir(c, u):  # arm_fir_f32 from a zeroed state: pCoeffs[0] on the oldest sample, taps in order
            up = np.concatenate([np.zeros(ORDER, F), u])
            acc = np.zeros(N, F)
            for j in range(ORDER + 1):
                acc = (acc + (c[j] * up[j:j + N]).astype(F)).astype(F)
            return acc

        t = fir(lp, fir(rl, x))
        if var == "twopass":
            mean = F(acc0(t) / F(N))
            sigma2 = F(acc0((t - mean) * (t - mean)) / F(N - 1))
        else:  # sum and sum of squares in one pass
            ssum, ssq = acc0(t), acc0(t * t)
            mean = F(ssum / F(N))
            sigma2 = F(F(ssq / F(N - 1)) - F(F(mean * mean) * F(F(N) / F(N - 1))))
        power = acc0(lp[:ORDER] * lp[:ORDER])
        thr = F(F(THRESH) * np.sqrt(F(sigma2 * power)))
        pos = scan(t, thr)
        fw, bw = (-rl[:ORDER]).astype(F), (-lp[1:]).astype(F)
        wfw, wbw = _windows()
        for p in pos:
            f = np.zeros(ORDER + IMP, F)
            b = np.zeros(ORDER + IMP, F)
            for k in range(ORDER):
                i = p - PL - ORDER + k
                f[k] = x[i] if i >= 0 else carry[p + k + (1 if carry_fix else 0)]
                b[IMP + k] = x[p + PL + 1 + k]
            for i in range(IMP):
                f[i + ORDER] = acc0(fw * f[i:i + ORDER])
                b[IMP - i - 1] = acc0(bw * b[IMP - i:IMP - i + ORDER])
            x[p - PL:p - PL + IMP] = ((wfw * f[ORDER:]).astype(F) + (wbw * b[:IMP]).astype(F)).astype(F)
        return x, pos, margin(t, thr), thr


def block_f64(x, carry, carry_fix=False):
    """the same block in float64 from the definitions: returns (output, impulse positions, threshold)"""
    from scipy.linalg import solve_toeplitz
    from scipy.signal import lfilter
    with np.errstate(all="ignore"):
        x = np.asarray(x, np.float64).copy()
        carry = np.asarray(carry, np.float64)
        R = np.array([np.dot(x[:N - i], x[i:]) for i in range(ORDER + 1)])
        try:
            a = solve_toeplitz(R[:ORDER], -R[1:])  # normal equations of the order-10 predictor x[n] ~ -sum a_i x[n - i]
        except (np.linalg.LinAlgError, ValueError):
            a = np.full(ORDER, np.nan)
        lp = np.concatenate([[1.0], a])
        e = lfilter(lp, [1.0], x)               # prediction error
        t = lfilter(lp[::-1], [1.0], e)         # matched filter (time-reversed error filter, 10 samples of delay)
        thr = THRESH * np.sqrt(np.var(t, ddof=1) * np.sum(lp[:ORDER] ** 2))
        pos = scan(t, thr) if np.isfinite(thr) else []
        w = np.arange(IMP) / (IMP - 1.0)
        for p in pos:
            hist = [x[p - PL - ORDER + k] if p - PL - ORDER + k >= 0 else carry[p + k + (1 if carry_fix else 0)] for k in range(ORDER)]
            fwd = []
            for _ in range(IMP):  # x[n] = -sum_i a_i x[n - i]
                nxt = -np.dot(a, hist[::-1][:ORDER])
                fwd.append(nxt)
                hist = hist[1:] + [nxt]
            fut = list(x[p + PL + 1:p + PL + 1 + ORDER])
            bwd = []
            for _ in range(IMP):  # backward: x[n] = -sum_i a_i x[n + i]
                nxt = -np.dot(a, fut[:ORDER])
                bwd.append(nxt)
                fut = [nxt] + fut[:ORDER - 1]
            bwd = bwd[::-1]
            x[p - PL:p - PL + IMP] = (1.0 - w) * np.array(fwd) + w * np.array(bwd)
        return x, pos, thr


def stream(x, carry=None, model="f32", **kw):
    """a channel's audio (a whole number of blocks) through the blanker; returns (output, per-block positions, per-block
    margins, carry after the last block).  `carry` = last_frame_end before the first block (default: power-on zero)."""
    x = np.asarray(x)
    carry = np.zeros(NCARRY + 1, F if model == "f32" else np.float64) if carry is None else np.asarray(carry)
    out = np.empty(x.shape, F if model == "f32" else np.float64)
    allpos, margins = [], []
    for b in range(x.size // N):
        blk = x[b * N:(b + 1) * N]
        if model == "f32":
            y, pos, mg, _ = block_f32(blk, carry, **kw)
        else:
            y, pos, _ = block_f64(blk, carry, **kw)
            mg = np.nan
        out[b * N:(b + 1) * N] = y
        allpos.append(pos)
        margins.append(mg)
        # the block's INPUT x[242 .. 254] (and x[255], which only the carry_fix variant reads)
        carry = np.asarray(blk[N - 1 - ORDER - PL:N], out.dtype).copy()
    return out, allpos, np.array(margins), carry
