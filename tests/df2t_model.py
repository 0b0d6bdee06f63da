"""What the CPU models of the receive equalizer (eq_model), the transmit equaliser (tx_model) and the CW narrow filter
(cw_model) share: cascades of arm_biquad_cascade_df2T_f32 sections, coefficients as CMSIS keeps them ({b0, b1, b2, a1,
a2} per section, the a's negated).

* ``cascade_oracle`` -- a cascade with persistent memories, every section the oracle's ``t41o_biquad_df2T_f32``
  (arm_biquad_cascade_df2T_f32 for one stage, oracle/t41_oracle.c): the f32 restatements' arithmetic.
* ``cascade_f32`` -- the same recurrence as a numpy float32 loop over samples from zero memories, vectorised over any
  leading axes of the coefficients (bands), with the contracted variant (every ``a*b + c`` rounded once).
* ``sos_of`` -- the coefficients as scipy's second-order sections, for the independent float64 models.
* ``block_rel`` -- per-block relative error.
"""
import numpy as np

import oracle_lib as O

F = np.float32


def cascade_oracle(coeffs, state, x):
    """x through the sections coeffs [S][5] in turn; state [S][2] (d1, d2 per section, float32) advances in place"""
    lib = O.lib()
    y = np.ascontiguousarray(x, F)
    for s in range(coeffs.shape[0]):
        c = np.ascontiguousarray(coeffs[s], F)
        st = np.ascontiguousarray(state[s])
        out = np.empty(y.size, F)
        lib.t41o_biquad_df2T_f32(O.fptr(c), O.fptr(st), O.fptr(y), O.fptr(out), y.size)
        state[s] = st
        y = out
    return y


def cascade_f32(x, coeffs, fma=False):
    """x [n] through the cascades coeffs [..., S, 5] from zero memories -> [..., n]: acc = b0*x + d1; d1 = b1*x + d2;
    d1 += a1*acc; d2 = b2*x; d2 += a2*acc in float32, one rounding per operation; ``fma=True`` rounds every a*b + c once"""
    c = np.asarray(coeffs, F)
    lead = c.shape[:-2]
    x = np.asarray(x, F)
    y = np.broadcast_to(x, lead + x.shape).copy()
    for s in range(c.shape[-2]):
        b0, b1, b2, a1, a2 = (c[..., s, i].copy() for i in range(5))
        d1, d2 = np.zeros(lead, F), np.zeros(lead, F)
        out = np.empty_like(y)
        if fma:
            b0, b1, b2, a1, a2 = (v.astype(np.float64) for v in (b0, b1, b2, a1, a2))
            for i in range(x.size):
                xi = y[..., i].astype(np.float64)
                acc = (b0 * xi + d1).astype(F)
                t = (b1 * xi + d2).astype(F)
                d1 = (a1 * acc.astype(np.float64) + t).astype(F).astype(np.float64)
                d2 = (a2 * acc.astype(np.float64) + (b2 * xi).astype(F)).astype(F).astype(np.float64)
                out[..., i] = acc
        else:
            for i in range(x.size):
                xi = y[..., i]
                acc = b0 * xi + d1
                d1 = b1 * xi + d2
                d1 = d1 + a1 * acc
                d2 = b2 * xi
                d2 = d2 + a2 * acc
                out[..., i] = acc
        y = out
    return y


def sos_of(coeffs):
    """one cascade [S][5] -> scipy sos rows [b0, b1, b2, 1, -a1, -a2] (float64)"""
    c = np.asarray(coeffs, np.float64).reshape(-1, 5)
    return np.column_stack([c[:, 0], c[:, 1], c[:, 2], np.ones(c.shape[0]), -c[:, 3], -c[:, 4]])


def block_rel(a, b, n=256):
    """per n-sample block: max|a - b| / max|b|"""
    a = np.asarray(a, np.float64).reshape(-1, n)
    b = np.asarray(b, np.float64).reshape(-1, n)
    return np.abs(a - b).max(1) / np.maximum(np.abs(b).max(1), 1e-30)
