"""The CPU-side reference pieces of the stage tests, once: what stands between the HIP path's own demodulated audio (the
`demod` tap, 24 kS/s, 256 samples per frame) and the audio it puts out.  A test file's stage24() is a composition of
these plus its own stage model.
"""
import ctypes as C

import numpy as np

import nb_model as NB
import oracle_lib as O

L, D = 2048, 256


def vol_scale(audioVolume=30):
    x = np.float32(audioVolume) / np.float32(100.0)
    ampl = np.float32(5) * x * x * x * x * x
    return np.float32(8.0) * ampl  # DF * VolumeToAmplification(), Process.cpp:929, 955-967


def interp(a24, kw):
    """the oracle's interpolators and volume (Process.cpp:917-931), continuous over the stream: [nch, n] -> [nch, 8 n]"""
    lib = O.lib()
    p = O.default_params(**kw)
    c = O.design(p)
    nch, n = a24.shape
    out = np.empty((nch, 8 * n), np.float32)
    for ch in range(nch):
        st1, st2 = np.zeros(23 + D, np.float32), np.zeros(7 + 2 * D, np.float32)
        mid, hi = np.empty(2 * D, np.float32), np.empty(8 * D, np.float32)
        for b in range(n // D):
            blk = np.ascontiguousarray(a24[ch, b * D:(b + 1) * D], np.float32)
            lib.t41o_fir_interpolate_f32(c.int1, 48, 2, O.fptr(st1), O.fptr(blk), O.fptr(mid), D)
            lib.t41o_fir_interpolate_f32(c.int2, 32, 4, O.fptr(st2), O.fptr(mid), O.fptr(hi), 2 * D)
            out[ch, b * L:(b + 1) * L] = hi * vol_scale(p.audioVolume)
    return out


def nr_stage(a, p):
    """the oracle's noise reduction / notch (Process.cpp:841-866) over one channel's 256-sample blocks, from power-on;
    a is changed in place and returned"""
    lib = O.lib()
    R = np.zeros(D, np.float32)
    s = lib.t41o_nr_create()
    for b in range(a.size // D):
        blk = a[b * D:(b + 1) * D].copy()
        lib.t41o_nr_block(s, C.byref(p), O.fptr(blk), O.fptr(R))
        a[b * D:(b + 1) * D] = blk
    lib.t41o_nr_destroy(s)
    return a


def nb_stage(a, model="f32", on=None, carry=None):
    """the blanker model (tests/nb_model.py) over one channel's blocks where on[b] (default: all); the carry is the
    input of the last block the blanker saw, as in the reference.  a is changed in place; returns (a, the positions
    per block (None where off), the f32 model's magnitudes per block (nan where off or f64))"""
    nb = a.size // D
    cy = np.zeros(NB.NCARRY + 1) if carry is None else carry
    pos_ch, mags = [], np.full(nb, np.nan)
    for b in range(nb):
        blk = a[b * D:(b + 1) * D]
        if on is not None and not on[b]:
            pos_ch.append(None)
            continue
        if model == "f32":
            y, pos, mags[b], _ = NB.block_f32(blk, cy)
        else:
            y, pos, _ = NB.block_f64(blk, cy)
        pos_ch.append(pos)
        cy = blk[NB.N - 1 - NB.ORDER - NB.PL:].copy()
        a[b * D:(b + 1) * D] = y
    return a, pos_ch, mags
