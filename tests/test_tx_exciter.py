"""The transmit exciter, ExciterIQData() (Exciter.cpp:46-169).  CPU: the oracle's
restatement against an independent float64 scipy stream model and the C ABI's symbols; GPU: the HIP
path against the oracle on q15 samples, bit for bit (the reference itself holds no vectors for it).
Its edges -- shapes, modes, rails, impulses, streaming, refusals -- are in test_tx_exciter_edges.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from tx_harness import F, mic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def stream_model(q, mode, amp, phase, tabs):
    """whole-stream float64 model (no frames, no CMSIS state): lfilter / slicing / zero stuffing"""
    from scipy.signal import lfilter
    c192, c48, h45, hn45 = [t.astype(np.float64) for t in tabs]
    x = q.astype(np.float64) / 32768.0
    # CMSIS holds the taps time-reversed: y[n] = sum_i c[i] x[n - (T - 1) + i]
    d1 = lfilter(c192[::-1], 1.0, x)[0::4]
    d2 = lfilter(c48[:24][::-1], 1.0, d1)[0::2]
    I = lfilter(h45[::-1], 1.0, d2)
    Q = lfilter(hn45[::-1], 1.0, d2)
    if mode in (O.DEMOD_LSB, O.DEMOD_USB):
        I = I * (amp if mode == O.DEMOD_LSB else -amp)
        if phase < 0:
            Q = Q + I * phase
        else:
            I = I + Q * phase

    def interp(v, L, c):  # arm_fir_interpolate_f32: zero stuffing + the same time-reversed taps, no make-up gain
        up = np.zeros(v.size * L)
        up[::L] = v
        return lfilter(c[::-1], 1.0, up)

    return [interp(interp(v, 2, c48), 4, c192[:32]) * 20.0 for v in (I, Q)]


def test_tx_oracle_matches_a_float64_stream_model():
    nch, nfr = 2, 4
    q = mic(nch, nfr)
    for mode, amp, phase in ((O.DEMOD_USB, 1.0, 0.0), (O.DEMOD_LSB, 0.97, -0.02), (O.DEMOD_USB, 1.03, 0.015)):
        ob = O.TxOracleBatch(nch, mode, amp, phase)
        tabs = [ob.table(i) for i in range(4)]
        oL, oR = ob.process(q)
        for c in range(nch):
            mI, mQ = stream_model(q[c], mode, amp, phase, tabs)
            n = min(mI.size, oL.shape[1])
            # q15 grid: the float chains agree to ~1e-6 of full scale, truncation adds one LSB
            assert np.abs(oL[c, :n] - np.trunc(mI[:n] * 32768.0)).max() <= 2, (mode, c)
            assert np.abs(oR[c, :n] - np.trunc(mQ[:n] * 32768.0)).max() <= 2, (mode, c)
        # it is an SSB exciter: I and Q are in quadrature (analytic signal) over the speech band
        # (with the deliberate pre-distortion of the other two cases the suppression is ~35 dB)
        if amp != 1.0 or phase != 0.0:
            continue
        z = (oL[0].astype(np.float64) + 1j * oR[0].astype(np.float64))[2 * F:]
        spec = np.abs(np.fft.fft(z * np.hanning(z.size)))
        f = np.fft.fftfreq(z.size, 1 / 192000.0)
        pos, neg = spec[(f > 300) & (f < 2800)].max(), spec[(f < -300) & (f > -2800)].max()
        assert max(pos, neg) > 100 * min(pos, neg), (mode, pos, neg)  # one sideband only


def test_tx_abi_symbols_and_struct(built):
    import t41_sdr_amd as T
    from t41_sdr_amd import tx
    hdr = open(os.path.join(ROOT, "include", "t41tx.h")).read()
    hdr_nc = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(t41tx_[a-z0-9_]+)\s*\(", hdr_nc))
    lib = C.CDLL(T.LIB_PATH)
    assert declared and all(hasattr(lib, s) for s in declared)
    assert declared == set(tx.TX_SYMBOLS)
    body = re.search(r"typedef struct t41tx_params \{(.*?)\} t41tx_params;", hdr_nc, re.S).group(1)
    fields = re.findall(r"(int32_t|float)\s+(\w+);", body)
    assert [n for _, n in fields] == [n for n, _ in tx.TxParams._fields_]
    p = T.default_tx_params()
    assert (p.mode, p.IQXAmpCorrectionFactor, p.IQXPhaseCorrectionFactor) == (0, 1.0, 0.0)
    # product tables == the oracle's copies of the reference tables (both extracted from FIR.cpp)
    ob = O.TxOracleBatch(1)
    assert ob.table(0).size == 48 and ob.table(2).size == 100


@pytest.mark.gpu
@pytest.mark.parametrize("mode,amp,phase", [(0, 1.0, 0.0), (1, 0.97, -0.02), (0, 1.03, 0.015), (2, 1.0, 0.0)],
                         ids=["usb", "lsb-corr", "usb-corr", "am-no-correction"])
def test_gpu_tx_parity(built, mode, amp, phase):
    import torch
    import t41_sdr_amd as T
    nch, nfr = 9, 5
    q = mic(nch, nfr, seed=3, level=0.9 if mode == 0 else 0.4)
    refL, refR = O.TxOracleBatch(nch, mode, amp, phase).process(q)
    tx = T.TxChain(nch, T.default_tx_params(mode=mode, IQXAmpCorrectionFactor=amp, IQXPhaseCorrectionFactor=phase))
    gL, gR = tx.ExciterIQData(torch.from_numpy(q).cuda())
    torch.cuda.synchronize()
    gL, gR = gL.cpu().numpy(), gR.cpu().numpy()
    # the same IEEE f32 operations in the same order, denormals kept: bit-identical
    for g, r in ((gL, refL), (gR, refR)):
        d = np.abs(g.astype(np.int32) - r.astype(np.int32))
        assert np.array_equal(g, r), (int(d.max()), int((d > 0).sum()))
    assert np.abs(refL).max() > 1000            # a real signal came out
    # frame by frame through the host entry == one device call (the delay lines carry over)
    tx.reset()
    parts = [tx.ExciterIQData(np.ascontiguousarray(q[:, k * F:(k + 1) * F])) for k in range(nfr)]
    assert np.array_equal(np.concatenate([p[0] for p in parts], axis=1), gL)
    assert np.array_equal(np.concatenate([p[1] for p in parts], axis=1), gR)
    with pytest.raises(ValueError):
        tx.ExciterIQData(torch.zeros(nch, 1000, dtype=torch.int16, device="cuda"))
