"""FT8 receive up to the waterfall: the restatement (tests/ft8_model.py) on its own, no device.

The q15 transform against numpy's float64 rfft, a synthetic FT8 transmission read back from the model's waterfall, the
collector's quirks (literal loop against the closed parallel form the kernel uses), and the slot timing with the default
clock.  The kernel is held to this model bit for bit in test_ft8_receive.py.
"""
import os

import numpy as np

import ft8_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRANSFORM_ERR_LSB = 12.63  # measured below: the largest |q15 bin - float64 bin| over bins 0..736 of the four inputs


def _transform_inputs():
    n = np.arange(M.FFT_SIZE)
    rng = np.random.default_rng(1)
    x = sum(np.cos(2 * np.pi * f * n / M.FFT_SIZE + p) for f, p in ((37, 0.3), (200.5, 1.1), (511, 2.0), (700.25, 0.7)))
    return np.array([np.round(x / np.abs(x).max() * 32767),                      # full-scale multi-tone
                     np.round(32767 * np.cos(2 * np.pi * 100 * n / M.FFT_SIZE)),  # one full-scale tone on a bin
                     rng.choice([-32768, 32767], M.FFT_SIZE),                     # +-full-scale noise
                     rng.integers(-32768, 32768, M.FFT_SIZE)]).astype(np.int64)   # uniform noise


def test_q15_transform_against_float64():
    """arm_rfft_q15 as restated, bins 0..736, against np.fft.rfft / 2048 in float64 on a full-scale multi-tone, a
    full-scale tone and +-full-scale and uniform noise.  Measured: 4.25, 2.02, 12.62 and 4.33 output LSBs (the q15
    stages floor every halving and saturate sums of full-scale noise); the bound is twice the largest, 2 x 12.63."""
    X = _transform_inputs()
    re, im = M.rfft2048_q15(X)
    ref = np.fft.rfft(X.astype(np.float64), axis=-1)[:, :M.BINS] / M.FFT_SIZE
    err = np.maximum(np.abs(re - ref.real), np.abs(im - ref.imag)).max(axis=1)
    print("q15 transform, largest error per input [LSB]:", np.round(err, 3), "peaks", np.round(np.abs(ref).max(axis=1), 1))
    assert np.abs(ref).max() > 16000  # the full-scale tone reaches half of full scale: X[k] / 2048
    assert err.max() <= 2 * TRANSFORM_ERR_LSB
    assert im[:, 0].max() == 0 and im[:, 0].min() == 0


def test_tables():
    w, m = M.ft8_tables()
    assert w.dtype == np.float32 and w.shape == (2048,) and m.dtype == np.float32 and m.shape == (16385,)
    assert abs(float(w[0])) < 1e-6 and 0.9999 < float(w.max()) <= 1.0 and np.allclose(w, w[::-1], atol=2e-6)
    assert m[0] == np.float32(10.0 * np.log(0.1)) and abs(float(m[16384]) - 120.07) < 0.01 and (np.diff(m) >= 0).all()
    import t41_sdr_amd.rx as rx  # the package's ft8_tables() is the same computation
    w2, m2 = rx.ft8_tables()
    assert np.array_equal(w, w2) and np.array_equal(m, m2)


# ---- a synthetic FT8 transmission --------------------------------------------------------------------------------------
J0 = 160  # tone 0 at 160 x 6.25 Hz = 1000 Hz: row index J0 + tone at freq_sub 0
# Full scale for this stage is where arm_shift_q15(., 5, .) starts to saturate: a tone of amplitude A (of the q15 range) on
# a bin gives A x 32768 x 0.42 (the Blackman window's mean) x 1024 / 2048 in arm_rfft_q15's output, and x 32 of that passes
# 32767 at A = 0.149.  Above it the tone's bins and the neighbouring tone's clip component by component and which of them
# reads larger hangs on their phases -- in the firmware as in any arithmetic (at 0.9 of the q15 range the model reads 66 of
# the 79 symbols, test_q15_full_scale_saturates_the_shift).  The transmission is built just below: 0.14.
AMP = 0.14


def _transmission(seed=8, amp=AMP):
    costas = np.load(os.path.join(ROOT, "tests", "golden", "ft8", "costas.npz"))["kCostas_map"]
    assert tuple(costas) == M.KCOSTAS
    rng = np.random.default_rng(seed)
    tones = rng.integers(0, 8, 79)
    for s0 in (0, 36, 72):
        tones[s0:s0 + 7] = costas
    # 8-FSK, 6.25 Hz spacing, 0.16 s per symbol = 3840 samples @24 kS/s = 15 frames, continuous phase, from a gulp boundary
    f = np.repeat(6.25 * (J0 + tones), 3840)
    ph = 2 * np.pi * np.cumsum(f) / 24000.0
    return tones, (amp * np.sin(ph)).astype(np.float32)


def _float64_waterfall(x, window):
    """the same pipeline in float64: the collector as written (its forwarding included) on unquantised samples, the
    window, rfft, power in dB, the pair averages of freq_sub 0; [block][time_sub 0 / 512][368]"""
    buf, dl, lo, rows = np.zeros(M.BUF_WORDS), 0, 0, []
    for fr in x.astype(np.float64).reshape(-1, 256):
        M.collect_literal(buf, fr, dl, lo)
        dl += 1
        if dl == 15:
            buf[3071], dl, lo = fr[255], 0, 0
            r = []
            for ts in (0, 512):
                p = np.abs(np.fft.rfft(buf[ts:ts + M.FFT_SIZE] * window.astype(np.float64))) ** 2
                db = 10 * np.log10(p[:M.BINS] + 1e-9)
                r.append((db[0:736:2] + db[1:737:2]) / 2)
            rows.append(r)
        elif dl in (4, 8, 12):
            buf[2048 + dl * 68 + lo] = fr[255]
            lo += 1
    return np.array(rows)


def test_synthetic_transmission_reads_back():
    """79 symbols, Costas arrays at 0 / 36 / 72, 58 random tones; symbol s fills gulp s.  Which row holds it follows
    from the collector's forwarding: from frame 4 of a gulp on (leftover >= 1) the middle third of the buffer takes the
    samples the same frame has just written, so behind gulp s the middle third holds gulp s too (its first 272 words
    gulp s - 1), and the time_sub 512 window, centred on the middle third, is dominated by symbol s.  In row [block s]
    [time_sub 512][freq_sub 0] the argmax over the 8 tone bins is the transmitted tone in all 79 symbols -- first in
    float64, then in the model"""
    tones, x = _transmission()
    w, m = M.ft8_tables()
    ref = _float64_waterfall(x, w)
    assert ref.shape == (79, 2, M.ROW)
    assert np.array_equal(np.argmax(ref[:, 1, J0:J0 + 8], axis=1), tones)
    mod = M.FT8Model(1, w, m)
    mod.collect = M.collect_closed_form  # (held to the literal loop below)
    mod.sync()
    st = mod.process(x[None, :])
    assert st[0, -1, 0] == 79 and (st[0, :, 2] == 0).all()
    wf = mod.power[0, 0, :79 * M.BLOCK_BYTES].reshape(79, 2, 2, M.ROW)
    assert np.array_equal(np.argmax(wf[:, 1, 0, J0:J0 + 8], axis=1), tones)
    assert 100 <= wf[40, 1, 0, J0:J0 + 8].max() <= wf.max() < 113  # near the top of the range, below any clipped component


def test_q15_full_scale_saturates_the_shift():
    """the same transmission at 0.9 of the q15 range: arm_shift_q15 clips the tone's bins (a bin with one component
    clipped reads 10 ln(81910) = 113, with both 120) and the argmax no longer names the tone in every symbol"""
    tones, x = _transmission(amp=0.9)
    w, m = M.ft8_tables()
    mod = M.FT8Model(1, w, m)
    mod.collect = M.collect_closed_form
    mod.sync()
    mod.process(x[None, :15 * 20 * 256])
    wf = mod.power[0, 0, :20 * M.BLOCK_BYTES].reshape(20, 2, 2, M.ROW)
    assert wf.max() == 120 and (wf[:, 1, 0, J0:J0 + 8].max(axis=1) >= 113).all()
    good = int((np.argmax(wf[:, 1, 0, J0:J0 + 8], axis=1) == tones[:20]).sum())
    print("symbols read at 0.9 of the q15 range: %d of 20" % good)
    assert good < 20


# ---- the collector -----------------------------------------------------------------------------------------------------
def test_collector_quirks_and_closed_form():
    """a ramp through several gulps: words 1020..1023 and 2044..2047 stay zero, the literal loop and the closed form
    agree in every frame (same-frame forwarding at leftover 1..3 included), and the leftover cell written behind
    frames 3 / 7 / 11 is rolled by the next frame"""
    w, m = M.ft8_tables()
    lit, par = M.FT8Model(1, w, m), M.FT8Model(1, w, m)
    par.collect = M.collect_closed_form
    for mod in (lit, par):
        mod.sync()
        mod.scal[0, M.S_FT8FLAG] = 0  # (the collector alone: no block, and no restart inside 50 frames)
        mod.scal[0, M.S_START] = (-5000) & 0xFFFFFFFF
    x = ((np.arange(50 * 256) % 30000 + 1) / 32768.0).astype(np.float32).reshape(50, 256)
    q = M.float_to_q15(x)
    assert np.array_equal(q.ravel(), np.arange(50 * 256) + 1)  # a ramp 1, 2, 3, ..: every cell names its source sample
    for f in range(50):
        dl, lo = int(lit.scal[0, M.S_DATALOOP]), int(lit.scal[0, M.S_LEFTOVER])
        assert lo == dl // 4
        before = lit.buf[0].copy()
        lit.frame(0, x[f])
        par.frame(0, x[f])
        assert np.array_equal(lit.buf, par.buf) and np.array_equal(lit.scal, par.scal), f
        b, k = lit.buf[0], 68 * dl
        if lo >= 1:
            # forwarding: the middle third's words k + lo .. k + 67 hold THIS frame's samples, not the last third's old ones
            assert np.array_equal(b[1024 + k + lo:1024 + k + 68], q[f, (np.arange(68 - lo) * 15) // 4])
            assert np.array_equal(b[1024 + k:1024 + k + lo], before[2048 + k:2048 + k + lo])
            if dl in (4, 8, 12):  # the cell behind frame 3 / 7 / 11 (sample 255 of the frame before) is rolled by this one
                assert b[1024 + k + lo - 1] == q[f - 1, 255]
        assert np.array_equal(b[2048 + k + lo:2048 + k + lo + 68], q[f, (np.arange(68) * 15) // 4])
    b = lit.buf[0]
    assert not b[1020:1024].any() and not b[2044:2048].any()
    assert b[:1020].all() and b[1024:2044].all() and b[2048:].all()  # everything else has been reached
    assert lit.scal[0, M.S_DSPFLAG] == 1 and lit.scal[0, M.S_N] == 50


def test_float_to_q15_truncates_and_saturates():
    x = np.array([0.99999, -0.99999, 1.5, -1.5, 1.0, -1.0, 3.05e-5, -3.05e-5, 3.06e-5, 1e30, -1e30], np.float32)
    assert M.float_to_q15(x).tolist() == [32767, -32767, 32767, -32768, 32767, -32768, 0, 0, 1, 32767, -32768]


# ---- slot timing -------------------------------------------------------------------------------------------------------
def test_slot_timing_default_clock():
    """sync at n = 0, millis(n) = floor(32 n / 3): block b fires in frame 15 b + 14, the completion is reported in frame
    1379 alone, ft8_flag returns in frame 1407 (millis = 15008, the first with millis % 15000 <= 200), and the DSP_Flag
    left standing since frame 1394 makes block 0 of the second slot fire in frame 1408, off the 15-frame phase, into the
    other half"""
    w, m = M.ft8_tables()
    mod = M.FT8Model(1, w, m)
    mod.collect = M.collect_closed_form
    mod.sync()
    rng = np.random.default_rng(3)
    x = (0.3 * rng.standard_normal(1410 * 256)).astype(np.float32)
    st = mod.process(x[None, :1409 * 256])[0]
    first = [n for n in range(1380, 1500) if mod.millis(n) % 15000 <= 200][0]
    assert first == 1407 and mod.millis(1407) == 15008
    assert np.array_equal(np.nonzero(st[:, 2])[0], [1379]) and st[1379].tolist() == [92, 0, 1, 0]
    assert np.array_equal(st[14::15][:92, 0], np.arange(1, 93)) and (st[:1379, 1] == 1).all()
    assert (st[1379:1407, 1] == 0).all() and (st[1379:1407, 0] == 92).all()
    assert st[1407].tolist() == [0, 1, 0, 1407 % 15 + 1] and st[1408].tolist() == [1, 1, 0, 1408 % 15 + 1]
    assert mod.scal[0, M.S_HALF] == 1 and mod.scal[0, M.S_DSPFLAG] == 0
    half0 = mod.power[0, 0].copy()
    assert half0.reshape(92, -1).any(axis=1).all()
    assert mod.power[0, 1, :M.BLOCK_BYTES].any() and not mod.power[0, 1, M.BLOCK_BYTES:].any()
    st2 = mod.process(x[None, 1409 * 256:])[0]  # frame 1409 = 15 x 93 + 14: back on the phase, block 1
    assert st2[0].tolist() == [2, 1, 0, 0] and mod.power[0, 1, M.BLOCK_BYTES:2 * M.BLOCK_BYTES].any()
    assert np.array_equal(mod.power[0, 0], half0)  # the finished slot stays readable


def test_record_round_trip():
    w, m = M.ft8_tables()
    a = M.FT8Model(2, w, m, t0=-5)
    a.sync([0, 1])
    x = (0.2 * np.random.default_rng(4).standard_normal((2, 20 * 256))).astype(np.float32)
    a.process(x)
    rec = a.record()
    assert rec.size == 32 + 4 * 2 * M.WORDS and bytes(rec[:4]) == b"T41F"
    words = rec.view(np.int32)[8:].reshape(2, M.WORDS)
    assert words[0, M.S_N] == 20 and words[0, M.S_SYNC] == 0 and not words[0, M.SCALARS:].any()
    assert words[1, M.S_SYNC] == 1 and words[1, M.S_START] == -5 and words[1, M.S_COUNTER] == 1 and words[1, M.S_DATALOOP] == 5
    b = M.FT8Model(2, w, m, t0=-5)
    b.load_record(rec)
    assert np.array_equal(a.process(x), b.process(x)) and np.array_equal(a.record(), b.record())
