"""IQ calibration: ProcessIQData2() (Process2.cpp:295-399) and PlotCalSpectrum()'s sideband measurement (:478-547).
CPU: the f32 restatements of tests/cal_model.py against independent float64 models, log10f_fast, the robustness of the
window maxima the GPU comparison leans on, the window / mode mapping, the updateDisplayFlag property, the closed loop on
the model, the C ABI's new symbols and refusals, and cal_tone().
GPU: tx_cal_kernel against the restatement bit for bit on q15; cal_kernel's FFT_spec within the display side output's
tolerances, its pixels and results exactly from its own FFT_spec, and end to end against the model; the sweep."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import cal_model as M
import oracle_lib as O
from rx_harness import to_q15
from test_cw_exciter import assert_same, cat, mic, rows
from test_display_spectrum import ZOOM_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, R = 2048, 512
USB, LSB, AM = O.DEMOD_USB, O.DEMOD_LSB, O.DEMOD_AM
OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2
TX_CASES = {"usb": (USB, 1.0, 0.0), "lsb-corr": (LSB, 0.97, -0.02), "usb-corr": (USB, 1.03, 0.015), "am": (AM, 1.0, 0.3)}
TX_SYMBOLS = ("t41tx_set_cal_tone", "t41tx_set_cal_corrections", "t41tx_process_cal_device_q15", "t41tx_process_cal_host_q15")
RX_SYMBOLS = ("t41rx_set_calibration", "t41rx_set_cal_corrections", "t41rx_calibrate_device", "t41rx_calibrate_device_q15",
              "t41rx_calibrate_host", "t41rx_calibrate_host_q15")


@functools.lru_cache(maxsize=None)
def tone():
    c, s = M.cal_tone()
    c.setflags(write=False)
    s.setflags(write=False)
    return c, s


@functools.lru_cache(maxsize=None)
def tx_cold(case, level=0.5, nfr=5):
    """the model's first nfr calibration frames from power-on, one channel: computed once, shared, never written to"""
    mode, amp, phase = TX_CASES[case]
    out = M.CalTxModelBatch(1, mode, amp, phase, cal=tone(), level=level).process_cal(nfr)
    for a in out:
        a.setflags(write=False)
    return out


def bin_hz(b, zoom, mode):
    """input frequency that shows at display bin b: 375 Hz / 2^zoom per bin around DC at 256, FreqShift1() moves up by
    Fs/4, and in USB / LSB the correction's I x -IQAmp mirrors the spectrum in front of it"""
    f = (b - 256) * 375.0 / (1 << zoom) - 48000.0
    return -f if mode in (USB, LSB) else f


@functools.lru_cache(maxsize=None)
def two_tones(nch, nfr, zoom, bins, mode=LSB, levels=None, seed=3, noise=1e-4):
    """I / Q float32 [nch, nfr * 2048]: a tone in the middle of each window, levels a few percent apart per channel.  The
    second tone lies 15 dB (zoom 0), 6 dB (zoom 2) or 2 dB (zoom 4) under the first: ZOOM_TOL grows with the zoom, and
    the window maxima must stay far above it (test_window_maxima_are_robust_to_the_spectrum_tolerance)"""
    levels = LEVELS[zoom] if levels is None else levels
    rng = np.random.default_rng(seed)
    n = np.arange(nfr * F)
    x = np.zeros((nch, n.size), complex)
    for c in range(nch):
        for b, a in zip(bins, levels):
            x[c] += a * (1.0 + 0.03 * c) * np.exp(1j * (2 * np.pi * bin_hz(b, zoom, mode) / 192000.0 * n + 0.7 * c))
        x[c] += noise * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
    I, Q = x.real.astype(np.float32), x.imag.astype(np.float32)
    I.setflags(write=False)
    Q.setflags(write=False)
    return I, Q


LEVELS = {0: (0.21, 0.037), 2: (0.21, 0.1), 4: (0.21273, 0.17221)}


def to_queues(I, Q):
    """the q15 wire format: float_buffer_L (= I) is filled from the R queue, float_buffer_R (= Q) from the L queue"""
    return to_q15(Q), to_q15(I)  # Q_in_L, Q_in_R


def corrections(nch):
    """per-channel candidates, all different, both signs of the phase factor"""
    c = np.arange(nch)
    return (1.0 + 0.004 * ((c % 21) - 10) + 1e-4 * c).astype(np.float32), (0.003 * (((c * 7) % 13) - 6) - 1e-5 * c).astype(np.float32)


def model_run(I, Q, mode, zoom, bins, mask=None, amps=None, phases=None, q15=False, shared=False, nch=None, **kw):
    """the f32 restatement on every channel -> spec [nch, nfr, 512] (NaN rows where unflagged), pixel, result"""
    nch = I.shape[0] if nch is None else nch
    out = []
    for c in range(nch):
        a = 1.0 if amps is None else amps[c]
        p = 0.0 if phases is None else phases[c]
        r = 0 if shared else c
        out.append(M.CalRxModel(mode, a, p, zoom, bins=bins, **kw).run(I[r], Q[r], mask, q15))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def count_moves(a, b):
    d = np.abs(np.asarray(a, np.int64) - np.asarray(b, np.int64))
    return int(d.max()), float((d != 0).mean())


# the receive cases both the CPU robustness test and the GPU comparison run: name -> (mode, zoom, bins, n_frames, mask)
RX_CASES = {
    "lsb-z0": (LSB, 0, (310, 460), 4, None),
    "usb-z0": (USB, 0, (65, 192), 4, (1, 0, 0, 1)),
    "usb-z2": (USB, 2, (209, 273), 4, (1, 0, 0, 1)),
    "lsb-z2": (LSB, 2, (240, 305), 4, (1, 0, 0, 0)),
    "lsb-z4": (LSB, 4, (240, 305), 4, None),
    "edges-z0": (LSB, 0, (12, 502), 1, None),
}


# ---- CPU: the models
def test_exciter_model_matches_a_float64_stream_model():
    """The bound is measured between two CPU models, neither the code under test: over these 8 inputs (4 mode / correction
    cases x levels 0.5 and 0.9, 4 frames) the f32 restatement lands on the float64 stream model's q15 value everywhere
    (measured: 0 LSB; the float chains agree to ~1e-7 of full scale, so a truncation that falls on the other side of an
    integer is possible and costs one LSB).  The bound is the 2 LSB test_cw_exciter.py uses, for the same reason: twice
    that one LSB.  Peaks lie at 2.1 k - 4.0 k LSB (no x 20 here): nothing saturates."""
    bound, nfr = 2, 4
    tabs = [O.TxOracleBatch(0).table(i) for i in range(4)]
    worst, peaks = 0, []
    for level in (0.5, 0.9):
        for case, (mode, amp, phase) in TX_CASES.items():
            got = M.CalTxModelBatch(1, mode, amp, phase, cal=tone(), level=level).process_cal(nfr)
            want = M.cal_tx_stream_model_f64(*tone(), level, nfr, mode, amp, phase, tabs)
            for o, m in zip(got, want):
                w = np.trunc(np.clip(m * 32768.0, -32768, 32767))
                worst = max(worst, int(np.abs(o[0] - w).max()))
                peaks.append(int(np.abs(o[0].astype(np.int32)).max()))
    print("calibration exciter, f32 restatement vs float64 stream model: max deviation %d LSB; peaks %d .. %d LSB" % (worst, min(peaks), max(peaks)))
    assert max(peaks) < 32767 and min(peaks) > 1500
    assert worst <= bound, worst


def test_exciter_model_properties():
    """frames repeat from the second on; LSB is USB with I negated at amplitude 1 / phase 0; AM applies no correction"""
    for case in TX_CASES:
        oL, oR = tx_cold(case)
        for o in (oL, oR):
            fr = o[0].reshape(5, F)
            assert not np.array_equal(fr[0], fr[1]) and all(np.array_equal(fr[1], fr[k]) for k in (2, 3, 4))
    neg = lambda x: (-x.astype(np.int32)).astype(np.int16)  # noqa: E731
    am = tx_cold("am")
    lsb = M.CalTxModelBatch(1, LSB, 1.0, 0.0, cal=tone(), level=0.5).process_cal(5)
    assert_same(tx_cold("usb"), am, "USB: I times +1")
    assert_same(lsb, (neg(am[0]), am[1]), "LSB: I times -1")
    assert_same(M.CalTxModelBatch(1, AM, 0.5, -0.4, cal=tone(), level=0.5).process_cal(5), am, "AM ignores the factors")


@pytest.mark.parametrize("case", list(RX_CASES))
def test_receive_model_matches_a_float64_model(case):
    """FFT_spec of the f32 restatement against the independent float64 model, bound test_display_spectrum.py's ZOOM_TOL x
    the row's maximum.  Measured between these two CPU models over the cases of RX_CASES, 3 channels each (the figure is
    printed): at most 1.1e-7 (zoom 0), 2.0e-7 (zoom 2) and 1.2e-6 (zoom 4) of the maximum -- clean tones excite the zoom
    IIR's f32 recursion far less than test_display_spectrum.py's noisy inputs, so the bound is met with room to spare."""
    mode, zoom, bins, nfr, mask = RX_CASES[case]
    I, Q = two_tones(3, nfr, zoom, bins, mode)
    amps, phases = corrections(3)
    worst = 0.0
    for c in range(3):
        got = M.CalRxModel(mode, amps[c], phases[c], zoom, bins=bins).run(I[c], Q[c], mask)[0]
        want = M.cal_rx_model_f64(I[c], Q[c], mode, amps[c], phases[c], zoom, mask)
        got = got[~np.isnan(got[:, 0])]
        assert got.shape == want.shape and len(got) == (nfr if mask is None else sum(mask))
        for g, w in zip(got, want):
            worst = max(worst, float(np.abs(g - w).max() / w.max()))
    print("%s: FFT_spec f32 restatement vs float64 model: %.2e of the maximum (bound %.0e)" % (case, worst, ZOOM_TOL[zoom]))
    assert worst <= ZOOM_TOL[zoom]


def test_log10f_fast_restatement():
    """exact at powers of two (F = 0.5: the polynomial's value there plus the exponent, all in f32), finite at 0, within the
    approximation's error of log10 across 1e-12 .. 1e6, and equal to the same steps taken one value at a time with libm's
    frexpf"""
    p2 = np.float32(2.0) ** np.arange(-40, 21, dtype=np.float32)
    h = np.float32(0.5)
    poly = ((np.float32(1.23149591368684) * h + np.float32(-4.11852516267426)) * h + np.float32(6.02197014179219)) * h + np.float32(-3.13396450166353)
    want = ((poly + np.arange(-39, 22).astype(np.float32)) * np.float32(0.3010299956639812)).astype(np.float32)
    assert np.array_equal(M.log10f_fast(p2), want)
    assert np.abs(M.log10f_fast(p2) - np.log10(p2.astype(np.float64))).max() < 3e-3
    z = M.log10f_fast(np.float32(0.0))
    assert np.isfinite(z) and z == np.float32(np.float32(-3.13396450166353) * np.float32(0.3010299956639812))
    x = np.logspace(-12, 6, 2001).astype(np.float32)
    got = M.log10f_fast(x)
    assert np.abs(got - np.log10(x.astype(np.float64))).max() < 3e-3
    assert np.array_equal(M.log10f_fast(-x), got)  # fabsf
    import math
    for v, g in zip(x[::97], got[::97]):
        f, e = math.frexp(float(v))
        y = np.float32(1.23149591368684) * np.float32(f)
        y = (y + np.float32(-4.11852516267426)) * np.float32(f)
        y = (y + np.float32(6.02197014179219)) * np.float32(f)
        y = y + np.float32(-3.13396450166353) + np.float32(e)
        assert np.float32(y * np.float32(0.3010299956639812)) == g


@pytest.mark.parametrize("case", list(RX_CASES))
def test_window_maxima_are_robust_to_the_spectrum_tolerance(case):
    """What the GPU's end-to-end comparison leans on: an FFT_spec that differs from the model's by ZOOM_TOL[zoom] x the row's
    maximum -- everywhere up, everywhere down, or with random signs -- moves no window maximum by more than 1 count, and
    at most 2 % of them at all.  The levels of two_tones() are chosen for this: both tones far above the perturbation, the
    closer together the higher the zoom, and no window maximum within twice the tolerance of a count's edge."""
    mode, zoom, bins, nfr, mask = RX_CASES[case]
    I, Q = two_tones(3, nfr, zoom, bins, mode)
    amps, phases = corrections(3)
    spec, pix, res = model_run(I, Q, mode, zoom, bins, mask, amps, phases)
    flagged = ~np.isnan(spec[:, :, 0])
    s = spec[flagged]
    base = M.measure(M.pixels(s), mode, *bins)[:, :2]
    assert np.array_equal(base, res[flagged][:, :2])
    rng = np.random.default_rng(17)
    worst, moved = 0, 0.0
    for sign in (1.0, -1.0, rng.choice([-1.0, 1.0], s.shape)):
        pert = (s.astype(np.float64) + sign * ZOOM_TOL[zoom] * s.max(axis=1, keepdims=True)).astype(np.float32)
        d, frac = count_moves(M.measure(M.pixels(pert), mode, *bins)[:, :2], base)
        worst, moved = max(worst, d), max(moved, frac)
    print("%s: window maxima under +-%.0e x max: max move %d count(s), %.1f %% moved" % (case, ZOOM_TOL[zoom], worst, 100 * moved))
    assert worst <= 1 and moved <= 0.02


def test_window_and_mode_mapping():
    pix = np.zeros(R, np.int16)
    pix[300:320] = 5
    pix[313] = 77
    pix[450:470] = -3
    pix[469] = 40
    pix[470] = 999  # just outside [450, 470)
    pix[299] = 999
    lsb, usb, am = (M.measure(pix, m, 310, 460) for m in (LSB, USB, AM))
    assert lsb.tolist() == [77.0, 40.0, float(np.float32((40.0 - 77.0) / 1.95))]
    assert usb.tolist() == [40.0, 77.0, float(np.float32((77.0 - 40.0) / 1.95))]
    assert am.tolist() == [0.0, 0.0, 0.0]
    I, Q = two_tones(1, 1, 0, (310, 460))
    for mode, ref_bin in ((LSB, 0), (USB, 1)):
        _, p, r = M.CalRxModel(mode, bins=(310, 460)).run(I[0], Q[0])
        w = [int(p[0, b - 10:b + 10].max()) for b in (310, 460)]
        assert r[0, 0] == w[ref_bin] and r[0, 1] == w[1 - ref_bin] and w[0] > w[1] + 20
    assert M.CalRxModel(AM, bins=(310, 460)).run(I[0], Q[0])[2].tolist() == [[0.0, 0.0, 0.0]]


@pytest.mark.parametrize("zoom", [0, 2])
def test_unflagged_frames_advance_nothing(zoom):
    """a stream with mask 1,0,0,1 gives on its flagged frames what the stream of frames 0 and 3 alone gives with every
    frame flagged (at zoom 2 the zoom memories and the ring must stand still), and its held frames repeat frame 0's result"""
    bins = (209, 273)
    I, Q = two_tones(1, 4, zoom, bins, USB)
    s, p, r = M.CalRxModel(USB, 1.01, -0.01, zoom, bins=bins).run(I[0], Q[0], (1, 0, 0, 1))
    pick = np.r_[0:F, 3 * F:4 * F]
    s2, p2, r2 = M.CalRxModel(USB, 1.01, -0.01, zoom, bins=bins).run(I[0][pick], Q[0][pick])
    assert np.array_equal(s[[0, 3]], s2) and np.array_equal(p[[0, 3]], p2) and np.array_equal(r[[0, 3]], r2)
    assert np.isnan(s[1]).all() and np.array_equal(p[1], p[0]) and np.array_equal(r[2], r[0])
    s3 = M.CalRxModel(USB, 1.01, -0.01, zoom, bins=bins).run(I[0], Q[0])[0]
    # the frames in between do count when they are flagged, where FFT_spec has a memory (zoom 0 draws it un-smoothed)
    assert np.array_equal(s3[3], s[3]) == (zoom == 0)
    none = M.CalRxModel(USB, 1.01, -0.01, zoom, bins=bins).run(I[0], Q[0], (0, 0, 0, 0))
    assert not none[1].any() and not none[2].any()


CLOSED_LOOP = {"lsb, phase < 0": (LSB, 1.02, -0.02), "usb, phase > 0": (USB, 0.98, 0.02)}


def grid(amp_star, phase_star):
    return (amp_star + 0.01 * np.arange(-3, 4)).astype(np.float32), (phase_star + 0.01 * np.arange(-3, 4)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def closed_loop(name, frames=2):
    """samples whose imbalance grid point (3, 3) removes exactly, and the model's sweep over the 7 x 7 grid"""
    mode, a, p = CLOSED_LOOP[name]
    I, Q = M.imbalanced_tone(frames, mode, a, p)
    return (I, Q) + M.sweep(I, Q, *grid(a, p), mode)


@pytest.mark.parametrize("name", list(CLOSED_LOOP))
def test_closed_loop_on_the_model(name):
    I, Q, g, best, res = closed_loop(name)
    print("%s: adjdB at the inverse %.1f, next best %.1f" % (name, g[best], np.sort(g.reshape(-1))[1]))
    assert best == (3, 3)
    assert g[3, 3] < np.sort(g.reshape(-1))[1] - 20.0 and g.shape == (7, 7)
    assert np.array_equal(res[:, 0], res[:, 1])  # the second frame is held


# ---- CPU: the C ABI
def test_calibration_abi_symbols_and_null_refusals(built):
    import t41_sdr_amd as T
    from t41_sdr_amd import _lib, cal, tx
    exports = set(re.findall(r"\b(t41[rt]x_[a-z0-9_]+);", re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())))
    raw = C.CDLL(T.LIB_PATH)
    for header, names, mirror in (("t41tx.h", TX_SYMBOLS, tx.TX_SYMBOLS), ("t41rx.h", RX_SYMBOLS, _lib.SYMBOLS)):
        raw_hdr = open(os.path.join(ROOT, "include", header)).read()
        hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
        for s in names:
            assert re.search(r"T41RX_API\s+int\s+%s\s*\(" % s, hdr), s
            assert s in exports and s in mirror and hasattr(raw, s), s
    assert "Not restated: the data exciter" in open(os.path.join(ROOT, "include", "t41tx.h")).read()
    rx_hdr = open(os.path.join(ROOT, "include", "t41rx.h")).read()
    for name, v in (("RX_LSB_BIN0", 310), ("RX_LSB_BIN1", 460), ("RX_USB_BIN0", 65), ("RX_USB_BIN1", 192), ("TX_LSB_BIN0", 240),
                    ("TX_LSB_BIN1", 305), ("TX_USB_BIN0", 209), ("TX_USB_BIN1", 273), ("CAPTURE_BINS", 10), ("RX_ZOOM", 0), ("TX_ZOOM", 2)):
        assert re.search(r"#define\s+T41RX_CAL_%s\s+%d\b" % (name, v), rx_hdr), name
    for m in ("set_cal_tone", "set_cal_corrections", "ProcessIQData2_tx"):
        assert callable(getattr(T.TxChain, m))
    for m in ("set_calibration", "set_cal_corrections", "ProcessIQData2_rx"):
        assert callable(getattr(T.RxChain, m))
    assert callable(T.cal_tone) and callable(cal.receive_iq_sweep) and callable(cal.transmit_iq_sweep)
    assert raw.t41rx_abi_version() == 5
    # refusals that need no device: a NULL context, each entry with its own message
    lib = tx._load()
    c, s = tone()
    out = np.zeros(2 * F + 8, np.int16)
    res = np.zeros(3, np.float32)
    fin = np.zeros(F, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cases = [
        ("t41tx_set_cal_tone", lambda: lib.t41tx_set_cal_tone(None, p(c), p(s), 0.5)),
        ("t41tx_set_cal_corrections", lambda: lib.t41tx_set_cal_corrections(None, p(res), p(res))),
        ("t41tx_process_cal_device_q15", lambda: lib.t41tx_process_cal_device_q15(None, p(out), p(out), 1, None)),
        ("t41tx_process_cal_host_q15", lambda: lib.t41tx_process_cal_host_q15(None, p(out), p(out), 1)),
        ("t41rx_set_calibration", lambda: lib.t41rx_set_calibration(None, 1, 0, 1, 0, 310, 460, 10)),
        ("t41rx_set_cal_corrections", lambda: lib.t41rx_set_cal_corrections(None, p(res), p(res))),
        ("t41rx_calibrate_device", lambda: lib.t41rx_calibrate_device(None, p(fin), p(fin), 0, None, p(res), None, None, 1, None)),
        ("t41rx_calibrate_device_q15", lambda: lib.t41rx_calibrate_device_q15(None, p(out), p(out), 0, None, p(res), None, None, 1, None)),
        ("t41rx_calibrate_host", lambda: lib.t41rx_calibrate_host(None, p(fin), p(fin), 0, None, p(res), None, None, 1)),
        ("t41rx_calibrate_host_q15", lambda: lib.t41rx_calibrate_host_q15(None, p(out), p(out), 0, None, p(res), None, None, 1)),
    ]
    for name, call in cases:
        ctx = C.c_void_p()
        assert lib.t41rx_create(C.byref(ctx), 0, 4, C.byref(T.default_params(fft_length=777))) == ERR_ARG  # another message
        assert lib.t41rx_last_error().decode() != "null argument"
        assert call() == ERR_ARG, name
        assert lib.t41rx_last_error().decode() == "null argument", name
    assert not out.any() and not res.any()


def test_cal_tone():
    from t41_sdr_amd import tx
    c, s = tx.cal_tone()
    assert c.dtype == np.float32 and s.dtype == np.float32 and c.shape == (256,) and s.shape == (256,)
    theta = np.array([np.float32(kf * 2.0 * np.pi * 3000.0 / 24000.0) for kf in range(256)]).astype(np.float64)
    assert np.array_equal(c, np.cos(theta).astype(np.float32)) and np.array_equal(s, np.sin(theta).astype(np.float32))
    assert np.array_equal(c, tone()[0]) and np.array_equal(s, tone()[1])
    # 3000 Hz at 24 kS/s: 8 samples per period, 32 whole periods per table; the float theta shows from the second period on
    assert abs(float(c[8]) - 1.0) < 1e-6 and abs(float(s[8])) < 1e-6 and abs(float(s[2]) - 1.0) < 1e-6
    exact = np.sin(np.arange(256) * 2.0 * np.pi * 3000.0 / 24000.0).astype(np.float32)
    assert not np.array_equal(s, exact) and np.abs(s - exact).max() < 2e-5


# ---- GPU helpers
def cal_chain(nch, mode=USB, amp=1.0, phase=0.0, level=0.5, per_channel=None):
    import t41_sdr_amd as T
    tx = T.TxChain(nch, T.default_tx_params(mode=mode, IQXAmpCorrectionFactor=amp, IQXPhaseCorrectionFactor=phase))
    tx.set_cal_tone(*tone(), level)
    if per_channel is not None:
        tx.set_cal_corrections(*per_channel)
    return tx


def run_cal(tx, nfr, device=True):
    if not device:
        return tx.ProcessIQData2_tx(nfr)
    import torch
    oL, oR = tx.ProcessIQData2_tx(nfr, device=True)
    torch.cuda.synchronize()
    assert oL.dtype == torch.int16 and oL.is_cuda and tuple(oL.shape) == (tx.n_channels, nfr * F)
    return oL.cpu().numpy(), oR.cpu().numpy()


def run_ssb(tx, q):
    import torch
    oL, oR = tx.ExciterIQData(torch.from_numpy(np.ascontiguousarray(q)).cuda())
    torch.cuda.synchronize()
    return oL.cpu().numpy(), oR.cpu().numpy()


def run_cw(tx, nfr):
    return tx.CW_ExciterIQData(nfr)


def rx_chain(nch, mode, zoom, bins, amps=None, phases=None, capture=10, **params):
    import t41_sdr_amd as T
    if mode == LSB:  # (the audio path's designer wants an LSB pass band below the carrier)
        params = dict(dict(FLoCut=-3000, FHiCut=-200), **params)
    rx = T.RxChain(nch, T.default_params(mode=mode, **params))
    rx.set_calibration(True, zoom, 1, 0, bins[0], bins[1], capture)
    if amps is not None:
        rx.set_cal_corrections(amps, phases)
    return rx


def run_rx(rx, I, Q, mask=None, shared=False, device=True, pixel=True, spec=True):
    """one calibration call -> numpy (result, pixel, spec)"""
    if not device:
        return rx.ProcessIQData2_rx(I, Q, mask, shared, pixel, spec)
    import torch
    out = rx.ProcessIQData2_rx(torch.from_numpy(np.array(I)).cuda(), torch.from_numpy(np.array(Q)).cuda(), mask, shared, pixel, spec)
    torch.cuda.synchronize()
    return tuple(None if o is None else o.cpu().numpy() for o in out)


def check_rx(got, ref, mode, zoom, bins, mask, what, capture=10):
    """the four comparisons of a receive case.  got = (result, pixel, spec) of the GPU, ref = (spec, pixel, result) of the
    model, rows of unflagged frames in the GPU's pixel / spec buffers still zero"""
    res, pix, spec = got
    mspec, mpix, mres = ref
    nfr = res.shape[1]
    flags = np.ones(nfr, bool) if mask is None else np.asarray(mask, bool)
    for f in range(nfr):
        if not flags[f]:
            assert not pix[:, f].any() and not spec[:, f].any(), (what, f, "an unflagged row was written")
            continue
        for c in range(res.shape[0]):
            tol = ZOOM_TOL[zoom] * mspec[c, f].max()
            assert np.abs(spec[c, f] - mspec[c, f]).max() <= tol, (what, c, f, "FFT_spec", float(np.abs(spec[c, f] - mspec[c, f]).max() / mspec[c, f].max()))
        # the mapping is integer and f32 arithmetic with nothing reordered: exact on the GPU's own FFT_spec
        assert np.array_equal(pix[:, f], M.pixels(spec[:, f])), (what, f, "pixelnew from the GPU's own FFT_spec")
    # the measurement, held frames included: exact on the GPU's own pixels (zero until the first flagged frame)
    held = np.zeros((res.shape[0], R), np.int16)
    for f in range(nfr):
        if flags[f]:
            held = pix[:, f]
        want = M.measure(held, mode, bins[0], bins[1], capture)
        assert np.array_equal(res[:, f].view(np.uint32), want.view(np.uint32)), (what, f, "refAmplitude / adjAmplitude / adjdB")
    # end to end against the model: each amplitude within 1 count, at most 2 % of them differ
    d, frac = count_moves(res[:, :, :2], mres[:, :, :2])
    print("%s: amplitudes vs the model: max |d| %d count(s), %.2f %% differ" % (what, d, 100 * frac))
    assert d <= 1 and frac <= 0.02, (what, d, frac)


# ---- GPU: the calibration exciter, bit for bit on q15
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(TX_CASES))
def test_gpu_cal_exciter_parity(built, case):
    """1 and 3 channels x 1, 2, 3 and 5 frames from power-on (from the third frame on the kernel replays the second),
    through both entries"""
    mode, amp, phase = TX_CASES[case]
    ref = tx_cold(case)
    assert np.abs(ref[0]).max() > 1500 and np.abs(ref[1]).max() > 1500
    for nch, nfr, device in ((1, 1, True), (3, 2, False), (3, 3, True), (1, 5, False), (3, 5, True)):
        got = run_cal(cal_chain(nch, mode, amp, phase), nfr, device=device)
        assert_same(got, rows(ref, nch, nfr), "%s, %d channels, %d frames, %s entry" % (case, nch, nfr, "device" if device else "host"))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [LSB, USB, AM])
def test_gpu_cal_exciter_per_channel_corrections(built, mode):
    """300 channels (more than there are CUs), every candidate different, both signs of the phase factor; NULL, NULL
    returns to the params' factors"""
    nch, nfr = 300, 3
    amps, phases = corrections(nch)
    assert len(set(zip(amps.tolist(), phases.tolist()))) == nch and (phases < 0).any() and (phases > 0).any()
    tx = cal_chain(nch, mode, 0.9, 0.05, per_channel=(amps, phases))
    got = run_cal(tx, nfr)
    ref = M.CalTxModelBatch(nch, mode, cal=tone(), level=0.5, amps=amps, phases=phases).process_cal(nfr)
    assert_same(got, ref, "per-channel candidates")
    if mode != AM:
        assert len({g.tobytes() for g in got[0]}) == nch
    tx.set_cal_corrections(None, None)
    tx.reset()
    one = M.CalTxModelBatch(1, mode, 0.9, 0.05, cal=tone(), level=0.5).process_cal(2)
    assert_same(run_cal(tx, 2, device=False), rows(one, nch), "back to the params' factors")


@pytest.mark.gpu
def test_gpu_cal_exciter_rails(built):
    """level 40: the interpolators' output is far beyond full scale, arm_float_to_q15 saturates at both rails"""
    nch, nfr = 3, 2
    got = run_cal(cal_chain(nch, LSB, 0.97, -0.02, level=40.0), nfr)
    assert_same(got, rows(M.CalTxModelBatch(1, LSB, 0.97, -0.02, cal=tone(), level=40.0).process_cal(nfr), nch), "rails")
    for o in got:
        assert (o == 32767).any() and (o == -32768).any()


@pytest.mark.gpu
def test_gpu_cal_exciter_streaming_and_shared_memories(built):
    """5 frames in one call == 2 + 3; then SSB -> calibration -> CW on the shared interpolator memories, every call
    against the model, the calibration call changing the interpolators' part of the checkpoint and nothing else"""
    from test_cw_exciter import tone as cw_tone
    nch = 3
    mode, amp, phase = TX_CASES["lsb-corr"]
    whole = run_cal(cal_chain(nch, mode, amp, phase), 5)
    assert_same(whole, rows(tx_cold("lsb-corr"), nch, 5), "5 frames in one call")
    tx = cal_chain(nch, mode, amp, phase)
    assert_same(cat([run_cal(tx, 2), run_cal(tx, 3, device=False)]), whole, "2 + 3")
    q = mic(nch, 2, seed=7)
    tx = cal_chain(nch, mode, amp, phase)
    tx.set_cw_tone(*cw_tone())
    mo = M.CalTxModelBatch(nch, mode, amp, phase, tone=cw_tone(), cal=tone(), level=0.5)
    records = lambda: tx.get_state()[32:].view(np.float32).reshape(nch, 448)  # noqa: E731
    assert_same(run_ssb(tx, q), mo.process(q), "SSB, 2 frames")
    before = records().copy()
    first = run_cal(tx, 2)
    assert_same(first, mo.process_cal(2), "calibration, 2 frames after SSB")
    assert not np.array_equal(first[0][:, :F], rows(tx_cold("lsb-corr"), nch, 1)[0])  # not a cold start
    after = records()
    assert np.array_equal(before[:, :272].view(np.uint32), after[:, :272].view(np.uint32))   # decimators, Hilbert pair
    assert np.array_equal(before[:, 336:].view(np.uint32), after[:, 336:].view(np.uint32))   # equaliser
    assert not np.array_equal(before[:, 272:336], after[:, 272:336])
    assert_same(run_cw(tx, 2), mo.process_cw(2), "CW, 2 frames after calibration")
    assert_same(run_ssb(tx, q), mo.process(q), "SSB again")


@pytest.mark.gpu
def test_gpu_cal_exciter_checkpoint_and_reset(built):
    nch = 3
    mode, amp, phase = TX_CASES["usb-corr"]
    amps, phases = corrections(nch)
    tx = cal_chain(nch, mode, amp, phase, per_channel=(amps, phases))
    mo = M.CalTxModelBatch(nch, mode, amp, phase, cal=tone(), level=0.5, amps=amps, phases=phases)  # (SSB frames: the params' factors)
    q = mic(nch, 1, seed=8)
    run_ssb(tx, q)
    mo.process(q)
    assert_same(run_cal(tx, 1), mo.process_cal(1), "first calibration call")
    ck = tx.get_state()
    assert ck.size == 32 + 4 * 448 * nch and list(ck[:32].view(np.int32)[1:4]) == [5, nch, 448]
    ref = mo.process_cal(2)
    tx2 = cal_chain(nch, mode, amp, phase, per_channel=(amps, phases))
    tx2.set_state(ck)
    assert_same(run_cal(tx2, 2, device=False), ref, "checkpoint between two calibration calls, restored into a fresh context")
    assert_same(run_cal(tx, 2), ref, "the original context")
    tx.reset()
    assert not tx.get_state()[32:].any()
    cold = M.CalTxModelBatch(nch, mode, cal=tone(), level=0.5, amps=amps, phases=phases).process_cal(2)
    assert_same(run_cal(tx, 2), cold, "after reset: a cold start, tone and candidates kept")


@pytest.mark.gpu
def test_gpu_cal_exciter_refusals(built):
    import torch
    import t41_sdr_amd as T
    nch = 3
    tx = T.TxChain(nch, T.default_tx_params(mode=USB))
    lib = tx._lib
    for device in (True, False):
        with pytest.raises(T.T41RxError, match="no tone table loaded") as e:
            tx.ProcessIQData2_tx(1, device=device)
        assert e.value.status == ERR_ARG
    bad = tone()[0].copy()
    bad[7] = np.nan
    for args in ((bad, tone()[1], 0.5), (tone()[0], bad, 0.5), (tone()[0], tone()[1], float("inf"))):
        with pytest.raises(T.T41RxError, match="non-finite"):
            tx.set_cal_tone(*args)
    with pytest.raises(T.T41RxError, match="no tone table loaded"):
        tx.ProcessIQData2_tx(1)
    tx.set_cal_tone(*tone(), 0.5)
    amps, phases = corrections(nch)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.t41tx_set_cal_corrections(tx._ctx, p(amps), None) == ERR_ARG
    assert lib.t41tx_set_cal_corrections(tx._ctx, None, p(phases)) == ERR_ARG
    nan = amps.copy()
    nan[1] = np.nan
    with pytest.raises(T.T41RxError, match="non-finite"):
        tx.set_cal_corrections(nan, phases)
    oL = torch.zeros((nch, 2 * F + 8), dtype=torch.int16, device="cuda")
    oR = torch.zeros_like(oL)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    refused = [
        ("n_frames must be > 0", lambda: lib.t41tx_process_cal_device_q15(tx._ctx, oL.data_ptr(), oR.data_ptr(), 0, stream)),
        ("device pointers must be 16-byte aligned", lambda: lib.t41tx_process_cal_device_q15(tx._ctx, oL.data_ptr() + 2, oR.data_ptr(), 1, stream)),
        ("device pointers must be 16-byte aligned", lambda: lib.t41tx_process_cal_device_q15(tx._ctx, oL.data_ptr(), oR.data_ptr() + 8, 1, stream)),
        ("null argument", lambda: lib.t41tx_process_cal_device_q15(tx._ctx, None, oR.data_ptr(), 1, stream)),
    ]
    for text, call in refused:
        assert call() == ERR_ARG, text
        assert lib.t41rx_last_error().decode() == text
    torch.cuda.synchronize()
    assert not oL.any() and not oR.any() and not tx.get_state()[32:].any()  # nothing ran, the refused candidates were not kept
    assert_same(run_cal(tx, 2), rows(tx_cold("usb"), nch, 2), "the context is usable, on the params' factors")


# ---- GPU: the receive half
@pytest.mark.gpu
@pytest.mark.parametrize("case", list(RX_CASES))
def test_gpu_receive_half(built, case):
    """3 channels with a candidate each on their own samples: f32 through the device entry, q15 through the host entry
    (I != Q, so a missing queue swap mirrors the spectrum), and every channel on channel 0's samples (shared_input)"""
    mode, zoom, bins, nfr, mask = RX_CASES[case]
    nch = 3
    I, Q = two_tones(nch, nfr, zoom, bins, mode)
    amps, phases = corrections(nch)
    ref = model_run(I, Q, mode, zoom, bins, mask, amps, phases)
    got = run_rx(rx_chain(nch, mode, zoom, bins, amps, phases), I, Q, mask)
    check_rx(got, ref, mode, zoom, bins, mask, case + ", f32, device entry")
    qL, qR = to_queues(I, Q)
    ref = model_run(qL, qR, mode, zoom, bins, mask, amps, phases, q15=True)
    got = run_rx(rx_chain(nch, mode, zoom, bins, amps, phases), qL, qR, mask, device=False)
    check_rx(got, ref, mode, zoom, bins, mask, case + ", q15, host entry")
    ref = model_run(I, Q, mode, zoom, bins, mask, amps, phases, shared=True, nch=nch)
    got = run_rx(rx_chain(nch, mode, zoom, bins, amps, phases), I[:1], Q[:1], mask, shared=True)
    check_rx(got, ref, mode, zoom, bins, mask, case + ", shared input")
    assert len({r.tobytes() for r in got[2][:, 0]}) == nch  # three candidates, three spectra


@pytest.mark.gpu
def test_gpu_receive_half_one_and_many_channels(built):
    """1 channel x 1 frame on the params' factors (q15, device entry), and 300 candidates -- more than there are CUs -- on
    one recording"""
    mode, zoom, bins = USB, 2, (209, 273)
    I, Q = two_tones(1, 1, zoom, bins, mode)
    qL, qR = to_queues(I, Q)
    import t41_sdr_amd as T
    rx = T.RxChain(1, T.default_params(mode=mode, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=-0.01, rfGainAllBands=6))
    rx.set_calibration(True, zoom, 1, 0, bins[0], bins[1], 10)
    ref = model_run(qL, qR, mode, zoom, bins, None, [1.02], [-0.01], q15=True, rf_gain_db=6)
    check_rx(run_rx(rx, qL, qR), ref, mode, zoom, bins, None, "1 channel, 1 frame, q15, the params' factors")
    nch, nfr, mask = 300, 4, (1, 0, 0, 1)
    I, Q = two_tones(1, nfr, zoom, bins, mode)
    amps, phases = corrections(nch)
    ref = model_run(I, Q, mode, zoom, bins, mask, amps, phases, shared=True, nch=nch)
    got = run_rx(rx_chain(nch, mode, zoom, bins, amps, phases), I, Q, mask, shared=True)
    check_rx(got, ref, mode, zoom, bins, mask, "300 channels, shared input")


@pytest.mark.gpu
def test_gpu_receive_half_other_modes_and_no_flag(built):
    """AM: the spectrum is drawn without a correction, the measurement stays 0, 0, 0.0; mask none: nothing is read or
    written but all-zero results"""
    zoom, bins, nch, nfr = 0, (310, 460), 3, 4
    I, Q = two_tones(nch, nfr, zoom, bins, AM)
    amps, phases = corrections(nch)
    ref = model_run(I, Q, AM, zoom, bins, None, amps, phases)
    got = run_rx(rx_chain(nch, AM, zoom, bins, amps, phases), I, Q)
    check_rx(got, ref, AM, zoom, bins, None, "AM")
    assert not got[0].any() and got[1].any()
    plain = model_run(I, Q, AM, zoom, bins)
    assert np.array_equal(ref[0], plain[0])  # the model draws AM without the candidates
    for z in (0, 2):
        res, pix, spec = run_rx(rx_chain(nch, LSB, z, bins, amps, phases), I, Q, (0, 0, 0, 0))
        assert not res.any() and not pix.any() and not spec.any() and res.shape == (nch, nfr, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("zoom", [0, 2])
def test_gpu_receive_half_streaming_and_restart(built, zoom):
    """split calls equal one call (the calibration memory's round trip, held pixels across calls included);
    t41rx_set_calibration() again and t41rx_reset() restart from power-on; buffers handed in keep their unflagged rows"""
    mode, bins, nch, nfr, mask = USB, (209, 273), 3, 4, (1, 0, 1, 1)
    I, Q = two_tones(nch, nfr, zoom, bins, mode)
    amps, phases = corrections(nch)
    rx = rx_chain(nch, mode, zoom, bins, amps, phases)
    whole = run_rx(rx, I, Q, mask)
    check_rx(whole, model_run(I, Q, mode, zoom, bins, mask, amps, phases), mode, zoom, bins, mask, "one call")
    for restart in ("set_calibration", "reset"):
        if restart == "reset":
            rx.reset()
        else:
            rx.set_calibration(True, zoom, 1, 0, bins[0], bins[1], 10)
        parts = [run_rx(rx, I[:, a * F:b * F], Q[:, a * F:b * F], mask[a:b], device=(a == 0)) for a, b in ((0, 2), (2, 4))]
        for k in range(3):
            assert np.array_equal(np.concatenate([p[k] for p in parts], axis=1), whole[k]), (restart, k)
    mine = np.full((nch, nfr, R), 7, np.int16)
    rx.set_calibration(True, zoom, 1, 0, bins[0], bins[1], 10)
    res, pix, _ = rx.ProcessIQData2_rx(I, Q, mask, pixel=mine, spec=False)
    assert pix is mine and (mine[:, 1] == 7).all() and np.array_equal(mine[:, [0, 2, 3]], whole[1][:, [0, 2, 3]]) and np.array_equal(res, whole[0])


@pytest.mark.gpu
def test_gpu_calibration_leaves_the_audio_path_alone(built):
    """process_host 2 frames, calibrate, process_host 2 frames == 4 frames uninterrupted, bit for bit; the checkpoint's
    size is unchanged by calibration being configured, and its bytes by a calibration call"""
    import siggen
    import t41_sdr_amd as T
    nch, nfr = 3, 4
    nco = siggen.nco_grid(nch, seed=5)
    I, Q = siggen.make_iq(nch, nfr * F, nco, seed=9)
    a = T.RxChain(nch, T.default_params(AGCMode=1), NCOFreq=nco)
    whole = a.ProcessIQData(I, Q)
    b = T.RxChain(nch, T.default_params(AGCMode=1), NCOFreq=nco)
    size = b._lib.t41rx_state_bytes(b._ctx)
    first = b.ProcessIQData(I[:, :2 * F], Q[:, :2 * F])
    b.set_calibration(True, 2, 1, 0, 209, 273, 10)
    assert b._lib.t41rx_state_bytes(b._ctx) == size
    ck = b.get_state()
    res, _, _ = b.ProcessIQData2_rx(I[:, :2 * F], Q[:, :2 * F])
    assert res.any() and np.array_equal(b.get_state(), ck) and b._lib.t41rx_state_bytes(b._ctx) == size
    second = b.ProcessIQData(I[:, 2 * F:], Q[:, 2 * F:])
    assert np.array_equal(np.concatenate([first, second], axis=1).view(np.uint32), whole.view(np.uint32))
    assert list(ck[:32].view(np.int32)[5:7]) == list(a.get_state()[:32].view(np.int32)[5:7])  # section mask, zoom word


@pytest.mark.gpu
def test_gpu_calibration_refusals(built):
    import t41_sdr_amd as T
    I, Q = two_tones(3, 1, 0, (310, 460))
    rx = T.RxChain(3, T.default_params(mode=LSB, FLoCut=-3000, FHiCut=-200))
    with pytest.raises(T.T41RxError, match="not switched on") as e:
        rx.ProcessIQData2_rx(I, Q)
    assert e.value.status == ERR_ARG
    for bad in (dict(spectrumZoom=5), dict(spectrumZoom=-1), dict(currentScale=5), dict(currentScale=-1), dict(capture_bins=0),
                dict(bin0=11), dict(bin1=503), dict(bin0=1, capture_bins=1), dict(bin1=512, capture_bins=1)):
        with pytest.raises(T.T41RxError) as e:
            rx.set_calibration(True, **bad)
        assert e.value.status == ERR_ARG, bad
    with pytest.raises(T.T41RxError, match="not switched on"):
        rx.ProcessIQData2_rx(I, Q)  # a refused configuration switched nothing on
    rx.set_calibration(True, bin0=12, bin1=502)  # the windows touch both edges: [2, 22) and [492, 512)
    lib, p = rx._lib, (lambda a: a.ctypes.data_as(C.c_void_p))
    res = np.zeros((3, 1, 3), np.float32)
    for text, call in (("n_frames must be > 0", lambda: lib.t41rx_calibrate_host(rx._ctx, p(I), p(Q), 0, None, p(res), None, None, 0)),
                       ("null argument", lambda: lib.t41rx_calibrate_host(rx._ctx, None, p(Q), 0, None, p(res), None, None, 1)),
                       ("null argument", lambda: lib.t41rx_calibrate_host(rx._ctx, p(I), p(Q), 0, None, None, None, None, 1))):
        assert call() == ERR_ARG and lib.t41rx_last_error().decode() == text
    amps, phases = corrections(3)
    assert lib.t41rx_set_cal_corrections(rx._ctx, p(amps), None) == ERR_ARG
    nan = phases.copy()
    nan[2] = np.inf
    with pytest.raises(T.T41RxError, match="non-finite"):
        rx.set_cal_corrections(amps, nan)
    rx.set_calibration(False)
    with pytest.raises(T.T41RxError, match="not switched on"):
        rx.ProcessIQData2_rx(I, Q)
    long = T.RxChain(2, T.default_params(fft_length=1024))
    with pytest.raises(T.T41RxError, match="fft_length 512") as e:
        long.set_calibration(True)
    assert e.value.status == ERR_UNSUPPORTED
    tm = T.RxChain(2, T.default_params())
    tm.set_buffer_layout("time")
    with pytest.raises(T.T41RxError, match="channel-major") as e:
        tm.set_calibration(True)
    assert e.value.status == ERR_UNSUPPORTED


# ---- GPU: the sweep
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CLOSED_LOOP))
def test_gpu_receive_iq_sweep(built, name):
    """receive_iq_sweep over the 7 x 7 grid of the CPU closed-loop test: the model's best candidate, and its adjdB grid
    within the end-to-end condition (amplitudes within 1 count, at most 2 % differ)"""
    from t41_sdr_amd import cal
    mode, a, p = CLOSED_LOOP[name]
    I, Q, g, best, res = closed_loop(name)
    amps, phases = grid(a, p)
    got = cal.receive_iq_sweep(I, Q, amps, phases, mode, frames=2)
    assert got.best == best == (3, 3) and got.amp == float(amps[3]) and got.phase == float(phases[3])
    assert got.adjdB.shape == (7, 7) and got.result.shape == (49, 2, 3)
    d, frac = count_moves(got.result[:, :, :2], res[:, :, :2])
    print("%s: sweep amplitudes vs the model: max |d| %d, %.2f %% differ" % (name, d, 100 * frac))
    assert d <= 1 and frac <= 0.02
    assert np.abs(got.adjdB - g).max() <= np.float32(2.0 / 1.95) + 1e-6


@pytest.mark.gpu
def test_gpu_transmit_iq_sweep(built):
    """transmit_iq_sweep through an ideal loop-back with an imbalance that is the exact inverse of grid point (2, 2) of the
    TX correction (USB: I x +IQXAmp, then I += Q x phase; the interpolators are the same linear filters on I and Q, so the
    inverse behind them still cancels): the sweep finds that point, and its amplitudes are those of the CPU models run
    through the same loop-back.  The loop-back also moves the 3 kHz tone to where the firmware's transmit calibration
    looks for it at spectrumZoom 2: the wanted sideband at bin 273, its image at 209, 32 bins either side of 241 (a
    receiver whose LO sits above the signal: the conjugate, then the offset)."""
    from t41_sdr_amd import cal
    a_star, p_star = 1.03, 0.02
    amps = (a_star + 0.01 * np.arange(-2, 3)).astype(np.float32)
    phases = (p_star + 0.01 * np.arange(-2, 3)).astype(np.float32)
    seen = {}

    def loopback(oL, oR):
        seen["shape"] = oL.shape
        I, Q = oL.astype(np.float64) / 32768.0, oR.astype(np.float64) / 32768.0
        I = (I - float(phases[2]) * Q) / float(amps[2])            # the analog path's imbalance
        n = np.arange(I.shape[1])
        # the receiver mirrors once more (I x -IQAmp) and FreqShift1() adds Fs/4: put DC at bin 241 of the 93.75 Hz grid
        z = (I - 1j * Q) * np.exp(2j * np.pi * (48000.0 + 15 * 93.75) / 192000.0 * n)
        rng = np.random.default_rng(4)
        z = z + 1e-5 * (rng.standard_normal(z.shape) + 1j * rng.standard_normal(z.shape))
        return z.real.astype(np.float32), z.imag.astype(np.float32)

    got = cal.transmit_iq_sweep(loopback, amps, phases, USB, level=0.5, frames=2)
    assert seen["shape"] == (25, 2 * F) and got.result.shape == (25, 2, 3)
    print("transmit sweep: adjdB at the inverse %.1f, next best %.1f" % (got.adjdB[got.best], np.sort(got.adjdB.reshape(-1))[1]))
    assert got.best == (2, 2) and got.amp == float(amps[2]) and got.phase == float(phases[2])
    assert got.adjdB[2, 2] < np.sort(got.adjdB.reshape(-1))[1] - 10.0
    assert (got.result[:, :, 0] > got.result[:, :, 1]).all()      # the wanted sideband is the stronger one everywhere
    ga, gp = cal.candidate_grid(amps, phases)
    I, Q = loopback(*M.CalTxModelBatch(25, USB, cal=tone(), level=0.5, amps=ga, phases=gp).process_cal(2))
    ref = np.array([M.CalRxModel(USB, 1.0, 0.0, 2, bins=(209, 273)).run(I[c], Q[c], (1, 0))[2] for c in range(25)])
    d, frac = count_moves(got.result[:, :, :2], ref[:, :, :2])
    print("transmit sweep amplitudes vs the models: max |d| %d, %.2f %% differ" % (d, 100 * frac))
    assert d <= 1 and frac <= 0.02
