"""Receive equalizer (receiveEQFlag; DoReceiveEQ(), Filter.cpp:117-165, call site Process.cpp:828-832).

The band table is the firmware's EQ_Band1Coeffs .. EQ_Band14Coeffs (FIR.cpp:279-370): 14 bands x 4 biquad sections x
{b0, b1, b2, a1, a2}, a's negated for CMSIS.  tests/golden/eq/rx_eq_bands.npz holds its literals as float64 (coeffs_f64)
and their float32 rounding (coeffs_f32, what the firmware compiles), extracted once from that file; the library has no
copy of its own and takes the table from the caller (t41rx_set_receive_eq_bands).  (It sits in a subdirectory: the
parity tests take every tests/golden/*.npz for a recorded path case.)

CPU: the fixture, the f32 restatement (tests/eq_model.py) against the float64 model, why the kernel must keep the
restatement's operations (a contracted recurrence drifts past the GPU bar in the narrow low bands), the levels, the
new entry points.  GPU (-m gpu): the HIP path with the equalizer on against the HIP path's own demodulated audio
through the restatement, the oracle's NR stage, the blanker model and the oracle's interpolators; a physical check
against the float64 model alone; streaming, checkpoints, formats, refusals, a large batch.
"""
import numpy as np
import pytest

import eq_model as M
import oracle_lib as O
import siggen
from rx_harness import assert_entry_points, calls
from stage_reference import interp, nb_stage, nr_stage

L, D = 2048, 256
RAMP = [0, 15, 30, 0, 61, 77, 92, 108, 0, 138, 154, 169, 185, 200]  # non-default levels, some zero


def audio(nblocks, seed, tones=((700.0, 0.2), (2100.0, 0.1)), noise=0.05):
    rng = np.random.default_rng(seed)
    n = np.arange(nblocks * D)
    x = noise * rng.standard_normal(n.size)
    for f, a in tones:
        x = x + a * np.sin(2 * np.pi * f / 24000.0 * n + f)
    return x.astype(np.float32)


def steady_gain(y, x, skip):
    return np.sqrt(np.mean(np.asarray(y[skip:], np.float64) ** 2) / np.mean(np.asarray(x[skip:], np.float64) ** 2))


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_firmware_table():
    c64, c32 = M.bands("f64"), M.bands("f32")
    assert c64.shape == (14, 4, 5) and c32.dtype == np.float32 and np.array_equal(c32, c64.astype(np.float32))
    assert not c64[:, :, 1].any()  # b1 = 0
    assert np.array_equal(c64[:, :, 2], -c64[:, :, 0])  # b2 = -b0: band-pass sections
    poles = np.array([np.abs(np.roots([1.0, -c64[b, s, 3], -c64[b, s, 4]])).max() for b in range(14) for s in range(4)])
    assert poles.max() < 1.0 and poles.max() > 0.98, poles.max()
    m = M.F64()
    f = np.linspace(50.0, 6000.0, 60000)
    for b in range(14):
        h = m.response(f, b)
        fpk = f[h.argmax()]
        assert abs(fpk / M.CENTRES[b] - 1.0) < 0.03, (b + 1, fpk, M.CENTRES[b])
        assert abs(h.max() - 1.0) < 0.02, (b + 1, h.max())  # unity gain at the centre


def test_restatement_matches_the_f64_model():
    """a long stream (500 blocks) of tones and noise through the f32 restatement and the float64 model: the stated bound;
    the numpy loop of the same operations is the oracle's biquad bit for bit"""
    x = audio(500, seed=1)
    r = M.Restatement().stream(x, RAMP)
    e = M.block_rel(r, M.F64().stream(x, RAMP))
    print("restatement vs float64 model, 500 blocks, ramp levels: max block-relative %.2e" % e.max())
    assert e.max() < 2e-6
    assert np.array_equal(M.bank_numpy(x[:40 * D], RAMP), r[:40 * D])


def test_contraction_drifts_past_the_gpu_bar():
    """why the kernel keeps every rounding: the two lowest bands (poles at |z| ~ 0.99) over 500 blocks of noise.  The
    contracted recurrence (each a*b + c rounded once) leaves the restatement by more than the GPU tests' 1e-5; the
    restatement itself sits ~2e-5 from the float64 model there.  The reordered 14-term sum moves ~3e-7 -- under the
    bar, but not bit-identical."""
    x = (0.1 * np.random.default_rng(2).standard_normal(500 * D)).astype(np.float32)
    low = [100, 100] + [0] * 12
    r = M.Restatement().stream(x, low)
    f = M.F64().stream(x, low)
    fm = M.bank_numpy(x, low, fma=True)
    d_fma, d_res = M.block_rel(fm, r).max(), M.block_rel(r, f).max()
    print("low bands: contracted vs restatement %.2e, restatement vs float64 %.2e" % (d_fma, d_res))
    assert d_fma > 1e-5
    x = audio(100, seed=3)
    ro = M.Restatement().stream(x, [100] * 14, order="reversed")
    d_ord = M.block_rel(ro, M.Restatement().stream(x, [100] * 14)).max()
    print("reordered sum vs restatement %.2e" % d_ord)
    assert d_ord > 0


def test_level_scales():
    lv = [100, 0, 1, 3, 7, 33, 67, 99, 101, 199, -50, 16777217, 2 ** 31 - 1, -(2 ** 31)]
    s = M.level_scales(lv)
    for v, got in zip(lv, s):
        want = np.float32(float(np.float32(v)) / 100.0)  # (float)int, / 100.0 in double, stored as float
        assert got == want and got.dtype == np.float32
    assert s[0] == np.float32(1.0) and s[11] == np.float32(167772.16)  # 16777217 -> 16777216.0f first
    sg = M.signed_scales([100] * 14)
    assert (sg[0::2] == -1.0).all() and (sg[1::2] == 1.0).all()


def test_sign_alternation_passes_a_crossover_tone():
    """all levels 100: a tone between bands 8 and 9 (1122 Hz) passes (gain ~1.5); without the alternating signs the two
    bands would cancel there (gain ~0.4)"""
    n = np.arange(80 * D)
    x = (0.3 * np.sin(2 * np.pi * np.sqrt(1000.0 * 1259.0) / 24000.0 * n)).astype(np.float32)
    y = M.Restatement().stream(x, [100] * 14)
    g = steady_gain(y, x, 40 * D)
    import scipy.signal as sg
    m = M.F64()
    h_unsigned = abs(sum(sg.sosfreqz(m.sos[b], worN=[np.sqrt(1000.0 * 1259.0)], fs=24000.0)[1][0] for b in range(14)))
    print("crossover gain: signed %.3f, unsigned (float64) %.3f" % (g, h_unsigned))
    assert g > 1.2 and h_unsigned < 0.6


def test_zero_levels_give_silence_and_the_state_still_advances():
    x = audio(20, seed=4)
    z, h = M.Restatement(), M.Restatement()
    out = z.stream(x, [0] * 14)
    ref = h.stream(x, [100] * 14)
    assert not out.any() and ref.any()
    assert np.array_equal(z.st, h.st) and z.st.any()


def test_entry_points_declared_and_exported(built):
    assert_entry_points(("t41rx_set_receive_eq_bands", "t41rx_set_receive_eq", "t41rx_get_receive_eq"))


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def stage24(pre, kw, levels, model="f32", on=None, nb=False, lv_per_block=None):
    """the HIP path's pre-stage audio through the equalizer model on the blocks where on[b] (default: all), then the
    oracle's NR stage (if on) and the blanker model (if nb), as in Process.cpp:828-876"""
    p = O.default_params(**kw)
    out = np.empty(pre.shape, np.float32)
    for ch in range(pre.shape[0]):
        eq = M.Restatement() if model == "f32" else M.F64()
        a = pre[ch].copy()
        for b in range(a.size // D):
            if on is None or on[b]:
                lv = levels if lv_per_block is None else lv_per_block[b]
                a[b * D:(b + 1) * D] = eq.block(pre[ch, b * D:(b + 1) * D], lv)
        if p.nrOptionSelect or p.ANR_notchOn:
            nr_stage(a, p)
        if nb:
            nb_stage(a)
        out[ch] = a
    return out


def expect(pre, kw, levels, **k):
    return interp(stage24(pre, kw, levels, **k), kw)


def make_rx(nch, kw, nco, levels=RAMP, on=1, nb=0):
    import t41_sdr_amd as T
    rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
    rx.set_receive_eq_bands(M.bands())
    rx.set_receive_eq(on, levels)
    if nb:
        rx.set_noise_blanker(1)
    return rx


def run_hip(kw, nch, nfr, seed, levels=RAMP, q15=False, layout="channel", splits=None, on=1, nb=0, iq=None):
    nco = siggen.nco_grid(nch, seed=seed)
    I, Q = siggen.make_iq(nch, nfr * L, nco, mode=kw.get("mode", 0), seed=seed, sigma=0.05) if iq is None else iq
    rx = make_rx(nch, kw, nco, levels, on, nb)
    if layout == "time":
        rx.set_buffer_layout("time")
    got, tap, _ = calls(rx, I, Q, splits or [0, nfr], layout=layout, q15_scale=1 / 4 if q15 else None, tap_floats=D)
    return got, tap, rx


CASES = {  # name: (params, NB behind it, tolerance)
    "usb": (dict(mode=0), 0, 1e-5), "lsb": (dict(mode=1, FLoCut=-3000, FHiCut=-200), 0, 1e-5), "am": (dict(mode=2), 0, 1e-5),
    "sam": (dict(mode=8), 0, 1e-5), "nfm": (dict(mode=3), 0, 1e-5), "nfm-atan": (dict(mode=3, nfm_demod=1), 0, 1e-5),
    "usb-agc": (dict(mode=0, AGCMode=1), 0, 1e-5), "sam-agc": (dict(mode=8, AGCMode=2), 0, 1e-5),
    # (Kim: its own f32 conditioning, 2e-5 as in the blanker's tests; spectral: test_noise_reduction.py's 5e-5)
    "kim": (dict(mode=0, nrOptionSelect=1), 0, 2e-5), "spectral": (dict(mode=0, nrOptionSelect=2), 0, 5e-5),
    "notch": (dict(mode=0, ANR_notchOn=1), 0, 1e-5), "nb": (dict(mode=0), 1, 1e-5),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_whole_path_with_eq(built, name):
    """the whole path with the equalizer on = the HIP path's own demodulated audio through the f32 restatement (then the
    oracle's NR stage / the blanker model) and the oracle's interpolators; and no farther from the float64 equalizer
    model than the restatement is"""
    kw, nb, tol = CASES[name]
    got, pre, _ = run_hip(kw, 12, 16, seed=21, nb=nb)
    assert np.isfinite(got).all() and np.abs(pre).max() > 0
    want = expect(pre, kw, RAMP, nb=nb)
    e = siggen.block_rel_err(got, want, L)
    want64 = expect(pre, kw, RAMP, model="f64", nb=nb)
    d_hip, d_res = siggen.block_rel_err(got, want64, L), siggen.block_rel_err(want, want64, L)
    off, _, _ = run_hip(kw, 12, 16, seed=21, nb=nb, on=0)
    moved = siggen.block_rel_err(got, off, L)
    print(name, "max block-relative %.2e; vs the f64 model: HIP %.2e, restatement %.2e; EQ on vs off %.2e"
          % (e.max(), d_hip.max(), d_res.max(), moved.max()))
    assert moved.max() > 0.1  # the stage ran
    assert e.max() <= tol, (e.max(), np.unravel_index(e.argmax(), e.shape))
    assert d_hip.max() <= d_res.max() + (tol if name in ("kim", "spectral") else 2e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [3, 6, 9, 12])
def test_gpu_band_gain_at_its_centre(built, k):
    """a tone at band k's centre frequency, band k at 100 and every other band at 0: the output amplitude is |H_k(f)| x
    the amplitude with the equalizer off, per the float64 model alone, within 1 %"""
    nch, nfr = 2, 24
    nco = siggen.nco_grid(nch, seed=40 + k)
    f = M.CENTRES[k - 1]
    n = np.arange(nfr * L)
    x = np.stack([0.3 * np.exp(2j * np.pi * siggen.passband_tone_hz(0, nco[c], f) / 192000.0 * n) for c in range(nch)])
    iq = (x.real.astype(np.float32), x.imag.astype(np.float32))
    lv = [0] * 14
    lv[k - 1] = 100
    on, _, _ = run_hip(dict(mode=0), nch, nfr, seed=40 + k, levels=lv, iq=iq)
    off, _, _ = run_hip(dict(mode=0), nch, nfr, seed=40 + k, levels=lv, iq=iq, on=0)
    h = float(M.F64().response(f, k - 1)[0])
    for c in range(nch):
        g = steady_gain(on[c], off[c], 12 * L)
        print("band %d @ %.1f Hz, channel %d: gain %.4f, |H| %.4f" % (k, f, c, g, h))
        assert abs(g / h - 1.0) < 0.01, (g, h)


@pytest.mark.gpu
def test_gpu_splits_checkpoint_reset_levels_and_params(built):
    import torch
    import t41_sdr_amd as T
    kw = dict(mode=0)
    nch, nfr, cut = 7, 16, 4
    whole, pre, _ = run_hip(kw, nch, nfr, seed=23)
    got, _, _ = run_hip(kw, nch, nfr, seed=23, splits=[0, 1, 4, 16])
    assert np.array_equal(got, whole)
    nco = siggen.nco_grid(nch, seed=23)
    I, Q = siggen.make_iq(nch, nfr * L, nco, mode=0, seed=23, sigma=0.05)
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    part = lambda a, b: (dI[:, a * L:b * L].contiguous(), dQ[:, a * L:b * L].contiguous())  # noqa: E731
    rx = make_rx(nch, kw, nco)
    fresh = rx.get_state()
    a = rx.ProcessIQData(*part(0, cut)).cpu().numpy()
    ck = rx.get_state()
    assert ck.size == fresh.size + 4 * 112 * nch and ck[:32].view(np.int32)[5] & 8
    rx.ProcessIQData(*part(0, 3))  # disturb
    rx.set_state(ck)
    b = rx.ProcessIQData(*part(cut, nfr)).cpu().numpy()
    assert np.array_equal(np.concatenate([a, b], axis=1), whole)
    ry = make_rx(nch, kw, nco)
    ry.set_state(ck)  # a fresh context: the section allocates and restores the memories
    assert np.array_equal(ry.ProcessIQData(*part(cut, nfr)).cpu().numpy(), b)
    rx.set_state(fresh)  # no section: the memories restart at zero (= the stream from power-on)
    assert np.array_equal(rx.ProcessIQData(*part(0, nfr)).cpu().numpy(), whole)
    rx.reset()
    assert np.array_equal(rx.ProcessIQData(*part(0, nfr)).cpu().numpy(), whole)
    # set_params / set_coeffs keep the switch, the levels and the table (and the memories)
    rx.reset()
    o1 = rx.ProcessIQData(*part(0, cut)).cpu().numpy()
    rx.CalcFilters(audioVolume=rx.params.audioVolume)
    rx.set_coeffs(rx.coeffs())
    on, lv = rx.receive_eq
    assert on == 1 and list(lv) == RAMP
    o2 = rx.ProcessIQData(*part(cut, nfr)).cpu().numpy()
    assert np.array_equal(np.concatenate([o1, o2], axis=1), whole)
    # levels changed between calls take effect at the next call
    lv2 = [200 - v for v in RAMP]
    rz = make_rx(nch, kw, nco)
    parts = []
    for (s, e), levels in zip(((0, cut), (cut, nfr)), (RAMP, lv2)):
        rz.set_receive_eq(1, levels)
        parts.append(calls(rz, I, Q, [s, e], tap_floats=D))
    got, tap = (np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1))
    per = [RAMP if b < cut else lv2 for b in range(nfr)]
    e = siggen.block_rel_err(got, interp(stage24(tap, kw, None, lv_per_block=per), kw), L)
    assert e.max() <= 1e-5, e.max()
    assert not np.array_equal(got[:, cut * L:], whole[:, cut * L:])


@pytest.mark.gpu
def test_gpu_off_on_keeps_the_stale_state(built):
    """switched off and on again, the equalizer resumes from the memories it had when it was switched off (they only
    change while it runs): the whole stream against the restatement that skips the off blocks; memories zeroed at the
    switch would not match"""
    kw = dict(mode=0)
    nch, nfr = 6, 10
    nco = siggen.nco_grid(nch, seed=24)
    I, Q = siggen.make_iq(nch, nfr * L, nco, mode=0, seed=24, sigma=0.05)
    rz = make_rx(nch, kw, nco)
    parts = []
    for (s, e), on in zip(((0, 3), (3, 6), (6, nfr)), (1, 0, 1)):
        rz.set_receive_eq(on)
        assert rz.receive_eq[0] == on and list(rz.receive_eq[1]) == RAMP
        parts.append(calls(rz, I, Q, [s, e], tap_floats=D))
    got, pre = (np.concatenate([p[k] for p in parts], axis=1) for k in (0, 1))
    on = [b < 3 or b >= 6 for b in range(nfr)]  # (one 256-sample block per frame)
    e = siggen.block_rel_err(got, interp(stage24(pre, kw, RAMP, on=on), kw), L)
    assert e.max() <= 1e-5, e.max()
    zero = [b >= 6 for b in range(nfr)]  # the same stream with the memories zeroed at the switch
    a24 = stage24(pre, kw, RAMP, on=on)
    a24[:, 6 * D:] = stage24(pre, kw, RAMP, on=zero)[:, 6 * D:]
    ez = siggen.block_rel_err(got, interp(a24, kw), L)
    assert ez[:, 6].max() > 1e-3, ez[:, 6]


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["q15", "time"])
def test_gpu_eq_formats(built, how):
    kw = dict(mode=8)
    whole, pre, _ = run_hip(kw, 5, 6, seed=22)
    if how == "time":
        got, _, _ = run_hip(kw, 5, 6, seed=22, layout="time")
        assert np.array_equal(got, whole)
    else:
        got, pre, _ = run_hip(kw, 5, 6, seed=22, q15=True)
        want = expect(pre, kw, RAMP)
        ref = np.clip(np.trunc(want.astype(np.float64) * 32768.0), -32768, 32767)
        assert np.abs(got.astype(np.float64) - ref).max() <= 1 and np.abs(ref).max() > 100


@pytest.mark.gpu
def test_gpu_eq_refusals(built):
    import t41_sdr_amd as T
    import t41_sdr_amd._lib as lib
    rx = T.RxChain(3, T.default_params())
    with pytest.raises(T.T41RxError) as ei:
        rx.set_receive_eq(1)  # no band table yet
    assert ei.value.status == lib.ERR_ARG
    bad = M.bands().copy()
    bad[5, 2, 3] = np.nan
    with pytest.raises(T.T41RxError) as ei:
        rx.set_receive_eq_bands(bad)
    assert ei.value.status == lib.ERR_ARG
    L_ = lib.load()
    assert L_.t41rx_set_receive_eq_bands(rx._ctx, None) == lib.ERR_ARG
    with pytest.raises(T.T41RxError):
        rx.set_receive_eq(1)  # (the refused tables loaded nothing)
    rx.set_receive_eq_bands(M.bands().reshape(14, 20))
    for v in (2, -1):
        with pytest.raises(T.T41RxError) as ei:
            rx.set_receive_eq(v)
        assert ei.value.status == lib.ERR_ARG
    assert rx.receive_eq[0] == 0 and list(rx.receive_eq[1]) == [100] * 14  # EEPROM.cpp:59
    rx.set_receive_eq(1, [-5, 300] * 7)
    assert rx.receive_eq[0] == 1 and list(rx.receive_eq[1]) == [-5, 300] * 7
    z = np.zeros((3, 2 * L), np.float32)
    import torch
    assert np.isfinite(rx.ProcessIQData(torch.from_numpy(z).cuda(), torch.from_numpy(z).cuda()).cpu().numpy()).all()
    ck = rx.get_state()
    rl = T.RxChain(2, T.default_params(fft_length=1024))
    rl.set_receive_eq_bands(M.bands())
    with pytest.raises(T.T41RxError) as ei:
        rl.set_receive_eq(1)
    assert ei.value.status == lib.ERR_UNSUPPORTED
    long_ck = rl.get_state()
    with_eq = np.concatenate([long_ck, np.zeros(4 * 112 * 2, np.uint8)])
    with_eq[:32].view(np.int32)[5] |= 8  # an equalizer section (sized right) at fft_length 1024
    with pytest.raises(T.T41RxError) as ei:
        rl.set_state(with_eq)
    assert ei.value.status == lib.ERR_STATE
    rl.set_state(long_ck)
    unknown = ck.copy()
    unknown[:32].view(np.int32)[5] |= 16
    with pytest.raises(T.T41RxError):
        rx.set_state(unknown)
    assert L_.t41rx_set_receive_eq(None, 1, None) == lib.ERR_ARG and L_.t41rx_get_receive_eq(None, None) == lib.ERR_ARG


@pytest.mark.gpu
def test_gpu_eq_large_batch_spot_check(built):
    kw = dict(mode=0)
    got, pre, _ = run_hip(kw, 4096, 4, seed=30)
    pick = [0, 1, 63, 64, 2047, 4095]
    assert siggen.block_rel_err(got[pick], expect(pre[pick], kw, RAMP), L).max() <= 1e-5
