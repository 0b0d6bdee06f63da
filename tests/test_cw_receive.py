"""CW receive (Process.cpp:878-913): the tone detector of DoCWReceiveProcessing() (CWProcessing.cpp:322-373) and the
narrow audio filter CWFilterIndex selects, as HIP stages behind the noise blanker and in front of the interpolators.

tests/golden/cw/cw_tables.npz holds the firmware's CW_AudioFilterCoeffs1..5 (FIR.cpp:15-65) and CW_Filter_Coeffs2
(FIR.cpp:93): their literals as float64 and the float32 rounding the firmware compiles, extracted once from that file.
The library has no copy; the caller loads them (t41rx_set_cw_tables).

CPU: the fixture, the f32 restatement (tests/cw_model.py) against float64 models, the detector's exact-tone and stale-R
properties, why the filter kernel must not contract, the entry points.  GPU (-m gpu): USB with xmtMode = CW; the
expected audio is the HIP path's own `demod` tap through the restatement and the oracle's interpolators
(stage_reference.interp), the expected detector output is the tap through the restatement; comparisons are
np.array_equal.
"""
import numpy as np
import pytest

import cw_model as M
import eq_model as EQ
import siggen
from rx_harness import assert_entry_points, calls, refused, to_q15
from stage_reference import interp

L, D = 2048, 256
CW = dict(mode=0, xmtMode=1)  # USB, xmtMode = CW_MODE
NEW = ("t41rx_set_cw_tables", "t41rx_set_cw_filter", "t41rx_get_cw_filter", "t41rx_set_cw_detector", "t41rx_get_cw_detector")


def audio(nblocks, seed, tone=750.0, amp=0.2, noise=0.05):
    rng = np.random.default_rng(seed)
    n = np.arange(nblocks * D)
    return (noise * rng.standard_normal(n.size) + amp * np.sin(2 * np.pi * tone / 24000.0 * n + 0.3)).astype(np.float32)


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_fixture_is_the_firmware_tables():
    f64, t64 = M.tables("f64")
    f32, t32 = M.tables("f32")
    assert f64.shape == (5, 6, 5) and f64.dtype == np.float64 and f32.dtype == np.float32
    assert t64.shape == (64,) and t64.dtype == np.float64 and t32.dtype == np.float32
    assert np.array_equal(f32, f64.astype(np.float32)) and np.array_equal(t32, t64.astype(np.float32))
    # low-pass sections: b1 = 2 b0 = 2 b2
    assert np.array_equal(f64[:, :, 2], f64[:, :, 0])
    assert np.allclose(f64[:, :, 1], 2 * f64[:, :, 0], rtol=1e-15, atol=0)
    poles = np.array([np.abs(np.roots([1.0, -f64[k, s, 3], -f64[k, s, 4]])).max() for k in range(5) for s in range(6)])
    assert 0.98 < poles.max() < 1.0, poles.max()
    assert np.array_equal(t64, t64[::-1])  # linear phase
    import scipy.signal as sg
    for k in range(5):  # unity in the pass band, -3 dB or less of the ripple at the corner of the comment, far down at 2 x
        _, h = sg.sosfreqz(M.sos_of(f64[k]), worN=[100.0, M.CUTOFFS[k], 2 * M.CUTOFFS[k]], fs=24000.0)
        assert abs(abs(h[0]) - 1.0) < 0.15 and abs(h[1]) > 0.6 and abs(h[2]) < 1e-3, (k, np.abs(h))


# The restatement (firmware-ordered f32) against float64 sosfilt: max block-relative error over 40 blocks of tone +
# noise, measured per table (CW receive).  The bar is the project's 1e-5; six cascaded sections with poles up
# to |z| = 0.99 put the f32 arithmetic itself just above it for tables 3 .. 5, and there the bound is 4 x the measured
# figure (f32 rounding varies by about that much with the signal).
FILTER_F64_MEASURED = (8.32e-6, 9.37e-6, 1.13e-5, 1.06e-5, 1.03e-5)
# The same for the detector's four outputs over 8 blocks (tone, noise only, a 600 Hz tone): the correlation columns sit
# at 1.5e-7; goertzel_mag's f32 recurrence (coeff = 2 cos(2 pi 8 / 256) ~ 1.96, 256 steps) at 1.93e-5 where bin 8 holds
# only leakage, and combinedCoeff inherits it.
DETECT_F64_MEASURED = (1.49e-7, 1.93e-5, 1.06e-7, 1.92e-5)


def bar(measured):
    return 1e-5 if measured < 1e-5 else 4 * measured


@pytest.mark.parametrize("index", range(5))
def test_filter_restatement_matches_float64(index):
    x = audio(40, seed=1)
    y, _ = M.Restatement().stream(x, index)
    e = M.block_rel(y, M.filter_f64(x, M.tables()[0][index]))
    bound = bar(FILTER_F64_MEASURED[index])
    print("filter %d: restatement vs float64 sosfilt, max block-relative %.2e (bound %.1e)" % (index, e.max(), bound))
    assert e.max() < bound
    assert np.array_equal(M.cascade_numpy(x[:8 * D], M.tables()[0][index]), y[:8 * D])  # the numpy loop is the same thing


def test_detector_restatement_matches_float64():
    x = np.concatenate([audio(3, seed=2), audio(2, seed=3, amp=0.0), audio(3, seed=4, tone=600.0)])
    _, got = M.Restatement().stream(x, detector=True)
    want = M.detect_f64(x)
    rel = np.abs(got - want) / np.abs(want)
    print("detector restatement vs float64: max relative per column", rel.max(0))
    for col in range(4):
        assert rel[:, col].max() < bar(DETECT_F64_MEASURED[col]), (col, rel[:, col].max())


def test_exact_tone_and_the_stale_right_side():
    """256 samples of an exact 750 Hz sine of amplitude A (bin 8 of the block) straight into goertzel_mag give A; and the
    first block's aveCorrResult is half its corrResultL (corrResultR is still the power-on 0), the second's the mean of
    the two blocks' corrResultL"""
    A = 0.25
    tone = (A * np.sin(2 * np.pi * 8 * np.arange(D) / D)).astype(np.float32)
    assert abs(float(M.goertzel_mag(tone)) / A - 1.0) < 1e-5
    m = M.Restatement()
    x = audio(3, seed=5)
    _, r = m.stream(x, detector=True)
    assert r[0, 2] == r[0, 0] / np.float32(2) and r[0, 0] > 0
    assert r[1, 2] == (r[0, 0] + r[1, 0]) / np.float32(2)
    assert r[1, 3] == np.float32(10) * r[1, 2] * np.float32(100) * r[1, 1]
    assert m.aveL == m.aveR and m.corrR == r[2, 0]  # kept although nothing reads them
    # keyed: a tone block scores far above a noise block, either side of the firmware's threshold of 50
    _, k = M.Restatement().stream(np.concatenate([audio(2, seed=6), audio(2, seed=7, amp=0.0, noise=0.01)]), detector=True)
    assert k[1, 3] > 50 > k[3, 3], k[:, 3]


def test_contraction_changes_the_filter_within_a_few_blocks():
    """why the kernel keeps every rounding: the contracted recurrence (each a*b + c rounded once) leaves the restatement
    within 4 blocks, and by more than the 1e-5 bar in the narrowest filter over 40 blocks of noise"""
    x = (0.1 * np.random.default_rng(8).standard_normal(40 * D)).astype(np.float32)
    c = M.tables()[0][0]
    r, fm = M.cascade_numpy(x, c), M.cascade_numpy(x, c, fma=True)
    assert not np.array_equal(r[:4 * D], fm[:4 * D])
    d = M.block_rel(fm, r).max()
    print("narrowest filter: contracted vs restatement %.2e" % d)
    assert d > 1e-5


def test_entry_points_declared_exported_and_bound(built):
    assert_entry_points(NEW, ("set_cw_tables", "set_cw_filter", "cw_filter", "set_cw_detector", "cw_detector"), abi_version=5,
                        pattern=r"T41RX_API\s+int\s+%s\s*\(")


# ---- GPU ---------------------------------------------------------------------------------------------------------------
KEY = np.array([1.0, 1.0, 0.0, 0.0, 1.0])  # frames keyed on, on, off, off, on


def keyed_iq(nch, nfr, seed, noise=0.02):
    """noise plus a carrier that lands on 750 Hz of audio, keyed on and off by whole frames (a frame is one detector block)"""
    nco = siggen.nco_grid(nch, seed=seed)
    rng = np.random.default_rng(seed)
    n = np.arange(nfr * L)
    key = np.repeat(KEY[np.arange(nfr) % 5], L)
    I = np.empty((nch, nfr * L), np.float32)
    Q = np.empty_like(I)
    for c in range(nch):
        # (CW mode moves the NCO by the side tone: a carrier that sits at the dial is heard at CWFreqShift = 750 Hz)
        f = siggen.passband_tone_hz(0, nco[c], 0.0)
        z = 0.3 * key * np.exp(2j * np.pi * f / 192000.0 * n) + noise * (rng.standard_normal(n.size) + 1j * rng.standard_normal(n.size))
        I[c], Q[c] = z.real, z.imag
    return nco, I, Q


def make_rx(nch, nco, kw=CW, index=5, det=0, frames=8, tables=True, eq=0, nb=0):
    import t41_sdr_amd as T
    rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
    if tables:
        rx.set_cw_tables(*M.tables())
    rx.set_cw_filter(index)
    if det:
        rx.set_cw_detector(1, frames)
    if eq:
        rx.set_receive_eq_bands(EQ.bands())
        rx.set_receive_eq(1, None)
    if nb:
        rx.set_noise_blanker(1)
    return rx


def run(rx, I, Q, edges, layout="channel"):
    """the stream in calls of edges[k] .. edges[k + 1] frames: (audio, demod tap, detector results [nch][nfr][4]); int16
    rows go through the q15 entry point"""
    nch = I.shape[0]
    if layout == "time":
        rx.set_buffer_layout("time")

    def det(rx, a, b):
        return rx.cw_results(b - a).cpu().numpy().copy() if rx.cw_detector and rx.params.xmtMode == 1 else np.full((nch, b - a, 4), np.nan, np.float32)

    out, tap, dets = calls(rx, I, Q, edges, after=det, layout=layout, tap_floats=D)
    return out, tap, np.concatenate(dets, 1)


def model(tap, index=5, detector=False, on=None, pre=None):
    """the tap through the restatement, channel by channel: (audio @24 kS/s, detector results); pre: a stage in front"""
    a24, res = np.empty_like(tap), np.empty((tap.shape[0], tap.shape[1] // D, 4), np.float32)
    for ch in range(tap.shape[0]):
        x = tap[ch] if pre is None else pre(tap[ch])
        a24[ch], res[ch] = M.Restatement().stream(x, index, detector, on)
    return a24, res


def report(what, got, want):
    """print the figure, hold it to the project's whole-path bar (1e-5: what the back kernel alone is held to against
    the oracle's interpolators), and leave the bit-for-bit comparison to the caller"""
    e = siggen.block_rel_err(got, want, L)
    print("%s: max block-relative %.2e, bit-identical %s" % (what, e.max(), np.array_equal(got, want)))
    assert e.max() <= 1e-5, (what, e.max())
    return np.array_equal(got, want)


def states(tap, index=5, detector=False, on=None, pre=None):
    """the 128 state floats per channel the restatement holds behind the tap"""
    ms = [M.Restatement() for _ in range(tap.shape[0])]
    for ch, m in enumerate(ms):
        m.stream(tap[ch] if pre is None else pre(tap[ch]), index, detector, on)
    return np.stack([m.state_vector() for m in ms])


SHAPES = [(1, 1), (3, 2), (9, 5)]  # channels 1, 3 and one more than the filter kernel's 8 per wave; frames 1, 2, 5


@pytest.mark.gpu
@pytest.mark.parametrize("index", range(5))
def test_gpu_each_filter(built, index):
    """CWFilterIndex 0..4 at every shape: the filter's memories behind the call are the restatement's, and the audio is
    interp(cw_model(tap)), both bit for bit.  (Behind the narrow filter the path interpolates with cw_back_kernel, the
    firmware's operations in its order; the fused back kernel, which folds the volume into the x4 taps and accumulates
    with fused multiply-adds, sits 1.5e-7 .. 3.4e-7 from the oracle's interpolators -- test_gpu_detector prints it.)"""
    exact = []
    for nch, nfr in SHAPES:
        nco, I, Q = keyed_iq(nch, nfr, seed=10 + index)
        rx = make_rx(nch, nco, index=index)
        got, tap, _ = run(rx, I, Q, [0, nfr])
        want = interp(model(tap, index)[0], CW)
        off, _, _ = run(make_rx(nch, nco), I, Q, [0, nfr])
        assert np.abs(tap).max() > 0 and siggen.block_rel_err(got, off, L).max() > 1e-3  # the stage ran
        # the filter's memories behind the call are the restatement's bit for bit (24 kS/s, no interpolator between)
        assert np.array_equal(_section(rx.get_state(), nch), states(tap, index)), (nch, nfr)
        exact.append(report("filter %d, %d x %d" % (index, nch, nfr), got, want))
    assert all(exact), exact


@pytest.mark.gpu
def test_gpu_off_is_untouched(built):
    """index 5 with the detector off = a context that never touched the feature; and xmtMode SSB with everything on = the
    feature off, d_cw untouched, memories not advanced: the later switch to CW continues from the earlier state"""
    nch, nfr = 9, 5
    nco, I, Q = keyed_iq(nch, nfr, seed=20)
    plain, _, _ = run(make_rx(nch, nco, tables=False), I, Q, [0, nfr])
    touched = make_rx(nch, nco, index=2, det=1)
    touched.set_cw_filter(5)
    touched.set_cw_detector(0)
    got, _, _ = run(touched, I, Q, [0, nfr])
    assert np.array_equal(got, plain)
    assert touched.get_state().size == make_rx(nch, nco, tables=False).get_state().size  # nothing ran: no section
    # SSB in the middle of a CW stream
    rx = make_rx(nch, nco, index=1, det=1)
    buf = rx.cw_results(8)
    a, ta, da = run(rx, I, Q, [0, 2])
    ck = rx.get_state()
    rx.CalcFilters(xmtMode=0)
    assert rx.cw_filter == 1 and rx.cw_detector == 1  # the settings are kept
    buf.fill_(-7.0)
    b, tb, _ = run(rx, I, Q, [2, 3])
    assert (buf == -7.0).all().item()  # d_cw is not written
    ssb = make_rx(nch, nco, kw=dict(mode=0, xmtMode=0), tables=False)
    ssb.set_state(_without_sections(ck, ssb))
    b_ref, _, _ = run(ssb, I, Q, [2, 3])
    assert np.array_equal(b, b_ref)
    after = rx.get_state()
    assert np.array_equal(_section(after, nch), _section(ck, nch))  # the memories did not advance
    rx.CalcFilters(xmtMode=1)
    c, tc, dc = run(rx, I, Q, [3, nfr])
    on = np.arange(nfr) != 2
    tap = np.concatenate([ta, tb, tc], 1)
    a24, res = model(tap, 1, True, on)
    assert np.array_equal(np.concatenate([da, dc], 1), res[:, on])
    assert np.array_equal(_section(rx.get_state(), nch), states(tap, 1, True, on))
    # (the audio to the whole-path bar: the SSB frame went through the fused kernel's interpolators, which are not the
    # oracle's bit for bit, and left their histories to the frames behind it)
    report("CW around an SSB frame", np.concatenate([a, b, c], 1), interp(a24, CW))


def _section(ck, nch):
    """the CW section of a checkpoint whose only section it is"""
    assert ck[:32].view(np.int32)[5] == 16
    return ck[-4 * 128 * nch:].view(np.float32).reshape(nch, 128)


def _without_sections(ck, like):
    """the path records of checkpoint ck under a header without sections, sized for context `like`"""
    out = ck[:like.get_state().size].copy()
    out[:32].view(np.int32)[5] = 0
    return out


@pytest.mark.gpu
def test_gpu_detector(built):
    """detector on, filter off: d_cw = the restatement bit for bit over a keyed 750 Hz tone; the audio is that of the
    detector-off run.  Both on: the detector sees the unfiltered audio."""
    for nch, nfr in SHAPES:
        nco, I, Q = keyed_iq(nch, nfr, seed=30, noise=0.002)
        off, _, _ = run(make_rx(nch, nco), I, Q, [0, nfr])
        got, tap, det = run(make_rx(nch, nco, det=1), I, Q, [0, nfr])
        _, want = model(tap, detector=True)
        print("%d x %d combinedCoeff, channel 0:" % (nch, nfr), det[0, :, 3], "model", want[0, :, 3])
        assert np.array_equal(det, want), (nch, nfr)
        assert np.array_equal(got, off)
        report("detector on, filter off, %d x %d (the back kernel against the oracle's interpolators)" % (nch, nfr), got, interp(tap, CW))
        both, tap2, det2 = run(make_rx(nch, nco, index=0, det=1), I, Q, [0, nfr])
        assert np.array_equal(tap2, tap) and np.array_equal(det2, want)
        only, _, _ = run(make_rx(nch, nco, index=0), I, Q, [0, nfr])
        assert np.array_equal(both, only)
    # (the last shape has 5 frames) combinedCoeff goes with the block's power at 750 Hz and the tone is 43 dB above the
    # noise per sample before the path narrows the band: a keyed frame scores orders of magnitude above frame 3, the
    # second silent one (frame 2 still holds the tail the path's filters delay)
    keyed = det[0, :, 3]
    assert keyed[1] > 100 * keyed[3] and keyed[4] > 100 * keyed[3] and keyed[1] > 50, keyed


@pytest.mark.gpu
def test_gpu_split_calls_checkpoint_reset(built):
    nch, nfr, cut = 9, 5, 2
    nco, I, Q = keyed_iq(nch, nfr, seed=40)
    whole, tap, dwhole = run(make_rx(nch, nco, index=3, det=1), I, Q, [0, nfr])
    got, _, dgot = run(make_rx(nch, nco, index=3, det=1), I, Q, [0, 1, 2, 3, 4, 5])
    assert np.array_equal(got, whole) and np.array_equal(dgot, dwhole)
    rx = make_rx(nch, nco, index=3, det=1)
    fresh = rx.get_state()
    assert fresh[:32].view(np.int32)[5] == 0
    a, _, da = run(rx, I, Q, [0, cut])
    ck = rx.get_state()
    assert ck.size == fresh.size + 4 * 128 * nch and ck[:32].view(np.int32)[5] == 16  # section bit 4
    assert np.array_equal(_section(ck, nch), states(tap[:, :cut * D], 3, True))
    run(rx, I, Q, [0, 1])  # disturb
    rx.set_state(ck)
    b, _, db = run(rx, I, Q, [cut, nfr])
    assert np.array_equal(np.concatenate([a, b], 1), whole) and np.array_equal(np.concatenate([da, db], 1), dwhole)
    ry = make_rx(nch, nco, index=3, det=1)
    ry.set_state(ck)  # a fresh context: the section allocates and restores the memories
    b2, _, db2 = run(ry, I, Q, [cut, nfr])
    assert np.array_equal(b2, b) and np.array_equal(db2, db)
    rx.set_state(fresh)  # no section: the memories restart at zero
    w2, _, dw2 = run(rx, I, Q, [0, nfr])
    assert np.array_equal(w2, whole) and np.array_equal(dw2, dwhole)
    rx.reset()
    w3, _, dw3 = run(rx, I, Q, [0, nfr])
    assert np.array_equal(w3, whole) and np.array_equal(dw3, dwhole)
    # the switches and tables survive set_params / set_coeffs
    rx.reset()
    o1, _, _ = run(rx, I, Q, [0, cut])
    rx.CalcFilters(audioVolume=rx.params.audioVolume)
    rx.set_coeffs(rx.coeffs())
    assert rx.cw_filter == 3 and rx.cw_detector == 1
    o2, _, _ = run(rx, I, Q, [cut, nfr])
    assert np.array_equal(np.concatenate([o1, o2], 1), whole)


@pytest.mark.gpu
def test_gpu_filter_switched_away_and_back_is_stale(built):
    """filter 1 -> 3 -> 1: the second run of filter 1 starts from the memory it had, as the model with five states does
    (memories and audio bit for bit; memories zeroed at the switch are told apart)"""
    nch, nfr = 3, 5
    nco, I, Q = keyed_iq(nch, nfr, seed=50)
    rx = make_rx(nch, nco, index=1)
    outs, taps = [], []
    for (a, b), idx in zip(((0, 2), (2, 3), (3, 5)), (1, 3, 1)):
        rx.set_cw_filter(idx)
        o, t, _ = run(rx, I, Q, [a, b])
        outs.append(o)
        taps.append(t)
    got, tap = np.concatenate(outs, 1), np.concatenate(taps, 1)
    per = [1, 1, 3, 1, 1]
    want = interp(model(tap, per)[0], CW)
    fresh = model(tap, per)[0]
    fresh[:, 3 * D:] = model(tap[:, 3 * D:], 1)[0]  # memories zeroed at the switch back: must differ
    assert np.array_equal(_section(rx.get_state(), nch), states(tap, per))
    exact = report("filter 1 -> 3 -> 1", got, want)
    assert siggen.block_rel_err(got, interp(fresh, CW), L)[:, 3].max() > 1e-3
    assert exact


@pytest.mark.gpu
def test_gpu_equalizer_in_front_of_the_filter(built):
    """order: the equalizer on in front of the narrow filter = cw_model(eq_model(tap)), detector off.  Two linear
    stages commute up to rounding, so only bits tell the order: the filter's memories are those of the restatement fed
    with equalized audio, bit for bit, and so is the audio."""
    nch, nfr = 3, 5
    nco, I, Q = keyed_iq(nch, nfr, seed=60)
    rx = make_rx(nch, nco, index=2, eq=1)
    got, tap, _ = run(rx, I, Q, [0, nfr])
    eq = lambda x: EQ.Restatement().stream(x, [100] * 14)  # noqa: E731
    want = interp(model(tap, 2, pre=eq)[0], CW)
    ck = rx.get_state()
    assert ck[:32].view(np.int32)[5] == 8 | 16  # the equalizer's section, then this one
    sec = ck[-4 * 128 * nch:].view(np.float32).reshape(nch, 128)
    assert np.array_equal(sec, states(tap, 2, pre=eq)) and not np.array_equal(sec, states(tap, 2))
    assert report("equalizer -> filter 2", got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["q15", "time"])
def test_gpu_formats(built, how):
    nch, nfr = 3, 2
    nco, I, Q = keyed_iq(nch, nfr, seed=70)
    if how == "time":
        whole, _, dwhole = run(make_rx(nch, nco, index=4, det=1), I, Q, [0, nfr])
        got, _, det = run(make_rx(nch, nco, index=4, det=1), I, Q, [0, nfr], layout="time")
        assert np.array_equal(got, whole) and np.array_equal(det, dwhole)
        return
    # q15 in: the f32 path on the converted samples (x / 32768, arm_q15_to_float) is the same stream; q15 out: the
    # firmware's conversion of the f32 result (truncating, saturating arm_float_to_q15)
    Iq, Qq = to_q15(I, 1 / 4), to_q15(Q, 1 / 4)
    If, Qf = [(v.astype(np.float32) / np.float32(32768.0)) for v in (Iq, Qq)]
    whole, _, dwhole = run(make_rx(nch, nco, index=4, det=1), If, Qf, [0, nfr])
    got, _, det = run(make_rx(nch, nco, index=4, det=1), Iq, Qq, [0, nfr])
    ref = np.clip(np.trunc(whole.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    assert np.abs(ref).max() > 100
    assert np.array_equal(det, dwhole) and np.array_equal(got, ref)


@pytest.mark.gpu
def test_gpu_refusals(built):
    import torch
    import t41_sdr_amd as T
    import t41_sdr_amd._lib as lib
    L_ = lib.load()
    nch = 3
    rx = T.RxChain(nch, T.default_params(**CW))

    assert rx.cw_filter == 5 and rx.cw_detector == 0  # the firmware's defaults
    refused(lambda: rx.set_cw_filter(6), lib.ERR_ARG, "CWFilterIndex")
    refused(lambda: rx.set_cw_filter(-1), lib.ERR_ARG, "CWFilterIndex")
    refused(lambda: rx.set_cw_filter(2), lib.ERR_ARG, "tables")  # before the tables are loaded
    refused(lambda: rx.set_cw_detector(1, 4), lib.ERR_ARG, "FIR")
    filt, fir = M.tables()
    bad = filt.copy()
    bad[3, 2, 1] = np.inf
    refused(lambda: rx.set_cw_tables(bad, fir), lib.ERR_ARG, "non-finite")
    refused(lambda: rx.set_cw_filter(2), lib.ERR_ARG, "tables")  # (the refused call loaded nothing)
    refused(lambda: rx.set_cw_detector(1, 4), lib.ERR_ARG, "FIR")
    rx.set_cw_tables(filt, None)
    rx.set_cw_filter(2)
    refused(lambda: rx.set_cw_detector(1, 4), lib.ERR_ARG, "FIR")
    rx.set_cw_tables(None, fir)
    assert L_.t41rx_set_cw_detector(rx._ctx, 1, None, 4) == lib.ERR_ARG and b"NULL" in L_.t41rx_last_error()
    assert L_.t41rx_set_cw_detector(rx._ctx, 2, None, 4) == lib.ERR_ARG
    assert L_.t41rx_set_cw_tables(None, None, None) == lib.ERR_ARG and L_.t41rx_get_cw_filter(None) == lib.ERR_ARG
    assert L_.t41rx_get_cw_detector(None) == lib.ERR_ARG and L_.t41rx_set_cw_filter(None, 1) == lib.ERR_ARG
    rx.set_cw_detector(1, 2)
    z = torch.zeros(nch, 3 * L, device="cuda")
    refused(lambda: rx.ProcessIQData(z, z), lib.ERR_ARG, "max_frames")  # more frames than max_frames
    assert np.isfinite(rx.ProcessIQData(z[:, :2 * L].contiguous(), z[:, :2 * L].contiguous()).cpu().numpy()).all()
    assert not rx.cw_results(2).cpu().numpy().any()  # silence scores 0
    # the detector behind a stage that splits L from R, with nothing that joins them again
    rx.set_receive_eq_bands(EQ.bands())
    rx.set_receive_eq(1)
    zz = z[:, :L].contiguous()
    refused(lambda: rx.ProcessIQData(zz, zz), lib.ERR_UNSUPPORTED, "receive equalizer")
    rx.set_noise_blanker(1)
    rx.ProcessIQData(zz, zz)  # the blanker joins them
    rx.set_noise_blanker(0)
    rx.CalcFilters(ANR_notchOn=1)
    rx.ProcessIQData(zz, zz)  # so does the notch
    rx.CalcFilters(ANR_notchOn=0, nrOptionSelect=2)
    rx.ProcessIQData(zz, zz)  # the spectral noise reduction ends with R = L
    rx.set_receive_eq(0)
    rx.CalcFilters(nrOptionSelect=1)
    refused(lambda: rx.ProcessIQData(zz, zz), lib.ERR_UNSUPPORTED, "Kim")
    rx.CalcFilters(nrOptionSelect=3)
    refused(lambda: rx.ProcessIQData(zz, zz), lib.ERR_UNSUPPORTED, "LMS")
    rx.set_cw_detector(0)
    rx.ProcessIQData(zz, zz)  # the filter alone reads L only
    # fft_length 1024
    rl = T.RxChain(2, T.default_params(fft_length=1024, **CW))
    rl.set_cw_tables(filt, fir)
    refused(lambda: rl.set_cw_filter(0), lib.ERR_UNSUPPORTED, "fft_length 512")
    refused(lambda: rl.set_cw_detector(1, 2), lib.ERR_UNSUPPORTED, "fft_length 512")
    rl.set_cw_filter(5)
    rl.set_cw_detector(0)
    long_ck = rl.get_state()
    with_cw = np.concatenate([long_ck, np.zeros(4 * 128 * 2, np.uint8)])
    with_cw[:32].view(np.int32)[5] |= 16  # a CW section (sized right) at fft_length 1024
    refused(lambda: rl.set_state(with_cw), lib.ERR_STATE, "CW-receive", "long fft_length")
    rl.set_state(long_ck)
