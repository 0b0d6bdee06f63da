"""Audio at 24 kS/s (t41rx_set_audio_rate): every process entry then writes, per channel and frame, the 256 samples of
float_buffer_L as they stand in front of Process.cpp:917 times g = VolumeToAmplification(audioVolume), and the
interpolators neither run nor change their memories.

References: the oracle's TAP_DEMOD (tests/oracle_lib.py) read frame by frame, the HIP path's own demod tap, the stage
models of the stage tests (imported from those files, so that a stage is held to the same model and the same tolerance at
either rate), and the 192 kS/s context for everything that must not move.  19 channels: one 16-wave workgroup and a ragged
tail, five 4-wave ones with a ragged last.  Calls of 1, 3 and 6 frames: 3 takes the barrier form of the AGC / SAM
kernels, 6 the pipelined one.

The synchronous detector is compared with the oracle as tests/test_sam.py compares it at 192 kS/s -- from frame LOCKED
on, within 1e-5, over a stream of three 6-frame calls -- because before lock two evaluations of the loop follow different
trajectories (test_gpu_sam_pull_in_bound's docstring); its first 6 frames are pinned bit for bit to the HIP path's own
demod tap instead.
"""
import numpy as np
import pytest

import oracle_lib as O
import siggen
import group_harness as G
from group_harness import D, L, NCH, SET_OF as SETOF
from rx_harness import ERR_UNSUPPORTED, INT1, INT2, TOL, T, calls, one_call, refused, same, to_q15  # noqa: F401  (T: a fixture)
from stage_reference import nr_stage, vol_scale

pytestmark = pytest.mark.gpu

AM_TOL = 5e-5  # tests/test_gpu_parity.py: the bound test_stage_taps_match_the_oracle applies to the AM demod tap
GENERAL = dict(RFgain=3, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=-0.013)  # the general front end (this file's)


def g_of(audioVolume=30):
    """VolumeToAmplification(audioVolume) as the float the firmware computes: Process.cpp:929's factor without DF = 8"""
    return np.float32(vol_scale(audioVolume) / np.float32(8.0))


def chain(T, kw, nco, rate=24000, layout="channel"):
    return G.chain(T, kw, nco, rate=rate, layout=layout)[0]


def signal(kw, nch, nfr, nco, seed):
    mode = kw.get("mode", 0)
    if mode == 3:
        return siggen.make_fm(nch, nfr * L, nco, seed=seed)
    if mode == 8:
        return siggen.make_am_carrier(nch, nfr * L, nco, seed=seed)
    return siggen.make_iq(nch, nfr * L, nco, mode=mode, seed=seed)


def oracle_demod(kw, nco, I, Q, q15=False):
    """the oracle's TAP_DEMOD of every frame, [nch, nfr * 256]; q15: I, Q are int16 and go through process_q15"""
    ob = O.OracleBatch(O.default_params(**kw), np.asarray(nco, np.int32))
    nch, nfr = I.shape[0], I.shape[1] // L
    out = np.empty((nch, nfr * D), np.float32)
    for f in range(nfr):
        sl = slice(f * L, (f + 1) * L)
        if q15:
            ob.process_q15(Q[:, sl], I[:, sl])  # (the L queue carries Q, the R queue I: Process.cpp:107-108)
        else:
            ob.process(I[:, sl], Q[:, sl])
        for c in range(nch):
            out[c, f * D:(f + 1) * D] = ob.tap(c, O.TAP_DEMOD, D)
    ob.close()
    return out


def tap_rel(got, ref):
    """test_stage_taps_match_the_oracle's figure for the demod tap, per channel and frame: max|a - b| / max|b|"""
    a = got.astype(np.float64).reshape(got.shape[0], -1, D)
    b = ref.astype(np.float64).reshape(ref.shape[0], -1, D)
    return np.abs(a - b).max(axis=2) / np.maximum(np.abs(b).max(axis=2), 1e-30)


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------
MODES = {
    "usb": (dict(mode=0, FLoCut=200, FHiCut=3000), TOL), "lsb": (dict(mode=1, FLoCut=-3000, FHiCut=-200), TOL),
    "am": (dict(mode=2, FLoCut=-3000, FHiCut=3000), AM_TOL), "nfm": (dict(mode=3, FLoCut=200, FHiCut=3000), TOL),
    "nfm-atan": (dict(mode=3, FLoCut=200, FHiCut=3000, nfm_demod=1), TOL),
}


@pytest.mark.parametrize("agc", [0, 2], ids=["agc-off", "agc-slow"])
@pytest.mark.parametrize("name", sorted(MODES))
def test_fused_form_against_the_oracle(T, name, agc):
    """6 frames in one call, no taps: the fused 24 kS/s form (AGC on: its pipelined form) against TAP_DEMOD x g"""
    kw, tol = MODES[name]
    kw = dict(kw, AGCMode=agc)
    nfr = 6
    nco = siggen.nco_grid(NCH, seed=21)
    I, Q = signal(kw, NCH, nfr, nco, seed=22)
    got, _ = one_call(chain(T, kw, nco), I, Q)
    ref = oracle_demod(kw, nco, I, Q) * g_of()
    e = tap_rel(got, ref)
    print("%s AGCMode %d: worst relative error %.2e (bound %.0e)" % (name, agc, e.max(), tol))
    assert np.isfinite(got).all() and np.abs(ref).reshape(NCH, nfr, D).max(axis=2).min() > 0
    assert e.max() <= tol, (e.max(), np.unravel_index(e.argmax(), e.shape))


@pytest.mark.parametrize("agc", [0, 2], ids=["agc-off", "agc-slow"])
def test_sam_against_the_oracle_and_its_own_tap(T, agc):
    """the synchronous detector (PSAM / PSA forms): three 6-frame calls, within 1e-5 of the oracle from frame LOCKED on
    as at 192 kS/s (test_gpu_sam_parity); and the first call bit for bit the demod tap x g of a context that runs the
    same 6 frames with the tap on"""
    import test_sam as S
    kw = dict(S.KW, AGCMode=agc)
    nfr = 18
    nco = siggen.nco_grid(NCH, seed=21)
    I, Q = siggen.make_am_carrier(NCH, nfr * L, nco, seed=40 + agc)
    got, _, _ = calls(chain(T, kw, nco), I, Q, [0, 6, 12, 18])
    ref = oracle_demod(kw, nco, I, Q) * g_of()
    e = tap_rel(got, ref)
    print("SAM AGCMode %d: worst relative error per frame %s" % (agc, " ".join("%.1e" % v for v in e.max(axis=0))))
    assert np.isfinite(got).all() and np.abs(ref[:, S.LOCKED * D:]).max() > 1e-4
    assert e[:, S.LOCKED:].max() <= TOL, e[:, S.LOCKED:].max()
    _, tap = one_call(chain(T, kw, nco, rate=192000), I[:, :6 * L], Q[:, :6 * L], tap_floats=D)
    assert same(got[:, :6 * D], tap * g_of())


# ---- 2. the multiply and the layout ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channel", "time"])
@pytest.mark.parametrize("name,kw", [("usb", dict(mode=0, audioVolume=37)), ("lsb-agc", dict(mode=1, FLoCut=-3000, FHiCut=-200, AGCMode=2)),
                                     ("am", dict(mode=2, FLoCut=-3000, FHiCut=3000, audioVolume=55)), ("nfm", dict(mode=3))])
def test_output_is_the_demod_tap_times_g(T, name, kw, layout):
    """general gains, so that the tap kernels and the fused kernels run the same front end: with the demod tap on in the
    same 24 kS/s call (tap kernel + finish kernel) the output is tap x float32(g) bit for bit, and the same call without
    the tap (the fused 24 kS/s form) gives the same bits.
    NFM: the first half holds bit for bit; the second within TOL only.  The tap instantiation of the NFM kernel writes
    the discriminator's output to the dec tap and its demodulator is not written contraction-free (SSB is a multiply, AM
    turns contraction off), so the two instantiations round the demodulated audio differently -- at 192 kS/s too, where
    the parent's outputs with and without a tap differ in the same way (measured on this input: 3.9e-7 of the frame's peak
    at 192 kS/s on the parent's library, 4.3e-7 here)."""
    kw = dict(kw, **GENERAL)
    nfr = 6
    nco = siggen.nco_grid(NCH, seed=31)
    I, Q = signal(kw, NCH, nfr, nco, seed=32)
    with_tap, tap = one_call(chain(T, kw, nco, layout=layout), I, Q, layout=layout, tap_floats=D)
    g = g_of(kw.get("audioVolume", 30))
    assert np.abs(tap).reshape(NCH, nfr, D).max(axis=2).min() > 0
    assert same(with_tap, tap * g)
    fused, _ = one_call(chain(T, kw, nco, layout=layout), I, Q, layout=layout)
    if name == "nfm":
        e = tap_rel(fused, with_tap)
        print("nfm: fused form against the tap kernel's audio, worst relative difference %.2e" % e.max())
        assert e.max() <= TOL
    else:
        assert same(fused, with_tap)


# ---- 3. nothing else moved ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw", [("usb", dict(mode=0)), ("usb-general", dict(mode=0, **GENERAL)), ("usb-agc", dict(mode=0, AGCMode=2)),
                                     ("am", dict(mode=2, FLoCut=-3000, FHiCut=3000)), ("sam-agc", dict(mode=8, FLoCut=-3000, FHiCut=3000, AGCMode=2)),
                                     ("nfm", dict(mode=3))])
def test_state_records_equal_but_for_the_interpolator_memories(T, name, kw):
    """2 frames at 192 kS/s on both contexts, then 6 frames of the same input at 24 kS/s on one and at 192 kS/s on the
    other: the records are equal bit for bit except kStInt1 / kStInt2, which at 24 kS/s still hold what the 2-frame call
    left; back at 192 kS/s the context goes on"""
    nco = siggen.nco_grid(NCH, seed=41)
    I, Q = signal(kw, NCH, 9, nco, seed=42)
    a, b = chain(T, kw, nco, rate=192000), chain(T, kw, nco, rate=192000)
    first, _ = one_call(a, I[:, :2 * L], Q[:, :2 * L])
    one_call(b, I[:, :2 * L], Q[:, :2 * L])
    before = a.state_records().copy()
    assert same(before, b.state_records()) and before[:, INT1].any() and before[:, INT2].any()
    size = len(a.get_state())
    a.set_audio_rate(24000)
    assert a.audio_rate == 24000 and a.audio_frame_len == D and len(a.get_state()) == size
    sl = slice(2 * L, 8 * L)
    got, _ = one_call(a, I[:, sl], Q[:, sl])
    one_call(b, I[:, sl], Q[:, sl])
    ra, rb = a.state_records(), b.state_records()
    rest = np.ones(ra.shape[1], bool)
    rest[INT1] = rest[INT2] = False
    assert same(ra[:, rest], rb[:, rest])
    assert same(ra[:, INT1], before[:, INT1]) and same(ra[:, INT2], before[:, INT2])
    assert not same(rb[:, INT1], before[:, INT1])  # (the 192 kS/s context's did move)
    assert np.abs(got).reshape(NCH, 6, D).max(axis=2).min() > 0
    a.set_audio_rate(192000)
    again, _ = one_call(a, I[:, 8 * L:], Q[:, 8 * L:])
    assert again.shape == (NCH, L) and np.isfinite(again).all() and np.abs(again).max() > 0


def test_side_outputs_equal_the_192k_context(T):
    """audio spectrum / S-meter words, the panadapter's rows and the FT8 stage's status words and power bytes: the same
    bits at either rate (16 frames, so that the FT8 stage finishes a block of 15)"""
    import torch
    nfr = 16
    kw = dict(mode=0, FLoCut=200, FHiCut=3000)
    nco = siggen.nco_grid(NCH, seed=51)
    I, Q = signal(kw, NCH, nfr, nco, seed=52)

    def spectrum(rx):
        sp, mx = torch.zeros(NCH, nfr, 1024, device="cuda"), torch.zeros(NCH, nfr, 3, device="cuda")
        rx.set_audio_spectrum(sp, mx)
        return lambda: [sp.cpu().numpy(), mx.cpu().numpy()]

    def panadapter(rx):
        bufs = G.panadapter(rx, nfr, spectrumZoom=1, currentScale=1, update_period=3)
        return lambda: [bufs[n].cpu().numpy() for n, _, _ in rx.PANADAPTER_ROWS]

    def ft8(rx):
        G.ft8_receive(rx, nfr)
        return lambda: G.ft8_results(rx, nfr)

    plain, _ = one_call(chain(T, dict(kw, **GENERAL), nco), I, Q)
    for what, setup in (("audio spectrum", spectrum), ("panadapter", panadapter), ("FT8", ft8)):
        res, aud = [], []
        for rate in (24000, 192000):
            rx = chain(T, dict(kw, **GENERAL), nco, rate=rate)
            read = setup(rx)
            aud.append(one_call(rx, I, Q)[0])
            res.append(read())
        assert all(same(x, y) for x, y in zip(*res)) and any(x.any() for x in res[0]), what
        # and the audio of the call with the side output on is the fused form's (general front end in both)
        assert same(aud[0], plain), what
        assert aud[1].shape == (NCH, nfr * L)


# ---- 4. forms against each other, bit for bit -----------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(mode=0), dict(mode=0, AGCMode=2), dict(mode=2, FLoCut=-3000, FHiCut=3000)], ids=["usb", "usb-agc", "am"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_time_major_equals_channel_major(T, kw, q15):
    nco = siggen.nco_grid(NCH, seed=61)
    I, Q = signal(kw, NCH, 6, nco, seed=62)
    opt = dict(q15_scale=1.0) if q15 else {}
    a, _ = one_call(chain(T, dict(kw, audioVolume=100), nco), I, Q, **opt)
    b, _ = one_call(chain(T, dict(kw, audioVolume=100), nco, layout="time"), I, Q, layout="time", **opt)
    assert a.dtype == (np.int16 if q15 else np.float32) and np.abs(a.astype(np.float64)).max(axis=1).min() > 0
    assert same(a, b)


@pytest.mark.parametrize("layout", ["channel", "time"])
@pytest.mark.parametrize("kw", [dict(mode=0), dict(mode=0, AGCMode=2)], ids=["usb", "usb-agc"])
def test_mapped_call_equals_replicated_rows(T, kw, layout):
    nco = siggen.nco_grid(NCH, seed=63)
    smap = (np.arange(NCH) * 7 % 2).astype(np.int32)
    I, Q = (0.2 * np.random.default_rng(64).standard_normal((2, 2, 6 * L))).astype(np.float32)  # two streams of noise
    a = chain(T, kw, nco, layout=layout)
    a.set_input_map(smap, 2)
    got, _ = one_call(a, I, Q, layout=layout)
    want, _ = one_call(chain(T, kw, nco, layout=layout), I[smap], Q[smap], layout=layout)
    assert np.abs(got).max(axis=1).min() > 0 and same(got, want)


# the sets differ in sideband, pass band and audioVolume
SETS = [dict(mode=1, FLoCut=-3000, FHiCut=-200, audioVolume=45), dict(mode=0, FLoCut=300, FHiCut=1000, audioVolume=18)]


@pytest.mark.parametrize("agc", [0, 2], ids=["agc-off", "agc-slow"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_mixed_context_equals_the_per_set_contexts(T, agc, q15):
    """3 sets in one context against three plain contexts, audio and records; g is the channel's own set's"""
    base = dict(mode=0, FLoCut=200, FHiCut=3000, AGCMode=agc, audioVolume=100 if q15 else 30)
    extra = [dict(s, audioVolume=s["audioVolume"] + (40 if q15 else 0)) for s in SETS]
    nco = siggen.nco_grid(NCH, seed=65)
    rng = np.random.default_rng(66)
    I, Q = (0.2 * rng.standard_normal((2, NCH, 6 * L))).astype(np.float32)
    opt = dict(q15_scale=1.0) if q15 else {}
    mixed = chain(T, base, nco)
    mixed.set_param_sets(extra, SETOF)
    got, _ = one_call(mixed, I, Q, **opt)
    assert np.abs(got.astype(np.float64)).max(axis=1).min() > 0
    for k, e in enumerate([{}] + extra):
        ref = chain(T, dict(base, **e), nco)
        want, _ = one_call(ref, I, Q, **opt)
        sel = SETOF == k
        assert same(got[sel], want[sel]), "audio of set %d" % k
        assert same(mixed.state_records()[sel], ref.state_records()[sel]), "records of set %d" % k


@pytest.mark.parametrize("kw", [dict(mode=0, AGCMode=2), dict(mode=8, FLoCut=-3000, FHiCut=3000, AGCMode=2), dict(mode=3, AGCMode=1),
                                dict(mode=8, FLoCut=-3000, FHiCut=3000), dict(mode=2, FLoCut=-3000, FHiCut=3000, AGCMode=4)],
                         ids=["usb-agc", "sam-agc", "nfm-agc", "sam", "am-agc"])
def test_calls_of_1_2_3_frames_equal_one_call_of_6(T, kw):
    nco = siggen.nco_grid(NCH, seed=67)
    I, Q = signal(kw, NCH, 6, nco, seed=68)
    a, b = chain(T, kw, nco), chain(T, kw, nco)
    whole, _ = one_call(a, I, Q)
    parts, _, _ = calls(b, I, Q, [0, 1, 3, 6])
    assert np.abs(whole).max(axis=1).min() > 0
    assert same(parts, whole) and same(a.state_records(), b.state_records())


@pytest.mark.parametrize("layout", ["channel", "time"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_host_entry_equals_device_entry(T, layout, q15):
    kw = dict(mode=0, AGCMode=2, audioVolume=100)
    nco = siggen.nco_grid(NCH, seed=69)
    I, Q = signal(kw, NCH, 6, nco, seed=70)
    opt = dict(q15_scale=1.0) if q15 else {}
    a, b = chain(T, kw, nco, layout=layout), chain(T, kw, nco, layout=layout)
    dev, _ = one_call(a, I, Q, layout=layout, **opt)
    host, _ = one_call(b, I, Q, layout=layout, host=True, **opt)
    assert host.dtype == (np.int16 if q15 else np.float32) and np.abs(dev.astype(np.float64)).max() > 0
    assert same(dev, host) and np.array_equal(a.get_state(), b.get_state())
    # the stage-tap path (tap kernel + finish kernel) through the host entry too
    c = chain(T, dict(kw, **GENERAL), nco, layout=layout)
    d = chain(T, dict(kw, **GENERAL), nco, layout=layout)
    assert same(one_call(c, I, Q, layout=layout, host=True, tap_floats=D, **opt)[0], one_call(d, I, Q, layout=layout, **opt)[0])


# ---- 5. q15 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
@pytest.mark.parametrize("name,kw", [("usb", dict(mode=0)), ("lsb-general", dict(mode=1, FLoCut=-3000, FHiCut=-200, **GENERAL)),
                                     ("usb-agc", dict(mode=0, AGCMode=2)), ("nfm", dict(mode=3))])
def test_q15_entries_against_the_oracle(T, name, kw, host):
    """the q15 entries within +-1 LSB of to_q15(oracle process_q15's TAP_DEMOD x g): the float chains differ by <= 1e-5 of
    the block maximum (<= 0.33 LSB), the kernel truncates (arm_float_to_q15) where to_q15 rounds"""
    kw = dict(kw, audioVolume=100)
    nfr = 6
    nco = siggen.nco_grid(NCH, seed=71)
    I, Q = signal(kw, NCH, nfr, nco, seed=72)
    qI, qQ = to_q15(I), to_q15(Q)
    got, _ = one_call(chain(T, kw, nco), qI, qQ, host=host)
    want = to_q15(oracle_demod(kw, nco, qI, qQ, q15=True).astype(np.float64) * np.float64(g_of(100)))
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print("%s: worst difference %d LSB, differing %.3f, peak %d" % (name, d.max(), (d > 0).mean(), np.abs(want.astype(np.int32)).max()))
    assert got.dtype == np.int16 and np.abs(want.astype(np.int32)).max() > 1000
    assert d.max() <= 1, (d.max(), np.unravel_index(d.argmax(), d.shape))


# ---- 6. stages ------------------------------------------------------------------------------------------------------------
def _stage_run(T, rx, I, Q):
    got, tap = one_call(rx, I, Q, tap_floats=D)
    assert np.isfinite(got).all() and np.abs(tap).max() > 0
    return got, tap


def test_equaliser_at_24k(T):
    """the equaliser's f32 restatement on the path's own demod tap, x g: bit for bit"""
    import test_receive_eq as E
    kw = dict(mode=0, audioVolume=42)
    nco = siggen.nco_grid(NCH, seed=81)
    I, Q = siggen.make_iq(NCH, 3 * L, nco, mode=0, seed=82, sigma=0.05)
    rx = E.make_rx(NCH, kw, nco)
    rx.set_audio_rate(24000)
    got, tap = _stage_run(T, rx, I, Q)
    want = E.stage24(tap, kw, E.RAMP) * g_of(42)
    assert siggen.block_rel_err(got, tap * g_of(42), D).max() > 0.1  # the stage ran
    assert same(got, want)


def test_cw_filter_at_24k(T):
    """the narrow CW filter's restatement on the demod tap, x g, bit for bit: the filter kernel only filters, the finish
    kernel stores (at 192 kS/s cw_back_kernel interpolates behind it)"""
    import test_cw_receive as W
    for index in (0, 3):
        nco, I, Q = W.keyed_iq(NCH, 3, seed=83 + index)
        rx = W.make_rx(NCH, nco, index=index)
        rx.set_audio_rate(24000)
        got, tap = _stage_run(T, rx, I, Q)
        want = W.model(tap, index)[0] * g_of()
        assert siggen.block_rel_err(got, tap * g_of(), D).max() > 1e-3  # the stage ran
        assert same(got, want), index
        b = rx.state_records()
        assert not b[:, INT1].any() and not b[:, INT2].any()  # power-on: nothing interpolated


@pytest.mark.parametrize("name,kw,tol", [("kim", dict(mode=0, nrOptionSelect=1), 1e-5), ("notch", dict(mode=0, ANR_notchOn=1), 3e-6)])
def test_noise_reduction_and_notch_at_24k(T, name, kw, tol):
    """the oracle's stage (Process.cpp:841-866) on the demod tap, x g, within the stage's own tolerance in isolation
    (tests/test_noise_reduction.py NR_CASES)"""
    nco = siggen.nco_grid(NCH, seed=85)
    I, Q = siggen.make_iq(NCH, 3 * L, nco, mode=0, seed=86)
    got, tap = _stage_run(T, chain(T, kw, nco), I, Q)
    p = O.default_params(**kw)
    want = np.stack([nr_stage(tap[c].copy(), p) for c in range(NCH)]) * g_of()
    e = siggen.block_rel_err(got, want, D)
    print("%s: worst block-relative error %.2e (bound %.0e)" % (name, e.max(), tol))
    assert siggen.block_rel_err(got, tap * g_of(), D).max() > 1e-3  # the stage ran
    assert e.max() <= tol, (e.max(), np.unravel_index(e.argmax(), e.shape))


def test_noise_blanker_at_24k(T):
    """the blanker's f32 restatement on the demod tap, x g, within test_gpu_whole_path_with_nb's 1e-5"""
    import test_noise_blanker as B
    kw = dict(mode=0, **B.WIDE[0])
    nco = siggen.nco_grid(NCH, seed=87)
    I, Q = B.clicky_iq(NCH, 3, 88)
    rx = chain(T, kw, nco)
    rx.set_noise_blanker(1)
    got, tap = _stage_run(T, rx, I, Q)
    a24, st, _ = B.stage24(tap, kw)
    e = siggen.block_rel_err(got, a24 * g_of(), D)
    print("blanker: %d repairs, worst block-relative error %.2e" % (st["repairs"], e.max()))
    assert st["repairs"] > 0 and e.max() <= 1e-5, (st["repairs"], e.max())


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(T):
    from t41_sdr_amd import _lib
    for N in (1024, 4096):
        rx = T.RxChain(3, T.default_params(fft_length=N))
        assert rx.audio_rate == 192000 and rx.audio_frame_len == 4 * N
        refused(lambda: rx.set_audio_rate(24000), ERR_UNSUPPORTED, "long-FFT pipeline")
        assert rx.audio_rate == 192000 and rx._lib.t41rx_get_audio_rate(rx._ctx) == 0
        assert rx._lib.t41rx_audio_frame_len(rx._ctx) == 4 * N
    rx = T.RxChain(3, T.default_params())
    lib = rx._lib
    assert rx.audio_rate == 192000 and lib.t41rx_get_audio_rate(rx._ctx) == 0 and lib.t41rx_audio_frame_len(rx._ctx) == L  # a fresh context
    for bad in (2, -1, 24000):
        assert lib.t41rx_set_audio_rate(rx._ctx, bad) == _lib.ERR_ARG and b"rate" in lib.t41rx_last_error()
        assert lib.t41rx_get_audio_rate(rx._ctx) == 0
    with pytest.raises(ValueError):
        rx.set_audio_rate(48000)
    rx.set_audio_rate(24000)
    assert lib.t41rx_get_audio_rate(rx._ctx) == 1 and lib.t41rx_audio_frame_len(rx._ctx) == D and lib.t41rx_frame_len(rx._ctx) == L
    assert lib.t41rx_set_audio_rate(rx._ctx, 7) == _lib.ERR_ARG and lib.t41rx_get_audio_rate(rx._ctx) == 1  # the rate survives
    with pytest.raises(ValueError):
        rx.set_audio_rate(12000)
    assert rx.audio_rate == 24000
    # configuration: kept across reset, a checkpoint and new parameters
    ck = rx.get_state()
    rx.reset()
    rx.set_state(ck)
    rx.CalcFilters(FHiCut=2400)
    assert rx.audio_rate == 24000 and lib.t41rx_get_audio_rate(rx._ctx) == 1
    # a wrongly shaped output is refused by the Python layer
    import torch
    z = torch.zeros(3, L, device="cuda")
    with pytest.raises(ValueError, match="shape"):
        rx.ProcessIQData(z, z, out=torch.zeros(3, L, device="cuda"))
    assert tuple(rx.ProcessIQData(z, z, out=torch.zeros(3, D, device="cuda")).shape) == (3, D)
    rx.set_audio_rate(192000)
    assert tuple(rx.ProcessIQData(z, z).shape) == (3, L)
