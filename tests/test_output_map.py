"""The output map (t41rx_set_output_map): channel c writes its audio to row map[c] of the n_rows rows of the audio buffer,
or with -1 writes none; everything else keeps its [n_channels] shape and its values.  The reference of every case is the
SAME call on an identical fresh context without an output map: a listened row must equal the reference's row of that
channel, and the checkpoint must equal the reference's except the two interpolator memories (kStInt1, kStInt2) of the
muted channels, which must hold what they held before the call (np.array_equal throughout, no tolerance).
19 channels: one full 16-wave workgroup of the resident forms and a ragged second one, several 4-wave workgroups of the
others, muted and listened channels sharing workgroups.  5 frames take the pipelined AGC / SAM forms, 3 the barrier
forms.  The audio buffer is prefilled with a sentinel, and has a guard behind its n_rows rows.
"""
import ctypes as C
from functools import partial

import numpy as np
import pytest

import group_harness as G
import oracle_lib as O
import siggen
from group_harness import D, L, NCH, NS, USB, check_rows, cw_receive, expected_state, ft8_receive, ft8_results, side_outputs
from group_harness import STREAM_OF as IMAP  # the input map of the cases that name one
from rx_harness import ERR_ARG, ERR_UNSUPPORTED, INT1, INT2, SENT_F32, TOL, T, first, pack, streams  # noqa: F401  (TOL: the bound test_parity_vs_oracle applies; T: a fixture)

pytestmark = pytest.mark.gpu

# the standard map: 10 of 19 muted, the other 9 permuted over 10 rows, row 4 unused; channel 18 (the ragged end) listened
OMAP = np.array([-1, 7, -1, 0, 9, -1, -1, 2, -1, 5, -1, 1, -1, -1, 8, -1, 3, -1, 6], np.int32)
NROWS = 10
UNUSED = 4
LISTENED = np.flatnonzero(OMAP >= 0)
MUTED = np.flatnonzero(OMAP < 0)
assert OMAP.shape == (NCH,) and len(LISTENED) == NROWS - 1 and UNUSED not in OMAP and len(set(OMAP[LISTENED])) == len(LISTENED)
SETOF = np.array([1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 1, 1, 0, 1], np.int32)
SETS = [dict(mode=0, FLoCut=300, FHiCut=1000, audioVolume=45)]  # two pass bands and volumes: set 0 is USB 200..3000 at 30 (45: some hundred q15 steps on the tests' noise; at 18 a q15 row is all zero)


run = partial(G.run, guard=True)  # every call into a sentinel-filled buffer of audio_rows rows with a guard behind it


def chain(T, kw, imap=None, sets=False, **options):
    return G.chain(T, kw, imap=imap, ns=None if imap is None else NS, sets=SETS if sets else None, setof=SETOF, **options)


def check_call(T, kw, nfr, layout="channel", q15=False, rate=192000, imap=None, sets=False, omap=OMAP, nrows=NROWS, setup=None,
               seed=5, warm=2, results=None):
    """`warm` frames without a map on both contexts (the interpolator memories then hold something), then nfr frames with the
    map on one of them: rows, sentinel, every checkpoint section, and whatever `results(rx, keep)` reads for all channels"""
    import torch
    (a, ka), (b, kb) = (chain(T, kw, layout=layout, rate=rate, imap=imap, sets=sets, setup=setup) for _ in range(2))
    I, Q = streams(NS if imap is not None else NCH, (warm + nfr) * L, seed, q15)
    if warm:
        w = slice(0, warm * L)
        assert np.array_equal(run(a, I[:, w], Q[:, w]), run(b, I[:, w], Q[:, w]))
    a.set_output_map(omap, nrows)
    assert a.audio_rows == nrows and np.array_equal(a.output_map, omap) and b.output_map is None and b.audio_rows == NCH
    before = a.get_state()
    assert np.array_equal(before, b.get_state())
    if rate == 192000 and warm:
        rb = a.state_records(before)
        assert rb[:, INT1].any(axis=1).all() and rb[:, INT2].any(axis=1).all()
    s = slice(warm * L, (warm + nfr) * L)
    got, ref = run(a, I[:, s], Q[:, s]), run(b, I[:, s], Q[:, s])
    check_rows(got, ref, omap, nrows)
    sa, sb = a.get_state(), b.get_state()
    assert len(sa) == len(sb) == len(before)
    assert np.array_equal(sa, expected_state(a, sb, before, omap))
    if rate == 192000 and (np.asarray(omap) < 0).any():  # (the reference's memories did move: the muted ones are not equal by accident)
        m = np.flatnonzero(np.asarray(omap) < 0)
        assert not np.array_equal(a.state_records(sb)[m][:, INT1], a.state_records(before)[m][:, INT1])
    if results:
        torch.cuda.synchronize()
        ra, rb = results(a, ka), results(b, kb)
        for x, y in zip(ra, rb):
            assert np.array_equal(x, y) and x.shape[0] == NCH
        assert all(x.any() for x in ra[:1]), "the results are all zero: nothing was compared"
    return a, b


# ---- 1. modes and shapes, 2. state ---------------------------------------------------------------------------------------
LSB = dict(mode=1, FLoCut=-3000, FHiCut=-200)
AM = dict(mode=2, FLoCut=-4000, FHiCut=4000)
SAM = dict(mode=8, FLoCut=-4000, FHiCut=4000)
NFM = dict(mode=3, FLoCut=200, FHiCut=3000)
GENERAL = dict(RFgain=2, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=0.01)
# name, params, frames, layout, q15, rate, input map, parameter sets
CASES = [
    ("usb", USB, 5, "channel", False, 192000, False, False),                 # resident, PLAIN
    ("usb-time", USB, 5, "time", False, 192000, False, False),
    ("usb-q15", USB, 5, "channel", True, 192000, False, False),
    ("usb-q15-time-24k", USB, 5, "time", True, 24000, False, False),         # the A24 twin, q15 stores
    ("lsb-24k", LSB, 5, "channel", False, 24000, False, False),
    ("usb-general", dict(USB, **GENERAL), 5, "time", False, 192000, False, False),
    ("am", AM, 5, "channel", False, 192000, False, False),
    ("am-q15-24k", AM, 5, "time", True, 24000, False, False),
    ("sam-pipe", SAM, 5, "time", False, 192000, False, False),               # PSAM
    ("sam-barrier", SAM, 3, "channel", False, 192000, False, False),
    ("sam-24k", SAM, 5, "channel", False, 24000, False, False),
    ("nfm", NFM, 5, "time", False, 192000, False, False),
    ("nfm-atan", dict(NFM, nfm_demod=1), 5, "channel", False, 192000, False, False),
    ("nfm-atan-24k", dict(NFM, nfm_demod=1), 5, "channel", False, 24000, False, False),
    ("usb-agc-barrier", dict(USB, AGCMode=1), 3, "time", False, 192000, False, False),
    ("usb-agc-pipe", dict(USB, AGCMode=1), 5, "channel", False, 192000, False, False),
    ("usb-agc-pipe-q15", dict(USB, AGCMode=2), 5, "time", True, 192000, False, False),
    ("lsb-agc-24k", dict(LSB, AGCMode=2), 5, "time", False, 24000, False, False),
    ("am-agc", dict(AM, AGCMode=1), 5, "channel", False, 192000, False, False),
    ("sam-agc-pipe", dict(SAM, AGCMode=2), 5, "channel", False, 192000, False, False),  # PSA
    ("sam-agc-barrier", dict(SAM, AGCMode=2), 3, "time", False, 192000, False, False),
    ("nfm-agc", dict(NFM, AGCMode=1), 5, "channel", False, 192000, False, False),
    ("usb-inmap", USB, 5, "channel", False, 192000, True, False),
    ("usb-inmap-time-q15", USB, 5, "time", True, 192000, True, False),
    ("usb-inmap-24k-time", USB, 5, "time", False, 24000, True, False),
    ("usb-agc-inmap", dict(USB, AGCMode=1), 5, "time", False, 192000, True, False),
    ("usb-sets", USB, 5, "channel", False, 192000, False, True),             # the set twin
    ("usb-sets-inmap-time", USB, 5, "time", False, 192000, True, True),
    ("usb-sets-24k-q15", USB, 5, "channel", True, 24000, False, True),
    ("usb-agc-sets", dict(USB, AGCMode=2), 5, "channel", False, 192000, False, True),
]


@pytest.mark.parametrize("name,kw,nfr,layout,q15,rate,imap,sets", CASES, ids=[c[0] for c in CASES])
def test_listened_rows_and_state(T, name, kw, nfr, layout, q15, rate, imap, sets):
    check_call(T, kw, nfr, layout=layout, q15=q15, rate=rate, imap=IMAP if imap else None, sets=sets)


# ---- 3. edge maps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channel", "time"])
def test_identity_map_equals_no_map(T, layout):
    ident = np.arange(NCH, dtype=np.int32)
    a, b = check_call(T, USB, 5, layout=layout, omap=ident, nrows=NCH)
    assert np.array_equal(a.get_state(), b.get_state())


@pytest.mark.parametrize("kw", [USB, dict(USB, AGCMode=1), dict(USB, nrOptionSelect=1)], ids=["usb", "usb-agc", "usb-kim"])
def test_nobody_listens(T, kw):
    """n_rows == 0: the device entry takes a NULL audio pointer, RxChain returns (0, ...); state and demod tap as ever"""
    import torch
    nfr = 5

    def setup(rx):
        tap = torch.zeros(NCH, (2 + nfr) * D, device="cuda")
        rx.set_debug_taps(demod=tap)
        return tap

    mute = np.full(NCH, -1, np.int32)
    a, b = check_call(T, kw, nfr, omap=mute, nrows=0, setup=setup, results=lambda rx, tap: [first(tap, NCH, nfr, D)])
    # the C entry with no audio pointer at all
    I, Q = streams(NCH, 3 * L, 31)
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    before = a.get_state()
    assert a._lib.t41rx_process_device(a._ctx, dI.data_ptr(), dQ.data_ptr(), None, 3, None) == 0
    run(b, I, Q)
    assert np.array_equal(a.get_state(), expected_state(a, b.get_state(), before, mute))
    out = a.ProcessIQData(dI, dQ)
    assert tuple(out.shape) == (0, 3 * L)
    a.set_buffer_layout("time")
    assert tuple(a.ProcessIQData(dI.view(NCH, 3, L).transpose(0, 1).contiguous(), dQ.view(NCH, 3, L).transpose(0, 1).contiguous()).shape) == (3, 0, L)
    # without a map a NULL audio pointer stays the refusal it is
    assert b._lib.t41rx_process_device(b._ctx, dI.data_ptr(), dQ.data_ptr(), None, 3, None) == ERR_ARG


@pytest.mark.parametrize("kw,nfr", [(USB, 5), (dict(USB, AGCMode=1), 5), (dict(USB, AGCMode=1), 3)], ids=["usb", "usb-agc-pipe", "usb-agc-barrier"])
def test_one_listener_at_the_ragged_end(T, kw, nfr):
    m = np.full(NCH, -1, np.int32)
    m[NCH - 1] = 0
    check_call(T, kw, nfr, omap=m, nrows=1)


def test_pure_permutation(T):
    perm = np.random.default_rng(8).permutation(NCH).astype(np.int32)
    assert not np.array_equal(perm, np.arange(NCH))
    a, b = check_call(T, USB, 5, layout="time", omap=perm, nrows=NCH)
    assert np.array_equal(a.get_state(), b.get_state())


# ---- 4. streaming --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [USB, dict(USB, AGCMode=2)], ids=["usb", "usb-agc"])
def test_split_calls_equal_one_call(T, kw):
    (one, _), (two, _) = (chain(T, kw, omap=OMAP, nrows=NROWS) for _ in range(2))
    I, Q = streams(NCH, 5 * L, 41)
    whole = run(one, I, Q)
    parts = np.concatenate([run(two, I[:, :2 * L], Q[:, :2 * L]), run(two, I[:, 2 * L:], Q[:, 2 * L:])], axis=1)
    assert np.array_equal(whole, parts)
    assert np.array_equal(one.get_state(), two.get_state())


def test_map_change_takes_effect_from_the_next_call(T):
    other = np.where(OMAP >= 0, -1, 0).astype(np.int32)
    other[MUTED] = np.arange(len(MUTED), dtype=np.int32)  # the muted become the listened
    (a, _), (b, _) = chain(T, USB), chain(T, USB)
    I, Q = streams(NCH, 6 * L, 42)
    for k, (m, n) in enumerate(((OMAP, NROWS), (other, len(MUTED)), (None, NCH), (OMAP, NROWS))):
        a.set_output_map(m, n if m is not None else None)
        assert a.audio_rows == n
        sl = slice(k * L, (k + 1) * L)
        got, ref = run(a, I[:, sl], Q[:, sl]), run(b, I[:, sl], Q[:, sl])
        check_rows(got, ref, np.arange(NCH) if m is None else m, n)
        b.set_state(a.get_state())  # the reference's interpolators go on from what the mapped context's hold


@pytest.mark.parametrize("kw", [USB, dict(USB, AGCMode=1)], ids=["usb", "usb-agc"])
def test_muted_then_listened_continues_from_the_old_interpolator_memories(T, kw):
    """a channel muted for one call and listened to in the next: the audio of a context that has the current state with
    the interpolator memories of the state before the muted call"""
    (a, _), (b, _) = chain(T, kw), chain(T, kw)
    I, Q = streams(NCH, 7 * L, 43)
    s0, s1, s2 = slice(0, 2 * L), slice(2 * L, 5 * L), slice(5 * L, 7 * L)
    run(a, I[:, s0], Q[:, s0])
    run(b, I[:, s0], Q[:, s0])
    a.set_output_map(OMAP, NROWS)
    before = a.get_state()
    run(a, I[:, s1], Q[:, s1])
    run(b, I[:, s1], Q[:, s1])
    b.set_state(expected_state(b, b.get_state(), before, OMAP))
    assert np.array_equal(a.get_state(), b.get_state())
    everyone = np.arange(NCH, dtype=np.int32)[::-1].copy()
    a.set_output_map(everyone)
    got, ref = run(a, I[:, s2], Q[:, s2]), run(b, I[:, s2], Q[:, s2])
    check_rows(got, ref, everyone, NCH)
    assert np.array_equal(a.get_state(), b.get_state())


def test_map_survives_reset_checkpoint_and_set_params(T):
    (a, _), (b, _) = chain(T, USB), chain(T, USB)
    I, Q = streams(NCH, 8 * L, 44)

    def step(k):
        sl = slice(2 * k * L, 2 * (k + 1) * L)
        before = a.get_state()
        assert np.array_equal(before, b.get_state())
        check_rows(run(a, I[:, sl], Q[:, sl]), run(b, I[:, sl], Q[:, sl]), OMAP, NROWS)
        n = C.c_int(-1)
        assert a._lib.t41rx_get_output_map(a._ctx, None, 0, C.byref(n)) == 1 and n.value == NROWS == a._lib.t41rx_audio_rows(a._ctx)
        assert np.array_equal(a.output_map, OMAP)
        b.set_state(a.get_state())

    a.set_output_map(OMAP, NROWS)
    step(0)
    assert a._lib.t41rx_state_bytes(a._ctx) == b._lib.t41rx_state_bytes(b._ctx)  # the map has no state
    a.reset()
    b.reset()
    step(1)
    a.set_state(a.get_state())
    step(2)
    a.CalcFilters(FHiCut=2400, audioVolume=40)
    b.CalcFilters(FHiCut=2400, audioVolume=40)
    a.set_coeffs(a.coeffs())
    step(3)


def test_checkpoint_with_a_map_restores_without_one(T):
    kw = dict(USB, AGCMode=1)
    (a, _), (b, _) = chain(T, kw, omap=OMAP, nrows=NROWS), chain(T, kw)
    I, Q = streams(NCH, 7 * L, 45)
    run(a, I[:, :3 * L], Q[:, :3 * L])
    b.set_state(a.get_state())
    assert b.output_map is None and b.audio_rows == NCH
    before = a.get_state()
    got, ref = run(a, I[:, 3 * L:], Q[:, 3 * L:]), run(b, I[:, 3 * L:], Q[:, 3 * L:])
    check_rows(got, ref, OMAP, NROWS)
    assert np.array_equal(a.get_state(), expected_state(a, b.get_state(), before, OMAP))


# ---- 5. behind the split -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [192000, 24000], ids=["192k", "24k"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_side_outputs_and_the_demod_tap(T, q15, rate):
    """audio spectrum, display spectrum and the demod tap: the tap kernels hand over, launch_back512's twin (or the 24 kS/s
    finish) stores"""
    nfr = 5

    def results(rx, keep):
        spect, mx, spec, _, dem = keep
        return [first(spect, NCH, nfr, 1024), first(mx, NCH, nfr, 3), first(spec, NCH, nfr, 512), first(dem, NCH, nfr, D)]

    check_call(T, dict(USB, AGCMode=1), nfr, q15=q15, rate=rate, layout="time" if q15 else "channel",
               setup=partial(side_outputs, nfr=2 + nfr, taps=("demod",)), results=results)  # (room for the 2 warm-up frames too)


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("side", ["spectrum", "ft8"])
def test_parameter_sets_behind_the_hand_over(T, side, q15):
    """parameter sets (set 1: another pass band and audioVolume) with a side output at 192 kS/s: the tap kernel hands over
    and launch_back512's twin interpolates with the taps of the channel's own set, which carry its volume"""
    import torch
    nfr = 16 if side == "ft8" else 5

    def setup(rx):
        if side == "ft8":
            return ft8_receive(rx, nfr)
        spect, mx = torch.zeros(NCH, 7, 1024, device="cuda"), torch.zeros(NCH, 7, 3, device="cuda")
        rx.set_audio_spectrum(spect, mx)
        return spect, mx

    def results(rx, keep):
        if side == "ft8":
            return ft8_results(rx, nfr)
        return [first(keep[0], NCH, nfr, 1024), first(keep[1], NCH, nfr, 3)]

    a, b = check_call(T, USB, nfr, warm=0 if side == "ft8" else 2, q15=q15, layout="time" if q15 else "channel", sets=True,
                      setup=setup, results=results)
    # (the sets' volumes differ: rows of set 1 stored with set 0's taps would not pass)
    assert set(SETOF[LISTENED]) == {0, 1}
    check_call(T, dict(USB, AGCMode=1), nfr, warm=0 if side == "ft8" else 2, q15=q15, imap=IMAP, sets=True, setup=setup, results=results)


def test_receive_equaliser(T):
    import test_receive_eq as E

    def setup(rx):
        rx.set_receive_eq_bands(E.M.bands())
        rx.set_receive_eq(1, E.RAMP)

    check_call(T, USB, 5, setup=setup)
    check_call(T, USB, 3, layout="time", q15=True, rate=24000, setup=setup)


@pytest.mark.parametrize("name,kw,nb", [("kim", dict(USB, nrOptionSelect=1), 0), ("blanker", USB, 1), ("notch-blanker", dict(USB, ANR_notchOn=1), 1)],
                         ids=["kim", "blanker", "notch-blanker"])
def test_noise_reduction_and_blanker(T, name, kw, nb):
    setup = (lambda rx: rx.set_noise_blanker(1)) if nb else None
    check_call(T, kw, 5, setup=setup)
    check_call(T, kw, 3, layout="time", q15=True, setup=setup)


@pytest.mark.parametrize("rate", [192000, 24000], ids=["cw-back", "cw-24k"])
@pytest.mark.parametrize("index", [3, 5], ids=["filter", "no-filter"])
def test_cw_filter_detector_and_decoder(T, rate, index):
    """the narrow filter runs for every channel; cw_back_kernel's twin (192 kS/s) or the finish (24 kS/s) stores the listened
    rows; with CWFilterIndex 5 the detector alone splits the chain and launch_back512's twin stores"""
    nfr = 6
    setup = partial(cw_receive, nfr=nfr, index=index)

    def results(rx, keep):
        return [keep[0].cpu().numpy(), rx.cw_text(nfr).cpu().numpy()[:, :, 1:]]  # (the character word is 0 in most frames)

    check_call(T, dict(USB, xmtMode=1), nfr, rate=rate, setup=setup, results=results)
    if index == 3:
        check_call(T, dict(USB, xmtMode=1), nfr, rate=rate, layout="time", q15=True, setup=setup, results=results)


@pytest.mark.parametrize("rate", [192000, 24000], ids=["192k", "24k"])
def test_ft8_receive(T, rate):
    nfr = 16

    def results(rx, keep):
        st, power = ft8_results(rx, nfr)
        assert (st[:, -1, 0] == 1).all()  # FT_8_counter: the 15 frames' two FFTs ran in the call
        return [st, power]

    a, b = check_call(T, USB, nfr, warm=0, rate=rate, setup=partial(ft8_receive, nfr=nfr), results=results)
    assert np.array_equal(a.ft8_state(), b.ft8_state())


def test_panadapter_with_the_beacon_monitor(T):
    nfr = 9

    def setup(rx):
        bufs = G.panadapter(rx, nfr, spectrumZoom=1, currentScale=1, update_period=3)
        rx.set_beacon_clock(0, 32, 3)
        snr, ev = rx.set_beacon(True, 1, (np.arange(NCH) * 3 + 1) % 5)
        return bufs, ev

    def results(rx, keep):
        bufs, ev = keep
        rows = 3  # update frames of the 9-frame call
        out = [bufs[n].cpu().numpy()[:, :rows] for n, _, _ in rx.PANADAPTER_ROWS]
        return out + [ev.cpu().numpy()[:, :rows, 1:], rx.beacon_status()]

    a, b = check_call(T, dict(USB, **GENERAL), nfr, warm=0, setup=setup, results=results)
    assert np.array_equal(a.beacon_snr(), b.beacon_snr()) and np.array_equal(a.beacon_state(), b.beacon_state())


# ---- 6. host forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", [NROWS, 0], ids=["standard", "nobody"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("layout", ["channel", "time"])
def test_host_forms_equal_device_forms(T, layout, q15, nrows):
    omap = OMAP if nrows else np.full(NCH, -1, np.int32)
    (a, _), (b, _) = (chain(T, USB, layout=layout, omap=omap, nrows=nrows) for _ in range(2))
    I, Q = streams(NCH, 5 * L, 61, q15)
    dev, host = run(a, I, Q), run(b, I, Q, host=True)
    assert host.dtype == (np.int16 if q15 else np.float32) and host.shape == (nrows, 5 * L) and np.array_equal(dev, host)
    assert np.array_equal(a.get_state(), b.get_state())
    if nrows == 0:  # the C entries take no audio pointer then
        h = pack(I, Q, layout, None, L)
        entry = b._lib.t41rx_process_host_q15 if q15 else b._lib.t41rx_process_host
        p = (lambda v: v.ctypes.data_as(C.c_void_p)) if q15 else (lambda v: v.ctypes.data_as(C.POINTER(C.c_float)))
        assert entry(b._ctx, p(h[0]), p(h[1]), None, 5) == 0


# ---- 7. against the oracle directly --------------------------------------------------------------------------------------
def test_mapped_call_against_the_oracle(T):
    """USB, default parameters: each listened row against oracle_lib run on its channel, within the bound
    test_parity_vs_oracle applies"""
    nfr = 6
    nco = siggen.nco_grid(NCH, seed=3)
    I, Q = siggen.make_iq(NCH, nfr * L, nco, mode=0, seed=21)
    got = run(chain(T, {}, nco=nco, omap=OMAP, nrows=NROWS)[0], I, Q)
    ref = O.OracleBatch(O.default_params(), nco).process(I, Q)
    assert np.isfinite(got[OMAP[LISTENED]]).all() and (got[UNUSED] == SENT_F32).all()
    err = siggen.block_rel_err(got[OMAP[LISTENED]], ref[LISTENED], L)
    print("worst block-relative error %.3e (bound %.0e)" % (err.max(), TOL))
    assert err.max() <= TOL, "worst block-relative error %.3e at %s" % (err.max(), np.unravel_index(err.argmax(), err.shape))


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_map(T):
    import torch
    (a, _), (b, _) = chain(T, USB, omap=OMAP, nrows=NROWS), chain(T, USB)
    lib = a._lib
    I, Q = streams(NCH, 2 * L, 71)
    ip = lambda m: np.ascontiguousarray(m, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    at = lambda i, v: np.where(np.arange(NCH) == i, v, OMAP)  # noqa: E731
    k = [0]

    def still_works():
        assert lib.t41rx_audio_rows(a._ctx) == NROWS and np.array_equal(a.output_map, OMAP)
        check_rows(run(a, I, Q), run(b, I, Q), OMAP, NROWS)
        b.set_state(a.get_state())
        k[0] += 1

    bad = [
        ("n != n_channels", "n (18)", lambda: lib.t41rx_set_output_map(a._ctx, ip(OMAP[:-1]), NCH - 1, NROWS)),
        ("n != n_channels", "n (20)", lambda: lib.t41rx_set_output_map(a._ctx, ip(np.append(OMAP, -1)), NCH + 1, NROWS)),
        ("entry -2", "channel 7 names row -2", lambda: lib.t41rx_set_output_map(a._ctx, ip(at(7, -2)), NCH, NROWS)),
        ("entry n_rows", "channel 18 names row 10", lambda: lib.t41rx_set_output_map(a._ctx, ip(at(18, NROWS)), NCH, NROWS)),
        ("a row named twice", "channel 5 names row 7, which channel 1 names already", lambda: lib.t41rx_set_output_map(a._ctx, ip(at(5, 7)), NCH, NROWS)),
        ("n_rows above n_channels", "n_rows 20", lambda: lib.t41rx_set_output_map(a._ctx, ip(OMAP), NCH, NCH + 1)),
        ("negative n_rows", "n_rows -1", lambda: lib.t41rx_set_output_map(a._ctx, ip(OMAP), NCH, -1)),
        ("null map with n_rows", "null map", lambda: lib.t41rx_set_output_map(a._ctx, None, 0, 2)),
        ("null context", "null", lambda: lib.t41rx_set_output_map(None, ip(OMAP), NCH, NROWS)),
        ("null context", "null", lambda: lib.t41rx_get_output_map(None, None, 0, None)),
        ("wrong n in the getter", "n (3)", lambda: lib.t41rx_get_output_map(a._ctx, ip(np.zeros(3)), 3, None)),
    ]
    still_works()
    for what, text, call in bad:
        assert call() == ERR_ARG, what
        assert text in lib.t41rx_last_error().decode(), (what, lib.t41rx_last_error())
        still_works()
    # Python: the wrapper raises what the C side refuses, and checks out= against the rows
    with pytest.raises(T.T41RxError):
        a.set_output_map(at(5, 7), NROWS)
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    with pytest.raises(ValueError, match="audio_rows=%d" % NROWS):
        a.ProcessIQData(dI, dQ, out=torch.empty_like(dI))  # out= of the input's shape instead of the output's
    with pytest.raises(ValueError, match="audio_rows=%d" % NROWS):
        a.ProcessIQData(I, Q, out=np.empty_like(I))
    still_works()
    # off again: one row per channel
    a.set_output_map(None)
    n = C.c_int(-1)
    assert a.output_map is None and lib.t41rx_get_output_map(a._ctx, None, 0, C.byref(n)) == 0 and n.value == NCH == a.audio_rows
    assert np.array_equal(run(a, I, Q), run(b, I, Q))


@pytest.mark.parametrize("fft_length", [1024, 4096])
def test_long_fft_lengths_refuse_in_both_orders(T, fft_length):
    # a long context, then the map
    rx = T.RxChain(NCH, T.default_params(fft_length=fft_length, FLoCut=400, FHiCut=600))
    with pytest.raises(T.T41RxError) as e:
        rx.set_output_map(OMAP, NROWS)
    assert e.value.status == ERR_UNSUPPORTED and "fft_length 512" in str(e.value)
    assert rx.output_map is None and rx.audio_rows == NCH
    rx.set_output_map(None)  # off is off at any length
    # the map, then a long length: fft_length does not change on a live context, and the map stays
    rx = T.RxChain(NCH, T.default_params(**USB))
    rx.set_output_map(OMAP, NROWS)
    with pytest.raises(T.T41RxError):
        rx.CalcFilters(fft_length=fft_length)
    assert np.array_equal(rx.output_map, OMAP) and rx.audio_rows == NROWS and rx.params.fft_length == 512
