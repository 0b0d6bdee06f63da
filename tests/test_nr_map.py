"""The noise-reduction map (t41rx_set_nr_map): while a map is loaded channel c is processed exactly as the same channel of a
context without a map whose parameters carry nrOptionSelect = nr_of_channel[c] and ANR_notchOn = notch_of_channel[c]; a
function runs where the entry asks for it and the stage map's STAGE_NR bit is set or no stage map is loaded; a channel with
0 / 0 keeps its audio and both records.

Every comparison is bit for bit against contexts WITHOUT a map (nr_map_harness.run_schedule): one reference context per
history of (kind, notch), driven with CalcFilters(nrOptionSelect=, ANR_notchOn=) call by call, so the stale statics of a
kind that changes across a call boundary are the library's own.  19 channels (the group harness's ragged NCH), 70 where
the Xanr() list's workgroups matter; 3 frames per call, 3 calls per stream.
"""
import ctypes as C

import numpy as np
import pytest

import group_harness as G
import nr_map_harness as N
import siggen
from group_harness import NCH, STREAM_OF
from nr_map_harness import L, pairs, run_schedule
from rx_harness import ERR_ARG, ERR_UNSUPPORTED, T, one_call, refused, same, streams  # noqa: F401  (T: a fixture)
from stage_map_harness import ALL, NR, sections

pytestmark = pytest.mark.gpu

EIGHT = np.array([(5 * c + 3) % 8 for c in range(NCH)], np.int32)  # 3 0 5 2 7 4 1 6 3 ..: neighbours differ
assert all((EIGHT == k).sum() >= 2 for k in range(8))


# ---- 1. all eight combinations in one context ------------------------------------------------------------------------------
def test_all_eight_combinations_in_one_context(T):
    """every (kind, notch) on two and more channels, and the assignment reversed in the third call: every channel changes
    its pair across a call boundary, most across both (spectral -> Kim starts from the stale NR_X / NR_E, LMS and notch
    share one record)"""
    a, eff, _ = run_schedule(T, [None, EIGHT, EIGHT[::-1].copy()], 3)
    assert set(eff[1]) == set(range(8)) and set(eff[2]) == set(range(8))
    assert ((eff[0] != eff[1]) | (eff[1] != eff[2])).all() and (eff[1] != eff[2]).sum() >= 12
    assert len({tuple(eff[:, c]) for c in range(NCH)}) >= 8


# ---- 2. the Xanr() list's workgroups ---------------------------------------------------------------------------------------
def test_classes_of_1_16_and_17_channels(T):
    """70 channels: Xanr() classes of 1, 16 and 17 channels -- four workgroups, then, with the classes turned, three --
    among Kim and spectral channels on interleaved channels; a short workgroup's dead lanes shadow its own class's last
    channel"""
    nch = 70
    codes = np.array([1 if c % 4 == 1 else 2 if c % 4 == 3 else 0 for c in range(nch)], np.int32)  # Kim, spectral, and 35 free
    free = np.flatnonzero(codes == 0)
    assert free.size == 35
    m1, m2 = codes.copy(), codes.copy()
    # LMS only (3): 1 channel; notch only (4): 16; both (7): 17 -- 1 + 1 + 2 = 4 workgroups, the last with one live column
    m1[free[17]] = 3
    m1[free[:16]] = 4
    m1[free[18:35]] = 7
    assert [(m1 == k).sum() for k in (3, 4, 7)] == [1, 16, 17] and (m1 == 0).sum() == 1
    # turned: LMS only 16, notch only 1 on a spectral channel (2, 1), both 16: three workgroups; LMS and notch swap records' roles
    m2[free[:16]] = 3
    m2[free[16:32]] = 7
    m2[3] = 6
    assert [(m2 == k).sum() for k in (3, 6, 7)] == [16, 1, 16]
    run_schedule(T, [None, m1, m2], 3, nch=nch, seed=8)


# ---- 3. one class only, and the empty map -------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", [1, 2, 3, 4, 7])
def test_one_class_only(T, code):
    """every channel the same pair: one list is empty and is not launched (a grid of zero blocks would be a launch error)"""
    run_schedule(T, [None, np.full(NCH, code, np.int32), np.full(NCH, code, np.int32)], 3)


def test_the_empty_map(T):
    """the all-zero map: the audio of a context with noise reduction off, both records untouched (the engine holds both),
    and on a fresh context no noise-reduction section appears -- the call does not allocate what only a call with noise
    reduction on allocates, and ends as the plain context's does"""
    zero = np.zeros(NCH, np.int32)
    run_schedule(T, [None, zero, zero, None], 3)
    a, _ = G.chain(T, dict(G.USB, nrOptionSelect=2, ANR_notchOn=1))
    b, _ = G.chain(T, G.USB)
    a.set_nr_map(zero, zero)
    I, Q = streams(NCH, 3 * L, 4)
    assert same(one_call(a, I, Q)[0], one_call(b, I, Q)[0])
    sa, sb = sections(a), sections(b)
    assert "nr" not in sa and set(sa) == set(sb) and np.array_equal(sa["path"], sb["path"])
    assert a._lib.t41rx_state_bytes(a._ctx) == b._lib.t41rx_state_bytes(b._ctx)


# ---- 4. composition with the other maps ------------------------------------------------------------------------------------------
OMAP = np.array([-1, 7, -1, 0, 9, -1, -1, 2, -1, 5, -1, 1, -1, -1, 8, -1, 3, -1, 6], np.int32)  # tests/test_output_map.py's
STAGES = np.full(NCH, ALL, np.uint32)
STAGES[1:9] &= ~np.uint32(NR)  # clear on one channel of each of the eight combinations: seven non-zero entries and one 0 / 0
VARIANTS = {
    "stage-map": dict(stages=[None, STAGES, STAGES[::-1].copy()]),
    "output-map": dict(omap=OMAP, nrows=10),
    "input-map": dict(imap=STREAM_OF),
    "24k": dict(rate=24000),
    "time-major": dict(layout="time"),
    "q15": dict(q15=True),
    "host": dict(host=True),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_composition(T, variant):
    """none of the other maps, rates, layouts, formats and entries sees the map; the stage map's bit gates every function"""
    a, eff, _ = run_schedule(T, [None, EIGHT, EIGHT[::-1].copy()], 3, **VARIANTS[variant])
    if variant == "stage-map":
        cleared = np.flatnonzero((STAGES & NR) == 0)
        assert (EIGHT[cleared] != 0).sum() >= 5 and (eff[1][cleared] == 0).all() and set(eff[1]) == set(range(8))


def test_stage_map_set_after_the_nr_map(T):
    """the lists follow the stage map whichever of the two is set last, and its removal"""
    a, b = N.context(T, NCH), N.context(T, NCH)
    kind, notch = pairs(EIGHT)
    a.set_nr_map(kind, notch)
    a.set_stage_map(STAGES)  # behind the map
    b.set_stage_map(STAGES)
    b.set_nr_map(kind, notch)
    I, Q = streams(NCH, 6 * L, 6)
    assert same(one_call(a, I[:, :3 * L], Q[:, :3 * L])[0], one_call(b, I[:, :3 * L], Q[:, :3 * L])[0])
    assert np.array_equal(a.get_state(), b.get_state())
    off = np.flatnonzero((STAGES & NR) == 0)
    a.set_stage_map(None)  # every entry runs again
    b.set_stage_map(None)
    before = sections(a)["nr"]
    assert same(one_call(a, I[:, 3 * L:], Q[:, 3 * L:])[0], one_call(b, I[:, 3 * L:], Q[:, 3 * L:])[0])
    moved = np.any(sections(a)["nr"] != before, axis=1)
    assert moved[off][EIGHT[off] != 0].all() and np.array_equal(moved, EIGHT != 0)


# ---- 5. checkpoint ------------------------------------------------------------------------------------------------------------
def test_checkpoint_continues_identically(T):
    run_schedule(T, [None, EIGHT, EIGHT, EIGHT[::-1].copy()], 3, checkpoint_after=1, seed=24)


# ---- 6. reset and removal -----------------------------------------------------------------------------------------------------
def test_map_survives_reset_and_removal_returns_to_the_contexts_values(T):
    a, b = N.context(T, NCH), N.context(T, NCH)  # b: never a map, the context-wide BASE
    kind, notch = pairs(EIGHT)
    a.set_nr_map(kind, notch)
    nbytes = a._lib.t41rx_state_bytes(a._ctx)
    I, Q = streams(NCH, 6 * L, 5)
    first = one_call(a, I[:, :3 * L], Q[:, :3 * L])[0]
    a.reset()
    assert np.array_equal(a.nr_map[0], kind) and np.array_equal(a.nr_map[1], notch), "the map is configuration: t41rx_reset() keeps it"
    assert same(first, one_call(a, I[:, :3 * L], Q[:, :3 * L])[0]), "reset: every channel's records at power-on"
    a.set_state(a.get_state())
    a.CalcFilters(FHiCut=2500)
    assert np.array_equal(a.nr_map[0], kind)
    a.CalcFilters(FHiCut=G.USB["FHiCut"])
    # removal: from power-on the context without a map and the one that had one are the same context again
    a.set_nr_map(None)
    a.reset()
    for k in range(2):
        sl = slice(3 * k * L, 3 * (k + 1) * L)
        assert same(one_call(a, I[:, sl], Q[:, sl])[0], one_call(b, I[:, sl], Q[:, sl])[0])
    assert np.array_equal(a.get_state(), b.get_state())
    assert a._lib.t41rx_state_bytes(a._ctx) == b._lib.t41rx_state_bytes(b._ctx) >= nbytes  # the map has no state


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------
NARROW = dict(mode=0, FLoCut=200, FHiCut=1000)  # VAD_high 10 < 17: the spectral function indexes outside its arrays
LSB_SET = dict(mode=1, FLoCut=-3000, FHiCut=-200)


def holds(rx, kind, notch):
    got = rx.nr_map
    return got is not None and np.array_equal(got[0], kind) and np.array_equal(got[1], notch)


def test_refusals_of_the_setter(T):
    rx, _ = G.chain(T, G.USB)
    kind, notch = pairs(EIGHT)
    rx.set_nr_map(kind, notch)
    i32p = C.POINTER(C.c_int32)
    kp, tp = kind.ctypes.data_as(i32p), notch.ctypes.data_as(i32p)
    refused(lambda: rx.set_nr_map(kind[:-1], notch[:-1]), ERR_ARG, "n (18) must equal n_channels", "n_channels 19")
    refused(lambda: rx.set_nr_map(np.append(kind, 0).astype(np.int32), np.append(notch, 0).astype(np.int32)), ERR_ARG, "n (20) must equal n_channels")
    for args, word in (((kp, None, NCH), b"notch_of_channel is null"), ((None, tp, NCH), b"nr_of_channel is null"), ((None, None, NCH), b"take n 0")):
        assert rx._lib.t41rx_set_nr_map(rx._ctx, *args) == ERR_ARG and word in rx._lib.t41rx_last_error(), args
    for value in (4, -1):
        bad = kind.copy()
        bad[5] = value
        refused(lambda: rx.set_nr_map(bad, notch), ERR_ARG, "channel 5", "nrOptionSelect %d" % value)
    for value in (2, -1):
        bad = notch.copy()
        bad[18] = value
        refused(lambda: rx.set_nr_map(kind, bad), ERR_ARG, "channel 18", "ANR_notchOn %d" % value)
    assert holds(rx, kind, notch), "a refused map must leave the previous one whole"
    # a long fft_length
    long_rx = T.RxChain(4, T.default_params(fft_length=1024), NCOFreq=siggen.nco_grid(4))
    z4 = np.zeros(4, np.int32)
    refused(lambda: long_rx.set_nr_map(z4, z4), ERR_UNSUPPORTED, "fft_length 512")
    long_rx.set_nr_map(None)  # (removing what is not there is no refusal)
    assert long_rx.nr_map is None


def test_the_spectral_functions_pass_band(T):
    """an entry 2 needs a pass band the spectral function accepts: params_valid()'s error and text, at the setter and at
    t41rx_set_params / CalcFilters() while such a map is loaded"""
    text = "nrOptionSelect = 2: the reference indexes outside its arrays for this pass band"
    narrow, _ = G.chain(T, NARROW)
    refused(lambda: narrow.CalcFilters(nrOptionSelect=2), ERR_ARG, text)  # the context-wide refusal whose text is borrowed
    narrow.CalcFilters(nrOptionSelect=1)  # (and the band is good for the other kinds)
    narrow.CalcFilters(nrOptionSelect=0)
    kind, notch = pairs(EIGHT)
    refused(lambda: narrow.set_nr_map(kind, notch), ERR_ARG, text)
    assert narrow.nr_map is None
    no2 = np.where(kind == 2, 1, kind).astype(np.int32)
    narrow.set_nr_map(no2, notch)  # without an entry 2 the band does not matter
    refused(lambda: narrow.set_nr_map(kind, notch), ERR_ARG, text)
    assert holds(narrow, no2, notch)
    # the other order: the map first, then the band
    wide, _ = G.chain(T, G.USB)
    wide.set_nr_map(kind, notch)
    refused(lambda: wide.CalcFilters(FHiCut=1000), ERR_ARG, text)
    p = T.default_params()
    assert wide._lib.t41rx_get_params(wide._ctx, C.byref(p)) == 0 and p.FHiCut == G.USB["FHiCut"] and wide.params.FHiCut == G.USB["FHiCut"]
    assert holds(wide, kind, notch)
    wide.set_nr_map(no2, notch)
    wide.CalcFilters(FHiCut=1000)  # accepted without an entry 2 -- and by a context without a map
    plain, _ = G.chain(T, G.USB)
    plain.CalcFilters(FHiCut=1000)
    # fft_length cannot change on a live context, map or not
    refused(lambda: wide.CalcFilters(fft_length=1024), ERR_ARG, "fft_length")
    assert wide.params.fft_length == 512


def test_nr_map_and_parameter_sets_refuse_each_other_in_both_orders(T):
    words = ("the noise reduction / notch", "splits the fused chain", "t41rx_set_param_sets")
    setof = (np.arange(NCH) % 2).astype(np.int32)
    kind, notch = pairs(EIGHT)
    zero = np.zeros(NCH, np.int32)
    # sets first: a map with a non-zero entry is refused in the stages' words, an all-zero map is accepted
    a, _ = G.chain(T, G.USB)
    a.set_param_sets([LSB_SET], setof)
    refused(lambda: a.set_nr_map(kind, notch), ERR_UNSUPPORTED, *words)
    assert a.nr_map is None
    a.set_nr_map(zero, zero)
    refused(lambda: a.set_nr_map(zero, np.eye(1, NCH, 7, dtype=np.int32)[0]), ERR_UNSUPPORTED, *words)
    assert holds(a, zero, zero) and len(a.param_sets) == 1
    # the map first: the sets are refused, naming the stage; with an all-zero map, or the map removed, they load
    b, _ = G.chain(T, G.USB)
    b.set_nr_map(kind, notch)
    refused(lambda: b.set_param_sets([LSB_SET], setof), ERR_UNSUPPORTED, *words)
    assert b.param_sets == [] and holds(b, kind, notch)
    b.set_nr_map(zero, zero)
    b.set_param_sets([LSB_SET], setof)
    b.set_param_sets(None)
    b.set_nr_map(kind, notch)
    b.set_nr_map(None)
    b.set_param_sets([LSB_SET], setof)
    assert len(b.param_sets) == 1


def test_the_cw_detectors_one_stream_rule_per_channel(T):
    """the detector refuses Kim or LMS without the notch (or the blanker) behind it: with a map per channel, with the
    channel's own two values, and the text names the first channel that trips it"""
    import cw_model as CWM
    kw = dict(G.USB, xmtMode=1)
    I, Q = streams(NCH, 3 * L, 7)

    def chain(**extra):
        rx, _ = G.chain(T, dict(kw, **extra))
        rx.set_cw_tables(*CWM.tables())
        rx._det = rx.set_cw_detector(1, 3)
        return rx

    # without a map nothing changes: Kim context-wide trips it, the text names no channel
    refused(lambda: one_call(chain(nrOptionSelect=1), I, Q), ERR_UNSUPPORTED, "CW detector: the Kim noise reduction (nrOptionSelect 1) leaves")
    rx = chain(nrOptionSelect=1)  # the context's own value is not consulted under a map
    kind = np.array([0, 2, 2, 0, 1, 3, 0, 2, 1, 3, 0, 0, 2, 2, 0, 0, 3, 1, 0], np.int32)
    notch = (kind % 2).astype(np.int32)  # Kim and LMS with the notch behind them: nobody trips the rule
    rx.set_nr_map(kind, notch)
    one_call(rx, I, Q)
    bad = notch.copy()
    bad[[9, 17]] = 0  # LMS on channel 9 and Kim on channel 17 without the notch
    rx.set_nr_map(kind, bad)
    before = rx.get_state()
    refused(lambda: one_call(rx, I, Q), ERR_UNSUPPORTED, "CW detector: the LMS noise reduction (nrOptionSelect 3) of channel 9", "noise-reduction map")
    assert np.array_equal(rx.get_state(), before) and holds(rx, kind, bad)
    rx.set_noise_blanker(1)  # the blanker joins the two streams again, for every channel
    one_call(rx, I, Q)
    rx.set_noise_blanker(0)
    rx.set_nr_map(None)  # back to the context's own Kim
    refused(lambda: one_call(rx, I, Q), ERR_UNSUPPORTED, "CW detector: the Kim noise reduction (nrOptionSelect 1) leaves")
