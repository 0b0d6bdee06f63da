"""Parameter sets next to the chain-splitting stages (t41rx_set_param_sets_ex with T41RX_SETS_STAGES;
RxChain.set_param_sets(..., stages=True)): channel c must be processed exactly as the same channel of a context created
with sets[set_of_channel[c]] and carrying the same stage switches and maps.  So the reference of set k is a PLAIN context of
the same channel count created with set k's parameters and given the same switches, maps, NCOFreq, inputs and sequence of
calls; for the channels with set_of_channel == k the audio rows, the detector's and the decoder's rows and every section of
the checkpoint must be equal bit for bit, and no audio row is all zero.  group_harness's geometry: 19 channels (ragged
against the 16- and 4-wave workgroups, anr_map_kernel's 1 .. 16 columns and the CW filter's groups of eight), 3 sets in the
non-monotone table SET_OF, 5 or 6 frames.
"""
import ctypes as C
from functools import partial

import numpy as np
import pytest

import siggen
from group_harness import L, NCH, NS, USB, chain, cw_receive, run
from group_harness import SET_OF as SETOF, STREAM_OF as MAP
from rx_harness import ERR_ARG, ERR_UNSUPPORTED, T, bits, first, refused, streams  # noqa: F401  (T: a fixture)
from stage_map_harness import DEC, DET, EQ, NB, NR, sections, sw_eq

pytestmark = pytest.mark.gpu

SSB3 = [dict(mode=1, FLoCut=-3000, FHiCut=-200), dict(mode=0, FLoCut=300, FHiCut=1000)]  # + LSB + a narrow USB
CW = dict(USB, xmtMode=1)
# the narrow CW filter: pass bands and volumes differ, so the volume factor and the two interpolators' taps are per set
CW3 = [dict(FLoCut=300, FHiCut=1200, audioVolume=45), dict(mode=1, FLoCut=-2400, FHiCut=-200, audioVolume=20)]
# noise reduction, a kind per set: Kim on set 0, the spectral function on set 1, LMS with the notch on set 2; NR_alpha /
# NR_beta / NR_PSI differ, and so do the VAD ranges of the pass bands -- bins [2, 32), [3, 25) and [1, 29) of 93.75 Hz --
# all of which pass the spectral function's check (VAD_high >= 17, VAD_low + 11 <= 127: design.cpp)
NR_BASE = dict(USB, nrOptionSelect=1, NR_alpha=0.95, NR_beta=0.85, NR_PSI=0.0)
NR3 = [dict(FLoCut=300, FHiCut=2400, nrOptionSelect=2, NR_alpha=0.9, NR_beta=0.8, NR_PSI=15.0),
       dict(mode=1, FLoCut=-2800, FHiCut=-100, nrOptionSelect=3, ANR_notchOn=1, NR_alpha=0.85, NR_beta=0.9, NR_PSI=5.0)]
MUTE = np.where(np.arange(NCH) % 4 == 1, -1, 0).astype(np.int32)  # channels 1, 5, 9, 13, 17: some of every set
OMAP = np.where(MUTE < 0, -1, np.cumsum(MUTE >= 0) - 1).astype(np.int32)
assert all((OMAP[SETOF == k] < 0).any() and (OMAP[SETOF == k] >= 0).any() for k in range(3))


def vad_range(flo, fhi):
    """nr_vad_range() (design.cpp) restated: the bins of the 256-point transforms at 24 kS/s the filter passes"""
    if flo <= 0 <= fhi:
        lf, uf = 0.0, float(max(-flo, fhi))
    elif flo > 0:
        lf, uf = float(flo), float(fhi)
    else:
        lf, uf = float(-fhi), float(-flo)
    lo, hi = int(lf / 93.75) & 255, int(uf / 93.75) & 255
    hi += lo == hi
    return min(max(lo, 1), 126), min(max(hi, 1), 128)


def test_the_noise_reduction_sets_pass_the_spectral_check_and_differ_in_vad_range():
    ranges = [vad_range(kw["FLoCut"], kw["FHiCut"]) for kw in [NR_BASE] + [dict(NR_BASE, **e) for e in NR3]]
    assert ranges == [(2, 32), (3, 25), (1, 29)] and len(set(ranges)) == 3
    assert all(hi >= 17 and lo + 11 <= 127 for lo, hi in ranges)


# ---- the engine -----------------------------------------------------------------------------------------------------------------
def stage_setup(rx, nfr, on=(), index=None, fmap=None, lmap=None, nrmap=None, smap=None):
    """the switches and maps of a case on one context, the same on the staged context and on every reference: the result
    tensors to compare (the detector's, the decoder's)"""
    kept = ()
    if EQ in on:
        sw_eq(rx, 1, nfr)
    if NB in on:
        rx.set_noise_blanker(1)
    if DET in on or index is not None or fmap is not None:
        det, txt = cw_receive(rx, nfr, index)
        if DEC in on:
            kept = (det, txt)
        elif DET in on:
            rx.set_cw_decoder(0)
            kept = (det,)
        else:
            rx.set_cw_decoder(0)
            rx.set_cw_detector(0)
    if fmap is not None:
        rx.set_cw_filter_map(fmap)
    if lmap is not None:
        rx.set_receive_eq_map(lmap)
    if nrmap is not None:
        rx.set_nr_map(*nrmap)
    if smap is not None:
        rx.set_stage_map(smap)
    return kept


def group(T, base, extra, setup, setof=SETOF, sets_first=False, **options):
    """(staged context, its tensors), [(plain context of set k, its tensors)]: every context gets setup(rx) and the same
    layout, rate and maps; the staged one its sets behind them (sets_first: in front of the switches)"""
    nch = len(setof)
    if sets_first:
        a, _ = chain(T, base, nch=nch, **options)
        a.set_param_sets(extra, setof, stages=True)
        ka = setup(a)
    else:
        a, ka = chain(T, base, nch=nch, setup=setup, **options)
        a.set_param_sets(extra, setof, stages=True)
    assert a.param_sets_stages and len(a.param_sets) == len(extra) and np.array_equal(a.set_of_channel, setof)
    # (a set no channel names has no reference: nothing is compared against it, and its plain context might refuse the maps)
    return (a, ka), [chain(T, dict(base, **e), nch=nch, setup=setup, **options) if (np.asarray(setof) == k).any() else None
                     for k, e in enumerate([{}] + list(extra))]


def equal_for_sets(got, refs, setof, what, rows=None, only=None):
    for k, ref in enumerate(refs):
        sel = np.flatnonzero(np.asarray(setof) == k)
        if ref is None:
            assert sel.size == 0
            continue
        if only is not None:
            sel = sel[only[sel]]
        if rows is not None:
            sel = rows[sel][rows[sel] >= 0]
        if sel.size:
            bad = sel[np.any(bits(got)[sel].reshape(sel.size, -1) != bits(ref)[sel].reshape(sel.size, -1), axis=1)]
            assert bad.size == 0, "%s differs for rows %s of set %d" % (what, bad, k)


def compare(a, ka, refs, setof, I, Q, sl, what, host=False, written=None):
    """written: per result tensor the channels whose rows the call writes (a stage map leaves the others' rows alone, and
    what a shorter call left at their place belongs to other channels), or None for all"""
    import torch
    a_rows = a.output_map
    got = run(a, I[:, sl], Q[:, sl], host=host)
    refs = [r or (None, None) for r in refs]
    outs = [None if b is None else run(b, I[:, sl], Q[:, sl], host=host) for b, _ in refs]
    equal_for_sets(got, outs, setof, "audio of " + what, rows=a_rows)
    assert np.abs(got.astype(np.float64)).max(axis=1).min() > 0, "an audio row is all zero"
    torch.cuda.synchronize()
    # a call of n frames fills the first n_channels * n rows of a result tensor sized for more, as [n_channels][n][width]
    nch, n = a.n_channels, (sl.stop - sl.start) // L
    for i, x in enumerate(ka):
        rows_of = lambda t: first(t, nch, n, t.shape[-1])  # noqa: E731
        equal_for_sets(rows_of(x), [None if kb is None else rows_of(kb[i]) for _, kb in refs], setof, "result tensor %d of %s" % (i, what),
                       only=None if written is None else written[i])
    sa, sr = sections(a), [None if b is None else sections(b) for b, _ in refs]
    assert all(s is None or set(s) == set(sa) for s in sr), (set(sa), [s and set(s) for s in sr])
    for name in sa:
        equal_for_sets(sa[name], [s and s[name] for s in sr], setof, "section %s behind %s" % (name, what))
    return got


def check(T, base, extra, nfr, setup, setof=SETOF, q15=False, calls=None, seed=7, host=False, imap=None, sets_first=False, **options):
    if imap is not None:
        options = dict(options, imap=imap, ns=NS)
    (a, ka), refs = group(T, base, extra, partial(setup, nfr=nfr), setof, sets_first, **options)
    I, Q = streams(NS if imap is not None else len(setof), nfr * L, seed, q15)
    f0 = 0
    for n in (calls or [nfr]):
        compare(a, ka, refs, setof, I, Q, slice(f0 * L, (f0 + n) * L), "the call at frame %d" % f0, host=host)
        f0 += n
    some = next(r for r in refs if r is not None)[0]
    assert a._lib.t41rx_state_bytes(a._ctx) == some._lib.t41rx_state_bytes(some._ctx)  # sets have no state
    return a, ka, refs


# ---- 1. the stages that read nothing of a set, one at a time ---------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channel", "time"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("stage", ["equalizer", "blanker", "detector-decoder"])
def test_one_stage_next_to_the_sets(T, stage, q15, layout):
    on = {"equalizer": (EQ,), "blanker": (NB,), "detector-decoder": (DET, DEC)}[stage]
    base = CW if DET in on else USB
    a, ka, _ = check(T, base, SSB3, 5, partial(stage_setup, on=on), q15=q15, layout=layout)
    assert len(ka) == (2 if DET in on else 0)


def test_the_switches_behind_the_sets_and_the_host_entry(T):
    """the other order -- staged sets first, then the stage setters -- and the host-pointer form of the call"""
    check(T, USB, SSB3, 5, partial(stage_setup, on=(EQ, NB)), sets_first=True, host=True)
    check(T, CW, SSB3, 5, partial(stage_setup, on=(DET, DEC)), sets_first=True, q15=True, host=True)


# ---- 2. noise reduction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout,q15", [("channel", False), ("time", True)], ids=["f32", "q15-time"])
def test_noise_reduction_kind_per_set(T, layout, q15):
    """Kim, spectral and LMS + notch, each with its set's NR_alpha / NR_beta / NR_PSI and VAD range; both records per set"""
    a, _, refs = check(T, NR_BASE, NR3, 6, partial(stage_setup), layout=layout, q15=q15, calls=[2, 4])
    assert [(b.params.nrOptionSelect, b.params.ANR_notchOn) for b, _ in refs] == [(1, 0), (2, 0), (3, 1)]
    assert "nr" in sections(a)


@pytest.mark.parametrize("kind", [1, 2])
def test_one_kind_on_every_set_with_its_own_parameters(T, kind):
    base = dict(NR_BASE, nrOptionSelect=kind)
    extra = [dict(e, nrOptionSelect=kind, ANR_notchOn=0) for e in NR3]
    check(T, base, extra, 5, partial(stage_setup))


def test_noise_reduction_map_on_top_of_the_sets(T):
    """the map supplies kind and notch (every combination somewhere, on every set), the set NR_alpha / NR_beta / NR_PSI and
    the VAD range; with a stage map that clears STAGE_NR on some channels of every set"""
    codes = (np.arange(NCH) * 3 + 1) % 8
    nrmap = ((codes & 3).astype(np.int32), (codes >> 2).astype(np.int32))
    check(T, NR_BASE, NR3, 5, partial(stage_setup, nrmap=nrmap))
    smap = np.where(np.arange(NCH) % 5 == 2, 31 & ~NR, 31).astype(np.uint32)
    check(T, NR_BASE, NR3, 5, partial(stage_setup, nrmap=nrmap, smap=smap, on=(NB,)), host=True)
    check(T, NR_BASE, NR3, 5, partial(stage_setup, smap=smap), sets_first=True)


# ---- 3. the narrow CW filter ---------------------------------------------------------------------------------------------------------
FMAP = ((np.arange(NCH) * 5 + 2) % 6).astype(np.int32)  # every index 0 .. 4 and 5 (off) ...
FMAP[7] = 5                                              # ... and an unfiltered channel on every set
assert all(set(FMAP[SETOF == k]) >= {5} and (FMAP[SETOF == k] < 5).any() for k in range(3))


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_cw_filter_context_wide_index(T, q15):
    check(T, CW, CW3, 5, partial(stage_setup, index=2), q15=q15, layout="time" if q15 else "channel")


def test_cw_filter_map_with_both_classes(T):
    check(T, CW, CW3, 5, partial(stage_setup, fmap=FMAP, on=(DET, DEC)))


@pytest.mark.parametrize("fmap", [None, FMAP], ids=["index", "map"])
def test_cw_filter_at_24k(T, fmap):
    check(T, CW, CW3, 5, partial(stage_setup, index=3 if fmap is None else None, fmap=fmap), rate=24000, q15=fmap is not None)


@pytest.mark.parametrize("fmap", [None, FMAP], ids=["index", "map"])
def test_cw_filter_with_an_output_map(T, fmap):
    nrows = int(OMAP.max()) + 1
    a, _, _ = check(T, CW, CW3, 5, partial(stage_setup, index=1 if fmap is None else None, fmap=fmap), omap=OMAP, nrows=nrows)
    assert a.audio_rows == nrows


# ---- 4. everything at once -------------------------------------------------------------------------------------------------------------
def test_everything_at_once_with_a_checkpoint_between_two_calls(T):
    """stage map + level map + filter map + noise-reduction map + input map + output map, calls of 2 + 3 frames; the
    checkpoint taken between them continues in a fresh context with the same staged sets"""
    nfr = 5
    rng = np.random.default_rng(31)
    smap = rng.integers(0, 32, NCH).astype(np.uint32)
    smap = np.where((smap & DEC) != 0, smap | DET, smap).astype(np.uint32)
    lmap = rng.integers(40, 160, (NCH, 14)).astype(np.int32)
    codes = (np.arange(NCH) * 3 + 6) % 8  # (with the detector on: the notch or the blanker joins the two streams)
    nrmap = ((codes & 3).astype(np.int32), (codes >> 2).astype(np.int32))
    setup = partial(stage_setup, on=(EQ, NB, DET, DEC), fmap=FMAP, lmap=lmap, nrmap=nrmap, smap=smap)
    base = dict(CW, **{k: NR_BASE[k] for k in ("NR_alpha", "NR_beta", "NR_PSI")})
    extra = [dict(CW3[0], NR_alpha=0.9, NR_beta=0.8, NR_PSI=15.0, FHiCut=2400), dict(CW3[1], NR_alpha=0.85, NR_beta=0.9, NR_PSI=5.0)]
    options = dict(imap=MAP, ns=NS, omap=OMAP, nrows=int(OMAP.max()) + 1)
    (a, ka), refs = group(T, base, extra, partial(setup, nfr=nfr), **options)
    I, Q = streams(NS, nfr * L, 9)
    det, dec = (smap & DET) != 0, (smap & DEC) != 0  # (the rows of a channel whose bit is clear are not written)
    assert det.any() and dec.any() and not det.all()
    compare(a, ka, refs, SETOF, I, Q, slice(0, 2 * L), "the first call", written=(det, dec))
    ck = a.get_state()
    (b, kb), _ = group(T, base, extra, partial(setup, nfr=nfr), **options)
    b.set_state(ck)
    got = compare(a, ka, refs, SETOF, I, Q, slice(2 * L, 5 * L), "the second call", written=(det, dec))
    assert np.array_equal(run(b, I[:, 2 * L:], Q[:, 2 * L:]), got) and np.array_equal(b.get_state(), a.get_state())
    assert np.array_equal(a.cw_results(3).cpu().numpy()[det], b.cw_results(3).cpu().numpy()[det])
    assert np.array_equal(a.cw_text(3).cpu().numpy()[dec], b.cw_text(3).cpu().numpy()[dec])


# ---- 5. degenerate tables --------------------------------------------------------------------------------------------------------------
def test_one_channel_on_the_last_set(T):
    check(T, NR_BASE, NR3, 5, partial(stage_setup, on=(NB,)), setof=np.array([2], np.int32))
    check(T, CW, CW3, 5, partial(stage_setup, index=0), setof=np.array([2], np.int32))


def test_all_channels_on_one_extra_set(T):
    check(T, NR_BASE, NR3[:1], 5, partial(stage_setup, on=(EQ,)), setof=np.ones(NCH, np.int32))
    check(T, CW, CW3[:1], 5, partial(stage_setup, fmap=FMAP), setof=np.ones(NCH, np.int32))


def test_a_set_nobody_names_that_fails_the_spectral_check(T):
    """the header's choice: a set whose own nrOptionSelect is 2 and whose pass band fails the check is an invalid
    t41rx_params and is refused whether a channel names it or not; the same pass band with another kind is accepted as long
    as no channel runs kind 2 on it -- under a map too"""
    narrow = dict(FLoCut=300, FHiCut=1000)
    table = np.where(SETOF == 2, 0, SETOF).astype(np.int32)  # nobody names set 2
    a, _ = chain(T, NR_BASE)
    refused(lambda: a.set_param_sets([NR3[0], dict(narrow, nrOptionSelect=2)], table, stages=True), ERR_ARG, "set 2 is invalid", "nrOptionSelect = 2")
    assert a.param_sets == [] and not a.param_sets_stages
    check(T, NR_BASE, [NR3[0], dict(narrow, nrOptionSelect=3)], 5, partial(stage_setup), setof=table)
    kind = np.where(table == 1, 2, 1).astype(np.int32)
    check(T, NR_BASE, [NR3[0], dict(narrow, nrOptionSelect=3)], 5, partial(stage_setup, nrmap=(kind, np.zeros(NCH, np.int32))), setof=table)


# ---- 6. refusals and interplay ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_configuration_whole(T):
    nfr = 2
    setup = partial(stage_setup, on=(NB,), nfr=nfr)
    (a, ka), refs = group(T, NR_BASE, NR3, setup)
    lib = a._lib
    I, Q = streams(NCH, nfr * L, 18)
    P = type(a.params)
    ip = lambda m: np.ascontiguousarray(m, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    n_ok = [0]

    def still_works():
        assert a.param_sets_stages and len(a.param_sets) == 2 and np.array_equal(a.set_of_channel, SETOF)
        compare(a, ka, refs, SETOF, I, Q, slice(0, nfr * L), "the call behind refusal %d" % n_ok[0])
        n_ok[0] += 1

    def arr(dicts):
        v = (P * len(dicts))()
        for i, d in enumerate(dicts):
            v[i] = T.default_params(**dict(NR_BASE, **d))
        return v

    still_works()
    # an unknown flag, whatever else is passed
    for flags in (2, 3, -1):
        assert lib.t41rx_set_param_sets_ex(a._ctx, arr(NR3), 2, ip(SETOF), NCH, flags) == ERR_ARG and b"unknown flag" in lib.t41rx_last_error()
        still_works()
    # the spectral check names the channel and the set: (1) the sets loaded onto a map with an entry 2 ...
    narrow = dict(FLoCut=300, FHiCut=1000, nrOptionSelect=0)
    first2 = int(np.flatnonzero(SETOF == 2)[0])
    kind = np.where(np.arange(NCH) == first2, 2, 1).astype(np.int32)
    a.set_nr_map(kind, np.zeros(NCH, np.int32))
    for b, _ in refs:
        b.set_nr_map(kind, np.zeros(NCH, np.int32))
    still_works()
    refused(lambda: a.set_param_sets([NR3[0], narrow], SETOF, stages=True), ERR_ARG, "channel %d " % first2, "set 2", "nrOptionSelect = 2")
    still_works()
    # (2) ... the map set onto the sets ...
    ones = np.ones(NCH, np.int32)
    a.set_nr_map(ones, np.zeros(NCH, np.int32))
    a.set_param_sets([NR3[0], dict(NR3[1], FLoCut=-1000, FHiCut=-300)], SETOF, stages=True)
    two = np.where(SETOF == 2, 2, 0).astype(np.int32)
    refused(lambda: a.set_nr_map(two, np.zeros(NCH, np.int32)), ERR_ARG, "channel %d " % first2, "set 2", "nrOptionSelect = 2")
    assert np.array_equal(a.nr_map[0], ones)
    a.set_param_sets(NR3, SETOF, stages=True)
    a.set_nr_map(kind, np.zeros(NCH, np.int32))
    still_works()
    # (3) ... and set 0's pass band through t41rx_set_params / t41rx_set_coeffs
    first0 = int(np.flatnonzero(SETOF == 0)[0])
    zero = np.where(SETOF == 0, 2, 0).astype(np.int32)
    a.set_nr_map(zero, np.zeros(NCH, np.int32))
    refused(lambda: a.CalcFilters(FLoCut=300, FHiCut=1000), ERR_ARG, "channel %d " % first0, "set 0", "nrOptionSelect = 2")
    blob = T.design_coeffs(T.default_params(**dict(NR_BASE, FLoCut=300, FHiCut=1000)))
    refused(lambda: a.set_coeffs(blob), ERR_ARG, "channel %d " % first0, "set 0")
    assert (a.params.FLoCut, a.params.FHiCut) == (200, 3000)
    a.set_nr_map(kind, np.zeros(NCH, np.int32))
    still_works()
    # the old entry point with a stage on: refused as ever, and the staged sets stay
    refused(lambda: a.set_param_sets(SSB3, SETOF), ERR_UNSUPPORTED, "noise blanker", "parameter sets")
    still_works()
    a.set_nr_map(None)
    for b, _ in refs:
        b.set_nr_map(None)
    still_works()
    # staged -> none -> plain -> a stage setter refuses in the old words
    a.set_noise_blanker(0)
    a.set_param_sets(None)
    assert a.param_sets == [] and not a.param_sets_stages
    a.CalcFilters(nrOptionSelect=0)
    a.set_param_sets(SSB3, SETOF)
    assert not a.param_sets_stages and len(a.param_sets) == 2
    refused(lambda: a.set_noise_blanker(1), ERR_UNSUPPORTED, "noise blanker", "splits the fused chain", "parameter sets")
    refused(lambda: a.set_nr_map(kind, np.zeros(NCH, np.int32)), ERR_UNSUPPORTED, "noise-reduction map", "parameter sets")
    assert not a.param_sets_stages and len(a.param_sets) == 2


def test_staged_sets_at_a_long_fft_length_and_the_one_stream_rule(T):
    for n_fft in (1024, 4096):
        lng = T.RxChain(NCH, T.default_params(fft_length=n_fft, mode=0, FLoCut=400, FHiCut=600))
        refused(lambda: lng.set_param_sets([dict(FHiCut=700)], np.ones(NCH, np.int32), stages=True), ERR_UNSUPPORTED, "fft_length %d" % n_fft, "long-FFT")
        assert lng.param_sets == [] and not lng.param_sets_stages
    # the detector's one-audio-stream rule, per channel with the channel's own set's kind and notch: set 1 runs Kim
    # without the notch or the blanker behind it
    nfr = 2
    a, _ = chain(T, dict(CW, nrOptionSelect=0), setup=partial(stage_setup, nfr=nfr, on=(DET,)))
    a.set_param_sets([dict(nrOptionSelect=1), dict(nrOptionSelect=3, ANR_notchOn=1)], SETOF, stages=True)
    I, Q = streams(NCH, nfr * L, 4)
    first1 = int(np.flatnonzero(SETOF == 1)[0])
    before = sections(a)["path"]
    refused(lambda: run(a, I, Q), ERR_UNSUPPORTED, "CW detector", "Kim", "channel %d " % first1, "parameter set 1")
    # nothing was processed (the refused call may have allocated the stages' memories, at power-on: new sections, as without sets)
    assert np.array_equal(sections(a)["path"], before)
    # a map overrides the sets' values, and the text says so
    kind = np.where(np.arange(NCH) == 4, 3, 0).astype(np.int32)
    a.set_nr_map(kind, np.zeros(NCH, np.int32))
    refused(lambda: run(a, I, Q), ERR_UNSUPPORTED, "CW detector", "LMS", "channel 4 ", "noise-reduction map")
    a.set_nr_map(None)
    a.set_noise_blanker(1)  # the blanker joins the two streams: the call runs
    assert np.abs(run(a, I, Q)).max(axis=1).min() > 0


# ---- 7. flags == 0 through the new entry is the old entry ------------------------------------------------------------------------------------
def test_flags_0_through_the_ex_entry_is_the_old_entry(T):
    a, _ = chain(T, USB)
    b, _ = chain(T, USB, sets=SSB3, setof=SETOF)
    lib, P = a._lib, type(a.params)
    v = (P * 2)()
    for i, d in enumerate(SSB3):
        v[i] = T.default_params(**dict(USB, **d))
    table = np.ascontiguousarray(SETOF, np.int32)
    tp = table.ctypes.data_as(C.POINTER(C.c_int32))
    assert lib.t41rx_set_param_sets_ex(a._ctx, v, 2, tp, NCH, 0) == 0
    assert lib.t41rx_get_param_sets_flags(a._ctx) == 0 and not a.param_sets_stages and len(a.param_sets) == 2
    I, Q = streams(NCH, 5 * L, 19)
    assert np.array_equal(run(a, I, Q), run(b, I, Q)) and np.array_equal(a.get_state(), b.get_state())
    # one refusal text: a stage setter, and the sets onto a stage
    texts = []
    for rx in (a, b):
        assert lib.t41rx_set_noise_blanker(rx._ctx, 1) == ERR_UNSUPPORTED
        texts.append(lib.t41rx_last_error())
    assert texts[0] == texts[1] and b"remove the sets first" in texts[0]
    for rx in (a, b):
        rx.set_param_sets(None)
        rx.set_noise_blanker(1)
    assert lib.t41rx_set_param_sets_ex(a._ctx, v, 2, tp, NCH, 0) == ERR_UNSUPPORTED
    new = lib.t41rx_last_error()
    assert lib.t41rx_set_param_sets(b._ctx, v, 2, tp, NCH) == ERR_UNSUPPORTED and lib.t41rx_last_error() == new and b"noise blanker" in new
    assert a.param_sets == [] and b.param_sets == []
