"""The CW filter map (t41rx_set_cw_filter_map): while a map is loaded, channel c is processed exactly as the same channel of a
context without a map whose t41rx_set_cw_filter() value is filter_of_channel[c] -- its audio row, the five per-filter
memories (only the selected one advances), the interpolator memories, every other state word.

Every comparison is bit for bit (uint32 views) against contexts WITHOUT a map, one per distinct history of indices, fed the
same input and switched with t41rx_set_cw_filter() call by call, as tests/stage_map_harness.py builds its references.  19
channels are two full eight-channel waves of the filter kernel and a ragged three; 1 and 8 channels one ragged and one full
wave.  One frame is four 64-sample chunks: the pipeline fills and drains in one call."""
import numpy as np
import pytest

import cw_model as CWM
import group_harness as G
import stage_map_harness as H
from group_harness import NCH, NS, STREAM_OF
from rx_harness import T, bits, one_call, streams  # noqa: F401  (T: a fixture)

pytestmark = pytest.mark.gpu

L = 2048
CW_KW = dict(G.USB, xmtMode=1)
OFF = 5
# mutes two filtered channels (1: index 1, 9: index 3) and two unfiltered ones (5, 11), the rest in reverse order
OMAP = np.full(NCH, -1, np.int32)
_listened = [c for c in range(NCH) if c not in (1, 5, 9, 11)]
OMAP[_listened] = np.arange(len(_listened))[::-1]
NROWS = len(_listened)


def cycle(nch, shift=0):
    """0, 1, 2, 3, 4, 5, 0, ..: every wave holds several indices and an off channel"""
    return ((np.arange(nch) + shift) % 6).astype(np.int32)


def context(T, nch, base=OFF, kw=CW_KW, **options):
    rx, _ = G.chain(T, kw, nch=nch, **options)
    rx.set_cw_tables(*CWM.tables())
    rx.set_cw_filter(base)
    return rx


def sections(rx, nch):
    """path and cw rows of the checkpoint; a context whose CW stages never ran has no cw section: power-on zeros"""
    s = H.sections(rx)
    return s["path"], s.get("cw", np.zeros((nch, 128), np.uint32))


def run_maps(T, schedule, nfrs, nch=NCH, base=OFF, kw=CW_KW, q15=False, seed=7, omap_after=False, **options):
    """The engine.  schedule: per call the map [nch] or None (no map: the context-wide index `base`); nfrs: frames per
    call.  Runs the mapped context and one reference without a map per history of effective indices, and holds after every
    call: the audio rows, the path records and the cw section of the history's channels.  omap_after: the mapped context
    takes the output map of `options` behind its first filter map, the references at creation."""
    mine = dict(options)
    if omap_after:
        mine.pop("omap"), mine.pop("nrows")
    a = context(T, nch, base, kw, **mine)
    eff = np.array([np.full(nch, base, np.int32) if m is None else np.asarray(m, np.int32) for m in schedule])
    history = [tuple(int(v) for v in eff[:, c]) for c in range(nch)]
    refs = {h: context(T, nch, OFF, kw, **options) for h in sorted(set(history))}
    rows_in = NS if options.get("imap") is not None else nch
    I, Q = streams(rows_in, sum(nfrs) * L, seed, q15)
    f0, audio = 0, []
    for k, (m, nfr) in enumerate(zip(schedule, nfrs)):
        sl = slice(f0 * L, (f0 + nfr) * L)
        f0 += nfr
        a.set_cw_filter_map(m)
        got_map = a.cw_filter_map
        assert (got_map is None) if m is None else np.array_equal(got_map, m)
        assert a.cw_filter == base  # the context-wide index is kept
        if omap_after and k == 0:
            a.set_output_map(options["omap"], options["nrows"])
        omap = a.output_map
        row_of = np.arange(nch) if omap is None else omap
        got, _ = one_call(a, I[:, sl], Q[:, sl])
        audio.append(got)
        path, cw = sections(a, nch)
        for h, r in refs.items():
            chans = np.array([c for c in range(nch) if history[c] == h])
            r.set_cw_filter(h[k])
            ref, _ = one_call(r, I[:, sl], Q[:, sl])
            rpath, rcw = sections(r, nch)
            rows = row_of[chans][row_of[chans] >= 0]
            assert got.shape == ref.shape and got.dtype == ref.dtype
            assert np.array_equal(bits(got)[rows], bits(ref)[rows]), "call %d, index %d: audio of channels %s" % (k, h[k], chans)
            assert np.array_equal(path[chans], rpath[chans]), "call %d, index %d: path records of channels %s" % (k, h[k], chans)
            assert np.array_equal(cw[chans], rcw[chans]), "call %d, index %d: cw section of channels %s" % (k, h[k], chans)
    return a, audio


SPLITS = {"1": [1], "3": [3], "2+1": [2, 1]}


@pytest.mark.parametrize("split", list(SPLITS))
@pytest.mark.parametrize("nch,shift", [(NCH, 0), (8, 2), (1, 2)])
def test_mixed_map_shapes(T, nch, shift, split):
    m = cycle(nch, shift)
    nfrs = SPLITS[split]
    run_maps(T, [m] * len(nfrs), nfrs, nch=nch)


VARIANTS = {
    "q15": dict(q15=True),
    "time-major": dict(layout="time"),
    "time-major-q15": dict(layout="time", q15=True),
    "24k": dict(rate=24000),
    "24k-q15": dict(rate=24000, q15=True),
    "24k-time-major": dict(rate=24000, layout="time"),
    "input-map": dict(imap=STREAM_OF, ns=NS),
    "output-map-before": dict(omap=OMAP, nrows=NROWS),
    "output-map-after": dict(omap=OMAP, nrows=NROWS, omap_after=True),
    "output-map-24k": dict(omap=OMAP, nrows=NROWS, rate=24000),
    "output-map-after-q15-time-major": dict(omap=OMAP, nrows=NROWS, omap_after=True, q15=True, layout="time"),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mixed_map_variants(T, variant):
    m = cycle(NCH)
    assert set(m[:8]) == set(range(6)) and m[1] < OFF and m[9] < OFF and m[5] == OFF and m[11] == OFF
    run_maps(T, [m, m], [2, 1], **VARIANTS[variant])


def test_output_map_changes_under_a_loaded_filter_map(T):
    """the two derived row maps follow the output map: set, replaced by another, removed, all under one filter map"""
    m = cycle(NCH)
    a = context(T, NCH)
    refs = {k: context(T, NCH, k) for k in range(6)}
    a.set_cw_filter_map(m)
    I, Q = streams(NCH, 4 * L, 19)
    other = np.roll(OMAP, 3)
    for k, om in enumerate((None, OMAP, other, None)):
        sl = slice(k * L, (k + 1) * L)
        for rx in [a] + list(refs.values()):
            rx.set_output_map(om, None if om is None else NROWS)
        got, _ = one_call(a, I[:, sl], Q[:, sl], guard=True)
        row_of = np.arange(NCH) if om is None else om
        for idx, r in refs.items():
            ref, _ = one_call(r, I[:, sl], Q[:, sl], guard=True)
            rows = row_of[m == idx]
            rows = rows[rows >= 0]
            assert np.array_equal(bits(got)[rows], bits(ref)[rows]), "call %d, index %d" % (k, idx)
            assert np.array_equal(H.sections(a)["path"][m == idx], H.sections(r)["path"][m == idx]), "call %d, index %d: path" % (k, idx)


def test_detector_and_decoder_do_not_see_the_map(T):
    """they read ahead of the filter: their result rows and the cwdec section are those of the same call without a map"""
    import test_cw_decoder as CWT
    nfr, ncall = 6, 2
    nco = __import__("siggen").nco_grid(NCH, seed=11)
    keys = (np.random.default_rng(4).random((NCH, ncall * nfr)) < 0.5).astype(np.float64)
    I, Q = CWT.call_iq(nco, keys, 0, 4)
    out = []
    for mapped in (True, False):
        rx, _ = G.chain(T, CW_KW)
        det, txt = G.cw_receive(rx, nfr)
        rx.set_cw_clock(*H.CW_CLOCK)
        if mapped:
            rx.set_cw_filter_map(cycle(NCH))
        seen = []
        for k in range(ncall):
            sl = slice(k * nfr * L, (k + 1) * nfr * L)
            audio, _ = one_call(rx, I[:, sl], Q[:, sl])
            import torch
            torch.cuda.synchronize()
            seen.append((audio, rx.cw_results(nfr).cpu().numpy().copy(), rx.cw_text(nfr).cpu().numpy().copy(), H.sections(rx)["cwdec"]))
        out.append(seen)
    off = cycle(NCH) == OFF
    for (a_aud, a_det, a_txt, a_dec), (b_aud, b_det, b_txt, b_dec) in zip(*out):
        assert np.array_equal(bits(a_det), bits(b_det)) and np.array_equal(a_txt, b_txt) and np.array_equal(a_dec, b_dec)
        assert np.abs(b_det).max() > 0
        assert np.array_equal(bits(a_aud)[off], bits(b_aud)[off])
        assert all(not np.array_equal(a_aud[c], b_aud[c]) for c in np.flatnonzero(~off)), "a filtered channel's audio is the unfiltered one"


@pytest.mark.parametrize("k", [0, 3, OFF])
def test_uniform_map_is_the_context_wide_index(T, k):
    """a uniform map k equals context-wide k (the all-filtered map plans the one CW back end), all 5 equals filter off --
    under a context-wide index of another value, which is not consulted"""
    run_maps(T, [np.full(NCH, k, np.int32)] * 2, [2, 1], base=1)


def test_removing_the_map_returns_to_the_context_wide_index(T):
    run_maps(T, [cycle(NCH), None, np.full(NCH, OFF, np.int32), None], [1, 2, 1, 1], base=3)


def test_mid_stream_change_resumes_the_filters_memory(T):
    """channel 6 goes 2 -> 4 -> 2 (and channel 13 4 -> 5 -> 4): the reference calls t41rx_set_cw_filter 2, 4, 2, so
    filter 2's memory resumes where it stopped and filter 4's holds what the middle call left"""
    m0 = cycle(NCH)
    m0[6], m0[13] = 2, 4
    m1 = m0.copy()
    m1[6], m1[13] = 4, OFF
    a, _ = run_maps(T, [m0, m1, m0], [2, 1, 2])
    cw = H.sections(a)["cw"].view(np.float32)
    assert np.abs(cw[6, 24:36]).max() > 0 and np.abs(cw[6, 48:60]).max() > 0  # filters 2 and 4 of channel 6 both ran
    assert not cw[6, 0:24].any() and not cw[6, 36:48].any()                   # and no other


def test_other_xmtmode_ignores_the_map(T):
    """xmtMode not CW: nothing of the CW block runs, a loaded map changes nothing"""
    I, Q = streams(NCH, 3 * L, 23)
    a, b = context(T, NCH, kw=G.USB), context(T, NCH, kw=G.USB)
    a.set_cw_filter_map(cycle(NCH))
    for sl in (slice(0, 2 * L), slice(2 * L, 3 * L)):
        got, _ = one_call(a, I[:, sl], Q[:, sl])
        ref, _ = one_call(b, I[:, sl], Q[:, sl])
        assert np.array_equal(bits(got), bits(ref))
    assert np.array_equal(a.get_state(), b.get_state())
    assert np.array_equal(a.cw_filter_map, cycle(NCH))


def test_reset_keeps_the_map(T):
    a = context(T, NCH)
    a.set_cw_filter_map(cycle(NCH))
    a.reset()
    assert np.array_equal(a.cw_filter_map, cycle(NCH))
