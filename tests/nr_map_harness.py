"""What the noise-reduction map's tests share (tests/test_nr_map.py; t41rx_set_nr_map): ONE engine, modelled on
stage_map_harness.run_schedule, that runs a schedule of maps on a mapped context next to reference contexts WITHOUT a map
and compares everything bit for bit.

The reference of a channel is built from the rule itself: while a map is loaded channel c is processed as the same channel
of a context without a map whose parameters carry nrOptionSelect = nr_of_channel[c] and ANR_notchOn = notch_of_channel[c]
-- 0 / 0 where a stage map clears the channel's STAGE_NR bit.  So for every distinct history of (kind, notch), one pair per
call, the engine keeps one context without a map and drives it with CalcFilters(nrOptionSelect=, ANR_notchOn=) call by call
-- the library's own switch, which keeps the records of a function that is off stale, as the firmware's statics are -- and
compares the channels with that history against it: audio rows and every section of the checkpoint.  Call 0 of every
schedule has no map and runs BASE on every channel, so that every context has the noise-reduction section allocated and both
records hold something before the first map is set.
"""
import numpy as np

import group_harness as G
from rx_harness import one_call, streams
from stage_map_harness import NR, sections

L = 2048
BASE = (2, 1)  # call 0, context-wide: the spectral function and the notch -- both records move
COMBOS = [(k, t) for t in (0, 1) for k in (0, 1, 2, 3)]  # code = kind + 4 * notch


def pairs(codes):
    """codes (kind + 4 * notch) -> (nr_of_channel, notch_of_channel)"""
    codes = np.asarray(codes, np.int32)
    return codes & 3, codes >> 2


def context(T, nch, kw=G.USB, **options):
    rx, _ = G.chain(T, dict(kw, nrOptionSelect=BASE[0], ANR_notchOn=BASE[1]), nch=nch, **options)
    return rx


def run_schedule(T, schedule, nfr, nch=G.NCH, kw=G.USB, seed=3, stages=None, q15=False, host=False, imap=None, checkpoint_after=None,
                 **options):
    """The engine.  schedule: per call None (no map: BASE on every channel) or the codes [nch] (kind + 4 * notch); call 0
    must be None.  stages: None, or per call None / the stage map of the mapped context for that call.  Runs the mapped
    context and one reference context without any map per history of effective pairs, nfr frames per call, and holds after
    every call, bit for bit: audio rows and every checkpoint section; where the effective pair is 0 / 0 also that both
    records are what a checkpoint in front of the call held.
    checkpoint_after=k: behind call k the mapped context's checkpoint goes into a fresh context with the same maps, which
    then runs the rest of the schedule too and must stay identical.
    Returns (the mapped context, the effective codes [calls, nch], its audio per call)."""
    assert schedule[0] is None
    ncall = len(schedule)
    stages = [None] * ncall if stages is None else stages
    base = BASE[0] + 4 * BASE[1]
    eff = np.array([np.full(nch, base, np.int32) if m is None else np.asarray(m, np.int32) for m in schedule])
    for k, s in enumerate(stages):
        if s is not None:
            eff[k][(np.asarray(s, np.uint32) & NR) == 0] = 0
    history = [tuple(int(v) for v in eff[:, c]) for c in range(nch)]
    if imap is not None:
        options = dict(options, imap=imap, ns=G.NS)
    a = context(T, nch, kw, **options)
    refs = {h: context(T, nch, kw, **options) for h in sorted(set(history))}
    omap = a.output_map
    row_of = np.arange(nch) if omap is None else omap
    I, Q = streams(G.NS if imap is not None else nch, ncall * nfr * L, seed, q15)
    twin, audio = None, []
    for k, m in enumerate(schedule):
        sl = slice(k * nfr * L, (k + 1) * nfr * L)
        for rx in (a, twin):
            if rx is None:
                continue
            rx.set_stage_map(stages[k])
            if m is None:
                rx.set_nr_map(None)
                assert rx.nr_map is None
            else:
                rx.set_nr_map(*pairs(m))
                got_map = rx.nr_map
                assert np.array_equal(got_map[0], pairs(m)[0]) and np.array_equal(got_map[1], pairs(m)[1])
            # the context's own two values are kept and not consulted
            assert (rx.params.nrOptionSelect, rx.params.ANR_notchOn) == BASE
        before = sections(a)
        got, _ = one_call(a, I[:, sl], Q[:, sl], host=host)
        after = sections(a)
        audio.append(got)
        assert (set(after) == set(before) or k == 0) and "nr" in after
        if twin is not None:
            got2, _ = one_call(twin, I[:, sl], Q[:, sl], host=host)
            assert np.array_equal(got2, got) and np.array_equal(twin.get_state(), a.get_state()), "call %d: the restored context went its own way" % k
        for h, r in refs.items():
            chans = np.array([c for c in range(nch) if history[c] == h])
            r.CalcFilters(nrOptionSelect=h[k] & 3, ANR_notchOn=h[k] >> 2)
            ref, _ = one_call(r, I[:, sl], Q[:, sl], host=host)
            rs = sections(r)
            rows = row_of[chans][row_of[chans] >= 0]
            assert np.array_equal(got[rows], ref[rows]), "call %d, (kind, notch) %s: audio of channels %s" % (k, COMBOS[h[k]], chans)
            assert set(rs) == set(after), (set(rs), set(after))
            for name in after:
                bad = chans[np.any(after[name][chans] != rs[name][chans], axis=1)]
                assert bad.size == 0, "call %d, (kind, notch) %s: section %s of channels %s" % (k, COMBOS[h[k]], name, bad)
        # 0 / 0: both records are what they were in front of the call; anything else: a record moved
        off, on = np.flatnonzero(eff[k] == 0), np.flatnonzero(eff[k] != 0)
        if k > 0:
            assert np.array_equal(after["nr"][off], before["nr"][off]), "call %d: a channel with 0 / 0 had its records moved" % k
        if k > 0 and on.size:
            assert np.any(after["nr"][on] != before["nr"][on], axis=1).all(), "call %d: a channel that asks for a function kept its records" % k
        if checkpoint_after == k:
            twin = context(T, nch, kw, **options)
            twin.set_state(a.get_state())
    return a, eff, audio
