"""What the stage-map tests share (tests/test_stage_map.py; t41rx_set_stage_map): the stages as cases with their switches,
a checkpoint cut into its sections per channel, and ONE engine that runs a schedule of maps on a mapped context next to
reference contexts WITHOUT a map and compares everything bit for bit.

The reference of a channel is built from the rule itself: stage S runs on channel c in a call exactly when the context's
switch is on and the channel's bit is set, and a channel whose bit is clear is processed as the same channel of a context
in which S is switched off.  So for every distinct history of effective masks (one mask per call) the engine keeps one
context without a map whose switches, call by call, are exactly that mask -- the library's own off / on switches, which
keep a stage's memory stale while it is off, as the firmware's statics do -- and compares the channels with that history
against it: audio rows, the detector's and the decoder's result rows, and every section of the checkpoint.  Call 0 of
every schedule has no map (every stage of the case on every channel), so that every context has every section allocated
and every memory holds something before the first bit is cleared.
"""
import numpy as np

import group_harness as G
import siggen
from rx_harness import one_call, streams

L, D = 2048, 256
EQ, NR, NB, DET, DEC, ALL = 1, 2, 4, 8, 16, 31
SENT_F, SENT_I = -7777.25, 0x5A5A5A5A
SECTION_OF = {EQ: "eq", NR: "nr", NB: "nb", DET: "cw", DEC: "cwdec"}
# the checkpoint's sections in bit order with their words per channel (rx_state.cpp: kSections; nr_kernels.hpp,
# nb_kernels.hpp, eq_kernels.hpp, cw_kernels.hpp; the display section, bit 2, is rx_internal.hpp's kDispFloats and is carried
# while the display spectrum is on: tests/test_batch_isolation.py's tap cases)
ANR_ROWS, NR_SPEC = 64 + 79 + 2, 3 * 128 + 15 * 128 + 9 * 128 + 8
SECTIONS = ((1, "nr", ANR_ROWS + NR_SPEC), (2, "disp", 64 + 1024 + 512), (4, "nb", 16), (8, "eq", 112), (16, "cw", 128), (32, "cwdec", 3104))


def sections(rx, buf=None):
    """a checkpoint as {name: uint32 [n_channels, words]}: the path's records and every section it carries, Xanr()'s
    channel-minor rows turned per channel"""
    buf = rx.get_state() if buf is None else buf
    nch, hdr = rx.n_channels, buf[:32].view(np.int32)
    per, sec = int(hdr[4]), int(hdr[5])
    off = 32 + 4 * per * nch
    out = {"path": buf[32:off].view(np.uint32).reshape(nch, per)}
    for bit, name, k in SECTIONS:
        if not sec & bit:
            continue
        w = buf[off:off + 4 * k * nch].view(np.uint32)
        off += 4 * k * nch
        if name == "nr":
            out[name] = np.concatenate([w[:ANR_ROWS * nch].reshape(ANR_ROWS, nch).T, w[ANR_ROWS * nch:].reshape(nch, NR_SPEC)], axis=1)
        else:
            out[name] = w.reshape(nch, k)
    assert off == len(buf), (off, len(buf), sec)
    return out


# ---- the stages' switches: fn(rx, on, nfr) ------------------------------------------------------------------------------
def sw_eq(rx, on, nfr):
    import eq_model as EQM
    import test_receive_eq as E
    if on:
        rx.set_receive_eq_bands(EQM.bands())
        rx.set_receive_eq(1, E.RAMP)
    else:
        rx.set_receive_eq(0)


def sw_nr(option, notch):
    return lambda rx, on, nfr: rx.CalcFilters(nrOptionSelect=option if on else 0, ANR_notchOn=notch if on else 0)


def sw_nb(rx, on, nfr):
    rx.set_noise_blanker(int(on))


def sw_det(rx, on, nfr):
    rx._sm_det = rx.set_cw_detector(int(on), nfr)


def sw_dec(rx, on, nfr):
    rx._sm_txt = rx.set_cw_decoder(int(on), nfr)


class Case:
    """the stages a context of the case has switched on, by bit; its parameters; its signal"""

    def __init__(self, name, switches, kw=G.USB, signal="noise"):
        self.name, self.switches, self.kw, self.signal = name, switches, kw, signal
        self.bits = sum(switches)

    def __repr__(self):
        return self.name


CW_KW = dict(G.USB, xmtMode=1)
WIDE = dict(mode=0, FLoCut=100, FHiCut=11000)  # tests/test_noise_blanker.py: a wide filter, so that the clicks stay short
CASES = {c.name: c for c in (
    Case("eq", {EQ: sw_eq}, signal="tones"),
    Case("kim", {NR: sw_nr(1, 0)}),
    Case("spectral", {NR: sw_nr(2, 0)}),
    Case("lms", {NR: sw_nr(3, 0)}),
    Case("notch", {NR: sw_nr(0, 1)}),
    Case("lms-notch", {NR: sw_nr(3, 1)}),  # Xanr() twice per frame in one launch: both passes take the same list
    Case("blanker", {NB: sw_nb}, kw=WIDE, signal="clicks"),
    Case("detector", {DET: sw_det}, kw=CW_KW, signal="cw"),
    Case("decoder", {DET: sw_det, DEC: sw_dec}, kw=CW_KW, signal="cw"),
    Case("eq-notch-blanker", {EQ: sw_eq, NR: sw_nr(0, 1), NB: sw_nb}, kw=WIDE, signal="clicks"),
    Case("eq-blanker", {EQ: sw_eq, NB: sw_nb}, kw=WIDE, signal="clicks"),
)}
# 700 ms per frame: a carrier of one frame is a signal of 20 .. 750 ms, and from frame 8 on the 5000 ms between two
# histogram calls have passed (tests that want the decoder's served calls run 6 frames per call)
CW_CLOCK = (0, 700, 1)


def signal(case, rows, nfr, seed, nco, q15=False):
    """the stream of a case, [rows, nfr * L] I and Q: distinct noise per row; tones in noise; the blanker's clicks; a keyed
    carrier per channel"""
    if case.signal == "clicks" and not q15:
        import test_noise_blanker as NBT
        return NBT.clicky_iq(rows, nfr, seed)
    if case.signal == "cw":
        import test_cw_decoder as CWT
        keys = (np.random.default_rng(seed).random((rows, nfr)) < 0.5).astype(np.float64)
        return CWT.call_iq(nco, keys, 0, seed)
    if case.signal == "tones" and not q15:
        return siggen.make_iq(rows, nfr * L, nco[:rows], mode=0, seed=seed, sigma=0.05)  # tests/test_receive_eq.py's
    return streams(rows, nfr * L, seed, q15)


def context(T, case, nfr, nch, **options):
    """a fresh context of the case with every switch of the case off, and what the CW stages need loaded"""
    rx, _ = G.chain(T, case.kw, nch=nch, **options)
    if case.bits & (DET | DEC):
        import cw_decode_model as DM
        import cw_model as CWM
        rx.set_cw_tables(*CWM.tables())
        rx.set_cw_decode_tree(DM.tree())
        rx.set_cw_clock(*CW_CLOCK)
    rx._sm_on, rx._sm_det, rx._sm_txt = 0, None, None
    return rx


def switch(rx, case, mask, nfr):
    """the context's switches become exactly `mask` (of the case's stages)"""
    for bit, fn in case.switches.items():
        if (rx._sm_on ^ mask) & bit:
            fn(rx, bool(mask & bit), nfr)
    rx._sm_on = mask


def results(rx, nfr):
    """(the detector's rows, the decoder's rows) of the last call as numpy, None where the stage is off"""
    import torch
    torch.cuda.synchronize()
    det = None if rx._sm_det is None else rx.cw_results(nfr).cpu().numpy()
    txt = None if rx._sm_txt is None else rx.cw_text(nfr).cpu().numpy()
    return det, txt


def run_schedule(T, case, schedule, nfr, nch=G.NCH, seed=3, tap=False, q15=False, host=False, imap=None, checkpoint_after=None,
                 **options):
    """The engine.  schedule: per call None (no map) or the masks [nch]; call 0 must be None.  Runs the mapped context
    and one reference context without a map per history of effective masks, nfr frames per call, and holds after every
    call, bit for bit: audio rows, result rows (a sentinel where the channel's bit is clear), every checkpoint section;
    where a bit is clear also that the stage's records are what a checkpoint in front of the call held.
    checkpoint_after=k: behind call k the mapped context's checkpoint goes into a fresh context with the same map, which
    then runs the rest of the schedule too and must stay identical.
    Returns (the mapped context, the effective masks [calls, nch], its audio per call, its demod tap per call or None)."""
    assert schedule[0] is None
    ncall = len(schedule)
    eff = np.array([np.full(nch, case.bits, np.uint32) if m is None else (np.asarray(m, np.uint32) & case.bits) for m in schedule])
    history = [tuple(int(v) for v in eff[:, c]) for c in range(nch)]
    if imap is not None:
        options = dict(options, imap=imap, ns=G.NS)
    a = context(T, case, nfr, nch, **options)
    switch(a, case, case.bits, nfr)
    refs = {h: context(T, case, nfr, nch, **options) for h in sorted(set(history))}
    omap = a.output_map
    row_of = np.arange(nch) if omap is None else omap
    rows_in = G.NS if imap is not None else nch
    nco = siggen.nco_grid(nch, seed=11)  # (G.chain's)
    I, Q = signal(case, rows_in, ncall * nfr, seed, nco, q15)
    call = dict(host=host, tap_floats=D if tap else None)
    twin, audio, taps = None, [], []
    for k, m in enumerate(schedule):
        sl = slice(k * nfr * L, (k + 1) * nfr * L)
        for rx in (a, twin):
            if rx is None:
                continue
            rx.set_stage_map(m)
            got_map = rx.stage_map
            assert (got_map is None) if m is None else np.array_equal(got_map, np.asarray(m, np.uint32))
            for t, s in ((rx._sm_det, SENT_F), (rx._sm_txt, SENT_I)):
                if t is not None:
                    t.fill_(s)
        before = sections(a)
        got, tp = one_call(a, I[:, sl], Q[:, sl], **call)
        after = sections(a)
        det, txt = results(a, nfr)
        audio.append(got)
        taps.append(tp)
        assert set(after) == set(before) or k == 0
        if twin is not None:
            got2, _ = one_call(twin, I[:, sl], Q[:, sl], **call)
            assert np.array_equal(got2, got) and np.array_equal(twin.get_state(), a.get_state()), "call %d: the restored context went its own way" % k
        for h, r in refs.items():
            chans = np.array([c for c in range(nch) if history[c] == h])
            switch(r, case, h[k], nfr)
            ref, _ = one_call(r, I[:, sl], Q[:, sl], **call)
            rs = sections(r)
            rdet, rtxt = results(r, nfr)
            rows = row_of[chans][row_of[chans] >= 0]
            assert np.array_equal(got[rows], ref[rows]), "call %d, mask %d: audio of channels %s" % (k, h[k], chans)
            assert set(rs) == set(after), (set(rs), set(after))
            for name in after:
                bad = chans[np.any(after[name][chans] != rs[name][chans], axis=1)]
                assert bad.size == 0, "call %d, mask %d: section %s of channels %s" % (k, h[k], name, bad)
            for bit, mine, theirs, sent in ((DET, det, rdet, np.float32(SENT_F)), (DEC, txt, rtxt, np.int32(SENT_I))):
                if mine is None:
                    continue
                if h[k] & bit:
                    assert np.array_equal(mine[chans], theirs[chans]), "call %d, mask %d: result rows of stage %d" % (k, h[k], bit)
                else:
                    assert (mine[chans] == sent).all(), "call %d, mask %d: stage %d wrote rows of channels it does not run on" % (k, h[k], bit)
        # a clear bit: the stage's records are what they were in front of the call; a set bit: the stage ran
        if k > 0:
            for bit in case.switches:
                name = SECTION_OF[bit]
                off = np.flatnonzero((eff[k] & bit) == 0)
                on = np.flatnonzero(eff[k] & bit)
                assert np.array_equal(after[name][off], before[name][off]), "call %d: stage %d moved the memory of a channel it does not run on" % (k, bit)
                if on.size:
                    assert np.any(after[name][on] != before[name][on], axis=1).all(), "call %d: stage %d left a listed channel's memory alone" % (k, bit)
        if checkpoint_after == k:
            twin = context(T, case, nfr, nch, **options)
            switch(twin, case, case.bits, nfr)
            twin.set_state(a.get_state())
    return a, eff, audio, (taps if tap else None)
