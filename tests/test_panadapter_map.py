"""The panadapter map (t41rx_set_panadapter_map): the panadapter stage only on the channels that ask, a row of the seven row
buffers per listed channel.

GPU (-m gpu).  Every comparison is bit for bit against the library's own path WITHOUT a map, which test_panadapter.py holds
to tests/panadapter_model.py: a listed channel's rows of all seven buffers are those of the same channel of the unmapped
context, in the row the map names; rows >= k of a call with k update frames and rows nobody names keep the 0xA5 they were
filled with; a listed channel's part of the checkpoint is the unmapped context's, an unlisted one's that of a context with
the stage off (audioMaxSquaredAve did not move); the audio is the audio with the stage off.  The panadapter memory has no
getter: that it stays for an unlisted channel and advances for a listed one shows in the rows of the call after.

5 channels, calls of 7 + 9 frames, update_period 3, update_phase 1, max_rows 3: the first call's update frames are its
frames 1 and 4 (two rows, row 2 of every named row stays 0xA5), the second call's its frames 0, 3 and 6 (7 % 3 == 1: three
rows, all of max_rows).  Every channel has a noise floor and a gain correction of its own, so that a level read by row
instead of by channel shows.
"""
import functools

import numpy as np
import pytest

import group_harness as G
import siggen
from rx_harness import ERR_ARG, ERR_UNSUPPORTED, T, bits, one_call, refused, same  # noqa: F401  (T: a fixture)

pytestmark = pytest.mark.gpu

L = 2048
NCH, SPLITS = 5, (7, 9)
PERIOD, PHASE, MAXR = 3, 1, 3
FILL = 0xA5
MAX_SQ_AVE = 184 + 12  # audioMaxSquaredAve in a channel's record (kStMisc + kMiscMaxSqAve)
# row per channel, rows: 1 of 5; 2 of 5 with the rows permuted and row 1 named by nobody; all 5 permuted
MAPS = {"1_of_5": ([-1, -1, -1, 0, -1], 1), "2_of_5": ([-1, 2, -1, -1, 0], 3), "all_5": ([3, 0, 4, 1, 2], 5)}
NAMES = ("pixel", "y_new", "y_old", "waterfall", "spec", "audio_spect", "smeter")
NOISE_FLOOR = np.array([3, -2, 5, 0, 7, 1, -4], np.int32)
GAIN_CORRECTION = np.array([1.5, -2.0, 6.0, 0.25, -0.75, 3.0, 2.5], np.float32)
SEED = 0x50414E


def rows_of(n0, nfr):
    """the call's update frames' number: frames f with (n0 + f) % PERIOD == PHASE"""
    return sum(1 for f in range(nfr) if (n0 + f) % PERIOD == PHASE)


@functools.lru_cache(maxsize=None)
def signal(nch=NCH, nfr=sum(SPLITS) + 6, seed=SEED):
    nco = siggen.nco_grid(nch, seed=seed & 0xFFFF)
    I, Q = siggen.make_iq(nch, nfr * L, nco, mode=0, seed=seed & 0xFFFF)
    for a in (nco, I, Q):
        a.setflags(write=False)
    return nco, I, Q


class Run:
    """a context with, in this order: the layout, setup(rx), the parameter sets, the panadapter map, the panadapter on with
    every row buffer and the levels.  call(f0, nfr) fills the row buffers with 0xA5, runs frames f0 .. f0 + nfr of the
    signal and returns (audio, {name: the buffer's bytes [rows, MAXR, bytes per row]})"""

    def __init__(self, T, entry="f32", rows=None, n_rows=None, on=True, zoom=0, setup=None, sets=None, setof=None, stages=False,
                 nch=NCH, shared=False, **params):
        self.entry, self.nch, self.shared = entry, nch, shared
        self.nco, self.I, self.Q = signal(nch)
        self.rx = T.RxChain(nch, T.default_params(**dict(G.USB, **params)), NCOFreq=self.nco)
        self.zoom, self.bufs = zoom, None
        if entry == "time":
            self.rx.set_buffer_layout("time")
        self.keep = setup(self.rx) if setup else None
        if sets is not None:
            self.rx.set_param_sets([T.default_params(**s) for s in sets], setof, stages=stages)
        if rows is not None:
            self.rx.set_panadapter_map(rows, n_rows)
        if on:
            self.switch_on()

    def switch_on(self):
        self.bufs = G.panadapter(self.rx, MAXR, spectrumZoom=self.zoom, currentScale=1, update_period=PERIOD, update_phase=PHASE)
        self.rx.set_panadapter_levels(NOISE_FLOOR[:self.nch], GAIN_CORRECTION[:self.nch], attenuator=3)

    def snap(self):
        import torch
        torch.cuda.synchronize()
        return {k: t.contiguous().view(torch.uint8).cpu().numpy().reshape(t.shape[0], MAXR, -1) for k, t in self.bufs.items()}

    def call(self, f0, nfr):
        import torch
        if self.bufs:
            for t in self.bufs.values():
                t.view(torch.uint8).fill_(FILL)
        sl = slice(f0 * L, (f0 + nfr) * L)
        I, Q = (self.I[:1, sl], self.Q[:1, sl]) if self.shared else (self.I[:, sl], self.Q[:, sl])
        audio, _ = one_call(self.rx, I, Q, q15_scale=1.0 if self.entry == "q15" else None)
        return audio, (self.snap() if self.bufs else None)

    def records(self):
        return bits(self.rx.state_records()).copy()


def stream(run, splits=SPLITS, between=None):
    """the signal in calls of `splits` frames: [(audio, rows, records) per call]; between(run, k) in front of call k > 0"""
    f0, out = 0, []
    for k, n in enumerate(splits):
        if k and between:
            between(run, k)
        audio, got = run.call(f0, n)
        out.append((audio, got, run.records()))
        f0 += n
    return out


@functools.lru_cache(maxsize=None)
def reference(entry, zoom):
    """the unmapped context with the stage on, and the context with the stage off: per call audio, rows, records"""
    import t41_sdr_amd as T
    on, off = stream(Run(T, entry, zoom=zoom)), stream(Run(T, entry, on=False))
    f0 = 0
    for k, n in enumerate(SPLITS):  # the reference does what the shapes were chosen for
        kr = rows_of(f0, n)
        assert kr == (2, 3)[k]
        for name in NAMES:
            assert (on[k][1][name][:, kr:] == FILL).all() and not (on[k][1][name][:, :kr] == FILL).all(), name
        assert same(on[k][0], off[k][0])
        assert not np.array_equal(on[k][2][:, MAX_SQ_AVE], off[k][2][:, MAX_SQ_AVE])
        f0 += n
    return on, off


def check(got, rows, n_rows, on, off, k, kr, what=NAMES):
    """call k of a mapped stream: listed channels are the unmapped context's in their rows, the rest of the buffers was not
    written, the records are the unmapped context's for the listed channels and the stage-off context's for the others"""
    audio, bufs, rec = got
    for name in what:
        b = bufs[name]
        assert b.shape[0] == n_rows, (name, b.shape)
        for c, r in enumerate(rows):
            if r >= 0:
                assert np.array_equal(b[r, :kr], on[k][1][name][c, :kr]), "%s of channel %d (row %d), call %d" % (name, c, r, k)
                assert (b[r, kr:] == FILL).all(), "%s: rows >= %d of row %d were written in call %d" % (name, kr, r, k)
        for r in sorted(set(range(n_rows)) - {r for r in rows if r >= 0}):
            assert (b[r] == FILL).all(), "%s: row %d has no channel and was written in call %d" % (name, r, k)
    assert same(audio, off[k][0]), "the audio moved in call %d" % k
    for c, r in enumerate(rows):
        want = on[k][2][c] if r >= 0 else off[k][2][c]
        assert np.array_equal(rec[c], want), "the record of %s channel %d, call %d" % ("listed" if r >= 0 else "unlisted", c, k)


@pytest.mark.parametrize("which", sorted(MAPS))
@pytest.mark.parametrize("entry,zoom", [("f32", 0), ("f32", 2), ("q15", 0), ("time", 0)])
def test_listed_channels_equal_the_unmapped_run(T, entry, zoom, which):
    rows, n_rows = MAPS[which]
    on, off = reference(entry, zoom)
    run = Run(T, entry, rows, n_rows, zoom=zoom)
    assert run.rx.panadapter_rows == n_rows and run.rx.panadapter_map.tolist() == rows
    assert all(t.shape[0] == n_rows for t in run.bufs.values())
    f0 = 0
    for k, got in enumerate(stream(run)):
        check(got, rows, n_rows, on, off, k, rows_of(f0, SPLITS[k]))
        f0 += SPLITS[k]
    assert run.rx.panadapter_status() == (True, sum(SPLITS), 3, 7)


@pytest.mark.parametrize("zoom", [0, 2])
def test_memory_stays_for_an_unlisted_channel(T, zoom):
    """channel 1 is unlisted in call 1 and listed (same n_rows) in call 2: its call-2 rows are those of a context that ran
    call 1 with the stage off, then switched the panadapter on -- zeroed memory, which is what the mapped channel's
    untouched memory still is -- at frame counter 7"""
    first, second = [-1, -1, 0, -1, 1], [1, 2, 0, -1, -1]
    run = Run(T, rows=first, n_rows=3, zoom=zoom)
    got = stream(run, between=lambda r, k: r.rx.set_panadapter_map(second, 3))
    ref = Run(T, on=False, zoom=zoom)
    ref.call(0, SPLITS[0])
    ref.switch_on()
    ref.rx.set_panadapter_counter(SPLITS[0])
    _, want = ref.call(SPLITS[0], SPLITS[1])
    kr = rows_of(SPLITS[0], SPLITS[1])
    for name in NAMES:
        assert np.array_equal(got[1][1][name][2, :kr], want[name][1, :kr]), name
        assert not (want[name][1, :kr] == FILL).all()
    # ... and channel 2, listed in both calls and moved from row 0 to row 0, goes on as in one unmapped stream
    on, off = reference("f32", zoom)
    for name in NAMES:
        assert np.array_equal(got[1][1][name][0, :kr], on[1][1][name][2, :kr]), name
    # the channel that joined differs from the unmapped stream's: that one's memory had advanced in call 1
    assert not np.array_equal(got[1][1]["y_old"][2, :kr], on[1][1]["y_old"][1, :kr])


def test_memory_stays_while_a_channel_is_unlisted(T):
    """The reverse: channel 3 is listed in call 1, unlisted in call 2 and listed again for a third call of 6 frames.  The
    reference is built from two unmapped contexts, as the case asks: S runs call 1 with the stage on, switches it off and
    runs call 2 -- its checkpoint then holds the path after both calls with audioMaxSquaredAve advanced by call 1's update
    frames only; P runs call 1 with the stage on -- its panadapter memory has seen call 1's rows only --, takes S's
    checkpoint (t41rx_set_state leaves the panadapter memory alone), sets the frame counter to 16 and runs call 3.  The
    mapped channel's rows of call 3 are P's."""
    splits = SPLITS + (6,)
    maps = ([-1, 1, -1, 0, -1], [-1, 1, -1, -1, -1], [-1, -1, 1, 0, -1])
    run = Run(T, rows=maps[0], n_rows=2, zoom=2)
    got = stream(run, splits, between=lambda r, k: r.rx.set_panadapter_map(maps[k], 2))
    s = Run(T, zoom=2)
    s.call(0, SPLITS[0])
    s.rx.set_beacon(False)
    s.rx.set_panadapter(False)
    s.bufs = None
    s.call(SPLITS[0], SPLITS[1])
    p = Run(T, zoom=2)
    p.call(0, SPLITS[0])
    p.rx.set_state(s.rx.get_state())
    p.rx.set_panadapter_counter(sum(SPLITS))
    _, want = p.call(sum(SPLITS), 6)
    kr = rows_of(sum(SPLITS), 6)
    assert kr == 2
    for name in NAMES:
        assert np.array_equal(got[2][1][name][0, :kr], want[name][3, :kr]), name
        assert (got[2][1][name][0, kr:] == FILL).all()
    # a channel that saw call 2's update frames differs: the case has teeth
    on = stream(Run(T, zoom=2), splits)
    assert not np.array_equal(on[2][1]["smeter"][3, :kr], want["smeter"][3, :kr])
    assert np.array_equal(got[2][2][3], bits(p.rx.state_records())[3])


def test_nobody_listed(T):
    """a map of -1s: no row is written, the records are those of the stage-off context, the counter counts"""
    on, off = reference("f32", 0)
    run = Run(T, rows=[-1] * NCH, n_rows=2)
    for k, (audio, bufs, rec) in enumerate(stream(run)):
        assert all((b == FILL).all() for b in bufs.values())
        assert np.array_equal(rec, off[k][2]) and same(audio, off[k][0])
    assert run.rx.panadapter_status()[:2] == (True, sum(SPLITS))


def test_with_the_other_maps(T):
    """one shared stream (input map), an output map that mutes the displayed channel, a stage map with the equalizer on
    another channel: the listed channel's rows are those of the context with the same maps and no panadapter map"""
    import eq_model as EQM
    import test_receive_eq as E

    def setup(rx):
        rx.set_input_map([0] * NCH, 1)
        rx.set_output_map([0, 1, -1, 2, 3], 4)
        rx.set_receive_eq_bands(EQM.bands())
        rx.set_receive_eq(1, E.RAMP)
        rx.set_stage_map([0, T.STAGE_EQ, 0, 0, 0])

    ref = stream(Run(T, setup=setup, shared=True))
    off = stream(Run(T, setup=setup, shared=True, on=False))
    rows, n_rows = [-1, -1, 1, -1, -1], 2
    f0 = 0
    for k, (audio, bufs, rec) in enumerate(stream(Run(T, rows=rows, n_rows=n_rows, setup=setup, shared=True))):
        kr = rows_of(f0, SPLITS[k])
        f0 += SPLITS[k]
        for name in NAMES:
            assert np.array_equal(bufs[name][1, :kr], ref[k][1][name][2, :kr]), name
            assert (bufs[name][1, kr:] == FILL).all() and (bufs[name][0] == FILL).all(), name
        assert same(audio, off[k][0]) and same(audio, ref[k][0])
        assert np.array_equal(rec[2], ref[k][2][2]) and np.array_equal(rec[[0, 1, 3, 4]], off[k][2][[0, 1, 3, 4]])


BASE = dict(rfGainAllBands=3, RFgain=2, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=0.01)
EXTRA = [dict(BASE, rfGainAllBands=-4, RFgain=3), dict(BASE, rfGainAllBands=8, RFgain=1, IQAmpCorrectionFactor=1.0, IQPhaseCorrectionFactor=0.03)]
SET_OF = [1, 0, 2, 2, 1]


@pytest.mark.parametrize("stages", [False, True], ids=["plain", "staged"])
def test_parameter_sets_with_their_own_gains(T, stages):
    """sets that differ in RFgain / rfGainAllBands: without a map the call is refused as ever; with one each listed
    channel's rows -- the smeter's dbm among them -- equal those of a context created with that channel's set"""
    kw = dict(sets=[dict(G.USB, **e) for e in EXTRA], setof=SET_OF, stages=stages)
    plain = Run(T, **dict(kw, **BASE))
    refused(lambda: plain.call(0, SPLITS[0]), ERR_UNSUPPORTED, "S-meter", "RFgain")
    rows, n_rows = [2, 0, -1, 3, 1], 4  # channels of set 1, 0, 2, 1
    got = stream(Run(T, rows=rows, n_rows=n_rows, **dict(kw, **BASE)))
    refs = [stream(Run(T, **p)) for p in [BASE] + EXTRA]
    dbm = []
    f0 = 0
    for k in range(len(SPLITS)):
        kr = rows_of(f0, SPLITS[k])
        f0 += SPLITS[k]
        for c, r in enumerate(rows):
            if r < 0:
                continue
            for name in NAMES:
                assert np.array_equal(got[k][1][name][r, :kr], refs[SET_OF[c]][k][1][name][c, :kr]), (name, c, k)
            dbm.append(got[k][1]["smeter"][r, 0].view(np.float32)[3])
        assert (got[k][1]["smeter"][:, kr:] == FILL).all()
    # the sets' gains show: the same channel's dbm under set 0 differs
    assert not np.array_equal(refs[0][0][1]["smeter"][0, :2], refs[1][0][1]["smeter"][0, :2])
    assert np.isfinite(dbm).all()
    # set 0 changes: the listed channels of set 0 follow it (t41rx_set_params makes the list again)
    run = Run(T, rows=rows, n_rows=n_rows, **dict(kw, **BASE))
    run.rx.CalcFilters(rfGainAllBands=5)
    moved = stream(Run(T, **dict(BASE, rfGainAllBands=5)), SPLITS[:1])
    _, bufs = run.call(0, SPLITS[0])
    assert np.array_equal(bufs["smeter"][0, :2], moved[0][1]["smeter"][1, :2])
    assert np.array_equal(bufs["smeter"][2, :2], refs[1][0][1]["smeter"][0, :2])


def test_refusals(T):
    run = Run(T, rows=[-1, 2, -1, -1, 0], n_rows=3)
    rx = run.rx
    kept = rx.panadapter_map.tolist()

    def held(fn, status, *words):
        refused(fn, status, *words)
        assert rx.panadapter_map.tolist() == kept and rx.panadapter_rows == 3

    lib, ctx = rx._lib, rx._ctx
    import ctypes as C
    arr = lambda v: (C.c_int32 * len(v))(*v)  # noqa: E731
    raw = lambda v, n, r: T.rx.check(lib.t41rx_set_panadapter_map(ctx, arr(v), n, r))  # noqa: E731
    held(lambda: raw([0, 1, 2, -1], 4, 3), ERR_ARG, "n (4) must equal n_channels")
    held(lambda: raw([0, 1, 2, -1, -1, -1], 6, 3), ERR_ARG, "n (6) must equal n_channels")
    held(lambda: T.rx.check(lib.t41rx_set_panadapter_map(ctx, None, 5, 3)), ERR_ARG, "null map")
    held(lambda: rx.set_panadapter_map([0, -1, -1, -1, -1], 0), ERR_ARG, "n_rows (0) must be 1 .. n_channels")
    held(lambda: rx.set_panadapter_map([0, -1, -1, -1, -1], 6), ERR_ARG, "n_rows (6) must be 1 .. n_channels")
    held(lambda: rx.set_panadapter_map([0, -1, 3, -1, -1], 3), ERR_ARG, "channel 2 has row 3")
    held(lambda: rx.set_panadapter_map([0, -2, 1, -1, -1], 3), ERR_ARG, "channel 1 has row -2")
    held(lambda: rx.set_panadapter_map([0, -1, 1, 0, -1], 3), ERR_ARG, "row 0 is named twice, by channel 0 and channel 3")
    # the stage is on: the rows are fixed, in both directions and for the map's removal
    held(lambda: rx.set_panadapter_map([0, -1, 1, -1, -1], 2), ERR_ARG, "n_rows (2) differs from the current rows")
    held(lambda: rx.set_panadapter_map([0, -1, 1, -1, -1], 4), ERR_ARG, "n_rows (4) differs from the current rows")
    held(lambda: T.rx.check(lib.t41rx_set_panadapter_map(ctx, None, 0, 0)), ERR_ARG, "removing the map would change the rows")
    # at equal rows the map changes; switched off, the rows change; the beacon monitor holds the switch
    rx.set_panadapter_map([0, -1, 1, -1, 2], 3)
    kept = [0, -1, 1, -1, 2]
    rx.set_beacon_clock(0, 10000, 1)
    rx.set_beacon(True, 1, [0, 1, 2, 3, 4])
    refused(lambda: rx.set_panadapter(False), ERR_UNSUPPORTED, "beacon monitor")
    held(lambda: rx.set_panadapter_map([0, -1, 1, -1, -1], 2), ERR_ARG, "differs from the current rows")
    rx.set_beacon(False)
    rx.set_panadapter(False)
    rx.set_panadapter_map([0, -1, 1, -1, -1], 2)
    assert rx.panadapter_rows == 2
    run.switch_on()
    assert all(t.shape[0] == 2 for t in run.bufs.values())
    # the map survives reset, set_state and CalcFilters
    state = rx.get_state()
    rx.reset()
    rx.set_state(state)
    rx.CalcFilters(FHiCut=2800)
    assert rx.panadapter_map.tolist() == [0, -1, 1, -1, -1] and rx.panadapter_rows == 2
    rx.set_panadapter(False)
    rx.set_panadapter_map(None)
    assert rx.panadapter_map is None and rx.panadapter_rows == NCH
    # a long fft_length
    nco = siggen.nco_grid(2, seed=3)
    lng = T.RxChain(2, T.default_params(fft_length=1024, **G.USB), NCOFreq=nco)
    refused(lambda: lng.set_panadapter_map([0, -1], 1), ERR_UNSUPPORTED, "fft_length 512")
