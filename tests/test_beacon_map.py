"""The beacon monitor under a panadapter map (t41rx_set_panadapter_map): BeaconLoop() on the listed channels only, each on the
smeter row its channel names; the table, the events and the record stay by channel.

GPU (-m gpu).  Every comparison is bit for bit against the library's own unmapped path, which test_beacon_monitor.py holds
to tests/beacon_model.py.  A row per frame (update_period 1), the fast clock of batch_harness.beacon_setup (one slot per
frame: every row past the first changes the beacon), modes 1 and 0; 5 channels with 2 listed, and 70 channels with 66
listed through a permuted map, so that the list crosses a wave and its last wave is ragged.  Calls of 4 + 6 frames.
With a slot per row every record is max - min of one dbm, so those cases do not depend on the dbm at all: the slow-clock
case beside them (four rows per slot, calls of 12 + 16 frames, a faded signal) has tables that are non-zero and differ from
channel to channel, and so sees WHICH smeter row a listed channel's lane reads.
"""
import functools

import numpy as np
import pytest

import group_harness as G
import siggen
from rx_harness import T, one_call  # noqa: F401  (T: a fixture)

pytestmark = pytest.mark.gpu

L = 2048
SPLITS = (4, 6)
FAST = (0, 10000, 1)          # batch_harness.beacon_setup's clock: a slot per row
SLOW, SLOW_SPLITS = (0, 2500, 1), (12, 16)  # four rows per slot, seven slots
FILL32 = np.frombuffer(bytes([0xA5] * 4), np.int32)[0]
WORDS, SNR = 8, 18


def shape(nch):
    """(row per channel, n_rows) of the two shapes"""
    if nch == 5:
        return [-1, 1, -1, -1, 0], 2
    rows = np.full(nch, -1, np.int64)
    listed = np.array([c for c in range(nch) if c not in (3, 17, 40, 69)])
    rows[listed] = (np.arange(len(listed)) * 29 + 7) % len(listed)  # 29 and 66 are coprime: a permutation
    assert sorted(rows[listed].tolist()) == list(range(66))
    return rows.tolist(), 66


@functools.lru_cache(maxsize=None)
def signal(nch, total=sum(SPLITS)):
    nco = siggen.nco_grid(nch, seed=77)
    I, Q = siggen.make_iq(nch, total * L, nco, mode=0, seed=78)
    I, Q = siggen.fade(I, Q, [(0.3, 2.0), (0.3, 0.05), (0.4, 1.5)])  # the dbm moves from row to row
    for a in (nco, I, Q):
        a.setflags(write=False)
    return nco, I, Q


class Run:
    def __init__(self, T, nch, mode, rows=None, n_rows=None, max_rows=max(SPLITS), counter=0, clock=FAST, total=sum(SPLITS)):
        self.nch = nch
        self.nco, self.I, self.Q = signal(nch, total)
        self.rx = rx = T.RxChain(nch, T.default_params(**G.USB), NCOFreq=self.nco)
        if rows is not None:
            rx.set_panadapter_map(rows, n_rows)
        self.bufs = G.panadapter(rx, max_rows, spectrumZoom=1, currentScale=1, update_period=1, outputs=["smeter", "pixel"])
        rx.set_panadapter_counter(counter)
        rx.set_beacon_clock(*clock)
        self.band = (np.arange(nch) * 3 + 1) % 5
        self.snr, self.ev = rx.set_beacon(True, mode, self.band, max_rows=max_rows)
        self.start = self.record()

    def record(self):
        """the record's per-channel part: [nch, 8 status words + 18 snr words]"""
        return self.rx.beacon_state()[32:].view(np.int32).reshape(self.nch, WORDS + SNR).copy()

    def call(self, f0, nfr):
        import torch
        self.ev.fill_(int(FILL32))
        one_call(self.rx, self.I[:, f0 * L:(f0 + nfr) * L], self.Q[:, f0 * L:(f0 + nfr) * L])
        torch.cuda.synchronize()
        return dict(events=self.ev.cpu().numpy().copy(), snr=self.rx.beacon_snr().view(np.int32).copy(), status=self.rx.beacon_status().copy(),
                    record=self.record())


def stream(run, splits=SPLITS):
    f0, out = 0, []
    for n in splits:
        out.append(run.call(f0, n))
        f0 += n
    return out


@functools.lru_cache(maxsize=None)
def reference(nch, mode):
    import t41_sdr_amd as T
    run = Run(T, nch, mode)
    ref = stream(run)
    # the reference is busy: every channel's words move in the first call (the walk over the bands: five rows from the
    # switch), beacons are recorded in the second, and the words differ from channel to channel (a band each).  With a
    # slot per row every record is max - min of one dbm: the table's values are zeros, the events say what was recorded
    assert all(not np.array_equal(ref[0]["record"][c], run.start[c]) for c in range(nch))
    assert (ref[1]["events"][:, :SPLITS[1], 0] >= 0).any(), "no beacon recorded"
    assert len({ref[1]["status"][c].tobytes() for c in range(nch)}) > 1
    return run.start, ref


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("nch", [5, 70])
def test_listed_channels_equal_the_unmapped_run(T, nch, mode):
    rows, n_rows = shape(nch)
    start, ref = reference(nch, mode)
    run = Run(T, nch, mode, rows, n_rows)
    assert np.array_equal(run.start, start)
    for k, got in enumerate(stream(run)):
        n = SPLITS[k]
        for c, r in enumerate(rows):
            if r >= 0:
                for name in ("snr", "status", "record"):
                    assert np.array_equal(got[name][c], ref[k][name][c]), "%s of channel %d (row %d), call %d" % (name, c, r, k)
                assert np.array_equal(got["events"][c, :n], ref[k]["events"][c, :n]), "events of channel %d, call %d" % (c, k)
                assert (got["events"][c, n:] == FILL32).all()
            else:
                assert np.array_equal(got["record"][c], start[c]), "the record of unlisted channel %d moved in call %d" % (c, k)
                assert not got["snr"][c].any() and (got["events"][c] == FILL32).all(), "unlisted channel %d was written in call %d" % (c, k)


@functools.lru_cache(maxsize=None)
def slow_reference(nch):
    """the unmapped context on the slow clock: the tables must carry the dbm, or the comparison below sees nothing"""
    import t41_sdr_amd as T
    run = Run(T, nch, 1, max_rows=max(SLOW_SPLITS), clock=SLOW, total=sum(SLOW_SPLITS))
    ref = stream(run, SLOW_SPLITS)
    snr = ref[-1]["snr"].view(np.float32)
    assert all(snr[c].any() for c in range(nch)), "a channel's table is all zero: its records do not depend on the dbm"
    assert len({snr[c].tobytes() for c in range(nch)}) == nch, "two channels have the same table"
    smeter = run.bufs["smeter"].cpu().numpy()[:, :SLOW_SPLITS[1], 3]
    assert len({smeter[c].tobytes() for c in range(nch)}) == nch, "two channels have the same dbm rows"
    return run.start, ref


@pytest.mark.parametrize("nch", [5, 70])
def test_a_listed_channel_reads_the_smeter_row_it_names(T, nch):
    """four rows per slot and a faded signal: every record is max - min over several dbm of the channel's own smeter rows,
    non-zero and different from channel to channel (slow_reference asserts both), so a lane that reads the smeter by
    channel, or any row but the one its channel names, gets another table"""
    rows, n_rows = shape(nch)
    start, ref = slow_reference(nch)
    run = Run(T, nch, 1, rows, n_rows, max_rows=max(SLOW_SPLITS), clock=SLOW, total=sum(SLOW_SPLITS))
    for k, got in enumerate(stream(run, SLOW_SPLITS)):
        n = SLOW_SPLITS[k]
        for c, r in enumerate(rows):
            if r >= 0:
                for name in ("snr", "status", "record"):
                    assert np.array_equal(got[name][c], ref[k][name][c]), "%s of channel %d (row %d), call %d" % (name, c, r, k)
                assert np.array_equal(got["events"][c, :n], ref[k]["events"][c, :n]), "events of channel %d, call %d" % (c, k)
            else:
                assert np.array_equal(got["record"][c], start[c]), "the record of unlisted channel %d moved in call %d" % (c, k)
                assert not got["snr"][c].any() and (got["events"][c] == FILL32).all(), "unlisted channel %d was written in call %d" % (c, k)


@pytest.mark.parametrize("mode", [1, 0])
def test_split_calls_equal_one_call(T, mode):
    rows, n_rows = shape(70)
    listed = np.flatnonzero(np.asarray(rows) >= 0)
    two = stream(Run(T, 70, mode, rows, n_rows, max_rows=sum(SPLITS)))
    one = stream(Run(T, 70, mode, rows, n_rows, max_rows=sum(SPLITS)), (sum(SPLITS),))[0]
    assert np.array_equal(two[1]["record"], one["record"])
    events = np.concatenate([two[0]["events"][:, :SPLITS[0]], two[1]["events"][:, :SPLITS[1]]], axis=1)
    assert np.array_equal(events[listed], one["events"][listed, :sum(SPLITS)])


def test_the_record_continues_in_a_fresh_mapped_context(T):
    """call 1 in one mapped context; its beacon record and its checkpoint go to a fresh mapped context whose panadapter
    counter is set to 4; call 2 there gives the listed channels what call 2 gives them in the first context (the beacon
    reads the smeter's dbm, which is a function of the path's state and not of the panadapter memory)"""
    rows, n_rows = shape(5)
    a = Run(T, 5, 1, rows, n_rows)
    first = a.call(0, SPLITS[0])
    rec, state = a.rx.beacon_state(), a.rx.get_state()
    want = a.call(SPLITS[0], SPLITS[1])
    b = Run(T, 5, 1, rows, n_rows, counter=SPLITS[0])
    b.rx.set_state(state)
    b.rx.set_beacon_state(rec)
    assert np.array_equal(b.record(), first["record"])
    got = b.call(SPLITS[0], SPLITS[1])
    for name in ("record", "snr", "status", "events"):
        assert np.array_equal(got[name], want[name]), name
    # a channel listed later continues from the record it has: channel 0 joins for a third call with the words it was given
    b.rx.set_panadapter_map([1, -1, -1, -1, 0], n_rows)
    before = b.record()
    assert np.array_equal(before[0], first["record"][0]) and np.array_equal(before[0], a.start[0])
    after = b.call(0, SPLITS[0])
    assert not np.array_equal(after["record"][0], before[0]) and np.array_equal(after["record"][1], before[1])
