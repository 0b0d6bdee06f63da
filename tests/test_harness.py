"""The test support code itself (tests/rx_harness.py, tests/group_harness.py, tests/stage_reference.py), without a device:
layouts, sample formats, the (Q, I) order of the q15 entry points, a stream cut into calls against a stub chain, one call
on a stub receiver group (rows, frame length and layout from the chain; the guard), the group tests' checkers made to
fail, and the reference interpolators against the oracle's primitive called directly."""
from types import SimpleNamespace

import numpy as np
import pytest

import group_harness as G
import oracle_lib as O
from rx_harness import (GUARD, INT1, INT2, SENT_F32, SENT_Q15, bits, calls, from_time_major, one_call, pack, same, sentinel_of,
                        streams, to_q15, to_time_major)
from stage_reference import interp, vol_scale


class Stub:
    """records what it is given and returns its I input (the second argument of the q15 entry point)"""
    frame_len, n_channels = 8, 3

    def __init__(self):
        self.seen = []

    def ProcessIQData(self, i, q):
        self.seen.append(("f32", i, q))
        return i.copy()

    def ProcessIQData_q15(self, q, i):
        self.seen.append(("q15", q, i))
        return i.copy()


def stream(nch, nfr, L, seed=1):
    rng = np.random.default_rng(seed)
    return (0.5 * rng.standard_normal((nch, nfr * L))).astype(np.float32), (0.5 * rng.standard_normal((nch, nfr * L))).astype(np.float32)


@pytest.mark.parametrize("nch,nfr", [(1, 1), (3, 2), (9, 5)])
def test_time_major_round_trip(nch, nfr):
    L = 16
    x, _ = stream(nch, nfr, L)
    t = to_time_major(x, nch, nfr, L)
    assert t.shape == (nfr, nch, L) and t.flags["C_CONTIGUOUS"] and t.dtype == x.dtype
    for f in range(nfr):
        for c in range(nch):
            assert np.array_equal(t[f, c], x[c, f * L:(f + 1) * L])
    assert np.array_equal(from_time_major(t, nch, nfr, L), x)


def test_pack_order_and_formats():
    L = 8
    i, q = stream(3, 2, L)
    a, b = pack(i[:, :L], q[:, :L], "channel", None, L)  # a slice: not contiguous on the way in
    assert a.flags["C_CONTIGUOUS"] and b.flags["C_CONTIGUOUS"] and a.dtype == b.dtype == np.float32
    assert np.array_equal(a, i[:, :L]) and np.array_equal(b, q[:, :L])
    a, b = pack(i, q, "channel", 1 / 4, L)  # q15: (Q, I)
    assert a.dtype == b.dtype == np.int16 and np.array_equal(a, to_q15(q, 1 / 4)) and np.array_equal(b, to_q15(i, 1 / 4))
    assert not np.array_equal(a, b)
    a, b = pack(to_q15(i), to_q15(q), "channel", None, L)  # int16 given: the same order
    assert np.array_equal(a, to_q15(q)) and np.array_equal(b, to_q15(i))
    a, b = pack(i, q, "time", 1.0, L)
    assert a.shape == (2, 3, L) and a.flags["C_CONTIGUOUS"] and np.array_equal(a, to_time_major(to_q15(q), 3, 2, L))
    assert np.array_equal(b, to_time_major(to_q15(i), 3, 2, L))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_to_q15_rounds_half_to_even_and_saturates(dtype):
    """numpy.round's documented rule (values exactly half way between two integers go to the even one), then the clip"""
    x = np.array([1.0, -1.0, 32767.5, -32768.5, 0.5, 1.5, 2.5, -0.5, -1.5, 32766.5, 0.0], np.float64) / np.array(
        [1, 1] + [32768.0] * 9)
    assert np.array_equal(x.astype(dtype).astype(np.float64), x)  # every value is exact in float32 as well
    want = [32767, -32768, 32767, -32768, 0, 2, 2, 0, -2, 32766, 0]  # 32767.5 -> 32768 -> clipped; -32768.5 -> -32768
    got = to_q15(x.astype(dtype))
    assert got.dtype == np.int16 and got.tolist() == want
    assert to_q15(x.astype(dtype) * 4, 1 / 4).tolist() == want and to_q15(x.astype(dtype) * 64, 1 / 64).tolist() == want


@pytest.mark.parametrize("layout", ["channel", "time"])
@pytest.mark.parametrize("q15", [False, True])
def test_calls_reassemble_the_uncut_stream(layout, q15):
    rx = Stub()
    L, nch, nfr = rx.frame_len, rx.n_channels, 5
    I, Q = stream(nch, nfr, L)
    opts = dict(layout=layout, q15_scale=1.0 if q15 else None, host=True)
    whole, tap = one_call(rx, I, Q, **opts)
    assert tap is None and np.array_equal(whole, to_q15(I) if q15 else I)
    cut = Stub()
    edges = [0, 1, 3, 5]
    got, tap, seen = calls(cut, I, Q, edges, after=lambda rx, a, b: (rx is cut, a, b, len(rx.seen)), **opts)
    assert tap is None and got.shape == whole.shape and np.array_equal(got, whole)
    assert seen == [(True, 0, 1, 1), (True, 1, 3, 2), (True, 3, 5, 3)]  # once per call, behind it
    assert len(cut.seen) == 3
    for (a, b), (entry, first, second) in zip(zip(edges[:-1], edges[1:]), cut.seen):
        i, q = I[:, a * L:b * L], Q[:, a * L:b * L]
        if q15:
            i, q = to_q15(i), to_q15(q)
        if layout == "time":
            i, q = to_time_major(i, nch, b - a, L), to_time_major(q, nch, b - a, L)
        assert entry == ("q15" if q15 else "f32") and first.flags["C_CONTIGUOUS"] and second.flags["C_CONTIGUOUS"]
        assert np.array_equal(first, q if q15 else i) and np.array_equal(second, i if q15 else q)


class GroupStub:
    """a numpy model of a receiver group in the shapes one_call() reads from a chain: channel c takes samples c .. c + 2
    of every frame of stream STREAM_OF[c]'s I and writes them to row ROW_OF[c] of the audio, or with -1 nowhere; row 1
    has no channel.  fault: "behind" writes one sample behind out's rows, "copy" returns another object than out, "shape"
    returns the input's shape."""
    frame_len, audio_frame_len, n_channels, n_streams, audio_rows = 8, 2, 5, 3, 4
    STREAM_OF, ROW_OF, UNUSED = (2, 0, 1, 0, 2), (3, -1, 0, -1, 2), 1

    def __init__(self, layout="channel", fault=None):
        self.layout, self.fault, self.seen = layout, fault, []

    def ProcessIQData(self, i, q, out=None):
        return self.process("f32", i, q, i, out)

    def ProcessIQData_q15(self, q, i, out=None):
        return self.process("q15", q, i, i, out)

    def process(self, entry, first, second, i, out):
        self.seen.append((entry, first, second, out))
        L, La, time = self.frame_len, self.audio_frame_len, self.layout == "time"
        nfr = i.shape[0] if time else i.shape[1] // L
        if out is None:
            out = np.zeros((nfr, self.audio_rows, La) if time else (self.audio_rows, nfr * La), i.dtype)
        for c, (s, r) in enumerate(zip(self.STREAM_OF, self.ROW_OF)):
            for f in range(nfr if r >= 0 else 0):
                if time:
                    out[f, r] = i[f, s, c:c + La]
                else:
                    out[r, f * La:(f + 1) * La] = i[s, f * L + c:f * L + c + La]
        if self.fault == "behind":
            out.base[out.size] = 0  # (out is a view of the guarded buffer's front)
        return {"copy": out.copy(), "shape": np.zeros(i.shape, i.dtype)}.get(self.fault, out)


@pytest.mark.parametrize("guard", [False, True], ids=["plain", "guard"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("layout", ["channel", "time"])
def test_one_call_takes_rows_frame_length_and_layout_from_the_chain(layout, q15, guard):
    """3 streams in, 5 channels, 4 rows out with one unused, 2 frames of 8 samples in and 2 out: the host form, with the
    layout left to the chain"""
    rx, nfr = GroupStub(layout), 2
    I, Q = streams(rx.n_streams, nfr * rx.frame_len, 7, q15)
    assert I.dtype == (np.int16 if q15 else np.float32) and len({r.tobytes() for r in np.concatenate([I, Q])}) == 2 * rx.n_streams
    got, tap = one_call(rx, I, Q, host=True, guard=guard)
    (entry, first, second, out), = rx.seen
    want_in = (nfr, rx.n_streams, rx.frame_len) if layout == "time" else (rx.n_streams, nfr * rx.frame_len)
    assert entry == ("q15" if q15 else "f32") and first.shape == second.shape == want_in  # the input's rows, not n_channels
    assert np.array_equal(first, pack(I, Q, layout, None, rx.frame_len)[0])
    if guard:
        assert out.shape == ((nfr, rx.audio_rows, rx.audio_frame_len) if layout == "time" else (rx.audio_rows, nfr * rx.audio_frame_len))
        assert out.dtype == I.dtype
    else:
        assert out is None
    want = np.full((rx.audio_rows, nfr * rx.audio_frame_len), sentinel_of(I) if guard else 0, I.dtype)  # what nobody writes
    for c, (s, r) in enumerate(zip(rx.STREAM_OF, rx.ROW_OF)):
        if r >= 0:
            want[r] = I[s].reshape(nfr, rx.frame_len)[:, c:c + rx.audio_frame_len].reshape(-1)
    assert tap is None and got.dtype == I.dtype and np.array_equal(got, want) and rx.UNUSED not in rx.ROW_OF
    assert np.array_equal(one_call(GroupStub(layout), I, Q, layout=layout, host=True, guard=guard)[0], got)  # given = the chain's own


@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("layout", ["channel", "time"])
def test_guard_and_shape_checks_fail_when_they_should(layout, q15):
    assert (SENT_F32, SENT_Q15, GUARD) == (np.float32(-7777.25), np.int16(0x5A5A), 512) and SENT_Q15.dtype == np.int16
    I, Q = streams(GroupStub.n_streams, 2 * GroupStub.frame_len, 8, q15)
    one_call(GroupStub(layout), I, Q, host=True, guard=True)  # (the stub without a fault passes)
    with pytest.raises(AssertionError, match="behind"):
        one_call(GroupStub(layout, "behind"), I, Q, host=True, guard=True)
    with pytest.raises(AssertionError):
        one_call(GroupStub(layout, "copy"), I, Q, host=True, guard=True)  # equal values in another object
    with pytest.raises(AssertionError):
        one_call(GroupStub(layout, "shape"), I, Q, host=True)
    one_call(GroupStub(layout, "copy"), I, Q, host=True)  # (without out= any object of the right shape is the result)


@pytest.mark.parametrize("dtype", [np.float32, np.int16], ids=["f32", "q15"])
def test_check_rows_fails_when_it_should(dtype):
    ref = np.random.default_rng(9).integers(1, 1000, (GroupStub.n_channels, 6)).astype(dtype)  # per channel, no sample zero
    omap, nrows = np.array(GroupStub.ROW_OF, np.int32), GroupStub.audio_rows
    got = np.full((nrows, 6), sentinel_of(ref), dtype)
    got[omap[omap >= 0]] = ref[omap >= 0]
    G.check_rows(got, ref, omap, nrows)
    bad = got.copy()
    bad[[0, 3]] = bad[[3, 0]]  # two listened rows swapped
    with pytest.raises(AssertionError, match="channel 0, row 3"):
        G.check_rows(bad, ref, omap, nrows)
    bad = got.copy()
    bad[GroupStub.UNUSED, 5] = 0  # one sample of the row nobody names
    with pytest.raises(AssertionError, match="row 1 has no channel"):
        G.check_rows(bad, ref, omap, nrows)
    zero, bad = ref.copy(), got.copy()
    zero[2] = bad[omap[2]] = 0  # equal, and nothing was compared
    with pytest.raises(AssertionError):
        G.check_rows(bad, zero, omap, nrows)
    with pytest.raises(AssertionError):
        G.check_rows(got.astype(np.float64), ref, omap, nrows)
    with pytest.raises(AssertionError):
        G.check_rows(got[:3], ref, omap, nrows)
    with pytest.raises(AssertionError):
        G.check_rows(got, ref, omap, nrows + 1)


def test_rows_equal_fails_for_the_channels_own_set_only():
    setof = np.array([2, 0, 1, 0, 2], np.int32)
    got = np.random.default_rng(10).standard_normal((5, 6)).astype(np.float32)
    got[2, 1] = np.array([0x7FC00001], np.uint32).view(np.float32)[0]  # a NaN word, as a state record may hold
    refs = [got.copy() for _ in range(3)]
    G.rows_equal(got, refs, setof, "rows")
    refs[1][0] += 1  # channel 0 runs set 2: what set 1's context holds for it does not count
    G.rows_equal(got, refs, setof, "rows")
    refs[1][2, 5] += 1  # channel 2 runs set 1
    with pytest.raises(AssertionError, match="rows differs for the channels of set 1"):
        G.rows_equal(got, refs, setof, "rows")


def test_expected_state_moves_the_interpolator_memories_of_muted_channels_only():
    chain = SimpleNamespace(state_records=lambda blob: blob.reshape(GroupStub.n_channels, 190))  # a view, like RxChain's
    rng = np.random.default_rng(11)
    ref, before = rng.standard_normal((2, GroupStub.n_channels * 190)).astype(np.float32)
    kept = ref.copy()
    omap = np.array(GroupStub.ROW_OF)
    want = G.expected_state(chain, ref, before, omap).reshape(-1, 190)
    assert np.array_equal(ref, kept)  # a copy: the reference's checkpoint stays
    r, b = ref.reshape(-1, 190), before.reshape(-1, 190)
    moved = np.zeros(190, bool)
    moved[INT1] = moved[INT2] = True
    assert moved.sum() == 32 and (INT1.start, INT2.stop) == (152, 184)
    assert np.array_equal(want[omap >= 0], r[omap >= 0])
    assert np.array_equal(want[omap < 0][:, moved], b[omap < 0][:, moved]) and np.array_equal(want[omap < 0][:, ~moved], r[omap < 0][:, ~moved])
    assert not np.array_equal(want[omap < 0], r[omap < 0])


def test_bits_and_same():
    nan = np.array([0x7FC00001, 0x3F800000, 0xFFC00000], np.uint32).view(np.float32)
    assert not np.array_equal(nan, nan.copy()) and same(nan, nan.copy()) and bits(nan).dtype == np.uint32
    assert not same(nan, np.array([0x7FC00002, 0x3F800000, 0xFFC00000], np.uint32).view(np.float32))  # another NaN word
    x = np.arange(12, dtype=np.float32)
    assert same(x, x.copy()) and not same(x, x.reshape(3, 4)) and not same(x[:6], x)
    assert same(x.reshape(3, 4)[:, ::2], x.reshape(3, 4)[:, ::2].copy())  # not contiguous on the way in
    q = np.arange(6, dtype=np.int16)
    assert bits(q).dtype == np.int16 and same(q, q.copy()) and not same(q, q[::-1])


def test_interp_is_the_oracles_two_interpolators(built):
    """one fixed 4-block input: interp() against t41o_fir_interpolate_f32 called directly, block by block, with the
    CMSIS state lengths 48 / 2 + 256 - 1 = 23 + D and 32 / 4 + 512 - 1 = 7 + 2 D; and against the same two filters run
    over the whole stream in one block each (a FIR's output does not depend on how the stream is cut)"""
    D, kw = 256, dict(mode=0, audioVolume=55)
    n = np.arange(4 * D)
    x = (0.2 * np.sin(2 * np.pi * 700.0 / 24000.0 * n + 0.3) + 0.05 * np.random.default_rng(3).standard_normal(n.size)).astype(np.float32)
    lib, c = O.lib(), O.design(O.default_params(**kw))
    scale = vol_scale(55)
    assert scale.dtype == np.float32 and vol_scale(100) == np.float32(40.0) and vol_scale(0) == 0
    st1, st2 = np.zeros(23 + D, np.float32), np.zeros(7 + 2 * D, np.float32)
    mid, hi, want = np.empty(2 * D, np.float32), np.empty(8 * D, np.float32), np.empty(8 * x.size, np.float32)
    for b in range(4):
        blk = x[b * D:(b + 1) * D].copy()
        lib.t41o_fir_interpolate_f32(c.int1, 48, 2, O.fptr(st1), O.fptr(blk), O.fptr(mid), D)
        lib.t41o_fir_interpolate_f32(c.int2, 32, 4, O.fptr(st2), O.fptr(mid), O.fptr(hi), 2 * D)
        want[b * 8 * D:(b + 1) * 8 * D] = hi * scale
    got = interp(np.stack([x, x[::-1].copy()]), kw)
    assert got.dtype == np.float32 and got.shape == (2, 8 * x.size) and np.array_equal(got[0], want) and np.abs(want).max() > 1e-3
    assert not np.array_equal(got[1], want)  # the channels have their own histories
    st1, st2 = np.zeros(23 + 4 * D, np.float32), np.zeros(7 + 8 * D, np.float32)
    mid, hi = np.empty(8 * D, np.float32), np.empty(32 * D, np.float32)
    lib.t41o_fir_interpolate_f32(c.int1, 48, 2, O.fptr(st1), O.fptr(x), O.fptr(mid), 4 * D)
    lib.t41o_fir_interpolate_f32(c.int2, 32, 4, O.fptr(st2), O.fptr(mid), O.fptr(hi), 8 * D)
    assert np.array_equal(hi * scale, want)


# ---- the batch-isolation engine (tests/batch_harness.py) on stub chains ----------------------------------------------------
class BatchStub:
    """a case of the engine whose chain is numpy: channel c's audio is a function of its own rows, its NCO and its own
    earlier state, and its record holds its last sample -- or, with a fault, not quite"""
    L, schedule, dagger, env = 8, (2, 3), True, None

    def __init__(self, fault=None):
        self.fault = fault

    def signal(self, rows, nfr, seed, nco):
        rng = np.random.default_rng([seed, 12])
        return tuple((0.05 * rng.standard_normal((rows, nfr * self.L))).astype(np.float32) for _ in range(2))

    def open(self, T, comp, nco):
        assert T is None and nco.shape == (comp.nch,)
        return BatchStubChain(self.fault, comp.nch, nco)


class BatchStubChain:
    def __init__(self, fault, nch, nco):
        self.fault, self.nch, self.nco = fault, nch, nco
        self.state = np.zeros((nch, 3), np.float32)

    def call(self, I, Q, nfr):
        assert I.shape == Q.shape == (self.nch, nfr * BatchStub.L)
        n, c = self.nch, np.arange(self.nch)
        y = np.float32(0.5) * I + np.float32(0.25) * Q + (self.nco[:, None] * np.float32(1e-6) + self.state[:, :1])
        if self.fault == "neighbour":  # 2**-20 of the left neighbour's sample
            y[1:] += np.float32(2.0 ** -20) * I[:-1]
        if self.fault == "mod16":  # the place in a group of 16
            y += ((c % 16) * np.float32(2.0 ** -20))[:, None]
        if self.fault == "tail" and n % 4 == 1:  # the single channel of a ragged group of 4
            y[-1] += np.float32(2.0 ** -20)
        if self.fault == "big tail" and n % 4 == 1 and n > 64:  # the same, in batches of more than one group of 64 only
            y[-1] += np.float32(2.0 ** -20)
        if self.fault == "zero":
            y[:] = 0
        self.state[:, 0], self.state[:, 1] = y[:, -1], I[:, 0]
        if self.fault == "record":  # the audio is clean: only a record holds the neighbour's value
            self.state[1:, 2] = I[:-1, -1]
        return {"audio": y.astype(np.float32), "tap": (y * np.float32(2)).astype(np.float32)}

    def records(self):
        return {"path": self.state.copy()}


def test_batch_engine_compositions():
    import batch_harness as B
    comps = {c.name: c for c in B.compositions(True)}
    assert sorted(comps) == ["A", "B", "C", "D", "one"] and "D" not in [c.name for c in B.compositions(False)]
    assert B.POS == (0, 3, 4, 15, 16, 17, 63, 64, 66) and (comps["B"].nch, comps["D"].nch, comps["A"].nch, comps["one"].nch) == (67, 65, 9, 1)
    assert comps["A"].pos.tolist() == list(range(9))[::-1] and comps["B"].pos.tolist() == list(B.POS) == comps["C"].pos.tolist()
    assert comps["D"].pos.tolist() == list(B.POS[:8]) + [-1] and comps["D"].pos.max() == 64  # the ragged tail is one probe
    assert (comps["one"].pos >= 0).sum() == 1 and len(comps["B"].crowd) == 58 and len(comps["D"].crowd) == 57
    assert not set(comps["B"].crowd) & set(B.POS)
    # both sides of every grouping: a probe on the last channel of a group and one on the first of the next
    for g in (4, 16, 64):
        assert any(p % g == g - 1 and p + 1 in B.POS for p in B.POS), g
    # the crowd: a third of each class, rotated in C; full scale, exact silence, the signal class loud and clipped
    case = BatchStub()
    I, Q, nco = B.crowd_rows(case, 5, 1, 0)
    cls = B.crowd_class(0)
    assert sorted(np.bincount(cls)) == [19, 19, 20] and (B.crowd_class(1) != cls).all()
    assert (np.abs(I[cls == B.FULL]) == np.float32(0.999)).all() and len(np.unique(I[cls == B.FULL])) == 2
    assert not I[cls == B.SILENT].any() and not Q[cls == B.SILENT].any()
    loud = I[cls == B.LOUD]
    assert np.abs(loud).max() == np.float32(0.999) and 0.2 < np.abs(loud).mean() < 0.6 and I.dtype == np.float32
    assert not np.array_equal(nco, B.crowd_rows(case, 5, 2, 1)[2])


def test_batch_engine_passes_a_per_channel_chain():
    import batch_harness as B
    got = B.run_composition(None, BatchStub())
    assert sorted(got) == ["A", "B", "C", "D", "one"] and len(got["B"]) == 2
    assert sorted(got["B"][0]) == ["audio", "record:path", "tap"] and sorted(got["B"][0]["audio"]) == list(range(9))
    assert sorted(got["D"][1]["audio"]) == list(range(8)) and sorted(got["one"][1]["audio"]) == [B.ONE]
    assert got["B"][1]["audio"][3].dtype == np.uint32 and got["B"][1]["audio"][3].shape == (3 * BatchStub.L,)


@pytest.mark.parametrize("fault,where", [
    ("neighbour", "B vs C: audio of probe 1 "), ("mod16", "A vs B: audio of probe 0 "), ("record", "B vs C: record:path of probe 1 "),
    ("tail", "A vs B: audio of probe 0 "), ("big tail", r"B vs D: audio of probe 7 \(channel 64 of 67\)"), ("zero", "audio is all zero")])
def test_batch_engine_fails_a_leaking_chain(fault, where):
    import batch_harness as B
    with pytest.raises(AssertionError, match=where):
        B.run_composition(None, BatchStub(fault))


def test_batch_engine_wants_crowds_that_differ():
    import batch_harness as B

    class Deaf(BatchStub):  # the crowd's audio does not follow its rows: equal probes would prove nothing
        def open(self, T, comp, nco):
            ch = BatchStubChain(None, comp.nch, nco)
            inner = ch.call
            probes = comp.pos[comp.pos >= 0]

            def call(I, Q, nfr):
                out = inner(I, Q, nfr)
                keep = out["audio"][probes].copy()
                out["audio"][:] = 1
                out["audio"][probes] = keep
                return out
            ch.call = call
            return ch
    with pytest.raises(AssertionError, match="the crowd's audio is the same in B and C"):
        B.run_composition(None, Deaf())
