"""The test support code itself (tests/rx_harness.py, tests/stage_reference.py), without a device: layouts, sample
formats, the (Q, I) order of the q15 entry points, a stream cut into calls against a stub chain, and the reference
interpolators against the oracle's primitive called directly."""
import numpy as np
import pytest

import oracle_lib as O
from rx_harness import calls, from_time_major, one_call, pack, to_q15, to_time_major
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
