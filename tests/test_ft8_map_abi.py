"""The FT8 map's entry points (t41rx_set_ft8_map / t41rx_get_ft8_map / t41rx_ft8_rows): declared, exported and bound; every
refusal leaves the previous map in place and names the entry; the getter's round trip, the rows, removal; the map is
configuration and survives reset / set_state / set_params / set_coeffs; the long FFT lengths refuse; the Python shapes.
What the map makes a call compute is test_ft8_map.py."""
import ctypes as C

import numpy as np
import pytest

from rx_harness import ERR_ARG, ERR_UNSUPPORTED, assert_entry_points, refused

NCH = 5
NEW = ("t41rx_set_ft8_map", "t41rx_get_ft8_map", "t41rx_ft8_rows")


def test_entry_points_declared_exported_and_bound(built):
    import t41_sdr_amd._lib as lib
    assert_entry_points(NEW, ("set_ft8_map", "ft8_map", "ft8_rows"), abi_version=5, pattern=r"T41RX_API\s+int\s+%s\s*\(")
    assert lib.load().t41rx_abi_version() == 5


def _chain(T, **kw):
    return T.RxChain(NCH, T.default_params(mode=0, **kw))


def _get(rx):
    """(the getter's return, the map, n_rows, t41rx_ft8_rows()) through the C ABI"""
    m, rows = np.full(NCH, -9, np.int32), C.c_int(-9)
    rc = rx._lib.t41rx_get_ft8_map(rx._ctx, m.ctypes.data_as(C.POINTER(C.c_int32)), NCH, C.byref(rows))
    return rc, m.tolist(), rows.value, rx._lib.t41rx_ft8_rows(rx._ctx)


def _set(rx, rows, n, n_rows):
    from t41_sdr_amd._lib import check
    a = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
    check(rx._lib.t41rx_set_ft8_map(rx._ctx, None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32)), n, n_rows))


@pytest.mark.gpu
def test_gpu_round_trip_rows_and_removal():
    import t41_sdr_amd as T
    rx = _chain(T)
    assert _get(rx) == (0, [0, 1, 2, 3, 4], NCH, NCH) and rx.ft8_map is None and rx.ft8_rows == NCH
    assert rx._lib.t41rx_get_ft8_map(rx._ctx, None, 0, None) == 0  # both pointers may be NULL
    rx.set_ft8_map([-1, 2, -1, -1, 0], 3)
    assert _get(rx) == (1, [-1, 2, -1, -1, 0], 3, 3) and rx.ft8_map.tolist() == [-1, 2, -1, -1, 0] and rx.ft8_rows == 3
    rx.set_ft8_map([-1, 1, -1, -1, 0])  # n_rows defaults to max + 1
    assert _get(rx) == (1, [-1, 1, -1, -1, 0], 2, 2) and rx.ft8_rows == 2
    rx.set_ft8_map([-1] * NCH)  # nobody listed: one row, never written
    assert _get(rx) == (1, [-1] * NCH, 1, 1)
    rx.set_ft8_map([4, 3, 2, 1, 0])
    assert _get(rx) == (1, [4, 3, 2, 1, 0], NCH, NCH)
    rx.set_ft8_map(None)
    assert _get(rx) == (0, [0, 1, 2, 3, 4], NCH, NCH) and rx.ft8_map is None and rx.ft8_rows == NCH
    lib = rx._lib  # a null context
    assert lib.t41rx_set_ft8_map(None, None, 0, 0) == ERR_ARG and lib.t41rx_get_ft8_map(None, None, 0, None) == ERR_ARG and lib.t41rx_ft8_rows(None) == ERR_ARG


@pytest.mark.gpu
def test_gpu_every_refusal_leaves_the_map():
    import t41_sdr_amd as T
    rx = _chain(T)
    good = [-1, 2, -1, -1, 0]
    rx.set_ft8_map(good, 3)
    before = _get(rx)

    def no(words, rows, n, n_rows, status=ERR_ARG):
        refused(lambda: _set(rx, rows, n, n_rows), status, "FT8 map", *words)
        assert _get(rx) == before, "a refused call changed the map"

    no(["n (4)", "n_channels"], good[:4], 4, 3)
    no(["n (6)", "n_channels"], good + [1], 6, 3)
    no(["n (0)"], good, 0, 3)
    for n_rows in (0, -1, NCH + 1):
        no(["n_rows (%d)" % n_rows, "1 .. n_channels"], good, NCH, n_rows)
    for c, bad in ((0, -2), (2, 3), (4, 4), (3, -2147483648), (1, 2147483647)):
        rows = list(good)
        rows[c] = bad
        no(["channel %d " % c, "row %d," % bad, "[-1, n_rows 3)"], rows, NCH, 3)
    no(["row 2 is named twice", "channel 1 ", "channel 3"], [-1, 2, -1, 2, 0], NCH, 3)
    no(["row 0 is named twice", "channel 0 ", "channel 4"], [0, 2, -1, -1, 0], NCH, 3)
    no(["null map", "n 0 and n_rows 0"], None, NCH, 0)
    no(["null map", "n 0 and n_rows 0"], None, 0, 3)
    # FT8 receive on: the buffers are sized by the rows
    rx.set_ft8_tables()
    power, status = rx.set_ft8(1, 4)
    assert tuple(power.shape) == (3, 2, 92 * 1472) and tuple(status.shape) == (3, 4, 4)
    no(["n_rows (2)", "FT8 receive is on", "switch FT8 off"], [-1, 1, -1, -1, 0], NCH, 2)
    no(["n_rows (5)", "FT8 receive is on"], [4, 3, 2, 1, 0], NCH, NCH)
    no(["removing the map", "from 3 to n_channels", "FT8 receive is on"], None, 0, 0)
    rx.set_ft8_map([1, -1, 2, -1, -1], 3)  # at equal n_rows the map may change
    assert _get(rx) == (1, [1, -1, 2, -1, -1], 3, 3)
    rx.set_ft8_map([-1] * NCH, 3)
    before = _get(rx)
    no(["n_rows (1)"], [-1] * NCH, NCH, 1)
    # the caller's way round: off, the map, on with buffers of the new size
    rx.set_ft8(0)
    rx.set_ft8_map([0, -1, -1, -1, 1])
    power, status = rx.set_ft8(1, 4)
    assert tuple(power.shape) == (2, 2, 92 * 1472) and rx.ft8_rows == 2
    # without a map FT8 on holds n_channels rows: a map of n_channels rows is accepted, any other refused; removal is free
    plain = _chain(T)
    plain.set_ft8_tables()
    plain.set_ft8(1, 4)
    before = _get(plain)
    refused(lambda: _set(plain, good, NCH, 3), ERR_ARG, "FT8 map", "n_rows (3)", "FT8 receive is on")
    assert _get(plain) == before
    plain.set_ft8_map([4, 3, -1, 1, 0], NCH)
    plain.set_ft8_map(None)
    assert _get(plain) == before


@pytest.mark.gpu
def test_gpu_the_map_is_configuration():
    """kept by t41rx_reset, t41rx_set_state, t41rx_set_params and t41rx_set_coeffs; in no checkpoint"""
    import t41_sdr_amd as T
    rx, bare = _chain(T), _chain(T)
    assert rx._lib.t41rx_state_bytes(rx._ctx) == bare._lib.t41rx_state_bytes(bare._ctx)
    rows = [-1, 2, -1, -1, 0]
    rx.set_ft8_map(rows, 3)
    want = _get(rx)
    assert rx._lib.t41rx_state_bytes(rx._ctx) == bare._lib.t41rx_state_bytes(bare._ctx)
    assert rx._lib.t41rx_ft8_state_bytes(rx._ctx) == 32 + 4 * 3088 * NCH  # the FT8 memory's record stays [n_channels]
    state = rx.get_state()
    assert np.array_equal(state, bare.get_state())
    rx.reset()
    assert _get(rx) == want
    rx.set_state(state)
    assert _get(rx) == want
    rx.CalcFilters(FLoCut=300, FHiCut=2700)
    assert _get(rx) == want
    rx.set_coeffs(bare.coeffs())
    assert _get(rx) == want
    bare.set_state(rx.get_state())  # a checkpoint taken with a map restores into a context without
    assert _get(bare)[0] == 0


@pytest.mark.gpu
def test_gpu_long_fft_refuses():
    import t41_sdr_amd as T
    for n in (1024, 4096):
        rx = _chain(T, fft_length=n)
        refused(lambda: rx.set_ft8_map([-1, 2, -1, -1, 0], 3), ERR_UNSUPPORTED, "FT8 map", "fft_length 512")
        assert _get(rx) == (0, [0, 1, 2, 3, 4], NCH, NCH)
        rx.set_ft8_map(None)  # nothing to remove, nothing refused


@pytest.mark.gpu
def test_gpu_python_shapes():
    import torch
    import t41_sdr_amd as T
    import ft8_decode_model as D
    from t41_sdr_amd._lib import check
    rx = _chain(T)
    rx.set_ft8_tables()
    rx.set_ft8_map([-1, 2, -1, -1, 0], 3)
    power, status = rx.set_ft8(1, 20)
    assert tuple(power.shape) == (3, 2, 92 * 1472) and power.dtype == torch.uint8 and tuple(status.shape) == (3, 20, 4)
    assert rx.ft8_power() is power and tuple(rx.ft8_status(7).shape) == (3, 7, 4)
    assert rx.ft8_status(7).data_ptr() == status.data_ptr() and rx.ft8_status(7).is_contiguous()
    st = rx.ft8_audio(np.zeros((3, 15 * 128), np.int16))
    assert tuple(st.shape) == (3, 15, 4) and st[0, -1, 3] == 0 and st[2, -1, 3] == 0
    for shape in ((NCH, 128), (2, 128), (3, 100)):
        with pytest.raises(ValueError, match="ft8_rows = 3"):
            rx.ft8_audio(np.zeros(shape, np.int16))
    t = D.tables()
    rx.set_ft8_decode_tables(t.costas, t.gray, t.nm, t.mn, t.nrw)
    res = rx.ft8_decode(select=[0, -1, 1])
    assert res.shape == (3,) and res["select"].tolist() == [0, -1, 1]
    with pytest.raises(ValueError, match="ft8_rows = 3"):
        rx.ft8_decode(select=[0] * NCH)
    own = torch.zeros(NCH, 92 * 1472, dtype=torch.uint8, device="cuda")
    assert rx.ft8_decode(waterfall=own).shape == (NCH,)  # a caller's waterfall stays by channel
    refused(lambda: check(rx._lib.t41rx_ft8_decode_host(rx._ctx, None, 0, None, NCH, np.zeros(NCH * 656, np.uint8).ctypes.data_as(C.c_void_p))),
            ERR_ARG, "t41rx_ft8_rows()")
    rx.set_ft8(0)
    rx.set_ft8_map(None)
    power, status = rx.set_ft8(1, 20)
    assert tuple(power.shape) == (NCH, 2, 92 * 1472) and tuple(rx.ft8_status(3).shape) == (NCH, 3, 4)
