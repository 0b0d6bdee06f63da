"""The beacon monitor's refusals that need no GPU: what RxChain's methods refuse before they call the library, with the
exception type and exact text, and for each entry point one valid argument set, which a null context makes the C side
refuse with T41RX_ERR_ARG -- so the Python checks let it through and the call arrived with the table's arity.  The
object is made with __new__ (no context is created), as in test_python_layer_refusals.py."""
import ctypes as C

import numpy as np
import pytest

N = 3


@pytest.fixture
def T(built):
    import t41_sdr_amd
    return t41_sdr_amd


@pytest.fixture
def rx(T):
    from t41_sdr_amd import _lib
    r = T.RxChain.__new__(T.RxChain)
    r._lib, r._ctx, r.params = _lib.load(), C.c_void_p(), T.default_params()
    r.n_channels, r.device, r.frame_len, r.layout, r._n_streams = N, 0, 2048, "channel", 0
    return r


def refused(exc, message, call, *a, **kw):
    with pytest.raises(exc) as e:
        call(*a, **kw)
    assert type(e.value) is exc and str(e.value) == message, (str(e.value), message)


def reaches_the_library(T, call, *a, **kw):
    from t41_sdr_amd import _lib
    with pytest.raises(T.T41RxError) as e:
        call(*a, **kw)
    assert e.value.status == _lib.ERR_ARG, str(e.value)


def test_set_beacon_arguments(T, rx):
    head = "band must be n_channels = 3 int32 values, got "
    refused(ValueError, head + "(0,) float64", rx.set_beacon, True)  # no band at all
    refused(ValueError, head + "(2,) int64", rx.set_beacon, True, 0, [0, 1])
    refused(ValueError, head + "(3,) float64", rx.set_beacon, True, 0, [0.0, 1.0, 2.0])
    refused(ValueError, head + "(1, 3) int64", rx.set_beacon, True, 0, [[0, 1, 2]])
    refused(ValueError, head + "(3,) int64", rx.set_beacon, True, 0, [0, 2**31, 0])
    refused(ValueError, "band must be 0 .. 4 (20, 17, 15, 12, 10 m), got [0, 5, 1]", rx.set_beacon, True, 0, [0, 5, 1])
    refused(ValueError, "band must be 0 .. 4 (20, 17, 15, 12, 10 m), got [-1, 0, 1]", rx.set_beacon, True, 0, [-1, 0, 1])
    refused(ValueError, "mode must be 0 (the firmware's cycle) or 1 (continuous), got 2", rx.set_beacon, True, 2, [0, 1, 2])
    refused(ValueError, "mode must be 0 (the firmware's cycle) or 1 (continuous), got -1", rx.set_beacon, True, -1, [0, 1, 2])
    refused(ValueError, head + "(2,) int64", rx.set_beacon, True, 7, [0, 1])  # the first wins
    refused(ValueError, "max_rows must be >= 1", rx.set_beacon, True, 0, [0, 1, 2], max_rows=0)
    rx._beacon = keep = ("snr", "events")
    reaches_the_library(T, rx.set_beacon, False)
    assert rx._beacon is keep  # a refused switch-off leaves the tensors


def test_the_other_entry_points_reach_the_library(T, rx):
    for call, args in ((rx.set_beacon_clock, ()), (rx.set_beacon_clock, (171000, 1000, 1)), (rx.beacon_snr, ()), (rx.beacon_status, ()),
                       (rx.beacon_state, ()), (rx.set_beacon_state, (np.zeros(64, np.uint8),)), (rx.set_beacon_state, (bytearray(32),))):
        reaches_the_library(T, call, *args)


def test_the_c_side_refuses_a_null_context_and_reports_no_size(T, rx):
    from t41_sdr_amd import _lib
    lib = rx._lib
    band = (C.c_int32 * N)(0, 1, 2)
    assert lib.t41rx_set_beacon(None, 1, 0, band, None, None, 1) == _lib.ERR_ARG
    assert lib.t41rx_set_beacon(None, 0, 0, None, None, None, 0) == _lib.ERR_ARG
    assert lib.t41rx_set_beacon_clock(None, 0, 32, 3) == _lib.ERR_ARG
    assert lib.t41rx_get_beacon(None, None, None) == _lib.ERR_ARG
    assert lib.t41rx_beacon_state_bytes(None) == 0
    buf = (C.c_uint8 * 64)()
    assert lib.t41rx_beacon_get_state(None, buf, 64) == _lib.ERR_ARG and lib.t41rx_beacon_set_state(None, buf, 64) == _lib.ERR_ARG
    assert lib.t41rx_last_error()
