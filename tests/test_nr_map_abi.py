"""The noise-reduction map at the ABI: t41rx_set_nr_map / t41rx_get_nr_map are declared with T41RX_API in include/t41rx.h,
listed in exports.map, bound by _lib.SYMBOLS and exported by the built library; the header states the rule; the ABI stays
5; a NULL context is refused before anything else is looked at; the Python layer's own refusals on an object made with
__new__ (no context is created).  All that needs no GPU.  The getter's round trips with and without a map, its NULL
outputs, the n mismatch, and t41rx_state_bytes() and the checkpoint's section word unchanged by the map need a context and
with it a device: those tests alone are marked gpu."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t41rx_set_nr_map", "t41rx_get_nr_map")
N = 3


def _header():
    return open(os.path.join(ROOT, "include", "t41rx.h")).read()


@pytest.fixture
def T(built):
    import t41_sdr_amd
    return t41_sdr_amd


def test_header_declares_the_entry_points_with_the_export_attribute():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    ctx, cctx, i32, ci32 = r"t41rx_ctx\s*\*\s*ctx", r"const\s+t41rx_ctx\s*\*\s*ctx", r"int32_t\s*\*\s*", r"const\s+int32_t\s*\*\s*"
    for name, first, x, y in (("t41rx_set_nr_map", ctx, ci32 + "nr_of_channel", ci32 + "notch_of_channel"),
                              ("t41rx_get_nr_map", cctx, i32 + "nr_of_channel_out", i32 + "notch_of_channel_out")):
        assert re.search(r"T41RX_API\s+int\s+%s\s*\(\s*%s\s*,\s*%s\s*,\s*%s\s*,\s*int\s+n\s*\)\s*;" % (name, first, x, y), code), name
    assert re.search(r"#define\s+T41RX_ABI_VERSION\s+5\b", code)


def test_header_states_the_rule():
    doc = re.sub(r"\s*\n\s*\*\s*", " ", _header())
    assert "parameters carry nrOptionSelect = nr_of_channel[c] (0 .. 3) and ANR_notchOn = notch_of_channel[c] (0 / 1)" in doc
    assert "the spectral function leaves NR_X[.][1..2] and NR_E alone and Kim1_NR() then starts from them" in doc
    assert "LMS and notch share one Xanr() record" in doc
    assert "are still what t41rx_get_params() returns" in doc
    assert "either no stage map is loaded or the channel's T41RX_STAGE_NR bit is set" in doc
    assert "audio not touched, both records as they were" in doc
    assert "in no checkpoint, survives t41rx_reset" in doc
    assert "Still per context: nrOptionSelect" not in doc


def test_export_list_and_binding_carry_them(T):
    from t41_sdr_amd import _lib
    m = re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())
    assert set(NEW) <= set(re.findall(r"\b(t41rx_[a-z0-9_]+);", m))
    i32p = C.POINTER(C.c_int32)
    for name in NEW:
        assert _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, i32p, i32p, C.c_int]), name
    lib = T.load()
    assert lib.t41rx_abi_version() == 5
    raw = C.CDLL(T.LIB_PATH)
    assert all(hasattr(raw, s) for s in NEW)
    # a NULL context: T41RX_ERR_ARG with a text, no device needed, nothing written
    k4, t4 = np.full(4, 2, np.int32), np.full(4, 1, np.int32)
    for name in NEW:
        assert getattr(lib, name)(None, k4.ctypes.data_as(i32p), t4.ctypes.data_as(i32p), 4) == _lib.ERR_ARG and lib.t41rx_last_error(), name
    assert (k4 == 2).all() and (t4 == 1).all()


def test_docstrings_exist(T):
    f = T.RxChain.set_nr_map
    assert callable(f) and f.__doc__ and "t41rx_set_nr_map" in f.__doc__
    p = T.RxChain.nr_map
    assert isinstance(p, property) and p.__doc__


def test_python_layer_refusals(T):
    """what rx.py refuses before it calls the library (ValueError, the message whole), and valid arguments, which the null
    context makes the C side refuse with T41RX_ERR_ARG"""
    from t41_sdr_amd import _lib
    rx = T.RxChain.__new__(T.RxChain)
    rx._lib, rx._ctx, rx.params = _lib.load(), C.c_void_p(), T.default_params()
    rx.n_channels, rx.device, rx.frame_len, rx.layout, rx._n_streams = N, 0, 2048, "channel", 0

    def refused(message, *args):
        with pytest.raises(ValueError) as e:
            rx.set_nr_map(*args)
        assert type(e.value) is ValueError and str(e.value) == message, (str(e.value), message)

    kind = "nr_of_channel must be a 1-d array of n_channels nrOptionSelect values (0 .. 3), got %s"
    refused(kind % "(3,) float64", [0.0, 3.0, 2.0], [0, 1, 0])
    refused(kind % "(1, 3) int64", [[0, 3, 2]], [0, 1, 0])
    refused(kind % "() int64", 2, [0, 1, 0])
    refused(kind % "(3,) int64", [0, 1 << 40, 2], [0, 1, 0])
    notch = "notch_of_channel must be a 1-d array of ANR_notchOn values (0 / 1) as long as nr_of_channel, got %s"
    refused(notch % "(3,) float64", [0, 3, 2], [0.0, 1.0, 0.0])
    refused(notch % "(2,) int64", [0, 3, 2], [0, 1])
    refused(notch % "(3,) int64", [0, 3, 2], [0, 1 << 40, 0])
    refused("notch_of_channel must be given with nr_of_channel: n_channels=3 values 0 / 1", [0, 3, 2])
    refused("notch_of_channel goes with nr_of_channel: pass both, or None to remove the map", None, [0, 1, 0])
    for call in (lambda: rx.set_nr_map([0, 3, 2], [0, 1, 0]), lambda: rx.set_nr_map(np.zeros(3, np.int32), np.zeros(3, np.int32)),
                 lambda: rx.set_nr_map(None), lambda: rx.nr_map):
        with pytest.raises(T.T41RxError) as e:
            call()
        assert e.value.status == _lib.ERR_ARG


# ---- the getter, and what the map leaves alone: a context, and with it a device ------------------------------------------------
NCH = 5
KW = dict(mode=0, FLoCut=200, FHiCut=3000, nrOptionSelect=3, ANR_notchOn=1)


@pytest.mark.gpu
def test_getter_round_trips_null_outputs_and_n(T):
    import torch
    from t41_sdr_amd import _lib
    assert torch.cuda.is_available()
    rx = T.RxChain(NCH, T.default_params(**KW), NCOFreq=np.zeros(NCH, np.int32))
    i32p = C.POINTER(C.c_int32)
    get = rx._lib.t41rx_get_nr_map
    k, t = np.full(NCH, -9, np.int32), np.full(NCH, -9, np.int32)
    kp, tp = k.ctypes.data_as(i32p), t.ctypes.data_as(i32p)
    # without a map: 0, and the context's own values in every entry; either output may be NULL
    assert rx.nr_map is None
    assert get(rx._ctx, kp, tp, NCH) == 0 and (k == 3).all() and (t == 1).all()
    k[:], t[:] = -9, -9
    assert get(rx._ctx, kp, None, NCH) == 0 and (k == 3).all() and (t == -9).all()
    k[:] = -9
    assert get(rx._ctx, None, tp, NCH) == 0 and (k == -9).all() and (t == 1).all()
    assert get(rx._ctx, None, None, 0) == 0 and get(rx._ctx, None, None, 77) == 0  # (no output: n is not looked at)
    # with a map: 1, and the map; n must be n_channels where there is an output
    kind, notch = np.array([0, 1, 2, 3, 2], np.int32), np.array([1, 0, 1, 1, 0], np.int32)
    rx.set_nr_map(kind, notch)
    got = rx.nr_map
    assert np.array_equal(got[0], kind) and np.array_equal(got[1], notch) and got[0].dtype == np.int32
    got[0][:] = 0  # (copies)
    assert np.array_equal(rx.nr_map[0], kind)
    t[:] = -9
    assert get(rx._ctx, kp, None, NCH) == 1 and np.array_equal(k, kind) and (t == -9).all()
    assert get(rx._ctx, None, tp, NCH) == 1 and np.array_equal(t, notch)
    assert get(rx._ctx, None, None, 0) == 1
    for n in (NCH - 1, NCH + 1, 0):
        assert get(rx._ctx, kp, tp, n) == _lib.ERR_ARG and b"must equal n_channels" in rx._lib.t41rx_last_error()
        assert rx._lib.t41rx_set_nr_map(rx._ctx, kp, tp, n) == _lib.ERR_ARG and b"must equal n_channels" in rx._lib.t41rx_last_error()
    assert np.array_equal(rx.nr_map[0], kind) and np.array_equal(rx.nr_map[1], notch)
    # the context's own two values are kept under the map, and removal returns to them
    p = T.default_params()
    assert rx._lib.t41rx_get_params(rx._ctx, C.byref(p)) == 0 and (p.nrOptionSelect, p.ANR_notchOn) == (3, 1)
    rx.set_nr_map(None)
    assert rx.nr_map is None and get(rx._ctx, kp, tp, NCH) == 0 and (k == 3).all() and (t == 1).all()


@pytest.mark.gpu
def test_state_bytes_and_the_section_word_do_not_see_the_map(T):
    import torch
    assert torch.cuda.is_available()
    L = 2048
    rng = np.random.default_rng(5)
    I, Q = (0.2 * rng.standard_normal((2, NCH, L))).astype(np.float32)
    a = T.RxChain(NCH, T.default_params(**KW), NCOFreq=np.zeros(NCH, np.int32))
    b = T.RxChain(NCH, T.default_params(**KW), NCOFreq=np.zeros(NCH, np.int32))
    a.set_nr_map(np.array([0, 1, 2, 3, 0], np.int32), np.array([1, 0, 0, 1, 0], np.int32))
    word = lambda rx: int(rx.get_state()[:32].view(np.int32)[5])  # noqa: E731
    assert a._lib.t41rx_state_bytes(a._ctx) == b._lib.t41rx_state_bytes(b._ctx) and word(a) == word(b)
    for rx in (a, b):
        rx.ProcessIQData(torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda())
        torch.cuda.synchronize()
    assert a._lib.t41rx_state_bytes(a._ctx) == b._lib.t41rx_state_bytes(b._ctx) and word(a) == word(b) and word(a) & 1
    a.set_nr_map(None)
    assert a._lib.t41rx_state_bytes(a._ctx) == b._lib.t41rx_state_bytes(b._ctx) and word(a) == word(b)
