"""Stage parameters per channel at the ABI: t41rx_set_cw_filter_map / _get_cw_filter_map / t41rx_set_receive_eq_map /
_get_receive_eq_map are declared with T41RX_API in include/t41rx.h, listed in exports.map, bound by _lib.SYMBOLS and
exported by the built library; the header states both rules; the ABI stays 5; a NULL context is refused before anything
else is looked at; the Python layer's own refusals on an object made with __new__ (no context is created).  All that
needs no GPU.  The setters' refusals -- status, text, the previous map left whole, the filter map and the parameter sets
in both orders -- need a context and with it a device: those tests alone are marked gpu."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t41rx_set_cw_filter_map", "t41rx_get_cw_filter_map", "t41rx_set_receive_eq_map", "t41rx_get_receive_eq_map")
METHODS = ("set_cw_filter_map", "set_receive_eq_map")
PROPERTIES = ("cw_filter_map", "receive_eq_map")
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
    for name, first, arg in (("t41rx_set_cw_filter_map", ctx, ci32 + "filter_of_channel"), ("t41rx_get_cw_filter_map", cctx, i32 + "filter_of_channel_out"),
                             ("t41rx_set_receive_eq_map", ctx, ci32 + "equalizerRec"), ("t41rx_get_receive_eq_map", cctx, i32 + "equalizerRec_out")):
        assert re.search(r"T41RX_API\s+int\s+%s\s*\(\s*%s\s*,\s*%s\s*,\s*int\s+n\s*\)\s*;" % (name, first, arg), code), name
    assert re.search(r"#define\s+T41RX_ABI_VERSION\s+5\b", code)


def test_header_states_both_rules():
    doc = re.sub(r"\s*\n\s*\*\s*", " ", _header())
    assert "whose t41rx_set_cw_filter() value is filter_of_channel[c]" in doc
    assert "only the selected one advances, the other four stay stale" in doc
    assert "is still what t41rx_get_cw_filter() returns" in doc
    assert "unless xmtMode == T41RX_CW_MODE" in doc
    assert "an entry outside [0, 5]" in doc and "t41rx_set_cw_tables()" in doc
    assert "whose t41rx_set_receive_eq(1, equalizerRec[c]) would process it" in doc
    assert "T41RX_STAGE_EQ bit is set or no stage map is loaded" in doc
    assert "returned by t41rx_get_receive_eq() as before" in doc
    assert "they are in no checkpoint" in doc and "survive t41rx_reset" in doc


def test_export_list_and_binding_carry_them(T):
    from t41_sdr_amd import _lib
    m = re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())
    assert set(NEW) <= set(re.findall(r"\b(t41rx_[a-z0-9_]+);", m))
    i32p = C.POINTER(C.c_int32)
    for name in NEW:
        assert _lib.SYMBOLS[name] == (C.c_int, [C.c_void_p, i32p, C.c_int]), name
    lib = T.load()
    assert lib.t41rx_abi_version() == 5
    raw = C.CDLL(T.LIB_PATH)
    assert all(hasattr(raw, s) for s in NEW)
    # a NULL context: T41RX_ERR_ARG with a text, no device needed, nothing written
    m4, l4 = np.full(4, 2, np.int32), np.full((4, 14), 100, np.int32)
    for name, a in (("t41rx_set_cw_filter_map", m4), ("t41rx_get_cw_filter_map", m4), ("t41rx_set_receive_eq_map", l4), ("t41rx_get_receive_eq_map", l4)):
        assert getattr(lib, name)(None, a.ctypes.data_as(i32p), 4) == _lib.ERR_ARG and lib.t41rx_last_error(), name
    assert (m4 == 2).all() and (l4 == 100).all()


def test_docstrings_exist(T):
    for meth in METHODS:
        f = getattr(T.RxChain, meth)
        assert callable(f) and f.__doc__ and "t41rx_" + meth in f.__doc__, meth
    for prop in PROPERTIES:
        p = getattr(T.RxChain, prop)
        assert isinstance(p, property) and p.__doc__, prop


def test_python_layer_refusals(T):
    """what rx.py refuses before it calls the library (ValueError, the message whole), and valid arguments, which the null
    context makes the C side refuse with T41RX_ERR_ARG"""
    from t41_sdr_amd import _lib
    rx = T.RxChain.__new__(T.RxChain)
    rx._lib, rx._ctx, rx.params = _lib.load(), C.c_void_p(), T.default_params()
    rx.n_channels, rx.device, rx.frame_len, rx.layout, rx._n_streams = N, 0, 2048, "channel", 0

    def refused(setter, message, arg):
        with pytest.raises(ValueError) as e:
            setter(arg)
        assert type(e.value) is ValueError and str(e.value) == message, (str(e.value), message)

    cw = "filter_of_channel must be a 1-d array of n_channels CWFilterIndex values (0 .. 5), got %s"
    refused(rx.set_cw_filter_map, cw % "(3,) float64", [0.0, 5.0, 2.0])
    refused(rx.set_cw_filter_map, cw % "(1, 3) int64", [[0, 5, 2]])
    refused(rx.set_cw_filter_map, cw % "() int64", 2)
    refused(rx.set_cw_filter_map, cw % "(3,) int64", [0, 1 << 40, 2])
    eq = "levels must be an [n_channels][14] array of ints, got %s"
    refused(rx.set_receive_eq_map, eq % "(3, 14) float64", np.full((3, 14), 100.0))
    refused(rx.set_receive_eq_map, eq % "(14,) int64", [100] * 14)
    refused(rx.set_receive_eq_map, eq % "(3, 13) int64", np.full((3, 13), 100))
    refused(rx.set_receive_eq_map, eq % "(3, 2, 7) int64", np.full((3, 2, 7), 100))
    refused(rx.set_receive_eq_map, "levels must fit int32, got (42,) int64", np.full((3, 14), 1 << 40))
    for call in (lambda: rx.set_cw_filter_map([0, 5, 2]), lambda: rx.set_cw_filter_map(np.array([5, 5, 5], np.int32)), lambda: rx.set_cw_filter_map(None),
                 lambda: rx.set_receive_eq_map(np.full((3, 14), 100)), lambda: rx.set_receive_eq_map(None),
                 lambda: rx.cw_filter_map, lambda: rx.receive_eq_map):
        with pytest.raises(T.T41RxError) as e:
            call()
        assert e.value.status == _lib.ERR_ARG


# ---- the setters' refusals: a context, and with it a device ------------------------------------------------------------------
NCH = 5
CW_KW = dict(mode=0, FLoCut=200, FHiCut=3000, xmtMode=1)
LONG_KW = dict(mode=0, FLoCut=400, FHiCut=600, fft_length=1024)
LSB_SET = dict(mode=1, FLoCut=-3000, FHiCut=-200)


def _chain(T, kw=CW_KW, tables=True):
    import torch
    import cw_model as CWM
    assert torch.cuda.is_available()
    rx = T.RxChain(NCH, T.default_params(**kw), NCOFreq=np.zeros(NCH, np.int32))
    if tables:
        rx.set_cw_tables(*CWM.tables())
    return rx


def _refused(T, fn, status, *words):
    with pytest.raises(T.T41RxError) as e:
        fn()
    msg = str(e.value)
    assert e.value.status == status and msg.strip(), (e.value.status, msg)
    for w in words:
        assert w in msg, (w, msg)


@pytest.mark.gpu
def test_cw_filter_map_refusals_leave_the_previous_map(T):
    from t41_sdr_amd import _lib
    rx = _chain(T)
    good = np.array([0, 5, 2, 4, 5], np.int32)
    rx.set_cw_filter_map(good)
    _refused(T, lambda: rx.set_cw_filter_map(good[:4]), _lib.ERR_ARG, "n (4)", "n_channels")
    _refused(T, lambda: rx.set_cw_filter_map(np.append(good, 1).astype(np.int32)), _lib.ERR_ARG, "n (6)")
    _refused(T, lambda: rx.set_cw_filter_map(np.array([0, 5, 6, 4, 5], np.int32)), _lib.ERR_ARG, "channel 2", "CWFilterIndex 6")
    _refused(T, lambda: rx.set_cw_filter_map(np.array([0, 5, 2, 4, -1], np.int32)), _lib.ERR_ARG, "channel 4", "CWFilterIndex -1")
    i32p = C.POINTER(C.c_int32)
    assert rx._lib.t41rx_set_cw_filter_map(rx._ctx, None, NCH) == _lib.ERR_ARG and rx._lib.t41rx_last_error()  # NULL removes, and takes n 0
    assert rx._lib.t41rx_get_cw_filter_map(rx._ctx, good.copy().ctypes.data_as(i32p), NCH - 1) == _lib.ERR_ARG
    assert np.array_equal(rx.cw_filter_map, good), "a refused call changed the map"
    assert rx.cw_filter == 5
    # with no map the getter answers 0 and fills in the context-wide index
    rx.set_cw_filter(3)
    rx.set_cw_filter_map(None)
    out = np.zeros(NCH, np.int32)
    assert rx._lib.t41rx_get_cw_filter_map(rx._ctx, out.ctypes.data_as(i32p), NCH) == 0 and (out == 3).all()
    assert rx.cw_filter_map is None
    # no filter tables: an index below 5 is refused and named, a map of 5s is not
    bare = _chain(T, tables=False)
    _refused(T, lambda: bare.set_cw_filter_map(np.array([5, 5, 5, 1, 5], np.int32)), _lib.ERR_ARG, "channel 3", "t41rx_set_cw_tables")
    assert bare.cw_filter_map is None
    bare.set_cw_filter_map(np.full(NCH, 5, np.int32))
    assert (bare.cw_filter_map == 5).all()
    # a long fft_length
    long = _chain(T, LONG_KW)
    _refused(T, lambda: long.set_cw_filter_map(good), _lib.ERR_UNSUPPORTED, "fft_length 512")
    assert long.cw_filter_map is None


@pytest.mark.gpu
def test_filter_map_and_parameter_sets_refuse_each_other_in_both_orders(T):
    from t41_sdr_amd import _lib
    words = ("the CW audio filter", "splits the fused chain", "t41rx_set_param_sets")
    setof = np.array([0, 1, 1, 0, 1], np.int32)
    some, nobody = np.array([5, 5, 2, 5, 5], np.int32), np.full(NCH, 5, np.int32)
    # sets first: a map with an index is refused in the stages' words, a map of 5s is accepted
    a = _chain(T)
    a.set_param_sets([LSB_SET], setof)
    _refused(T, lambda: a.set_cw_filter_map(some), _lib.ERR_UNSUPPORTED, *words)
    assert a.cw_filter_map is None
    a.set_cw_filter_map(nobody)
    _refused(T, lambda: a.set_cw_filter_map(some), _lib.ERR_UNSUPPORTED, *words)
    assert np.array_equal(a.cw_filter_map, nobody) and len(a.param_sets) == 1
    # the map first: the sets are refused, naming the stage; with a map of 5s, or the map removed, they load
    b = _chain(T)
    b.set_cw_filter_map(some)
    _refused(T, lambda: b.set_param_sets([LSB_SET], setof), _lib.ERR_UNSUPPORTED, "the CW audio filter")
    assert b.param_sets == [] and np.array_equal(b.cw_filter_map, some)
    b.set_cw_filter_map(nobody)
    b.set_param_sets([LSB_SET], setof)
    b.set_param_sets(None)
    b.set_cw_filter_map(some)
    b.set_cw_filter_map(None)
    b.set_param_sets([LSB_SET], setof)
    assert len(b.param_sets) == 1


@pytest.mark.gpu
def test_receive_eq_map_refusals_leave_the_previous_map(T):
    from t41_sdr_amd import _lib
    rx = _chain(T)
    good = (np.arange(NCH * 14, dtype=np.int32).reshape(NCH, 14) * 3) - 50
    rx.set_receive_eq_map(good)  # (a map may be loaded with the switch off and no band table: it has no effect until the equalizer runs)
    _refused(T, lambda: rx.set_receive_eq_map(good[:4]), _lib.ERR_ARG, "n (4)", "n_channels")
    _refused(T, lambda: rx.set_receive_eq_map(np.concatenate([good, good[:1]])), _lib.ERR_ARG, "n (6)")
    i32p = C.POINTER(C.c_int32)
    assert rx._lib.t41rx_set_receive_eq_map(rx._ctx, None, NCH) == _lib.ERR_ARG and rx._lib.t41rx_last_error()
    assert rx._lib.t41rx_get_receive_eq_map(rx._ctx, good.copy().ctypes.data_as(i32p), NCH + 1) == _lib.ERR_ARG
    assert np.array_equal(rx.receive_eq_map, good), "a refused call changed the map"
    on, own = rx.receive_eq
    assert on == 0 and (own == 100).all()
    rx.set_receive_eq_map(None)
    out = np.zeros((NCH, 14), np.int32)
    assert rx._lib.t41rx_get_receive_eq_map(rx._ctx, out.ctypes.data_as(i32p), NCH) == 0 and (out == 100).all()
    long = _chain(T, LONG_KW, tables=False)
    _refused(T, lambda: long.set_receive_eq_map(good), _lib.ERR_UNSUPPORTED, "fft_length 512")
    assert long.receive_eq_map is None
