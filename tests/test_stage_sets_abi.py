"""Parameter sets next to the chain-splitting stages at the ABI: t41rx_set_param_sets_ex, t41rx_get_param_sets_flags and
t41rx_param_sets_compatible_ex are declared with T41RX_API in include/t41rx.h, listed in exports.map, bound by _lib.SYMBOLS
and exported by the built library; T41RX_SETS_STAGES is 1; the header states the rule and no longer says that the refusal
stands unconditionally; the ABI stays 5; a NULL context is refused before anything else is looked at; the rule on two
structs with and without the flag (it needs no context); the Python layer's own refusals on an object made with __new__ (no
context is created).  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t41rx_set_param_sets_ex", "t41rx_get_param_sets_flags", "t41rx_param_sets_compatible_ex")
N = 3


def _header():
    return open(os.path.join(ROOT, "include", "t41rx.h")).read()


@pytest.fixture
def T(built):
    import t41_sdr_amd
    return t41_sdr_amd


def test_header_declares_the_entry_points_with_the_export_attribute():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    P = r"const\s+t41rx_params\s*\*\s*"
    assert re.search(r"T41RX_API\s+int\s+t41rx_set_param_sets_ex\s*\(\s*t41rx_ctx\s*\*\s*ctx\s*,\s*%ssets\s*,\s*int\s+n_sets\s*,\s*"
                     r"const\s+int32_t\s*\*\s*set_of_channel\s*,\s*int\s+n\s*,\s*int32_t\s+flags\s*\)\s*;" % P, code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_get_param_sets_flags\s*\(\s*const\s+t41rx_ctx\s*\*\s*ctx\s*\)\s*;", code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_param_sets_compatible_ex\s*\(\s*%sa\s*,\s*%sb\s*,\s*int32_t\s+flags\s*\)\s*;" % (P, P), code)
    assert re.search(r"#define\s+T41RX_SETS_STAGES\s+1u\b", code)
    assert re.search(r"#define\s+T41RX_ABI_VERSION\s+5\b", code)


def test_header_states_the_rule():
    doc = re.sub(r"\s*\n\s*\*\s*", " ", _header())
    assert "go on refusing each other" not in doc
    assert doc.count("stands for sets loaded without T41RX_SETS_STAGES") >= 2
    assert "flags == 0 is t41rx_set_param_sets() / t41rx_param_sets_compatible() word for word" in doc
    assert "an unknown flag bit returns T41RX_ERR_ARG" in doc
    assert "keeps every clause except \"both 0\" on nrOptionSelect / ANR_notchOn" in doc
    assert "the channel takes its own set's NR_alpha, NR_beta, NR_PSI and the VAD range of its own pass band" in doc
    assert "the text names the channel and the set" in doc
    assert "refused as such (T41RX_ERR_ARG, \"set i is invalid\") whether a channel names it or not" in doc
    assert "leaves loaded staged sets in place" in doc


def test_export_list_and_binding_carry_them(T):
    from t41_sdr_amd import _lib
    m = re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())
    assert set(NEW) <= set(re.findall(r"\b(t41rx_[a-z0-9_]+);", m))
    pp, i32p = C.POINTER(_lib.Params), C.POINTER(C.c_int32)
    assert _lib.SYMBOLS["t41rx_set_param_sets_ex"] == (C.c_int, [C.c_void_p, pp, C.c_int, i32p, C.c_int, C.c_int32])
    assert _lib.SYMBOLS["t41rx_get_param_sets_flags"] == (C.c_int, [C.c_void_p])
    assert _lib.SYMBOLS["t41rx_param_sets_compatible_ex"] == (C.c_int, [pp, pp, C.c_int32])
    assert _lib.SETS_STAGES == 1 and T.SETS_STAGES == 1
    lib = T.load()
    assert lib.t41rx_abi_version() == 5
    raw = C.CDLL(T.LIB_PATH)
    assert all(hasattr(raw, s) for s in NEW)
    # a NULL context: T41RX_ERR_ARG with a text, no device needed, whatever the flags say
    sets = (_lib.Params * 1)(T.default_params())
    table = np.zeros(4, np.int32)
    for flags in (0, 1, 2):
        assert lib.t41rx_set_param_sets_ex(None, sets, 1, table.ctypes.data_as(i32p), 4, flags) == _lib.ERR_ARG and lib.t41rx_last_error()
        assert b"null argument" in lib.t41rx_last_error()
    assert lib.t41rx_get_param_sets_flags(None) == _lib.ERR_ARG and b"null argument" in lib.t41rx_last_error()
    assert (table == 0).all()


def test_the_rule_with_and_without_the_flag(T):
    """t41rx_param_sets_compatible_ex needs no context: flags 0 is the old entry word for word, the flag drops the one
    clause on nrOptionSelect / ANR_notchOn and keeps the others, an unknown bit and a NULL are T41RX_ERR_ARG"""
    from t41_sdr_amd import _lib
    lib = T.load()
    usb = dict(mode=0, FLoCut=200, FHiCut=3000)
    a = T.default_params(**usb)
    text = lambda: lib.t41rx_last_error().decode()  # noqa: E731
    for change in (dict(nrOptionSelect=1), dict(nrOptionSelect=2), dict(nrOptionSelect=3, ANR_notchOn=1), dict(ANR_notchOn=1)):
        b = T.default_params(**dict(usb, **change))
        assert lib.t41rx_param_sets_compatible(C.byref(a), C.byref(b)) == _lib.ERR_UNSUPPORTED
        old = text()
        assert "noise reduction / notch" in old and "both must be 0" in old
        assert lib.t41rx_param_sets_compatible_ex(C.byref(a), C.byref(b), 0) == _lib.ERR_UNSUPPORTED and text() == old
        assert lib.t41rx_param_sets_compatible_ex(C.byref(a), C.byref(b), 1) == 0
        assert lib.t41rx_param_sets_compatible_ex(C.byref(b), C.byref(a), 1) == 0
        assert T.param_sets_compatible(a, b) == (False, old) and T.param_sets_compatible(a, b, stages=True) == (True, "")
    for word, change in (("demodulators", dict(mode=2, FLoCut=-4000, FHiCut=4000)), ("AGC", dict(AGCMode=2)), ("xmtMode", dict(xmtMode=1)),
                         ("gains", dict(RFgain=2)), ("fft_length", dict(fft_length=1024, FLoCut=400, FHiCut=600))):
        b = T.default_params(**dict(usb, nrOptionSelect=0, **change))
        for flags in (0, 1):
            assert lib.t41rx_param_sets_compatible_ex(C.byref(a), C.byref(b), flags) == _lib.ERR_UNSUPPORTED, (change, flags)
            assert word in text(), (change, flags, text())
        assert lib.t41rx_param_sets_compatible(C.byref(a), C.byref(b)) == _lib.ERR_UNSUPPORTED
        old = text()
        assert lib.t41rx_param_sets_compatible_ex(C.byref(a), C.byref(b), 0) == _lib.ERR_UNSUPPORTED and text() == old
    # the long lengths stay refused under the flag, in the same words
    lng = T.default_params(fft_length=2048, mode=0, FLoCut=400, FHiCut=600)
    assert lib.t41rx_param_sets_compatible_ex(C.byref(lng), C.byref(lng), 1) == _lib.ERR_UNSUPPORTED and "long-FFT" in text()
    for flags in (2, 3, -1, -(1 << 31)):
        assert lib.t41rx_param_sets_compatible_ex(C.byref(a), C.byref(a), flags) == _lib.ERR_ARG and "unknown flag" in text()
    assert lib.t41rx_param_sets_compatible_ex(None, C.byref(a), 1) == _lib.ERR_ARG
    assert lib.t41rx_param_sets_compatible_ex(C.byref(a), None, 1) == _lib.ERR_ARG
    # an invalid struct: a spectral set whose pass band fails the function's array-bounds check
    bad = T.default_params(mode=0, FLoCut=300, FHiCut=1000, nrOptionSelect=2)
    assert lib.t41rx_param_sets_compatible_ex(C.byref(a), C.byref(bad), 1) == _lib.ERR_ARG and "second struct is invalid" in text()


def test_docstrings_exist(T):
    f = T.RxChain.set_param_sets
    assert callable(f) and "t41rx_set_param_sets_ex" in f.__doc__ and "stages=True" in f.__doc__
    p = T.RxChain.param_sets_stages
    assert isinstance(p, property) and p.__doc__ and "t41rx_get_param_sets_flags" in p.__doc__
    assert "stages=True" in T.param_sets_compatible.__doc__


def test_python_layer_refusals(T):
    """what rx.py refuses before it calls the library (ValueError, the message whole), and valid arguments, which the null
    context makes the C side refuse with T41RX_ERR_ARG"""
    from t41_sdr_amd import _lib
    rx = T.RxChain.__new__(T.RxChain)
    rx._lib, rx._ctx, rx.params = _lib.load(), C.c_void_p(), T.default_params()
    rx.n_channels, rx.device, rx.frame_len, rx.layout, rx._n_streams = N, 0, 2048, "channel", 0

    def refused(message, *args, **kw):
        with pytest.raises(ValueError) as e:
            rx.set_param_sets(*args, **kw)
        assert type(e.value) is ValueError and str(e.value) == message, (str(e.value), message)

    refused("stages must be False or True, got 2", [dict(FHiCut=2400)], [0, 1, 0], stages=2)
    refused("stages must be False or True, got 'yes'", [dict(FHiCut=2400)], [0, 1, 0], stages="yes")
    refused("set_of_channel goes with sets: pass both, or None to remove the sets", None, [0, 1, 0], stages=True)
    refused("set_of_channel must be given with sets: n_channels=3 set numbers in [0, 1]", [dict(FHiCut=2400)], stages=True)
    refused("sets[0] must be a t41rx_params or a dict of changes against set 0, got int", [5], [0, 1, 0], stages=True)
    refused("set_of_channel must be a 1-d array of int32 set numbers, got (3,) float64", [dict(FHiCut=2400)], [0.0, 1.0, 0.0], stages=True)
    for call in (lambda: rx.set_param_sets([dict(FHiCut=2400, nrOptionSelect=1)], [0, 1, 0], stages=True),
                 lambda: rx.set_param_sets([dict(FHiCut=2400)], np.zeros(3, np.int32), stages=False),
                 lambda: rx.set_param_sets(None, stages=True), lambda: rx.param_sets_stages):
        with pytest.raises(T.T41RxError) as e:
            call()
        assert e.value.status == _lib.ERR_ARG
