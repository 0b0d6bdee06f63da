"""Parameter sets without a GPU: the three entry points and T41RX_MAX_PARAM_SETS are declared in include/t41rx.h, listed
in exports.map, bound by _lib.SYMBOLS and exported by the built library; the ABI stays 5.  The compatibility rule
(t41rx_param_sets_compatible: host only, no context) on a table of pairs that covers every clause, both results, the
reason text non-empty.  The Python layer's own refusals, on an object made with __new__ (no context is created)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t41rx_set_param_sets", "t41rx_get_param_sets", "t41rx_param_sets_compatible")
N = 3


def _header():
    return open(os.path.join(ROOT, "include", "t41rx.h")).read()


@pytest.fixture
def T(built):
    import t41_sdr_amd
    return t41_sdr_amd


def test_header_declares_the_entry_points_and_the_cap():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"T41RX_API\s+int\s+t41rx_set_param_sets\s*\(\s*t41rx_ctx\s*\*\s*ctx\s*,\s*const\s+t41rx_params\s*\*\s*sets\s*,\s*int\s+n_sets\s*,"
                     r"\s*const\s+int32_t\s*\*\s*set_of_channel\s*,\s*int\s+n\s*\)\s*;", code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_get_param_sets\s*\(\s*const\s+t41rx_ctx\s*\*\s*ctx\s*,\s*t41rx_params\s*\*\s*sets_out\s*,\s*int\s+cap\s*,"
                     r"\s*int32_t\s*\*\s*set_of_channel_out\s*,\s*int\s+n\s*\)\s*;", code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_param_sets_compatible\s*\(\s*const\s+t41rx_params\s*\*\s*a\s*,\s*const\s+t41rx_params\s*\*\s*b\s*\)\s*;", code)
    assert re.search(r"#define\s+T41RX_MAX_PARAM_SETS\s+64\b", code)
    assert re.search(r"#define\s+T41RX_ABI_VERSION\s+5\b", code)
    # the header states the rule: what must be equal, what is free
    doc = _header()
    for word in ("fft_length", "demodulator family", "AGC off", "nfm_demod", "xmtMode", "nrOptionSelect", "ANR_notchOn", "plain",
                 "Free to differ", "audioVolume", "AGC_thresh", "am_lpf_f0", "nfmFilterBW", "CWFreqShift"):
        assert word in doc, word


def test_export_list_and_binding_carry_them(T):
    from t41_sdr_amd import _lib
    m = re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())
    assert set(NEW) <= set(re.findall(r"\b(t41rx_[a-z0-9_]+);", m))
    pp, i32p = C.POINTER(_lib.Params), C.POINTER(C.c_int32)
    assert _lib.SYMBOLS["t41rx_set_param_sets"] == (C.c_int, [C.c_void_p, pp, C.c_int, i32p, C.c_int])
    assert _lib.SYMBOLS["t41rx_get_param_sets"] == (C.c_int, [C.c_void_p, pp, C.c_int, i32p, C.c_int])
    assert _lib.SYMBOLS["t41rx_param_sets_compatible"] == (C.c_int, [pp, pp])
    lib = T.load()
    assert lib.t41rx_abi_version() == 5
    raw = C.CDLL(T.LIB_PATH)
    assert all(hasattr(raw, s) for s in NEW)
    for meth in ("set_param_sets", "param_sets", "set_of_channel"):
        assert hasattr(T.RxChain, meth)
    # a NULL context: T41RX_ERR_ARG with a text, no device needed
    m4 = np.zeros(4, np.int32)
    sets = (_lib.Params * 1)(T.default_params())
    assert lib.t41rx_set_param_sets(None, sets, 1, m4.ctypes.data_as(i32p), 4) == _lib.ERR_ARG and lib.t41rx_last_error()
    assert lib.t41rx_get_param_sets(None, None, 0, None, 0) == _lib.ERR_ARG and lib.t41rx_last_error()


USB = dict(mode=0, FLoCut=200, FHiCut=3000)
LSB = dict(mode=1, FLoCut=-3000, FHiCut=-200)
AM = dict(mode=2, FLoCut=-4000, FHiCut=4000)
NFM = dict(mode=3, FLoCut=200, FHiCut=3000)
SAM = dict(mode=8, FLoCut=-4000, FHiCut=4000)
GEN = dict(RFgain=2, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=0.01)
# (a, b, None when compatible or a word of the reason)
PAIRS = [
    # free to differ
    (USB, USB, None), (USB, LSB, None), (LSB, USB, None),
    (USB, dict(USB, FLoCut=300, FHiCut=1000), None),
    (USB, dict(USB, rfGainAllBands=9), None),
    (USB, dict(USB, audioVolume=70), None),
    (dict(USB, **GEN), dict(LSB, RFgain=3, IQAmpCorrectionFactor=0.9, IQPhaseCorrectionFactor=-0.02, rfGainAllBands=4), None),
    (dict(USB, **GEN), dict(USB, RFgain=1, IQAmpCorrectionFactor=1.0, IQPhaseCorrectionFactor=0.03), None),
    (dict(USB, AGCMode=1, AGC_thresh=20), dict(LSB, AGCMode=4, AGC_thresh=5), None),
    (dict(USB, AGCMode=2), dict(USB, AGCMode=3), None),
    (dict(AM, am_lpf_f0=3000), dict(AM, am_lpf_f0=2000, FLoCut=-2500, FHiCut=2500), None),
    (dict(NFM, nfmFilterBW=12000), dict(NFM, nfmFilterBW=8000), None),
    (dict(NFM, nfm_demod=1), dict(NFM, nfm_demod=1, nfmFilterBW=8000), None),
    (SAM, dict(SAM, FLoCut=-2500, FHiCut=2500), None),
    (dict(USB, xmtMode=1, CWFreqShift=750), dict(LSB, xmtMode=1, CWFreqShift=562), None),
    (dict(NFM, RFgain=1, IQAmpCorrectionFactor=1.02), dict(NFM, IQPhaseCorrectionFactor=0.5), None),  # NFM: no IQ correction, both plain
    (USB, dict(USB, NR_alpha=0.9, NR_beta=0.8), None),
    # must be equal
    (USB, dict(USB, fft_length=1024, FLoCut=400, FHiCut=600), "fft_length differs"),
    (dict(USB, fft_length=4096, FLoCut=400, FHiCut=600), dict(USB, fft_length=4096, FLoCut=400, FHiCut=700), "long-FFT"),
    (USB, AM, "demodulators"), (USB, NFM, "demodulators"), (LSB, SAM, "demodulators"), (AM, SAM, "demodulators"), (AM, NFM, "demodulators"),
    (USB, dict(USB, AGCMode=1), "AGC"), (dict(LSB, AGCMode=4), LSB, "AGC"),
    (NFM, dict(NFM, nfm_demod=1), "nfm_demod"),
    (USB, dict(USB, xmtMode=1), "xmtMode"), (dict(USB, xmtMode=2), USB, "xmtMode"),
    (USB, dict(USB, nrOptionSelect=1), "noise reduction"), (dict(USB, nrOptionSelect=3), dict(USB, nrOptionSelect=3), "noise reduction"),
    (dict(USB, ANR_notchOn=1), USB, "noise reduction"), (dict(USB, ANR_notchOn=1), dict(USB, ANR_notchOn=1), "noise reduction"),
    (USB, dict(USB, RFgain=2), "gains"), (USB, dict(USB, IQAmpCorrectionFactor=1.02), "gains"), (dict(USB, IQPhaseCorrectionFactor=0.01), USB, "gains"),
    (NFM, dict(NFM, RFgain=2), "gains"),
]


@pytest.mark.parametrize("i", range(len(PAIRS)))
def test_compatibility_rule(T, i):
    from t41_sdr_amd import _lib
    a, b, why = PAIRS[i]
    pa, pb = T.default_params(**a), T.default_params(**b)
    lib = T.load()
    rc = lib.t41rx_param_sets_compatible(C.byref(pa), C.byref(pb))
    if why is None:
        assert rc == 0, lib.t41rx_last_error()
        assert T.param_sets_compatible(pa, pb) == (True, "") and T.param_sets_compatible(pb, pa) == (True, "")
    else:
        msg = lib.t41rx_last_error().decode()
        assert rc == _lib.ERR_UNSUPPORTED and msg and why in msg, (rc, msg)
        ok, reason = T.param_sets_compatible(pb, pa)  # the rule is symmetric
        assert not ok and why in reason


def test_compatibility_rule_refuses_what_is_not_a_parameter_set(T):
    from t41_sdr_amd import _lib
    lib = T.load()
    good, bad = T.default_params(), T.default_params(FLoCut=3000, FHiCut=200)
    assert lib.t41rx_param_sets_compatible(None, C.byref(good)) == _lib.ERR_ARG and lib.t41rx_last_error()
    assert lib.t41rx_param_sets_compatible(C.byref(good), None) == _lib.ERR_ARG
    assert lib.t41rx_param_sets_compatible(C.byref(good), C.byref(bad)) == _lib.ERR_ARG and b"FHiCut" in lib.t41rx_last_error()
    with pytest.raises(T.T41RxError):
        T.param_sets_compatible(bad, good)


def test_python_layer_refusals(T):
    """what rx.py refuses before it calls the library, and one valid argument set, which the null context makes the C
    side refuse with T41RX_ERR_ARG"""
    from t41_sdr_amd import _lib
    rx = T.RxChain.__new__(T.RxChain)
    rx._lib, rx._ctx, rx.params = _lib.load(), C.c_void_p(), T.default_params()
    rx.n_channels, rx.device, rx.frame_len, rx.layout, rx._n_streams = N, 0, 2048, "channel", 0

    def refused(exc, message, *a, **kw):
        with pytest.raises(exc) as e:
            rx.set_param_sets(*a, **kw)
        assert type(e.value) is exc and str(e.value) == message, (str(e.value), message)

    refused(ValueError, "set_of_channel goes with sets: pass both, or None to remove the sets", None, [0, 0, 0])
    refused(ValueError, "set_of_channel must be given with sets: n_channels=3 set numbers in [0, 1]", [dict(FHiCut=2400)])
    refused(ValueError, "sets[1] must be a t41rx_params or a dict of changes against set 0, got int", [dict(FHiCut=2400), 7], [0, 1, 2])
    refused(AttributeError, "t41rx_params has no field 'nope'", [dict(nope=1)], [0, 1, 1])
    refused(ValueError, "set_of_channel must be a 1-d array of int32 set numbers, got (3,) float64", [dict(FHiCut=2400)], [0.0, 1.0, 1.0])
    refused(ValueError, "set_of_channel must be a 1-d array of int32 set numbers, got (1, 3) int64", [dict(FHiCut=2400)], [[0, 1, 1]])
    before = bytes(rx.params)
    for args in (([dict(FHiCut=2400)], [0, 1, 1]), ([T.default_params(mode=1, FLoCut=-3000, FHiCut=-200)], np.array([1, 0, 1], np.int32)), (None,)):
        with pytest.raises(T.T41RxError) as e:
            rx.set_param_sets(*args)
        assert e.value.status == _lib.ERR_ARG
    for prop in ("param_sets", "set_of_channel"):
        with pytest.raises(T.T41RxError) as e:
            getattr(rx, prop)
        assert e.value.status == _lib.ERR_ARG
    assert bytes(rx.params) == before  # a dict of changes does not touch set 0
