"""The stage map without a GPU: t41rx_set_stage_map / t41rx_get_stage_map are declared with T41RX_API in include/t41rx.h,
listed in exports.map, bound by _lib.SYMBOLS and exported by the built library; the T41RX_STAGE_* constants of the header
are _lib.py's; the header states the rule and what the map leaves alone; the ABI stays 5 (entry points are only added); a
NULL context is refused before anything else is looked at."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t41rx_set_stage_map", "t41rx_get_stage_map")
STAGES = dict(EQ=1, NR=2, NB=4, CW_DETECT=8, CW_DECODE=16, ALL=31)


def _header():
    return open(os.path.join(ROOT, "include", "t41rx.h")).read()


def test_header_declares_the_entry_points_with_the_export_attribute():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"T41RX_API\s+int\s+t41rx_set_stage_map\s*\(\s*t41rx_ctx\s*\*\s*ctx\s*,\s*const\s+uint32_t\s*\*\s*stages_of_channel\s*,"
                     r"\s*int\s+n\s*\)\s*;", code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_get_stage_map\s*\(\s*const\s+t41rx_ctx\s*\*\s*ctx\s*,\s*uint32_t\s*\*\s*stages_of_channel_out\s*,"
                     r"\s*int\s+n\s*\)\s*;", code)


def test_constants_of_the_header_are_the_bindings():
    from t41_sdr_amd import _lib
    import t41_sdr_amd
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, want in STAGES.items():
        m = re.search(r"#define\s+T41RX_STAGE_%s\s+(\d+)u\b" % name, code)
        assert m and int(m.group(1)) == want, name
        assert getattr(_lib, "STAGE_" + name) == want and getattr(t41_sdr_amd, "STAGE_" + name) == want
    assert _lib.STAGE_ALL == _lib.STAGE_EQ | _lib.STAGE_NR | _lib.STAGE_NB | _lib.STAGE_CW_DETECT | _lib.STAGE_CW_DECODE


def test_header_states_the_rule_and_what_the_map_leaves_alone():
    doc = re.sub(r"\s*\n\s*\*\s*", " ", _header())
    assert "the context's switch for S is on" in doc and "bit S of stages_of_channel[c] is set" in doc
    assert "S's memory for the channel stays exactly as it was" in doc
    assert "T41RX_STAGE_CW_DECODE and without T41RX_STAGE_CW_DETECT" in doc
    assert re.search(r"narrow CW filter \(t41rx_set_cw_filter\) stays a switch of the context", doc)
    assert "two back ends per call" in doc
    assert "t41rx_set_stage_map() answers T41RX_ERR_UNSUPPORTED" in doc
    assert "T41RX_STAGE_ALL in every entry with none" in doc
    assert "it is in no checkpoint" in doc


def test_abi_version_is_still_5():
    assert re.search(r"#define\s+T41RX_ABI_VERSION\s+5\b", _header())


def test_export_list_names_them():
    m = re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())
    listed = set(re.findall(r"\b(t41rx_[a-z0-9_]+);", m))
    assert set(NEW) <= listed


def test_binding_carries_them(built):
    import t41_sdr_amd
    from t41_sdr_amd import _lib
    u32p = C.POINTER(C.c_uint32)
    assert _lib.SYMBOLS["t41rx_set_stage_map"] == (C.c_int, [C.c_void_p, u32p, C.c_int])
    assert _lib.SYMBOLS["t41rx_get_stage_map"] == (C.c_int, [C.c_void_p, u32p, C.c_int])
    lib = t41_sdr_amd.load()
    assert lib.t41rx_abi_version() == 5
    raw = C.CDLL(t41_sdr_amd.LIB_PATH)
    assert all(hasattr(raw, s) for s in NEW)
    assert callable(t41_sdr_amd.RxChain.set_stage_map) and isinstance(t41_sdr_amd.RxChain.stage_map, property)
    assert t41_sdr_amd.RxChain.set_stage_map.__doc__ and t41_sdr_amd.RxChain.stage_map.__doc__
    # a NULL context: T41RX_ERR_ARG with a text, no device needed
    m = np.full(4, 31, np.uint32)
    for call in (lambda: lib.t41rx_set_stage_map(None, m.ctypes.data_as(u32p), 4),
                 lambda: lib.t41rx_get_stage_map(None, m.ctypes.data_as(u32p), 4)):
        assert call() == _lib.ERR_ARG and lib.t41rx_last_error()
    assert (m == 31).all()
