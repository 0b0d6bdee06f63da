"""Receiver groups without a GPU: t41rx_set_input_map / t41rx_get_input_map are declared with T41RX_API in
include/t41rx.h, listed in exports.map, bound by _lib.SYMBOLS and exported by the built library; the ABI stays 5 (entry
points are only added); a NULL context is refused before anything else is looked at."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t41rx_set_input_map", "t41rx_get_input_map")


def _header():
    return open(os.path.join(ROOT, "include", "t41rx.h")).read()


def test_header_declares_the_entry_points_with_the_export_attribute():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"T41RX_API\s+int\s+t41rx_set_input_map\s*\(\s*t41rx_ctx\s*\*\s*ctx\s*,\s*const\s+int32_t\s*\*\s*stream_of_channel\s*,"
                     r"\s*int\s+n\s*,\s*int\s+n_streams\s*\)\s*;", code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_get_input_map\s*\(\s*const\s+t41rx_ctx\s*\*\s*ctx\s*,\s*int32_t\s*\*\s*stream_of_channel_out\s*,"
                     r"\s*int\s+n\s*\)\s*;", code)
    # the header says what the map does to the process calls' shapes and that the calibration ignores it
    doc = _header()
    assert "[n_streams][n_frames * frame_len]" in doc and "[n_frames][n_streams][frame_len]" in doc
    assert re.search(r"calibration calls[^.]*ignore (it|the map)", doc)


def test_abi_version_is_still_5():
    assert re.search(r"#define\s+T41RX_ABI_VERSION\s+5\b", _header())


def test_export_list_names_them():
    m = re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())
    listed = set(re.findall(r"\b(t41rx_[a-z0-9_]+);", m))
    assert set(NEW) <= listed


def test_binding_carries_them(built):
    import t41_sdr_amd
    from t41_sdr_amd import _lib
    i32p = C.POINTER(C.c_int32)
    assert _lib.SYMBOLS["t41rx_set_input_map"] == (C.c_int, [C.c_void_p, i32p, C.c_int, C.c_int])
    assert _lib.SYMBOLS["t41rx_get_input_map"] == (C.c_int, [C.c_void_p, i32p, C.c_int])
    lib = t41_sdr_amd.load()
    assert lib.t41rx_abi_version() == 5
    raw = C.CDLL(t41_sdr_amd.LIB_PATH)
    assert all(hasattr(raw, s) for s in NEW)
    for meth in ("set_input_map", "input_map", "n_streams"):
        assert hasattr(t41_sdr_amd.RxChain, meth)
    # a NULL context: T41RX_ERR_ARG with a text, no device needed
    m = np.zeros(4, np.int32)
    assert lib.t41rx_set_input_map(None, m.ctypes.data_as(i32p), 4, 1) == _lib.ERR_ARG and lib.t41rx_last_error()
    assert lib.t41rx_get_input_map(None, None, 0) == _lib.ERR_ARG
