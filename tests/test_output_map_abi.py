"""The output map without a GPU: t41rx_set_output_map / t41rx_get_output_map / t41rx_audio_rows are declared with
T41RX_API in include/t41rx.h, listed in exports.map, bound by _lib.SYMBOLS and exported by the built library; the header
states the audio's shapes; the ABI stays 5 (entry points are only added); a NULL context is refused before anything else
is looked at."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t41rx_set_output_map", "t41rx_get_output_map", "t41rx_audio_rows")


def _header():
    return open(os.path.join(ROOT, "include", "t41rx.h")).read()


def test_header_declares_the_entry_points_with_the_export_attribute():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"T41RX_API\s+int\s+t41rx_set_output_map\s*\(\s*t41rx_ctx\s*\*\s*ctx\s*,\s*const\s+int32_t\s*\*\s*row_of_channel\s*,"
                     r"\s*int\s+n\s*,\s*int\s+n_rows\s*\)\s*;", code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_get_output_map\s*\(\s*const\s+t41rx_ctx\s*\*\s*ctx\s*,\s*int32_t\s*\*\s*row_of_channel_out\s*,"
                     r"\s*int\s+n\s*,\s*int\s*\*\s*n_rows_out\s*\)\s*;", code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_audio_rows\s*\(\s*const\s+t41rx_ctx\s*\*\s*ctx\s*\)\s*;", code)


def test_header_states_the_shapes_and_the_semantics():
    doc = _header()
    assert "[n_rows][n_frames * audio_frame_len]" in doc and "[n_frames][n_rows][audio_frame_len]" in doc
    assert re.search(r"keep their \[n_channels\]", doc)
    assert re.search(r"interpolator memories of a muted channel stay", doc)
    assert re.search(r"No row may be named twice", doc)
    assert re.search(r"t41rx_calibrate_\*\) and the\s+\*?\s*t41rx_ft8_audio_\* entries write no audio and ignore the map", doc)
    assert re.search(r"t41rx_set_output_map\(\) answers T41RX_ERR_UNSUPPORTED", doc)


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
    assert _lib.SYMBOLS["t41rx_set_output_map"] == (C.c_int, [C.c_void_p, i32p, C.c_int, C.c_int])
    assert _lib.SYMBOLS["t41rx_get_output_map"] == (C.c_int, [C.c_void_p, i32p, C.c_int, C.POINTER(C.c_int)])
    assert _lib.SYMBOLS["t41rx_audio_rows"] == (C.c_int, [C.c_void_p])
    lib = t41_sdr_amd.load()
    assert lib.t41rx_abi_version() == 5
    raw = C.CDLL(t41_sdr_amd.LIB_PATH)
    assert all(hasattr(raw, s) for s in NEW)
    for meth in ("set_output_map", "output_map", "audio_rows"):
        assert hasattr(t41_sdr_amd.RxChain, meth)
    # a NULL context: T41RX_ERR_ARG with a text, no device needed
    m = np.zeros(4, np.int32)
    rows = C.c_int(7)
    for call in (lambda: lib.t41rx_set_output_map(None, m.ctypes.data_as(i32p), 4, 1),
                 lambda: lib.t41rx_get_output_map(None, None, 0, C.byref(rows)),
                 lambda: lib.t41rx_audio_rows(None)):
        assert call() == _lib.ERR_ARG and lib.t41rx_last_error()
    assert rows.value == 7
