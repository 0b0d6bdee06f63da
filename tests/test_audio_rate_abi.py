"""Audio at 24 kS/s without a GPU: t41rx_set_audio_rate / t41rx_get_audio_rate / t41rx_audio_frame_len are declared with
T41RX_API in include/t41rx.h, listed in exports.map, bound by _lib.SYMBOLS and exported by the built library; the ABI
stays 5 (entry points are only added); a NULL context is refused before anything else is looked at; the Python layer
refuses an unknown rate and a wrongly shaped output before it calls the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from rx_harness import assert_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t41rx_set_audio_rate", "t41rx_get_audio_rate", "t41rx_audio_frame_len")


def _header():
    return open(os.path.join(ROOT, "include", "t41rx.h")).read()


def test_header_declares_the_entry_points_and_the_rates():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"T41RX_API\s+int\s+t41rx_set_audio_rate\s*\(\s*t41rx_ctx\s*\*\s*ctx\s*,\s*int\s+rate\s*\)\s*;", code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_get_audio_rate\s*\(\s*const\s+t41rx_ctx\s*\*\s*ctx\s*\)\s*;", code)
    assert re.search(r"T41RX_API\s+int\s+t41rx_audio_frame_len\s*\(\s*const\s+t41rx_ctx\s*\*\s*ctx\s*\)\s*;", code)
    assert re.search(r"#define\s+T41RX_AUDIO_RATE_192K\s+0\b", code) and re.search(r"#define\s+T41RX_AUDIO_RATE_24K\s+1\b", code)
    # the header says what the samples are, which shapes the calls write, and what becomes of the interpolator memories
    doc = _header()
    assert "[n_channels][n_frames * 256]" in doc and "[n_frames][n_channels][256]" in doc
    assert "VolumeToAmplification(audioVolume)" in doc and "Process.cpp:917" in doc
    assert re.search(r"interpolators continue from what they last held", re.sub(r"\s*\n \*\s*", " ", doc))


def test_abi_version_is_still_5():
    assert re.search(r"#define\s+T41RX_ABI_VERSION\s+5\b", _header())


def test_export_list_names_them():
    m = re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())
    assert set(NEW) <= set(re.findall(r"\b(t41rx_[a-z0-9_]+);", m))


def test_binding_carries_them(built):
    import t41_sdr_amd
    from t41_sdr_amd import _lib
    assert_entry_points(NEW, methods=("set_audio_rate", "audio_rate", "audio_frame_len"), abi_version=5)
    assert _lib.SYMBOLS["t41rx_set_audio_rate"] == (C.c_int, [C.c_void_p, C.c_int])
    assert _lib.SYMBOLS["t41rx_get_audio_rate"] == (C.c_int, [C.c_void_p])
    assert _lib.SYMBOLS["t41rx_audio_frame_len"] == (C.c_int, [C.c_void_p])
    lib = t41_sdr_amd.load()
    assert lib.t41rx_abi_version() == 5
    # a NULL context: T41RX_ERR_ARG, no device needed; the setter leaves a text
    assert lib.t41rx_set_audio_rate(None, 1) == _lib.ERR_ARG and lib.t41rx_last_error()
    assert lib.t41rx_get_audio_rate(None) == _lib.ERR_ARG
    assert lib.t41rx_audio_frame_len(None) == _lib.ERR_ARG


class _NoLibrary:
    """stands in for the loaded library on an object made with __new__: any call into it fails the test"""

    def __getattr__(self, name):
        def entry(*args):
            raise AssertionError("the Python layer called %s before it refused" % name)
        return entry


def _bare(layout="channel", rate=None, nch=3):
    import t41_sdr_amd as T
    rx = T.RxChain.__new__(T.RxChain)
    rx._lib, rx._ctx = _NoLibrary(), None
    rx.n_channels, rx.device, rx.frame_len, rx.layout, rx._n_streams = nch, 0, 2048, layout, 0
    if rate is not None:
        rx._audio_rate = rate
    return rx


def test_python_layer_refuses_an_unknown_rate(built):
    rx = _bare()
    assert rx.audio_rate == 192000 and rx.audio_frame_len == 2048  # an object that never set a rate
    for bad in (48000, 12000, 8000, 0, 1, 24000.5, "24000", None, True):
        with pytest.raises(ValueError, match="24000 or 192000"):
            rx.set_audio_rate(bad)
    assert rx.audio_rate == 192000 and rx.audio_frame_len == 2048


def test_python_layer_refuses_a_wrong_output_shape(built):
    i = np.zeros((3, 2 * 2048), np.float32)
    # 24 kS/s: 256 samples per channel and frame, in either layout; the 192 kS/s shape is refused, and the other way round
    rx = _bare(rate=24000)
    assert rx.audio_frame_len == 256 and rx._out_shape(2) == (3, 512)
    for wrong in ((3, 2 * 2048), (3, 256), (2, 512), (512, 3)):
        with pytest.raises(ValueError, match="shape"):
            rx.ProcessIQData(i, i, out=np.zeros(wrong, np.float32))
    with pytest.raises(ValueError, match="shape"):
        rx.ProcessIQData(i, i, out=np.zeros((3, 512), np.int16))  # right shape, wrong type
    with pytest.raises(ValueError, match="shape"):
        rx.ProcessIQData_q15(i.astype(np.int16), i.astype(np.int16), out=np.zeros((3, 2 * 2048), np.int16))
    with pytest.raises(ValueError, match="shape"):
        _bare(rate=192000).ProcessIQData(i, i, out=np.zeros((3, 512), np.float32))
    rt = _bare("time", rate=24000)
    it = np.zeros((2, 3, 2048), np.float32)
    assert rt._out_shape(2) == (2, 3, 256)
    for wrong in ((2, 3, 2048), (3, 2, 256), (3, 512)):
        with pytest.raises(ValueError, match="shape"):
            rt.ProcessIQData(it, it, out=np.zeros(wrong, np.float32))
    # the inputs keep their frames of frame_len samples at either rate
    with pytest.raises(ValueError, match="frame_len"):
        rx.ProcessIQData(np.zeros((3, 512), np.float32), np.zeros((3, 512), np.float32))
