"""The GPU-side driver of the receive tests, once: sample formats, buffer layouts, one process call, a stream cut into
calls, and the small checks the stage tests share.  A test file keeps what is its own -- which signal it generates,
which setters it calls on the chain, which q15 scale it uses -- as a thin wrapper over calls().  Pure numpy up to
one_call(); torch and the package are imported where a device is used.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5  # the whole-path bar (test_gpu_parity.py's docstring): block-relative error against the oracle


def to_q15(x, scale=1.0):
    """float samples as the ADC's int16: x * 32768 * scale, numpy's round-half-even, saturated"""
    return np.clip(np.round(x * 32768.0 * scale), -32768, 32767).astype(np.int16)


def to_time_major(x, nch, nfr, L):
    """channel-major [nch, nfr * L] -> time-major [nfr, nch, L], contiguous"""
    return np.ascontiguousarray(x.reshape(nch, nfr, L).transpose(1, 0, 2))


def from_time_major(o, nch, nfr, L):
    """time-major [nfr, nch, L] -> channel-major [nch, nfr * L]"""
    return o.reshape(nfr, nch, L).transpose(1, 0, 2).reshape(nch, nfr * L)


def pack(i, q, layout="channel", q15_scale=None, L=2048):
    """channel-major rows [rows, nfr * L] as the contiguous argument tuple of the entry point that takes them: int16
    rows (given so, or converted here with q15_scale) go to ProcessIQData_q15, everything else to ProcessIQData"""
    if q15_scale is not None:
        i, q = to_q15(i, q15_scale), to_q15(q, q15_scale)
    if layout == "time":
        rows, nfr = i.shape[0], i.shape[1] // L
        i, q = to_time_major(i, rows, nfr, L), to_time_major(q, rows, nfr, L)
    i, q = np.ascontiguousarray(i), np.ascontiguousarray(q)
    # the q15 entry points take (Q, I): the firmware's I comes from the R queue (Process.cpp:107)
    return (q, i) if i.dtype == np.int16 else (i, q)


def one_call(rx, i, q, *, layout="channel", q15_scale=None, tap_floats=None, host=False):
    """one process call on channel-major numpy rows: (audio [n_channels, nfr * L], demod tap [n_channels, nfr *
    tap_floats] or None).  layout says how the context was set up (the caller calls set_buffer_layout); host=True
    hands numpy arrays to the host-pointer form of the entry point."""
    L, nch = rx.frame_len, rx.n_channels
    nfr = i.shape[1] // L
    tap = None
    if tap_floats:
        import torch
        tap = torch.zeros(nch, nfr * tap_floats, device="cuda")
        rx.set_debug_taps(demod=tap)
    args = pack(i, q, layout, q15_scale, L)
    entry = rx.ProcessIQData_q15 if args[0].dtype == np.int16 else rx.ProcessIQData
    if not host:
        import torch
        args = tuple(torch.from_numpy(v).cuda() for v in args)
    out = entry(*args)
    if not host:
        out = out.cpu().numpy()
    assert out.shape == ((nfr, nch, L) if layout == "time" else (nch, nfr * L))
    if layout == "time":
        out = from_time_major(out, nch, nfr, L)
    return out, None if tap is None else tap.cpu().numpy()


def calls(rx, I, Q, edges, *, after=None, **one_call_options):
    """the stream in calls of frames edges[k] .. edges[k + 1]: (audio, demod tap or None, [after(rx, a, b) per call]),
    audio and tap concatenated along the samples"""
    L = rx.frame_len
    outs, taps, seen = [], [], []
    for a, b in zip(edges[:-1], edges[1:]):
        o, t = one_call(rx, I[:, a * L:b * L], Q[:, a * L:b * L], **one_call_options)
        outs.append(o)
        taps.append(t)
        if after is not None:
            seen.append(after(rx, a, b))
    return np.concatenate(outs, axis=1), None if taps[0] is None else np.concatenate(taps, axis=1), seen


@pytest.fixture(scope="module")
def T(built):
    """the loaded package, on a machine with a device (a test file imports the fixture by name)"""
    import torch
    import t41_sdr_amd
    assert torch.cuda.is_available()
    t41_sdr_amd.load()
    return t41_sdr_amd


def refused(fn, status, *words):
    """fn() raises T41RxError with this status and a message that holds every one of words"""
    import t41_sdr_amd as T
    with pytest.raises(T.T41RxError) as ei:
        fn()
    assert ei.value.status == status, ei.value
    for w in words:
        assert w in str(ei.value), ei.value


def assert_entry_points(names, methods=(), abi_version=None, pattern=r"\b%s\s*\("):
    """every name is declared in include/t41rx.h (pattern % name), listed in exports.map, bound by _lib.SYMBOLS and
    exported by the built library; RxChain has the methods; the header states the ABI version.  Returns the header."""
    import t41_sdr_amd._lib as lib
    hdr = open(os.path.join(ROOT, "include", "t41rx.h")).read()
    m = open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read()
    for name in names:
        assert re.search(pattern % name, hdr) and (name + ";") in m and name in lib.SYMBOLS, name
        assert hasattr(C.CDLL(lib.LIB_PATH), name)
    if methods:
        import t41_sdr_amd as T
        for meth in methods:
            assert hasattr(T.RxChain, meth)
    if abi_version is not None:
        assert "T41RX_ABI_VERSION %d" % abi_version in hdr
    return hdr
