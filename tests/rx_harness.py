"""The GPU-side driver of the receive tests, once: sample formats, buffer layouts, one process call (its rows, frame
length and layout taken from the chain), a stream cut into calls, and the small checks the stage tests share.  A test file keeps what is its own -- which signal it generates,
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
ERR_ARG, ERR_UNSUPPORTED = -1, -2  # T41RX_ERR_ARG, T41RX_ERR_UNSUPPORTED (include/t41rx.h)
INT1, INT2 = slice(152, 176), slice(176, 184)  # kStInt1, kStInt2 in a channel's state record (rx_internal.hpp): the x2 and x4 interpolator memories
SENT_F32, SENT_Q15 = np.float32(-7777.25), np.int16(0x5A5A)  # what one_call(guard=True) prefills the audio buffer with
GUARD = 512  # samples behind the audio's rows that must keep the sentinel


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


def streams(rows, nsamp, seed, q15=False):
    """distinct random samples per row [rows, nsamp]: a wrong row cannot pass"""
    rng = np.random.default_rng(seed)
    I = (0.2 * rng.standard_normal((rows, nsamp))).astype(np.float32)
    Q = (0.2 * rng.standard_normal((rows, nsamp))).astype(np.float32)
    if q15:
        I, Q = to_q15(I), to_q15(Q)
    return I, Q


def sentinel_of(a):
    return SENT_Q15 if a.dtype == np.int16 else SENT_F32


def guarded_call(entry, args, shape, sent, host):
    """entry(*args, out=) into a sentinel-filled buffer of this shape with GUARD samples behind it: the entry returns that
    very object and leaves the guard alone.  Returns the buffer's rows as numpy, what nobody wrote still the sentinel."""
    n = int(np.prod(shape))
    if host:
        big = np.full(n + GUARD, sent, sent.dtype)
        out = big[:n].reshape(shape)
        assert entry(*args, out=out) is out
    else:
        import torch
        q15 = sent.dtype == np.int16
        big = torch.full((n + GUARD,), int(sent) if q15 else float(sent), dtype=torch.int16 if q15 else torch.float32, device="cuda")
        out = big[:n].view(shape)
        assert entry(*args, out=out) is out
        torch.cuda.synchronize()
        big = big.cpu().numpy()
    assert (big[n:] == sent).all(), "the call wrote behind the audio's rows"
    return big[:n].reshape(shape)


def one_call(rx, i, q, *, layout=None, q15_scale=None, tap_floats=None, host=False, guard=False):
    """one process call on channel-major numpy rows [input rows, nfr * frame_len]: (audio [audio_rows, nfr *
    audio_frame_len], demod tap [n_channels, nfr * tap_floats] or None).  The rows and the frame length of the audio are
    the chain's (audio_rows, audio_frame_len; n_channels and frame_len for a chain that has neither), the layout is the
    chain's unless given (the caller calls set_buffer_layout), the input rows are the arrays'.  host=True hands numpy
    arrays to the host-pointer form of the entry point; guard=True passes out= through guarded_call()."""
    L, nch = rx.frame_len, rx.n_channels
    rows, La = getattr(rx, "audio_rows", nch), getattr(rx, "audio_frame_len", L)
    if layout is None:
        layout = getattr(rx, "layout", "channel")
    nfr = i.shape[1] // L
    tap = None
    if tap_floats:
        import torch
        tap = torch.zeros(nch, nfr * tap_floats, device="cuda")
        rx.set_debug_taps(demod=tap)
    args = pack(i, q, layout, q15_scale, L)
    q15 = args[0].dtype == np.int16
    entry = rx.ProcessIQData_q15 if q15 else rx.ProcessIQData
    shape = (nfr, rows, La) if layout == "time" else (rows, nfr * La)
    if not host:
        import torch
        args = tuple(torch.from_numpy(v).cuda() for v in args)
    if guard:
        out = guarded_call(entry, args, shape, SENT_Q15 if q15 else SENT_F32, host)
    else:
        out = entry(*args)
        if not host:
            out = out.cpu().numpy()
    assert out.shape == shape
    if layout == "time":
        out = from_time_major(out, rows, nfr, La)
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


def bits(x):
    """float32 arrays as their words: a state record holds the oscillator's 64-bit phase, whose halves read as floats may
    be NaNs, and equal NaNs do not compare equal"""
    x = np.ascontiguousarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def first(t, nch, nfr, per):
    """what a call of nfr frames wrote to a side-output tensor sized for more: [nch][nfr * per] from its start"""
    return t.reshape(-1)[:nch * nfr * per].reshape(nch, nfr * per).cpu().numpy()


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
