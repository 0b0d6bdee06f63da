"""What rx.py and tx.py do to an argument on its way to the C ABI, once each: conversions, shape checks, pointers.
Plain functions; every message is the caller's, so a refusal reads as it did when each method carried its own copy."""
import ctypes as C

import numpy as np

from ._lib import check

F32P, I32P, U16P, U32P = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32)


def value(v):
    """a getter's return: the value, or a negative status raised as T41RxError"""
    if v < 0:
        check(v)
    return v


def ptr(a, ctype=C.c_void_p):
    """the address of a numpy array or a torch tensor as the table's pointer type, NULL for None"""
    if a is None:
        return None
    return a.ctypes.data_as(ctype) if isinstance(a, np.ndarray) else ctype(a.data_ptr())


def table(x, dtype, shape, message, rows=False):
    """x as a contiguous array of dtype and of this shape -- with rows, of any shape that holds shape[0] rows of
    shape[1] values in all ([14][4][5] for (14, 20)) -- or ValueError(message % its shape)"""
    a = np.ascontiguousarray(np.asarray(x, dtype=dtype))
    if (a.size != shape[0] * shape[1] or a.shape[0] != shape[0]) if rows else a.shape != shape:
        raise ValueError(message % (a.shape,))
    return a


def table_pair(x, y, shape_x, shape_y, message):
    """two float32 tables that are checked together: ValueError(message % both shapes) if either is wrong"""
    a, b = np.ascontiguousarray(np.asarray(x, dtype=np.float32)), np.ascontiguousarray(np.asarray(y, dtype=np.float32))
    if a.shape != shape_x or b.shape != shape_y:
        raise ValueError(message % (a.shape, b.shape))
    return a, b


def int_table(x, dtype, shape, message):
    """x, which must hold integers already and fit dtype (no float is truncated, no value wraps), as a contiguous array of
    dtype; shape None is any 1-d array.  ValueError(message % (shape, dtype)) otherwise"""
    a, lim = np.asarray(x), np.iinfo(dtype)
    if (a.ndim != 1 if shape is None else a.shape != shape) or not np.issubdtype(a.dtype, np.integer) or (
            a.size and (a.min() < lim.min or a.max() > lim.max)):
        raise ValueError(message % (a.shape, a.dtype))
    return np.ascontiguousarray(a, dtype=dtype)


def channel_mask(channels, n_channels):
    """(mask, n) of the calls that act on some channels: (NULL, 0) for None = all, else one byte per channel, non-zero = act"""
    if channels is None:
        return None, 0
    m = np.ascontiguousarray(np.asarray(channels).astype(bool).astype(np.uint8))
    if m.shape != (n_channels,):
        raise ValueError("channels must have n_channels = %d entries, got %r" % (n_channels, m.shape))
    return ptr(m), n_channels


def get_blob(get, first, n):
    """n bytes from a get(first, buffer, n) entry as a numpy uint8 array"""
    buf = np.zeros(n, dtype=np.uint8)
    check(get(first, ptr(buf), n))
    return buf


def set_blob(put, ctx, buf):
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    check(put(ctx, ptr(buf), buf.size))


def with_fields(struct, what, changes):
    """struct with these fields set; a name the C struct `what` does not have is an AttributeError"""
    for k, v in changes.items():
        if not hasattr(struct, k):
            raise AttributeError("%s has no field %r" % (what, k))
        setattr(struct, k, v)
    return struct


def cuda_tensor(t, dtype, device=None):
    """a contiguous CUDA tensor of this dtype (or one of these), and with `device` on that device"""
    return (t.is_cuda and (t.dtype in dtype if isinstance(dtype, tuple) else t.dtype == dtype) and t.is_contiguous()
            and (device is None or t.device.index == device))


def cuda(device):
    return "cuda:%d" % device


def stream_of(device):
    """the current torch stream of the device, as the device entries take it"""
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def run(host, host_entry, device_entry, device, ctx, *args):
    """a call of the host entry, or of its device twin: the same arguments and the current stream behind them"""
    if host:
        check(host_entry(ctx, *args))
    else:
        check(device_entry(ctx, *args, stream_of(device)))


def kept(chain, attr, off):
    """what a stage switch keeps alive in chain.<attr>, or ValueError(off) if it is off or was never on"""
    t = getattr(chain, attr, None)
    if t is None:
        raise ValueError(off)
    return t


def set_cal_corrections(chain, entry, amp, phase):
    """set_cal_corrections() of both chains: two arrays of n_channels floats, or None, None"""
    if amp is None and phase is None:
        check(entry(chain._ctx, None, None))
        return
    if amp is None or phase is None:
        raise ValueError("amp and phase must both be given or both be None")
    n = (chain.n_channels,)
    a, p = table_pair(amp, phase, n, n, "corrections must be %d floats each, got %%r and %%r" % n)
    check(entry(chain._ctx, ptr(a), ptr(p)))


def close(chain, destroy):
    if getattr(chain, "_ctx", None) is not None and chain._ctx:
        getattr(chain._lib, destroy)(chain._ctx)
        chain._ctx = C.c_void_p()


def finalize(chain):
    """__del__ of both chains"""
    try:
        chain.close()
    except Exception:
        pass
