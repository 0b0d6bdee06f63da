"""Host-side mirror of the reference's transmit exciter interface, over the C ABI (include/t41tx.h).

The reference drives the exciter through globals and one function:
  ExciterIQData()      Exciter.cpp:46-169     -> TxChain.ExciterIQData(Q_in_L_Ex, Q_in_R_Ex)
  CW_ExciterIQData()   CW_Excite.cpp:66-118   -> TxChain.CW_ExciterIQData(n_frames, key)
  sineTone()           Utility.cpp:66-83      -> sine_tone(numCycles), then TxChain.set_cw_tone(cos, sin)
  ProcessIQData2()     Process2.cpp:309-349   -> cal_tone(), TxChain.set_cal_tone(cos, sin, level), TxChain.ProcessIQData2_tx(n_frames)
All arithmetic happens in libt41rx.so (HIP); PyTorch only owns device memory and streams.  No CPU
fallback exists.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


class TxParams(C.Structure):
    """struct t41tx_params (include/t41tx.h)"""
    _fields_ = [("mode", C.c_int32), ("IQXAmpCorrectionFactor", C.c_float), ("IQXPhaseCorrectionFactor", C.c_float)]


_vp = C.c_void_p
TX_SYMBOLS = {
    "t41tx_default_params": (None, [C.POINTER(TxParams)]),
    "t41tx_create": (C.c_int, [C.POINTER(_vp), C.c_int, C.c_int, C.POINTER(TxParams)]),
    "t41tx_destroy": (C.c_int, [_vp]),
    "t41tx_set_params": (C.c_int, [_vp, C.POINTER(TxParams)]),
    "t41tx_reset": (C.c_int, [_vp]),
    "t41tx_n_channels": (C.c_int, [_vp]),
    "t41tx_process_device_q15": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, _vp]),
    "t41tx_process_host_q15": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int]),
    "t41tx_set_transmit_eq_bands": (C.c_int, [_vp, _vp]),
    "t41tx_set_transmit_eq": (C.c_int, [_vp, C.c_int, _vp]),
    "t41tx_get_transmit_eq": (C.c_int, [_vp, _vp]),
    "t41tx_state_bytes": (C.c_size_t, [_vp]),
    "t41tx_get_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41tx_set_state": (C.c_int, [_vp, _vp, C.c_size_t]),
    "t41tx_set_cw_tone": (C.c_int, [_vp, _vp, _vp]),
    "t41tx_process_cw_device_q15": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int, _vp]),
    "t41tx_process_cw_host_q15": (C.c_int, [_vp, _vp, _vp, _vp, C.c_int]),
    "t41tx_set_cal_tone": (C.c_int, [_vp, _vp, _vp, C.c_float]),
    "t41tx_set_cal_corrections": (C.c_int, [_vp, _vp, _vp]),
    "t41tx_process_cal_device_q15": (C.c_int, [_vp, _vp, _vp, C.c_int, _vp]),
    "t41tx_process_cal_host_q15": (C.c_int, [_vp, _vp, _vp, C.c_int]),
}
_bound = False


def _load():
    global _bound
    lib = _lib.load()
    if not _bound:
        for name, (res, args) in TX_SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return lib


def default_tx_params(**overrides):
    p = TxParams()
    _load().t41tx_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise AttributeError("t41tx_params has no field %r" % k)
        setattr(p, k, v)
    return p


def sine_tone(numCycles=8):
    """(cosBuffer2, sinBuffer2) as sineTone(numCycles) fills them (Utility.cpp:66-83), 256 float32 each: the frequency
    numCycles * 24000 / 256 in integer arithmetic (8 -> 750 Hz, 8 whole cycles per table; 5 -> 468 Hz, not 468.75), the
    angle kf * 2 * PI * f / 24000 and its cosine / sine in float64, rounded to float32.  A convenience for callers
    who do not bring the firmware's own table, whose values come from the Teensy's libm."""
    f = float((int(numCycles) * 24000) // 256)
    theta = np.arange(256, dtype=np.float64) * 2.0 * np.pi * f / 24000.0
    return np.cos(theta).astype(np.float32), np.sin(theta).astype(np.float32)


def cal_tone():
    """(cosBuffer3, sinBuffer3) as sineTone() fills them (Utility.cpp:78-80), 256 float32 each, 3000 Hz: the angle
    kf * 2.0 * PI * 3000 / 24000 is computed in float64 and stored in the float ``theta``, whose float64 cosine / sine
    are rounded to float32.  A convenience, like sine_tone()."""
    theta = (np.arange(256, dtype=np.float64) * 2.0 * np.pi * 3000.0 / 24000.0).astype(np.float32)
    return np.cos(theta.astype(np.float64)).astype(np.float32), np.sin(theta.astype(np.float64)).astype(np.float32)


class TxChain:
    """n_channels independent T41 exciters (SSB and CW) resident on one MI355X."""
    FRAME = 2048
    KEY_PER_FRAME = 16  # gate bytes per frame: one per 128-sample audio block

    def __init__(self, n_channels, params=None, device=0):
        self._lib = _load()
        self.params = params if params is not None else default_tx_params()
        self._ctx = C.c_void_p()
        check(self._lib.t41tx_create(C.byref(self._ctx), int(device), int(n_channels), C.byref(self.params)))
        self.n_channels = int(n_channels)
        self.device = int(device)

    def set_params(self, **changes):
        """change fields between two ExciterIQData() calls; states are kept.  A refused change leaves self.params
        as it was (the C side validates before it changes anything)."""
        p = TxParams.from_buffer_copy(self.params)
        for k, v in changes.items():
            if not hasattr(p, k):
                raise AttributeError("t41tx_params has no field %r" % k)
            setattr(p, k, v)
        check(self._lib.t41tx_set_params(self._ctx, C.byref(p)))
        self.params = p

    def reset(self):
        check(self._lib.t41tx_reset(self._ctx))

    def set_transmit_eq_bands(self, coeffs):
        """The transmit equaliser's band table (t41tx_set_transmit_eq_bands): the firmware's EQ_Band1Coeffs ..
        EQ_Band14Coeffs as [14][4][5] or [14][20], {b0, b1, b2, a1, a2} per section with the a's negated.  Kept across
        set_params(); the filter memories are not reset."""
        c = np.ascontiguousarray(np.asarray(coeffs, dtype=np.float32))
        if c.size != 14 * 4 * 5 or c.shape[0] != 14:
            raise ValueError("transmit-EQ band table must be [14][4][5] or [14][20], got %r" % (c.shape,))
        check(self._lib.t41tx_set_transmit_eq_bands(self._ctx, c.ctypes.data_as(C.c_void_p)))

    def set_transmit_eq(self, on, levels=None):
        """xmitEQFlag and EEPROMData.equalizerXmt (Exciter.cpp:94-98, Filter.cpp:176-224): the equaliser between the
        decimators and the Hilbert pair (t41tx_set_transmit_eq; 0 / 1, a band table loaded first).  levels: 14 ints, or
        None to keep the current ones (the firmware's defaults until set); a level counts in whole hundreds, as in the
        reference.  Kept across set_params()."""
        if levels is None:
            check(self._lib.t41tx_set_transmit_eq(self._ctx, int(on), None))
            return
        lv = np.ascontiguousarray(np.asarray(levels, dtype=np.int32))
        if lv.shape != (14,):
            raise ValueError("transmit-EQ levels must be 14 ints, got %r" % (lv.shape,))
        check(self._lib.t41tx_set_transmit_eq(self._ctx, int(on), lv.ctypes.data_as(C.c_void_p)))

    def get_transmit_eq(self):
        """(on, levels): the transmit equaliser's switch and its 14 levels"""
        lv = np.zeros(14, np.int32)
        v = self._lib.t41tx_get_transmit_eq(self._ctx, lv.ctypes.data_as(C.c_void_p))
        if v < 0:
            check(v)
        return v, lv

    def get_state(self):
        """checkpoint of every channel's memories (t41tx_get_state) as a numpy uint8 array; synchronises"""
        n = self._lib.t41tx_state_bytes(self._ctx)
        buf = np.zeros(n, dtype=np.uint8)
        check(self._lib.t41tx_get_state(self._ctx, buf.ctypes.data_as(C.c_void_p), n))
        return buf

    def set_state(self, buf):
        buf = np.ascontiguousarray(buf, dtype=np.uint8)
        check(self._lib.t41tx_set_state(self._ctx, buf.ctypes.data_as(C.c_void_p), buf.size))

    def ExciterIQData(self, Q_in_L_Ex, Q_in_R_Ex=None):
        """int16 (q15) microphone samples [n_channels, k * 2048] -> (Q_out_L_Ex, Q_out_R_Ex), the I and Q
        drive.  torch CUDA int16 tensors run on the current stream; numpy arrays use the host entry."""
        if isinstance(Q_in_L_Ex, np.ndarray):
            a = np.ascontiguousarray(Q_in_L_Ex, dtype=np.int16)
            nfr = self._frames(a.shape)
            oL, oR = np.empty_like(a), np.empty_like(a)
            p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731
            check(self._lib.t41tx_process_host_q15(self._ctx, p(a), None, p(oL), p(oR), nfr))
            return oL, oR
        import torch
        a = Q_in_L_Ex
        if not (a.is_cuda and a.dtype == torch.int16 and a.is_contiguous() and a.device.index == self.device):
            raise ValueError("Q_in_L_Ex must be a contiguous int16 CUDA tensor on device %d" % self.device)
        nfr = self._frames(tuple(a.shape))
        oL, oR = torch.empty_like(a), torch.empty_like(a)
        stream = torch.cuda.current_stream(a.device).cuda_stream
        check(self._lib.t41tx_process_device_q15(self._ctx, a.data_ptr(), None, oL.data_ptr(), oR.data_ptr(), nfr, C.c_void_p(stream)))
        return oL, oR

    def set_cw_tone(self, cos, sin):
        """cosBuffer2 and sinBuffer2 (t41tx_set_cw_tone), 256 floats each, e.g. sine_tone(8).  Kept across set_params()
        and reset(); takes effect from the next CW_ExciterIQData()."""
        c = np.ascontiguousarray(np.asarray(cos, dtype=np.float32))
        s = np.ascontiguousarray(np.asarray(sin, dtype=np.float32))
        if c.shape != (256,) or s.shape != (256,):
            raise ValueError("CW tone tables must be 256 floats each, got %r and %r" % (c.shape, s.shape))
        check(self._lib.t41tx_set_cw_tone(self._ctx, c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p)))

    def CW_ExciterIQData(self, n_frames, key=None, device=False):
        """n_frames frames of the CW exciter on every channel -> (Q_out_L_Ex, Q_out_R_Ex), [n_channels, n_frames * 2048]
        int16.  key: uint8 [n_channels, n_frames * 16], one byte per 128-sample block (nonzero passes it, zero writes
        zeros), or None for key down throughout.  A numpy key, or None with device=False, uses the host entry and
        returns numpy arrays; a torch uint8 CUDA key, or device=True, runs on the current stream and returns torch
        tensors.  The interpolator memories are the ones ExciterIQData() uses."""
        nfr = int(n_frames)
        kshape = (self.n_channels, nfr * self.KEY_PER_FRAME)
        if key is None and not device or isinstance(key, np.ndarray):
            k = None
            if key is not None:
                k = np.ascontiguousarray(key, dtype=np.uint8)
                if k.shape != kshape:
                    raise ValueError("key must be [n_channels=%d, n_frames*16=%d], got %r" % (kshape + (k.shape,)))
            oL = np.empty((self.n_channels, max(nfr, 0) * self.FRAME), np.int16)
            oR = np.empty_like(oL)
            p = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
            check(self._lib.t41tx_process_cw_host_q15(self._ctx, p(k), p(oL), p(oR), nfr))
            return oL, oR
        import torch
        dev = torch.device("cuda", self.device)
        if key is not None:
            if not (isinstance(key, torch.Tensor) and key.is_cuda and key.dtype == torch.uint8 and key.is_contiguous()
                    and key.device.index == self.device):
                raise ValueError("key must be a numpy array or a contiguous uint8 CUDA tensor on device %d" % self.device)
            if tuple(key.shape) != kshape:
                raise ValueError("key must be [n_channels=%d, n_frames*16=%d], got %r" % (kshape + (tuple(key.shape),)))
        oL = torch.empty((self.n_channels, max(nfr, 0) * self.FRAME), dtype=torch.int16, device=dev)
        oR = torch.empty_like(oL)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(self._lib.t41tx_process_cw_device_q15(self._ctx, None if key is None else key.data_ptr(), oL.data_ptr(), oR.data_ptr(),
                                                    nfr, C.c_void_p(stream)))
        return oL, oR

    def set_cal_tone(self, cos, sin, level):
        """cosBuffer3, sinBuffer3 (256 floats each, e.g. cal_tone()) and the firmware's bandOutputFactor
        (t41tx_set_cal_tone).  Kept across set_params() and reset(); takes effect from the next ProcessIQData2_tx()."""
        c = np.ascontiguousarray(np.asarray(cos, dtype=np.float32))
        s = np.ascontiguousarray(np.asarray(sin, dtype=np.float32))
        if c.shape != (256,) or s.shape != (256,):
            raise ValueError("calibration tone tables must be 256 floats each, got %r and %r" % (c.shape, s.shape))
        check(self._lib.t41tx_set_cal_tone(self._ctx, c.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), float(level)))

    def set_cal_corrections(self, amp=None, phase=None):
        """one (IQXAmpCorrectionFactor, IQXPhaseCorrectionFactor) candidate per channel for the calibration exciter
        (t41tx_set_cal_corrections): two arrays of n_channels floats, or None, None for the params' factors"""
        if amp is None and phase is None:
            check(self._lib.t41tx_set_cal_corrections(self._ctx, None, None))
            return
        if amp is None or phase is None:
            raise ValueError("amp and phase must both be given or both be None")
        a = np.ascontiguousarray(np.asarray(amp, dtype=np.float32))
        p = np.ascontiguousarray(np.asarray(phase, dtype=np.float32))
        if a.shape != (self.n_channels,) or p.shape != (self.n_channels,):
            raise ValueError("corrections must be %d floats each, got %r and %r" % (self.n_channels, a.shape, p.shape))
        check(self._lib.t41tx_set_cal_corrections(self._ctx, a.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p)))

    def ProcessIQData2_tx(self, n_frames, device=False):
        """n_frames frames of the calibration exciter (the transmit half of ProcessIQData2()) on every channel ->
        (Q_out_L_Ex, Q_out_R_Ex), [n_channels, n_frames * 2048] int16: numpy arrays through the host entry, or with
        device=True torch tensors on the current stream.  The interpolator memories are ExciterIQData()'s."""
        nfr = int(n_frames)
        if not device:
            oL = np.empty((self.n_channels, max(nfr, 0) * self.FRAME), np.int16)
            oR = np.empty_like(oL)
            check(self._lib.t41tx_process_cal_host_q15(self._ctx, oL.ctypes.data_as(C.c_void_p), oR.ctypes.data_as(C.c_void_p), nfr))
            return oL, oR
        import torch
        dev = torch.device("cuda", self.device)
        oL = torch.empty((self.n_channels, max(nfr, 0) * self.FRAME), dtype=torch.int16, device=dev)
        oR = torch.empty_like(oL)
        stream = torch.cuda.current_stream(dev).cuda_stream
        check(self._lib.t41tx_process_cal_device_q15(self._ctx, oL.data_ptr(), oR.data_ptr(), nfr, C.c_void_p(stream)))
        return oL, oR

    def _frames(self, shape):
        if len(shape) != 2 or shape[0] != self.n_channels or shape[1] == 0 or shape[1] % self.FRAME:
            raise ValueError("samples must be [n_channels=%d, k*2048], got %r" % (self.n_channels, shape))
        return shape[1] // self.FRAME

    def close(self):
        if getattr(self, "_ctx", None) is not None and self._ctx:
            self._lib.t41tx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
