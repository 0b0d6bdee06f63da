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

from . import _args, _lib
from ._args import cuda, cuda_tensor, ptr, run, table, table_pair, value, with_fields
from ._lib import TX_SYMBOLS, TxParams, check  # noqa: F401

_load = _lib.load  # one table loop binds both headers' symbols


def default_tx_params(**overrides):
    p = TxParams()
    _load().t41tx_default_params(C.byref(p))
    return with_fields(p, "t41tx_params", overrides)


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
        p = with_fields(TxParams.from_buffer_copy(self.params), "t41tx_params", changes)
        check(self._lib.t41tx_set_params(self._ctx, C.byref(p)))
        self.params = p

    def reset(self):
        check(self._lib.t41tx_reset(self._ctx))

    def set_transmit_eq_bands(self, coeffs):
        """The transmit equaliser's band table (t41tx_set_transmit_eq_bands): the firmware's EQ_Band1Coeffs ..
        EQ_Band14Coeffs as [14][4][5] or [14][20], {b0, b1, b2, a1, a2} per section with the a's negated.  Kept across
        set_params(); the filter memories are not reset."""
        c = table(coeffs, np.float32, (14, 20), "transmit-EQ band table must be [14][4][5] or [14][20], got %r", rows=True)
        check(self._lib.t41tx_set_transmit_eq_bands(self._ctx, ptr(c)))

    def set_transmit_eq(self, on, levels=None):
        """xmitEQFlag and EEPROMData.equalizerXmt (Exciter.cpp:94-98, Filter.cpp:176-224): the equaliser between the
        decimators and the Hilbert pair (t41tx_set_transmit_eq; 0 / 1, a band table loaded first).  levels: 14 ints, or
        None to keep the current ones (the firmware's defaults until set); a level counts in whole hundreds, as in the
        reference.  Kept across set_params()."""
        lv = None if levels is None else table(levels, np.int32, (14,), "transmit-EQ levels must be 14 ints, got %r")
        check(self._lib.t41tx_set_transmit_eq(self._ctx, int(on), ptr(lv)))

    def get_transmit_eq(self):
        """(on, levels): the transmit equaliser's switch and its 14 levels"""
        lv = np.zeros(14, np.int32)
        return value(self._lib.t41tx_get_transmit_eq(self._ctx, ptr(lv))), lv

    def get_state(self):
        """checkpoint of every channel's memories (t41tx_get_state) as a numpy uint8 array; synchronises"""
        return _args.get_blob(self._lib.t41tx_get_state, self._ctx, self._lib.t41tx_state_bytes(self._ctx))

    def set_state(self, buf):
        _args.set_blob(self._lib.t41tx_set_state, self._ctx, buf)

    def ExciterIQData(self, Q_in_L_Ex, Q_in_R_Ex=None):
        """int16 (q15) microphone samples [n_channels, k * 2048] -> (Q_out_L_Ex, Q_out_R_Ex), the I and Q
        drive.  torch CUDA int16 tensors run on the current stream; numpy arrays use the host entry."""
        a, host = Q_in_L_Ex, isinstance(Q_in_L_Ex, np.ndarray)
        if host:
            a = np.ascontiguousarray(a, dtype=np.int16)
        else:
            import torch
            if not cuda_tensor(a, torch.int16, self.device):
                raise ValueError("Q_in_L_Ex must be a contiguous int16 CUDA tensor on device %d" % self.device)
        nfr = self._frames(tuple(a.shape))
        empty = np.empty_like if host else torch.empty_like
        oL, oR = empty(a), empty(a)
        run(host, self._lib.t41tx_process_host_q15, self._lib.t41tx_process_device_q15, self.device,
            self._ctx, ptr(a), None, ptr(oL), ptr(oR), nfr)
        return oL, oR

    def set_cw_tone(self, cos, sin):
        """cosBuffer2 and sinBuffer2 (t41tx_set_cw_tone), 256 floats each, e.g. sine_tone(8).  Kept across set_params()
        and reset(); takes effect from the next CW_ExciterIQData()."""
        c, s = table_pair(cos, sin, (256,), (256,), "CW tone tables must be 256 floats each, got %r and %r")
        check(self._lib.t41tx_set_cw_tone(self._ctx, ptr(c), ptr(s)))

    def CW_ExciterIQData(self, n_frames, key=None, device=False):
        """n_frames frames of the CW exciter on every channel -> (Q_out_L_Ex, Q_out_R_Ex), [n_channels, n_frames * 2048]
        int16.  key: uint8 [n_channels, n_frames * 16], one byte per 128-sample block (nonzero passes it, zero writes
        zeros), or None for key down throughout.  A numpy key, or None with device=False, uses the host entry and
        returns numpy arrays; a torch uint8 CUDA key, or device=True, runs on the current stream and returns torch
        tensors.  The interpolator memories are the ones ExciterIQData() uses."""
        nfr = int(n_frames)
        kshape = (self.n_channels, nfr * self.KEY_PER_FRAME)
        host = key is None and not device or isinstance(key, np.ndarray)
        if host and key is not None:
            key = np.ascontiguousarray(key, dtype=np.uint8)
        elif key is not None:
            import torch
            if not (isinstance(key, torch.Tensor) and cuda_tensor(key, torch.uint8, self.device)):
                raise ValueError("key must be a numpy array or a contiguous uint8 CUDA tensor on device %d" % self.device)
        if key is not None and tuple(key.shape) != kshape:
            raise ValueError("key must be [n_channels=%d, n_frames*16=%d], got %r" % (kshape + (tuple(key.shape),)))
        oL, oR = self._outputs(nfr, host)
        run(host, self._lib.t41tx_process_cw_host_q15, self._lib.t41tx_process_cw_device_q15, self.device,
            self._ctx, ptr(key), ptr(oL), ptr(oR), nfr)
        return oL, oR

    def set_cal_tone(self, cos, sin, level):
        """cosBuffer3, sinBuffer3 (256 floats each, e.g. cal_tone()) and the firmware's bandOutputFactor
        (t41tx_set_cal_tone).  Kept across set_params() and reset(); takes effect from the next ProcessIQData2_tx()."""
        c, s = table_pair(cos, sin, (256,), (256,), "calibration tone tables must be 256 floats each, got %r and %r")
        check(self._lib.t41tx_set_cal_tone(self._ctx, ptr(c), ptr(s), float(level)))

    def set_cal_corrections(self, amp=None, phase=None):
        """one (IQXAmpCorrectionFactor, IQXPhaseCorrectionFactor) candidate per channel for the calibration exciter
        (t41tx_set_cal_corrections): two arrays of n_channels floats, or None, None for the params' factors"""
        _args.set_cal_corrections(self, self._lib.t41tx_set_cal_corrections, amp, phase)

    def ProcessIQData2_tx(self, n_frames, device=False):
        """n_frames frames of the calibration exciter (the transmit half of ProcessIQData2()) on every channel ->
        (Q_out_L_Ex, Q_out_R_Ex), [n_channels, n_frames * 2048] int16: numpy arrays through the host entry, or with
        device=True torch tensors on the current stream.  The interpolator memories are ExciterIQData()'s."""
        oL, oR = self._outputs(int(n_frames), not device)
        run(not device, self._lib.t41tx_process_cal_host_q15, self._lib.t41tx_process_cal_device_q15, self.device,
            self._ctx, ptr(oL), ptr(oR), int(n_frames))
        return oL, oR

    def _outputs(self, nfr, host):
        """empty (Q_out_L_Ex, Q_out_R_Ex) for nfr frames: numpy arrays for a host entry, torch tensors for a device entry"""
        shape = (self.n_channels, max(nfr, 0) * self.FRAME)
        if host:
            return np.empty(shape, np.int16), np.empty(shape, np.int16)
        import torch
        oL = torch.empty(shape, dtype=torch.int16, device=cuda(self.device))
        return oL, torch.empty_like(oL)

    def _frames(self, shape):
        if len(shape) != 2 or shape[0] != self.n_channels or shape[1] == 0 or shape[1] % self.FRAME:
            raise ValueError("samples must be [n_channels=%d, k*2048], got %r" % (self.n_channels, shape))
        return shape[1] // self.FRAME

    def close(self):
        _args.close(self, "t41tx_destroy")

    __del__ = _args.finalize
