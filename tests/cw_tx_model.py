"""CPU models of the CW exciter, CW_ExciterIQData() (CW_Excite.cpp:66-118), which the frozen oracle does not hold.

* ``CwTxModel`` -- the f32 restatement of one channel.  It extends ``tx_model.TxModel``, so SSB frames (``frame``) and CW
  frames (``cw_frame``) drive the same ``int1`` / ``int2`` memories, as the firmware's two exciters drive the same
  FIR_int1_EX_I/Q and FIR_int2_EX_I/Q instances.  The scalings are numpy float32 products (one rounding each, no
  contraction); the interpolators and the conversion are the oracle's exported primitives ``t41o_fir_interpolate_f32``
  and ``t41o_float_to_q15`` on the oracle's tables.
* ``CwTxModelBatch`` -- n channels that share the tone table and differ by their key, the interface of ``TxModelBatch``
  plus ``process_cw``.
* ``gate`` -- the key: modeSelectOutExL/R at gain 0 or on (T41_SDR.ino:1193-1289), one byte per 128-sample audio block.
* ``cw_stream_model_f64`` -- an independent float64 model of a whole ungated stream from power-on: the table tiled,
  zero stuffing and scipy's lfilter, no frames and no CMSIS state.
"""
import ctypes as C

import numpy as np

import oracle_lib as O
from tx_model import F32, TxModel, TxModelBatch

FRAME, TONE, BLOCK, KEYS = 2048, 256, 128, 16
CW_SCALE = F32(0.127)  # arm_scale_f32(cosBuffer2, 0.127, ...): the double constant becomes a float32_t argument


def gate(q, key):
    """q15 samples [..., k * 2048] through the key [..., k * 16]: nonzero passes a 128-sample block, zero writes zeros"""
    if key is None:
        return q
    on = np.repeat(np.asarray(key) != 0, BLOCK, axis=-1)
    assert on.shape == q.shape, (on.shape, q.shape)
    return np.where(on, q, np.int16(0)).astype(np.int16)


class CwTxModel(TxModel):
    """one exciter channel with both entries; cw_frame() touches int1 / int2 and nothing else"""

    def cw_frame(self, cos, sin, mode=O.DEMOD_USB, amp=1.0, phase=0.0, key=None):
        """one frame -> (Q_out_L_Ex, Q_out_R_Ex), 2048 q15 each; key: 16 bytes or None"""
        sp = C.POINTER(C.c_int16)
        I = np.asarray(cos, F32) * CW_SCALE                                                         # CW_Excite.cpp:69
        Q = np.asarray(sin, F32) * CW_SCALE                                                         # :70
        assert I.shape == (TONE,) and Q.shape == (TONE,)
        amp, phase = F32(amp), F32(phase)
        if mode in (O.DEMOD_LSB, O.DEMOD_USB):                                                      # :77-87
            I = I * (-amp if mode == O.DEMOD_LSB else amp)
            if phase < 0.0:                                                                         # Utility.cpp:178-187
                Q = Q + I * phase
            else:
                I = I + Q * phase
        L, T = np.empty(FRAME, F32), np.empty(FRAME, F32)
        lib = self.lib
        outs = []
        for k, v in enumerate((I, Q)):
            L[:TONE] = v
            lib.t41o_fir_interpolate_f32(O.fptr(self.c48), 48, 2, O.fptr(self.int1[k]), O.fptr(L), O.fptr(T), 256)   # :93, 99
            lib.t41o_fir_interpolate_f32(O.fptr(self.c192), 32, 4, O.fptr(self.int2[k]), O.fptr(T), O.fptr(L), 512)  # :96, 100
            y = np.ascontiguousarray(L * F32(20.0))                                                 # :103-104
            o = np.empty(FRAME, np.int16)
            lib.t41o_float_to_q15(O.fptr(y), o.ctypes.data_as(sp), FRAME)                           # :113-114
            outs.append(gate(o, key))
        return outs[0], outs[1]


class CwTxModelBatch(TxModelBatch):
    """nchan CwTxModel channels; process() runs SSB frames and process_cw() CW frames on the same memories"""

    def __init__(self, nchan, mode=O.DEMOD_USB, amp=1.0, phase=0.0, tone=None, **kw):
        super().__init__(nchan, mode, amp, phase, **kw)
        coeffs = kw.get("coeffs")
        self.chs = [CwTxModel(coeffs) for _ in range(nchan)]
        self.tone = tone

    def process_cw(self, n_frames, key=None):
        cos, sin = self.tone
        oL, oR = np.empty((self.nchan, n_frames * FRAME), np.int16), np.empty((self.nchan, n_frames * FRAME), np.int16)
        for c, ch in enumerate(self.chs):
            for f in range(n_frames):
                k = None if key is None else np.asarray(key)[c, f * KEYS:(f + 1) * KEYS]
                sl = slice(f * FRAME, (f + 1) * FRAME)
                oL[c, sl], oR[c, sl] = ch.cw_frame(cos, sin, self.mode, self.amp, self.phase, k)
        return oL, oR


def cw_stream_model_f64(cos, sin, n_frames, mode, amp, phase, tabs):
    """whole-stream float64 model of one ungated channel from power-on; tabs: the oracle's four TX tables.  Returns
    the I and Q drive as float64 in units of full scale."""
    from scipy.signal import lfilter
    c192, c48 = np.asarray(tabs[0], np.float64), np.asarray(tabs[1], np.float64)
    I = np.tile(np.asarray(cos, np.float64), n_frames) * np.float64(CW_SCALE)
    Q = np.tile(np.asarray(sin, np.float64), n_frames) * np.float64(CW_SCALE)
    amp, phase = np.float64(F32(amp)), np.float64(F32(phase))
    if mode in (O.DEMOD_LSB, O.DEMOD_USB):
        I = I * (-amp if mode == O.DEMOD_LSB else amp)
        if phase < 0:
            Q = Q + I * phase
        else:
            I = I + Q * phase

    def interp(v, L, c):  # arm_fir_interpolate_f32: zero stuffing + the time-reversed taps, no make-up gain
        up = np.zeros(v.size * L)
        up[::L] = v
        return lfilter(c[::-1], 1.0, up)

    return [interp(interp(v, 2, c48), 4, c192[:32]) * 20.0 for v in (I, Q)]
