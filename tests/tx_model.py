"""CPU models of the transmit exciter with its equaliser in place: ExciterIQData() (Exciter.cpp:46-169) with DoExciterEQ()
(Filter.cpp:176-224) between the /2 decimator and the copy L -> R, where the frozen oracle (oracle/t41_tx_oracle.c) has
xmitEQFlag = OFF.

* ``TxModel`` -- the f32 restatement of one channel, frame by frame, with persistent state.  Every stage is one of the
  oracle's exported primitives (``t41o_q15_to_float``, ``t41o_fir_decimate_f32``, ``t41o_fir_interpolate_f32``,
  ``t41o_biquad_df2T_f32``, ``t41o_float_to_q15``) on the oracle's tables (``TxOracleBatch.table()``); arm_fir_f32, static
  in the oracle, is restated in numpy float32 (taps in order, separate multiply and add).  With the equaliser off it
  is the oracle bit for bit (tests/test_tx_equalizer.py pins that), so the equaliser is the only new arithmetic.
* ``TxModelBatch`` -- n independent channels, the interface of ``TxOracleBatch`` plus the equaliser's switches.
* ``stream_model_f64`` -- an independent float64 model of a whole stream (scipy lfilter / sosfilt, no frames, no CMSIS
  state), with the same level rule.
"""
import ctypes as C
import os

import numpy as np

import oracle_lib as O
from df2t_model import cascade_oracle, sos_of

BANDS, STAGES = 14, 4
F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LEVELS = (0, 0, 100, 100, 100, 100, 100, 100, 100, 100, 100, 0, 0, 0)  # equalizerXmt, gwv.cpp:50


def bands():
    """EQ_Band1Coeffs .. EQ_Band14Coeffs as the firmware compiles them, [14][4][5]: S1_Xmt .. S14_Xmt point at the
    receive equaliser's tables (Filter.cpp:89-102)"""
    return np.load(os.path.join(HERE, "golden", "eq", "rx_eq_bands.npz"))["coeffs_f32"].astype(F32).reshape(BANDS, STAGES, 5)


def whole_levels(levels):
    """``equalizerXmt[i] = (float)EEPROMData.equalizerXmt[i] / 100.0`` into an int array (Filter.cpp:178, gwv.h:44): int
    to float, divided in double, truncated toward zero"""
    return [int(np.float64(F32(int(v))) / 100.0) for v in levels]


def signed_scales(levels):
    """arm_scale_f32's factor per band: -equalizerXmt[k] (an int negation) for bands 1, 3, .., 13, +equalizerXmt[k] for
    2, 4, .., 14 (Filter.cpp:195-208), converted to float at the call"""
    return np.array([F32(-w if b % 2 == 0 else w) for b, w in enumerate(whole_levels(levels))], F32)


def fir_f32(coeffs, state, src):
    """arm_fir_f32 as oracle/t41_tx_oracle.c restates it: state = [numTaps - 1 history | blockSize new];
    y[n] = sum_i coeffs[i] * state[n + i], one float32 accumulator in tap order; the history rolls"""
    nt, n = coeffs.size, src.size
    state[nt - 1:nt - 1 + n] = src
    acc = np.zeros(n, F32)
    for i in range(nt):
        acc = acc + state[i:i + n] * coeffs[i]
    state[:nt - 1] = state[n:n + nt - 1].copy()
    return acc


class TxModel:
    """one exciter channel; the CMSIS instance states of T41_SDR.ino:278-299 and Filter.cpp:74-87, zero at power-on"""

    def __init__(self, coeffs=None):
        self.lib = O.lib()
        ob = O.TxOracleBatch(0)
        self.c192, self.c48, self.h45, self.hn45 = [np.ascontiguousarray(ob.table(i), F32) for i in range(4)]
        self.c = np.ascontiguousarray(bands() if coeffs is None else coeffs, F32).reshape(BANDS, STAGES, 5)
        self.reset()

    def reset(self):
        z = lambda n: np.zeros(n, F32)  # noqa: E731
        self.dec1, self.dec2 = z(47 + 2048), z(23 + 512)
        self.hil_l, self.hil_r = z(99 + 256), z(99 + 256)
        self.int1 = [z(23 + 256), z(23 + 256)]
        self.int2 = [z(7 + 512), z(7 + 512)]
        self.eq = np.zeros((BANDS, STAGES, 2), F32)  # xmt_EQ_Band1_state .. xmt_EQ_Band14_state

    def exciter_eq(self, x, levels):
        """DoExciterEQ() on one 256-sample block; every cascade advances, whatever its level"""
        eq = np.stack([cascade_oracle(self.c[b], self.eq[b], x) for b in range(BANDS)])
        eq *= signed_scales(levels)[:, None]       # arm_scale_f32
        out = eq[0] + eq[1]                        # arm_add_f32: EQ1 + EQ2, then + EQ3, .., + EQ14
        for k in range(2, BANDS):
            out = out + eq[k]
        return out

    def frame(self, q, mode=O.DEMOD_USB, amp=1.0, phase=0.0, eq_on=False, levels=DEFAULT_LEVELS):
        """one frame of 2048 q15 microphone samples -> (Q_out_L_Ex, Q_out_R_Ex), 2048 q15 each"""
        sp = C.POINTER(C.c_int16)
        q = np.ascontiguousarray(q, np.int16)
        L, R, T = np.empty(2048, F32), np.empty(2048, F32), np.empty(2048, F32)
        lib = self.lib
        lib.t41o_q15_to_float(q.ctypes.data_as(sp), O.fptr(L), 2048)                                # Exciter.cpp:63-64
        lib.t41o_fir_decimate_f32(O.fptr(self.c192), 48, 4, O.fptr(self.dec1), O.fptr(L), O.fptr(L), 2048)  # :84
        lib.t41o_fir_decimate_f32(O.fptr(self.c48), 24, 2, O.fptr(self.dec2), O.fptr(L), O.fptr(L), 512)    # :88
        if eq_on:
            L[:256] = self.exciter_eq(L[:256].copy(), levels)                                       # :94-97
        R[:256] = L[:256]                                                                           # :98
        I = fir_f32(self.h45, self.hil_l, L[:256])                                                  # :110
        Q = fir_f32(self.hn45, self.hil_r, R[:256])                                                 # :111
        amp, phase = F32(amp), F32(phase)
        if mode in (O.DEMOD_LSB, O.DEMOD_USB):                                                      # :117-126
            I = I * (amp if mode == O.DEMOD_LSB else -amp)
            if phase < 0.0:
                Q = Q + I * phase
            else:
                I = I + Q * phase
        Q = Q * F32(1.0)                                                                            # :127
        outs = []
        for k, v in enumerate((I, Q)):
            L[:256] = v
            lib.t41o_fir_interpolate_f32(O.fptr(self.c48), 48, 2, O.fptr(self.int1[k]), O.fptr(L), O.fptr(T), 256)   # :141, 147
            lib.t41o_fir_interpolate_f32(O.fptr(self.c192), 32, 4, O.fptr(self.int2[k]), O.fptr(T), O.fptr(L), 512)  # :144, 148
            y = np.ascontiguousarray(L * F32(20.0))                                                 # :151-152
            o = np.empty(2048, np.int16)
            lib.t41o_float_to_q15(O.fptr(y), o.ctypes.data_as(sp), 2048)                            # :161-162
            outs.append(o)
        return outs[0], outs[1]


class TxModelBatch:
    """nchan independent TxModel channels run through consecutive frames; mode / amp / phase / eq_on / levels / coeffs
    may change between calls, the states are kept (stale equaliser memories across off / on included)"""

    def __init__(self, nchan, mode=O.DEMOD_USB, amp=1.0, phase=0.0, eq_on=False, levels=DEFAULT_LEVELS, coeffs=None):
        self.nchan, self.mode, self.amp, self.phase = nchan, mode, amp, phase
        self.eq_on, self.levels = eq_on, tuple(levels)
        self.chs = [TxModel(coeffs) for _ in range(nchan)]

    def set_bands(self, coeffs):
        for ch in self.chs:
            ch.c = np.ascontiguousarray(coeffs, F32).reshape(BANDS, STAGES, 5)

    def reset(self):
        for ch in self.chs:
            ch.reset()

    def process(self, Q_in_L_Ex):
        a = np.ascontiguousarray(Q_in_L_Ex, np.int16)
        assert a.shape[0] == self.nchan and a.shape[1] % 2048 == 0
        oL, oR = np.empty_like(a), np.empty_like(a)
        for c, ch in enumerate(self.chs):
            for f in range(a.shape[1] // 2048):
                sl = slice(f * 2048, (f + 1) * 2048)
                oL[c, sl], oR[c, sl] = ch.frame(a[c, sl], self.mode, self.amp, self.phase, self.eq_on, self.levels)
        return oL, oR


def stream_model_f64(q, mode, amp, phase, tabs, eq_on=False, levels=DEFAULT_LEVELS, coeffs=None):
    """whole-stream float64 model of one channel: lfilter / slicing / zero stuffing, and scipy's second-order sections
    for the equaliser's banks (the float32-rounded coefficients, whole-number levels, a float64 sum); returns the I and
    Q drive as float64 in units of full scale"""
    from scipy.signal import lfilter, sosfilt
    c192, c48, h45, hn45 = [np.asarray(t, np.float64) for t in tabs]
    x = np.asarray(q, np.float64) / 32768.0
    # CMSIS holds the taps time-reversed: y[n] = sum_i c[i] x[n - (T - 1) + i]
    d1 = lfilter(c192[::-1], 1.0, x)[0::4]
    d2 = lfilter(c48[:24][::-1], 1.0, d1)[0::2]
    if eq_on:
        c = np.asarray(bands() if coeffs is None else coeffs, np.float64).reshape(BANDS, STAGES, 5)
        out = np.zeros(d2.size)
        for b, w in enumerate(whole_levels(levels)):
            out += (-w if b % 2 == 0 else w) * sosfilt(sos_of(c[b]), d2)
        d2 = out
    I = lfilter(h45[::-1], 1.0, d2)
    Q = lfilter(hn45[::-1], 1.0, d2)
    if mode in (O.DEMOD_LSB, O.DEMOD_USB):
        I = I * (amp if mode == O.DEMOD_LSB else -amp)
        if phase < 0:
            Q = Q + I * phase
        else:
            I = I + Q * phase

    def interp(v, L, c):  # arm_fir_interpolate_f32: zero stuffing + the same time-reversed taps, no make-up gain
        up = np.zeros(v.size * L)
        up[::L] = v
        return lfilter(c[::-1], 1.0, up)

    return [interp(interp(v, 2, c48), 4, c192[:32]) * 20.0 for v in (I, Q)]
