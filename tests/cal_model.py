"""CPU models of the IQ calibration, ProcessIQData2() (Process2.cpp:295-399) with PlotCalSpectrum()'s measurement
(:478-547), which the frozen oracle does not hold.

Transmit half (:309-349):
* ``CalTxModel`` / ``CalTxModelBatch`` -- the f32 restatement.  It extends ``cw_tx_model.CwTxModel``, so SSB, CW and
  calibration frames drive the same ``int1`` / ``int2`` memories, as the firmware's FIR_int1_EX_I/Q and FIR_int2_EX_I/Q.
  The scalings are numpy float32 products; the interpolators and the conversion are the oracle's exported primitives.
* ``cal_tx_stream_model_f64`` -- an independent float64 model of a whole stream from power-on (scipy lfilter).
Receive half and measurement (:352-397, FFT.cpp:67-157, 208-251):
* ``CalRxModel`` -- the f32 restatement of one channel in the firmware's operation order: numpy float32 products and
  sums (one rounding each), the float / double mix of FFT.cpp:110-111, 153, 221-222, 241, and the oracle's exported
  primitives ``t41o_cfft_f32``, ``t41o_biquad_df1_f32``, ``t41o_fir_decimate_f32`` and ``t41o_CalcFIRCoeffs``.
* ``log10f_fast`` / ``pixels`` / ``measure`` -- Utility.cpp:245-258, the pixel mapping and the two window maxima with
  adjdB, usable on any FFT_spec (the GPU's own included).
* ``cal_rx_model_f64`` -- an independent float64 model of FFT_spec (numpy FFT, scipy lfilter, no CMSIS state).
* ``imbalanced_tone`` / ``sweep`` -- the closed loop: samples whose imbalance a grid point of the firmware's correction
  formula removes exactly, and the sweep's verdict on the model.
"""
import ctypes as C

import numpy as np

import oracle_lib as O
from cw_tx_model import FRAME, TONE, CwTxModel, CwTxModelBatch
from tx_model import F32

L, R = 2048, 512
DISPLAY_SCALE = ((10.0, 24), (20.0, 10), (40.0, 58), (100.0, 120), (200.0, 200))  # dBScale, baseOffset: Display.cpp:127-135
RX_BINS = {O.DEMOD_LSB: (310, 460), O.DEMOD_USB: (65, 192)}   # cal_bins[], Process2.cpp:429-444
TX_BINS = {O.DEMOD_LSB: (240, 305), O.DEMOD_USB: (209, 273)}
WIN = 0.5 - 0.5 * np.cos(6.28 * np.arange(R) / R)             # FFT.cpp:110, 221: a double expression, 6.28 as written


def cal_tone():
    """cosBuffer3 / sinBuffer3, Utility.cpp:78-80: theta is a float holding the double kf * 2.0 * PI * 3000 / 24000"""
    theta = np.array([np.float32(kf * 2.0 * np.pi * 3000.0 / 24000.0) for kf in range(TONE)], np.float32)
    return np.cos(theta.astype(np.float64)).astype(F32), np.sin(theta.astype(np.float64)).astype(F32)


# ---- transmit half
class CalTxModel(CwTxModel):
    """one exciter channel with all three entries; cal_frame() touches int1 / int2 and nothing else"""

    def cal_frame(self, cos, sin, level, mode=O.DEMOD_USB, amp=1.0, phase=0.0):
        sp = C.POINTER(C.c_int16)
        I = np.asarray(cos, F32) * F32(level)                                                        # Process2.cpp:313
        Q = np.asarray(sin, F32) * F32(level)                                                        # :314
        assert I.shape == (TONE,) and Q.shape == (TONE,)
        amp, phase = F32(amp), F32(phase)
        if mode in (O.DEMOD_LSB, O.DEMOD_USB):                                                       # :317-325
            I = I * (-amp if mode == O.DEMOD_LSB else amp)
            if phase < 0.0:                                                                          # Utility.cpp:178-187
                Q = Q + I * phase
            else:
                I = I + Q * phase
        A, T = np.empty(FRAME, F32), np.empty(FRAME, F32)
        outs = []
        for k, v in enumerate((I, Q)):
            A[:TONE] = v
            self.lib.t41o_fir_interpolate_f32(O.fptr(self.c48), 48, 2, O.fptr(self.int1[k]), O.fptr(A), O.fptr(T), 256)   # :327, 333
            self.lib.t41o_fir_interpolate_f32(O.fptr(self.c192), 32, 4, O.fptr(self.int2[k]), O.fptr(T), O.fptr(A), 512)  # :330, 334
            o = np.empty(FRAME, np.int16)
            self.lib.t41o_float_to_q15(O.fptr(A), o.ctypes.data_as(sp), FRAME)                       # :344-345, no x 20
            outs.append(o)
        return outs[0], outs[1]


class CalTxModelBatch(CwTxModelBatch):
    """nchan CalTxModel channels: process() SSB frames, process_cw() CW frames, process_cal() calibration frames on the
    same memories.  amps / phases: per-channel candidates for process_cal(), None = the scalar amp / phase"""

    def __init__(self, nchan, mode=O.DEMOD_USB, amp=1.0, phase=0.0, tone=None, cal=None, level=0.5, amps=None, phases=None, **kw):
        super().__init__(nchan, mode, amp, phase, tone=tone, **kw)
        self.chs = [CalTxModel(kw.get("coeffs")) for _ in range(nchan)]
        self.cal, self.level, self.amps, self.phases = cal, level, amps, phases

    def process_cal(self, n_frames):
        cos, sin = self.cal
        oL, oR = np.empty((self.nchan, n_frames * FRAME), np.int16), np.empty((self.nchan, n_frames * FRAME), np.int16)
        for c, ch in enumerate(self.chs):
            a = self.amp if self.amps is None else self.amps[c]
            p = self.phase if self.phases is None else self.phases[c]
            for f in range(n_frames):
                sl = slice(f * FRAME, (f + 1) * FRAME)
                oL[c, sl], oR[c, sl] = ch.cal_frame(cos, sin, self.level, self.mode, a, p)
        return oL, oR


def cal_tx_stream_model_f64(cos, sin, level, n_frames, mode, amp, phase, tabs):
    """whole-stream float64 model of one channel from power-on; tabs: the oracle's four TX tables.  Returns the I and Q
    drive as float64 in units of full scale."""
    from scipy.signal import lfilter
    c192, c48 = np.asarray(tabs[0], np.float64), np.asarray(tabs[1], np.float64)
    I = np.tile(np.asarray(cos, np.float64), n_frames) * np.float64(F32(level))
    Q = np.tile(np.asarray(sin, np.float64), n_frames) * np.float64(F32(level))
    amp, phase = np.float64(F32(amp)), np.float64(F32(phase))
    if mode in (O.DEMOD_LSB, O.DEMOD_USB):
        I = I * (-amp if mode == O.DEMOD_LSB else amp)
        if phase < 0:
            Q = Q + I * phase
        else:
            I = I + Q * phase

    def interp(v, up, c):  # arm_fir_interpolate_f32: zero stuffing + the time-reversed taps, no make-up gain
        z = np.zeros(v.size * up)
        z[::up] = v
        return lfilter(c[::-1], 1.0, z)

    return [interp(interp(v, 2, c48), 4, c192[:32]) for v in (I, Q)]


# ---- the measurement
def log10f_fast(X):
    """Utility.cpp:245-258 in float32, element-wise; frexpf(0) = (0, 0), so log10f_fast(0) is finite"""
    F, E = np.frexp(np.abs(np.asarray(X, F32)))
    F = F.astype(F32)
    Y = F32(1.23149591368684) * F
    Y = Y + F32(-4.11852516267426)
    Y = Y * F
    Y = Y + F32(6.02197014179219)
    Y = Y * F
    Y = Y + F32(-3.13396450166353)
    Y = Y + E.astype(F32)
    return (Y * F32(0.3010299956639812)).astype(F32)


def pixels(spec, scale=1, pixel_offset=0):
    """pixelnew[] from FFT_spec[] (FFT.cpp:157, 245): uint16 + int16 + (int16_t)(float * float) in int, stored to int16"""
    dB, base = DISPLAY_SCALE[scale]
    t = (F32(dB) * log10f_fast(spec)).astype(F32)
    return (base + pixel_offset + np.trunc(t).astype(np.int32).astype(np.int16).astype(np.int32)).astype(np.int16)


def measure(pix, mode, bin0, bin1, capture=10):
    """(refAmplitude, adjAmplitude, adjdB) from pixelnew[] (Process2.cpp:498-505, 524), float32 [..., 3]"""
    pix = np.asarray(pix, np.int16)
    m0 = pix[..., bin0 - capture:bin0 + capture].max(axis=-1).astype(np.int32)
    m1 = pix[..., bin1 - capture:bin1 + capture].max(axis=-1).astype(np.int32)
    if mode == O.DEMOD_LSB:
        ref, adj = m0, m1
    elif mode == O.DEMOD_USB:
        ref, adj = m1, m0
    else:
        ref, adj = np.zeros_like(m0), np.zeros_like(m0)
    d = (adj.astype(F32) - ref.astype(F32)).astype(np.float64) / 1.95
    return np.stack([ref.astype(F32), adj.astype(F32), d.astype(F32)], axis=-1)


def zoom_tables(zoom):
    from test_display_spectrum_tables import MAG_COEFFS
    coeffs = np.array(MAG_COEFFS[zoom - 1], F32)
    fir = np.zeros(4, F32)
    O.lib().t41o_CalcFIRCoeffs(O.fptr(fir), 4, np.float32(0.5 * 192000 / (1 << zoom)), 60.0, 0, 0.0, 192000.0)
    return coeffs, fir


def front(I, Q, mode, amp, phase, rf_gain_db=1, q15=False, dtype=F32):
    """one frame up to and including FreqShift1() (Process2.cpp:359-385) in ``dtype``; q15: I / Q are the queues Q_in_L /
    Q_in_R, float_buffer_L is filled from the R queue"""
    if q15:
        I, Q = (np.asarray(Q, np.int16).astype(dtype) / dtype(32768.0)), (np.asarray(I, np.int16).astype(dtype) / dtype(32768.0))
    else:
        I, Q = np.asarray(I, F32).astype(dtype), np.asarray(Q, F32).astype(dtype)
    g = dtype(F32(10.0 ** float(F32(rf_gain_db) / F32(20.0))))  # (float)pow(10, (float)rfGainAllBands / 20)
    I, Q = I * g, Q * g
    I, Q = I * dtype(1.0), Q * dtype(1.0)                      # recBandFactor
    amp, phase = dtype(F32(amp)), dtype(F32(phase))
    if mode in (O.DEMOD_LSB, O.DEMOD_USB):
        I = I * -amp
        if phase < 0.0:
            Q = Q + I * phase
        else:
            I = I + Q * phase
    oi, oq = I.copy(), Q.copy()                                # FreqShift1: x j^n
    oi[1::4], oq[1::4] = -Q[1::4], I[1::4]
    oi[2::4], oq[2::4] = -I[2::4], -Q[2::4]
    oi[3::4], oq[3::4] = Q[3::4], -I[3::4]
    return oi, oq


class CalRxModel:
    """one channel's receive half in float32: the calibration memory (FFT_spec_old, zoom memories, ring and pointer,
    pixelnew) starts at power-on values"""

    def __init__(self, mode, amp=1.0, phase=0.0, zoom=0, scale=1, pixel_offset=0, bins=None, capture=10, rf_gain_db=1):
        self.mode, self.amp, self.phase, self.zoom, self.scale, self.pixel_offset = mode, amp, phase, zoom, scale, pixel_offset
        self.bins = RX_BINS.get(mode, (310, 460)) if bins is None else bins
        self.capture, self.rf_gain_db = capture, rf_gain_db
        self.lib = O.lib()
        if zoom:
            self.coeffs, self.fir = zoom_tables(zoom)
        self.reset()

    def reset(self):
        self.old = np.zeros(R, F32)
        self.iir = np.zeros((2, 4, 4), F32)
        self.firstate = [np.zeros(3 + L, F32), np.zeros(3 + L, F32)]
        self.ring = np.zeros((2, R), F32)
        self.ptr = 0
        self.pix = np.zeros(R, np.int16)

    def fft_spec(self, I, Q, q15=False):
        """one flagged frame -> FFT_spec[512] as the firmware leaves it (un-smoothed at zoom 0, smoothed above)"""
        x, y = front(I, Q, self.mode, self.amp, self.phase, self.rf_gain_db, q15)
        buf = np.empty(2 * R, F32)
        lpf = F32(0.7)
        if self.zoom == 0:
            buf[0::2] = (x[:R].astype(np.float64) * WIN).astype(F32)                                 # FFT.cpp:221-222
            buf[1::2] = (y[:R].astype(np.float64) * WIN).astype(F32)
        else:
            M = 1 << self.zoom
            n = min(L // M, R)
            dec = []
            for k, v in enumerate((x, y)):
                src = np.ascontiguousarray(v, F32)
                for s in range(4):                                                                   # :83-84
                    dst = np.empty(L, F32)
                    self.lib.t41o_biquad_df1_f32(O.fptr(np.ascontiguousarray(self.coeffs[5 * s:5 * s + 5])), O.fptr(self.iir[k, s]),
                                                 O.fptr(src), O.fptr(dst), L)
                    src = dst
                out = np.empty(L, F32)
                self.lib.t41o_fir_decimate_f32(O.fptr(self.fir), 4, M, O.fptr(self.firstate[k]), O.fptr(src), O.fptr(out), L)  # :87-88
                dec.append(out[:n])
            idx = (self.ptr + np.arange(n)) % R                                                      # :97-103
            self.ring[0, idx], self.ring[1, idx] = dec[0], dec[1]
            self.ptr = (self.ptr + n) % R
            mult = F32(1 << self.zoom) if self.zoom > 3 else F32(self.zoom)                          # :105-108
            rd = (self.ptr + np.arange(R)) % R
            buf[0::2] = ((mult * self.ring[0, rd]).astype(np.float64) * WIN).astype(F32)            # :110-111
            buf[1::2] = ((mult * self.ring[1, rd]).astype(np.float64) * WIN).astype(F32)
        self.lib.t41o_cfft_f32(O.fptr(buf), R, 0)
        m = np.roll(buf[0::2] * buf[0::2] + buf[1::2] * buf[1::2], R // 2)                           # :136-139, 234-237
        if self.zoom == 0:                                                                           # :241-245
            self.old = ((lpf * m).astype(np.float64) + (1.0 - np.float64(lpf)) * self.old.astype(np.float64)).astype(F32)
            return m
        onem = F32(1.0 - np.float64(lpf))                                                            # :130, 153-154
        self.old = lpf * m + onem * self.old
        return self.old.copy()

    def frame(self, I, Q, update=True, q15=False):
        """one ProcessIQData2() + PlotCalSpectrum(): (FFT_spec or None, pixelnew copy, result[3])"""
        spec = None
        if update:
            spec = self.fft_spec(I, Q, q15)
            self.pix = pixels(spec, self.scale, self.pixel_offset)
        return spec, self.pix.copy(), measure(self.pix, self.mode, self.bins[0], self.bins[1], self.capture)

    def run(self, I, Q, mask=None, q15=False):
        """a stream of frames -> (spec [nfr, 512] with NaN rows where the flag is 0, pixel [nfr, 512], result [nfr, 3])"""
        nfr = np.asarray(I).size // L
        mask = np.ones(nfr, np.uint8) if mask is None else np.asarray(mask)
        S, P, Rs = np.full((nfr, R), np.nan, F32), np.zeros((nfr, R), np.int16), np.zeros((nfr, 3), F32)
        for f in range(nfr):
            sl = slice(f * L, (f + 1) * L)
            s, P[f], Rs[f] = self.frame(np.asarray(I)[sl], np.asarray(Q)[sl], bool(mask[f]), q15)
            if s is not None:
                S[f] = s
        return S, P, Rs


def cal_rx_model_f64(I, Q, mode, amp, phase, zoom, mask=None, rf_gain_db=1, q15=False):
    """independent float64 model of FFT_spec for the flagged frames of a stream, [n_flagged, 512]"""
    from scipy.signal import lfilter
    nfr = np.asarray(I).size // L
    mask = np.ones(nfr, np.uint8) if mask is None else np.asarray(mask)
    old = np.zeros(R)
    ring, ptr = np.zeros(R, complex), 0
    zi, hist = [np.zeros(2, complex) for _ in range(4)], np.zeros(3, complex)
    if zoom:
        coeffs, fir = zoom_tables(zoom)
    out = []
    for f in range(nfr):
        if not mask[f]:
            continue
        sl = slice(f * L, (f + 1) * L)
        x, y = front(np.asarray(I)[sl], np.asarray(Q)[sl], mode, amp, phase, rf_gain_db, q15, dtype=np.float64)
        z = x + 1j * y
        if zoom == 0:
            blk = z[:R] * WIN
        else:
            for s in range(4):
                b = coeffs[5 * s:5 * s + 3].astype(np.float64)
                a = np.array([1.0, -coeffs[5 * s + 3], -coeffs[5 * s + 4]], np.float64)
                z, zi[s] = lfilter(b, a, z, zi=zi[s])
            M = 1 << zoom
            ext = np.concatenate([hist, z])
            dec = np.array([np.dot(fir.astype(np.float64), ext[k * M:k * M + 4]) for k in range(L // M)])
            hist = z[-3:]
            n = min(L // M, R)
            ring[(ptr + np.arange(n)) % R] = dec[:n]
            ptr = (ptr + n) % R
            blk = (float(1 << zoom) if zoom > 3 else float(zoom)) * ring[(ptr + np.arange(R)) % R] * WIN
        spec = np.roll(np.abs(np.fft.fft(blk)) ** 2, R // 2)
        if zoom == 0:
            out.append(spec)
        else:
            lpf = np.float64(F32(0.7))
            old = lpf * spec + np.float64(F32(1.0 - lpf)) * old
            out.append(old.copy())
    return np.array(out)


# ---- the closed loop
def imbalanced_tone(nfr, mode, amp_star, phase_star, f_hz=None, level=0.25, noise=1e-4, seed=5):
    """I / Q (float32, nfr * 2048) of a clean single-sideband tone whose imbalance is the exact inverse of the firmware's
    correction at (amp_star, phase_star): after I' = I x -amp and IQPhaseCorrection() the corrected pair is the balanced
    -cos / sin (or its mirror) again.  The tone sits where the firmware's receive calibration expects it after the
    Fs/4 shift: bin 310 (LSB) or 192 (USB) of the 375 Hz grid carries the wanted sideband, its image the other window.  A little noise keeps
    log10f_fast off the -inf side of an empty bin."""
    bins = RX_BINS[mode]
    want = bins[0] if mode == O.DEMOD_LSB else bins[1]
    f_disp = (want - 256) * 375.0 if f_hz is None else f_hz       # where the wanted tone shows
    f0 = f_disp - 48000.0                                          # FreqShift1 moves everything up by Fs/4
    n = np.arange(nfr * L)
    w = 2 * np.pi * f0 / 192000.0 * n
    Ic, Qc = level * np.cos(w), level * np.sin(w)                  # the balanced pair the correction must restore
    a, p = float(F32(amp_star)), float(F32(phase_star))
    # invert: Ic = -a I (+ p Qc if p >= 0);  Qc = Q (+ p Ic' if p < 0), with Ic' = -a I
    if p < 0:
        I = Ic / -a
        Q = Qc - p * Ic
    else:
        Q = Qc
        I = (Ic - p * Qc) / -a
    rng = np.random.default_rng(seed)
    I = I + noise * rng.standard_normal(n.size)
    Q = Q + noise * rng.standard_normal(n.size)
    return I.astype(F32), Q.astype(F32)


def sweep(I, Q, amps, phases, mode, zoom=0, frames=None, **kw):
    """the model's receive_iq_sweep: update mask 1 on the first frame only; returns (adjdB grid of the last frame,
    (i_amp, i_phase) of the lowest, ties to the lowest index, result [channels, frames, 3])"""
    nfr = np.asarray(I).size // L if frames is None else frames
    mask = np.zeros(nfr, np.uint8)
    mask[0] = 1
    res = np.array([CalRxModel(mode, a, p, zoom, **kw).run(I, Q, mask)[2] for a in amps for p in phases])
    grid = res[:, -1, 2].reshape(len(amps), len(phases))
    c = int(np.argmin(grid.reshape(-1)))
    return grid, (c // len(phases), c % len(phases)), res
