"""CPU models of the CW receive block (Process.cpp:878-913) on streams of 24 kS/s audio, 256-sample blocks.

* ``Restatement`` -- the f32 restatement of one channel, a block at a time, with persistent state: the tone detector
  of DoCWReceiveProcessing() (CWProcessing.cpp:322-373; goertzel_mag, :830-857) on one audio stream (float_buffer_R =
  float_buffer_L), then the narrow audio filter CWFilterIndex selects (five arm_biquad_cascade_df2T_f32 instances of six
  sections, CWProcessing.cpp:36-48, each with its own memory), by ``df2t_model.cascade_oracle``;
  arm_fir_f32 is ``tx_model.fir_f32`` (one accumulator in tap order); arm_correlate_f32 sums every lag sequentially in
  increasing sample index; all in float32 with one rounding per multiply and per add.  CMSIS-DSP itself is not
  available here: this restatement is the pin.
* ``cascade_numpy`` -- one filter on ``df2t_model.cascade_f32``, the numpy float32 loop over samples, with the
  contracted variant (every ``a*b + c`` rounded once) the tests set against it.
* ``filter_f64`` / ``detect_f64`` -- independent float64 models (scipy sosfilt, lfilter, np.correlate, the DFT bin).
"""
import os

import numpy as np

from df2t_model import block_rel, cascade_f32, cascade_oracle, sos_of  # noqa: F401  (block_rel, sos_of: for the tests)
from tx_model import fir_f32

N, TAPS, FILTERS, STAGES, OFF = 256, 64, 5, 6, 5
F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
CUTOFFS = (840.0, 1080.0, 1320.0, 1800.0, 2000.0)  # Hz, from the tables' comments (FIR.cpp:13-56)


def tables(kind="f32"):
    """(filters [5][6][5], fir [64]): the firmware's CW_AudioFilterCoeffs1..5 and CW_Filter_Coeffs2 -- the literals
    (``f64``) or the float32 values the firmware compiles (``f32``)"""
    z = np.load(os.path.join(HERE, "golden", "cw", "cw_tables.npz"))
    return z["filters_" + kind].copy(), z["fir_" + kind].copy()


def sin_buffer():
    """sineTone() (Utility.cpp:72-74): float theta = kf * 0.19634950849362; sinBuffer[kf] = sin(theta)"""
    theta = (np.arange(N) * 0.19634950849362).astype(F)
    return np.sin(theta.astype(np.float64)).astype(F)


def goertzel_consts():
    """goertzel_mag(256, 750, 24000, .)'s k, and sine, cosine, coeff as floats (CWProcessing.cpp:835-842)"""
    fn = F(N)
    k = int(0.5 + float(fn * F(750) / F(24000)))
    omega = F((2.0 * np.pi * k) / float(fn))
    sine, cosine = F(np.sin(np.float64(omega))), F(np.cos(np.float64(omega)))
    return k, sine, cosine, F(2.0 * np.float64(cosine))


def goertzel_mag(data):
    _, sine, cosine, coeff = goertzel_consts()
    q1 = q2 = F(0)
    for v in np.asarray(data, F):
        q0 = coeff * q1 - q2 + v
        q2, q1 = q1, q0
    real = (q1 - q2 * cosine) / F(128.0)
    imag = (q2 * sine) / F(128.0)
    return np.sqrt(real * real + imag * imag)


def correlate_f32(a, b):
    """arm_correlate_f32(a, 256, b, 256, .): lag j = sum_i a[i] * b[255 - j + i], every sum in increasing i"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    acc = np.zeros(2 * N - 1, F)
    brev = b[::-1].copy()
    for i in range(N):
        acc[i:i + N] = acc[i:i + N] + a[i] * brev
    return acc


class Restatement:
    """one channel; CW_AudioFilter1..5_state, FIR_CW_DecodeL_state, corrResultR, aveCorrResultL / R: zero at power-on"""

    def __init__(self, filters=None, fir=None):
        t = tables()
        self.c = np.ascontiguousarray(t[0] if filters is None else filters, F).reshape(FILTERS, STAGES, 5)
        self.fir = np.ascontiguousarray(t[1] if fir is None else fir, F)
        self.st = np.zeros((FILTERS, STAGES, 2), F)
        self.fir_state = np.zeros(TAPS - 1 + N, F)
        self.corrR = self.aveL = self.aveR = F(0)
        self.sinb = sin_buffer()

    def detect(self, x):
        """one block through the detector: (corrResultL, goertzelMagnitude, aveCorrResult, combinedCoeff)"""
        cw = fir_f32(self.fir, self.fir_state, np.ascontiguousarray(x, F))
        corrL = correlate_f32(cw, self.sinb).max()
        self.aveL = F(.7 * np.float64(corrL) + .3 * np.float64(self.aveL))
        ave = (self.corrR + corrL) / F(2)  # corrResultR is still the block before's (:339 runs before :348)
        g1 = goertzel_mag(cw)
        self.corrR = corrL  # float_buffer_R = float_buffer_L: the right side repeats the left
        self.aveR = F(.7 * np.float64(self.corrR) + .3 * np.float64(self.aveR))
        g = (g1 + g1) / F(2)
        comb = F(10) * ave * F(100) * g
        return np.array([corrL, g, ave, comb], F)

    def filter(self, x, index):
        return cascade_oracle(self.c[index], self.st[index], x)

    def block(self, x, index=OFF, detector=False):
        """one 256-sample block as Process.cpp:878-913 runs it: (audio, detector results or None)"""
        x = np.ascontiguousarray(x, F)
        d = self.detect(x) if detector else None
        return (x.copy() if index == OFF else self.filter(x, index)), d

    def stream(self, x, index=OFF, detector=False, on=None):
        """a stream of blocks; index / detector may be per-block sequences; blocks where on[b] is False (another
        xmtMode) pass unchanged, leave the state alone and yield a row of NaN"""
        x = np.asarray(x, F)
        nb = x.size // N
        idx = [index] * nb if np.isscalar(index) else list(index)
        det = [detector] * nb if isinstance(detector, (bool, int)) else list(detector)
        out, res = x.copy(), np.full((nb, 4), np.nan, F)
        for b in range(nb):
            if on is not None and not on[b]:
                continue
            y, d = self.block(x[b * N:(b + 1) * N], idx[b], det[b])
            out[b * N:(b + 1) * N] = y
            if d is not None:
                res[b] = d
        return out, res

    def state_vector(self):
        """the 128 floats of the checkpoint section"""
        v = np.zeros(128, F)
        v[:60] = self.st.reshape(-1)
        v[60:123] = self.fir_state[:TAPS - 1]
        v[123], v[124], v[125] = self.corrR, self.aveL, self.aveR
        return v


def cascade_numpy(x, coeffs, fma=False):
    """one six-section filter from zero memories as a float32 loop over samples; ``fma=True`` rounds every a*b + c once"""
    return cascade_f32(x, np.asarray(coeffs, F).reshape(STAGES, 5), fma)


def filter_f64(x, coeffs):
    """the whole stream through one filter in float64 (the float32-rounded coefficients), from zero memories"""
    import scipy.signal as sg
    return sg.sosfilt(sos_of(coeffs), np.asarray(x, np.float64))


def detect_f64(x, fir=None):
    """float64 detector over a stream: per block (corrResultL, goertzelMagnitude, aveCorrResult, combinedCoeff), the
    FIR continuous over the stream, the correlation by np.correlate, the Goertzel magnitude as |DFT bin 8| / 128"""
    import scipy.signal as sg
    fir = np.asarray(tables()[1] if fir is None else fir, np.float64)
    # arm_fir_f32 applies coeffs[i] to state[n + i]: coeffs[63] meets the newest sample
    cw = sg.lfilter(fir[::-1], [1.0], np.asarray(x, np.float64))
    sinb = sin_buffer().astype(np.float64)
    k = goertzel_consts()[0]
    w = np.exp(-2j * np.pi * k * np.arange(N) / N)
    res, prev = [], 0.0
    for b in range(cw.size // N):
        blk = cw[b * N:(b + 1) * N]
        corr = np.correlate(blk, sinb, "full").max()
        g = abs(np.dot(blk, w)) / 128.0
        ave = (prev + corr) / 2
        prev = corr
        res.append((corr, g, ave, 10 * ave * 100 * g))
    return np.array(res)
