"""CPU models of the receive equalizer (DoReceiveEQ(), Filter.cpp:117-165; call site Process.cpp:828-832) on streams of
24 kS/s audio, 256-sample blocks.

* ``Restatement`` -- the f32 restatement: every band is ``df2t_model.cascade_oracle`` (the oracle's
  ``t41o_biquad_df2T_f32`` section by section), band k's output times ``signed_scales()[k - 1]`` (arm_scale_f32) and
  the sum EQ1 + EQ2, then + EQ3, .., + EQ14 (arm_add_f32), all in float32 with one rounding per operation.
* ``bank_numpy`` -- the same bank on ``df2t_model.cascade_f32``, the numpy float32 loop over samples, with the variants
  the tests set against it: contraction (every ``a*b + c`` rounded once) and a reordered sum.
* ``F64`` -- an independent float64 model: scipy's second-order sections on the same (float32-rounded) coefficients,
  float64 levels, a float64 sum.
"""
import os

import numpy as np
import scipy.signal as sg

from df2t_model import block_rel, cascade_f32, cascade_oracle, sos_of  # noqa: F401  (block_rel: for the tests)

BANDS, STAGES, N = 14, 4, 256
F = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))
# centre frequencies in the table's comments (FIR.cpp:279-370), Hz
CENTRES = (198.425, 250.0, 314.98, 400.0, 500.0, 630.0, 793.0, 1000.0, 1259.0, 1587.0, 2000.0, 2500.0, 3150.0, 4000.0)


def bands(kind="f32"):
    """the firmware's EQ_Band1Coeffs .. EQ_Band14Coeffs as [14][4][5]: the literals (``f64``) or the float32 values the
    firmware compiles (``f32``)"""
    z = np.load(os.path.join(HERE, "golden", "eq", "rx_eq_bands.npz"))
    return z["coeffs_f32"].copy() if kind == "f32" else z["coeffs_f64"].copy()


def level_scales(levels):
    """recEQ_LevelScale[i] = (float)EEPROMData.equalizerRec[i] / 100.0: int to float, divided in double, stored as float"""
    return np.array([F(np.float64(F(int(v))) / 100.0) for v in levels], F)


def signed_scales(levels):
    """arm_scale_f32's factor per band: -scale for bands 1, 3, .., 13, +scale for 2, 4, .., 14"""
    s = level_scales(levels)
    return np.where(np.arange(BANDS) % 2 == 0, -s, s).astype(F)


def sum_bands(eq, order="ref"):
    """eq [14][n] scaled band outputs -> out = EQ1 + EQ2, then + EQ3 .. + EQ14 (float32, that order)"""
    if order == "ref":
        out = eq[0] + eq[1]
        for k in range(2, BANDS):
            out = out + eq[k]
        return out
    out = eq[BANDS - 1] + eq[BANDS - 2]  # "reversed": the same terms from band 14 down
    for k in range(BANDS - 3, -1, -1):
        out = out + eq[k]
    return out


class Restatement:
    """one channel's equalizer with persistent state (rec_EQ_Band1_state .. rec_EQ_Band14_state, zero at power-on)"""

    def __init__(self, coeffs=None):
        self.c = np.ascontiguousarray(bands() if coeffs is None else coeffs, F).reshape(BANDS, STAGES, 5)
        self.st = np.zeros((BANDS, STAGES, 2), F)

    def block(self, x, levels, order="ref"):
        """one 256-sample block (or any length): the equalized samples; the state advances even where a level is 0"""
        x = np.ascontiguousarray(x, F)
        eq = np.stack([cascade_oracle(self.c[b], self.st[b], x) for b in range(BANDS)])
        eq *= signed_scales(levels)[:, None]
        return sum_bands(eq, order)

    def stream(self, x, levels, on=None, order="ref"):
        """a stream of 256-sample blocks; blocks where on[b] is False pass unchanged and leave the state alone"""
        x = np.asarray(x, F)
        out = x.copy()
        for b in range(x.size // N):
            if on is None or on[b]:
                out[b * N:(b + 1) * N] = self.block(x[b * N:(b + 1) * N], levels, order)
        return out


def bank_numpy(x, levels, coeffs=None, fma=False, order="ref"):
    """the whole bank on one stream as a float32 loop over samples, vectorised over bands; ``fma=True`` rounds every
    a*b + c once (the contracted form), ``order="reversed"`` sums from band 14 down"""
    c = (bands() if coeffs is None else np.asarray(coeffs, F)).reshape(BANDS, STAGES, 5)
    y = cascade_f32(x, c, fma)
    return sum_bands(y * signed_scales(levels)[:, None], order)


class F64:
    """the independent float64 model of the same bank (scipy sosfilt, float64 levels and sum)"""

    def __init__(self, coeffs=None):
        c = np.asarray(bands() if coeffs is None else coeffs, np.float64).reshape(BANDS, STAGES, 5)
        self.sos = [sos_of(c[b]) for b in range(BANDS)]
        self.zi = [np.zeros((STAGES, 2)) for _ in range(BANDS)]

    def block(self, x, levels):
        x = np.asarray(x, np.float64)
        sign = np.where(np.arange(BANDS) % 2 == 0, -1.0, 1.0)
        out = np.zeros(x.size)
        for b in range(BANDS):
            y, self.zi[b] = sg.sosfilt(self.sos[b], x, zi=self.zi[b])
            out += sign[b] * (float(levels[b]) / 100.0) * y
        return out

    def stream(self, x, levels, on=None):
        x = np.asarray(x, np.float64)
        out = x.copy()
        for b in range(x.size // N):
            if on is None or on[b]:
                out[b * N:(b + 1) * N] = self.block(x[b * N:(b + 1) * N], levels)
        return out

    def response(self, f_hz, band, fs=24000.0):
        """|H_band(f)| of one band's 4-section cascade"""
        _, h = sg.sosfreqz(self.sos[band], worN=np.atleast_1d(np.asarray(f_hz, np.float64)), fs=fs)
        return np.abs(h)
