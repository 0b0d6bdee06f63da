"""The panadapter stage's integer mapping and dBm, restated in numpy from the firmware's text (float32 / float64 where
the firmware computes in float / double):

  pixelnew[x] = baseOffset + pixel_offset + (int16_t)(dBScale * log10f_fast(FFT_spec[x]))   FFT.cpp:157, 245
  y = spectrumNoiseFloor - pixel[x] - NF, held to [SPECTRUM_TOP_Y, SPECTRUM_BOTTOM] = [100, 249]  Display.cpp:343-358
  waterfall[x] = gradient[230 - y_new held to 0 .. 116], x = 0 .. 510                        Display.cpp:460-466
  oldNF = the row before's currentNF, this row's on the first row (newSpectrumFlag)          Display.cpp:250-256, 474
  pixelold[] = the row before's pixelnew[], zero at power-on                                 FFT.cpp:151, 216
  dbm, TCVSDR_SMETER                                                                         Display.cpp:959-962, 980-981

Everything here works on FFT_spec rows and audioMaxSquaredAve values that are given: the transform in front of them is
tested against the display side output."""
import numpy as np

F32 = np.float32
DISPLAY_SCALE = ((10.0, 24), (20.0, 10), (40.0, 58), (100.0, 120), (200.0, 200))  # displayScale[]: dBScale, baseOffset
TOP_Y, BOTTOM = 100, 249  # SPEC_BOX_T + 1; SPECTRUM_TOP_Y + SPECTRUM_HEIGHT - 1 (Display.h:13-22)
RES = 512


def log10f_fast(X):
    """Utility.cpp:245-258 in float32, element-wise; frexpf(0) = (0, 0), so log10f_fast(0) is finite"""
    F, E = np.frexp(np.abs(np.asarray(X, F32)))
    F = np.asarray(F, F32)
    Y = F32(1.23149591368684) * F
    Y = Y + F32(-4.11852516267426)
    Y = Y * F
    Y = Y + F32(6.02197014179219)
    Y = Y * F
    Y = Y + F32(-3.13396450166353)
    Y = Y + np.asarray(E).astype(F32)
    return np.asarray(Y * F32(0.3010299956639812), F32)


def pixelnew(spec, scale, pixel_offset):
    """int16 pixelnew[] of FFT_spec[]: uint16 + int16 + (int16_t)(float * float) in int, stored to an int16"""
    dB, base = DISPLAY_SCALE[scale]
    t = np.asarray(F32(dB) * log10f_fast(spec), F32)
    return (base + pixel_offset + np.trunc(t).astype(np.int32).astype(np.int16).astype(np.int32)).astype(np.int16)


def y_plot(pixel, noise_floor_y, nf):
    """y_new_plot / y_old_plot: int arithmetic, first held below SPECTRUM_BOTTOM, then above SPECTRUM_TOP_Y"""
    y = int(noise_floor_y) - np.asarray(pixel, np.int32) - int(nf)
    y = np.where(y > BOTTOM, BOTTOM, y)
    return np.where(y < TOP_Y, TOP_Y, y).astype(np.int16)


def waterfall(y_new, gradient):
    """the waterfall row: gradient[-y_new + 230 held to 0 .. 116] for x = 0 .. 510; [511] is never written: 0"""
    g = np.asarray(gradient, np.uint16)
    t = 230 - np.asarray(y_new, np.int32)
    t = np.where(t < 0, 0, t)
    t = np.where(t > 116, 116, t)
    w = g[t].astype(np.uint16)
    w[..., RES - 1] = 0
    return w


def rows(spec_rows, gradient, scale=1, pixel_offset=0, noise_floor_y=247, noise_floors=0, pixelold=None, old_nf=None):
    """One channel's rows in order.  spec_rows [k, 512] FFT_spec; noise_floors: currentNF of each row (a scalar: the same
    for all); pixelold / old_nf: the stage's memory in front of row 0 (None: power-on -- zero pixels, newSpectrumFlag 0).
    Returns dict pixel / y_new / y_old / waterfall [k, 512] and the memory behind the last row (pixelold, old_nf)."""
    spec_rows = np.asarray(spec_rows, F32)
    k = spec_rows.shape[0]
    nfs = np.broadcast_to(np.asarray(noise_floors, np.int64), (k,))
    pold = np.zeros(RES, np.int16) if pixelold is None else np.asarray(pixelold, np.int16)
    out = {n: np.zeros((k, RES), np.uint16 if n == "waterfall" else np.int16) for n in ("pixel", "y_new", "y_old", "waterfall")}
    for r in range(k):
        nf = int(nfs[r])
        if old_nf is None:  # newSpectrumFlag == 0
            old_nf = nf
        p = pixelnew(spec_rows[r], scale, pixel_offset)
        out["pixel"][r] = p
        out["y_new"][r] = y_plot(p, noise_floor_y, nf)
        out["y_old"][r] = y_plot(pold, noise_floor_y, old_nf)
        out["waterfall"][r] = waterfall(out["y_new"][r], gradient)
        pold, old_nf = p, nf
    return out, (pold, old_nf)


def dbm(ave, gain_correction=0.0, attenuator=0, RFgain=1, rfGainAllBands=1):
    """DrawSmeterBar(), TCVSDR_SMETER: float left to right up to cons, then - (float32_t)RFgain * 1.5 - rfGainAllBands in
    double, stored to the float32 dbm; no contraction"""
    t = F32(22.0) + F32(gain_correction)
    t = F32(t + F32(int(attenuator)))
    t = F32(t + F32(F32(10.0) * log10f_fast(F32(ave))))
    t = F32(t + F32(-92.0))
    d = np.float64(t) - np.float64(F32(int(RFgain))) * np.float64(1.5)
    d = d - np.float64(int(rfGainAllBands))
    return F32(d)


def ave_recurrence(max_squared, ave0=0.0):
    """audioMaxSquaredAve = .5 * audioMaxSquared + .5 * audioMaxSquaredAve (Process.cpp:569) over the given frames: double
    products and sum, stored to float32"""
    ave, out = F32(ave0), []
    for m in np.asarray(max_squared, F32):
        ave = F32(0.5 * np.float64(m) + 0.5 * np.float64(ave))
        out.append(ave)
    return np.asarray(out, F32)
