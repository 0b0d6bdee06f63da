"""IQ calibration sweeps: what DoReceiveCalibrate() / DoXmitCalibrate() (Process2.cpp:159-283) do with an operator and an
encoder, done with the batch axis.  Every channel of a context tries its own (amplitude, phase) candidate; one launch
measures them all, and the candidate with the lowest adjdB -- the unwanted sideband against the wanted one, as
PlotCalSpectrum() computes it -- wins.

  receive_iq_sweep()   one recording of the receiver's I / Q, a grid of IQAmpCorrectionFactor x IQPhaseCorrectionFactor
  transmit_iq_sweep()  a grid of IQXAmpCorrectionFactor x IQXPhaseCorrectionFactor through the calibration exciter, the
                       caller's loop-back (the analog path between DAC and ADC), and the receiver's measurement
All arithmetic happens in libt41rx.so (HIP); there is no CPU fallback.
"""
import collections

import numpy as np

from ._lib import DEMOD_LSB, DEMOD_USB
from .rx import RxChain, default_params
from .tx import TxChain, cal_tone, default_tx_params

RX_FRAMES, TX_FRAMES = 40, 64  # ProcessIQData2() calls per ShowSpectrum2() sweep: receive / transmit calibration
RX_ZOOM, TX_ZOOM = 0, 2        # spectrumZoom the firmware calibrates at
FRAME = 2048

SweepResult = collections.namedtuple("SweepResult", "adjdB best amp phase result")
SweepResult.__doc__ = """adjdB [len(amps), len(phases)]: the last frame's adjdB per candidate; best = (i_amp, i_phase) of the
lowest one, ties to the lowest channel index; amp, phase: that candidate; result [channels, frames, 3]: refAmplitude,
adjAmplitude, adjdB of every frame"""


def candidate_grid(amps, phases):
    """channel c = i_amp * len(phases) + i_phase -> (amp[c], phase[c]) as float32"""
    a = np.asarray(amps, np.float32).reshape(-1)
    p = np.asarray(phases, np.float32).reshape(-1)
    if a.size == 0 or p.size == 0:
        raise ValueError("amps and phases must not be empty")
    return np.repeat(a, p.size), np.tile(p, a.size)


def best_candidate(result, amps, phases):
    """the sweep's verdict from result [channels, frames, 3]"""
    na, npz = np.asarray(amps).size, np.asarray(phases).size
    last = np.asarray(result)[:, -1, 2].reshape(na, npz)
    c = int(np.argmin(last.reshape(-1)))  # the first minimum: ties to the lowest index
    ga, gp = candidate_grid(amps, phases)
    return SweepResult(last, (c // npz, c % npz), float(ga[c]), float(gp[c]), np.asarray(result))


def _params(mode, params):
    """the context's parameters: the caller's, or the defaults with the pass band on the mode's side of the carrier"""
    if params is not None:
        params.mode = mode
        return params
    p = default_params()
    if mode == DEMOD_LSB:
        p.FLoCut, p.FHiCut = -p.FHiCut, -p.FLoCut
    p.mode = mode
    return p


def _update_mask(frames):
    u = np.zeros(frames, np.uint8)
    u[0] = 1  # PlotCalSpectrum() sets updateDisplayFlag on the first call of a sweep only (Process2.cpp:485-488)
    return u


def receive_iq_sweep(I, Q, amps, phases, mode, frames=RX_FRAMES, spectrumZoom=RX_ZOOM, currentScale=1, pixel_offset=0,
                     bins=None, capture_bins=10, params=None, device=0):
    """One receive-calibration sweep over the grid amps x phases on one recording.  I / Q: the receiver's samples during
    the calibration tone, frames * 2048 each, float32 (float_buffer_L / _R) or int16 (Q_in_L / Q_in_R).  mode: DEMOD_LSB
    or DEMOD_USB; bins: (bin0, bin1), default the firmware's receive pair for the mode.  The other fields of params
    (rfGainAllBands ...) are the context's.  Returns a SweepResult."""
    if mode not in (DEMOD_LSB, DEMOD_USB):
        raise ValueError("IQ calibration runs in LSB or USB")
    I, Q = np.asarray(I), np.asarray(Q)
    if I.shape != Q.shape or I.reshape(-1).size != frames * FRAME:
        raise ValueError("I / Q must hold frames * 2048 = %d samples each, got %r / %r" % (frames * FRAME, I.shape, Q.shape))
    ga, gp = candidate_grid(amps, phases)
    p = _params(mode, params)
    b0, b1 = RxChain.CAL_BINS[("rx", mode)] if bins is None else bins
    rx = RxChain(ga.size, p, device=device)
    try:
        rx.set_calibration(True, spectrumZoom, currentScale, pixel_offset, b0, b1, capture_bins)
        rx.set_cal_corrections(ga, gp)
        res, _, _ = rx.ProcessIQData2_rx(I.reshape(1, -1), Q.reshape(1, -1), update=_update_mask(frames), shared_input=True)
    finally:
        rx.close()
    return best_candidate(res, amps, phases)


def transmit_iq_sweep(loopback, amps, phases, mode, level, frames=TX_FRAMES, spectrumZoom=TX_ZOOM, currentScale=1,
                      pixel_offset=0, bins=None, capture_bins=10, params=None, tone=None, device=0):
    """One transmit-calibration sweep: every candidate's calibration exciter output (Q_out_L_Ex, Q_out_R_Ex, int16
    [channels, frames * 2048]) goes through loopback(Q_out_L_Ex, Q_out_R_Ex) -> what RxChain.ProcessIQData2_rx() takes, two
    arrays of the same shape: float32 (I, Q) or int16 (Q_in_L, Q_in_R) -- the analog path between DAC and ADC is the
    caller's -- and the receiver measures each channel with the RX
    corrections of params.  level: the firmware's bandOutputFactor; tone: (cosBuffer3, sinBuffer3), default cal_tone().
    Returns a SweepResult."""
    if mode not in (DEMOD_LSB, DEMOD_USB):
        raise ValueError("IQ calibration runs in LSB or USB")
    ga, gp = candidate_grid(amps, phases)
    tx = TxChain(ga.size, default_tx_params(mode=mode), device=device)
    try:
        tx.set_cal_tone(*(cal_tone() if tone is None else tone), level)
        tx.set_cal_corrections(ga, gp)
        oL, oR = tx.ProcessIQData2_tx(frames)
    finally:
        tx.close()
    I, Q = loopback(oL, oR)
    I, Q = np.asarray(I), np.asarray(Q)
    if I.shape != oL.shape or Q.shape != oL.shape:
        raise ValueError("loopback must return two arrays of shape %r, got %r / %r" % (oL.shape, I.shape, Q.shape))
    p = _params(mode, params)
    b0, b1 = RxChain.CAL_BINS[("tx", mode)] if bins is None else bins
    rx = RxChain(ga.size, p, device=device)
    try:
        rx.set_calibration(True, spectrumZoom, currentScale, pixel_offset, b0, b1, capture_bins)
        res, _, _ = rx.ProcessIQData2_rx(I, Q, update=_update_mask(frames))
    finally:
        rx.close()
    return best_candidate(res, amps, phases)
