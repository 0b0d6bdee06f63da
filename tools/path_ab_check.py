#!/usr/bin/env python3
"""GPU box: the receive path of the product against another build of the library (t41_sdr_amd/abl/libt41rx_NAME.so), bit for
bit: outputs and checkpoints of the same streams, two calls each (1 frame, then the rest), one process per library --
SSB, LSB with IQ correction and band gain (the non-PLAIN kernels), NFM both ways, AM, SAM, each with the AGC off and on,
q15 samples, FFT_LENGTH 4096 / 1024, the time-major layout; then the side outputs and the exciters: the display spectrum at
zoom 0 / 2 / 4 (spec, spec_old, checkpoint), the calibration receive kernel at zoom 0 / 2 with per-channel candidates and an
unflagged frame (f32 and q15: result, pixel, spec), the SSB exciter with the equaliser off and on, the keyed CW exciter
and the calibration exciter (outputs and checkpoint).  Round 5 uses it to show that the same-result switches of
rx_device.hpp (addresses, phases, start values, lane writes, register tails) really are that.
usage: python tools/path_ab_check.py NAME"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import hashlib, json, os, sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
import t41_sdr_amd as T
import siggen
out = {}
CASES = [("usb", dict(mode=0, FLoCut=200, FHiCut=3000), 70, 9),
         ("lsb-iqcorr", dict(mode=1, FLoCut=-3000, FHiCut=-200, IQAmpCorrectionFactor=1.07, IQPhaseCorrectionFactor=0.03, RFgain=6), 33, 7),
         ("usb-agc", dict(mode=0, FLoCut=200, FHiCut=3000, AGCMode=2), 70, 9),
         ("nfm", dict(mode=3, FLoCut=-5000, FHiCut=5000), 40, 6),
         ("nfm-atan", dict(mode=3, FLoCut=-5000, FHiCut=5000, nfm_demod=1), 40, 6),
         ("am", dict(mode=2, FLoCut=-3000, FHiCut=3000), 40, 6),
         ("am-agc", dict(mode=2, FLoCut=-3000, FHiCut=3000, AGCMode=4), 40, 6),
         ("sam", dict(mode=8, FLoCut=-3000, FHiCut=3000), 20, 14),
         ("sam-agc", dict(mode=8, FLoCut=-3000, FHiCut=3000, AGCMode=1), 20, 14),
         ("fft4096", dict(mode=0, FLoCut=200, FHiCut=3000, fft_length=4096), 12, 16),
         ("fft1024-agc", dict(mode=0, FLoCut=200, FHiCut=3000, fft_length=1024, AGCMode=3), 12, 8)]
for name, kw, nch, nfr in CASES:
    try:
        p = T.default_params(**kw)
    except Exception as e:
        out[name] = "params: %%s" %% e
        continue
    nco = siggen.nco_grid(nch, seed=7)
    I, Q = siggen.make_iq(nch, nfr * 2048, nco, mode=min(kw["mode"], 3) if kw["mode"] != 8 else 2, seed=31)
    rx = T.RxChain(nch, p, NCOFreq=nco)
    h = hashlib.sha256()
    seg = p.fft_length // 512
    for sl in (slice(0, seg * 2048), slice(seg * 2048, nfr * 2048)):
        o = rx.ProcessIQData(torch.from_numpy(I[:, sl].copy()).cuda(), torch.from_numpy(Q[:, sl].copy()).cuda())
        h.update(o.cpu().numpy().tobytes())
    h.update(np.asarray(rx.get_state()).tobytes())
    out[name] = h.hexdigest()[:16]

# the side outputs and the exciters, whose tests compare within a tolerance or against a model: 3 channels x 3 frames in two
# calls (1 + 2) where the kernel streams; every buffer is hashed whole after every call
def digest(parts):
    h = hashlib.sha256()
    for t in parts:
        h.update(np.ascontiguousarray(t.cpu().numpy() if hasattr(t, "cpu") else t).tobytes())
    return h.hexdigest()[:16]
nch, nfr = 3, 3
calls = (slice(0, 2048), slice(2048, nfr * 2048))
nco = siggen.nco_grid(nch, seed=7)
I, Q = siggen.make_iq(nch, nfr * 2048, nco, mode=0, seed=31)
for zoom in (0, 2, 4):
    rx = T.RxChain(nch, T.default_params(mode=0, FLoCut=200, FHiCut=3000), NCOFreq=nco)
    spec = torch.zeros(nch, 2, 512, device="cuda")
    old = torch.zeros_like(spec)
    rx.set_display_spectrum(spec, old, zoom)
    parts = []
    for sl in calls:
        rx.ProcessIQData(torch.from_numpy(I[:, sl].copy()).cuda(), torch.from_numpy(Q[:, sl].copy()).cuda())
        torch.cuda.synchronize()
        parts += [spec.clone(), old.clone()]
    out["display-zoom%%d" %% zoom] = digest(parts + [np.asarray(rx.get_state())])
amps = (1.0 + 0.01 * np.arange(nch)).astype(np.float32)
phases = (0.005 * (np.arange(nch) - 1)).astype(np.float32)
update = np.array([1, 0, 1], np.uint8)  # one frame without updateDisplayFlag
scale = 0.25 / max(np.abs(I).max(), np.abs(Q).max())
for zoom, bins in ((0, (65, 192)), (2, (209, 273))):
    for q15 in (False, True):
        rx = T.RxChain(nch, T.default_params(mode=T.DEMOD_USB))
        rx.set_calibration(True, zoom, 1, 0, bins[0], bins[1], 10)
        rx.set_cal_corrections(amps, phases)
        conv = (lambda x: np.round(x * scale * 32768.0).astype(np.int16)) if q15 else (lambda x: (x * scale).astype(np.float32))
        parts = []
        for sl in calls:
            res, pix, sp = rx.ProcessIQData2_rx(torch.from_numpy(conv(I[:, sl])).cuda(), torch.from_numpy(conv(Q[:, sl])).cuda(),
                                                update=update[sl.start // 2048:sl.stop // 2048], pixel=True, spec=True)
            torch.cuda.synchronize()
            parts += [res, pix, sp]
        out["cal-rx-zoom%%d-%%s" %% (zoom, "q15" if q15 else "f32")] = digest(parts)
t = np.arange(nfr * 2048) / 192000.0
mic = np.round(0.4 * 32767 * np.sin(2 * np.pi * (400.0 + 700.0 * np.arange(nch))[:, None] * t)).astype(np.int16)
txp = dict(mode=T.DEMOD_LSB, IQXAmpCorrectionFactor=1.03, IQXPhaseCorrectionFactor=-0.02)
for eq in (0, 1):
    tx = T.TxChain(nch, T.default_tx_params(**txp))
    if eq:
        tx.set_transmit_eq_bands(np.load(os.path.join(%r, "golden", "eq", "rx_eq_bands.npz"))["coeffs_f32"])
        tx.set_transmit_eq(1)
    parts = list(tx.ExciterIQData(torch.from_numpy(mic).cuda()))
    torch.cuda.synchronize()
    out["tx-ssb-eq%%d" %% eq] = digest(parts + [tx.get_state()])
tx = T.TxChain(nch, T.default_tx_params(**txp))
tx.set_cw_tone(*T.sine_tone(8))
key = (np.random.default_rng(5).random((nch, nfr * 16)) < 0.6).astype(np.uint8)
out["tx-cw-keyed"] = digest(list(tx.CW_ExciterIQData(nfr, key=key)) + [tx.get_state()])
tx = T.TxChain(nch, T.default_tx_params(**txp))
tx.set_cal_tone(*T.cal_tone(), 0.5)
tx.set_cal_corrections(amps, phases)
out["tx-cal"] = digest(list(tx.ProcessIQData2_tx(nfr)) + [tx.get_state()])
print(json.dumps(out))
'''


def run(lib):
    env = dict(os.environ)
    env.pop("T41RX_LIB", None)
    if lib:
        env["T41RX_LIB"] = os.path.join(ROOT, "t41_sdr_amd", "abl", "libt41rx_%s.so" % lib)
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests"))], env=env, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit(p.stderr[-3000:])
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def main():
    other = sys.argv[1]
    a, b = run(None), run(other)
    diff = sorted(k for k in a if a[k] != b.get(k))
    print(json.dumps({"product": a, other: b, "identical": not diff, "differ": diff}))
    raise SystemExit(0 if not diff else 1)


if __name__ == "__main__":
    main()
