"""t41rx_set_buffer_layout (ABI 5): the frames of a call as [n_frames][n_channels][frame_len] -- the buffers of
consecutive single-frame ProcessIQData() calls (float_buffer_L/R[2048] per channel, T41_SDR.ino:375-376) stacked as
they arrive -- instead of [n_channels][n_frames * frame_len].  Same arithmetic on the same samples: outputs and
checkpoints must match the channel-major call bit for bit, in every mode, sample format and kernel form; and against
the oracle like any other call.
"""
from functools import partial

import numpy as np
import pytest

import oracle_lib as O
import siggen
from group_harness import L, chain, side_outputs
from rx_harness import T, one_call, to_q15  # noqa: F401  (T: the loaded package, a fixture)


def test_layout_symbols_and_constants(built):
    """CPU: the header's two constants and both entry points are there (no device needed to bind them)"""
    import re
    import os
    import t41_sdr_amd
    lib = t41_sdr_amd.load()
    assert hasattr(lib, "t41rx_set_buffer_layout") and hasattr(lib, "t41rx_get_buffer_layout")
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "t41rx.h")).read()
    assert re.search(r"#define T41RX_LAYOUT_CHANNEL_MAJOR 0", hdr) and re.search(r"#define T41RX_LAYOUT_TIME_MAJOR 1", hdr)
    assert lib.t41rx_set_buffer_layout(None, 1) == -1 and lib.t41rx_get_buffer_layout(None) == -1  # T41RX_ERR_ARG


CASES = [
    ("usb", dict(mode=0, FLoCut=200, FHiCut=3000), 5),
    ("usb-gains", dict(mode=0, FLoCut=200, FHiCut=3000, rfGainAllBands=3, RFgain=2, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=0.01), 3),
    ("lsb", dict(mode=1, FLoCut=-3000, FHiCut=-200), 3),
    ("am", dict(mode=2, FLoCut=-4000, FHiCut=4000), 3),
    ("nfm", dict(mode=3, FLoCut=200, FHiCut=3000), 3),
    ("sam", dict(mode=8, FLoCut=-4000, FHiCut=4000), 4),
    ("usb-agc-short", dict(mode=0, FLoCut=200, FHiCut=3000, AGCMode=1), 3),   # barrier form (fewer than 4 frames)
    ("usb-agc-pipe", dict(mode=0, FLoCut=200, FHiCut=3000, AGCMode=2), 6),    # pipelined form
    ("am-agc-pipe", dict(mode=2, FLoCut=-4000, FHiCut=4000, AGCMode=3), 5),
    ("sam-pipe", dict(mode=8, FLoCut=-4000, FHiCut=4000), 6),
    ("notch", dict(mode=0, FLoCut=200, FHiCut=3000, ANR_notchOn=1), 3),
    # the kernel forms that compute their I / Q / out addresses from chan_stride / frame_stride and were not compared
    ("sam-agc-pipe", dict(mode=8, FLoCut=-4000, FHiCut=4000, AGCMode=1), 7),  # SAM behind the AGC: the PSA pipeline (kSkew 4)
    ("kim", dict(mode=0, FLoCut=200, FHiCut=3000, nrOptionSelect=1), 5),         # launch_back512 behind the stage kernels
    ("spectral", dict(mode=0, FLoCut=200, FHiCut=3000, nrOptionSelect=2), 12),   # (its first 19 half-blocks pass the audio through)
    ("spectral-agc", dict(mode=0, FLoCut=200, FHiCut=3000, nrOptionSelect=2, AGCMode=2), 12),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,nfr", CASES, ids=[c[0] for c in CASES])
def test_time_major_equals_channel_major(T, name, kw, nfr):
    nch = 37  # ragged last workgroup
    nco = siggen.nco_grid(nch, seed=3)
    I, Q = siggen.make_iq(nch, 2 * nfr * L, nco, mode=min(kw["mode"], 3) if kw["mode"] != 8 else 2, seed=21)
    (a, _), (b, _) = chain(T, kw, nco), chain(T, kw, nco, layout="time")
    for call in range(2):  # the second call continues from the state the first left
        sl = slice(call * nfr * L, (call + 1) * nfr * L)
        oa, ob = one_call(a, I[:, sl], Q[:, sl])[0], one_call(b, I[:, sl], Q[:, sl])[0]  # (b's is [nfr, nch, L]: one_call checks)
        assert np.array_equal(oa, ob), (name, call)
    assert np.array_equal(a.get_state(), b.get_state())


@pytest.mark.gpu
def test_time_major_q15_and_host_entry_points(T):
    kw = dict(mode=0, FLoCut=200, FHiCut=3000, AGCMode=1)
    nch, nfr = 19, 5
    nco = siggen.nco_grid(nch, seed=4)
    I, Q = siggen.make_iq(nch, nfr * L, nco, mode=0, seed=22)
    qi, qq = to_q15(I), to_q15(Q)
    (a, _), (b, _) = chain(T, kw, nco), chain(T, kw, nco, layout="time")
    oa, ob = one_call(a, qi, qq)[0], one_call(b, qi, qq)[0]
    assert oa.dtype == np.int16 and np.array_equal(oa, ob)
    # host pointers, f32
    (c, _), (d, _) = chain(T, kw, nco), chain(T, kw, nco, layout="time")
    assert np.array_equal(one_call(c, I, Q, host=True)[0], one_call(d, I, Q, host=True)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["f32", "q15"])
def test_time_major_side_outputs_and_taps(T, fmt):
    """the <DEBUG, WQ15> instantiations and the side-output kernels under the time-major layout -- the audio
    spectrum / S-meter words, the display FFT and the stage taps keep their [n_channels][n_frames][...] shapes whatever
    the call buffers' layout, and hold the same bits"""
    import torch
    kw = dict(mode=0, FLoCut=200, FHiCut=3000, AGCMode=1)
    nch, nfr = 21, 5
    nco = siggen.nco_grid(nch, seed=6)
    I, Q = siggen.make_iq(nch, nfr * L, nco, mode=0, seed=24)
    if fmt == "q15":
        I, Q = to_q15(I), to_q15(Q)
    outs = {}
    for layout in ("channel", "time"):
        rx, side = chain(T, kw, nco, layout=layout, setup=partial(side_outputs, nfr=nfr, taps=("dec", "demod"), nch=nch))
        o, _ = one_call(rx, I, Q)
        torch.cuda.synchronize()
        outs[layout] = [o] + [t.cpu().numpy() for t in side] + [rx.get_state()]  # audio, spect, mx, spec, old, dec, dem, state
    for a, b in zip(outs["channel"], outs["time"]):
        assert np.array_equal(a, b)
    assert np.abs(outs["time"][1]).max() > 0 and np.abs(outs["time"][3]).max() > 0 and np.abs(outs["time"][6]).max() > 0


@pytest.mark.gpu
def test_time_major_against_the_oracle(T):
    """not only equal to the other layout: the time-major call is checked against the oracle directly"""
    kw = dict(mode=0, FLoCut=200, FHiCut=3000)
    nch, nfr = 24, 6
    nco = siggen.nco_grid(nch, seed=5)
    I, Q = siggen.make_iq(nch, nfr * L, nco, mode=0, seed=23)
    got, _ = one_call(chain(T, kw, nco, layout="time")[0], I, Q)
    ref = O.OracleBatch(O.default_params(**kw), nco).process(I, Q)
    err = siggen.block_rel_err(got, ref, L)
    assert err.max() <= 1e-5, err.max()


@pytest.mark.gpu
def test_time_major_refused_for_the_long_fft(T):
    rx = T.RxChain(4, T.default_params(fft_length=4096, FLoCut=400, FHiCut=600))
    with pytest.raises(T.T41RxError) as e:
        rx.set_buffer_layout("time")
    assert e.value.status == -2  # T41RX_ERR_UNSUPPORTED
    assert rx._lib.t41rx_get_buffer_layout(rx._ctx) == 0
    rx.set_buffer_layout("channel")
    assert rx._lib.t41rx_set_buffer_layout(rx._ctx, 7) == -1  # T41RX_ERR_ARG: unknown layout
