"""Receiver groups (t41rx_set_input_map): channel c reads row map[c] of I / Q, which hold n_streams rows; audio, side
outputs, taps and state stay per channel.  The feature changes addresses only, so the reference of every case is the SAME
context configuration without a map, fed the replicated inputs I_rep[c] = I_streams[map[c]]: audio and t41rx_get_state()
bytes must be equal (np.array_equal, no tolerance).  19 channels (ragged against the 16-wave and the 4-wave workgroups),
3 streams, a map with repeats in a non-monotone order, distinct random samples per stream.
"""
import ctypes as C
from functools import partial

import numpy as np
import pytest

import oracle_lib as O
import siggen
from group_harness import L, NCH, NS, USB, chain, cw_receive, ft8_receive, ft8_results, run, side_outputs
from group_harness import STREAM_OF as MAP
from rx_harness import ERR_ARG, ERR_UNSUPPORTED, TOL, T, streams  # noqa: F401  (TOL: the bound test_parity_vs_oracle applies; T: a fixture)

pytestmark = pytest.mark.gpu


def pair(T, kw, smap=MAP, ns=None, layout="channel", setup=None):
    """(mapped context, reference context without a map), configured alike"""
    return tuple(chain(T, kw, nch=len(smap), layout=layout, setup=setup, imap=m, ns=ns) for m in (smap, None))


def check_equal(T, kw, nfr, layout="channel", q15=False, smap=MAP, ns=NS, seed=5, setup=None, calls=None):
    """mapped call(s) on [ns] rows against the unmapped call(s) on the replicated rows: audio, whatever `setup` returns
    to be compared (side-output tensors), and the state bytes"""
    import torch
    (a, ka), (b, kb) = pair(T, kw, smap=smap, ns=ns, layout=layout, setup=setup)
    Lf = a.frame_len
    I, Q = streams(ns, nfr * Lf, seed, q15)
    f0 = 0
    for n in (calls or [nfr]):
        sl = slice(f0 * Lf, (f0 + n) * Lf)
        got = run(a, I[:, sl], Q[:, sl])
        ref = run(b, I[smap][:, sl], Q[smap][:, sl])
        assert np.array_equal(got, ref), "audio differs in the call at frame %d" % f0
        assert np.abs(got.astype(np.float64)).max() > 0
        for x, y in zip(ka or (), kb or ()):
            torch.cuda.synchronize()
            assert torch.equal(x, y)
        f0 += n
    assert np.array_equal(a.get_state(), b.get_state())
    return a, b


# ---- 1. modes and shapes ------------------------------------------------------------------------------------------------
MODES = [
    ("usb-channel", USB, 5, "channel", False),
    ("usb-time", USB, 5, "time", False),      # input and output frame strides differ
    ("usb-q15-channel", USB, 5, "channel", True),
    ("usb-q15-time", USB, 5, "time", True),
    ("lsb", dict(mode=1, FLoCut=-3000, FHiCut=-200), 5, "channel", False),
    ("am", dict(mode=2, FLoCut=-4000, FHiCut=4000), 5, "channel", False),
    ("nfm", dict(mode=3, FLoCut=200, FHiCut=3000), 5, "time", False),
    ("nfm-atan", dict(mode=3, FLoCut=200, FHiCut=3000, nfm_demod=1), 5, "channel", False),
    ("sam", dict(mode=8, FLoCut=-4000, FHiCut=4000), 5, "time", False),
    ("usb-agc-barrier", dict(AGCMode=1, **USB), 3, "time", False),
    ("usb-agc-pipe", dict(AGCMode=1, **USB), 5, "time", False),
    ("usb-gains", dict(rfGainAllBands=3, RFgain=2, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=0.01, **USB), 5, "channel", False),
]


@pytest.mark.parametrize("name,kw,nfr,layout,q15", MODES, ids=[m[0] for m in MODES])
def test_mapped_equals_replicated(T, name, kw, nfr, layout, q15):
    check_equal(T, kw, nfr, layout=layout, q15=q15)


# ---- 2. map edge cases --------------------------------------------------------------------------------------------------
def test_one_stream_for_all_channels(T):
    check_equal(T, USB, 5, smap=np.zeros(NCH, np.int32), ns=1)


def test_permutation_is_read(T):
    """n_streams = n_channels with a random permutation: the outputs are permuted accordingly"""
    perm = np.random.default_rng(8).permutation(NCH).astype(np.int32)
    assert not np.array_equal(perm, np.arange(NCH))
    nco = np.full(NCH, 1500, np.int32)  # every channel tuned alike: the rows alone tell the outputs apart
    I, Q = streams(NCH, 5 * L, 9)
    a = T.RxChain(NCH, T.default_params(**USB), NCOFreq=nco)
    plain = run(a, I, Q)
    b = T.RxChain(NCH, T.default_params(**USB), NCOFreq=nco)
    b.set_input_map(perm)
    assert b.n_streams == NCH and np.array_equal(b.input_map, perm)
    got = run(b, I, Q)
    assert np.array_equal(got, plain[perm])
    assert not np.array_equal(got, plain)


def test_identity_map_equals_no_map(T):
    ident = np.arange(NCH, dtype=np.int32)
    for layout in ("channel", "time"):
        a, b = check_equal(T, USB, 5, layout=layout, smap=ident, ns=NCH)
        assert a.input_map is not None and b.input_map is None and b.n_streams == NCH


# ---- 3. streaming -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [USB, dict(AGCMode=2, **USB)], ids=["usb", "usb-agc"])
def test_split_calls_equal_one_call(T, kw):
    a, _ = check_equal(T, kw, 5)
    b, _ = check_equal(T, kw, 5, calls=[2, 3])
    assert np.array_equal(a.get_state(), b.get_state())
    I, Q = streams(NS, 5 * L, 5)
    (one, _), (two, _) = chain(T, kw, imap=MAP), chain(T, kw, imap=MAP)
    whole = run(one, I, Q)
    parts = np.concatenate([run(two, I[:, :2 * L], Q[:, :2 * L]), run(two, I[:, 2 * L:], Q[:, 2 * L:])], axis=1)
    assert np.array_equal(whole, parts)


def test_map_change_takes_effect_from_the_next_call(T):
    other = ((MAP + 1) % NS).astype(np.int32)
    (a, _), (b, _) = pair(T, USB)
    I, Q = streams(NS, 6 * L, 12)
    for k, m in enumerate((MAP, other, MAP)):
        a.set_input_map(m)
        sl = slice(2 * k * L, 2 * (k + 1) * L)
        assert np.array_equal(run(a, I[:, sl], Q[:, sl]), run(b, I[m][:, sl], Q[m][:, sl])), k
    assert np.array_equal(a.get_state(), b.get_state())


def test_map_survives_reset_checkpoint_and_set_params(T):
    (a, _), (b, _) = pair(T, USB)
    I, Q = streams(NS, 8 * L, 13)

    def step(k):
        sl = slice(2 * k * L, 2 * (k + 1) * L)
        assert np.array_equal(run(a, I[:, sl], Q[:, sl]), run(b, I[MAP][:, sl], Q[MAP][:, sl])), k
        assert np.array_equal(a.input_map, MAP) and a._lib.t41rx_get_input_map(a._ctx, None, 0) == NS

    step(0)
    nbytes = a._lib.t41rx_state_bytes(a._ctx)
    assert nbytes == b._lib.t41rx_state_bytes(b._ctx)  # streams have no state
    a.reset()
    b.reset()
    step(1)
    a.set_state(a.get_state())
    step(2)
    a.CalcFilters(FHiCut=2400, audioVolume=40)
    b.CalcFilters(FHiCut=2400, audioVolume=40)
    a.set_coeffs(a.coeffs())
    step(3)
    assert np.array_equal(a.get_state(), b.get_state())


def test_checkpoint_with_a_map_restores_without_one(T):
    """the map is not in the state: a checkpoint taken with the map on continues identically in a context with the map off"""
    kw = dict(AGCMode=1, **USB)
    (a, _), (b, _) = pair(T, kw)
    I, Q = streams(NS, 7 * L, 14)
    run(a, I[:, :3 * L], Q[:, :3 * L])
    ck = a.get_state()
    b.set_state(ck)
    assert b.input_map is None
    got = run(a, I[:, 3 * L:], Q[:, 3 * L:])
    ref = run(b, I[MAP][:, 3 * L:], Q[MAP][:, 3 * L:])
    assert np.array_equal(got, ref)
    assert np.array_equal(a.get_state(), b.get_state())


# ---- 4. paths behind the split ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_side_outputs_and_taps(T, q15):
    nfr = 5
    check_equal(T, dict(AGCMode=1, **USB), nfr, q15=q15, setup=partial(side_outputs, nfr=nfr))


def test_side_outputs_are_written(T):
    """(the equality above is not one of untouched zeros)"""
    import torch
    rx = T.RxChain(NCH, T.default_params(**USB), NCOFreq=siggen.nco_grid(NCH, seed=11))
    spect, mx, dem = torch.zeros(NCH, 2, 1024, device="cuda"), torch.zeros(NCH, 2, 3, device="cuda"), torch.zeros(NCH, 2 * 256, device="cuda")
    rx.set_audio_spectrum(spect, mx)
    rx.set_debug_taps(demod=dem)
    rx.set_input_map(MAP)
    I, Q = streams(NS, 2 * L, 15)
    run(rx, I, Q)
    assert all(float(t.abs().max()) > 0 for t in (spect, mx, dem))
    assert all(float(t.abs().amax(dim=tuple(range(1, t.dim()))).min()) > 0 for t in (spect, dem))  # every channel's rows


@pytest.mark.parametrize("name,kw,nb,q15", [("kim", dict(nrOptionSelect=1, **USB), 0, False), ("blanker", USB, 1, False),
                                            ("kim-q15-time", dict(nrOptionSelect=1, **USB), 0, True)],
                         ids=["kim", "blanker", "kim-q15"])
def test_stages_behind_the_demodulator(T, name, kw, nb, q15):
    """nrOptionSelect = 1 and the noise blanker: the aud_out split and launch_back512"""
    check_equal(T, kw, 5, layout="time" if q15 else "channel", q15=q15, setup=(lambda rx: rx.set_noise_blanker(1)) if nb else None)


def test_cw_detector_and_decoder(T):
    nfr = 6
    check_equal(T, dict(xmtMode=1, **USB), nfr, setup=partial(cw_receive, nfr=nfr))


def test_ft8_receive(T):
    nfr = 16
    (a, _), (b, _) = pair(T, USB)
    for rx in (a, b):
        ft8_receive(rx, nfr)
    I, Q = streams(NS, nfr * L, 16)
    assert np.array_equal(run(a, I, Q), run(b, I[MAP], Q[MAP]))
    (sa, pa), (sb, pb) = ft8_results(a, nfr), ft8_results(b, nfr)
    assert np.array_equal(sa, sb) and (sa[:, -1, 0] == 1).all()  # FT_8_counter: the 15 frames' two FFTs ran in the call
    assert np.array_equal(pa, pb) and pa.reshape(NCH, -1).any(axis=1).all()  # ... and left their rows
    assert np.array_equal(a.ft8_state(), b.ft8_state())
    assert np.array_equal(a.get_state(), b.get_state())


# ---- 5. long FFT --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg_run", [None, "1", "3"], ids=["default", "run1", "run3"])
@pytest.mark.parametrize("fft_length", [1024, 4096])
def test_long_fft(T, fft_length, seg_run, monkeypatch):
    """the segment-parallel front end with its pre-roll (explicit run lengths: a wave that starts inside the call reads the
    512 samples in front of its run from the mapped row) and, at 4096 without T41RX_SEG_RUN, the one-kernel form"""
    if seg_run is None:
        monkeypatch.delenv("T41RX_SEG_RUN", raising=False)
    else:
        monkeypatch.setenv("T41RX_SEG_RUN", seg_run)  # read when a call's arguments are made; set before the contexts exist
    kw = dict(fft_length=fft_length, mode=0, FLoCut=400, FHiCut=600)
    check_equal(T, kw, 3, calls=[2, 1])
    if seg_run is None:
        check_equal(T, dict(kw, mode=3, FLoCut=200, FHiCut=3000), 3)                    # NFM: the sequential front end
        check_equal(T, dict(kw, AGCMode=1), 3, q15=True)                                # q15 halving of the mapped base
        check_equal(T, dict(kw, RFgain=2, IQAmpCorrectionFactor=1.02), 3)               # the general (not PLAIN) kernels


def test_time_major_stays_refused_for_the_long_fft(T):
    rx = T.RxChain(NCH, T.default_params(fft_length=4096, FLoCut=400, FHiCut=600))
    rx.set_input_map(MAP)
    with pytest.raises(T.T41RxError) as e:
        rx.set_buffer_layout("time")
    assert e.value.status == ERR_UNSUPPORTED
    assert np.array_equal(rx.input_map, MAP)


# ---- 6. host forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("layout", ["channel", "time"])
def test_host_forms_equal_device_forms(T, layout, q15):
    (a, _), (b, _) = pair(T, USB, layout=layout)
    b.set_input_map(MAP)
    I, Q = streams(NS, 5 * L, 17, q15)
    dev = run(a, I, Q)
    host = run(b, I, Q, host=True)
    assert host.dtype == (np.int16 if q15 else np.float32) and np.array_equal(dev, host)
    assert np.array_equal(a.get_state(), b.get_state())


# ---- 7. against the oracle directly -------------------------------------------------------------------------------------
def test_mapped_call_against_the_oracle(T):
    """USB, default parameters: each channel's audio against oracle_lib run on that channel's own stream, within the bound
    test_parity_vs_oracle applies"""
    nfr = 6
    nco = siggen.nco_grid(NCH, seed=3)
    Ic, Qc = siggen.make_iq(NCH, nfr * L, nco, mode=0, seed=21)
    # stream s carries the signals of the channels tuned across it
    I = np.stack([Ic[MAP == s].mean(axis=0) for s in range(NS)]).astype(np.float32)
    Q = np.stack([Qc[MAP == s].mean(axis=0) for s in range(NS)]).astype(np.float32)
    got = run(chain(T, {}, nco, imap=MAP)[0], I, Q)
    ref = O.OracleBatch(O.default_params(), nco).process(I[MAP], Q[MAP])
    err = siggen.block_rel_err(got, ref, L)
    assert np.isfinite(got).all()
    assert err.max() <= TOL, "worst block-relative error %.3e at %s" % (err.max(), np.unravel_index(err.argmax(), err.shape))


# ---- 8. refusals --------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_map(T):
    import torch
    (a, _), (b, _) = pair(T, USB)
    lib = a._lib
    I, Q = streams(NS, 2 * L, 18)
    ip = lambda m: np.ascontiguousarray(m, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    k = [0]

    def still_works():
        assert lib.t41rx_get_input_map(a._ctx, None, 0) == NS and np.array_equal(a.input_map, MAP)
        assert np.array_equal(run(a, I, Q), run(b, I[MAP], Q[MAP])), k[0]
        k[0] += 1

    bad = [
        ("n != n_channels", lambda: lib.t41rx_set_input_map(a._ctx, ip(MAP[:-1]), NCH - 1, NS)),
        ("n != n_channels", lambda: lib.t41rx_set_input_map(a._ctx, ip(np.append(MAP, 0)), NCH + 1, NS)),
        ("n_streams 0 with a map", lambda: lib.t41rx_set_input_map(a._ctx, ip(MAP), NCH, 0)),
        ("n_streams above n_channels", lambda: lib.t41rx_set_input_map(a._ctx, ip(MAP), NCH, NCH + 1)),
        ("null map with n_streams", lambda: lib.t41rx_set_input_map(a._ctx, None, 0, 2)),
        ("entry -1", lambda: lib.t41rx_set_input_map(a._ctx, ip(np.where(np.arange(NCH) == 7, -1, MAP)), NCH, NS)),
        ("entry n_streams", lambda: lib.t41rx_set_input_map(a._ctx, ip(np.where(np.arange(NCH) == NCH - 1, NS, MAP)), NCH, NS)),
        ("null context", lambda: lib.t41rx_set_input_map(None, ip(MAP), NCH, NS)),
        ("null context", lambda: lib.t41rx_get_input_map(None, None, 0)),
    ]
    still_works()
    for what, call in bad:
        assert call() == ERR_ARG, what
        assert lib.t41rx_last_error(), what
        still_works()
    # the texts name both counts
    lib.t41rx_set_input_map(a._ctx, ip(MAP), NCH, NCH + 1)
    msg = lib.t41rx_last_error().decode()
    assert "n_channels %d" % NCH in msg and "n_streams %d" % (NCH + 1) in msg
    # Python: the wrapper raises what the C side refuses, and checks shapes against both counts
    with pytest.raises(T.T41RxError):
        a.set_input_map(np.where(np.arange(NCH) == 3, NS, MAP), NS)
    with pytest.raises(ValueError, match="n_channels=%d, n_streams=%d" % (NCH, NS)):
        a.ProcessIQData(torch.zeros(NCH, 2 * L, device="cuda"), torch.zeros(NCH, 2 * L, device="cuda"))  # one row per channel
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    with pytest.raises(ValueError, match="n_streams=%d" % NS):
        a.ProcessIQData(dI, dQ, out=torch.empty_like(dI))  # out= of the input's shape instead of the output's
    with pytest.raises(ValueError, match="n_streams=%d" % NS):
        a.ProcessIQData(I, Q, out=np.empty_like(I))
    out = torch.empty(NCH, 2 * L, device="cuda")
    assert a.ProcessIQData(dI, dQ, out=out) is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), run(b, I[MAP], Q[MAP]))
    still_works()
    # off again: one row per channel
    a.set_input_map(None)
    assert a.input_map is None and lib.t41rx_get_input_map(a._ctx, None, 0) == 0
    assert np.array_equal(run(a, I[MAP], Q[MAP]), run(b, I[MAP], Q[MAP]))
