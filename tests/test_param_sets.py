"""Receiver groups with parameter sets (t41rx_set_param_sets): the context's own t41rx_params are set 0, the extra sets
1..K and a table set_of_channel[n_channels] sit on top.  Channel c must be processed exactly as a context created with
set set_of_channel[c] processes it.  So the reference of set k is a PLAIN context of the same channel count created with
set k's parameters, given the same NCOFreq, inputs and sequence of calls; for the channels with set_of_channel == k the
audio rows and the channel's records of t41rx_get_state() must be np.array_equal -- no tolerance -- and the audio is not
all zero.  19 channels (ragged against the 16-wave and the 4-wave workgroups, so sets mix inside every workgroup), 3
sets in a non-monotone table with repeats, every set used, set 0 used by some channels.
"""
import ctypes as C
from functools import partial

import numpy as np
import pytest

import oracle_lib as O
import siggen
from group_harness import L, NCH, USB, chain, ft8_receive, ft8_results, panadapter, rows_equal, run, side_outputs
from group_harness import SET_OF as SETOF, STREAM_OF as MAP
from rx_harness import ERR_ARG, ERR_UNSUPPORTED, TOL, T, refused, streams  # noqa: F401  (TOL: the bound test_parity_vs_oracle applies; T: a fixture)

pytestmark = pytest.mark.gpu

MAXSETS = 64
assert SETOF.shape == (NCH,) and set(SETOF) == {0, 1, 2}


def group(T, base, extra, setof=SETOF, layout="channel", setup=None, smap=None):
    """(mixed context, its setup's tensors), [(plain context of set k, its tensors) for k = 0..K]: base = set 0 as keywords
    of default_params, extra = the sets 1..K as dicts of changes against it"""
    make = lambda kw, **sets: chain(T, kw, nch=len(setof), layout=layout, setup=setup, **sets)  # noqa: E731
    mixed = make(base, sets=extra, setof=setof)
    if smap is not None:
        mixed[0].set_input_map(smap)  # (behind the sets, as ever)
    return mixed, [make(dict(base, **e)) for e in [{}] + list(extra)]


def check_sets(T, base, extra, nfr, setof=SETOF, layout="channel", q15=False, setup=None, smap=None, calls=None, seed=5):
    """the mixed context against the per-set plain contexts: audio of every call, whatever `setup` returns (side-output
    tensors), and the channels' state records"""
    import torch
    (a, ka), refs = group(T, base, extra, setof, layout, setup, smap)
    nch, Lf = len(setof), a.frame_len
    rows = nch if smap is None else int(np.max(smap)) + 1
    I, Q = streams(rows, nfr * Lf, seed, q15)
    f0 = 0
    for n in (calls or [nfr]):
        sl = slice(f0 * Lf, (f0 + n) * Lf)
        got = run(a, I[:, sl], Q[:, sl])
        Ir, Qr = (I[:, sl], Q[:, sl]) if smap is None else (I[smap][:, sl], Q[smap][:, sl])
        outs = [run(b, Ir, Qr) for b, _ in refs]
        rows_equal(got, outs, setof, "audio of the call at frame %d" % f0)
        assert np.abs(got.astype(np.float64)).max(axis=1).min() > 0, "a channel's audio is all zero"
        if ka:
            torch.cuda.synchronize()
            for i, x in enumerate(ka):
                rows_equal(x.cpu().numpy(), [kb[i].cpu().numpy() for _, kb in refs], setof, "side output %d" % i)
        f0 += n
    rows_equal(a.state_records(), [b.state_records() for b, _ in refs], setof, "state records")
    assert a._lib.t41rx_state_bytes(a._ctx) == refs[0][0]._lib.t41rx_state_bytes(refs[0][0]._ctx)  # sets have no state
    return a, [b for b, _ in refs]


SSB3 = [dict(mode=1, FLoCut=-3000, FHiCut=-200), dict(mode=0, FLoCut=300, FHiCut=1000)]  # + LSB + a narrow USB


# ---- 1. SSB: mask, level, both signs -------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channel", "time"])
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_ssb_usb_lsb_narrow(T, layout, q15):
    check_sets(T, USB, SSB3, 5, layout=layout, q15=q15)


# ---- 2. / 3. / 4. AM, NFM, SAM ---------------------------------------------------------------------------------------------
def test_am_cutoffs_and_lowpass(T):
    check_sets(T, dict(mode=2, FLoCut=-4000, FHiCut=4000, am_lpf_f0=3000),
               [dict(FLoCut=-2500, FHiCut=2500, am_lpf_f0=2000), dict(FLoCut=-4000, FHiCut=4000, am_lpf_f0=4500)], 5)


@pytest.mark.parametrize("nfm_demod", [0, 1], ids=["quadri", "atan"])
def test_nfm_filter_bandwidths(T, nfm_demod):
    check_sets(T, dict(mode=3, FLoCut=200, FHiCut=3000, nfmFilterBW=12000, nfm_demod=nfm_demod),
               [dict(nfmFilterBW=8000), dict(nfmFilterBW=16000, FHiCut=2400)], 5)


def test_sam_pipelined(T):
    check_sets(T, dict(mode=8, FLoCut=-4000, FHiCut=4000), [dict(FLoCut=-2500, FHiCut=2500), dict(FLoCut=-3000, FHiCut=3500, audioVolume=45)], 6)


# ---- 5. AGC: the serial chain runs on a wave that does not own the channel ----------------------------------------------
AGC3 = [dict(AGCMode=3, AGC_thresh=35, mode=1, FLoCut=-2800, FHiCut=-100), dict(AGCMode=4, AGC_thresh=5, FHiCut=2400)]


@pytest.mark.parametrize("nfr", [3, 6], ids=["barrier", "pipelined"])
def test_agc_modes_and_thresholds(T, nfr):
    check_sets(T, dict(AGCMode=1, AGC_thresh=20, **USB), AGC3, nfr)


def test_agc_am_pipelined(T):
    check_sets(T, dict(mode=2, FLoCut=-4000, FHiCut=4000, AGCMode=2),
               [dict(AGCMode=1, AGC_thresh=30, am_lpf_f0=2000), dict(AGCMode=4, FLoCut=-2500, FHiCut=2500)], 6)


@pytest.mark.parametrize("nfr", [3, 8], ids=["barrier", "psa"])
def test_sam_behind_the_agc(T, nfr):
    check_sets(T, dict(mode=8, FLoCut=-4000, FHiCut=4000, AGCMode=1),
               [dict(AGCMode=3, AGC_thresh=35, FLoCut=-2500, FHiCut=2500), dict(AGCMode=4, AGC_thresh=5)], nfr)


# ---- 6. gains --------------------------------------------------------------------------------------------------------------
def test_gains_general_class(T):
    base = dict(rfGainAllBands=3, RFgain=2, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=0.01, **USB)
    extra = [dict(rfGainAllBands=-4, RFgain=3, IQAmpCorrectionFactor=0.97, IQPhaseCorrectionFactor=-0.02),
             dict(rfGainAllBands=8, RFgain=1, IQAmpCorrectionFactor=1.0, IQPhaseCorrectionFactor=0.03, mode=1, FLoCut=-3000, FHiCut=-200)]
    check_sets(T, base, extra, 5)
    check_sets(T, base, extra, 5, q15=True, layout="time")


def test_gains_plain_class(T):
    check_sets(T, dict(rfGainAllBands=1, **USB), [dict(rfGainAllBands=7), dict(rfGainAllBands=-5)], 5)


# ---- 7. degenerate tables --------------------------------------------------------------------------------------------------
def test_one_channel_on_the_last_set(T):
    check_sets(T, USB, SSB3, 5, setof=np.array([2], np.int32))


def test_all_channels_on_one_extra_set(T):
    check_sets(T, USB, SSB3[:1], 5, setof=np.ones(NCH, np.int32))


def test_copies_of_set_0(T):
    """K identical copies of set 0, the cap's worth: whatever set a channel names, it runs as the plain context does"""
    k = MAXSETS - 1
    setof = ((np.arange(NCH) * 7) % (k + 1)).astype(np.int32)
    (a, _), refs = group(T, USB, [{}] * k, setof)
    I, Q = streams(NCH, 5 * L, 6)
    got, ref = run(a, I, Q), run(refs[0][0], I, Q)
    assert np.array_equal(got, ref) and np.abs(got).max(axis=1).min() > 0
    assert np.array_equal(a.get_state(), refs[0][0].get_state())
    assert len(a.param_sets) == k and np.array_equal(a.set_of_channel, setof)


# ---- 8. with an input map ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["channel", "time"])
def test_sets_with_an_input_map(T, layout):
    check_sets(T, USB, SSB3, 5, smap=MAP, layout=layout)
    check_sets(T, dict(AGCMode=1, **USB), AGC3, 6, smap=MAP, layout=layout)


# ---- 9. streaming -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,extra", [(USB, SSB3), (dict(AGCMode=2, **USB), AGC3)], ids=["usb", "usb-agc"])
def test_split_calls_equal_one_call(T, base, extra):
    a, _ = check_sets(T, base, extra, 7)
    b, _ = check_sets(T, base, extra, 7, calls=[1, 2, 4])
    assert np.array_equal(a.get_state(), b.get_state())


def test_sets_change_takes_effect_from_the_next_call(T):
    """a new table (and new sets) between two calls: the state is left alone, and the next call runs every channel as
    a plain context of its NEW set does from the mixed context's checkpoint"""
    other = ((SETOF + 1) % 3).astype(np.int32)
    kws = [dict(USB, **e) for e in [{}] + SSB3]
    nco = siggen.nco_grid(NCH, seed=11)
    (a, _), _ = group(T, USB, SSB3)
    I, Q = streams(NCH, 6 * L, 12)
    for k, table in enumerate((SETOF, other, SETOF)):
        before = a.get_state()
        a.set_param_sets(SSB3, table)
        assert np.array_equal(a.get_state(), before) and np.array_equal(a.set_of_channel, table)
        sl = slice(2 * k * L, 2 * (k + 1) * L)
        got = run(a, I[:, sl], Q[:, sl])
        outs, recs = [], []
        for kw in kws:
            p = T.RxChain(NCH, T.default_params(**kw), NCOFreq=nco)
            p.set_state(before)
            outs.append(run(p, I[:, sl], Q[:, sl]))
            recs.append(p.state_records())
        rows_equal(got, outs, table, "audio of call %d" % k)
        rows_equal(a.state_records(), recs, table, "state records behind call %d" % k)
        assert np.abs(got).max(axis=1).min() > 0


# ---- 10. configuration, not state ---------------------------------------------------------------------------------------------
def test_sets_survive_reset_checkpoint_and_set_params(T):
    (a, _), refs = group(T, USB, SSB3)
    I, Q = streams(NCH, 8 * L, 13)

    def step(k):
        sl = slice(2 * k * L, 2 * (k + 1) * L)
        rows_equal(run(a, I[:, sl], Q[:, sl]), [run(b, I[:, sl], Q[:, sl]) for b, _ in refs], SETOF, "audio of step %d" % k)
        assert np.array_equal(a.set_of_channel, SETOF) and len(a.param_sets) == 2
        assert a.param_sets[0].mode == 1 and a.param_sets[1].FHiCut == 1000

    step(0)
    a.reset()
    for b, _ in refs:
        b.reset()
    step(1)
    a.set_state(a.get_state())
    step(2)
    a.CalcFilters(FHiCut=2400, audioVolume=40)  # set 0 alone
    refs[0][0].CalcFilters(FHiCut=2400, audioVolume=40)
    a.set_coeffs(a.coeffs())
    step(3)
    rows_equal(a.state_records(), [b.state_records() for b, _ in refs], SETOF, "state records")


def test_checkpoint_with_sets_restores_without(T):
    base = dict(AGCMode=1, **USB)
    (a, _), refs = group(T, base, AGC3)
    I, Q = streams(NCH, 7 * L, 14)
    run(a, I[:, :3 * L], Q[:, :3 * L])
    ck = a.get_state()
    got = run(a, I[:, 3 * L:], Q[:, 3 * L:])
    outs = []
    for b, _ in refs:
        b.set_state(ck)
        assert b.set_of_channel is None and b.param_sets == []
        outs.append(run(b, I[:, 3 * L:], Q[:, 3 * L:]))
    rows_equal(got, outs, SETOF, "audio behind the restored checkpoint")
    rows_equal(a.state_records(), [b.state_records() for b, _ in refs], SETOF, "state records")


# ---- 11. what taps the fused chain --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
def test_side_outputs_and_taps(T, q15):
    nfr = 5
    a, _ = check_sets(T, dict(AGCMode=1, **USB), AGC3, nfr, q15=q15, setup=partial(side_outputs, nfr=nfr))
    assert all(float(t.abs().amax(dim=tuple(range(1, t.dim()))).min()) > 0 for t in (a._spect[0], a._taps[2]))  # written, every channel


def test_panadapter_rows(T):
    nfr = 3

    def setup(rx):
        bufs = panadapter(rx, nfr, spectrumZoom=1, currentScale=1, update_period=1)
        return tuple(bufs[name] for name, _, _ in rx.PANADAPTER_ROWS)

    check_sets(T, USB, SSB3, nfr, setup=setup)


def test_beacon_monitor_behind_the_panadapter(T):
    """the monitor reads the dBm of the panadapter's rows: a fast clock (a slot per frame) so that beacons change inside
    the call, three calls; the SNR table, the events and the monitor's record per set"""
    nfr = 4
    kept = []

    def setup(rx):
        sm = panadapter(rx, nfr, update_period=1, outputs=["smeter"])["smeter"]
        rx.set_panadapter_levels(gain_correction=np.linspace(-6.0, 6.0, NCH).astype(np.float32))
        rx.set_beacon_clock(0, 10000, 1)
        snr, ev = rx.set_beacon(True, 1, (np.arange(NCH) * 3 + 1) % 5)
        kept.append(rx)
        return sm, snr, ev

    check_sets(T, USB, SSB3, 3 * nfr, setup=setup, calls=[nfr, nfr, nfr])
    st = [rx.beacon_state()[32:].reshape(NCH, -1) for rx in kept]  # (behind the record's 8-word header: per channel)
    rows_equal(st[0], st[1:], SETOF, "the beacon monitor's record")
    assert kept[0]._beacon[1].cpu().numpy().any()  # the events of the last call were written


def test_ft8_receive_on_a_mixed_usb_context(T):
    nfr = 16
    extra = [dict(FLoCut=100, FHiCut=3200), dict(FLoCut=300, FHiCut=2700, audioVolume=50)]
    (a, _), refs = group(T, USB, extra)
    chains = [a] + [b for b, _ in refs]
    for rx in chains:
        ft8_receive(rx, nfr)
    I, Q = streams(NCH, nfr * L, 16)
    outs = [run(rx, I, Q) for rx in chains]
    rows_equal(outs[0], outs[1:], SETOF, "audio")
    st, pw = zip(*(ft8_results(rx, nfr) for rx in chains))
    rows_equal(st[0], st[1:], SETOF, "FT8 status")
    assert (st[0][:, -1, 0] == 1).all()
    rows_equal(pw[0], pw[1:], SETOF, "FT8 power")
    assert pw[0].reshape(NCH, -1).any(axis=1).all()
    # an LSB set cannot run under FT8 receive: the call is refused, nothing is processed
    a.set_param_sets(SSB3, SETOF)
    refused(lambda: run(a, I, Q), ERR_UNSUPPORTED, "FT8", "parameter set")


# ---- 12. host forms -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q15", [False, True], ids=["f32", "q15"])
@pytest.mark.parametrize("layout", ["channel", "time"])
def test_host_forms_equal_device_forms(T, layout, q15):
    (a, _), _ = group(T, USB, SSB3, layout=layout)
    (b, _), _ = group(T, USB, SSB3, layout=layout)
    I, Q = streams(NCH, 5 * L, 17, q15)
    dev, host = run(a, I, Q), run(b, I, Q, host=True)
    assert host.dtype == (np.int16 if q15 else np.float32) and np.array_equal(dev, host)
    assert np.array_equal(a.get_state(), b.get_state())


# ---- 13. against the oracle directly ------------------------------------------------------------------------------------------
def test_mixed_context_against_the_oracle(T):
    """each channel against oracle_lib run with the channel's own set, within the bound test_parity_vs_oracle applies"""
    nfr = 6
    nco = siggen.nco_grid(NCH, seed=3)
    kws = [dict(USB, **e) for e in [{}] + SSB3]
    I = np.empty((NCH, nfr * L), np.float32)
    Q = np.empty((NCH, nfr * L), np.float32)
    for k, kw in enumerate(kws):  # every channel gets a signal inside its own set's pass band
        Ik, Qk = siggen.make_iq(NCH, nfr * L, nco, mode=kw["mode"], seed=21, audio_hz=(400.0, 900.0))
        I[SETOF == k], Q[SETOF == k] = Ik[SETOF == k], Qk[SETOF == k]
    got = run(chain(T, USB, nco, sets=SSB3, setof=SETOF)[0], I, Q)
    assert np.isfinite(got).all()
    for k, kw in enumerate(kws):
        ref = O.OracleBatch(O.default_params(**kw), nco).process(I, Q)
        err = siggen.block_rel_err(got[SETOF == k], ref[SETOF == k], L)
        assert err.max() <= TOL, "set %d: worst block-relative error %.3e" % (k, err.max())


# ---- 14. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_previous_sets(T):
    (a, _), refs = group(T, USB, SSB3)
    lib = a._lib
    I, Q = streams(NCH, 2 * L, 18)
    ip = lambda m: np.ascontiguousarray(m, np.int32).ctypes.data_as(C.POINTER(C.c_int32))  # noqa: E731
    P = type(a.params)

    def arr(dicts):
        v = (P * max(len(dicts), 1))()
        for i, d in enumerate(dicts):
            v[i] = T.default_params(**dict(USB, **d))
        return v

    k = [0]

    def still_works():
        assert lib.t41rx_get_param_sets(a._ctx, None, 0, None, 0) == 2 and np.array_equal(a.set_of_channel, SETOF)
        rows_equal(run(a, I, Q), [run(b, I, Q) for b, _ in refs], SETOF, "audio behind refusal %d" % k[0])
        k[0] += 1

    def set_(dicts, table, n=None, n_sets=None):
        return lib.t41rx_set_param_sets(a._ctx, arr(dicts), len(dicts) if n_sets is None else n_sets, ip(table), len(table) if n is None else n)

    bad_arg = [
        ("n != n_channels", lambda: set_(SSB3, SETOF[:-1])),
        ("n != n_channels", lambda: set_(SSB3, np.append(SETOF, 0))),
        ("entry -1", lambda: set_(SSB3, np.where(np.arange(NCH) == 7, -1, SETOF))),
        ("entry n_sets + 1", lambda: set_(SSB3, np.where(np.arange(NCH) == NCH - 1, 3, SETOF))),
        ("n_sets over the cap", lambda: set_([{}] * MAXSETS, SETOF)),
        ("n_sets negative", lambda: set_(SSB3, SETOF, n_sets=-1)),
        ("an invalid set", lambda: set_([SSB3[0], dict(FLoCut=3000, FHiCut=200)], SETOF)),
        ("n_sets 0 with pointers", lambda: set_(SSB3, SETOF, n_sets=0)),
        ("null sets", lambda: lib.t41rx_set_param_sets(a._ctx, None, 2, ip(SETOF), NCH)),
        ("null context", lambda: lib.t41rx_set_param_sets(None, arr(SSB3), 2, ip(SETOF), NCH)),
        ("null context", lambda: lib.t41rx_get_param_sets(None, None, 0, None, 0)),
        ("cap too small", lambda: lib.t41rx_get_param_sets(a._ctx, arr(SSB3), 1, None, 0)),
    ]
    still_works()
    for what, call in bad_arg:
        assert call() == ERR_ARG, what
        assert lib.t41rx_last_error(), what
        still_works()
    # each incompatible pairing of the rule, against set 0 and through set_params / set_coeffs on set 0
    incompatible = [
        ("demodulators", dict(mode=2, FLoCut=-4000, FHiCut=4000)), ("demodulators", dict(mode=3)), ("demodulators", dict(mode=8, FLoCut=-4000, FHiCut=4000)),
        ("AGC", dict(AGCMode=2)), ("xmtMode", dict(xmtMode=1)), ("noise reduction", dict(nrOptionSelect=1)), ("noise reduction", dict(ANR_notchOn=1)),
        ("gains", dict(RFgain=2)), ("gains", dict(IQAmpCorrectionFactor=1.02)), ("gains", dict(IQPhaseCorrectionFactor=0.01)),
        ("fft_length", dict(fft_length=1024, FLoCut=400, FHiCut=600)),
    ]
    for word, change in incompatible:
        assert set_([SSB3[0], change], SETOF) == ERR_UNSUPPORTED, change
        assert word in lib.t41rx_last_error().decode() and "set 2 against set 0" in lib.t41rx_last_error().decode(), change
        still_works()
        if "fft_length" in change:
            continue  # (set_params refuses a change of fft_length on a live context as ever)
        refused(lambda: a.CalcFilters(**change), ERR_UNSUPPORTED, word, "new set 0")
        blob = T.design_coeffs(T.default_params(**dict(USB, **change)))
        refused(lambda: a.set_coeffs(blob), ERR_UNSUPPORTED, word, "new set 0")
        still_works()
    # NFM sets must agree in nfm_demod
    n = T.RxChain(NCH, T.default_params(mode=3, FLoCut=200, FHiCut=3000))
    refused(lambda: n.set_param_sets([dict(nfm_demod=1)], np.ones(NCH, np.int32)), ERR_UNSUPPORTED, "nfm_demod")
    assert n.param_sets == []
    # every chain-splitting stage, in both orders
    import cw_decode_model as DM
    import cw_model as CWM
    a.set_cw_tables(*CWM.tables())
    a.set_cw_decode_tree(DM.tree())
    a.set_receive_eq_bands(np.tile(np.array([1, 0, 0, 0, 0], np.float32), (14, 4)))
    stages = [("noise blanker", lambda on: a.set_noise_blanker(on)), ("receive equalizer", lambda on: a.set_receive_eq(on)),
              ("CW audio filter", lambda on: a.set_cw_filter(2 if on else 5)), ("CW detector", lambda on: a.set_cw_detector(on, 2)),
              ("CW decoder", lambda on: a.set_cw_decoder(on, 2))]
    for name, switch in stages:
        refused(lambda: switch(1), ERR_UNSUPPORTED, name, "parameter sets")
        still_works()
    a.set_param_sets(None)
    assert a.param_sets == [] and a.set_of_channel is None
    for name, switch in stages:
        switch(1)
        refused(lambda: a.set_param_sets(SSB3, SETOF), ERR_UNSUPPORTED, name, "parameter sets")
        assert a.param_sets == []
        switch(0)
    a.CalcFilters(nrOptionSelect=1)
    refused(lambda: a.set_param_sets(SSB3, SETOF), ERR_UNSUPPORTED, "noise reduction")
    a.CalcFilters(nrOptionSelect=0)
    a.set_param_sets(SSB3, SETOF)
    k[0] = 100
    still_works()
    # the long FFT lengths
    for n_fft in (1024, 2048, 4096):
        lng = T.RxChain(NCH, T.default_params(fft_length=n_fft, mode=0, FLoCut=400, FHiCut=600))
        refused(lambda: lng.set_param_sets([dict(FHiCut=700)], np.ones(NCH, np.int32)), ERR_UNSUPPORTED, "fft_length %d" % n_fft, "long-FFT")
        assert lng.param_sets == []
    # off again: every channel runs set 0
    a.set_param_sets(None)
    plain = T.RxChain(NCH, T.default_params(**USB), NCOFreq=siggen.nco_grid(NCH, seed=11))
    plain.set_state(a.get_state())  # (the channels that ran sets 1 and 2 carry those sets' filter histories)
    assert np.array_equal(run(a, I, Q), run(plain, I, Q))
    assert np.array_equal(a.get_state(), plain.get_state())
