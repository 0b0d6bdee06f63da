"""FT8 decode of a finished slot (ft8.cpp:270-616, 669-703, 727-790) as HIP kernels: ft8_sync_kernel and ft8_ldpc_kernel
against their restatement (tests/ft8_decode_model.py).

GPU (-m gpu): synthetic waterfalls uploaded directly (no receive chain) -- silence, clean and noisy transmissions at the
edges of the search, uniform noise with a full heap and ties at its minimum, the two fixed belief-propagation cases -- with
every 656-byte record, every plain byte and every log174 word (NaNs in the same places) the model's; the parameters, the
addressing, every refusal with nothing launched; one case through the receive chain on the device's own waterfall; and a
stream with decode calls in between that leaves the receive path as it was.  The CPU side is test_ft8_decode_model.py.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import ft8_codec as Cd
import ft8_decode_model as D
from test_ft8_decode_model import BP_FAIL_ERRORS, BP_FAIL_SEED, BP_SLOW_ITER, BP_SLOW_SEED, WHERE

L = 2048
TEXTS = ("W9XYZ K1ABC -12", "CQ K1ABC FN42", "K1ABC W9XYZ RR73")


def _payload(k):
    return (Cd.pack_standard("W9XYZ", "K1ABC", "-12"), Cd.pack_standard("CQ", "K1ABC", "FN42"), Cd.pack_standard("K1ABC", "W9XYZ", "RR73"))[k]


@functools.lru_cache(maxsize=None)
def _waterfalls():
    """the eight channels, [8][SLOT_BYTES] uint8, read only"""
    t0, _ = Cd.encode(_payload(0))
    t1, _ = Cd.encode(_payload(1))
    t2, _ = Cd.encode(_payload(2))
    rng = np.random.default_rng(0x465438)
    three = rng.integers(0, 20, (D.NUM_BLOCKS, 4, D.NUM_BINS)).astype(np.uint8)
    Cd.paint(three, t0, 0, 60, 0, 150, 40)
    Cd.paint(three, t1, 5, 150, 2, 110, 40)
    Cd.paint(three, t2, -3, 300, 3, 90, 40)
    w = [Cd.blank(0),
         Cd.paint(Cd.blank(0), t0, 3, 200, 1, 120, 40),
         three,
         Cd.paint(Cd.blank(0), t1, -7, 120, 3, 120, 40),
         Cd.paint(Cd.blank(0), t2, 19, 359, 1, 120, 40),
         rng.integers(0, 256, (D.NUM_BLOCKS, 4, D.NUM_BINS)).astype(np.uint8),
         Cd.noisy_transmission(BP_SLOW_SEED, t0),
         Cd.noisy_transmission(BP_FAIL_SEED, t0)]
    w = np.array(w).reshape(8, D.SLOT_BYTES)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def _model(max_candidates=20, min_score=40, ldpc_iterations=10):
    stats = [dict() for _ in range(8)]
    out = [D.decode(w, 0, max_candidates, min_score, ldpc_iterations, stats=s) for w, s in zip(_waterfalls(), stats)]
    res = np.array([o[0] for o in out], D.RESULT)
    log174, plain = np.array([o[1] for o in out]), np.array([o[2] for o in out])
    for a in (res, log174, plain):
        a.setflags(write=False)
    return res, log174, plain, stats


def _chain(T, n=8, **kw):
    rx = T.RxChain(n, T.default_params(mode=0, **kw))
    t = D.tables()
    rx.set_ft8_decode_tables(t.costas, t.gray, t.nm, t.mn, t.nrw)
    return rx


def _same(got, want, what=""):
    """records byte for byte, with the first differing field named"""
    got, want = np.asarray(got), np.asarray(want)
    if got.tobytes() != want.tobytes():
        for c in range(len(want)):
            for k in ("num_candidates", "num_valid", "select", "reserved"):
                assert got[c][k] == want[c][k], "%s channel %d %s: %r != %r" % (what, c, k, got[c][k], want[c][k])
            for i in range(20):
                for k in D.CAND.names:
                    assert np.array_equal(got[c]["cand"][i][k], want[c]["cand"][i][k]), "%s channel %d candidate %d %s: %r != %r" % (
                        what, c, i, k, got[c]["cand"][i][k], want[c]["cand"][i][k])
    assert got.tobytes() == want.tobytes()


def _same_log(got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "NaNs in other places"
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), "log174 differs from the model"


def _at(res, c, where):
    want = (where[0], where[1], where[2] // 2, where[2] % 2)
    hit = [x for x in res[c]["cand"][:int(res[c]["num_candidates"])]
           if (int(x["time_offset"]), int(x["freq_offset"]), int(x["time_sub"]), int(x["freq_sub"])) == want]
    assert len(hit) == 1, (c, where)
    return hit[0]


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_decode_equals_model():
    import torch
    import t41_sdr_amd as T
    want, wlog, wplain, stats = _model()
    # the cases are what they are meant to be (on the model)
    assert want[0]["num_candidates"] == 0 and want[1]["num_valid"] >= 1 and want[2]["num_valid"] >= 3
    assert _at(want, 3, (-7, 120, 3))["flags"] == 3 and _at(want, 4, (19, 359, 1))["flags"] == 3
    assert stats[5]["full"] and stats[5]["tie_at_minimum"] >= 1 and stats[5]["qualifying"] > 10000 and want[5]["num_valid"] == 0
    c6, c7 = _at(want, 6, WHERE), _at(want, 7, WHERE)
    assert (c6["n_errors"], c6["iterations"], c6["flags"]) == (0, BP_SLOW_ITER, 3)
    assert (c7["n_errors"], c7["iterations"], c7["flags"]) == (BP_FAIL_ERRORS, 10, 0)
    rx = _chain(T)
    assert rx.ft8_decode_params == (20, 40, 10)
    wf = torch.from_numpy(np.array(_waterfalls())).cuda()
    got, glog, gplain = rx.ft8_decode(waterfall=wf, debug=True)
    _same(got, want)
    assert np.array_equal(gplain, wplain), "plain differs from the model"
    _same_log(glog, wlog)
    texts = [[m["text"] for m in ch] for ch in T.ft8.messages(got)]
    assert texts[0] == [] and texts[1] == [TEXTS[0]] and set(texts[2]) == set(TEXTS) and texts[3] == [TEXTS[1]] and texts[4] == [TEXTS[2]]
    assert texts[5] == [] and texts[6] == [TEXTS[0]]
    # without the taps: the same records; the host entry point: the same
    _same(rx.ft8_decode(waterfall=wf), want)
    host = np.zeros(8, T.ft8.RESULT)
    T._lib.check(rx._lib.t41rx_ft8_decode_host(rx._ctx, C.c_void_p(wf.data_ptr()), D.SLOT_BYTES, None, 8, host.ctypes.data_as(C.c_void_p)))
    _same(host, want, "host entry")


@pytest.mark.gpu
@pytest.mark.parametrize("params", [(1, 40, 10), (7, 40, 10), (20, 40, 1), (20, 2000, 10), (3, 0, 10)])
def test_gpu_parameters(params):
    """max_candidates 1 and 7, ldpc_iterations 1, a min_score that leaves nothing; and min_score 0, where the silent
    channel's first three entries fill the heap and "decode" through NaN to the all-zero payload (the firmware's quirk)"""
    import torch
    import t41_sdr_amd as T
    want, wlog, wplain, _ = _model(*params)
    if params[1] == 2000:
        assert not want["num_candidates"].any()
    if params[1] == 0:
        assert want[0]["num_valid"] == 3 and np.isnan(wlog[0, :3]).all()
    rx = _chain(T)
    rx.set_ft8_decode(*params)
    assert rx.ft8_decode_params == params
    got, glog, gplain = rx.ft8_decode(waterfall=torch.from_numpy(np.array(_waterfalls())).cuda(), debug=True)
    _same(got, want)
    assert np.array_equal(gplain, wplain)
    _same_log(glog, wlog)


@pytest.mark.gpu
def test_gpu_addressing():
    """an explicit buffer whose channel stride is larger than two slots, with select 0 / 1 / -1 (the other slot holds
    another channel's waterfall), and the context's own d_power"""
    import torch
    import t41_sdr_amd as T
    want = _model()[0]
    w = _waterfalls()
    sel = np.array([0, 1, -1, 1, 0, -1, 1, 0], np.int8)
    two = np.zeros((8, 2, D.SLOT_BYTES), np.uint8)
    for c in range(8):
        two[c, max(int(sel[c]), 0)] = w[c]
        two[c, 1 - max(int(sel[c]), 0)] = w[(c + 3) % 8]
    expect = want.copy()
    for c in range(8):
        if sel[c] < 0:
            expect[c] = np.zeros((), D.RESULT)
        expect[c]["select"] = sel[c]
    rx = _chain(T)
    stride = 2 * D.SLOT_BYTES + 68
    buf = torch.full((8, stride), 0xEE, dtype=torch.uint8, device="cuda")
    buf[:, :2 * D.SLOT_BYTES] = torch.from_numpy(two.reshape(8, -1)).cuda()
    _same(rx.ft8_decode(select=sel, waterfall=buf), expect, "strided")
    view = buf[:, :2 * D.SLOT_BYTES]  # a view: its row stride is the buffer's
    assert view.stride(0) == stride
    _same(rx.ft8_decode(select=sel, waterfall=view), expect, "view")
    rx.set_ft8_tables()
    power, _ = rx.set_ft8(1, 1)
    power.copy_(torch.from_numpy(two).cuda())
    _same(rx.ft8_decode(select=sel), expect, "own d_power")
    zero = expect[2]
    assert zero["select"] == -1 and not zero["cand"].view(np.uint8).any() and zero["num_candidates"] == 0


@pytest.mark.gpu
def test_gpu_refusals():
    """each with T41RX_ERR_ARG, its message, and nothing launched: the result buffer keeps its sentinel"""
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd import _lib
    t = D.tables()
    rx = T.RxChain(8, T.default_params(mode=0))
    lib, ctx = rx._lib, rx._ctx
    wf = torch.from_numpy(np.array(_waterfalls())).cuda()
    res = torch.full((8, 656), 0xA5, dtype=torch.uint8, device="cuda")

    def refused(what, wfp=wf.data_ptr(), stride=D.SLOT_BYTES, select=None, n=8, out=res.data_ptr()):
        sp = None if select is None else np.asarray(select, np.int8).ctypes.data_as(C.c_void_p)
        rc = lib.t41rx_ft8_decode_device(ctx, C.c_void_p(wfp) if wfp else None, stride, sp, n, C.c_void_p(out) if out else None, None)
        msg = lib.t41rx_last_error().decode()
        assert rc == _lib.ERR_ARG and what in msg, (rc, msg)
        torch.cuda.synchronize()
        assert bool((res == 0xA5).all()), "something was launched: " + what

    refused("no tables loaded")

    def bad_tables(what, **change):
        arrs = dict(costas=t.costas.copy(), gray=t.gray.copy(), nm=t.nm.copy(), mn=t.mn.copy(), nrw=t.nrw.copy())
        for k, (idx, v) in change.items():
            arrs[k][idx] = v
        with pytest.raises(T.T41RxError) as e:
            rx.set_ft8_decode_tables(**arrs)
        assert e.value.status == _lib.ERR_ARG and what in str(e.value), str(e.value)

    bad_tables("kCostas_map entry outside 0..7", costas=(3, 8))
    bad_tables("kGray_map entry outside 0..7", gray=(7, 9))
    bad_tables("kNrw entry outside 1..7", nrw=(5, 0))
    bad_tables("kNrw entry outside 1..7", nrw=(82, 8))
    bad_tables("kNm entry outside 1..174", nm=((0, 0), 0))
    bad_tables("kNm entry outside 1..174", nm=((82, 5), 175))
    bad_tables("kMn entry outside 1..83", mn=((0, 0), 0))
    bad_tables("kMn entry outside 1..83", mn=((173, 2), 84))
    bad_tables("does not list its bit exactly once", mn=((0, 0), 2))      # check 2 does not hold bit 1
    bad_tables("does not list its bit exactly once", nm=((0, 1), 4))      # check 1 holds bit 4 twice
    bad_tables("does not list its check exactly once", nrw=(1, 7), nm=((1, 6), 1))  # check 2 names bit 1, which does not name it
    refused("no tables loaded")  # a refused table load wrote nothing
    rx.set_ft8_decode_tables(t.costas, t.gray, t.nm, t.mn, t.nrw)
    refused("n must equal n_channels", n=7)
    refused("d_results is NULL", out=0)
    refused("select must be -1 (skip), 0 or 1", select=[0, 0, 2, 0, 0, 0, 0, 0], stride=2 * D.SLOT_BYTES)
    refused("select must be -1 (skip), 0 or 1", select=[0, 0, 0, 0, 0, 0, 0, -2])
    refused("FT8 receive is off", wfp=0)
    refused("4-byte aligned", wfp=wf.data_ptr() + 1)
    refused("4-byte aligned", stride=D.SLOT_BYTES + 2)
    refused("smaller than the slots", stride=D.SLOT_BYTES - 4)
    refused("smaller than the slots", select=[1] * 8)
    for bad in ((0, 40, 10), (21, 40, 10), (20, 40, 0), (20, 40, 51)):
        with pytest.raises(T.T41RxError) as e:
            rx.set_ft8_decode(*bad)
        assert e.value.status == _lib.ERR_ARG and ("max_candidates must be 1..20" in str(e.value) or "ldpc_iterations must be 1..50" in str(e.value))
    assert rx.ft8_decode_params == (20, 40, 10)
    with pytest.raises(ValueError):
        rx.ft8_decode(select=[0] * 7, waterfall=wf)
    _same(rx.ft8_decode(waterfall=wf), _model()[0])  # and the context still decodes


def _iq_of(tones, nco, amp):
    """the transmission as USB I/Q @192 kS/s: audio tone f sits at 48000 - NCO - f (siggen.passband_tone_hz), 15 frames per
    symbol, continuous phase, from a frame boundary"""
    f = np.repeat(48000.0 - float(nco) - 6.25 * (160 + np.asarray(tones)), 15 * L)
    ph = 2 * np.pi * np.cumsum(f) / 192000.0
    return (amp * np.cos(ph)).astype(np.float32), (amp * np.sin(ph)).astype(np.float32)


@pytest.mark.gpu
def test_gpu_through_the_receive_chain():
    """2 channels, USB, FT8 on, one encoded message per channel as I/Q, 1380 frames: status word 2 names the finished half,
    ft8_decode(select = that half) equals the decode model on the downloaded waterfall, and messages() holds the text.
    The decode is checked against the device's own waterfall here; test_ft8_receive.py proves the waterfall."""
    import torch
    import t41_sdr_amd as T
    nco = np.array([-12000, 7350], np.int32)
    tones = [Cd.encode(_payload(k))[0] for k in (0, 1)]

    def chain(frames):
        rx = T.RxChain(2, T.default_params(mode=0), NCOFreq=nco)
        tap = torch.zeros(2, frames * 256, dtype=torch.float32, device="cuda")
        rx.set_debug_taps(demod=tap)
        return rx, tap

    def run(rx, amps, frames):
        iq = [_iq_of(tones[c][:frames // 15], nco[c], amps[c]) for c in range(2)]  # 79 symbols, then silence
        I = np.zeros((2, frames * L), np.float32)
        Q = np.zeros((2, frames * L), np.float32)
        for c in range(2):
            I[c, :iq[c][0].size], Q[c, :iq[c][1].size] = iq[c]
        rx.ProcessIQData(torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda())
        torch.cuda.synchronize()

    # the chain is linear with the AGC off: its gain is measured on 30 frames of the first symbols, then the level is set
    rx, tap = chain(30)
    run(rx, (0.1, 0.1), 30)
    gain = tap.view(2, -1)[:, 15 * 256:].abs().max(dim=1).values.cpu().numpy() / 0.1
    amps = 0.12 / gain
    print("chain gain", gain, "amplitudes", amps)
    assert (amps < 0.99).all()
    rx.close()

    rx, tap = chain(1380)
    t = D.tables()
    rx.set_ft8_decode_tables(t.costas, t.gray, t.nm, t.mn, t.nrw)
    rx.set_ft8_tables()
    power, _ = rx.set_ft8(1, 1380)
    rx.ft8_sync()
    run(rx, amps, 1380)
    peak = tap.view(2, -1).abs().max(dim=1).values.cpu().numpy()
    print("demod tap peaks", peak)
    assert ((peak >= 0.10) & (peak <= 0.14)).all()
    st = rx.ft8_status(1380).cpu().numpy()
    for c in range(2):
        assert np.array_equal(np.nonzero(st[c, :, 2])[0], [1379]) and st[c, 1379, 2] == 1
    sel = st[:, 1379, 2] - 1
    got = rx.ft8_decode(select=sel)
    wf = power.cpu().numpy()
    want = D.decode_all([wf[c, sel[c]] for c in range(2)], select=sel)[0]
    _same(got, want)
    texts = [[m["text"] for m in ch] for ch in T.ft8.messages(got)]
    print(texts, got["num_valid"])
    assert TEXTS[0] in texts[0] and TEXTS[1] in texts[1]


@pytest.mark.gpu
def test_gpu_decode_only_reads():
    """the same stream of process calls with decode calls in between and without: audio, get_state(), the FT8 record, the
    status words and d_power are equal"""
    import t41_sdr_amd as T
    import test_ft8_receive as R
    nch, splits = 2, R.SPLITS
    nco, I, Q = R._iq(nch, sum(splits))
    t = D.tables()
    out = []
    for with_decode in (False, True):
        run = R.Run(T, nch, nco, max(splits))
        run.rx.set_ft8_decode_tables(t.costas, t.gray, t.nm, t.mn, t.nrw)
        run.rx.ft8_sync()
        f0, audio, status, decoded = 0, [], [], []
        for n in splits:
            a, _, st = run.process(I[:, f0 * L:(f0 + n) * L], Q[:, f0 * L:(f0 + n) * L])
            if with_decode:
                decoded.append(run.rx.ft8_decode(select=[0, 1], debug=bool(f0)))
            audio.append(a)
            status.append(st)
            f0 += n
        out.append((np.concatenate(audio, axis=1), np.concatenate(status, axis=1), run.rx.get_state(), run.rx.ft8_state(),
                    run.power.cpu().numpy()))
        if with_decode:
            assert len(decoded) == len(splits) and all(d.shape == (nch,) if not isinstance(d, tuple) else d[0].shape == (nch,) for d in decoded)
    for a, b in zip(*out):
        assert np.array_equal(a, b)
