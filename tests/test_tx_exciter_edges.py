"""The transmit exciter at its edges.  Every FIR of tx_kernel sums its taps in the oracle's order without contraction,
and the kernel keeps denormals like the CPU, so the q15 outputs must equal the oracle's bit for bit:
every GPU test here asserts equality, at channel counts around a wave, frames per call, every mode, both branches of
the IQ phase correction, both rails, impulses around a frame boundary (with the independent float64 stream model of
test_tx_exciter.py as a second witness), split and long streams, parameter changes, resets, a large batch, a side
stream, and the C ABI's refusals and error messages."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from test_tx_exciter import stream_model
from tx_harness import F, assert_same, dev, mic, run

USB, LSB, AM, NFM, SAM = O.DEMOD_USB, O.DEMOD_LSB, O.DEMOD_AM, O.DEMOD_NFM, O.DEMOD_SAM
ERR_ARG, OK = -1, 0


# ---- inputs (q15, [nch, nfr * 2048])
def tones(nch, nfr, seed=5, level=0.02):
    """three speech-band tones per channel at ~0.02 full scale: the output sits mid-range and crosses many
    truncation boundaries"""
    rng = np.random.default_rng(seed)
    n = np.arange(nfr * F)
    x = np.zeros((nch, nfr * F))
    for c in range(nch):
        for _ in range(3):
            x[c] += np.sin(2 * np.pi * rng.uniform(300, 2800) / 192000.0 * n + rng.uniform(0, 6.28))
    x *= level / np.abs(x).max()
    return np.round(x * 32768.0).astype(np.int16)


def noise(nch, nfr, seed=7):
    """uniform full-range int16"""
    return np.random.default_rng(seed).integers(-32768, 32768, (nch, nfr * F)).astype(np.int16)


def neg_full(nch, nfr):
    return np.full((nch, nfr * F), -32768, np.int16)


def pos_full(nch, nfr):
    return np.full((nch, nfr * F), 32767, np.int16)


def nyquist(nch, nfr):
    x = np.full((nch, nfr * F), 32767, np.int16)
    x[:, 1::2] = -32767
    return x


INPUTS = {
    "tones": tones,
    "mic09": lambda nch, nfr: mic(nch, nfr, seed=3, level=0.9),
    "noise": noise,
    "neg": neg_full,
    "pos": pos_full,
    "nyq": nyquist,
    "zero": lambda nch, nfr: np.zeros((nch, nfr * F), np.int16),
}


# ---- GPU helpers
def params(mode, amp=1.0, phase=0.0):
    import t41_sdr_amd as T
    return T.default_tx_params(mode=mode, IQXAmpCorrectionFactor=amp, IQXPhaseCorrectionFactor=phase)


def chain(nch, mode=USB, amp=1.0, phase=0.0):
    import t41_sdr_amd as T
    return T.TxChain(nch, params(mode, amp, phase))


def oracle(q, mode=USB, amp=1.0, phase=0.0):
    return O.TxOracleBatch(q.shape[0], mode, amp, phase).process(q)


# ---- A. bit-exact parity: every value of every axis appears in some row
#      (channels, frames per call, mode, amp, phase, input)
ROWS = [
    (1, 1, USB, 1.0, 0.0, "tones"),
    (2, 2, LSB, 0.97, -0.02, "mic09"),
    (63, 7, USB, 1.03, 0.015, "noise"),   # white: the 10 kHz low-pass keeps it at about half scale, off both rails
    (64, 2, LSB, 0.0, 0.0, "mic09"),      # an exactly-zero amplitude factor: I is (signed) zero throughout
    (65, 1, USB, -1.0, 0.0, "nyq"),
    (2, 7, LSB, 1.0, 1.0, "neg"),         # phase >= 0 branch of IQPhaseCorrection at its extreme
    (1, 2, USB, 1.0, -1.0, "tones"),      # phase < 0 branch
    (64, 7, AM, 0.9, 0.3, "mic09"),       # AM / NFM / SAM: the correction is off (Exciter.cpp:117-127)
    (65, 2, NFM, 1.2, -0.4, "noise"),
    (63, 1, SAM, 0.5, 0.7, "tones"),
    (2, 1, USB, 1.0, 0.0, "zero"),
    (1, 7, LSB, 0.97, -0.02, "nyq"),
    (63, 2, SAM, 1.0, 0.0, "neg"),
    (64, 1, LSB, 1.0, 1.0, "pos"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("nch,nfr,mode,amp,phase,inp", ROWS,
                         ids=["%dch-%dfr-m%d-%g,%g-%s" % r for r in ROWS])
def test_gpu_tx_bit_exact(built, nch, nfr, mode, amp, phase, inp):
    q = INPUTS[inp](nch, nfr)
    got = run(chain(nch, mode, amp, phase), q)
    assert_same(got, oracle(q, mode, amp, phase))
    if mode not in (USB, LSB):  # the factors must not reach the output in these modes
        assert_same(got, run(chain(nch, mode), q), "mode %d with (%g, %g) vs (1, 0)" % (mode, amp, phase))
    if inp == "zero":
        assert not got[0].any() and not got[1].any()
    if inp == "mic09":  # the clamp at both rails, on both outputs unless the amplitude factor silences I
        for o in (got[1],) if amp == 0.0 else got:
            assert (o == 32767).any() and (o == -32768).any()
    # a full-scale constant reaches one rail only, the one of its sign (the low-pass passes DC, the Hilbert pair does
    # not block it); "neg" and "pos" together pin both rails on a DC input, "mic09" on speech
    if inp == "neg":
        assert (got[1] == -32768).any() and not (got[1] == 32767).any()
    if inp == "pos":
        assert (got[1] == 32767).any() and not (got[1] == -32768).any()
    if inp == "noise":
        assert np.abs(got[0].astype(np.int32)).max() < 32767 and np.abs(got[1].astype(np.int32)).max() < 32767
    if amp == 0.0:
        assert not got[0].any()


# ---- B. impulses straddling a frame boundary vs the float64 model and the oracle
TAPS = dict(dec1=48, dec2=24, hil=100, int1=48, int2=32)


def support(p):
    """first and last output sample (192 kS/s) an input impulse at sample p can reach, from the tap counts and the
    rates: /4 output m reads x[4m - 47 .. 4m], /2 output k reads y[2k - 23 .. 2k], the Hilbert output n reads
    z[n - 99 .. n], the x2 / x4 polyphase outputs of input n read inputs n - 23 .. n / n - 7 .. n.  An outer bound:
    the cascade's tails fall below one LSB and truncate to zero, so for an 8192 impulse the first nonzero output
    comes about 170 samples after it and the last about 280 before its end.  The zero checks against it only catch
    gross leaks; shifts of a few samples are caught by the float64 model and the oracle."""
    m0, m1 = -(-p // 4), (p + TAPS["dec1"] - 1) // 4
    k0, k1 = -(-m0 // 2), (m1 + TAPS["dec2"] - 1) // 2
    h0, h1 = k0, k1 + TAPS["hil"] - 1
    a0, a1 = 2 * h0, 2 * (h1 + TAPS["int1"] // 2 - 1) + 1
    return 4 * a0, 4 * (a1 + TAPS["int2"] // 4 - 1) + 3


@pytest.mark.gpu
@pytest.mark.parametrize("mode,amp,phase", [(USB, 1.0, 0.0), (LSB, 0.97, -0.02)], ids=["usb", "lsb-corr"])
def test_gpu_tx_impulses_around_frame_boundaries(built, mode, amp, phase):
    nfr = 4
    pos = [F * k + r for k in (1, 2) for r in range(-9, 9)]  # every phase mod 8 of /4 /2, both sides of the roll
    q = np.zeros((len(pos), nfr * F), np.int16)
    q[np.arange(len(pos)), pos] = 8192
    got = run(chain(len(pos), mode, amp, phase), q)
    assert_same(got, oracle(q, mode, amp, phase), "impulses")
    ob = O.TxOracleBatch(1)
    tabs = [ob.table(i) for i in range(4)]
    for c, p in enumerate(pos):
        lo, hi = support(p)
        assert hi < nfr * F - 1000, (p, hi)  # the whole response is inside the call, with silence behind it
        model = stream_model(q[c], mode, amp, phase, tabs)
        for o, m, side in ((got[0][c], model[0], "I"), (got[1][c], model[1], "Q")):
            assert not o[:lo].any(), (side, p, np.flatnonzero(o[:lo])[:4])           # nothing before the support
            assert not o[hi + 1:].any(), (side, p, hi + 1 + np.flatnonzero(o[hi + 1:])[:4])  # nor after it
            want = np.trunc(np.clip(m[lo:hi + 1] * 32768.0, -32768, 32767))
            d = np.abs(o[lo:hi + 1] - want)
            assert d.max() <= 2, (side, p, int(d.max()), lo + int(d.argmax()))
            assert np.abs(o).max() > 20, (side, p)  # the impulse got through


# ---- C. streaming state
@pytest.mark.gpu
def test_gpu_tx_uneven_splits(built):
    nch = 5
    q = mic(nch, 11, seed=21, level=0.7)
    whole8 = run(chain(nch, LSB, 0.97, -0.02), q[:, :8 * F])
    tx = chain(nch, LSB, 0.97, -0.02)
    parts = [run(tx, q[:, a * F:b * F]) for a, b in ((0, 1), (1, 3), (3, 8))]
    assert_same(tuple(np.concatenate([p[i] for p in parts], axis=1) for i in (0, 1)), whole8, "device 1+2+5 vs 8")
    # host entry 4, 1, 6 frames: staging allocated, reused, grown
    whole11 = run(chain(nch, LSB, 0.97, -0.02), q)
    tx = chain(nch, LSB, 0.97, -0.02)
    parts = [tx.ExciterIQData(np.ascontiguousarray(q[:, a * F:b * F])) for a, b in ((0, 4), (4, 5), (5, 11))]
    assert_same(tuple(np.concatenate([p[i] for p in parts], axis=1) for i in (0, 1)), whole11, "host 4+1+6 vs device 11")
    assert_same(whole11, oracle(q, LSB, 0.97, -0.02))


@pytest.mark.gpu
def test_gpu_tx_integration_one_channel_frame_by_frame(built):
    """one channel, one frame per host call"""
    q = mic(1, 16, seed=8, level=0.9)
    tx = chain(1)
    parts = [tx.ExciterIQData(np.ascontiguousarray(q[:, k * F:(k + 1) * F])) for k in range(16)]
    got = tuple(np.concatenate([p[i] for p in parts], axis=1) for i in (0, 1))
    assert_same(got, oracle(q))


@pytest.mark.gpu
def test_gpu_tx_long_stream(built):
    q = mic(3, 64, seed=12, level=0.5)
    assert_same(run(chain(3, USB, 1.03, 0.015), q), oracle(q, USB, 1.03, 0.015), "3 x 64 frames")


@pytest.mark.gpu
def test_gpu_tx_parameter_changes_keep_the_states(built):
    nch = 4
    q = mic(nch, 8, seed=14, level=0.6)
    steps = [((0, 2), dict(mode=USB, IQXAmpCorrectionFactor=1.0, IQXPhaseCorrectionFactor=0.0)),
             ((2, 4), dict(mode=LSB, IQXAmpCorrectionFactor=0.95, IQXPhaseCorrectionFactor=-0.03)),
             ((4, 5), dict(mode=AM)),
             ((5, 8), dict(mode=USB))]
    tx, ob = chain(nch), O.TxOracleBatch(nch)
    got, ref = [], []
    for (a, b), change in steps:
        tx.set_params(**change)
        for k, v in change.items():
            setattr(ob, {"mode": "mode", "IQXAmpCorrectionFactor": "amp", "IQXPhaseCorrectionFactor": "phase"}[k], v)
        got.append(run(tx, q[:, a * F:b * F]))
        ref.append(ob.process(q[:, a * F:b * F]))
    cat = lambda xs: tuple(np.concatenate([x[i] for x in xs], axis=1) for i in (0, 1))  # noqa: E731
    assert_same(cat(got), cat(ref), "USB -> LSB corr -> AM -> USB")
    # the states did carry: the same segments from cleared states differ
    fresh = run(chain(nch, LSB, 0.95, -0.03), q[:, 2 * F:4 * F])
    assert not np.array_equal(fresh[0], got[1][0])


@pytest.mark.gpu
def test_gpu_tx_reset_and_independent_contexts(built):
    nch = 6
    q = mic(nch, 6, seed=17, level=0.8)
    tx = chain(nch, LSB, 0.97, -0.02)
    run(tx, q[:, :3 * F])
    tx.reset()
    assert_same(run(tx, q[:, 3 * F:]), run(chain(nch, LSB, 0.97, -0.02), q[:, 3 * F:]), "after reset vs fresh")
    # two contexts, called alternately, frame by frame: each equals its own uninterrupted run
    qb = tones(nch, 6, seed=18, level=0.3)
    a, b = chain(nch, LSB, 0.97, -0.02), chain(nch, USB, 1.03, 0.015)
    ga, gb = [], []
    for k in range(6):
        ga.append(run(a, q[:, k * F:(k + 1) * F]))
        gb.append(run(b, qb[:, k * F:(k + 1) * F]))
    cat = lambda xs: tuple(np.concatenate([x[i] for x in xs], axis=1) for i in (0, 1))  # noqa: E731
    assert_same(cat(ga), run(chain(nch, LSB, 0.97, -0.02), q), "context A interleaved")
    assert_same(cat(gb), run(chain(nch, USB, 1.03, 0.015), qb), "context B interleaved")


# ---- D. batch and stream contract
@pytest.mark.gpu
def test_gpu_tx_large_batch(built):
    nch, nfr = 4096, 4
    rng = np.random.default_rng(30)
    q = (mic(nch, nfr, seed=31, level=1.0).astype(np.float64) * rng.uniform(0.05, 0.95, (nch, 1))).astype(np.int16)
    got = run(chain(nch, LSB, 0.97, -0.02), q)
    pick = np.unique(np.concatenate([[0, 1, 63, 64, 2047, 2048, 4094, 4095], rng.choice(nch, 56, replace=False)]))
    ref = oracle(q[pick], LSB, 0.97, -0.02)
    assert_same((got[0][pick], got[1][pick]), ref, "sampled channels of 4096")


@pytest.mark.gpu
def test_gpu_tx_channel_permutation(built):
    nch = 65
    q = mic(nch, 3, seed=33, level=0.9)
    perm = np.random.default_rng(34).permutation(nch)
    a = run(chain(nch), q)
    b = run(chain(nch), q[perm])
    assert_same(b, (a[0][perm], a[1][perm]), "permuted channels")


@pytest.mark.gpu
def test_gpu_tx_side_stream(built):
    import torch
    nch = 9
    q = mic(nch, 3, seed=40, level=0.9)
    base = dev(q)
    ref_tx = chain(nch, LSB, 0.97, -0.02)
    r1 = run(ref_tx, q)
    ref_tx.reset()
    r2 = run(ref_tx, q)
    tx = chain(nch, LSB, 0.97, -0.02)
    s = torch.cuda.Stream()
    outs = []
    for k in range(2):
        with torch.cuda.stream(s):
            x = torch.empty_like(base)
            x.copy_(base)  # the input is produced on s right before the call
            outs.append(tx.ExciterIQData(x))
        if k == 0:
            tx.reset()
    s.synchronize()
    assert_same(tuple(o.cpu().numpy() for o in outs[0]), r1, "side stream, first call")
    assert_same(tuple(o.cpu().numpy() for o in outs[1]), r2, "side stream, after reset")


@pytest.mark.gpu
def test_gpu_rx_side_stream(built):
    import torch
    import siggen
    import t41_sdr_amd as T
    nch, L = 8, 2048
    nco = siggen.nco_grid(nch, seed=42)
    I, Q = siggen.make_iq(nch, 2 * L, nco, mode=0, seed=43)
    dI, dQ = torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda()
    ref = T.RxChain(nch, T.default_params(), NCOFreq=nco)
    r = [ref.ProcessIQData(dI, dQ).cpu().numpy()]
    ref.reset()
    r.append(ref.ProcessIQData(dI, dQ).cpu().numpy())
    rx = T.RxChain(nch, T.default_params(), NCOFreq=nco)
    s = torch.cuda.Stream()
    outs = []
    for k in range(2):
        with torch.cuda.stream(s):
            x, y = torch.empty_like(dI), torch.empty_like(dQ)
            x.copy_(dI)
            y.copy_(dQ)
            outs.append(rx.ProcessIQData(x, y))
        if k == 0:
            rx.reset()
    s.synchronize()
    for o, want in zip(outs, r):
        assert np.array_equal(o.cpu().numpy(), want)


# ---- E. refusals, messages and the R queue
def _raw():
    from t41_sdr_amd import tx
    return tx._load()


def _rx_failure(lib):
    """an unrelated RX refusal that leaves a message no TX call uses"""
    import t41_sdr_amd as T
    ctx = C.c_void_p()
    assert lib.t41rx_create(C.byref(ctx), 0, 4, C.byref(T.default_params(fft_length=777))) == ERR_ARG
    assert lib.t41rx_last_error().decode() == "fft_length must be 512, 1024, 2048 or 4096"


def test_tx_refusals_report_their_own_message(built):
    """every refused t41tx_* call returns its code and leaves its own text in t41rx_last_error(), not what the
    last RX failure said (no device needed: the arguments are checked first)"""
    import t41_sdr_amd as T
    lib = _raw()
    ctx = C.c_void_p()
    dp = T.default_tx_params()
    cases = [
        ("create(out=NULL)", lambda: lib.t41tx_create(None, 0, 3, C.byref(dp)), "null argument"),
        ("create(params=NULL)", lambda: lib.t41tx_create(C.byref(ctx), 0, 3, None), "null argument"),
        ("create(n=0)", lambda: lib.t41tx_create(C.byref(ctx), 0, 0, C.byref(dp)), "n_channels must be > 0"),
        ("create(n=-1)", lambda: lib.t41tx_create(C.byref(ctx), 0, -1, C.byref(dp)), "n_channels must be > 0"),
    ]
    for mode in (4, 5, 7, 9, -1):
        bad = T.default_tx_params(mode=mode)
        cases.append(("create(mode=%d)" % mode, lambda bad=bad: lib.t41tx_create(C.byref(ctx), 0, 3, C.byref(bad)),
                      "mode must be USB, LSB, AM, NFM or SAM"))
    buf = (C.c_int16 * F)()
    cases += [
        ("set_params(NULL)", lambda: lib.t41tx_set_params(None, C.byref(dp)), "null argument"),
        ("reset(NULL)", lambda: lib.t41tx_reset(None), "null argument"),
        ("n_channels(NULL)", lambda: lib.t41tx_n_channels(None), "null argument"),
        ("process_device(NULL)", lambda: lib.t41tx_process_device_q15(None, buf, None, buf, buf, 1, None), "null argument"),
        ("process_host(NULL)", lambda: lib.t41tx_process_host_q15(None, buf, None, buf, buf, 1), "null argument"),
    ]
    for name, call, msg in cases:
        _rx_failure(lib)
        assert call() == ERR_ARG, name
        assert lib.t41rx_last_error().decode() == msg, name
    assert lib.t41tx_destroy(None) == OK
    # through the Python layer: the exception carries the TX text
    _rx_failure(lib)
    with pytest.raises(T.T41RxError, match="n_channels must be > 0") as e:
        T.TxChain(0)
    assert e.value.status == ERR_ARG
    _rx_failure(lib)
    with pytest.raises(T.T41RxError, match="mode must be USB, LSB, AM, NFM or SAM"):
        T.TxChain(3, T.default_tx_params(mode=5))


def test_python_mirrors_keep_their_params_when_refused(built):
    """TxChain.set_params / RxChain.CalcFilters assign the new fields only after the C side accepted them.  (A
    null context stands in for a live one here: the C side refuses without looking further, as it does for a bad
    field; the GPU test below does it on a live context.)"""
    import t41_sdr_amd as T
    tx = T.TxChain.__new__(T.TxChain)
    tx._lib, tx._ctx, tx.params = _raw(), C.c_void_p(), T.default_tx_params(mode=LSB, IQXPhaseCorrectionFactor=-0.02)
    with pytest.raises(T.T41RxError):
        tx.set_params(mode=AM, IQXAmpCorrectionFactor=0.5)
    assert (tx.params.mode, tx.params.IQXAmpCorrectionFactor) == (LSB, 1.0)
    with pytest.raises(AttributeError):
        tx.set_params(IQXAmpCorrectionFactor=0.5, nope=1)
    assert tx.params.IQXAmpCorrectionFactor == 1.0
    rx = T.RxChain.__new__(T.RxChain)
    rx._lib, rx._ctx, rx.params = _raw(), C.c_void_p(), T.default_params()
    before = bytes(rx.params)
    with pytest.raises(T.T41RxError):
        rx.CalcFilters(audioVolume=30, FHiCut=2500)
    assert bytes(rx.params) == before


@pytest.mark.gpu
def test_gpu_tx_device_entry_refusals(built):
    import torch
    import t41_sdr_amd as T
    lib = _raw()
    nch = 3
    tx = chain(nch)
    x = torch.zeros(nch, F, dtype=torch.int16, device="cuda")
    oL, oR = torch.empty_like(x), torch.empty_like(x)
    for n in (0, -1):
        _rx_failure(lib)
        assert lib.t41tx_process_device_q15(tx._ctx, x.data_ptr(), None, oL.data_ptr(), oR.data_ptr(), n, None) == ERR_ARG
        assert lib.t41rx_last_error().decode() == "n_frames must be > 0"
    for args in ((x.data_ptr(), None, None, oR.data_ptr()), (x.data_ptr(), None, oL.data_ptr(), None),
                 (None, None, oL.data_ptr(), oR.data_ptr())):
        _rx_failure(lib)
        assert lib.t41tx_process_device_q15(tx._ctx, *args, 1, None) == ERR_ARG
        assert lib.t41rx_last_error().decode() == "null argument"
    # contiguous, on the device, 2 bytes off a 16-byte boundary: refused before any launch
    odd = torch.zeros(nch * F + 1, dtype=torch.int16, device="cuda")[1:].view(nch, F)
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 2
    _rx_failure(lib)
    with pytest.raises(T.T41RxError, match="16-byte aligned") as e:
        tx.ExciterIQData(odd)
    assert e.value.status == ERR_ARG
    assert tx.n_channels == lib.t41tx_n_channels(tx._ctx) == nch
    # nothing ran: the states are still clear
    q = mic(nch, 2, seed=50, level=0.9)
    assert_same(run(tx, q), oracle(q))


@pytest.mark.gpu
def test_gpu_tx_r_queue_never_reaches_the_output(built):
    import torch
    lib = _raw()
    nch, nfr = 4, 3
    q = mic(nch, nfr, seed=51, level=0.9)
    r = mic(nch, nfr, seed=52, level=0.9)
    x, xr = dev(q), dev(r)
    outs = []
    for tx, rp in ((chain(nch), None), (chain(nch), xr.data_ptr())):
        oL, oR = torch.empty_like(x), torch.empty_like(x)
        stream = torch.cuda.current_stream().cuda_stream
        assert lib.t41tx_process_device_q15(tx._ctx, x.data_ptr(), rp, oL.data_ptr(), oR.data_ptr(), nfr,
                                            C.c_void_p(stream)) == OK
        torch.cuda.synchronize()
        outs.append((oL.cpu().numpy(), oR.cpu().numpy()))
    assert_same(outs[1], outs[0], "R queue given vs NULL")
    assert_same(outs[0], oracle(q))


@pytest.mark.gpu
def test_gpu_python_mirrors_after_a_refusal(built):
    import t41_sdr_amd as T
    nch = 3
    q = mic(nch, 4, seed=60, level=0.8)
    tx = chain(nch, LSB, 0.97, -0.02)
    a = run(tx, q[:, :2 * F])
    with pytest.raises(T.T41RxError, match="mode must be"):
        tx.set_params(mode=5)
    assert (tx.params.mode, tx.params.IQXPhaseCorrectionFactor) == (LSB, np.float32(-0.02))
    tx.set_params(IQXAmpCorrectionFactor=0.9)  # refused on main: the mirror still held mode 5
    b = run(tx, q[:, 2 * F:])
    ob = O.TxOracleBatch(nch, LSB, 0.97, -0.02)
    ra = ob.process(q[:, :2 * F])
    ob.amp = 0.9
    assert_same(a, ra)
    assert_same(b, ob.process(q[:, 2 * F:]), "LSB with the new amplitude")
    # the receive path's mirror
    rx = T.RxChain(2, T.default_params())
    with pytest.raises(T.T41RxError):
        rx.CalcFilters(audioVolume=30, AGCMode=9)
    assert bytes(rx.params) == bytes(rx.get_params())
    rx.CalcFilters(audioVolume=30)
    assert bytes(rx.params) == bytes(rx.get_params()) and rx.params.audioVolume == 30 and rx.params.AGCMode == 0
