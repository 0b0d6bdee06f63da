"""CW transmit: the CW exciter (CW_ExciterIQData(), CW_Excite.cpp:66-118) beside the SSB exciter, on its interpolators.
CPU: the f32 restatement tests/cw_tx_model.py against an independent float64 stream model, the properties that follow
from the frame's constant input and from the shared memories, the key on the model, the correction's signs, the C ABI's new
symbols and refusals, and sine_tone().
GPU: tx_cw_kernel against the restatement, bit for bit (the same IEEE operations in the same order, contraction off: the
standard tests/test_tx_equalizer.py holds the SSB exciter to) -- parity, streaming, the key, SSB and CW calls in turn,
more channels than CUs, changes in mid-stream, checkpoints, reset, the rails and refusals."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import cw_tx_model as W
import oracle_lib as O
import tx_model as M
from tx_harness import cat, mic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, K = 2048, 16
USB, LSB, AM = O.DEMOD_USB, O.DEMOD_LSB, O.DEMOD_AM
OK, ERR_ARG = 0, -1
CASES = {"usb": (USB, 1.0, 0.0), "lsb-corr": (LSB, 0.97, -0.02), "usb-corr": (USB, 1.03, 0.015), "am": (AM, 1.0, 0.3)}
NEW_SYMBOLS = ("t41tx_set_cw_tone", "t41tx_process_cw_device_q15", "t41tx_process_cw_host_q15")


def assert_same(got, ref, what=""):
    for g, r, side in ((got[0], ref[0], "I"), (got[1], ref[1], "Q")):
        assert g.shape == r.shape and g.dtype == r.dtype == np.int16, (what, side, g.shape, r.shape)
        if not np.array_equal(g, r):
            d = g.astype(np.int32) - r.astype(np.int32)
            bad = np.argwhere(d)
            raise AssertionError("%s %s: %d of %d samples differ (max |d| %d), first at [channel, sample] %s"
                                 % (what, side, len(bad), d.size, np.abs(d).max(), bad[0].tolist()))


@functools.lru_cache(maxsize=None)
def tone(num_cycles=8, scale=1.0):
    from t41_sdr_amd import tx
    c, s = tx.sine_tone(num_cycles)
    c, s = (c * np.float32(scale)).astype(np.float32), (s * np.float32(scale)).astype(np.float32)
    c.setflags(write=False)
    s.setflags(write=False)
    return c, s


@functools.lru_cache(maxsize=None)
def cold(case, num_cycles=8, nfr=4):
    """the model's first nfr frames from power-on, one channel, ungated: computed once, shared, never written to"""
    mode, amp, phase = CASES[case]
    out = W.CwTxModelBatch(1, mode, amp, phase, tone=tone(num_cycles)).process_cw(nfr)
    for a in out:
        a.setflags(write=False)
    return out


def rows(ref, nch, nfr=None):
    """a one-channel reference repeated over nch channels, its first nfr frames"""
    n = ref[0].shape[1] if nfr is None else nfr * F
    return tuple(np.repeat(r[:, :n], nch, axis=0) for r in ref)


# ---- CPU: the models
def test_model_matches_a_float64_stream_model():
    """The bound is measured between two CPU models, neither the code under test: over these 12 inputs the f32
    restatement deviates from the float64 stream model by at most 1 LSB on the q15 grid (the float chains agree to ~1e-6 of
    full scale, truncation adds one LSB), so twice that is 2 LSB -- the floor test_tx_equalizer.py uses, for the same
    reason.  Peaks lie at 10.6 k - 12.3 k LSB: nothing saturates."""
    bound = 2
    nfr = 4
    tabs = [O.TxOracleBatch(0).table(i) for i in range(4)]
    worst, peaks = 0, []
    for nc in (5, 8, 32):
        for case, (mode, amp, phase) in CASES.items():
            got = W.CwTxModelBatch(1, mode, amp, phase, tone=tone(nc)).process_cw(nfr)
            want = W.cw_stream_model_f64(*tone(nc), nfr, mode, amp, phase, tabs)
            for o, m in zip(got, want):
                w = np.trunc(np.clip(m * 32768.0, -32768, 32767))
                worst = max(worst, int(np.abs(o[0] - w).max()))
                peaks.append(int(np.abs(o[0].astype(np.int32)).max()))
    print("f32 restatement vs float64 stream model: max deviation %d LSB; peaks %d .. %d LSB" % (worst, min(peaks), max(peaks)))
    assert max(peaks) < 32767 and min(peaks) > 8000
    assert worst <= bound, worst


@pytest.mark.parametrize("case", list(CASES))
def test_model_frames_repeat_from_the_second_on(case):
    """the input is the same 256 samples every frame and both interpolators are FIRs: frame 0 starts from the zeroed
    memories, every later frame from memories that hold the tone"""
    oL, oR = cold(case)
    for o in (oL, oR):
        fr = o[0].reshape(4, F)
        assert not np.array_equal(fr[0], fr[1])
        assert np.array_equal(fr[1], fr[2]) and np.array_equal(fr[1], fr[3])


def test_model_ssb_and_cw_share_the_interpolator_memories():
    q = mic(1, 3, seed=2)
    # SSB frames before: the first CW frame is neither the cold one nor the steady one
    mo = W.CwTxModelBatch(1, tone=tone())
    mo.process(q[:, :2 * F])
    first = mo.process_cw(2)
    ref = cold("usb")
    nd = int((first[0][0, :F] != ref[0][0, :F]).sum())
    print("first CW frame after two SSB frames: %d of %d I samples differ from a cold start" % (nd, F))
    assert nd > 0 and not np.array_equal(first[1][:, :F], ref[1][:, :F])
    assert not np.array_equal(first[0][:, :F], ref[0][:, F:2 * F])
    assert_same((first[0][:, F:], first[1][:, F:]), (ref[0][:, F:2 * F], ref[1][:, F:2 * F]), "second CW frame: steady")
    # a CW frame before: the next SSB frame differs from the one of an exciter that sent no CW in between
    a, b = W.CwTxModelBatch(1, tone=tone()), W.CwTxModelBatch(1, tone=tone())
    a.process(q[:, :2 * F])
    b.process(q[:, :2 * F])
    a.process_cw(1)
    sa, sb = a.process(q[:, 2 * F:]), b.process(q[:, 2 * F:])
    assert not np.array_equal(sa[0], sb[0]) and not np.array_equal(sa[1], sb[1])
    # ... only through int1 / int2: the decimators', the Hilbert pair's and the equaliser's memories are untouched by CW
    for name in ("dec1", "dec2", "hil_l", "hil_r", "eq"):
        assert np.array_equal(getattr(a.chs[0], name), getattr(b.chs[0], name)), name


def random_key(nch, nfr, seed=11):
    """channel 0 all off, 1 all on, 2 a random 0 / 1 gate, 3 a 0 / 255 mix, the others any byte with about a third zeros"""
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 256, (nch, nfr * K)).astype(np.uint8)
    key[rng.random((nch, nfr * K)) < 0.35] = 0
    key[0] = 0
    key[1] = 1
    key[2] = rng.integers(0, 2, nfr * K)
    key[3] = 255 * rng.integers(0, 2, nfr * K)
    return key


def check_gate(got, ungated, key):
    on = np.repeat(key != 0, W.BLOCK, axis=1)
    for g, u in zip(got, ungated):
        assert not g[~on].any(), "a gated block is not zero"
        assert np.array_equal(g[on], u[on]), "a passed block differs from the ungated run"


def test_model_gate():
    nch, nfr = 5, 3
    key = random_key(nch, nfr)
    a, b = W.CwTxModelBatch(nch, LSB, 0.97, -0.02, tone=tone()), W.CwTxModelBatch(nch, LSB, 0.97, -0.02, tone=tone())
    got, ungated = a.process_cw(nfr, key), b.process_cw(nfr)
    check_gate(got, ungated, key)
    assert not got[0][0].any() and np.array_equal(got[0][1], ungated[0][1]) and got[0][2].any()
    # the memories advance whether a block is gated or not: channel 0 was gated throughout
    for x, y in zip(a.chs, b.chs):
        for k in (0, 1):
            assert np.array_equal(x.int1[k], y.int1[k]) and np.array_equal(x.int2[k], y.int2[k])
            assert x.int1[k].any() and x.int2[k].any()


def test_model_signs_are_the_opposite_of_the_ssb_exciters():
    """CW_Excite.cpp:79, 84 against Exciter.cpp:119, 124.  With amplitude 1 and phase 0 the correction is a bare sign
    on I, and a sign passes exactly through a FIR, x 20 and the truncating conversion"""
    am = cold("am", nfr=2)  # no correction: + cos
    neg = lambda x: (-x.astype(np.int32)).astype(np.int16)  # noqa: E731
    usb = W.CwTxModelBatch(1, USB, 1.0, 0.0, tone=tone()).process_cw(2)
    lsb = W.CwTxModelBatch(1, LSB, 1.0, 0.0, tone=tone()).process_cw(2)
    assert_same(usb, am, "CW USB: I times +1")
    assert_same(lsb, (neg(am[0]), am[1]), "CW LSB: I times -1")
    q = mic(1, 2, seed=3)
    s_am, s_usb, s_lsb = (M.TxModelBatch(1, m, 1.0, 0.0).process(q) for m in (AM, USB, LSB))
    assert_same(s_usb, (neg(s_am[0]), s_am[1]), "SSB USB: I times -1")
    assert_same(s_lsb, s_am, "SSB LSB: I times +1")
    assert am[0].any() and s_am[0].any()


def test_model_am_applies_no_correction():
    got = W.CwTxModelBatch(1, AM, 0.5, -0.4, tone=tone()).process_cw(2)
    assert_same(got, tuple(r[:, :2 * F] for r in cold("am")), "AM ignores the amplitude and phase factors")
    assert not np.array_equal(got[0], W.CwTxModelBatch(1, USB, 0.5, -0.4, tone=tone()).process_cw(2)[0])


def test_sine_tone():
    from t41_sdr_amd import tx
    c, s = tx.sine_tone(8)
    assert c.dtype == np.float32 and s.dtype == np.float32 and c.shape == (256,) and s.shape == (256,)
    theta = np.arange(256, dtype=np.float64) * 2.0 * np.pi * 750.0 / 24000.0
    assert np.array_equal(c, np.cos(theta).astype(np.float32)) and np.array_equal(s, np.sin(theta).astype(np.float32))
    assert abs(float(s[32])) < 1e-6 and abs(float(c[32]) - 1.0) < 1e-6  # one full period
    c0, s0 = tx.sine_tone()
    assert np.array_equal(c0, c) and np.array_equal(s0, s)  # numCycles = 8 is the firmware's
    # the firmware's frequency is an integer division: 5 cycles are 468 Hz, not 468.75
    c5, s5 = tx.sine_tone(5)
    assert np.array_equal(s5, np.sin(np.arange(256, dtype=np.float64) * 2.0 * np.pi * 468.0 / 24000.0).astype(np.float32))


# ---- CPU: the C ABI
def test_cw_exciter_abi_symbols_and_null_refusals(built):
    import t41_sdr_amd as T
    from t41_sdr_amd import tx
    raw_hdr = open(os.path.join(ROOT, "include", "t41tx.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", raw_hdr, flags=re.S)
    listed = set(re.findall(r"\b(t41tx_[a-z0-9_]+);", re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())))
    raw = C.CDLL(T.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert re.search(r"T41RX_API\s+int\s+%s\s*\(" % s, hdr), s
        assert s in listed and s in tx.TX_SYMBOLS and hasattr(raw, s), s
    for m in ("set_cw_tone", "CW_ExciterIQData"):
        assert callable(getattr(T.TxChain, m))
    assert callable(T.sine_tone)
    assert raw.t41rx_abi_version() == 5
    assert "Not restated: the data exciter" in raw_hdr and "CW and data exciters" not in raw_hdr
    # refusals that need no device: a NULL context, each entry with its own message
    lib = tx._load()
    c, s = tone()
    out = np.zeros(2 * F + 8, np.int16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cases = [
        ("set_cw_tone(NULL ctx)", lambda: lib.t41tx_set_cw_tone(None, p(c), p(s))),
        ("process_cw_device_q15(NULL ctx)", lambda: lib.t41tx_process_cw_device_q15(None, None, p(out), p(out), 1, None)),
        ("process_cw_host_q15(NULL ctx)", lambda: lib.t41tx_process_cw_host_q15(None, None, p(out), p(out), 1)),
    ]
    for name, call in cases:
        ctx = C.c_void_p()
        assert lib.t41rx_create(C.byref(ctx), 0, 4, C.byref(T.default_params(fft_length=777))) == ERR_ARG  # another message
        assert lib.t41rx_last_error().decode() != "null argument"
        assert call() == ERR_ARG, name
        assert lib.t41rx_last_error().decode() == "null argument", name
    assert not out.any()


# ---- GPU helpers
def cw_chain(nch, mode=USB, amp=1.0, phase=0.0, tn=None):
    import t41_sdr_amd as T
    tx = T.TxChain(nch, T.default_tx_params(mode=mode, IQXAmpCorrectionFactor=amp, IQXPhaseCorrectionFactor=phase))
    tx.set_cw_tone(*(tone() if tn is None else tn))
    return tx


def run_cw(tx, nfr, key=None, device=True):
    """one call; device=True: the device entry on the current stream, else the host entry.  numpy (I, Q)"""
    if not device:
        return tx.CW_ExciterIQData(nfr, key)
    import torch
    k = None if key is None else torch.from_numpy(np.ascontiguousarray(key)).cuda()
    oL, oR = tx.CW_ExciterIQData(nfr, k, device=True)
    torch.cuda.synchronize()
    assert oL.dtype == torch.int16 and oL.is_cuda and tuple(oL.shape) == (tx.n_channels, nfr * F)
    return oL.cpu().numpy(), oR.cpu().numpy()


def run_ssb(tx, q):
    import torch
    oL, oR = tx.ExciterIQData(torch.from_numpy(np.ascontiguousarray(q)).cuda())
    torch.cuda.synchronize()
    return oL.cpu().numpy(), oR.cpu().numpy()


def records(tx):
    return tx.get_state()[32:].view(np.float32).reshape(tx.n_channels, 448)


# ---- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("num_cycles", [8, 5])
@pytest.mark.parametrize("case", list(CASES))
def test_gpu_cw_parity(built, case, num_cycles):
    """3 channels x 1, 2 and 3 frames from power-on: the first frame alone, the first and the second (the last one
    computed), and a frame that repeats the second; through both entries"""
    mode, amp, phase = CASES[case]
    ref = cold(case, num_cycles)
    assert np.abs(ref[0]).max() > 8000 and np.abs(ref[1]).max() > 8000
    for nfr in (1, 2, 3):
        for device in (True, False):
            got = run_cw(cw_chain(3, mode, amp, phase, tone(num_cycles)), nfr, device=device)
            assert_same(got, rows(ref, 3, nfr), "%s, numCycles %d, %d frames, %s entry" % (case, num_cycles, nfr, "device" if device else "host"))


@pytest.mark.gpu
def test_gpu_cw_streaming(built):
    """4 frames in one call == 1 + 3 == 1 + 1 + 1 + 1, keyed: the memories' round trip through HBM and the key's offsets"""
    nch, nfr = 3, 4
    mode, amp, phase = CASES["lsb-corr"]
    key = random_key(5, nfr, seed=12)[2:]
    ref = tuple(W.gate(r, key) for r in rows(cold("lsb-corr"), nch))
    whole = run_cw(cw_chain(nch, mode, amp, phase), nfr, key)
    assert_same(whole, ref, "4 frames in one call")
    for split in ((1, 3), (1, 1, 1, 1)):
        tx, parts, f0 = cw_chain(nch, mode, amp, phase), [], 0
        for i, n in enumerate(split):
            parts.append(run_cw(tx, n, key[:, f0 * K:(f0 + n) * K], device=(i % 2 == 0)))
            f0 += n
        assert_same(cat(parts), whole, "+".join(map(str, split)))


@pytest.mark.gpu
def test_gpu_cw_gate(built):
    nch, nfr = 5, 3
    mode, amp, phase = CASES["usb-corr"]
    key = random_key(nch, nfr)
    assert not key[0].any() and key[1].all() and set(np.unique(key[3])) == {0, 255}
    a, b = cw_chain(nch, mode, amp, phase), cw_chain(nch, mode, amp, phase)
    ungated = run_cw(b, nfr)
    assert_same(ungated, rows(cold("usb-corr"), nch, nfr), "key = NULL")
    for device in (True, False):
        a.reset()
        got = run_cw(a, nfr, key, device=device)
        check_gate(got, ungated, key)
        assert not got[0][0].any() and not got[1][0].any() and np.array_equal(got[0][1], ungated[0][1])
        # the memories advanced under the gate as without it
        assert np.array_equal(a.get_state(), b.get_state())
    assert records(a)[:, 272:336].any()


@pytest.mark.gpu
def test_gpu_cw_and_ssb_share_the_interpolator_memories(built):
    """SSB (equaliser off) -> CW -> SSB (equaliser on) -> CW, every call against the model; a CW call changes the
    interpolators' part of the checkpoint and nothing else"""
    nch = 2
    q = mic(nch, 3, seed=7)
    key = random_key(5, 3, seed=13)[2:4]
    tx = cw_chain(nch, LSB, 0.97, -0.02)
    tx.set_transmit_eq_bands(M.bands())
    mo = W.CwTxModelBatch(nch, LSB, 0.97, -0.02, tone=tone(), levels=(100,) * 14)
    tx.set_transmit_eq(0, (100,) * 14)
    assert_same(run_ssb(tx, q[:, :2 * F]), mo.process(q[:, :2 * F]), "SSB, 2 frames, equaliser off")
    before = records(tx).copy()
    got = run_cw(tx, 2, key[:, :2 * K])
    assert_same(got, mo.process_cw(2, key[:, :2 * K]), "CW, 2 frames after SSB")
    after = records(tx)
    assert np.array_equal(before[:, :272].view(np.uint32), after[:, :272].view(np.uint32))   # decimators, Hilbert pair
    assert np.array_equal(before[:, 336:].view(np.uint32), after[:, 336:].view(np.uint32))   # equaliser
    assert not np.array_equal(before[:, 272:336], after[:, 272:336])
    tx.set_transmit_eq(1)
    mo.eq_on = True
    assert_same(run_ssb(tx, q[:, 2 * F:]), mo.process(q[:, 2 * F:]), "SSB, 1 frame after CW, equaliser on")
    before = records(tx).copy()
    assert before[:, 336:].any()
    assert_same(run_cw(tx, 1, key[:, 2 * K:]), mo.process_cw(1, key[:, 2 * K:]), "CW, 1 frame, the equaliser's switch on")
    after = records(tx)
    assert np.array_equal(before[:, :272].view(np.uint32), after[:, :272].view(np.uint32))
    assert np.array_equal(before[:, 336:].view(np.uint32), after[:, 336:].view(np.uint32))


@pytest.mark.gpu
def test_gpu_cw_more_channels_than_cus(built):
    nch, nfr = 300, 2
    got = run_cw(cw_chain(nch, *CASES["lsb-corr"]), nfr)
    for g in got:
        assert np.array_equal(g, np.repeat(g[:1], nch, axis=0)), "a row differs from row 0"
    assert_same(tuple(g[:1] for g in got), rows(cold("lsb-corr"), 1, nfr), "row 0")


@pytest.mark.gpu
def test_gpu_cw_changes_in_mid_stream(built):
    """USB -> LSB with the phase factor's sign flipped, then another tone table, between calls; the memories are kept"""
    nch = 3
    tx = cw_chain(nch, USB, 1.03, 0.015)
    mo = W.CwTxModelBatch(1, USB, 1.03, 0.015, tone=tone())
    got, ref = [run_cw(tx, 2)], [mo.process_cw(2)]
    tx.set_params(mode=LSB, IQXPhaseCorrectionFactor=-0.015)
    mo.mode, mo.phase = LSB, -0.015
    got.append(run_cw(tx, 2, device=False))
    ref.append(mo.process_cw(2))
    tx.set_cw_tone(*tone(5))
    mo.tone = tone(5)
    got.append(run_cw(tx, 2))
    ref.append(mo.process_cw(2))
    ref = rows(cat(ref), nch)
    assert_same(cat(got), ref, "USB, LSB with -phase, numCycles 5")
    for a, b in ((1, 2), (3, 4)):  # each change shows in the frame behind it
        assert not np.array_equal(ref[0][:, a * F:(a + 1) * F], ref[0][:, b * F:(b + 1) * F])


@pytest.mark.gpu
def test_gpu_cw_checkpoint(built):
    nch = 3
    mode, amp, phase = CASES["lsb-corr"]
    q = mic(nch, 1, seed=8)
    tx, mo = cw_chain(nch, mode, amp, phase), W.CwTxModelBatch(nch, mode, amp, phase, tone=tone())
    run_ssb(tx, q)
    mo.process(q)
    ck = tx.get_state()
    assert ck.size == 32 + 4 * 448 * nch and list(ck[:32].view(np.int32)[1:4]) == [5, nch, 448]
    ref = mo.process_cw(2)
    tx2 = cw_chain(nch, mode, amp, phase)
    tx2.set_state(ck)
    assert_same(run_cw(tx2, 2), ref, "SSB frame, checkpoint, 2 CW frames in a new context")
    assert_same(run_cw(tx, 2), ref, "the original context")
    assert not np.array_equal(ref[0][:, :F], rows(cold("lsb-corr"), nch, 1)[0])
    # between two CW calls
    ck = tx.get_state()
    tx3 = cw_chain(nch, mode, amp, phase)
    tx3.set_state(ck)
    assert_same(run_cw(tx3, 1, device=False), mo.process_cw(1), "2 CW frames, checkpoint, 1 CW frame in a new context")


@pytest.mark.gpu
def test_gpu_cw_reset_keeps_the_tone_table(built):
    nch = 3
    tx = cw_chain(nch, *CASES["usb-corr"], tn=tone(5))
    run_cw(tx, 2)
    tx.reset()
    assert not records(tx).any()
    assert_same(run_cw(tx, 2), rows(cold("usb-corr", 5), nch, 2), "after reset: a cold start on the same table")


@pytest.mark.gpu
def test_gpu_cw_rails(built):
    """a table of 4 cos / 4 sin: 0.127 x 4 x 20 is ten times full scale, arm_float_to_q15 saturates at both rails"""
    nch, nfr = 3, 2
    big = tone(8, 4.0)
    got = run_cw(cw_chain(nch, LSB, 0.97, -0.02, big), nfr)
    assert_same(got, rows(W.CwTxModelBatch(1, LSB, 0.97, -0.02, tone=big).process_cw(nfr), nch), "rails")
    for o in got:
        assert (o == 32767).any() and (o == -32768).any()


@pytest.mark.gpu
def test_gpu_cw_refusals_leave_the_context_usable(built):
    import torch
    import t41_sdr_amd as T
    nch = 3
    mode, amp, phase = CASES["usb-corr"]
    ref = rows(cold("usb-corr"), nch, 3)
    tx = T.TxChain(nch, T.default_tx_params(mode=mode, IQXAmpCorrectionFactor=amp, IQXPhaseCorrectionFactor=phase))
    lib = tx._lib
    # before a tone table, through both entries
    for device in (True, False):
        with pytest.raises(T.T41RxError, match="no tone table loaded") as e:
            tx.CW_ExciterIQData(1, device=device)
        assert e.value.status == ERR_ARG
    # a NaN in either table is refused and not kept
    for which in (0, 1):
        bad = [t.copy() for t in tone()]
        bad[which][255] = np.nan
        with pytest.raises(T.T41RxError, match="non-finite") as e:
            tx.set_cw_tone(*bad)
        assert e.value.status == ERR_ARG
    with pytest.raises(T.T41RxError, match="no tone table loaded"):
        tx.CW_ExciterIQData(1)
    with pytest.raises(ValueError):
        tx.set_cw_tone(np.zeros(255, np.float32), np.zeros(255, np.float32))
    assert lib.t41tx_set_cw_tone(tx._ctx, None, None) == ERR_ARG
    assert not records(tx).any()  # nothing ran
    tx.set_cw_tone(*tone())
    first = run_cw(tx, 1)
    # on a running exciter: a NaN table does not replace the good one; n_frames = 0; NULL and misaligned outputs
    bad = [t.copy() for t in tone()]
    bad[1][0] = np.inf
    with pytest.raises(T.T41RxError, match="non-finite"):
        tx.set_cw_tone(*bad)
    oL = torch.zeros((nch, 2 * F + 8), dtype=torch.int16, device="cuda")
    oR = torch.zeros_like(oL)
    hL, hR = np.zeros((nch, F), np.int16), np.zeros((nch, F), np.int16)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    refused = [
        ("n_frames must be > 0", lambda: lib.t41tx_process_cw_device_q15(tx._ctx, None, oL.data_ptr(), oR.data_ptr(), 0, stream)),
        ("n_frames must be > 0", lambda: lib.t41tx_process_cw_device_q15(tx._ctx, None, oL.data_ptr(), oR.data_ptr(), -1, stream)),
        ("n_frames must be > 0", lambda: lib.t41tx_process_cw_host_q15(tx._ctx, None, p(hL), p(hR), 0)),
        ("device pointers must be 16-byte aligned", lambda: lib.t41tx_process_cw_device_q15(tx._ctx, None, oL.data_ptr() + 2, oR.data_ptr(), 1, stream)),
        ("device pointers must be 16-byte aligned", lambda: lib.t41tx_process_cw_device_q15(tx._ctx, None, oL.data_ptr(), oR.data_ptr() + 8, 1, stream)),
        ("null argument", lambda: lib.t41tx_process_cw_device_q15(tx._ctx, None, None, oR.data_ptr(), 1, stream)),
        ("null argument", lambda: lib.t41tx_process_cw_host_q15(tx._ctx, None, p(hL), None, 1)),
    ]
    for text, call in refused:
        assert call() == ERR_ARG, text
        assert lib.t41rx_last_error().decode() == text
    with pytest.raises(ValueError):
        tx.CW_ExciterIQData(2, np.ones((nch, K), np.uint8))
    torch.cuda.synchronize()
    assert not oL.any() and not oR.any() and not hL.any()  # a refused call wrote nothing
    assert_same(cat([first, run_cw(tx, 2)]), ref, "the stream goes on unharmed, on the good table")
