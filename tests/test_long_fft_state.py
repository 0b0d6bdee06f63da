"""Checkpoints, resets and mid-stream changes of the receive path at fft_length 1024 / 2048 / 4096 (-m gpu).

At the long FFT lengths a channel record holds TWO copies of the oscillator state: the kernels of a call read copy
`nco_sel` and write the other one, and rx_host.cpp flips `nco_sel` after every process call.  t41rx_get_state() (which
writes the current copy into both slots), t41rx_set_state() and t41rx_reset() (which set nco_sel = 0) and every entry
point (which must flip it exactly once, and not at all when it refuses the call) have to agree with that flip.  So the
variable of every test here is CALL PARITY: "odd" / "even" = the number of process calls the context has made since it
was created, reset or restored.

  A  checkpoint / restore / reset of the path: continuation bit for bit from a checkpoint taken at either parity, in
     contexts of either parity; the checkpoint bytes do not depend on the parity; get_state() does not disturb the
     stream; each row's uninterrupted stream is itself held to the oracle.
  B  CalcFilters / SetNCOFreq / CW side tone / mode and AGC switches / t41rx_set_coeffs between two calls, after an
     odd and after an even number of calls, frame by frame against an OracleBatch that makes the same changes.
  C  one stream through the device-f32, host-f32, device-q15 and host-q15 entry points in turn, against one
     OracleBatch fed the same pieces, and against the same stream through device-f32 calls only.
  D  refused calls between the calls of a stream change nothing; the noise blanker's two carry slots (fft_length 512,
     `nb_sel` flips with every blanker launch) under the same parity cases as A.

Tolerances are the suite's: block-relative error against the oracle <= TOL (AM_TOL in AM: the note above
test_parity_am), the first frame at 4096 points compared absolutely (test_parity_fft4096), q15 samples by the rule of
test_gpu_q15_long_fft; "the same stream" is np.array_equal on samples and on checkpoint bytes.  Every frame compared
with the oracle must hold a signal (peak above 1e-3 of the stream's peak), so that no case passes on silence.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_lib as O
import siggen
from rx_harness import TOL, T, calls, one_call, to_q15  # noqa: F401  (T: the loaded package, a fixture)
from test_gpu_parity import AM_TOL
from test_noise_blanker import WIDE, clicky_iq

pytestmark = pytest.mark.gpu

USB = dict(mode=0, FLoCut=200, FHiCut=3000)
LSB = dict(mode=1, FLoCut=-3000, FHiCut=-200)
AM = dict(mode=2, FLoCut=-3000, FHiCut=3000)
NFM = dict(mode=3, FLoCut=200, FHiCut=3000)
FADE = [(0.4, 2.0), (0.25, 0.1), (0.35, 1.0)]  # the AGC attacks, decays and attacks again


# ---- helpers ---------------------------------------------------------------------------------------------------------
def signal(mode, nch, n, nco, seed, audio_hz=(500.0, 2400.0), fade=FADE):
    if mode == 3:
        I, Q = siggen.make_fm(nch, n, nco, seed=seed)
    else:
        I, Q = siggen.make_iq(nch, n, nco, mode=mode, seed=seed, audio_hz=audio_hz)
    return siggen.fade(I, Q, fade) if fade else (I, Q)


def cut(x, a, b, Lf):
    return np.ascontiguousarray(x[:, a * Lf:b * Lf])


def dev(rx, i, q):
    """one call through the device-pointer entry point"""
    return one_call(rx, i, q)[0]


def run(rx, I, Q, Lf, edges, between=None):
    """frames edges[k] .. edges[k + 1] per call; between(k) runs after call k (not after the last one)"""
    assert rx.frame_len == Lf
    after = None if between is None else lambda rx, a, b: b < edges[-1] and between(edges.index(a))
    return calls(rx, I, Q, edges, after=after)[0]


def check_vs_oracle(got, ref, N, tol, what):
    """block-relative error per frame against tol[frame]; frame 0 at 4096 points (filter start-up) absolutely.  Returns
    the worst error over tolerance's own scale (the block-relative figure)."""
    Lf = 4 * N
    assert np.isfinite(got).all() and np.isfinite(ref).all(), what
    tol = np.broadcast_to(np.asarray(tol, np.float64), (got.shape[1] // Lf,))
    err = siggen.block_rel_err(got, ref, Lf)
    peak = np.abs(ref).reshape(ref.shape[0], -1, Lf).max(axis=2)
    first = 0
    if N == 4096:
        assert np.abs(got[:, :Lf] - ref[:, :Lf]).max() <= 1e-5 * np.abs(ref).max(), what
        first = 1
    # the reference holds a signal in every compared frame
    assert (peak[:, first:] > 1e-3 * peak.max()).all(), (what, "silent reference frame", (peak / peak.max()).min(axis=0))
    worst = err[:, first:].max()
    print("%s: worst block-relative error %.3e" % (what, worst))
    bad = err[:, first:] > tol[first:]
    assert not bad.any(), (what, "worst %.3e" % worst, "channel, frame", np.argwhere(bad) + [0, first], err.max(axis=0))
    return worst


NCO = 200  # rx_internal.hpp kStNco: two oscillator states of four floats each


def records(ck, nch):
    """the path's per-channel records of a checkpoint, float32 [nch, floats] (a view)"""
    per = int(ck[:32].view(np.int32)[4])
    return ck[32:32 + 4 * per * nch].view(np.float32).reshape(nch, per)


def refused(T, fn):
    """the status a refused call answers (None if it was accepted)"""
    try:
        rc = fn()
    except T.T41RxError as e:
        return e.status
    return rc if isinstance(rc, int) and rc != 0 else None


# ---- A: checkpoint and reset of the path ---------------------------------------------------------------------------------
ROWS = {"usb": USB, "lsb-agc3": dict(LSB, AGCMode=3), "am-agc1": dict(AM, AGCMode=1), "nfm": NFM}
A_CASES = [(1024, "usb", 5), (2048, "lsb-agc3", 7), (4096, "am-agc1", 5), (2048, "nfm", 6), (4096, "usb", 7), (1024, "am-agc1", 9)]
A_IDS = ["%s-%d" % (name, N) for N, name, _ in A_CASES]
NFR, N1 = 5, 3  # x = x1 | x2: three frames (one call, or calls of 1 + 2 frames), then two
_A = {}


def a_case(T, N, name, nch):
    """the row's stream, its uninterrupted run (x1 in one call, x2 in one call) and the checkpoints after x1 at both
    parities"""
    key = (N, name)
    if key in _A:
        return _A[key]
    kw = dict(ROWS[name], fft_length=N)
    Lf = 4 * N
    nco = siggen.nco_grid(nch, seed=N + nch)
    assert (nco != 0).all()  # (at 0 Hz a stale oscillator copy equals the current one)
    I, Q = signal(kw["mode"], nch, NFR * Lf, nco, seed=N + 7)
    s = SimpleNamespace(kw=kw, N=N, Lf=Lf, nch=nch, nco=nco, I=I, Q=Q)
    s.new = lambda: T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
    s.x1 = lambda rx, calls: run(rx, I, Q, Lf, [0, N1] if calls == 1 else [0, 1, N1])
    s.x2 = lambda rx, calls=1: run(rx, I, Q, Lf, [N1, NFR] if calls == 1 else [N1, N1 + 1, NFR])
    ref = s.new()
    s.o1 = s.x1(ref, 1)
    s.ck = {1: ref.get_state()}
    s.o2 = s.x2(ref)
    s.final = ref.get_state()
    even = s.new()
    s.o1_even = s.x1(even, 2)
    s.ck[2] = even.get_state()
    _A[key] = s
    return s


@pytest.mark.parametrize("N,name,nch", A_CASES, ids=A_IDS)
def test_a5_uninterrupted_stream_matches_the_oracle(T, N, name, nch):
    """the anchor of the bit-for-bit comparisons below: the row's stream is within tolerance of the oracle's"""
    s = a_case(T, N, name, nch)
    ref = O.OracleBatch(O.default_params(**s.kw), s.nco).process(s.I, s.Q, nthreads=8)
    check_vs_oracle(np.concatenate([s.o1, s.o2], axis=1), ref, N, AM_TOL if s.kw["mode"] == 2 else TOL, "A.5 " + name + "-%d" % N)
    assert np.array_equal(s.o1, s.o1_even)


@pytest.mark.parametrize("N,name,nch", A_CASES, ids=A_IDS)
def test_a2_checkpoint_does_not_depend_on_call_parity(T, N, name, nch):
    """x1 in one call (odd: the current oscillator state sits in slot 1) and in two calls (even: in slot 0) leave the
    same checkpoint bytes: get_state() writes the CURRENT copy into both slots"""
    s = a_case(T, N, name, nch)
    a, b = s.ck[1], s.ck[2]
    assert a.size == b.size
    diff = np.flatnonzero(a != b)
    assert diff.size == 0, ("checkpoints differ at byte offsets (32-byte header, then %d floats per channel)" % (a[:32].view(np.int32)[4]), diff[:16])
    rec = records(a, nch)
    osc = lambda r: r[:, NCO:NCO + 8].copy().view(np.uint8).reshape(nch, 2, 16)  # noqa: E731  (bytes: phase words are not floats)
    assert np.array_equal(osc(rec)[:, 0], osc(rec)[:, 1])  # both oscillator slots hold the same state
    assert not np.array_equal(osc(rec), osc(records(s.final, nch)))  # (which moves with the stream)


@pytest.mark.parametrize("calls", [1, 2], ids=["ck-odd", "ck-even"])
@pytest.mark.parametrize("N,name,nch", A_CASES, ids=A_IDS)
def test_a1_continuation_from_a_checkpoint(T, N, name, nch, calls):
    """x2 after set_state(checkpoint behind x1) equals the uninterrupted stream's x2 bit for bit, wherever the
    checkpoint goes: the context it came from (which has moved on by one call: the other parity), a fresh context
    (even), a context that has made one call on other data (odd), and a fresh one that takes x2 in two calls"""
    s = a_case(T, N, name, nch)
    rx = s.new()
    assert np.array_equal(s.x1(rx, calls), s.o1)
    ck = rx.get_state()
    assert np.array_equal(rx.get_state(), ck)
    s.x2(rx)  # moves on: parity flips
    busy = s.new()
    dev(busy, cut(s.Q, 1, 2, s.Lf), cut(s.I, 1, 2, s.Lf))  # one call on other data
    for label, ctx, x2_calls in (("same context", rx, 1), ("fresh context", s.new(), 1), ("context after one call", busy, 1),
                                 ("fresh context, x2 in two calls", s.new(), 2)):
        ctx.set_state(ck)
        o2 = s.x2(ctx, x2_calls)
        bad = np.argwhere(np.any(o2.reshape(nch, -1, s.Lf) != s.o2.reshape(nch, -1, s.Lf), axis=2))
        assert bad.size == 0, (label, "x2 differs in (channel, frame)", bad[:8])
        assert np.array_equal(ctx.get_state(), s.final), label


@pytest.mark.parametrize("N,name,nch", A_CASES, ids=A_IDS)
def test_a3_get_state_does_not_disturb_the_stream(T, N, name, nch):
    s = a_case(T, N, name, nch)
    edges = [0, 1, N1, N1 + 1, NFR]
    rx = s.new()

    def look(k):
        a = rx.get_state()
        assert np.array_equal(a, rx.get_state()), "two consecutive get_state() calls differ after call %d" % k

    seen = run(rx, s.I, s.Q, s.Lf, edges, between=look)
    plain_rx = s.new()
    plain = run(plain_rx, s.I, s.Q, s.Lf, edges)
    assert np.array_equal(seen, plain)
    assert np.array_equal(plain, np.concatenate([s.o1, s.o2], axis=1))
    assert np.array_equal(rx.get_state(), plain_rx.get_state()) and np.array_equal(rx.get_state(), s.final)


@pytest.mark.parametrize("calls", [1, 2], ids=["after-odd", "after-even"])
@pytest.mark.parametrize("N,name,nch", A_CASES, ids=A_IDS)
def test_a4_reset_at_either_parity(T, N, name, nch, calls):
    """reset() after an odd and after an even number of calls, then x1: a fresh context's x1, samples and checkpoint"""
    s = a_case(T, N, name, nch)
    rx = s.new()
    s.x2(rx, calls)
    rx.reset()
    assert np.array_equal(rx.get_state(), s.new().get_state())
    assert np.array_equal(s.x1(rx, 1), s.o1)
    assert np.array_equal(rx.get_state(), s.ck[1])
    # and from a restored checkpoint: reset() does not depend on what set_state() left either
    rx.set_state(s.final)
    rx.reset()
    assert np.array_equal(s.x1(rx, 2), s.o1) and np.array_equal(rx.get_state(), s.ck[1])


# ---- B: control calls between two calls, against the oracle doing the same -----------------------------------------------
def play(T, N, kw0, nco0, I, Q, steps):
    """steps: ("run", frames) one process call | ("calc", changes) CalcFilters | ("nco", NCOFreq) | ("coeffs", params)
    t41rx_set_coeffs with a blob designed for default_params(**params) -- on a context and on an OracleBatch alike"""
    Lf = 4 * N
    kw0 = dict(kw0, fft_length=N)
    rx = T.RxChain(I.shape[0], T.default_params(**kw0), NCOFreq=nco0)
    ob = O.OracleBatch(O.default_params(**kw0), np.asarray(nco0, np.int32))
    got, ref, tol, calls, pos = [], [], [], 0, 0
    parities = []  # of the call count at every change
    for op, arg in steps:
        if op == "run":
            i, q = cut(I, pos, pos + arg, Lf), cut(Q, pos, pos + arg, Lf)
            got.append(dev(rx, i, q))
            ref.append(ob.process(i, q, nthreads=8))
            tol += [AM_TOL if ob.p.mode == 2 else TOL] * arg
            pos += arg
            calls += 1
            continue
        parities.append(calls & 1)
        if op == "calc":
            rx.CalcFilters(**arg)
            for k, v in arg.items():
                setattr(ob.p, k, v)
        elif op == "nco":
            rx.SetNCOFreq(arg)
            ob.nco[:] = arg
        elif op == "coeffs":
            p = T.default_params(**dict(arg, fft_length=N))
            rx.set_coeffs(T.design_coeffs(p))
            now = rx.get_params()
            for f, _ in O.Params._fields_:  # (t41rx_params and the oracle's parameters are the same record)
                assert getattr(now, f) == getattr(p, f), f
                setattr(ob.p, f, getattr(p, f))
        ob.redesign()  # (raises if the oracle's designer refuses the parameters)
    assert pos * Lf == I.shape[1]
    return np.concatenate(got, axis=1), np.concatenate(ref, axis=1), tol, parities


def first_segment(frames, lead):
    """the stream's first segment in `lead` calls: every later change then falls on the other call parity"""
    return [("run", frames)] if lead == 1 else [("run", 1), ("run", frames - 1)]


LEADS = pytest.mark.parametrize("lead", [1, 2], ids=["first-change-odd", "first-change-even"])


@LEADS
@pytest.mark.parametrize("N", [1024, 4096])
def test_b_filters_tuning_and_side_tone(T, N, lead):
    """CalcFilters (cut-offs, audioVolume), SetNCOFreq, then xmtMode SSB -> CW (the side-tone offset is part of the
    oscillator increment: upload_nco) between the calls of one stream; the tone stays inside every filter"""
    nch, Lf = 7, 4 * N
    nco1 = siggen.nco_grid(nch, seed=N + 1)
    nco2 = nco1 + 300  # the audio tone moves down by 300 Hz
    I, Q = signal(0, nch, 6 * Lf, nco1, seed=N + 2, audio_hz=(1900.0, 2100.0), fade=[(0.5, 1.5), (0.5, 0.4)])
    steps = first_segment(2, lead) + [("calc", dict(FLoCut=300, FHiCut=2600, audioVolume=45)), ("run", 1), ("nco", nco2), ("run", 2),
                                      ("calc", dict(xmtMode=1, CWFreqShift=750)), ("run", 1)]
    got, ref, tol, par = play(T, N, USB, nco1, I, Q, steps)
    assert par == ([1, 0, 1] if lead == 1 else [0, 1, 0])
    check_vs_oracle(got, ref, N, tol, "B filters/tuning/side-tone %d lead %d" % (N, lead))


def mode_stream(nch, Lf, nco, seed, modes, frames=2):
    parts = [signal(m, nch, frames * Lf, nco, seed=seed + 10 * k, fade=[(0.5, 1.5), (0.5, 0.4)]) for k, m in enumerate(modes)]
    return np.concatenate([p[0] for p in parts], axis=1), np.concatenate([p[1] for p in parts], axis=1)


@LEADS
@pytest.mark.parametrize("N", [512, 1024, 4096])
def test_b_mode_sequence(T, N, lead):
    """USB -> AM -> NFM -> USB in one stream, state never reset: the back kernel keeps the AM / NFM demodulator words
    and the filter memories across the switches as the reference keeps its statics.  NFM's overlap-save is real
    (Process.cpp:765-816): its first frame takes the decimated I samples of the mode before as the previous block,
    with a zero imaginary half, and leaves last_sample_buffer_R alone, so the first frame after NFM pairs the last
    NFM audio block with the Q samples of the last AM frame.  (512 points: the same rule in the fused kernel.)"""
    nch, Lf = 5, 4 * N
    nco = siggen.nco_grid(nch, seed=N + 3)
    I, Q = mode_stream(nch, Lf, nco, N + 4, [0, 2, 3, 0])
    steps = first_segment(2, lead) + [("calc", AM), ("run", 2), ("calc", NFM), ("run", 2), ("calc", USB), ("run", 2)]
    got, ref, tol, par = play(T, N, USB, nco, I, Q, steps)
    assert par == ([1, 0, 1] if lead == 1 else [0, 1, 0])
    check_vs_oracle(got, ref, N, tol, "B modes %d lead %d" % (N, lead))


@LEADS
@pytest.mark.parametrize("N,kw", [(2048, LSB), (4096, USB)], ids=["lsb-2048", "usb-4096"])
def test_b_agc_sequence(T, N, kw, lead):
    """AGCMode 0 -> 2 -> 0 -> 4, then AGC_thresh, in one stream: the AGC's delay line and gain words are kept while it
    is off and picked up where they stand when it comes back"""
    nch, Lf = 6, 4 * N
    nco = siggen.nco_grid(nch, seed=N + 5)
    I, Q = signal(kw["mode"], nch, 8 * Lf, nco, seed=N + 6, fade=[(0.3, 1.5), (0.3, 0.4), (0.4, 1.2)])
    steps = first_segment(2, lead) + [("calc", dict(AGCMode=2)), ("run", 2), ("calc", dict(AGCMode=0)), ("run", 1),
                                      ("calc", dict(AGCMode=4)), ("run", 2), ("calc", dict(AGC_thresh=30)), ("run", 1)]
    got, ref, tol, par = play(T, N, kw, nco, I, Q, steps)
    assert par == ([1, 0, 1, 0] if lead == 1 else [0, 1, 0, 1])
    check_vs_oracle(got, ref, N, tol, "B agc %d lead %d" % (N, lead))


@LEADS
@pytest.mark.parametrize("N", [1024, 2048])
def test_b_set_coeffs_mid_stream(T, N, lead):
    """t41rx_set_coeffs with a blob designed for other parameters (filter, AGC on, volume) between two calls; the
    context then reports the designer's parameters (asserted in play()) and a later CalcFilters starts from them"""
    nch, Lf = 5, 4 * N
    nco = siggen.nco_grid(nch, seed=N + 8)
    I, Q = signal(0, nch, 6 * Lf, nco, seed=N + 9, audio_hz=(800.0, 2000.0), fade=[(0.5, 1.5), (0.5, 0.3)])
    steps = first_segment(2, lead) + [("coeffs", dict(mode=0, FLoCut=300, FHiCut=2400, AGCMode=3, audioVolume=40)), ("run", 2),
                                      ("calc", dict(audioVolume=55)), ("run", 2)]
    got, ref, tol, par = play(T, N, USB, nco, I, Q, steps)
    assert par == ([1, 0] if lead == 1 else [0, 1])
    check_vs_oracle(got, ref, N, tol, "B set_coeffs %d lead %d" % (N, lead))


# ---- C: mixed entry points in one stream ---------------------------------------------------------------------------------
def q15_to_float(q):
    out = np.empty(q.shape, np.float32)
    q = np.ascontiguousarray(q)
    O.lib().t41o_q15_to_float(q.ctypes.data_as(C.POINTER(C.c_int16)), O.fptr(out), q.size)
    return out


# entry point and frames per call: every entry point once at even and once at odd call parity.  The host entry points'
# staging buffers grow at calls 1, 3 and 4 (bytes per array: f32 frames x 4, q15 frames x 2), the pipeline's scratch at 3
C_CALLS = [("dev-f32", 1), ("host-f32", 1), ("dev-q15", 1), ("host-q15", 3), ("host-f32", 2), ("dev-q15", 1), ("host-q15", 1), ("dev-f32", 1)]


@pytest.mark.parametrize("N,kw", [(1024, dict(USB, AGCMode=2, audioVolume=100)), (4096, dict(LSB, audioVolume=100))], ids=["usb-agc-1024", "lsb-4096"])
def test_c_mixed_entry_points(T, N, kw):
    import torch
    nch, Lf = 5, 4 * N
    nfr = sum(n for _, n in C_CALLS)
    kw = dict(kw, fft_length=N)
    nco = siggen.nco_grid(nch, seed=N + 11)
    I, Q = signal(kw["mode"], nch, nfr * Lf, nco, seed=N + 12, fade=[(0.4, 1.5), (0.3, 0.4), (0.3, 1.2)])
    qI, qQ = to_q15(I), to_q15(Q)          # generated as q15 ...
    fI, fQ = q15_to_float(qI), q15_to_float(qQ)  # ... and converted for the f32 calls: both sides see the same samples
    rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
    f32 = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)  # the same stream through device-f32 calls only
    ob = O.OracleBatch(O.default_params(**kw), np.asarray(nco, np.int32))
    seen, pos, worst, worst_q = set(), 0, 0.0, 0
    startup, f_peaks, q_peaks = None, [], []
    for k, (entry, n) in enumerate(C_CALLS):
        seen.add((entry, k & 1))
        what = "C %d call %d (%s, %d frames)" % (N, k, entry, n)
        only = dev(f32, cut(fI, pos, pos + n, Lf), cut(fQ, pos, pos + n, Lf))
        if entry.endswith("f32"):
            i, q = cut(fI, pos, pos + n, Lf), cut(fQ, pos, pos + n, Lf)
            got = dev(rx, i, q) if entry == "dev-f32" else rx.ProcessIQData(i, q)
            ref = ob.process(i, q, nthreads=8)
            assert np.array_equal(got, only), what
            tol = AM_TOL if kw["mode"] == 2 else TOL
            if N == 4096 and k == 0:  # filter start-up: compared absolutely, below
                startup = np.abs(got - ref).max()
            else:
                err = siggen.block_rel_err(got, ref, Lf)
                worst = max(worst, err.max())
                assert err.max() <= tol, (what, err.max())
                f_peaks.append(np.abs(ref).reshape(nch, n, Lf).max(axis=2))
        else:
            l, r = cut(qQ, pos, pos + n, Lf), cut(qI, pos, pos + n, Lf)  # the L queue carries Q, the R queue I (Process.cpp:107-108)
            if entry == "dev-q15":
                got = rx.ProcessIQData_q15(torch.from_numpy(l).cuda(), torch.from_numpy(r).cuda()).cpu().numpy()
            else:
                got = rx.ProcessIQData_q15(l, r)
            ref = ob.process_q15(l, r)
            assert got.dtype == np.int16
            q_peaks.append(np.abs(ref.astype(np.int32)).reshape(nch, n, Lf).max(axis=2))
            # the q15 entry points are the f32 path on the converted samples, then arm_float_to_q15 (test_gpu_q15_long_fft)
            assert np.array_equal(got, np.clip(np.trunc(only.astype(np.float64) * 32768.0), -32768, 32767).astype(np.int16)), what
            d = np.abs(got.astype(np.int32) - ref.astype(np.int32))
            tol = 5e-5 if kw["mode"] == 2 else 1e-5
            assert d.max() <= 1 + np.ceil(tol * np.abs(ref.astype(np.int32)).max()), (what, d.max())
            worst_q = max(worst_q, int(d.max()))
        pos += n
    assert len(seen) == 8  # four entry points x two parities
    # every compared piece of the reference holds a signal
    f_peaks, q_peaks = np.concatenate(f_peaks, axis=1), np.concatenate(q_peaks, axis=1)
    assert f_peaks.min() > 1e-3 * f_peaks.max() and q_peaks.min() > max(1e-3 * q_peaks.max(), 500), (f_peaks.min(axis=0), q_peaks.min(axis=0))
    if startup is not None:
        assert startup <= 1e-5 * f_peaks.max(), startup
    assert np.array_equal(rx.get_state(), f32.get_state())
    print("C %d: worst block-relative error %.3e in the f32 pieces, worst q15 difference %d LSB" % (N, worst, worst_q))


# ---- D: refusals leave the stream alone; the blanker's slot parity --------------------------------------------------------
@pytest.mark.parametrize("N,kw", [(2048, dict(LSB, AGCMode=3)), (4096, USB)], ids=["lsb-agc-2048", "usb-4096"])
def test_d_refused_calls_change_nothing(T, N, kw):
    """calls that must be refused, between the calls of a stream at either parity: each answers its documented status
    (include/t41rx.h), and the stream's samples and final checkpoint are those of the undisturbed stream.  All of them
    are argument checks that return before any kernel is launched."""
    import torch
    from t41_sdr_amd import _lib
    lib = T.load()
    nch, Lf, nfr = 5, 4 * N, 5
    kw = dict(kw, fft_length=N)
    nco = siggen.nco_grid(nch, seed=N + 13)
    I, Q = signal(kw["mode"], nch, nfr * Lf, nco, seed=N + 14)
    edges = [0, 1, 2, 4, 5]
    new = lambda: T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)  # noqa: E731
    plain_rx = new()
    plain = run(plain_rx, I, Q, Lf, edges)
    rx = new()
    other_n = T.RxChain(nch + 1, T.default_params(**kw)).get_state()
    other_fft = T.RxChain(nch, T.default_params(**dict(kw, fft_length=1024 if N != 1024 else 2048))).get_state()
    x = torch.zeros(nch * Lf + 4, device="cuda")  # one frame and one float4 to spare
    h = np.zeros(nch * Lf, np.float32)
    hp = h.ctypes.data_as(C.POINTER(C.c_float))
    hq = np.zeros(nch * Lf, np.int16).ctypes.data_as(C.c_void_p)
    tap = torch.zeros(nch, 2 * N, device="cuda")

    def refusals():
        ck = rx.get_state()
        sections = ck.copy()
        sections[:32].view(np.int32)[5] |= 1 << 6  # a section no build knows
        agc = ck.copy()
        records(agc, nch)[:, -8:].view(np.int32)[1, 4] = 9  # AGC state word (rx_internal.hpp: kAgcStState) out of 0..4
        p, p4 = x.data_ptr(), x.data_ptr() + 4  # (p4: an offset view of the same tensor, not 16-byte aligned)
        return [
            ("set_state: other channel count", lambda: rx.set_state(other_n), _lib.ERR_STATE),
            ("set_state: other fft_length", lambda: rx.set_state(other_fft), _lib.ERR_STATE),
            ("set_state: unknown section", lambda: rx.set_state(sections), _lib.ERR_STATE),
            ("set_state: AGC state word", lambda: rx.set_state(agc), _lib.ERR_STATE),
            ("set_state: truncated", lambda: rx.set_state(ck[:-4]), _lib.ERR_STATE),
            ("set_params: fft_length", lambda: rx.CalcFilters(fft_length=512), _lib.ERR_ARG),
            ("set_params: nrOptionSelect", lambda: rx.CalcFilters(nrOptionSelect=1), _lib.ERR_ARG),
            ("set_params: nfm_demod", lambda: rx.CalcFilters(mode=3, FLoCut=200, FHiCut=3000, nfm_demod=1), _lib.ERR_ARG),
            ("set_params: cut-offs", lambda: rx.CalcFilters(FLoCut=3000, FHiCut=200), _lib.ERR_ARG),
            ("set_buffer_layout", lambda: rx.set_buffer_layout("time"), _lib.ERR_UNSUPPORTED),
            ("set_noise_blanker", lambda: rx.set_noise_blanker(1), _lib.ERR_UNSUPPORTED),
            ("set_receive_eq", lambda: rx.set_receive_eq(1), _lib.ERR_UNSUPPORTED),
            ("set_debug_taps", lambda: rx.set_debug_taps(demod=tap), _lib.ERR_UNSUPPORTED),
            ("set_nco_freq: beyond Fs/2", lambda: rx.SetNCOFreq(np.full(nch, 96001)), _lib.ERR_ARG),
            ("process_device: n_frames 0", lambda: lib.t41rx_process_device(rx._ctx, p, p, p, 0, None), _lib.ERR_ARG),
            ("process_device_q15: n_frames 0", lambda: lib.t41rx_process_device_q15(rx._ctx, p, p, p, 0, None), _lib.ERR_ARG),
            ("process_host: n_frames 0", lambda: lib.t41rx_process_host(rx._ctx, hp, hp, hp, 0), _lib.ERR_ARG),
            ("process_host_q15: n_frames 0", lambda: lib.t41rx_process_host_q15(rx._ctx, hq, hq, hq, 0), _lib.ERR_ARG),
            ("process_device: unaligned I", lambda: lib.t41rx_process_device(rx._ctx, p4, p, p, 1, None), _lib.ERR_ARG),
            ("process_device: unaligned audio", lambda: lib.t41rx_process_device(rx._ctx, p, p, p4, 1, None), _lib.ERR_ARG),
            ("process_device_q15: unaligned Q", lambda: lib.t41rx_process_device_q15(rx._ctx, p, p4, p, 1, None), _lib.ERR_ARG),
            ("process_device: null", lambda: lib.t41rx_process_device(rx._ctx, p, None, p, 1, None), _lib.ERR_ARG),
        ]

    def disturb(k):
        before = rx.get_params()
        for what, fn, status in refusals():
            assert refused(T, fn) == status, (what, "after call %d" % k)
        now = rx.get_params()
        assert all(getattr(now, f) == getattr(before, f) for f, _ in _lib.Params._fields_)
        assert rx.layout == "channel" and rx.noise_blanker == 0 and rx.receive_eq[0] == 0

    got = run(rx, I, Q, Lf, edges, between=disturb)
    assert np.array_equal(got, plain)
    assert np.array_equal(rx.get_state(), plain_rx.get_state())
    assert np.abs(plain).reshape(nch, nfr, Lf).max(axis=2)[:, 1:].min() > 0


@pytest.mark.parametrize("stamp_taps", [None, "1"], ids=["unset", "T41RX_STAMP_TAPS"])
def test_d_product_ignores_the_stamp_taps_variable(T, stamp_taps, monkeypatch):
    """T41RX_STAMP_TAPS lets a -DT41RX_STAMP diagnostic build put its cycle stamps behind the demod tap at the long FFT
    lengths.  The product library does not read it: with it in the environment, as without, the demod tap at fft_length
    1024 is refused with T41RX_ERR_UNSUPPORTED.  One channel, no process call."""
    import torch
    from t41_sdr_amd import _lib
    if stamp_taps is None:
        monkeypatch.delenv("T41RX_STAMP_TAPS", raising=False)
    else:
        monkeypatch.setenv("T41RX_STAMP_TAPS", stamp_taps)  # before the context exists
    rx = T.RxChain(1, T.default_params(fft_length=1024, **USB))
    tap = torch.zeros(1, 512, device="cuda")
    assert refused(T, lambda: rx.set_debug_taps(demod=tap)) == _lib.ERR_UNSUPPORTED
    assert "stage taps" in T.load().t41rx_last_error().decode()


def test_d_noise_blanker_carry_under_launch_parity(T):
    """fft_length 512, blanker on: its carry (last_frame_end) lives in two slots and `nb_sel` flips with every blanker
    launch.  Checkpoints behind x1 after one (odd) and two (even) launches are the same bytes; x2 continues bit for
    bit from either in the context it came from, a fresh one and one that has made one launch; reset at either
    parity gives the fresh stream.  The input puts impulses into the first 13 samples of blocks, and the carry is
    shown to matter at the seam: a checkpoint with the blanker section zeroed continues differently.  (The stream and
    the seam of test_noise_blanker.py's test_gpu_checkpoint_and_refusals, where the blanker model finds an impulse below
    sample 13 in the first block behind the seam.)"""
    L = 2048
    kw = dict(mode=8, **WIDE[8])
    nch, nfr, n1 = 5, 10, 6
    nco = siggen.nco_grid(nch, seed=23)
    I, Q = clicky_iq(nch, nfr, 23)

    def new():
        rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
        rx.set_noise_blanker(1)
        return rx

    x1 = lambda rx, calls: run(rx, I, Q, L, [0, n1] if calls == 1 else [0, 2, n1])  # noqa: E731
    x2 = lambda rx, calls=1: run(rx, I, Q, L, [n1, nfr] if calls == 1 else [n1, n1 + 1, nfr])  # noqa: E731
    ref = new()
    o1, o2 = x1(ref, 1), x2(ref)
    final = ref.get_state()
    cks = {}
    for calls in (1, 2):
        rx = new()
        assert np.array_equal(x1(rx, calls), o1)
        ck = cks[calls] = rx.get_state()
        assert ck[:32].view(np.int32)[5] == 4 and np.array_equal(rx.get_state(), ck)  # the blanker's section, nothing else
        x2(rx)  # moves on: the other parity
        busy = new()
        dev(busy, cut(Q, 1, 2, L), cut(I, 1, 2, L))
        for label, ctx, x2_calls in (("same context", rx, 1), ("fresh context", new(), 1), ("context after one launch", busy, 1),
                                     ("fresh context, x2 in two calls", new(), 2)):
            ctx.set_state(ck)
            assert np.array_equal(x2(ctx, x2_calls), o2), (label, "checkpoint after %d launches" % calls)
            assert np.array_equal(ctx.get_state(), final), (label, calls)
    assert np.array_equal(cks[1], cks[2])
    # the carry matters at this seam
    blank = cks[1].copy()
    blank[-64 * nch:] = 0
    assert cks[1][-64 * nch:].any()
    rx = new()
    rx.set_state(blank)
    assert not np.array_equal(x2(rx), o2)
    # reset after an odd and after an even number of launches
    for calls in (1, 2):
        rx = new()
        x2(rx, calls)
        rx.reset()
        assert np.array_equal(x1(rx, 1), o1) and np.array_equal(rx.get_state(), cks[1]), calls
