"""The transmit equaliser (xmitEQFlag, DoExciterEQ(), Filter.cpp:176-224) inside the exciter, and the exciter's checkpoint.
CPU: the f32 restatement tests/tx_model.py against the frozen oracle (equaliser off, bit for bit), against an independent
float64 stream model (equaliser on), the reference's whole-hundreds level rule, and the C ABI's new symbols and refusals.
GPU: tx_kernel<true> against the restatement on q15 samples, bit for bit -- parity, streaming, switches in mid-stream with
stale memories, reset, the rails, more channels than CUs, checkpoints and refusals."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import tx_model as M
from tx_harness import F, assert_same, cat, mic, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USB, LSB, AM = O.DEMOD_USB, O.DEMOD_LSB, O.DEMOD_AM
OK, ERR_ARG, ERR_STATE = 0, -1, -5
ALL100 = (100,) * 14
QUIRK = (50, 99, 100, 150, 199, 200, -50, -100, -199, 0, 1, 250, 100, 100)
NEW_SYMBOLS = ("t41tx_set_transmit_eq_bands", "t41tx_set_transmit_eq", "t41tx_get_transmit_eq",
               "t41tx_state_bytes", "t41tx_get_state", "t41tx_set_state")


# ---- CPU: the models
CASES = ((USB, 1.0, 0.0), (LSB, 0.97, -0.02), (USB, 1.03, 0.015))  # test_tx_exciter.py's three


def test_model_with_the_equaliser_off_is_the_oracle():
    """pins every stage of tx_model.TxModel except the equaliser to the frozen oracle, bit for bit"""
    nch, nfr = 2, 4
    q = mic(nch, nfr)
    for mode, amp, phase in CASES:
        assert_same(M.TxModelBatch(nch, mode, amp, phase).process(q), O.TxOracleBatch(nch, mode, amp, phase).process(q),
                    "mode %d (%g, %g)" % (mode, amp, phase))


@pytest.mark.parametrize("levels", [M.DEFAULT_LEVELS, ALL100], ids=["default-levels", "all-100"])
def test_model_with_the_equaliser_on_matches_a_float64_stream_model(levels):
    """The bound is measured between these two CPU models (neither is the code under test): over these inputs the
    largest deviation on the q15 grid is 1 LSB for both level sets and every case (the float chains agree to ~1e-6 of
    full scale, truncation adds one LSB), so twice that is 2 LSB -- the floor, test_tx_exciter.py's own bound."""
    bound = 2
    nch, nfr = 2, 4
    q = mic(nch, nfr)
    tabs = [O.TxOracleBatch(0).table(i) for i in range(4)]
    worst = 0
    for mode, amp, phase in CASES:
        oL, oR = M.TxModelBatch(nch, mode, amp, phase, eq_on=True, levels=levels).process(q)
        offL, _ = M.TxModelBatch(nch, mode, amp, phase).process(q)
        assert not np.array_equal(oL, offL) and np.abs(oL).max() > 1000  # the equaliser did something audible
        for c in range(nch):
            mI, mQ = M.stream_model_f64(q[c], mode, amp, phase, tabs, eq_on=True, levels=levels)
            for o, m in ((oL[c], mI), (oR[c], mQ)):
                want = np.trunc(np.clip(m[:o.size] * 32768.0, -32768, 32767))
                worst = max(worst, int(np.abs(o - want).max()))
    print("f32 restatement vs float64 stream model, %r: max deviation %d LSB" % (levels, worst))
    assert worst <= bound, worst


def test_level_rule_counts_whole_hundreds():
    """equalizerXmt[] is an int array (gwv.h:44): (float)level / 100.0 is truncated toward zero on the way in"""
    assert M.whole_levels(QUIRK) == [0, 0, 1, 1, 1, 2, 0, -1, -1, 0, 0, 2, 1, 1]
    sign = np.where(np.arange(14) % 2 == 0, -1.0, 1.0)
    assert np.array_equal(M.signed_scales(QUIRK), (sign * M.whole_levels(QUIRK)).astype(np.float32))
    assert M.whole_levels(M.DEFAULT_LEVELS) == [0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0]
    # levels of 50 everywhere: every scale is 0 and the output silent, yet the cascades' memories advance -- switched to
    # 100 afterwards the channel continues like one that ran at 100 throughout
    q = mic(1, 5, seed=4)
    a = M.TxModelBatch(1, eq_on=True, levels=(50,) * 14)
    b = M.TxModelBatch(1, eq_on=True, levels=ALL100)
    a0, b0 = a.process(q[:, :2 * F]), b.process(q[:, :2 * F])
    assert not a0[0].any() and not a0[1].any() and b0[0].any()
    assert np.array_equal(a.chs[0].eq, b.chs[0].eq) and a.chs[0].eq.any()
    a.levels = ALL100
    a1, b1 = a.process(q[:, 2 * F:]), b.process(q[:, 2 * F:])
    # the first frame at 100 still has silence in the Hilbert delay line (99 samples @24 kS/s); from the next on, equal
    assert not np.array_equal(a1[0][:, :F], b1[0][:, :F])
    assert_same((a1[0][:, F:], a1[1][:, F:]), (b1[0][:, F:], b1[1][:, F:]), "after 50 -> 100")


# ---- CPU: the C ABI
def _raw():
    from t41_sdr_amd import tx
    return tx._load()


def test_tx_equaliser_abi_symbols_and_null_refusals(built):
    import t41_sdr_amd as T
    from t41_sdr_amd import tx
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "t41tx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(t41tx_[a-z0-9_]+)\s*\(", hdr))
    listed = set(re.findall(r"\b(t41tx_[a-z0-9_]+);", re.sub(r"#.*", "", open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read())))
    raw = C.CDLL(T.LIB_PATH)
    for s in NEW_SYMBOLS:
        assert s in declared and s in listed and s in tx.TX_SYMBOLS and hasattr(raw, s), s
    for m in ("set_transmit_eq_bands", "set_transmit_eq", "get_transmit_eq", "get_state", "set_state"):
        assert callable(getattr(T.TxChain, m))
    assert raw.t41rx_abi_version() == 5
    # refusals that need no device: a NULL context (and NULL arguments), each with its own text
    lib = _raw()
    coef = np.ascontiguousarray(M.bands())
    lv = np.zeros(14, np.int32)
    buf = np.zeros(64, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    cases = [
        ("set_transmit_eq_bands(NULL ctx)", lambda: lib.t41tx_set_transmit_eq_bands(None, p(coef))),
        ("set_transmit_eq(NULL ctx)", lambda: lib.t41tx_set_transmit_eq(None, 0, None)),
        ("get_transmit_eq(NULL ctx)", lambda: lib.t41tx_get_transmit_eq(None, p(lv))),
        ("get_state(NULL ctx)", lambda: lib.t41tx_get_state(None, p(buf), buf.size)),
        ("set_state(NULL ctx)", lambda: lib.t41tx_set_state(None, p(buf), buf.size)),
    ]
    for name, call in cases:
        ctx = C.c_void_p()
        assert lib.t41rx_create(C.byref(ctx), 0, 4, C.byref(T.default_params(fft_length=777))) == ERR_ARG  # another message
        assert call() == ERR_ARG, name
        assert lib.t41rx_last_error().decode() == "null argument", name
    assert lib.t41tx_state_bytes(None) == 0
    assert not lv.any()  # a refused getter writes nothing


# ---- GPU helpers
def chain(nch, mode=USB, amp=1.0, phase=0.0, on=True, levels=None):
    """a context with the band table loaded and the equaliser switched"""
    import t41_sdr_amd as T
    tx = T.TxChain(nch, T.default_tx_params(mode=mode, IQXAmpCorrectionFactor=amp, IQXPhaseCorrectionFactor=phase))
    tx.set_transmit_eq_bands(M.bands())
    tx.set_transmit_eq(on, levels)
    return tx


NCH, NFR = 9, 5
PARITY = {"usb-default": (USB, 1.0, 0.0, M.DEFAULT_LEVELS, 0.9),
          "lsb-corr-quirk": (LSB, 0.97, -0.02, QUIRK, 0.4),
          "am-all-100": (AM, 1.0, 0.0, ALL100, 0.4)}


@functools.lru_cache(maxsize=None)
def parity_case(name):
    """(q, the model's output with the equaliser on, with it off): computed once, shared, never written to"""
    mode, amp, phase, levels, lvl = PARITY[name]
    q = mic(NCH, NFR, seed=3, level=lvl)
    on = M.TxModelBatch(NCH, mode, amp, phase, eq_on=True, levels=levels).process(q)
    off = M.TxModelBatch(NCH, mode, amp, phase).process(q)
    for a in (q,) + on + off:
        a.setflags(write=False)
    return q, on, off


# ---- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARITY))
def test_gpu_tx_eq_parity(built, name):
    mode, amp, phase, levels, _ = PARITY[name]
    q, ref_on, ref_off = parity_case(name)
    tx = chain(NCH, mode, amp, phase, True, None if name == "usb-default" else levels)
    on, lv = tx.get_transmit_eq()
    assert on == 1 and tuple(lv) == tuple(levels)
    got = run(tx, q)
    assert_same(got, ref_on, name)
    off = run(chain(NCH, mode, amp, phase, False), q)
    assert_same(off, ref_off, name + ", equaliser off")           # the switch off is the exciter of before
    assert not np.array_equal(got[0], off[0]) and not np.array_equal(got[1], off[1])
    assert np.abs(got[0]).max() > 1000 and np.abs(got[1]).max() > 1000  # not silent


@pytest.mark.gpu
def test_gpu_tx_eq_streaming_frame_by_frame(built):
    """five 1-frame host calls == one 5-frame device call: the memories, the per-call fill / drain of the section
    pipeline and the round trip of the state through HBM"""
    q, ref_on, _ = parity_case("lsb-corr-quirk")
    mode, amp, phase, levels, _ = PARITY["lsb-corr-quirk"]
    whole = run(chain(NCH, mode, amp, phase, True, levels), q)
    tx = chain(NCH, mode, amp, phase, True, levels)
    parts = [tx.ExciterIQData(np.ascontiguousarray(q[:, k * F:(k + 1) * F])) for k in range(NFR)]
    assert_same(cat(parts), whole, "5 x 1 frame (host) vs 1 x 5 frames (device)")
    assert_same(whole, ref_on)


@pytest.mark.gpu
def test_gpu_tx_eq_switches_in_mid_stream(built):
    """frames 0-1 on, 2 off, 3-4 on: the memories are stale across the gap, as in the reference; a new band table
    between frames 3 and 4 takes effect at once and does not reset them"""
    q = mic(NCH, NFR, seed=5, level=0.6)
    other = M.bands()[::-1].copy()  # the same 14 cascades on other bands' memories
    tx, mo = chain(NCH, LSB, 0.97, -0.02, True, ALL100), M.TxModelBatch(NCH, LSB, 0.97, -0.02, eq_on=True, levels=ALL100)
    got, ref = [], []
    for (a, b), on, table in (((0, 2), 1, None), ((2, 3), 0, None), ((3, 4), 1, None), ((4, 5), 1, other)):
        if table is not None:
            tx.set_transmit_eq_bands(table)
            mo.set_bands(table)
        tx.set_transmit_eq(on)
        mo.eq_on = bool(on)
        tx.set_params(mode=LSB)  # switch, levels and table survive set_params
        got.append(run(tx, q[:, a * F:b * F]))
        ref.append(mo.process(q[:, a * F:b * F]))
    assert_same(cat(got), cat(ref), "on, on, off, on, on with a new table")
    assert tx.get_transmit_eq()[0] == 1 and tuple(tx.get_transmit_eq()[1]) == ALL100
    # the stale memories matter: a model whose memories are cleared at frame 3 gives other samples
    fresh = M.TxModelBatch(NCH, LSB, 0.97, -0.02, eq_on=True, levels=ALL100)
    fresh.process(q[:, :3 * F])
    for ch in fresh.chs:
        ch.eq[:] = 0
    assert not np.array_equal(fresh.process(q[:, 3 * F:4 * F])[0], ref[2][0])


@pytest.mark.gpu
def test_gpu_tx_eq_reset_clears_the_memories(built):
    q = mic(NCH, 4, seed=6, level=0.6)
    tx = chain(NCH, USB, 1.0, 0.0, True, ALL100)
    run(tx, q[:, :2 * F])
    tx.reset()
    after = run(tx, q[:, 2 * F:])
    assert_same(after, run(chain(NCH, USB, 1.0, 0.0, True, ALL100), q[:, 2 * F:]), "after reset vs a fresh context")
    assert_same(after, M.TxModelBatch(NCH, eq_on=True, levels=ALL100).process(q[:, 2 * F:]), "after reset vs the model")


@pytest.mark.gpu
def test_gpu_tx_eq_rails(built):
    """a full-scale square wave through levels of 250 (scale 2 on every band): the clamp at both rails"""
    nch, nfr = 3, 3
    n = np.arange(nfr * F)
    q = np.stack([np.where((n // h) % 2 == 0, 32767, -32767) for h in (96, 160, 37)]).astype(np.int16)  # 1 kHz, 600 Hz, 2.6 kHz
    levels = (250,) * 14
    got = run(chain(nch, USB, 1.0, 0.0, True, levels), q)
    assert_same(got, M.TxModelBatch(nch, eq_on=True, levels=levels).process(q), "rails")
    for o in got:
        assert (o == 32767).any() and (o == -32768).any()


@pytest.mark.gpu
def test_gpu_tx_eq_more_channels_than_cus(built):
    nch, nfr = 257, 2
    rng = np.random.default_rng(8)
    q = (mic(1, nfr, seed=9, level=1.0).astype(np.float64) * rng.uniform(0.05, 0.9, (nch, 1))).astype(np.int16)
    q = np.ascontiguousarray(np.stack([np.roll(q[c], 7 * c) for c in range(nch)]))
    got = run(chain(nch, LSB, 0.97, -0.02, True, QUIRK), q)
    assert_same(got, M.TxModelBatch(nch, LSB, 0.97, -0.02, eq_on=True, levels=QUIRK).process(q), "257 channels")


@pytest.mark.gpu
def test_gpu_tx_checkpoint(built):
    import t41_sdr_amd as T
    mode, amp, phase, levels, _ = PARITY["lsb-corr-quirk"]
    q, ref_on, _ = parity_case("lsb-corr-quirk")
    tx = chain(NCH, mode, amp, phase, True, levels)
    lib = tx._lib
    n0 = lib.t41tx_state_bytes(tx._ctx)
    assert n0 == 32 + 4 * 448 * NCH
    first = run(tx, q[:, :2 * F])
    ck = tx.get_state()
    assert ck.size == n0 == lib.t41tx_state_bytes(tx._ctx)
    hdr = ck[:32].view(np.int32)
    assert hdr[0] == int.from_bytes(b"T41X", "little") and list(hdr[1:]) == [5, NCH, 448, 0, 0, 0, 0]
    rec = ck[32:].view(np.float32).reshape(NCH, 448)
    assert rec[:, 336:].any() and rec[:, :336].any()  # the equaliser's memories ride along
    # a new context with the same configuration continues the stream
    tx2 = chain(NCH, mode, amp, phase, True, levels)
    tx2.set_state(ck)
    assert_same(cat([first, run(tx2, q[:, 2 * F:])]), ref_on, "2 frames, checkpoint, 3 frames in a new context")
    assert lib.t41tx_state_bytes(tx2._ctx) == n0
    # refused checkpoints: truncated, another channel count, a NaN -- and the stream goes on unharmed
    other = chain(5, mode, amp, phase, True, levels).get_state()
    nan = ck.copy()
    nan[32:].view(np.float32)[448 + 340] = np.nan
    magic = ck.copy()
    magic[:4] = np.frombuffer(b"T41S", np.uint8)
    for bad, what in ((ck[:-4], "size"), (ck[:16], "size"), (other, "header"), (nan, "non-finite"), (magic, "header")):
        with pytest.raises(T.T41RxError, match=what) as e:
            tx.set_state(bad)
        assert e.value.status == ERR_STATE, what
    small = np.zeros(n0 - 1, np.uint8)
    assert lib.t41tx_get_state(tx._ctx, small.ctypes.data_as(C.c_void_p), small.size) == ERR_STATE
    assert lib.t41rx_last_error().decode() == "state buffer too small"
    assert_same(cat([first, run(tx, q[:, 2 * F:])]), ref_on, "the original context after the refusals")


@pytest.mark.gpu
def test_gpu_tx_eq_refusals_leave_the_context_alone(built):
    import t41_sdr_amd as T
    q, ref_on, ref_off = parity_case("usb-default")
    q1 = q[:, :F]
    tx = T.TxChain(NCH)
    # switch-on before a table
    with pytest.raises(T.T41RxError, match="no band table loaded") as e:
        tx.set_transmit_eq(1)
    assert e.value.status == ERR_ARG and tx.get_transmit_eq()[0] == 0
    assert tuple(tx.get_transmit_eq()[1]) == M.DEFAULT_LEVELS
    bad = M.bands()
    bad[13, 3, 4] = np.nan
    with pytest.raises(T.T41RxError, match="non-finite coefficient") as e:
        tx.set_transmit_eq_bands(bad)
    assert e.value.status == ERR_ARG
    with pytest.raises(T.T41RxError, match="no band table loaded"):  # the refused table was not kept
        tx.set_transmit_eq(1)
    assert tx._lib.t41tx_set_transmit_eq_bands(tx._ctx, None) == ERR_ARG
    assert_same(run(tx, q1), (ref_off[0][:, :F], ref_off[1][:, :F]), "still off")
    # on a running equaliser: flag 2, with levels that must not be taken; a NaN table that must not replace the good one
    tx = chain(NCH)
    with pytest.raises(T.T41RxError, match="xmitEQFlag must be 0 or 1") as e:
        tx.set_transmit_eq(2, ALL100)
    assert e.value.status == ERR_ARG
    with pytest.raises(T.T41RxError, match="xmitEQFlag must be 0 or 1"):
        tx.set_transmit_eq(-1)
    with pytest.raises(T.T41RxError, match="non-finite coefficient"):
        tx.set_transmit_eq_bands(bad)
    with pytest.raises(ValueError):
        tx.set_transmit_eq(1, [100] * 13)
    with pytest.raises(ValueError):
        tx.set_transmit_eq_bands(np.zeros((14, 4, 4), np.float32))
    on, lv = tx.get_transmit_eq()
    assert on == 1 and tuple(lv) == M.DEFAULT_LEVELS
    assert_same(run(tx, q1), (ref_on[0][:, :F], ref_on[1][:, :F]), "still on, default levels, the good table")
