"""The stage map (t41rx_set_stage_map): stage S runs on channel c exactly when the context's switch for S is on and bit S
of the channel's mask is set; a channel whose bit is clear is processed as the same channel of a context with S switched
off, S's memory for it stays as it was, and its rows of the detector's and the decoder's results are not written.

Every comparison is bit for bit against contexts WITHOUT a map (stage_map_harness.run_schedule): for a channel whose
effective mask is the stage set S the reference is the same channel of a context whose switches are exactly S, fed the same
input.  For S empty that is the plain context, whose fused kernel stores the audio itself where the mapped context hands
over and stores through launch_back512: tests/test_output_map.py's tap cases hold those two bit-equal, and so do these.
19 channels (the group harness's ragged NCH), 70 where the decoder's 64-lane block or a second Xanr() workgroup matters;
3 frames per call (1 as well where the blanker's ping-pong carry is the subject), 3 or 4 calls per stream.
"""
import ctypes as C

import numpy as np
import pytest

import siggen
import stage_map_harness as H
from group_harness import NCH, STREAM_OF
from rx_harness import ERR_ARG, ERR_UNSUPPORTED, T, refused, same  # noqa: F401  (T: a fixture)
from stage_map_harness import ALL, CASES, DEC, DET, EQ, L, NB, NR, run_schedule
from stage_reference import interp

pytestmark = pytest.mark.gpu

# a ragged subset: channel 0, the last channel, and of the neighbours 3 | 4 and 16 | 17 | 18 one each side
LISTED = np.array([0, 3, 7, 8, 12, 18])
assert LISTED[-1] == NCH - 1


def masks(case, listed, nch=NCH, rest=0):
    """every channel ALL but for the case's bits, which the listed channels carry whole and the others as `rest`"""
    clear = case.bits | (DEC if case.bits & DET else 0)  # (no decoder without the detector: the setter's rule)
    m = np.full(nch, (ALL & ~clear) | rest, np.uint32)
    m[np.asarray(listed)] = ALL
    return m


# ---- 1. each stage alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eq", "kim", "spectral", "lms", "notch", "lms-notch", "blanker", "detector", "decoder"])
def test_each_stage_alone(T, name):
    case = CASES[name]
    m = masks(case, LISTED)
    if name == "decoder":  # three kinds of channel: detector and decoder, the detector alone, neither
        m[[1, 4, 17]] = (ALL & ~DEC)
    assert (m[LISTED] == ALL).all() and not (m[16] & case.bits)
    a, eff, audio, _ = run_schedule(T, case, [None, m, m], 6 if name == "decoder" else 3)
    assert len({tuple(eff[:, c]) for c in range(NCH)}) == (3 if name == "decoder" else 2)
    if name == "decoder":
        # the stream keys the carrier: a listed channel's histograms took a call (the wave serves it in the frame loop)
        hist = H.sections(a)["cwdec"][:, 32:32 + 768]  # signalHistogram (cw_kernels.hpp: kCwDecOffSig, kCwDecSigWords)
        assert hist[LISTED].any(), "no listed channel's signal histogram took an entry: the decoder's served calls went untested"


# ---- 2. mixed masks in one context -----------------------------------------------------------------------------------------
def test_mixed_masks_in_one_context(T):
    """equalizer, notch and blanker on; the channels carry each of the eight combinations, two and more channels each"""
    case = CASES["eq-notch-blanker"]
    combo = np.array([(5 * c + 3) % 8 for c in range(NCH)], np.uint32)  # 3 0 5 2 7 4 1 6 3 ..: neighbours differ
    assert all((combo == k).sum() >= 2 for k in range(8))
    m1 = (ALL & ~case.bits) | combo
    m2 = (ALL & ~case.bits) | combo[::-1]  # and another assignment in the next call
    a, eff, _, _ = run_schedule(T, case, [None, m1, m2], 3)
    assert set(eff[1]) == set(range(8))


# ---- 3. list lengths -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,count", [("notch", 1), ("notch", 16), ("notch", 17), ("lms-notch", 17), ("decoder", 64), ("decoder", 65),
                                        ("decoder", 1)])
def test_list_lengths(T, name, count):
    """Xanr()'s workgroup of 16 columns: a list of 17 has a workgroup with one live column, whose dead lanes shadow the
    last LISTED channel; the decoder's block of 64 lanes: a list of 65 has a block with one live lane"""
    nch = 70
    listed = np.array([37]) if count == 1 else np.unique(np.round(np.linspace(0, nch - 1, count)).astype(int))
    assert listed.size == count
    case = CASES[name]
    run_schedule(T, case, [None, masks(case, listed, nch), masks(case, listed, nch)], 6 if name == "decoder" else 3, nch=nch)


# ---- 4. the empty list -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["eq", "spectral", "lms-notch", "blanker", "decoder", "eq-notch-blanker"])
def test_empty_list(T, name):
    """a stage on and nobody listed: the call answers T41RX_OK and launches nothing for the stage (a grid of zero blocks
    would be a launch error); audio as with the stage off, every record of the stage untouched (the engine holds both)"""
    case = CASES[name]
    nobody = np.full(NCH, ALL & ~case.bits, np.uint32)
    run_schedule(T, case, [None, nobody, nobody, None], 3)


# ---- 5. off and on again across calls ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfr", [1, 3])
@pytest.mark.parametrize("name", ["eq", "blanker"])
def test_off_and_on_again(T, name, nfr):
    """on in call 1, off in call 2, on in call 3 (call 0: no map).  Bit for bit the context that switches the stage off
    and on for every channel (the engine), and the stage model run over the blocks of calls 0, 1 and 3 only with its
    memory carried over the gap, at the bar the stage's own off / on test holds that model to (1e-5 block-relative:
    tests/test_receive_eq.py, tests/test_noise_blanker.py).  The blanker is trap 1: its carry ping-pongs between two
    slots and the slot flips for the whole context in call 2, which the bypassed channels must survive -- with one frame
    per call the flip happens every frame.  A checkpoint behind call 2, restored in a fresh context with the same map,
    continues identically."""
    case = CASES[name]
    gap = np.array([0, 4, 5, 11, 18])  # off in call 2
    everyone = np.full(NCH, ALL, np.uint32)
    off = everyone.copy()
    off[gap] &= ~np.uint32(case.bits)
    a, eff, audio, taps = run_schedule(T, case, [None, everyone, off, everyone], nfr, tap=True, checkpoint_after=2, seed=24)
    got, pre = np.concatenate(audio, axis=1), np.concatenate(taps, axis=1)
    pick = np.array([0, 5, 18, 7])  # three with the gap, one without
    on = np.ones((NCH, 4 * nfr), bool)
    on[gap, 2 * nfr:3 * nfr] = False
    want = np.empty((pick.size, 4 * nfr * L), np.float32)
    for i, c in enumerate(pick):
        if name == "eq":
            import test_receive_eq as E
            a24 = E.stage24(pre[c:c + 1], case.kw, E.RAMP, on=on[c])
        else:
            import test_noise_blanker as NBT
            a24, _, pos = NBT.stage24(pre[c:c + 1], case.kw, on=on[c])
        want[i] = interp(a24, case.kw)[0]
    e = siggen.block_rel_err(got[pick], want, L)
    print(name, nfr, "frames per call: max block-relative error against the stage model %.2e" % e.max())
    assert e.max() <= 1e-5, (e.max(), np.unravel_index(e.argmax(), e.shape))


# ---- 6. composition --------------------------------------------------------------------------------------------------------
OMAP = np.array([-1, 7, -1, 0, 9, -1, -1, 2, -1, 5, -1, 1, -1, -1, 8, -1, 3, -1, 6], np.int32)  # tests/test_output_map.py's
VARIANTS = {
    "input-map": dict(imap=STREAM_OF),
    "output-map": dict(omap=OMAP, nrows=10),
    "24k": dict(rate=24000),
    "q15": dict(q15=True),
    "time-major": dict(layout="time"),
    "host": dict(host=True),
    "all-at-once": dict(imap=STREAM_OF, omap=OMAP, nrows=10, rate=24000, q15=True, layout="time", host=True),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_composition(T, variant):
    """none of the other maps, rates, layouts, formats and entries sees the stage map: a call where every mask is
    STAGE_ALL is the call without a map, and a mixed map is the per-combination references, under each of them"""
    case = CASES["eq-blanker"]
    combo = np.array([[EQ | NB, NB, 0, EQ][k % 4] for k in range(NCH)], np.uint32)
    mixed = (ALL & ~case.bits) | combo
    everyone = np.full(NCH, ALL, np.uint32)
    a, eff, _, _ = run_schedule(T, case, [None, everyone, mixed], 3, **VARIANTS[variant])
    assert set(eff[2]) == {0, EQ, NB, EQ | NB} and (eff[1] == case.bits).all()


# ---- 7. refusals, reset, removal -------------------------------------------------------------------------------------------
def test_refusals(T):
    case = CASES["eq"]
    rx = H.context(T, case, 3, NCH)
    good = masks(case, LISTED)
    rx.set_stage_map(good)
    refused(lambda: rx.set_stage_map(good[:-1]), ERR_ARG, "n (18) must equal n_channels", "n_channels 19")
    refused(lambda: rx.set_stage_map(np.append(good, 0).astype(np.uint32)), ERR_ARG, "n (20) must equal n_channels")
    bad = good.copy()
    bad[5] = 32
    refused(lambda: rx.set_stage_map(bad), ERR_ARG, "channel 5", "mask 32", "bits outside T41RX_STAGE_ALL")
    bad[5] = DEC | EQ
    refused(lambda: rx.set_stage_map(bad), ERR_ARG, "channel 5", "T41RX_STAGE_CW_DECODE without T41RX_STAGE_CW_DETECT")
    assert rx._lib.t41rx_set_stage_map(rx._ctx, None, 3) == ERR_ARG and b"takes n 0" in rx._lib.t41rx_last_error()
    with pytest.raises(ValueError):
        rx.set_stage_map(good.astype(np.float32))
    with pytest.raises(ValueError):
        rx.set_stage_map(-good.astype(np.int64))
    assert np.array_equal(rx.stage_map, good), "a refused map must leave the previous one whole"
    # the getter: n, and STAGE_ALL in every entry without a map
    out = np.zeros(NCH, np.uint32)
    p = out.ctypes.data_as(C.POINTER(C.c_uint32))
    assert rx._lib.t41rx_get_stage_map(rx._ctx, p, NCH - 1) == ERR_ARG
    assert rx._lib.t41rx_get_stage_map(rx._ctx, p, NCH) == 1 and np.array_equal(out, good)
    assert rx._lib.t41rx_get_stage_map(rx._ctx, None, 0) == 1
    rx.set_stage_map(None)
    assert rx.stage_map is None and rx._lib.t41rx_get_stage_map(rx._ctx, p, NCH) == 0 and (out == ALL).all()
    # the long FFT lengths: the stages themselves refuse there
    long_rx = T.RxChain(4, T.default_params(fft_length=1024), NCOFreq=siggen.nco_grid(4))
    refused(lambda: long_rx.set_stage_map(np.full(4, ALL, np.uint32)), ERR_UNSUPPORTED, "fft_length 512")
    long_rx.set_stage_map(None)  # (removing what is not there is no refusal)
    assert long_rx.stage_map is None
    # a bit for a stage that is off in the context is allowed and has no effect
    plain, ref = H.context(T, case, 3, NCH), H.context(T, case, 3, NCH)
    plain.set_stage_map(np.full(NCH, DET | DEC | NR, np.uint32))
    I, Q = H.signal(case, NCH, 3, 9, siggen.nco_grid(NCH, seed=11))
    assert same(H.one_call(plain, I, Q)[0], H.one_call(ref, I, Q)[0]) and np.array_equal(plain.get_state(), ref.get_state())


def test_map_survives_reset_and_removal_restores_the_parents_launches(T):
    case = CASES["eq-blanker"]
    a, b = H.context(T, case, 3, NCH), H.context(T, case, 3, NCH)
    for rx in (a, b):
        H.switch(rx, case, case.bits, 3)
    m = masks(case, LISTED)
    a.set_stage_map(m)
    nbytes = a._lib.t41rx_state_bytes(a._ctx)
    I, Q = H.signal(case, NCH, 6, 5, siggen.nco_grid(NCH, seed=11))
    first = H.one_call(a, I[:, :3 * L], Q[:, :3 * L])[0]
    a.reset()
    assert np.array_equal(a.stage_map, m), "the map is configuration: t41rx_reset() keeps it"
    again = H.one_call(a, I[:, :3 * L], Q[:, :3 * L])[0]
    assert same(first, again), "reset: every channel's memories at power-on, listed or not"
    a.set_state(a.get_state())
    a.CalcFilters(FHiCut=9000)
    assert np.array_equal(a.stage_map, m)
    a.CalcFilters(FHiCut=case.kw["FHiCut"])
    # removal: from power-on the context without a map and the one that had one are the same context again
    a.set_stage_map(None)
    a.reset()
    for k in range(2):
        sl = slice(3 * k * L, 3 * (k + 1) * L)
        assert same(H.one_call(a, I[:, sl], Q[:, sl])[0], H.one_call(b, I[:, sl], Q[:, sl])[0])
    assert np.array_equal(a.get_state(), b.get_state())
    assert a._lib.t41rx_state_bytes(a._ctx) == b._lib.t41rx_state_bytes(b._ctx) >= nbytes  # the map has no state
