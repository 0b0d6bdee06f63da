"""CW receive: the Morse decoder behind the tone detector (DoCWDecoding() and its histograms, CWProcessing.cpp:365-371,
:501-815) as a HIP stage: cw_decode_kernel against its restatement (tests/cw_decode_model.py).

CPU: the restatement on ideal keying (texts and the frames in which the histograms run), one-frame blips, the entry
points, the tree fixture against the firmware's literal (where a reference tree is present), and the coverage condition:
the prepared case the GPU runs makes the model take every branch.

GPU (-m gpu): USB with xmtMode = CW; the I/Q is a carrier keyed by whole frames, built call by call; the model is fed
with the GPU's own `combinedCoeff > 50` per frame (the detector is pinned by test_cw_receive.py) and every d_text word
and every word of the checkpoint section is compared with np.array_equal.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cw_decode_model as DM
import cw_model as CWM
import siggen
from rx_harness import assert_entry_points, one_call, refused

L = 2048
CW = dict(mode=0, xmtMode=1)  # USB, xmtMode = CW_MODE
NEW = ("t41rx_set_cw_decode_tree", "t41rx_set_cw_decoder", "t41rx_get_cw_decoder", "t41rx_set_cw_clock",
       "t41rx_reset_cw_histograms")
MESSAGE = "CQ DE T41 5 TEST"
CLOCK = (0, 33, 1)  # 33 ms per frame: 3 frames per dit are 99 ms, inside the decoder's power-on windows
SEC_BYTES = 4 * DM.WORDS


# ---- CPU ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("unit,num,events", [(3, 33, [174, 354]), (4, 25, [232, 472])])
def test_model_decodes_ideal_keying(unit, num, events):
    """3 frames per dit at 33 ms per frame and 4 at 25 ms: the message comes back, and the histograms run in the first
    signal end past every 5000 ms (both calls are DoSignalHistogram(): the gaps of that moment are out of range)"""
    key = DM.keying(MESSAGE, unit, lead=3 * unit, tail=12 * unit)
    assert len(key) == (453 if unit == 3 else 604)
    text, out, dec = DM.decode(key, num=num, den=1)
    assert text == MESSAGE + " "
    assert [n for n, _ in dec.events] == events and {k for _, k in dec.events} == {"signal"}
    assert all(DM.millis(n, 0, num, 1) == num * n > 5000 * (k + 1) for k, n in enumerate(events))
    # from power-on the first call meets a histogram that holds nothing but its dah: the all-zero dit range yields its
    # last index, and so does the window of 7 around the dah (`>=`)
    first = DM.decode(key[:events[0] + 1], num=num, den=1)[2]
    assert first.signalElapsedTime == 3 * num * unit and first.dahLength == 3 * num * unit + 3
    assert first.ditLength == int(first.thresholdGeometricMean) - 1 - 2
    assert out[-1, 1] == dec.ditLength and (out[:events[0], 1] == 80).all()


def test_model_ignores_one_frame_blips():
    """the default clock (32 / 3 ms per frame), 8 frames per dit: single keyed frames are 10 or 11 ms, below
    LOWEST_ATOM_TIME, and print nothing"""
    key = DM.keying("TEST 5", 8, lead=24, tail=96)
    text, out, dec = DM.decode(key)
    assert text == "TEST 5 " and dec.events == []
    blips = key.copy()
    quiet = [f for f in range(4, len(key) - 4) if not key[f - 4:f + 5].any()]
    for f in quiet[::9]:
        blips[f] = 1
    assert blips.sum() >= key.sum() + 8
    text2, out2, dec2 = DM.decode(blips)
    assert text2 == text and dec2.events == []
    assert {DM.millis(n + 1) - DM.millis(n) for n in range(300)} == {10, 11}
    assert np.array_equal(out2[:, 1], out[:, 1])


def test_entry_points_declared_exported_and_bound(built):
    import t41_sdr_amd._lib as lib
    assert_entry_points(NEW, ("set_cw_decode_tree", "set_cw_decoder", "cw_decoder", "cw_text", "set_cw_clock", "reset_cw_histograms"),
                        abi_version=5, pattern=r"T41RX_API\s+int\s+%s\s*\(")
    assert lib.load().t41rx_abi_version() == 5


def test_tree_fixture_is_the_firmware_literal():
    t = DM.tree()
    assert t.dtype == np.uint8 and t.shape == (DM.TREE_CHARS,)
    s = bytes(t).decode("ascii")
    assert s[0] == "-" and s[1] == "E" and s[64] == "T" and s[2] == "I" and s[96] == "M"  # dit: + 1, dah: + the halved jump
    # (the firmware sources: T41_REFERENCE, or the place include/t41rx.h cites its file:line references from)
    src = os.path.join(os.environ.get("T41_REFERENCE", "/root/reference/software/T41_SDR"), "CWProcessing.cpp")
    if not os.path.exists(src):
        pytest.skip("no reference tree here")
    m = re.search(r'bigMorseCodeTree\s*=\s*\(char \*\)"([^"]*)"', open(src).read())
    assert m and m.group(1) == s


# The prepared case: what reaches the decoder's deep states without thousands of frames.  Every channel starts from a
# checkpoint with oldTime = -6000 (the next edge in range runs a histogram), n = 3 (not 0: the frame with n == 0 would
# set oldTime), both histograms filled with counts 0 .. 40, its own averages, and by kind (channel % 7):
#   0  value reference 99 waiting, a dah first: DoSignalHistogram(), averaging with the dit first
#   1  value reference 297 waiting, a dit first: DoSignalHistogram(), averaging with the dah first
#   2  the last signal ended 80 ms before the first one here: DoGapHistogram(), atom branch
#   3  ... 220 ms before: DoGapHistogram(), character-gap branch
#   4  a character in progress at index 200, past the tree: state 5 prints '-'
#   5  silence: no histogram call at all
#   6  slow keying behind it -- averages 300 and 400, thresholdGeometricMean 346 -- and the last signal 800 ms back:
#      DoGapHistogram() on a word past the 750 that are scaled (gapLen runs up to 3 * thresholdGeometricMean)
# Channels of one kind are keyed alike, so several have their call in the same frame.  5000 ms later (frame 152 or so)
# the histograms run a second time.
TEXTS = ("TEAM SET NINE TIMES", "EAT MEAT IN TENTS", "TEN TEA MEN SIT", "NET SITE TEAM", "TIME TEST SENT", "", "TEN TEA MEN SIT")
LEADS = (2, 2, 2, 2, 8, 0, 2)
KINDS = len(TEXTS)
N0 = 3


def prepared_case(nch, nfr, seed=5):
    rng = np.random.default_rng(seed)
    words = np.zeros((nch, DM.WORDS), np.int32)
    keys = np.zeros((nch, nfr), np.int32)
    for c in range(nch):
        kind = c % KINDS
        d = DM.Decoder()
        d.n = N0
        d.oldTime = -6000
        d.aveDitLength, d.aveDahLength = (300 + c % 3, 400 + c % 5) if kind == 6 else (80 + c % 7, 240 + c % 5)
        d.thresholdGeometricMean = np.float32(np.sqrt(float(d.aveDitLength * d.aveDahLength)))
        d.sig = [int(v) for v in rng.integers(0, 41, DM.SIG_WORDS)]
        d.gap = [int(v) for v in rng.integers(0, 41, DM.GAP_WORDS)]
        t_on = CLOCK[1] * (N0 + LEADS[kind])
        if kind in (0, 1):
            d.valFlag, d.valRef1, d.signalStartOld = 1, (99, 297)[kind], -6000
            d.signalEnd = t_on + 50  # a gap of -50 ms: no DoGapHistogram() in front of the signal, and gapRef1 below any bound
        elif kind in (2, 3):
            d.signalEnd = t_on - (80, 220)[kind - 2]
        elif kind == 6:
            d.signalEnd = t_on - 800
        elif kind == 4:
            d.currentDecoderIndex, d.charProcessFlag, d.currentDashJump, d.signalEnd = 200, 1, 4, -1000
        words[c] = d.words()
        k = DM.keying(TEXTS[kind], 3, lead=LEADS[kind], tail=nfr) if TEXTS[kind] else np.zeros(nfr, np.int32)
        keys[c] = k[:nfr]
    return words, keys


def run_model(words, keys, clock=CLOCK, clock_at=None):
    """the restatement over [nch][nfr] key bits from the section's words: (text words [nch][nfr][2], words behind, the
    decoders); clock_at = (frame, clock): the clock changes there"""
    nch, nfr = keys.shape
    text, behind, decs = np.zeros((nch, nfr, 2), np.int32), np.zeros_like(words), []
    for c in range(nch):
        d = DM.Decoder(t0=clock[0], num=clock[1], den=clock[2]).load(words[c])
        for f in range(nfr):
            if clock_at is not None and f == clock_at[0]:
                d.clock = clock_at[1]
            ch, dit = d.frame(int(keys[c, f]))
            text[c, f] = (ch, DM.i32(dit))
        behind[c] = d.words()
        decs.append(d)
    return text, behind, decs


def power_on_words(nch):
    return np.tile(DM.Decoder().words(), (nch, 1))


def test_prepared_case_takes_every_branch():
    """the coverage condition, on the model alone: the inputs of test_gpu_short_stream_from_a_prepared_checkpoint"""
    words, keys = prepared_case(67, 176)
    _, _, decs = run_model(words, keys)
    total = {b: sum(d.count[b] for d in decs) for b in DM.BRANCHES}
    print(total)
    assert all(v > 0 for v in total.values()), total
    frames = {}
    for c, d in enumerate(decs):
        for n, _ in d.events:
            frames.setdefault(n, []).append(c)
    assert max(len(v) for v in frames.values()) >= 8  # several channels in one frame
    assert all(not d.events for c, d in enumerate(decs) if c % KINDS == 5)  # others in none
    assert all(len(d.events) == 2 for c, d in enumerate(decs) if c % KINDS < 4)
    assert all(d.events[0][1] == "gap" and d.gapLength >= 0 for c, d in enumerate(decs) if c % KINDS == 6)


# ---- GPU ---------------------------------------------------------------------------------------------------------------
# The carrier's level.  The path delays the tone by most of a frame and the detector averages two blocks: a keyed run of
# k frames reaches the detector as about 5 %, 67 %, 100 % .. 100 %, 59 %, 0 % of the steady combinedCoeff (measured on the
# device at several levels; the figure goes with the square of the amplitude).  A strong carrier (0.3: steady 2.5e6) is
# above 50 in every one of those frames and every signal comes out two frames longer, every gap two shorter -- at 3
# frames per dit that turns dits into dahs.  At 0.003 the steady figure is 250, five times the threshold: 14 < 50 < 147,
# so a frame counts as keyed when the tone fills more than about half of the detector's block, and a run of k keyed
# frames is seen as k frames, one frame late.  The noise sits 43 dB below the carrier.
AMP, NOISE = 0.003, 2e-5


def call_iq(nco, keys, first, seed, amp=AMP, noise=NOISE):
    """the I/Q of one call: frames first .. first + keys.shape[1] of a carrier that lands on 750 Hz of audio, keyed by
    whole frames (a frame is one detector block), phase-continuous over the calls, plus noise"""
    nch, nfr = keys.shape
    n = np.arange(first * L, (first + nfr) * L)
    I = np.empty((nch, nfr * L), np.float32)
    Q = np.empty_like(I)
    for c in range(nch):
        rng = np.random.default_rng([seed, first, c])
        f = siggen.passband_tone_hz(0, nco[c], 0.0)  # (CW mode moves the NCO by the side tone)
        z = amp * np.repeat(keys[c], L) * np.exp(2j * np.pi * f / 192000.0 * n)
        I[c] = z.real + noise * rng.standard_normal(n.size)
        Q[c] = z.imag + noise * rng.standard_normal(n.size)
    return I, Q


def make_rx(nch, nco, frames, dec=1, det=1, kw=CW, clock=CLOCK):
    import t41_sdr_amd as T
    rx = T.RxChain(nch, T.default_params(**kw), NCOFreq=nco)
    rx.set_cw_tables(*CWM.tables())
    rx.set_cw_decode_tree(DM.tree())
    if det:
        rx.set_cw_detector(1, frames)
    if dec:
        rx.set_cw_decoder(1, frames)
    rx.set_cw_clock(*clock)
    return rx


def run(rx, nco, keys, edges, seed, how="f32", keep_audio=False):
    """the stream in calls of frames edges[k] .. edges[k + 1]: (GPU key bits, d_cw, d_text, audio or None)"""
    dets, texts, auds = [], [], []
    for a, b in zip(edges[:-1], edges[1:]):
        I, Q = call_iq(nco, keys[:, a:b], a, seed)
        o, _ = one_call(rx, I, Q, layout="time" if how == "time" else "channel", q15_scale=1.0 if how == "q15" else None)
        if keep_audio:
            auds.append(o)
        dets.append(rx.cw_results(b - a).cpu().numpy().copy())
        if rx.cw_decoder:
            texts.append(rx.cw_text(b - a).cpu().numpy().copy())
    det = np.concatenate(dets, 1)
    return ((det[:, :, 3] > np.float32(50)).astype(np.int32), det, np.concatenate(texts, 1) if texts else None,
            np.concatenate(auds, 1) if keep_audio else None)


def dec_section(ck, nch):
    """the decoder's section of a checkpoint: the last one"""
    assert ck[:32].view(np.int32)[5] & 32
    return ck[-SEC_BYTES * nch:].view(np.int32).reshape(nch, DM.WORDS)


def with_sections(rx, words):
    """a checkpoint of context rx (no section yet) with the CW section at power-on and the decoder's section = words"""
    ck = rx.get_state()
    assert ck[:32].view(np.int32)[5] == 0
    ck = np.concatenate([ck, np.zeros(4 * 128 * rx.n_channels, np.uint8), np.ascontiguousarray(words, np.int32).view(np.uint8).reshape(-1)])
    ck[:32].view(np.int32)[5] = 16 | 32
    return ck


def printed(text_words):
    return "".join(chr(c) for c in text_words[:, 0] if c)


@pytest.mark.gpu
@pytest.mark.parametrize("unit,clock,nfr,edges", [(3, (0, 33, 1), 453, [0, 1, 8, 72, 73, 200, 453]),
                                                  (4, (0, 25, 1), 604, [0, 1, 8, 72, 73, 200, 453, 604])])
def test_gpu_long_stream(built, unit, clock, nfr, edges):
    """5 channels from power-on in ragged calls: four messages and a channel of noise.  Every word against the model; the
    clean channels print what was sent.

    3 frames per dit run at 33 ms per frame over 453 frames, 4 frames per dit at 25 ms over 604 frames -- the two pairs the
    restatement decodes on ideal keying (test_model_decodes_ideal_keying).  One context has one clock, and at 33 ms a
    4-frame dit is outside the decoder's power-on windows: its letter gap, 396 ms, is above 4.5 x ditLength = 360 ms, so
    the firmware's state machine prints a blank inside every word, on ideal keying too."""
    sent = [MESSAGE, "TEST DE T41 K", "5 NN CQ T41", "", "T41 TEST 73 E E"]
    nch = len(sent)
    keys = np.zeros((nch, nfr), np.int32)
    for c, msg in enumerate(sent):
        if msg:
            k = DM.keying(msg, unit, lead=3 * unit, tail=nfr)[:nfr]
            assert not k[-12 * unit:].any(), (msg, len(k))  # the message and its last blank fit
            assert DM.decode(k, num=clock[1], den=clock[2])[0] == msg + " "
            keys[c] = k
    nco = siggen.nco_grid(nch, seed=81)
    rx = make_rx(nch, nco, max(b - a for a, b in zip(edges[:-1], edges[1:])), clock=clock)
    got_keys, det, text, _ = run(rx, nco, keys, edges, seed=81)
    want, behind, decs = run_model(power_on_words(nch), got_keys, clock=clock)
    for c in range(nch):
        print("channel %d: sent %r printed %r; key bits off the ideal moved by a frame in %d frames; histogram calls %r; ditLength %d"
              % (c, sent[c], printed(text[c]), int((got_keys[c, 1:] != keys[c, :-1]).sum()), decs[c].events, text[c, -1, 1]))
    assert np.array_equal(text, want)
    assert np.array_equal(dec_section(rx.get_state(), nch), behind)
    assert sum(len(d.events) for d in decs) >= 4 and {k for d in decs for _, k in d.events} == {"gap", "signal"}  # the histograms ran
    for c, msg in enumerate(sent):
        if msg:
            assert printed(text[c]) == msg + " ", (c, printed(text[c]))


@pytest.mark.gpu
def test_gpu_short_stream_from_a_prepared_checkpoint(built):
    """67 channels -- one wave of the kernel (a lane per channel) and a ragged three -- over 176 frames from the prepared
    checkpoints: the histogram calls, the scaling passes and every branch of them, several channels in one frame"""
    nch, nfr = 67, 176
    words, keys = prepared_case(nch, nfr)
    nco = siggen.nco_grid(nch, seed=82)
    rx = make_rx(nch, nco, 106)
    rx.set_state(with_sections(rx, words))
    assert np.array_equal(dec_section(rx.get_state(), nch), words)
    got_keys, det, text, _ = run(rx, nco, keys, [0, 5, 69, 70, 176], seed=82)
    want, behind, decs = run_model(words, got_keys)
    total = {b: sum(d.count[b] for d in decs) for b in DM.BRANCHES}
    frames = {}
    for c, d in enumerate(decs):
        for n, _ in d.events:
            frames.setdefault(n - N0, []).append(c)
    print("branches:", total)
    print("histogram calls by frame:", {f: len(v) for f, v in sorted(frames.items())})
    print("key bits off the ideal: %d of %d" % (int((got_keys != keys).sum()), keys.size))
    assert np.array_equal(text, want)
    assert np.array_equal(dec_section(rx.get_state(), nch), behind)
    # the coverage condition on the device's own key bits (they arrive a frame late): every branch, several calls in a frame
    assert all(v > 0 for v in total.values()), total
    assert max(len(v) for v in frames.values()) >= 8


def small_case(nfr=64):
    nch = 7
    words, keys = prepared_case(nch, nfr, seed=9)
    return nch, nfr, words, keys, siggen.nco_grid(nch, seed=83)


@pytest.mark.gpu
def test_gpu_checkpoints(built):
    import t41_sdr_amd as T
    import t41_sdr_amd._lib as lib
    nch, nfr, words, keys, nco = small_case()
    cut = 23
    # the section appears once the decoder has run: a context that ran the detector alone is smaller by exactly it
    rd = make_rx(nch, nco, nfr, dec=0)
    run(rd, nco, keys, [0, 2], seed=83)
    rx = make_rx(nch, nco, nfr)
    before = rx.get_state().size
    run(rx, nco, keys, [0, 2], seed=83)
    assert rd.get_state().size == before + 4 * 128 * nch and rx.get_state().size == before + 4 * 128 * nch + SEC_BYTES * nch
    assert rx.get_state()[:32].view(np.int32)[5] == 16 | 32
    # reset gives power-on
    rx.reset()
    assert np.array_equal(dec_section(rx.get_state(), nch), power_on_words(nch))
    # mid-stream: get, set into a fresh context, both continue identically (and as the model says)
    rx.set_state(with_sections(make_rx(nch, nco, nfr), words))
    k1, _, t1, _ = run(rx, nco, keys, [0, cut], seed=83)
    ck = rx.get_state()
    ry = make_rx(nch, nco, nfr)
    ry.set_state(ck)
    k2, _, t2, _ = run(rx, nco, keys, [cut, nfr], seed=83)
    k2y, _, t2y, _ = run(ry, nco, keys, [cut, nfr], seed=83)
    assert np.array_equal(t2, t2y) and np.array_equal(k2, k2y) and np.array_equal(rx.get_state(), ry.get_state())
    want, behind, decs = run_model(words, np.concatenate([k1, k2], 1))
    assert np.array_equal(np.concatenate([t1, t2], 1), want) and np.array_equal(dec_section(rx.get_state(), nch), behind)
    assert sum(len(d.events) for d in decs) >= 4
    # t41rx_reset_cw_histograms() with a mask: the masked channels only, and only what ResetHistograms() names
    sec = dec_section(rx.get_state(), nch).copy()
    mask = np.array([1, 0, 1, 0, 0, 0, 1], np.uint8)
    rx.reset_cw_histograms(mask)
    after = dec_section(rx.get_state(), nch)
    expect = sec.copy()
    for c in np.flatnonzero(mask):
        d = DM.Decoder().load(sec[c])
        d.reset_histograms()
        expect[c] = d.words()
    assert np.array_equal(after, expect) and not np.array_equal(after[0], sec[0]) and np.array_equal(after[1], sec[1])
    named = [DM.W[k] for k in DM.RESET_SCALARS]
    changed = np.flatnonzero((after != sec).any(0))
    assert set(changed) <= set(named) | set(range(DM.OFF_SIG, DM.OFF_SIG + 750)) | set(range(DM.OFF_GAP, DM.OFF_GAP + 750))
    assert (after[0, DM.OFF_GAP + 750:] == sec[0, DM.OFF_GAP + 750:]).all() and sec[0, DM.OFF_GAP + 750:].any()
    rx.reset_cw_histograms()  # NULL: all channels
    allc = dec_section(rx.get_state(), nch)
    assert (allc[:, DM.OFF_SIG:DM.OFF_SIG + 750] == 0).all() and (allc[:, DM.W["ditLength"]] == 80).all()
    assert np.array_equal(allc[:, DM.W["n"]], sec[:, DM.W["n"]]) and np.array_equal(allc[:, DM.W["decodeStates"]], sec[:, DM.W["decodeStates"]])
    # the refusals: every word the kernel indexes or loops with
    good = with_sections(make_rx(nch, nco, nfr), words)
    rz = make_rx(nch, nco, nfr)
    rz.set_state(good)
    nanbits = int(np.array([np.nan], np.float32).view(np.int32)[0])
    infbits = int(np.array([np.inf], np.float32).view(np.int32)[0])
    fbits = lambda v: int(np.array([v], np.float32).view(np.int32)[0])  # noqa: E731
    bad_words = [("decodeStates", 3), ("decodeStates", 7), ("decodeStates", -1), ("currentDecoderIndex", -1), ("currentDecoderIndex", 256),
                 ("currentDashJump", 129), ("currentDashJump", -1), ("thresholdGeometricMean", nanbits),
                 ("thresholdGeometricMean", infbits), ("thresholdGeometricMean", fbits(0.5)), ("thresholdGeometricMean", fbits(750.0)),
                 ("aveDitLength", -1), ("aveDahLength", 32768), ("valFlag", 2), ("valFlag", -1),
                 ("valRef1", -1), ("valRef1", 32768), ("valRef2", -1), ("valRef2", 32768), ("charProcessFlag", 2), ("charProcessFlag", -1),
                 ("blankFlag", 2), ("blankFlag", -1),
                 (DM.OFF_SIG + 700, -1), (DM.OFF_GAP + 2303, (1 << 27) + 1), (DM.OFF_GAP + 5, -3)]
    for name, v in bad_words:
        bad = good.copy()
        dec_section(bad, nch)[nch - 2, DM.W[name] if isinstance(name, str) else name] = v
        with pytest.raises(T.T41RxError) as ei:
            rz.set_state(bad)
        assert ei.value.status == lib.ERR_STATE and "CW decoder" in str(ei.value), (name, v, ei.value)
    assert np.array_equal(rz.get_state(), good)  # a refused checkpoint changes nothing
    edge = good.copy()  # the ends of the ranges pass
    w = dec_section(edge, nch)[0]
    w[DM.W["currentDecoderIndex"]], w[DM.W["currentDashJump"]], w[DM.W["aveDahLength"]] = 255, 128, 32767
    w[DM.W["thresholdGeometricMean"]], w[DM.OFF_GAP + 2303] = fbits(1.0), 1 << 27
    rz.set_state(edge)


@pytest.mark.gpu
def test_gpu_gating_and_refusals(built):
    import torch
    import t41_sdr_amd as T
    import t41_sdr_amd._lib as lib
    L_ = lib.load()
    nch, nfr, words, keys, nco = small_case()

    # gating: another xmtMode, or the detector off: d_text untouched, the section unchanged
    rx = make_rx(nch, nco, nfr)
    rx.set_state(with_sections(rx, words))
    run(rx, nco, keys, [0, 9], seed=84)
    sec = dec_section(rx.get_state(), nch).copy()
    assert not np.array_equal(sec, words)
    buf = rx.cw_text(nfr)
    for off in ("xmtMode", "detector"):
        if off == "xmtMode":
            rx.CalcFilters(xmtMode=0)
        else:
            rx.set_cw_detector(0)
        assert rx.cw_decoder == 1  # the setting is kept
        buf.fill_(-7)
        I, Q = call_iq(nco, keys[:, 9:20], 9, 84)
        rx.ProcessIQData(torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda())
        assert (buf == -7).all().item(), off
        assert np.array_equal(dec_section(rx.get_state(), nch), sec), off
        if off == "xmtMode":
            rx.CalcFilters(xmtMode=1)
        else:
            rx.set_cw_detector(1, nfr)
    # the switches, the tree and the clock survive set_params / set_coeffs; the stream goes on as the model's, which saw
    # no frame in between
    rx.set_coeffs(rx.coeffs())
    k2, _, t2, _ = run(rx, nco, keys, [20, 40], seed=84)
    want, behind, _ = run_model(sec, k2)
    assert np.array_equal(t2, want) and np.array_equal(dec_section(rx.get_state(), nch), behind)
    # the clock: t41rx_set_cw_clock() from the next call on, the frame counter untouched
    rc = make_rx(nch, nco, nfr)
    rc.set_state(with_sections(rc, words))
    ka, _, ta, _ = run(rc, nco, keys, [0, 30], seed=84)
    rc.set_cw_clock(-40, 47, 2)
    kb, _, tb, _ = run(rc, nco, keys, [30, nfr], seed=84)
    kk = np.concatenate([ka, kb], 1)
    want, behind, _ = run_model(words, kk, clock_at=(30, (-40, 47, 2)))
    assert np.array_equal(np.concatenate([ta, tb], 1), want) and np.array_equal(dec_section(rc.get_state(), nch), behind)
    assert not np.array_equal(want, run_model(words, kk)[0])  # (the change is seen)
    assert np.array_equal(behind[:, DM.W["n"]], np.full(nch, N0 + nfr))
    # the argument refusals
    r = T.RxChain(nch, T.default_params(**CW))
    r.set_cw_tables(*CWM.tables())
    t = torch.zeros(nch, 4, 2, dtype=torch.int32, device="cuda")
    ptr = C.c_void_p(t.data_ptr())
    assert r.cw_decoder == 0
    assert L_.t41rx_set_cw_decoder(r._ctx, 1, ptr, 4) == lib.ERR_ARG and b"tree" in L_.t41rx_last_error()  # before the tree
    tree = DM.tree()
    tp = tree.ctypes.data_as(C.c_void_p)
    assert L_.t41rx_set_cw_decode_tree(r._ctx, tp, 128) == lib.ERR_ARG and L_.t41rx_set_cw_decode_tree(r._ctx, tp, 130) == lib.ERR_ARG
    assert L_.t41rx_set_cw_decode_tree(r._ctx, None, 129) == lib.ERR_ARG and L_.t41rx_set_cw_decode_tree(None, tp, 129) == lib.ERR_ARG
    assert L_.t41rx_set_cw_decoder(r._ctx, 1, ptr, 4) == lib.ERR_ARG  # (the refused calls loaded nothing)
    r.set_cw_decode_tree(bytes(tree))
    assert L_.t41rx_set_cw_decoder(r._ctx, 2, ptr, 4) == lib.ERR_ARG and L_.t41rx_set_cw_decoder(r._ctx, -1, ptr, 4) == lib.ERR_ARG
    assert L_.t41rx_set_cw_decoder(r._ctx, 1, None, 4) == lib.ERR_ARG and b"NULL" in L_.t41rx_last_error()
    assert L_.t41rx_set_cw_decoder(r._ctx, 1, ptr, 0) == lib.ERR_ARG and L_.t41rx_set_cw_decoder(None, 1, ptr, 4) == lib.ERR_ARG
    assert L_.t41rx_get_cw_decoder(None) == lib.ERR_ARG
    assert L_.t41rx_set_cw_clock(r._ctx, 0, -1, 3) == lib.ERR_ARG and L_.t41rx_set_cw_clock(r._ctx, 0, 32, 0) == lib.ERR_ARG
    assert L_.t41rx_set_cw_clock(None, 0, 32, 3) == lib.ERR_ARG and L_.t41rx_reset_cw_histograms(None, None, 0) == lib.ERR_ARG
    m = np.ones(nch + 1, np.uint8)
    assert L_.t41rx_reset_cw_histograms(r._ctx, m.ctypes.data_as(C.c_void_p), nch + 1) == lib.ERR_ARG
    assert L_.t41rx_set_cw_decoder(r._ctx, 1, ptr, 4) == 0 and r.cw_decoder == 1
    r.set_cw_detector(1, 8)
    z = torch.zeros(nch, 5 * L, device="cuda")
    refused(lambda: r.ProcessIQData(z, z), lib.ERR_ARG, "max_frames", "decoder")  # more frames than the text buffer holds
    assert not r.get_state()[:32].view(np.int32)[5] & 32  # a refused call is not a run: no section yet
    r.ProcessIQData(z[:, :4 * L].contiguous(), z[:, :4 * L].contiguous())
    assert (t.cpu().numpy()[:, :, 0] == 0).all() and (t.cpu().numpy()[:, :, 1] == 80).all()  # silence: no character, ditLength 80
    # fft_length 1024
    rl = T.RxChain(2, T.default_params(fft_length=1024, **CW))
    rl.set_cw_decode_tree(tree)
    refused(lambda: rl.set_cw_decoder(1, 2), lib.ERR_UNSUPPORTED, "fft_length 512")
    rl.set_cw_decoder(0)
    long_ck = rl.get_state()
    with_dec = np.concatenate([long_ck, power_on_words(2).view(np.uint8).reshape(-1)])
    with_dec[:32].view(np.int32)[5] |= 32
    refused(lambda: rl.set_state(with_dec), lib.ERR_STATE, "CW-decoder", "long fft_length")
    rl.set_state(long_ck)


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["f32", "q15", "time"])
def test_gpu_existing_outputs_unmoved(built, how):
    """audio and d_cw with the decoder on are those with it off, bit for bit"""
    nch, nfr, words, keys, nco = small_case(40)
    outs = []
    for dec in (0, 1):
        rx = make_rx(nch, nco, nfr, dec=dec)
        if how == "time":
            rx.set_buffer_layout("time")
        _, det, text, aud = run(rx, nco, keys, [0, 33, nfr], seed=85, how=how, keep_audio=True)
        outs.append((det, aud))
        if dec:
            assert text is not None and (text[:, :, 1] > 0).all()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    assert np.abs(outs[0][1].astype(np.float64)).max() > 0 and (outs[0][0][:, :, 3] > 50).any()
