"""The FT8 map (t41rx_set_ft8_map): FT8 receive only on the channels that ask, a row of d_power / d_status per listed
channel.

GPU (-m gpu).  Every comparison is bit for bit against the library's own path WITHOUT a map, which test_ft8_receive.py holds
to tests/ft8_model.py and test_ft8_audio.py to tests/ft8_audio_model.py: a listed channel's status words, both power halves
and FT8 memory are those of the same channel of the unmapped context, in the row the map names; an unlisted channel's
memory does not move (n included); a row nobody names keeps the 0xA5 it was filled with; the receive path's audio and side
outputs are those with FT8 off.  5 channels from test_ft8_receive._prepared()'s records (classes c % 4: a completion with
the half's flip, a restart, an unsynced channel, a block in frame 0), calls of 7 + 33 frames.
"""
import functools

import numpy as np
import pytest

import ft8_audio_model as A
import ft8_decode_model as D
import ft8_model as M
import siggen
from rx_harness import ERR_UNSUPPORTED, refused, same
from test_ft8_audio_model import TEXT, clone, random_model, recording
from test_ft8_receive import L, Run, _iq, _prepared, _tables

NCH, SPLITS = 5, (7, 33)
MAXF = max(SPLITS)
FILL = 0xA5
FILL32 = np.frombuffer(bytes([FILL] * 4), np.int32)[0]
# row per channel, rows: 1 of 5; 2 of 5 with the rows permuted and row 1 named by nobody; all 5 permuted
MAPS = {"1_of_5": ([-1, -1, -1, 0, -1], 1), "2_of_5": ([-1, 2, -1, -1, 0], 3), "all_5": ([3, 0, 4, 1, 2], 5)}
SEED = 0x4D4150
USB = dict(mode=0, FLoCut=200, FHiCut=3000)
LSB = dict(mode=1, FLoCut=-3000, FHiCut=-200)


def _words(rx):
    return rx.ft8_state().view(np.int32)[8:].reshape(-1, M.WORDS).copy()


def _open(entry="f32", rows=None, n_rows=None, rec=None, nch=NCH, nco=None, on=True, setup=None, **params):
    """a USB context of test_ft8_receive.Run with, in this order, setup(rx), the FT8 map, FT8 receive on with d_power and
    d_status filled with 0xA5, and the record"""
    import torch
    import t41_sdr_amd as T
    run = Run.__new__(Run)  # (Run's process() on a context made here: the map goes in front of the switch)
    run.torch, run.nch, run.entry, run.tap, run.power = torch, nch, entry, None, None
    run.rx = T.RxChain(nch, T.default_params(**dict(USB, **params)), NCOFreq=_iq(nch, sum(SPLITS), seed=SEED)[0] if nco is None else nco)
    if entry == "time":
        run.rx.set_buffer_layout("time")
    run.keep = setup(run.rx) if setup else None
    if rows is not None:
        run.rx.set_ft8_map(rows, n_rows)
    if on:
        run.rx.set_ft8_tables(*_tables())
        run.power, run.status = run.rx.set_ft8(1, MAXF)
        run.power.fill_(FILL)
        if rec is not None:
            run.rx.set_ft8_state(rec)
    return run


def _calls(run, I, Q, splits=SPLITS, between=None):
    """the stream in calls of `splits` frames, d_status filled with 0xA5 in front of each: (audio, [status per call])"""
    f0, audio, status = 0, [], []
    for k, n in enumerate(splits):
        if k and between:
            between(run)
        if run.power is not None:
            run.status.fill_(int(FILL32))
        a, _, st = run.process(I[:, f0 * L:(f0 + n) * L], Q[:, f0 * L:(f0 + n) * L])
        audio.append(a)
        status.append(st)
        f0 += n
    return np.concatenate(audio, axis=1), status


@functools.lru_cache(maxsize=None)
def _reference(entry):
    """the unmapped context on the prepared records: audio, status per call, power, FT8 memory; and the audio with FT8 off"""
    _, I, Q = _iq(NCH, sum(SPLITS), seed=SEED)
    run = _open(entry, rec=_prepared(NCH))
    audio, status = _calls(run, I, Q)
    off = _calls(_open(entry, on=False), I, Q)[0]
    ref = dict(audio=audio, status=status, power=run.power.cpu().numpy(), words=_words(run.rx), off=off)
    for v in [audio, off, ref["power"], ref["words"]] + status:
        v.setflags(write=False)
    # the reference does what the records were prepared for: a completion in channel 0, a block in frame 0 of channel 3
    assert status[1][0, 16 - 7].tolist() == [92, 0, 1, 0] and status[0][3, 0, :3].tolist() == [92, 0, 2] and (ref["power"][2] == FILL).all()
    return ref


def _check(run, status, rows, n_rows, ref, start):
    """listed channels are the reference's in their rows, unlisted ones have not moved, unnamed rows were not written"""
    power, words = run.power.cpu().numpy(), _words(run.rx)
    assert power.shape == (n_rows, 2, M.HALF_BYTES)
    for c, r in enumerate(rows):
        if r >= 0:
            for k, st in enumerate(status):
                assert st.shape[0] == n_rows and np.array_equal(st[r], ref["status"][k][c]), "status of channel %d (row %d), call %d" % (c, r, k)
            assert np.array_equal(power[r], ref["power"][c]), "power of channel %d (row %d)" % (c, r)
            assert np.array_equal(words[c], ref["words"][c]), "FT8 memory of listed channel %d" % c
        else:
            assert np.array_equal(words[c], start[c]), "FT8 memory of unlisted channel %d moved" % c
    for r in sorted(set(range(n_rows)) - {r for r in rows if r >= 0}):
        assert (power[r] == FILL).all() and all((st[r] == FILL32).all() for st in status), "row %d has no channel and was written" % r


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(MAPS))
@pytest.mark.parametrize("entry", ["f32", "q15", "time"])
def test_gpu_listed_channels_equal_the_unmapped_run(entry, which):
    rows, n_rows = MAPS[which]
    _, I, Q = _iq(NCH, sum(SPLITS), seed=SEED)
    rec = _prepared(NCH)
    ref = _reference(entry)
    run = _open(entry, rows, n_rows, rec)
    assert run.rx.ft8_rows == n_rows and run.rx.ft8_map.tolist() == rows
    audio, status = _calls(run, I, Q)
    _check(run, status, rows, n_rows, ref, rec.view(np.int32)[8:].reshape(NCH, M.WORDS))
    assert same(audio, ref["audio"]) and same(audio, ref["off"]), "the receive path's audio moved"


@pytest.mark.gpu
def test_gpu_nobody_listed():
    """a map of -1s: nothing is written, no word of the FT8 memory moves, and the audio is that with FT8 off"""
    _, I, Q = _iq(NCH, sum(SPLITS), seed=SEED)
    rec = _prepared(NCH)
    run = _open("f32", [-1] * NCH, 1, rec)
    audio, status = _calls(run, I, Q)
    assert (run.power.cpu().numpy() == FILL).all() and all((st == FILL32).all() for st in status)
    assert np.array_equal(run.rx.ft8_state(), rec)
    assert same(audio, _reference("f32")["off"])


@pytest.mark.gpu
def test_gpu_map_changes_between_two_calls():
    """3 rows; channel 4 stays listed and moves from row 0 to row 2, channel 1 leaves, channel 0 joins: channel 4 goes on as
    in one unmapped stream -- its second call's status, its memory, and its power bytes, which lie where each call put them"""
    _, I, Q = _iq(NCH, sum(SPLITS), seed=SEED)
    rec = _prepared(NCH)
    ref = _reference("f32")
    run = _open("f32", [-1, 1, -1, -1, 0], 3, rec)
    seen = {}

    def move(r):
        seen["power"] = r.power.cpu().numpy().copy()
        seen["words"] = _words(r.rx)
        r.rx.set_ft8_map([0, -1, -1, -1, 2], 3)

    _, status = _calls(run, I, Q, between=move)
    power, words = run.power.cpu().numpy(), _words(run.rx)
    assert np.array_equal(status[0][0], ref["status"][0][4]) and np.array_equal(status[0][1], ref["status"][0][1])
    assert np.array_equal(status[1][2], ref["status"][1][4]), "channel 4 in its new row"
    assert np.array_equal(words[4], ref["words"][4])
    first, second, want = seen["power"][0] != FILL, power[2] != FILL, ref["power"][4] != FILL
    assert first.any() and second.any() and np.array_equal(first | second, want), "channel 4's blocks: call 1 in row 0, call 2 in row 2"
    assert np.array_equal(seen["power"][0][first], ref["power"][4][first]) and np.array_equal(power[2][second], ref["power"][4][second])
    assert np.array_equal(words[1], seen["words"][1]), "channel 1 left the list: its memory stays as the first call left it"
    assert np.array_equal(seen["words"][0], rec.view(np.int32)[8:].reshape(NCH, M.WORDS)[0]) and words[0, M.S_N] == 1363 + SPLITS[1]


def _eq_on(rx):
    import eq_model
    from test_receive_eq import RAMP
    rx.set_receive_eq_bands(eq_model.bands())
    rx.set_receive_eq(1, RAMP)


def _spectrum(rx):
    import torch
    keep = torch.zeros(NCH, MAXF, 1024, device="cuda"), torch.zeros(NCH, MAXF, 3, device="cuda")
    rx.set_audio_spectrum(*keep)
    return keep


def _muted(rx):
    rx.set_output_map([0, -1, 1, 2, -1], 3)  # the two listed channels have no audio row


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["spectrum", "equalizer", "muted"])
def test_gpu_audio_unmoved(case):
    """audio, the audio spectrum and the path checkpoint with a map of 2 of 5 are those with FT8 off; the listed channels'
    FT8 results are the unmapped context's of the same setup -- with the equalizer on the stage reads the hand-over
    buffer, with the output map the listed channels are muted"""
    setup = dict(spectrum=_spectrum, equalizer=_eq_on, muted=_muted)[case]
    rows, n_rows = MAPS["2_of_5"]
    _, I, Q = _iq(NCH, sum(SPLITS), seed=SEED)
    rec = _prepared(NCH)
    off, plain, mapped = _open(on=False, setup=setup), _open(rec=rec, setup=setup), _open("f32", rows, n_rows, rec, setup=setup)
    got = {}
    for name, run in (("off", off), ("plain", plain), ("mapped", mapped)):
        audio, status = _calls(run, I, Q)
        side = [t.cpu().numpy() for t in run.keep] if run.keep else []
        got[name] = dict(audio=audio, status=status, side=side, state=run.rx.get_state())
    assert got["off"]["audio"].shape[0] == (3 if case == "muted" else NCH) and np.abs(got["off"]["audio"]).max() > 0
    for name in ("plain", "mapped"):
        assert same(got[name]["audio"], got["off"]["audio"]), name
        assert np.array_equal(got[name]["state"], got["off"]["state"]), name
        assert all(same(a, b) for a, b in zip(got[name]["side"], got["off"]["side"])), name
    ref = dict(status=got["plain"]["status"], power=plain.power.cpu().numpy(), words=_words(plain.rx))
    _check(mapped, got["mapped"]["status"], rows, n_rows, ref, rec.view(np.int32)[8:].reshape(NCH, M.WORDS))
    if case != "equalizer":  # (the equalizer splits the chain; the stage's input is the same audio either way)
        assert np.array_equal(ref["power"], _reference("f32")["power"])


@pytest.mark.gpu
@pytest.mark.parametrize("ch", [1, 4])
def test_gpu_isolation(ch):
    """a listed channel's words depend neither on who else is listed nor on its row number: alone in row 0 of 1, alone in
    row 4 of 5, and in row 4 with every other channel listed"""
    _, I, Q = _iq(NCH, sum(SPLITS), seed=SEED)
    rec = _prepared(NCH)
    ref = _reference("f32")
    alone0 = [0 if c == ch else -1 for c in range(NCH)]
    alone4 = [4 if c == ch else -1 for c in range(NCH)]
    others = iter(range(4))
    crowd = [4 if c == ch else next(others) for c in range(NCH)]
    for rows, n_rows in ((alone0, 1), (alone4, 5), (crowd, 5)):
        run = _open("f32", rows, n_rows, rec)
        _, status = _calls(run, I, Q)
        _check(run, status, rows, n_rows, ref, rec.view(np.int32)[8:].reshape(NCH, M.WORDS))


# ---- USB next to LSB ---------------------------------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("staged", [False, True])
def test_gpu_usb_next_to_lsb(staged):
    """6 channels on one shared stream; set 0 is LSB, set 1 USB at 200..3000 Hz.  The listed USB channels equal a context
    created with the USB set; listing an LSB channel refuses the process call and names the channel and the set"""
    nch = 6
    nco = siggen.nco_grid(nch)
    _, I, Q = _iq(nch, sum(SPLITS), seed=SEED)
    I, Q = I[1:2], Q[1:2]  # one stream for all
    set_of = [0, 1, 0, 1, 1, 0]
    rows, n_rows = [-1, 2, -1, 0, 1, -1], 3

    def shared(rx):
        rx.set_input_map([0] * nch, 1)

    def group(rx):
        shared(rx)
        rx.set_param_sets([USB], set_of, stages=staged)

    ref = _open(nch=nch, nco=nco, setup=shared, **USB)
    ref.rx.ft8_sync()
    _, ref_status = _calls(ref, I, Q)
    run = _open("f32", rows, n_rows, nch=nch, nco=nco, setup=group, **LSB)
    run.rx.ft8_sync()
    start = _words(run.rx)
    _, status = _calls(run, I, Q)
    want = dict(status=ref_status, power=ref.power.cpu().numpy(), words=_words(ref.rx))
    assert (want["status"][1][:, -1, 0] == 2).all() and (want["power"][:, 0, :2 * M.BLOCK_BYTES] != FILL).all()
    _check(run, status, rows, n_rows, want, start)
    # an LSB channel in the list: the call is refused, nothing moves
    before = run.rx.ft8_state()
    run.rx.set_ft8_map([-1, 2, 1, 0, -1, -1], 3)
    run.status.fill_(int(FILL32))
    refused(lambda: run.process(I[:, :L], Q[:, :L]), ERR_UNSUPPORTED, "DEMOD_FT8 as USB", "channel 2 ", "parameter set 0")
    assert np.array_equal(run.rx.ft8_state(), before) and (run.status.cpu().numpy() == FILL32).all()
    run.rx.set_ft8_map(rows, n_rows)
    run.process(I[:, :L], Q[:, :L])
    # without a map the refusal stands word for word
    run.rx.set_ft8(0)
    run.rx.set_ft8_map(None)
    run.power, run.status = run.rx.set_ft8(1, MAXF)
    refused(lambda: run.process(I[:, :L], Q[:, :L]), ERR_UNSUPPORTED,
            "FT8 receive: the firmware demodulates DEMOD_FT8 as USB (Process.cpp:616-617); this context's mode is not T41RX_DEMOD_USB")


# ---- the audio entry under a map ---------------------------------------------------------------------------------------
def _audio_model():
    m = random_model(NCH, 0x465439, dataLoop=np.array([13, 7, 4, 0, 14]), counter=np.array([90, 0, 57, 91, 3]))
    m.power[:] = FILL  # (what _audio_chain() fills d_power with)
    return m


def _audio_chain(model, rows=None, n_rows=None, max_frames=31):
    import torch
    import t41_sdr_amd as T
    rx = T.RxChain(NCH, T.default_params(mode=0))
    if rows is not None:
        rx.set_ft8_map(rows, n_rows)
    rx.set_ft8_tables(*_tables())
    power, status = rx.set_ft8(1, max_frames)
    power.fill_(FILL)
    rx.set_ft8_state(model.record())
    return rx, power, status, torch


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["device_q15", "device_f32", "host_q15", "host_f32"])
def test_gpu_audio_entry_under_a_map(form):
    """pcm is [n_rows]: row r feeds the channel that names it, a row nobody names is not read (it holds NaNs / garbage and
    its status and power rows keep their fill).  Calls of 16 and 31 frames against the unmapped entry and the model"""
    rows, n_rows = MAPS["2_of_5"]  # channel 1 -> row 2, channel 4 -> row 0, row 1 unnamed
    model = _audio_model()
    start = clone(model)
    rng = np.random.default_rng(7)
    pcm = rng.integers(-32768, 32768, (n_rows, 47 * 128)).astype(np.int16)
    full = np.zeros((NCH, 47 * 128), np.int16)
    for c, r in enumerate(rows):
        if r >= 0:
            full[c] = pcm[r]
    if form.endswith("f32"):
        pcm, full = pcm.astype(np.float32) / np.float32(32768.0), full.astype(np.float32) / np.float32(32768.0)
        pcm[1] = np.nan
    plain, p_power, _, torch = _audio_chain(start)
    rx, power, status, _ = _audio_chain(start, rows, n_rows)
    give = (lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()) if form.startswith("device") else np.ascontiguousarray
    f0 = 0
    for n in (16, 31):
        status.fill_(int(FILL32))
        want = model.audio(full[:, f0 * 128:(f0 + n) * 128], "gulp")
        ref = plain.ft8_audio(give(full[:, f0 * 128:(f0 + n) * 128])).cpu().numpy()
        got = rx.ft8_audio(give(pcm[:, f0 * 128:(f0 + n) * 128])).cpu().numpy()
        assert np.array_equal(ref, want) and got.shape == (n_rows, n, 4)
        for c, r in enumerate(rows):
            if r >= 0:
                assert np.array_equal(got[r], want[c]), "status of channel %d, call at frame %d" % (c, f0)
        assert (got[1] == FILL32).all()
        f0 += n
    p, words = power.cpu().numpy(), _words(rx)
    assert np.array_equal(p_power.cpu().numpy(), model.power)
    for c, r in enumerate(rows):
        if r >= 0:
            assert np.array_equal(p[r], model.power[c]) and np.array_equal(words[c], _words(plain)[c])
        else:
            assert np.array_equal(words[c], start.record().view(np.int32)[8:].reshape(NCH, M.WORDS)[c])
    assert (p[1] == FILL).all() and (p[0] != FILL).any()
    with pytest.raises(ValueError):
        rx.ft8_audio(give(full[:, :128]))  # [n_channels] rows under a map


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["audio_then_live", "live_then_audio"])
def test_gpu_handover_between_live_and_audio_under_a_map(order):
    """32 frames each way on one record: the listed channels as in the unmapped context that makes the same two calls"""
    rows, n_rows = MAPS["2_of_5"]
    nfr = 32
    _, I, Q = _iq(NCH, sum(SPLITS), seed=SEED)
    I, Q = I[:, :nfr * L], Q[:, :nfr * L]
    pcm = np.random.default_rng(9).integers(-32768, 32768, (n_rows, nfr * 128)).astype(np.int16)
    full = np.zeros((NCH, nfr * 128), np.int16)
    for c, r in enumerate(rows):
        if r >= 0:
            full[c] = pcm[r]
    plain, mapped = _open(), _open("f32", rows, n_rows)
    results = {}
    for name, run, data in (("plain", plain, full), ("mapped", mapped, pcm)):
        run.rx.ft8_sync()
        start = _words(run.rx)
        status = []
        for call in (("audio", "live") if order == "audio_then_live" else ("live", "audio")):
            run.status.fill_(int(FILL32))
            if call == "audio":
                status.append(run.rx.ft8_audio(run.torch.from_numpy(data).cuda()).cpu().numpy().copy())
            else:
                status.append(run.process(I, Q)[2])
        results[name] = dict(status=status, power=run.power.cpu().numpy(), words=_words(run.rx), start=start)
    assert (results["plain"]["words"][:, M.S_COUNTER] == 4).all()
    _check(mapped, results["mapped"]["status"], rows, n_rows, results["plain"], results["mapped"]["start"])


# ---- the decode by row -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_gpu_decode_by_row():
    """one synthetic transmission through the audio entry to row 1 of 2 (channel 3) of a 5-channel context, silence to row 0
    (channel 1), 1380 frames: the rows' records are the unmapped decode's of those channels, the transmission reads
    CQ K1ABC FN42, the other row has no valid record"""
    from t41_sdr_amd import ft8 as F
    rows, n_rows = [-1, 0, -1, 1, -1], 2
    pcm = np.stack([np.zeros_like(recording(0)), recording(0)])
    full = np.zeros((NCH, pcm.shape[1]), np.int16)
    full[1], full[3] = pcm[0], pcm[1]
    t = D.tables()
    fresh = A.FT8AudioModel(NCH, *_tables())
    out = {}
    for name, r, n, data in (("plain", None, None, full), ("mapped", rows, n_rows, pcm)):
        rx, power, status, torch = _audio_chain(fresh, r, n, max_frames=1380)
        rx.ft8_audio_begin()
        st = rx.ft8_audio(torch.from_numpy(data).cuda()).cpu().numpy()
        rx.set_ft8_decode_tables(t.costas, t.gray, t.nm, t.mn, t.nrw)
        assert (st[:, 1379, 2] == 1).all()
        res, log174, plain_bits = rx.ft8_decode(select=st[:, 1379, 2] - 1, debug=True)
        out[name] = dict(res=res, log174=log174, plain=plain_bits, power=power.cpu().numpy())
    got, ref = out["mapped"], out["plain"]
    assert got["res"].shape == (n_rows,) and got["log174"].shape[0] == n_rows and ref["res"].shape == (NCH,)
    for c, r in ((1, 0), (3, 1)):
        assert got["res"][r].tobytes() == ref["res"][c].tobytes(), "decode records of row %d differ from channel %d's" % (r, c)
        assert same(got["log174"][r], ref["log174"][c]) and np.array_equal(got["plain"][r], ref["plain"][c])
        assert np.array_equal(got["power"][r], ref["power"][c])
    texts = [[m["text"] for m in found] for found in F.messages(got["res"])]
    assert texts == [[], [TEXT]] and int(got["res"][0]["num_valid"]) == 0 and int(got["res"][1]["num_valid"]) >= 1
    with pytest.raises(ValueError):
        rx.ft8_decode(select=[0] * NCH)  # by row: n_rows entries
