"""FT8 from 12 kS/s audio (the collector of DEMOD_FT8_WAV, Process.cpp:278-335) as a HIP entry: ft8_audio_kernel against its
restatement (tests/ft8_audio_model.py).

GPU (-m gpu): every status word, every power byte of both halves and every word of the FT8 state record is compared with
np.array_equal -- on ragged calls from prepared records, through the four entry forms, across a hand-over with the live
stage in both directions, over a whole slot with the decode behind it, and after every refusal.  The CPU side is
test_ft8_audio_model.py, whose slots() this file reuses.
"""
import ctypes as C

import numpy as np
import pytest

import ft8_audio_model as A
import ft8_decode_model as D
import ft8_model as M
from test_ft8_audio_model import TEXT, clone, random_model, recording, slots, tables


class Chain:
    """a USB context with FT8 on and, with a model, that model's record and power halves loaded"""

    def __init__(self, nch, max_frames, model=None, **kw):
        import torch
        import t41_sdr_amd as T
        self.torch = torch
        self.rx = T.RxChain(nch, T.default_params(mode=0), **kw)
        self.rx.set_ft8_tables(*tables())
        self.power, self.status = self.rx.set_ft8(1, max_frames)
        if model is not None:
            self.rx.set_ft8_state(model.record())
            self.power.copy_(torch.from_numpy(model.power))

    def audio(self, pcm, form="device"):
        st = self.rx.ft8_audio(self.torch.from_numpy(np.ascontiguousarray(pcm)).cuda() if form == "device" else np.ascontiguousarray(pcm))
        self.torch.cuda.synchronize()
        return st.cpu().numpy().copy()

    def same_as(self, model, what=""):
        assert np.array_equal(self.power.cpu().numpy(), model.power), "d_power differs from the model " + what
        assert np.array_equal(self.rx.ft8_state(), model.record()), "the FT8 state record differs from the model " + what


def _prepared():
    """3 channels with random records: two frames before block 90 of 92, mid-gulp at the start of a slot, and random"""
    return random_model(3, 0x465438, dataLoop=np.array([13, 7, 4]), counter=np.array([90, 0, 57]))


def _pcm(nch, nfr, seed):
    return np.random.default_rng(seed).integers(-32768, 32768, (nch, nfr * 128)).astype(np.int16)


@pytest.mark.gpu
def test_gpu_ragged_calls():
    """calls of 1, 14, 15, 16 and 31 frames from prepared records; channel 0 completes its slot 17 frames in"""
    model = _prepared()
    half0 = int(model.scal[0, M.S_HALF])
    ch = Chain(3, 31, model)
    pcm = _pcm(3, 77, 1)
    f0, status = 0, []
    for n in (1, 14, 15, 16, 31):
        got = ch.audio(pcm[:, f0 * 128:(f0 + n) * 128])
        want = model.audio(pcm[:, f0 * 128:(f0 + n) * 128], "literal")
        assert np.array_equal(got, want), "status words differ in the call at frame %d" % f0
        ch.same_as(model, "behind the call at frame %d" % f0)
        status.append(got)
        f0 += n
    st = np.concatenate(status, axis=1)
    assert st[0, 16, 2] == 1 + half0 and not st[0, :16, 2].any() and not st[0, 17:, 2].any() and st[0, 16, 0] == 0 and st[0, 16, 1] == 0
    assert not st[1:, :, 2].any() and st[1, -1, 0] == 5


@pytest.mark.gpu
def test_gpu_one_call_equals_three():
    pcm = _pcm(3, 31, 2)
    model = _prepared()
    a, b = Chain(3, 31, model), Chain(3, 31, model)
    whole = a.audio(pcm)
    parts = np.concatenate([b.audio(pcm[:, :128]), b.audio(pcm[:, 128:15 * 128]), b.audio(pcm[:, 15 * 128:])], axis=1)
    want = model.audio(pcm, "literal")
    assert np.array_equal(whole, want) and np.array_equal(parts, want)
    a.same_as(model)
    b.same_as(model)


@pytest.mark.gpu
def test_gpu_entry_forms():
    """int16 data through the q15 and float entries, device and host: one result; the float entry on samples outside the
    q15 range, infinities and NaNs: the model's"""
    pcm = _pcm(3, 16, 3)
    f32 = pcm.astype(np.float32) / np.float32(32768.0)
    model = _prepared()
    start = clone(model)
    want = model.audio(pcm, "literal")
    for data, form in ((pcm, "device"), (f32, "device"), (pcm, "host"), (f32, "host")):
        ch = Chain(3, 16, start)
        assert np.array_equal(ch.audio(data, form), want), (data.dtype, form)
        ch.same_as(model, "%s %s" % (data.dtype, form))
    wild = (np.random.default_rng(4).standard_normal((3, 16 * 128)) * 0.8).astype(np.float32)
    wild[:, 5::17] = np.array([1.0, -1.0, 1.5, -2.5, 1e10, -1e10, np.inf, -np.inf, np.nan, 32767.5 / 32768, -32768.5 / 32768, 1e-9, -1e-9],
                              np.float32)[np.arange(wild[:, 5::17].shape[1]) % 13]
    model = clone(start)
    want = model.audio(wild, "literal")
    assert {32767, -32768, 0} <= set(A.to_q15(wild).ravel().tolist())
    for form in ("device", "host"):
        ch = Chain(3, 16, start)
        assert np.array_equal(ch.audio(wild, form), want), form
        ch.same_as(model, "float " + form)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["audio_then_live", "live_then_audio"])
def test_gpu_handover_with_the_live_stage(order):
    """32 frames each way on one record; the receive path's audio is what it is without the audio call"""
    from test_ft8_receive import L, Run, _iq
    import t41_sdr_amd as T
    nch, nfr = 4, 32
    nco, I, Q = _iq(nch, nfr)
    pcm = _pcm(nch, nfr, 5)
    run, plain = Run(T, nch, nco, nfr), Run(T, nch, nco, nfr)
    model = A.FT8AudioModel(nch, *tables())
    for r in (run, plain):
        r.rx.ft8_sync()
    model.sync()

    def audio_call():
        got = run.rx.ft8_audio(run.torch.from_numpy(pcm).cuda()).cpu().numpy().copy()
        assert np.array_equal(got, model.audio(pcm, "literal")), "status words of the audio call"

    def live_call():
        out, tap, st = run.process(I, Q)
        assert np.array_equal(st, model.process(tap)), "status words of the process call"
        assert np.array_equal(out, plain.process(I, Q)[0]), "the receive path's audio changed"

    for call in ((audio_call, live_call) if order == "audio_then_live" else (live_call, audio_call)):
        call()
    assert np.array_equal(run.power.cpu().numpy(), model.power), "d_power differs from the model"
    assert np.array_equal(run.rx.ft8_state(), model.record()), "the FT8 state record differs from the model"
    assert (model.scal[:, M.S_COUNTER] == 4).all() and L == 2048


@pytest.mark.gpu
def test_gpu_whole_slot_and_decode():
    """2 channels x 1380 frames in one call, transmissions 0 and 2; the decode of the device's own waterfall is the model's"""
    from t41_sdr_amd import ft8 as F
    pick = [0, 2]
    st, power, words, res = slots()
    recs = [recording(k) for k in pick]
    ch = Chain(2, 1380)
    ch.rx.ft8_audio_begin()
    got = ch.audio(np.stack(recs))
    assert np.array_equal(got, st[pick]), "status words"
    assert np.array_equal(ch.power.cpu().numpy(), power[pick]), "d_power differs from the model"
    assert np.array_equal(ch.rx.ft8_state()[32:].view(np.int32).reshape(2, M.WORDS), words[pick]), "the FT8 state record differs from the model"
    assert (got[:, 1379, 2] == 1).all() and not got[:, :1379, 2].any()
    t = D.tables()
    ch.rx.set_ft8_decode_tables(t.costas, t.gray, t.nm, t.mn, t.nrw)
    dec = ch.rx.ft8_decode(select=got[:, 1379, 2] - 1)
    assert dec.tobytes() == np.ascontiguousarray(res[pick]).tobytes(), "decode records differ from the model"
    assert [[m["text"] for m in found] for found in F.messages(dec)] == [[TEXT], [TEXT]]
    assert F.decode_recordings(recs) == [[TEXT], [TEXT]]


@pytest.mark.gpu
def test_gpu_begin_and_end():
    model = _prepared()
    model.scal[:, [M.S_SYNC, M.S_FT8FLAG]] = 1
    ch = Chain(3, 1, model)
    ch.rx.ft8_audio_begin([0, 1, 0])
    model.begin([0, 1, 0])
    ch.same_as(model, "behind begin")
    ch.rx.ft8_audio_end([1, 0, 0])
    model.end([1, 0, 0])
    ch.same_as(model, "behind end")
    ch.rx.ft8_audio_end()
    model.end()
    ch.same_as(model, "behind end on all")


@pytest.mark.gpu
def test_gpu_refusals():
    """every refusal returns T41RX_ERR_ARG with nothing launched: the record, d_power and d_status read back unchanged"""
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd import _lib
    lib = _lib.load()
    model = _prepared()
    ch = Chain(3, 16, model)
    ch.status.fill_(-7)
    pcm = torch.zeros(3, 1381 * 128, dtype=torch.int16, device="cuda")
    f32 = torch.zeros(3, 17 * 128, dtype=torch.float32, device="cuda")
    host = np.zeros((3, 17 * 128), np.int16)
    entries = (("t41rx_ft8_audio_device_q15", pcm.data_ptr(), 2), ("t41rx_ft8_audio_device", f32.data_ptr(), 4),
               ("t41rx_ft8_audio_host_q15", host.ctypes.data, 2), ("t41rx_ft8_audio_host", host.ctypes.data, 4))

    def refused(rx, name, ptr, n, why):
        rc = getattr(lib, name)(rx._ctx, C.c_void_p(ptr), n)
        assert rc == _lib.ERR_ARG, "%s %s: returned %d" % (name, why, rc)
        return lib.t41rx_last_error().decode()

    for name, ptr, size in entries:
        for n in (0, -1):
            assert "n_frames" in refused(ch.rx, name, ptr, n, "n_frames %d" % n)
        assert "max_frames" in refused(ch.rx, name, ptr, 17, "n_frames > max_frames")
        assert "NULL" in refused(ch.rx, name, None, 16, "NULL")
        assert "aligned" in refused(ch.rx, name, ptr + size // 2, 16, "misaligned")
    big = Chain(3, 1380, model)
    big.status.fill_(-7)
    for name, ptr, size in entries[:1]:
        assert "1380" in refused(big.rx, name, ptr, 1381, "n_frames > T41RX_FT8_MAX_FRAMES")
    for c in (ch, big):
        torch.cuda.synchronize()
        c.same_as(model, "behind the refusals")
        assert (c.status == -7).all(), "d_status was written"
    # FT8 off: the switch off again, and a context whose stage was never on; no tables: a fresh context
    ch.rx.set_ft8(0)
    fresh = T.RxChain(3, T.default_params(mode=0))
    tabled = T.RxChain(3, T.default_params(mode=0))
    tabled.set_ft8_tables(*tables())
    for name, ptr, size in entries:
        assert "is off" in refused(ch.rx, name, ptr, 16, "FT8 off")
        assert "is off" in refused(tabled, name, ptr, 16, "FT8 never on")
        assert "no tables" in refused(fresh, name, ptr, 16, "no tables")
    assert np.array_equal(ch.rx.ft8_state(), model.record()) and np.array_equal(ch.power.cpu().numpy(), model.power)
    assert not fresh.ft8_state()[32:].any()
    # the Python wrapper refuses what it can see
    for bad in (np.zeros((3, 100), np.int16), np.zeros((2, 128), np.int16), np.zeros((3, 128), np.float64)):
        with pytest.raises(ValueError):
            big.rx.ft8_audio(bad)
