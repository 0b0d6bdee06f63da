"""FT8 from 12 kS/s audio, the CPU side: the restatement of DEMOD_FT8_WAV's collector (tests/ft8_audio_model.py) in its two
forms, its quirks, a whole slot through it and the decode model, the entry points' declarations, and ft8.read_wav().

The four transmissions of `CASES` (CQ K1ABC FN42 as continuous-phase 8-FSK at 12 kS/s, 1920 samples per symbol) run through
the gulp form for all 1380 frames and through tests/ft8_decode_model.py; test_ft8_audio.py reuses slots() on the GPU.
"""
import functools
import os
import re
import subprocess
import wave

import numpy as np
import pytest

import ft8_audio_model as A
import ft8_codec as Cd
import ft8_decode_model as D
import ft8_model as M
from rx_harness import assert_entry_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("t41rx_ft8_audio_device_q15", "t41rx_ft8_audio_device", "t41rx_ft8_audio_host_q15", "t41rx_ft8_audio_host",
       "t41rx_ft8_audio_begin", "t41rx_ft8_audio_end")
TEXT = "CQ K1ABC FN42"
# tone 0 in units of 6.25 Hz, amplitude, start sample, noise sigma, seed
CASES = ((160, 0.14, 3 * 1920, 0.0, None), (160, 0.14, 3 * 1920 + 700, 0.0, None), (300, 0.05, 5 * 1920, 0.02, 1), (100, 0.5, 0, 0.0, None))
LENGTHS = (1, 14, 15, 16, 31)
COUNTERS = np.array([91, 90, 0, 45, 91, 92, 91, 3, 91, 90, 91, 92, 7, 91, 90])  # per dataLoop start; 92 stands only next to ft8_flag 0


@functools.lru_cache(maxsize=None)
def tables():
    return M.ft8_tables()


def payload():
    return Cd.pack_standard("CQ", "K1ABC", "FN42")


@functools.lru_cache(maxsize=None)
def recording(k):
    """transmission k of CASES as the int16 samples of a 15 s recording (176 640 samples); read only"""
    j0, amp, start, sigma, seed = CASES[k]
    x = A.pcm16(A.transmission(Cd.encode(payload())[0], j0, amp, start, sigma=sigma, seed=seed))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def slots():
    """the four recordings through the collector (gulp form, from power-on records) and the decode model:
    (status [4][1380][4], power [4][2][92 * 1472], state words [4][3088], decode records [4]); read only"""
    m = A.FT8AudioModel(len(CASES), *tables())
    m.begin()
    st = m.audio(np.stack([recording(k) for k in range(len(CASES))]), form="gulp")
    res = D.decode_all(m.power[:, 0])[0]
    out = (st, m.power.copy(), m.words(), res)
    for a in out:
        a.setflags(write=False)
    return out


def random_model(nch, seed, dataLoop=None, counter=None):
    """records as no stream leaves them: every buffer word random q15, random flags, leftover, start_time and n"""
    rng = np.random.default_rng(seed)
    m = A.FT8AudioModel(nch, *tables())
    m.buf[:] = rng.integers(-32768, 32768, m.buf.shape)
    m.scal[:, M.S_N] = rng.integers(0, 1 << 32, nch)
    m.scal[:, M.S_START] = rng.integers(0, 1 << 32, nch)
    for k in (M.S_SYNC, M.S_FT8FLAG, M.S_DSPFLAG, M.S_HALF):
        m.scal[:, k] = rng.integers(0, 2, nch)
    m.scal[:, M.S_LEFTOVER] = rng.integers(0, 4, nch)
    m.scal[:, M.S_DATALOOP] = rng.integers(0, 15, nch) if dataLoop is None else dataLoop
    m.scal[:, M.S_COUNTER] = rng.integers(0, 92, nch) if counter is None else counter
    m.power[:] = rng.integers(0, 256, m.power.shape)
    return m


def clone(m):
    c = A.FT8AudioModel(m.nch, m.window, m.mag_db)
    c.scal, c.buf, c.power = m.scal.copy(), m.buf.copy(), m.power.copy()
    return c


def same(a, b):
    return np.array_equal(a.scal, b.scal) and np.array_equal(a.buf, b.buf) and np.array_equal(a.power, b.power)


def test_index_table():
    i = np.arange(68)
    assert np.array_equal(A.INDEX, (i * 15) >> 3) and A.INDEX.max() == 125
    assert np.array_equal(A.INDEX, (i.astype(np.float32).astype(np.float64) * 120.0 / 64.0).astype(np.int64))


@pytest.mark.parametrize("nfr", LENGTHS)
def test_literal_and_gulp_forms_agree(nfr):
    """15 channels, one per dataLoop start, with counters that cross a slot's end within the call for some of them"""
    rng = np.random.default_rng(nfr)
    pcm = rng.integers(-32768, 32768, (15, nfr * 128)).astype(np.int16)
    a = random_model(15, 100 + nfr, dataLoop=np.arange(15), counter=COUNTERS)
    a.scal[[5, 11], M.S_FT8FLAG] = 0
    b = clone(a)
    sa, sb = a.audio(pcm, "literal"), b.audio(pcm, "gulp")
    assert np.array_equal(sa, sb) and same(a, b)
    f = pcm.astype(np.float32) / np.float32(32768.0)  # readWave()'s floats: the identity through arm_float_to_q15
    c = random_model(15, 100 + nfr, dataLoop=np.arange(15), counter=COUNTERS)
    c.scal[[5, 11], M.S_FT8FLAG] = 0
    assert np.array_equal(c.audio(f, "gulp"), sa) and same(a, c)


def test_one_call_equals_the_same_frames_split_at_every_point():
    rng = np.random.default_rng(31)
    pcm = rng.integers(-32768, 32768, (3, 31 * 128)).astype(np.int16)
    start = random_model(3, 7, dataLoop=np.array([13, 7, 0]), counter=np.array([90, 0, 91]))
    whole = clone(start)
    want = whole.audio(pcm, "gulp")
    for cut in range(1, 31):
        for first, second in (("gulp", "gulp"), ("literal", "gulp"), ("gulp", "literal")):
            m = clone(start)
            st = np.concatenate([m.audio(pcm[:, :cut * 128], first), m.audio(pcm[:, cut * 128:], second)], axis=1)
            assert np.array_equal(st, want) and same(m, whole), (cut, first, second)


def test_hole_cells_keep_the_record():
    m = random_model(2, 3, dataLoop=np.array([0, 9]))
    before = m.buf[:, list(A.HOLES)].copy()
    assert len(A.HOLES) == 12
    rng = np.random.default_rng(4)
    m.audio(rng.integers(-32768, 32768, (2, 45 * 128)).astype(np.int16), "literal")
    assert np.array_equal(m.buf[:, list(A.HOLES)], before)
    other = np.setdiff1d(np.arange(M.BUF_WORDS), A.HOLES)
    n = random_model(2, 3, dataLoop=np.array([0, 9]))
    assert (m.buf[:, other] != n.buf[:, other]).mean() > 0.99  # every other cell has been rolled out


def test_slot_completes_at_frame_1379():
    st, power, words, _ = slots()
    assert (st[:, :1379, 2] == 0).all() and (st[:, 1379, 2] == 1).all()
    assert (st[:, 1378, 0] == 91).all() and (st[:, 1379, 0] == 0).all() and (st[:, 1379, 1] == 0).all() and (st[:, 1379, 3] == 0).all()
    assert (words[:, M.S_HALF] == 1).all() and (words[:, M.S_COUNTER] == 0).all() and (words[:, M.S_N] == 1380).all()
    assert not power[:, 1].any()
    # frame 1380 .. 1394: block 0 of the other half
    m = A.FT8AudioModel(1, *tables())
    m.load_record(np.concatenate([np.array([M.MAGIC, M.ABI, 1, M.WORDS, 0, 0, 0, 0], np.int32), words[0]]).view(np.uint8))
    m.power[:] = 255  # (no row of a block reaches 255: the largest entry of mag_db is 10 ln(163840.1) = 120.07)
    st2 = m.audio(recording(0)[None, :15 * 128], "literal")
    assert st2[0, -1].tolist() == [1, 0, 0, 0]
    assert (m.power[0, 1, :M.BLOCK_BYTES] < 255).all() and (m.power[0, 1, M.BLOCK_BYTES:] == 255).all() and (m.power[0, 0] == 255).all()


def test_counter_92_without_begin_writes_nothing():
    m = random_model(1, 5, dataLoop=14, counter=92)
    m.scal[0, M.S_FT8FLAG] = 0
    p = m.power.copy()
    st = m.audio(np.zeros((1, 16 * 128), np.int16), "literal")
    assert np.array_equal(m.power, p) and (st[0, :, 0] == 92).all() and (st[0, :, 2] == 0).all()
    m.begin()
    st = m.audio(np.zeros((1, 15 * 128), np.int16), "literal")
    assert st[0, -1, 0] == 1 and not np.array_equal(m.power, p)


def test_begin_and_end_touch_exactly_their_words():
    m = random_model(4, 6)
    m.scal[:, M.S_COUNTER] = 17
    m.scal[:, [M.S_SYNC, M.S_FT8FLAG]] = 1
    before = clone(m)
    m.begin([1, 0, 1, 0])
    want = before.scal.copy()
    want[[0, 2], M.S_COUNTER] = 0
    assert np.array_equal(m.scal, want) and np.array_equal(m.buf, before.buf) and np.array_equal(m.power, before.power)
    m.end([0, 1, 1, 0])
    want[[1, 2], M.S_COUNTER] = want[[1, 2], M.S_SYNC] = want[[1, 2], M.S_FT8FLAG] = 0
    assert np.array_equal(m.scal, want) and np.array_equal(m.buf, before.buf) and np.array_equal(m.power, before.power)
    m.end()
    assert not m.scal[:, [M.S_COUNTER, M.S_SYNC, M.S_FT8FLAG]].any() and np.array_equal(m.scal[:, M.S_DATALOOP], before.scal[:, M.S_DATALOOP])


@pytest.mark.parametrize("k", range(len(CASES)))
def test_transmission_decodes(k):
    """the recording through the collector and the decode model: at least one valid candidate, every valid candidate the sent
    payload (no false decode), and the de-duplicated list the one text"""
    from t41_sdr_amd import ft8 as F
    res = slots()[3][k]
    a91 = Cd.a91_of(payload())
    valid = [c for c in res["cand"][:int(res["num_candidates"])] if int(c["flags"]) == 3]
    print("case %d: %d candidates, %d valid" % (k, int(res["num_candidates"]), len(valid)))
    assert int(res["num_valid"]) == len(valid) >= 1
    for c in valid:
        assert np.array_equal(c["a91"], a91)
    assert [m["text"] for m in F.messages(res)[0]] == [TEXT]


def test_entry_points_declared_exported_and_bound(built):
    import t41_sdr_amd as T
    import t41_sdr_amd._lib as lib
    hdr = assert_entry_points(NEW, pattern=r"T41RX_API\s+int\s+%s\s*\(")
    # nothing else is exported: the dynamic symbol table is what the two headers declare
    declared = set()
    for h in ("t41rx.h", "t41tx.h"):
        text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
        declared |= set(re.findall(r"T41[RT]X_API\s+[\w\s\*]+?\b(t41[rt]x_\w+)\s*\(", text))
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib.LIB_PATH], text=True)
    exported = {line.split()[-1].split("@")[0] for line in out.splitlines() if line.strip()}
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert "T41RX_ABI_VERSION 5" in hdr and lib.load().t41rx_abi_version() == 5
    for meth in ("ft8_audio", "ft8_audio_begin", "ft8_audio_end"):
        assert hasattr(T.RxChain, meth)
    assert callable(T.ft8.read_wav) and callable(T.ft8.decode_recordings)
    assert "t41rx_set_input_map" in hdr and re.search(r"input map.*do not apply", hdr) and "arm_float_to_q15" in hdr


def _write_wav(path, samples, channels=1, width=2, rate=12000):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(channels)
        f.setsampwidth(width)
        f.setframerate(rate)
        f.writeframes(samples.tobytes())


def test_read_wav(tmp_path):
    from t41_sdr_amd import ft8 as F
    x = np.random.default_rng(2).integers(-32768, 32768, 4000).astype("<i2")
    _write_wav(tmp_path / "ok.wav", x)
    got = F.read_wav(str(tmp_path / "ok.wav"))
    assert got.dtype == np.int16 and np.array_equal(got, x)
    _write_wav(tmp_path / "stereo.wav", x, channels=2)
    _write_wav(tmp_path / "bytes.wav", (x >> 8).astype(np.uint8), width=1)
    for bad in ("stereo.wav", "bytes.wav"):
        with pytest.raises(ValueError):
            F.read_wav(str(tmp_path / bad))
