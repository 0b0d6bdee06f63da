"""The panadapter stage (t41rx_set_panadapter): ShowSpectrum()'s pixels and waterfall row and DrawSmeterBar()'s dBm at
the firmware's update cadence.  CPU: hand-checked points of the restatement (panadapter_model.py), the cadence rule over
ragged splits, the ctypes mirrors against the header.  GPU: the transform against the display / audio-spectrum side
outputs of a twin context bit for bit, the cadence over split calls, an exact replay at zoom 2 and 4, every integer word
against the restatement applied to the kernel's own FFT_spec rows, the S-meter, the entry forms, the refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import panadapter_model as M
import siggen
from rx_harness import one_call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L, R = 2048, 512
NCH, NFR = 3, 7
INTS = ("pixel", "y_new", "y_old", "waterfall")
NAMES = ("t41rx_set_panadapter_tables", "t41rx_set_panadapter", "t41rx_set_panadapter_levels", "t41rx_get_panadapter",
         "t41rx_set_panadapter_counter")


def gradient():
    return np.load(os.path.join(ROOT, "tests", "golden", "display", "gradient.npz"))["gradient"]


# ---------------------------------------------------------------------------------------------- CPU

def test_model_hand_checked_points():
    g = gradient()
    assert g.shape == (117,) and g.dtype == np.uint16
    # log10f_fast(0): frexpf(0) = (0, 0), so Y = -3.13396450166353 * 0.30103 = -0.943..: finite
    l0 = M.log10f_fast(np.zeros(1, np.float32))[0]
    assert np.isfinite(l0) and abs(float(l0) - (-3.13396450166353 * 0.3010299956639812)) < 1e-6
    # scale 1 = {20.0, 10}: (int16_t)(20 * -0.943) = -18 (toward zero), + 10 = -8; y = 247 + 8 - 0 = 255 -> 249;
    # -249 + 230 < 0 -> gradient[0]
    out, mem = M.rows(np.zeros((1, R), np.float32), g, scale=1, pixel_offset=0, noise_floor_y=247, noise_floors=0)
    assert (out["pixel"] == -8).all() and (out["y_new"] == 249).all()
    assert (out["waterfall"][0, :R - 1] == g[0]).all() and out["waterfall"][0, R - 1] == 0
    # power-on pixelold = 0 and oldNF = this row's currentNF: y_old = 247 - 0 - 0 = 247
    assert (out["y_old"] == 247).all()
    # a value that drives y to the top: spec = 1e9 at scale 1 -> pixel = 10 + (int16_t)(20 * ~9.0) = 189 or 190;
    # y = 247 - 190 = 57 -> 100; -100 + 230 = 130 -> 116
    out, _ = M.rows(np.full((1, R), 1e9, np.float32), g, scale=1)
    assert set(np.unique(out["pixel"])) <= {189, 190} and (out["y_new"] == 100).all()
    assert (out["waterfall"][0, :R - 1] == g[116]).all() and out["waterfall"][0, R - 1] == 0
    # 230 - y: y = 230 is gradient[0]'s last, y = 114 gradient[116]'s first row
    for y, idx in ((230, 0), (229, 1), (114, 116), (115, 115)):
        assert M.waterfall(np.full(R, y, np.int16), g)[0] == g[idx]
    # the first-row oldNF rule and its successor: row 0 takes its own currentNF, row 1 the one of row 0
    spec = np.full((2, R), 100.0, np.float32)  # pixel = 10 + 40 = 50 at scale 1
    out, mem = M.rows(spec, g, scale=1, noise_floors=[30, -20])
    assert (out["pixel"] == 50).all()
    assert (out["y_new"][0] == 247 - 50 - 30).all() and (out["y_old"][0] == 247 - 0 - 30).all()
    assert (out["y_new"][1] == 247 - 50 + 20).all() and (out["y_old"][1] == 247 - 50 - 30).all()
    assert mem[1] == -20 and (mem[0] == 50).all()
    # continuing from that memory gives what one run over three rows gives
    more, _ = M.rows(spec[:1], g, scale=1, noise_floors=5, pixelold=mem[0], old_nf=mem[1])
    whole, _ = M.rows(np.concatenate([spec, spec[:1]]), g, scale=1, noise_floors=[30, -20, 5])
    assert all(np.array_equal(more[k][0], whole[k][2]) for k in INTS)
    # dbm: 22 + 0 + 0 + 10 * log10f_fast(1) - 92 - 1 * 1.5 - 1; log10f_fast(1) = (poly(0.5) + 1) * 0.30103 ~ 0
    d = M.dbm(1.0)
    assert d.dtype == np.float32 and abs(float(d) - (-72.5)) < 0.02
    assert abs(float(M.dbm(100.0, gain_correction=2.0, attenuator=3, RFgain=4, rfGainAllBands=-10)) - (22 + 2 + 3 + 20 - 92 - 6 + 10)) < 0.02
    assert np.isfinite(M.dbm(0.0))
    assert np.array_equal(M.ave_recurrence([4.0, 2.0]), np.array([2.0, 2.0], np.float32))


def test_rows_of_call_over_ragged_splits():
    from t41_sdr_amd.panadapter import rows_of_call
    rng = np.random.default_rng(5)
    for period, phase in ((1, 0), (2, 1), (3, 1), (7, 0), (7, 6), (511, 0), (511, 37)):
        total = 3 * period + 5
        want = [n for n in range(total) if n % period == phase]
        assert rows_of_call(0, total, period, phase) == want
        for _ in range(6):  # ragged splits: the calls' rows, shifted by their start, concatenate to the whole
            cuts = sorted(set(rng.integers(0, total + 1, 4).tolist()) | {0, total})
            got = []
            for a, b in zip(cuts[:-1], cuts[1:]):
                r = rows_of_call(a, b - a, period, phase)
                assert all(0 <= f < b - a for f in r) and r == sorted(r)
                got += [a + f for f in r]
            assert got == want, (period, phase, cuts)
    assert rows_of_call(5, 0, 3, 1) == [] and rows_of_call(4, 1, 3, 1) == [0] and rows_of_call(5, 1, 3, 1) == []
    with pytest.raises(ValueError):
        rows_of_call(0, 4, 3, 3)


def test_ctypes_mirrors_match_the_header():
    from t41_sdr_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "t41rx.h")).read()
    exports = open(os.path.join(ROOT, "t41_sdr_amd", "csrc", "exports.map")).read()
    ctype = {"t41rx_ctx *": C.c_void_p, "const t41rx_ctx *": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64,
             "const uint16_t *": C.POINTER(C.c_uint16), "const int32_t *": C.POINTER(C.c_int32), "int32_t *": C.POINTER(C.c_int32),
             "const float *": C.POINTER(C.c_float), "int64_t *": C.POINTER(C.c_int64),
             "const t41rx_panadapter_out *": C.POINTER(_lib.PanadapterOut)}
    for name in NAMES:
        m = re.search(r"T41RX_API\s+int\s+%s\s*\(([^;]*)\);" % name, hdr)
        assert m, name
        args = []
        for a in m.group(1).replace("\n", " ").split(","):
            a = re.sub(r"\s+", " ", a.strip())
            t = re.match(r"(.*?)(\w+)$", a).group(1).strip()  # drop the parameter's name
            args.append(ctype[t])
        res, mirror = _lib.SYMBOLS[name]
        assert res is C.c_int and mirror == args, (name, mirror, args)
        assert (name + ";") in exports, name
    m = re.search(r"typedef struct t41rx_panadapter_out \{(.*?)\} t41rx_panadapter_out;", hdr, re.S)
    fields = re.findall(r"\*(\w+);", m.group(1))
    assert fields == [f[0] for f in _lib.PanadapterOut._fields_] and all(f[1] is C.c_void_p for f in _lib.PanadapterOut._fields_)
    assert re.search(r"#define\s+T41RX_ABI_VERSION\s+5\b", hdr)  # the stage adds entry points, not an ABI


# ---------------------------------------------------------------------------------------------- GPU

_STREAM = {}


def stream():
    """3 channels x 7 frames, computed once: seeded noise plus carriers, a silent channel, and one loud enough for the top
    clamp; and the two rows a 2-stream input map [0, 1, 0] reads"""
    if not _STREAM:
        nco = np.array([5000, -12000, 8000], np.int32)
        I, Q = siggen.make_iq(NCH, NFR * L, nco, seed=91)
        I[1] = 0.0
        Q[1] = 0.0
        n = np.arange(NFR * L, dtype=np.float64)
        I[2] = (0.95 * np.cos(2 * np.pi * 30000.0 / 192000.0 * n)).astype(np.float32)
        Q[2] = (0.95 * np.sin(2 * np.pi * 30000.0 / 192000.0 * n)).astype(np.float32)
        _STREAM.update(nco=nco, I=I, Q=Q, Im=np.ascontiguousarray(I[[0, 2]]), Qm=np.ascontiguousarray(Q[[0, 2]]), map=np.array([0, 1, 0], np.int32))
    return _STREAM


def chain(T, mapped=False, **params):
    s = stream()
    rx = T.RxChain(NCH, T.default_params(**params), NCOFreq=s["nco"])
    if mapped:
        rx.set_input_map(s["map"], 2)
    return rx


def frames(mapped, a, b):
    """I, Q of frames [a, b) as CUDA tensors"""
    import torch
    s = stream()
    I, Q = (s["Im"], s["Qm"]) if mapped else (s["I"], s["Q"])
    return torch.from_numpy(np.ascontiguousarray(I[:, a * L:b * L])).cuda(), torch.from_numpy(np.ascontiguousarray(Q[:, a * L:b * L])).cuda()


def host(t):
    import torch
    if t.dtype == torch.uint16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def snap(bufs, rows):
    return {k: host(v)[:, :rows].copy() for k, v in bufs.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_ints(got, spec_rows, ch_noise_floors, scale, pixel_offset, noise_floor_y=247, memory=None):
    """every pixel / y_new / y_old / waterfall word of `got` [nch, k, 512] against the restatement applied to the kernel's own
    FFT_spec rows; ch_noise_floors [nch][k]; memory: per channel (pixelold, oldNF) in front of row 0, None = power-on.
    Returns the memories behind the last row."""
    g, out = gradient(), []
    for ch in range(spec_rows.shape[0]):
        mem = (None, None) if memory is None else memory[ch]
        want, m = M.rows(spec_rows[ch], g, scale, pixel_offset, noise_floor_y, ch_noise_floors[ch], mem[0], mem[1])
        for k in INTS:
            assert np.array_equal(got[k][ch], want[k]), (ch, k, np.argwhere(got[k][ch] != want[k])[:4])
        out.append(m)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("zoom", [0, 1, 2, 3, 4])
def test_gpu_period_one_spec_rows_equal_the_display_side_output(built, zoom):
    import torch
    import t41_sdr_amd as T
    dI, dQ = frames(False, 0, NFR)
    twin = chain(T)
    ts, to = torch.zeros(NCH, NFR, R, device="cuda"), torch.zeros(NCH, NFR, R, device="cuda")
    twin.set_display_spectrum(ts, to, zoom)
    twin.ProcessIQData(dI, dQ)
    rx = chain(T)
    rx.set_panadapter_tables(gradient())
    bufs = rx.set_panadapter(True, spectrumZoom=zoom, currentScale=1, update_period=1, max_rows=NFR)
    audio = rx.ProcessIQData(dI, dQ)
    assert rx.panadapter_status() == (True, NFR, NFR, 0)
    assert same_bits(host(bufs["spec"]), host(ts)), zoom
    assert torch.equal(audio, chain(T).ProcessIQData(dI, dQ))
    spec = host(bufs["spec"])
    assert (spec[1] == 0).all() and spec[0].max() > 0  # the silent channel, noise + carrier
    if zoom == 0:
        assert spec[2].max() > spec[0].max()  # the loud one (its carrier lies outside the zoomed spans)
    check_ints(snap(bufs, NFR), spec, np.zeros((NCH, NFR), np.int64), 1, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("zoom,mapped", [(0, False), (0, True), (3, False)])
def test_gpu_cadence_one_call_against_split_calls(built, zoom, mapped):
    import torch
    import t41_sdr_amd as T
    period, phase, flagged = 3, 1, [1, 4]
    whole = chain(T, mapped)
    whole.set_panadapter_tables(gradient())
    wb = whole.set_panadapter(True, spectrumZoom=zoom, currentScale=2, update_period=period, update_phase=phase, max_rows=2)
    plain_whole, plain_split = chain(T, mapped), chain(T, mapped)
    dI, dQ = frames(mapped, 0, NFR)
    assert torch.equal(whole.ProcessIQData(dI, dQ), plain_whole.ProcessIQData(dI, dQ))
    assert whole.panadapter_status() == (True, NFR, 2, 1)
    want = snap(wb, 2)
    split = chain(T, mapped)
    split.set_panadapter_tables(gradient())
    sentinel = {}
    for name, dt, width in T.RxChain.PANADAPTER_ROWS:
        fill = np.full((NCH, 2, width), 0x5A5A if "int" in dt else 12345.0, dtype=dt)
        sentinel[name] = torch.from_numpy(fill.view(np.int16) if dt == "uint16" else fill).cuda()
        if dt == "uint16":
            sentinel[name] = sentinel[name].view(torch.uint16)
    before = snap(sentinel, 2)
    sb = split.set_panadapter(True, spectrumZoom=zoom, currentScale=2, update_period=period, update_phase=phase, max_rows=2, outputs=sentinel)
    status, got = [], []
    for a, b in ((0, 1), (1, 3), (3, 7)):
        cI, cQ = frames(mapped, a, b)
        assert torch.equal(split.ProcessIQData(cI, cQ), plain_split.ProcessIQData(cI, cQ)), (a, b)  # the audio of every call
        status.append(split.panadapter_status())
        if a == 0:  # no update frame: no row, the buffers untouched
            now = snap(sb, 2)
            assert all(same_bits(now[k], before[k]) for k in before)
        else:
            got.append(snap(sb, 1))
    assert status == [(True, 1, 0, -1), (True, 3, 1, 1), (True, 7, 1, 4)]
    for row in range(2):
        for k in want:
            assert same_bits(want[k][:, row], got[row][k][:, 0]), (k, row)
    if zoom == 0:  # un-smoothed FFT_spec does not depend on history: the twin's rows of those frames
        twin = chain(T, mapped)
        ts, to = torch.zeros(NCH, NFR, R, device="cuda"), torch.zeros(NCH, NFR, R, device="cuda")
        twin.set_display_spectrum(ts, to, 0)
        twin.ProcessIQData(dI, dQ)
        assert same_bits(want["spec"], host(ts)[:, flagged])


@pytest.mark.gpu
@pytest.mark.parametrize("zoom", [2, 4])
def test_gpu_zoomed_rows_by_replay_from_checkpoints(built, zoom):
    """period 3: the zoom chain sees frames 1 and 4 back to back.  A period-1 context that restores the path's checkpoint in
    front of each of them (from a context without the stage) and processes that one frame draws the same rows bit for
    bit -- which also needs t41rx_set_state() to leave the stage's memory alone."""
    import t41_sdr_amd as T
    flagged = [1, 4]
    rx = chain(T)
    rx.set_panadapter_tables(gradient())
    pb = rx.set_panadapter(True, spectrumZoom=zoom, currentScale=3, pixel_offset=-4, update_period=3, update_phase=1, max_rows=2)
    rx.ProcessIQData(*frames(False, 0, NFR))
    want = snap(pb, 2)
    plain, ck = chain(T), {}
    for f in range(NFR):
        if f in flagged:
            ck[f] = plain.get_state()
        plain.ProcessIQData(*frames(False, f, f + 1))
    rep = chain(T)
    rep.set_panadapter_tables(gradient())
    rb = rep.set_panadapter(True, spectrumZoom=zoom, currentScale=3, pixel_offset=-4, update_period=1, max_rows=1)
    size = rep.get_state().size
    for row, f in enumerate(flagged):
        assert ck[f].size == size  # no section of the stage's in the checkpoint
        rep.set_state(ck[f])
        rep.ProcessIQData(*frames(False, f, f + 1))
        got = snap(rb, 1)
        for k in INTS + ("spec",):
            assert same_bits(got[k][:, 0], want[k][:, row]), (zoom, k, f)


@pytest.mark.gpu
def test_gpu_integer_rows_from_the_kernels_own_spectra(built):
    import t41_sdr_amd as T
    reached = {"y": set(), "gradient": set()}
    g = gradient()
    nf1, nf2 = np.array([3, -5, 20], np.int32), np.array([-60, 40, -100], np.int32)
    for scale in range(5):
        rx = chain(T)
        rx.set_panadapter_tables(g)
        bufs = rx.set_panadapter(True, spectrumZoom=1, currentScale=scale, pixel_offset=7, update_period=1, max_rows=4)
        rx.set_panadapter_levels(noise_floor=nf1)
        rx.ProcessIQData(*frames(False, 0, 3))
        a = snap(bufs, 3)
        mem = check_ints(a, a["spec"], np.repeat(nf1[:, None], 3, 1), scale, 7)
        rx.set_panadapter_levels(noise_floor=nf2)  # between two rows: the next row's oldNF is not its currentNF
        rx.ProcessIQData(*frames(False, 3, 7))
        b = snap(bufs, 4)
        check_ints(b, b["spec"], np.repeat(nf2[:, None], 4, 1), scale, 7, memory=mem)
        assert (b["waterfall"][:, :, R - 1] == 0).all()
        for part in (a, b):
            reached["y"] |= set(np.unique(part["y_new"]).tolist()) | set(np.unique(part["y_old"]).tolist())
            reached["gradient"] |= set(np.unique(230 - part["y_new"].astype(np.int32)[:, :, :R - 1]).tolist())
    assert {M.TOP_Y, M.BOTTOM} <= reached["y"] and min(reached["y"]) == M.TOP_Y and max(reached["y"]) == M.BOTTOM
    assert min(reached["gradient"]) <= 0 and max(reached["gradient"]) >= 116  # both ends of gradient[] were drawn


@pytest.mark.gpu
def test_gpu_smeter_rows(built):
    import torch
    import t41_sdr_amd as T
    kw = dict(RFgain=2, rfGainAllBands=3)
    flagged = [0, 2, 4, 6]
    dI, dQ = frames(False, 0, NFR)
    twin = chain(T, **kw)
    tsp, tmx = torch.zeros(NCH, NFR, 1024, device="cuda"), torch.zeros(NCH, NFR, 3, device="cuda")
    twin.set_audio_spectrum(tsp, tmx)
    twin.ProcessIQData(dI, dQ)
    rx = chain(T, **kw)
    rx.set_panadapter_tables(gradient())
    bufs = rx.set_panadapter(True, spectrumZoom=0, update_period=2, update_phase=0, max_rows=4, outputs=["smeter", "audio_spect"])
    gc = np.array([1.5, -2.0, 6.0], np.float32)
    rx.set_panadapter_levels(gain_correction=gc, attenuator=4)
    rx.ProcessIQData(dI, dQ)
    assert rx.panadapter_status() == (True, NFR, 4, 0)
    got = snap(bufs, 4)
    assert same_bits(got["audio_spect"], host(tsp)[:, flagged])
    assert same_bits(got["smeter"][:, :, :2], host(tmx)[:, flagged, :2])
    for ch in range(NCH):
        ave = M.ave_recurrence(got["smeter"][ch, :, 0])
        assert same_bits(got["smeter"][ch, :, 2], ave), ch  # over the update frames only
        want = np.array([M.dbm(a, gc[ch], 4, 2, 3) for a in ave], np.float32)
        assert same_bits(got["smeter"][ch, :, 3], want), (ch, got["smeter"][ch, :, 3], want)
    assert (got["smeter"][1, :, 2] == 0).all() and np.isfinite(got["smeter"][1, :, 3]).all()  # the silent channel: log10f_fast(0)
    # the path's own word carries it: a checkpoint's audioMaxSquaredAve is the last update frame's
    assert np.array_equal(rx.state_records()[:, 184 + 12], got["smeter"][:, 3, 2])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["q15", "time", "am"])
def test_gpu_entry_forms(built, form):
    import torch
    import t41_sdr_amd as T
    s = stream()
    flagged = [1, 3, 5]
    params = dict(mode=T.DEMOD_AM) if form == "am" else {}

    def run(rx):
        if form == "time":
            rx.set_buffer_layout("time")
        return one_call(rx, s["I"], s["Q"], layout="time" if form == "time" else "channel", q15_scale=1.0 if form == "q15" else None)[0]

    twin = chain(T, **params)
    ts, to = torch.zeros(NCH, NFR, R, device="cuda"), torch.zeros(NCH, NFR, R, device="cuda")
    twin.set_display_spectrum(ts, to, 0)
    run(twin)
    rx = chain(T, **params)
    rx.set_panadapter_tables(gradient())
    bufs = rx.set_panadapter(True, spectrumZoom=0, currentScale=2, pixel_offset=-3, update_period=2, update_phase=1, max_rows=3)
    nf = np.array([10, 0, -30], np.int32)
    rx.set_panadapter_levels(noise_floor=nf)
    audio = run(rx)
    assert np.array_equal(audio, run(chain(T, **params)))
    assert rx.panadapter_status() == (True, NFR, 3, 1)
    got = snap(bufs, 3)
    assert same_bits(got["spec"], host(ts)[:, flagged])
    check_ints(got, got["spec"], np.repeat(nf[:, None], 3, 1), 2, -3)


@pytest.mark.gpu
def test_gpu_refusals_and_reset(built):
    import torch
    import t41_sdr_amd as T
    from t41_sdr_amd import _lib
    g = gradient()

    def refused(status, fn, *a, **k):
        with pytest.raises(T.T41RxError) as e:
            fn(*a, **k)
        assert e.value.status == status, (e.value.status, str(e.value))
        assert str(e.value).split(": ", 1)[1]  # t41rx_last_error() names the reason

    rx = chain(T)
    refused(_lib.ERR_ARG, rx.set_panadapter, True)  # no table yet
    refused(_lib.ERR_ARG, rx.set_panadapter_tables, g[:116])
    refused(_lib.ERR_ARG, rx.set_panadapter_tables, np.concatenate([g, g[:1]]))
    assert rx.panadapter_status()[0] is False
    rx.set_panadapter_tables(g)
    good = dict(spectrumZoom=1, currentScale=1, pixel_offset=0, spectrumNoiseFloor=247, update_period=3, update_phase=1, max_rows=2)
    for bad in (dict(spectrumZoom=-1), dict(spectrumZoom=5), dict(currentScale=-1), dict(currentScale=5), dict(pixel_offset=32768),
                dict(pixel_offset=-32769), dict(spectrumNoiseFloor=32768), dict(spectrumNoiseFloor=-32769), dict(update_period=0),
                dict(update_phase=-1), dict(update_phase=3)):
        refused(_lib.ERR_ARG, rx.set_panadapter, True, **dict(good, **bad))
        assert rx.panadapter_status()[0] is False
    out = _lib.PanadapterOut()
    assert rx._lib.t41rx_set_panadapter(rx._ctx, 1, 1, 1, 0, 247, 3, 1, C.byref(out), 0) == _lib.ERR_ARG  # max_rows < 1
    assert rx._lib.t41rx_set_panadapter(rx._ctx, 1, 1, 1, 0, 247, 3, 1, None, 2) == _lib.ERR_ARG
    refused(_lib.ERR_ARG, rx.set_panadapter_levels, noise_floor=np.array([0, 40000, 0]))
    refused(_lib.ERR_ARG, rx.set_panadapter_levels, noise_floor=np.array([0, 0, -32769]))
    # one owner per tap, both ways round
    spec, old = torch.zeros(NCH, NFR, R, device="cuda"), torch.zeros(NCH, NFR, R, device="cuda")
    spect, mx = torch.zeros(NCH, NFR, 1024, device="cuda"), torch.zeros(NCH, NFR, 3, device="cuda")
    rx.set_display_spectrum(spec, old, 0)
    refused(_lib.ERR_UNSUPPORTED, rx.set_panadapter, True, **good)
    rx.set_display_spectrum(None, None)
    rx.set_audio_spectrum(spect, mx)
    refused(_lib.ERR_UNSUPPORTED, rx.set_panadapter, True, **good)
    rx.set_audio_spectrum(None, None)
    bufs = rx.set_panadapter(True, **good)
    refused(_lib.ERR_UNSUPPORTED, rx.set_display_spectrum, spec, old, 0)
    refused(_lib.ERR_UNSUPPORTED, rx.set_audio_spectrum, spect, mx)
    assert rx.panadapter_status() == (True, 0, 0, -1)
    long_rx = T.RxChain(NCH, T.default_params(fft_length=1024), NCOFreq=stream()["nco"])
    long_rx.set_panadapter_tables(g)
    refused(_lib.ERR_UNSUPPORTED, long_rx.set_panadapter, True, **good)
    # a call with more update frames than max_rows: nothing is processed (frames 1, 4, 7 of eight would be three)
    s = stream()
    I8 = torch.from_numpy(np.concatenate([s["I"], s["I"][:, :L]], 1)).cuda()
    Q8 = torch.from_numpy(np.concatenate([s["Q"], s["Q"][:, :L]], 1)).cuda()
    state = rx.get_state()
    refused(_lib.ERR_ARG, rx.ProcessIQData, I8, Q8)
    assert rx.panadapter_status() == (True, 0, 0, -1) and np.array_equal(rx.get_state(), state)
    # t41rx_reset(): memory and counter back to power-on -- the same stream draws the same rows again
    dI, dQ = frames(False, 0, NFR)
    rx.set_panadapter_levels(noise_floor=np.array([4, 5, 6]))
    rx.ProcessIQData(dI, dQ)
    first, st1 = snap(bufs, 2), rx.panadapter_status()
    refused(_lib.ERR_ARG, rx.ProcessIQData, dI, dQ)  # frames 7 .. 13: rows at 7, 10, 13 -- one too many
    assert rx.panadapter_status() == st1
    rx.ProcessIQData(dI[:, :6 * L].contiguous(), dQ[:, :6 * L].contiguous())  # 7 .. 12: rows at 7, 10
    assert rx.panadapter_status() == (True, 13, 2, 7)
    assert not same_bits(snap(bufs, 2)["y_old"], first["y_old"])  # pixelold carried over
    rx.reset()
    assert rx.panadapter_status() == (True, 0, 0, -1)
    rx.ProcessIQData(dI, dQ)
    again = snap(bufs, 2)
    assert rx.panadapter_status() == st1 == (True, 7, 2, 1)
    assert all(same_bits(first[k], again[k]) for k in first)
    # the counter can be set: from 2, frames 0 .. 6 count 2 .. 8 and flag 4 and 7, i.e. the call's frames 2 and 5
    rx.set_panadapter_counter(2)
    rx.ProcessIQData(dI, dQ)
    assert rx.panadapter_status() == (True, 9, 2, 4)
    refused(_lib.ERR_ARG, rx.set_panadapter_counter, -1)
    rx.set_panadapter(False)
    assert rx.panadapter_status()[0] is False
    rx.set_display_spectrum(spec, old, 0)  # the tap is free again
