"""The beacon monitor stage (t41rx_set_beacon) on the GPU: every table, event and status word against the restatement
(beacon_model.py) applied to the kernel's own smeter rows -- integers and comparisons only, so bit for bit -- over
channel counts 1, 5 and 65, update periods 1 and 3 and both modes; split calls; the stage's record into a fresh context;
the audio of every entry form untouched; the refusals; and five channels, one per band, on one stream with two keyed
beacons.  A fast clock of 1000 ms per frame makes a slot ten frames."""
import numpy as np
import pytest

import beacon_model as M
import siggen
from rx_harness import T, calls, refused  # noqa: F401  (T: the fixture)
from t41_sdr_amd import beacon as B

pytestmark = pytest.mark.gpu
L = 2048
FAST = (0, 1000, 1)
NFR = 210
NSTREAMS = 2
_STREAMS = {}


def streams(nch=NSTREAMS):
    """the rows a mapped chain of nch channels reads (at most two): rows of noise with a 1 kHz tone whose level changes from frame to frame, computed once: dbm moves by tens of
    dB between rows"""
    if not _STREAMS:
        rng = np.random.default_rng(0xB0)
        n = np.arange(NFR * L, dtype=np.float64)
        tone = np.exp(2j * np.pi * siggen.passband_tone_hz(0, 0, 1000.0) / siggen.FS * n)
        I, Q = np.empty((NSTREAMS, NFR * L), np.float32), np.empty((NSTREAMS, NFR * L), np.float32)
        for r in range(NSTREAMS):
            amp = np.repeat(rng.choice([0.0, 0.001, 0.01, 0.05, 0.3], NFR), L)
            x = amp * tone + 0.01 * (rng.standard_normal(NFR * L) + 1j * rng.standard_normal(NFR * L)) / np.sqrt(2)
            I[r], Q[r] = x.real, x.imag
        _STREAMS.update(I=I, Q=Q)
    n = min(NSTREAMS, nch)
    return _STREAMS["I"][:n], _STREAMS["Q"][:n]


def gradient():
    import os
    from rx_harness import ROOT
    return np.load(os.path.join(ROOT, "tests", "golden", "display", "gradient.npz"))["gradient"]


def chain(T, nch, mapped=True, **params):
    """nch channels at NCOFreq 0; mapped: channel c reads stream c % 2"""
    rx = T.RxChain(nch, T.default_params(**params), NCOFreq=np.zeros(nch, np.int32))
    if mapped:
        rx.set_input_map(np.arange(nch, dtype=np.int32) % NSTREAMS, min(NSTREAMS, nch))
    return rx


def monitor(T, nch, period, mode, max_rows, clock=FAST, mapped=True, bands=None, **params):
    """a chain with the panadapter's smeter rows and the beacon stage on: (rx, smeter, snr, events, bands)"""
    rx = chain(T, nch, mapped, **params)
    rx.set_panadapter_tables(gradient())
    sm = rx.set_panadapter(True, update_period=period, update_phase=period - 1 if period > 1 else 0, max_rows=max_rows, outputs=["smeter"])["smeter"]
    rx.set_panadapter_levels(gain_correction=np.linspace(-6.0, 6.0, nch).astype(np.float32))
    bands = (np.arange(nch) * 3 + 1) % 5 if bands is None else np.asarray(bands)
    rx.set_beacon_clock(*clock)
    snr, ev = rx.set_beacon(True, mode, bands)
    assert tuple(snr.shape) == (nch, 18) and tuple(ev.shape) == (nch, max_rows, 4)
    return rx, sm, snr, ev, bands


def drive(rx, sm, ev, I, Q, edges, period, phase, offset=0, **options):
    """the stream in calls, its frame 0 being the panadapter's frame `offset`; returns (audio, frame numbers of the rows, dbm
    [nch, rows], events [nch, rows, 4])"""
    frames, dbms, events = [], [], []

    def after(rx, a, b):
        _, counter, k, first = rx.panadapter_status()
        assert counter == b + offset
        want = [n for n in range(a + offset, b + offset) if n % period == phase]
        assert k == len(want) and (first == want[0] if want else first == -1)
        if k:
            frames.extend(want)
            dbms.append(sm[:, :k, 3].cpu().numpy().copy())
            events.append(ev[:, :k].cpu().numpy().copy())

    audio, _, _ = calls(rx, I, Q, edges, after=after, **options)
    return audio, frames, np.concatenate(dbms, 1), np.concatenate(events, 1)


def model(bands, frames, dbm, clock, mode, n_on=0):
    """the restatement per channel on the kernel's own dbm rows: (snr [nch, 18], events [nch, rows, 4], status [nch, 8])"""
    snr, ev, st = [], [], []
    for c, band in enumerate(bands):
        m = M.Monitor(int(band), n_on, clock, mode)
        ev.append(m.run(dbm[c], frames))
        snr.append(m.snr)
        st.append(m.status())
    return np.stack(snr), np.stack(ev), np.stack(st)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def record_of(status, snr):
    """the stage's record from status [nch, 8] and snr [nch, 18]"""
    nch = status.shape[0]
    hdr = np.array([0x42313454, 5, nch, 26, 0, 0, 0, 0], np.int32)
    body = np.concatenate([status.astype(np.int32), snr.astype(np.float32).view(np.int32)], 1)
    return np.concatenate([hdr, body.reshape(-1)]).view(np.uint8)


# calls without a row (period 3: single frames that are no update frame), with one and with several
RAGGED = [0, 1, 2, 3, 4, 10, 11, 31, 32, 33, 70, 71, 110, 150, 151, 190, NFR]


@pytest.mark.parametrize("nch,period,mode", [(1, 1, 0), (5, 1, 1), (65, 1, 0), (1, 3, 1), (5, 3, 0), (65, 3, 1)])
def test_every_word_equals_the_model_on_the_kernels_own_rows(T, nch, period, mode):
    I, Q = streams(nch)
    phase = period - 1 if period > 1 else 0
    rx, sm, snr, ev, bands = monitor(T, nch, period, mode, 40)
    audio, frames, dbm, events = drive(rx, sm, ev, I, Q, RAGGED, period, phase)
    assert frames == [n for n in range(NFR) if n % period == phase] and np.isfinite(dbm).all()
    # the rows do move: the strongest tone lies 30 dB above the next level and audioMaxSquaredAve halves per row, 3 dB, so
    # four rows in a row without it (the seeded levels hold such runs) are worth over 10 dB
    assert (dbm.max(1) - dbm.min(1) > 10).all()
    want_snr, want_ev, want_st = model(bands, frames, dbm, FAST, mode)
    assert same_bits(events.astype(np.int32), want_ev)
    assert same_bits(rx.beacon_snr(), want_snr) and same_bits(snr.cpu().numpy(), want_snr)
    assert same_bits(rx.beacon_status(), want_st)
    assert same_bits(rx.beacon_state(), record_of(want_st, want_snr))
    recorded = (want_ev[:, :, 0] >= 0).sum(1)
    assert (recorded >= 18).all() and (want_snr > 0).sum() >= 10 * nch
    if mode == 0:  # the cycle ended and the band walk began again: the 4 changes of `band` at the start and more
        assert (np.diff(want_ev[:, :, 3], axis=1) != 0).sum(1).min() >= 5
    else:
        assert (want_ev[:, 20:, 2] == 1).all() and (np.diff(want_ev[:, :, 3], axis=1) != 0).sum(1).max() == 4
    # the audio of every call is the audio without the stage
    plain = chain(T, nch)
    assert same_bits(audio, calls(plain, I, Q, RAGGED)[0])


def test_split_calls_equal_one_call(T):
    import torch
    I, Q = streams()
    nch, period, phase, mode = 5, 3, 2, 1
    whole, wsm, _, wev, _ = monitor(T, nch, period, mode, NFR // period)
    one = drive(whole, wsm, wev, I, Q, [0, NFR], period, phase)
    split, ssm, ssnr, sev, _ = monitor(T, nch, period, mode, NFR // period)
    sev.fill_(0x5A5A5A5A)
    # a first call with no update frame launches nothing for the stage: table, events and status as the switch left them
    st0 = split.beacon_status()
    head = split.ProcessIQData(*(torch.from_numpy(np.ascontiguousarray(v[:, :2 * L])).cuda() for v in (I, Q))).cpu().numpy()
    assert split.panadapter_status()[1:] == (2, 0, -1) and same_bits(split.beacon_status(), st0)
    assert bool((sev == 0x5A5A5A5A).all()) and not split.beacon_snr().any()
    # then calls with no row, one row and many
    rest = drive(split, ssm, sev, I[:, 2 * L:], Q[:, 2 * L:], [0, 1, 2, 9, 10, 11, 12, 100, 101, NFR - 2], period, phase, offset=2)
    assert rest[1] == one[1] and same_bits(rest[2], one[2]) and same_bits(rest[3], one[3])
    assert same_bits(split.beacon_snr(), whole.beacon_snr()) and same_bits(split.beacon_state(), whole.beacon_state())
    assert same_bits(np.concatenate([head, rest[0]], 1), one[0])
    assert whole.beacon_snr().any() and ((one[3][:, :, 0] >= 0).sum(1) >= 18).all()


def test_the_record_continues_in_a_fresh_context(T):
    import torch
    I, Q = streams()
    nch, period, phase, mode, cut = 5, 3, 2, 0, 100
    ref = monitor(T, nch, period, mode, 64)
    drive(ref[0], ref[1], ref[3], I, Q, [0, cut, NFR], period, phase)
    a = monitor(T, nch, period, mode, 64)
    drive(a[0], a[1], a[3], I, Q, [0, cut], period, phase)
    path, record, status = a[0].get_state(), a[0].beacon_state(), a[0].beacon_status()
    assert record.size == 32 + nch * 26 * 4 and record.size == a[0]._lib.t41rx_beacon_state_bytes(a[0]._ctx)
    b = monitor(T, nch, period, mode, 64, bands=np.zeros(nch, np.int64))  # the record's bands replace these
    b[0].set_state(path)
    b[0].set_panadapter_counter(cut)
    b[0].set_beacon_state(record)
    assert same_bits(b[0].beacon_state(), record) and same_bits(b[0].beacon_status(), status)
    cI, cQ = (torch.from_numpy(np.ascontiguousarray(v[:, cut * L:])).cuda() for v in (I, Q))
    b[0].ProcessIQData(cI, cQ)
    assert same_bits(b[0].beacon_state(), ref[0].beacon_state()) and same_bits(b[3].cpu().numpy(), ref[3].cpu().numpy())
    assert not same_bits(ref[0].beacon_state(), record)
    # t41rx_set_state() leaves the stage alone; t41rx_reset() is the switch-on at frame 0 with the record's bands
    end = b[0].beacon_state()
    b[0].set_state(path)
    assert same_bits(b[0].beacon_state(), end)
    b[0].reset()
    st = b[0].beacon_status()
    assert not b[0].beacon_snr().any() and same_bits(st, model(a[4], [], np.zeros((nch, 0)), FAST, mode)[2])
    # refused records change nothing
    from t41_sdr_amd import _lib
    b[0].set_beacon_state(record)
    words = record.view(np.int32).copy()
    for at, value in ((0, 1), (1, 4), (2, nch + 1), (3, 25), (8 + 2, -1), (8 + 3, 19), (8 + 3, -1), (8 + 4, 2), (8 + 5, 18), (8 + 5, -1),
                      (8 + 6, 5), (8 + 7, -1), (8 + 26 + 7, 5)):
        bad = words.copy()
        bad[at] = value
        refused(lambda: b[0].set_beacon_state(bad.view(np.uint8)), _lib.ERR_STATE)
    bad = words.copy()  # listening (count > 0) on a band that is not the channel's
    bad[8 + 3], bad[8 + 6], bad[8 + 7] = 3, 1, 2
    refused(lambda: b[0].set_beacon_state(bad.view(np.uint8)), _lib.ERR_STATE, "not the channel's")
    refused(lambda: b[0].set_beacon_state(record[:-4]), _lib.ERR_STATE, "size")
    assert same_bits(b[0].beacon_state(), record)


@pytest.mark.parametrize("form", ["f32", "q15", "time", "unmapped", "host"])
def test_the_audio_of_every_call_is_the_audio_without_the_stage(T, form):
    I, Q = streams()
    nch, period, mode, nfr = 5, 3, 1, 36
    mapped = form != "unmapped"
    if not mapped:
        I, Q = I[np.arange(nch) % NSTREAMS], Q[np.arange(nch) % NSTREAMS]
    I, Q = I[:, :nfr * L], Q[:, :nfr * L]
    options = dict(layout="time" if form == "time" else "channel", q15_scale=1.0 if form == "q15" else None, host=form == "host")
    edges = [0, 1, 2, 7, 8, 20, nfr]
    rx, sm, snr, ev, bands = monitor(T, nch, period, mode, 8, mapped=mapped)
    plain = chain(T, nch, mapped)
    if form == "time":
        rx.set_buffer_layout("time")
        plain.set_buffer_layout("time")
    audio, frames, dbm, events = drive(rx, sm, ev, I, Q, edges, period, period - 1, **options)
    assert same_bits(audio, calls(plain, I, Q, edges, **options)[0]) and np.abs(audio.astype(np.float64)).max() > 0
    want_snr, want_ev, want_st = model(bands, frames, dbm, FAST, mode)
    assert same_bits(events.astype(np.int32), want_ev) and same_bits(rx.beacon_snr(), want_snr) and same_bits(rx.beacon_status(), want_st)


def test_refusals(T):
    import torch
    from t41_sdr_amd import _lib
    nch = 3
    rx = chain(T, nch, mapped=False)
    lib, ctx = rx._lib, rx._ctx
    band = np.array([0, 2, 4], np.int32)
    bp = band.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32))
    snr = torch.zeros(nch, 18, device="cuda")
    ev = torch.zeros(nch, 4, 4, dtype=torch.int32, device="cuda")

    def status(*a):
        rc = lib.t41rx_set_beacon(ctx, *a)
        assert rc == 0 or lib.t41rx_last_error()
        return rc

    assert lib.t41rx_get_beacon(ctx, None, None) == 0  # off
    # the panadapter off, then on without smeter rows
    assert status(1, 0, bp, snr.data_ptr(), ev.data_ptr(), 4) == _lib.ERR_UNSUPPORTED
    rx.set_panadapter_tables(gradient())
    rx.set_panadapter(True, update_period=1, max_rows=4, outputs=["pixel"])
    assert status(1, 0, bp, snr.data_ptr(), ev.data_ptr(), 4) == _lib.ERR_UNSUPPORTED
    refused(rx.beacon_state, _lib.ERR_STATE, "off")
    with pytest.raises(ValueError):
        rx.beacon_snr()
    keep = rx.set_panadapter(True, update_period=1, max_rows=4, outputs=["smeter"])  # (kept: a refused re-set drops RxChain's reference)
    for bad_band in ([0, 5, 1], [-1, 0, 0]):
        b = np.array(bad_band, np.int32)
        assert status(1, 0, b.ctypes.data_as(_lib.C.POINTER(_lib.C.c_int32)), snr.data_ptr(), ev.data_ptr(), 4) == _lib.ERR_ARG
    assert status(1, 2, bp, snr.data_ptr(), ev.data_ptr(), 4) == _lib.ERR_ARG and status(1, -1, bp, snr.data_ptr(), ev.data_ptr(), 4) == _lib.ERR_ARG
    assert status(1, 0, None, snr.data_ptr(), ev.data_ptr(), 4) == _lib.ERR_ARG
    assert status(1, 0, bp, None, ev.data_ptr(), 4) == _lib.ERR_ARG
    assert status(1, 0, bp, snr.data_ptr() + 2, ev.data_ptr(), 4) == _lib.ERR_ARG
    assert status(1, 0, bp, snr.data_ptr(), ev.data_ptr() + 4, 4) == _lib.ERR_ARG
    assert status(1, 0, bp, snr.data_ptr(), ev.data_ptr(), 3) == _lib.ERR_ARG  # max_rows smaller than the panadapter's
    assert status(2, 0, bp, snr.data_ptr(), ev.data_ptr(), 4) == _lib.ERR_ARG
    assert lib.t41rx_get_beacon(ctx, None, None) == 0  # nothing changed
    for bad_clock in ((-1, 32, 3), (180000, 32, 3), (0, -1, 3), (0, 32, 0)):
        refused(lambda: rx.set_beacon_clock(*bad_clock), _lib.ERR_ARG, "beacon clock")
    # on (without events): the panadapter cannot leave, lose its smeter rows or outgrow the stage
    assert status(1, 1, bp, snr.data_ptr(), None, 4) == 0 and lib.t41rx_get_beacon(ctx, None, None) == 1
    refused(lambda: rx.set_panadapter(False), _lib.ERR_UNSUPPORTED, "beacon")
    refused(lambda: rx.set_panadapter(True, update_period=1, max_rows=4, outputs=["pixel"]), _lib.ERR_UNSUPPORTED, "beacon")
    refused(lambda: rx.set_panadapter(True, update_period=1, max_rows=5, outputs=["smeter"]), _lib.ERR_ARG, "beacon")
    assert rx.panadapter_status()[0] is True
    # it runs, NULL events and all, and a refused re-switch leaves it running
    I, Q = streams()
    cI, cQ = (torch.from_numpy(np.ascontiguousarray(v[[0, 1, 0], :4 * L])).cuda() for v in (I, Q))
    rx.ProcessIQData(cI, cQ)
    assert status(1, 2, bp, snr.data_ptr(), None, 4) == _lib.ERR_ARG and lib.t41rx_get_beacon(ctx, None, None) == 1
    assert rx.beacon_status()[:, 6].tolist() == [4, 1, 3]  # four steps of band++ from 0, 2, 4
    # a frame number the clock cannot reach in 64 bits: the call processes nothing
    rx.set_beacon_clock(0, 2**31 - 1, 1)
    rx.set_panadapter_counter(2**62)
    state = rx.get_state()
    refused(lambda: rx.ProcessIQData(cI, cQ), _lib.ERR_ARG, "64 bits")
    assert np.array_equal(rx.get_state(), state) and rx.panadapter_status()[1] == 2**62
    assert status(1, 0, bp, snr.data_ptr(), None, 4) == _lib.ERR_ARG  # and the switch refuses there too
    # off: the panadapter is free again
    assert status(0, 0, None, None, None, 0) == 0 and lib.t41rx_get_beacon(ctx, None, None) == 0
    rx.set_panadapter(False)
    assert keep["smeter"].shape[1] == 4


def test_five_bands_on_one_stream_find_the_two_keyed_beacons(T):
    """Five channels, one per band, read one stream of weak noise in which a 1 kHz tone is keyed on during frames 2 .. 7 of
    the slots of two beacons (beacon_model.e2e_stream: sigma 0.01, amplitude 0.02, 20 frames per slot, the clock 19 frames
    late so that a slot's window closes with its last frame).  mode 0, 18 records per channel.  On the CPU
    (test_beacon_model.py, the oracle's audioMaxSquaredAve through the model's dBm) the smaller of the two chosen entries
    is 33.8 dB and the largest other entry 5.13 dB on every band: a ratio of 0.152 against the condition's 0.5."""
    import torch
    I, Q = M.e2e_stream()
    nch = 5
    rx = T.RxChain(nch, T.default_params(**M.E2E_PARAMS), NCOFreq=np.zeros(nch, np.int32))
    rx.set_input_map(np.zeros(nch, np.int32), 1)
    rx.set_panadapter_tables(gradient())
    sm = rx.set_panadapter(True, update_period=1, max_rows=M.E2E_FRAMES, outputs=["smeter"])["smeter"]
    rx.set_beacon_clock(*M.E2E_CLOCK)
    snr, ev = rx.set_beacon(True, 0, np.arange(5))
    rx.ProcessIQData(torch.from_numpy(I).cuda(), torch.from_numpy(Q).cuda())
    tables = rx.beacon_snr()
    assert ((ev.cpu().numpy()[:, :, 0] >= 0).sum(1) == 18).all()
    margins = M.e2e_conditions(tables)
    print("beacon e2e: per band (smaller chosen entry, largest other entry):", margins)
    # and the words are the model's on these rows, the record with them
    dbm = sm[:, :, 3].cpu().numpy()
    want_snr, want_ev, _ = model(np.arange(5), range(M.E2E_FRAMES), dbm, M.E2E_CLOCK, 0)
    assert same_bits(tables, want_snr) and same_bits(ev.cpu().numpy(), want_ev)
    st = rx.beacon_status()
    rec = B.monitor_record(tables, int(st[4, 6]), int(st[4, 5]), rx.params.audioVolume)
    assert rec == M.monitor_record(want_snr.T, int(st[4, 6]), int(st[4, 5]), rx.params.audioVolume) and len(rec) == 96
    levels = np.frombuffer(rec[5:95], np.uint8).reshape(18, 5)
    for k in range(5):
        assert all(levels[(s - k) % 18, k] >= 5 for s in M.E2E_SLOTS), levels[:, k]
