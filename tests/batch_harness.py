"""The batch-isolation engine (tests/test_batch_isolation.py): a channel's words must not depend on the rest of the batch.

run_composition() takes a case and nine PROBE channels, each with rows and an NCO of its own, generated once.  It runs
them in these compositions, each in fresh contexts:

  A    the probes by themselves, in reversed order (a batch of 9)
  one  one of them alone (a batch of 1)
  B    the probes at POS = {0, 3, 4, 15, 16, 17, 63, 64, 66} of a batch of 67 -- both sides of every grouping of 4, 16 and
       64 channels and the ragged tail -- among 58 channels of CROWD: a third +-0.999 random-sign full scale, a third
       exact silence, a third the case's own signal class at 10x the amplitude (clipped to +-0.999), NCOs of another seed
  C    as B with another crowd: another seed, the three classes rotated, other NCOs
  D    B cut to 65 channels (the cases marked dagger): the last probe drops out, the ragged tail is one channel

and holds, after every call of the schedule, for every probe: the audio row, every result the case collects and the
probe's rows of every checkpoint section are the same WORDS (rx_harness.bits) in every composition.  B against C says
whether a channel reads another channel's data; A, one and D against B whether the arithmetic depends on the batch's shape.
Equal results count only if every probe's audio is non-zero in every call, B's and C's crowd rows differ and the crowd's
audio in B differs from the same channels' in C; the engine asserts all three.

Pure numpy up to a case's open(): a case is anything with the attributes of Case below, and the CPU tests of the engine
(tests/test_harness.py) run it on stub chains.
"""
import os

import numpy as np

import siggen
from rx_harness import bits, first, one_call, to_q15

POS = (0, 3, 4, 15, 16, 17, 63, 64, 66)
NP_, NB, ND = len(POS), 67, 65
ONE = 4  # the probe that also runs alone: the one at channel 16 of B
CROWD = np.array([c for c in range(NB) if c not in POS])
FULL, SILENT, LOUD = 0, 1, 2  # the crowd's classes


class Comp:
    """one composition: its name, its batch size, pos[p] = the channel of probe p (-1: not in it), its crowd channels (of
    the 67-channel numbering) with their seed and class rotation"""

    def __init__(self, name, nch, pos, crowd_seed=None, rot=0):
        self.name, self.nch, self.pos = name, nch, np.asarray(pos)
        self.crowd = CROWD[CROWD < nch] if crowd_seed is not None else np.zeros(0, int)
        self.crowd_seed, self.rot = crowd_seed, rot
        self.probes = np.flatnonzero(self.pos >= 0)

    def __repr__(self):
        return self.name


def compositions(dagger):
    pos = np.array(POS)
    out = [Comp("A", NP_, np.arange(NP_)[::-1]), Comp("one", 1, np.where(np.arange(NP_) == ONE, 0, -1)),
           Comp("B", NB, pos, crowd_seed=1, rot=0), Comp("C", NB, pos, crowd_seed=2, rot=1)]
    if dagger:
        out.append(Comp("D", ND, np.where(pos < ND, pos, -1), crowd_seed=1, rot=0))
    return out


def crowd_class(rot):
    """the class of every crowd channel of the 67-channel batch"""
    return (np.arange(len(CROWD)) + rot) % 3


def crowd_rows(case, total, seed, rot):
    """(I, Q, nco) of the 58 crowd channels: hostile but ordinary data"""
    n = len(CROWD)
    nco = siggen.nco_grid(n, seed=500 + seed)
    cls = crowd_class(rot)
    rng = np.random.default_rng([seed, 4177])
    I, Q = np.zeros((2, n, total * case.L), np.float32)
    full, loud = cls == FULL, cls == LOUD
    I[full] = np.where(rng.random((full.sum(), total * case.L)) < 0.5, -0.999, 0.999)
    Q[full] = np.where(rng.random((full.sum(), total * case.L)) < 0.5, -0.999, 0.999)
    li, lq = case.signal(int(loud.sum()), total, 900 + seed, nco[loud])
    I[loud] = np.clip(10.0 * li.astype(np.float64), -0.999, 0.999)
    Q[loud] = np.clip(10.0 * lq.astype(np.float64), -0.999, 0.999)
    return I, Q, nco


def batch_rows(comp, probe, crowds):
    """the composition's rows and NCOs, [nch, samples]: the crowd first, the probes on their channels"""
    pI, pQ, pnco = probe
    I, Q = np.zeros((2, comp.nch, pI.shape[1]), np.float32)
    nco = np.zeros(comp.nch, np.int32)
    if comp.crowd_seed is not None:
        cI, cQ, cnco = crowds[(comp.crowd_seed, comp.rot)]
        k = len(comp.crowd)
        I[comp.crowd], Q[comp.crowd], nco[comp.crowd] = cI[:k], cQ[:k], cnco[:k]
    for p in comp.probes:
        I[comp.pos[p]], Q[comp.pos[p]], nco[comp.pos[p]] = pI[p], pQ[p], pnco[p]
    return I, Q, nco


def words(x):
    """a per-channel result as its words, [nch, words per channel]"""
    x = bits(np.asarray(x))
    assert x.dtype.kind in "iu", x.dtype  # every comparison is on integer words
    return x.reshape(x.shape[0], -1)


def run_composition(T, case, seed=1):
    """The engine: the case in every composition, every probe's words compared.  case.open(T, comp, nco) gives a context
    with call(I, Q, nfr) -> {name: per-channel array [nch, ...]} holding at least "audio", and records() -> {section:
    [nch, words]}.  Returns {composition: [per call {name: the probes' words}]}."""
    total = sum(case.schedule)
    assert len(case.schedule) >= 2
    pnco = siggen.nco_grid(NP_, seed=101)
    pI, pQ = case.signal(NP_, total, seed, pnco)
    comps = compositions(case.dagger)
    crowds = {key: crowd_rows(case, total, *key) for key in sorted({(c.crowd_seed, c.rot) for c in comps if c.crowd_seed is not None})}
    env = dict(getattr(case, "env", None) or {})
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        got, crowd_in, crowd_audio = {}, {}, {}
        for comp in comps:
            I, Q, nco = batch_rows(comp, (pI, pQ, pnco), crowds)
            ctx = case.open(T, comp, nco)
            f0, per_call, heard = 0, [], []
            for nfr in case.schedule:
                sl = slice(f0 * case.L, (f0 + nfr) * case.L)
                f0 += nfr
                out = {k: words(v) for k, v in ctx.call(I[:, sl], Q[:, sl], nfr).items()}
                out.update({"record:" + k: words(v) for k, v in ctx.records().items()})
                assert all(v.shape[0] == comp.nch for v in out.values()), {k: v.shape for k, v in out.items()}
                per_call.append({k: {int(p): v[comp.pos[p]].copy() for p in comp.probes} for k, v in out.items()})
                heard.append(out["audio"][comp.crowd])
            got[comp.name] = per_call
            crowd_in[comp.name] = (I[comp.crowd], Q[comp.crowd])
            crowd_audio[comp.name] = heard
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    # what makes equal results evidence
    for name, per_call in got.items():
        for k, out in enumerate(per_call):
            for p, row in out["audio"].items():
                assert row.any(), "%s: probe %d's audio is all zero in call %d" % (name, p, k)
    differs = lambda a, b: [i for i in range(len(a)) if not np.array_equal(a[i], b[i])]  # noqa: E731
    assert len(differs(crowd_in["B"][0], crowd_in["C"][0])) == len(CROWD), "B's and C's crowd rows do not differ"
    for k in range(len(case.schedule)):
        assert differs(crowd_audio["B"][k], crowd_audio["C"][k]), "call %d: the crowd's audio is the same in B and C" % k
    # the comparison: nothing left out, no tolerance
    for x, y in (("B", "C"), ("A", "B"), ("one", "B"), ("B", "D")):
        if x not in got or y not in got:
            continue
        for k in range(len(case.schedule)):
            a, b = got[x][k], got[y][k]
            assert set(a) == set(b), "%s vs %s: call %d collects %s / %s" % (x, y, k, sorted(a), sorted(b))
            for name in sorted(a):
                for p in sorted(set(a[name]) & set(b[name])):
                    if a[name][p].shape != b[name][p].shape or not np.array_equal(a[name][p], b[name][p]):
                        bad = np.flatnonzero(a[name][p] != b[name][p]) if a[name][p].shape == b[name][p].shape else []
                        raise AssertionError("%s vs %s: %s of probe %d (channel %d of 67) differs in call %d: %d of %d words, first at %s"
                                             % (x, y, name, p, POS[p], k, len(bad), a[name][p].size, bad[:4]))
    return got


# ---- the receive cases ------------------------------------------------------------------------------------------------------
_SIGNALS = {}


def mode_signal(mode, L, fade=False):
    """the signal class of a demodulator: FM carriers, AM carriers for the synchronous detector, tones in noise; with a
    fade through which an AGC leaves its attack state"""
    def signal(rows, nfr, seed, nco):
        key = (mode, L, fade, rows, nfr, seed, np.asarray(nco).tobytes())
        if key not in _SIGNALS:  # generated once, shared among the cases, never written to
            _SIGNALS[key] = generate(rows, nfr, seed, nco)
            for a in _SIGNALS[key]:
                a.setflags(write=False)
        return _SIGNALS[key]

    def generate(rows, nfr, seed, nco):
        if mode == 3:
            I, Q = siggen.make_fm(rows, nfr * L, nco, seed=seed)
        elif mode == 8:
            I, Q = siggen.make_am_carrier(rows, nfr * L, nco, seed=seed)
        else:
            I, Q = siggen.make_iq(rows, nfr * L, nco, mode=mode, seed=seed)
        return siggen.fade(I, Q, [(0.3, 2.0), (0.3, 0.05), (0.4, 1.5)]) if fade else (I, Q)
    return signal


class Case:
    """A receive case: the parameters, the signal class, the call schedule, what setup(rx, comp, nfr) switches on (it
    returns read(nfr) -> {name: per-channel array} or None), the group options per composition (group(comp) -> the
    keywords of group_harness.chain, plus "after": fn(rx) for the maps set behind them), the sample format, layout and
    audio rate, and the environment of the contexts.  hcase: a stage_map_harness.Case whose context and switches are used."""

    def __init__(self, name, kw, signal=None, schedule=(2, 5), dagger=False, setup=None, group=None, q15=False, layout="channel",
                 rate=192000, env=None, hcase=None, route=""):
        self.name, self.kw, self.schedule, self.dagger, self.setup, self.group = name, kw, schedule, dagger, setup, group
        self.q15, self.layout, self.rate, self.env, self.hcase, self.route = q15, layout, rate, env, hcase, route
        self.L = 4 * kw.get("fft_length", 512)
        if signal is None:
            signal = mode_signal(kw.get("mode", 0), self.L, fade=bool(kw.get("AGCMode", 0)))
        self.signal = signal

    def __repr__(self):
        return self.name

    def open(self, T, comp, nco):
        return RxContext(T, self, comp, nco)


class RxContext:
    def __init__(self, T, case, comp, nco):
        import group_harness as G
        import stage_map_harness as H
        self.case, self.comp, self.H = case, comp, H
        nfr = max(case.schedule)
        opts = dict(case.group(comp)) if case.group else {}
        self.after = opts.pop("after", None)
        self.imap = opts.get("imap")
        keep = {}
        setup = (lambda rx: keep.setdefault("read", case.setup(rx, comp, nfr))) if case.setup else None
        if case.hcase is not None:
            self.rx = H.context(T, case.hcase, nfr, comp.nch, nco=nco, layout=case.layout, rate=case.rate, setup=setup, **opts)
            H.switch(self.rx, case.hcase, case.hcase.bits, nfr)
        else:
            self.rx, _ = G.chain(T, case.kw, nco, nch=comp.nch, layout=case.layout, rate=case.rate, setup=setup, **opts)
        if self.after:
            self.after(self.rx)
        self.read = keep.get("read")

    def call(self, I, Q, nfr):
        rx, comp = self.rx, self.comp
        if self.imap is not None:  # channel c reads stream imap[c]: the streams hold the channels' rows
            sI, sQ = np.zeros((2, rx.n_streams, I.shape[1]), np.float32)
            sI[self.imap], sQ[self.imap] = I, Q
            I, Q = sI, sQ
        got, _ = one_call(rx, I, Q, q15_scale=1.0 if self.case.q15 else None)
        omap = rx.output_map
        if omap is not None:  # by channel; a muted channel has no audio
            by = np.zeros((comp.nch, got.shape[1]), got.dtype)
            by[omap >= 0] = got[omap[omap >= 0]]
            got = by
        out = {"audio": got}
        if self.case.hcase is not None:
            det, txt = self.H.results(rx, nfr)
            out.update({k: v for k, v in (("cw detector", det), ("cw decoder", txt)) if v is not None})
        if self.read is not None:
            import torch
            torch.cuda.synchronize()
            out.update(self.read(nfr))
        return out

    def records(self):
        return self.H.sections(self.rx)


# ---- setups: setup(rx, comp, nfr) -> read(nfr) --------------------------------------------------------------------------------
def tap_setup(rx, comp, nfr, taps=("post_nco", "dec", "demod")):
    """audio spectrum and maxima, display spectrum, the stage taps"""
    import group_harness as G
    t = G.side_outputs(rx, nfr, taps=taps, nch=comp.nch)
    names = ("audio spectrum", "maxima", "display spectrum", "display spectrum old") + tuple(taps)
    per = dict(zip(names, (1024, 3, 512, 512) + tuple(dict(post_nco=2 * rx.frame_len, dec=512, demod=256)[k] for k in taps)))
    return lambda n: {k: first(x, comp.nch, n, per[k]) for k, x in zip(names, t)}


def cw_filter_setup(rx, comp, nfr, index=3):
    import cw_model as CWM
    rx.set_cw_tables(*CWM.tables())
    rx.set_cw_filter(index)
    return None


def ft8_setup(rx, comp, nfr):
    import group_harness as G
    G.ft8_receive(rx, nfr)
    return lambda n: dict(zip(("ft8 status", "ft8 power"), G.ft8_results(rx, n)))


def beacon_setup(rx, comp, nfr):
    """the panadapter, a row per frame, with the beacon monitor behind it; a band per channel that goes with the probe"""
    import group_harness as G
    bufs = G.panadapter(rx, nfr, spectrumZoom=1, currentScale=1, update_period=1)
    rx.set_beacon_clock(0, 10000, 1)
    band = (np.arange(comp.nch) * 3 + 1) % 5
    for p in comp.probes:
        band[comp.pos[p]] = p % 5
    snr, ev = rx.set_beacon(True, 1, band)

    def read(n):
        out = {"panadapter " + k: bufs[k].cpu().numpy()[:, :n] for k, _, _ in rx.PANADAPTER_ROWS}
        out.update({"beacon events": ev.cpu().numpy()[:, :n], "beacon snr": rx.beacon_snr(), "beacon status": rx.beacon_status()})
        return out
    return read


# ---- the transmit twin: the same engine on a TxChain ----------------------------------------------------------------------------
class TxCase:
    """A transmit case.  kind "ssb": the rows are microphone samples (I; Q is not used); "cw": L = 16 key bytes per frame,
    key down where I is not zero; "cal": the calibration exciter has no input, the rows' first sample is the channel's
    (amplitude / 10, phase) correction candidate -- a tenth, so that the crowd's 10x class is another candidate and not
    the clip."""
    dagger, env = True, None

    def __init__(self, name, kind, schedule=(2, 5), eq=False):
        self.name, self.kind, self.schedule, self.eq = name, kind, schedule, eq
        self.L = {"ssb": 2048, "cw": 16, "cal": 1}[kind]

    def __repr__(self):
        return self.name

    def signal(self, rows, nfr, seed, nco):
        rng = np.random.default_rng([seed, 31])
        if self.kind == "ssb":
            import tx_harness as X
            m = X.mic(rows, nfr, seed=seed, level=0.05).astype(np.float32) / np.float32(32768.0)
            return m, np.zeros_like(m)
        if self.kind == "cw":
            k = (rng.random((rows, nfr * 16)) < 0.6).astype(np.float32) * np.float32(0.05)
            k[:, ::5] = 0.05  # every call has a block with the key down
            return k, np.zeros_like(k)
        amp = np.repeat(rng.uniform(0.05, 0.099, (rows, 1)), nfr, axis=1).astype(np.float32)
        ph = np.repeat(rng.uniform(-0.02, 0.02, (rows, 1)), nfr, axis=1).astype(np.float32)
        return amp, ph

    def open(self, T, comp, nco):
        return TxContext(T, self, comp)


class TxContext:
    def __init__(self, T, case, comp):
        import tx_model as M
        from t41_sdr_amd import tx as TX
        self.case, self.comp = case, comp
        self.tx = T.TxChain(comp.nch, T.default_tx_params(mode=0, IQXAmpCorrectionFactor=1.03, IQXPhaseCorrectionFactor=0.02))
        if case.eq:
            self.tx.set_transmit_eq_bands(M.bands())
            self.tx.set_transmit_eq(1, [100, 50, 0, 150, 100, 200, 100, 100, 50, 100, 150, 0, 100, 200])
        if case.kind == "cw":
            self.tx.set_cw_tone(*TX.sine_tone(8))
        if case.kind == "cal":
            self.tx.set_cal_tone(*TX.cal_tone(), 0.5)

    def call(self, I, Q, nfr):
        import torch
        tx, kind = self.tx, self.case.kind
        if kind == "ssb":
            oL, oR = tx.ExciterIQData(torch.from_numpy(to_q15(I)).cuda())
        elif kind == "cw":
            oL, oR = tx.CW_ExciterIQData(nfr, torch.from_numpy(np.ascontiguousarray((I != 0).astype(np.uint8))).cuda())
        else:
            tx.set_cal_corrections(np.ascontiguousarray(10.0 * I[:, 0]), np.ascontiguousarray(Q[:, 0]))
            oL, oR = tx.ProcessIQData2_tx(nfr, device=True)
        torch.cuda.synchronize()
        return {"audio": oL.cpu().numpy(), "Q drive": oR.cpu().numpy()}

    def records(self):
        buf = self.tx.get_state()
        per = int(buf[:32].view(np.int32)[3])
        return {"tx": buf[32:].view(np.uint32).reshape(self.comp.nch, per)}
