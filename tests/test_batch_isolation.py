"""A channel's bits must not depend on the rest of the batch ("Channels are independent").

Every case below runs through tests/batch_harness.py: run_composition(): nine probe channels alone (9 channels, reversed;
one of them as a batch of 1), embedded at {0, 3, 4, 15, 16, 17, 63, 64, 66} of 67 channels among a hostile crowd (B), among
another crowd (C), and -- the cases marked dagger -- in the batch cut to 65 (D).  After every call the probes' audio,
every collected result and their rows of every checkpoint section are compared as uint32 / int16 words; there is no
tolerance.  B != C: a channel reads another channel's data.  A != B or B != D with B == C: the arithmetic depends on the
batch's shape.  Either is a defect of the kernel or of its host arguments.

The cases against rx_plan.hpp (plan_call):

  KernelForm           family ssb / am / nfm / sam: ssb-*, am*, nfm*, sam*;  plain: ssb-plain;  general front end:
                       ssb-general;  agc (barrier form in the 2-frame call, pipe in the 5-frame call): *-agc;  pipe
                       without agc: sam;  q15: ssb-q15, ssb-agc-q15;  taps: taps, taps-24k, am-taps and every stage
                       case;  map_form: input-map;  set_form: param-sets;  a24_form: ssb-24k, ssb-agc-24k;  omap_form:
                       output-map;  time-major rows: ssb-time-major
  Back                 fused: the whole-chain cases;  back512: the stage cases;  finish24: taps-24k;  cw_back: cw-filter;
                       cw_24k: cw-filter-24k;  cw_mixed: cw-filter-map;  long_pipe: the long-* cases
  long FFT             fused_back: long-1024-ssb, long-2048-ssb, long-2048-general (the front end that is not PLAIN),
                       long-2048-nfm, long-4096-ssb-segrun;  one_kernel:
                       long-4096-ssb;  cplx: long-1024-agc, long-4096-agc, long-1024-am, long-4096-am;  q15 (the third
                       kernel): long-1024-q15.  4 frames per call: at least 2 runs per channel, so that a workgroup holds
                       runs of different channels
  Ft8Source            own_tap: ft8 (schedule 2 + 14 frames: the stage's FFTs run once 15 frames are collected)
  stage kernels        plain form: stage-<case> for every case of stage_map_harness.CASES (eq, kim, spectral, lms, notch,
                       lms-notch, blanker, detector, decoder, eq-notch-blanker, eq-blanker);  list form: stage-map-<case>,
                       where a stage map lists the probes and in C also half the crowd, so that a probe's place in the
                       kernels' lists moves;  the EQ level map and the CW filter map: eq-level-map, cw-filter-map
  side stages          panadapter with the beacon monitor: panadapter-beacon;  audio and display spectra, stage taps: taps*
  transmit             tx-eq (ExciterIQData with the transmit equaliser), tx-cw (CW_ExciterIQData, a key per channel),
                       tx-cal (ProcessIQData2_tx, a correction candidate per channel); the plain exciter's permutation test
                       is tests/test_tx_exciter.py's
"""
from functools import partial

import numpy as np
import pytest

import batch_harness as B
import group_harness as G
import stage_map_harness as H
from batch_harness import Case, TxCase
from rx_harness import T  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

USB = G.USB
GENERAL = dict(RFgain=3, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=-0.013)  # tests/test_audio_rate.py's general front end
AM = dict(mode=2, FLoCut=-3000, FHiCut=3000)
NFM = dict(mode=3, FLoCut=200, FHiCut=3000, nfmFilterBW=12000)
SAM = dict(mode=8, FLoCut=-3000, FHiCut=3000)
SEG_RUN = {"T41RX_SEG_RUN": "3"}  # tests/test_gpu_parity.py: test_segment_run_length_invariance


def hsignal(hcase):
    return lambda rows, nfr, seed, nco: H.signal(hcase, rows, nfr, seed, nco)


def lng(N, **kw):
    return dict(fft_length=N, **kw)


# ---- group features: group(comp) -> the options of group_harness.chain (+ "after") --------------------------------------------
def shuffle(comp):
    """a permutation of the batch's channels that differs between the compositions"""
    c = np.arange(comp.nch)
    return ({"B": comp.nch - 1 - c, "C": (5 * c + 3) % comp.nch, "D": (7 * c + 2) % comp.nch}.get(comp.name, c[::-1])).astype(np.int32)


def crowd_values(comp, probe_value, crowd_value, dtype=np.int32):
    """per channel: probe p's own value on its channel, crowd_value(channel, shift) elsewhere, the shift another in C"""
    shift = 1 if comp.name == "C" else 0
    v = np.array([crowd_value(c, shift) for c in range(comp.nch)], dtype)
    for p in comp.probes:
        v[comp.pos[p]] = probe_value(p)
    return v


def input_map(comp):
    m = shuffle(comp)  # the crowd reads other streams; in C the probes' stream index moves
    return dict(imap=m, ns=comp.nch)


SETS = [dict(mode=1, FLoCut=-3000, FHiCut=-200), dict(mode=0, FLoCut=300, FHiCut=1000)]  # tests/test_param_sets.py: SSB3


def param_sets(comp):
    return dict(sets=SETS, setof=crowd_values(comp, lambda p: 0, lambda c, s: 1 + (c + s) % 2))


def output_map(comp):
    if comp.name in ("B", "D"):  # the crowd is muted: the probes' rows alone
        m = np.full(comp.nch, -1, np.int32)
        m[comp.pos[comp.probes]] = np.arange(len(comp.probes))[::-1]
        return dict(omap=m, nrows=len(comp.probes))
    return dict(omap=shuffle(comp), nrows=comp.nch)  # C: the crowd is listened to


def stage_map(comp):
    m = crowd_values(comp, lambda p: H.ALL, lambda c, s: H.ALL if s and c % 2 else 0, np.uint32)
    return dict(after=lambda rx: rx.set_stage_map(m))


def cw_filter_map(comp):
    m = crowd_values(comp, lambda p: (0, 1, 2, 3, 4, 0, 1, 2, 5)[p], lambda c, s: (c + 2 * s) % 6)
    return dict(after=lambda rx: rx.set_cw_filter_map(m))


def eq_level_map(comp):
    from test_receive_eq_map import VECTORS
    m = crowd_values(comp, lambda p: p % 3, lambda c, s: (c + s) % 3)
    return dict(after=lambda rx: rx.set_receive_eq_map(VECTORS[m]))


CW_KW = H.CW_KW
CW_SIGNAL = hsignal(H.CASES["detector"])

CASES = [
    # -- the whole chain, fft 512
    Case("ssb-plain", USB), Case("ssb-general", dict(USB, **GENERAL)), Case("am", AM), Case("nfm", NFM),
    Case("nfm-atan", dict(NFM, nfm_demod=1)), Case("sam", SAM),
    Case("ssb-agc", dict(USB, AGCMode=2), dagger=True), Case("ssb-general-agc", dict(USB, AGCMode=1, **GENERAL), dagger=True),
    Case("am-agc", dict(AM, AGCMode=3), dagger=True), Case("nfm-agc", dict(NFM, AGCMode=4), dagger=True),
    Case("nfm-atan-agc", dict(NFM, nfm_demod=1, AGCMode=2), dagger=True), Case("sam-agc", dict(SAM, AGCMode=1), dagger=True),
    Case("ssb-q15", USB, q15=True), Case("ssb-agc-q15", dict(USB, AGCMode=2), q15=True, dagger=True),
    Case("ssb-time-major", USB, layout="time"), Case("ssb-agc-time-major", dict(USB, AGCMode=2), layout="time", dagger=True),
    Case("ssb-24k", USB, rate=24000), Case("ssb-agc-24k", dict(USB, AGCMode=2), rate=24000, dagger=True),
    Case("taps", dict(USB, **GENERAL), setup=B.tap_setup), Case("am-taps", AM, setup=B.tap_setup),
    Case("taps-24k", dict(USB, **GENERAL), setup=B.tap_setup, rate=24000),
    # -- the long FFT lengths
    Case("long-1024-ssb", lng(1024, **USB), schedule=(4, 4), dagger=True), Case("long-2048-ssb", lng(2048, **USB), schedule=(4, 4), dagger=True),
    Case("long-2048-general", lng(2048, **dict(USB, **GENERAL)), schedule=(4, 4), dagger=True),
    Case("long-4096-ssb", lng(4096, **USB), schedule=(4, 4), dagger=True),
    Case("long-4096-ssb-segrun", lng(4096, **USB), schedule=(4, 4), dagger=True, env=SEG_RUN),
    Case("long-1024-agc", lng(1024, AGCMode=2, **USB), schedule=(4, 4), dagger=True),
    Case("long-4096-agc", lng(4096, AGCMode=1, **USB), schedule=(4, 4), dagger=True),
    Case("long-1024-am", lng(1024, **AM), schedule=(4, 4), dagger=True), Case("long-4096-am", lng(4096, **AM), schedule=(4, 4), dagger=True),
    Case("long-1024-q15", lng(1024, **USB), schedule=(4, 4), dagger=True, q15=True),
    Case("long-2048-nfm", lng(2048, **NFM), schedule=(4, 4), dagger=True),
] + [
    # -- the stages behind the hand-over: every stage kernel in its plain form and, behind a stage map, in its list form
    Case("stage-" + name, hc.kw, signal=hsignal(hc), dagger=True, hcase=hc) for name, hc in H.CASES.items()
] + [
    Case("stage-map-" + name, hc.kw, signal=hsignal(hc), dagger=True, hcase=hc, group=stage_map) for name, hc in H.CASES.items()
] + [
    Case("cw-filter", CW_KW, signal=CW_SIGNAL, setup=B.cw_filter_setup), Case("cw-filter-24k", CW_KW, signal=CW_SIGNAL, setup=B.cw_filter_setup, rate=24000),
    Case("ft8", dict(USB, **GENERAL), setup=B.ft8_setup, schedule=(2, 14)),
    Case("panadapter-beacon", dict(USB, **GENERAL), setup=B.beacon_setup),
    # -- the group features, the probes' own mapping unchanged across the compositions
    Case("input-map", USB, group=input_map), Case("input-map-agc", dict(USB, AGCMode=2), group=input_map, dagger=True),
    Case("param-sets", USB, group=param_sets), Case("output-map", USB, group=output_map),
    Case("cw-filter-map", CW_KW, signal=CW_SIGNAL, setup=partial(B.cw_filter_setup, index=5), group=cw_filter_map),
    Case("eq-level-map", H.CASES["eq"].kw, signal=hsignal(H.CASES["eq"]), hcase=H.CASES["eq"], group=eq_level_map),
    # -- transmit
    TxCase("tx-eq", "ssb", eq=True), TxCase("tx-cw", "cw"), TxCase("tx-cal", "cal"),
]
assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_a_channels_words_do_not_depend_on_the_batch(T, case):
    B.run_composition(T, case)


class Detuned(Case):
    """the plain SSB case, but in composition C the probe at channel 16 is tuned one step (50 Hz) away"""

    def open(self, T, comp, nco):
        if comp.name == "C":
            nco = nco.copy()
            nco[16] += 50
        return Case.open(self, T, comp, nco)


def test_the_engine_sees_one_tuning_step_on_the_real_chain(T):
    """the comparison has teeth on the device too: 50 Hz on one probe in one composition fails it, on that probe"""
    with pytest.raises(AssertionError, match=r"B vs C: audio of probe 4 \(channel 16 of 67\) differs in call 0"):
        B.run_composition(T, Detuned("detuned", USB))
