"""What the receiver-group tests share (input map, parameter sets, audio rate, output map, buffer layout): the group's shape,
one chain builder, the setups of the stages that more than one of them runs behind the split, and the checkers of the
output map and the parameter sets.  The calls themselves are rx_harness.one_call()'s; how a reference is built and what may
differ from it stays in the test files.  Pure numpy but for the setups, which allocate on the device.
"""
import os

import numpy as np

import siggen
from rx_harness import INT1, INT2, ROOT, bits, one_call, sentinel_of

L, D = 2048, 256
NCH, NS = 19, 3  # ragged against the 16-wave and the 4-wave workgroups; 3 streams
# channel -> stream, with repeats in a non-monotone order and every stream used
STREAM_OF = np.array([2, 0, 0, 1, 2, 1, 1, 0, 2, 2, 0, 1, 0, 0, 2, 1, 2, 0, 1], np.int32)
assert STREAM_OF.shape == (NCH,) and set(STREAM_OF) == set(range(NS))
SET_OF = STREAM_OF.copy()  # channel -> parameter set of the tests with three sets: the same numbers, every set used, set 0 by some
USB = dict(mode=0, FLoCut=200, FHiCut=3000)


def chain(T, kw, nco=None, *, nch=NCH, layout="channel", rate=192000, setup=None, imap=None, ns=None, sets=None, setof=None,
          omap=None, nrows=None):
    """(a fresh context, what setup(rx) returned): created, then layout, audio rate, setup(rx), input map, parameter sets
    and output map, each only where asked for"""
    nco = siggen.nco_grid(nch, seed=11) if nco is None else nco
    rx = T.RxChain(len(nco), T.default_params(**kw), NCOFreq=nco)
    if layout != "channel":
        rx.set_buffer_layout(layout)
    if rate != 192000:
        rx.set_audio_rate(rate)
    keep = setup(rx) if setup else None
    if imap is not None:
        rx.set_input_map(imap, ns)
    if sets is not None:
        rx.set_param_sets(sets, setof)
    if omap is not None:
        rx.set_output_map(omap, nrows)
    return rx, keep


def run(rx, I, Q, host=False, guard=False):
    """one call on channel-major numpy rows in the context's layout and the arrays' sample format: the audio alone"""
    return one_call(rx, I, Q, host=host, guard=guard)[0]


# ---- setups: setup=partial(name, nfr=...) for chain(), or called on a context ----------------------------------------------
def side_outputs(rx, nfr, taps=("post_nco", "dec", "demod"), nch=NCH):
    """audio spectrum, display spectrum (zoom 2) and these stage taps, with room for nfr frames: (spect, maxima, spec,
    spec_old, the taps in the order given)"""
    import torch
    z = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    spect, mx, spec, old = z(nch, nfr, 1024), z(nch, nfr, 3), z(nch, nfr, 512), z(nch, nfr, 512)
    tap = {name: z(nch, nfr * dict(post_nco=2 * L, dec=512, demod=D)[name]) for name in taps}
    rx.set_audio_spectrum(spect, mx)
    rx.set_display_spectrum(spec, old, spectrumZoom=2)
    rx.set_debug_taps(**tap)
    return (spect, mx, spec, old) + tuple(tap.values())


def cw_receive(rx, nfr, index=None):
    """the CW tables and decode tree, the narrow filter where an index is given, detector and decoder with room for nfr
    frames: (the detector's tensor, the decoder's)"""
    import cw_decode_model as DM
    import cw_model as CWM
    rx.set_cw_tables(*CWM.tables())
    rx.set_cw_decode_tree(DM.tree())
    if index is not None:
        rx.set_cw_filter(index)
    return rx.set_cw_detector(1, nfr), rx.set_cw_decoder(1, nfr)


def ft8_receive(rx, nfr):
    """FT8 receive switched on with room for nfr frames and synchronised to a slot's start"""
    rx.set_ft8_tables()
    rx.set_ft8(1, nfr)
    rx.ft8_sync()


def ft8_results(rx, nfr):
    return [rx.ft8_status(nfr).cpu().numpy(), rx.ft8_power().cpu().numpy()]


def panadapter(rx, max_rows, **options):
    """the waterfall's gradient table and the panadapter switched on: its row buffers"""
    rx.set_panadapter_tables(np.load(os.path.join(ROOT, "tests", "golden", "display", "gradient.npz"))["gradient"])
    return rx.set_panadapter(True, max_rows=max_rows, **options)


# ---- checkers ----------------------------------------------------------------------------------------------------------------
def check_rows(got, ref, omap, nrows):
    """listened rows are the reference's rows of their channels; rows nobody names keep the sentinel"""
    omap = np.asarray(omap)
    assert got.shape == (nrows, ref.shape[1]) and got.dtype == ref.dtype
    for c in np.flatnonzero(omap >= 0):
        assert np.array_equal(got[omap[c]], ref[c]), "channel %d, row %d" % (c, omap[c])
        assert np.abs(ref[c].astype(np.float64)).max() > 0
    for r in sorted(set(range(nrows)) - set(omap[omap >= 0].tolist())):
        assert (got[r] == sentinel_of(got)).all(), "row %d has no channel and was written" % r


def expected_state(a, ref_state, before, omap):
    """the reference's checkpoint with the interpolator memories of the muted channels as `before` (a checkpoint of the
    mapped context in front of the call) held them"""
    want = ref_state.copy()
    rw, rb = a.state_records(want), a.state_records(before)
    for c in np.flatnonzero(np.asarray(omap) < 0):
        rw[c, INT1] = rb[c, INT1]
        rw[c, INT2] = rb[c, INT2]
    return want


def rows_equal(got, refs, setof, what):
    for k, ref in enumerate(refs):
        sel = np.asarray(setof) == k
        if sel.any():
            assert np.array_equal(bits(got)[sel], bits(ref)[sel]), "%s differs for the channels of set %d" % (what, k)
