"""The equalizer level map (t41rx_set_receive_eq_map): while a map is loaded and the equalizer runs on channel c -- the
context's switch on, and the stage map's T41RX_STAGE_EQ bit set or no stage map -- channel c is processed exactly as a
context whose t41rx_set_receive_eq(1, equalizerRec[c]) would process it.

Every comparison is bit for bit (uint32 views) against contexts WITHOUT a level map: one per distinct level vector, and
for the channels a stage map leaves out the context with the equalizer off.  19 channels, three vectors, the context-wide
levels a fourth one that no channel may show."""
import numpy as np
import pytest

import eq_model as EQM
import group_harness as G
import stage_map_harness as H
from group_harness import NCH
from rx_harness import T, bits, one_call  # noqa: F401  (T: a fixture)
from test_receive_eq import RAMP

pytestmark = pytest.mark.gpu

L = 2048
VECTORS = np.array([RAMP, [100] * 14, [-50, 0, 120, -7, 0, 33, -200, 100, 0, 0, -1, 250, 7, -100]], np.int32)
VEC_OF = (np.arange(NCH) % 3).astype(np.int32)
LEVELS = VECTORS[VEC_OF]
OWN = [7] * 14  # the context-wide levels of the mapped context: kept, returned, and not consulted
LISTED = np.array([0, 4, 8, 12, 18])  # the stage map's equalizer channels: vectors 0, 1, 2, 0, 0


def context(T, levels=None, **options):
    """a context with the band table loaded, and the equalizer on with these levels"""
    rx, _ = G.chain(T, G.USB, **options)
    rx.set_receive_eq_bands(EQM.bands())
    if levels is not None:
        rx.set_receive_eq(1, levels)
    return rx


def sections(rx):
    s = H.sections(rx)
    return s["path"], s.get("eq", np.zeros((NCH, 112), np.uint32))  # (the equalizer never ran: power-on zeros)


def run_levels(T, nfrs, listed=None, q15=False, seed=31, **options):
    a = context(T, OWN, **options)
    a.set_receive_eq_map(LEVELS)
    assert np.array_equal(a.receive_eq_map, LEVELS)
    on, own = a.receive_eq
    assert on == 1 and list(own) == OWN
    runs = np.ones(NCH, bool)
    if listed is not None:
        m = np.full(NCH, H.ALL & ~H.EQ, np.uint32)
        m[listed] = H.ALL
        a.set_stage_map(m)
        runs[:] = False
        runs[listed] = True
    refs = [(runs & (VEC_OF == v), context(T, VECTORS[v], **options)) for v in range(3)]
    if not runs.all():
        refs.append((~runs, context(T, None, **options)))
    import siggen
    I, Q = H.signal(H.CASES["eq"], NCH, sum(nfrs), seed, siggen.nco_grid(NCH, seed=11), q15)
    f0 = 0
    for nfr in nfrs:
        sl = slice(f0 * L, (f0 + nfr) * L)
        f0 += nfr
        got, _ = one_call(a, I[:, sl], Q[:, sl])
        path, eq = sections(a)
        for sel, r in refs:
            assert sel.any()
            ref, _ = one_call(r, I[:, sl], Q[:, sl])
            rpath, req = sections(r)
            assert np.array_equal(bits(got)[sel], bits(ref)[sel]), "audio of channels %s" % np.flatnonzero(sel)
            assert np.array_equal(path[sel], rpath[sel]) and np.array_equal(eq[sel], req[sel]), "records of channels %s" % np.flatnonzero(sel)
            assert np.abs(ref[sel].astype(np.float64)).max() > 0
    return a, got


@pytest.mark.parametrize("split", ["1", "3", "2+1"])
@pytest.mark.parametrize("stage_map", [False, True])
def test_levels_per_channel(T, stage_map, split):
    run_levels(T, [int(s) for s in split.split("+")], listed=LISTED if stage_map else None)


@pytest.mark.parametrize("stage_map", [False, True])
def test_levels_per_channel_q15(T, stage_map):
    run_levels(T, [2, 1], listed=LISTED if stage_map else None, q15=True)


def test_levels_per_channel_24k(T):
    run_levels(T, [2, 1], listed=LISTED, rate=24000)


def test_vectors_differ_and_removing_the_map_returns_to_the_context_wide_levels(T):
    a, got = run_levels(T, [1])
    a.reset()
    assert np.array_equal(a.receive_eq_map, LEVELS)  # reset keeps the map
    a.set_receive_eq_map(None)
    assert a.receive_eq_map is None
    b = context(T, OWN)
    import siggen
    I, Q = H.signal(H.CASES["eq"], NCH, 1, 5, siggen.nco_grid(NCH, seed=11))
    x, _ = one_call(a, I, Q)
    y, _ = one_call(b, I, Q)
    assert np.array_equal(bits(x), bits(y)) and np.array_equal(a.get_state(), b.get_state())
    # and the map is not idle: with it, on the same input from the same state, every channel's audio is another
    c = context(T, OWN)
    c.set_receive_eq_map(LEVELS)
    z, _ = one_call(c, I, Q)
    assert all(not np.array_equal(z[ch], y[ch]) for ch in range(NCH))
