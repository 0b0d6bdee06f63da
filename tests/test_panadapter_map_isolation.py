"""A listed channel's panadapter rows and beacon words must not depend on the rest of the batch ("Channels are
independent"), under a panadapter map (t41rx_set_panadapter_map).

GPU (-m gpu).  tests/batch_harness.py's engine, imported and not edited: nine probe channels by themselves (reversed), one
of them alone, and at {0, 3, 4, 15, 16, 17, 63, 64, 66} of 67 channels among two hostile crowds (B, C) and in the batch
cut to 65 (D).  The map lists the probes, in rows that run against the channels' order; in C it also lists every other
crowd channel, so that a probe's row, its place in the list and the list's length move between B and C while its words
must not.  Every probe's seven row buffers, beacon events, table, status words, audio and checkpoint rows are compared as
words, without a tolerance.  A row per frame, zoom 1, the general front end, the beacon monitor's fast clock.
"""
import numpy as np
import pytest

import batch_harness as B
import group_harness as G
from batch_harness import Case
from rx_harness import T  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

GENERAL = dict(RFgain=3, IQAmpCorrectionFactor=1.02, IQPhaseCorrectionFactor=-0.013)


def pan_map_setup(rx, comp, nfr):
    """the panadapter map, the panadapter with a row per frame, the beacon monitor behind it; results back by channel"""
    probes = [int(comp.pos[p]) for p in comp.probes]
    crowd = [int(c) for c in comp.crowd[::2]] if comp.rot else []
    listed = np.array(sorted(probes + crowd))
    rows = np.full(comp.nch, -1, np.int32)
    rows[listed] = np.arange(len(listed))[::-1]
    rx.set_panadapter_map(rows, len(listed))
    assert rx.panadapter_rows == len(listed)
    bufs = G.panadapter(rx, nfr, spectrumZoom=1, currentScale=1, update_period=1)
    rx.set_beacon_clock(0, 10000, 1)
    band = (np.arange(comp.nch) * 3 + 1) % 5
    floor, gain = (np.arange(comp.nch) % 7 - 3).astype(np.int32), np.zeros(comp.nch, np.float32)
    for p in comp.probes:  # a band, a noise floor and a gain correction that go with the probe
        band[comp.pos[p]], floor[comp.pos[p]], gain[comp.pos[p]] = p % 5, p % 4 - 1, 0.5 * p
    rx.set_panadapter_levels(floor, gain)
    snr, ev = rx.set_beacon(True, 1, band)

    def by_channel(t, n):
        b = t.cpu().numpy()[:, :n]
        out = np.zeros((comp.nch,) + b.shape[1:], b.dtype)
        out[listed] = b[rows[listed]]
        return out

    def read(n):
        out = {"panadapter " + k: by_channel(bufs[k], n) for k, _, _ in rx.PANADAPTER_ROWS}
        out.update({"beacon events": ev.cpu().numpy()[:, :n], "beacon snr": rx.beacon_snr(), "beacon status": rx.beacon_status()})
        return out
    return read


def test_a_listed_channels_words_do_not_depend_on_the_batch(T):
    case = Case("panadapter-map-beacon", dict(G.USB, **GENERAL), setup=pan_map_setup, dagger=True)
    got = B.run_composition(T, case)
    # the probes' rows are rows of a spectrum and the monitor recorded: equal words are not equal zeros
    last = got["B"][-1]
    assert all(v.any() for v in last["panadapter pixel"].values()) and all(v.any() for v in last["beacon status"].values())
    assert any((v.reshape(-1, 4)[:, 0] >= 0).any() for v in last["beacon events"].values())
