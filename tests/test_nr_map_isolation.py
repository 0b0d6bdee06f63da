"""The noise-reduction map's two kernels (nrspec_map_kernel, anr_map_kernel) through the batch-isolation engine
(batch_harness.run_composition, in the manner of tests/test_batch_isolation.py): a channel's words must not depend on the
rest of the batch.  The nine probes carry all eight combinations of (nrOptionSelect, ANR_notchOn) -- and with them every
class of the Xanr() list and both kinds of the spectral list -- among the two hostile crowds, whose own entries are another
assignment in composition C, so that a probe's place in both lists, its workgroup of the Xanr() list and that workgroup's
live columns move between the compositions while its own pair stays."""
import numpy as np
import pytest

import batch_harness as B
import group_harness as G
from batch_harness import Case
from rx_harness import T  # noqa: F401  (a fixture)
from test_batch_isolation import crowd_values

pytestmark = pytest.mark.gpu

PROBE_CODE = (0, 1, 2, 3, 4, 5, 6, 7, 6)  # kind + 4 * notch per probe: the probe that also runs alone (4) is notch only
assert set(PROBE_CODE) == set(range(8)) and len(PROBE_CODE) == B.NP_ and PROBE_CODE[B.ONE] != 0


def nr_map(crowd):
    def group(comp):
        m = crowd_values(comp, lambda p: PROBE_CODE[p], crowd)
        return dict(after=lambda rx: rx.set_nr_map(m & 3, m >> 2))
    return group


CASES = [
    # the crowd carries every combination too, turned by three in C
    Case("nr-map", G.USB, dagger=True, group=nr_map(lambda c, s: (c + 3 * s) % 8)),
    # the crowd asks for nothing in B and D and for LMS and notch in C: a probe's workgroup of the Xanr() list is short in one and full in the other
    Case("nr-map-idle-crowd", G.USB, dagger=True, group=nr_map(lambda c, s: 7 * s)),
    # under a context-wide pair of its own (not consulted), at 24 kS/s
    Case("nr-map-24k", dict(G.USB, nrOptionSelect=1, ANR_notchOn=1), rate=24000, group=nr_map(lambda c, s: (3 * c + s) % 8)),
]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_a_channels_words_do_not_depend_on_the_batch(T, case):
    got = B.run_composition(T, case)
    # the probes' records are in the comparison: the noise-reduction section is carried in every composition
    assert all("record:nr" in call for per_call in got.values() for call in per_call)
