"""The HIP kernels against H.264 itself on the MI355X: the directed pictures of tests/inter_stim.py through p264hip_submit (one
picture at a time) and through p264hip_upload + p264hip_reconstruct (three distinct pictures per batch), all three planes byte
for byte against tests/spec_recon.py - inter prediction from 8.4.2.2 / 8.4.2.3, the residual from 8.5, intra from 8.3, the loop
filter from 8.7, nothing of the oracle.  The expected planes are computed once per module; the coverage assertions of the CPU
files are repeated on what was actually submitted (inter_stim.assert_covered)."""
import pytest

from tests import inter_stim as S
from tests import spec_recon
from tests.hip_harness import by_size, expect, run_batches, submit_each

pytestmark = pytest.mark.gpu
SLOTS = 3


@pytest.fixture(scope="module")
def expected():
    """{set: [(stim, [y, u, v] by the standard)]}"""
    return {which: [(st, expect(st, spec_recon.SpecRecon, SLOTS)) for st in getattr(S, which)()] for which in S.SETS}


@pytest.mark.parametrize("which", S.SETS)
def test_submit_equals_the_standard(lib, expected, which):
    bad, sent = submit_each(lib, expected[which], SLOTS)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    S.assert_covered(which, sent)


@pytest.mark.parametrize("which", [w for w in S.SETS if w != "shape_set"])         # (one picture of this size: it rides in the mixed batches)
def test_batches_of_three_equal_the_standard(lib, expected, which):
    cases = by_size(expected[which])[(S.MB_W, S.MB_H)]
    bad, sent, _ = run_batches(lib, cases, slots=SLOTS)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    S.assert_covered(which, list({id(st.pic): st for st in sent}.values()))


def test_mixed_batches_equal_the_standard(lib, expected):
    """P pictures, B pictures and pictures with explicit weights in one batch: the batch, not the picture, picks the kernel
    instances (a weighted picture sends every picture of its batch through the _wp instances, a B picture through the two-pass ones)"""
    take = lambda which, k: expected[which][k % len(expected[which])]
    cases = []
    for k in range(5):
        cases += [take("window_set", 7 * k), take("b_set", k), take("weighted_set", k), take("residual_set", 5 * k), take("b_set", k + 6), take("limit_set", k), take("shape_set", 0)]
    seen, distinct = set(), []
    for c in cases:
        if id(c[0].pic) not in seen:
            seen.add(id(c[0].pic))
            distinct.append(c)
    bad, sent, _ = run_batches(lib, distinct, slots=SLOTS)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert {bool(st.pic.desc.explicit_wp) for st in sent} == {False, True}
