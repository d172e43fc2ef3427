"""The HIP kernels against H.264 itself on the MI355X: the directed pictures of tests/inter_stim.py through p264hip_submit (one
picture at a time) and through p264hip_upload + p264hip_reconstruct (three distinct pictures per batch), all three planes byte
for byte against tests/spec_recon.py - inter prediction from 8.4.2.2 / 8.4.2.3, the residual from 8.5, intra from 8.3, the loop
filter from 8.7, nothing of the oracle.  The expected planes are computed once per module; the coverage assertions of the CPU
files are repeated on what was actually submitted (inter_stim.assert_covered)."""
import numpy as np
import pytest

from p264decoder_amd import HipReconstructor
from tests import inter_stim as S
from tests import spec_recon

pytestmark = pytest.mark.gpu
SLOTS = 3


@pytest.fixture(scope="module")
def expected():
    """{set: [(stim, [y, u, v] by the standard)]}"""
    out = {}
    for which in S.SETS:
        out[which] = []
        for st in getattr(S, which)():
            spec = spec_recon.SpecRecon(st.pic.mb_w, st.pic.mb_h, SLOTS)
            for slot, f in st.frames.items():
                spec.store.write(slot, f)
            out[which].append((st, [p.copy() for p in spec.reconstruct(st.pic)]))
    return out


def differences(got, want, what, pic):
    for plane, (a, b) in enumerate(zip(got, want)):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            s = 16 if plane == 0 else 8
            m = (ys[0] // s) * pic.mb_w + xs[0] // s
            r = pic.mb_records()[m]
            return ["%s plane %d: %d samples differ, first (y=%d, x=%d) macroblock %d type %d qp %d mask %#x vector %s: HIP %d standard %d" % (
                what, plane, len(ys), ys[0], xs[0], m, r["mb_type"], r["qp"], r["coef_mask"], pic.mv[m * 32:m * 32 + 2].tolist(), a[ys[0], xs[0]], b[ys[0], xs[0]])]
    return []


def by_size(cases):
    sizes = {}
    for st, want in cases:
        sizes.setdefault((st.pic.mb_w, st.pic.mb_h), []).append((st, want))
    return sizes


@pytest.mark.parametrize("which", S.SETS)
def test_submit_equals_the_standard(lib, expected, which):
    bad, sent = [], []
    for (mb_w, mb_h), cases in by_size(expected[which]).items():
        hip = HipReconstructor(mb_w, mb_h, n_streams=1, slots=SLOTS, max_pictures=1, lib=lib)
        for st, want in cases:
            for slot, f in st.frames.items():
                hip.write_frame(0, slot, *f)
            hip.submit(0, st.pic)
            bad += differences(hip.read_frame(0, st.pic.desc.dst_slot), want, st.name, st.pic)
            sent.append(st)
        hip.close()
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    S.assert_covered(which, sent)


def run_batches(lib, cases, n=3):
    """the cases (one picture size) in batches of n distinct pictures, one stream each"""
    (mb_w, mb_h), = {(st.pic.mb_w, st.pic.mb_h) for st, _ in cases}
    hip = HipReconstructor(mb_w, mb_h, n_streams=n, slots=SLOTS, max_pictures=n, lib=lib)
    bad, sent = [], []
    for at in range(0, len(cases), n):
        batch = [cases[(at + k) % len(cases)] for k in range(n)]       # (the last batch is filled up from the front)
        assert len({id(st.pic) for st, _ in batch}) == n
        for k, (st, _) in enumerate(batch):
            for slot, f in st.frames.items():
                hip.write_frame(k, slot, *f)
        hip.upload(0, [st.pic for st, _ in batch])
        hip.reconstruct(list(range(n)), list(range(n)))
        for k, (st, want) in enumerate(batch):
            bad += differences(hip.read_frame(k, st.pic.desc.dst_slot), want, "%s (stream %d of a batch)" % (st.name, k), st.pic)
            sent.append(st)
    hip.close()
    return bad, sent


@pytest.mark.parametrize("which", [w for w in S.SETS if w != "shape_set"])         # (one picture of this size: it rides in the mixed batches)
def test_batches_of_three_equal_the_standard(lib, expected, which):
    cases = by_size(expected[which])[(S.MB_W, S.MB_H)]
    bad, sent = run_batches(lib, cases)
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
    bad, sent = run_batches(lib, distinct)
    assert not bad, "%d of %d pictures differ: %s" % (len(bad), len(sent), bad[:3])
    assert {bool(st.pic.desc.explicit_wp) for st in sent} == {False, True}
