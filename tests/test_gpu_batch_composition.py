"""A picture's bytes do not depend on its batch.  p264hip_reconstruct picks its kernels by looking at the whole batch once: any B
picture switches every picture to k_mc_sort_b + k_mc_second + k_deblock_bs<true>, any explicit weights to the _wp instances (any
explicit weights or any P list that holds a frame twice to k_deblock_bs<true>), any
I picture to the dense k_intra without the fused edge-info pass, and the batch size sets intra_waves, the loop filter's pictures
per workgroup / band height / odd_single and the motion-compensation workgroups per picture.  So an unweighted P picture decodes
through different code depending on what shares its call.  A pool of one picture per kind (each on its own stream and frame store)
is reconstructed alone, in every pair and all together, then ~600 small pictures of random kinds in one call (more than
2 x the compute units: the large-batch shapes); every picture must be its oracle / checker frame every time."""
import itertools

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor
from tests import seam_fuzz, wp_checker
from tests.test_gpu_seam_fuzz import compare

pytestmark = pytest.mark.gpu

SLOTS, DST = 4, 3                # reference frames in slots 0 .. 2, every picture writes slot 3
KINDS = {
    "I": dict(p_picture=False),
    "P": dict(n_ref=1),
    "P_multi_dup": dict(n_ref=3, dup_refs=True),
    "P_weighted": dict(n_ref=2, explicit_wp="legal"),
    "B": dict(n_ref=2, n_ref_l1=2, b_picture=True, weighted=False),
    "B_implicit": dict(n_ref=2, n_ref_l1=2, b_picture=True, weighted=True),
    "B_weighted": dict(n_ref=2, n_ref_l1=2, b_picture=True, explicit_wp="legal"),
}
PLAIN_P = {"P"}                  # the kinds whose batches alone keep the fused edge-info pass (P_multi_dup: one frame at two indices -
                                 # the loop filter compares pictures, H.264 8.7.2.1, which the two-list edge-info kernel does)


def draw(rng, mb_w, mb_h, kind):
    return seam_fuzz.make_picture(rng, mb_w, mb_h, slots=SLOTS, dst_slot=DST, level_style="mixed", qp_mode="random", intra_share=0.2,
                                  slices=2, **KINDS[kind])


class Pool:
    """one stream and frame store per picture, on the device and in a checker; want[i] = the checker's frame of picture i"""

    def __init__(self, rng, oracle, lib, mb_w, mb_h, kinds):
        self.kinds = kinds
        self.hip = HipReconstructor(mb_w, mb_h, n_streams=len(kinds), slots=SLOTS, max_pictures=len(kinds), lib=lib)
        self.pics, self.want = [], []
        for s, kind in enumerate(kinds):
            chk = wp_checker.WeightedChecker(oracle, mb_w, mb_h, SLOTS)
            for slot in range(DST):
                f = seam_fuzz.random_frame(rng, mb_w, mb_h, "smooth" if (s + slot) % 2 else "noise")
                for dst, src in zip(chk.store[slot], f):
                    dst[:] = src
                self.hip.write_frame(s, slot, *f)
            pic = draw(rng, mb_w, mb_h, kind)
            self.pics.append(pic)
            self.want.append([a.copy() for a in chk.reconstruct(pic)])
        self.blank = [np.zeros_like(a) for a in self.want[0]]

    def run(self, members):
        """reconstruct the pictures `members` in one call (input slots 0.., their own streams); check them; the launch info"""
        for s in members:
            self.hip.write_frame(s, DST, *self.blank)
        self.hip.upload(0, [self.pics[s] for s in members])
        self.hip.reconstruct(list(range(len(members))), list(members))
        li = self.hip.last_launch()
        names = [self.kinds[s] for s in members]
        for s in members:
            compare(self.hip.read_frame(s, DST), self.want[s], "%s in batch %s" % (self.kinds[s], names), self.pics[s])
        return li


def test_every_kind_alone_in_pairs_and_together(lib, oracle):
    rng = np.random.default_rng(1016)
    kinds = list(KINDS)
    pool = Pool(rng, oracle, lib, 5, 4, kinds)
    subsets = [(s,) for s in range(len(kinds))] + list(itertools.combinations(range(len(kinds)), 2)) + [tuple(range(len(kinds)))]
    waves = {}
    for members in subsets:
        li = pool.run(members)
        plain_p = {kinds[s] for s in members} <= PLAIN_P
        assert (li["edge_info_fused"] > 0) == plain_p, "batch %s: edge_info_fused %d" % ([kinds[s] for s in members], li["edge_info_fused"])
        waves[len(members)] = li["intra_waves"]
    pool.hip.close()
    assert len(set(waves.values())) == 1          # (small batches: one shape; the large one is below)


def test_a_large_batch_of_random_kinds(lib, oracle):
    """more pictures than 2 x compute units in one call: intra_waves drops to a quarter, the loop filter packs several pictures per
    workgroup - every picture still its checker frame"""
    rng = np.random.default_rng(600)
    n = 600
    kinds = [str(k) for k in rng.choice(list(KINDS), size=n)]
    pool = Pool(rng, oracle, lib, 3, 2, kinds)
    small = pool.run(tuple(range(len(KINDS))))
    big = pool.run(tuple(range(n)))
    pool.hip.close()
    assert n > 2 * big["compute_units"], "the batch does not reach the large-batch shapes on this device (%d CUs)" % big["compute_units"]
    assert big["intra_waves"] < small["intra_waves"], (small, big)
    assert big["deblock_pics_per_wg"] > 1 and big["edge_info_fused"] == 0
    assert set(kinds) == set(KINDS)
