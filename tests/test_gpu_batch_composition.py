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

from tests import seam_fuzz, wp_checker
from tests.hip_harness import compare, reconstructor
from tests.stream_args import DST, KINDS, PLAIN_P, SLOTS, draw

pytestmark = pytest.mark.gpu


class Pool:
    """one stream and frame store per picture, on the device and in a checker; want[i] = the checker's frame of picture i"""

    def __init__(self, rng, oracle, hip, mb_w, mb_h, kinds):
        self.kinds, self.hip = kinds, hip
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
    subsets = [(s,) for s in range(len(kinds))] + list(itertools.combinations(range(len(kinds)), 2)) + [tuple(range(len(kinds)))]
    waves = {}
    with reconstructor(lib, 5, 4, n_streams=len(kinds), slots=SLOTS, max_pictures=len(kinds)) as hip:
        pool = Pool(rng, oracle, hip, 5, 4, kinds)
        for members in subsets:
            li = pool.run(members)
            plain_p = {kinds[s] for s in members} <= PLAIN_P
            assert (li["edge_info_fused"] > 0) == plain_p, "batch %s: edge_info_fused %d" % ([kinds[s] for s in members], li["edge_info_fused"])
            waves[len(members)] = li["intra_waves"]
    assert len(set(waves.values())) == 1          # (small batches: one shape; the large one is below)


def test_a_large_batch_of_random_kinds(lib, oracle):
    """more pictures than 2 x compute units in one call: intra_waves drops to a quarter, the loop filter packs several pictures per
    workgroup - every picture still its checker frame"""
    rng = np.random.default_rng(600)
    n = 600
    kinds = [str(k) for k in rng.choice(list(KINDS), size=n)]
    with reconstructor(lib, 3, 2, n_streams=n, slots=SLOTS, max_pictures=n) as hip:
        pool = Pool(rng, oracle, hip, 3, 2, kinds)
        small = pool.run(tuple(range(len(KINDS))))
        big = pool.run(tuple(range(n)))
    assert n > 2 * big["compute_units"], "the batch does not reach the large-batch shapes on this device (%d CUs)" % big["compute_units"]
    assert big["intra_waves"] < small["intra_waves"], (small, big)
    assert big["deblock_pics_per_wg"] > 1 and big["edge_info_fused"] == 0
    assert set(kinds) == set(KINDS)
