"""cr_qp_offset_delta without a GPU: the stimuli of tests/cr_offset_stim.py reach what the GPU tests claim to compare (a condition
on the stimuli, not a measurement) - chain B's V differs from chain A's for every directed picture, Cr's qPI is clipped at 0 and at
51, QPc(Cr) != QPc(Cb) on chroma edges of every class and strength, edges that only one of the two planes filters, filtered Cr edges
of I_PCM macroblocks; the host roads: packed and compact blocks do not depend on the delta, and the two changed structs lie as the C
header says."""
import collections
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

from p264decoder_amd import HipReconstructor
from p264decoder_amd import _native as N
from tests import cr_offset_checker as CR
from tests import cr_offset_stim as CS
from tests import scaling_checker as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def directed():
    return CS.directed_set()


def test_every_directed_picture_has_a_cr_plane_of_its_own(directed):
    assert len(directed) >= 20
    assert {(int(s.pic.desc.chroma_qp_offset), CR.delta_of(s.pic)) for s in directed} == set(CS.PAIRS)
    assert {(s.pic.mb_w, s.pic.mb_h) for s in directed} >= {(1, 1), (2, 5), (9, 1), (11, 9), (70, 3)}
    kinds = collections.Counter()
    for st in directed:
        two = CR.TwoChains(SC.SpecRecon, st.pic.mb_w, st.pic.mb_h, CS.SLOTS)
        for slot, f in st.frames.items():
            two.store.write(slot, f)
        y, u, v = two.reconstruct(st.pic)
        assert two.v_differs == 1, "%s: chain B's V equals chain A's" % st.name
        d, rec = st.pic.desc, st.pic.mb_records()
        kinds[int(d.slice_type)] += 1
        kinds["lists"] += bool(int(d.scaling_lists))
        kinds["t8"] += bool((rec["intra_modes"] & N.MB_T8X8).any())
        kinds["i8"] += bool((rec["intra_modes"] & N.MB_I8X8).any())
        kinds["wp"] += bool(int(d.explicit_wp))
        kinds["ipcm"] += bool((rec["mb_type"] == N.MB_IPCM).any() and (rec["mb_type"] != N.MB_IPCM).any())
        kinds["unfiltered"] += not int(d.deblock)
        kinds["offsets"] += bool(int(d.alpha_c0_offset) or int(d.beta_offset))
        kinds["flags"] += bool(rec["flags"].any())
        kinds["qps"] += int(rec["qp"].max()) - int(rec["qp"].min()) >= 40
    for k in (N.SLICE_I, N.SLICE_P, N.SLICE_B, "lists", "t8", "i8", "wp", "ipcm", "unfiltered", "offsets", "flags", "qps"):
        assert kinds[k], "no directed picture with %r: %s" % (k, dict(kinds))


def test_the_directed_set_reaches_the_filter_and_the_clips(directed):
    c = collections.Counter()
    for st in directed:
        CR.reach(st.pic, c)
    CR.assert_reached(c)
    # and a picture without a delta reaches none of it
    flat = collections.Counter()
    for st in CS.flat_set():
        CR.reach(st.pic, flat)
    assert not [k for k in flat if k[0] != "clip"], flat


def test_two_chains_with_delta_0_are_one_chain():
    st = CS.flat_set()[0]
    two = CR.TwoChains(SC.SpecRecon, st.pic.mb_w, st.pic.mb_h, CS.SLOTS)
    one = SC.SpecRecon(st.pic.mb_w, st.pic.mb_h, CS.SLOTS)
    for slot, f in st.frames.items():
        two.store.write(slot, f)
        one.store.write(slot, f)
    for a, b in zip(two.reconstruct(st.pic), one.reconstruct(st.pic)):
        assert np.array_equal(a, b)
    assert two.v_differs == 0


def test_packed_and_compact_blocks_do_not_know_the_delta(lib, directed):
    """desc travels beside the blocks: p264hip_input_layout, p264hip_pack_input and p264hip_pack_compact give the same bytes whatever
    the delta, and the compact header's reserved words stay zero"""
    for st in directed[3:12] + directed[13:]:
        pic = st.pic
        blocks = []
        for delta in (CR.delta_of(pic), 0, 24):
            keep = CR.delta_of(pic)
            pic.desc.cr_qp_offset_delta = delta
            try:
                lay = N.InputLayout()
                assert lib.p264hip_input_layout(C.byref(pic.desc), C.byref(lay)) == 0
                blocks.append((bytes(lay), HipReconstructor.pack(pic, lib).tobytes(), HipReconstructor.pack_compact(pic, lib).tobytes()))
            finally:
                pic.desc.cr_qp_offset_delta = keep
        assert blocks[0] == blocks[1] == blocks[2], st.name
        hdr = N.CompactHdr.from_buffer_copy(blocks[0][2][:C.sizeof(N.CompactHdr)])
        assert list(hdr.reserved)[1:] == [0] * 9


def test_the_changed_structs_lie_as_the_header_says():
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "p264hip.h"
#include "p264parse.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu ", sizeof(p264hip_picture_t), offsetof(p264hip_picture_t, cr_qp_offset_delta), offsetof(p264hip_picture_t, scaling8x8),
           offsetof(p264hip_picture_t, scaling_lists), offsetof(p264hip_picture_t, chroma_qp_offset));
    printf("%zu %zu %zu %zu %zu %zu ", sizeof(p264hip_launch_info_t), offsetof(p264hip_launch_info_t, t8x8_wgs), offsetof(p264hip_launch_info_t, scaled_pictures),
           offsetof(p264hip_launch_info_t, cr_pictures), offsetof(p264hip_launch_info_t, reserved), offsetof(p264hip_launch_info_t, intra_i8));
    printf("%d\n", (int)P264PARSE_OPT_CR_OFFSET);
    return 0;
}
'''
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "t.c"), "w").write(src)
        subprocess.run(["gcc", "-I" + os.path.join(ROOT, "include"), os.path.join(td, "t.c"), "-o", os.path.join(td, "t")], check=True)
        out = [int(x) for x in subprocess.run([os.path.join(td, "t")], stdout=subprocess.PIPE, text=True, check=True).stdout.split()]
    P, L = N.Picture, N.LaunchInfo
    assert out[:5] == [C.sizeof(P), P.cr_qp_offset_delta.offset, P.scaling8x8.offset, P.scaling_lists.offset, P.chroma_qp_offset.offset]
    assert P.cr_qp_offset_delta.offset == P.scaling8x8.offset + 128                       # appended behind scaling8x8
    assert out[5:11] == [C.sizeof(L), L.t8x8_wgs.offset, L.scaled_pictures.offset, L.cr_pictures.offset, L.reserved.offset, L.intra_i8.offset]
    assert out[5:11] == [64, 40, 44, 48, 52, 60]
    assert out[11] == 16
    z = N.Picture()
    assert z.cr_qp_offset_delta == 0                                                       # what every zeroed descriptor says
