"""What tests/long_lists_stim.py reaches, and that each of its pictures can notice the faults it is there for - on the CPU.

The set's pictures carry up to 16 entries per list in a store of 17 slots.  `assert_covered` states what the SET reaches (every
entry of both lists through whole-macroblock and quadrant items, pairs with both indices at 8 or more, the pair (15, 15), the
generic two-list class with a high index, implicit weights that differ both ways round).  Then every picture is decoded by five
deliberately wrong copies of the REFERENCE - never a kernel - and every picture that uses the feature a wrong decoder breaks must
differ from its true expectation in luma and in chroma: a stimulus that could not tell would be no test of the kernels."""
import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import inter_checker as IC
from tests import long_lists_stim as LS
from tests import seam_fuzz
from tests import spec_recon


@pytest.fixture(scope="module")
def expected():
    return {st.name: LS.expected(st) for st in LS.pictures()}


def test_the_set_reaches_what_it_is_there_for():
    stims = LS.pictures()
    c = LS.assert_covered(stims)
    assert 20 <= len(stims) <= 36
    roads = {k[4] for k in c.entries}
    assert roads >= {"p", "wp", "generic", "list0 only", "list1 only", "second pass whole", "second pass quadrants",
                     "second pass with carried quadrants"}, sorted(roads)
    # the slots: every list entry of a picture names a slot other than its destination; the 16-entry lists name all the others
    for st in stims:
        d = st.pic.desc
        l0 = [int(d.ref_slot[i]) for i in range(int(d.n_ref))]
        assert int(d.dst_slot) not in l0 and all(0 <= s < LS.SLOTS for s in l0), st.name
        if int(d.n_ref) == 16 and "dup" not in st.name:
            assert sorted(l0 + [int(d.dst_slot)]) == list(range(LS.SLOTS)), st.name
        if d.slice_type == N.SLICE_B and int(d.n_ref) == 16 == int(d.n_ref_l1):
            l1 = [int(d.ref_slot_l1[i]) for i in range(16)]
            assert sorted(l1) == sorted(l0) and l1 != l0, st.name
    frames = [f for st in stims for f in st.frames.values()]
    assert len({f[0].tobytes() for f in frames}) == len(frames) and all(len(st.frames) == LS.SLOTS for st in stims)


def test_the_issue_s_draw_decodes_unchanged():
    """seam_fuzz and spec_recon take 16 entries and 17 slots as they are: nothing in either had to change for this set"""
    rng = np.random.default_rng(16)
    pic = seam_fuzz.make_picture(rng, 8, 6, n_ref=16, n_ref_l1=16, slots=17, dst_slot=16, b_picture=True, weighted=True)
    from tests import residual_checker
    residual_checker.make_conformant(pic)
    spec = spec_recon.SpecRecon(8, 6, 17)
    for s in range(17):
        spec.store.write(s, seam_fuzz.random_frame(rng, 8, 6))
    out = spec.reconstruct(pic)
    assert out[0].shape == (96, 128)
    c = IC.survey(pic, IC.Census())
    assert {k[1] for k in c.entries if k[0] == 0} == set(range(16)) == {k[1] for k in c.entries if k[0] == 1}


def test_a_copied_picture_decodes_to_the_same_bytes(expected):
    for name in ("P dup 16", "B wp 16+16", "P cr 16", "B t8 16+16"):
        st = LS.by_name(name)
        twin = LS.copy_picture(st.pic)
        assert seam_fuzz.picture_digest(twin) == seam_fuzz.picture_digest(st.pic)
        for a, b in zip(LS.decode(st, twin), expected[name]):
            assert np.array_equal(a, b), name


@pytest.mark.parametrize("fault", list(LS.WRONG))
def test_every_stimulus_tells_the_wrong_decoder(expected, fault):
    decode, uses = LS.WRONG[fault]
    users = [st for st in LS.pictures() if uses(st)]
    names = [st.name for st in users]
    assert set(names) >= set(LS.MUST_USE[fault]), "%s: %s do not use the feature" % (fault, sorted(set(LS.MUST_USE[fault]) - set(names)))
    blind = []
    for st in users:
        got, want = decode(st), expected[st.name]
        luma = int((got[0] != want[0]).sum())
        chroma = int((got[1] != want[1]).sum()) + int((got[2] != want[2]).sum())
        print("%-28s %-24s luma %5d chroma %5d" % (fault, st.name, luma, chroma))
        if not luma or not chroma:
            blind.append((st.name, luma, chroma))
    assert not blind, "%s: pictures that cannot tell (name, luma bytes, chroma bytes): %s" % (fault, blind)


def test_pictures_that_do_not_use_a_feature_are_left_alone(expected):
    """the wrong decoders are wrong about ONE thing: a picture with short lists decodes as before under `index & 7`"""
    st = LS.by_name("P 8")
    assert not LS.WRONG["index & 7"][1](st)
    for a, b in zip(LS.WRONG["index & 7"][0](st), expected[st.name]):
        assert np.array_equal(a, b)
    st = LS.by_name("P 16")
    assert not LS.strengths_differ(st)
    for a, b in zip(LS.WRONG["strengths by index"][0](st), expected[st.name]):
        assert np.array_equal(a, b)
