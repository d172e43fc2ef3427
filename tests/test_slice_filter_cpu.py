"""The checker for per-macroblock filter offsets (tests/slice_filter_checker.py) and the seam's `flags` on the host, no device:
the checker is deblock_checker where no record carries a delta; the pictures the GPU test decodes (tests/slice_filter_fuzz.py)
reach every cell of the coverage tables; the 16-byte record travels unchanged through the packed and the compact form."""
import collections
import ctypes as C

import numpy as np
from p264decoder_amd import HipReconstructor, _native as N
from tests import deblock_checker as dc
from tests import deblock_stim, oracle_bind, seam_fuzz
from tests import slice_filter_checker as sfc
from tests import slice_filter_fuzz as sff


def test_without_deltas_the_checker_is_the_deblock_checker(oracle):
    """deblock_checker's own stimulus set, every flags 0: the same bytes and the same census"""
    a, b = collections.Counter(), sfc.Counts()
    for st in deblock_stim.stimulus_set():
        assert not st.pic.rec["flags"].any()
        store = deblock_stim.store_of(st)
        before = [p.copy() for p in oracle_bind.reconstruct(oracle, store, st.pic, deblock=False)]
        one, two = [p.copy() for p in before], [p.copy() for p in before]
        dc.deblock(st.pic, one, a)
        sfc.deblock(st.pic, two, b)
        for plane, (x, y) in enumerate(zip(one, two)):
            assert np.array_equal(x, y), "%s plane %d" % (st.name, plane)
        assert any(not np.array_equal(x, y) for x, y in zip(before, one)), st.name
    assert a == b.census and sum(a.values()) > 10000
    assert not b.seams and not b.inner and not b.tells


def test_flags_encoding():
    for a, b in ((0, 0), (-128, 127), (127, -128), (-1, 1), (12, -12)):
        assert sfc.deltas_of(sfc.flags_of(a, b)) == (a, b)
    assert sfc.flags_of(0, 0) == 0 and sfc.flags_of(1, 0) == 1 and sfc.flags_of(0, 1) == 0x100 and sfc.flags_of(-1, -1) == 0xffff


def test_the_deltas_change_the_expected_pictures(oracle):
    """a filter that ignores `flags` (the oracle's, the parent's kernels) gives other bytes for the pictures that carry deltas"""
    for name in sff.FAMILIES:
        cases, _ = sff.family(oracle, name)
        differ = 0
        for c in cases:
            if c.mode is None or not c.pic.desc.deblock:
                assert c.mode is not None or not c.pic.rec["flags"].any()
                continue
            saved = c.pic.rec["flags"].copy()
            c.pic.rec["flags"][:] = 0
            plain = sff.expected(oracle, c.pic, c.refs)
            c.pic.rec["flags"][:] = saved
            differ += any(not np.array_equal(x, y) for x, y in zip(plain, c.want))
        assert differ >= 2, name


def test_coverage_of_the_drawn_families(oracle):
    """Lines that the filter works on and whose two macroblocks carry different offsets: every cell of {left, top macroblock edge} x
    {luma, chroma} x {strength below 4, equal to 4}, and the same for the inner edges of macroblocks whose offsets differ from the
    picture's (strength below 3 / equal to 3: an inner edge has no 4), counted and as lines whose result depends on WHOSE offsets
    are taken - over all families, and over the families of each edge-info instance on its own.  Deltas per slice run and per
    macroblock, over the whole int8 range and over -12 .. 12, all occur, next to pictures without deltas in every family."""
    all_counts = sff.total(oracle)
    assert not all_counts.missing(), all_counts.missing()
    for instance in ("fused", "one_list", "two_lists"):
        names = [n for n, f in sff.FAMILIES.items() if f[2] == instance]
        c = sff.total(oracle, names)
        assert not c.missing(), (instance, c.missing())
    for name, (mb_w, mb_h, instance, specs) in sff.FAMILIES.items():
        cases, counts = sff.family(oracle, name)
        assert sum(counts.tells.values()) > 0, name
        assert any(c.mode is None for c in cases), name
    modes = {spec[3] for f in sff.FAMILIES.values() for spec in f[3]}
    assert modes == {None, ("slice", 12), ("slice", "int8"), ("mb", 12), ("mb", "int8")}
    # I_PCM macroblocks carry deltas like any other
    pcm = [c.pic for n in ("pcm_p", "pcm_b_i") for c in sff.family(oracle, n)[0]]
    assert sum(int(((p.rec["mb_type"] == N.MB_IPCM) & (p.rec["flags"] != 0)).sum()) for p in pcm) > 50


def _all_pictures(oracle):
    return [(name, i, c.pic) for name in sff.FAMILIES for i, c in enumerate(sff.family(oracle, name)[0])]


def test_the_record_travels_unchanged_through_packed_and_compact_forms(lib, oracle):
    """expand(pack_compact(p)) == pack_input(p), p264hip_compact_check passes, and the records inside the packed block are the
    picture's sixteen bytes per macroblock, flags included - pictures with non-zero flags, I_PCM macroblocks with deltas among them"""
    with_flags = pcm_with_flags = 0
    for name, i, pic in _all_pictures(oracle):
        packed = HipReconstructor.pack(pic, lib)
        compact = HipReconstructor.pack_compact(pic, lib)
        assert lib.p264hip_compact_check(C.byref(pic.desc), compact.ctypes.data, compact.size) == 0, (name, i)
        back = HipReconstructor.expand_compact(pic, compact, lib)
        lay = N.InputLayout()
        assert lib.p264hip_input_layout(C.byref(pic.desc), C.byref(lay)) == 0
        raw = pic.rec.view(np.uint8).reshape(-1)
        for what, blk in (("packed", packed), ("expanded", back)):
            assert np.array_equal(blk[lay.off_mb:lay.off_mb + raw.size], raw), (name, i, what)
        for blk in (packed, back):
            assert np.array_equal(np.frombuffer(blk, seam_fuzz.MB_DT, pic.n_mb, lay.off_mb)["flags"], pic.rec["flags"])
        # section by section: everything a kernel reads is the same in both blocks
        sizes = {lay.off_mb: 16 * pic.n_mb, lay.off_mv: 64 * pic.n_mb, lay.off_ref: 4 * pic.n_mb, lay.off_i4: 16 * pic.n_mb, lay.off_coef: 32 * pic.desc.n_coef_blocks}
        if pic.desc.slice_type == N.SLICE_B:
            sizes.update({lay.off_mv_l1: 64 * pic.n_mb, lay.off_ref_l1: 4 * pic.n_mb, lay.off_weights: 512})
        if pic.desc.explicit_wp:
            sizes[lay.off_wp] = 384
        for off, size in sizes.items():
            assert np.array_equal(packed[off:off + size], back[off:off + size]), (name, i, off)
        with_flags += bool(pic.rec["flags"].any())
        pcm_with_flags += int(((pic.rec["mb_type"] == N.MB_IPCM) & (pic.rec["flags"] != 0)).sum())
    assert with_flags >= 20 and pcm_with_flags > 50


def test_any_int8_pair_is_accepted_by_the_upload_checks(lib, oracle):
    """the seam has no refusal for `flags`: the extreme pairs pack on both host roads"""
    pic = sff.family(oracle, "p_plain")[0][1].pic
    saved = pic.rec["flags"].copy()
    try:
        for a, b in ((-128, -128), (127, 127), (-128, 127), (127, -128)):
            pic.rec["flags"][:] = sfc.flags_of(a, b)
            HipReconstructor.pack(pic, lib)
            c = HipReconstructor.pack_compact(pic, lib)
            assert lib.p264hip_compact_check(C.byref(pic.desc), c.ctypes.data, c.size) == 0
    finally:
        pic.rec["flags"][:] = saved
