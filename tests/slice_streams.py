"""Streams whose slices differ in what H.264 makes a per-slice property (TEST INFRASTRUCTURE): disable_deblocking_filter_idc and
the filter offsets, reference-list reordering and num_ref_idx_active_override - written by tools/synth264 (--slice-deblock,
--slice-lists), with the writer's own record of what it means (--dump-slices): per macroblock its slice, idc and offsets, per 8x8
quadrant and list the PICTURE it predicts from.  `check_against_dump` compares a parse with that record; `expected_pictures`
decodes the parsed pictures on the CPU: the oracle's unfiltered reconstruction, then tests/slice_filter_checker.py."""

import numpy as np

from p264decoder_amd import Parser, _native as N
from tests import pcm_checker, synth_cases
from tests import slice_filter_checker as sfc

BOTH = "--slice-deblock --slice-lists"
STREAMS = {
    # CAVLC and CABAC, P and B, 2 - 4 slices, small pictures including one macroblock row and one column
    "p_cavlc_2": "--mbw 9 --mbh 7 --frames 10 --gop 10 --seed 101 --refs 2 --slices 2 --coded 15 --maxlevel 6 --qp 34 " + BOTH,
    "p_cavlc_4_sub8x8": "--mbw 8 --mbh 6 --frames 12 --gop 12 --seed 102 --refs 2 --slices 4 --sub8x8 --qp-delta 6 --coded 15 --maxlevel 6 --qp 36 " + BOTH,
    "p_cabac_3": "--mbw 9 --mbh 6 --frames 10 --gop 10 --seed 103 --refs 2 --slices 3 --cabac --coded 15 --maxlevel 6 --qp 34 " + BOTH,
    "b_cavlc_3": "--mbw 8 --mbh 6 --frames 16 --seed 104 --refs 3 --bframes 2 --slices 3 --sub8x8 --coded 10 --maxlevel 6 --qp 34 " + BOTH,
    "b_cavlc_temporal_4": "--mbw 7 --mbh 6 --frames 17 --seed 105 --refs 4 --bframes 3 --temporal --d8inf --implicit --slices 4 --coded 8 --maxlevel 6 --qp 36 " + BOTH,
    "b_cabac_spatial_2": "--mbw 8 --mbh 5 --frames 13 --seed 106 --refs 3 --bframes 2 --implicit --slices 2 --cabac --coded 10 --maxlevel 6 --qp 34 " + BOTH,
    "b_cabac_temporal_3": "--mbw 7 --mbh 5 --frames 13 --seed 107 --refs 3 --bframes 1 --temporal --slices 3 --cabac --coded 10 --maxlevel 6 --qp 36 " + BOTH,
    "row_p_cavlc": "--mbw 11 --mbh 1 --frames 8 --gop 8 --seed 108 --refs 2 --slices 3 --coded 20 --maxlevel 6 --qp 34 " + BOTH,
    "column_b_cabac": "--mbw 1 --mbh 9 --frames 11 --seed 109 --refs 2 --bframes 1 --slices 4 --cabac --coded 20 --maxlevel 6 --qp 34 " + BOTH,
    "ipcm_p_cavlc": "--mbw 8 --mbh 6 --frames 8 --gop 8 --seed 110 --refs 2 --slices 3 --ipcm 12 --coded 15 --maxlevel 6 --qp 36 " + BOTH,
    # each property on its own
    "only_deblock_p": "--mbw 9 --mbh 7 --frames 8 --gop 8 --seed 111 --slices 4 --coded 15 --maxlevel 6 --qp 38 --slice-deblock",
    "only_lists_b": "--mbw 8 --mbh 6 --frames 13 --seed 112 --refs 3 --bframes 2 --slices 3 --coded 10 --maxlevel 6 --slice-lists",
}


def make(tmp_path, args, extra=()):
    """(stream bytes, the --dump-slices record as bytes)"""
    data, dump = synth_cases.write_stream(tmp_path, " ".join([args, *extra]), dumps=("slices",))
    return data, np.fromfile(dump, dtype=np.uint8)


def records(dump, n_mb):
    """per picture (slice int8[n], idc int8[n], alpha int8[n], beta int8[n], pictures int16[2][n][4], [(list 0, list 1) per slice])"""
    out = []
    at = 0
    while at < len(dump):
        s = dump[at:at + n_mb * 4].view(np.int8).reshape(n_mb, 4)
        at += n_mb * 4
        q = dump[at:at + 2 * n_mb * 4 * 2].view(np.int16).reshape(2, n_mb, 4)
        at += 2 * n_mb * 4 * 2
        ns = int(dump[at:at + 2].view(np.int16)[0])
        at += 2
        lists = []
        for _ in range(ns):
            pair = []
            for X in range(2):
                k = int(dump[at:at + 2].view(np.int16)[0])
                pair.append(dump[at + 2:at + 2 + 2 * k].view(np.int16).tolist())
                at += 2 + 2 * k
            lists.append(tuple(pair))
        out.append((s[:, 0], s[:, 1], s[:, 2], s[:, 3], q, lists))
    assert at == len(dump)
    return out


def check_against_dump(pics, dump, seen=None):
    """every macroblock's offsets (descriptor + flags) and `edges`, every inter quadrant's reference PICTURE in both lists, against the
    writer's record; tracks which decoded picture sits in which frame-store slot.  seen: a dict of what the stream contained."""
    n = pics[0].n_mb
    recs = records(dump, n)
    assert len(recs) == len(pics)
    seen = {} if seen is None else seen
    for k in ("pics_offsets_differ", "pics_lists_differ", "pics_with_deltas", "idc1_slices", "quadrants"):
        seen.setdefault(k, 0)
    slot_pic = {}
    for i, (p, (sl, idc, alpha, beta, qpic, lists)) in enumerate(zip(pics, recs)):
        d = p.desc
        rec = p.mb_records()
        # the picture's lists: the first P / B slice's verbatim, then whatever the later slices add; every entry of every slice is there
        coded = [pair for pair in lists if pair[0]]
        for X, (slots, n_list) in enumerate(((d.ref_slot, d.n_ref), (d.ref_slot_l1, d.n_ref_l1))):
            canon = [slot_pic[int(slots[k])] for k in range(n_list)]
            per_slice = [pair[X] for pair in coded if X == 0 or d.slice_type == N.SLICE_B]
            if per_slice:
                assert canon[:len(per_slice[0])] == per_slice[0], "picture %d list %d: %s does not start with the first slice's %s" % (i, X, canon, per_slice[0])
                assert set(canon) == set(sum(per_slice, [])), "picture %d list %d: %s against the slices' %s" % (i, X, canon, per_slice)
                seen["pics_lists_differ"] += any(l != per_slice[0] for l in per_slice)
                seen["lists_grew"] = seen.get("lists_grew", 0) + (len(canon) > len(per_slice[0]))
                seen["lengths_differ"] = seen.get("lengths_differ", 0) + (len({len(l) for l in per_slice}) > 1)
            else:
                assert n_list == 0 or (X == 1 and d.slice_type != N.SLICE_B)
        for m in range(n):
            what = "picture %d macroblock %d (slice %d)" % (i, m, sl[m])
            if idc[m] == 1:
                assert rec["edges"][m] == 0 and rec["flags"][m] == 0, what
            else:
                assert rec["edges"][m] & N.EDGE_INNER, what
                assert sfc.offsets_of(p, m) == (int(alpha[m]), int(beta[m])), "%s: offsets %s, the writer meant %s" % (what, sfc.offsets_of(p, m), (alpha[m], beta[m]))
            inter = rec["mb_type"][m] > N.MB_IPCM
            for q in range(4):
                for X, (idx, slots, n_list) in enumerate(((p.ref_idx, d.ref_slot, d.n_ref), (getattr(p, "ref_idx_l1", None), d.ref_slot_l1, d.n_ref_l1))):
                    want = int(qpic[X][m][q])
                    r = int(idx[m * 4 + q]) if inter and (X == 0 or d.slice_type == N.SLICE_B) else -1
                    if want < 0:
                        assert r < 0, "%s quadrant %d list %d: index %d, the writer meant none" % (what, q, X, r)
                    else:
                        assert 0 <= r < n_list, "%s quadrant %d list %d: index %d of %d" % (what, q, X, r, n_list)
                        assert slot_pic[int(slots[r])] == want, "%s quadrant %d list %d: index %d names picture %d, the writer meant %d" % (what, q, X, r, slot_pic[int(slots[r])], want)
                        seen["quadrants"] += 1
        filt = idc != 1
        seen["pics_offsets_differ"] += len({(int(a), int(b)) for a, b in zip(alpha[filt], beta[filt])}) > 1
        seen["idc1_slices"] += len(set(sl[~filt].tolist()))
        seen["pics_with_deltas"] += int(rec["flags"].any())
        if d.slice_type != N.SLICE_B:                           # (B pictures are not references in these streams)
            slot_pic[int(d.dst_slot)] = i
    return seen


def expected_pictures(oracle, pics, slots):
    """the decoded pictures [[y, u, v]] of a parsed stream: per picture the oracle's unfiltered reconstruction (pcm_checker composes
    explicit weights and I_PCM around it), then the checker's loop filter with every macroblock's own offsets"""
    chk = pcm_checker.PcmChecker(oracle, pics[0].mb_w, pics[0].mb_h, slots)
    out = []
    for p in pics:
        planes = chk.nodeblock(p)
        if p.desc.deblock:
            work = [a.copy() for a in planes]
            sfc.deblock(p, work)
            for dst, src in zip(planes, work):
                dst[:] = src
        out.append([a.copy() for a in chk.store[p.desc.dst_slot]])
    return out


def parse(lib, data):
    parser = Parser(quiet=True, lib=lib)
    return parser, parser.parse_stream(data)


# ---- slices that agree: the existing sliced streams, whose parse must stay what it was ------------------------------------------
# (the sliced streams of tests/test_gpu_weighted_pred.py, tests/test_bslices.py and tests/test_cabac_streams.py; their digests under
# tests/golden/sliced_streams_parse.json were recorded from the commit before slices could differ)
AGREEING = {
    "wp_p_2": "--mbw 8 --mbh 6 --frames 8 --gop 0 --seed 81 --refs 2 --sub8x8 --slices 2 --coded 25 --maxlevel 8 --wp",
    "wp_mmco_2": "--mbw 10 --mbh 7 --frames 8 --gop 0 --seed 101 --refs 3 --mmco --sub8x8 --slices 2 --coded 25 --maxlevel 8 --wp",
    "wp_b_temporal_2": "--mbw 9 --mbh 6 --frames 10 --seed 103 --refs 3 --bframes 2 --temporal --slices 2 --coded 25 --maxlevel 8 --wp --wp-bi",
    "b_temporal_implicit_2": "--mbw 7 --mbh 5 --frames 25 --seed 85 --refs 4 --bframes 3 --temporal --d8inf --implicit --slices 2 --coded 8 --maxlevel 6",
    "cabac_p_3": "--mbw 8 --mbh 6 --frames 10 --gop 0 --seed 102 --refs 2 --sub8x8 --slices 3 --coded 20 --maxlevel 12 --cabac",
    "cabac_b_temporal_2": "--mbw 7 --mbh 6 --frames 16 --seed 105 --refs 3 --bframes 3 --temporal --d8inf --slices 2 --coded 10 --maxlevel 8 --qp-delta 4 --cabac",
}


def parse_digest(pics):
    """per picture: SHA-256 (first 16 hex digits) over the descriptor's fields and every array"""
    import hashlib
    out = []
    for p in pics:
        d = p.desc
        h = hashlib.sha256()
        scal = [d.mb_w, d.mb_h, d.slice_type, d.chroma_qp_offset, d.deblock, d.alpha_c0_offset, d.beta_offset, d.dst_slot, d.n_ref, d.n_coef_blocks,
                d.frame_num, d.n_ref_l1, d.weighted_bipred, d.explicit_wp, d.wp_log2_denom[0], d.wp_log2_denom[1]]
        h.update(np.array(scal + list(d.ref_slot) + list(d.ref_slot_l1) + list(d.bipred_weight), np.int64).tobytes())
        h.update(np.ctypeslib.as_array(d.wp).astype(np.int64).tobytes())
        arrays = [p.mb, p.mv, p.ref_idx, p.i4modes, p.coefs[:16 * int(d.n_coef_blocks)]]
        if d.slice_type == N.SLICE_B:
            arrays += [p.mv_l1, p.ref_idx_l1]
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        out.append(h.hexdigest()[:16])
    return out
