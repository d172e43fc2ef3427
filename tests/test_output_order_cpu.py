"""Pictures in display order (H.264 C.4.5.3; include/p264parse.h, include/p264pipe.h), without a GPU: the parser's rule against
tests/output_order_model.py on drawn sequences (p264parse_kat_output_order) and on the writer's streams, the safety of the slots it
hands out replayed on the host, what the VUI and the level give for D and R, and the pipeline's deliveries with device = -1.

The order counts of the streams are recomputed here from the writer's documented rule (output_order_model.bframes_pictures), never
asked of the parser."""
import ctypes as C
import random

import pytest

from p264decoder_amd import Parser, Pipeline
from p264decoder_amd import _native as N
from tests import output_order_model as M
from tests import synth_cases
from tests.stream_args import B_STREAMS, MMCO, REORDER, SLICED, SUB8X8
from tests.test_multiref import ARGS

MB = (5, 4)
REFS = 2
LEVEL = 40                                          # what the writer puts into every SPS
B_ARGS = "--mbw %d --mbh %d --frames %%d --seed %%d --refs %d --bframes %%d --coded 8 --maxlevel 6" % (MB[0], MB[1], REFS)


def b_stream(bframes, vui=None, frames=14, seed=7):
    args = B_ARGS % (frames, seed, bframes) + (" --vui-reorder %s" % vui if vui else "")
    return open(synth_cases.generate(args), "rb").read()


def depths(vui):
    """(D, R) of a B stream of this file: the restriction the writer puts down, or the level's MaxDpbFrames for both"""
    if vui is None:
        d = M.dpb_frames(LEVEL, MB[0], MB[1], REFS)
        return d, d
    n = int(vui.split(":")[0])
    return M.dpb_frames(LEVEL, MB[0], MB[1], REFS, max(n, REFS)), n


def parse(lib, data, depth="off"):
    """(per picture (dst_slot, the slots its lists name, its outputs), the flush, the parser's slots); depth "off": no output order"""
    ps = Parser(lib=lib)
    if depth != "off":
        ps.set_output_order(depth)
    pics = []
    for typ, idc, rbsp in N.split_annexb(lib, data):
        p = ps.feed(typ, idc, rbsp)
        if p is not None:
            d = p.desc
            refs = [d.ref_slot[i] for i in range(d.n_ref)] + ([d.ref_slot_l1[i] for i in range(d.n_ref_l1)] if d.slice_type == N.SLICE_B else [])
            pics.append((d.dst_slot, refs, ps.outputs() if depth != "off" else []))
    flush = ps.flush() if depth != "off" else []
    slots = ps.slots
    ps.close()
    return pics, flush, slots


def replay(pics, flush):
    """Walk the pictures in decode order with a map slot -> decode index of its last writer: every output names a slot whose last
    writer is that picture, no picture is written into a slot that waits or that its own lists name, every picture comes out once.
    Returns the decode indices in output order."""
    writer, waiting, order = {}, set(), []
    for i, (dst, refs, outs) in enumerate(pics + [(None, [], flush)]):
        if dst is not None:
            assert dst not in waiting, "picture %d is decoded into slot %d, whose picture still waits" % (i, dst)
            assert dst not in refs, "picture %d is decoded into slot %d, which its own lists name" % (i, dst)
            writer[dst] = i
            waiting.add(dst)
        for slot, _, idx, _ in outs:
            assert writer.get(slot) == idx, "output of picture %d names slot %d, last written by picture %s" % (idx, slot, writer.get(slot))
            assert slot in waiting
            waiting.discard(slot)
            order.append(idx)
    assert not waiting and sorted(order) == list(range(len(pics)))
    return order


# ---- the rule: C against the model ---------------------------------------------------------------------------------------------
def draw_sequence(rng, depth):
    """[(poc, flags)] in decode order: segments that begin with an IDR picture or one with operation 5 (order count 0, first of its
    segment in both orders); inside a segment the display order is permuted so that no picture has more than `depth` pictures that
    are decoded before it and shown after it"""
    seq = []
    for seg in range(rng.randint(1, 4)):
        m = rng.randint(1, 14)
        flag = N.OUT_IDR if seg == 0 or rng.random() < 0.5 else N.OUT_MMCO5
        seq.append((0 if flag == N.OUT_IDR else rng.randint(3, 40), flag))      # (the order count of an operation-5 picture counts as 0)
        left, done = list(range(1, m)), []
        while left:
            later = sum(1 for d in done if d > left[0])          # decoded before the first one still to come, shown after it
            k = rng.randrange(min(len(left), 5)) if later < depth and rng.random() < 0.6 else 0
            done.append(left.pop(k))
            seq.append((2 * done[-1], 0))
    return seq


def kat(lib, depth, seq):
    n = len(seq)
    poc, flags = (C.c_int * n)(*[s[0] for s in seq]), (C.c_int * n)(*[s[1] for s in seq])
    order, after = (C.c_int * n)(), (C.c_int * n)()
    assert lib.p264parse_kat_output_order(depth, n, poc, flags, order, after) == 0
    return list(order), list(after)


@pytest.mark.parametrize("depth", range(5))
def test_rule_c_against_the_model(lib, depth):
    rng = random.Random(2640 + depth)
    reordered = 0
    for _ in range(80):
        seq = draw_sequence(rng, depth)
        n = len(seq)
        order, after = kat(lib, depth, seq)
        per, flush, _ = M.run([(p, bool(f & N.OUT_IDR), bool(f & N.OUT_MMCO5), True) for p, f in seq], depth)
        assert order == [i for due in per for i in due] + flush
        assert after == [i for i, due in enumerate(per) for _ in due] + [n] * len(flush)
        assert sorted(order) == list(range(n))                   # every picture exactly once
        # order counts ascend strictly between two flushes: inside a segment; and the segments come out one after the other
        seg_of, s = [], -1
        for _, f in seq:
            s += 1 if f else 0
            seg_of.append(s)
        for a, b in zip(order, order[1:]):
            assert seg_of[a] < seg_of[b] or (seg_of[a] == seg_of[b] and (0 if seq[a][1] else seq[a][0]) < seq[b][0])
        for i in range(n):                                       # |W| <= R after every step
            assert i + 1 - sum(1 for a in after if a <= i) <= depth
        reordered += order != list(range(n))
    assert (reordered > 20) == (depth > 0)


# ---- the parser on streams -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vui", [None, "1", "3", "1:full"])
@pytest.mark.parametrize("bframes", [1, 2, 4])
def test_parser_on_streams(lib, bframes, vui):
    want = M.bframes_pictures(14, bframes)
    d, r = depths(vui)
    pics, flush, slots = parse(lib, b_stream(bframes, vui), None)
    assert len(pics) == 14 and slots == d + 1
    per, last, _ = M.run(want, r, d, REFS)
    assert [[o[2] for o in outs] for _, _, outs in pics] == per and [o[2] for o in flush] == last      # due exactly when the model says
    if vui is None:
        assert (d, r) == (16, 16) and not any(per) and len(last) == 14                                 # everything comes at the flush
    order = replay(pics, flush)
    assert order == sorted(range(14), key=lambda i: want[i][0])                                        # the writer's display order
    everything = [o for _, _, outs in pics for o in outs] + flush
    assert [o[1] for o in everything] == sorted(p[0] for p in want)                                    # ... with the order counts of its rule
    assert [o[3] for o in everything] == [True] + [False] * 13


def test_slots_run_out_before_the_depth_does(lib):
    """--vui-reorder 3 with --refs 2: D = 3, four slots, and two of them hold references - step 4 (no free slot) is what makes
    pictures due, not step 3"""
    want = M.bframes_pictures(14, 2)
    pics, flush, slots = parse(lib, b_stream(2, "3"), None)
    assert slots == 4
    per, last, model = M.run(want, 3, 3, REFS)
    assert model.bumped_for_room >= 1
    assert [[o[2] for o in outs] for _, _, outs in pics] == per and [o[2] for o in flush] == last
    _, _, unbounded = M.run(want, 3, None, REFS)
    assert unbounded.bumped_for_room == 0 and M.run(want, 3, None, REFS)[0] != per                     # (steps 1 - 3 alone give other moments)
    assert replay(pics, flush) == sorted(range(14), key=lambda i: want[i][0])


def test_a_second_idr_picture_flushes_the_first_stream(lib):
    for vui in (None, "1"):
        data = b_stream(2, vui, frames=8, seed=11) + b_stream(2, vui, frames=8, seed=12)
        want = M.bframes_pictures(8, 2) * 2
        d, r = depths(vui)
        pics, flush, slots = parse(lib, data, None)
        per, last, _ = M.run(want, r, d, REFS)
        assert len(pics) == 16 and slots == d + 1
        assert [[o[2] for o in outs] for _, _, outs in pics] == per and [o[2] for o in flush] == last
        order = replay(pics, flush)
        assert order == sorted(range(8), key=lambda i: want[i][0]) + [8 + i for i in sorted(range(8), key=lambda i: want[i][0])]
        # everything of the first stream is out when the second's IDR picture is complete, in front of it
        upto = [o[2] for _, _, outs in pics[:9] for o in outs]
        assert set(range(8)) <= set(upto) and all(upto.index(i) < len(upto) - (8 in upto) for i in range(8))


def test_override_zero_is_decode_order(lib):
    pics, flush, _ = parse(lib, b_stream(2, "1"), 0)
    assert [[o[2] for o in outs] for _, _, outs in pics] == [[i] for i in range(14)] == M.run(M.bframes_pictures(14, 2), 0, 2, REFS)[0]
    assert not flush
    replay(pics, flush)


@pytest.mark.parametrize("args", [ARGS] + SLICED + SUB8X8 + [REORDER] + MMCO)
def test_baseline_streams_come_out_with_themselves(lib, args):
    """pic_order_cnt_type 2: R = 0 (8.2.1.3), whatever the level's buffer holds"""
    a = args.split()
    mb_w, mb_h, refs = int(a[a.index("--mbw") + 1]), int(a[a.index("--mbh") + 1]), int(a[a.index("--refs") + 1]) if "--refs" in a else 1
    pics, flush, slots = parse(lib, open(synth_cases.generate(args), "rb").read(), None)
    assert len(pics) == int(a[a.index("--frames") + 1])
    assert slots == M.dpb_frames(LEVEL, mb_w, mb_h, refs) + 1
    assert [[o[2] for o in outs] for _, _, outs in pics] == [[i] for i in range(len(pics))] and not flush
    replay(pics, flush)


def test_off_is_off(lib):
    """Without p264parse_set_output_order: num_ref_frames + 1 slots, and every picture in the first slot that holds no reference
    (the IDR picture in slot 0) - computed here from the SPS's num_ref_frames and the writer's picture kinds, not by a second run"""
    args = B_STREAMS[0]
    a = args.split()
    refs, bframes, frames = int(a[a.index("--refs") + 1]), int(a[a.index("--bframes") + 1]), int(a[a.index("--frames") + 1])
    pics, flush, slots = parse(lib, open(synth_cases.generate(args), "rb").read())
    assert slots == refs + 1 and not flush
    held, cur, want = [], 0, []                     # held: (slot, decode index) of the references, oldest first
    for i, (_, idr, _, ref) in enumerate(M.bframes_pictures(frames, bframes)):
        if idr:
            held, cur = [], 0
        want.append(cur)
        if ref:
            if not idr and len(held) >= refs:
                held.pop(0)
            held.append((cur, i))
        cur = min(s for s in range(slots) if s not in [h[0] for h in held])
    assert [p[0] for p in pics] == want
    ps = Parser(lib=lib)
    assert ps.outputs() == [] and ps.flush() == []
    ps.close()


# ---- a damaged VUI -------------------------------------------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.bits = []

    def u(self, n, v):
        self.bits += [(v >> i) & 1 for i in range(n - 1, -1, -1)]

    def ue(self, v):
        n = (v + 1).bit_length() - 1
        self.u(n, 0)
        self.u(n + 1, v + 1)

    def rbsp(self):
        b = self.bits + [1]
        b += [0] * (-len(b) % 8)
        return bytes(sum(bit << (7 - k) for k, bit in enumerate(b[i:i + 8])) for i in range(0, len(b), 8))


def sps_head():
    """... up to vui_parameters_present_flag"""
    b = Bits()
    b.u(8, 77); b.u(8, 0x40); b.u(8, LEVEL); b.ue(0)
    b.ue(8 - 4); b.ue(0); b.ue(8 - 4)
    b.ue(REFS); b.u(1, 0); b.ue(MB[0] - 1); b.ue(MB[1] - 1)
    b.u(1, 1); b.u(1, 0); b.u(1, 0)
    return b


def sps_with_restriction(reorder, buffering):
    """the SPS of b_stream(...) as synth264 --vui-reorder writes it (main profile, order-count type 0), with these two numbers"""
    b = sps_head()
    b.u(1, 1)                                       # vui_parameters_present_flag
    for _ in range(7):                              # aspect ratio, overscan, video signal, chroma location, timing, NAL HRD, VCL HRD: absent
        b.u(1, 0)
    b.u(1, 0); b.u(1, 1)                            # pic_struct_present_flag, bitstream_restriction_flag
    b.u(1, 1); b.ue(2); b.ue(1); b.ue(16); b.ue(16); b.ue(reorder); b.ue(buffering)
    return b.rbsp()


def nals(lib, data):
    return list(N.split_annexb(lib, data))


def with_sps(lib, data, sps):
    """the stream's NAL units with its SPS replaced; outputs and slots of the parse with output order on"""
    ps = Parser(lib=lib)
    ps.set_output_order()
    outs, n = [], 0
    for typ, idc, rbsp in nals(lib, data):
        p = ps.feed(typ, idc, sps if typ == 7 else rbsp)
        if p is not None:
            n += 1
            outs.append([o[2] for o in ps.outputs()])
    flush, slots = [o[2] for o in ps.flush()], ps.slots
    ps.close()
    return n, outs, flush, slots


def test_a_damaged_vui_counts_as_absent(lib):
    data = b_stream(2, "1")
    sps = [rbsp for typ, _, rbsp in nals(lib, data) if typ == 7][0]
    assert sps == sps_with_restriction(1, 2)                              # (the SPS built here is the writer's)
    want = M.bframes_pictures(14, 2)
    fallback = M.run(want, 16, 16, REFS)
    assert with_sps(lib, data, sps) == (14, M.run(want, 1, 2, REFS)[0], M.run(want, 1, 2, REFS)[1], 3)
    assert with_sps(lib, data, sps_with_restriction(2, 4)) == (14, M.run(want, 2, 4, REFS)[0], M.run(want, 2, 4, REFS)[1], 5)
    for bad in (sps_with_restriction(17, 17), sps_with_restriction(17, 16), sps_with_restriction(3, 2), sps_with_restriction(0, 17)):
        assert with_sps(lib, data, bad) == (14, fallback[0], fallback[1], 17)
    # the writer's full VUI, cut inside the NAL HRD parameters (148 bits behind the flag, 109 bits each)
    full = b_stream(2, "1:full")
    sps_full = [rbsp for typ, _, rbsp in nals(lib, full) if typ == 7][0]
    assert with_sps(lib, full, sps_full)[3] == 3 and len(sps_full) > 50
    at = len(sps_head().bits) // 8                                        # the byte of vui_parameters_present_flag
    for cut in (at + 21, at + 27, at + 36):
        assert with_sps(lib, full, sps_full[:cut]) == (14, fallback[0], fallback[1], 17), cut


# ---- the pipeline without a device ---------------------------------------------------------------------------------------------
def pipeline_streams():
    base = "--mbw %d --mbh %d --frames 9 --gop 4 --seed 21 --coded 10 --maxlevel 6" % MB
    return [b_stream(2, "1"), b_stream(2, None, seed=8), open(synth_cases.generate(base), "rb").read()]


def pipeline_model(capacity):
    """the deliveries of pipeline_streams(): [[(stream, decode index)]], and the order count and IDR mark of every (stream, index)"""
    kinds = [M.bframes_pictures(14, 2), M.bframes_pictures(14, 2), M.baseline_pictures(9, 4)]
    runs = [M.run(kinds[0], 1, 2, REFS), M.run(kinds[1], 16, 16, REFS), M.run(kinds[2], 0, 16, 1)]
    rounds = [[run[0][r] if r < len(run[0]) else None for run in runs] for r in range(14)]
    about = {(s, i): (k[0], k[1]) for s, kind in enumerate(kinds) for i, k in enumerate(kind)}
    return M.deliveries(rounds, [run[1] for run in runs], capacity), about


@pytest.mark.parametrize("threads", [1, 4])
def test_pipeline_deliveries_without_a_device(lib, threads):
    streams = pipeline_streams()
    want, about = pipeline_model(3)
    pipe = Pipeline(streams, threads=threads, device=-1, lib=lib)
    with pytest.raises(RuntimeError):
        pipe.set_sink("i420", lambda *a: None)                    # decode order: a pipeline without a device has no sink
    pipe.set_output_order()
    seen = []

    def sink(d, which, dev, per):
        assert dev is None
        got = pipe.delivery()
        assert [g[0] for g in got] == list(which)
        seen.append((d, got))
    pipe.set_sink("i420", sink)
    st = pipe.run()
    assert pipe.delivery() == []
    pipe.close()
    assert st["pictures"] == 14 + 14 + 9 and st["rounds"] == 14
    assert [d for d, _ in seen] == list(range(len(want)))
    assert [[(g[0], g[2]) for g in got] for _, got in seen] == want
    assert all(about[(g[0], g[2])] == (g[1], g[3]) for _, got in seen for g in got)
    # (the flush - one picture of stream 0, all fourteen of stream 1 - is cut into five deliveries of three)
    assert max(len(w) for w in want) == 3 and sum(len(w) for w in want) == 37 and len(want) == len(pipeline_model(100)[0]) + 4
