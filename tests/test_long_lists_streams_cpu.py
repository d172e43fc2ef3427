"""Streams whose reference lists grow to 16 entries (tests/stream_args.py: LONG_LISTS), on the CPU: the host parser against the
stream writer's own records, the way tests/test_multiref.py, tests/test_bslices.py and tests/slice_streams.py compare theirs.

tools/synth264 writes --refs up to 16 with the sliding window alone, with --mmco and with --bframes; its model of the decoded
picture buffer (8.2.4, 8.2.5) is written separately from the parser's.  Per stream: the parsed list lengths grow to the stream's
--refs and stay there; the per-block indices and vectors equal --dump-mv; the PICTURE every quadrant predicts from equals
--dump-slices (which also holds every slice's lists as picture numbers); the parser hands out --refs + 1 slots and writes none
while a later list still names its picture; the 16 x 16 implicit weights equal 8.4.2.3.1 restated here from the pictures' order
counts; with the output order on, the slot count stays within 17 and no waiting picture is overwritten."""
import numpy as np
import pytest

from p264decoder_amd import Parser, _native as N
from tests import slice_streams, synth_cases
from tests.stream_args import LONG_LISTS

NAMES = list(LONG_LISTS)


def option(args, name, default=0):
    a = args.split()
    return int(a[a.index(name) + 1]) if name in a else default


@pytest.fixture(scope="module")
def parsed(lib, tmp_path_factory):
    """{name: (args, stream bytes, the parser's slots, pictures, --dump-mv bytes, --dump-slices bytes)}"""
    out = {}
    for name, args in LONG_LISTS.items():
        data, mv, sl = synth_cases.write_stream(tmp_path_factory.mktemp(name), args, "ll", dumps=("mv", "slices"))
        parser = Parser(quiet=True, lib=lib)
        pics = parser.parse_stream(data)
        out[name] = (args, data, parser.slots, pics, np.fromfile(mv, dtype=np.uint8), np.fromfile(sl, dtype=np.uint8))
    return out


def order_counts(args, n):
    """picture order count per decode index, from the structure the arguments name: the IDR picture, then groups of one P picture
    and the --bframes B pictures displayed in front of it, order count = 2 x display position"""
    b = option(args, "--bframes")
    out = []
    for i in range(n):
        if i == 0:
            out.append((0, False))
            continue
        pos, group = (i - 1) % (b + 1), (i - 1) // (b + 1) + 1
        out.append((2 * ((group - 1) * (b + 1) + pos), True) if pos else (2 * group * (b + 1), False))
    return out


def mv_records(args, pics, dump):
    """per picture what --dump-mv holds: vectors and indices of list 0 and - B streams - list 1, both lists as picture numbers, the
    writer's implicit weights; --mmco: list 0 as picture numbers"""
    n, at, out = pics[0].n_mb, 0, []
    for p in pics:
        def take(count, dtype):
            nonlocal at
            a = dump[at:at + count * np.dtype(dtype).itemsize].view(dtype)
            at += count * np.dtype(dtype).itemsize
            return a
        r = {"mv0": take(n * 32, np.int16).reshape(n, 16, 2), "rf0": take(n * 16, np.int8).reshape(n, 16)}
        if "--bframes" in args:
            r["mv1"], r["rf1"] = take(n * 32, np.int16).reshape(n, 16, 2), take(n * 16, np.int8).reshape(n, 16)
            r["l0"] = take(int(take(1, np.uint8)[0]), np.uint16).tolist()
            r["l1"] = take(int(take(1, np.uint8)[0]), np.uint16).tolist()
            if p.desc.slice_type == N.SLICE_B:
                r["w"] = take(len(r["l0"]) * len(r["l1"]), np.int16).reshape(len(r["l0"]), len(r["l1"]))
        if "--mmco" in args:
            r["l0"] = take(int(take(1, np.uint8)[0]), np.uint16).tolist()
        out.append(r)
    assert at == len(dump)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_the_lists_grow_to_the_window_and_stay_there(parsed, name):
    args, _, slots, pics, _, _ = parsed[name]
    refs, frames = option(args, "--refs"), option(args, "--frames")
    assert len(pics) == frames and slots == refs + 1 and (refs < 16 or slots == 17)
    p_lengths = [int(p.desc.n_ref) for p in pics if p.desc.slice_type == N.SLICE_P]
    if "--slice-lists" not in args:                            # (a slice of such a stream may shorten its list)
        assert p_lengths == sorted(p_lengths), p_lengths
    assert max(p_lengths) == refs and p_lengths[-1] == refs and p_lengths.count(refs) >= (4 if "--slice-lists" not in args else 2)
    if "--bframes" in args:
        b = [(int(p.desc.n_ref), int(p.desc.n_ref_l1)) for p in pics if p.desc.slice_type == N.SLICE_B]
        assert b[-1] == (refs, refs) and b.count((refs, refs)) >= 6 and [x[0] for x in b] == sorted(x[0] for x in b), b
        assert sum(p.desc.slice_type != N.SLICE_B for p in pics) > 17 or refs < 16
    else:
        assert frames > 17 or refs < 16


@pytest.mark.parametrize("name", NAMES)
def test_indices_and_vectors_equal_the_writers_record(parsed, name):
    args, _, _, pics, dump, _ = parsed[name]
    refs = option(args, "--refs")
    n = pics[0].n_mb
    quad = [0, 2, 8, 10]
    slot_pic, used = {}, [set(), set()]
    for i, (p, r) in enumerate(zip(pics, mv_records(args, pics, dump))):
        d = p.desc
        inter = p.mb_records()["mb_type"] > N.MB_IPCM
        if "--slice-lists" not in args:             # (per-slice lists: the parser renumbers a later slice's indices into the picture's
            #                                          one list, tests/slice_streams.py - there the PICTURES are compared, next test)
            assert np.array_equal(p.ref_idx.reshape(n, 4)[inter], r["rf0"][:, quad][inter]), "picture %d: list-0 indices" % i
        assert np.array_equal(p.mv.reshape(n, 16, 2)[inter], r["mv0"][inter]), "picture %d: list-0 vectors" % i
        used[0] |= set(p.ref_idx.reshape(n, 4)[inter].reshape(-1).tolist())
        if d.slice_type == N.SLICE_B:
            assert np.array_equal(p.ref_idx_l1.reshape(n, 4)[inter], r["rf1"][:, quad][inter]), "picture %d: list-1 indices" % i
            assert np.array_equal(p.mv_l1.reshape(n, 16, 2)[inter], r["mv1"][inter]), "picture %d: list-1 vectors" % i
            used[1] |= set(p.ref_idx_l1.reshape(n, 4)[inter].reshape(-1).tolist())
        if "l0" in r:                                           # the lists as the writer means them, as picture numbers
            assert [slot_pic[int(d.ref_slot[k])] for k in range(int(d.n_ref))] == r["l0"], "picture %d: list 0" % i
        if d.slice_type == N.SLICE_B:
            assert [slot_pic[int(d.ref_slot_l1[k])] for k in range(int(d.n_ref_l1))] == r["l1"], "picture %d: list 1" % i
        elif "--bframes" not in args and "--mmco" not in args and "--slice-lists" not in args:
            # the sliding window alone: the pictures before this one, the most recent first
            assert [slot_pic[int(d.ref_slot[k])] for k in range(int(d.n_ref))] == list(range(i - 1, max(i - 1 - refs, -1), -1)), "picture %d: list 0" % i
        if d.slice_type != N.SLICE_B:
            slot_pic[int(d.dst_slot)] = i
    # every index of the longest list is coded somewhere (te(v) / the CABAC unary binarisation up to refs - 1)
    assert used[0] - {-1} == set(range(refs)), sorted(used[0])
    if "--bframes" in args:
        assert used[1] - {-1} == set(range(refs)), sorted(used[1])


@pytest.mark.parametrize("name", NAMES)
def test_every_quadrant_predicts_from_the_picture_the_writer_meant(parsed, name):
    args, _, _, pics, _, dump = parsed[name]
    seen = slice_streams.check_against_dump(pics, dump)
    assert seen["quadrants"] > 40 * len(pics) // 2
    if "--slice-lists" in args:
        assert seen["pics_lists_differ"] >= 3


@pytest.mark.parametrize("name", NAMES)
def test_no_slot_is_written_while_a_list_still_names_it(parsed, name):
    """replayed on the host with the WRITER's lists (--dump-slices: every slice's lists as picture numbers): the picture a slot holds
    is overwritten only after the last picture whose lists name it"""
    args, _, slots, pics, _, dump = parsed[name]
    recs = slice_streams.records(dump, pics[0].n_mb)
    last_use = {}
    for i, rec in enumerate(recs):
        for pair in rec[5]:
            for lst in pair:
                for pic in lst:
                    last_use[int(pic)] = i
    holds, overwritten = {}, 0
    for i, p in enumerate(pics):
        d = p.desc
        dst = int(d.dst_slot)
        assert 0 <= dst < slots
        named = [int(d.ref_slot[k]) for k in range(int(d.n_ref))] + ([int(d.ref_slot_l1[k]) for k in range(int(d.n_ref_l1))] if d.slice_type == N.SLICE_B else [])
        assert dst not in named and all(0 <= s < slots for s in named), "picture %d" % i
        if dst in holds:
            overwritten += 1
            assert last_use.get(holds[dst], -1) < i, "picture %d is decoded into slot %d, whose picture %d is named by picture %d" % (i, dst, holds[dst], last_use[holds[dst]])
        holds[dst] = i
    assert overwritten >= 3 and len(holds) == slots


def implicit_weight(cur, poc0, poc1):
    """8.4.2.3.1 (implicit mode, frame pictures, short-term references): w0 of the pair, 32 where the standard falls back"""
    clip = lambda lo, hi, v: max(lo, min(hi, v))
    tb, td = clip(-128, 127, cur - poc0), clip(-128, 127, poc1 - poc0)
    if td == 0:
        return 32
    num = 16384 + abs(td) // 2
    tx = num // td if td > 0 else -(num // -td)                # "/": towards zero
    dsf = clip(-1024, 1023, (tb * tx + 32) >> 6)
    w1 = dsf >> 2
    return 32 if w1 < -64 or w1 > 128 else 64 - w1


def test_sixteen_by_sixteen_implicit_weights(parsed):
    args, _, _, pics, dump, _ = parsed["b_cabac_temporal"]
    poc = order_counts(args, len(pics))
    assert [is_b for _, is_b in poc] == [p.desc.slice_type == N.SLICE_B for p in pics]
    slot_pic, full, values = {}, 0, set()
    for i, (p, r) in enumerate(zip(pics, mv_records(args, pics, dump))):
        d = p.desc
        if d.slice_type != N.SLICE_B:
            slot_pic[int(d.dst_slot)] = i
            continue
        assert int(d.weighted_bipred) == 1 and not int(d.explicit_wp)
        n0, n1 = int(d.n_ref), int(d.n_ref_l1)
        got = np.array(d.bipred_weight[:]).reshape(16, 16)[:n0, :n1]
        want = np.array([[implicit_weight(poc[i][0], poc[slot_pic[int(d.ref_slot[a])]][0], poc[slot_pic[int(d.ref_slot_l1[b])]][0])
                          for b in range(n1)] for a in range(n0)])
        assert np.array_equal(got, want), "picture %d: weights %s, 8.4.2.3.1 gives %s" % (i, got.tolist(), want.tolist())
        assert np.array_equal(got, r["w"]), "picture %d: the writer meant %s" % (i, r["w"].tolist())
        full += (n0, n1) == (16, 16)
        values |= set(got.reshape(-1).tolist())
        if (n0, n1) == (16, 16):
            assert (got != got.T).any()                        # (r0, r1) and (r1, r0) are different pairs
    assert full >= 6 and len(values) > 20 and min(values) < 0 and max(values) > 64, sorted(values)


@pytest.mark.parametrize("name", NAMES)
def test_with_the_output_order_on_the_slots_stay_within_17(lib, parsed, name):
    from tests.test_output_order_cpu import parse, replay
    _, data, slots, pics, _, _ = parsed[name]
    got, flush, with_order = parse(lib, data, None)
    assert len(got) == len(pics) and slots <= with_order <= 17
    replay(got, flush)
    assert all(0 <= dst < with_order and all(0 <= s < with_order for s in refs) for dst, refs, _ in got)
