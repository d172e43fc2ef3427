"""B slices (BASELINE config 4's slice type; the reference rejects B macroblock types,
decoder/macroblock.c:168-171, and stops at decoder/lists.c:136): the host parser against the stream writer's own record -
two implementations written separately from the standard (csrc/host/parser.c, tools/synth264_b.h): both lists in
picture-order-count order, list-wise vector prediction over every B macroblock and sub-macroblock type, B_Skip / direct
prediction (spatial and temporal, with and without direct_8x8_inference), implicit weights.  Then (GPU) the parsed
pictures through the HIP kernels against the CPU oracle.  No reference decoder exists for these streams: parity with the
reference is unpinned here; what is pinned to it are the two bi-prediction combines (kat_bipred.npz)."""

import numpy as np
import pytest

from p264decoder_amd import Parser, _native as N
from tests import synth_cases
from tests.stream_args import B_STREAMS as STREAMS



def make(tmp_path, args):
    data, dump = synth_cases.write_stream(tmp_path, args, "b", dumps=("mv",))
    return data, np.fromfile(dump, dtype=np.uint8)


@pytest.mark.parametrize("args", STREAMS)
def test_parser_against_writer(lib, tmp_path, args):
    data, dump = make(tmp_path, args)
    parser = Parser(quiet=True, lib=lib)
    pics = parser.parse_stream(data)
    assert len(pics) == int(args.split("--frames ")[1].split()[0])
    n = pics[0].n_mb
    at, slot_pic, seen = 0, {}, dict(b=0, bi=0, l1_only=0, weights=set(), direct_zero=0)
    for i, p in enumerate(pics):
        def take(count, dtype):
            nonlocal at
            a = dump[at:at + count * np.dtype(dtype).itemsize].view(dtype)
            at += count * np.dtype(dtype).itemsize
            return a
        mv0, rf0 = take(n * 32, np.int16).reshape(n, 16, 2), take(n * 16, np.int8).reshape(n, 16)
        mv1, rf1 = take(n * 32, np.int16).reshape(n, 16, 2), take(n * 16, np.int8).reshape(n, 16)
        n0 = int(take(1, np.uint8)[0]); l0 = take(n0, np.uint16).tolist()
        n1 = int(take(1, np.uint8)[0]); l1 = take(n1, np.uint16).tolist()
        is_b = p.desc.slice_type == N.SLICE_B
        assert is_b == (n1 > 0), "picture %d: slice type" % i
        inter = p.mb_records()["mb_type"] > N.MB_IPCM
        quad = [0, 2, 8, 10]
        assert np.array_equal(p.ref_idx.reshape(n, 4)[inter], rf0[:, quad][inter]), "picture %d: list-0 indices" % i
        assert np.array_equal(p.mv.reshape(n, 16, 2)[inter], mv0[inter]), "picture %d: list-0 vectors" % i
        assert p.desc.n_ref == n0 and [slot_pic[p.desc.ref_slot[k]] for k in range(n0)] == l0, "picture %d: list 0" % i
        if is_b:
            assert np.array_equal(p.ref_idx_l1.reshape(n, 4)[inter], rf1[:, quad][inter]), "picture %d: list-1 indices" % i
            assert np.array_equal(p.mv_l1.reshape(n, 16, 2)[inter], mv1[inter]), "picture %d: list-1 vectors" % i
            assert p.desc.n_ref_l1 == n1 and [slot_pic[p.desc.ref_slot_l1[k]] for k in range(n1)] == l1, "picture %d: list 1" % i
            w = take(n0 * n1, np.int16).reshape(n0, n1)
            assert bool(p.desc.weighted_bipred) == ("--implicit" in args)
            got = np.array(p.desc.bipred_weight[:]).reshape(16, 16)[:n0, :n1]
            assert np.array_equal(got, w), "picture %d: implicit weights %s, the writer meant %s" % (i, got.tolist(), w.tolist())
            assert (p.mb_records()["mb_type"][inter] == N.MB_B).all()
            r0, r1 = p.ref_idx.reshape(n, 4)[inter], p.ref_idx_l1.reshape(n, 4)[inter]
            seen["b"] += 1
            seen["bi"] += int(((r0 >= 0) & (r1 >= 0)).sum())
            seen["l1_only"] += int(((r0 < 0) & (r1 >= 0)).sum())
            seen["weights"] |= set(w.reshape(-1).tolist())
            # unused lists carry index -1 and zero vectors (the seam's convention, include/p264hip.h)
            m0 = p.mv.reshape(n, 4, 4, 2)
            for q in range(4):
                off = p.ref_idx.reshape(n, 4)[:, q] < 0
                assert not m0[off][:, (q >> 1) * 2:(q >> 1) * 2 + 2, (q & 1) * 2:(q & 1) * 2 + 2].any()
        else:
            assert p.desc.dst_slot not in [p.desc.ref_slot[k] for k in range(n0)]
        if p.desc.slice_type != N.SLICE_B:                      # B pictures are not references here: their slot is free again at once
            slot_pic[p.desc.dst_slot] = i
        else:
            assert p.desc.dst_slot not in [p.desc.ref_slot[k] for k in range(n0)] + [p.desc.ref_slot_l1[k] for k in range(n1)]
    assert at == len(dump)
    assert seen["b"] >= 8 and seen["bi"] > 50 and seen["l1_only"] > 20
    if "--implicit" in args:
        assert len(seen["weights"] - {32}) >= 2, "implicit weights never left 32: %s" % seen["weights"]


@pytest.mark.gpu
@pytest.mark.parametrize("args", STREAMS)
def test_b_streams_hip_vs_oracle(lib, oracle, tmp_path, args):
    from p264decoder_amd import HipReconstructor
    from tests import oracle_bind
    data, _ = make(tmp_path, args)
    parser = Parser(quiet=True, lib=lib)
    pics = parser.parse_stream(data)
    mb_w, mb_h = pics[0].mb_w, pics[0].mb_h
    store = oracle_bind.FrameStore(mb_w, mb_h, parser.slots)
    hip = HipReconstructor(mb_w, mb_h, n_streams=1, slots=parser.slots, max_pictures=1, lib=lib)
    oracle.oracle_stats_reset()
    for i, p in enumerate(pics):
        want = oracle_bind.reconstruct(oracle, store, p)
        hip.submit(0, p)
        got = hip.read_frame(0, p.desc.dst_slot)
        for plane, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), "picture %d (slice type %d) plane %d differs" % (i, p.desc.slice_type, plane)
    import ctypes as C
    oracle.oracle_bipred_blocks.restype = C.c_longlong
    assert oracle.oracle_bipred_blocks() > 200
    hip.close()
