"""p264hip_export_rois_device on the MI355X: the exports of per-picture windows from an ROI list that lives in device memory
(include/p264hip.h; csrc/hip/kernel_roi_dev.h).  The fixture is tests/test_gpu_roi.py's: 5 x 3 macroblocks, 3 streams x 2 slots of
random planes.  Every test prefills the whole destination with 0xA5 and compares ALL of it, floats as bytes, with
tests/roi_device_checker.py: the picture of every valid ROI as the host-list models have it, the prefill over every other picture
and round them.  Bit-exact, no tolerance.  The invalid ROIs are ones the rule rejects: a correct build reads nothing out of range."""
import ctypes as C

import numpy as np
import pytest

from p264decoder_amd import _native as N
from tests import resize_checker as R
from tests import roi_aa_checker as KA
from tests import roi_checker as K
from tests import roi_device_checker as DK
from tests.device_mem import DeviceBuffer
from tests.test_gpu_export import MB_H, MB_W, SLOTS, STREAMS, TAIL
from tests.test_gpu_resize import INSTANCES
from tests.test_gpu_roi import FILLS, MIXED, PICS, RECTANGLES, rotation, same, store  # noqa: F401  (store: the fixture)
from tests.test_gpu_roi_aa import MIXED as MIXED_AA

pytestmark = pytest.mark.gpu

AA = N.FILTER_BILINEAR_AA
FRAME, STORE = (MB_W * 16, MB_H * 16), (STREAMS, SLOTS)
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
FILTERS = {0: "bilinear", AA: "bilinear_aa"}


def rows10(rois):
    """rows of 6 or 10 members as an (n, 10) int32 array"""
    return np.array([tuple(r) + (0, 0, 0, 0) if len(r) == 6 else tuple(r) for r in rois], np.int64).astype(np.int32).reshape(len(rois), 10)


def on_device(lib, a):
    buf = DeviceBuffer(lib, a.nbytes)
    assert lib.p264hip_copy_to_device(buf.ptr, a.ctypes.data, a.nbytes) == 0
    return buf


def run(hip, planes, rois, size, fmt, dtype="u8", filter=0, fill=K.FILL, scale=None, bias=None, matrix="bt601", full=False, pitch=0, stride=0, offset=0,
        count=None, status=True, table=None, max_reduction=0, capacity=None):
    """one call into a prefilled destination; returns (what the device holds, what the model says it holds, the status words, the
    model's).  capacity: the n of the call (None: the list's); table: the slot table, through the C entry (the Python one has none)"""
    lib = hip.lib
    a = rows10(rois)
    n = len(a) if capacity is None else capacity
    per = R.frame_bytes(fmt, size[0], size[1], dtype, pitch)
    total = offset + (n - 1) * (stride or per) + per + TAIL
    dst = DeviceBuffer(lib, total)
    d_rois, d_count = on_device(lib, a), on_device(lib, np.array([count], np.int32)) if count is not None else None
    d_status = DeviceBuffer(lib, 4 * n + 8, 0x5A) if status else None
    out = (dst.ptr + offset, total - offset - TAIL)
    if table is None:
        hip.export_rois_device((d_rois.ptr, n), size, fmt, dtype, fill, scale, bias, matrix, full, pitch, stride, out, count=d_count.ptr if d_count else None,
                               status=d_status.ptr if status else False, filter=FILTERS[filter], max_reduction=max_reduction, stream=None)
    else:
        r = N.resize_desc(fmt, size, (0, 0, 2, 2), None, dtype, scale, bias, matrix, full, pitch, stride, filter)
        l = N.RoisDev(d_rois.ptr, d_count.ptr if d_count else None, d_status.ptr if status else None, (C.c_int32 * STREAMS)(*table), None, None, n, max_reduction, 0)
        assert lib.p264hip_export_rois_device(hip.h, C.byref(l), C.byref(r), N.fill_word(fill), out[0], out[1]) == 0, lib.p264hip_last_error()
        hip.sync()
    st = DK.statuses(a.tolist(), size, filter, FRAME, STORE, max_reduction, table, count)
    want = DK.expected(a.tolist(), st, planes, size, fmt, filter, dtype, fill, scale, bias, matrix, full, pitch, stride, offset, total, tag="store", table=table)
    got = dst.host()
    got_st = None
    if status:
        words = d_status.host()
        assert np.all(words[4 * n:] == 0x5A), "status words written behind the list"
        got_st = words[:4 * n].view(np.int32).tolist()
    for b in (dst, d_rois, d_count, d_status):
        if b is not None:
            b.free()
    return got, want, got_st, st


def host_list(hip, rois, size, fmt, dtype, filter, fill, kw):
    """what the host-list call writes for the same (valid) list"""
    per = R.frame_bytes(fmt, size[0], size[1], dtype, kw["pitch"])
    total = kw["offset"] + (len(rois) - 1) * (kw["stride"] or per) + per + TAIL
    dst = DeviceBuffer(hip.lib, total)
    call = hip.export_rois_aa if filter == AA else hip.export_rois
    call(rois, size, fmt, dtype, fill, kw["scale"], kw["bias"], kw["matrix"], kw["full"], kw["pitch"], kw["stride"], out=(dst.ptr + kw["offset"], total - kw["offset"] - TAIL))
    got = dst.host()
    dst.free()
    return got


def lists_of(filter):
    """(output, ROIs) of the instance sweep: the mixed lists and the rectangle lists of the host-list tests"""
    out = []
    for n, size in enumerate(((34, 18), (162, 98), (6, 70), (2, 2))):
        out.append((size, MIXED_AA[size] if filter == AA and size in MIXED_AA else MIXED[n % 7:] + MIXED[:n % 7]))
    for size, rects in RECTANGLES.items():
        rois = [MIXED[i % 7] + (rect if rect else (0, 0, 0, 0)) for i, rect in enumerate(rects)]
        rois += [MIXED[3][:2] + (16, 10) + rect[2:] + rect for rect in rects if rect and rect[2] <= 64 and rect[3] <= 38]
        out.append((size, rois))
    return out


@pytest.mark.parametrize("filter", [0, AA])
@pytest.mark.parametrize("fmt,dtype", INSTANCES)
def test_a_device_list_writes_what_the_host_list_writes(store, fmt, dtype, filter):
    hip, planes = store
    compared = 0
    for n, (size, rois) in enumerate(lists_of(filter)):
        kw = rotation(fmt, dtype, size, n + INSTANCES.index((fmt, dtype)))
        fill = FILLS[n % 3]
        got, want, got_st, st = run(hip, planes, rois, size, fmt, dtype, filter, fill, status=n % 2 == 0, **kw)
        what = "%s %s filter %d to %s, %s" % (fmt, dtype, filter, size, kw)
        assert got_st is None or got_st == st, what
        same(got, want, what + " against the model")
        if all(s == 0 for s in st):
            same(got, host_list(hip, rois, size, fmt, dtype, filter, fill, kw), what + " against the host list")
            compared += 1
        else:
            assert filter == AA and set(st) <= {0, DK.REDUCTION}
    assert compared >= (7 if filter == 0 else 4)


VALID = [(0, 0, 2, 2, 62, 30), (2, 1, 16, 10, 48, 22, 2, 2, 20, 10), (1, 0, 0, 0, 80, 48), (1, 1, 78, 46, 2, 2, 30, 14, 4, 4)]
# one ROI of every status 2 .. 10 (3 with the slot table [1, -1, 0]), and hostile 32-bit members the rule must reject before any use
INVALID = [
    (DK.BAD_PICTURE, (STREAMS, 0, 2, 2, 62, 30, 0, 0, 0, 0)), (DK.BAD_PICTURE, (I32_MAX, I32_MAX, 2, 2, 62, 30, 0, 0, 0, 0)), (DK.BAD_PICTURE, (0, SLOTS, 2, 2, 62, 30, 0, 0, 0, 0)),
    (DK.BAD_PICTURE, (I32_MIN, 0, 0, 0, 80, 48, 0, 0, 0, 0)), (DK.NO_PICTURE, (1, -1, 2, 2, 62, 30, 0, 0, 0, 0)),
    (DK.WINDOW_EMPTY, (0, 0, -2, 2, 62, 30, 0, 0, 0, 0)), (DK.WINDOW_EMPTY, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)), (DK.WINDOW_EMPTY, (0, 0, 2, I32_MIN, 62, 30, 0, 0, 0, 0)),
    (DK.WINDOW_ODD, (0, 0, 3, 2, 62, 30, 0, 0, 0, 0)), (DK.WINDOW_ODD, (0, 0, 2, 2, I32_MAX, 30, 0, 0, 0, 0)),
    (DK.WINDOW_OUTSIDE, (0, 0, 20, 2, 62, 30, 0, 0, 0, 0)), (DK.WINDOW_OUTSIDE, (0, 0, I32_MAX - 1, 2, I32_MAX - 1, 30, 0, 0, 0, 0)), (DK.WINDOW_OUTSIDE, (0, 0, 2, 2, 62, 2 ** 30, 0, 0, 0, 0)),
    (DK.RECT_SMALL, (0, 0, 2, 2, 62, 30, -2, 0, 10, 10)), (DK.RECT_SMALL, (0, 0, 2, 2, 62, 30, 0, 0, 0, 10)), (DK.RECT_SMALL, (0, 0, 2, 2, 62, 30, 0, 0, 10, I32_MIN)),
    (DK.RECT_ODD, (0, 0, 2, 2, 62, 30, 1, 0, 10, 10)), (DK.RECT_ODD, (0, 0, 2, 2, 62, 30, 0, 0, I32_MAX, 10)),
    (DK.RECT_OUTSIDE, (0, 0, 2, 2, 62, 30, 30, 0, 10, 10)), (DK.RECT_OUTSIDE, (0, 0, 2, 2, 62, 30, I32_MAX - 1, 0, I32_MAX - 1, 10)), (DK.RECT_OUTSIDE, (0, 0, 2, 2, 62, 30, 0, 2 ** 30, 10, 2 ** 30)),
    (DK.REDUCTION, (0, 0, 0, 0, 66, 30, 4, 4, 2, 10)), (DK.REDUCTION, (0, 0, 0, 0, 80, 48, 32, 16, 2, 2)),
]
TABLE = [1, -1, 0]


@pytest.mark.parametrize("fmt,dtype,filter", [("rgbp", "f32", AA), ("i420", "u8", AA), ("nv12", "u8", 0), ("rgb24", "f16", 0)])
def test_every_status_and_nothing_written_for_an_invalid_roi(store, fmt, dtype, filter):
    hip, planes = store
    size = (34, 18)
    rois, codes = [], []
    for i, (code, row) in enumerate(INVALID):
        rois += [VALID[i % 4], row]
        codes += [0, code if code != DK.REDUCTION or filter == AA else 0]
    rois += [(2, -1, 16, 10, 48, 22)]                       # slot -1 of a stream that has a picture: TABLE's slot 0
    codes += [0]
    kw = rotation(fmt, dtype, size, 5)
    got, want, got_st, st = run(hip, planes, rois, size, fmt, dtype, filter, FILLS[1], table=TABLE, **kw)
    assert st == codes and set(codes) == ({0} | set(range(2, 11)) if filter == AA else set(range(10)) - {1})
    assert got_st == codes
    same(got, want, "%s %s filter %d" % (fmt, dtype, filter))
    # every byte of an invalid picture's range is the prefill still (the model says so; here without a model)
    per = R.frame_bytes(fmt, size[0], size[1], dtype, kw["pitch"])
    for i, c in enumerate(codes):
        if c:
            at = kw["offset"] + i * (kw["stride"] or per)
            assert np.all(got[at:at + per] == 0xA5), i


def test_slot_minus_one_with_and_without_a_table(store):
    hip, planes = store
    rois = [(0, -1, 2, 2, 62, 30), (1, -1, 2, 2, 62, 30), (2, -1, 2, 2, 62, 30), (2, 1, 0, 0, 80, 48), (STREAMS, -1, 2, 2, 62, 30)]
    got, want, got_st, st = run(hip, planes, rois, (34, 18), "rgbp", "u8", 0, table=TABLE)
    assert got_st == st == [0, DK.NO_PICTURE, 0, 0, DK.BAD_PICTURE]
    same(got, want, "with the table")
    assert np.array_equal(got[:3 * 34 * 18], K.expected([(0, 1, 2, 2, 62, 30)], planes, (34, 18), "rgbp"))      # the table's slot 1, not slot 0
    got, want, got_st, st = run(hip, planes, rois, (34, 18), "rgbp", "u8", AA)
    assert got_st == st == [DK.BAD_PICTURE] * 3 + [0, DK.BAD_PICTURE]
    same(got, want, "without a table")


@pytest.mark.parametrize("filter", [0, AA])
def test_the_device_count(store, filter):
    hip, planes = store
    rois = [VALID[i % 4] for i in range(6)]
    rois[2] = INVALID[5][1]                                 # (an invalid ROI keeps its own status in front of the count, UNUSED behind it)
    n = len(rois)
    for count in (0, 1, n - 1, n, n + 5, -3):
        got, want, got_st, st = run(hip, planes, rois, (34, 18), "nv12", "u8", filter, count=count)
        used = min(max(count, 0), n)
        assert st == [DK.WINDOW_EMPTY if i == 2 else 0 for i in range(used)] + [DK.UNUSED] * (n - used) and got_st == st, count
        same(got, want, "count %d" % count)
    # no status wanted: the same bytes
    got, want, got_st, st = run(hip, planes, rois, (34, 18), "nv12", "u8", filter, count=4, status=False)
    assert got_st is None
    same(got, want, "without status words")


@pytest.mark.parametrize("filter,size", [(AA, (34, 18)), (0, (518, 4))])
def test_more_than_one_launch_pair(store, filter, size):
    """n = 2 * rois_per_pair + 1: three pairs of launches, the last with one ROI; the ROIs cycle through seven, so every ROI that
    opens or closes a pair, and the last of the call, is compared with the model of its kind"""
    hip, planes = store
    lib = hip.lib
    r = N.resize_desc("i420", size, (0, 0, 2, 2), None, filter=filter)
    per_pair = N.rois_device_plan(r, 0, lib)["rois_per_pair"]
    n = 2 * per_pair + 1
    # 2:1 and less in both directions for the first four; more for the others
    kinds = [(0, 0, 2, 2, 62, 30), (2, 1, 16, 10, 48, 22) + ((2, 0, 24, 12) if size == (34, 18) else (500, 0, 12, 4)), (1, 0, 0, 0, 68, 36), (1, 1, 78, 46, 2, 2, 30, 0, 4, 4),
             (0, 1, 0, 0, 80, 48, 0, 0, 8, 2), (2, 0, 0, 0, 64, 32, size[0] - 2, 2, 2, 2), (0, 0, 6, 4, 40, 44, 4, 0, 12, 4)]
    kinds = [k if len(k) == 10 else k + (0, 0, 0, 0) for k in kinds]
    which = (np.arange(n) * 3 + 2 * (np.arange(n) // per_pair)) % 7               # (the pattern shifts at the seams)
    assert which[per_pair - 1] != which[per_pair] and which[0] != which[per_pair] and which[n - 1] != which[0]
    a = np.array(kinds, np.int32)[which]
    per = R.frame_bytes("i420", *size)
    put = KA.expected if filter == AA else K.expected
    table = np.stack([put([k], planes, size, "i420", fill=(1, 2, 3)) for k in kinds])
    dst, d_rois, d_status = DeviceBuffer(lib, n * per + TAIL), on_device(lib, a), DeviceBuffer(lib, 4 * n)
    for m in ((0, 2) if filter == AA else (0,)):
        st = np.array([DK.status(k, size, filter, FRAME, STORE, m) for k in kinds])
        assert np.all(st == 0) if m == 0 else (set(st.tolist()) == {0, DK.REDUCTION} and np.all(st[:4] == 0))
        if m:
            assert N.rois_device_plan(r, m, lib)["rois_per_pair"] > n       # the same list in one pair now
        dst.fill(0xA5)
        hip.export_rois_device((d_rois.ptr, n), size, "i420", fill=(1, 2, 3), out=(dst.ptr, n * per), status=d_status.ptr, filter=FILTERS[filter], max_reduction=m, stream=None)
        got = dst.host()
        assert np.array_equal(d_status.host().view(np.int32), st[which]), m
        want = np.where((st[which] == 0)[:, None], table[which], np.uint8(0xA5))
        bad = np.flatnonzero(np.any(got[:n * per].reshape(n, per) != want, axis=1))
        assert bad.size == 0, "max_reduction %d: %d pictures differ, the first %d (pairs of %d)" % (m, bad.size, bad[0], per_pair)
        assert np.all(got[n * per:] == 0xA5)
    for b in (dst, d_rois, d_status):
        b.free()


def test_host_refusals_queue_nothing(store):
    hip, planes = store
    lib = hip.lib
    size = (34, 18)
    per = 3 * 34 * 18
    dst, d_rois, d_status = DeviceBuffer(lib, 2 * per + TAIL), on_device(lib, rows10(VALID[:2])), DeviceBuffer(lib, 16, 0x5A)

    def call(r, fill=N.fill_word(K.FILL), d=dst.ptr, cap=2 * per, ctx=hip.h, null=False, **kw):
        f = dict(rois_dev=d_rois.ptr, count_dev=None, status_dev=d_status.ptr, slot_of_stream=None, after_stream=None, before_stream=None, n=2, max_reduction=0, flags=0)
        f.update(kw)
        l = N.RoisDev(*[f[k] for k, _ in N.RoisDev._fields_])
        return lib.p264hip_export_rois_device(ctx, None if null else C.byref(l), C.byref(r) if r is not None else None, fill, d, cap)

    def D(filter=0, **kw):
        return N.resize_desc("rgbp", size, (0, 0, 2, 2), None, filter=filter, **kw)
    refused = [
        lambda: call(D(), ctx=None), lambda: call(D(), null=True), lambda: call(None), lambda: call(D(), d=None), lambda: call(D(), rois_dev=None), lambda: call(D(), rois_dev=d_rois.ptr + 4),
        lambda: call(D(), n=0), lambda: call(D(), fill=1 << 24), lambda: call(D(), max_reduction=2), lambda: call(D(AA), max_reduction=33), lambda: call(D(), flags=4),
        lambda: call(D(filter=1)), lambda: call(D(pitch=32)), lambda: call(D(dtype="f16"), d=dst.ptr + 1), lambda: call(D(), cap=2 * per - 1), lambda: call(D(), n=3),
        lambda: call(D(), slot_of_stream=(C.c_int32 * STREAMS)(0, SLOTS, 0)), lambda: call(D(AA), slot_of_stream=(C.c_int32 * STREAMS)(-2, 0, 0)),
    ]
    for i, f in enumerate(refused):
        assert f() == -1, "refusal %d" % i
        assert lib.p264hip_last_error().startswith(b"p264hip_export_rois_device:"), i
    hip.sync()
    assert np.all(dst.host() == 0xA5) and np.all(d_status.host() == 0x5A)
    assert call(D(AA), flags=3) == 0                        # both orders against the legacy default stream: the same bytes
    hip.sync()
    assert lib.hipDeviceSynchronize() == 0
    assert np.array_equal(dst.host(), KA.expected(VALID[:2], planes, size, "rgbp", total=2 * per + TAIL))
    assert d_status.host()[:8].view(np.int32).tolist() == [0, 0]
    for b in (dst, d_rois, d_status):
        b.free()


TORCH_CHILD = r"""
import sys
import torch                                   # first: the library then shares torch's HIP runtime
if not torch.cuda.is_available():
    print("no device")
    sys.exit(0)
sys.path.insert(0, %r)
import numpy as np
from p264decoder_amd import HipReconstructor
from p264decoder_amd.rois import rois_from_boxes
from tests import roi_device_checker as DK
hip = HipReconstructor(5, 3, n_streams=3, slots=2, max_pictures=1)
g = np.random.default_rng(2673)
for s in range(3):
    for k in range(2):
        hip.write_frame(s, k, g.integers(0, 256, (48, 80), np.uint8), g.integers(0, 256, (24, 40), np.uint8), g.integers(0, 256, (24, 40), np.uint8))
planes = {(s, k): hip.read_frame(s, k) for s in range(3) for k in range(2)}
size = (34, 18)
valid = [(0, 0, 2, 2, 62, 30, 0, 0, 0, 0), (2, 1, 16, 10, 48, 22, 2, 2, 20, 10), (1, 0, 0, 0, 80, 48, 0, 0, 0, 0), (1, 1, 78, 46, 2, 2, 30, 14, 4, 4)]
invalid = [(0, 0, 0, 0, 0, 0, 0, 0, 0, 0)] * 4
# ---- stream order: the list is what torch's current stream has queued, and torch's stream sees what the call wrote
for filter in ("bilinear", "bilinear_aa"):
    lst = torch.tensor(invalid, dtype=torch.int32, device="cuda")
    good = torch.tensor(valid, dtype=torch.int32, device="cuda")
    out = torch.full((4, 3, 18, 34), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        torch.cuda._sleep(10000000)
        lst.copy_(good, non_blocking=True)
        back, st = hip.export_rois_device(lst, size, "rgbp", out=out, status=True, filter=filter, stream="current")
        seen, seen_st = out.clone(), st.clone()
    torch.cuda.synchronize()
    assert back is out and st.dtype == torch.int32 and tuple(st.shape) == (4,)
    assert seen_st.cpu().tolist() == [0, 0, 0, 0], seen_st.cpu().tolist()
    f = 2 if filter == "bilinear_aa" else 0
    want = DK.expected(valid, [0] * 4, planes, size, "rgbp", f)
    assert np.array_equal(seen.cpu().numpy().reshape(-1), want), filter
# ---- a detector's boxes on the device: rois_from_boxes feeds the call, letterboxed, without the host seeing a box
boxes = torch.tensor([[2.5, 3.0, 60.2, 31.9], [0, 0, 80, 48], [70, 40, 200, 100], [10, 10, 10, 30], [float("nan"), 0, 5, 5], [-20, -20, -1, -1], [77.5, 45.5, 78.5, 46.5],
                      [4, 4, 30, 47], [30, 20, 10, 5]], dtype=torch.float32, device="cuda")
streams = torch.tensor([0, 1, 2, 0, 1, 2, 0, 1, 2], device="cuda")
slots = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1, 0], device="cuda")
for filter, dtype in (("bilinear_aa", "f32"), ("bilinear", "u8")):
    rois = rois_from_boxes(boxes, streams, slots, (80, 48), letterbox_to=size)
    scale = 1 / 255 if dtype == "f32" else None
    out, st = hip.export_rois_device(rois, size, "rgbp", dtype, scale=scale, status=True, filter=filter)
    rows = rois.cpu().tolist()
    f = 2 if filter == "bilinear_aa" else 0
    model = DK.statuses(rows, size, f, (80, 48), (3, 2))
    assert st.cpu().tolist() == model and model == [0, 0, 0, 4, 4, 4, 0, 0, 4], (st.cpu().tolist(), model)
    assert rows[0] == [0, 0, 2, 2, 60, 30, 0, 0, 34, 18] and rows[7][6:] == [12, 0, 10, 18], rows
    got = out.cpu().numpy().view(np.uint8).reshape(-1)
    want = DK.expected(rows, model, planes, size, "rgbp", f, dtype, scale=scale, prefill=0)
    per = want.size // 9
    for i, s in enumerate(model):                           # (a new tensor: the invalid pictures hold whatever it held)
        if s == 0:
            assert np.array_equal(got[i * per:(i + 1) * per], want[i * per:(i + 1) * per]), (filter, i)
hip.sync()
hip.close()
print("ok")
"""


def test_stream_order_and_boxes_from_torch():
    """in a process of its own, which imports torch BEFORE the library is loaded: the list tensor holds invalid ROIs; on a side stream a
    sleep and, behind it, a copy of the valid list over the tensor are queued, then the call with stream="current" and a clone of out
    - no host wait between them.  The clone holds the valid list's pictures and status 0 (without the wait for torch's stream it
    would hold the prefill).  Then rois_from_boxes on device tensors feeds the call."""
    import importlib.util
    import os
    import subprocess
    import sys
    if importlib.util.find_spec("torch") is None:          # (looked for, NOT imported: this process keeps the one HIP runtime it has)
        pytest.skip("no torch")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", TORCH_CHILD % root], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    if r.returncode == 0 and r.stdout.strip().endswith("no device"):
        pytest.skip("torch sees no device")
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-3000:]
