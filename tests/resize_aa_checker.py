"""A numpy model of the ANTIALIASED filter of the resized device export (include/p264hip.h: P264HIP_FILTER_BILINEAR_AA), written from
its definition alone: the integer taps, the two passes with one rounding each (vertical first), and the exact real-valued filter to
hold them against.  Layouts, RGB and the float step are the existing ones: tests/export_checker.py's put_frame and
tests/resize_checker.py's to_float / tight_pitch / frame_bytes, imported.  The checker of tests/test_resize_aa_cpu.py and
tests/test_gpu_resize_aa*.py - never the product."""
import numpy as np

from tests import export_checker as X
from tests.resize_checker import frame_bytes, three, tight_pitch, to_float

MAX_TAPS = 64


def aa_taps(S, D):
    """(first[D], count[D], weights[D, 64]) of an axis with S source and D destination samples: Python integers throughout"""
    U = 2 * max(S, D)
    first, count, weights = np.zeros(D, np.int64), np.zeros(D, np.int64), np.zeros((D, MAX_TAPS), np.int64)
    for d in range(D):
        c = (2 * d + 1) * S
        # r(j) > 0  <=>  c - U < (2j+1) D < c + U; the j around the centre, then those inside 0 .. S-1
        lo = max((c - U - D) // (2 * D) + 1, 0)
        hi = min(-((-(c + U - D)) // (2 * D)) - 1, S - 1)
        r = [U - abs((2 * j + 1) * D - c) for j in range(lo, hi + 1)]
        assert r and min(r) > 0
        assert lo == 0 or U - abs((2 * lo - 1) * D - c) <= 0
        assert hi == S - 1 or U - abs((2 * hi + 3) * D - c) <= 0
        R = sum(r)
        w = [x * 32768 // R for x in r]
        w[r.index(max(r))] += 32768 - sum(w)
        first[d], count[d] = lo, len(r)
        weights[d, :len(r)] = w
    return first, count, weights


def _matrix(S, D):
    """the D x S matrix of an axis' weights (int64)"""
    first, count, w = aa_taps(S, D)
    m = np.zeros((D, S), np.int64)
    for d in range(D):
        m[d, first[d]:first[d] + count[d]] = w[d, :count[d]]
    return m, int(count.max())


def resize_plane_aa(src, W, H):
    """src (a window, uint8, 2-D) -> (the H x W uint8 plane, the largest sum of pass 1, of pass 2, (nx, ny) the largest tap counts)"""
    S_h, S_w = src.shape
    my, ny = _matrix(S_h, H)
    mx, nx = _matrix(S_w, W)
    # (the products in float64: every partial sum is an integer below 2^30, so they are exact - and numpy multiplies them fast)
    s1 = (my.astype(np.float64) @ src.astype(np.float64)).astype(np.int64)         # H x S_w
    t = (s1 + 256) >> 9
    s2 = (t.astype(np.float64) @ mx.T.astype(np.float64)).astype(np.int64)          # H x W
    v = (s2 + (1 << 20)) >> 21
    assert v.min() >= 0 and v.max() <= 255 and t.max() <= 16320
    return v.astype(np.uint8), int(s1.max()), int(s2.max()), (nx, ny)


def real_aa(src, W, H):
    """the exact filter in float64: the triangle r(j) / R on both axes, samples outside the window dropped and the rest renormalised"""
    def axis(S, D):
        U = 2.0 * max(S, D)
        j, d = np.arange(S, dtype=np.float64)[None, :], np.arange(D, dtype=np.float64)[:, None]
        r = np.maximum(U - np.abs((2 * j + 1) * D - (2 * d + 1) * S), 0.0)
        return r / r.sum(axis=1, keepdims=True)
    return axis(src.shape[0], H) @ src.astype(np.float64) @ axis(src.shape[1], W).T


def bound(nx, ny):
    """|v - real| of include/p264hip.h for an axis pair with at most nx and ny taps"""
    return 0.5 + 1.0 / 128 + 255.0 * (nx + ny - 2) / 32768


def resize_planes_aa(planes, crop, size):
    """(y, u, v) of a frame -> the three resized planes of the window"""
    y, u, v = planes
    x0, y0, cw, ch = crop
    W, H = size
    return (resize_plane_aa(y[y0:y0 + ch, x0:x0 + cw], W, H)[0],
            resize_plane_aa(u[y0 // 2:(y0 + ch) // 2, x0 // 2:(x0 + cw) // 2], W // 2, H // 2)[0],
            resize_plane_aa(v[y0 // 2:(y0 + ch) // 2, x0 // 2:(x0 + cw) // 2], W // 2, H // 2)[0])


def put_frame_aa(dst, planes, fmt, crop, size, dtype="u8", scale=None, bias=None, matrix="bt601", full_range=False, pitch=0):
    """One resized picture into dst (a uint8 array of at least frame_bytes): only the bytes the layout names are written."""
    W, H = size
    ry, ru, rv = resize_planes_aa(planes, crop, size)
    if dtype == "u8":
        X.put_frame(dst, (ry, ru, rv), fmt, (0, 0, W, H), matrix, full_range, pitch)
        return
    assert fmt in ("rgb24", "rgbp")
    up, vp = (np.repeat(np.repeat(c, 2, axis=0), 2, axis=1) for c in (ru, rv))       # the chroma sample (x >> 1, y >> 1)
    chans, _ = X.rgb(ry, up, vp, matrix, full_range)
    f = [to_float(c, s, b, dtype) for c, s, b in zip(chans, three(scale), three(bias))]
    elem = f[0].itemsize
    p = pitch or tight_pitch(fmt, W, dtype)

    def rows(off, n_bytes):
        return np.lib.stride_tricks.as_strided(dst[off:], (H, n_bytes), (p, 1))
    if fmt == "rgb24":
        rows(0, 3 * W * elem)[:] = np.ascontiguousarray(np.stack(f, axis=-1)).view(np.uint8).reshape(H, 3 * W * elem)
    else:
        for i, c in enumerate(f):
            rows(i * p * H, W * elem)[:] = np.ascontiguousarray(c).view(np.uint8).reshape(H, W * elem)


def expected_aa(frames, fmt, crop, size, dtype="u8", scale=None, bias=None, matrix="bt601", full_range=False, pitch=0, frame_stride=0, offset=0,
                total=None, fill=0xA5):
    """The whole destination: `total` bytes of `fill` with resized picture i of `frames` (each (y, u, v)) at offset + i * frame_stride."""
    per = frame_bytes(fmt, size[0], size[1], dtype, pitch)
    stride = frame_stride or per
    need = offset + (len(frames) - 1) * stride + per
    dst = np.full(total if total is not None else need, fill, np.uint8)
    assert dst.size >= need
    for i, f in enumerate(frames):
        put_frame_aa(dst[offset + i * stride:], f, fmt, crop, size, dtype, scale, bias, matrix, full_range, pitch)
    return dst
