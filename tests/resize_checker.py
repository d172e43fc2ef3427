"""A numpy model of the resized device export (include/p264hip.h: p264hip_resize_t), written from its description alone: the tap
positions, the fixed-point bilinear sum and the float step.  The resized planes go to tests/export_checker.py (put_frame / rgb) for
the layouts and the RGB arithmetic: a resized export is the existing export of a virtual W x H picture.  The checker of
tests/test_resize_cpu.py and tests/test_gpu_resize*.py - never the product."""
import numpy as np

from tests import export_checker as X

DTYPES = {"u8": np.uint8, "f16": np.float16, "f32": np.float32}


def taps(S, D):
    """pos(d) for d = 0 .. D-1, in 1/256 of a source sample (int64)"""
    d = np.arange(D, dtype=np.int64)
    return np.clip(((2 * d + 1) * S * 256 + D) // (2 * D) - 128, 0, (S - 1) * 256)


def resize_plane(src, W, H):
    """src (a window, uint8, 2-D) -> (the H x W uint8 plane, the largest sum met)"""
    S_h, S_w = src.shape
    px, py = taps(S_w, W), taps(S_h, H)
    x0, fx, y0, fy = px >> 8, px & 255, py >> 8, py & 255
    x1, y1 = np.minimum(x0 + 1, S_w - 1), np.minimum(y0 + 1, S_h - 1)
    s = src.astype(np.int64)
    fx, fy = fx[None, :], fy[:, None]
    a, b, c, d = s[y0][:, x0], s[y0][:, x1], s[y1][:, x0], s[y1][:, x1]
    total = a * (256 - fx) * (256 - fy) + b * fx * (256 - fy) + c * (256 - fx) * fy + d * fx * fy + 32768
    return (total >> 16).astype(np.uint8), int(total.max())


def resize_real(src, W, H):
    """floor(float64 bilinear + 1/2) with sample centres at half positions and clamped taps"""
    S_h, S_w = src.shape

    def axis(S, D):
        p = np.clip((np.arange(D) + 0.5) * S / D - 0.5, 0, S - 1)
        i0 = np.floor(p).astype(np.int64)
        return i0, np.minimum(i0 + 1, S - 1), p - i0
    x0, x1, fx = axis(S_w, W)
    y0, y1, fy = axis(S_h, H)
    s = src.astype(np.float64)
    fx, fy = fx[None, :], fy[:, None]
    real = (s[y0][:, x0] * (1 - fx) + s[y0][:, x1] * fx) * (1 - fy) + (s[y1][:, x0] * (1 - fx) + s[y1][:, x1] * fx) * fy
    return np.floor(real + 0.5).astype(np.int64)


def resize_planes(planes, crop, size):
    """(y, u, v) of a frame -> the three resized planes of the window"""
    y, u, v = planes
    x0, y0, cw, ch = crop
    W, H = size
    return (resize_plane(y[y0:y0 + ch, x0:x0 + cw], W, H)[0],
            resize_plane(u[y0 // 2:(y0 + ch) // 2, x0 // 2:(x0 + cw) // 2], W // 2, H // 2)[0],
            resize_plane(v[y0 // 2:(y0 + ch) // 2, x0 // 2:(x0 + cw) // 2], W // 2, H // 2)[0])


def to_float(c, scale, bias, dtype):
    """the float step on a uint8 array: two separately rounded float32 operations, then the conversion"""
    e = c.astype(np.float32) * np.float32(scale)
    e = e + np.float32(bias)
    return e.astype(DTYPES[dtype])


def three(v):
    return (0.0, 0.0, 0.0) if v is None else tuple(v) if hasattr(v, "__len__") else (v, v, v)


def tight_pitch(fmt, W, dtype="u8"):
    return X.tight_pitch(fmt, W) * np.dtype(DTYPES[dtype]).itemsize


def frame_bytes(fmt, W, H, dtype="u8", pitch=0):
    p = pitch or tight_pitch(fmt, W, dtype)
    return {"i420": p * H * 3 // 2, "nv12": p * H * 3 // 2, "rgb24": p * H, "rgbp": 3 * p * H}[fmt]


def put_frame(dst, planes, fmt, crop, size, dtype="u8", scale=None, bias=None, matrix="bt601", full_range=False, pitch=0):
    """One resized picture into dst (a uint8 array of at least frame_bytes): only the bytes the layout names are written."""
    W, H = size
    ry, ru, rv = resize_planes(planes, crop, size)
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


def expected(frames, fmt, crop, size, dtype="u8", scale=None, bias=None, matrix="bt601", full_range=False, pitch=0, frame_stride=0, offset=0,
             total=None, fill=0xA5):
    """The whole destination: `total` bytes of `fill` with resized picture i of `frames` (each (y, u, v)) at offset + i * frame_stride."""
    per = frame_bytes(fmt, size[0], size[1], dtype, pitch)
    stride = frame_stride or per
    need = offset + (len(frames) - 1) * stride + per
    dst = np.full(total if total is not None else need, fill, np.uint8)
    assert dst.size >= need
    for i, f in enumerate(frames):
        put_frame(dst[offset + i * stride:], f, fmt, crop, size, dtype, scale, bias, matrix, full_range, pitch)
    return dst
