"""A numpy model of the device export (include/p264hip.h: p264hip_export_t), written from its description alone: the byte
layouts of I420 / NV12 / RGB24 / planar RGB with a window, a pitch and a frame stride, and the fixed-point RGB arithmetic.
The checker of tests/test_export_cpu.py and tests/test_gpu_export*.py - never the product."""
from fractions import Fraction

import numpy as np

FORMATS = ("i420", "nv12", "rgb24", "rgbp")
K = {"bt601": (Fraction(299, 1000), Fraction(114, 1000)), "bt709": (Fraction(2126, 10000), Fraction(722, 10000))}


def rationals(matrix, full_range):
    """(cy, R.cv, G.cu, G.cv, B.cu) as exact fractions"""
    kr, kb = K[matrix]
    kg = 1 - kr - kb
    sy, sc = (Fraction(1), Fraction(1)) if full_range else (Fraction(255, 219), Fraction(255, 224))
    return sy, 2 * (1 - kr) * sc, -2 * kb * (1 - kb) * sc / kg, -2 * kr * (1 - kr) * sc / kg, 2 * (1 - kb) * sc


def coefficients(matrix, full_range):
    """the five integers: floor(c * 8192 + 1/2)"""
    return tuple(int((c * 8192 + Fraction(1, 2)).__floor__()) for c in rationals(matrix, full_range))


def rgb(y, cb, cr, matrix="bt601", full_range=False):
    """The fixed-point arithmetic on integer arrays of equal shape -> (R, G, B) uint8; also the largest |sum| met."""
    cy, rcv, gcu, gcv, bcu = coefficients(matrix, full_range)
    y = y.astype(np.int64) - (0 if full_range else 16)
    cb = cb.astype(np.int64) - 128
    cr = cr.astype(np.int64) - 128
    sums = (cy * y + rcv * cr + 4096, cy * y + gcu * cb + gcv * cr + 4096, cy * y + bcu * cb + 4096)
    return tuple(np.clip(s >> 13, 0, 255).astype(np.uint8) for s in sums), max(int(np.abs(s).max()) for s in sums)


def rgb_real(y, cb, cr, matrix="bt601", full_range=False):
    """clip(floor(real + 1/2)) in float64"""
    cy, rcv, gcu, gcv, bcu = (float(c) for c in rationals(matrix, full_range))
    y = y.astype(np.float64) - (0 if full_range else 16)
    cb = cb.astype(np.float64) - 128
    cr = cr.astype(np.float64) - 128
    real = (cy * y + rcv * cr, cy * y + gcu * cb + gcv * cr, cy * y + bcu * cb)
    return tuple(np.clip(np.floor(r + 0.5), 0, 255).astype(np.int64) for r in real)


def tight_pitch(fmt, w):
    return 3 * w if fmt == "rgb24" else w


def frame_bytes(fmt, w, h, pitch=0):
    p = pitch or tight_pitch(fmt, w)
    return {"i420": p * h * 3 // 2, "nv12": p * h * 3 // 2, "rgb24": p * h, "rgbp": 3 * p * h}[fmt]


def put_frame(dst, planes, fmt, crop, matrix="bt601", full_range=False, pitch=0):
    """One picture into dst (a uint8 array of at least frame_bytes): only the bytes the layout names are written."""
    y, u, v = planes
    x0, y0, w, h = crop
    p = pitch or tight_pitch(fmt, w)
    yw = y[y0:y0 + h, x0:x0 + w]
    uw = u[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]
    vw = v[y0 // 2:(y0 + h) // 2, x0 // 2:(x0 + w) // 2]

    def rows(off, row_pitch, n_rows, n_bytes):
        """a view of n_rows rows of n_bytes bytes, row_pitch apart, from byte `off` of dst"""
        return np.lib.stride_tricks.as_strided(dst[off:], (n_rows, n_bytes), (row_pitch, 1))
    if fmt in ("i420", "nv12"):
        rows(0, p, h, w)[:] = yw
        if fmt == "i420":
            rows(p * h, p // 2, h // 2, w // 2)[:] = uw
            rows(p * h + (p // 2) * (h // 2), p // 2, h // 2, w // 2)[:] = vw
        else:
            uv = np.empty((h // 2, w), np.uint8)
            uv[:, 0::2] = uw
            uv[:, 1::2] = vw
            rows(p * h, p, h // 2, w)[:] = uv
        return
    up = np.repeat(np.repeat(u, 2, axis=0), 2, axis=1)[y0:y0 + h, x0:x0 + w]      # nearest sample: (x >> 1, y >> 1) of the FRAME
    vp = np.repeat(np.repeat(v, 2, axis=0), 2, axis=1)[y0:y0 + h, x0:x0 + w]
    (r, g, b), _ = rgb(yw, up, vp, matrix, full_range)
    if fmt == "rgb24":
        rows(0, p, h, 3 * w)[:] = np.stack([r, g, b], axis=-1).reshape(h, 3 * w)
    else:
        for i, c in enumerate((r, g, b)):
            rows(i * p * h, p, h, w)[:] = c


def expected(frames, fmt, crop, matrix="bt601", full_range=False, pitch=0, frame_stride=0, offset=0, total=None, fill=0xA5):
    """The whole destination: `total` bytes of `fill` with picture i of `frames` (each (y, u, v)) at offset + i * frame_stride."""
    per = frame_bytes(fmt, crop[2], crop[3], pitch)
    stride = frame_stride or per
    need = offset + (len(frames) - 1) * stride + per
    dst = np.full(total if total is not None else need, fill, np.uint8)
    assert dst.size >= need
    for i, f in enumerate(frames):
        put_frame(dst[offset + i * stride:], f, fmt, crop, matrix, full_range, pitch)
    return dst
