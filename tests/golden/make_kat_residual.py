#!/usr/bin/env python3
"""Records known-answer vectors of the residual path at levels a conformant stream can carry, at EVERY QP, by calling the REAL
reference's function tables (oracle/_ref/libp264ref_kat.so = reference objects + oracle/ref_kat.c).  kat_hotpath.npz draws its
levels from +-40 (4x4 blocks) and +-300 (DC blocks) whatever the QP: above QP 32 every one of its cases leaves the range H.264
bounds (8.5.10 - 8.5.12), so its in-range cases - the only ones the standard defines a result for - stop there.  Here the
magnitudes shrink with the quantiser step, as an encoder's levels do.  Its own file and generator: kat_hotpath.npz stays
byte-identical.  Output: tests/golden/kat_residual.npz (inputs and the reference's outputs only)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libp264ref_kat.so"))
assert lib.refk_init() == 0
rng = np.random.default_rng(2648500)


def P(a):
    return a.ctypes.data_as(C.c_void_p)


PER_QP = 8
qps = np.repeat(np.arange(52), PER_QP).astype(np.int32)
n = len(qps)
step = 2.0 ** (qps / 6.0)                                    # the quantiser step doubles every 6


def levels(count, top):
    """`count` levels per case: sparse, magnitudes up to about top / step (at least 1)"""
    mag = np.maximum(1, (top / step)[:, None] * rng.random((n, count))).astype(np.int64)
    lv = np.where(rng.random((n, count)) < 0.45, mag * rng.choice([-1, 1], (n, count)), 0)
    lv[np.arange(n), rng.integers(0, count, n)] |= 1         # never all zero
    return lv.astype(np.int16)


coef = levels(16, 300.0)
dst = rng.integers(0, 256, (n, 16)).astype(np.uint8)
deq, rec = coef.copy(), dst.copy()
for i in range(n):
    lib.refk_dequant_idct_add(P(deq[i]), int(qps[i]), 0, P(rec[i]), 4)
d16 = levels(16, 1500.0)
r16 = d16.copy()
for i in range(n):
    lib.refk_luma_dc(P(r16[i]), int(qps[i]))
d4 = levels(4, 3000.0)
r4 = d4.copy()
for i in range(n):
    lib.refk_chroma_dc(P(r4[i]), int(qps[i]))
np.savez_compressed(os.path.join(HERE, "kat_residual.npz"), qp=qps, di_coef=coef, di_dst=dst, di_deq=deq, di_rec=rec,
                    ldc_in=d16, ldc_out=r16, cdc_in=d4, cdc_out=r4)
print(n, "cases per family; largest levels", int(np.abs(coef).max()), int(np.abs(d16).max()), int(np.abs(d4).max()))
