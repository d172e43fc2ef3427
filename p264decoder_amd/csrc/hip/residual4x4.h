// residual4x4.h - the residual of one 4x4 block, entirely in a lane's registers: unscan, dequantisation and the inverse transform
// on the block in COLUMNS, two int16 per word (the inter roles of kernel_mc.h and the intra kernels share it), and the chroma DC
// level of a block.
//
// Arithmetic to preserve: core/quant.c:66-99,138-159, core/dct.c:55-68,205-247 with their int16 stores (A-Q8).
#pragma once
#include "device_common.h"
#include "lane_ops.h"

// half `ha` of word pa into the low half, half `hb` of word pb into the high half
template <int HA, int HB> __device__ __forceinline__ uint32_t pick2(uint32_t pa, uint32_t pb)
{
    return perm(pb, pa, (uint32_t)(2 * HA) | (uint32_t)(2 * HA + 1) << 8 | (uint32_t)(4 + 2 * HB) << 16 | (uint32_t)(5 + 2 * HB) << 24);
}
// Levels in scan order, two per word (lv[j] = levels 2j, 2j+1) -> the block in COLUMNS: col[x][0] = (d[0][x], d[1][x]),
// col[x][1] = (d[2][x], d[3][x]) (zig-zag, decoder/macroblock.c:602-603).  AC: the 15 levels sit at scan positions 1..15
// (level k-1 at position k); position 0 is filled by the caller.
template <bool AC> __device__ __forceinline__ void unscan_cols(const uint32_t (&lv)[8], uint32_t (&col)[4][2])
{
    // scan index of raster position (y,x): 0 1 5 6 / 2 4 7 12 / 3 8 11 13 / 9 10 14 15
    if (!AC) {
        col[0][0] = pick2<0, 0>(lv[0], lv[1]);  col[0][1] = pick2<1, 1>(lv[1], lv[4]);      // s0 s2 | s3 s9
        col[1][0] = pick2<1, 0>(lv[0], lv[2]);  col[1][1] = pick2<0, 0>(lv[4], lv[5]);      // s1 s4 | s8 s10
        col[2][0] = pick2<1, 1>(lv[2], lv[3]);  col[2][1] = pick2<1, 0>(lv[5], lv[7]);      // s5 s7 | s11 s14
        col[3][0] = pick2<0, 0>(lv[3], lv[6]);  col[3][1] = pick2<1, 1>(lv[6], lv[7]);      // s6 s12 | s13 s15
    } else {   // level index = scan index - 1
        col[0][0] = lv[0] & 0xffff0000u;        col[0][1] = pick2<0, 0>(lv[1], lv[4]);      // -  l1 | l2 l8
        col[1][0] = pick2<0, 1>(lv[0], lv[1]);  col[1][1] = pick2<1, 1>(lv[3], lv[4]);      // l0 l3 | l7 l9
        col[2][0] = pick2<0, 0>(lv[2], lv[3]);  col[2][1] = pick2<0, 1>(lv[5], lv[6]);      // l4 l6 | l10 l13
        col[3][0] = pick2<1, 1>(lv[2], lv[5]);  col[3][1] = pick2<0, 0>(lv[6], lv[7]);      // l5 l11 | l12 l14
    }
}
// dequant_4x4 (core/quant.c:66-99) on the column form.  For every QP the reference's value is level * (scale << qp/6)
// truncated to int16: below QP 24 its rounding shift divides a multiple of 16 exactly (16 * scale * level >> n, n <= 4).
__device__ __forceinline__ void dequant_cols(uint32_t (&col)[4][2], int qp)
{
    const int per = (qp * 43) >> 8, rem = qp - per * 6;
    const uint32_t m0 = dq_s(0, rem) << per, m1 = dq_s(1, rem) << per, m2 = dq_s(2, rem) << per;
    const u16x2 even = __builtin_bit_cast(u16x2, m0 | (m1 << 16)), odd = __builtin_bit_cast(u16x2, m1 | (m2 << 16));
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int j = 0; j < 2; j++)
            col[x][j] = __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, col[x][j]) * ((x & 1) ? odd : even)));
}
// add4x4_idct (core/dct.c:205-247): first pass along the rows in packed 16-bit (int16 stores, as the reference's tmp),
// second pass along the columns in 32-bit ((sum + 32) >> 6 is taken before the int16 store), added to the prediction.
// (the first pass: T[x][j] = the pairs of row sums)
__device__ __forceinline__ void idct_rows(const uint32_t (&col)[4][2], s16x2 (&T)[4][2])
{
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const s16x2 c0 = as_s16x2(col[0][j]), c1 = as_s16x2(col[1][j]), c2 = as_s16x2(col[2][j]), c3 = as_s16x2(col[3][j]);
        const s16x2 s02 = c0 + c2, d02 = c0 - c2, s13 = c1 + (c3 >> 1), d13 = (c1 >> 1) - c3;
        T[0][j] = s02 + s13; T[1][j] = d02 + d13; T[2][j] = d02 - d13; T[3][j] = s02 - s13;
    }
}
__device__ __forceinline__ void idct_add(const uint32_t (&col)[4][2], uint32_t (&px)[4])
{
    s16x2 T[4][2];
    idct_rows(col, T);
    // (sum + 32) >> 6 added to the prediction and clipped = (sum + 32 + 64 * prediction) >> 6 clipped: shift, saturation
    // and packing in one instruction per two samples
    int res[4][4];
#pragma unroll
    for (int x = 0; x < 4; x++) {
        const int a0 = T[x][0].x, a1 = T[x][0].y, a2 = T[x][1].x, a3 = T[x][1].y;
        const int s02 = a0 + a2 + 32, d02 = a0 - a2 + 32, s13 = a1 + (a3 >> 1), d13 = (a1 >> 1) - a3;
        res[0][x] = s02 + s13; res[1][x] = d02 + d13; res[2][x] = d02 - d13; res[3][x] = s02 - s13;
    }
#pragma unroll
    for (int y = 0; y < 4; y++) {
        const uint32_t p = px[y];
        const int v[4] = { res[y][0] + (int)((p & 255u) << 6), res[y][1] + (int)(((p >> 8) & 255u) << 6),
                           res[y][2] + (int)(((p >> 16) & 255u) << 6), res[y][3] + (int)((p >> 24) << 6) };
        px[y] = round_pack4<6>(v);
    }
}
// The DC level of one of the four blocks of a chroma plane (`right`, `lower`: its place in the plane's 2x2) from the plane's four
// DC levels dcl: idct2x2dc (core/dct.c:55-68, int16 stores), then p264_mb_dequant_2x2_dc (core/quant.c:138-159): for every QP
// its value is (f * (scale << qp/6)) >> 1 - exact for the shifts left, the truncating shift below QP 6.  Goes into position 0
// of the block's AC levels (unscan_cols<true>).  (The two flags come from the caller as flags: taken from the block number in
// here, the role bodies of k_mc, k_mc_wp and k_mc_second compile to other code.)
__device__ __forceinline__ int chroma_dc_level(uint2 dcl, bool right, bool lower, int qpc)
{
    const int d0 = (int)(int16_t)(dcl.x & 0xffff), d1 = (int)dcl.x >> 16, d2 = (int)(int16_t)(dcl.y & 0xffff), d3 = (int)dcl.y >> 16;
    const int t0 = d0 + d1, t1 = d0 - d1, t2 = d2 + d3, t3 = d2 - d3;
    int f = pick_addsub(t0, t1, t2, t3, right, lower);                        // {t0+t2, t1+t3, t0-t2, t1-t3}[2 * lower + right]
    f = (int)(int16_t)f;
    const int per = (qpc * 43) >> 8, rem = qpc - per * 6;
    return (f * (int)(dq_s(0, rem) << per)) >> 1;
}
