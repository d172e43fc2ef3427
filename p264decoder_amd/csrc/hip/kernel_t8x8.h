// kernel_t8x8.h - the luma residual of inter macroblocks coded with the 8x8 transform (transform_size_8x8_flag, High profile).
//
// No counterpart in the reference (Baseline / Main tools only).  H.264 8.5.6 (inverse 8x8 scan), 8.5.9 / 8.5.13 (scaling with flat
// scaling lists, the 8x8 inverse transform) and the picture construction of 8.5.14 for the macroblocks whose record carries
// P264_MB_T8X8 (include/p264hip.h).  k_mc_sort files the luma of such a macroblock as "no residual", so k_mc / k_mc_second leave
// its plain prediction in the frame store; this kernel, launched behind them and in front of the intra stage, adds the residual of
// every coded 8x8 block in place.  Chroma of the macroblock went the usual way.
//
// Shape: one wavefront per TWO macroblocks, 8 lanes per 8x8 block, lane r of a block = its row r (levels 8r .. 8r+7 in scan
// order, then row r of the horizontal pass, column r of the vertical pass, row r of the samples).  The three changes of
// ownership go through LDS; nothing leaves the wavefront, so fences do (device_common.h: wave_lds_fence).  All arithmetic is
// 32-bit: a conforming stream keeps every value inside 16 bits, anything else still gives a defined result here.
//
// The 8x8 residual of every kernel is written here, once: t8_scale and t8_scatter (the weights from a T8Flat, or from a T8List
// where the picture has scaling lists), t8_idct1d, t8_row_pass; and what k_t8x8 and k_scaled_inter (kernel_scaling.h) have in
// common - T8Lane / t8_lane, a lane's macroblock, block and tile, and t8_walk, everything behind the scatter.  intra_luma4
// (kernel_intra.h) takes the scatter and the one-dimensional stage; its passes are its own, its lanes own other things.
#pragma once
#include "device_common.h"
#include "launch_shared.h"           // (T8_THREADS, T8_MBS_PER_WG)

#define T8_BLK_STRIDE 72             // dwords between the 8x8 tiles of a wavefront in LDS: 64 + 8, so that the eight blocks' column reads meet no bank twice

// 8x8 zig-zag frame scan (H.264 8.5.6): scan index -> x + 8 * y
__device__ __constant__ __attribute__((aligned(8))) const uint8_t c_scan8x8[64] = {
     0,  1,  8, 16,  9,  2,  3, 10, 17, 24, 32, 25, 18, 11,  4,  5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13,  6,  7, 14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63 };
// normAdjust8x8 (H.264 8.5.9, equation 8-316 ff.): v by qP % 6 for the six position classes, one byte per class
#define T8_V6(a, b, c, d, e, f) ((uint64_t)(a) | (uint64_t)(b) << 8 | (uint64_t)(c) << 16 | (uint64_t)(d) << 24 | (uint64_t)(e) << 32 | (uint64_t)(f) << 40)
__device__ __constant__ const uint64_t c_t8_v[6] = {
    T8_V6(20, 18, 32, 19, 25, 24), T8_V6(22, 19, 35, 21, 28, 26), T8_V6(26, 23, 42, 24, 33, 31),
    T8_V6(28, 25, 45, 26, 35, 33), T8_V6(32, 28, 51, 30, 40, 38), T8_V6(36, 32, 58, 34, 46, 43) };
// position class by (y & 3) * 4 + (x & 3): 0 3 4 3 / 3 1 5 1 / 4 5 2 5 / 3 1 5 1, one nibble each
#define T8_CLASSES 0x1513525415133430ull

// one level at raster position p of the block, scaled: LevelScale = w * normAdjust8x8, w the scaling list's weight at p (flat lists: 16)
__device__ __forceinline__ int t8_scale(int c, int p, uint64_t vrow, int per, int w)
{
    const int cls = (int)((T8_CLASSES >> (4 * (((p >> 3) & 3) * 4 + (p & 3)))) & 15u);
    const int t = c * (w * (int)((vrow >> (8 * cls)) & 255u));
    return per >= 6 ? (int)((unsigned)t << (per - 6)) : (t + (1 << (5 - per))) >> (6 - per);
}
// Where t8_scatter takes the weight at raster position p from.  A type, so that the flat instances hold the constant and no table:
// nothing at run time tells flat from scaled.
struct T8Flat { __device__ __forceinline__ int operator()(int) const { return 16; } };
struct T8List {                      // an 8x8 list of the workgroup's raster table in LDS (kernel_scaling.h: scaling_to_lds)
    const uint8_t *w;
    __device__ __forceinline__ int operator()(int p) const { return (int)w[p]; }
};

// Levels 8r .. 8r+7 of a block's scan (l: eight int16, as loaded), scaled, to their raster places in the block's tile of 64 ints.
// vrow, per: c_t8_v[qP % 6], qP / 6.  Every 8x8 residual starts here: k_t8x8, k_scaled_inter, intra_luma4 (kernel_intra.h).
template <class Weight>
__device__ __forceinline__ void t8_scatter(const uint4 l, int r, uint64_t vrow, int per, int *tile, const Weight weight)
{
    const uint2 sc = *(const uint2 *)(c_scan8x8 + r * 8);
    const uint32_t lw[4] = { l.x, l.y, l.z, l.w };
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int c = (i & 1) ? (int)lw[i >> 1] >> 16 : (int)(int16_t)(lw[i >> 1] & 0xffffu);
        const int p = (int)(((i < 4 ? sc.x : sc.y) >> (8 * (i & 3))) & 63u);
        tile[p] = t8_scale(c, p, vrow, per, weight(p));
    }
}

// the one-dimensional stage of 8.5.13, in place
__device__ __forceinline__ void t8_idct1d(int (&d)[8])
{
    const int a0 = d[0] + d[4], a4 = d[0] - d[4], a2 = (d[2] >> 1) - d[6], a6 = d[2] + (d[6] >> 1);
    const int a1 = -d[3] + d[5] - d[7] - (d[7] >> 1), a3 = d[1] + d[7] - d[3] - (d[3] >> 1);
    const int a5 = -d[1] + d[7] + d[5] + (d[5] >> 1), a7 = d[3] + d[5] + d[1] + (d[1] >> 1);
    const int b0 = a0 + a6, b2 = a4 + a2, b4 = a4 - a2, b6 = a0 - a6;
    const int b1 = a1 + (a7 >> 2), b3 = a3 + (a5 >> 2), b5 = (a3 >> 2) - a5, b7 = a7 - (a1 >> 2);
    d[0] = b0 + b7; d[1] = b2 + b5; d[2] = b4 + b3; d[3] = b6 + b1;
    d[4] = b6 - b1; d[5] = b4 - b3; d[6] = b2 - b5; d[7] = b0 - b7;
}

// The horizontal pass of a block's walk: rows first (the >> 1 and >> 2 of the stage make the order observable) - row r of the tile,
// back in place.  d: the lane's eight values, the column pass goes on in them.
__device__ __forceinline__ void t8_row_pass(int *tile, int r, int (&d)[8])
{
    const int4 lo = *(const int4 *)(tile + r * 8), hi = *(const int4 *)(tile + r * 8 + 4);
    d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w; d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
    t8_idct1d(d);
    *(int4 *)(tile + r * 8) = make_int4(d[0], d[1], d[2], d[3]);
    *(int4 *)(tile + r * 8 + 4) = make_int4(d[4], d[5], d[6], d[7]);
}

// A lane's place in the two inter kernels (the shape above), from its number alone.  tiles: the workgroup's
// (T8_THREADS / 64) * 8 * T8_BLK_STRIDE ints.
struct T8Lane {
    int mbi;                         // the macroblock of the wavefront's pair; behind the picture's last one rec is all zero
    int k, r;                        // 8x8 block of the macroblock (quadrants in raster order), row / column of the block
    uint4 rec;                       // the macroblock's record
    int *tile;                       // the block's tile
    __device__ __forceinline__ int mby(const Geom &g) const { return mbi / g.mb_w; }
    __device__ __forceinline__ int mbx(const Geom &g) const { return mbi - mby(g) * g.mb_w; }
    // row r of the block in the frame store
    __device__ __forceinline__ uint8_t *px(const PicDev *pd, const Geom &g) const { return pd->dst + mb_luma_off(g, mbx(g), mby(g)) + (uint32_t)(((k >> 1) * 8 + r) * 16 + (k & 1) * 8); }
};
__device__ __forceinline__ T8Lane t8_lane(const PicDev *pd, const Geom &g, int *tiles)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T8Lane t;
    t.mbi = ((int)blockIdx.x * (T8_THREADS / 64) + wave) * 2 + (lane >> 5);
    t.k = (lane >> 3) & 3; t.r = lane & 7;
    t.rec = make_uint4(0, 0, 0, 0);
    if (t.mbi < g.n_mb) t.rec = gload4(pd->mb + t.mbi);
    t.tile = tiles + (wave * 8 + (lane >> 3)) * T8_BLK_STRIDE;
    return t;
}

// The walk of the inter kernels behind t8_scatter, every lane of the wavefront in it (coded: the lane's block has levels in its tile)
__device__ __forceinline__ void t8_walk(const PicDev *pd, const Geom &g, const T8Lane &t, bool coded)
{
    int *tile = t.tile;
    const int r = t.r;
    wave_lds_fence();
    int d[8];
    if (coded) t8_row_pass(tile, r, d);
    wave_lds_fence();
    // ---- column r, rounded, back in place (a lane reads and writes its own column only)
    if (coded) {
#pragma unroll
        for (int y = 0; y < 8; y++) d[y] = tile[y * 8 + r];
        t8_idct1d(d);
#pragma unroll
        for (int y = 0; y < 8; y++) tile[y * 8 + r] = (d[y] + 32) >> 6;
    }
    wave_lds_fence();
    // ---- row r of the block: 8 samples of the prediction the inter launches left, plus the residual, clipped
    if (coded) {
        uint8_t *px = t.px(pd, g);
        const uint2 s = gload2(px);
        const int4 lo = *(const int4 *)(tile + r * 8), hi = *(const int4 *)(tile + r * 8 + 4);
        const int res[8] = { lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w };
        uint32_t o[2] = { 0, 0 };
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int v = clip255((int)(((i < 4 ? s.x : s.y) >> (8 * (i & 3))) & 255u) + res[i]);
            o[i >> 2] |= (uint32_t)v << (8 * (i & 3));
        }
        gstore2(px, make_uint2(o[0], o[1]));
    }
}

// grid: (macroblocks of a picture / T8_MBS_PER_WG, pictures of the batch)
__global__ __launch_bounds__(T8_THREADS)
void k_t8x8(const PicDev *__restrict__ pics, Geom g)
{
    __shared__ int tiles[(T8_THREADS / 64) * 8 * T8_BLK_STRIDE];
    const PicDev *pd = pics + blockIdx.y;
    if (pd->slice_type == P264_SLICE_I) return;            // (no inter record, and only those may carry the flag)
    const T8Lane t = t8_lane(pd, g, tiles);
    const bool coded = ((t.rec.x >> 24) & P264_MB_T8X8) && !P264_MB_IS_INTRA(t.rec.x & 255u) && ((t.rec.y >> (4 * t.k)) & 1u);
    if (!__ballot(coded)) return;                          // unflagged macroblocks leave at once
    if (coded) {
        const int qp = (int)((t.rec.x >> 8) & 63u), per = (qp * 43) >> 8;
        const int16_t *lv = pd->coefs + ((size_t)t.rec.z + coef_slot(t.rec.y, 4 * t.k)) * 16 + t.r * 8;     // four entries per coded block: 64 levels
        t8_scatter(gload4(lv), t.r, c_t8_v[qp - per * 6], per, t.tile, T8Flat());
    }
    t8_walk(pd, g, t, coded);
}
