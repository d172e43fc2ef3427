// kernel_scaling.h - scaling matrices (High profile): the scaling of H.264 8.5.9 - 8.5.13 with the picture's own lists, and
// k_scaled_inter, which adds the residual of the inter macroblocks of pictures with scaling_lists (include/p264hip.h).
//
// No counterpart in the reference, whose decoder forces flat lists (decoder/set.c:261-263).  LevelScale = weightScale * normAdjust
// (8.5.9); with weight 16 everywhere the functions below give what dequant_cols and chroma_dc_level give.  The levels of 8x8 blocks have
// no function of their own here: t8_scale / t8_scatter of kernel_t8x8.h take the weight from a T8List of this table.  All scaling is
// 32-bit: the packed 16-bit multiply of dequant_cols is exact only because flat products are multiples of 16.  A conforming stream
// keeps every value inside 16 bits; anything else still gives a defined result here (shifts on unsigned values, QP taken modulo 64).
//
// The table: 224 bytes per picture in its input slot, the eight resolved lists in SCAN order (4x4 lists 0 .. 5, then 8x8 lists 6, 7).
// A workgroup of every kernel that reads it works on one picture: it turns the table into RASTER order in LDS once
// (scaling_to_lds: 4x4 list n at 16 n, position y * 4 + x; 8x8 list 6 + n at 96 + 64 n, position y * 8 + x) and its lanes read
// the weights from there - same address across a macroblock's lanes, a broadcast.
//
// Who finds the table: a side array with one ScaleDev per picture of the batch, passed only to the launches that a batch with
// such a picture takes (k_mc_sort_scaled / k_mc_sort_scaled_p, k_scaled_inter, k_intra_scaled / k_intra_sparse_scaled); PicDev and
// the kernels of flat batches are what they were.  The batch's flat pictures get an all-16 table from the host: nothing in here
// branches on "flat".
//
// A picture whose Cr has a QP offset of its own (cr_qp_offset_delta != 0) takes the same road, with the all-16 table where it has no
// lists: the delta sits beside the table in its ScaleDev, and the lanes of plane 1 add it to the offset (plane_qpc below).  The same
// rule: PicDev and the kernels of flat batches do not know it.
#pragma once
#include "device_common.h"
#include "residual4x4.h"
#include "kernel_t8x8.h"

struct ScaleDev {
    const uint8_t *lists;          // P264HIP_SCALING_BYTES: the picture's table in its input slot, or the context's all-16 table
    int32_t scaled, cr_delta;      // scaled: the picture has scaling_lists or a Cr offset of its own: the sort files its residuals as absent,
                                   // k_scaled_inter adds them.  cr_delta: cr_qp_offset_delta (include/p264hip.h), what Cr's qPI adds to Cb's
};
static_assert(sizeof(ScaleDev) == 16, "ScaleDev: one per picture, indexed by every kernel that takes the array");

#define SCL_8X8_AT 96              // first 8x8 list in the table, in the slot and in LDS

// the table in raster order into the workgroup's LDS (every thread of the workgroup calls this; the caller's barrier follows)
__device__ __forceinline__ void scaling_to_lds(uint8_t *sw, const uint8_t *lists)
{
    for (int i = (int)threadIdx.x; i < P264HIP_SCALING_BYTES; i += (int)blockDim.x) {
        const uint8_t w = glob(lists)[i];
        if (i < SCL_8X8_AT) sw[(i & ~15) + zigzag_pos(i & 15)] = w;
        else sw[SCL_8X8_AT + ((i - SCL_8X8_AT) & 64) + c_scan8x8[(i - SCL_8X8_AT) & 63]] = w;
    }
}

// 8.5.12.1 on the column form of residual4x4.h (col[x][j] = rows 2j, 2j + 1 of column x): d = (c * LS) << (qP / 6 - 4) from qP 24,
// (c * LS + 2^(3 - qP / 6)) >> (4 - qP / 6) below, LS = weight * normAdjust4x4.  wr: the list's sixteen weights in raster order,
// row y in word y.  Position (0, 0) is scaled like the others; callers whose DC is scaled apart overwrite it.
__device__ __forceinline__ void scale_cols_w(uint32_t (&col)[4][2], int qp, const uint4 wr)
{
    qp &= 63;
    const int per = (qp * 43) >> 8, rem = qp - per * 6;
    const int s[3] = { (int)dq_s(0, rem), (int)dq_s(1, rem), (int)dq_s(2, rem) };     // both even, mixed, both odd
    const uint32_t w[4] = { wr.x, wr.y, wr.z, wr.w };
#pragma unroll
    for (int x = 0; x < 4; x++)
#pragma unroll
        for (int j = 0; j < 2; j++) {
            int v[2];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int y = 2 * j + h;
                const int c = h ? (int)col[x][j] >> 16 : (int)(int16_t)(col[x][j] & 0xffffu);
                const int t = c * ((int)((w[y] >> (8 * x)) & 255u) * s[(x & 1) + (y & 1)]);
                v[h] = per >= 4 ? (int)((unsigned)t << (per - 4)) : (t + (1 << (3 - per))) >> (4 - per);
            }
            col[x][j] = ((uint32_t)v[0] & 0xffffu) | (uint32_t)v[1] << 16;
        }
}
// 8.5.11: the DC level of one of the four blocks of a chroma plane, ((f * LS(QP'c % 6, 0, 0)) << (QP'c / 6)) >> 5 with the plane's own
// list (w00: its weight at position 0); chroma_dc_level of residual4x4.h with that weight in place of 16
__device__ __forceinline__ int chroma_dc_level_w(uint2 dcl, bool right, bool lower, int qpc, int w00)
{
    const int d0 = (int)(int16_t)(dcl.x & 0xffff), d1 = (int)dcl.x >> 16, d2 = (int)(int16_t)(dcl.y & 0xffff), d3 = (int)dcl.y >> 16;
    const int t0 = d0 + d1, t1 = d0 - d1, t2 = d2 + d3, t3 = d2 - d3;
    int f = pick_addsub(t0, t1, t2, t3, right, lower);
    f = (int)(int16_t)f;
    qpc &= 63;
    const int per = (qpc * 43) >> 8, rem = qpc - per * 6;
    return (int)((unsigned)(f * (w00 * (int)dq_s(0, rem))) << per) >> 5;
}
// QPc of a lane's chroma plane (8.5.8 with the plane's own offset): Cb's qPI is Clip3(0, 51, QPY + offset), Cr's
// Clip3(0, 51, QPY + offset + cr_delta) - cr_offset_of (device_common.h) keeps the sum of any two ints defined
__device__ __forceinline__ int plane_qpc(int qp, int offset, int cr_delta, bool cr) { return chroma_qp(clip3i(qp + (cr ? cr_offset_of(offset, cr_delta) : offset), 0, 51)); }
__device__ __forceinline__ int cr_delta_of(const ScaleDev *scale, int pic) { return scale[pic].cr_delta; }     // (declared in kernel_deblock.h, which does not know the struct)
// 8.5.13, the levels of an 8x8 block: t8_scatter of kernel_t8x8.h with a T8List of the table's list 6 (intra) or 7 (inter)
__device__ __forceinline__ T8List scaling_list8(const uint8_t *sw, int n) { return T8List{ sw + SCL_8X8_AT + 64 * (n - 6) }; }

// ------------------------------------------------------------------------------------------
// k_scaled_inter: the residual of the inter macroblocks of scaled pictures, added in place.  The batch's sort files luma and
// chroma of such a picture's inter macroblocks as "no residual" (as every sort files the luma of P264_MB_T8X8 records), so the
// inter launches leave the clipped prediction in the frame store; this kernel, launched behind them and in front of the intra
// stage - where k_t8x8 runs in other batches - adds
//   the coded 4x4 luma blocks (list 3), chroma DC and AC of both planes (lists 4, 5): lane = block, everything in its registers
//   (unscan_cols, scale_cols_w, idct_add on the block's four rows of samples);
//   the coded 8x8 blocks of P264_MB_T8X8 records (list 7): k_t8x8's lane plan, scatter and walk (kernel_t8x8.h: t8_lane, t8_scatter,
//   t8_walk), eight lanes per block, the weights from the table.
// It owns the 8x8 blocks of the batch's FLAT pictures too (k_t8x8 is not launched beside it): they take the all-16 table, and
// nothing else of a flat picture is touched - its 4x4 and chroma residuals went through k_mc as ever.
//
// Shape: as k_t8x8, one wavefront per two macroblocks, 32 lanes each: lanes 0 .. 15 the luma 4x4 blocks in decoding order, 16 .. 23
// the chroma blocks (plane, block), then all 32 the four 8x8 blocks.  Bound by memory: it re-reads and re-writes the samples of every
// block that has a residual.
// ------------------------------------------------------------------------------------------
// grid: (macroblocks of a picture / T8_MBS_PER_WG, pictures of the batch)
__global__ __launch_bounds__(T8_THREADS)
void k_scaled_inter(const PicDev *__restrict__ pics, const ScaleDev *__restrict__ scale, Geom g)
{
    __shared__ int tiles[(T8_THREADS / 64) * 8 * T8_BLK_STRIDE];
    __shared__ __attribute__((aligned(16))) uint8_t sw[P264HIP_SCALING_BYTES];
    const PicDev *pd = pics + blockIdx.y;
    if (pd->slice_type == P264_SLICE_I) return;            // (no inter record)
    const ScaleDev *sd = scale + blockIdx.y;
    const bool scaled = sd->scaled != 0;                   // (per workgroup)
    scaling_to_lds(sw, sd->lists);
    __syncthreads();
    const T8Lane t = t8_lane(pd, g, tiles);
    const int h = threadIdx.x & 31, mbx = t.mbx(g), mby = t.mby(g);
    const uint4 rec = t.rec;
    const bool inter = t.mbi < g.n_mb && !P264_MB_IS_INTRA(rec.x & 255u);
    const unsigned mask = inter ? rec.y : 0u;
    const bool t8 = ((rec.x >> 24) & P264_MB_T8X8) != 0;
    const int qp = (int)((rec.x >> 8) & 63u);
    const int16_t *cf = pd->coefs + (size_t)rec.z * 16;
    // ---- 4x4 blocks: lane h < 16 the luma block h (decoding order), 16 .. 23 chroma block (h - 16) & 3 of plane (h - 16) >> 2 ----
    {
        const bool chroma = h >= 16;
        const int p = (h >> 2) & 1, j = h & 3;             // (chroma lanes: plane, block of the plane's 2 x 2)
        const bool coded = h < 24 && ((mask >> h) & 1u) && !(t8 && !chroma);
        const bool has_dc = chroma && h < 24 && (mask & P264_COEF_CHROMA_DC);
        if (scaled && (coded || has_dc)) {
            uint4 la = make_uint4(0, 0, 0, 0), lb = la; uint2 dcl = make_uint2(0, 0);
            if (coded) { const int16_t *c = cf + coef_slot(mask, h) * 16; la = gload4(c); lb = gload4(c + 8); }
            if (has_dc) dcl = gload2(cf + ((mask >> 24) & 1) * 16 + p * 4);
            uint8_t *px = chroma ? pd->dst + mb_chroma_off(g, mbx, mby) + (uint32_t)((j >> 1) * 64 + p * 8 + (j & 1) * 4)
                                 : pd->dst + mb_luma_off(g, mbx, mby) + (uint32_t)(blk_y(h) * 64 + blk_x(h) * 4);
            uint32_t s[4] = { gload1(px), gload1(px + 16), gload1(px + 32), gload1(px + 48) };
            const int list = chroma ? 4 + p : 3;
            const uint4 wr = *(const uint4 *)(sw + list * 16);
            const uint32_t lv[8] = { la.x, la.y, la.z, la.w, lb.x, lb.y, lb.z, lb.w };
            uint32_t col[4][2];
            if (chroma) {
                const int qpc = plane_qpc(qp, pd->chroma_qp_offset, sd->cr_delta, p != 0);
                unscan_cols<true>(lv, col);
                scale_cols_w(col, qpc, wr);
                const int dc = chroma_dc_level_w(dcl, j & 1, j & 2, qpc, (int)(wr.x & 255u));
                col[0][0] = (col[0][0] & 0xffff0000u) | ((uint32_t)dc & 0xffffu);
            } else {
                unscan_cols<false>(lv, col);
                scale_cols_w(col, qp, wr);
            }
            idct_add(col, s);
            gstore1(px, s[0]); gstore1(px + 16, s[1]); gstore1(px + 32, s[2]); gstore1(px + 48, s[3]);
        }
    }
    // ---- 8x8 blocks of P264_MB_T8X8 records (kernel_t8x8.h's walk): 8 lanes per block, lane r = its row, then its column ----
    const bool coded8 = inter && t8 && ((mask >> (4 * t.k)) & 1u);
    if (!__ballot(coded8)) return;
    if (coded8) {
        const int per = (qp * 43) >> 8;
        t8_scatter(gload4(cf + coef_slot(mask, 4 * t.k) * 16 + t.r * 8), t.r, c_t8_v[qp - per * 6], per, t.tile, scaling_list8(sw, 7));
    }
    t8_walk(pd, g, t, coded8);
}
