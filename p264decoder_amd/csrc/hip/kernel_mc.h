// kernel_mc.h - K1: inter prediction + residual for every non-intra macroblock of a batch.
//
// Replaces p264_mb_mc / p264_mb_mc_0xywh (core/macroblock.c:506-524,633-676), mc_luma / pixel_avg / mc_copy
// (core/mc.c:58-74,160-171,237-266), the half-pel plane generator p264_frame_filter (core/mc.c:172-235,409-451 -
// computed on the fly here, never stored), motion_compensation_chroma (core/mc.c:303-334), p264_macroblock_decode_skip
// (decoder/macroblock.c:895-934), the border expansion (core/frame.c:183-222 - clamped coordinates instead, SURVEY A-Q9)
// and the inter half of p264_macroblock_decode (decoder/macroblock.c:832-890: unscan, dequant_4x4, add4x4_idct, chroma DC).
//
// The first version of this stage (one wavefront per macroblock, everything about the macroblock in SGPRs) was bound by
// scalar and vector instruction issue.  This version is built on three ideas:
//
//  1. ONE LANE = ONE 4x4 BLOCK.  The lane interpolates its 16 samples from a 9x9 (or smaller) window held in registers,
//     runs the whole inverse transform of its block in registers and stores two rows of 8 samples (after swapping halves
//     with its neighbour lane).  Every partition shape down to 4x4 is the same code: a lane only ever looks at its own
//     vector.  All per-macroblock header work is vector work shared by 64 blocks.
//  2. WORK LISTS SORTED BY WHAT THE CODE HAS TO DO.  The quarter-pel phase decides the arithmetic (copy / horizontal /
//     vertical / both / centre ...), so k_mc_sort (one workgroup per picture, a counting sort in LDS) hands the work over
//     grouped by {phase class, window inside the picture or not, residual present or not} (and by band of macroblock
//     rows, for cache locality).  A wavefront takes one chunk of ONE key: the class is a scalar, the switch on it is free,
//     nobody executes code it does not need - a P_SKIP macroblock at an integer position costs a few loads and stores,
//     windows inside the picture need no clamping, wavefronts without coded blocks skip the transform.  Sorting on the
//     device keeps the host parser and the CPU->GPU seam unchanged.
//  3. WINDOWS SHARED THROUGH LDS, AT THE LARGEST GRANULARITY THAT HAS ONE VECTOR.  A lane fetching its own window from
//     memory costs one L1 tag look-up per lane and dword (measured: ~50 look-ups per load instruction, 27 loads per
//     wavefront - the L1's look-up rate was the bound).  So the lanes of a work item stage the item's window in LDS with
//     16-byte loads of consecutive rows of a strip (64 contiguous bytes per four lanes) and read their own 9x9 windows out
//     of that image: one address register, rows and columns as immediates.  Work items are whole macroblocks where the
//     macroblock has one vector (16 lanes, a 21-row window: P_SKIP, 16x16 - most of a typical stream) and 8x8 quadrants
//     otherwise (4 lanes, a 13-row window); quadrants whose 4x4 blocks differ (sub-8x8 partitions) fetch per lane with
//     clamped coordinates.
//
// Chroma (4x4 per quadrant and plane, bilinear) has no phase classes; it has its own roles and lists (macroblock items
// of 8 lanes; quadrant items of 2 lanes, the four of a macroblock consecutive), keys {inside / clamped, residual or not}.
//
// One launch (k_mc) runs the four kinds of work - luma / chroma x macroblock / quadrant items - as roles of the workgroups a
// picture gets (see k_mc below); B pictures take a second launch (k_mc_second) for the list-1 half of the blocks that
// predict from both lists (mc_classify).
//
// This file: the windows, their staging and the interpolation, the role bodies and the three kernels.  The work lists (keys,
// layout, entry format, classification, k_mc_sort*) are kernel_mc_sort.h, the residual of a 4x4 block residual4x4.h, buffer and
// lane plumbing lane_ops.h.
//
// Arithmetic to preserve: core/mc.c:172-266 (half-pel planes, quarter-pel averages), :303-334 (chroma),
// core/quant.c:66-99,138-159, core/dct.c:55-68,205-247 with their int16 stores (A-Q8).
#pragma once
#include "device_common.h"
#include "lane_ops.h"
#include "residual4x4.h"
#include "kernel_mc_sort.h"
#include <type_traits>


// ------------------------------------------------------------------------------------------
// reference windows in registers
// ------------------------------------------------------------------------------------------
// d[r][k] = the aligned dword k of window row r.  The window starts at sample (xw, yw); xa = xw & ~3 is the first dword.
// Rows R0 .. R0+NR-1 and NC dword columns are fetched.  Two sources:
// LWin - out of the work item's image in LDS (see the file header): one address register, rows and columns as immediates.
// GWin - straight from memory with clamped coordinates; only for quadrants whose 4x4 blocks have different vectors
//        (sub-8x8 partitions), where there is no common window.
//
// Luma work items: MB = a whole macroblock (16 lanes, window 21 rows x up to 3 strips) or an 8x8 quadrant (4 lanes, 13 rows x 2
// strips).  The image holds only the dword columns the item reads, ROTATED so that column 0 is the dword of the first
// sample the class needs (x0 = xs & ~3): a lane's reads are at column (its block column + k) whatever the vector, and pitch
// and item placement are chosen so that every read instruction of a wavefront is free of bank conflicts BY CONSTRUCTION.  For
// ds_read_b32 / ds_read2_b32 and every ds_write the LDS of gfx950 has 32 banks of 4 bytes and serves a wavefront as two groups
// of 32 lanes (MI355X_MICROARCH.md, LDS): the 32 lanes of a group must land on 32 different banks.
//   macroblock items: dword = item * 208 + (4 by + r) * 9 + bx + k   ->  bank = 16 item + 4 by + bx + const (two items per group);
//   quadrant items:   dword = (item / 2) * 264 + (item % 2) * 130 + (4 ly + r) * 9 + lx + k
//                                                                    ->  bank = 8 (item / 2) + 2 (item % 2) + 4 ly + lx + const
//                     (eight items per group).  Rounds 3 - 5 had a pitch of 8 dwords and 130 dwords per item, laid out for 64
//                     banks across all 64 lanes: 32 ly fell away modulo 32 and the two block rows of every item met on the
//                     same banks in every read - 150 M of the kernel's 271 M bank-conflict cycles per launch (scratch/r5_ldsconf.sh).
// (With the strips stored side by side at a pitch of 52 / 36 bytes, the lanes of different items met on the same banks at
// random: LDS bank-conflict cycles were twice the LDS issue cycles of these kernels.)  The staging stores of a 16-byte row
// piece go to columns 4 s - dx .. 4 s - dx + 3; columns outside 0 .. 5 (0 .. 3) fall into the row's padding or the padding of
// the row above - nobody reads them.  LEAD bytes in front of the first item take the negative columns of its first row.
template <bool MB> struct YItem {
    static constexpr int LANES = MB ? 16 : 4, PER_WAVE = 64 / LANES, STRIPS = MB ? 3 : 2, ROWS = MB ? 21 : 13;
    static constexpr int PITCH = 36, BYTES = MB ? 832 : 520, LEAD = 16;
    static constexpr int PAIR = 1056;                       // quadrant items: bytes per pair of items (264 dwords)
    static constexpr int WAVE_BYTES = MB ? PER_WAVE * BYTES : (PER_WAVE / 2) * PAIR;
    static_assert(ROWS * PITCH + 12 <= BYTES && (MB || BYTES + ROWS * PITCH + 12 <= PAIR), "item image");
    // first byte of item i (counted over the workgroup's wavefronts) behind LEAD
    __device__ static __forceinline__ int item_off(int i) { return MB ? i * BYTES : (i >> 1) * PAIR + (i & 1) * BYTES; }
};

// Stage rows R0S .. R0S+NRS-1 of the window whose first needed sample is (xs, wy); li = lane inside the item.  Piece p = strip
// p / NRS, row p % NRS: consecutive lanes fetch consecutive rows of one strip (64 contiguous bytes per four lanes).  A
// macroblock window reaches into its third strip only when it starts in the last dword of a strip: `third` says so.
// CLAMP: coordinates clamped to the picture = the reference's replicated borders (core/frame.c:183-222, A-Q9): a strip
// that lies outside the picture becomes the replicated first (last) sample of the row.
// Every piece is requested by the SAME straight-line sequence of loads, all in flight together, one wait: a piece a lane does
// not need (the third strip of an item that does not reach into it) is requested at an offset beyond the buffer, which the
// bounds check of the descriptor answers with zeros without going to memory.  (Written as `if (needed) load`, the compiler
// wrapped every such load into a branch of its own with a wait for the data inside it: up to three memory round trips one
// after the other per chunk instead of one.)  NS = strips the class can reach into (2: copy / vertical, which read no columns
// left of the blocks).
#define MC_OOB 0xffffff00u             // raw buffer offset beyond any frame store (< 4 GiB, p264hip_create): reads return 0
template <bool MB, int R0S, int NRS, bool CLAMP, int NS>
__device__ __forceinline__ void stage_luma(uint8_t *img, rsrc_t rs, uint32_t roff, const Geom &g, int xs, int wy, int li, bool third)
{
    typedef YItem<MB> I;
    static_assert(NS == 2 || (MB && NS == 3), "strips");
    constexpr int NP = NS * NRS, NJ = (NP + I::LANES - 1) / I::LANES;
    const int sA = xs >> 4, dx4 = xs & 12;                  // first strip, byte offset of the first needed dword inside it
    u32x4 v[NJ];
    int dst[NJ];
    bool on[NJ];
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        const int p = min(li + I::LANES * j, NP - 1), s = p >= 2 * NRS ? 2 : p >= NRS ? 1 : 0, row = R0S + p - s * NRS;
        dst[j] = row * I::PITCH + s * 16 - dx4;
        on[j] = NS == 2 || s < 2 || third;
        if (!CLAMP) {
            const uint32_t off = roff + strip_mul(sA + s, g.ystrip) + (uint32_t)((wy + row) * 16);
            v[j] = wload4(rs, on[j] ? off : MC_OOB);
        } else {
            const int st = sA + s, sc = clip3i(st, 0, g.mb_w - 1);
            const uint32_t off = roff + strip_mul(sc, g.ystrip) + (uint32_t)(clip3i(wy + row, 0, g.h - 1) * 16);
            v[j] = wload4(rs, on[j] ? off : MC_OOB);
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) loads_land(v[j]);
    if (CLAMP) {
#pragma unroll
        for (int j = 0; j < NJ; j++) {
            const int p = min(li + I::LANES * j, NP - 1), s = p >= 2 * NRS ? 2 : p >= NRS ? 1 : 0, st = sA + s;
            u32x4 t = v[j];
            if (st < 0) { const uint32_t e = perm(t.x, t.x, 0x00000000u); t.x = t.y = t.z = t.w = e; }
            if (st >= g.mb_w) { const uint32_t e = perm(t.w, t.w, 0x03030303u); t.x = t.y = t.z = t.w = e; }
            v[j] = t;
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; j++) {
        if (on[j]) {
            uint32_t *o = (uint32_t *)(img + dst[j]);       // (4-byte aligned: pairs of dwords)
            o[0] = v[j].x; o[1] = v[j].y; o[2] = v[j].z; o[3] = v[j].w;
        }
    }
}
template <int PITCH> struct LWin {
    // (Round 5 tried dword reads at the window's own byte address - gfx950's LDS takes unaligned reads - to drop the v_alignbyte per
    // window dword: 6 % fewer vector instructions in the luma roles, and the MC stage went from 4.95 to 5.54 ms per 2048 pictures:
    // the compiler merges them into unaligned ds_read_b64 / b96 and the LDS pipe serves those far below its aligned rate.)
    const uint8_t *img; int x0, y0;                        // the image's sample (0,0) is (x0, y0) of the reference
    template <int R0, int NR, int NC> __device__ __forceinline__ void load(uint32_t (&d)[9][3], int xw, int yw) const
    {
        const uint8_t *b = img + __mul24(yw - y0, PITCH) + ((xw & ~3) - x0);
#pragma unroll
        for (int r = R0; r < R0 + NR; r++)
#pragma unroll
            for (int k = 0; k < NC; k++) d[r][k] = *(const uint32_t *)(b + r * PITCH + 4 * k);
    }
};
struct GWin {
    rsrc_t rs; uint32_t roff; const Geom &g;
    template <int R0, int NR, int NC> __device__ __forceinline__ void load(uint32_t (&d)[9][3], int xw, int yw) const
    {
        const int xa = xw & ~3;
        uint32_t col[NC], sel[NC];
#pragma unroll
        for (int k = 0; k < NC; k++) {
            const int x = xa + 4 * k, xc = clip3i(x, 0, g.w - 4);
            col[k] = roff + strip_mul(xc >> 4, g.ystrip) + (uint32_t)(xc & 15);
            sel[k] = x < 0 ? 0x00000000u : x >= g.w ? 0x03030303u : 0x03020100u;
        }
#pragma unroll
        for (int r = R0; r < R0 + NR; r++) {
            const uint32_t ro = (uint32_t)clip3i(yw + r, 0, g.h - 1) * 16u;
#pragma unroll
            for (int k = 0; k < NC; k++) { const uint32_t v = bload(rs, col[k] + ro); d[r][k] = perm(v, v, sel[k]); }
        }
    }
};

// horizontal 6-tap sums (core/mc.c:53-56) for 4 adjacent samples; n0..n2 hold window bytes 0..11, output sample i uses
// bytes i..i+5.  Samples are taken as (s - 128) in int8: the taps sum to 32, so the true sum is the dot product + 4096;
// `bias` = 4096 + rounding term.
__device__ __forceinline__ void tap_h4(uint32_t n0, uint32_t n1, uint32_t n2, int bias, int t[4])
{
    // Sample i needs bytes i..i+5.  Instead of shifting the window to each sample (two v_alignbyte per sample) the TAPS are
    // shifted: every sample is a sum of dot products of the same aligned dwords with its own constant vectors.
    n0 ^= 0x80808080u; n1 ^= 0x80808080u; n2 ^= 0x80808080u;
    t[0] = __builtin_amdgcn_sdot4((int)n0, 0x1414fb01, __builtin_amdgcn_sdot4((int)n1, 0x000001fb, bias, false), false);   // (1,-5,20,20 | -5,1,0,0)
    t[1] = __builtin_amdgcn_sdot4((int)n0, 0x14fb0100, __builtin_amdgcn_sdot4((int)n1, 0x0001fb14, bias, false), false);   // (0,1,-5,20 | 20,-5,1,0)
    t[2] = __builtin_amdgcn_sdot4((int)n0, (int)0xfb010000u, __builtin_amdgcn_sdot4((int)n1, 0x01fb1414, bias, false), false);   // (0,0,1,-5 | 20,20,-5,1)
    t[3] = __builtin_amdgcn_sdot4((int)n0, 0x01000000, __builtin_amdgcn_sdot4((int)n1, (int)0xfb1414fbu, __builtin_amdgcn_sdot4((int)n2, 0x00000001, bias, false), false), false);   // (0,0,0,1 | -5,20,20,-5 | 1,0,0,0)
}
// window bytes 0..11 of a row, the window starting at byte s of dword 0
__device__ __forceinline__ void align_row(const uint32_t (&w)[3], uint32_t s, uint32_t &n0, uint32_t &n1, uint32_t &n2)
{
    n0 = alignbyte(w[1], w[0], s); n1 = alignbyte(w[2], w[1], s); n2 = w[2] >> (8 * s);
}
// vertical 6-tap of four columns over six rows of samples (mc_hv, core/mc.c:186-199), packed 16-bit
__device__ __forceinline__ uint32_t tap_v4(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3, uint32_t r4, uint32_t r5)
{
    // The pair sums of samples are 32-bit adds of two non-negative 16-bit halves (nothing carries across; v_add_u32 issues in 2.4
    // cycles per wavefront on gfx950, the packed add in 4.3 - scratch/r4_rates/), the rounding term rides on the first of them;
    // the taps are two packed multiply-adds.
    const uint32_t M = 0x00ff00ffu;
    const s16x2 c20 = { 20, 20 }, cm5 = { -5, -5 };
    const uint32_t a05 = (r0 & M) + (r5 & M) + 0x00100010u, a23 = (r2 & M) + (r3 & M), a14 = (r1 & M) + (r4 & M);
    const uint32_t b05 = ((r0 >> 8) & M) + ((r5 >> 8) & M) + 0x00100010u, b23 = ((r2 >> 8) & M) + ((r3 >> 8) & M), b14 = ((r1 >> 8) & M) + ((r4 >> 8) & M);
    s16x2 a = cm5 * as_s16x2(a14) + (c20 * as_s16x2(a23) + as_s16x2(a05));
    s16x2 b = cm5 * as_s16x2(b14) + (c20 * as_s16x2(b23) + as_s16x2(b05));
    // (v >> 5) clipped to a byte: v_sat_pk_u8_i16 saturates both halves of a pair into bytes 0 and 1 (two instructions per pair
    // instead of shift, max, min; one v_perm interleaves the even and the odd samples)
    a = a >> 5; b = b >> 5;
    return perm(sat_pk_u8_i16(as_u32(b)), sat_pk_u8_i16(as_u32(a)), 0x05010400u);
}

// ------------------------------------------------------------------------------------------
// bi-prediction (B pictures): the two ways the reference combines two predictions, four samples at a
// time; used by the two-list class of the luma and chroma quadrant kernels.  pixel_avg_wxh (core/mc.c:76-88) is the byte-parallel rounding average above; the implicit-weight
// form pixel_avg_weight_wxh (core/mc.c:106-132): clip((a * w1 + b * (64 - w1) + 32) >> 6), weights from -64 to 128.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t bipred_avg4(uint32_t a, uint32_t b) { return avg4(a, b); }
__device__ __forceinline__ uint32_t bipred_weight4(uint32_t a, uint32_t b, int w1)
{
    const int w2 = 64 - w1;
    int v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = (int)((a >> (8 * i)) & 255u) * w1 + (int)((b >> (8 * i)) & 255u) * w2 + 32;
    return round_pack4<6>(v);
}
// explicit weighted sample prediction (H.264 8.4.2.3.2), four samples at a time; wo = weight | offset << 16 (int16 each, one
// entry of PicDev::wp), d = logWD.  One list: Clip1(((p * w + 2^(d-1)) >> d) + o), d = 0: Clip1(p * w + o); both lists:
// Clip1(((p0 * w0 + p1 * w1 + 2^d) >> (d + 1)) + ((o0 + o1 + 1) >> 1)).  32-bit products (p0 * w0 + p1 * w1 needs 17 bits).
__device__ __forceinline__ uint32_t wp_combine4(uint32_t a, uint32_t b, uint32_t wa, uint32_t wb, int d, bool use_a, bool use_b)
{
    const int w0 = (int)(int16_t)(wa & 0xffffu), o0 = (int)wa >> 16, w1 = (int)(int16_t)(wb & 0xffffu), o1 = (int)wb >> 16;
    const bool bi = use_a && use_b;
    // one list: the used one as "a" with its weight, the other one's weight 0; the shift and rounding of its form
    const int wA = bi || use_a ? w0 : w1, wB = bi ? w1 : 0;
    const uint32_t pa = bi || use_a ? a : b;
    const int sh = bi ? d + 1 : d, rnd = bi ? 1 << d : (d ? 1 << (d - 1) : 0);
    const int off = bi ? (o0 + o1 + 1) >> 1 : use_a ? o0 : o1;
    int v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = clip255((((int)((pa >> (8 * i)) & 255u) * wA + (int)((b >> (8 * i)) & 255u) * wB + rnd) >> sh) + off);
    return pack4(v[0], v[1], v[2], v[3]);
}
// ---- the seven phase classes: out[y] = the four samples of row y of the lane's 4x4 block -----------------------------
// (ix, iy) = integer position of the block's first sample in the reference, (fx, fy) = quarter-pel phase.
template <class W> __device__ __forceinline__ void mc_copy(uint32_t (&out)[4], const W &w, int ix, int iy)
{
    uint32_t d[9][3];
    w.template load<0, 4, 2>(d, ix, iy);
    const uint32_t s = (uint32_t)ix & 3u;
#pragma unroll
    for (int y = 0; y < 4; y++) out[y] = alignbyte(d[y][1], d[y][0], s);
}
template <class W> __device__ __forceinline__ void mc_h(uint32_t (&out)[4], const W &w, int ix, int iy, int fx)
{   // fx = 1: avg(G, h), 2: h, 3: avg(h, G one to the right)
    uint32_t d[9][3];
    w.template load<0, 4, 3>(d, ix - 2, iy);
    const uint32_t s = (uint32_t)(ix - 2) & 3u, gs = 2u + (uint32_t)(fx == 3);
#pragma unroll
    for (int y = 0; y < 4; y++) {
        uint32_t n0, n1, n2; int t[4];
        align_row(d[y], s, n0, n1, n2);
        tap_h4(n0, n1, n2, 4096 + 16, t);
        const uint32_t hh = round_pack4<5>(t);
        out[y] = sel32(fx == 2, hh, avg4(hh, alignbyte(n1, n0, gs)));
    }
}
template <class W> __device__ __forceinline__ void mc_v(uint32_t (&out)[4], const W &w, int ix, int iy, int fy)
{   // fy = 1: avg(v, G), 2: v, 3: avg(G one down, v)
    uint32_t d[9][3], c[9];
    w.template load<0, 9, 2>(d, ix, iy - 2);
    const uint32_t s = (uint32_t)ix & 3u;
#pragma unroll
    for (int r = 0; r < 9; r++) c[r] = alignbyte(d[r][1], d[r][0], s);
#pragma unroll
    for (int y = 0; y < 4; y++) {
        const uint32_t vv = tap_v4(c[y], c[y + 1], c[y + 2], c[y + 3], c[y + 4], c[y + 5]);
        out[y] = sel32(fy == 2, vv, avg4(vv, sel32(fy == 3, c[y + 3], c[y + 2])));
    }
}
template <class W> __device__ __forceinline__ void mc_diag(uint32_t (&out)[4], const W &w, int ix, int iy, int fx, int fy)
{   // avg(h of row y + (fy == 3), v of column x + (fx == 3)); rows are consumed one at a time to keep the live set small
    uint32_t d[9][3], c[9], hh[5];
    w.template load<0, 9, 3>(d, ix - 2, iy - 2);
    const uint32_t s = (uint32_t)(ix - 2) & 3u, vs = 2u + (uint32_t)(fx == 3);
#pragma unroll
    for (int r = 0; r < 9; r++) {
        uint32_t n0, n1, n2;
        align_row(d[r], s, n0, n1, n2);
        c[r] = alignbyte(n1, n0, vs);
        if (r >= 2 && r <= 6) { int t[4]; tap_h4(n0, n1, n2, 4096 + 16, t); hh[r - 2] = round_pack4<5>(t); }
    }
#pragma unroll
    for (int y = 0; y < 4; y++)
        out[y] = avg4(sel32(fy == 3, hh[y + 1], hh[y]), tap_v4(c[y], c[y + 1], c[y + 2], c[y + 3], c[y + 4], c[y + 5]));
}
// centre position (mc_hc, core/mc.c:200-235): horizontal sums of nine rows, unrounded, then the vertical filter on them,
// (sum + 512) >> 10.  Each row's sum carries + 16, which the vertical taps (sum 32) turn into the + 512 - and which is
// also the rounding term of the horizontal half-pel sample of that row.  A row's sums are folded into the (up to four)
// output rows they belong to as soon as they exist: 16 accumulators instead of 36 sums kept alive.
// WITH: 0 centre only, 1 avg with h of row y + (fy == 3), 2 avg with v of column x + (fx == 3).
template <class W, int WITH> __device__ __forceinline__ void mc_centre(uint32_t (&out)[4], const W &w, int ix, int iy, int fx, int fy)
{
    uint32_t d[9][3];
    w.template load<0, 9, 3>(d, ix - 2, iy - 2);
    const uint32_t s = (uint32_t)(ix - 2) & 3u;
    int acc[4][4];
    uint32_t c[9], hsel[4];
#pragma unroll
    for (int r = 0; r < 9; r++) {
        uint32_t n0, n1, n2; int t[4];
        align_row(d[r], s, n0, n1, n2);
        tap_h4(n0, n1, n2, 4096 + 16, t);
        if (WITH == 2) c[r] = alignbyte(n1, n0, 2u + (uint32_t)(fx == 3));
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const int k = r - y;                           // tap of output row y this window row meets
            if (k < 0 || k > 5) continue;
            const int cv = (k == 0 || k == 5) ? 1 : (k == 1 || k == 4) ? -5 : 20;
#pragma unroll
            for (int x = 0; x < 4; x++) acc[y][x] = k == 0 ? t[x] : acc[y][x] + cv * t[x];
        }
        if (WITH == 1 && r >= 2 && r <= 6) {               // horizontal half-pel sample of window row r: output row r-2 (fy = 1) or r-3 (fy = 3)
            const uint32_t hh = round_pack4<5>(t);
            if (r <= 5) hsel[r - 2] = hh;
            if (r >= 3) hsel[r - 3] = sel32(fy == 3, hh, hsel[r - 3]);
        }
    }
#pragma unroll
    for (int y = 0; y < 4; y++) {
        const uint32_t cc = round_pack4<10>(acc[y]);
        out[y] = WITH == 0 ? cc : WITH == 1 ? avg4(cc, hsel[y]) : avg4(cc, tap_v4(c[y], c[y + 1], c[y + 2], c[y + 3], c[y + 4], c[y + 5]));
    }
}

template <class W> __device__ __forceinline__ void mc_luma_class(int pc, uint32_t (&out)[4], const W &w, int ix, int iy, int fx, int fy)
{
    switch (pc) {                                          // wave-uniform
    case PC_COPY: mc_copy(out, w, ix, iy); break;
    case PC_H:    mc_h(out, w, ix, iy, fx); break;
    case PC_V:    mc_v(out, w, ix, iy, fy); break;
    case PC_DIAG: mc_diag(out, w, ix, iy, fx, fy); break;
    case PC_C:    mc_centre<W, 0>(out, w, ix, iy, fx, fy); break;
    case PC_CH:   mc_centre<W, 1>(out, w, ix, iy, fx, fy); break;
    default:      mc_centre<W, 2>(out, w, ix, iy, fx, fy); break;
    }
}

// XCD-aware block mapping: the dispatcher deals workgroups round-robin over the 8 XCDs; every XCD gets one contiguous
// eighth of the batch, so that the windows of a picture meet in ONE L2 (speed only, never correctness).
__device__ __forceinline__ int xcd_logical_block()
{
    const int per_xcd = gridDim.x >> 3;
    return (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
}

// A list entry as the consumers keep it (first pass: x, y; second pass: all four words), and the macroblock record behind a
// first-pass entry of a chunk with residual (other chunks and padding entries: record 0, one cached request per wavefront -
// asked for without a condition so that the wait for it stays where the record is used).
template <bool PB>
__device__ __forceinline__ uint4 mc_entry_load(const uint32_t *list, int item)
{
    if (PB) return gload4(list + (size_t)item * 4);
    const uint2 t = gload2(list + (size_t)item * 2);
    return make_uint4(t.x, t.y, 0, 0);
}
__device__ __forceinline__ uint3 mc_entry_record(const PicDev *__restrict__ pd, const Geom &g, uint32_t ex, bool resid)
{
    const bool use = resid && mce_valid(ex);
    const int mbi = use ? mce_row(ex) * g.mb_w + mce_col(ex) : 0;
    return gload3(pd->mb + mbi);          // (three words: asked for all four, the compiler recycles the unused register at once and waits for the load there)
}

// ------------------------------------------------------------------------------------------
// what the two role bodies share: the walk over a list's chunks, a chunk's residual fields, the weight of a pair of references
// ------------------------------------------------------------------------------------------
// A wavefront walks the list's chunks from chunk (its workgroup's number among those of the role) * 4 + (its number in the
// workgroup) with a stride of all the wavefronts that work on this list of this picture; the key and the list entries of its
// NEXT chunk are requested before it starts on the current one, so that only the window fetch itself is a memory round trip
// the wavefront has to sit through, and the next chunk's record (first pass, chunks with residual: mc_entry_record) behind the
// current chunk's prediction: its entries have long arrived then, and it is in flight while the chunk adds its residual and
// stores.  (The first chunk and the test for an empty walk stay written out in the bodies, and so do the requests: as members
// of this struct, or as one function returning key word and entry, they moved instructions in k_mc, k_mc_wp and k_mc_second.)
struct McWalk {
    int stride, n_chunks;
    __device__ __forceinline__ int next(int chunk) const { return chunk + stride; }
    __device__ __forceinline__ bool more(int chunk) const { return chunk + stride < n_chunks; }
    // the chunk to request ahead, without a condition - past the list's end the last chunk once more: under `if (more)` the
    // compiler waits for the data inside the branch, one memory round trip per chunk that is no prefetch at all
    __device__ __forceinline__ int ahead(int chunk) const { return min(chunk + stride, n_chunks - 1); }
};
// a chunk's key bits out of the word of class bytes that holds them (k_mc_sort: one byte per chunk); scalar.  (A macro: as a
// function, its two uses in front of mc_entry_record moved instructions in k_mc and k_mc_wp.)
#define MC_CHUNK_KEY(key_w, chunk) ((int)(((key_w) >> (8 * ((chunk) & 3))) & 255u))
// implicit weight of the list-0 prediction for a pair of references of the two-list class (32 = plain average)
__device__ __forceinline__ int mc_pair_weight(const PicDev *__restrict__ pd, int r0c, int r1c)
{
    int wgt = 32;
    if (pd->weighted) wgt = (int)glob(pd->bipred_w)[r0c * P264HIP_MAX_REFS + r1c];
    return wgt;
}
// QP, coded-block mask and place in the coefficient stream of a chunk with residual: with the entry (second pass) or with the
// macroblock's record, requested while the previous chunk was at work.  The bodies call this where the chunk asks for its
// levels, BEHIND its window requests: the record is waited for there and nowhere else - read further up, the wait sat in
// front of the windows, a memory round trip per wavefront at its first chunk.
template <bool PB>
__device__ __forceinline__ void mc_resid_fields(const uint4 &e, uint3 &rec, unsigned &mask, int &qp, uint32_t &cidx)
{
    if (PB) { cidx = mce2_cidx(e.w); mask = mce2_mask(e.z); qp = mce2_qp(e.z); }
    else {
        asm volatile("" : "+v"(rec.x), "+v"(rec.y), "+v"(rec.z));
        cidx = rec.z; mask = (e.x & MCE_Z) ? 0u : (rec.y & 0x03ffffffu); qp = (int)((rec.x >> 8) & 63u);
    }
}
// ------------------------------------------------------------------------------------------
// mc_luma_body<MB, PB> (a role of k_mc / k_mc_second): one wavefront = one chunk of one key: 4 macroblock items of 16 lanes, or 16 quadrant items of 4 lanes;
// the lane is one 4x4 block
// ------------------------------------------------------------------------------------------
template <bool MB, bool PB, bool WP>
__device__ __forceinline__ void mc_luma_body(uint8_t *images, const uint32_t *ref_tab, const PicDev *__restrict__ pd, const uint32_t *__restrict__ mc, const Geom &g,
                                             const McLayout &ml, int sub, int role_wgs)
{
    typedef YItem<MB> I;
    constexpr int LIST = (MB ? ML_YM : ML_YQ) + (PB ? ML_LISTS : 0);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const int stride = role_wgs * 4, n_chunks = (int)mc[LIST];
    const McWalk wk = { stride, n_chunks };
    int chunk = sub * 4 + wave;
    if (chunk >= n_chunks) return;
    const int lane = threadIdx.x & 63, li = lane & (I::LANES - 1), it = lane / I::LANES;
    const uint32_t *cls_w = mc + ml.off_cls[LIST], *list = mc + ml.off_list[LIST];
    const rsrc_t rs = make_rsrc(pd->store, pd->store_bytes);
    uint32_t key_w = cls_w[chunk >> 2];
    uint4 e = mc_entry_load<PB>(list, chunk * I::PER_WAVE + it);
    uint3 rec = make_uint3(0, 0, 0);
    if (!PB) rec = mc_entry_record(pd, g, e.x, (MC_CHUNK_KEY(key_w, chunk) & MCY_RESID) != 0);
  for (;;) {
    const bool more = wk.more(chunk);
    const int nx = wk.ahead(chunk);
    const uint32_t key_w_next = cls_w[nx >> 2];
    const uint4 e_next = mc_entry_load<PB>(list, nx * I::PER_WAVE + it);
    const int key = MC_CHUNK_KEY(key_w, chunk);                   // scalar: the chunk's key bits
    const int pc = key & 7;
    wave_lds_fence();                                      // the previous chunk's image has been read
    const bool valid = mce_valid(e.x);
    const int mbx = valid ? mce_col(e.x) : 0, mby = valid ? mce_row(e.x) : 0;
    // block position inside the macroblock
    const int q = MB ? 0 : (valid ? mce_quad(e.x) : 0);
    const int bx = MB ? (li & 3) : (q & 1) * 2 + (li & 1), by = MB ? (li >> 2) : (q >> 1) * 2 + (li >> 1);
    int mvp = (int)e.y;
    if (!MB && pc == PC_GEN) mvp = (int)gload1(pd->mv + (mby * g.mb_w + mbx) * 16 + by * 4 + bx);   // sub-8x8 partitions: the block's own vector
    // the reference frame of the entry's (list, index): out of the workgroup's table in LDS (mc_roles) - as a load from the
    // picture's tables it was a memory round trip in front of every chunk's window requests (and the wait for it also waited
    // for the next chunk's entries, requested just before: no prefetch)
    const uint32_t roff = ref_tab[MCE_REF_SLOT(e.x)];
    const int ix = mbx * 16 + bx * 4 + (mv_x(mvp) >> 2), iy = mby * 16 + by * 4 + (mv_y(mvp) >> 2);
    const int fx = mv_x(mvp) & 3, fy = mv_y(mvp) & 3;
    const int blk = blk_at(bx, by);                        // decode-order index: bit of coef_mask, position in the packed stream
    // (filled in where the chunk asks for its levels, behind its window requests: mc_resid_fields)
    unsigned mask = 0; int qp = 0; uint32_t cidx = 0; bool coded = false;
    auto resid_fields = [&]() {
        mc_resid_fields<PB>(e, rec, mask, qp, cidx);
        coded = valid && ((mask >> blk) & 1);
    };
    if (PB) resid_fields();
    // coded levels (requested right behind the windows: they fly while the prediction is computed)
    uint4 la = make_uint4(0, 0, 0, 0), lb = la;
    // second pass: the list-0 prediction the first pass left in the destination, as the lane will store it (requested in
    // front of the windows: it has arrived when they have)
    const uint32_t dsto = pd->dst_off + mb_luma_off(g, mbx, mby) + (MB ? (uint32_t)((by * 4 + bx) * 16) : (uint32_t)((by * 4 + ((bx & 1) ? 2 : 0)) * 16 + (bx >> 1) * 8));
    u32x4 prev = { 0, 0, 0, 0 };
    if (PB) {                                              // (compile time; padding lanes read beyond the buffer: zeros, no branch)
        const uint32_t po = valid ? dsto : MC_OOB;
        if (MB) prev = bload4(rs, po);
        else { const u32x2 a = bload2(rs, po), b = bload2(rs, po + 16); prev = u32x4{ a.x, a.y, b.x, b.y }; }
    }
    // ---- prediction ----
    uint32_t out[4];
    if (MB || pc != PC_GEN) {
        // the item's window (all its lanes hold the same vector): top-left sample (wx, wy), staged in LDS
        const int ox = MB ? bx * 4 : (li & 1) * 4, oy = MB ? by * 4 : (li >> 1) * 4;
        const int wx = ix - ox - 2, wy = iy - oy - 2;
        uint8_t *img = images + I::LEAD + I::item_off(wave * I::PER_WAVE + it);
        const bool rows_mid = pc <= PC_H;                  // copy / horizontal: no rows above and below the blocks
        // first sample the class reads in a row (copy / vertical: no columns left of the blocks); image column 0 = its dword
        const int xs = (pc == PC_COPY || pc == PC_V) ? wx + 2 : wx;
        // (macroblock items) six dwords from the first one: the third strip is needed when they start in a strip's last dword
        const bool third = MB && (xs & 12) == 12 && !(pc == PC_COPY || pc == PC_V);
        constexpr int RM = MB ? 16 : 8;
        // (scalar branches: one straight-line staging sequence per shape - rows, strips, clamped or not)
        const bool two = !MB || pc == PC_COPY || pc == PC_V;     // the class reads no columns left of the blocks: two strips at most
        constexpr int S3 = MB ? 3 : 2;
        if (!(key & MCY_CLAMP)) {
            if (rows_mid) { if (two) stage_luma<MB, 2, RM, false, 2>(img, rs, roff, g, xs, wy, li, third); else stage_luma<MB, 2, RM, false, S3>(img, rs, roff, g, xs, wy, li, third); }
            else          { if (two) stage_luma<MB, 0, I::ROWS, false, 2>(img, rs, roff, g, xs, wy, li, third); else stage_luma<MB, 0, I::ROWS, false, S3>(img, rs, roff, g, xs, wy, li, third); }
        } else {
            if (rows_mid) { if (two) stage_luma<MB, 2, RM, true, 2>(img, rs, roff, g, xs, wy, li, third); else stage_luma<MB, 2, RM, true, S3>(img, rs, roff, g, xs, wy, li, third); }
            else          { if (two) stage_luma<MB, 0, I::ROWS, true, 2>(img, rs, roff, g, xs, wy, li, third); else stage_luma<MB, 0, I::ROWS, true, S3>(img, rs, roff, g, xs, wy, li, third); }
        }
        if (key & MCY_RESID) {
            if (!PB) resid_fields();
            if (coded) {
                const int16_t *cf = pd->coefs + ((size_t)cidx + coef_slot(mask, blk)) * 16;
                la = gload4(cf); lb = gload4(cf + 8);
            }
        }
        wave_lds_fence();
        const LWin<I::PITCH> w = { img, xs & ~3, wy };
        mc_luma_class(pc, out, w, ix, iy, fx, fy);
    } else {
        // The vectors differ inside the quadrant (sub-8x8 partitions), every lane has its own window and phase: windows
        // straight from memory, one pass per phase class present among the lanes.
        if (key & MCY_RESID) {
            if (!PB) resid_fields();
            if (coded) {
                const int16_t *cf = pd->coefs + ((size_t)cidx + coef_slot(mask, blk)) * 16;
                la = gload4(cf); lb = gload4(cf + 8);
            }
        }
        // one prediction per lane from reference frame `ro` with vector `mv` (lanes with use = false are left alone)
        auto predict = [&](uint32_t ro, int mv, bool use, uint32_t (&o4)[4]) {
            const GWin w = { rs, ro, g };
            const int px = mbx * 16 + bx * 4 + (mv_x(mv) >> 2), py = mby * 16 + by * 4 + (mv_y(mv) >> 2);
            const int qx = mv_x(mv) & 3, qy = mv_y(mv) & 3;
            const int mine = phase_class(qx, qy);
            o4[0] = o4[1] = o4[2] = o4[3] = 0;
#pragma unroll 1
            for (int c = 0; c < 7; c++) {
                if (__ballot(use && mine == c) == 0) continue;
                // (the window addresses do not depend on c: without this the compiler computes the clamped addresses of every
                // class in front of the loop and keeps all of them alive - far more registers than the rest of the kernel needs)
                int jx = px, jy = py;
                asm volatile("" : "+v"(jx), "+v"(jy));
                uint32_t o[4];
                mc_luma_class(c, o, w, jx, jy, qx, qy);
                if (mine == c) { o4[0] = o[0]; o4[1] = o[1]; o4[2] = o[2]; o4[3] = o[3]; }
            }
        };
        if (key & MCY_CLAMP) predict(roff, mvp, valid, out);
        else if (WP && pd->explicit_wp) {
            // explicit weighted prediction (every inter block of such a picture is here, mc_classify): the lane's lists and
            // indices, a prediction from each list it uses, the weights of (list, index) for luma
            const int mbi = mby * g.mb_w + mbx;
            const bool bpic = pd->slice_type == P264_SLICE_B;         // (wave-uniform)
            const int r0 = (int)glob(pd->ref_idx)[mbi * 4 + q];
            int r1 = -1, mv1 = 0;
            if (bpic) { r1 = (int)glob(pd->ref_idx_l1)[mbi * 4 + q]; mv1 = (int)gload1(pd->mv_l1 + mbi * 16 + by * 4 + bx); }
            const bool u1 = valid && r1 >= 0, u0 = valid && (r0 >= 0 || r1 < 0);
            const int r0c = ref_entry(r0, pd->n_ref), r1c = bpic ? ref_entry(r1, pd->n_ref_l1) : 0;
            const uint32_t ro0 = glob(pd->ref_off)[r0c], ro1 = glob(pd->ref_off_l1)[r1c];
            const uint32_t wa = gload1(pd->wp + r0c * 6), wb = gload1(pd->wp + (P264HIP_MAX_REFS + r1c) * 6);
            uint32_t p0[4], p1[4];
            predict(ro0, mvp, u0, p0);
            predict(ro1, mv1, u1, p1);
#pragma unroll
            for (int y = 0; y < 4; y++) out[y] = wp_combine4(p0[y], p1[y], wa, wb, pd->wp_denom_y, u0, u1);
        } else {
            // B picture, two lists (core/macroblock.c:525-583): which lists the lane's quadrant uses, a prediction from each,
            // then pixel_avg / pixel_avg_weight (core/mc.c:76-132)
            const int mbi = mby * g.mb_w + mbx;
            const int r0 = (int)glob(pd->ref_idx)[mbi * 4 + q], r1 = (int)glob(pd->ref_idx_l1)[mbi * 4 + q];
            const bool u0 = valid && r0 >= 0, u1 = valid && r1 >= 0;
            const int r0c = ref_entry(r0, pd->n_ref), r1c = ref_entry(r1, pd->n_ref_l1);
            const int mv1 = (int)gload1(pd->mv_l1 + mbi * 16 + by * 4 + bx);
            const uint32_t ro0 = glob(pd->ref_off)[r0c], ro1 = glob(pd->ref_off_l1)[r1c];
            const int wgt = mc_pair_weight(pd, r0c, r1c);
            uint32_t p0[4], p1[4];
            predict(ro0, mvp, u0, p0);
            predict(ro1, mv1, u1, p1);
#pragma unroll
            for (int y = 0; y < 4; y++) {
                const uint32_t both = pd->weighted ? bipred_weight4(p0[y], p1[y], wgt) : bipred_avg4(p0[y], p1[y]);
                out[y] = (u0 && u1) ? both : u0 ? p0[y] : p1[y];
            }
        }
    }
    // the next chunk's record (McWalk)
    if (!PB) rec = mc_entry_record(pd, g, e_next.x, (MC_CHUNK_KEY(key_w_next, nx) & MCY_RESID) != 0);
    if (PB) {
        // (core/macroblock.c:525-583, core/mc.c:76-132) the first pass's rows back into block order, then the mean or the weighted sum
        uint32_t p0[4];
        if (MB) { const uint32_t pr[4] = { prev.x, prev.y, prev.z, prev.w }; quad_transpose(p0, pr, lane); }
        else {
            // the lane loaded rows (2 * right, 2 * right + 1) of the pair of blocks: its own halves stay, the others swap
            const bool right = bx & 1;
            const uint32_t g0 = lane_xor1(right ? prev.x : prev.y), g1 = lane_xor1(right ? prev.z : prev.w);
            p0[0] = right ? g0 : prev.x; p0[1] = right ? g1 : prev.z; p0[2] = right ? prev.y : g0; p0[3] = right ? prev.w : g1;
        }
        const int wgt = mce2_weight(e.w);
#pragma unroll
        for (int y = 0; y < 4; y++) out[y] = pd->weighted ? bipred_weight4(p0[y], out[y], wgt) : bipred_avg4(p0[y], out[y]);
    }
    // ---- residual (decoder/macroblock.c:839-847) ----
    if ((key & MCY_RESID) && __ballot(coded)) {
        const uint32_t lv[8] = { la.x, la.y, la.z, la.w, lb.x, lb.y, lb.z, lb.w };
        uint32_t col[4][2];
        unscan_cols<false>(lv, col);
        dequant_cols(col, qp);
        uint32_t px[4] = { out[0], out[1], out[2], out[3] };
        idct_add(col, px);
        if (coded) { out[0] = px[0]; out[1] = px[1]; out[2] = px[2]; out[3] = px[3]; }
    }
    // ---- store: the two lanes of a block row swap halves, so that a lane writes two rows of 8 samples (four lanes: eight
    // consecutive rows, one or two cache lines) instead of four rows of 4 ----
    if (MB) {
        // macroblock items: the four lanes of a quad are the four blocks of a block row - transposed, a lane writes one
        // whole 16-byte row and the macroblock's sixteen lanes two whole cache lines
        uint32_t t[4];
        quad_transpose(t, out, lane);
        if (valid) bstore4(rs, dsto, t[0], t[1], t[2], t[3]);
    } else {
        const bool right = bx & 1;
        const uint32_t g0 = lane_xor1(right ? out[0] : out[2]), g1 = lane_xor1(right ? out[1] : out[3]);
        const uint32_t r0a = right ? g0 : out[0], r0b = right ? out[2] : g0;       // row 4*by + 2*right: samples 0-3, 4-7
        const uint32_t r1a = right ? g1 : out[1], r1b = right ? out[3] : g1;       // the row below
        if (valid) {
            bstore2(rs, dsto, r0a, r0b);
            bstore2(rs, dsto + 16, r1a, r1b);
        }
    }
    if (!more) break;
    chunk = wk.next(chunk); key_w = key_w_next; e = e_next;
  }
}
// ------------------------------------------------------------------------------------------
// mc_chroma_body<MB, PB> (a role of k_mc / k_mc_second): one wavefront = one chunk: 8 macroblock items of 8 lanes or 32 quadrant items of 2 lanes;
// the lane is one 4x4 chroma block (quadrant, plane)
// ------------------------------------------------------------------------------------------
// 1/8-pel bilinear (core/mc.c:303-334) of one 4x4 block from the two aligned dwords d0, d1 of five window rows; the
// block's first sample is byte s of d0; weights (dx, dy)
__device__ __forceinline__ void chroma_bilinear(uint32_t (&out)[4], const uint32_t (&d0)[5], const uint32_t (&d1)[5], uint32_t s, int dx, int dy)
{
    uint32_t a[5], b[5];                                   // bytes cx..cx+3 and cx+1..cx+4 of rows cy..cy+4
#pragma unroll
    for (int r = 0; r < 5; r++) { a[r] = alignbyte(d1[r], d0[r], s); b[r] = alignbyte(d1[r] >> (8 * s), a[r], 1); }
    // sample x of row y: (8-dx)(8-dy) A + dx (8-dy) B + (8-dx) dy C + dx dy D + 32 >> 6 as one 4-byte dot product with
    // the weights (they fit a byte: at most 64), A B adjacent in row y, C D in row y + 1
    const uint32_t wts = (uint32_t)((8 - dx) * (8 - dy)) | (uint32_t)(dx * (8 - dy)) << 8 | (uint32_t)((8 - dx) * dy) << 16 | (uint32_t)(dx * dy) << 24;
#pragma unroll
    for (int y = 0; y < 4; y++) {
        const uint32_t v0 = __builtin_amdgcn_udot4(perm(a[y + 1], a[y], 0x05040100u), wts, 32u, false);
        const uint32_t v1 = __builtin_amdgcn_udot4(perm(a[y + 1], a[y], 0x06050201u), wts, 32u, false);
        const uint32_t v2 = __builtin_amdgcn_udot4(perm(a[y + 1], a[y], 0x07060302u), wts, 32u, false);
        const uint32_t v3 = __builtin_amdgcn_udot4(perm(b[y + 1], b[y], 0x07060302u), wts, 32u, false);
        // v < 2^14: (v0 | v1 << 16) >> 6 leaves sample 0 in byte 0 and sample 1 in byte 2
        const uint32_t w01 = (v0 | (v1 << 16)) >> 6, w23 = (v2 | (v3 << 16)) >> 6;
        out[y] = perm(w23, w01, 0x06040200u);
    }
}
// the window straight from memory, coordinates clamped to the picture (slow class only)
__device__ __forceinline__ void mc_chroma_clamped(uint32_t (&out)[4], rsrc_t rs, uint32_t roff, const Geom &g, int p, int cx, int cy, int dx, int dy)
{
    const int xa = cx & ~3;
    uint32_t d0[5], d1[5], col[2], sel[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int x = xa + 4 * k, xc = clip3i(x, 0, g.cw - 4);
        col[k] = roff + g.coff + strip_mul(xc >> 3, g.cstrip) + (uint32_t)(p * 8 + (xc & 7));
        sel[k] = x < 0 ? 0x00000000u : x >= g.cw ? 0x03030303u : 0x03020100u;
    }
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const uint32_t ro = (uint32_t)clip3i(cy + r, 0, g.ch - 1) * 16u;
        const uint32_t v0 = bload(rs, col[0] + ro), v1 = bload(rs, col[1] + ro);
        d0[r] = perm(v0, v0, sel[0]); d1[r] = perm(v1, v1, sel[1]);
    }
    chroma_bilinear(out, d0, d1, (uint32_t)cx & 3u, dx, dy);
}


// Chroma work items: image row = strip A (8 U, 8 V) | strip B (8 U, 8 V) + 8 bytes; a macroblock window has 9 rows, a
// quadrant window 5.
template <bool MB> struct CItem {
    static constexpr int LANES = MB ? 8 : 2, PER_WAVE = 64 / LANES, ROWS = MB ? 9 : 5;
    static constexpr int PITCH = 40, BYTES = ROWS * PITCH + 8;
    // macroblock items: a lane reads dword row * 10 + 2 plane + (block column) of its item, the block rows 40 dwords apart: the
    // eight lanes of an item cover banks {0 .. 3} and {8 .. 11} (of 32, see YItem).  Items in pairs, 100 dwords apart inside a
    // pair and 208 from pair to pair: bank = 16 (item / 2) + 4 (item % 2) + ... - the four items of a 32-lane group tile the 32
    // banks (92 dwords per item as before put items 0 and 2, 1 and 3 on the same banks).  What is left of this role's conflicts
    // comes from the windows' own column offset (0, 1, 4 or 5 dwords by the vector), which differs from item to item.
    static constexpr int PAIR = 832, SECOND = 400;
    static constexpr int WAVE_BYTES = MB ? (PER_WAVE / 2) * PAIR : PER_WAVE * BYTES;
    static_assert(!MB || (BYTES <= SECOND && SECOND + BYTES <= PAIR), "item image");
    __device__ static __forceinline__ int item_off(int i) { return MB ? (i >> 1) * PAIR + (i & 1) * SECOND : i * BYTES; }
};
// one 16-byte row piece of a chroma strip, coordinates clamped to the picture if CLAMP (a strip outside becomes the
// replicated first / last sample of each plane's 8 bytes)
template <bool CLAMP> __device__ __forceinline__ u32x4 chroma_piece_load(rsrc_t rs, uint32_t roff, const Geom &g, int strip, int y, bool need)
{
    if (!CLAMP) return wload4(rs, need ? roff + g.coff + strip_mul(strip, g.cstrip) + (uint32_t)(y * 16) : MC_OOB);
    const int sc = clip3i(strip, 0, g.mb_w - 1);             // (a chroma strip is 8 samples wide: one per macroblock column)
    return wload4(rs, need ? roff + g.coff + strip_mul(sc, g.cstrip) + (uint32_t)(clip3i(y, 0, g.ch - 1) * 16) : MC_OOB);
}
// a strip outside the picture becomes the replicated first / last sample of each plane's 8 bytes
__device__ __forceinline__ u32x4 chroma_piece_clamp(u32x4 t, const Geom &g, int strip)
{
    if (strip < 0) { const uint32_t u = perm(t.x, t.x, 0x00000000u), v = perm(t.z, t.z, 0x00000000u); t.x = t.y = u; t.z = t.w = v; }
    if (strip >= g.mb_w) { const uint32_t u = perm(t.y, t.y, 0x03030303u), v = perm(t.w, t.w, 0x03030303u); t.x = t.y = u; t.z = t.w = v; }
    return t;
}
__device__ __forceinline__ void lds_put16(uint8_t *p, u32x4 v) { *(uint2 *)p = make_uint2(v.x, v.y); *(uint2 *)(p + 8) = make_uint2(v.z, v.w); }

template <bool MB, bool PB, bool WP>
__device__ __forceinline__ void mc_chroma_body(uint8_t *images, const uint32_t *ref_tab, const PicDev *__restrict__ pd, const uint32_t *__restrict__ mc, const Geom &g,
                                               const McLayout &ml, int sub, int role_wgs)
{
    typedef CItem<MB> I;
    constexpr int LIST = (MB ? ML_CM : ML_CQ) + (PB ? ML_LISTS : 0);
    const int wave = rfl((int)(threadIdx.x >> 6));
    const int stride = role_wgs * 4, n_chunks = (int)mc[LIST];
    const McWalk wk = { stride, n_chunks };
    int chunk = sub * 4 + wave;
    if (chunk >= n_chunks) return;
    const int lane = threadIdx.x & 63, p = lane & 1, li = lane & (I::LANES - 1), it = lane / I::LANES;
    const uint32_t *cls_w = mc + ml.off_cls[LIST], *list = mc + ml.off_list[LIST];
    const rsrc_t rs = make_rsrc(pd->store, pd->store_bytes);
    uint32_t key_w = cls_w[chunk >> 2];
    uint4 e = mc_entry_load<PB>(list, chunk * I::PER_WAVE + it);
    uint3 rec = make_uint3(0, 0, 0);
    if (!PB) rec = mc_entry_record(pd, g, e.x, (MC_CHUNK_KEY(key_w, chunk) & MCC_RESID) != 0);
  for (;;) {
    const bool more = wk.more(chunk);
    const int nx = wk.ahead(chunk);
    const uint32_t key_w_next = cls_w[nx >> 2];
    const uint4 e_next = mc_entry_load<PB>(list, nx * I::PER_WAVE + it);
    const int key = MC_CHUNK_KEY(key_w, chunk);
    wave_lds_fence();                                      // the previous chunk's image has been read
    const bool valid = mce_valid(e.x);
    const int mbx = valid ? mce_col(e.x) : 0, mby = valid ? mce_row(e.x) : 0;
    const int q = MB ? (li >> 1) : (valid ? mce_quad(e.x) : 0);
    const uint32_t roff = ref_tab[MCE_REF_SLOT(e.x)];         // (the workgroup's table in LDS: see mc_luma_body)
    // the 16-byte row this lane stores (see the end of the loop); second pass: what the first pass left there
    const uint32_t dsto = pd->dst_off + mb_chroma_off(g, mbx, mby) + (uint32_t)((q >> 1) * 64 + (lane & 3) * 16);
    u32x4 prev = { 0, 0, 0, 0 };
    if (PB) prev = bload4(rs, valid ? dsto : MC_OOB);
    const int CX = mbx * 8 + (q & 1) * 4, CY = mby * 8 + (q >> 1) * 4;      // the block's first sample
    const int cb = 16 + 4 * p + q;                           // this block's bit of coef_mask
    unsigned mask = 0; int qp = 0; uint32_t cidx = 0; bool has_res = false;      // (filled in behind the window requests: mc_resid_fields)
    auto resid_fields = [&]() {
        mc_resid_fields<PB>(e, rec, mask, qp, cidx);
        has_res = valid && (mask & (0x00ff0000u | P264_COEF_CHROMA_DC)) != 0;
    };
    if (PB) resid_fields();
    uint4 la = make_uint4(0, 0, 0, 0), lb = la; uint2 dcl = make_uint2(0, 0);
    // ---- prediction ----
    uint32_t out[4];
    const bool staged = MB || !(key & (MCC_CLAMP | MCC_BI));
    if (staged) {
        // the item's window goes through LDS like the luma windows: 16-byte pieces (8 U, 8 V) of consecutive rows
        const int mvx = mv_x((int)e.y), mvy = mv_y((int)e.y);
        const int cx = CX + (mvx >> 3), cy = CY + (mvy >> 3);                // the block's window
        const int wx = cx - (q & 1) * 4, wy = cy - (q >> 1) * 4;             // the macroblock's window (MB); equals (cx, cy) for q = 0
        uint8_t *img;
        int x0, y0;                                                          // image origin
        if (MB) {
            // 9 rows x 2 strips = 18 pieces over 8 lanes: piece li + 8j = strip (p / 9), row p % 9
            img = images + I::item_off(wave * I::PER_WAVE + it);
            const int sA = wx >> 3;
            x0 = sA * 8; y0 = wy;
            // (ONE scalar branch around the whole sequence, every piece requested in a row and waited for once: with the clamped /
            // plain choice made per piece the compiler waited for every piece inside its own branch - three round trips)
            auto stage = [&](auto clamp_tag) {
                constexpr bool CL = decltype(clamp_tag)::value;
                u32x4 v[3]; int dst[3];
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    const int pp = min(li + 8 * j, 17), s = pp >= 9 ? 1 : 0, row = pp - 9 * s;
                    dst[j] = row * I::PITCH + s * 16;
                    // (pieces 16 and 17 only in the third round: the other lanes ask beyond the buffer - zeros, no memory request)
                    v[j] = chroma_piece_load<CL>(rs, roff, g, sA + s, wy + row, j < 2 || li < 2);
                }
#pragma unroll
                for (int j = 0; j < 3; j++) loads_land(v[j]);
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    if (CL) v[j] = chroma_piece_clamp(v[j], g, sA + (min(li + 8 * j, 17) >= 9 ? 1 : 0));
                    if (j < 2 || li < 2) lds_put16(img + dst[j], v[j]);
                }
            };
            if (key & MCC_CLAMP) stage(std::true_type{}); else stage(std::false_type{});
        } else {
            // Four lanes = two quadrants stage together: rows 0..3 of one strip of one quadrant per load (64 contiguous
            // bytes), then row 4 of their own strips.
            const int sA = cx >> 3;
            x0 = sA * 8; y0 = cy;
            const uint32_t own = roff + g.coff + strip_mul(sA, g.cstrip) + (uint32_t)(cy * 16), other = lane_xor2(own);
            const int i = lane & 3;
            uint8_t *pimg = images + (wave * I::PER_WAVE + (lane >> 2) * 2) * I::BYTES;
            u32x4 v[5];
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = wload4(rs, (((j >> 1) == (i >> 1)) ? own : other) + (uint32_t)(j & 1) * g.cstrip + (uint32_t)(i * 16));
            v[4] = wload4(rs, own + (uint32_t)(i & 1) * g.cstrip + 64u);
#pragma unroll
            for (int j = 0; j < 4; j++) lds_put16(pimg + (j >> 1) * I::BYTES + i * I::PITCH + (j & 1) * 16, v[j]);
            lds_put16(pimg + (i >> 1) * I::BYTES + 4 * I::PITCH + (i & 1) * 16, v[4]);
            img = pimg + (i >> 1) * I::BYTES;
        }
        if (key & MCC_RESID) {
            if (!PB) resid_fields();
            const int16_t *cf = pd->coefs + (size_t)cidx * 16;
            if (has_res && ((mask >> cb) & 1)) { const int16_t *c = cf + coef_slot(mask, cb) * 16; la = gload4(c); lb = gload4(c + 8); }
            if (has_res && (mask & P264_COEF_CHROMA_DC)) dcl = gload2(cf + ((mask >> 24) & 1) * 16 + p * 4);
        }
        wave_lds_fence();
        // the lane's five rows, two aligned dwords each: sample x of plane p sits at ((x - x0) >> 3) * 16 + p * 8 + (x & 7)
        const int xa = cx & ~3;
        const uint8_t *b = img + (cy - y0) * I::PITCH + p * 8;
        const int o0 = ((xa - x0) >> 3) * 16 + (xa & 7), o1 = ((xa + 4 - x0) >> 3) * 16 + ((xa + 4) & 7);
        uint32_t d0[5], d1[5];
#pragma unroll
        for (int r = 0; r < 5; r++) { d0[r] = *(const uint32_t *)(b + r * I::PITCH + o0); d1[r] = *(const uint32_t *)(b + r * I::PITCH + o1); }
        chroma_bilinear(out, d0, d1, (uint32_t)cx & 3u, mvx & 7, mvy & 7);
    } else {
        // quadrant items outside the picture or with different vectors inside (sub-8x8 partitions: every 2x2 chroma piece
        // follows its own vector): clamped windows straight from memory, one pass per piece, wave-uniformly skipped when
        // nobody needs it
        if (key & MCC_RESID) {
            if (!PB) resid_fields();
            const int16_t *cf = pd->coefs + (size_t)cidx * 16;
            if (has_res && ((mask >> cb) & 1)) { const int16_t *c = cf + coef_slot(mask, cb) * 16; la = gload4(c); lb = gload4(c + 8); }
            if (has_res && (mask & P264_COEF_CHROMA_DC)) dcl = gload2(cf + ((mask >> 24) & 1) * 16 + p * 4);
        }
        const int b0 = (q >> 1) * 8 + (q & 1) * 2;
        const int mbi = mby * g.mb_w + mbx;
        // the lane's 4x4 chroma block from reference frame `ro`, the vectors of the quadrant's four luma blocks at `mvs`
        auto predict = [&](uint32_t ro, const int *mvs, bool use, uint32_t (&o4)[4]) {
            const uint2 va = gload2(mvs + mbi * 16 + b0), vb = gload2(mvs + mbi * 16 + b0 + 4);
            const bool uniform = va.x == va.y && va.x == vb.x && va.x == vb.y;
            const int v4[4] = { (int)va.x, (int)va.y, (int)vb.x, (int)vb.y };
            o4[0] = o4[1] = o4[2] = o4[3] = 0;
#pragma unroll 1
            for (int sb = 0; sb < 4; sb++) {
                if (sb > 0 && __ballot(use && !uniform) == 0) break;
                const int mv = sb == 0 ? v4[0] : sb == 1 ? v4[1] : sb == 2 ? v4[2] : v4[3];
                uint32_t o[4];
                mc_chroma_clamped(o, rs, ro, g, p, CX + (mv_x(mv) >> 3), CY + (mv_y(mv) >> 3), mv_x(mv) & 7, mv_y(mv) & 7);
                if (uniform) { if (sb == 0) { o4[0] = o[0]; o4[1] = o[1]; o4[2] = o[2]; o4[3] = o[3]; } }
                else {
                    const uint32_t m = (sb & 1) ? 0xffff0000u : 0x0000ffffu;
                    const int r0 = (sb >> 1) * 2;
                    o4[0] = r0 == 0 ? (o4[0] & ~m) | (o[0] & m) : o4[0]; o4[1] = r0 == 0 ? (o4[1] & ~m) | (o[1] & m) : o4[1];
                    o4[2] = r0 == 2 ? (o4[2] & ~m) | (o[2] & m) : o4[2]; o4[3] = r0 == 2 ? (o4[3] & ~m) | (o[3] & m) : o4[3];
                }
            }
        };
        if (!(key & MCC_BI)) predict(roff, (valid && (e.x & MCE_LIST1)) ? pd->mv_l1 : pd->mv, valid, out);      // (padding lanes: list 0, mv_l1 is null outside B pictures)
        else if (WP && pd->explicit_wp) {
            // explicit weighted prediction: as in mc_luma_body, with the weights of the lane's plane (Cb = plane 0, Cr = plane 1)
            const bool bpic = pd->slice_type == P264_SLICE_B;         // (wave-uniform)
            const int r0 = (int)glob(pd->ref_idx)[mbi * 4 + q], r1 = bpic ? (int)glob(pd->ref_idx_l1)[mbi * 4 + q] : -1;
            const bool u1 = valid && r1 >= 0, u0 = valid && (r0 >= 0 || r1 < 0);
            const int r0c = ref_entry(r0, pd->n_ref), r1c = bpic ? ref_entry(r1, pd->n_ref_l1) : 0;
            const uint32_t ro0 = glob(pd->ref_off)[r0c], ro1 = glob(pd->ref_off_l1)[r1c];
            const uint32_t wa = gload1(pd->wp + r0c * 6 + 2 + 2 * p), wb = gload1(pd->wp + (P264HIP_MAX_REFS + r1c) * 6 + 2 + 2 * p);
            uint32_t p0[4], p1[4] = { 0, 0, 0, 0 };
            predict(ro0, pd->mv, u0, p0);
            if (bpic) predict(ro1, pd->mv_l1, u1, p1);
#pragma unroll
            for (int y = 0; y < 4; y++) out[y] = wp_combine4(p0[y], p1[y], wa, wb, pd->wp_denom_c, u0, u1);
        } else {
            // B picture, two lists: as in mc_luma_body
            const int r0 = (int)glob(pd->ref_idx)[mbi * 4 + q], r1 = (int)glob(pd->ref_idx_l1)[mbi * 4 + q];
            const bool u0 = valid && r0 >= 0, u1 = valid && r1 >= 0;
            const int r0c = ref_entry(r0, pd->n_ref), r1c = ref_entry(r1, pd->n_ref_l1);
            const uint32_t ro0 = glob(pd->ref_off)[r0c], ro1 = glob(pd->ref_off_l1)[r1c];
            const int wgt = mc_pair_weight(pd, r0c, r1c);
            uint32_t p0[4], p1[4];
            predict(ro0, pd->mv, u0, p0);
            predict(ro1, pd->mv_l1, u1, p1);
#pragma unroll
            for (int y = 0; y < 4; y++) {
                const uint32_t both = pd->weighted ? bipred_weight4(p0[y], p1[y], wgt) : bipred_avg4(p0[y], p1[y]);
                out[y] = (u0 && u1) ? both : u0 ? p0[y] : p1[y];
            }
        }
    }
    // the next chunk's record (McWalk)
    if (!PB) rec = mc_entry_record(pd, g, e_next.x, (MC_CHUNK_KEY(key_w_next, nx) & MCC_RESID) != 0);
    if (PB) {
        // the first pass's rows (dwords U left, U right, V left, V right) back into block order; then the mean or the weighted
        // sum, or - quadrants that were finished in the first pass - the samples as they are
        const uint32_t pr[4] = { prev.x, prev.z, prev.y, prev.w };
        uint32_t p0[4];
        quad_transpose(p0, pr, lane);
        const int wgt = mce2_weight(e.w);
        const bool keep = (e.x & MCE_KEEP) != 0;
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const uint32_t both = pd->weighted ? bipred_weight4(p0[y], out[y], wgt) : bipred_avg4(p0[y], out[y]);
            out[y] = keep ? p0[y] : both;
        }
    }
    // ---- residual (decoder/macroblock.c:851-890): chroma DC through the 2x2 transform, AC, inverse transform ----
    if ((key & MCC_RESID) && __ballot(has_res)) {
        const int qpc = chroma_qp(clip3i(qp + pd->chroma_qp_offset, 0, 51));
        const uint32_t lv[8] = { la.x, la.y, la.z, la.w, lb.x, lb.y, lb.z, lb.w };
        uint32_t col[4][2];
        unscan_cols<true>(lv, col);
        dequant_cols(col, qpc);
        const int dc = chroma_dc_level(dcl, q & 1, q & 2, qpc);
        col[0][0] = (col[0][0] & 0xffff0000u) | ((uint32_t)dc & 0xffffu);
        uint32_t px[4] = { out[0], out[1], out[2], out[3] };
        idct_add(col, px);
        if (has_res) { out[0] = px[0]; out[1] = px[1]; out[2] = px[2]; out[3] = px[3]; }
    }
    {
        // (Quadrant items: the four entries of a split macroblock are consecutive, so its eight lanes sit exactly like the
        // eight lanes of a macroblock item.)  The four lanes of a quad hold the four dwords of the same four rows (U left, V left, U right, V right block):
        // transpose among them, so that a lane writes ONE whole 16-byte row and a macroblock's eight lanes one cache line
        // (four 4-byte stores per lane kept the address unit busier than anything else in this kernel).
        uint32_t t[4];
        quad_transpose(t, out, lane);
        if (valid) bstore4(rs, dsto, t[0], t[2], t[1], t[3]);      // lane-in-quad = plane + 2 * (block column): dwords U0 U1 V0 V1
    }
    if (!more) break;
    chunk = wk.next(chunk); key_w = key_w_next; e = e_next;
  }
}
// ------------------------------------------------------------------------------------------
// k_mc: ONE launch for the four kinds of work.  A picture gets `wgs_per_pic` consecutive (logical) workgroups; they split
// into the four roles - luma macroblock items, luma quadrant items, chroma macroblock items, chroma quadrant items - in
// proportion to the work the picture's lists hold (chunks in use x a cost weight per chunk, measured), decided on the device
// from the counts k_mc_sort left.  All four roles of a picture run at the same time on the same XCD and walk the picture's
// bands in step: a reference line fetched for a macroblock item is in L2 when the quadrant item next to it and the chroma
// windows ask for it (as four launches every kernel pulled the whole reference through HBM again: measured 7.0 GB of reads
// against 3.1 GB of reference samples), and the bandwidth-bound chroma work shares its CU with the issue-bound luma work.
// ------------------------------------------------------------------------------------------
#define MC_COST_YM 7u               // relative cost of one chunk (wavefront pass) per role, from the round-2 profiles (swept again in round 5: scratch/r5_mccost.sh)
#define MC_COST_YQ 10u
#define MC_COST_CM 5u
#define MC_COST_CQ 9u
template <bool PB, bool WP>
__device__ __forceinline__ void mc_roles(uint8_t *images, uint32_t *ref_tab, const PicDev *__restrict__ pics, const uint32_t *__restrict__ mc_all, const Geom &g, const McLayout &ml,
                                         int wgs_per_pic, int n_wgs, uint32_t inv_wgs)
{
    constexpr int L0 = PB ? ML_LISTS : 0;
    const int logical = xcd_logical_block();
    if (logical >= n_wgs) return;
    int pic = (int)__umulhi((unsigned)logical, inv_wgs);
    if (logical - pic * wgs_per_pic >= wgs_per_pic) pic++;
    const int s = logical - pic * wgs_per_pic;
    const PicDev *pd = pics + pic;
    const uint32_t *mc = mc_all + (size_t)pic * ml.words;  // (addresses from kernel arguments only: the first loads depend on nothing)
    // the picture's reference frames by (list, index) for the workgroup's wavefronts: entries past a list's end repeat entry 0
    // (p264hip_reconstruct), list 1 exists for B pictures only; the bodies index it with MCE_REF_SLOT
    if (threadIdx.x < 2 * P264HIP_MAX_REFS) {
        const int k = threadIdx.x & (P264HIP_MAX_REFS - 1);
        ref_tab[threadIdx.x] = threadIdx.x < P264HIP_MAX_REFS ? pd->ref_off[k] : (pd->slice_type == P264_SLICE_B ? pd->ref_off_l1[k] : pd->ref_off[0]);
    }
    __syncthreads();
    // role split (scalar): every non-empty list gets one workgroup, the rest go by cost
    const uint32_t n0 = mc[L0 + ML_YM], n1 = mc[L0 + ML_YQ], n2 = mc[L0 + ML_CM], n3 = mc[L0 + ML_CQ];
    const uint32_t t0 = n0 * MC_COST_YM, t1 = n1 * MC_COST_YQ, t2 = n2 * MC_COST_CM, t3 = n3 * MC_COST_CQ, tt = t0 + t1 + t2 + t3;
    if (tt == 0) return;
    const uint32_t nz = (n0 != 0) + (n1 != 0) + (n2 != 0) + (n3 != 0), spare = (uint32_t)wgs_per_pic - nz;       // wgs_per_pic >= 4
    const float inv = (float)spare / (float)tt;
    const int w1 = (n1 != 0) + (int)((float)t1 * inv), w2 = (n2 != 0) + (int)((float)t2 * inv), w3 = (n3 != 0) + (int)((float)t3 * inv);
    const int w0 = wgs_per_pic - w1 - w2 - w3;             // (luma macroblock items take the rounding remainder)
    if (s < w0) mc_luma_body<true, PB, WP>(images, ref_tab, pd, mc, g, ml, s, w0);
    else if (s < w0 + w1) mc_luma_body<false, PB, WP>(images, ref_tab, pd, mc, g, ml, s - w0, w1);
    else if (s < w0 + w1 + w2) mc_chroma_body<true, PB, WP>(images, ref_tab, pd, mc, g, ml, s - w0 - w1, w2);
    else mc_chroma_body<false, PB, WP>(images, ref_tab, pd, mc, g, ml, s - w0 - w1 - w2, w3);
}
#define MC_IMAGE_BYTES (YItem<false>::LEAD + 4 * YItem<false>::WAVE_BYTES)         // the largest of the four roles' images
static_assert(MC_IMAGE_BYTES >= YItem<true>::LEAD + 4 * YItem<true>::WAVE_BYTES && MC_IMAGE_BYTES >= 4 * CItem<true>::WAVE_BYTES && MC_IMAGE_BYTES >= 4 * CItem<false>::WAVE_BYTES, "image space");
#define MC_WAVES_PER_EU 4
__global__ __launch_bounds__(256, MC_WAVES_PER_EU)
void k_mc(const PicDev *__restrict__ pics, const uint32_t *__restrict__ mc_all, Geom g, McLayout ml, int wgs_per_pic, int n_wgs, uint32_t inv_wgs)
{
    __shared__ __attribute__((aligned(16))) uint8_t images[MC_IMAGE_BYTES];
    __shared__ uint32_t ref_tab[2 * P264HIP_MAX_REFS];
    mc_roles<false, false>(images, ref_tab, pics, mc_all, g, ml, wgs_per_pic, n_wgs, inv_wgs);
}
// batches with a picture of explicit weighted prediction: k_mc with the weighted generic class compiled in (mc_classify sends every
// inter macroblock of such a picture there; the batch's other pictures run exactly as in k_mc) - a launch of its own so that k_mc
// keeps its registers and unweighted batches run nothing new.  (Three wavefronts per SIMD: with k_mc's four the weighted generic
// class spills three registers.)
__global__ __launch_bounds__(256, 3)
void k_mc_wp(const PicDev *__restrict__ pics, const uint32_t *__restrict__ mc_all, Geom g, McLayout ml, int wgs_per_pic, int n_wgs, uint32_t inv_wgs)
{
    __shared__ __attribute__((aligned(16))) uint8_t images[MC_IMAGE_BYTES];
    __shared__ uint32_t ref_tab[2 * P264HIP_MAX_REFS];
    mc_roles<false, true>(images, ref_tab, pics, mc_all, g, ml, wgs_per_pic, n_wgs, inv_wgs);
}
// B pictures: the second pass (list-1 predictions of the blocks that use both lists), behind k_mc
__global__ __launch_bounds__(256, 4)
void k_mc_second(const PicDev *__restrict__ pics, const uint32_t *__restrict__ mc_all, Geom g, McLayout ml, int wgs_per_pic, int n_wgs, uint32_t inv_wgs)
{
    __shared__ __attribute__((aligned(16))) uint8_t images[MC_IMAGE_BYTES];
    __shared__ uint32_t ref_tab[2 * P264HIP_MAX_REFS];
    mc_roles<true, false>(images, ref_tab, pics, mc_all, g, ml, wgs_per_pic, n_wgs, inv_wgs);
}
