// kernel_resize.h - a batch of decoded pictures out of the frame stores into the caller's device memory, a window of each RESIZED
// by the fixed-point bilinear filter of include/p264hip.h (p264hip_resize_t has the taps, the sum, the layouts and the float step):
// as I420 / NV12 / RGB24 / planar RGB bytes, the two RGB formats also as float16 / float32 after a scale and a bias per channel.
//
// Destination-driven: a lane produces RESIZE_PX = 4 horizontally adjacent output samples, a wavefront a TILE of 256 samples of a row
//   luma tiles    two output rows (y, y + 1) of 256 samples; the RGB formats resize the chroma row y >> 1 beside them - a lane's two
//                 chroma samples per plane, computed once for its 2 x 2 output blocks and used for both rows
//   chroma tiles  I420 / NV12 only: one row of 256 chroma samples, U and V
// so the source rows of a tile are the same for all of its lanes: the row taps are wave-uniform in every tile.  The taps come from
// four tables the host builds per call with p264hip_resize_taps (luma and chroma, x and y; the window's offset folded in): one word
// per destination index, fraction | (i1 - i0) << 8 | i0 << 16 with i0 a coordinate of the FRAME - the kernel divides nothing.  They
// travel behind the call's frame indices in the same table.  A lane gathers the four source bytes of each of its samples one by
// one from the strip layout (device_common.h: luma_off / chroma_off), all of them before its first store: 48 byte loads for
// an RGB lane, 32 for the others.  Reducing 1920 x 1080 to 224 x 224 a tile's taps are 8 and more samples apart, so staging source
// rows in LDS would carry seven unused bytes in eight; enlarging, neighbouring lanes read the same bytes and the vector cache
// serves them.  (Staging rows in LDS was not measured.)  No LDS.
// The lanes of a row store contiguous bytes: 4 per lane for a u8 plane, 8 as float16, 16 as float32 (RGB24: three times that).  A lane
// whose samples all lie in the row and whose destination is aligned to that size stores 4 / 8 / 16 bytes at a time, non-temporal
// as kernel_export.h's; any other lane - the last one of a row whose width is no multiple of 4, every lane of a destination or
// pitch that is not aligned - stores its elements one by one (kernel_export.h's put_piece, chosen per lane).
// Grid: (tiles of a picture / 4, pictures); a wavefront never mixes pictures.
#pragma once
#include "device_common.h"
#include "lane_ops.h"
#include "kernel_export.h"

#define RESIZE_THREADS 256
#define RESIZE_PX      4                        // output samples of a lane in a row
#define RESIZE_TILE_W  (WAVE * RESIZE_PX)       // output samples of a tile in a row

struct ResizeParams {
    int32_t w, h;                   // the output
    int32_t ltx, n_ltiles;          // luma tiles: per tile row, per picture
    int32_t ctx, n_tiles;           // chroma tiles per tile row (I420 / NV12); tiles of a picture, luma and chroma
    uint32_t inv_ltx, inv_ctx;      // 0xffffffff / ltx, / ctx: a tile index is split without a division
    int32_t t_xl, t_yl, t_xc, t_yc; // where the tap tables begin in the call's table, in words (multiples of 4)
    int64_t pitch, frame_stride;    // bytes
    int32_t cy, yo, r_cv, g_cu, g_cv, b_cu;   // RGB formats
    float scale[3], bias[3];        // float dtypes
};

__device__ __forceinline__ uint32_t gbyte(const uint8_t *p) { return *(const AS1 uint8_t *)p; }
// a table word -> the two source coordinates and the fraction
__device__ __forceinline__ void tap_of(uint32_t e, int &i0, int &i1, uint32_t &f) { f = e & 255u; i0 = (int)(e >> 16); i1 = i0 + (int)((e >> 8) & 1u); }
// (a, b of the upper source row, c, d of the lower: every product and the sum stay below 2^24 + 2^15)
__device__ __forceinline__ int bilinear(const uint32_t (&s)[4], uint32_t fx, uint32_t fy)
{
    const uint32_t top = __umul24(s[0], 256u - fx) + __umul24(s[1], fx), bot = __umul24(s[2], 256u - fx) + __umul24(s[3], fx);
    return (int)((__umul24(top, 256u - fy) + __umul24(bot, fy) + 32768u) >> 16);
}
// tile index -> row and column of tiles (device_common.h's split_mb)
__device__ __forceinline__ void split_tile(int t, int per_row, uint32_t inv, int &ty, int &tx)
{
    int row = (int)__umulhi((unsigned)t, inv);
    if (t - row * per_row >= per_row) row++;
    ty = row; tx = t - row * per_row;
}

// the float step: two separately rounded operations, never one fused multiply-add - contraction is off for this function and the
// product is a value of its own (the empty asm).  Not hip's __fmul_rn / __fadd_rn: its header compiles them as contractible operators.
__device__ __forceinline__ float scale_bias(int c, float scale, float bias)
{
#pragma clang fp contract(off)
    float m = (float)c * scale;
    asm("" : "+v"(m));
    return m + bias;
}
__device__ __forceinline__ uint32_t half_bits(float e) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)e); }   // (round to nearest even, subnormals kept)

// NW words of a row piece to p: its first n_valid elements of ELEM bytes are inside the row.  A: bytes of a wide store
template <int NW, int A, int ELEM> __device__ __forceinline__ void put_elems(uint8_t *p, const uint32_t (&w)[NW], int n_valid)
{
    constexpr int NE = NW * 4 / ELEM;
    static_assert(NW % (A / 4) == 0, "a piece is whole wide stores");
    if (n_valid == NE && ((uintptr_t)p & (uintptr_t)(A - 1)) == 0) {
#pragma unroll
        for (int i = 0; i < NW; i += A / 4) {
            if constexpr (A == 16) nt_store4(p + i * 4, w[i], w[i + 1], w[i + 2], w[i + 3]);
            else if constexpr (A == 8) { const u32x2 v = { w[i], w[i + 1] }; __builtin_nontemporal_store(v, (AS1 u32x2 *)(p + i * 4)); }
            else __builtin_nontemporal_store(w[i], (AS1 uint32_t *)(p + i * 4));
        }
    } else {
#pragma unroll
        for (int k = 0; k < NE; k++) {
            if (k >= n_valid) continue;
            if constexpr (ELEM == 1) *(AS1 uint8_t *)(p + k) = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            else if constexpr (ELEM == 2) *(AS1 uint16_t *)(p + 2 * k) = (uint16_t)(w[k >> 1] >> (16 * (k & 1)));
            else *(AS1 uint32_t *)(p + 4 * k) = w[k];
        }
    }
}

// four samples of a channel (bytes of `packed`) as DT elements at p; n: how many of them the row holds
template <int DT> __device__ __forceinline__ void put_channel4(uint8_t *p, uint32_t packed, int n, float scale, float bias)
{
    if (DT == P264HIP_DTYPE_U8) {
        const uint32_t w[1] = { packed };
        put_elems<1, 4, 1>(p, w, n);
    } else {
        float e[4];
#pragma unroll
        for (int j = 0; j < 4; j++) e[j] = scale_bias((int)((packed >> (8 * j)) & 255u), scale, bias);
        if (DT == P264HIP_DTYPE_F16) {
            const uint32_t w[2] = { half_bits(e[0]) | half_bits(e[1]) << 16, half_bits(e[2]) | half_bits(e[3]) << 16 };
            put_elems<2, 8, 2>(p, w, n);
        } else {
            const uint32_t w[4] = { __float_as_uint(e[0]), __float_as_uint(e[1]), __float_as_uint(e[2]), __float_as_uint(e[3]) };
            put_elems<4, 16, 4>(p, w, n);
        }
    }
}

// four pixels R, G, B (bytes of the three words) interleaved as DT elements at p; n: how many PIXELS the row holds
template <int DT> __device__ __forceinline__ void put_rgb24(uint8_t *p, uint32_t R, uint32_t G, uint32_t B, int n, const ResizeParams &e)
{
    if (DT == P264HIP_DTYPE_U8) {
        uint32_t o[3] = { 0, 0, 0 };
#pragma unroll
        for (int k = 0; k < 4; k++) {
            o[(3 * k) >> 2]     |= ((R >> (8 * k)) & 255u) << (8 * ((3 * k) & 3));
            o[(3 * k + 1) >> 2] |= ((G >> (8 * k)) & 255u) << (8 * ((3 * k + 1) & 3));
            o[(3 * k + 2) >> 2] |= ((B >> (8 * k)) & 255u) << (8 * ((3 * k + 2) & 3));
        }
        put_elems<3, 4, 1>(p, o, 3 * n);
    } else {
        float f[12];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            f[3 * k]     = scale_bias((int)((R >> (8 * k)) & 255u), e.scale[0], e.bias[0]);
            f[3 * k + 1] = scale_bias((int)((G >> (8 * k)) & 255u), e.scale[1], e.bias[1]);
            f[3 * k + 2] = scale_bias((int)((B >> (8 * k)) & 255u), e.scale[2], e.bias[2]);
        }
        if (DT == P264HIP_DTYPE_F16) {
            uint32_t o[6];
#pragma unroll
            for (int i = 0; i < 6; i++) o[i] = half_bits(f[2 * i]) | half_bits(f[2 * i + 1]) << 16;
            put_elems<6, 8, 2>(p, o, 3 * n);
        } else {
            uint32_t o[12];
#pragma unroll
            for (int i = 0; i < 12; i++) o[i] = __float_as_uint(f[i]);
            put_elems<12, 16, 4>(p, o, 3 * n);
        }
    }
}

// four luma samples v of an output row (`row`: its first byte in plane 0) from column x on, n of them inside the row, with the two
// chroma pairs under them (cb, cr: less 128; RGB formats only) -> the elements of the format.  Shared with kernel_resize_aa.h.
template <int FMT, int DT>
__device__ __forceinline__ void put_luma4(uint8_t *row, int x, const int (&v)[4], const int (&cb)[2], const int (&cr)[2], int n, const ResizeParams &e)
{
    constexpr bool RGB = FMT == P264HIP_FMT_RGB24 || FMT == P264HIP_FMT_RGBP;
    constexpr int ELEM = DT == P264HIP_DTYPE_U8 ? 1 : DT == P264HIP_DTYPE_F16 ? 2 : 4;
    if (!RGB) {
        const uint32_t w[1] = { pack4(v[0], v[1], v[2], v[3]) };
        put_elems<1, 4, 1>(row + x, w, n);
    } else {
        int tr[4], tg[4], tb[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {       // (kernel_export.h's rgb_row: every sum of the pixel stays below 2^23)
            const int yy = __mul24(e.cy, v[j] - e.yo) + 4096;
            tr[j] = yy + __mul24(e.r_cv, cr[j >> 1]);
            tg[j] = yy + __mul24(e.g_cu, cb[j >> 1]) + __mul24(e.g_cv, cr[j >> 1]);
            tb[j] = yy + __mul24(e.b_cu, cb[j >> 1]);
        }
        const uint32_t R = round_pack4<13>(tr), G = round_pack4<13>(tg), B = round_pack4<13>(tb);
        if (FMT == P264HIP_FMT_RGBP) {
            const int64_t plane = e.pitch * e.h;
            put_channel4<DT>(row + x * ELEM, R, n, e.scale[0], e.bias[0]);
            put_channel4<DT>(row + plane + x * ELEM, G, n, e.scale[1], e.bias[1]);
            put_channel4<DT>(row + 2 * plane + x * ELEM, B, n, e.scale[2], e.bias[2]);
        } else {
            put_rgb24<DT>(row + 3 * x * ELEM, R, G, B, n, e);
        }
    }
}

// four chroma samples u, v of chroma row y from chroma column x on, n of them inside the row, behind the luma plane of picture `out`
// (I420 / NV12).  Shared with kernel_resize_aa.h.
template <int FMT>
__device__ __forceinline__ void put_chroma4(uint8_t *out, int y, int x, const int (&u)[4], const int (&v)[4], int n, const ResizeParams &e)
{
    uint8_t *planes = out + e.pitch * e.h;
    if (FMT == P264HIP_FMT_NV12) {
        const uint32_t w[2] = { pack4(u[0], v[0], u[1], v[1]), pack4(u[2], v[2], u[3], v[3]) };
        put_elems<2, 8, 1>(planes + (int64_t)y * e.pitch + 2 * x, w, 2 * n);
    } else {
        const int64_t cp = e.pitch >> 1;
        const uint32_t uw[1] = { pack4(u[0], u[1], u[2], u[3]) }, vw[1] = { pack4(v[0], v[1], v[2], v[3]) };
        uint8_t *row = planes + (int64_t)y * cp + x;
        put_elems<1, 4, 1>(row, uw, n);
        put_elems<1, 4, 1>(row + cp * (e.h >> 1), vw, n);
    }
}

template <int FMT, int DT>
__device__ __forceinline__ void resize_body(const uint8_t *frames, size_t frame_bytes, const Geom &g, const uint32_t *table, int pic_base, uint8_t *dst, const ResizeParams &e)
{
    constexpr bool RGB = FMT == P264HIP_FMT_RGB24 || FMT == P264HIP_FMT_RGBP;
    const int lane = threadIdx.x & 63;
    const int wt = rfl((int)(blockIdx.x * (RESIZE_THREADS / WAVE) + (threadIdx.x >> 6)));
    if (wt >= e.n_tiles) return;
    const int pic = pic_base + (int)blockIdx.y;
    const uint8_t *src = frames + (size_t)gload1(table + pic) * frame_bytes;
    uint8_t *out = dst + (int64_t)pic * e.frame_stride;
    if (wt < e.n_ltiles) {
        int ty, tx;
        split_tile(wt, e.ltx, e.inv_ltx, ty, tx);
        const int x = (tx * WAVE + lane) * RESIZE_PX, y = ty * 2;
        if (x >= e.w) return;
        const uint4 xq = gload4(table + e.t_xl + x);
        const uint32_t xt[4] = { xq.x, xq.y, xq.z, xq.w };
        uint32_t fx[4], fy[2], s[2][4][4];
        int r0[2], r1[2];
#pragma unroll
        for (int r = 0; r < 2; r++) { tap_of(gload1(table + e.t_yl + y + r), r0[r], r1[r], fy[r]); r0[r] *= 16; r1[r] *= 16; }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int x0, x1;
            tap_of(xt[j], x0, x1, fx[j]);
            const uint8_t *c0 = src + luma_off(g, x0, 0), *c1 = src + luma_off(g, x1, 0);
#pragma unroll
            for (int r = 0; r < 2; r++) { s[r][j][0] = gbyte(c0 + r0[r]); s[r][j][1] = gbyte(c1 + r0[r]); s[r][j][2] = gbyte(c0 + r1[r]); s[r][j][3] = gbyte(c1 + r1[r]); }
        }
        uint32_t cs[2][2][4], cfx[2] = { 0, 0 }, cfy = 0;          // [plane][sample][tap]
        if (RGB) {
            const uint2 cq = gload2(table + e.t_xc + (x >> 1));
            const uint32_t ct[2] = { cq.x, cq.y };
            int q0, q1;
            tap_of(gload1(table + e.t_yc + ty), q0, q1, cfy);
            q0 *= 16; q1 *= 16;
#pragma unroll
            for (int j = 0; j < 2; j++) {
                int x0, x1;
                tap_of(ct[j], x0, x1, cfx[j]);
                const uint8_t *c0 = src + chroma_off(g, 0, x0, 0), *c1 = src + chroma_off(g, 0, x1, 0);
#pragma unroll
                for (int p = 0; p < 2; p++) { cs[p][j][0] = gbyte(c0 + p * 8 + q0); cs[p][j][1] = gbyte(c1 + p * 8 + q0); cs[p][j][2] = gbyte(c0 + p * 8 + q1); cs[p][j][3] = gbyte(c1 + p * 8 + q1); }
            }
        }
        const int n = min(e.w - x, RESIZE_PX);
        int cb[2] = { 0, 0 }, cr[2] = { 0, 0 };
        if (RGB) {
#pragma unroll
            for (int j = 0; j < 2; j++) { cb[j] = bilinear(cs[0][j], cfx[j], cfy) - 128; cr[j] = bilinear(cs[1][j], cfx[j], cfy) - 128; }
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            int v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = bilinear(s[r][j], fx[j], fy[r]);
            put_luma4<FMT, DT>(out + (int64_t)(y + r) * e.pitch, x, v, cb, cr, n, e);
        }
    } else if (!RGB) {
        int y, tx;
        split_tile(wt - e.n_ltiles, e.ctx, e.inv_ctx, y, tx);
        const int x = (tx * WAVE + lane) * RESIZE_PX, cw = e.w >> 1;
        if (x >= cw) return;
        const uint4 xq = gload4(table + e.t_xc + x);
        const uint32_t xt[4] = { xq.x, xq.y, xq.z, xq.w };
        uint32_t fx[4], fy, s[2][4][4];
        int q0, q1;
        tap_of(gload1(table + e.t_yc + y), q0, q1, fy);
        q0 *= 16; q1 *= 16;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int x0, x1;
            tap_of(xt[j], x0, x1, fx[j]);
            const uint8_t *c0 = src + chroma_off(g, 0, x0, 0), *c1 = src + chroma_off(g, 0, x1, 0);
#pragma unroll
            for (int p = 0; p < 2; p++) { s[p][j][0] = gbyte(c0 + p * 8 + q0); s[p][j][1] = gbyte(c1 + p * 8 + q0); s[p][j][2] = gbyte(c0 + p * 8 + q1); s[p][j][3] = gbyte(c1 + p * 8 + q1); }
        }
        int u[4], v[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { u[j] = bilinear(s[0][j], fx[j], fy); v[j] = bilinear(s[1][j], fx[j], fy); }
        const int n = min(cw - x, RESIZE_PX);
        put_chroma4<FMT>(out, y, x, u, v, n, e);
    }
}

// The instances of a resizing export: X(family, suffix, format, dtype) for each (format, dtype) the description may name.  The four
// families - k_resize_*, k_resize_aa_*, k_roi_*, k_roi_aa_* - define their kernels from this list, one named kernel per instance
// (tools/kernel_resources.py and the tests find them by name: family ## suffix), and the host (p264hip.hip) builds its tables of
// kernel pointers and the index into them from it.
#define EXPORT_INSTANCES(X, family) \
    X(family, i420, P264HIP_FMT_I420, P264HIP_DTYPE_U8) \
    X(family, nv12, P264HIP_FMT_NV12, P264HIP_DTYPE_U8) \
    X(family, rgb24_u8, P264HIP_FMT_RGB24, P264HIP_DTYPE_U8) \
    X(family, rgb24_f16, P264HIP_FMT_RGB24, P264HIP_DTYPE_F16) \
    X(family, rgb24_f32, P264HIP_FMT_RGB24, P264HIP_DTYPE_F32) \
    X(family, rgbp_u8, P264HIP_FMT_RGBP, P264HIP_DTYPE_U8) \
    X(family, rgbp_f16, P264HIP_FMT_RGBP, P264HIP_DTYPE_F16) \
    X(family, rgbp_f32, P264HIP_FMT_RGBP, P264HIP_DTYPE_F32)

#define RESIZE_KERNEL(family, sfx, fmt, dt) \
    __global__ __launch_bounds__(RESIZE_THREADS) void family##sfx(const uint8_t *frames, size_t frame_bytes, Geom g, const uint32_t *table, int pic_base, uint8_t *dst, ResizeParams e) \
    { resize_body<fmt, dt>(frames, frame_bytes, g, table, pic_base, dst, e); }
EXPORT_INSTANCES(RESIZE_KERNEL, k_resize_)
