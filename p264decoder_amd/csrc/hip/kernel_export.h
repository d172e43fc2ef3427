// kernel_export.h - a batch of decoded pictures out of the frame stores into the caller's device memory: cropped to a window,
// as I420 / NV12 / RGB24 / planar RGB (include/p264hip.h: p264hip_export_t has the layouts and the RGB arithmetic).
//
// The kernels move bytes and are bound by them.  The source is the strip layout (device_common.h): a luma strip row is 16
// bytes, eight rows of a strip are one 128-byte line; a chroma row is 8 bytes of U and 8 of V.  A wavefront takes a TILE of
// 8 strips x 32 rows: lane l holds row (l & 7) of strip (l >> 3) in each of the tile's four 8-row groups, 16 bytes per lane and
// group.  Eight neighbouring lanes load one whole 128-byte line; the eight lanes of one row store 128 contiguous bytes of a
// destination row (384 for RGB24).  The four loads of a lane are issued before its first store.  No LDS: the transposition
// is in the lane mapping.
//   luma tiles      every format; the RGB formats load the chroma row (y >> 1) of the same strip beside each luma row
//   chroma tiles    NV12: the same tile shape over chroma rows, U and V interleaved with two v_perm per dword;
//                   I420: a lane takes the rows of a strip PAIR, so that it has 16 bytes of U and 16 of V to store
// A lane whose 16 (48) bytes lie wholly inside the window and whose destination is 16-byte aligned - every lane of an export
// with crop_left % 16 == 0, a width that is a multiple of 16 and dst, pitch and frame_stride 16-byte aligned (I420's chroma: a
// multiple of 32) - stores 16 bytes at a time; any other lane stores the bytes of its row piece that the window holds one by
// one: correct for every even window, any pitch and any alignment, at the speed of byte stores.
// The 16-byte stores are non-temporal, as k_mc's are: the pictures leave for another consumer, while the frame stores
// they are read from stay the references of the next pictures.
// Grid: (tiles of a picture / 4, pictures); a wavefront never mixes pictures.
#pragma once
#include "device_common.h"
#include "lane_ops.h"

#define EXPORT_THREADS 256
#define EXPORT_GROUPS  4            // 8-row groups of a tile

struct ExportParams {
    int32_t x0, y0, w, h;           // the window
    int32_t s0, n_cols;             // luma tiles: the first strip the window touches, and how many it touches
    int32_t c0, n_ccols;            // chroma tiles: the same in strips (NV12) or in strip pairs (I420); 0 columns for RGB
    int32_t g0, n_groups;           // first 8-row group of luma rows the window touches, and how many
    int32_t cg0, n_cgroups;         // the same of chroma rows
    int32_t ltx, n_ltiles;          // luma tiles: per tile row, per picture
    int32_t ctx, n_tiles;           // chroma tiles per tile row; tiles of a picture, luma and chroma
    int64_t pitch, frame_stride;    // bytes
    int32_t cy, yo, r_cv, g_cu, g_cv, b_cu;   // RGB formats
};

// (cy, R.cv, G.cu, G.cv, B.cu) by [matrix][full_range]: include/p264hip.h derives them
static const int32_t export_coefs[2][2][5] = {
    { { 9539, 13075, -3209, -6660, 16525 }, { 8192, 11485, -2819, -5850, 14516 } },
    { { 9539, 14686, -1747, -4366, 17305 }, { 8192, 12901, -1535, -3835, 15201 } } };

__device__ __forceinline__ void nt_store4(uint8_t *p, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const u32x4 v = { a, b, c, d };
    __builtin_nontemporal_store(v, (AS1 u32x4 *)p);
}

// NW dwords of a row piece to p: bytes [b0, b1) of them are inside the window (p itself may lie in front of it)
template <int NW> __device__ __forceinline__ void put_piece(uint8_t *p, const uint32_t (&w)[NW], int b0, int b1)
{
    if (b0 == 0 && b1 == NW * 4 && ((uintptr_t)p & 15) == 0) {
#pragma unroll
        for (int i = 0; i < NW; i += 4) nt_store4(p + i * 4, w[i], w[i + 1], w[i + 2], w[i + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < NW * 4; k++)
            if (k >= b0 && k < b1) *(AS1 uint8_t *)(p + k) = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    }
}

// sixteen pixels of a luma strip row with the chroma row under them -> R, G, B, four pixels per dword.  The clip of (sum >> 13) to
// a byte is lane_ops.h's round_pack4 (v_ashr_pk_u8_i32, two values per instruction, only its defined low half used): written as
// clip255(v >> 13) << 8k the compiler picks that instruction itself and ORs the other bytes onto its undefined upper half.
__device__ __forceinline__ void rgb_row(const uint4 yv, const uint4 cv, const ExportParams &e, uint32_t (&R)[4], uint32_t (&G)[4], uint32_t (&B)[4])
{
    const uint32_t yw[4] = { yv.x, yv.y, yv.z, yv.w }, uw[2] = { cv.x, cv.y }, vw[2] = { cv.z, cv.w };
    int rv = 0, gg = 0, bu = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int tr[4], tg[4], tb[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = 4 * i + j;
            if (!(k & 1)) {         // (every sum of the pixel stays below 2^23: the 24-bit multiplies are exact)
                const int cb = (int)((uw[k >> 3] >> (8 * ((k >> 1) & 3))) & 255u) - 128, cr = (int)((vw[k >> 3] >> (8 * ((k >> 1) & 3))) & 255u) - 128;
                rv = __mul24(e.r_cv, cr); gg = __mul24(e.g_cu, cb) + __mul24(e.g_cv, cr); bu = __mul24(e.b_cu, cb);
            }
            const int yy = __mul24(e.cy, (int)((yw[i] >> (8 * j)) & 255u) - e.yo) + 4096;
            tr[j] = yy + rv; tg[j] = yy + gg; tb[j] = yy + bu;
        }
        R[i] = round_pack4<13>(tr); G[i] = round_pack4<13>(tg); B[i] = round_pack4<13>(tb);
    }
}

template <int FMT>
__device__ __forceinline__ void export_body(const uint8_t *frames, size_t frame_bytes, const Geom &g, const uint32_t *table, int pic_base, uint8_t *dst, const ExportParams &e)
{
    const int lane = threadIdx.x & 63;
    const int wt = rfl((int)(blockIdx.x * (EXPORT_THREADS / WAVE) + (threadIdx.x >> 6)));
    if (wt >= e.n_tiles) return;
    const int pic = pic_base + (int)blockIdx.y;
    const uint8_t *src = frames + (size_t)gload1(table + pic) * frame_bytes;
    uint8_t *out = dst + (int64_t)pic * e.frame_stride;
    const int r = lane & 7, col = lane >> 3;
    if (wt < e.n_ltiles) {
        const int ty = wt / e.ltx, tx = wt - ty * e.ltx;
        const int c = tx * 8 + col, s = e.s0 + c;
        const int b0 = max(e.x0 - s * 16, 0), b1 = min(e.x0 + e.w - s * 16, 16);
        const int64_t dx = (int64_t)s * 16 - e.x0;          // where byte 0 of the strip row lies in the destination row
        const uint8_t *ls = src + strip_mul(s, g.ystrip);
        const uint8_t *cs = src + g.coff + strip_mul(s, g.cstrip);
        uint4 yv[EXPORT_GROUPS], cv[EXPORT_GROUPS];
        bool ok[EXPORT_GROUPS];
#pragma unroll
        for (int j = 0; j < EXPORT_GROUPS; j++) {
            const int grp = ty * EXPORT_GROUPS + j, y = (e.g0 + grp) * 8 + r;
            ok[j] = c < e.n_cols && grp < e.n_groups && y >= e.y0 && y < e.y0 + e.h;
            yv[j] = make_uint4(0, 0, 0, 0); cv[j] = make_uint4(0, 0, 0, 0);
            if (ok[j]) {
                yv[j] = gload4(ls + y * 16);
                if (FMT == P264HIP_FMT_RGB24 || FMT == P264HIP_FMT_RGBP) cv[j] = gload4(cs + (y >> 1) * 16);
            }
        }
#pragma unroll
        for (int j = 0; j < EXPORT_GROUPS; j++) {
            if (!ok[j]) continue;
            const int y = (e.g0 + ty * EXPORT_GROUPS + j) * 8 + r;
            uint8_t *row = out + (int64_t)(y - e.y0) * e.pitch;
            if (FMT == P264HIP_FMT_I420 || FMT == P264HIP_FMT_NV12) {
                const uint32_t w[4] = { yv[j].x, yv[j].y, yv[j].z, yv[j].w };
                put_piece<4>(row + dx, w, b0, b1);
            } else {
                uint32_t R[4], G[4], B[4];
                rgb_row(yv[j], cv[j], e, R, G, B);
                if (FMT == P264HIP_FMT_RGBP) {
                    const int64_t plane = e.pitch * e.h;
                    put_piece<4>(row + dx, R, b0, b1);
                    put_piece<4>(row + plane + dx, G, b0, b1);
                    put_piece<4>(row + 2 * plane + dx, B, b0, b1);
                } else {
                    uint32_t w[12];
#pragma unroll
                    for (int i = 0; i < 12; i++) w[i] = 0;
#pragma unroll
                    for (int k = 0; k < 16; k++) {
                        w[(3 * k) >> 2]     |= ((R[k >> 2] >> (8 * (k & 3))) & 255u) << (8 * ((3 * k) & 3));
                        w[(3 * k + 1) >> 2] |= ((G[k >> 2] >> (8 * (k & 3))) & 255u) << (8 * ((3 * k + 1) & 3));
                        w[(3 * k + 2) >> 2] |= ((B[k >> 2] >> (8 * (k & 3))) & 255u) << (8 * ((3 * k + 2) & 3));
                    }
                    put_piece<12>(row + 3 * dx, w, 3 * b0, 3 * b1);
                }
            }
        }
    } else if (FMT == P264HIP_FMT_I420 || FMT == P264HIP_FMT_NV12) {
        const int ct = wt - e.n_ltiles, ty = ct / e.ctx, tx = ct - ty * e.ctx;
        const int c = tx * 8 + col, u = e.c0 + c;            // a strip (NV12) or a pair of strips (I420)
        const int cy0 = e.y0 >> 1, ch = e.h >> 1;
        // NV12: bytes of the strip's interleaved row; I420: samples of the pair's 16
        const int left = FMT == P264HIP_FMT_NV12 ? e.x0 : e.x0 >> 1, wide = FMT == P264HIP_FMT_NV12 ? e.w : e.w >> 1;
        const int b0 = max(left - u * 16, 0), b1 = min(left + wide - u * 16, 16);
        const int64_t dx = (int64_t)u * 16 - left;
        const int sa = FMT == P264HIP_FMT_NV12 ? u : 2 * u;
        const bool second = FMT == P264HIP_FMT_I420 && sa + 1 < g.mb_w;        // (an odd frame's last pair has one strip; the window ends in it)
        const uint8_t *ca = src + g.coff + strip_mul(sa, g.cstrip);
        uint4 av[EXPORT_GROUPS], bv[EXPORT_GROUPS];
        bool ok[EXPORT_GROUPS];
#pragma unroll
        for (int j = 0; j < EXPORT_GROUPS; j++) {
            const int grp = ty * EXPORT_GROUPS + j, y = (e.cg0 + grp) * 8 + r;
            ok[j] = c < e.n_ccols && grp < e.n_cgroups && y >= cy0 && y < cy0 + ch;
            av[j] = make_uint4(0, 0, 0, 0); bv[j] = make_uint4(0, 0, 0, 0);
            if (ok[j]) {
                av[j] = gload4(ca + y * 16);
                if (second) bv[j] = gload4(ca + g.cstrip + y * 16);
            }
        }
#pragma unroll
        for (int j = 0; j < EXPORT_GROUPS; j++) {
            if (!ok[j]) continue;
            const int y = (e.cg0 + ty * EXPORT_GROUPS + j) * 8 + r;
            uint8_t *planes = out + e.pitch * e.h;
            if (FMT == P264HIP_FMT_NV12) {
                const uint32_t w[4] = { perm(av[j].z, av[j].x, 0x05010400u), perm(av[j].z, av[j].x, 0x07030602u),
                                        perm(av[j].w, av[j].y, 0x05010400u), perm(av[j].w, av[j].y, 0x07030602u) };
                put_piece<4>(planes + (int64_t)(y - cy0) * e.pitch + dx, w, b0, b1);
            } else {
                const int64_t cp = e.pitch >> 1;
                const uint32_t uw[4] = { av[j].x, av[j].y, bv[j].x, bv[j].y }, vw[4] = { av[j].z, av[j].w, bv[j].z, bv[j].w };
                uint8_t *row = planes + (int64_t)(y - cy0) * cp + dx;
                put_piece<4>(row, uw, b0, b1);
                put_piece<4>(row + cp * ch, vw, b0, b1);
            }
        }
    }
}

// (one named kernel per format: tools/kernel_resources.py and the tests find them by name)
#define EXPORT_KERNEL(name, fmt) \
    __global__ __launch_bounds__(EXPORT_THREADS) void name(const uint8_t *frames, size_t frame_bytes, Geom g, const uint32_t *table, int pic_base, uint8_t *dst, ExportParams e) \
    { export_body<fmt>(frames, frame_bytes, g, table, pic_base, dst, e); }
EXPORT_KERNEL(k_export_i420, P264HIP_FMT_I420)
EXPORT_KERNEL(k_export_nv12, P264HIP_FMT_NV12)
EXPORT_KERNEL(k_export_rgb24, P264HIP_FMT_RGB24)
EXPORT_KERNEL(k_export_rgbp, P264HIP_FMT_RGBP)
