// kernel_resize_aa.h - kernel_resize.h's export with the ANTIALIASED bilinear filter of include/p264hip.h (P264HIP_FILTER_BILINEAR_AA):
// a triangle whose half-width grows with the reduction, Q15 weights, vertical pass first, one rounding per pass.  The layouts, the RGB
// sums, the float step and the stores are kernel_resize.h's (put_luma4 / put_chroma4 and what they call); only the resize is new.
//
// A workgroup (256 threads) owns a TILE of AA_TH = 16 output rows by TW output samples of the luma plane and the TW/2 x 8 chroma
// samples under it, U and V.  TW is 64, or the largest of 32, 16, 8 at which the tile's source columns fit the LDS (the host
// chooses it per call: reducing 1920 to 60 a tile of 32 samples spans 65 strips; up to the 32:1 limit 32 always fit).  Chroma first, then luma, each in two passes:
//   pass 1  a lane takes one output row and one 16-byte strip row of the tile's source column span: it runs the row's tap loop - one
//           16-byte load and sixteen multiply-adds (v_mad_u32_u24, sums below 2^23) per tap, consecutive rows of a strip are 16 bytes
//           apart - and writes sixteen 16-bit t to LDS.  t[row][16 * strip + i]: a chroma strip row is 8 t of U then 8 of V.
//   pass 2  a lane owns RESIZE_PX = 4 adjacent output samples of a row (chroma: of U and of V): for each it reads its run of t from
//           LDS and applies the column weights (14 x 16 bit products: __umul24, sums below 2^30).  Chroma lanes of I420 / NV12 store
//           their samples, those of the RGB formats leave them in LDS as bytes; luma lanes fetch the chroma of their two pairs
//           there and go through put_luma4.  A row's lanes store contiguous bytes, as in kernel_resize.h.
// The taps come from the call's table behind the frame indices: per axis (luma / chroma, x / y) one word first | count << 16 per
// destination index, first a coordinate of the FRAME, and the Q15 weights as 16-bit values with a row stride of the axis' largest
// count rounded up to even.  The kernel divides nothing: tasks are split with reciprocals from the host.
// LDS: the t of a tile (used by chroma and then by luma) are DYNAMIC, sized by the host for the call's widest tile - 18 KB reducing
// 1920 to 224, 7 KB to 640, at most AA_T_CAP 16-bit values = 40 KB -, beside 512 static bytes of chroma samples (RGB formats).
// Measured: allocating the 40 KB statically costs 17 % at 224 x 224 and 31 % at 640 x 360 (three workgroups a CU).
// Grid: (tiles of a picture, pictures); a workgroup never mixes pictures.
#pragma once
#include "kernel_resize.h"

#define AA_THREADS 256
#define AA_TH      16                       // output rows of a tile (luma; chroma: 8)
#define AA_TW      64                       // output samples of a tile's row, at most
#define AA_T_CAP   20480                    // 16-bit t of a tile at most: AA_TH rows x 80 luma strips, or 8 rows x 160 chroma strips

struct AaAxis {
    int32_t pos, wts, stride;               // where the axis' first | count words and its weights begin in the table (words), 16-bit weights per row
};
struct AaParams {
    ResizeParams r;                         // w, h, pitch, frame_stride, the RGB coefficients, scale and bias (the tile fields are not used)
    AaAxis xl, yl, xc, yc;
    int32_t tw_shift;                       // lanes of a luma row of a tile = 1 << tw_shift = TW / 4
    int32_t ntx;                            // tiles per tile row
    uint32_t inv_ntx;
    int32_t ns_l, ns_c;                     // strips of the widest tile span, luma and chroma: the LDS row stride is 16 times that
    uint32_t inv_ns_l, inv_ns_c;
};

__device__ __forceinline__ uint32_t gu16(const uint16_t *p) { return *(const AS1 uint16_t *)p; }

// pass 1 of a plane pair: rows output rows from y0 on, strips strip0 .. strip0 + ns - 1 (of strip_bytes each, from `plane`)
__device__ __forceinline__ void aa_pass1(const uint8_t *plane, uint32_t strip_bytes, const uint32_t *table, const AaAxis &ay, int y0, int rows, int strip0, int ns,
                                         int ns_max, uint32_t inv_ns, uint16_t *t)
{
    const int n_tasks = rows * ns_max;
    for (int i = (int)threadIdx.x; i < n_tasks; i += AA_THREADS) {
        int row, s;
        split_tile(i, ns_max, inv_ns, row, s);
        if (s >= ns) continue;
        const uint32_t pw = gload1(table + ay.pos + y0 + row);
        const int first = (int)(pw & 0xffffu), count = (int)(pw >> 16);
        const uint8_t *p = plane + strip_mul(strip0 + s, strip_bytes) + first * 16;
        const uint16_t *w = (const uint16_t *)(table + ay.wts) + (y0 + row) * ay.stride;
        uint32_t acc[16];
#pragma unroll
        for (int j = 0; j < 16; j++) acc[j] = 256u;
        for (int k = 0; k < count; k++) {
            const uint32_t wk = gu16(w + k);
            const uint4 q = gload4(p + k * 16);
            const uint32_t d[4] = { q.x, q.y, q.z, q.w };
#pragma unroll
            for (int j = 0; j < 16; j++) acc[j] += __umul24((d[j >> 2] >> (8 * (j & 3))) & 255u, wk);
        }
        uint32_t o[8];
#pragma unroll
        for (int j = 0; j < 8; j++) o[j] = (acc[2 * j] >> 9) | (acc[2 * j + 1] >> 9) << 16;
        uint4 *dst = (uint4 *)(t + row * (ns_max * 16) + s * 16);
        dst[0] = make_uint4(o[0], o[1], o[2], o[3]);
        dst[1] = make_uint4(o[4], o[5], o[6], o[7]);
    }
}

// the span of source strips of output columns x0 .. x1 - 1 of an axis (sh: log2 of a strip's samples), clipped to the LDS row
__device__ __forceinline__ void aa_span(const uint32_t *table, const AaAxis &ax, int x0, int x1, int sh, int ns_max, int &strip0, int &ns)
{
    const uint32_t a = gload1(table + ax.pos + x0), b = gload1(table + ax.pos + x1 - 1);
    strip0 = (int)(a & 0xffffu) >> sh;
    ns = min((((int)(b & 0xffffu) + (int)(b >> 16) - 1) >> sh) - strip0 + 1, ns_max);
}

// pass 2, one sample: the column weights of destination index xx of the axis over a row of t whose first strip is strip0
__device__ __forceinline__ int aa_col_luma(const uint32_t *table, const AaAxis &ax, int xx, int strip0, const uint16_t *trow)
{
    const uint32_t pw = gload1(table + ax.pos + xx);
    const int first = (int)(pw & 0xffffu) - strip0 * 16, count = (int)(pw >> 16);
    const uint16_t *w = (const uint16_t *)(table + ax.wts) + xx * ax.stride;
    uint32_t sum = 1u << 20;
    for (int k = 0; k < count; k++) sum += __umul24(gu16(w + k), (uint32_t)trow[first + k]);
    return (int)(sum >> 21);
}
// the same for a chroma sample, U and V: a strip row of t is 8 of U, then 8 of V
__device__ __forceinline__ void aa_col_chroma(const uint32_t *table, const AaAxis &ax, int xx, int strip0, const uint16_t *trow, int &u, int &v)
{
    const uint32_t pw = gload1(table + ax.pos + xx);
    const int first = (int)(pw & 0xffffu) - strip0 * 8, count = (int)(pw >> 16);
    const uint16_t *w = (const uint16_t *)(table + ax.wts) + xx * ax.stride;
    uint32_t su = 1u << 20, sv = 1u << 20;
    for (int k = 0; k < count; k++) {
        const int c = first + k, at = ((c >> 3) << 4) + (c & 7);
        const uint32_t wk = gu16(w + k);
        su += __umul24(wk, (uint32_t)trow[at]); sv += __umul24(wk, (uint32_t)trow[at + 8]);
    }
    u = (int)(su >> 21); v = (int)(sv >> 21);
}
// the chroma of a luma lane's two pairs out of the tile's resized chroma (RGB formats): lane q of luma row `row`
__device__ __forceinline__ void aa_lane_chroma(const uint32_t (&cs)[2][AA_TH / 2][AA_TW / 8], int row, int q, int (&cb)[2], int (&cr)[2])
{
    const uint32_t uw = cs[0][row >> 1][q >> 1] >> (16 * (q & 1)), vw = cs[1][row >> 1][q >> 1] >> (16 * (q & 1));
    cb[0] = (int)(uw & 255u) - 128; cb[1] = (int)((uw >> 8) & 255u) - 128;
    cr[0] = (int)(vw & 255u) - 128; cr[1] = (int)((vw >> 8) & 255u) - 128;
}

template <int FMT, int DT>
__device__ __forceinline__ void resize_aa_body(const uint8_t *frames, size_t frame_bytes, const Geom &g, const uint32_t *table, int pic_base, uint8_t *dst, const AaParams &e)
{
    constexpr bool RGB = FMT == P264HIP_FMT_RGB24 || FMT == P264HIP_FMT_RGBP;
    extern __shared__ __attribute__((aligned(16))) uint16_t t[];     // the call's largest tile: 16 * max(AA_TH * ns_l, AA_TH / 2 * ns_c)
    __shared__ uint32_t cs[2][AA_TH / 2][AA_TW / 8];        // the tile's resized chroma, four bytes a word (RGB formats)
    const int tid = (int)threadIdx.x;
    const int pic = pic_base + (int)blockIdx.y;
    const uint8_t *src = frames + (size_t)gload1(table + pic) * frame_bytes;
    uint8_t *out = dst + (int64_t)pic * e.r.frame_stride;
    int ty, tx;
    split_tile((int)blockIdx.x, e.ntx, e.inv_ntx, ty, tx);
    const int W = e.r.w, H = e.r.h, cw = W >> 1;
    const int x0 = tx << (e.tw_shift + 2), x1 = min(x0 + (4 << e.tw_shift), W), y0 = ty * AA_TH, rows = min(AA_TH, H - y0);
    const int cx0 = x0 >> 1, cx1 = x1 >> 1, cy0 = y0 >> 1, crows = rows >> 1;
    // ---- chroma
    {
        int strip0, ns;
        aa_span(table, e.xc, cx0, cx1, 3, e.ns_c, strip0, ns);
        aa_pass1(src + g.coff, g.cstrip, table, e.yc, cy0, crows, strip0, ns, e.ns_c, e.inv_ns_c, t);
        __syncthreads();
        const int lanes = e.tw_shift - 1, row = tid >> lanes, q = tid & ((1 << lanes) - 1), x = cx0 + q * RESIZE_PX;
        if (row < crows && x < cx1) {
            const uint16_t *trow = t + row * (e.ns_c * 16);
            int u[4], v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) aa_col_chroma(table, e.xc, min(x + j, cw - 1), strip0, trow, u[j], v[j]);
            if (RGB) { cs[0][row][q] = pack4(u[0], u[1], u[2], u[3]); cs[1][row][q] = pack4(v[0], v[1], v[2], v[3]); }
            else put_chroma4<FMT>(out, cy0 + row, x, u, v, min(cw - x, RESIZE_PX), e.r);
        }
        __syncthreads();
    }
    // ---- luma
    {
        int strip0, ns;
        aa_span(table, e.xl, x0, x1, 4, e.ns_l, strip0, ns);
        aa_pass1(src, g.ystrip, table, e.yl, y0, rows, strip0, ns, e.ns_l, e.inv_ns_l, t);
        __syncthreads();
        const int row = tid >> e.tw_shift, q = tid & ((1 << e.tw_shift) - 1), x = x0 + q * RESIZE_PX;
        if (row < rows && x < x1) {
            const uint16_t *trow = t + row * (e.ns_l * 16);
            int v[4], cb[2] = { 0, 0 }, cr[2] = { 0, 0 };
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = aa_col_luma(table, e.xl, min(x + j, W - 1), strip0, trow);
            if (RGB) aa_lane_chroma(cs, row, q, cb, cr);
            put_luma4<FMT, DT>(out + (int64_t)(y0 + row) * e.r.pitch, x, v, cb, cr, min(W - x, RESIZE_PX), e.r);
        }
    }
}

// (a named kernel per instance of kernel_resize.h's EXPORT_INSTANCES)
#define RESIZE_AA_KERNEL(family, sfx, fmt, dt) \
    __global__ __launch_bounds__(AA_THREADS) void family##sfx(const uint8_t *frames, size_t frame_bytes, Geom g, const uint32_t *table, int pic_base, uint8_t *dst, AaParams e) \
    { resize_aa_body<fmt, dt>(frames, frame_bytes, g, table, pic_base, dst, e); }
EXPORT_INSTANCES(RESIZE_AA_KERNEL, k_resize_aa_)
