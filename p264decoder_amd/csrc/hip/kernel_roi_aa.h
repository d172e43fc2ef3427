// kernel_roi_aa.h - kernel_roi.h's export with the ANTIALIASED filter (include/p264hip.h: p264hip_export_rois_aa): a source window PER
// PICTURE, each resized by kernel_resize_aa.h's two passes into a rectangle of the output and a constant round it.  Two kernels a call:
//
// k_roi_aa_taps  one thread per (ROI, axis, destination index), on k_roi_taps' grid: it writes the word first | count << 16 and the
//                row of Q15 weights into the ROI's SEGMENT of the context's scratch.  The text is include/p264hip_aa.h's
//                p264hip_roi_aa_entry, which the host compiles as p264hip_roi_aa_segment: 64-bit integers, a division per tap.
// k_roi_aa_*     resize_aa_body's shape: a workgroup of 256 threads owns a tile of AA_TH = 16 rows by TW samples of the OUTPUT,
//                chroma first and then luma, pass 1 (aa_pass1) from the strips to 16-bit t in dynamic LDS, pass 2 (aa_col_luma /
//                aa_col_chroma) from there; stores through put_luma4 / put_chroma4.  What is new:
//   clipping     the tile is clipped to the ROI's rectangle - rectangles are even, so luma pairs and their chroma sample are inside
//                or outside together.  Pass 1 runs over the clipped rows and the strips of the clipped columns only, table indices
//                are relative to the rectangle, and a sample outside gets the fill and reads nothing: a tile wholly outside loads
//                no frame byte and no table word.  Whether the tile meets the rectangle is workgroup-uniform; whether a sample is
//                inside is decided per lane behind the barriers, which all 256 threads reach.
//   TW per ROI   the host puts log2(TW / 4) and the strips of a tile row in LDS into RoiDev.pad[0] (tw_shift | ns_l << 8 | ns_c << 16:
//                p264hip_aa.h's p264hip_roi_aa_tile, a closed-form bound of the span) and the four weight strides into pad[1], a byte
//                each.  The grid is the call's largest tile count and the dynamic LDS its largest need; a workgroup whose index is
//                beyond its ROI's tiles returns before the first barrier (workgroup-uniform).  One 32:1 ROI does not force
//                8-sample tiles on its neighbours.
// The host check (p264hip_rois_aa_check) is what guarantees that every coordinate k_roi_aa_taps writes lies in the frame; the
// kernels clamp nothing.  Two 32-bit divisions a workgroup (the reciprocals of its two LDS row lengths); a tile index is split with
// the host's reciprocal of its ROI's tile width.
// Grid: k_roi_aa_taps (entries of the largest segment / 256, ROIs); k_roi_aa_* (most tiles of an ROI, ROIs).
#pragma once
#include "kernel_resize_aa.h"
#include "kernel_roi.h"
#include "p264hip_aa.h"

static_assert(AA_T_CAP == P264HIP_ROI_AA_TILE_VALUES, "the header names the LDS bound of a tile");

struct RoiAaParams {
    ResizeParams r;                         // w, h, pitch, frame_stride, the RGB coefficients, scale and bias (the tile fields are not used)
    int32_t tile_rows;                      // rows of tiles of the output
    uint32_t inv_ntx[4];                    // 0xffffffff / tiles per tile row, for tw_shift 1 .. 4
};

__global__ __launch_bounds__(ROI_TAPS_THREADS) void k_roi_aa_taps(const RoiDev *rois, int roi_base, uint32_t *scratch)
{
    const RoiDev *o = rois + roi_base + (int)blockIdx.y;
    const uint4 q = gload4(o);
    if (q.x == ROI_SKIP) return;
    const uint2 s = gload2(&o->sx);
    (void)p264hip_roi_aa_entry(scratch + q.y, (int)(s.x & 0xffffu), (int)(s.y & 0xffffu), (int)(s.x >> 16), (int)(s.y >> 16), (int)(q.z >> 16), (int)(q.w >> 16),
                         (int)(blockIdx.x * ROI_TAPS_THREADS + threadIdx.x));
}

// an axis of a segment that begins at word `at`; returns the word behind it
__device__ __forceinline__ int roi_aa_axis(AaAxis &ax, int at, int D, int stride)
{
    ax.pos = at; ax.wts = at + roi_pad4(D); ax.stride = stride;
    return ax.wts + roi_pad4(D * (stride >> 1));
}

template <int FMT, int DT>
__device__ __forceinline__ void roi_aa_body(const uint8_t *frames, size_t frame_bytes, const Geom &g, const RoiDev *rois, const uint32_t *scratch, int pic_base,
                                            uint8_t *dst, const RoiAaParams &e, uint32_t fill)
{
    constexpr bool RGB = FMT == P264HIP_FMT_RGB24 || FMT == P264HIP_FMT_RGBP;
    extern __shared__ __attribute__((aligned(16))) uint16_t t[];     // the call's largest tile: 16 * max(AA_TH * ns_l, AA_TH / 2 * ns_c)
    __shared__ uint32_t cs[2][AA_TH / 2][AA_TW / 8];        // the tile's chroma, resized or the fill, four bytes a word (RGB formats)
    const int tid = (int)threadIdx.x;
    const int pic = pic_base + (int)blockIdx.y;
    const RoiDev *o = rois + pic;
    const uint4 q = gload4(o);
    if (q.x == ROI_SKIP) return;                            // (workgroup-uniform, before the first barrier: a device list's invalid ROI)
    const uint2 cfg = gload2(&o->pad[0]);
    const int tw_shift = rfl((int)(cfg.x & 255u)), ns_l = rfl((int)((cfg.x >> 8) & 255u)), ns_c = rfl((int)((cfg.x >> 16) & 255u));
    const int W = e.r.w, H = e.r.h, cw = W >> 1;
    const int ntx = (W + (4 << tw_shift) - 1) >> (tw_shift + 2);
    if ((int)blockIdx.x >= ntx * e.tile_rows) return;       // (workgroup-uniform, before the first barrier: this ROI has fewer tiles than the widest)
    const uint32_t inv_ntx = tw_shift == 4 ? e.inv_ntx[3] : tw_shift == 3 ? e.inv_ntx[2] : tw_shift == 2 ? e.inv_ntx[1] : e.inv_ntx[0];
    int ty, tx;
    split_tile((int)blockIdx.x, ntx, inv_ntx, ty, tx);
    const uint8_t *src = frames + (size_t)q.x * frame_bytes;
    const uint32_t *seg = scratch + q.y;
    uint8_t *out = dst + (int64_t)pic * e.r.frame_stride;
    const int dl = rfl((int)(q.z & 0xffffu)), dw = rfl((int)(q.z >> 16)), dt = rfl((int)(q.w & 0xffffu)), dh = rfl((int)(q.w >> 16));
    const int x0 = tx << (tw_shift + 2), x1 = min(x0 + (4 << tw_shift), W), y0 = ty * AA_TH, rows = min(AA_TH, H - y0);
    // the tile clipped to the rectangle: columns ix0 .. ix1 - 1, rows iy0 .. iy1 - 1, all even
    const int ix0 = max(x0, dl), ix1 = min(x1, dl + dw), iy0 = max(y0, dt), iy1 = min(y0 + rows, dt + dh);
    const bool meets = ix0 < ix1 && iy0 < iy1;              // (workgroup-uniform)
    const int cx0 = x0 >> 1, cx1 = x1 >> 1, cy0 = y0 >> 1, crows = rows >> 1;
    const int fill_y = (int)(fill & 255u), fill_cb = (int)((fill >> 8) & 255u), fill_cr = (int)((fill >> 16) & 255u);
    AaAxis xl, yl, xc, yc;
    int at = roi_aa_axis(xl, 0, dw, (int)(cfg.y & 255u));
    at = roi_aa_axis(yl, at, dh, (int)((cfg.y >> 8) & 255u));
    at = roi_aa_axis(xc, at, dw >> 1, (int)((cfg.y >> 16) & 255u));
    (void)roi_aa_axis(yc, at, dh >> 1, (int)(cfg.y >> 24));
    // ---- chroma
    {
        int strip0 = 0, ns = 0;
        if (meets) {
            aa_span(seg, xc, (ix0 - dl) >> 1, (ix1 - dl) >> 1, 3, ns_c, strip0, ns);
            aa_pass1(src + g.coff, g.cstrip, seg, yc, (iy0 - dt) >> 1, (iy1 - iy0) >> 1, strip0, ns, ns_c, 0xffffffffu / (uint32_t)ns_c, t);
        }
        __syncthreads();
        const int lanes = tw_shift - 1, row = tid >> lanes, ql = tid & ((1 << lanes) - 1), x = cx0 + ql * RESIZE_PX;
        if (row < crows && x < cx1) {
            const int y = cy0 + row;
            const bool row_in = meets && y >= (iy0 >> 1) && y < (iy1 >> 1);
            const uint16_t *trow = t + (y - (iy0 >> 1)) * (ns_c * 16);       // (not read where the row is outside)
            int u[4], v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                u[j] = fill_cb; v[j] = fill_cr;
                if (row_in && x + j >= (ix0 >> 1) && x + j < (ix1 >> 1)) aa_col_chroma(seg, xc, x + j - (dl >> 1), strip0, trow, u[j], v[j]);
            }
            if (RGB) { cs[0][row][ql] = pack4(u[0], u[1], u[2], u[3]); cs[1][row][ql] = pack4(v[0], v[1], v[2], v[3]); }
            else put_chroma4<FMT>(out, y, x, u, v, min(cw - x, RESIZE_PX), e.r);
        }
        __syncthreads();
    }
    // ---- luma
    {
        int strip0 = 0, ns = 0;
        if (meets) {
            aa_span(seg, xl, ix0 - dl, ix1 - dl, 4, ns_l, strip0, ns);
            aa_pass1(src, g.ystrip, seg, yl, iy0 - dt, iy1 - iy0, strip0, ns, ns_l, 0xffffffffu / (uint32_t)ns_l, t);
        }
        __syncthreads();
        const int row = tid >> tw_shift, ql = tid & ((1 << tw_shift) - 1), x = x0 + ql * RESIZE_PX;
        if (row < rows && x < x1) {
            const int y = y0 + row;
            const bool row_in = meets && y >= iy0 && y < iy1;
            const uint16_t *trow = t + (y - iy0) * (ns_l * 16);
            int v[4], cb[2] = { 0, 0 }, cr[2] = { 0, 0 };
#pragma unroll
            for (int j = 0; j < 4; j++) {
                v[j] = fill_y;
                if (row_in && x + j >= ix0 && x + j < ix1) v[j] = aa_col_luma(seg, xl, x + j - dl, strip0, trow);
            }
            if (RGB) aa_lane_chroma(cs, row, ql, cb, cr);
            put_luma4<FMT, DT>(out + (int64_t)y * e.r.pitch, x, v, cb, cr, min(W - x, RESIZE_PX), e.r);
        }
    }
}

// (a named kernel per instance of kernel_resize.h's EXPORT_INSTANCES)
#define ROI_AA_KERNEL(family, sfx, fmt, dt) \
    __global__ __launch_bounds__(AA_THREADS) void family##sfx(const uint8_t *frames, size_t frame_bytes, Geom g, const RoiDev *rois, const uint32_t *scratch, int pic_base, uint8_t *dst, RoiAaParams e, uint32_t fill) \
    { roi_aa_body<fmt, dt>(frames, frame_bytes, g, rois, scratch, pic_base, dst, e, fill); }
EXPORT_INSTANCES(ROI_AA_KERNEL, k_roi_aa_)
