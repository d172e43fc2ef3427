// kernel_roi.h - kernel_resize.h's export with a source window PER PICTURE, each resized by the same fixed-point bilinear filter
// into a rectangle of the output and a constant round it (include/p264hip.h: p264hip_roi_t has the contract).  Two kernels a call:
//
// k_roi_taps   the tap tables, made on the device: one thread per (ROI, axis, destination index) writes the word kernel_resize.h
//              reads (tap_of: fraction | (i1 - i0) << 8 | i0 << 16, i0 a coordinate of the FRAME) into the ROI's SEGMENT of the
//              context's scratch.  A segment is four tables over the RECTANGLE's sizes - x luma, y luma, x chroma, y chroma -, each
//              padded to a multiple of 4 words with its last word, as the host's resize_table pads.  The position is
//              p264hip_pos.h's, the text p264hip_resize_taps compiles; its division is a 32-bit one wherever the dividend fits.
// k_roi_*      resize_body's shape: a lane has 4 adjacent output samples, a wavefront a tile of 256 samples, a luma tile two rows
//              with the chroma row under them for RGB; stores through put_luma4 / put_chroma4.  The taps come from the picture's
//              own segment, and every sample is chosen between the filter's value and the fill.
//
// What is read for a sample outside the rectangle: nothing.  Rectangles are even, so luma samples are inside or outside in PAIRS
// (a lane has two pairs, each over one chroma sample); a tile whose rows lie outside the rectangle (wave-uniform) and a lane with no
// sample inside skip every load.  A lane that straddles an edge reads table words through indices clamped into the table - so the
// words it reads for its outside samples are other samples' valid taps, whose frame bytes it may read and then drops for the fill.
// The host check (p264hip_rois_check) is what guarantees that every coordinate k_roi_taps writes lies in the frame.
// Grid: k_roi_taps (words of the largest segment / 256, ROIs); k_roi_* (tiles of a picture / 4, pictures).  No LDS.
#pragma once
#include "kernel_resize.h"
#include "p264hip_pos.h"

#define ROI_TAPS_THREADS 256

struct RoiDev {                     // one ROI as the kernels read it: 32 bytes
    uint32_t frame, seg;            // stream * slots + slot; where its segment begins in the scratch, in words (a multiple of 4)
    uint32_t dx, dy;                // the rectangle: dst_left | dst_width << 16, dst_top | dst_height << 16
    uint32_t sx, sy;                // the window: left | width << 16, top | height << 16
    uint32_t pad[2];
};
// frame == ROI_SKIP: an ROI of a device list that k_roi_plan (kernel_roi_dev.h) found invalid - every kernel returns for it behind
// its first load of the record.  A host list never holds it: its frame indices are below n_streams * slots
#define ROI_SKIP 0xffffffffu

__host__ __device__ __forceinline__ int roi_pad4(int n) { return (n + 3) & ~3; }
// words of the segment of a dw x dh rectangle
__host__ __device__ __forceinline__ int roi_seg_words(int dw, int dh) { return roi_pad4(dw) + roi_pad4(dh) + roi_pad4(dw >> 1) + roi_pad4(dh >> 1); }

__global__ __launch_bounds__(ROI_TAPS_THREADS) void k_roi_taps(const RoiDev *rois, int roi_base, uint32_t *scratch)
{
    const RoiDev *o = rois + roi_base + (int)blockIdx.y;
    const uint4 q = gload4(o);
    if (q.x == ROI_SKIP) return;
    const uint2 s = gload2(&o->sx);
    const int dw = (int)(q.z >> 16), dh = (int)(q.w >> 16);
    const int t = (int)(blockIdx.x * ROI_TAPS_THREADS + threadIdx.x);
    const int n0 = roi_pad4(dw), n1 = n0 + roi_pad4(dh), n2 = n1 + roi_pad4(dw >> 1), n3 = n2 + roi_pad4(dh >> 1);
    if (t >= n3) return;
    // the axis of this word: first sample of the window, its samples S, the rectangle's D, the destination index
    const bool chroma = t >= n1, vertical = chroma ? t >= n2 : t >= n0;
    const uint32_t w = vertical ? s.y : s.x;
    const int sh = chroma ? 1 : 0;
    const int first = (int)(w & 0xffffu) >> sh, S = (int)(w >> 16) >> sh, D = (vertical ? dh : dw) >> sh;
    int d = t - (chroma ? (vertical ? n2 : n1) : (vertical ? n0 : 0));
    d = min(d, D - 1);                                      // (the padding repeats the last word)
    const int32_t pos = p264hip_resize_pos(S, D, d);
    const int i0 = pos >> 8;
    scratch[q.y + (uint32_t)t] = (uint32_t)(pos & 255) | (i0 < S - 1 ? 1u << 8 : 0u) | (uint32_t)(first + i0) << 16;
}

__device__ __forceinline__ int roi_clamp(int v, int hi) { return min(max(v, 0), hi); }      // into 0 .. hi

template <int FMT, int DT>
__device__ __forceinline__ void roi_body(const uint8_t *frames, size_t frame_bytes, const Geom &g, const RoiDev *rois, const uint32_t *scratch, int pic_base,
                                         uint8_t *dst, const ResizeParams &e, uint32_t fill)
{
    constexpr bool RGB = FMT == P264HIP_FMT_RGB24 || FMT == P264HIP_FMT_RGBP;
    const int lane = threadIdx.x & 63;
    const int wt = rfl((int)(blockIdx.x * (RESIZE_THREADS / WAVE) + (threadIdx.x >> 6)));
    if (wt >= e.n_tiles) return;
    const int pic = pic_base + (int)blockIdx.y;
    const uint4 q = gload4(rois + pic);
    if (q.x == ROI_SKIP) return;                            // (a device list's invalid ROI: its picture is not written)
    const uint8_t *src = frames + (size_t)q.x * frame_bytes;
    const uint32_t *seg = scratch + q.y;
    uint8_t *out = dst + (int64_t)pic * e.frame_stride;
    const int dl = (int)(q.z & 0xffffu), dw = (int)(q.z >> 16), dt = (int)(q.w & 0xffffu), dh = (int)(q.w >> 16);
    const int t_yl = roi_pad4(dw), t_xc = t_yl + roi_pad4(dh), t_yc = t_xc + roi_pad4(dw >> 1);     // the tables of the segment
    const int fill_y = (int)(fill & 255u), fill_cb = (int)((fill >> 8) & 255u), fill_cr = (int)((fill >> 16) & 255u);
    if (wt < e.n_ltiles) {
        int ty, tx;
        split_tile(wt, e.ltx, e.inv_ltx, ty, tx);
        const int x = (tx * WAVE + lane) * RESIZE_PX, y = ty * 2;
        if (x >= e.w) return;
        const int rx = x - dl, ry = y - dt;                 // both even; negative left of / above the rectangle
        const bool rows_in = (unsigned)ry < (unsigned)dh;   // (wave-uniform; rows y and y + 1 together)
        const bool in[2] = { rows_in && (unsigned)rx < (unsigned)dw, rows_in && (unsigned)(rx + 2) < (unsigned)dw };    // the lane's two pairs
        int v[2][4], cb[2] = { fill_cb - 128, fill_cb - 128 }, cr[2] = { fill_cr - 128, fill_cr - 128 };
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int j = 0; j < 4; j++) v[r][j] = fill_y;
        if (in[0] || in[1]) {
            // a pair inside has its own two words (rx <= dw - 2 <= t_yl - 2); a pair outside reads the nearest pair of the table
            const uint2 qa = gload2(seg + roi_clamp(rx, t_yl - 2)), qb = gload2(seg + roi_clamp(rx + 2, t_yl - 2));
            const uint32_t xt[4] = { qa.x, qa.y, qb.x, qb.y };
            uint32_t fx[4], fy[2], s[2][4][4];
            int r0[2], r1[2];
#pragma unroll
            for (int r = 0; r < 2; r++) { tap_of(gload1(seg + t_yl + ry + r), r0[r], r1[r], fy[r]); r0[r] *= 16; r1[r] *= 16; }
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
                const int crx = rx >> 1, cw = dw >> 1;      // (rx is even: the shift is exact, also below 0)
                int q0, q1;
                tap_of(gload1(seg + t_yc + (ry >> 1)), q0, q1, cfy);
                q0 *= 16; q1 *= 16;
#pragma unroll
                for (int j = 0; j < 2; j++) {
                    int x0, x1;
                    tap_of(gload1(seg + t_xc + roi_clamp(crx + j, cw - 1)), x0, x1, cfx[j]);
                    const uint8_t *c0 = src + chroma_off(g, 0, x0, 0), *c1 = src + chroma_off(g, 0, x1, 0);
#pragma unroll
                    for (int p = 0; p < 2; p++) { cs[p][j][0] = gbyte(c0 + p * 8 + q0); cs[p][j][1] = gbyte(c1 + p * 8 + q0); cs[p][j][2] = gbyte(c0 + p * 8 + q1); cs[p][j][3] = gbyte(c1 + p * 8 + q1); }
                }
#pragma unroll
                for (int j = 0; j < 2; j++)
                    if (in[j]) { cb[j] = bilinear(cs[0][j], cfx[j], cfy) - 128; cr[j] = bilinear(cs[1][j], cfx[j], cfy) - 128; }
            }
#pragma unroll
            for (int r = 0; r < 2; r++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    if (in[j >> 1]) v[r][j] = bilinear(s[r][j], fx[j], fy[r]);
        }
        const int n = min(e.w - x, RESIZE_PX);
#pragma unroll
        for (int r = 0; r < 2; r++) put_luma4<FMT, DT>(out + (int64_t)(y + r) * e.pitch, x, v[r], cb, cr, n, e);
    } else if (!RGB) {
        int y, tx;
        split_tile(wt - e.n_ltiles, e.ctx, e.inv_ctx, y, tx);
        const int x = (tx * WAVE + lane) * RESIZE_PX, cw_out = e.w >> 1;
        if (x >= cw_out) return;
        const int cw = dw >> 1, rx = x - (dl >> 1), ry = y - (dt >> 1);
        const bool row_in = (unsigned)ry < (unsigned)(dh >> 1);         // (wave-uniform)
        bool in[4], any = false;
#pragma unroll
        for (int j = 0; j < 4; j++) { in[j] = row_in && (unsigned)(rx + j) < (unsigned)cw; any = any || in[j]; }
        int u[4] = { fill_cb, fill_cb, fill_cb, fill_cb }, v[4] = { fill_cr, fill_cr, fill_cr, fill_cr };
        if (any) {
            uint32_t fx[4], fy, s[2][4][4];
            int q0, q1;
            tap_of(gload1(seg + t_yc + ry), q0, q1, fy);
            q0 *= 16; q1 *= 16;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                int x0, x1;
                tap_of(gload1(seg + t_xc + roi_clamp(rx + j, cw - 1)), x0, x1, fx[j]);
                const uint8_t *c0 = src + chroma_off(g, 0, x0, 0), *c1 = src + chroma_off(g, 0, x1, 0);
#pragma unroll
                for (int p = 0; p < 2; p++) { s[p][j][0] = gbyte(c0 + p * 8 + q0); s[p][j][1] = gbyte(c1 + p * 8 + q0); s[p][j][2] = gbyte(c0 + p * 8 + q1); s[p][j][3] = gbyte(c1 + p * 8 + q1); }
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (in[j]) { u[j] = bilinear(s[0][j], fx[j], fy); v[j] = bilinear(s[1][j], fx[j], fy); }
        }
        const int n = min(cw_out - x, RESIZE_PX);
        put_chroma4<FMT>(out, y, x, u, v, n, e);
    }
}

// (a named kernel per instance of kernel_resize.h's EXPORT_INSTANCES)
#define ROI_KERNEL(family, sfx, fmt, dt) \
    __global__ __launch_bounds__(RESIZE_THREADS) void family##sfx(const uint8_t *frames, size_t frame_bytes, Geom g, const RoiDev *rois, const uint32_t *scratch, int pic_base, uint8_t *dst, ResizeParams e, uint32_t fill) \
    { roi_body<fmt, dt>(frames, frame_bytes, g, rois, scratch, pic_base, dst, e, fill); }
EXPORT_INSTANCES(ROI_KERNEL, k_roi_)
