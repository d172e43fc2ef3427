// kernel_roi_dev.h - what the host decided per ROI in p264hip_export_rois / p264hip_export_rois_aa, decided on the device for a list
// that lives there (include/p264hip.h: p264hip_export_rois_device).  One kernel a call, in front of the launch pairs:
//
// k_roi_plan   one thread per index i of the list's capacity n.  It reads the 40 bytes of the ROI (five 8-byte loads: the list is at
//              a multiple of 8), the device count (clamped into 0 .. n) and, for slot -1, the stream's entry of the slot table; applies
//              include/p264hip_roi_rule.h's rule - the text the host compiles as p264hip_roi_status -; and writes the RoiDev record
//              k_roi_taps / k_roi_aa_taps and the body kernels read, exactly as the host writes it for a host list, but for the
//              segment: every ROI has one of the plan's seg_words, ROI i the (i mod rois_per_pair)-th of its pair.
//              A record whose status is not 0 carries the SKIP mark, frame == ROI_SKIP: the taps kernels and the sixteen bodies
//              return for it behind their first load of the record - before a table word, a frame byte or LDS is read, before the
//              first barrier (the mark is workgroup-uniform: a workgroup has one ROI) and before anything is written.  The host-list
//              calls never produce the mark: their frame index is below n_streams * slots.
// Grid: (n / 256).  No LDS.  Stores are plain vector stores.
#pragma once
#include "kernel_roi.h"
#include "p264hip_aa.h"
#include "p264hip_roi_rule.h"

#define ROI_PLAN_THREADS 256

struct RoiPlanParams {
    int32_t n, w, h, filter;                // the list's capacity; the output and its filter
    int32_t fw, fh, n_streams, slots;       // the frame in samples; the store
    int32_t max_reduction, seg_words, rois_per_pair, lds_cap;   // (lds_cap: AA_T_CAP, what p264hip_roi_aa_tile fits a tile to)
};

__global__ __launch_bounds__(ROI_PLAN_THREADS) void k_roi_plan(const p264hip_roi_t *rois, const int32_t *count, const int32_t *slot_of_stream, RoiPlanParams p,
                                                               RoiDev *table, int32_t *status)
{
    const int i = (int)(blockIdx.x * ROI_PLAN_THREADS + threadIdx.x);
    if (i >= p.n) return;
    int32_t o[10];
#pragma unroll
    for (int k = 0; k < 5; k++) { const uint2 v = gload2((const uint32_t *)(rois + i) + 2 * k); o[2 * k] = (int32_t)v.x; o[2 * k + 1] = (int32_t)v.y; }
    const int used = count ? min(max((int)gload1(count), 0), p.n) : p.n;
    int32_t st;
    if (i >= used) st = P264HIP_ROI_UNUSED;
    else {
        st = -1;
        if (o[1] == -1 && slot_of_stream && o[0] >= 0 && o[0] < p.n_streams) {
            o[1] = (int32_t)gload1(slot_of_stream + o[0]);
            if (o[1] < 0) st = P264HIP_ROI_NO_PICTURE;
        }
        if (st < 0) st = p264hip_roi_rule(o, p.w, p.h, p.filter, p.fw, p.fh, p.n_streams, p.slots, p.max_reduction);
    }
    if (status) gstore1(status + i, (uint32_t)st);
    uint4 a = make_uint4(ROI_SKIP, 0u, 0u, 0u), b = make_uint4(0u, 0u, 0u, 0u);
    if (st == P264HIP_ROI_OK) {
        const bool whole = !(o[6] | o[7] | o[8] | o[9]);
        const int dl = whole ? 0 : o[6], dt = whole ? 0 : o[7], dw = whole ? p.w : o[8], dh = whole ? p.h : o[9];
        a = make_uint4((uint32_t)(o[0] * p.slots + o[1]), (uint32_t)((i % p.rois_per_pair) * p.seg_words), (uint32_t)dl | (uint32_t)dw << 16, (uint32_t)dt | (uint32_t)dh << 16);
        b.x = (uint32_t)o[2] | (uint32_t)o[4] << 16; b.y = (uint32_t)o[3] | (uint32_t)o[5] << 16;
        if (p.filter == P264HIP_FILTER_BILINEAR_AA) {
            // the ROI's tile width and LDS rows, and its four weight strides (kernel_roi_aa.h reads them)
            int ns_l, ns_c;
            const int tw_shift = p264hip_roi_aa_tile(o[4], dw, p.lds_cap, &ns_l, &ns_c);
            b.z = (uint32_t)tw_shift | (uint32_t)ns_l << 8 | (uint32_t)ns_c << 16;
            b.w = (uint32_t)p264hip_aa_stride(o[4], dw) | (uint32_t)p264hip_aa_stride(o[5], dh) << 8
                | (uint32_t)p264hip_aa_stride(o[4] >> 1, dw >> 1) << 16 | (uint32_t)p264hip_aa_stride(o[5] >> 1, dh >> 1) << 24;
        }
    }
    gstore4(table + i, a);
    gstore4(&table[i].sx, b);
}
