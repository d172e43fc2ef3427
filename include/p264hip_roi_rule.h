/* p264hip_roi_rule.h - the ONE definition of what makes a p264hip_roi_t valid (include/p264hip.h: P264HIP_ROI_*) and of what a call
 * whose ROI list lives in device memory reserves per ROI, in plain C so that the host (csrc/host/resize_layout.c: p264hip_roi_status,
 * p264hip_rois_device_plan) and the device (csrc/hip/kernel_roi_dev.h: k_roi_plan) compile the same text.  As p264hip_pos.h and
 * p264hip_aa.h do for the taps.
 *
 * The STATUS of an ROI is the first rule of rois_why (csrc/host/resize_layout.c) it breaks, in that function's order; its messages
 * stay that function's.  Every sum of two members is a 64-bit one: the members are whatever 32 bits a device list holds.
 *
 * The PLAN (p264hip_rois_plan_t) is a bound over every ROI that passes the rule, computed from the output size and the largest
 * reduction m alone:
 *   a weight row  stride(S, D) grows with S, and S <= min(m D, 65534): the widest window of a rectangle side D is known
 *   a segment     the sum, per direction, of the luma axis of D and the chroma axis of D / 2; D is walked, as the stride falls once
 *                 m D passes 65534 and the words need not grow with D there
 *   a tile        p264hip_roi_aa_tile's width falls as S grows and, at one width, its strips grow with S: the most tiles are those
 *                 of the widest window, the most LDS is that of the widest window of each tile width (a bisection per width) */
#ifndef P264HIP_ROI_RULE_H
#define P264HIP_ROI_RULE_H
#include <stdint.h>
#include "p264hip_aa.h"

#ifdef __HIPCC__
#define P264HIP_RULE_FN __host__ __device__ static inline
#else
#define P264HIP_RULE_FN static inline
#endif

#define P264HIP_ROI_RULE_FRAME_MAX 65534      /* the widest even window of a frame of at most 65535 samples a side */

/* the status of the ROI o[0 .. 9] (the members of p264hip_roi_t in their order, the slot resolved) in a W x H output with `filter`,
 * a frame of fw x fh samples and a store of n_streams x slots; max_reduction 0 means 32.  One of 0, 2, 4 .. 10 */
P264HIP_RULE_FN int32_t p264hip_roi_rule(const int32_t *o, int32_t W, int32_t H, int32_t filter, int64_t fw, int64_t fh, int32_t n_streams, int32_t slots, int32_t max_reduction)
{
    const int32_t stream = o[0], slot = o[1], left = o[2], top = o[3], width = o[4], height = o[5], dl = o[6], dt = o[7], dw = o[8], dh = o[9];
    if (stream < 0 || stream >= n_streams || slot < 0 || slot >= slots) return 2;
    if (left < 0 || top < 0 || width < 1 || height < 1) return 4;
    if ((left | top | width | height) & 1) return 5;
    if ((int64_t)left + width > fw || (int64_t)top + height > fh) return 6;
    const int whole = !(dl | dt | dw | dh);
    if (!whole) {
        if (dl < 0 || dt < 0 || dw < 2 || dh < 2) return 7;
        if ((dl | dt | dw | dh) & 1) return 8;
        if ((int64_t)dl + dw > W || (int64_t)dt + dh > H) return 9;
    }
    if (filter == 2) {
        const int64_t m = max_reduction ? max_reduction : 32;
        if (width > m * (int64_t)(whole ? W : dw) || height > m * (int64_t)(whole ? H : dh)) return 10;
    }
    return 0;
}

/* the widest (highest) window a rectangle side of D samples may have at the reduction m */
P264HIP_RULE_FN int32_t p264hip_roi_rule_widest(int32_t D, int32_t m)
{
    const int64_t s = (int64_t)m * D;
    return (int32_t)(s < P264HIP_ROI_RULE_FRAME_MAX ? s : P264HIP_ROI_RULE_FRAME_MAX);
}

/* the most words the two axes of one direction (luma of D, chroma of D / 2) take over the even D of 2 .. out_n */
P264HIP_RULE_FN int32_t p264hip_roi_rule_axis_bound(int32_t out_n, int32_t m)
{
    int32_t most = 0;
    for (int32_t D = 2; D <= out_n; D += 2) {
        const int32_t S = p264hip_roi_rule_widest(D, m);
        const int32_t words = p264hip_aa_axis_words(D, p264hip_aa_stride(S, D)) + p264hip_aa_axis_words(D >> 1, p264hip_aa_stride(S >> 1, D >> 1));
        most = words > most ? words : most;
    }
    return most;
}

/* the dynamic LDS of k_roi_aa_* for a window of `width` into a rectangle `dw` wide, and its tile width as log2(lanes) */
P264HIP_RULE_FN int32_t p264hip_roi_rule_lds(int32_t width, int32_t dw, int32_t cap, int32_t *shift)
{
    int ns_l, ns_c;
    *shift = p264hip_roi_aa_tile(width, dw, cap, &ns_l, &ns_c);
    return 32 * (ns_l * 16 > ns_c * 8 ? ns_l * 16 : ns_c * 8);
}

/* the most tiles of any passing ROI of a W x H output (the tile rows are 16 high: kernel_resize_aa.h's AA_TH); *lds_bytes: the most
 * dynamic LDS */
P264HIP_RULE_FN int32_t p264hip_roi_rule_tiles(int32_t W, int32_t H, int32_t m, int32_t cap, int32_t *lds_bytes)
{
    int32_t most_tiles = 0, most_lds = 0;
    for (int32_t dw = 2; dw <= W; dw += 2) {
        const int32_t widest = p264hip_roi_rule_widest(dw, m);
        int32_t shift;
        int32_t lds = p264hip_roi_rule_lds(widest, dw, cap, &shift);
        const int32_t tw = 4 << shift, t = ((W + tw - 1) / tw) * ((H + 15) / 16);
        most_tiles = t > most_tiles ? t : most_tiles;
        most_lds = lds > most_lds ? lds : most_lds;
        /* the widest even window that still takes a tile of at least 4 << s samples: the tile width never grows with the window */
        for (int32_t s = shift + 1; s <= 4; s++) {
            int32_t lo = 1, hi = widest >> 1, sh;           /* (halves of a width: 2 lo takes s or more where any width does) */
            (void)p264hip_roi_rule_lds(2, dw, cap, &sh);
            if (sh < s) break;
            while (lo < hi) {
                const int32_t mid = (lo + hi + 1) >> 1;
                (void)p264hip_roi_rule_lds(2 * mid, dw, cap, &sh);
                if (sh >= s) lo = mid; else hi = mid - 1;
            }
            lds = p264hip_roi_rule_lds(2 * lo, dw, cap, &sh);
            most_lds = lds > most_lds ? lds : most_lds;
        }
    }
    *lds_bytes = most_lds;
    return most_tiles;
}
#endif
