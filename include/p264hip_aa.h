/* p264hip_aa.h - the ONE definition of the taps of the antialiased filter (include/p264hip.h: P264HIP_FILTER_BILINEAR_AA) and of the
 * tap SEGMENT of an ROI (p264hip_export_rois_aa), in plain C so that the host (csrc/host/resize_layout.c: p264hip_resize_aa_taps,
 * p264hip_roi_aa_segment) and the device (csrc/hip/kernel_roi_aa.h: k_roi_aa_taps) compile the same text: the CPU tests of the two
 * host functions pin the arithmetic the device runs.  As p264hip_pos.h does for the filter-0 position.
 *
 * The taps of destination index d of an axis with S source and D destination samples (64-bit integers throughout: tap making is not
 * a hot path):
 *   U = 2 max(S, D),  r(j) = U - |(2j+1) D - (2d+1) S|,  taps = the j of 0 .. S-1 with r(j) > 0,  R = their sum,
 *   w(j) = floor(r(j) 32768 / R),  the residue 32768 - sum w to the tap with the largest r (the lowest index among equals)
 *
 * The segment of an ROI whose window is S_x x S_y luma samples and whose rectangle is D_x x D_y: four AXES in the order x luma,
 * y luma, x chroma, y chroma (chroma: every number halved), each
 *   pad4(D) words       first | count << 16 per destination index, first a coordinate of the FRAME; the padding repeats the last
 *   pad4(D stride / 2)  words of 16-bit Q15 weights, a row of `stride` per destination index, 0 behind its count and in the padding
 * with stride a closed-form bound of the count, so that segments are sized without making taps:
 *   stride = 2 for S <= D,  min(64, ceil(2 S / D)) rounded up to even otherwise
 * (the j with r(j) > 0 lie in an open interval of length 2 max(S, D) / D.)  A segment is made ENTRY by entry: entry t of
 * pad4(D_x) + pad4(D_y) + pad4(D_x / 2) + pad4(D_y / 2) is one destination index of one axis - a thread of k_roi_aa_taps. */
#ifndef P264HIP_AA_H
#define P264HIP_AA_H
#include <stdint.h>

#ifdef __HIPCC__
#define P264HIP_AA_FN __host__ __device__ static inline
#else
#define P264HIP_AA_FN static inline
#endif

/* the taps of destination index d: the count (at most cap), *first relative to the window, the Q15 weights in w[0 .. count-1] */
P264HIP_AA_FN int32_t p264hip_aa_tap(int32_t src_n, int32_t dst_n, int32_t d, int cap, int32_t *first, uint16_t *w)
{
    const int64_t S = src_n, D = dst_n, U = 2 * (S > D ? S : D), c = (2 * (int64_t)d + 1) * S;
    /* r(j) > 0: c - U < (2j+1)*D < c + U */
    const int64_t below = c - U - D, above = -(c + U - D), den = 2 * D;        /* (floors of quotients of either sign) */
    int64_t lo = (below >= 0 ? below / den : -((-below + den - 1) / den)) + 1, hi = -(above >= 0 ? above / den : -((-above + den - 1) / den)) - 1;
    if (lo < 0) lo = 0;
    if (hi > S - 1) hi = S - 1;
    int64_t R = 0, best = -1, sum = 0, top = 0;
    int n = 0, at = 0;
    for (int64_t j = lo; j <= hi && n < cap; j++, n++) {
        const int64_t a = (2 * j + 1) * D - c;
        R += U - (a < 0 ? -a : a);
    }
    for (int k = 0; k < n; k++) {
        const int64_t a = (2 * (lo + k) + 1) * D - c;
        const int64_t r = U - (a < 0 ? -a : a), q = r * 32768 / R;
        if (r > best) { best = r; at = k; top = q; }
        w[k] = (uint16_t)q; sum += q;
    }
    w[at] = (uint16_t)(top + (32768 - sum));
    *first = (int32_t)lo;
    return n;
}

P264HIP_AA_FN int32_t p264hip_aa_pad4(int n) { return (n + 3) & ~3; }
/* 16-bit weights of a row: no destination index of S -> D has more taps (1 <= S <= 65535, S <= 32 D) */
P264HIP_AA_FN int32_t p264hip_aa_stride(int32_t src_n, int32_t dst_n)
{
    if (src_n <= dst_n) return 2;
    const uint32_t q = (2u * (uint32_t)src_n + (uint32_t)dst_n - 1u) / (uint32_t)dst_n;
    return (int)((q > 64u ? 64u : q) + 1u) & ~1;
}
/* words of an axis: its first | count words, then its weights */
P264HIP_AA_FN int32_t p264hip_aa_axis_words(int dst_n, int stride) { return p264hip_aa_pad4(dst_n) + p264hip_aa_pad4(dst_n * (stride >> 1)); }
/* entries of a segment, and its words */
P264HIP_AA_FN int32_t p264hip_roi_aa_entries(int dw, int dh) { return p264hip_aa_pad4(dw) + p264hip_aa_pad4(dh) + p264hip_aa_pad4(dw >> 1) + p264hip_aa_pad4(dh >> 1); }
P264HIP_AA_FN int32_t p264hip_roi_aa_words(int width, int height, int dw, int dh)
{
    return p264hip_aa_axis_words(dw, p264hip_aa_stride(width, dw)) + p264hip_aa_axis_words(dh, p264hip_aa_stride(height, dh))
         + p264hip_aa_axis_words(dw >> 1, p264hip_aa_stride(width >> 1, dw >> 1)) + p264hip_aa_axis_words(dh >> 1, p264hip_aa_stride(height >> 1, dh >> 1));
}

/* entry t of the segment `seg` of the window (left, top, width, height) into a dw x dh rectangle: the word and the weight row of one
 * destination index of one axis; returns the taps it made.  An entry of an axis' padding writes nothing and returns 0: the axis' last
 * index writes the padding with its own. */
P264HIP_AA_FN int32_t p264hip_roi_aa_entry(uint32_t *seg, int left, int top, int width, int height, int dw, int dh, int t)
{
    const int n0 = p264hip_aa_pad4(dw), n1 = n0 + p264hip_aa_pad4(dh), n2 = n1 + p264hip_aa_pad4(dw >> 1), n3 = n2 + p264hip_aa_pad4(dh >> 1);
    if (t < 0 || t >= n3) return 0;
    const int w_xl = p264hip_aa_axis_words(dw, p264hip_aa_stride(width, dw)), w_yl = p264hip_aa_axis_words(dh, p264hip_aa_stride(height, dh));
    const int w_xc = p264hip_aa_axis_words(dw >> 1, p264hip_aa_stride(width >> 1, dw >> 1));
    /* the axis of this entry: where it begins in the segment, the first sample of the window, its samples S, the rectangle's D */
    const int chroma = t >= n1, vertical = chroma ? t >= n2 : t >= n0, sh = chroma ? 1 : 0;
    const int base = chroma ? (vertical ? w_xl + w_yl + w_xc : w_xl + w_yl) : (vertical ? w_xl : 0);
    const int origin = (vertical ? top : left) >> sh, S = (vertical ? height : width) >> sh, D = (vertical ? dh : dw) >> sh;
    const int d = t - (chroma ? (vertical ? n2 : n1) : (vertical ? n0 : 0));
    if (d >= D) return 0;
    const int stride = p264hip_aa_stride(S, D), padded = p264hip_aa_pad4(D);
    uint16_t *weights = (uint16_t *)(seg + base + padded), *w = weights + d * stride;
    int32_t first;
    const int n = p264hip_aa_tap(S, D, d, stride, &first, w);
    for (int k = n; k < stride; k++) w[k] = 0;
    const uint32_t word = (uint32_t)(origin + first) | (uint32_t)n << 16;
    seg[base + d] = word;
    if (d == D - 1) {
        for (int p = D; p < padded; p++) seg[base + p] = word;
        const int rows_end = p264hip_aa_pad4(D * (stride >> 1)) * 2;           /* (16-bit values of the axis' weights, padding included) */
        for (int k = D * stride; k < rows_end; k++) weights[k] = 0;
    }
    return n;
}

/* the tile of an ROI in k_roi_aa_*: log2 of the lanes of a luma row of a tile (4, 3, 2, 1: 64, 32, 16, 8 samples), the widest
 * whose source columns fit `cap` 16-bit values of 16 luma rows and of 8 chroma rows; *ns_l, *ns_c: strips (of 16 luma, of 8 chroma
 * samples) of a tile row at most.  A tile of tw destination samples, wherever it begins, spans at most
 *   ceil((tw - 1) S / D) + stride + 1
 * source samples (first(x) moves by at most ceil(S / D) per index and the last index has at most stride taps), and n samples touch
 * at most (n - 2) / 16 + 2 strips of 16.  At 32:1 a tile of 8 spans 289 samples, 19 strips: it always fits. */
P264HIP_AA_FN int32_t p264hip_roi_aa_tile(int width, int dw, int cap, int *ns_l, int *ns_c)
{
    for (int shift = 4;; shift--) {
        const int tw = 4 << shift, S = width, D = dw, cs = width >> 1, cd = dw >> 1, ctw = tw >> 1;
        int n_l = (int)(((int64_t)(tw - 1) * S + D - 1) / D) + p264hip_aa_stride(S, D) + 1;
        int n_c = (int)(((int64_t)(ctw - 1) * cs + cd - 1) / cd) + p264hip_aa_stride(cs, cd) + 1;
        n_l = n_l < S ? n_l : S; n_c = n_c < cs ? n_c : cs;          /* (and no more than the window has) */
        *ns_l = (n_l + 30) >> 4; *ns_c = (n_c + 14) >> 3;
        if (shift == 1 || (*ns_l * 16 * 16 <= cap && *ns_c * 16 * 8 <= cap)) return shift;
    }
}
#endif
