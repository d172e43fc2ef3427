/* resize_layout.c - the layout of a resized exported picture (include/p264hip.h: p264hip_resize_t), the checks every resized
 * export runs before anything is queued - the lists of per-picture windows of p264hip_export_rois and p264hip_export_rois_aa among
 * them -, the taps of the two filters and the tap segment of an ROI.  Pure host code, no device involved; the kernels are
 * csrc/hip/kernel_resize.h, kernel_resize_aa.h, kernel_roi.h and kernel_roi_aa.h. */
#include <math.h>
#include "p264hip.h"
#include "p264hip_pos.h"
#include "p264hip_aa.h"
#include "p264hip_roi_rule.h"

static int is_rgb(int format) { return format == P264HIP_FMT_RGB24 || format == P264HIP_FMT_RGBP; }

/* why the description is refused on its own (NULL: it is not); *pitch, *bytes: the pitch in bytes and one picture's bytes */
static const char *describe(const p264hip_resize_t *r, int64_t *pitch, int64_t *bytes, int *elem)
{
    if (!r) return "null description";
    if (r->format < P264HIP_FMT_I420 || r->format > P264HIP_FMT_RGBP) return "unknown format";
    if (r->matrix != P264HIP_MATRIX_BT601 && r->matrix != P264HIP_MATRIX_BT709) return "unknown matrix";
    if (r->full_range != 0 && r->full_range != 1) return "full_range is neither 0 nor 1";
    if (!is_rgb(r->format) && (r->matrix || r->full_range)) return "matrix / full_range set on a YUV format";
    if (r->crop_left < 0 || r->crop_top < 0 || r->crop_width < 1 || r->crop_height < 1) return "window with a negative offset or without samples";
    if ((r->crop_left | r->crop_top | r->crop_width | r->crop_height) & 1) return "window with an odd member";
    if (r->width < 2 || r->height < 2 || r->width > 16384 || r->height > 16384) return "output size outside 2 .. 16384";
    if ((r->width | r->height) & 1) return "odd output size";
    if (r->dtype != P264HIP_DTYPE_U8 && r->dtype != P264HIP_DTYPE_F16 && r->dtype != P264HIP_DTYPE_F32) return "unknown dtype";
    if (r->filter != P264HIP_FILTER_BILINEAR && r->filter != P264HIP_FILTER_BILINEAR_AA) return "unknown filter";
    if (r->dtype != P264HIP_DTYPE_U8 && !is_rgb(r->format)) return "float dtype on a YUV format";
    for (int k = 0; k < 3; k++) {
        if (!isfinite(r->scale[k]) || !isfinite(r->bias[k])) return "scale / bias not finite";
        if (r->dtype == P264HIP_DTYPE_U8 && (r->scale[k] != 0.0f || r->bias[k] != 0.0f)) return "scale / bias set on the dtype U8";
    }
    const int64_t e = r->dtype == P264HIP_DTYPE_U8 ? 1 : r->dtype == P264HIP_DTYPE_F16 ? 2 : 4;
    const int64_t tight = (r->format == P264HIP_FMT_RGB24 ? 3 * (int64_t)r->width : (int64_t)r->width) * e;
    const int64_t p = r->pitch ? (int64_t)r->pitch : tight;
    if (p < tight) return "pitch below the tight pitch";
    if (p % e) return "pitch no multiple of the element size";
    if (r->format == P264HIP_FMT_I420 && (p & 1)) return "odd pitch for I420";
    if (r->filter == P264HIP_FILTER_BILINEAR_AA && (r->crop_width > 32 * (int64_t)r->width || r->crop_height > 32 * (int64_t)r->height))
        return "reduction above 32:1 with the antialiased filter";
    const int64_t h = r->height;
    *pitch = p; *elem = (int)e;
    *bytes = r->format == P264HIP_FMT_RGB24 ? p * h : r->format == P264HIP_FMT_RGBP ? 3 * p * h : p * h + p * (h / 2);
    return 0;
}

/* the same with the frame and the stride (what p264hip_export_resized reports through p264hip_last_error) */
const char *p264hip_resize_why_(const p264hip_resize_t *r, int mb_w, int mb_h)
{
    int64_t pitch, bytes;
    int elem;
    const char *why = describe(r, &pitch, &bytes, &elem);
    if (why) return why;
    if (mb_w < 1 || mb_h < 1) return "no frame";
    if ((int64_t)r->crop_left + r->crop_width > (int64_t)mb_w * 16 || (int64_t)r->crop_top + r->crop_height > (int64_t)mb_h * 16) return "window leaves the frame";
    if (r->frame_stride < 0 || (r->frame_stride && r->frame_stride < bytes)) return "frame_stride below the picture's bytes";
    if (r->frame_stride % elem) return "frame_stride no multiple of the element size";
    return 0;
}

int64_t p264hip_resize_frame_bytes(const p264hip_resize_t *r)
{
    int64_t pitch, bytes;
    int elem;
    return describe(r, &pitch, &bytes, &elem) ? P264HIP_EINVAL : bytes;
}

int p264hip_resize_check(const p264hip_resize_t *r, int mb_w, int mb_h)
{
    return p264hip_resize_why_(r, mb_w, mb_h) ? P264HIP_EINVAL : P264HIP_OK;
}

int p264hip_resize_taps(int src_n, int dst_n, int32_t *pos)
{
    if (!pos || src_n < 1 || dst_n < 1 || src_n > (1 << 20) || dst_n > (1 << 20)) return P264HIP_EINVAL;
    for (int d = 0; d < dst_n; d++) pos[d] = p264hip_resize_pos(src_n, dst_n, d);      /* (p264hip_pos.h: the device runs the same text) */
    return P264HIP_OK;
}

/* ---- per-picture windows into rectangles of the output (include/p264hip.h: p264hip_roi_t; csrc/hip/kernel_roi.h) ---- */
/* the description with a window every frame holds: crop_* are not read on this road */
static p264hip_resize_t without_window(const p264hip_resize_t *r)
{
    p264hip_resize_t q = *r;
    q.crop_left = q.crop_top = 0; q.crop_width = q.crop_height = 2;
    return q;
}

/* why the call is refused (NULL: it is not); *bad: the index of the first bad ROI, -1 where the call is refused on its own */
/* aa: the call is p264hip_export_rois_aa's, whose filter is the antialiased one, limited to 32:1 per ROI */
static const char *rois_why(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots, int *bad, int aa)
{
    *bad = -1;
    if (!r) return "null description";
    if (!aa && r->filter == P264HIP_FILTER_BILINEAR_AA) return "the antialiased filter is p264hip_export_rois_aa's (filter must be P264HIP_FILTER_BILINEAR)";
    if (aa && r->filter != P264HIP_FILTER_BILINEAR_AA) return "filter must be P264HIP_FILTER_BILINEAR_AA (p264hip_export_rois has the plain bilinear filter)";
    const p264hip_resize_t q = without_window(r);
    const char *why = p264hip_resize_why_(&q, mb_w, mb_h);
    if (why) return why;
    if (!rois) return "null ROI list";
    if (n < 1) return "no ROI";
    if (n_streams < 1 || slots < 1) return "no frame store";
    if (fill >> 24) return "fill with a bit above 23 set";
    const int64_t fw = (int64_t)mb_w * 16, fh = (int64_t)mb_h * 16;
    for (int i = 0; i < n; i++) {
        const p264hip_roi_t *o = rois + i;
        *bad = i;
        if (o->stream < 0 || o->stream >= n_streams || o->slot < 0 || o->slot >= slots) return "stream or slot out of range";
        if (o->left < 0 || o->top < 0 || o->width < 1 || o->height < 1) return "window with a negative offset or without samples";
        if ((o->left | o->top | o->width | o->height) & 1) return "window with an odd member";
        if ((int64_t)o->left + o->width > fw || (int64_t)o->top + o->height > fh) return "window leaves the frame";
        const int whole = !(o->dst_left | o->dst_top | o->dst_width | o->dst_height);
        if (!whole) {
            if (o->dst_left < 0 || o->dst_top < 0 || o->dst_width < 2 || o->dst_height < 2) return "rectangle with a negative offset or below 2 x 2";
            if ((o->dst_left | o->dst_top | o->dst_width | o->dst_height) & 1) return "rectangle with an odd member";
            if ((int64_t)o->dst_left + o->dst_width > r->width || (int64_t)o->dst_top + o->dst_height > r->height) return "rectangle leaves the output";
        }
        if (aa && (o->width > 32 * (int64_t)(whole ? r->width : o->dst_width) || o->height > 32 * (int64_t)(whole ? r->height : o->dst_height)))
            return "reduction above 32:1 with the antialiased filter";
    }
    *bad = -1;
    return 0;
}

/* bytes of one picture of a call whose filter is `filter` */
static int64_t rois_frame_bytes(const p264hip_resize_t *r, int filter)
{
    if (!r || r->filter != filter) return P264HIP_EINVAL;
    const p264hip_resize_t q = without_window(r);
    return p264hip_resize_frame_bytes(&q);
}

static int rois_check(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots, int aa)
{
    int bad;
    return rois_why(rois, n, r, fill, mb_w, mb_h, n_streams, slots, &bad, aa) ? P264HIP_EINVAL : P264HIP_OK;
}

const char *p264hip_rois_why_(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots, int *bad)
{
    return rois_why(rois, n, r, fill, mb_w, mb_h, n_streams, slots, bad, 0);
}

int64_t p264hip_rois_frame_bytes(const p264hip_resize_t *r) { return rois_frame_bytes(r, P264HIP_FILTER_BILINEAR); }

int p264hip_rois_check(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots)
{
    return rois_check(rois, n, r, fill, mb_w, mb_h, n_streams, slots, 0);
}

int p264hip_resize_aa_taps(int src_n, int dst_n, int32_t *first, int32_t *count, uint16_t *weights)
{
    if (!first || !count || !weights || src_n < 1 || dst_n < 1 || src_n > (1 << 20) || dst_n > (1 << 20) || (int64_t)src_n > 32 * (int64_t)dst_n) return P264HIP_EINVAL;
    for (int d = 0; d < dst_n; d++) {
        uint16_t *w = weights + (size_t)d * P264HIP_AA_MAX_TAPS;
        count[d] = p264hip_aa_tap(src_n, dst_n, d, P264HIP_AA_MAX_TAPS, first + d, w);         /* (p264hip_aa.h: the device runs the same text) */
        for (int k = count[d]; k < P264HIP_AA_MAX_TAPS; k++) w[k] = 0;
    }
    return P264HIP_OK;
}

/* ---- per-picture windows with the antialiased filter (include/p264hip.h: p264hip_export_rois_aa; csrc/hip/kernel_roi_aa.h) ---- */
const char *p264hip_rois_aa_why_(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots, int *bad)
{
    return rois_why(rois, n, r, fill, mb_w, mb_h, n_streams, slots, bad, 1);
}

int64_t p264hip_rois_aa_frame_bytes(const p264hip_resize_t *r) { return rois_frame_bytes(r, P264HIP_FILTER_BILINEAR_AA); }

int p264hip_rois_aa_check(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots)
{
    return rois_check(rois, n, r, fill, mb_w, mb_h, n_streams, slots, 1);
}

/* the rectangle of an ROI in a W x H output; 0 where the segment helpers cannot take the pair (they check sizes, not the frame) */
static int segment_rect(const p264hip_roi_t *o, const p264hip_resize_t *r, int *dw, int *dh)
{
    if (!o || !r) return 0;
    const int whole = !(o->dst_left | o->dst_top | o->dst_width | o->dst_height);
    *dw = whole ? r->width : o->dst_width; *dh = whole ? r->height : o->dst_height;
    if (*dw < 2 || *dh < 2 || *dw > 16384 || *dh > 16384 || ((*dw | *dh) & 1)) return 0;
    if (o->left < 0 || o->top < 0 || o->width < 2 || o->height < 2 || ((o->left | o->top | o->width | o->height) & 1)) return 0;
    if ((int64_t)o->left + o->width > 65536 || (int64_t)o->top + o->height > 65536) return 0;
    return o->width <= 32 * (int64_t)*dw && o->height <= 32 * (int64_t)*dh;
}

int p264hip_roi_aa_segment_words(const p264hip_roi_t *roi, const p264hip_resize_t *r)
{
    int dw, dh;
    return segment_rect(roi, r, &dw, &dh) ? p264hip_roi_aa_words(roi->width, roi->height, dw, dh) : P264HIP_EINVAL;
}

int p264hip_roi_aa_segment(const p264hip_roi_t *roi, const p264hip_resize_t *r, uint32_t *words)
{
    int dw, dh;
    if (!words || !segment_rect(roi, r, &dw, &dh)) return P264HIP_EINVAL;
    const int n = p264hip_roi_aa_entries(dw, dh);
    for (int t = 0; t < n; t++) (void)p264hip_roi_aa_entry(words, roi->left, roi->top, roi->width, roi->height, dw, dh, t);   /* (k_roi_aa_taps: a thread each) */
    return P264HIP_OK;
}

int p264hip_roi_aa_tile_width(const p264hip_roi_t *roi, const p264hip_resize_t *r, int *luma_strips, int *chroma_strips)
{
    int dw, dh, ns_l, ns_c;
    if (!segment_rect(roi, r, &dw, &dh)) return P264HIP_EINVAL;
    const int shift = p264hip_roi_aa_tile(roi->width, dw, P264HIP_ROI_AA_TILE_VALUES, &ns_l, &ns_c);
    if (luma_strips) *luma_strips = ns_l;
    if (chroma_strips) *chroma_strips = ns_c;
    return 4 << shift;
}

/* ---- ROI lists that live in device memory (include/p264hip.h: p264hip_export_rois_device; csrc/hip/kernel_roi_dev.h) ---- */
int p264hip_roi_status(const p264hip_roi_t *roi, const p264hip_resize_t *r, int mb_w, int mb_h, int n_streams, int slots, int max_reduction)
{
    if (!roi || !r) return P264HIP_EINVAL;
    return p264hip_roi_rule(&roi->stream, r->width, r->height, r->filter, (int64_t)mb_w * 16, (int64_t)mb_h * 16, n_streams, slots, max_reduction);     /* (p264hip_roi_rule.h: the device runs the same text) */
}

/* why a description and a reduction give no plan (NULL: they do) */
static const char *plan_why(const p264hip_resize_t *r, int max_reduction)
{
    if (!r) return "null description";
    if (r->filter != P264HIP_FILTER_BILINEAR && r->filter != P264HIP_FILTER_BILINEAR_AA) return "unknown filter";
    if (rois_frame_bytes(r, r->filter) < 0) return "p264hip_rois_frame_bytes / p264hip_rois_aa_frame_bytes refuses the description";
    if (r->filter == P264HIP_FILTER_BILINEAR ? max_reduction != 0 : (max_reduction < 0 || max_reduction > 32)) return "max_reduction must be 0 with the bilinear filter and 0 .. 32 with the antialiased one";
    return 0;
}

int p264hip_rois_device_plan(const p264hip_resize_t *r, int max_reduction, p264hip_rois_plan_t *out)
{
    if (!out || plan_why(r, max_reduction)) return P264HIP_EINVAL;
    const int m = max_reduction ? max_reduction : 32;
    out->aa_tiles = out->aa_lds_bytes = 0;
    if (r->filter == P264HIP_FILTER_BILINEAR) out->seg_words = p264hip_roi_aa_entries(r->width, r->height);      /* (a word per entry: kernel_roi.h) */
    else {
        out->seg_words = p264hip_roi_rule_axis_bound(r->width, m) + p264hip_roi_rule_axis_bound(r->height, m);
        out->aa_tiles = p264hip_roi_rule_tiles(r->width, r->height, m, P264HIP_ROI_AA_TILE_VALUES, &out->aa_lds_bytes);
    }
    out->rois_per_pair = (int32_t)(P264HIP_ROI_SCRATCH_BYTES / 4 / out->seg_words);
    return out->rois_per_pair >= 1 ? P264HIP_OK : P264HIP_EINVAL;
}

const char *p264hip_rois_device_why_(const p264hip_rois_dev_t *l, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots)
{
    if (!l) return "null list";
    const char *why = plan_why(r, l->max_reduction);
    if (why) return why;
    const p264hip_resize_t q = without_window(r);
    if ((why = p264hip_resize_why_(&q, mb_w, mb_h))) return why;
    if (!l->rois_dev) return "null ROI list";
    if ((uintptr_t)l->rois_dev & 7) return "ROI list at an address that is no multiple of 8";
    if (l->n < 1) return "no ROI";
    if (n_streams < 1 || slots < 1) return "no frame store";
    if (fill >> 24) return "fill with a bit above 23 set";
    if ((int64_t)mb_w * 16 > 65535 || (int64_t)mb_h * 16 > 65535) return "a frame above 65535 samples a side (a tap holds a coordinate in 16 bits)";
    if (l->flags & ~(P264HIP_ROIS_AFTER | P264HIP_ROIS_BEFORE)) return "unknown flag bits";
    if (l->slot_of_stream)
        for (int i = 0; i < n_streams; i++)
            if (l->slot_of_stream[i] < -1 || l->slot_of_stream[i] >= slots) return "slot table with an entry outside -1 .. slots - 1";
    return 0;
}

int p264hip_rois_device_check(const p264hip_rois_dev_t *l, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots)
{
    return p264hip_rois_device_why_(l, r, fill, mb_w, mb_h, n_streams, slots) ? P264HIP_EINVAL : P264HIP_OK;
}
