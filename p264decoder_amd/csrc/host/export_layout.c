/* export_layout.c - the layout of an exported picture (include/p264hip.h: p264hip_export_t) and the checks every export runs
 * before anything is queued.  Pure host code, no device involved; the kernel is csrc/hip/kernel_export.h. */
#include "p264hip.h"

static int is_rgb(int format) { return format == P264HIP_FMT_RGB24 || format == P264HIP_FMT_RGBP; }

/* why the description is refused on its own (NULL: it is not); *pitch, *bytes: the pitch in bytes and one picture's bytes */
static const char *describe(const p264hip_export_t *e, int64_t *pitch, int64_t *bytes)
{
    if (!e) return "null description";
    if (e->format < P264HIP_FMT_I420 || e->format > P264HIP_FMT_RGBP) return "unknown format";
    if (e->matrix != P264HIP_MATRIX_BT601 && e->matrix != P264HIP_MATRIX_BT709) return "unknown matrix";
    if (e->full_range != 0 && e->full_range != 1) return "full_range is neither 0 nor 1";
    if (!is_rgb(e->format) && (e->matrix || e->full_range)) return "matrix / full_range set on a YUV format";
    if (e->crop_left < 0 || e->crop_top < 0 || e->width < 1 || e->height < 1) return "window with a negative offset or without samples";
    if ((e->crop_left | e->crop_top | e->width | e->height) & 1) return "window with an odd member";
    const int64_t tight = e->format == P264HIP_FMT_RGB24 ? 3 * (int64_t)e->width : (int64_t)e->width;
    const int64_t p = e->pitch ? (int64_t)e->pitch : tight;
    if (p < tight) return "pitch below the tight pitch";
    if (e->format == P264HIP_FMT_I420 && (p & 1)) return "odd pitch for I420";
    const int64_t h = e->height;
    *pitch = p;
    *bytes = e->format == P264HIP_FMT_RGB24 ? p * h : e->format == P264HIP_FMT_RGBP ? 3 * p * h : p * h + p * (h / 2);
    return 0;
}

/* the same with the frame and the stride (what p264hip_export_frames reports through p264hip_last_error) */
const char *p264hip_export_why_(const p264hip_export_t *e, int mb_w, int mb_h)
{
    int64_t pitch, bytes;
    const char *why = describe(e, &pitch, &bytes);
    if (why) return why;
    if (mb_w < 1 || mb_h < 1) return "no frame";
    if ((int64_t)e->crop_left + e->width > (int64_t)mb_w * 16 || (int64_t)e->crop_top + e->height > (int64_t)mb_h * 16) return "window leaves the frame";
    if (e->frame_stride < 0 || (e->frame_stride && e->frame_stride < bytes)) return "frame_stride below the picture's bytes";
    return 0;
}

int64_t p264hip_export_frame_bytes(const p264hip_export_t *e)
{
    int64_t pitch, bytes;
    return describe(e, &pitch, &bytes) ? P264HIP_EINVAL : bytes;
}

int p264hip_export_check(const p264hip_export_t *e, int mb_w, int mb_h)
{
    return p264hip_export_why_(e, mb_w, mb_h) ? P264HIP_EINVAL : P264HIP_OK;
}
