/* pipeline_resize.c - the pipeline's two exits in device memory with a resize on them (include/p264pipe.h:
 * p264pipe_export_last_resized, p264pipe_set_sink_resized): the export kind p264hip_resize_t / p264hip_export_resized, installed
 * through pipeline_sink.h.  pipeline.c runs the sink and knows nothing of the description. */
#include <stdio.h>
#include <stdlib.h>
#include "pipeline_sink.h"

static int export_resized(p264hip_ctx *ctx, const int *streams, const int *slots, int n, const void *desc, void *dst_dev, size_t bytes)
{
    return p264hip_export_resized(ctx, streams, slots, n, (const p264hip_resize_t *)desc, dst_dev, bytes);
}

int p264pipe_export_last_resized(p264pipe *p, const p264hip_resize_t *r, void *dst_dev, size_t bytes)
{
    return p264pipe_export_last_with_(p, "p264pipe_export_last_resized", export_resized, r, dst_dev, bytes);
}

/* per-picture windows of the streams' last decoded pictures (p264hip_roi_t / p264hip_export_rois, p264hip_export_rois_aa by r->filter): slot -1 becomes the stream's slot */
int p264pipe_export_last_rois(p264pipe *p, const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, void *dst_dev, size_t bytes)
{
    if (!p || !rois || n < 1 || !r || !dst_dev) return -1;
    p264hip_roi_t *mine = (p264hip_roi_t *)malloc(sizeof *mine * (size_t)n);
    if (!mine) return -1;
    p264hip_ctx *ctx = NULL;
    int rc = 0;
    for (int i = 0; i < n && !rc; i++) {
        int slot;
        ctx = p264pipe_last_slot_(p, rois[i].stream, &slot);
        if (!ctx || rois[i].slot != -1 || slot < 0) {
            fprintf(stderr, "p264pipe_export_last_rois: ROI %d: stream %d slot %d (the slot must be -1, the stream one with a decoded picture)\n", i, rois[i].stream, rois[i].slot);
            rc = -1;
        }
        mine[i] = rois[i]; mine[i].slot = slot;
    }
    /* (the antialiased filter has entry points of its own; any other value is p264hip_export_rois' to accept or refuse) */
    if (!rc && ((r->filter == P264HIP_FILTER_BILINEAR_AA ? p264hip_export_rois_aa : p264hip_export_rois)(ctx, mine, n, r, fill, dst_dev, bytes) || p264hip_sync(ctx))) {
        fprintf(stderr, "p264pipe_export_last_rois: %s\n", p264hip_last_error()); rc = -1;
    }
    free(mine);
    return rc;
}

/* the same from an ROI list in device memory (p264hip_export_rois_device): the slot table is every stream's last decoded picture */
int p264pipe_export_last_rois_device(p264pipe *p, const p264hip_rois_dev_t *l, const p264hip_resize_t *r, uint32_t fill, void *dst_dev, size_t bytes)
{
    int slot;
    if (!p || !l || !r || !dst_dev) return -1;
    p264hip_ctx *ctx = p264pipe_last_slot_(p, 0, &slot);
    if (!ctx || l->slot_of_stream) {
        fprintf(stderr, "p264pipe_export_last_rois_device: %s\n", ctx ? "slot_of_stream must be NULL (the pipeline fills it)" : "no stream has a decoded picture yet");
        return -1;
    }
    const int n_streams = p264pipe_streams_(p);
    int32_t *table = (int32_t *)malloc(sizeof *table * (size_t)n_streams);
    if (!table) return -1;
    for (int i = 0; i < n_streams; i++) { (void)p264pipe_last_slot_(p, i, &slot); table[i] = slot < 0 ? -1 : slot; }
    p264hip_rois_dev_t mine = *l;
    mine.slot_of_stream = table;
    int rc = 0;
    /* (with P264HIP_ROIS_BEFORE the call is queued only: the next round's reconstruct is on the same stream behind it) */
    if (p264hip_export_rois_device(ctx, &mine, r, fill, dst_dev, bytes) || (!(l->flags & P264HIP_ROIS_BEFORE) && p264hip_sync(ctx))) {
        fprintf(stderr, "p264pipe_export_last_rois_device: %s\n", p264hip_last_error()); rc = -1;
    }
    free(table);
    return rc;
}

int p264pipe_set_sink_resized(p264pipe *p, const p264hip_resize_t *r, void *const *bufs, int n_bufs, size_t buf_bytes, p264pipe_sink_fn fn, void *user)
{
    if (!p) return -1;
    if (!fn) { p264pipe_sink_remove_(p); return 0; }
    int device, mb_w, mb_h;
    p264pipe_geometry_(p, &device, &mb_w, &mb_h);
    if (device < 0 || !r || !bufs || n_bufs < 1) return -1;
    /* (before the first round the frame is not known: the description is checked against the smallest frame that holds its window,
     * and p264hip_export_resized checks the window against the streams' frame in the first round) */
    const int64_t bytes = p264hip_resize_frame_bytes(r);
    const int64_t fw = bytes < 0 ? 0 : ((int64_t)r->crop_left + r->crop_width + 15) / 16, fh = bytes < 0 ? 0 : ((int64_t)r->crop_top + r->crop_height + 15) / 16;
    if (bytes < 0 || fw > 65536 || fh > 65536 || p264hip_resize_check(r, mb_w ? mb_w : (int)fw, mb_w ? mb_h : (int)fh)) {
        fprintf(stderr, "p264pipe_set_sink_resized: bad resize description\n"); return -1;
    }
    return p264pipe_sink_install_(p, "p264pipe_set_sink_resized", export_resized, r, sizeof *r, bytes, r->frame_stride, bufs, n_bufs, buf_bytes, fn, user);
}
