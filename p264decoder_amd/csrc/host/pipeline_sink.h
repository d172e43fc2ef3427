/* pipeline_sink.h - what pipeline.c offers the files that add a KIND of export to the pipeline's two exits in device memory (the sink
 * of p264pipe_run, the last picture of every stream).  An export kind is a description the pipeline copies and a function that
 * hands a batch to the HIP layer with it: pipeline.c's own is p264hip_export_t / p264hip_export_frames, pipeline_resize.c's is
 * p264hip_resize_t / p264hip_export_resized.  pipeline.c calls the function and knows nothing of the description.  Internal: not
 * part of include/. */
#ifndef P264_PIPELINE_SINK_H
#define P264_PIPELINE_SINK_H
#include "p264pipe.h"
#include "p264hip.h"

typedef int (*p264pipe_export_fn)(p264hip_ctx *ctx, const int *streams, const int *slots, int n, const void *desc, void *dst_dev, size_t bytes);

/* device (-1: parsers only) and, once the first round has run, the frame in macroblocks (0 x 0 before) */
void p264pipe_geometry_(const p264pipe *p, int *device, int *mb_w, int *mb_h);
/* the device context (NULL before the first round) and the frame-store slot of the stream's last decoded picture (-1: none yet, or no
 * such stream) */
p264hip_ctx *p264pipe_last_slot_(const p264pipe *p, int stream, int *slot);
/* the streams of the pipeline: the n_streams of its device context */
int p264pipe_streams_(const p264pipe *p);
/* the pipeline's ONE sink becomes this one: pictures of `bytes` bytes, frame_stride (0: bytes) apart, exported by ex with a copy of
 * desc into bufs[round % n_bufs] - with output order on, a delivery's pictures into bufs[delivery % n_bufs], as many as fit buf_bytes.
 * -1 (and the sink as it was) if a buffer is null or too small for a picture of every stream.  On a pipeline without a device bufs
 * may be NULL: nothing is exported there.  The caller has checked the description. */
int p264pipe_sink_install_(p264pipe *p, const char *who, p264pipe_export_fn ex, const void *desc, size_t desc_bytes, int64_t bytes, int64_t frame_stride,
                           void *const *bufs, int n_bufs, size_t buf_bytes, p264pipe_sink_fn fn, void *user);
/* no sink */
void p264pipe_sink_remove_(p264pipe *p);
/* the last picture of every stream through ex, complete when the call returns */
int p264pipe_export_last_with_(p264pipe *p, const char *who, p264pipe_export_fn ex, const void *desc, void *dst_dev, size_t bytes);
#endif
