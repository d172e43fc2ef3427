/* p264pipe.h - C ABI of the multi-stream decode pipeline.
 *
 * N Annex-B streams are decoded side by side: a pool of host threads runs the CAVLC parsers (one stream at a
 * time per thread, the part of the decoder that stays on the CPU), and the next picture of every stream goes to the
 * MI355X as ONE batch (p264hip_upload_async + p264hip_reconstruct).  The parsers write their picture arrays straight
 * into pinned memory (registered huge pages, p264hip_host_alloc), so the uploads are plain DMA; while the GPU works on round r
 * the threads already parse round r+1 - they do not stop at the end of a round: a stream's next picture may be parsed as
 * soon as its previous one is and the device has finished with the round before that (whose buffers the parser reuses).  Output pictures stay in HBM (the frame stores of p264hip); p264pipe_read_frame fetches the last one of a
 * stream to the host, p264pipe_export_last hands the last one of every stream on in device memory, and a sink
 * (p264pipe_set_sink) receives every round's pictures there while the run goes on - in decode order, or in display order (p264pipe_set_output_order).  There is no counterpart in the reference (its decoder is single-stream, single-threaded,
 * p264decoder.c:164-381); the per-stream behaviour is that of p264_decoder_decode.
 *
 * device < 0 runs the parsers only (no GPU is touched): the host-side ceiling of the pipeline.
 */
#ifndef P264PIPE_H
#define P264PIPE_H
#include <stdint.h>
#include <stddef.h>
#include "p264hip.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct p264pipe p264pipe;

typedef struct {
    int64_t pictures;            /* pictures decoded, all streams */
    int64_t bytes;               /* Annex-B bytes consumed */
    double  seconds;             /* wall clock of p264pipe_run */
    double  parse_seconds;       /* summed over the threads: time inside the parsers */
    double  submit_seconds;      /* host time spent enqueuing uploads and launches */
    int     rounds, streams, threads;
    int     reserved;
    int64_t bytes_uploaded;      /* parsed-picture bytes copied host -> HBM (0 when the parsers run alone) */
    double  wait_parse_seconds;  /* the main thread's wait for the last parse task of a round, summed (parser-bound run: most of `seconds`) */
    double  wait_device_seconds; /* ... and for the device to be through a round's uploads and kernels (a GPU-bound run shows here) */
} p264pipe_stats_t;

p264pipe *p264pipe_open(int device, int n_streams, int n_threads);
/* The stream's bytes are borrowed until p264pipe_close.  All streams must have the same picture size. */
int  p264pipe_set_input(p264pipe *p, int stream, const uint8_t *annexb, int64_t size);
/* Decode every stream to its end (or max_pictures per stream, 0 = no limit).  0 on success, -1 on error. */
int  p264pipe_run(p264pipe *p, int max_pictures, p264pipe_stats_t *stats);
/* Last decoded picture of a stream (MB-aligned planes, as p264_decoder_decode returns them). */
int  p264pipe_frame_size(p264pipe *p, int *width, int *height);
int  p264pipe_read_frame(p264pipe *p, int stream, uint8_t *y, int y_stride, uint8_t *u, uint8_t *v, int c_stride);
int64_t p264pipe_stream_pictures(p264pipe *p, int stream);

/* ---- pictures handed on in device memory (p264hip_export_t, include/p264hip.h: formats, layouts, the RGB arithmetic) ----
 * The display window of stream 0's SPS (p264parse_crop), for the caller to put into a p264hip_export_t.  -1 before a slice of
 * stream 0 has been parsed. */
int  p264pipe_crop(p264pipe *p, int *left, int *top, int *width, int *height);
/* The last decoded picture of EVERY stream, stream i at dst_dev + i * frame_stride, in one launch; complete when the call
 * returns.  -1 if a stream has no picture yet, or where p264hip_export_frames refuses. */
int  p264pipe_export_last(p264pipe *p, const p264hip_export_t *e, void *dst_dev, size_t bytes);
/* A sink receives every picture of a run, round by round.  Inside p264pipe_run the pictures of round r are exported into
 * bufs[r % n_bufs] (device memory of the caller, buf_bytes each) right behind the round's p264hip_reconstruct, picture k of the
 * round at k * frame_stride; fn is called on the thread that runs p264pipe_run, after the wait for the round's marker - the
 * buffer is complete - with the round's number, its n pictures' streams (ascending; a stream that has ended is absent) and the
 * buffer.  The buffer is written again n_bufs rounds later: whatever still reads it then (work the callback queued on another
 * stream) is the caller's to wait for.  Pictures arrive in DECODE order unless p264pipe_set_output_order says
 * otherwise (below).  A buf_bytes too small for n_streams pictures is refused here, a window that does
 * not fit the streams' frame at the first round (p264pipe_run fails): never by writing short.  fn = NULL takes the sink away.
 * The description and the pointers are copied; the buffers are borrowed until the sink is replaced or the pipeline closed. */
typedef void (*p264pipe_sink_fn)(void *user, int round, int n, const int *streams, void *dev);
int  p264pipe_set_sink(p264pipe *p, const p264hip_export_t *e, void *const *bufs, int n_bufs, size_t buf_bytes, p264pipe_sink_fn fn, void *user);
/* The same two exits with a resize on them (p264hip_resize_t, include/p264hip.h: a window of each picture resized, as bytes or -
 * RGB formats - normalised floats; p264hip_export_resized).  The description's `filter` goes through unchanged: with
 * P264HIP_FILTER_BILINEAR_AA every round's pictures, and the last ones, are resized by the antialiased filter (at most 32:1; a
 * description above that is refused here as p264hip_resize_check refuses it).  A pipeline has ONE sink: setting either kind replaces the other, and
 * fn = NULL to either call takes it away.  p264pipe_export_last and p264pipe_set_sink behave as before. */
int  p264pipe_export_last_resized(p264pipe *p, const p264hip_resize_t *r, void *dst_dev, size_t bytes);
int  p264pipe_set_sink_resized(p264pipe *p, const p264hip_resize_t *r, void *const *bufs, int n_bufs, size_t buf_bytes, p264pipe_sink_fn fn, void *user);
/* Windows of the streams' last decoded pictures, each resized into a rectangle of the output (p264hip_roi_t / p264hip_export_rois,
 * include/p264hip.h), ROI i at dst_dev + i * frame_stride, in one call; complete when the call returns.  rois[i].slot must be -1:
 * it stands for the last DECODED picture of rois[i].stream, what p264pipe_read_frame and p264pipe_export_last mean by "last".  A
 * stream may be named any number of times, or not at all.  -1 where a named stream has no picture yet, a slot is not -1, or
 * p264hip_export_rois refuses.  With r->filter P264HIP_FILTER_BILINEAR_AA the call goes to p264hip_export_rois_aa, the antialiased
 * filter with its limit of 32:1 per ROI, and fails where that one refuses.
 * It may be called between runs AND FROM INSIDE A SINK CALLBACK.  The callback runs on the thread that runs p264pipe_run, after the
 * round's marker and before the next round's reconstruct is queued: with a decode-order sink the pictures the callback has just
 * received are exactly the "last decoded" ones of their streams.  That is the detect-then-crop cascade: the sink hands round r's
 * pictures to a detector, and the callback asks for round r's boxes at the second model's input size before round r + 1 overwrites
 * anything.  With output order on (below) "last decoded" is NOT what a delivery carries - a delivery's pictures were decoded rounds
 * ago -, so this call is of no use to a delivery's callback; deliveries in output order as ROI sources, and a sink that takes ROIs,
 * are not built. */
int  p264pipe_export_last_rois(p264pipe *p, const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, void *dst_dev, size_t bytes);
/* The same from an ROI LIST IN DEVICE MEMORY (p264hip_export_rois_device, include/p264hip.h: one entry for both filters).  The
 * ROIs carry slot -1; the pipeline fills the slot table from every stream's last decoded picture, so l->slot_of_stream must be NULL.
 * A stream without a picture yet refuses nothing: its ROIs get the status P264HIP_ROI_NO_PICTURE and their pictures are not
 * written, as any invalid ROI's.  -1 before the first round (there is no device context), for a slot table, and for what
 * p264hip_export_rois_device refuses.  The rest of l passes through.  Callable between runs and from inside a decode-order sink's
 * callback, as its sibling.  Without P264HIP_ROIS_BEFORE it is complete on return; with it the call is queued only, before_stream
 * waits for it, and the next round's reconstruct is on the context's stream behind it. */
int  p264pipe_export_last_rois_device(p264pipe *p, const p264hip_rois_dev_t *l, const p264hip_resize_t *r, uint32_t fill, void *dst_dev, size_t bytes);

/* ---- pictures in OUTPUT (display) order ----
 * on != 0: every stream's parser runs the output process of H.264 C.4 (p264parse_set_output_order, include/p264parse.h: the rule,
 * D and R; reorder_depth < 0 takes each stream's own depth, 0 .. 16 overrides it for all of them - 0 is decode order, one picture
 * per picture).  Pictures that are decoded but not yet due stay in their frame-store slots; the context gets the largest frame
 * store any stream asks for (at most 17 slots).  Only before the first p264pipe_run; -1 afterwards.
 *
 * The sink - either kind, one sink as before - then receives DELIVERIES instead of rounds.  Behind round r's reconstruct the
 * pictures that became due in round r go out in one export into bufs[d % n_bufs], d counting the deliveries of the run from 0:
 * ordered by stream ascending and in output order within a stream, picture k at k * frame_stride.  fn(user, d, n, streams, dev) is
 * called after the wait for the marker behind the export; `streams` may name a stream several times.  A round in which nothing
 * became due makes no call.  A round with more due pictures than a buffer holds (the pictures that fit buf_bytes at frame_stride;
 * setting the sink still asks for n_streams at least) goes out as several deliveries.  A buffer is never written again before
 * its own callback has returned.  After the last round - the end of the streams, or max_pictures - every stream is flushed and what
 * still waited is delivered the same way, ascending by order count within a stream.
 *
 * p264pipe_delivery, inside the callback: what the delivery's n pictures are (NULL and 0 outside).
 *
 * With device < 0 and output order on, p264pipe_set_sink is accepted (after p264pipe_set_output_order; bufs may be NULL, buf_bytes
 * and the description still give the capacity) and fn is called with dev = NULL: nothing is exported, the order and the grouping are
 * what the device pipeline would deliver.  With output order off the sink stays refused there, as before.
 *
 * p264pipe_export_last and p264pipe_read_frame keep meaning the last DECODED picture of a stream: its slot is intact after the
 * final flush, since nothing is decoded behind it. */
typedef struct {
    int stream;          /* which input */
    int poc;             /* picture order count, as the stream's frame store records it */
    int decode_index;    /* which of the stream's decoded pictures, from 0 */
    int flags;           /* P264PARSE_OUT_* of include/p264parse.h (bit 0: an IDR picture) */
} p264pipe_output_t;
int  p264pipe_set_output_order(p264pipe *p, int on, int reorder_depth);
const p264pipe_output_t *p264pipe_delivery(p264pipe *p, int *n);
void p264pipe_close(p264pipe *p);

#ifdef __cplusplus
}
#endif
#endif
