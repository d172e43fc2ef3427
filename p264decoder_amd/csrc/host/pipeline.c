/* pipeline.c - multi-stream, multi-threaded decode pipeline on top of the two C ABIs
 * (p264parse.h: host bitstream layer, p264hip.h: MI355X reconstruction).  See include/p264pipe.h.
 *
 * Round r = the next picture of every stream that still has data.  The parser threads pull (round, stream) tasks from one
 * running counter and do NOT stop at the end of a round (round 5; until then they met at a barrier per round and the
 * stragglers of every round cost 4 - 8 % of 16 threads): a task of round R may start once the stream's picture of round R - 1 is
 * parsed and the device has finished with round R - 2, whose buffers the parser is about to reuse (it has two per stream).
 * The main thread waits for the last task of round r, hands the pictures to the GPU - asynchronous uploads out of the parsers'
 * pinned double buffers, one batched reconstruct - and waits for the marker behind them: by then the threads are well into
 * round r + 1, and that wait is what lets them into round r + 2.
 *
 * Output order (p264pipe_set_output_order): the parsers keep pictures that are not yet due in their slots, the task that completes
 * a picture copies the list of those that became due with it (the parser's own list does not survive its next picture, and the
 * parsers run ahead of the device), and the sink receives deliveries of due pictures instead of rounds (deliver).
 */
#define _GNU_SOURCE
#include <pthread.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include "p264pipe.h"
#include "p264parse.h"
#include "p264hip.h"
#include "p264_dropin.h"
#include "host_cpu.h"
#include "annexb_reader.h"
#include "pipeline_sink.h"

typedef struct {
    annexb_reader_t rd;
    const p264hip_picture_t *pic;        /* picture completed in the current round, or NULL */
    int last_slot;
} pstream_t;

struct p264pipe {
    int device, n_streams, n_threads;
    pstream_t *st;
    p264hip_ctx *ctx; int mb_w, mb_h, slots;
    /* thread pool */
    pthread_t *threads; int started;
    pthread_mutex_t mu; pthread_cond_t go, idle, turn;
    int turn_waiters;                    /* (under mu) threads blocked on `turn`: a stream's previous picture is still being parsed */
    int generation, busy, quit, max_pictures;
    int started_run;                     /* p264pipe_run has been called: the parsers' options are settled */
    /* one run: tasks t = round * n_streams + stream, taken in order */
    long long next_task;                 /* (atomic) */
    int done_rounds;                     /* rounds the device has finished with (under mu; waited for through `go`) */
    int stop;                            /* (atomic) no more tasks */
    int *parsed;                         /* [stream] rounds parsed so far (atomic) */
    int *ids, *sts, *dsts; const p264hip_picture_t **pics;   /* [stream] the round being submitted: input slots, streams, frame-store slots, pictures */
    int parsed_in_round[2];              /* tasks finished per round parity (under mu; its last one signals `idle`) */
    int failed_in_round[2];              /* a task of the round failed (under mu) */
    const p264hip_picture_t **round_pic[2];  /* [round parity][stream]: the picture a round's task produced, or NULL */
    double parse_seconds;
    /* the sink (p264pipe_set_sink; pipeline_sink.h): every round's pictures exported into the caller's device buffers by sink_export
     * with the description sink_desc (a copy) */
    p264pipe_export_fn sink_export; void *sink_desc; void **sink_bufs; int sink_n_bufs; size_t sink_bytes; p264pipe_sink_fn sink_fn; void *sink_user;
    int sink_capacity;                   /* pictures a sink buffer holds at its frame stride */
    /* output order: on / the reorder depth for every parser (< 0: the stream's); what became due with the picture a round's task
     * produced; the delivery being handed to the sink (p264pipe_delivery) and how many there were */
    int out_on, out_depth;
    p264parse_output_t *round_out[2]; int *round_n_out[2];   /* [round parity][stream][P264PARSE_MAX_OUTPUTS], [round parity][stream] */
    int *due_sts, *due_slots; p264pipe_output_t *due;        /* [n_streams * P264PARSE_MAX_OUTPUTS] the pictures due in a round, or at the flush */
    const p264pipe_output_t *delivery; int delivery_n, deliveries;
};

static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

static void *worker(void *arg)
{
    p264pipe *p = (p264pipe *)arg;
    int seen = 0;
    for (;;) {
        pthread_mutex_lock(&p->mu);
        while (p->generation == seen && !p->quit) pthread_cond_wait(&p->go, &p->mu);
        if (p->quit) { pthread_mutex_unlock(&p->mu); return NULL; }
        seen = p->generation;
        pthread_mutex_unlock(&p->mu);
        double spent = 0;
        const int S = p->n_streams;
        while (!__atomic_load_n(&p->stop, __ATOMIC_ACQUIRE)) {
            const long long t = __atomic_fetch_add(&p->next_task, 1, __ATOMIC_RELAXED);
            const int R = (int)(t / S), s = (int)(t % S);
            /* the device is done with round R - 2 (whose buffers this task writes) */
            pthread_mutex_lock(&p->mu);
            while (R > p->done_rounds + 1 && !p->stop) pthread_cond_wait(&p->go, &p->mu);
            pthread_mutex_unlock(&p->mu);
            if (__atomic_load_n(&p->stop, __ATOMIC_ACQUIRE)) break;
            /* the stream's previous picture is parsed (tasks are taken in order, so it nearly always is: a parser is not reentrant) */
            /* (a few yields, then BLOCK: with about as many threads as streams a finished thread routinely draws a stream whose
             * previous picture another thread is still parsing - spinning there burns the CPU quota the parsers need) */
            for (int spins = 0; __atomic_load_n(&p->parsed[s], __ATOMIC_ACQUIRE) < R && !__atomic_load_n(&p->stop, __ATOMIC_ACQUIRE); ) {
                if (++spins <= 32) { sched_yield(); continue; }
                pthread_mutex_lock(&p->mu);
                p->turn_waiters++;
                while (__atomic_load_n(&p->parsed[s], __ATOMIC_ACQUIRE) < R && !__atomic_load_n(&p->stop, __ATOMIC_ACQUIRE)) pthread_cond_wait(&p->turn, &p->mu);
                p->turn_waiters--;
                pthread_mutex_unlock(&p->mu);
            }
            if (__atomic_load_n(&p->stop, __ATOMIC_ACQUIRE)) break;
            double t0 = now_s();
            p->st[s].pic = annexb_reader_next(&p->st[s].rd, p->max_pictures);
            spent += now_s() - t0;
            p->round_pic[R & 1][s] = p->st[s].pic;
            if (p->out_on) p->round_n_out[R & 1][s] = p->st[s].pic ? p264parse_outputs(p->st[s].rd.parser, p->round_out[R & 1] + (size_t)s * P264PARSE_MAX_OUTPUTS, P264PARSE_MAX_OUTPUTS) : 0;
            __atomic_store_n(&p->parsed[s], R + 1, __ATOMIC_RELEASE);
            const int failed = annexb_reader_failed(&p->st[s].rd);
            pthread_mutex_lock(&p->mu);
            if (failed) p->failed_in_round[R & 1] = 1;
            if (p->turn_waiters) pthread_cond_broadcast(&p->turn);     /* (parsed[s] was stored before mu was taken: a waiter has seen it or is waiting) */
            if (++p->parsed_in_round[R & 1] == S) pthread_cond_signal(&p->idle);
            pthread_mutex_unlock(&p->mu);
        }
        pthread_mutex_lock(&p->mu);
        p->parse_seconds += spent;
        if (--p->busy == 0) pthread_cond_broadcast(&p->idle);
        pthread_mutex_unlock(&p->mu);
    }
}

/* release the threads into a run / end it and wait until every thread has left its task loop */
static void start_run(p264pipe *p)
{
    pthread_mutex_lock(&p->mu);
    p->next_task = 0; p->done_rounds = 0; p->stop = 0; p->parsed_in_round[0] = p->parsed_in_round[1] = 0; p->failed_in_round[0] = p->failed_in_round[1] = 0;
    memset(p->parsed, 0, sizeof(int) * (size_t)p->n_streams);
    p->busy = p->n_threads; p->generation++;
    pthread_cond_broadcast(&p->go);
    pthread_mutex_unlock(&p->mu);
}
static void end_run(p264pipe *p)
{
    pthread_mutex_lock(&p->mu);
    __atomic_store_n(&p->stop, 1, __ATOMIC_RELEASE);
    pthread_cond_broadcast(&p->go);
    pthread_cond_broadcast(&p->turn);
    while (p->busy) pthread_cond_wait(&p->idle, &p->mu);
    pthread_mutex_unlock(&p->mu);
}
/* wait for the last task of round r; returns whether one of them failed */
static int finish_round(p264pipe *p, int r)
{
    pthread_mutex_lock(&p->mu);
    while (p->parsed_in_round[r & 1] < p->n_streams) pthread_cond_wait(&p->idle, &p->mu);
    const int failed = p->failed_in_round[r & 1];
    p->parsed_in_round[r & 1] = 0; p->failed_in_round[r & 1] = 0;   /* (nobody starts round r + 2 before round r is through the device) */
    pthread_mutex_unlock(&p->mu);
    return failed;
}
/* the device has finished with rounds 0 .. r: the threads may start round r + 2 */
static void rounds_done(p264pipe *p, int r)
{
    pthread_mutex_lock(&p->mu);
    p->done_rounds = r + 1;
    pthread_cond_broadcast(&p->go);
    pthread_mutex_unlock(&p->mu);
}

p264pipe *p264pipe_open(int device, int n_streams, int n_threads)
{
    if (p264amd_cpu_refuse("p264pipe_open")) return NULL;
    if (n_streams < 1 || n_threads < 1) return NULL;
    if (device >= 0 && p264hip_device_count() <= device) {
        fprintf(stderr, "p264pipe_open: no HIP device %d (there is no CPU fallback for the reconstruction; device -1 runs the parsers only)\n", device);
        return NULL;
    }
    p264pipe *p = (p264pipe *)calloc(1, sizeof *p);
    if (!p) return NULL;
    p->device = device; p->n_streams = n_streams; p->n_threads = n_threads < n_streams ? n_threads : n_streams;
    p->st = (pstream_t *)calloc((size_t)n_streams, sizeof *p->st);
    p->threads = (pthread_t *)calloc((size_t)p->n_threads, sizeof *p->threads);
    p->parsed = (int *)calloc((size_t)n_streams, sizeof(int));
    p->round_pic[0] = (const p264hip_picture_t **)calloc((size_t)n_streams, sizeof(void *));
    p->round_pic[1] = (const p264hip_picture_t **)calloc((size_t)n_streams, sizeof(void *));
    p->ids = (int *)malloc(sizeof(int) * (size_t)n_streams); p->sts = (int *)malloc(sizeof(int) * (size_t)n_streams);
    p->dsts = (int *)malloc(sizeof(int) * (size_t)n_streams);
    p->pics = (const p264hip_picture_t **)malloc(sizeof(void *) * (size_t)n_streams);
    const size_t due = (size_t)n_streams * P264PARSE_MAX_OUTPUTS;
    for (int i = 0; i < 2; i++) { p->round_out[i] = (p264parse_output_t *)calloc(due, sizeof(p264parse_output_t)); p->round_n_out[i] = (int *)calloc((size_t)n_streams, sizeof(int)); }
    p->due_sts = (int *)malloc(sizeof(int) * due); p->due_slots = (int *)malloc(sizeof(int) * due); p->due = (p264pipe_output_t *)malloc(sizeof(p264pipe_output_t) * due);
    pthread_mutex_init(&p->mu, NULL); pthread_cond_init(&p->go, NULL); pthread_cond_init(&p->idle, NULL); pthread_cond_init(&p->turn, NULL);
    if (!p->st || !p->threads || !p->parsed || !p->round_pic[0] || !p->round_pic[1] || !p->ids || !p->sts || !p->dsts || !p->pics ||
        !p->round_out[0] || !p->round_out[1] || !p->round_n_out[0] || !p->round_n_out[1] || !p->due_sts || !p->due_slots || !p->due) { p264pipe_close(p); return NULL; }
    /* picture buffers in pinned host memory when they are uploaded (P264AMD_PIPE_PINNED=0 / 1 forces either kind: experiments) */
    const char *pin = getenv("P264AMD_PIPE_PINNED");
    const int pinned = pin ? atoi(pin) != 0 : device >= 0;
    for (int i = 0; i < n_streams; i++) {
        /* (the pictures go to this library's HIP layer, which knows Intra 8x8 records and reads the scaling lists and Cr's offset delta; device -1 runs
         * the same parsers, so that what it accepts, counts and times is what the device pipeline would be fed) */
        p->st[i].rd.parser = p264parse_open(P264PARSE_OPT_QUIET | P264PARSE_OPT_INTRA8X8 | P264PARSE_OPT_SCALING | P264PARSE_OPT_CR_OFFSET);
        if (!p->st[i].rd.parser) { p264pipe_close(p); return NULL; }
        if (pinned) p264parse_set_allocator(p->st[i].rd.parser, p264hip_host_alloc, p264hip_host_free);
        p->st[i].last_slot = -1;
    }
    for (int i = 0; i < p->n_threads; i++) {
        if (pthread_create(&p->threads[i], NULL, worker, p)) { p264pipe_close(p); return NULL; }
        p->started++;
    }
    return p;
}

int p264pipe_set_input(p264pipe *p, int stream, const uint8_t *annexb, int64_t size)
{
    if (!p || stream < 0 || stream >= p->n_streams || !annexb || size < 0) return -1;
    annexb_reader_set_input(&p->st[stream].rd, annexb, size);
    p->st[stream].pic = NULL;
    return 0;
}

/* round r's pictures, in stream order, into p->pics / sts / ids / dsts; returns how many */
static int collect_round(p264pipe *p, int r)
{
    int n = 0;
    for (int i = 0; i < p->n_streams; i++) {
        const p264hip_picture_t *pic = p->round_pic[r & 1][i];
        if (pic) { p->pics[n] = pic; p->sts[n] = i; p->ids[n] = i * 2 + (r & 1); p->dsts[n] = p->st[i].last_slot = pic->dst_slot; n++; }
    }
    return n;
}
/* the device context, once: geometry is known after the first picture (n: pictures of the round) */
static int ensure_context(p264pipe *p, int n)
{
    if (p->device < 0 || p->ctx) return 0;
    p->mb_w = p->pics[0]->mb_w; p->mb_h = p->pics[0]->mb_h; p->slots = p264parse_slots(p->st[p->sts[0]].rd.parser);
    /* with output order on a stream's frame store follows its own buffering (VUI, level): the context gets the largest */
    for (int k = 1; p->out_on && k < n; k++) { const int s = p264parse_slots(p->st[p->sts[k]].rd.parser); if (s > p->slots) p->slots = s; }
    if (p264hip_create(&p->ctx, p->device, p->mb_w, p->mb_h, p->n_streams, p->slots, p->n_streams * 2)) {
        fprintf(stderr, "p264pipe_run: %s\n", p264hip_last_error()); return -1;
    }
    return 0;
}
/* ---- output order ----
 * one stream's due pictures appended to the list of due pictures */
static int add_due(p264pipe *p, int n, int stream, const p264parse_output_t *out, int n_out)
{
    for (int k = 0; k < n_out; k++, n++) {
        p->due_sts[n] = stream; p->due_slots[n] = out[k].slot;
        p->due[n].stream = stream; p->due[n].poc = out[k].poc; p->due[n].decode_index = out[k].decode_index; p->due[n].flags = out[k].flags;
    }
    return n;
}
/* the pictures that became due in round r, by stream and in output order within a stream; returns how many */
static int collect_due(p264pipe *p, int r)
{
    int n = 0;
    for (int i = 0; i < p->n_streams; i++)
        if (p->round_pic[r & 1][i]) n = add_due(p, n, i, p->round_out[r & 1] + (size_t)i * P264PARSE_MAX_OUTPUTS, p->round_n_out[r & 1][i]);
    return n;
}
/* ... and what every stream's parser still holds, at the end of a run (the threads have left their task loop) */
static int collect_flush(p264pipe *p)
{
    int n = 0;
    p264parse_output_t out[P264PARSE_MAX_OUTPUTS];
    for (int i = 0; i < p->n_streams; i++) n = add_due(p, n, i, out, p264parse_flush(p->st[i].rd.parser, out, P264PARSE_MAX_OUTPUTS));
    return n;
}
/* The n due pictures to the sink, as many deliveries as the buffers' capacity makes of them: delivery d is exported into
 * bufs[d % n_bufs] behind everything queued so far (the round's reconstruct), and fn is called after the wait for the marker
 * behind the export - before the next delivery is exported, so no buffer is written before its callback has returned.  Without a
 * device nothing is exported and fn gets dev = NULL. */
static int deliver(p264pipe *p, int n, p264pipe_stats_t *S)
{
    for (int at = 0; at < n; ) {
        const int k = n - at < p->sink_capacity ? n - at : p->sink_capacity;
        void *buf = p->ctx ? p->sink_bufs[p->deliveries % p->sink_n_bufs] : NULL;
        if (p->ctx) {
            const double s0 = now_s();
            int rc = p->sink_export(p->ctx, p->due_sts + at, p->due_slots + at, k, p->sink_desc, buf, p->sink_bytes);
            const int marker = rc ? -1 : p264hip_marker(p->ctx);
            S->submit_seconds += now_s() - s0;
            if (rc || marker < 0) { fprintf(stderr, "p264pipe_run: %s\n", p264hip_last_error()); return -1; }
            const double w0 = now_s();
            if (p264hip_marker_wait(p->ctx, marker)) return -1;
            S->wait_device_seconds += now_s() - w0;
        }
        p->delivery = p->due + at; p->delivery_n = k;
        p->sink_fn(p->sink_user, p->deliveries++, k, p->due_sts + at, buf);
        p->delivery = NULL; p->delivery_n = 0;
        at += k;
    }
    return 0;
}

/* round r's n pictures to the device: uploads, one batched reconstruct, the sink's export behind the round's kernels, and the
 * wait for the marker behind all of it.  With output order on the sink gets the round's due pictures instead (deliver), behind
 * that wait. */
static int submit_round(p264pipe *p, int r, int n, p264pipe_stats_t *S)
{
    const double s0 = now_s();
    int rc = 0;
    for (int k = 0; k < n && !rc; k++) {
        if (p->pics[k]->mb_w != p->mb_w || p->pics[k]->mb_h != p->mb_h) { fprintf(stderr, "p264pipe_run: stream %d has a different picture size\n", p->sts[k]); rc = -1; }
        else if (p264hip_upload_async(p->ctx, p->ids[k], p->pics[k])) { fprintf(stderr, "p264pipe_run: %s\n", p264hip_last_error()); rc = -1; }
        else S->bytes_uploaded += (int64_t)p->mb_w * p->mb_h * (16 + 64 + 4 + 16) + (int64_t)p->pics[k]->n_coef_blocks * 32;
    }
    if (!rc && p264hip_reconstruct(p->ctx, p->ids, p->sts, n)) { fprintf(stderr, "p264pipe_run: %s\n", p264hip_last_error()); rc = -1; }
    void *sink = p->sink_fn && !p->out_on ? p->sink_bufs[r % p->sink_n_bufs] : NULL;       /* the round's pictures, behind its kernels */
    if (!rc && sink && p->sink_export(p->ctx, p->sts, p->dsts, n, p->sink_desc, sink, p->sink_bytes)) { fprintf(stderr, "p264pipe_run: %s\n", p264hip_last_error()); rc = -1; }
    int marker = -1;
    if (!rc) { marker = p264hip_marker(p->ctx); if (marker < 0) rc = -1; }
    S->submit_seconds += now_s() - s0;
    if (rc) return rc;
    /* the parsers reuse round r's buffers in round r + 2: its uploads must have been consumed (the threads are in round r + 1) */
    const double w0 = now_s();
    if (p264hip_marker_wait(p->ctx, marker)) return -1;
    S->wait_device_seconds += now_s() - w0;
    if (sink) p->sink_fn(p->sink_user, r, n, p->sts, sink);
    return 0;
}

int p264pipe_run(p264pipe *p, int max_pictures, p264pipe_stats_t *stats)
{
    if (!p) return -1;
    for (int i = 0; i < p->n_streams; i++) if (!p->st[i].rd.in) { fprintf(stderr, "p264pipe_run: stream %d has no input\n", i); return -1; }
    p->max_pictures = max_pictures; p->parse_seconds = 0; p->deliveries = 0;
    if (!p->started_run) for (int i = 0; i < p->n_streams; i++) (void)p264parse_set_output_order(p->st[i].rd.parser, p->out_on, p->out_depth);
    p->started_run = 1;
    p264pipe_stats_t S; memset(&S, 0, sizeof S);                /* (the main thread's waits: P264AMD_PIPE_DEBUG=1 prints them) */
    int rc = 0;
    const double t0 = now_s();
    start_run(p);
    for (int r = 0;; r++) {
        { const double w0 = now_s(); if (finish_round(p, r)) rc = -1; S.wait_parse_seconds += now_s() - w0; }
        const int n = collect_round(p, r);
        if (n == 0 || rc) break;
        S.rounds++; S.pictures += n;
        if ((rc = ensure_context(p, n)) || (p->ctx && (rc = submit_round(p, r, n, &S)))) break;
        if (p->out_on && p->sink_fn && (rc = deliver(p, collect_due(p, r), &S))) break;
        rounds_done(p, r);
    }
    end_run(p);
    /* the end of the streams (or max_pictures): what still waits is due now */
    if (p->out_on && !rc) { const int n = collect_flush(p); if (p->sink_fn) rc = deliver(p, n, &S); }
    if (p->ctx && p264hip_sync(p->ctx)) { fprintf(stderr, "p264pipe_run: %s\n", p264hip_last_error()); rc = -1; }
    S.seconds = now_s() - t0; S.parse_seconds = p->parse_seconds; S.streams = p->n_streams; S.threads = p->n_threads;
    if (getenv("P264AMD_PIPE_DEBUG"))
        fprintf(stderr, "p264pipe_run: %d rounds, %.3f s: main thread waited %.3f s for the parsers, %.3f s for the device, submitted for %.3f s; parser threads %.3f s in all (%d threads)\n",
                S.rounds, S.seconds, S.wait_parse_seconds, S.wait_device_seconds, S.submit_seconds, p->parse_seconds, p->n_threads);
    for (int i = 0; i < p->n_streams; i++) S.bytes += p->st[i].rd.pos;
    if (stats) *stats = S;
    return rc;
}

int p264pipe_frame_size(p264pipe *p, int *width, int *height)
{
    if (!p || !p->mb_w) return -1;
    if (width) *width = p->mb_w * 16;
    if (height) *height = p->mb_h * 16;
    return 0;
}

int p264pipe_read_frame(p264pipe *p, int stream, uint8_t *y, int y_stride, uint8_t *u, uint8_t *v, int c_stride)
{
    if (!p || !p->ctx || stream < 0 || stream >= p->n_streams || p->st[stream].last_slot < 0) return -1;
    return p264hip_read_frame(p->ctx, stream, p->st[stream].last_slot, y, y_stride, u, v, c_stride) ? -1 : 0;
}

int p264pipe_crop(p264pipe *p, int *left, int *top, int *width, int *height)
{
    return p ? p264parse_crop(p->st[0].rd.parser, left, top, width, height) : -1;
}

/* the export kind of this file: p264hip_export_t through p264hip_export_frames */
static int export_plain(p264hip_ctx *ctx, const int *streams, const int *slots, int n, const void *desc, void *dst_dev, size_t bytes)
{
    return p264hip_export_frames(ctx, streams, slots, n, (const p264hip_export_t *)desc, dst_dev, bytes);
}

void p264pipe_geometry_(const p264pipe *p, int *device, int *mb_w, int *mb_h)
{
    *device = p->device; *mb_w = p->mb_w; *mb_h = p->mb_h;
}

p264hip_ctx *p264pipe_last_slot_(const p264pipe *p, int stream, int *slot)
{
    *slot = p->ctx && stream >= 0 && stream < p->n_streams ? p->st[stream].last_slot : -1;
    return p->ctx;
}

int p264pipe_streams_(const p264pipe *p) { return p->n_streams; }

int p264pipe_export_last_with_(p264pipe *p, const char *who, p264pipe_export_fn ex, const void *desc, void *dst_dev, size_t bytes)
{
    if (!p || !p->ctx || !desc || !dst_dev) return -1;
    int *sts = (int *)malloc(sizeof(int) * 2 * (size_t)p->n_streams);
    if (!sts) return -1;
    int rc = 0;
    for (int i = 0; i < p->n_streams; i++) {
        if (p->st[i].last_slot < 0) rc = -1;
        sts[i] = i; sts[p->n_streams + i] = p->st[i].last_slot;
    }
    if (!rc && (ex(p->ctx, sts, sts + p->n_streams, p->n_streams, desc, dst_dev, bytes) || p264hip_sync(p->ctx))) {
        fprintf(stderr, "%s: %s\n", who, p264hip_last_error()); rc = -1;
    }
    free(sts);
    return rc;
}

int p264pipe_export_last(p264pipe *p, const p264hip_export_t *e, void *dst_dev, size_t bytes)
{
    return p264pipe_export_last_with_(p, "p264pipe_export_last", export_plain, e, dst_dev, bytes);
}

void p264pipe_sink_remove_(p264pipe *p)
{
    free(p->sink_bufs); free(p->sink_desc);
    p->sink_bufs = NULL; p->sink_desc = NULL; p->sink_fn = NULL; p->sink_export = NULL; p->sink_n_bufs = 0;
}

int p264pipe_sink_install_(p264pipe *p, const char *who, p264pipe_export_fn ex, const void *desc, size_t desc_bytes, int64_t bytes, int64_t frame_stride,
                           void *const *bufs, int n_bufs, size_t buf_bytes, p264pipe_sink_fn fn, void *user)
{
    /* (parsers only: nothing is exported, so there need be no buffers - buf_bytes still says how many pictures a delivery holds) */
    const int no_bufs = p && p->device < 0 && !bufs;
    if (no_bufs) n_bufs = 0;
    if (!p || !ex || !desc || !fn || (!no_bufs && (!bufs || n_bufs < 1)) || bytes < 1) return -1;
    for (int i = 0; i < n_bufs; i++) if (!bufs[i]) return -1;
    /* every round may bring a picture of every stream */
    const int64_t stride = frame_stride ? frame_stride : bytes;
    if (stride > (INT64_MAX - bytes) / p->n_streams || (uint64_t)buf_bytes < (uint64_t)(p->n_streams - 1) * (uint64_t)stride + (uint64_t)bytes) {
        fprintf(stderr, "%s: %d pictures %lld bytes apart do not fit %zu bytes\n", who, p->n_streams, (long long)stride, buf_bytes); return -1;
    }
    void **copy = (void **)malloc(sizeof(void *) * (size_t)(n_bufs ? n_bufs : 1));
    void *d = malloc(desc_bytes);
    if (!copy || !d) { free(copy); free(d); return -1; }
    memcpy(copy, bufs, sizeof(void *) * (size_t)n_bufs);
    memcpy(d, desc, desc_bytes);
    p264pipe_sink_remove_(p);
    const uint64_t more = ((uint64_t)buf_bytes - (uint64_t)bytes) / (uint64_t)stride;      /* pictures behind the first */
    p->sink_capacity = more < (uint64_t)INT32_MAX ? (int)more + 1 : INT32_MAX;
    p->sink_export = ex; p->sink_desc = d; p->sink_bufs = copy; p->sink_n_bufs = n_bufs; p->sink_bytes = buf_bytes; p->sink_fn = fn; p->sink_user = user;
    return 0;
}

int p264pipe_set_sink(p264pipe *p, const p264hip_export_t *e, void *const *bufs, int n_bufs, size_t buf_bytes, p264pipe_sink_fn fn, void *user)
{
    if (!p) return -1;
    if (!fn) { p264pipe_sink_remove_(p); return 0; }
    if ((p->device < 0 && !p->out_on) || !e || (p->device >= 0 && (!bufs || n_bufs < 1))) return -1;
    /* (the frame itself is known at the first round: p264hip_export_frames checks the window) */
    const int64_t bytes = p264hip_export_frame_bytes(e);
    if (bytes < 0 || (p->mb_w && p264hip_export_check(e, p->mb_w, p->mb_h)) || e->frame_stride < 0 || (e->frame_stride && e->frame_stride < bytes)) {
        fprintf(stderr, "p264pipe_set_sink: bad export description\n"); return -1;
    }
    return p264pipe_sink_install_(p, "p264pipe_set_sink", export_plain, e, sizeof *e, bytes, e->frame_stride, bufs, n_bufs, buf_bytes, fn, user);
}

int p264pipe_set_output_order(p264pipe *p, int on, int reorder_depth)
{
    if (!p || p->started_run || reorder_depth > P264HIP_MAX_REFS) return -1;
    p->out_on = on != 0; p->out_depth = reorder_depth < 0 ? -1 : reorder_depth;
    return 0;
}

const p264pipe_output_t *p264pipe_delivery(p264pipe *p, int *n)
{
    if (n) *n = p ? p->delivery_n : 0;
    return p ? p->delivery : NULL;
}

int64_t p264pipe_stream_pictures(p264pipe *p, int stream)
{
    return (p && stream >= 0 && stream < p->n_streams) ? p->st[stream].rd.pictures : -1;
}

void p264pipe_close(p264pipe *p)
{
    if (!p) return;
    pthread_mutex_lock(&p->mu); p->quit = 1; pthread_cond_broadcast(&p->go); pthread_mutex_unlock(&p->mu);
    for (int i = 0; i < p->started; i++) pthread_join(p->threads[i], NULL);
    if (p->ctx) { (void)p264hip_sync(p->ctx); }
    if (p->st) for (int i = 0; i < p->n_streams; i++) annexb_reader_close(&p->st[i].rd);
    if (p->ctx) p264hip_destroy(p->ctx);
    pthread_mutex_destroy(&p->mu); pthread_cond_destroy(&p->go); pthread_cond_destroy(&p->idle); pthread_cond_destroy(&p->turn);
    free(p->parsed); free((void *)p->round_pic[0]); free((void *)p->round_pic[1]);
    for (int i = 0; i < 2; i++) { free(p->round_out[i]); free(p->round_n_out[i]); }
    free(p->due_sts); free(p->due_slots); free(p->due);
    free(p->sink_bufs); free(p->sink_desc); free(p->ids); free(p->sts); free(p->dsts); free((void *)p->pics);
    free(p->st); free(p->threads); free(p);
}
