/* fanout.c - stream fan-out over a point-to-point transport (include/p264fan.h): protocol, root and worker loops, the
 * TCP transport and the default (MI355X) backend.  The RCCL transport lives next to the HIP code (csrc/hip/fan_rccl.hip). */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <errno.h>
#include <time.h>
#include <unistd.h>
#include <pthread.h>
#include <sys/socket.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <arpa/inet.h>
#include "p264fan.h"
#include "p264parse.h"
#include "p264_dropin.h"
#include "host_cpu.h"
#include "annexb_reader.h"

static __thread char g_err[512] = "";
static int fail(const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return -1;
}
const char *p264fan_last_error(void) { return g_err; }
/* (for the RCCL transport in csrc/hip/fan_rccl.hip: same message slot) */
int p264fan_set_error(const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return -1;
}
/* keep the error text across calls that may overwrite it */
typedef struct { char text[sizeof g_err]; } err_keep_t;
static void err_keep(err_keep_t *k) { memcpy(k->text, g_err, sizeof g_err); }
static void err_restore(const err_keep_t *k) { memcpy(g_err, k->text, sizeof g_err); }
/* fit *buf to `need` bytes (contents are not kept): grown with a quarter to spare, never shrunk.  -1 = out of memory, the
 * buffer is gone then */
static int fit_buffer(uint8_t **buf, size_t *cap, size_t need)
{
    if (need <= *cap) return 0;
    free(*buf); *cap = 0;
    *buf = (uint8_t *)malloc(need + need / 4);
    if (!*buf) return -1;
    *cap = need + need / 4;
    return 0;
}
static double now_s(void) { struct timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec; }

/* ---------------------------------------------------------------- messages -------------- */
/* Per round and worker, always in this order and always of these sizes (a fixed-size exchange keeps both sides in step
 * whatever fails):
 *   root -> worker   fan_ctrl_t                      how many pictures follow and their sizes, or FAN_FINISHED
 *   root -> worker   n fan_head_t in one message     the pictures' descriptors (host memory: the worker lays its input slots out
 *                                                    from them)
 *   root -> worker   n packed pictures               each ONE block in the layout of an input slot (p264hip_input_layout_t); a worker
 *                                                    whose transport and backend have the device road receives it straight into the
 *                                                    slot (recv_dev), otherwise into host memory
 *   worker -> root   fan_status_t                    0, or what failed on the worker (it keeps serving: the root ends the job
 *                                                    with FAN_FINISHED at the next round boundary)
 *   worker -> root   n frames of MB-aligned I420     only when the status is 0
 * Each line is a step of the two loops further down, named after it: the root's root_scatter sends the first three (the
 * FAN_FINISHED block: root_finish) and its root_gather receives the last two; the worker receives them in worker_recv_ctrl,
 * worker_recv_heads and worker_recv_pictures and sends both answers in worker_answer.  What the steps keep, by number in their
 * comments:
 *   1. Everything on the root that can fail without the transport failing (parse, allocation, packing, opening the backend)
 *      happens BEFORE the round's control block goes out.
 *   2. A failure of the root's own reconstruction is reported only after the round's gather.  With 1: the root never leaves
 *      a worker in the middle of a round.
 *   3. A worker always receives the round's pictures, whatever state it is in; what fails there becomes the round's status, and
 *      the first failure every later round's.  FAN_FINISHED only arrives where a worker expects a control block.
 *   4. A rank that cannot stay in step (`fatal`) aborts the transport and keeps its error text.  A plain transport failure does
 *      not: there is nothing left to say - both transports' calls return an error then (TCP: peer closed).
 *   5. Order and sizes of the messages are fixed: the table above, the structs below.
 *   6. The error texts are part of the interface (callers and tests match on them).
 *   7. Every field of p264fan_stats_t is accumulated by one step, named in that step's comment. */
#define FAN_MAX_PER_ROUND 64            /* pictures one worker takes per round */
#define FAN_FINISHED (-1)
typedef struct {                        /* root -> worker, once per round, fixed size */
    int32_t n;                          /* pictures that follow, or FAN_FINISHED */
    int32_t mb_w, mb_h, slots, n_local_streams;
    uint32_t bytes[FAN_MAX_PER_ROUND];  /* size of each packed picture */
} fan_ctrl_t;
typedef struct {                        /* worker -> root, once per round, fixed size */
    int32_t rc, n;
    int32_t device_road;                /* this round's pictures and planes never touched the worker's host memory */
    char msg[244];
} fan_status_t;
typedef struct {                        /* descriptor of a packed picture (travels apart from the arrays) */
    uint32_t magic;
    int32_t  local_stream;
    p264hip_picture_t desc;             /* pointers are meaningless on the wire */
    uint32_t n_mb;
} fan_head_t;
#define FAN_MAGIC 0x70464e33u
/* the arrays of a picture as one block in the layout of an input slot; the head beside it */
static size_t packed_size(const p264hip_picture_t *p)
{
    p264hip_input_layout_t L;
    return p264hip_input_layout(p, &L) ? 0 : L.bytes;
}
static int pack_picture(fan_head_t *h, uint8_t *dst, size_t cap, int local_stream, const p264hip_picture_t *p)
{
    memset(h, 0, sizeof *h);
    h->magic = FAN_MAGIC; h->local_stream = local_stream; h->desc = *p; h->n_mb = (uint32_t)((size_t)p->mb_w * p->mb_h);
    h->desc.mb = NULL; h->desc.mv = NULL; h->desc.ref_idx = NULL; h->desc.i4modes = NULL; h->desc.coefs = NULL; h->desc.mv_l1 = NULL; h->desc.ref_idx_l1 = NULL;
    return p264hip_pack_input(p, dst, cap) < 0 ? fail("a parsed picture does not pack (inconsistent macroblock records)") : 0;
}
static int check_head(const fan_head_t *h, size_t bytes)
{
    if (h->magic != FAN_MAGIC || h->desc.mb_w < 1 || h->desc.mb_h < 1 || h->n_mb != (uint32_t)(h->desc.mb_w * h->desc.mb_h)) return fail("packed picture: bad header");
    if (packed_size(&h->desc) != bytes) return fail("packed picture: %zu bytes, its header says %zu", bytes, packed_size(&h->desc));
    return 0;
}
/* the picture described by a head and its block, the arrays pointing into the block */
static int unpack_picture(const fan_head_t *h, const uint8_t *body, size_t bytes, p264hip_picture_t *out, int *local_stream)
{
    if (check_head(h, bytes)) return -1;
    *local_stream = h->local_stream;
    return p264hip_unpack_input(&h->desc, body, bytes, out) ? fail("packed picture: bad layout") : 0;
}

/* ---------------------------------------------------------------- default backend ------- */
/* The MI355X path of this library.  reconstruct() only uploads (asynchronously) and NOTES the picture; sync() reconstructs
 * everything noted since the last sync() as ONE batch - the pictures of a round belong to different local streams, and the
 * kernels are built for batches: a round of 64 pictures as 64 single-picture batches would run the GPU nearly empty, one
 * launch latency after the other - then converts and downloads the frames and waits once.  The picture's arrays and the
 * output buffers must stay untouched until sync() (the fan-out keeps a round's messages and frames alive until then; frames
 * live in pinned memory so that the downloads are real DMA transfers). */
typedef struct { p264hip_ctx *hip; int mb_w, mb_h, n_local, n_pend, n_last; int *stream, *slot; uint8_t **out; void **planes; size_t plane_bytes; } hipbk_t;
static void hipbk_close(void *ctx);
static int hipbk_open(void **ctx, int device, int mb_w, int mb_h, int n_local, int slots)
{
    hipbk_t *b = (hipbk_t *)calloc(1, sizeof *b);
    if (!b) return fail("out of memory");
    b->stream = (int *)malloc(sizeof(int) * (size_t)n_local); b->slot = (int *)malloc(sizeof(int) * (size_t)n_local);
    b->out = (uint8_t **)malloc(sizeof(uint8_t *) * (size_t)n_local); b->planes = (void **)calloc((size_t)n_local, sizeof(void *));
    if (!b->stream || !b->slot || !b->out || !b->planes) { hipbk_close(b); return fail("out of memory"); }
    if (p264hip_create(&b->hip, device, mb_w, mb_h, n_local, slots, n_local) != P264HIP_OK) { fail("%s", p264hip_last_error()); b->hip = NULL; hipbk_close(b); return -1; }
    b->mb_w = mb_w; b->mb_h = mb_h; b->n_local = n_local;
    *ctx = b;
    return 0;
}
static int hipbk_sync(void *ctx)
{
    hipbk_t *b = (hipbk_t *)ctx;
    const int w = b->mb_w * 16, h = b->mb_h * 16, n = b->n_pend;
    b->n_pend = 0; b->n_last = 0;
    if (n) {
        /* input slot = local stream (hipbk_reconstruct); one batch, then the frames: downloaded, or - pictures that came the
         * device road - converted to planes that stay on the device (hipbk_planes) */
        if (p264hip_reconstruct(b->hip, b->stream, b->stream, n) != P264HIP_OK) return fail("%s", p264hip_last_error());
        for (int i = 0; i < n; i++) {
            uint8_t *o = b->out[i];
            b->planes[i] = NULL;
            if (o) { if (p264hip_read_frame_async(b->hip, b->stream[i], b->slot[i], o, w, o + (size_t)w * h, o + (size_t)w * h * 5 / 4, w / 2) != P264HIP_OK) return fail("%s", p264hip_last_error()); }
            else if (p264hip_frame_planar_device(b->hip, b->stream[i], b->slot[i], i, &b->planes[i], &b->plane_bytes) != P264HIP_OK) return fail("%s", p264hip_last_error());
        }
        b->n_last = n;
    }
    return p264hip_sync(b->hip) == P264HIP_OK ? 0 : fail("%s", p264hip_last_error());
}
/* one more picture of the round: its stream (= input slot), frame-store slot and where its frame goes (NULL: planes on the device) */
static void hipbk_note(hipbk_t *b, int s, int dst_slot, uint8_t *i420)
{
    b->stream[b->n_pend] = s; b->slot[b->n_pend] = dst_slot; b->out[b->n_pend] = i420;
    b->n_pend++;
}
static int hipbk_reconstruct(void *ctx, int s, const p264hip_picture_t *pic, uint8_t *i420)
{
    hipbk_t *b = (hipbk_t *)ctx;
    if (s < 0 || s >= b->n_local) return fail("local stream %d out of range", s);
    for (int i = 0; i < b->n_pend; i++)
        if (b->stream[i] == s) { if (hipbk_sync(b)) return -1; break; }     /* (a second picture of a stream: the first one has to be through) */
    if (p264hip_upload_async(b->hip, s, pic) != P264HIP_OK) return fail("%s", p264hip_last_error());
    hipbk_note(b, s, pic->dst_slot, i420);
    return 0;
}
/* the device road: the picture's arrays are written into the stream's input slot by the transport */
static int hipbk_reserve(void *ctx, int s, const p264hip_picture_t *desc, void **dev, size_t *bytes)
{
    hipbk_t *b = (hipbk_t *)ctx;
    if (s < 0 || s >= b->n_local) return fail("local stream %d out of range", s);
    for (int i = 0; i < b->n_pend; i++)
        if (b->stream[i] == s) return fail("two pictures of local stream %d in one round", s);     /* (its slot is still to be read) */
    if (p264hip_input_reserve(b->hip, s, desc, dev, bytes) != P264HIP_OK) return fail("%s", p264hip_last_error());
    return 0;
}
static int hipbk_reconstruct_reserved(void *ctx, int s, const p264hip_picture_t *desc)
{
    hipbk_t *b = (hipbk_t *)ctx;
    if (s < 0 || s >= b->n_local || b->n_pend >= b->n_local) return fail("local stream %d out of range", s);
    if (p264hip_input_commit(b->hip, s) != P264HIP_OK) return fail("%s", p264hip_last_error());
    hipbk_note(b, s, desc->dst_slot, NULL);
    return 0;
}
static int hipbk_planes(void *ctx, int k, void **dev, size_t *bytes)
{
    hipbk_t *b = (hipbk_t *)ctx;
    if (k < 0 || k >= b->n_last || !b->planes[k]) return fail("no device planes for picture %d of the round", k);
    *dev = b->planes[k]; *bytes = b->plane_bytes;
    return 0;
}
static void hipbk_close(void *ctx)
{
    hipbk_t *b = (hipbk_t *)ctx;
    if (!b) return;
    if (b->hip) p264hip_destroy(b->hip);
    free(b->stream); free(b->slot); free(b->out); free(b->planes); free(b);
}
static const p264fan_backend_t g_hip_backend = { NULL, hipbk_open, hipbk_reconstruct, hipbk_close, hipbk_sync, hipbk_reserve, hipbk_reconstruct_reserved, hipbk_planes };
/* frames: pinned when a HIP device is there (downloads and RCCL staging copies become DMA), plain memory otherwise */
static uint8_t *frames_alloc(size_t bytes, int *pinned)
{
    uint8_t *p = (uint8_t *)p264hip_host_alloc(bytes);
    *pinned = p != NULL;
    return p ? p : (uint8_t *)malloc(bytes);
}
static void frames_free(uint8_t *p, int pinned) { if (pinned) p264hip_host_free(p); else free(p); }

/* ---------------------------------------------------------------- TCP transport --------- */
typedef struct { int rank, world; int *fd; uint8_t *bounce; size_t bounce_cap; } tcp_t;        /* fd[peer]; root: one per worker, worker: fd[0] */
static int io_all(int fd, void *buf, size_t n, int wr)
{
    uint8_t *p = (uint8_t *)buf;
    while (n) {
        ssize_t k = wr ? send(fd, p, n, MSG_NOSIGNAL) : recv(fd, p, n, 0);
        if (k < 0 && errno == EINTR) continue;
        if (k <= 0) return fail("tcp %s: %s", wr ? "send" : "recv", k == 0 ? "peer closed" : strerror(errno));
        p += k; n -= (size_t)k;
    }
    return 0;
}
static int tcp_send(void *c, int peer, const void *buf, size_t n) { tcp_t *t = (tcp_t *)c; return io_all(t->fd[peer], (void *)buf, n, 1); }
static int tcp_recv(void *c, int peer, void *buf, size_t n) { tcp_t *t = (tcp_t *)c; return io_all(t->fd[peer], buf, n, 0); }
static int tcp_nop(void *c) { (void)c; return 0; }
/* P264AMD_FAN_TCP_DEVICE=1: device buffers through a host bounce buffer - stands in for a device-to-device transport where
 * ranks share one GPU (tests of the device road; RCCL needs one GPU per rank) */
static uint8_t *tcp_bounce(tcp_t *t, size_t n)
{
    if (fit_buffer(&t->bounce, &t->bounce_cap, n) || !t->bounce) fail("out of memory");
    return t->bounce;
}
static int tcp_send_dev(void *c, int peer, const void *dev, size_t n)
{
    tcp_t *t = (tcp_t *)c;
    uint8_t *b = tcp_bounce(t, n);
    if (!b) return -1;
    if (p264hip_copy_from_device(b, dev, n) != P264HIP_OK) return fail("%s", p264hip_last_error());
    return io_all(t->fd[peer], b, n, 1);
}
static int tcp_recv_dev(void *c, int peer, void *dev, size_t n)
{
    tcp_t *t = (tcp_t *)c;
    uint8_t *b = tcp_bounce(t, n);
    if (!b) return -1;
    if (io_all(t->fd[peer], b, n, 0)) return -1;
    return p264hip_copy_to_device(dev, b, n) != P264HIP_OK ? fail("%s", p264hip_last_error()) : 0;
}
static void tcp_abort(void *c)
{
    tcp_t *t = (tcp_t *)c;
    if (!t) return;
    for (int i = 0; i < t->world; i++) if (t->fd[i] >= 0) shutdown(t->fd[i], SHUT_RDWR);
}
static void tcp_close(void *c)
{
    tcp_t *t = (tcp_t *)c;
    if (!t) return;
    for (int i = 0; i < t->world; i++) if (t->fd[i] >= 0) close(t->fd[i]);
    free(t->fd); free(t->bounce); free(t);
}
int p264fan_tcp_transport(p264fan_transport_t *out, int rank, int world, const char *host, int port)
{
    if (p264amd_cpu_refuse("p264fan_tcp_transport")) return p264fan_set_error("p264fan_tcp_transport: CPU older than the build's target (x86-64-v3)");
    if (!out || world < 1 || rank < 0 || rank >= world || port < 1 || port > 65535) return fail("p264fan_tcp_transport: bad argument");
    tcp_t *t = (tcp_t *)calloc(1, sizeof *t);
    if (!t) return fail("out of memory");
    t->rank = rank; t->world = world; t->fd = (int *)malloc(sizeof(int) * (size_t)world);
    if (!t->fd) { free(t); return fail("out of memory"); }
    for (int i = 0; i < world; i++) t->fd[i] = -1;
    struct sockaddr_in a; memset(&a, 0, sizeof a);
    a.sin_family = AF_INET; a.sin_port = htons((uint16_t)port);
    const int one = 1;
    if (rank == 0) {
        a.sin_addr.s_addr = htonl(INADDR_ANY);
        int ls = socket(AF_INET, SOCK_STREAM, 0);
        if (ls < 0 || setsockopt(ls, SOL_SOCKET, SO_REUSEADDR, &one, sizeof one) || bind(ls, (struct sockaddr *)&a, sizeof a) || listen(ls, world)) {
            if (ls >= 0) close(ls);
            tcp_close(t); return fail("tcp root: cannot listen on port %d: %s", port, strerror(errno));
        }
        for (int k = 1; k < world; k++) {                     /* every worker introduces itself with its rank */
            int fd = accept(ls, NULL, NULL);
            int32_t r = -1;
            if (fd < 0 || io_all(fd, &r, sizeof r, 0) || r < 1 || r >= world || t->fd[r] >= 0) { if (fd >= 0) close(fd); close(ls); tcp_close(t); return fail("tcp root: bad worker connection"); }
            setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
            t->fd[r] = fd;
        }
        close(ls);
    } else {
        if (inet_pton(AF_INET, host ? host : "127.0.0.1", &a.sin_addr) != 1) { tcp_close(t); return fail("tcp worker: bad root address %s", host); }
        int fd = -1;
        for (int tries = 0; tries < 600; tries++) {            /* the root may not be listening yet */
            fd = socket(AF_INET, SOCK_STREAM, 0);
            if (fd >= 0 && connect(fd, (struct sockaddr *)&a, sizeof a) == 0) break;
            if (fd >= 0) close(fd);
            fd = -1;
            usleep(100000);
        }
        int32_t r = rank;
        if (fd < 0 || io_all(fd, &r, sizeof r, 1)) { if (fd >= 0) close(fd); tcp_close(t); return fail("tcp worker %d: cannot reach the root at %s:%d", rank, host ? host : "127.0.0.1", port); }
        setsockopt(fd, IPPROTO_TCP, TCP_NODELAY, &one, sizeof one);
        t->fd[0] = fd;
    }
    out->ctx = t; out->send = tcp_send; out->recv = tcp_recv; out->group_begin = tcp_nop; out->group_end = tcp_nop; out->close = tcp_close; out->name = "tcp"; out->abort = tcp_abort;
    out->send_dev = NULL; out->recv_dev = NULL;
    { const char *e = getenv("P264AMD_FAN_TCP_DEVICE"); if (e && atoi(e) > 0) { out->send_dev = tcp_send_dev; out->recv_dev = tcp_recv_dev; } }
    return 0;
}

/* ---------------------------------------------------------------- fan-out --------------- */
struct p264fan {
    int rank, world, device;
    p264fan_transport_t t;
    p264fan_backend_t bk; void *bk_ctx;
    int own_bk;                               /* the backend is this library's HIP path: it knows P264_MB_I8X8, the parsers may hand it out */
};

p264fan *p264fan_open(int rank, int world, const p264fan_transport_t *t, const p264fan_backend_t *backend, int device)
{
    if (p264amd_cpu_refuse("p264fan_open")) { p264fan_set_error("p264fan_open: CPU older than the build's target (x86-64-v3)"); return NULL; }
    if (world < 1 || rank < 0 || rank >= world || (world > 1 && (!t || !t->send || !t->recv))) { fail("p264fan_open: bad argument"); return NULL; }
    p264fan *f = (p264fan *)calloc(1, sizeof *f);
    if (!f) { fail("out of memory"); return NULL; }
    f->rank = rank; f->world = world; f->device = device;
    if (t) f->t = *t;
    f->bk = backend ? *backend : g_hip_backend;
    f->own_bk = backend == NULL;
    return f;
}
void p264fan_close(p264fan *f)
{
    if (!f) return;
    if (f->bk_ctx && f->bk.close) f->bk.close(f->bk_ctx);
    if (f->t.close) f->t.close(f->t.ctx);
    free(f);
}
static int bk_sync(p264fan *f) { return (f->bk.sync && f->bk_ctx) ? f->bk.sync(f->bk_ctx) : 0; }

/* One step of a round's exchange: n transfers of one kind, posted inside one group_begin / group_end.  Any failure in it is
 * the transport's, and ends the rank's loop: there is nobody left to talk to. */
typedef enum { FAN_SEND, FAN_RECV, FAN_SEND_DEV, FAN_RECV_DEV } fan_dir_t;
typedef struct { int peer; void *buf; size_t bytes; } fan_xfer_t;
static int post_group(p264fan *f, fan_dir_t dir, const fan_xfer_t *x, int n)
{
    if (f->t.group_begin && f->t.group_begin(f->t.ctx)) return -1;
    int rc = 0;
    for (int i = 0; i < n && !rc; i++)
        switch (dir) {
        case FAN_SEND:     rc = f->t.send(f->t.ctx, x[i].peer, x[i].buf, x[i].bytes); break;
        case FAN_RECV:     rc = f->t.recv(f->t.ctx, x[i].peer, x[i].buf, x[i].bytes); break;
        case FAN_SEND_DEV: rc = f->t.send_dev(f->t.ctx, x[i].peer, x[i].buf, x[i].bytes); break;
        case FAN_RECV_DEV: rc = f->t.recv_dev(f->t.ctx, x[i].peer, x[i].buf, x[i].bytes); break;
        }
    if (f->t.group_end && f->t.group_end(f->t.ctx)) rc = -1;
    return rc ? -1 : 0;
}

/* ---------------------------------------------------------------- worker ---------------- */
/* A round on a worker, in the words of the protocol comment above: receive the control block, worker_recv_heads,
 * worker_open_backend_once, worker_recv_pictures, worker_reconstruct, worker_answer.  Only a transport failure (or a rank out of
 * step: `fatal`) ends the loop; whatever else fails becomes the round's status (w->st). */
typedef struct {
    p264fan *f;
    int dev_road;                       /* the device road: pictures straight into their input slots, planes straight out of the conversion buffers */
    fan_head_t *heads;                  /* [FAN_MAX_PER_ROUND] the round's descriptors */
    uint8_t *msg[FAN_MAX_PER_ROUND]; size_t cap[FAN_MAX_PER_ROUND];       /* the round's packed pictures (host road) */
    uint8_t *out; size_t frame; int out_pinned;                           /* the round's frames (host road), `frame` bytes each */
    int on_device;                      /* this round goes the device road */
    void *slot_dev[FAN_MAX_PER_ROUND], *plane_dev[FAN_MAX_PER_ROUND];
    fan_xfer_t x[FAN_MAX_PER_ROUND];
    fan_status_t st;                    /* the round's answer */
    char first_err[248];                /* the first round that failed: every later round answers with it */
    int fatal;                          /* this rank cannot stay in step */
} worker_t;

static int worker_init(worker_t *w, p264fan *f)
{
    memset(w, 0, sizeof *w);
    w->f = f;
    w->dev_road = f->t.recv_dev && f->t.send_dev && f->bk.reserve && f->bk.reconstruct_reserved && f->bk.planes;
    w->heads = (fan_head_t *)malloc(sizeof(fan_head_t) * FAN_MAX_PER_ROUND);
    if (!w->heads) { w->fatal = 1; return fail("out of memory"); }
    return 0;
}
/* Invariant 4: leaving out of step (`fatal`) aborts the transport - the root must not wait for this rank's status or frames
 * (RCCL has no "peer closed") - and keeps the error text; a plain transport failure does not abort.  Invariant 3: a worker
 * that left in step, on FINISHED, still returns its first error. */
static int worker_free(worker_t *w, int rc)
{
    if (w->fatal && w->f->t.abort) { err_keep_t keep; err_keep(&keep); w->f->t.abort(w->f->t.ctx); err_restore(&keep); }
    for (int k = 0; k < FAN_MAX_PER_ROUND; k++) free(w->msg[k]);
    free(w->heads);
    if (w->out) frames_free(w->out, w->out_pinned);
    if (!rc && w->first_err[0]) rc = fail("%s", w->first_err);    /* the job failed on this worker, even though it left in step */
    return rc;
}
/* The round's control block - or FAN_FINISHED, which only ever arrives here (invariant 3).  A block out of range means this
 * rank is out of step: nothing sane left to do (invariant 4). */
static int worker_recv_ctrl(worker_t *w, fan_ctrl_t *c)
{
    const fan_xfer_t x = { 0, c, sizeof *c };
    if (post_group(w->f, FAN_RECV, &x, 1)) return -1;
    if (c->n == FAN_FINISHED) return 0;
    if (c->n < 0 || c->n > FAN_MAX_PER_ROUND) { w->fatal = 1; return fail("worker %d: bad control block", w->f->rank); }
    memset(&w->st, 0, sizeof w->st); w->st.n = c->n;
    return 0;
}
/* The round's descriptors, one message (invariant 5: none when the round brings this worker no picture).  A bad head, or a
 * round that failed earlier - this worker's frame stores are stale then - is the round's status (invariant 3). */
static int worker_recv_heads(worker_t *w, const fan_ctrl_t *c)
{
    const fan_xfer_t x = { 0, w->heads, sizeof(fan_head_t) * (size_t)c->n };
    if (c->n && post_group(w->f, FAN_RECV, &x, 1)) return -1;
    for (int k = 0; k < c->n && !w->st.rc; k++) if (check_head(&w->heads[k], c->bytes[k])) w->st.rc = -1;
    if (w->first_err[0]) { w->st.rc = -1; fail("%s", w->first_err); }
    return 0;
}
/* The backend and the frame area, at the first round that is sound; a failure is the round's status (invariant 3). */
static void worker_open_backend_once(worker_t *w, const fan_ctrl_t *c)
{
    p264fan *f = w->f;
    if (w->st.rc || f->bk_ctx) return;
    if (f->bk.open(&f->bk_ctx, f->device, c->mb_w, c->mb_h, c->n_local_streams, c->slots)) { w->st.rc = -1; f->bk_ctx = NULL; return; }
    w->frame = (size_t)c->mb_w * c->mb_h * 384;
    if (w->dev_road) return;
    w->out = frames_alloc(w->frame * FAN_MAX_PER_ROUND, &w->out_pinned);
    if (!w->out) { w->st.rc = -1; fail("worker %d: out of memory", f->rank); }
}
/* Invariant 3: the round's pictures are ALWAYS received, whatever state this worker is in - the error text of the state kept
 * across the receives.  Device road: every picture's slot is reserved first; if that fails for one of them the whole round
 * goes to host buffers and is answered with the error.  No memory to receive into: out of step (invariant 4). */
static int worker_recv_pictures(worker_t *w, const fan_ctrl_t *c)
{
    p264fan *f = w->f;
    w->on_device = w->dev_road && !w->st.rc;
    for (int k = 0; k < c->n && w->on_device; k++) {
        size_t bytes = 0;
        if (f->bk.reserve(f->bk_ctx, w->heads[k].local_stream, &w->heads[k].desc, &w->slot_dev[k], &bytes) || bytes != c->bytes[k]) {
            if (bytes && bytes != c->bytes[k]) fail("worker %d: slot of %zu bytes for a picture of %u", f->rank, bytes, c->bytes[k]);
            w->st.rc = -1; w->on_device = 0;
        }
    }
    for (int k = 0; k < c->n && !w->on_device; k++)
        if (fit_buffer(&w->msg[k], &w->cap[k], c->bytes[k])) { w->fatal = 1; return fail("worker %d: out of memory", f->rank); }
    for (int k = 0; k < c->n; k++) w->x[k] = (fan_xfer_t){ 0, w->on_device ? w->slot_dev[k] : (void *)w->msg[k], c->bytes[k] };
    err_keep_t keep; err_keep(&keep);
    if (post_group(f, w->on_device ? FAN_RECV_DEV : FAN_RECV, w->x, c->n)) return -1;
    if (w->st.rc) err_restore(&keep);
    return 0;
}
/* Reconstruct the round; a failure becomes the round's status, and the first one every later round's (invariant 3). */
static void worker_reconstruct(worker_t *w, const fan_ctrl_t *c)
{
    p264fan *f = w->f;
    fan_status_t *st = &w->st;
    for (int k = 0; k < c->n && !st->rc; k++) {
        if (w->on_device) { if (f->bk.reconstruct_reserved(f->bk_ctx, w->heads[k].local_stream, &w->heads[k].desc)) st->rc = -1; continue; }
        p264hip_picture_t pic; int ls = 0;
        if (unpack_picture(&w->heads[k], w->msg[k], c->bytes[k], &pic, &ls) || f->bk.reconstruct(f->bk_ctx, ls, &pic, w->out + w->frame * (size_t)k)) st->rc = -1;
    }
    if (!st->rc && bk_sync(f)) st->rc = -1;
    for (int k = 0; k < c->n && !st->rc && w->on_device; k++) {
        size_t bytes = 0;
        if (f->bk.planes(f->bk_ctx, k, &w->plane_dev[k], &bytes) || bytes != w->frame) {
            if (bytes && bytes != w->frame) fail("worker %d: planes of %zu bytes, a frame has %zu", f->rank, bytes, w->frame);
            st->rc = -1;
        }
    }
    if (!st->rc) return;
    snprintf(st->msg, sizeof st->msg, "%.236s", g_err[0] ? g_err : "reconstruction failed");
    if (!w->first_err[0]) snprintf(w->first_err, sizeof w->first_err, "%.236s", st->msg);
}
/* The status block, then - only when the status is 0 - the round's frames (invariant 5). */
static int worker_answer(worker_t *w, const fan_ctrl_t *c)
{
    w->st.device_road = w->on_device && !w->st.rc && c->n > 0;
    const fan_xfer_t x = { 0, &w->st, sizeof w->st };
    if (post_group(w->f, FAN_SEND, &x, 1)) return -1;
    if (w->st.rc) return 0;
    for (int k = 0; k < c->n; k++) w->x[k] = (fan_xfer_t){ 0, w->on_device ? w->plane_dev[k] : (void *)(w->out + w->frame * (size_t)k), w->frame };
    return post_group(w->f, w->on_device ? FAN_SEND_DEV : FAN_SEND, w->x, c->n);
}

int p264fan_worker_run(p264fan *f)
{
    if (!f || f->rank == 0) return fail("p264fan_worker_run: not a worker");
    worker_t w;
    int rc = worker_init(&w, f);        /* rc: transport failures (and `fatal`) only - they end the loop */
    while (!rc) {
        fan_ctrl_t c;
        if ((rc = worker_recv_ctrl(&w, &c)) || c.n == FAN_FINISHED) break;
        if ((rc = worker_recv_heads(&w, &c))) break;
        worker_open_backend_once(&w, &c);
        if ((rc = worker_recv_pictures(&w, &c))) break;
        worker_reconstruct(&w, &c);
        rc = worker_answer(&w, &c);
    }
    return worker_free(&w, rc);
}

/* ---------------------------------------------------------------- the root's parse side - */
/* One round's worth of work, produced by the parse side and consumed by the exchange side: every stream's next picture,
 * PACKED (the parser's arrays only live until the stream's next call; a packed copy lets the next round be parsed while
 * this one travels and is reconstructed - for the root's own streams too). */
typedef struct {
    uint8_t **msg; size_t *cap, *len;   /* [n_streams]; len 0 = the stream has no picture in this round */
    fan_head_t *head;                   /* [n_streams] the descriptors of the packed pictures */
    int64_t *index;                     /* picture number inside its stream */
    int n, failed, slots, mb_w, mb_h;
    char err[200];
} fan_round_t;
typedef struct {
    annexb_reader_t *st; int n_streams, world, max_pictures, threads;
    fan_round_t rounds[2];
    int ready[2];                       /* 0 free, 1 filled */
    int stop;
    pthread_mutex_t mu; pthread_cond_t cv;
    double parse_seconds;
} fan_producer_t;

typedef struct { fan_producer_t *P; fan_round_t *R; int first, step, failed; } parse_job_t;
static void *parse_worker(void *arg)
{
    parse_job_t *j = (parse_job_t *)arg;
    fan_producer_t *P = j->P; fan_round_t *R = j->R;
    for (int s = j->first; s < P->n_streams; s += j->step) {
        R->len[s] = 0;
        const p264hip_picture_t *pic = annexb_reader_next(&P->st[s], P->max_pictures);
        if (!pic) { if (annexb_reader_failed(&P->st[s])) j->failed = 1; continue; }
        const size_t need = packed_size(pic);
        if (fit_buffer(&R->msg[s], &R->cap[s], need)) { j->failed = 1; continue; }
        if (!need || pack_picture(&R->head[s], R->msg[s], R->cap[s], s / P->world, pic)) { j->failed = 1; continue; }
        R->len[s] = need;
        R->index[s] = P->st[s].pictures - 1;
    }
    return NULL;
}
/* the round's pictures are parsed side by side on `threads` host threads: the streams are independent, and the serial
 * parse of one stream is what bounds the fan-out */
static void fill_round(fan_producer_t *P, fan_round_t *R)
{
    int threads = P->threads;
    if (threads > P->n_streams) threads = P->n_streams;
    if (threads > 64) threads = 64;
    parse_job_t jobs[64];
    pthread_t tid[64];
    int started = 0;
    for (int t = 0; t < threads; t++) jobs[t] = (parse_job_t){ P, R, t, threads, 0 };
    for (int t = 1; t < threads; t++) { if (pthread_create(&tid[t], NULL, parse_worker, &jobs[t])) break; started = t; }
    for (int t = started + 1; t < threads; t++) parse_worker(&jobs[t]);     /* (threads that could not be started: done here) */
    parse_worker(&jobs[0]);
    for (int t = 1; t <= started; t++) pthread_join(tid[t], NULL);
    R->n = 0; R->failed = 0; R->slots = 0; R->mb_w = R->mb_h = 0; R->err[0] = 0;
    for (int t = 0; t < threads; t++) if (jobs[t].failed) { R->failed = 1; snprintf(R->err, sizeof R->err, "a stream failed to parse (or the host ran out of memory)"); }
    for (int s = 0; s < P->n_streams && !R->failed; s++) {
        if (!R->len[s]) continue;
        const fan_head_t h = R->head[s];
        if (!R->n) { R->mb_w = h.desc.mb_w; R->mb_h = h.desc.mb_h; }
        else if (h.desc.mb_w != R->mb_w || h.desc.mb_h != R->mb_h) { R->failed = 1; snprintf(R->err, sizeof R->err, "stream %d has a different picture size (%dx%d macroblocks, the job runs at %dx%d)", s, h.desc.mb_w, h.desc.mb_h, R->mb_w, R->mb_h); }
        const int sl = p264parse_slots(P->st[s].parser);       /* every rank's frame stores are sized for the stream that needs most */
        if (sl > R->slots) R->slots = sl;
        R->n++;
    }
}
static void *producer_main(void *arg)
{
    fan_producer_t *P = (fan_producer_t *)arg;
    for (int k = 0;; k ^= 1) {
        pthread_mutex_lock(&P->mu);
        while (P->ready[k] && !P->stop) pthread_cond_wait(&P->cv, &P->mu);
        const int stop = P->stop;
        pthread_mutex_unlock(&P->mu);
        if (stop) break;
        const double t0 = now_s();
        fill_round(P, &P->rounds[k]);
        const int last = P->rounds[k].n == 0 || P->rounds[k].failed;
        pthread_mutex_lock(&P->mu);
        P->parse_seconds += now_s() - t0;
        P->ready[k] = 1;
        pthread_cond_broadcast(&P->cv);
        pthread_mutex_unlock(&P->mu);
        if (last) break;
    }
    return NULL;
}

/* ---------------------------------------------------------------- root ------------------ */
/* A round on the root, in the words of the protocol comment above: wait for the parsed round, root_first_round,
 * root_check_round, root_scatter, root_own_streams, root_gather, root_deliver; root_finish at the round boundary where the
 * job ends, whatever ended it. */
typedef struct {
    p264fan *f; int n_streams, W, per_rank;         /* per_rank: local streams of every rank (the biggest share) */
    fan_producer_t P; pthread_t producer; int have_producer;
    fan_ctrl_t *ctrl; fan_status_t *status;         /* [W] the round's control and status blocks */
    fan_head_t *heads; int *head_at;                /* the round's descriptors grouped by worker: heads[head_at[r] .. head_at[r + 1]) in the order of r's control block */
    fan_xfer_t *x;                                  /* [max(n_streams, W)] one step's transfers */
    uint8_t *frames; size_t frame; int frames_pinned;       /* [n_streams] the round's frames, `frame` bytes each */
    int mb_w, mb_h, slots;                          /* the job's geometry: the first round's */
    int rc_local; char err_local[256];              /* the root's own reconstruction of the round */
    p264fan_frame_cb on_frame; void *user;
    p264fan_stats_t S; double t0;
} root_job_t;

static int root_job_init(root_job_t *J, p264fan *f, int n_streams, const uint8_t *const *annexb, const int64_t *sizes, int max_pictures, p264fan_frame_cb on_frame, void *user)
{
    memset(J, 0, sizeof *J);
    const int W = f->world;
    fan_producer_t *P = &J->P;
    J->f = f; J->n_streams = n_streams; J->W = W; J->per_rank = (n_streams + W - 1) / W; J->on_frame = on_frame; J->user = user;
    P->st = (annexb_reader_t *)calloc((size_t)n_streams, sizeof *P->st);
    J->ctrl = (fan_ctrl_t *)calloc((size_t)W, sizeof *J->ctrl);
    J->status = (fan_status_t *)calloc((size_t)W, sizeof *J->status);
    J->heads = (fan_head_t *)malloc(sizeof(fan_head_t) * (size_t)n_streams);
    J->head_at = (int *)calloc((size_t)W + 1, sizeof(int));
    J->x = (fan_xfer_t *)calloc((size_t)(n_streams > W ? n_streams : W), sizeof *J->x);
    int rc = (P->st && J->ctrl && J->status && J->heads && J->head_at && J->x) ? 0 : fail("out of memory");
    for (int k = 0; k < 2 && !rc; k++) {
        fan_round_t *R = &P->rounds[k];
        R->msg = (uint8_t **)calloc((size_t)n_streams, sizeof *R->msg); R->cap = (size_t *)calloc((size_t)n_streams, sizeof *R->cap);
        R->len = (size_t *)calloc((size_t)n_streams, sizeof *R->len); R->index = (int64_t *)calloc((size_t)n_streams, sizeof *R->index);
        R->head = (fan_head_t *)calloc((size_t)n_streams, sizeof *R->head);
        if (!R->msg || !R->cap || !R->len || !R->index || !R->head) rc = fail("out of memory");
    }
    for (int s = 0; s < n_streams && !rc; s++) {
        /* (Intra 8x8 macroblocks only for the library's own backend on every rank - a plug-in backend's owner has not said that it
         * knows the record, include/p264parse.h) */
        P->st[s].parser = p264parse_open(P264PARSE_OPT_QUIET | (f->own_bk ? P264PARSE_OPT_INTRA8X8 | P264PARSE_OPT_SCALING | P264PARSE_OPT_CR_OFFSET : 0));
        annexb_reader_set_input(&P->st[s], annexb[s], sizes[s]);
        if (!P->st[s].parser) rc = fail("p264parse_open failed");
    }
    J->S.world = W;
    P->n_streams = n_streams; P->world = W; P->max_pictures = max_pictures;
    P->threads = n_streams;                                  /* one parser thread per stream unless P264AMD_FAN_THREADS says otherwise */
    { const char *e = getenv("P264AMD_FAN_THREADS"); if (e && atoi(e) >= 1) P->threads = atoi(e); }
    J->S.parse_threads = P->threads < n_streams ? P->threads : n_streams;
    if (J->S.parse_threads > 64) J->S.parse_threads = 64;
    if (!rc) {
        pthread_mutex_init(&P->mu, NULL); pthread_cond_init(&P->cv, NULL);
        if (pthread_create(&J->producer, NULL, producer_main, P)) rc = fail("cannot start the parse thread");
        else J->have_producer = 1;
    }
    J->t0 = now_s();
    return rc;
}
static void root_job_free(root_job_t *J)
{
    fan_producer_t *P = &J->P;
    if (P->st) for (int s = 0; s < J->n_streams; s++) annexb_reader_close(&P->st[s]);
    for (int k = 0; k < 2; k++) {
        fan_round_t *R = &P->rounds[k];
        if (R->msg) for (int s = 0; s < J->n_streams; s++) free(R->msg[s]);
        free(R->msg); free(R->cap); free(R->len); free(R->index); free(R->head);
    }
    if (J->frames) frames_free(J->frames, J->frames_pinned);
    free(P->st); free(J->ctrl); free(J->status); free(J->heads); free(J->head_at); free(J->x);
}
/* the next round, parsed and packed while the previous one travelled (invariant 7: parse_wait_seconds) / hand its buffers back
 * to the parse side */
static fan_round_t *root_wait_round(root_job_t *J, int k)
{
    const double w0 = now_s();
    pthread_mutex_lock(&J->P.mu);
    while (!J->P.ready[k]) pthread_cond_wait(&J->P.cv, &J->P.mu);
    pthread_mutex_unlock(&J->P.mu);
    J->S.parse_wait_seconds += now_s() - w0;
    return &J->P.rounds[k];
}
static void root_release_round(root_job_t *J, int k)
{
    pthread_mutex_lock(&J->P.mu); J->P.ready[k] = 0; pthread_cond_broadcast(&J->P.cv); pthread_mutex_unlock(&J->P.mu);
}
/* The job's geometry, the frames and the root's backend, from the first round.  Invariant 1: it can fail, so it runs before
 * the round's control block goes out. */
static int root_first_round(root_job_t *J, const fan_round_t *R)
{
    p264fan *f = J->f;
    if (J->mb_w) return 0;
    J->mb_w = R->mb_w; J->mb_h = R->mb_h; J->slots = R->slots;
    J->frame = (size_t)J->mb_w * J->mb_h * 384;
    J->frames = frames_alloc(J->frame * (size_t)J->n_streams, &J->frames_pinned);
    if (!J->frames) return fail("out of memory");
    if (f->bk.open(&f->bk_ctx, f->device, J->mb_w, J->mb_h, J->per_rank, J->slots)) { f->bk_ctx = NULL; return -1; }
    return 0;
}
/* A later round must fit what every rank opened with: same picture size, no more frame slots.  Invariant 1 again. */
static int root_check_round(root_job_t *J, const fan_round_t *R)
{
    if (R->mb_w != J->mb_w || R->mb_h != J->mb_h) return fail("the picture size changed inside the job (%dx%d -> %dx%d macroblocks)", J->mb_w, J->mb_h, R->mb_w, R->mb_h);
    if (R->slots > J->slots) return fail("a stream now needs %d frame slots, the ranks' frame stores were opened with %d (num_ref_frames grew inside the job)", R->slots, J->slots);
    return 0;
}
/* Scatter: every worker's control block, then its pictures' heads as one message (none for a worker without a picture in
 * this round), then the packed pictures (invariant 5).
 * Invariant 1: from here to the end of the gather nothing but the transport ends the round.  Invariant 7: bytes_scattered,
 * pictures_remote and this half of exchange_seconds. */
static int root_scatter(root_job_t *J, const fan_round_t *R)
{
    const int W = J->W, n_streams = J->n_streams;
    fan_ctrl_t *ctrl = J->ctrl;
    const double e0 = now_s();
    for (int r = 1; r < W; r++) { memset(&ctrl[r], 0, sizeof ctrl[r]); ctrl[r].mb_w = J->mb_w; ctrl[r].mb_h = J->mb_h; ctrl[r].slots = J->slots; ctrl[r].n_local_streams = J->per_rank; }
    for (int s = 0; s < n_streams; s++) {
        const int r = s % W;
        if (!R->len[s] || r == 0) continue;
        ctrl[r].bytes[ctrl[r].n++] = (uint32_t)R->len[s];
        J->S.bytes_scattered += (int64_t)R->len[s]; J->S.pictures_remote++;
    }
    J->head_at[0] = J->head_at[1] = 0;
    for (int r = 1; r < W; r++) {
        int at = J->head_at[r];
        for (int s = r; s < n_streams; s += W) if (R->len[s]) J->heads[at++] = R->head[s];
        J->head_at[r + 1] = at;
    }
    for (int r = 1; r < W; r++) J->x[r - 1] = (fan_xfer_t){ r, &ctrl[r], sizeof ctrl[r] };
    if (post_group(J->f, FAN_SEND, J->x, W - 1)) return -1;
    int n = 0;
    for (int r = 1; r < W; r++) if (ctrl[r].n) J->x[n++] = (fan_xfer_t){ r, J->heads + J->head_at[r], sizeof(fan_head_t) * (size_t)ctrl[r].n };
    if (post_group(J->f, FAN_SEND, J->x, n)) return -1;
    n = 0;
    for (int s = 0; s < n_streams; s++) if (R->len[s] && s % W) J->x[n++] = (fan_xfer_t){ s % W, R->msg[s], R->len[s] };
    if (post_group(J->f, FAN_SEND, J->x, n)) return -1;
    J->S.exchange_seconds += now_s() - e0;
    return 0;
}
/* The root's own streams while the workers are busy.  Invariant 2: a failure is only noted here (rc_local, err_local);
 * root_deliver reports it after the round's gather.  Invariant 7: reconstruct_seconds. */
static void root_own_streams(root_job_t *J, const fan_round_t *R)
{
    p264fan *f = J->f;
    const double r0 = now_s();
    J->rc_local = 0; J->err_local[0] = 0;
    for (int s = 0; s < J->n_streams && !J->rc_local; s += J->W) {
        if (!R->len[s]) continue;
        p264hip_picture_t pic; int ls = 0;
        if (unpack_picture(&R->head[s], R->msg[s], R->len[s], &pic, &ls) || f->bk.reconstruct(f->bk_ctx, ls, &pic, J->frames + J->frame * (size_t)s)) J->rc_local = -1;
    }
    if (!J->rc_local && bk_sync(f)) J->rc_local = -1;
    if (J->rc_local) snprintf(J->err_local, sizeof J->err_local, "root: %.240s", g_err);
    J->S.reconstruct_seconds += now_s() - r0;
}
/* Gather: every worker's status, then the frames of those whose status is 0 (invariant 5).  Invariant 7: bytes_gathered, the
 * other half of exchange_seconds, device_road_rounds. */
static int root_gather(root_job_t *J, const fan_round_t *R)
{
    const int W = J->W;
    const double g0 = now_s();
    for (int r = 1; r < W; r++) J->x[r - 1] = (fan_xfer_t){ r, &J->status[r], sizeof J->status[r] };
    if (post_group(J->f, FAN_RECV, J->x, W - 1)) return -1;
    int n = 0;
    for (int s = 0; s < J->n_streams; s++)
        if (R->len[s] && s % W && J->status[s % W].rc == 0) { J->x[n++] = (fan_xfer_t){ s % W, J->frames + J->frame * (size_t)s, J->frame }; J->S.bytes_gathered += (int64_t)J->frame; }
    if (post_group(J->f, FAN_RECV, J->x, n)) return -1;
    J->S.exchange_seconds += now_s() - g0;
    for (int r = 1; r < W; r++) if (!J->status[r].rc && J->status[r].device_road) J->S.device_road_rounds++;
    return 0;
}
/* The round's outcome: the first worker's error, then the root's own (invariant 2: only now, after the gather), else every
 * picture to on_frame.  Invariant 7: pictures, rounds. */
static int root_deliver(root_job_t *J, const fan_round_t *R)
{
    for (int r = 1; r < J->W; r++)
        if (J->status[r].rc) { J->status[r].msg[sizeof J->status[r].msg - 1] = 0; return fail("worker %d: %s", r, J->status[r].msg); }
    if (J->rc_local) return fail("%s", J->err_local);
    for (int s = 0; s < J->n_streams; s++)
        if (R->len[s]) { J->S.pictures++; if (J->on_frame) J->on_frame(J->user, s, R->index[s], J->mb_w * 16, J->mb_h * 16, J->frames + J->frame * (size_t)s); }
    J->S.rounds++;
    return 0;
}
/* The round boundary where the job ends (or a dead transport): FAN_FINISHED to every worker - each gets its block whatever
 * happens to the others', so not post_group - with the job's error text kept (invariant 6); then the parse side is stopped and
 * everything freed.
 * Invariant 3: this is the only place FINISHED is sent from, and every way out of a round leads here with the workers waiting
 * for a control block, or with the transport dead.
 * Invariant 7: seconds, parse_seconds. */
static int root_finish(root_job_t *J, int rc, p264fan_stats_t *stats)
{
    p264fan *f = J->f;
    fan_producer_t *P = &J->P;
    err_keep_t keep; err_keep(&keep);
    if (J->ctrl && f->t.send) {
        if (f->t.group_begin) f->t.group_begin(f->t.ctx);
        for (int r = 1; r < J->W; r++) { memset(&J->ctrl[r], 0, sizeof J->ctrl[r]); J->ctrl[r].n = FAN_FINISHED; f->t.send(f->t.ctx, r, &J->ctrl[r], sizeof J->ctrl[r]); }
        if (f->t.group_end) f->t.group_end(f->t.ctx);
    }
    if (rc) err_restore(&keep);
    if (J->have_producer) {
        pthread_mutex_lock(&P->mu); P->stop = 1; P->ready[0] = P->ready[1] = 0; pthread_cond_broadcast(&P->cv); pthread_mutex_unlock(&P->mu);
        pthread_join(J->producer, NULL);
        pthread_mutex_destroy(&P->mu); pthread_cond_destroy(&P->cv);
    }
    J->S.seconds = now_s() - J->t0;
    J->S.parse_seconds = P->parse_seconds;
    if (stats) *stats = J->S;
    root_job_free(J);
    return rc;
}

int p264fan_root_run(p264fan *f, int n_streams, const uint8_t *const *annexb, const int64_t *sizes, int max_pictures,
                     p264fan_frame_cb on_frame, void *user, p264fan_stats_t *stats)
{
    if (!f || f->rank != 0 || n_streams < 1 || !annexb || !sizes) return fail("p264fan_root_run: bad argument");
    if ((n_streams + f->world - 1) / f->world > FAN_MAX_PER_ROUND) return fail("p264fan_root_run: more than %d streams per rank", FAN_MAX_PER_ROUND);
    root_job_t J;
    int rc = root_job_init(&J, f, n_streams, annexb, sizes, max_pictures, on_frame, user);
    for (int k = 0; !rc; k ^= 1) {
        const fan_round_t *R = root_wait_round(&J, k);
        if (R->failed) { rc = fail("%s", R->err); break; }
        if (!R->n) break;
        if ((rc = root_first_round(&J, R)) || (rc = root_check_round(&J, R)) || (rc = root_scatter(&J, R))) break;
        root_own_streams(&J, R);
        if ((rc = root_gather(&J, R)) || (rc = root_deliver(&J, R))) break;
        root_release_round(&J, k);
    }
    return root_finish(&J, rc, stats);
}
