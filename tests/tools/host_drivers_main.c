/* host_drivers_main.c - the host drivers (csrc/host/fanout.c, pipeline.c and the Annex-B reader they share) as a stand-alone
 * program for the sanitizers: CPU only, the HIP layer stubbed out (hip_stub.c plus the one entry point below).
 *
 *   host_drivers_main [-n max_pictures] a.264 [b.264 ...]
 *
 * Every file becomes two streams ([a, a, b, b]; all of one picture size), and the program
 *   1. runs a two-rank fan-out inside this process - two threads, the TCP transport on 127.0.0.1, a port of its own choice -
 *      with a backend that fills the whole i420 buffer from a checksum of the local stream, the picture's descriptor and its
 *      arrays.  Stream 2k
 *      stays on the root, stream 2k + 1 is packed, sent, unpacked and "reconstructed" on the worker: their frames must be
 *      equal picture by picture, and every stream must bring as many pictures as a plain parse of its file finds;
 *   2. runs p264pipe with device -1 (the parsers only) on three threads over the same streams and checks the picture counts.
 * Exit status 0 only if all of that holds.  tests/test_host_drivers_sanitized_cpu.py builds it with -fsanitize=address,undefined
 * and with -fsanitize=thread.
 */
#define _GNU_SOURCE
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <pthread.h>
#include <unistd.h>
#include <sys/socket.h>
#include <netinet/in.h>
#include <arpa/inet.h>
#include "p264fan.h"
#include "p264pipe.h"
#include "p264parse.h"
#include "p264_dropin.h"

/* (the stub file has every p264hip entry point the host objects call but this one) */
int p264hip_export_frames(p264hip_ctx *c, const int *st, const int *sl, int n, const p264hip_export_t *e, void *dst, size_t bytes)
{
    (void)c; (void)st; (void)sl; (void)n; (void)e; (void)dst; (void)bytes;
    return -1;
}

#define MAX_FILES 8
#define MAX_PICS 4096
static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { fprintf(stderr, "host_drivers_main: " __VA_ARGS__); fprintf(stderr, "\n"); g_fail = 1; } } while (0)

/* ---- the backend: a frame that depends on the local stream, on every field of the descriptor and on every array ------------ */
/* (both streams of a pair go through pack_picture / unpack_picture - the root's own too - so what the comparison checks is the
 * road between them: the control block, the heads, TCP and the worker's loop) */
static uint64_t fnv(uint64_t h, const void *p, size_t n)
{
    const uint8_t *b = (const uint8_t *)p;
    for (size_t i = 0; i < n; i++) h = (h ^ b[i]) * 0x100000001b3ull;
    return h;
}
#define FNV_FIELD(h, d, m) fnv(h, &(d)->m, sizeof (d)->m)      /* (field by field: no padding, no pointers) */
static uint64_t picture_sum(int s, const p264hip_picture_t *p)
{
    const size_t n = (size_t)p->mb_w * p->mb_h;
    uint64_t h = fnv(0xcbf29ce484222325ull, &s, sizeof s);
    h = FNV_FIELD(h, p, mb_w); h = FNV_FIELD(h, p, mb_h); h = FNV_FIELD(h, p, slice_type); h = FNV_FIELD(h, p, chroma_qp_offset);
    h = FNV_FIELD(h, p, deblock); h = FNV_FIELD(h, p, alpha_c0_offset); h = FNV_FIELD(h, p, beta_offset); h = FNV_FIELD(h, p, dst_slot);
    h = FNV_FIELD(h, p, n_ref); h = FNV_FIELD(h, p, ref_slot); h = FNV_FIELD(h, p, n_coef_blocks); h = FNV_FIELD(h, p, frame_num);
    h = FNV_FIELD(h, p, n_ref_l1); h = FNV_FIELD(h, p, weighted_bipred); h = FNV_FIELD(h, p, ref_slot_l1); h = FNV_FIELD(h, p, bipred_weight);
    h = FNV_FIELD(h, p, explicit_wp); h = FNV_FIELD(h, p, wp_log2_denom); h = FNV_FIELD(h, p, wp); h = FNV_FIELD(h, p, transform_8x8);
    h = fnv(h, p->mb, n * sizeof(p264hip_mb_t)); h = fnv(h, p->mv, n * 64); h = fnv(h, p->ref_idx, n * 4);
    h = fnv(h, p->i4modes, n * 16); h = fnv(h, p->coefs, (size_t)p->n_coef_blocks * 32);
    if (p->slice_type == P264_SLICE_B) { h = fnv(h, p->mv_l1, n * 64); h = fnv(h, p->ref_idx_l1, n * 4); }
    return h;
}
typedef struct { int mb_w, mb_h; } sumbk_t;
static int sumbk_open(void **ctx, int device, int mb_w, int mb_h, int n_local, int slots)
{
    (void)device; (void)n_local; (void)slots;
    sumbk_t *b = (sumbk_t *)calloc(1, sizeof *b);
    if (!b) return -1;
    b->mb_w = mb_w; b->mb_h = mb_h;
    *ctx = b;
    return 0;
}
static int sumbk_reconstruct(void *ctx, int s, const p264hip_picture_t *pic, uint8_t *i420)
{
    sumbk_t *b = (sumbk_t *)ctx;
    if (pic->mb_w != b->mb_w || pic->mb_h != b->mb_h) return -1;
    uint64_t x = picture_sum(s, pic) | 1;
    const size_t bytes = (size_t)b->mb_w * b->mb_h * 384;
    for (size_t i = 0; i < bytes; i++) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; i420[i] = (uint8_t)(x >> 32); }
    return 0;
}
static void sumbk_close(void *ctx) { free(ctx); }
static const p264fan_backend_t g_sum_backend = { NULL, sumbk_open, sumbk_reconstruct, sumbk_close, NULL, NULL, NULL, NULL };

/* ---- the job ------------------------------------------------------------------------------------------------------------- */
typedef struct { int n_streams; uint64_t (*sum)[MAX_PICS]; int64_t *count; } frames_t;
static void on_frame(void *user, int stream, int64_t picture, int width, int height, const uint8_t *i420)
{
    frames_t *F = (frames_t *)user;
    if (stream < 0 || stream >= F->n_streams || picture < 0 || picture >= MAX_PICS) { g_fail = 1; return; }
    F->sum[stream][picture] = fnv(0xcbf29ce484222325ull, i420, (size_t)width * height * 3 / 2);
    F->count[stream]++;
}

static int free_port(void)
{
    struct sockaddr_in a; memset(&a, 0, sizeof a);
    socklen_t len = sizeof a;
    a.sin_family = AF_INET; a.sin_addr.s_addr = htonl(INADDR_LOOPBACK);
    int fd = socket(AF_INET, SOCK_STREAM, 0), port = -1;
    if (fd >= 0 && bind(fd, (struct sockaddr *)&a, sizeof a) == 0 && getsockname(fd, (struct sockaddr *)&a, &len) == 0) port = ntohs(a.sin_port);
    if (fd >= 0) close(fd);
    return port;
}

typedef struct { int port, rc; char err[512]; } worker_arg_t;
static void *worker_main(void *arg)
{
    worker_arg_t *w = (worker_arg_t *)arg;
    p264fan_transport_t t;
    w->rc = -1;
    if (p264fan_tcp_transport(&t, 1, 2, "127.0.0.1", w->port)) { snprintf(w->err, sizeof w->err, "transport: %s", p264fan_last_error()); return NULL; }
    p264fan *f = p264fan_open(1, 2, &t, &g_sum_backend, 0);
    if (!f) { snprintf(w->err, sizeof w->err, "open: %s", p264fan_last_error()); if (t.close) t.close(t.ctx); return NULL; }
    w->rc = p264fan_worker_run(f);
    if (w->rc) snprintf(w->err, sizeof w->err, "run: %s", p264fan_last_error());
    p264fan_close(f);
    return NULL;
}

/* pictures of a stream as a plain loop over its NAL units counts them */
static int64_t count_pictures(const uint8_t *in, int64_t size, int max_pictures)
{
    p264parse *parser = p264parse_open(P264PARSE_OPT_QUIET);
    uint8_t *rbsp = (uint8_t *)malloc((size_t)size + 8);
    int64_t pos = 0, off, len, n = 0;
    if (!parser || !rbsp) { if (parser) p264parse_close(parser); free(rbsp); return -1; }
    while ((max_pictures <= 0 || n < max_pictures) && p264_annexb_next(in, size, &pos, &off, &len)) {
        if (len < 1) continue;
        p264_nal_t nal; nal.p_payload = rbsp;
        p264_nal_decode(&nal, (void *)(in + off), (int)len);
        const p264hip_picture_t *pic = NULL;
        const int rc = p264parse_nal(parser, nal.i_type, nal.i_ref_idc, nal.p_payload, nal.i_payload, &pic);
        if (rc < 0) { n = -1; break; }
        n += rc == 1;
    }
    p264parse_close(parser); free(rbsp);
    return n;
}

static uint8_t *read_file(const char *path, int64_t *size)
{
    FILE *fp = fopen(path, "rb");
    if (!fp) return NULL;
    fseek(fp, 0, SEEK_END);
    const long n = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    uint8_t *buf = n >= 0 ? (uint8_t *)malloc((size_t)n + 1) : NULL;
    if (buf && fread(buf, 1, (size_t)n, fp) != (size_t)n) { free(buf); buf = NULL; }
    fclose(fp);
    *size = n;
    return buf;
}

int main(int argc, char **argv)
{
    int max_pictures = 0, first = 1;
    if (argc > 2 && !strcmp(argv[1], "-n")) { max_pictures = atoi(argv[2]); first = 3; }
    const int n_files = argc - first;
    if (n_files < 1 || n_files > MAX_FILES) { fprintf(stderr, "usage: %s [-n max_pictures] a.264 [b.264 ...] (at most %d files)\n", argv[0], MAX_FILES); return 2; }
    const int S = 2 * n_files;
    uint8_t *data[MAX_FILES] = { 0 };
    const uint8_t *in[2 * MAX_FILES]; int64_t size[2 * MAX_FILES], want[2 * MAX_FILES], got[2 * MAX_FILES] = { 0 };
    for (int k = 0; k < n_files; k++) {
        int64_t n = 0;
        data[k] = read_file(argv[first + k], &n);
        if (!data[k]) { fprintf(stderr, "host_drivers_main: cannot read %s\n", argv[first + k]); return 2; }
        in[2 * k] = in[2 * k + 1] = data[k]; size[2 * k] = size[2 * k + 1] = n;
        want[2 * k] = want[2 * k + 1] = count_pictures(data[k], n, max_pictures);
        CHECK(want[2 * k] > 0 && want[2 * k] <= MAX_PICS, "%s: %lld pictures", argv[first + k], (long long)want[2 * k]);
    }
    if (g_fail) return 1;

    /* ---- 1. two ranks, one process */
    frames_t F = { S, calloc((size_t)S, sizeof *F.sum), got };
    worker_arg_t w; memset(&w, 0, sizeof w);
    w.port = free_port();
    pthread_t tid;
    if (!F.sum || w.port < 0 || pthread_create(&tid, NULL, worker_main, &w)) { fprintf(stderr, "host_drivers_main: cannot start\n"); return 2; }
    p264fan_transport_t t;
    p264fan_stats_t st; memset(&st, 0, sizeof st);
    if (p264fan_tcp_transport(&t, 0, 2, NULL, w.port)) { fprintf(stderr, "host_drivers_main: root transport: %s\n", p264fan_last_error()); return 2; }   /* (the worker gives up by itself) */
    p264fan *f = p264fan_open(0, 2, &t, &g_sum_backend, 0);
    CHECK(f != NULL, "p264fan_open: %s", p264fan_last_error());
    if (f) {
        const int rc = p264fan_root_run(f, S, in, size, max_pictures, on_frame, &F, &st);
        CHECK(rc == 0, "p264fan_root_run: %s", p264fan_last_error());
        p264fan_close(f);
    } else if (t.close) t.close(t.ctx);
    pthread_join(tid, NULL);
    CHECK(w.rc == 0, "worker: %s", w.err);
    int64_t total = 0;
    for (int s = 0; s < S; s++) {
        total += want[s];
        CHECK(got[s] == want[s], "fan-out: stream %d brought %lld pictures, its file has %lld", s, (long long)got[s], (long long)want[s]);
    }
    CHECK(st.pictures == total && st.pictures_remote == total / 2 && st.world == 2, "fan-out: %lld pictures (%lld remote), expected %lld", (long long)st.pictures, (long long)st.pictures_remote, (long long)total);
    for (int s = 0; s < S && !g_fail; s += 2)
        for (int64_t i = 0; i < want[s]; i++)
            CHECK(F.sum[s][i] == F.sum[s + 1][i], "fan-out: picture %lld of stream %d (root) and of stream %d (worker) differ", (long long)i, s, s + 1);
    printf("fan-out: %lld pictures in %d rounds, %lld through the worker\n", (long long)st.pictures, st.rounds, (long long)st.pictures_remote);
    free(F.sum);

    /* ---- 2. the pipeline's parsers alone, three threads */
    p264pipe *p = p264pipe_open(-1, S, 3);
    CHECK(p != NULL, "p264pipe_open failed");
    if (p) {
        p264pipe_stats_t ps; memset(&ps, 0, sizeof ps);
        for (int s = 0; s < S; s++) CHECK(p264pipe_set_input(p, s, in[s], size[s]) == 0, "p264pipe_set_input(%d)", s);
        CHECK(p264pipe_run(p, max_pictures, &ps) == 0, "p264pipe_run failed");
        for (int s = 0; s < S; s++)
            CHECK(p264pipe_stream_pictures(p, s) == want[s], "pipeline: stream %d has %lld pictures, its file has %lld", s, (long long)p264pipe_stream_pictures(p, s), (long long)want[s]);
        CHECK(ps.pictures == total && ps.streams == S && ps.threads == (S < 3 ? S : 3), "pipeline: %lld pictures on %d threads, expected %lld", (long long)ps.pictures, ps.threads, (long long)total);
        printf("pipeline: %lld pictures in %d rounds on %d threads\n", (long long)ps.pictures, ps.rounds, ps.threads);
        p264pipe_close(p);
    }
    for (int k = 0; k < n_files; k++) free(data[k]);
    printf(g_fail ? "FAILED\n" : "ok\n");
    return g_fail;
}
