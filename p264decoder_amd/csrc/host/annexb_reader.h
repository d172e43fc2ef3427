/* annexb_reader.h - one Annex-B stream read picture by picture: next NAL unit, RBSP buffer, p264_nal_decode, p264parse_nal,
 * until a picture completes.  Shared by the host drivers (pipeline.c, fanout.c); one reader belongs to one thread at a time.
 * `failed` alone may be read by another thread while the reader runs, hence the relaxed atomics. */
#ifndef P264AMD_ANNEXB_READER_H
#define P264AMD_ANNEXB_READER_H
#include <stdint.h>
#include <stdlib.h>
#include "p264parse.h"
#include "p264_dropin.h"

typedef struct {
    p264parse *parser;                   /* the caller opens it; annexb_reader_close closes it */
    const uint8_t *in; int64_t size, pos;
    uint8_t *rbsp; int64_t rbsp_cap;
    int done;                            /* end of the stream, the picture limit, or a failure */
    int failed;                          /* (atomic) a NAL unit did not parse, or no memory for the RBSP buffer */
    int64_t pictures;
} annexb_reader_t;

static inline void annexb_reader_set_input(annexb_reader_t *r, const uint8_t *annexb, int64_t size)
{
    r->in = annexb; r->size = size; r->pos = 0; r->done = 0; r->pictures = 0;
    __atomic_store_n(&r->failed, 0, __ATOMIC_RELAXED);
}
static inline int annexb_reader_failed(annexb_reader_t *r) { return __atomic_load_n(&r->failed, __ATOMIC_RELAXED); }
static inline const p264hip_picture_t *annexb_reader_fail(annexb_reader_t *r)
{
    __atomic_store_n(&r->failed, 1, __ATOMIC_RELAXED); r->done = 1;
    return NULL;
}
/* the stream's next picture (its arrays live until the next call), or NULL: at the end of the stream, at max_pictures (> 0)
 * or on a failure, which sets `failed` - and `done` in every case */
static inline const p264hip_picture_t *annexb_reader_next(annexb_reader_t *r, int max_pictures)
{
    if (r->done || (max_pictures > 0 && r->pictures >= max_pictures)) { r->done = 1; return NULL; }
    int64_t off, len;
    while (p264_annexb_next(r->in, r->size, &r->pos, &off, &len)) {
        if (len < 1) continue;
        if (len + 8 > r->rbsp_cap) {
            free(r->rbsp); r->rbsp_cap = len * 2 + 64; r->rbsp = (uint8_t *)malloc((size_t)r->rbsp_cap);
            if (!r->rbsp) { r->rbsp_cap = 0; return annexb_reader_fail(r); }
        }
        p264_nal_t nal; nal.p_payload = r->rbsp;
        p264_nal_decode(&nal, (void *)(r->in + off), (int)len);
        const p264hip_picture_t *pic = NULL;
        const int rc = p264parse_nal(r->parser, nal.i_type, nal.i_ref_idc, nal.p_payload, nal.i_payload, &pic);
        if (rc < 0) return annexb_reader_fail(r);
        if (rc == 1) { r->pictures++; return pic; }
    }
    r->done = 1;
    return NULL;
}
static inline void annexb_reader_close(annexb_reader_t *r)
{
    if (r->parser) p264parse_close(r->parser);
    free(r->rbsp);
    r->parser = NULL; r->rbsp = NULL; r->rbsp_cap = 0;
}
#endif
