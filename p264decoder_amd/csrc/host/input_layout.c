/* input_layout.c - the layout of a picture's arrays inside an input slot of the HIP layer (include/p264hip.h), and the host
 * side of it: packing a parsed picture into one block and viewing such a block as a picture again.  Pure host code (the
 * stream fan-out packs pictures on the rank that parses them, include/p264fan.h); the device side is p264hip.hip. */
#include <string.h>
#include "p264hip.h"
#include "host_cpu.h"

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

int p264hip_input_layout(const p264hip_picture_t *d, p264hip_input_layout_t *o)
{
    if (!d || !o || d->mb_w < 1 || d->mb_h < 1 || d->mb_w > 4096 || d->mb_h > 4096) return P264HIP_EINVAL;
    const size_t n = (size_t)d->mb_w * (size_t)d->mb_h;
    memset(o, 0, sizeof *o);
    o->off_mb = 0;
    o->off_mv = up256(n * sizeof(p264hip_mb_t));
    o->off_ref = o->off_mv + up256(n * 64);
    o->off_i4 = o->off_ref + up256(n * 4);
    o->off_coef = o->off_i4 + up256(n * 16);
    size_t end = o->off_coef + up256((size_t)d->n_coef_blocks * 32) + 256;      /* (+256: the kernels' 16-byte loads of the last block's tail) */
    if (d->slice_type == P264_SLICE_B) {
        o->off_mv_l1 = end;
        o->off_ref_l1 = o->off_mv_l1 + up256(n * 64);
        o->off_weights = o->off_ref_l1 + up256(n * 4);
        end = o->off_weights + 512;
    }
    if (d->explicit_wp) {                                                       /* (unweighted pictures: the layout of before, byte for byte) */
        o->off_wp = end;
        end += up256(sizeof d->wp);
    }
    if (d->scaling_lists) {                                                     /* (flat pictures: the layout of before, byte for byte) */
        o->off_scaling = end;
        end += up256(P264HIP_SCALING_BYTES);
    }
    o->bytes = end;
    return P264HIP_OK;
}

int64_t p264hip_pack_input(const p264hip_picture_t *p, void *dst_, size_t cap)
{
    if (p264amd_cpu_refuse("p264hip_pack_input")) return P264HIP_EINVAL;
    p264hip_input_layout_t L;
    if (!p || !dst_ || p264hip_input_layout(p, &L)) return P264HIP_EINVAL;
    if (cap < L.bytes) return P264HIP_ENOMEM;
    if (!p->mb || !p->mv || !p->ref_idx || !p->i4modes || (p->n_coef_blocks && !p->coefs)) return P264HIP_EINVAL;
    const int isB = p->slice_type == P264_SLICE_B;
    if (isB && (!p->mv_l1 || !p->ref_idx_l1)) return P264HIP_EINVAL;
    const size_t n = (size_t)p->mb_w * (size_t)p->mb_h;
    if (p264hip_records_check_pic(p, p->mb) >= 0) return P264HIP_EINVAL;
    uint8_t *dst = (uint8_t *)dst_;
    memcpy(dst + L.off_mb, p->mb, n * sizeof(p264hip_mb_t));
    memcpy(dst + L.off_mv, p->mv, n * 64);
    memcpy(dst + L.off_ref, p->ref_idx, n * 4);
    memcpy(dst + L.off_i4, p->i4modes, n * 16);
    if (p->n_coef_blocks) memcpy(dst + L.off_coef, p->coefs, (size_t)p->n_coef_blocks * 32);
    if (isB) {
        memcpy(dst + L.off_mv_l1, p->mv_l1, n * 64);
        memcpy(dst + L.off_ref_l1, p->ref_idx_l1, n * 4);
        memcpy(dst + L.off_weights, p->bipred_weight, sizeof p->bipred_weight);
    }
    if (p->explicit_wp) {
        if (p264hip_wp_check(p)) return P264HIP_EINVAL;
        memcpy(dst + L.off_wp, p->wp, sizeof p->wp);
    }
    if (p->scaling_lists) {                                                     /* scaling4x4 then scaling8x8: contiguous in the descriptor too */
        memcpy(dst + L.off_scaling, p->scaling4x4, sizeof p->scaling4x4);
        memcpy(dst + L.off_scaling + sizeof p->scaling4x4, p->scaling8x8, sizeof p->scaling8x8);
    }
    return (int64_t)L.bytes;
}

/* The rule every road into a slot holds the macroblock records to: a macroblock's packed blocks lie inside coefs[] (the
 * kernels index the coefficient stream without further checks), an I_PCM record carries its twelve-block mask (the intra
 * kernels read twelve blocks of samples), and a record with P264_MB_T8X8 is inter with whole luma nibbles (k_t8x8 reads four
 * entries per set nibble), and a record with P264_MB_I8X8 is I4x4 with whole luma nibbles and without P264_MB_T8X8 (the Intra 8x8
 * instances of the intra kernels read four entries per set nibble; every other kernel knows no intra 8x8 block).  The index of the first record that breaks it, or -1.  On the
 * device, for blocks that never pass through the host: k_check_records (p264hip.hip). */
int64_t p264hip_records_check(const p264hip_mb_t *mb, size_t n_mb, uint32_t n_coef_blocks)
{
    for (size_t i = 0; i < n_mb; i++) {
        const p264hip_mb_t *m = &mb[i];
        if (m->coef_mask && (uint64_t)m->coef_index + (uint64_t)__builtin_popcount(m->coef_mask & 0x3ffffffu) > n_coef_blocks) return (int64_t)i;
        if (m->mb_type == P264_MB_IPCM && m->coef_mask != P264_IPCM_COEF_MASK) return (int64_t)i;
        if (m->intra_modes & P264_MB_T8X8) {
            const uint32_t lo = m->coef_mask & 0x1111u;                          /* whole nibbles: every bit equals its nibble's lowest */
            if (P264_MB_IS_INTRA(m->mb_type) || (m->coef_mask & 0xffffu) != lo * 15u) return (int64_t)i;
        }
        if (m->intra_modes & P264_MB_I8X8) {
            const uint32_t lo = m->coef_mask & 0x1111u;
            if (m->mb_type != P264_MB_I4x4 || (m->intra_modes & P264_MB_T8X8) || (m->coef_mask & 0xffffu) != lo * 15u) return (int64_t)i;
        }
    }
    return -1;
}

int64_t p264hip_records_check_pic(const p264hip_picture_t *d, const p264hip_mb_t *mb)
{
    const size_t n = (size_t)d->mb_w * (size_t)d->mb_h;
    const int64_t bad = p264hip_records_check(mb, n, d->n_coef_blocks);
    if (bad >= 0) return bad;
    /* the flags the descriptor does not announce */
    const int off = ((d->transform_8x8 & ~P264_T8X8_INTRA) ? 0 : P264_MB_T8X8) | ((d->transform_8x8 & P264_T8X8_INTRA) ? 0 : P264_MB_I8X8);
    if (!off) return -1;
    for (size_t i = 0; i < n; i++) if (mb[i].intra_modes & off) return (int64_t)i;
    return -1;
}

/* the ranges of H.264 7.4.3.2 (include/p264hip.h): denominators 0 .. 7, offsets -128 .. 127, weights -128 .. 128 (128: the
 * inferred 2^7 of a reference without coded weights).  What pairs of a B picture add up to is the parser's check (it is a rule
 * for the stream; every sum gives a defined result here). */
int p264hip_wp_check(const p264hip_picture_t *p)
{
    if (!p->explicit_wp) return 0;
    if (p->weighted_bipred || p->slice_type == P264_SLICE_I) return P264HIP_EINVAL;
    for (int c = 0; c < 2; c++) if (p->wp_log2_denom[c] < 0 || p->wp_log2_denom[c] > 7) return P264HIP_EINVAL;
    for (int l = 0; l < 2; l++)
        for (int i = 0; i < P264HIP_MAX_REFS; i++)
            for (int c = 0; c < 3; c++)
                if (p->wp[l][i][c][0] < -128 || p->wp[l][i][c][0] > 128 || p->wp[l][i][c][1] < -128 || p->wp[l][i][c][1] > 127) return P264HIP_EINVAL;
    return 0;
}

int p264hip_unpack_input(const p264hip_picture_t *desc, const void *packed, size_t bytes, p264hip_picture_t *pic)
{
    if (p264amd_cpu_refuse("p264hip_unpack_input")) return P264HIP_EINVAL;
    p264hip_input_layout_t L;
    if (!desc || !packed || !pic || p264hip_input_layout(desc, &L) || bytes < L.bytes) return P264HIP_EINVAL;
    const uint8_t *b = (const uint8_t *)packed;
    *pic = *desc;
    pic->mb = (const p264hip_mb_t *)(b + L.off_mb);
    pic->mv = (const int16_t *)(b + L.off_mv);
    pic->ref_idx = (const int8_t *)(b + L.off_ref);
    pic->i4modes = b + L.off_i4;
    pic->coefs = (const int16_t *)(b + L.off_coef);
    pic->mv_l1 = NULL; pic->ref_idx_l1 = NULL;
    if (desc->slice_type == P264_SLICE_B) {
        pic->mv_l1 = (const int16_t *)(b + L.off_mv_l1);
        pic->ref_idx_l1 = (const int8_t *)(b + L.off_ref_l1);
    }
    if (desc->explicit_wp) memcpy(pic->wp, b + L.off_wp, sizeof pic->wp);     /* the table the block carries (what the kernels read) */
    if (desc->scaling_lists) {                                                /* and the block's scaling lists */
        memcpy(pic->scaling4x4, b + L.off_scaling, sizeof pic->scaling4x4);
        memcpy(pic->scaling8x8, b + L.off_scaling + sizeof pic->scaling4x4, sizeof pic->scaling8x8);
    }
    return P264HIP_OK;
}
