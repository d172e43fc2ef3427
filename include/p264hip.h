/* p264hip.h - C ABI of the MI355X (gfx950) macroblock-reconstruction layer.
 *
 * This is the CPU->GPU seam of the decoder: the host keeps the serial CAVLC
 * parse and hands one p264hip_picture_t per coded picture to this layer, which
 * runs dequant + inverse transforms, intra prediction, motion compensation and
 * the in-loop deblocking filter as hand-written HIP kernels.
 *
 * What each entry point stands in for in the reference (lspbeyond/p264decoder):
 *   p264hip_picture_t / p264hip_mb_t  <- what p264_macroblock_decode and the deblocking
 *        driver read from h->mb.* / h->dct.*  (core/core.h:330-341, 344-463)
 *   p264hip_submit / p264hip_reconstruct <- the per-MB reconstruction driver
 *        decoder/macroblock.c:755-934 plus the picture post-process sequence
 *        decoder/decoder.c:635-661 (deblock; the border pads and half-pel planes are
 *        replaced by clamped on-the-fly interpolation inside the MC kernel)
 *   p264hip_read_frame  <- the plane aliasing at decoder/decoder.c:652-657
 *   frame slots          <- h->frames.reference[] (decoder/lists.c:152-228)
 *
 * Plain C types only (no torch / C++ types).  All functions return 0 on success and a
 * negative P264HIP_E* code on failure; p264hip_last_error() gives a message.
 */
#ifndef P264HIP_H
#define P264HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P264HIP_MAX_REFS 16

/* macroblock classes (our own numbering; cf. core/macroblock.h:42-65) */
enum {
    P264_MB_I4x4   = 0,
    P264_MB_I16x16 = 1,
    P264_MB_IPCM   = 2,   /* I_PCM: 384 samples instead of levels, see P264_IPCM_COEF_MASK (the reference rejects the type,
                             decoder/macroblock.c:510-514: H.264 7.3.5, 8.3.5) */
    P264_MB_P_L0   = 3,   /* 16x16, 16x8, 8x16 */
    P264_MB_P_8x8  = 4,
    P264_MB_P_SKIP = 5,
    P264_MB_B      = 6    /* any inter macroblock of a B picture (B_L0 / B_L1 / B_Bi / B_8x8 / direct / skip): which list(s)
                             an 8x8 quadrant predicts from is given by ref_idx[] / ref_idx_l1[] (>= 0 = used); the
                             reference's partition walk is core/macroblock.c:525-631, 677-765 */
};
#define P264_MB_IS_INTRA(t) ((t) <= P264_MB_IPCM)

enum { P264_SLICE_P = 0, P264_SLICE_B = 1, P264_SLICE_I = 2 };

enum {
    P264HIP_OK = 0,
    P264HIP_EINVAL = -1,
    P264HIP_ENODEV = -2,      /* no usable HIP device: the product never falls back to the CPU */
    P264HIP_ENOMEM = -3,
    P264HIP_EHIP = -4
};

/* coef_mask bits */
#define P264_COEF_LUMA_DC   (1u << 24)   /* Intra16x16 DC block present (16 levels, zig-zag order) */
#define P264_COEF_CHROMA_DC (1u << 25)   /* one packed block: Cb DC[0..3], Cr DC[4..7] (raster 2x2) */

/* An I_PCM macroblock (mb_type P264_MB_IPCM, in a picture of any slice type) carries its samples where other macroblocks
 * carry levels: TWELVE consecutive 32-byte blocks of coefs[] from coef_index, read as 384 bytes in bitstream order - 256 luma
 * (raster, 16 per row), 64 Cb, 64 Cr (raster, 8 per row).  Its record: coef_mask = P264_IPCM_COEF_MASK exactly (popcount 12: the
 * range rule "coef_index + popcount(coef_mask & 0x3ffffff) <= n_coef_blocks" covers the samples as it covers levels, and so do
 * the compact format's per-block sums), qp = 0 (H.264 8.7.2.2: the loop filter treats its edges with qPp = 0; the filter reads
 * the record's qp), cbp = 0, intra_modes = 0; flags: its slice's filter-offset deltas, like any other macroblock; ref_idx -1, vectors 0, the sixteen i4modes 2, like every macroblock
 * that is not Intra4x4.  avail and edges mean what they mean everywhere.  Every road into an input slot (p264hip_upload,
 * p264hip_pack_input, p264hip_pack_compact, p264hip_compact_check, the device check behind p264hip_input_commit) rejects an
 * I_PCM record with any other mask: the kernels read twelve blocks whatever the mask says. */
#define P264_IPCM_COEF_MASK 0x00000fffu
#define P264_IPCM_BLOCKS    12

/* transform_size_8x8_flag (High profile, H.264 7.3.5 / 8.5.13): bit 2 of intra_modes - free on every record, inter records
 * leave the rest of the byte 0 - says that the macroblock's luma residual is coded as 8x8 blocks.  Legal on INTER records only
 * (mb_type >= P264_MB_P_L0), in pictures whose descriptor says transform_8x8 != 0.  On a flagged record
 *   bits 0-15 of coef_mask come in nibbles: nibble k (bits 4k .. 4k+3) is 0xF where luma 8x8 block k (the quadrants in raster
 *   order) has a non-zero level, else 0x0;
 *   a coded 8x8 block occupies FOUR consecutive 16-level entries of the packed stream: its 64 levels in the 8x8 frame zig-zag
 *   order (entry j holds scan positions 16j .. 16j+15).
 * The range rule (coef_index + popcount(mask) <= n_coef_blocks), the compact format's int8 / int16 choice per entry and the loop
 * filter's "the block that holds the sample has coefficients" (8.7.2.1: the 8x8 block, for such a macroblock) read the mask as
 * they read any other.  Chroma (bits 16-25, its entries behind the luma ones) is as on every record; the levels are scaled with
 * list 7 of a picture with scaling_lists, else with flat lists.  The loop filter leaves the macroblock's inner luma edges 1 and 3 alone (8.7: no transform edges).  Every
 * road into an input slot (the list at P264_IPCM_COEF_MASK) rejects a flagged record that is not inter, one whose luma nibbles are
 * neither 0x0 nor 0xF, and one in a picture whose descriptor says 0. */
#define P264_MB_T8X8 0x04

/* Intra 8x8 prediction (High profile, H.264 8.3.2: an I_NxN macroblock with transform_size_8x8_flag 1): bit 3 of intra_modes.
 * Legal only on records of mb_type P264_MB_I4x4 - the type stays I4x4, so availability, constrained intra prediction, the work
 * lists and P264_MB_IS_INTRA see what they see on any Intra4x4 record - in pictures whose descriptor carries P264_T8X8_INTRA in
 * transform_8x8, and never together with P264_MB_T8X8.  On a flagged record
 *   the luma bits of coef_mask and the luma entries are laid out as on a P264_MB_T8X8 record (whole nibbles; four consecutive
 *   entries per coded 8x8 block, its 64 levels in the 8x8 frame zig-zag order);
 *   i4modes[4k .. 4k+3] all hold Intra8x8PredMode of 8x8 block k (decode-order indices 4k .. 4k+3 are quadrant k), so that the
 *   mode predictor of a neighbouring Intra4x4 block (8.3.1.1) and the compact format read them as they read any other;
 *   chroma, cbp, qp, avail, edges and flags are as on any Intra4x4 record.
 * The loop filter leaves luma edges 1 and 3 alone, as for P264_MB_T8X8.  Every road into an input slot (the list at
 * P264_IPCM_COEF_MASK) rejects a flagged record that is not I4x4, one whose luma nibbles are neither 0x0 nor 0xF, one that also
 * carries P264_MB_T8X8 and one in a picture whose descriptor lacks P264_T8X8_INTRA. */
#define P264_MB_I8X8 0x08
/* bits of p264hip_picture_t.transform_8x8 */
#define P264_T8X8_INTRA 2

/* One per macroblock, 16 bytes.  Everything is as parsed (before dequantisation). */
typedef struct p264hip_mb {
    uint8_t  mb_type;      /* P264_MB_* */
    uint8_t  qp;           /* luma QP as the reference stores it for the MB (core/macroblock.c:1247-1252) */
    uint8_t  cbp;          /* bits 0-3: luma 8x8 coded, bits 4-5: chroma (0 none, 1 DC, 2 DC+AC) */
    uint8_t  intra_modes;  /* bits 0-1 intra16x16_pred_mode, bits 4-5 intra_chroma_pred_mode (as coded) */
    uint32_t coef_mask;    /* bit b<24: 4x4 block b has total_coeff>0 (0-15 luma in decode order
                              core/macroblock.h:194-201, 16-19 Cb, 20-23 Cr); | P264_COEF_* */
    uint32_t coef_index;   /* index, in 16-level blocks, of this MB's first packed block (I_PCM: of its first sample block) */
    uint8_t  avail;        /* P264_AVAIL_*: neighbouring MBs usable for intra prediction (core/macroblock.c:926-1033): inside the
                              picture, in this macroblock's slice and - for an intra macroblock of a picture with
                              constrained_intra_pred_flag - intra themselves; the four flags are independent, any of the
                              sixteen combinations may occur */
    uint8_t  edges;        /* P264_EDGE_*: which MB edges the loop filter touches (core/frame.c:524) */
    uint16_t flags;        /* the macroblock's loop-filter offsets, as signed DELTAS on the picture's: bits 0-7 (int8) are added to
                              p264hip_picture_t.alpha_c0_offset, bits 8-15 (int8) to beta_offset - in the units of those fields, as
                              given (the unshifted convention of the descriptor stays).  The offsets that govern an edge are those
                              of the macroblock whose left, top or inner edge is filtered (H.264 8.7.2.2: filterOffsetA / B of the
                              slice that holds q0); both macroblocks' QPs still count.  0 = the picture's offsets: what every
                              record said while the field was reserved.  Any int8 pair is legal - indexA / indexB are clipped to
                              0 .. 51 - so no upload path checks or refuses anything here; every road into an input slot
                              (p264hip_upload, the packed and compact forms, reserve / commit, p264hip_clone_picture) carries
                              the record's sixteen bytes unchanged.  The host parser writes (slice's offsets - picture's), 0 in
                              slices that do not filter */
} p264hip_mb_t;

#define P264_AVAIL_LEFT     1
#define P264_AVAIL_TOP      2
#define P264_AVAIL_TOPRIGHT 4
#define P264_AVAIL_TOPLEFT  8
#define P264_EDGE_LEFT      1   /* filter the left MB edge  */
#define P264_EDGE_TOP       2   /* filter the top MB edge   */
#define P264_EDGE_INNER     4   /* filter the inner edges   */

/* Packed coefficient stream: for each MB, in this order and only when present:
 *   [luma DC][chroma DC][block 0]...[block 23]; each entry is int16[16] in scan order
 *   (AC-only blocks - I16x16 luma and all chroma - hold their 15 levels in [0..14], [15]=0). */

typedef struct p264hip_picture {
    int32_t  mb_w, mb_h;
    int32_t  slice_type;            /* P264_SLICE_P / P264_SLICE_I */
    int32_t  chroma_qp_offset;      /* pps chroma_qp_index_offset */
    int32_t  deblock;               /* run the loop filter (decoder/decoder.c:639) */
    int32_t  alpha_c0_offset;       /* used unshifted, as the reference does (core/frame.c:476-478); per macroblock plus the deltas */
    int32_t  beta_offset;           /* of its record's flags.  (The host parser: the offsets of the picture's first slice that filters) */
    int32_t  dst_slot;              /* frame-store slot reconstructed into */
    int32_t  n_ref;                 /* list-0 length */
    int32_t  ref_slot[P264HIP_MAX_REFS];   /* ONE list 0 (and one list 1, one weight table) per picture.  The host parser makes that true for
                                            * pictures whose slices reorder or size their lists differently: the first P / B slice's lists
                                            * verbatim, later slices' entries merged into them or appended, their indices remapped */
    uint32_t n_coef_blocks;         /* entries in coefs[] */
    uint32_t frame_num;             /* informational */
    const p264hip_mb_t *mb;         /* [mb_w*mb_h] raster order */
    const int16_t      *mv;         /* [mb][16][2] quarter-pel, 4x4 blocks in raster order inside the MB */
    const int8_t       *ref_idx;    /* [mb][4] per 8x8 (raster), -1 for intra.  An index at or past its list's length (n_ref .. 15;
                                     * ref_idx_l1 the same with n_ref_l1) means entry 0 on every road: the prediction, the implicit
                                     * and explicit weights and the loop filter's reference picture.  The loop filter compares
                                     * reference PICTURES (H.264 8.7.2.1), i.e. the frame-store slots ref_slot[] / ref_slot_l1[] of
                                     * the entries, in P and B pictures alike: two indices that name one slot are one picture.  An
                                     * inter quadrant without any list (negative index, P) counts as list 0, entry 0 */
    const uint8_t      *i4modes;    /* [mb][16] Intra4x4PredMode per block in decode order (0..8) */
    const int16_t      *coefs;      /* [n_coef_blocks][16] */
    /* ---- B pictures only (slice_type == P264_SLICE_B; ignored otherwise).  A quadrant whose list-X index is negative
     * does not predict from list X and its list-X vectors must be 0 (the loop filter compares them, core/frame.c:565-577);
     * both indices >= 0 = bi-prediction: the two predictions are combined as the reference does (core/macroblock.c:543-583):
     * weighted_bipred == 0: (p0 + p1 + 1) >> 1 (core/mc.c:76-88); != 0: clip((p0 * w + p1 * (64 - w) + 32) >> 6) with
     * w = bipred_weight[ref_idx * 16 + ref_idx_l1] (core/mc.c:106-132; the implicit weights of core/macroblock.c:1400-1430,
     * computed by the host from the picture order counts). */
    const int16_t      *mv_l1;      /* [mb][16][2] */
    const int8_t       *ref_idx_l1; /* [mb][4] */
    int32_t             n_ref_l1;   /* list-1 length */
    int32_t             weighted_bipred;
    int32_t             ref_slot_l1[P264HIP_MAX_REFS];
    int16_t             bipred_weight[P264HIP_MAX_REFS * P264HIP_MAX_REFS];   /* [ref_idx][ref_idx_l1], -64 .. 128 */
    /* ---- explicit weighted prediction (H.264 8.4.2.3: P pictures with weighted_pred_flag, B pictures with weighted_bipred_idc 1;
     * no counterpart in the reference, whose pred_weight_table parser is a stub).  explicit_wp != 0: every inter prediction of
     * the picture is weighted - one list: Clip1(((p * w + 2^(d-1)) >> d) + o) (d = 0: Clip1(p * w + o)); two lists:
     * Clip1(((p0 * w0 + p1 * w1 + 2^d) >> (d + 1)) + ((o0 + o1 + 1) >> 1)) - with d = wp_log2_denom[plane != 0] (0 .. 7),
     * (w, o) = wp[list][ref_idx][plane] (offsets -128 .. 127; weights -128 .. 128, where 128 is only the inferred 2^7 of a reference
     * without coded weights; a stream keeps the pairs its blocks use within -128 <= w0 + w1 <= (d == 7 ? 127 : 128), any sum gives
     * a defined result here).  weighted_bipred must be 0 then.  Explicit pictures carry the table in their input slot (off_wp
     * below): p264hip_upload copies the descriptor's, the packed and compact roads carry the block's. */
    int32_t             explicit_wp;
    int32_t             wp_log2_denom[2];                                      /* luma, chroma */
    int16_t             wp[2][P264HIP_MAX_REFS][3][2];                         /* [list][ref_idx][Y, Cb, Cr][weight, offset] */
    /* ---- the 8x8 transform, a bit set.  Bit 1 (P264_T8X8_INTRA): Intra4x4 records of the picture may carry P264_MB_I8X8, and a
     * batch that holds the picture launches the Intra 8x8 instances of the intra kernels (k_intra_i8 / k_intra_sparse_i8).  Any
     * other bit: inter records of the picture may carry P264_MB_T8X8, and a batch that holds the picture launches the kernel that
     * adds their luma residual (k_t8x8, between motion compensation and intra prediction).  0 and 1 mean what they always meant. */
    int32_t             transform_8x8;
    /* ---- scaling matrices (High profile, H.264 7.3.2.1.1.1, 8.5.9: LevelScale = weightScale * normAdjust).  scaling_lists != 0: the
     * levels of the picture are scaled with the eight lists below instead of Flat_4x4_16 / Flat_8x8_16 - 4x4: 0 Intra Y, 1 Intra Cb,
     * 2 Intra Cr, 3 Inter Y, 4 Inter Cb, 5 Inter Cr; 8x8: 0 Intra Y (list 6, records with P264_MB_I8X8), 1 Inter Y (list 7, records
     * with P264_MB_T8X8) - RESOLVED (defaults and fall-backs applied) and in SCAN order: weight [k] belongs to scan position k, the
     * order the levels of an entry are in (an AC-only entry holds scan positions 1 .. 15 at [0 .. 14]: its level [k] pairs with weight
     * [k + 1]).  Intra or inter is the macroblock's, not the picture's.  Any byte is legal (0 zeroes the coefficient), no road checks
     * or refuses anything here.  Such a picture carries the 224 bytes in its input slot (off_scaling below): p264hip_upload copies the
     * descriptor's, the packed and compact roads carry the block's.  A batch that holds such a picture launches instances of the sort
     * and intra kernels that know the table and a kernel that adds the residual of its inter macroblocks (k_scaled_inter);
     * 0 = flat: what every zeroed descriptor says. */
    int32_t             scaling_lists;
    uint8_t             scaling4x4[6][16];
    uint8_t             scaling8x8[2][64];
    /* ---- Cr's own QP offset (High profile, H.264 7.3.2.2: second_chroma_qp_index_offset), as a DELTA on chroma_qp_offset:
     * second_chroma_qp_index_offset - chroma_qp_index_offset.  Cb's qPI is Clip3(0, 51, QPY + chroma_qp_offset) as ever, Cr's is
     * Clip3(0, 51, QPY + chroma_qp_offset + cr_qp_offset_delta): in the chroma residual (8.5.8, 8.5.11) of inter and intra
     * macroblocks and in the loop filter's indexA / indexB / tc0 of Cr's edges (8.7.2.2), those of I_PCM macroblocks included (QPY 0
     * with the plane's offset).  Any int gives a defined result, no road checks or refuses anything here; a stream's offsets are
     * -12 .. 12 each, its delta -24 .. 24.  A descriptor scalar: it travels beside the packed and compact blocks, whose layouts do
     * not know it.  A batch that holds a picture with a non-zero delta runs that picture through the instances that read the
     * scaling table (with the all-16 table where it has no lists: scaling_lists above) and launches the Cr instances of the loop
     * filter's two kernels (k_deblock_bs_cr, k_deblock_cr); 0 = Cr uses chroma_qp_offset: what every zeroed descriptor says. */
    int32_t             cr_qp_offset_delta;
} p264hip_picture_t;
#define P264HIP_SCALING_BYTES 224                    /* scaling4x4 and scaling8x8 back to back: the table as it lies in a slot and in a compact block */

typedef struct p264hip_ctx p264hip_ctx;

/* Device context: n_streams independent frame stores of `slots` frames each (4:2:0, MB-aligned,
 * no padding; kept macroblock-tiled in HBM - the host only ever sees planes, through
 * p264hip_read_frame / p264hip_write_frame) and `max_pictures` device-resident picture inputs. */
int  p264hip_create(p264hip_ctx **out, int device, int mb_w, int mb_h,
                    int n_streams, int slots, int max_pictures);
void p264hip_destroy(p264hip_ctx *ctx);
const char *p264hip_last_error(void);
int  p264hip_device_count(void);

/* Copy parsed pictures host->HBM into resident input slots [first, first+n). Asynchronous. */
int  p264hip_upload(p264hip_ctx *ctx, int first, const p264hip_picture_t *pics, int n);
/* The same without the final wait: the copies are only enqueued.  The picture's arrays must stay untouched until
 * a marker taken after this call has been reached (p264hip_marker / p264hip_marker_wait) or p264hip_sync returns;
 * they should live in pinned memory (p264hip_host_alloc) for the copies to be real DMA transfers. */
int  p264hip_upload_async(p264hip_ctx *ctx, int slot, const p264hip_picture_t *pic);
/* Both notice arrays that already lie in host memory the way an input slot is laid out (p264hip_input_layout_t below: the
 * parser of this library builds its pictures like that) and then copy records, vectors, indices, modes and levels in ONE
 * transfer instead of five.  Host -> HBM copies queued so far by the two calls (diagnostic; -1 without a context): */
int64_t p264hip_upload_copies(p264hip_ctx *ctx);
/* Pinned host memory for picture inputs and frame downloads; usable without a context.  Ordinary (huge) pages registered with
 * the runtime - the CPU writes and re-reads them at full speed, which it does not on hipHostMalloc'ed memory;
 * P264AMD_HOST_ALLOC = 0 gives hipHostMalloc back. */
void *p264hip_host_alloc(size_t bytes);
void  p264hip_host_free(void *p);
/* A marker is a point in the context's stream; marker_wait blocks the calling host thread until everything
 * enqueued before the marker has completed.  Markers are small integers >= 0 (a ring of P264HIP_MARKERS). */
#define P264HIP_MARKERS 8
int  p264hip_marker(p264hip_ctx *ctx);
int  p264hip_marker_wait(p264hip_ctx *ctx, int marker);
/* Device-side copy of resident picture `src` into slot `dst` (private HBM copy; bench set-up). */
int  p264hip_clone_picture(p264hip_ctx *ctx, int dst, int src);

/* ---- the layout of a picture's arrays inside its input slot, and ways into the slot that do not pass through
 * p264hip_upload's five copies.  An input slot is ONE block of device memory with the arrays at 256-byte aligned offsets
 * (a pure function of mb_w, mb_h, n_coef_blocks and slice_type).  A host buffer packed in this layout goes into a slot
 * with one copy (p264hip_upload_packed); a producer that can write device memory itself - the RCCL transport of the
 * stream fan-out receiving a picture from another rank (include/p264fan.h) - asks for the slot's address
 * (p264hip_input_reserve), fills it and commits it.  Nothing of this has a counterpart in the reference. */
typedef struct p264hip_input_layout {
    size_t off_mb, off_mv, off_ref, off_i4, off_coef;      /* p264hip_mb_t[n], int16[n][16][2], int8[n][4], uint8[n][16], int16[n_coef_blocks][16] */
    size_t off_mv_l1, off_ref_l1, off_weights;             /* B pictures only (0 otherwise): list-1 vectors, indices, bipred_weight[] */
    size_t bytes;                                          /* of the whole block */
    size_t off_wp;                                         /* explicit_wp pictures only (0 otherwise): wp[][][][], behind everything above */
    size_t off_scaling;                                    /* scaling_lists pictures only (0 otherwise): scaling4x4, scaling8x8 (P264HIP_SCALING_BYTES), behind everything else */
} p264hip_input_layout_t;
int  p264hip_input_layout(const p264hip_picture_t *desc, p264hip_input_layout_t *out);
/* 0, or P264HIP_EINVAL where an explicit_wp picture's denominators, weights or offsets are out of range (every upload path checks it) */
int  p264hip_wp_check(const p264hip_picture_t *desc);
/* the index of the first of n_mb records whose coefficient blocks do not lie inside coefs[n_coef_blocks], which is an I_PCM
 * record without its twelve-block mask, or which carries P264_MB_T8X8 without being inter or with a luma nibble that is neither
 * 0x0 nor 0xF, or which carries P264_MB_I8X8 without being I4x4, with such a nibble or together with P264_MB_T8X8; -1 where there is
 * none (every upload path checks it, device producers' blocks on the device) */
int64_t p264hip_records_check(const p264hip_mb_t *mb, size_t n_mb, uint32_t n_coef_blocks);
/* the same for the records of a picture with this descriptor: also the first record that carries P264_MB_T8X8 where
 * desc->transform_8x8 has no bit other than P264_T8X8_INTRA, or P264_MB_I8X8 where it lacks that bit (what the roads that check on
 * the host run) */
int64_t p264hip_records_check_pic(const p264hip_picture_t *desc, const p264hip_mb_t *mb);
/* host side, no device involved: the picture's arrays copied into `dst` (cap >= layout.bytes) in that layout; the
 * macroblock records are checked as p264hip_upload checks them (coefficient ranges inside coefs[]).  Returns the bytes used
 * or a negative P264HIP_E* code. */
int64_t p264hip_pack_input(const p264hip_picture_t *pic, void *dst, size_t cap);
/* the inverse view: *pic = *desc with its array pointers set into `packed` (nothing is copied) */
int  p264hip_unpack_input(const p264hip_picture_t *desc, const void *packed, size_t bytes, p264hip_picture_t *pic);
/* packed host buffer -> slot, one asynchronous copy (the buffer stays untouched until a marker / p264hip_sync; the records are
 * trusted to have been checked by p264hip_pack_input) */
int  p264hip_upload_packed(p264hip_ctx *ctx, int slot, const p264hip_picture_t *desc, const void *packed, size_t bytes);
/* ---- the compact LINK format (round 6).  A picture's arrays as they travel where the link is the bound (a packed upload over
 * PCIe, a scatter over xGMI / TCP): 1.42 MB per 1080p P picture of the bench stream in the slot layout, ~0.5 MB compact -
 *   records and reference indices verbatim (16 + 4 bytes per macroblock and list);
 *   vectors by shape, 2 bits per macroblock and list: 0 sixteen zero vectors (intra macroblocks, an unused list, a block at
 *   rest), 1 one vector (16x16 / skip), 2 one per 8x8 quadrant, 3 all sixteen;
 *   Intra4x4 modes only for the macroblocks whose sixteen modes are not all 2 (DC: what a parser leaves everywhere else), one
 *   flag bit per macroblock;
 *   coded levels as sixteen int8 per block where every level of the block fits (one flag bit per block), else sixteen int16;
 *   B pictures: the same for list 1, and the 512 bytes of bipred_weight[].
 * Nothing is lost: p264hip_expand_compact (host; the reference of the device kernel) gives back the slot layout byte for byte
 * (p264hip_pack_input's block, up to the padding between its sections).
 * p264hip_upload_compact copies the block into a staging area of the slot (one asynchronous copy, on a side stream of the context)
 * and queues its expansion: ONE kernel expands every picture uploaded since the last one, in front of the next
 * p264hip_reconstruct (or clone / sync), which also is where the context's stream starts to wait for the copies - the caller's
 * block must stay untouched until a marker taken AFTER that call has been reached (or p264hip_sync has returned).
 * Like p264hip_upload_packed the call trusts the block to come from the packer (which checks the records as p264hip_upload
 * does): it checks the header (O(1): p264hip_compact_header_ok - sections inside the block, in order, large enough for the
 * header's counts) and the device clamps every place it derives from the block's bits to its section - an inconsistent block
 * gives a wrong picture, never an access outside the block or the slot.  p264hip_compact_check is the full check (counts implied
 * by the shape and flag bits, records, weights) for blocks from anywhere else. */
#define P264HIP_COMPACT_MAGIC 0x43343632u           /* "264C" */
#define P264HIP_COMPACT_MAX_MB 8192                 /* macroblocks per picture the device expansion takes (its offsets live in LDS) */
typedef struct p264hip_compact_hdr {                /* 128 bytes; sections follow at 16-byte aligned offsets from the block's start */
    uint32_t magic, n_mb, n_coef_blocks, bytes;     /* bytes: of the whole block */
    uint32_t n_lists;                               /* 1; 2 for a B picture */
    uint32_t off_rec, off_i4flag, off_i4, off_lvflag, off_levels, off_weights;      /* off_weights: 0 unless n_lists == 2 */
    uint32_t n_i4, level_bytes;                     /* macroblocks with an Intra4x4 mode entry, bytes of levels */
    struct { uint32_t off_ref, off_shape, off_vec, n_vec; } list[2];               /* n_vec: vectors (dwords) in the list's vec section */
    uint32_t off_wp;                                /* explicit_wp pictures: wp[][][][] (384 bytes), 0 otherwise */
    uint32_t off_scaling;                           /* scaling_lists pictures: the table (P264HIP_SCALING_BYTES), 0 otherwise */
    uint32_t reserved[9];
} p264hip_compact_hdr_t;
/* bytes a compact block of this picture needs at most */
size_t  p264hip_compact_bound(const p264hip_picture_t *pic);
int64_t p264hip_pack_compact(const p264hip_picture_t *pic, void *dst, size_t cap);          /* bytes used, or a negative P264HIP_E* code */
/* host: compact block -> the slot layout (p264hip_input_layout of desc), `out` of at least layout.bytes */
int     p264hip_expand_compact(const p264hip_picture_t *desc, const void *compact, size_t bytes, void *out, size_t cap);
int     p264hip_compact_header_ok(const p264hip_picture_t *desc, const void *compact, size_t bytes);   /* 1 / 0; what upload_compact checks */
int     p264hip_compact_check(const p264hip_picture_t *desc, const void *compact, size_t bytes);       /* 0 or P264HIP_EINVAL; the full check, no device */
int     p264hip_upload_compact(p264hip_ctx *ctx, int slot, const p264hip_picture_t *desc, const void *compact, size_t bytes);

/* device producers: reserve makes room in `slot` for a picture described by desc (scalar fields; its pointers are ignored)
 * and returns where its packed arrays are to be written (it waits for the context's stream only if work that still uses the
 * slot's previous picture is in flight: one wait covers a whole round of reserves); the slot becomes usable with commit, which
 * the caller issues once its writes have completed (the context's stream does not wait for anybody else's).  Commit is
 * P264HIP_EINVAL unless the slot is still reserved: any other road into the slot in between (an upload, a clone into it)
 * takes the reservation back, and a reserved slot that was not committed is empty to p264hip_reconstruct.  commit queues
 * the record check p264hip_upload runs on the host (every macroblock's packed blocks inside coefs[]) as a kernel over the
 * block; p264hip_reconstruct reads the verdicts of a batch's committed pictures with one wait and fails with P264HIP_EINVAL
 * where a block is inconsistent - the producer is not trusted. */
int  p264hip_input_reserve(p264hip_ctx *ctx, int slot, const p264hip_picture_t *desc, void **dev, size_t *bytes);
int  p264hip_input_commit(p264hip_ctx *ctx, int slot);
/* frame `slot` of `stream` converted to planar I420 (Y, U, V back to back, MB-aligned) in device buffer number `index` of
 * the context (buffers are created on demand and live as long as the context); enqueued on the context's stream - *dev is
 * readable by other streams / RCCL after p264hip_sync or a marker. */
int  p264hip_frame_planar_device(p264hip_ctx *ctx, int stream, int slot, int index, void **dev, size_t *bytes);
/* ---- frames handed on ON THE DEVICE: a batch of pictures, cropped to a window, as I420 / NV12 / RGB, in ONE launch into memory
 * the caller owns (a torch tensor's data_ptr(), an encoder's input surface).  Nothing of this has a counterpart in the reference,
 * whose frames leave as MB-aligned planes on the host (decoder/decoder.c:652-657).
 *
 * Layout of one picture in dst, in bytes; P = pitch, W x H = the window (tight P: the value pitch = 0 stands for):
 *   I420   tight P = W    Y row y at y*P; U at P*H, rows P/2 apart, H/2 rows; V at P*H + (P/2)*(H/2).  P even.     P*H*3/2 bytes
 *   NV12   tight P = W    Y as above; ONE plane of interleaved U, V pairs at P*H, rows P apart, H/2 rows           P*H*3/2 bytes
 *   RGB24  tight P = 3W   row y at y*P; pixel x is the bytes R, G, B at 3x                                         P*H bytes
 *   RGBP   tight P = W    three planes of P*H bytes each, in the order R, G, B                                     3*P*H bytes
 * Picture i of a call lies at dst + i*frame_stride (0 = tight: the picture's bytes).  Every byte of dst outside the rows' W
 * (RGB24: 3W) bytes is left untouched: between a row's end and P, between a picture's end and frame_stride.
 *
 * RGB arithmetic (bit-exact; tests/export_checker.py is the same in numpy).  Chroma is the nearest sample, (x >> 1, y >> 1).
 *   channel = clip255((cy*(Y - yo) + cu*(Cb - 128) + cv*(Cr - 128) + 4096) >> 13)     (arithmetic shift)
 * yo = 16 for limited range, 0 for full range; each coefficient is floor(c*8192 + 1/2) of the matrix's exact rational c:
 * Kr, Kb = 0.299, 0.114 (BT.601) or 0.2126, 0.0722 (BT.709), Kg = 1 - Kr - Kb; luma scale 255/219 and chroma scale s = 255/224
 * for limited range, both 1 for full range;  R: cv = 2(1-Kr)s;  G: cu = -2Kb(1-Kb)s/Kg, cv = -2Kr(1-Kr)s/Kg;  B: cu = 2(1-Kb)s:
 *                    cy    R.cv   G.cu   G.cv   B.cu
 *   601 limited     9539  13075  -3209  -6660  16525
 *   601 full        8192  11485  -2819  -5850  14516
 *   709 limited     9539  14686  -1747  -4366  17305
 *   709 full        8192  12901  -1535  -3835  15201
 * Over all 2^24 (Y, Cb, Cr) the result is within 1 of clip(floor(real + 1/2)), and every sum stays below 2^23 in magnitude. */
enum { P264HIP_FMT_I420 = 0, P264HIP_FMT_NV12 = 1, P264HIP_FMT_RGB24 = 2, P264HIP_FMT_RGBP = 3 };
enum { P264HIP_MATRIX_BT601 = 0, P264HIP_MATRIX_BT709 = 1 };
typedef struct p264hip_export {
    int32_t format, matrix, full_range;          /* matrix / full_range: RGB formats only, otherwise must be 0 */
    int32_t crop_left, crop_top, width, height;  /* window of the luma plane, in samples; all four even, width, height > 0 */
    int32_t pitch;                               /* bytes per row of plane 0; 0 = tight */
    int64_t frame_stride;                        /* bytes from one picture to the next in dst; 0 = tight */
} p264hip_export_t;
/* bytes of one picture (host only, no device); < 0 = P264HIP_EINVAL: a null argument, an unknown format or matrix, matrix /
 * full_range on a YUV format, a window with an odd or non-positive member, a pitch below the tight one, an odd pitch for I420 */
int64_t p264hip_export_frame_bytes(const p264hip_export_t *e);
/* 0, or P264HIP_EINVAL for what p264hip_export_frame_bytes refuses, a window that leaves the frame of mb_w x mb_h macroblocks and a
 * frame_stride (other than 0) below the picture's bytes (host only) */
int     p264hip_export_check(const p264hip_export_t *e, int mb_w, int mb_h);
/* picture i = frame slots[i] of stream streams[i], written at dst_dev + i*frame_stride.  Asynchronous on the context's stream: it
 * runs behind every reconstruct queued before it, and dst_dev is complete after p264hip_sync or a marker.  streams[] and slots[]
 * are consumed before the call returns; entries may repeat; n >= 1, bounded only by dst_bytes (more than 65535 pictures go out
 * as several launches).  P264HIP_EINVAL, before anything is queued, for a null argument, n < 1, a stream or slot out of range,
 * whatever p264hip_export_check refuses, and dst_bytes < (n-1)*frame_stride + the picture's bytes.  The kernel writes the bytes
 * listed above and no others. */
int     p264hip_export_frames(p264hip_ctx *ctx, const int *streams, const int *slots, int n,
                              const p264hip_export_t *e, void *dst_dev, size_t dst_bytes);

/* ---- the same road with a RESIZE on it: a source window of each picture resized to width x height, written in one of the four
 * layouts above as uint8, or - the two RGB formats - as float16 / float32 after a per-channel scale and bias.  "The existing export
 * of a virtual width x height picture": with width x height equal to the window it writes the bytes p264hip_export_frames writes.
 *
 * Taps.  Each plane is resized on its own: luma from the window's cw x ch samples to W x H, U and V from cw/2 x ch/2 to W/2 x H/2.
 * Sample centres sit at half positions (the geometry of align_corners = False), positions are in 1/256 of a sample.  For the
 * destination index d of an axis with S source and D destination samples
 *   pos(d) = clamp( floor(((2d+1)*S*256 + D) / (2D)) - 128,  0,  (S-1)*256 )
 *   i0 = pos >> 8,  f = pos & 255,  i1 = min(i0+1, S-1)
 * with indices relative to the window: taps clamp at the WINDOW's edges, a sample outside it is never read (p264hip_resize_taps
 * gives pos[]).  With a, b the samples (i0, i1) of source row j0 and c, d those of row j1, fx and fy the two fractions:
 *   v = (a*(256-fx)*(256-fy) + b*fx*(256-fy) + c*(256-fx)*fy + d*fx*fy + 32768) >> 16
 * Every sum stays below 2^24.  D == S returns the source, D == S/2 is exactly (a+b+c+d+2) >> 2, and the result is within 1 of
 * floor(real bilinear + 1/2) (each axis' position is off by at most 1/512: at most 255/512 per axis, and two roundings of 1/2).
 * This filter (P264HIP_FILTER_BILINEAR, 0) has no antialiasing prefilter: a large reduction aliases exactly as
 * torch.nn.functional.interpolate(mode="bilinear", align_corners=False, antialias=False) does.  For a reduction set `filter` to
 * P264HIP_FILTER_BILINEAR_AA (2), below.  Value 1 is not assigned and is refused.
 *
 * The antialiased filter (P264HIP_FILTER_BILINEAR_AA).  The triangle filter whose half-width grows with the reduction - what PIL's
 * BILINEAR and torch's interpolate(mode="bilinear", align_corners=False, antialias=True) compute -, separable and in integers only.
 * For an axis with S source samples (the window's), D destination samples and the destination index d
 *   U    = 2 * max(S, D)
 *   r(j) = U - | (2j+1)*D - (2d+1)*S |        for the source index j = 0 .. S-1, relative to the window
 *   taps = the j with r(j) > 0                (a contiguous run first .. first+n-1, never empty)
 *   R    = the sum of r(j) over the taps
 *   w(j) = floor( r(j) * 32768 / R )          (64-bit integers)
 *   w(k) += 32768 - sum of w(j)               k = the tap with the largest r, the lowest index among equals
 * The weights are Q15, not negative, and their sum is exactly 32768.  A source sample outside the WINDOW is no tap: it is dropped
 * and the others renormalised (not clamped), and it is never read.  With D >= S this is bilinear at exact rational positions (two
 * taps, D == S: one of 32768); with D == S/2 the inner weights are 1, 3, 3, 1 over 8.  Planes are resized one by one as above,
 * vertically FIRST and then horizontally, with one rounding each:
 *   t(y, c) = ( sum_k wy[y][k] * src[firsty[y]+k][c]  + 256  ) >> 9       0 .. 16320, the sample times 64; sums below 2^23
 *   v(y, x) = ( sum_k wx[x][k] * t(y, firstx[x]+k)    + 2^20 ) >> 21      0 .. 255; sums below 2^30, no clip
 * The order is part of the contract (the two roundings do not commute); vertical first because rows of a strip of the frame
 * store are 16 contiguous bytes one after the other.  Against the real-valued filter |v - real| <= 1/2 + 1/128 + 255*(nx+ny-2)/32768
 * with nx, ny the largest tap counts of the two axes: below 1 for 1080p to 224 x 224, below 2.5 at the limit.  The limit: a
 * description with crop_width > 32 * width or crop_height > 32 * height is refused with this filter, so that an output sample has at
 * most P264HIP_AA_MAX_TAPS taps per axis.  Layouts, RGB and the float step below are the same for both filters;
 * tests/resize_aa_checker.py is this filter in numpy.
 *
 * Layouts.  The resized planes are treated as p264hip_export_t treats a frame: I420 / NV12 store them; RGB24 / RGBP take the chroma
 * sample (x >> 1, y >> 1) of the RESIZED chroma planes and the formula, coefficients and clip above.  The layout table above holds
 * with W x H the output size and every byte count times the element size (1, 2 or 4): tight P = W*elem (RGB24: 3*W*elem).
 *
 * Float elements (RGB24 and RGBP only).  For channel k in the order R, G, B and the 8-bit value c
 *   e = fl32( fl32((float)c * scale[k]) + bias[k] )
 * two separately rounded IEEE single operations, never contracted into one; float16 is e converted round-to-nearest-even with
 * subnormals kept (numpy's astype(float16)).  tests/resize_checker.py is all of this in numpy. */
enum { P264HIP_DTYPE_U8 = 0, P264HIP_DTYPE_F16 = 1, P264HIP_DTYPE_F32 = 2 };
enum { P264HIP_FILTER_BILINEAR = 0, P264HIP_FILTER_BILINEAR_AA = 2 };
#define P264HIP_AA_MAX_TAPS 64
typedef struct p264hip_resize {
    int32_t format, matrix, full_range;                     /* as in p264hip_export_t */
    int32_t crop_left, crop_top, crop_width, crop_height;   /* source window, luma samples, all even, inside the frame */
    int32_t width, height;                                  /* output, both even, 2 .. 16384 */
    int32_t dtype, filter;
    int32_t pitch;                                          /* bytes per row of plane 0; 0 = tight = W*elem (RGB24: 3*W*elem) */
    int64_t frame_stride;                                   /* bytes; 0 = tight */
    float   scale[3], bias[3];                              /* R, G, B; float dtypes only, all 0 otherwise */
} p264hip_resize_t;
/* bytes of one picture (host only, no device); < 0 = P264HIP_EINVAL for what p264hip_export_frame_bytes refuses in the fields the two
 * share, an output size that is odd, below 2 or above 16384, an unknown dtype or filter, a float dtype on a YUV format, a scale or
 * bias that is not finite - or not 0 where the dtype is U8 -, a pitch below the tight one or no multiple of the element size (I420: of
 * twice the element size, as its chroma pitch is pitch/2), and with P264HIP_FILTER_BILINEAR_AA a window more than 32 times the output
 * in width or in height */
int64_t p264hip_resize_frame_bytes(const p264hip_resize_t *r);
/* 0, or P264HIP_EINVAL for the above, a window that leaves the frame of mb_w x mb_h macroblocks and a frame_stride (other than 0)
 * below the picture's bytes or no multiple of the element size (host only) */
int     p264hip_resize_check(const p264hip_resize_t *r, int mb_w, int mb_h);
/* pos[d] above for d = 0 .. dst_n - 1 (host only); P264HIP_EINVAL for a null pos or a count outside 1 .. 2^20 */
int     p264hip_resize_taps(int src_n, int dst_n, int32_t *pos);
/* the taps of P264HIP_FILTER_BILINEAR_AA (host only): first[d], count[d] and the Q15 weights of destination index d in
 * weights[d * P264HIP_AA_MAX_TAPS ..], the entries behind count[d] 0; indices relative to the window.  P264HIP_EINVAL for a null
 * pointer, a count outside 1 .. 2^20 or src_n > 32 * dst_n */
int     p264hip_resize_aa_taps(int src_n, int dst_n, int32_t *first, int32_t *count, uint16_t *weights);
/* the contract of p264hip_export_frames: picture i = frame slots[i] of stream streams[i], resized, at dst_dev + i*frame_stride;
 * asynchronous on the context's stream behind every reconstruct queued before it, complete after p264hip_sync or a marker; entries
 * may repeat; more than 65535 pictures go out as several launches.  P264HIP_EINVAL, before anything is queued, for a null argument,
 * n < 1, a stream or slot out of range, whatever p264hip_resize_check refuses, a dst_dev that is no multiple of the element size and
 * dst_bytes < (n-1)*frame_stride + the picture's bytes.  The kernel writes the bytes of the layout and no others. */
int     p264hip_export_resized(p264hip_ctx *ctx, const int *streams, const int *slots, int n,
                               const p264hip_resize_t *r, void *dst_dev, size_t dst_bytes);

/* ---- the same road with a window PER PICTURE, each resized into a rectangle of the output (a letterbox), in one call: crops of
 * different places in different pictures (a detector's boxes for a second model), or a 1920 x 1080 picture into the 640 x 360
 * middle of a 640 x 640 input with a constant round it.
 *
 * r gives the output as it does for p264hip_export_resized: format, matrix, full_range, width x height (W x H), dtype, pitch,
 * frame_stride, scale, bias, with the same meanings and refusals.  Its crop_* fields are NOT READ: the windows are the ROIs'.
 * Its filter must be P264HIP_FILTER_BILINEAR; the antialiased filter is refused here because it has entry points of its own,
 * p264hip_export_rois_aa and its two siblings below (their limit is per ROI, their taps carry weights and their tile width is chosen
 * per ROI).  fill is Y | Cb << 8 | Cr << 16, bits 24 - 31 must be 0.
 *
 * Output picture i, at dst_dev + i*frame_stride, is the existing export of a VIRTUAL W x H 4:2:0 picture V:
 *   luma    V.Y[y][x] = fill.Y outside the rectangle (dst_left, dst_top, dst_width, dst_height); inside, sample (x - dst_left,
 *           y - dst_top) of the ROI's luma window resized to dst_width x dst_height by exactly the filter-0 arithmetic above - pos(d),
 *           i0, i1, f and the >> 16 sum, S the window's size and D the rectangle's.  Taps clamp at the window's edges; nothing outside
 *           the window is read
 *   chroma  the same with every number halved: fill.Cb / fill.Cr outside, the window's width/2 x height/2 samples to
 *           dst_width/2 x dst_height/2 at (dst_left/2, dst_top/2)
 * and then the layout step of p264hip_resize_t unchanged: I420 / NV12 store the planes of V; RGB24 / RGBP take chroma sample
 * (x >> 1, y >> 1) of V, the fixed-point formula and the clip; the float step is scale / bias as two separately rounded operations.
 * The fill goes through the same RGB and float steps as any sample.  So: with every rectangle the whole output and every ROI naming
 * one window the call writes what p264hip_export_resized writes for that window; a rectangle of the window's own size pastes the
 * window unchanged; the bytes outside the rectangle are those of the export of a constant picture.  tests/roi_checker.py is this
 * in numpy.
 *
 * The taps are made on the device (k_roi_taps) into a scratch area of the context of at most P264HIP_ROI_SCRATCH_BYTES; a call
 * whose ROIs need more goes out as several pairs of launches on the one stream.  Per call the host sends the n descriptors and
 * nothing per destination index.
 *
 * ROI lists that live in device memory - a detector's boxes - have an entry of their own, p264hip_export_rois_device below.
 * Not built: a pipeline sink that takes ROIs; deliveries in output order as ROI sources. */
typedef struct p264hip_roi {            /* 40 bytes */
    int32_t stream, slot;               /* the picture */
    int32_t left, top, width, height;   /* source window, luma samples: all even, width, height > 0, inside the frame */
    int32_t dst_left, dst_top, dst_width, dst_height;   /* where in the W x H output the resized window lands: all even, inside the
                                           output, dst_width, dst_height >= 2; all four 0 = the whole output */
} p264hip_roi_t;
#define P264HIP_ROI_SCRATCH_BYTES (16 << 20)     /* the tap scratch of one pair of launches: 4096 ROIs to 224 x 224 take 11 MB */
/* what p264hip_resize_frame_bytes gives for the same description with a valid window (host only); P264HIP_EINVAL also for a filter
 * other than P264HIP_FILTER_BILINEAR */
int64_t p264hip_rois_frame_bytes(const p264hip_resize_t *r);
/* 0, or P264HIP_EINVAL (host only) for what p264hip_rois_frame_bytes refuses, a frame_stride p264hip_resize_check refuses, a null
 * list, n < 1, a fill with bits above 23, and for any ROI: a stream or slot outside n_streams x slots, a window with an odd or
 * non-positive member or leaving the frame of mb_w x mb_h macroblocks, a rectangle - unless all four members are 0 - with an odd
 * member, below 2 x 2 or leaving the output */
int     p264hip_rois_check(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill,
                           int mb_w, int mb_h, int n_streams, int slots);
/* asynchronous on the context's stream behind every reconstruct queued before it, complete after p264hip_sync or a marker; rois[] is
 * consumed before the call returns; entries may repeat; n >= 1, bounded only by dst_bytes.  P264HIP_EINVAL, before anything is
 * queued, for whatever p264hip_rois_check refuses against the context's geometry (the message names the first bad ROI's index), a
 * dst_dev that is no multiple of the element size, dst_bytes < (n-1)*frame_stride + the picture's bytes, and a frame above 65535
 * samples a side (a tap holds a coordinate in 16 bits).  The kernel writes the bytes of the layout and no others. */
int     p264hip_export_rois(p264hip_ctx *ctx, const p264hip_roi_t *rois, int n, const p264hip_resize_t *r,
                            uint32_t fill, void *dst_dev, size_t dst_bytes);

/* ---- the same three with the ANTIALIASED filter (P264HIP_FILTER_BILINEAR_AA): the letterbox of a 1920 x 1080 picture and a
 * detector's boxes at 224 x 224 are reductions, on which filter 0 aliases.  Everything said of p264hip_export_rois holds, but:
 *   - r->filter must be P264HIP_FILTER_BILINEAR_AA; every other value is refused;
 *   - the 32:1 limit is PER ROI: an ROI with width > 32 * dst_width or height > 32 * dst_height - the rectangle being the whole
 *     W x H output where all four dst_* are 0 - is refused, and the message names its index;
 *   - inside the rectangle each plane of the window is resized to the rectangle's size by exactly the filter-2 arithmetic above:
 *     r(j), the Q15 weights with the residue to the largest tap, the vertical pass first, one rounding per pass, S the window's size
 *     and D the rectangle's (chroma: every number halved).  Samples outside the WINDOW are dropped and the rest renormalised: they
 *     are never read.
 * Outside the rectangle V holds the fill; the layout, RGB and float steps are unchanged and the fill goes through them like any
 * sample.  So: with every rectangle the whole output and every ROI naming one window the bytes are those of p264hip_export_resized
 * with filter 2 for that window; a rectangle of the window's own size pastes the window unchanged (D == S: one tap of 32768, and
 * (64 s * 32768 + 2^20) >> 21 is s); the bytes outside the rectangle are those of p264hip_export_rois.  tests/roi_aa_checker.py is
 * this in numpy.
 *
 * The taps are made on the device (k_roi_aa_taps) into the same scratch with the same cap.  The SEGMENT of an ROI there: four axes
 * in the order x luma, y luma, x chroma, y chroma, each D words first | count << 16 (first a coordinate of the frame) padded to a
 * multiple of 4 with the last one, then D rows of 16-bit Q15 weights with the row stride 2 for S <= D and min(64, ceil(2 S / D))
 * rounded up to even otherwise, padded with 0 to a multiple of 4 words (include/p264hip_aa.h has the text host and device compile).
 * A workgroup of k_roi_aa_* holds 16 rows of a tile's source columns as 16-bit values in LDS, P264HIP_ROI_AA_TILE_VALUES at most;
 * the tile is 64, 32, 16 or 8 output samples wide, chosen per ROI. */
#define P264HIP_ROI_AA_TILE_VALUES 20480
int64_t p264hip_rois_aa_frame_bytes(const p264hip_resize_t *r);
int     p264hip_rois_aa_check(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill,
                              int mb_w, int mb_h, int n_streams, int slots);
int     p264hip_export_rois_aa(p264hip_ctx *ctx, const p264hip_roi_t *rois, int n, const p264hip_resize_t *r,
                               uint32_t fill, void *dst_dev, size_t dst_bytes);
/* host only, no device: the words of the segment of one ROI in the output r describes, and the segment itself as k_roi_aa_taps
 * writes it (the same text).  They read the ROI's window and rectangle and r's width and height, nothing else; P264HIP_EINVAL for a
 * null pointer, an odd or non-positive size, a rectangle above 16384 or a window more than 32 times the rectangle */
int     p264hip_roi_aa_segment_words(const p264hip_roi_t *roi, const p264hip_resize_t *r);
int     p264hip_roi_aa_segment(const p264hip_roi_t *roi, const p264hip_resize_t *r, uint32_t *words);
/* host only: the tile width k_roi_aa_* use for this ROI (64, 32, 16 or 8) and the strips of 16 luma / 8 chroma samples of a tile
 * row in LDS (either pointer may be null); P264HIP_EINVAL as above */
int     p264hip_roi_aa_tile_width(const p264hip_roi_t *roi, const p264hip_resize_t *r, int *luma_strips, int *chroma_strips);

/* ---- the same exports from an ROI LIST IN DEVICE MEMORY: a detector's boxes go to a second model without the host seeing them.
 * One entry for both filters (r->filter is 0 or 2).  The host knows the capacity n of the list and the output, nothing of an ROI;
 * what it decided per ROI above - the check, the descriptor, the segment's place, the tile - the kernel k_roi_plan decides on the
 * device (csrc/hip/kernel_roi_dev.h), by the text of include/p264hip_roi_rule.h, which the host compiles as p264hip_roi_status.
 *
 * An ROI has a STATUS: 0, or the first rule it breaks in the order of the refusals of p264hip_rois_check / p264hip_rois_aa_check.
 * Picture i with status 0 gets exactly the bytes p264hip_export_rois / p264hip_export_rois_aa writes for that ROI at index i; for a
 * picture with any other status NO byte at dst_dev + i*frame_stride is written.  An invalid ROI refuses nothing: the call cannot
 * know of it.  status_dev, where given, receives the n status words. */
enum { P264HIP_ROI_OK = 0,              /* the ROI is valid */
       P264HIP_ROI_UNUSED = 1,          /* index at or beyond the device count */
       P264HIP_ROI_BAD_PICTURE = 2,     /* stream or slot out of range */
       P264HIP_ROI_NO_PICTURE = 3,      /* slot -1 and the slot table has no picture for the stream */
       P264HIP_ROI_WINDOW_EMPTY = 4,    /* negative offset or no samples */
       P264HIP_ROI_WINDOW_ODD = 5,      /* window with an odd member */
       P264HIP_ROI_WINDOW_OUTSIDE = 6,  /* window leaves the frame */
       P264HIP_ROI_RECT_SMALL = 7,      /* rectangle with a negative offset or below 2 x 2 */
       P264HIP_ROI_RECT_ODD = 8,        /* rectangle with an odd member */
       P264HIP_ROI_RECT_OUTSIDE = 9,    /* rectangle leaves the output */
       P264HIP_ROI_REDUCTION = 10 };    /* filter 2 only: width > m*dst_width or height > m*dst_height, m = max_reduction; 0 means 32 */
/* host only, no device: the status of one ROI (one of 0, 2, 4 .. 10: the slot is taken as it stands) in the output r describes
 * (width, height and filter are read), a frame of mb_w x mb_h macroblocks and a store of n_streams x slots.  0 exactly where
 * p264hip_rois_check / p264hip_rois_aa_check - with max_reduction 0 - accepts the ROI in an acceptable description */
int     p264hip_roi_status(const p264hip_roi_t *roi, const p264hip_resize_t *r, int mb_w, int mb_h, int n_streams, int slots, int max_reduction);
/* The plan of a call.  The host cannot add up segments it has not seen, so EVERY ROI of a device-list call gets a segment of
 * seg_words words - with filter 2 the largest segment of any ROI that passes the rule at max_reduction - and a pair of launches
 * takes rois_per_pair = P264HIP_ROI_SCRATCH_BYTES / 4 / seg_words ROIs (at least 1); the antialiased bodies launch with aa_tiles
 * workgroups per ROI and aa_lds_bytes of dynamic LDS, the most any passing ROI needs (both 0 with filter 0).  max_reduction is what
 * keeps a caller whose boxes reduce by 3:1 from paying for 32:1.  Host only; P264HIP_EINVAL for a description
 * p264hip_rois_frame_bytes / _aa_frame_bytes refuses and a max_reduction other than 0 with filter 0, outside 0 .. 32 with filter 2 */
typedef struct p264hip_rois_plan { int32_t seg_words, rois_per_pair, aa_tiles, aa_lds_bytes; } p264hip_rois_plan_t;
int     p264hip_rois_device_plan(const p264hip_resize_t *r, int max_reduction, p264hip_rois_plan_t *out);
enum { P264HIP_ROIS_AFTER = 1, P264HIP_ROIS_BEFORE = 2 };
typedef struct p264hip_rois_dev {
    const p264hip_roi_t *rois_dev;      /* device memory, n entries, address a multiple of 8 */
    const int32_t *count_dev;           /* device, one value, clamped into 0 .. n: the ROIs from it on are P264HIP_ROI_UNUSED; NULL: all n */
    int32_t       *status_dev;          /* device, n entries; NULL: not written */
    const int32_t *slot_of_stream;      /* HOST, n_streams entries (a slot, or -1: no picture), consumed before the call returns: what
                                           slot -1 of an ROI stands for; NULL: slot -1 is invalid */
    void          *after_stream, *before_stream;    /* hipStream_t; read with the flags below, NULL: the legacy default stream */
    int32_t n, max_reduction, flags;    /* P264HIP_ROIS_AFTER: the context's stream waits for what after_stream has queued before it
                                           reads the list; P264HIP_ROIS_BEFORE: before_stream waits for the call's last launch */
} p264hip_rois_dev_t;
/* 0, or P264HIP_EINVAL (host only) for what can be known without the list: whatever p264hip_rois_frame_bytes / _aa_frame_bytes
 * refuses in the description, a frame_stride p264hip_resize_check refuses, a null or misaligned rois_dev, n < 1, a fill with a bit
 * above 23 set, a frame above 65535 samples a side, a max_reduction p264hip_rois_device_plan refuses, unknown flag bits and a
 * slot-table entry outside -1 .. slots - 1 */
int     p264hip_rois_device_check(const p264hip_rois_dev_t *l, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots);
/* Asynchronous on the context's stream behind every reconstruct queued before it: one k_roi_plan launch, then a pair of launches
 * (taps, body) per rois_per_pair ROIs.  P264HIP_EINVAL, before anything is queued, for what p264hip_rois_device_check refuses
 * against the context's geometry, a null dst_dev or one that is no multiple of the element size, and dst_bytes <
 * (n-1)*frame_stride + the picture's bytes.  Per call the host stages the parameters and, where given, the n_streams integers of
 * the slot table: nothing per ROI, and it reads nothing back.  The descriptors and the taps lie in buffers of the context that
 * grow with n and the plan; growing one waits for the context's stream.  A call that finds them large enough does not synchronise
 * the host with the device (it may wait for the copy of the slot table of three calls before, long done in any steady state).
 * Without P264HIP_ROIS_BEFORE the call is complete after p264hip_sync or a marker; rois_dev, count_dev and status_dev belong to
 * the call until then (with the flag: until before_stream has passed the wait).  The kernels write the bytes of the layout of the
 * pictures with status 0, the status words, and no others. */
int     p264hip_export_rois_device(p264hip_ctx *ctx, const p264hip_rois_dev_t *l, const p264hip_resize_t *r, uint32_t fill, void *dst_dev, size_t dst_bytes);

/* plain synchronous copies between host and device memory (the fan-out's TCP transport uses them where it stands in for a
 * device-to-device transport in tests) */
int  p264hip_copy_to_device(void *dev, const void *host, size_t bytes);
int  p264hip_copy_from_device(void *host, const void *dev, size_t bytes);

/* Reconstruct a batch: picture input slot pic_ids[i] is decoded into stream streams[i].
 * All pictures of one call are mutually independent (different streams).  Asynchronous. */
int  p264hip_reconstruct(p264hip_ctx *ctx, const int *pic_ids, const int *streams, int n);

/* upload + reconstruct of one picture for one stream (the p264_decoder_decode path) */
int  p264hip_submit(p264hip_ctx *ctx, int stream, const p264hip_picture_t *pic);

int  p264hip_sync(p264hip_ctx *ctx);

/* Frame-store access (synchronous).  Strides in bytes; planes are mb_w*16 x mb_h*16 (luma). */
int  p264hip_read_frame(p264hip_ctx *ctx, int stream, int slot,
                        uint8_t *y, int y_stride, uint8_t *u, uint8_t *v, int c_stride);
int  p264hip_write_frame(p264hip_ctx *ctx, int stream, int slot,
                         const uint8_t *y, int y_stride, const uint8_t *u, const uint8_t *v, int c_stride);
/* The asynchronous pair for callers that keep their buffers pinned (p264hip_host_alloc): nothing waits until
 * p264hip_sync / a marker.  submit_async = upload_async + reconstruct; read_frame_async enqueues the layout conversion and
 * the three plane copies behind whatever was submitted before.  (The drop-in path uses them: one wait per picture.) */
int  p264hip_submit_async(p264hip_ctx *ctx, int stream, const p264hip_picture_t *pic);
int  p264hip_read_frame_async(p264hip_ctx *ctx, int stream, int slot,
                              uint8_t *y, int y_stride, uint8_t *u, uint8_t *v, int c_stride);

/* Timing hooks used by bench.py: HIP events on the context's own stream.
 * kernel index: 0 inter (MC + residual), 1 intra, 2 deblock, 3 whole reconstruct call. */
#define P264HIP_NKERNELS 4
int  p264hip_timing_enable(p264hip_ctx *ctx, int on);
int  p264hip_timing_read(p264hip_ctx *ctx, double ms_sum[P264HIP_NKERNELS], int64_t count[P264HIP_NKERNELS]);
int  p264hip_timing_reset(p264hip_ctx *ctx);

/* What the last p264hip_reconstruct call launched (the workgroup shapes follow from the batch size and the device's compute
 * units; tests assert that a batch of the bench's size selects the bench's shapes, bench.py records them).  Diagnostics only. */
typedef struct p264hip_launch_info {
    int32_t pictures;              /* pictures of the batch */
    int32_t compute_units;         /* of the context's device */
    int32_t mc_wgs_per_picture;    /* k_mc: workgroups per picture (0: no inter launch) */
    int32_t intra_waves;           /* k_intra / k_intra_sparse: wavefronts per workgroup */
    int32_t edge_info_fused;       /* edge-info workgroups per picture inside the k_intra_sparse launch (0: own launch k_deblock_bs) */
    int32_t deblock_pics_per_wg, deblock_rb_log2, deblock_waves, deblock_wgs;
    int32_t deblock_odd_single;    /* 1: odd pictures per workgroup - pairs in bands of 4 rows, the last picture alone in bands of 8 */
    int32_t t8x8_wgs;              /* k_t8x8: workgroups of the launch (0: no picture of the batch has transform_8x8, no launch - or a picture of the
                                      batch has scaling_lists: k_scaled_inter then adds the 8x8 blocks of every picture of the batch) */
    int32_t scaled_pictures;       /* pictures of the batch that take the scaled road: those with scaling_lists and those with a non-zero cr_qp_offset_delta
                                      (a picture with both counts once).  Not 0: the batch ran the instances that know the table (k_mc_sort_scaled / k_mc_sort_scaled_p,
                                      k_scaled_inter behind the inter launches, k_intra_scaled / k_intra_sparse_scaled) */
    int32_t cr_pictures;           /* pictures of the batch with a non-zero cr_qp_offset_delta.  Not 0: the loop filter ran its Cr instances (k_deblock_bs_cr, k_deblock_cr) */
    int32_t reserved[2];
    int32_t intra_i8;              /* 1: the intra launch ran the Intra 8x8 instances (a picture of the batch has P264_T8X8_INTRA) */
} p264hip_launch_info_t;
int  p264hip_last_launch(p264hip_ctx *ctx, p264hip_launch_info_t *out);

/* Properties of the library build.  Bit 0 (P264HIP_BUILD_TIMING) is reserved and always clear: it marked builds with pieces of
 * the kernels compiled out to time the rest, which no longer exist.  bench.py records the bit and the test suite asserts it is
 * clear. */
#define P264HIP_BUILD_TIMING 1
int  p264hip_build_info(void);

#ifdef __cplusplus
}
#endif
#endif
