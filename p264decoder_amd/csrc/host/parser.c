/* parser.c - host-side H.264 bitstream layer (see include/p264parse.h).
 *
 * CPU work by design: entropy decoding is bit-serial.  Everything it learns about a picture
 * is written straight into the structure-of-arrays buffers of p264hip_picture_t, which the
 * HIP layer uploads as they are.
 *
 * Supported subset = what the reference decodes: CAVLC, I and P slices,
 * frame MBs, one reference list.  Beyond it we follow ITU-T H.264 (several slices per picture,
 * multiple reference frames, list reordering, sub-8x8 partitions, memory management control
 * operations, and - SURVEY 8f rank 4, where the reference stops at decoder/lists.c:136 and
 * decoder/macroblock.c:168-171 - CAVLC B slices: two lists ordered by picture order count,
 * every B macroblock and sub-macroblock type, spatial and temporal direct prediction, implicit
 * bi-prediction weights, explicit weighted prediction); everything else is rejected with -1 and a line on stderr, the
 * reference's error convention (decoder/decoder.c:558-577,780-795).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "p264parse.h"
#include "host_cpu.h"
#include "bits.h"
#include "vlc.h"
#include "cavlc_tables.h"
#include "cabac.h"

#define NAL_SLICE     1
#define NAL_SLICE_DPA 2
#define NAL_SLICE_DPB 3
#define NAL_SLICE_DPC 4
#define NAL_SLICE_IDR 5
#define NAL_SPS       7
#define NAL_PPS       8

/* scaling matrices (7.3.2.1.1.1, 7.4.2.1.1; P264PARSE_OPT_SCALING).  One scaling_list( ) as coded: present, with
 * useDefaultScalingMatrixFlag, or its values in scan order; a parameter set's matrix: the lists it codes (SPS: 8; PPS: 6, and 2
 * more with transform_8x8_mode_flag).  What a list that is absent or says "default" stands for is table 7-2's (cqm_resolve). */
typedef struct { uint8_t present, use_default, v[64]; } cqm_list_t;
typedef struct { uint8_t l4[6][16], l8[2][64]; } cqm_t;      /* eight resolved lists, scan order: the table of p264hip_picture_t */

typedef struct {
    int valid, profile_idc, level_idc;
    int log2_max_frame_num, poc_type, log2_max_poc_lsb;
    int delta_pic_order_always_zero, num_ref_frames_in_poc_cycle;
    int num_ref_frames, gaps_allowed, mb_w, mb_h, frame_mbs_only, direct_8x8_inference;
    int crop[4];
    int high;                                        /* one of the profiles whose SPS and PPS carry the High extensions (sps_is_high) */
    int cqm; cqm_t lists;                            /* seq_scaling_matrix_present_flag, and its lists resolved with fall-back rule A */
    /* bitstream_restriction_flag of the VUI and the two of its fields that bound the output process (parse_vui); a VUI that is
     * damaged counts as absent */
    int restriction, num_reorder_frames, max_dec_frame_buffering;
} sps_t;

typedef struct {
    int valid, sps_id, cabac, pic_order_present, num_slice_groups;
    int num_ref_idx[2], weighted_pred, weighted_bipred;    /* num_ref_idx: the default active length per list */
    int pic_init_qp, chroma_qp_offset, deblock_ctrl, constrained_intra, redundant_pic_cnt;
    /* what follows while more_rbsp_data( ) (7.3.2.2), as read; honoured only by slices whose SPS is a High one (open_slice) */
    int ext, t8x8_mode, scaling_matrix, second_chroma_qp_offset;
    /* P264PARSE_OPT_SCALING: the PPS's lists as coded - which rule resolves them depends on the SPS, known at activation - and
     * whether the extension ended inside them (a complaint that waits for the activation by a slice of a High-profile SPS too) */
    cqm_list_t cqm[8]; int cqm_read, ext_short;
} pps_t;

typedef struct {
    int first_mb, type, pps_id, frame_num, idr_pic_id;
    int qp, disable_deblock, alpha_off, beta_off;
    int num_ref_idx[2], n_reorder[2];                /* per list ([1]: B slices) */
    struct { int idc, arg; } reorder[2][34];
    int poc_lsb, delta_poc_bottom, direct_spatial, cabac_init_idc;
    int no_output_of_prior, long_term_flag, adaptive_marking;
    int n_mmco; struct { int op, a, b; } mmco[34];   /* memory_management_control_operation 1..6 and its operands */
    int wp, wp_denom[2];                             /* pred_weight_table( ) (7.3.3.2): present, luma / chroma log2 denominators */
    int16_t wp_tab[2][P264HIP_MAX_REFS][3][2];       /* [list][ref_idx][Y, Cb, Cr][weight, offset], defaults filled in */
} slice_t;

typedef struct { int used, frame_num, pic_num, is_long, long_idx;   /* long_idx = LongTermFrameIdx (= LongTermPicNum for frames) */
                 int poc; uint32_t uid; } dpb_frame_t;              /* picture order count; uid: which decoded picture the slot holds */

typedef struct {
    p264hip_mb_t *mb; int16_t *mv[2]; int8_t *ref[2]; uint8_t *i4; int16_t *coef;   /* mv, ref: per list ([1]: B pictures; allocated for non-Baseline streams) */
    size_t coef_cap, coef_n;
    /* mb, mv[0], ref[0], i4 and coef are sections of ONE allocation laid out like an input slot of the HIP layer (p264hip_input_layout:
     * records | vectors | reference indices | intra 4x4 modes | coded levels, each on a 256-byte boundary), so that a picture goes
     * host -> HBM as one copy (p264hip_upload / _upload_async notice it); coef_own: the coded levels outgrew their section and
     * moved to an allocation of their own (the picture then travels in pieces, as every picture did until round 5) */
    uint8_t *block; int coef_own;
    void *(*alloc)(size_t); void (*release)(void *);   /* where the arrays live (p264parse_set_allocator) */
} picbuf_t;

/* The picture being built: everything that is a property of the PICTURE, from its first slice to the hand-over. */
typedef struct {
    int open, is_idr, ref_idc;
    int next_mb, slice_no;
    int poc; uint32_t uid;                    /* picture order count (8.2.1); which decoded picture this is */
    slice_t first;                            /* header of the first slice: written when the picture opens, read-only from then on (marking and
                                               * the order count read frame_num, poc_lsb, delta_poc_bottom, long_term_flag, the marking commands) */
    /* what the device gets */
    int type;                                 /* P264_SLICE_*: B with any B slice, P with any P slice, else I */
    int deblock, alpha, beta;                 /* loop filter: on if any slice enables it, offsets of the first such slice */
    /* the CANONICAL lists: the first P / B slice's verbatim; a later slice's entries are mapped onto them (ref_map: slice index ->
     * canonical index), new ones appended, and the indices the slice wrote are rewritten when it ends (end_slice) */
    int list[2][P264HIP_MAX_REFS], n_list[2];
    /* explicit weights: taken from the first P / B slice (wp_set).  wp_tab is the canonical table, which grows with the canonical
     * lists; wp_coded stays the first slice's table as coded: what every other slice's must equal */
    int wp_set, wp, wp_denom[2];
    int16_t wp_tab[2][P264HIP_MAX_REFS][3][2], wp_coded[2][P264HIP_MAX_REFS][3][2];
    int weighted_bipred;
    int16_t bipred_weight[P264HIP_MAX_REFS * P264HIP_MAX_REFS];   /* implicit weights (8.4.2.3.1) */
    int t8x8;                                 /* a slice of the picture had transform_8x8_mode_flag: its inter records may carry P264_MB_T8X8 */
    int i8x8;                                 /* the picture holds at least one Intra 8x8 record (P264_MB_I8X8) */
    int cqm; cqm_t lists;                     /* the picture's resolved scaling lists (its first slice's; cqm 0: every weight is 16) */
} curpic_t;

/* output order (H.264 C.4; p264parse_set_output_order): per frame-store slot, whether the picture in it waits for its output,
 * with what the output entry will say of it */
typedef struct { int waiting, poc, index, flags; } wait_t;

struct p264parse {
    int opts;
    sps_t sps[32];
    pps_t pps[256];
    int active_sps, active_pps, generation;
    int mb_w, mb_h, n_mb, slots;

    picbuf_t buf[2]; int cur;                 /* cur: being built; 1-cur: last completed */
    picbuf_t retired[2];                      /* the buffers of the previous context: released at the NEXT re-init (see free_context) */
    void *(*alloc)(size_t); void (*release)(void *);
    p264hip_picture_t desc[2];
    uint8_t  *nnz;                            /* [n_mb][24] total_coeff per 4x4 block */
    uint16_t *slice_of;                       /* [n_mb] slice number inside the picture, 0xffff = not decoded */

    curpic_t pic;
    /* slice scope */
    slice_t sh;                               /* current slice */
    uint16_t slice_flags;                     /* the records' `flags` of the current slice: its offsets minus the picture's (include/p264hip.h) */
    int t8x8_mode;                            /* transform_8x8_mode_flag of the slice's PPS, under a High SPS (0 otherwise) */
    /* the slice's OWN lists: what its macroblocks are parsed against (vector prediction, CABAC contexts, skip / direct inference and
     * temporal direct's list-0 mapping are slice-local) and what end_slice resolves its indices through */
    int list[2][P264HIP_MAX_REFS], n_list[2];
    int8_t ref_map[2][P264HIP_MAX_REFS]; int ref_map_used[2];
    /* picture order count (8.2.1): what the next picture measures its own against */
    int prev_poc_msb, prev_poc_lsb, prev_frame_num, frame_num_offset;
    uint32_t next_uid;
    /* motion of every reference picture, kept for the direct prediction of later B pictures (the co-located picture is
     * RefPicList1[0]): per frame-store slot, per 4x4 block the vector, per 8x8 the reference index it used and the uid of the
     * picture that index meant (-1 = intra) */
    int has_col;
    int16_t *col_mv[P264HIP_MAX_REFS + 1]; int8_t *col_ref[P264HIP_MAX_REFS + 1]; int32_t *col_uid[P264HIP_MAX_REFS + 1];

    dpb_frame_t dpb[P264HIP_MAX_REFS + 1];
    int cur_slot;
    /* output order: off unless asked for.  out_depth: the caller's reorder depth (< 0: the stream's); reorder: the depth in
     * force (R); wait: the set W; outs: the pictures that became due with the last completed picture, or the last flush */
    int out_on, out_depth, reorder;
    wait_t wait[P264HIP_MAX_REFS + 1];
    p264parse_output_t outs[P264PARSE_MAX_OUTPUTS]; int n_outs;
    int decode_index;                         /* completed pictures so far */
    int last_qp;                              /* never reset, like h->mb.i_last_qp (core/macroblock.c:1248-1252) */
    int qp_pred;                              /* conformant chain only (strict_qp) */
    int strict_qp;                            /* this slice: QP_Y = (QP_Y,PRED + mb_qp_delta + 52) % 52 (H.264 7.4.5) */

    /* current MB */
    int mbx, mby, mbi;
    unsigned mv_done[2];                      /* per list, bit (y*4+x): that 4x4 of the current MB has its motion */
    int      cur_avail;                       /* P264_AVAIL_* of the current MB (set by begin_mb) */
    int skip_run;
    /* CABAC (parser_cabac.h): the engine, and what context selection needs from earlier macroblocks */
    int cabac_on, last_dqp;
    p264cabac_t cb;
    uint16_t *cinfo;                          /* [n_mb] CI_* */
    uint8_t *mvd_abs[2];                      /* [n_mb][16][2] |mvd| per list, 4x4 block and component, saturated at 255 */
};

#define ERR(p, ...) do { fprintf(stderr, "p264amd: " __VA_ARGS__); fputc('\n', stderr); } while (0)
#define INFO(p, ...) do { if (!((p)->opts & P264PARSE_OPT_QUIET)) { fprintf(stderr, __VA_ARGS__); } } while (0)

static inline int clip3i(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
static inline int median3(int a, int b, int c)
{
    int lo = a < b ? a : b, hi = a < b ? b : a;
    return c < lo ? lo : c > hi ? hi : c;
}

/* ---------------------------------------------------------------- parameter sets -------- */
static long rbsp_stop_bit(const uint8_t *buf, int size);
/* the profiles whose SPS carries chroma_format_idc .. seq_scaling_matrix_present_flag behind its id (7.3.2.1.1) and whose PPS may
 * carry transform_8x8_mode_flag */
static int sps_is_high(int profile)
{
    return profile == 100 || profile == 110 || profile == 122 || profile == 244 || profile == 44 || profile == 83 || profile == 86 ||
           profile == 118 || profile == 128;
}
/* tables 7-3 and 7-4, scan order */
static const uint8_t cqm_default4[2][16] = {
    { 6, 13, 13, 20, 20, 20, 28, 28, 28, 28, 32, 32, 32, 37, 37, 42 }, { 10, 14, 14, 20, 20, 20, 24, 24, 24, 24, 27, 27, 27, 30, 30, 34 } };
static const uint8_t cqm_default8[2][64] = {
    { 6, 10, 10, 13, 11, 13, 16, 16, 16, 16, 18, 18, 18, 18, 18, 23, 23, 23, 23, 23, 23, 25, 25, 25, 25, 25, 25, 25, 27, 27, 27, 27, 27, 27, 27, 27,
      29, 29, 29, 29, 29, 29, 29, 31, 31, 31, 31, 31, 31, 33, 33, 33, 33, 33, 36, 36, 36, 36, 38, 38, 38, 40, 40, 42 },
    { 9, 13, 13, 15, 13, 15, 17, 17, 17, 17, 19, 19, 19, 19, 19, 21, 21, 21, 21, 21, 21, 22, 22, 22, 22, 22, 22, 22, 24, 24, 24, 24, 24, 24, 24, 24,
      25, 25, 25, 25, 25, 25, 25, 27, 27, 27, 27, 27, 27, 28, 28, 28, 28, 28, 30, 30, 30, 30, 32, 32, 32, 33, 33, 35 } };
/* scaling_list( ) (7.3.2.1.1.1) behind its present flag: nextScale = (lastScale + delta_scale + 256) % 256; a first nextScale of 0
 * is useDefaultScalingMatrixFlag, a later one ends the list - the remaining positions repeat lastScale */
static void cqm_read_list(bitrd_t *b, int size, cqm_list_t *o)
{
    memset(o, 0, sizeof *o);
    o->present = (uint8_t)br_u1(b);
    if (!o->present) return;
    int last = 8, next = 8;
    for (int j = 0; j < size; j++) {
        if (next != 0) {
            next = (int)((unsigned)(last + br_se(b)) & 255u);
            if (j == 0 && next == 0) o->use_default = 1;
        }
        o->v[j] = (uint8_t)(next == 0 ? last : next);
        last = o->v[j];
    }
}
/* table 7-2: the eight lists of a set that codes the first `coded` of them.  fb = NULL: fall-back rule A (an absent list 0 / 3 / 6 / 7
 * takes its default); fb = the SPS's resolved lists: rule B (... takes the SPS's list of that number).  Either way an absent list
 * 1, 2, 4, 5 takes the list before it, and useDefaultScalingMatrixFlag the default. */
static void cqm_resolve(const cqm_list_t *l, int coded, const cqm_t *fb, cqm_t *o)
{
    for (int n = 0; n < 6; n++) {
        if (n < coded && l[n].present) memcpy(o->l4[n], l[n].use_default ? cqm_default4[n / 3] : l[n].v, 16);
        else if (n % 3) memcpy(o->l4[n], o->l4[n - 1], 16);
        else memcpy(o->l4[n], fb ? fb->l4[n] : cqm_default4[n / 3], 16);
    }
    for (int n = 0; n < 2; n++) {
        if (6 + n < coded && l[6 + n].present) memcpy(o->l8[n], l[6 + n].use_default ? cqm_default8[n] : l[6 + n].v, 64);
        else memcpy(o->l8[n], fb ? fb->l8[n] : cqm_default8[n], 64);
    }
}
static int cqm_is_flat(const cqm_t *c)
{
    const uint8_t *v = &c->l4[0][0];
    for (size_t i = 0; i < sizeof *c; i++) if (v[i] != 16) return 0;
    return 1;
}

/* hrd_parameters( ) (E.1.2), skipped; 0 where cpb_cnt_minus1 is out of range */
static int skip_hrd(bitrd_t *b)
{
    const unsigned cpb_cnt = br_ue(b);
    if (cpb_cnt > 31) return 0;
    br_skip(b, 8);                                  /* bit_rate_scale, cpb_size_scale */
    for (unsigned i = 0; i <= cpb_cnt; i++) { br_ue(b); br_ue(b); br_u1(b); }
    br_skip(b, 20);                                 /* four lengths of five bits */
    return 1;
}
/* vui_parameters( ) (E.1.1), read for one thing: num_reorder_frames and max_dec_frame_buffering of the bitstream restriction,
 * which bound the output process (p264parse_set_output_order).  Everything in front of them is skipped.  Nothing here refuses a
 * parameter set: a VUI that runs past the rbsp_stop_one_bit or holds a value out of range leaves the SPS as it is without one. */
static void parse_vui(bitrd_t *b, sps_t *s)
{
    if (br_u1(b) && br_u(b, 8) == 255) br_skip(b, 32);          /* aspect ratio; Extended_SAR: sar_width, sar_height */
    if (br_u1(b)) br_u1(b);                                     /* overscan */
    if (br_u1(b)) { br_skip(b, 4); if (br_u1(b)) br_skip(b, 24); }   /* video signal type; colour description */
    if (br_u1(b)) { br_ue(b); br_ue(b); }                       /* chroma sample location */
    if (br_u1(b)) { br_skip(b, 32); br_skip(b, 32); br_u1(b); } /* timing: num_units_in_tick, time_scale, fixed_frame_rate_flag */
    const int nal_hrd = (int)br_u1(b);
    if (nal_hrd && !skip_hrd(b)) return;
    const int vcl_hrd = (int)br_u1(b);
    if (vcl_hrd && !skip_hrd(b)) return;
    if (nal_hrd || vcl_hrd) br_u1(b);                           /* low_delay_hrd_flag */
    br_u1(b);                                                   /* pic_struct_present_flag */
    if (!br_u1(b)) return;                                      /* bitstream_restriction_flag */
    br_u1(b);                                                   /* motion_vectors_over_pic_boundaries_flag */
    for (int i = 0; i < 4; i++) br_ue(b);                       /* max_bytes_per_pic_denom, max_bits_per_mb_denom, log2_max_mv_length_horizontal / _vertical */
    const unsigned reorder = br_ue(b), buffering = br_ue(b);
    if ((long)br_consumed(b) > rbsp_stop_bit(b->buf, (int)b->size) || buffering > 16 || reorder > buffering) return;
    s->restriction = 1; s->num_reorder_frames = (int)reorder; s->max_dec_frame_buffering = (int)buffering;
}

/* The frames the decoded picture buffer holds (D) and the reorder depth (R) of an SPS, for the output process: the bitstream
 * restriction's where there is one; else MaxDpbFrames of the level (A.3.1 h, table A-1) and - nothing bounds the reordering - the
 * same again, except under pic_order_cnt_type 2, whose output order is decode order (8.2.1.3). */
static int sps_dpb_frames(const sps_t *s)
{
    static const struct { int level, mbs; } max_dpb_mbs[] = {
        { 9, 396 }, { 10, 396 }, { 11, 900 }, { 12, 2376 }, { 13, 2376 }, { 20, 2376 }, { 21, 4752 }, { 22, 8100 }, { 30, 8100 }, { 31, 18000 },
        { 32, 20480 }, { 40, 32768 }, { 41, 32768 }, { 42, 34816 }, { 50, 110400 }, { 51, 184320 }, { 52, 184320 } };
    int d = 16;
    if (s->restriction) d = s->max_dec_frame_buffering;
    else for (size_t i = 0; i < sizeof max_dpb_mbs / sizeof max_dpb_mbs[0]; i++)
        if (max_dpb_mbs[i].level == s->level_idc) { d = max_dpb_mbs[i].mbs / (s->mb_w * s->mb_h); break; }
    if (d < s->num_ref_frames) d = s->num_ref_frames;
    return d < 1 ? 1 : d > 16 ? 16 : d;                         /* (one frame at least: the frame store has two slots at least) */
}
static int sps_reorder_depth(const sps_t *s)
{
    return s->restriction ? s->num_reorder_frames : s->poc_type == 2 ? 0 : sps_dpb_frames(s);
}
/* slots of the frame store under an SPS: one per reference frame and the picture being decoded; with output order on, one per frame
 * of the decoded picture buffer and that one */
static int sps_slots(const p264parse *p, const sps_t *s)
{
    const int slots = (p->out_on ? sps_dpb_frames(s) : s->num_ref_frames) + 1;
    return slots < 2 ? 2 : slots;
}

/* decoder/set.c:37-167 */
static int parse_sps(p264parse *p, bitrd_t *b)
{
    int profile = (int)br_u(b, 8);
    br_skip(b, 8);                                  /* constraint flags + reserved */
    int level = (int)br_u(b, 8);
    unsigned id = br_ue(b);
    if (br_eof(b) || id >= 32) return -1;
    sps_t *s = &p->sps[id];
    sps_t old = *s;
    memset(s, 0, sizeof *s);
    s->profile_idc = profile; s->level_idc = level;
    s->high = sps_is_high(profile);
    if (s->high) {
        /* what the kernels decode of the High tools: 4:2:0, 8 bits, no transform bypass; scaling lists where the backend is said to
         * read the picture's table (P264PARSE_OPT_SCALING), else flat ones only */
        const unsigned cf = br_ue(b);
        const int separate = cf == 3 ? (int)br_u1(b) : 0;
        const unsigned bd_y = br_ue(b), bd_c = br_ue(b);
        const int bypass = (int)br_u1(b), matrices = (int)br_u1(b);
        if (br_eof(b) || cf != 1 || separate || bd_y || bd_c || bypass || (matrices && !(p->opts & P264PARSE_OPT_SCALING))) {
            ERR(p, "SPS %u (profile %d): chroma_format_idc %u, bit depths %u / %u, transform bypass %d, scaling matrices %d unsupported (4:2:0, 8 bits, flat lists)",
                id, profile, cf, bd_y + 8, bd_c + 8, bypass, matrices);
            *s = old;                                   /* keep the set we had */
            return -1;
        }
        if (matrices) {                                 /* eight lists for 4:2:0, resolved with rule A */
            cqm_list_t l[8];
            for (int n = 0; n < 8; n++) cqm_read_list(b, n < 6 ? 16 : 64, &l[n]);
            if (br_eof(b)) { ERR(p, "SPS %u: incomplete scaling matrix", id); *s = old; return -1; }
            s->cqm = 1;
            cqm_resolve(l, 8, NULL, &s->lists);
        }
    }
    s->log2_max_frame_num = (int)br_ue(b) + 4;
    s->poc_type = (int)br_ue(b);
    if (s->poc_type == 0) s->log2_max_poc_lsb = (int)br_ue(b) + 4;
    else if (s->poc_type == 1) {
        s->delta_pic_order_always_zero = (int)br_u1(b);
        br_se(b); br_se(b);
        s->num_ref_frames_in_poc_cycle = (int)br_ue(b);
        if (s->num_ref_frames_in_poc_cycle > 256) s->num_ref_frames_in_poc_cycle = 256;
        for (int i = 0; i < s->num_ref_frames_in_poc_cycle; i++) br_se(b);
    } else if (s->poc_type > 2) return -1;
    s->num_ref_frames = (int)br_ue(b);
    s->gaps_allowed = (int)br_u1(b);
    s->mb_w = (int)br_ue(b) + 1;
    s->mb_h = (int)br_ue(b) + 1;
    s->frame_mbs_only = (int)br_u1(b);
    if (!s->frame_mbs_only) br_u1(b);
    s->direct_8x8_inference = (int)br_u1(b);
    if (br_u1(b)) for (int i = 0; i < 4; i++) s->crop[i] = (int)br_ue(b);   /* left, right, top, bottom: never applied to what the parser delivers (A-Q1), reported by p264parse_crop */
    const int vui = (int)br_u1(b);                  /* vui_parameters_present (not parsed by set.c:136-144) */
    if (br_eof(b)) { ERR(p, "incomplete SPS"); return -1; }
    if (vui) parse_vui(b, s);                       /* (behind the check: whatever the VUI holds, the set is accepted as it was without it) */
    /* untrusted input: H.264 7.4.2.1 ranges (the slice header reads fields of these widths; sizes drive every allocation) */
    if (s->log2_max_frame_num < 4 || s->log2_max_frame_num > 16 || (s->poc_type == 0 && (s->log2_max_poc_lsb < 4 || s->log2_max_poc_lsb > 16)) ||
        s->mb_w < 1 || s->mb_w > 1024 || s->mb_h < 1 || s->mb_h > 512 || s->num_ref_frames < 0 || s->num_ref_frames > 16) {
        ERR(p, "SPS field out of range (frame_num bits %d, poc bits %d, %dx%d macroblocks, %d reference frames)",
            s->log2_max_frame_num, s->log2_max_poc_lsb, s->mb_w, s->mb_h, s->num_ref_frames);
        *s = old;                                   /* keep the set we had */
        return -1;
    }
    s->valid = 1;
    if ((int)id == p->active_sps && (old.mb_w != s->mb_w || old.mb_h != s->mb_h || old.num_ref_frames != s->num_ref_frames || (p->out_on && sps_slots(p, &old) != sps_slots(p, s))))
        p->active_sps = -1;                         /* same id, new geometry: force a context re-init */
    INFO(p, "p264amd: sps:%u profile:%d/%d poc:%d ref:%d %dx%d crop:%d-%d-%d-%d\n", id, profile, level,
         s->poc_type, s->num_ref_frames, s->mb_w, s->mb_h, s->crop[0], s->crop[1], s->crop[2], s->crop[3]);
    return (int)id;
}

/* decoder/set.c:171-272; scaling lists are forced flat there (:261-263), so none are parsed */
static int parse_pps(p264parse *p, bitrd_t *b)
{
    unsigned id = br_ue(b);
    if (br_eof(b) || id >= 256) { ERR(p, "pps id invalid"); return -1; }
    pps_t *q = &p->pps[id];
    memset(q, 0, sizeof *q);
    q->sps_id = (int)br_ue(b);
    if (q->sps_id < 0 || q->sps_id >= 32) return -1;
    q->cabac = (int)br_u1(b);
    q->pic_order_present = (int)br_u1(b);
    q->num_slice_groups = (int)br_ue(b) + 1;
    if (q->num_slice_groups > 1) { ERR(p, "FMO unsupported"); return -1; }
    q->num_ref_idx[0] = (int)br_ue(b) + 1;
    q->num_ref_idx[1] = (int)br_ue(b) + 1;
    if (q->num_ref_idx[0] < 1 || q->num_ref_idx[0] > 32 || q->num_ref_idx[1] < 1 || q->num_ref_idx[1] > 32) { ERR(p, "pps: num_ref_idx out of range"); return -1; }
    q->weighted_pred = (int)br_u1(b);
    q->weighted_bipred = (int)br_u(b, 2);
    q->pic_init_qp = br_se(b) + 26;
    br_se(b);                                       /* pic_init_qs */
    q->chroma_qp_offset = br_se(b);
    q->deblock_ctrl = (int)br_u1(b);
    q->constrained_intra = (int)br_u1(b);
    q->redundant_pic_cnt = (int)br_u1(b);
    if (br_eof(b)) { ERR(p, "incomplete PPS"); return -1; }
    /* while more_rbsp_data( ): the High extension.  Only remembered here - which SPS the PPS goes with is known when a slice
     * activates the pair, and under any other profile nothing of it is looked at (a PPS of such a stream never fails on it) */
    if ((long)br_consumed(b) < rbsp_stop_bit(b->buf, (int)b->size)) {
        q->t8x8_mode = (int)br_u1(b);
        q->scaling_matrix = (int)br_u1(b);
        if (q->scaling_matrix && (p->opts & P264PARSE_OPT_SCALING)) {
            /* the lists as coded, then the real second offset.  Nothing here fails: a short extension is remembered */
            const int coded = 6 + 2 * q->t8x8_mode;
            for (int n = 0; n < coded; n++) cqm_read_list(b, n < 6 ? 16 : 64, &q->cqm[n]);
            q->cqm_read = 1;
            q->second_chroma_qp_offset = br_se(b);
            q->ext_short = br_eof(b);
            q->ext = 1;
        } else {
        q->second_chroma_qp_offset = q->scaling_matrix ? q->chroma_qp_offset : br_se(b);      /* (behind matrices nothing can be read without parsing them) */
        q->ext = !br_eof(b);
        }
    }
    q->valid = 1;
    INFO(p, "p264amd: pps:%u sps:%d %s ref0:%d QP:%d QC=%d DFC:%d CIP:%d\n", id, q->sps_id,
         q->cabac ? "CABAC" : "CAVLC", q->num_ref_idx[0], q->pic_init_qp, q->chroma_qp_offset,
         q->deblock_ctrl, q->constrained_intra);
    return (int)id;
}

/* ---------------------------------------------------------------- context --------------- */
static void release_bufs(picbuf_t *q)
{
    if (q->release) { q->release(q->block); if (q->coef_own) q->release(q->coef); if (q->mv[1]) q->release(q->mv[1]); if (q->ref[1]) q->release(q->ref[1]); }
    memset(q, 0, sizeof *q);
}
/* A caller may still be reading the last completed picture's arrays when the next slice re-initialises the context (the
 * pipeline issues its asynchronous uploads while the parser threads are already on the next picture), so a re-init only
 * RETIRES the current buffers; they are released by the re-init after that, or by close. */
static void free_context(p264parse *p, int final)
{
    for (int i = 0; i < 2; i++) {
        release_bufs(&p->retired[i]);
        if (final) release_bufs(&p->buf[i]);
        else { p->retired[i] = p->buf[i]; memset(&p->buf[i], 0, sizeof p->buf[i]); }
    }
    free(p->nnz); p->nnz = NULL;
    free(p->slice_of); p->slice_of = NULL;
    free(p->cinfo); p->cinfo = NULL; free(p->mvd_abs[0]); free(p->mvd_abs[1]); p->mvd_abs[0] = p->mvd_abs[1] = NULL;
    for (int i = 0; i <= P264HIP_MAX_REFS; i++) { free(p->col_mv[i]); free(p->col_ref[i]); free(p->col_uid[i]); p->col_mv[i] = NULL; p->col_ref[i] = NULL; p->col_uid[i] = NULL; }
    p->has_col = 0;
}

/* decoder/decoder.c:304-343: (re)size everything when the active SPS/PPS pair changes */
static int init_context(p264parse *p, int sps_id, int pps_id)
{
    const sps_t *s = &p->sps[sps_id];
    free_context(p, 0);
    p->mb_w = s->mb_w; p->mb_h = s->mb_h; p->n_mb = s->mb_w * s->mb_h;
    p->slots = sps_slots(p, s);
    size_t n = (size_t)p->n_mb;
    for (int i = 0; i < 2; i++) {
        picbuf_t *q = &p->buf[i];
        q->alloc = p->alloc ? p->alloc : malloc; q->release = p->release ? p->release : free;
        q->coef_cap = n * 8 + 64;                   /* (at most 26 per macroblock; beyond the section: coef_reserve) */
        p264hip_picture_t shape; p264hip_input_layout_t lay;
        memset(&shape, 0, sizeof shape);
        shape.mb_w = s->mb_w; shape.mb_h = s->mb_h; shape.slice_type = P264_SLICE_P; shape.n_coef_blocks = (uint32_t)q->coef_cap;
        if (p264hip_input_layout(&shape, &lay)) return -1;
        q->block = (uint8_t *)q->alloc(lay.bytes);
        if (!q->block) return -1;
        q->mb  = (p264hip_mb_t *)(q->block + lay.off_mb);
        q->mv[0]  = (int16_t *)(q->block + lay.off_mv);
        q->ref[0] = (int8_t *)(q->block + lay.off_ref);
        q->i4  = (uint8_t *)(q->block + lay.off_i4);
        q->coef = (int16_t *)(q->block + lay.off_coef); q->coef_own = 0;
        memset(q->mb, 0, n * sizeof(p264hip_mb_t)); memset(q->mv[0], 0, n * 32 * sizeof(int16_t));
        memset(q->ref[0], 0, n * 4); memset(q->i4, 0, n * 16);
        if (s->profile_idc != 66) {                 /* anything but Baseline may carry B slices: list-1 arrays */
            q->mv[1] = (int16_t *)q->alloc(n * 32 * sizeof(int16_t)); q->ref[1] = (int8_t *)q->alloc(n * 4);
            if (!q->mv[1] || !q->ref[1]) return -1;
            memset(q->mv[1], 0, n * 32 * sizeof(int16_t)); memset(q->ref[1], -1, n * 4);
        }
    }
    if (s->profile_idc != 66) {
        for (int i = 0; i < p->slots; i++) {
            p->col_mv[i] = (int16_t *)calloc(n * 32, sizeof(int16_t)); p->col_ref[i] = (int8_t *)malloc(n * 4); p->col_uid[i] = (int32_t *)malloc(n * 4 * sizeof(int32_t));
            if (!p->col_mv[i] || !p->col_ref[i] || !p->col_uid[i]) return -1;
            memset(p->col_ref[i], -1, n * 4); memset(p->col_uid[i], 0xff, n * 4 * sizeof(int32_t));
        }
        p->has_col = 1;
        p->cinfo = (uint16_t *)calloc(n, sizeof(uint16_t)); p->mvd_abs[0] = (uint8_t *)calloc(n, 32); p->mvd_abs[1] = (uint8_t *)calloc(n, 32);
        if (!p->cinfo || !p->mvd_abs[0] || !p->mvd_abs[1]) return -1;
    }
    p->nnz = (uint8_t *)calloc(n, 24);
    p->slice_of = (uint16_t *)malloc(n * sizeof(uint16_t));
    if (!p->nnz || !p->slice_of) return -1;
    memset(p->dpb, 0, sizeof p->dpb);
    memset(p->wait, 0, sizeof p->wait);             /* (a new frame store: what waited in the old one is gone with it, include/p264parse.h) */
    p->cur_slot = 0;
    p->active_sps = sps_id; p->active_pps = pps_id;
    p->generation++;
    p->pic.open = 0;
    INFO(p, "p264amd: %dx%d\n", 16 * p->mb_w, 16 * p->mb_h);
    return 0;
}

/* ---------------------------------------------------------------- slice header ---------- */
/* pred_weight_table( ) (H.264 7.3.3.2, 4:2:0) with the semantics of 7.4.3.2: a reference without coded weights gets weight
 * 2^denom and offset 0; denominators 0 .. 7, coded weights and offsets -128 .. 127.  The limit on the pairs of a B picture is
 * checked on the pairs its blocks use (bipred_sums_bad). */
static int parse_pred_weight_table(p264parse *p, bitrd_t *b, slice_t *sh)
{
    (void)p;
    const unsigned dl = br_ue(b), dc = br_ue(b);
    if (dl > 7 || dc > 7) { ERR(p, "log2 weight denominators %u / %u out of range (0 .. 7)", dl, dc); return -1; }
    sh->wp_denom[0] = (int)dl; sh->wp_denom[1] = (int)dc;
    const int isB = sh->type == P264_SLICE_B;
    for (int l = 0; l < (isB ? 2 : 1); l++) {
        for (int i = 0; i < sh->num_ref_idx[l]; i++) {
            int16_t (*e)[2] = sh->wp_tab[l][i];
            for (int c = 0; c < 3; c++) { e[c][0] = (int16_t)(1 << sh->wp_denom[c > 0]); e[c][1] = 0; }
            for (int k = 0; k < 2; k++) {                 /* luma_weight_lX_flag, then chroma_weight_lX_flag */
                if (!br_u1(b)) continue;
                for (int c = k ? 1 : 0; c < (k ? 3 : 1); c++) {
                    const int w = br_se(b), o = br_se(b);
                    if (w < -128 || w > 127 || o < -128 || o > 127 || br_overrun(b)) {
                        ERR(p, "list %d index %d: weight %d / offset %d out of range (-128 .. 127)", l, i, w, o); return -1;
                    }
                    e[c][0] = (int16_t)w; e[c][1] = (int16_t)o;
                }
            }
        }
    }
    return br_overrun(b) ? -1 : 0;
}

/* decoder/decoder.c:70-301,368-488.  Fields the reconstruction does not need are skipped. */
static int parse_slice_header(p264parse *p, bitrd_t *b, int nal_type, int nal_ref_idc, slice_t *sh)
{
    memset(sh, 0, sizeof *sh);
    sh->first_mb = (int)br_ue(b);
    sh->type = (int)br_ue(b);
    if (sh->type >= 5) sh->type -= 5;
    sh->pps_id = (int)br_ue(b);
    if (br_eof(b) || sh->pps_id < 0 || sh->pps_id >= 256 || !p->pps[sh->pps_id].valid) {
        ERR(p, "invalid pps_id %d in slice header", sh->pps_id); return -1;
    }
    const pps_t *pps = &p->pps[sh->pps_id];
    if (!p->sps[pps->sps_id].valid) { ERR(p, "slice refers to missing sps %d", pps->sps_id); return -1; }
    const sps_t *sps = &p->sps[pps->sps_id];
    if (sh->type != P264_SLICE_P && sh->type != P264_SLICE_I && sh->type != P264_SLICE_B) { ERR(p, "only I, P and B slices supported (type %d)", sh->type); return -1; }
    if (sh->type == P264_SLICE_B && (sps->profile_idc == 66 || nal_type == NAL_SLICE_IDR)) { ERR(p, "B slice in a Baseline stream or an IDR picture"); return -1; }
    if (sh->type == P264_SLICE_B && sps->poc_type == 1) { ERR(p, "B slices with pic_order_cnt_type 1 unsupported"); return -1; }
    if (pps->cabac && sps->profile_idc == 66) { ERR(p, "CABAC in a Baseline stream"); return -1; }
    if (!sps->frame_mbs_only) { ERR(p, "field/MBAFF coding unsupported"); return -1; }

    sh->frame_num = (int)br_u(b, sps->log2_max_frame_num);
    if (nal_type == NAL_SLICE_IDR) sh->idr_pic_id = (int)br_ue(b);
    if (sps->poc_type == 0) {
        sh->poc_lsb = (int)br_u(b, sps->log2_max_poc_lsb);
        if (pps->pic_order_present) sh->delta_poc_bottom = br_se(b);
    } else if (sps->poc_type == 1 && !sps->delta_pic_order_always_zero) {
        br_se(b);
        if (pps->pic_order_present) br_se(b);
    }
    if (pps->redundant_pic_cnt && br_ue(b) != 0) return 1;       /* redundant picture: ignore the slice */
    if (sh->type == P264_SLICE_B) sh->direct_spatial = (int)br_u1(b);
    if (sh->type == P264_SLICE_P || sh->type == P264_SLICE_B) {
        const int n_lists = sh->type == P264_SLICE_B ? 2 : 1;
        sh->num_ref_idx[0] = pps->num_ref_idx[0]; sh->num_ref_idx[1] = pps->num_ref_idx[1];
        if (br_u1(b)) for (int l = 0; l < n_lists; l++) sh->num_ref_idx[l] = (int)br_ue(b) + 1;
        for (int l = 0; l < n_lists; l++)
            if (sh->num_ref_idx[l] < 1 || sh->num_ref_idx[l] > P264HIP_MAX_REFS) { ERR(p, "num_ref_idx_l%d_active %d too large", l, sh->num_ref_idx[l]); return -1; }
        for (int l = 0; l < n_lists; l++) {
            if (!br_u1(b)) continue;                              /* ref_pic_list_reordering_flag_l0 / _l1 */
            for (;;) {
                unsigned idc = br_ue(b);
                int *n = &sh->n_reorder[l];
                if (idc == 3) break;
                if (idc > 3 || *n >= 33 || br_overrun(b)) { ERR(p, "wrong reordering of pic nums idc"); return -1; }
                sh->reorder[l][*n].idc = (int)idc; sh->reorder[l][*n].arg = (int)br_ue(b);
                (*n)++;
            }
        }
        /* explicit weighted prediction (the reference's pred_weight_table parser is a stub, decoder/decoder.c:259-262) */
        sh->wp = (pps->weighted_pred && sh->type == P264_SLICE_P) || (pps->weighted_bipred == 1 && sh->type == P264_SLICE_B);
        if (sh->wp && parse_pred_weight_table(p, b, sh) < 0) return -1;
    }
    if (nal_ref_idc != 0) {
        if (nal_type == NAL_SLICE_IDR) { sh->no_output_of_prior = (int)br_u1(b); sh->long_term_flag = (int)br_u1(b); }
        else if (br_u1(b)) {
            /* dec_ref_pic_marking with adaptive_ref_pic_marking_mode_flag (H.264 7.3.3.3; the reference parses the
             * commands and then ignores them, decoder/decoder.c:264-297, decoder/lists.c:183-187) */
            sh->adaptive_marking = 1;
            for (;;) {
                const unsigned op = br_ue(b);
                if (op == 0) break;
                if (op > 6 || sh->n_mmco >= 33 || br_overrun(b)) { ERR(p, "bad memory_management_control_operation %u", op); return -1; }
                /* operands are bounded by the syntax (7.4.3.3): picture-number differences below MaxFrameNum, long-term
                 * indices at most num_ref_frames - anything else is a broken stream, not something to compute with */
                unsigned a = 0, c = 0;
                const unsigned max_fn_u = 1u << sps->log2_max_frame_num, max_lt = (unsigned)(sps->num_ref_frames > 0 ? sps->num_ref_frames : 1);
                if (op == 1 || op == 3) { a = br_ue(b); if (a >= max_fn_u) { ERR(p, "difference_of_pic_nums_minus1 %u out of range", a); return -1; } }
                if (op == 2) { a = br_ue(b); if (a >= 2 * max_lt) { ERR(p, "long_term_pic_num %u out of range", a); return -1; } }
                if (op == 3 || op == 6) { c = br_ue(b); if (c >= max_lt) { ERR(p, "long_term_frame_idx %u out of range (num_ref_frames %u)", c, max_lt); return -1; } }
                if (op == 4) { a = br_ue(b); if (a > max_lt) { ERR(p, "max_long_term_frame_idx_plus1 %u out of range", a); return -1; } }
                sh->mmco[sh->n_mmco].op = (int)op; sh->mmco[sh->n_mmco].a = (int)a; sh->mmco[sh->n_mmco].b = (int)c;
                sh->n_mmco++;
            }
        }
    }
    if (pps->cabac && sh->type != P264_SLICE_I) { sh->cabac_init_idc = (int)br_ue(b); if (sh->cabac_init_idc > 2) { ERR(p, "cabac_init_idc %d out of range", sh->cabac_init_idc); return -1; } }
    sh->qp = pps->pic_init_qp + br_se(b);
    if (pps->deblock_ctrl) {
        sh->disable_deblock = (int)br_ue(b);
        if (sh->disable_deblock > 2) { ERR(p, "disable_deblocking_filter_idc %d out of range", sh->disable_deblock); return -1; }
        if (sh->disable_deblock != 1) {
            sh->alpha_off = br_se(b); sh->beta_off = br_se(b);
            if (sh->alpha_off < -6 || sh->alpha_off > 6 || sh->beta_off < -6 || sh->beta_off > 6) {          /* 7.4.3 */
                ERR(p, "slice_alpha_c0_offset_div2 %d / slice_beta_offset_div2 %d out of range (-6 .. 6)", sh->alpha_off, sh->beta_off); return -1;
            }
        }
    }
    if (br_overrun(b)) { ERR(p, "slice header overruns the NAL"); return -1; }
    return 0;
}

/* A B picture with explicit weights: every pair of references a bi-predicted 8x8 quadrant uses keeps
 * -128 <= w0 + w1 <= (logWD == 7 ? 127 : 128) for each component (H.264 8.4.2.3).  Pairs no block uses are not limited. */
static int bipred_sums_bad(p264parse *p)
{
    const picbuf_t *q = &p->buf[p->cur];
    for (int i = 0; i < p->n_mb * 4; i++) {
        const int r0 = q->ref[0][i], r1 = q->ref[1][i];
        if (r0 < 0 || r1 < 0 || r0 >= P264HIP_MAX_REFS || r1 >= P264HIP_MAX_REFS) continue;
        for (int c = 0; c < 3; c++) {
            const int d = p->pic.wp_denom[c > 0], sum = p->pic.wp_tab[0][r0][c][0] + p->pic.wp_tab[1][r1][c][0];
            if (sum < -128 || sum > (d == 7 ? 127 : 128)) {
                ERR(p, "macroblock %d: weights of list-0 index %d and list-1 index %d add up to %d (component %d, denominator %d; H.264 8.4.2.3)", i / 4, r0, r1, sum, c, d);
                return 1;
            }
        }
    }
    return 0;
}

/* ---------------------------------------------------------------- frame store ----------- */
/* Picture order count of the picture whose first slice header is sh (H.264 8.2.1; frames only: PicOrderCnt =
 * Min(TopFieldOrderCnt, BottomFieldOrderCnt)).  Types 0 and 2; type 1 is only ever met in streams without B slices,
 * where nothing depends on the count.  The state behind it (prevPicOrderCntMsb / Lsb, prevFrameNumOffset) moves on in
 * finish_picture_marking. */
static int poc_msb_of(const p264parse *p, const sps_t *sps, const slice_t *sh, int idr)
{
    const int max_lsb = 1 << sps->log2_max_poc_lsb, prev_msb = idr ? 0 : p->prev_poc_msb, prev_lsb = idr ? 0 : p->prev_poc_lsb;
    if (sh->poc_lsb < prev_lsb && prev_lsb - sh->poc_lsb >= max_lsb / 2) return prev_msb + max_lsb;
    if (sh->poc_lsb > prev_lsb && sh->poc_lsb - prev_lsb > max_lsb / 2) return prev_msb - max_lsb;
    return prev_msb;
}
static int frame_num_offset_of(const p264parse *p, const sps_t *sps, const slice_t *sh, int idr)
{
    if (idr) return 0;
    return p->prev_frame_num > sh->frame_num ? p->frame_num_offset + (1 << sps->log2_max_frame_num) : p->frame_num_offset;
}
static int picture_order_count(const p264parse *p, const slice_t *sh, int idr, int nal_ref_idc)
{
    const sps_t *sps = &p->sps[p->active_sps];
    if (sps->poc_type == 0) {
        const int top = poc_msb_of(p, sps, sh, idr) + sh->poc_lsb, bottom = top + sh->delta_poc_bottom;
        return top < bottom ? top : bottom;
    }
    if (sps->poc_type == 2) return idr ? 0 : 2 * (frame_num_offset_of(p, sps, sh, idr) + sh->frame_num) - (nal_ref_idc == 0);
    return 0;
}

/* PicNum of a short-term frame as the picture with frame_num `cur` sees it (8.2.4.1: FrameNumWrap) */
static inline int pic_num_of(int frame_num, int cur, int max_fn) { return frame_num > cur ? frame_num - max_fn : frame_num; }

/* Reference list X of the slice (H.264 8.2.4.2, 8.2.4.3).  Initial order - P slices: short-term pictures by descending
 * PicNum (decoder/lists.c:72-143); B slices (the reference stops at decoder/lists.c:136): list 0 the short-term pictures
 * before the current one in output order, nearest first, then those after it, nearest first - list 1 the other way round;
 * both: then the long-term pictures by ascending LongTermPicNum; a list 1 of more than one entry that equals list 0 gets its
 * first two entries swapped.  Then the slice's reordering commands (short-term: idc 0 / 1, long-term: idc 2; the reference
 * ignores them, decoder/lists.c:146-149). */
static int build_list(p264parse *p, const slice_t *sh, int X, int *out)
{
    const sps_t *sps = &p->sps[p->active_sps];
    const int max_fn = 1 << sps->log2_max_frame_num, isB = sh->type == P264_SLICE_B;
    int idx[2][P264HIP_MAX_REFS + 1], n = 0, n_short;
    for (int L = 0; L < (isB ? 2 : 1); L++) {
        n = 0;
        for (int i = 0; i < p->slots; i++) {
            if (!p->dpb[i].used || p->dpb[i].is_long || i == p->cur_slot) continue;
            p->dpb[i].pic_num = pic_num_of(p->dpb[i].frame_num, sh->frame_num, max_fn);
            int j = n++;
            if (!isB) while (j > 0 && p->dpb[idx[L][j-1]].pic_num < p->dpb[i].pic_num) { idx[L][j] = idx[L][j-1]; j--; }
            else {
                /* order key: list 0 wants POC below the current one first, descending, then the rest ascending; list 1 the mirror image */
                const int before_i = p->dpb[i].poc < p->pic.poc;
                for (; j > 0; j--) {
                    const dpb_frame_t *o = &p->dpb[idx[L][j-1]];
                    const int before_o = o->poc < p->pic.poc;
                    int i_first;
                    if (before_i != before_o) i_first = L == 0 ? before_i : !before_i;
                    else i_first = before_i ? p->dpb[i].poc > o->poc : p->dpb[i].poc < o->poc;     /* nearest first on either side */
                    if (!i_first) break;
                    idx[L][j] = idx[L][j-1];
                }
            }
            idx[L][j] = i;
        }
        n_short = n;
        for (int i = 0; i < p->slots; i++) {
            if (!p->dpb[i].used || !p->dpb[i].is_long || i == p->cur_slot) continue;
            int j = n++;
            while (j > n_short && p->dpb[idx[L][j-1]].long_idx > p->dpb[i].long_idx) { idx[L][j] = idx[L][j-1]; j--; }
            idx[L][j] = i;
        }
    }
    n_short = 0;
    for (int i = 0; i < p->slots; i++) if (p->dpb[i].used && !p->dpb[i].is_long && i != p->cur_slot) n_short++;
    if (n == 0) { ERR(p, "%s slice without a reference picture", isB ? "B" : "P"); return -1; }
    if (isB && n > 1 && !memcmp(idx[0], idx[1], sizeof(int) * (size_t)n)) { const int t = idx[1][0]; idx[1][0] = idx[1][1]; idx[1][1] = t; }
    const int *ini = idx[isB ? X : 0];
    const int len = sh->num_ref_idx[X], n_cmd = sh->n_reorder[X];
    int list[P264HIP_MAX_REFS + 1];
    for (int i = 0; i < len; i++) list[i] = ini[i < n ? i : n - 1];
    int pred = sh->frame_num, at = 0;
    for (int k = 0; k < n_cmd && at < len; k++) {
        const int idc = sh->reorder[X][k].idc, arg = sh->reorder[X][k].arg;
        int slot = -1;
        if (idc == 2) {                                   /* long_term_pic_num */
            for (int i = n_short; i < n; i++) if (p->dpb[ini[i]].long_idx == arg) slot = ini[i];
        } else {
            int d = arg + 1;
            pred = idc == 0 ? pred - d : pred + d;
            if (pred < 0) pred += max_fn;
            if (pred >= max_fn) pred -= max_fn;
            int want = pic_num_of(pred, sh->frame_num, max_fn);
            for (int i = 0; i < p->slots; i++) if (p->dpb[i].used && !p->dpb[i].is_long && i != p->cur_slot && p->dpb[i].pic_num == want) slot = i;
        }
        if (slot < 0) { ERR(p, "reordering names a picture that is not in the frame store"); return -1; }
        for (int i = len; i > at; i--) list[i] = list[i-1];
        list[at++] = slot;
        int w = at;
        for (int r = at; r <= len; r++) if (list[r] != slot) list[w++] = list[r];
    }
    for (int i = 0; i < len; i++) out[i] = list[i];
    return len;
}

/* Implicit bi-prediction weights of the picture (H.264 8.4.2.3.1 with weighted_bipred_idc 2; the reference computes the same
 * numbers in p264_macroblock_bipred_init, core/macroblock.c:1400-1430): weight of the list-0 prediction for every pair of
 * reference indices; 32 (the plain average) where the distances do not give a weight in -64 .. 128. */
static void implicit_weights(p264parse *p)
{
    for (int r0 = 0; r0 < P264HIP_MAX_REFS; r0++)
        for (int r1 = 0; r1 < P264HIP_MAX_REFS; r1++) {
            int w0 = 32;
            if (p->pic.weighted_bipred && r0 < p->pic.n_list[0] && r1 < p->pic.n_list[1]) {
                const dpb_frame_t *f0 = &p->dpb[p->pic.list[0][r0]], *f1 = &p->dpb[p->pic.list[1][r1]];
                const int td = clip3i(f1->poc - f0->poc, -128, 127), tb = clip3i(p->pic.poc - f0->poc, -128, 127);
                if (td != 0 && !f0->is_long && !f1->is_long) {
                    const int tx = (16384 + (td < 0 ? -td : td) / 2) / td;
                    const int dsf = clip3i((tb * tx + 32) >> 6, -1024, 1023) >> 2;
                    if (dsf >= -64 && dsf <= 128) w0 = 64 - dsf;
                }
            }
            p->pic.bipred_weight[r0 * P264HIP_MAX_REFS + r1] = (int16_t)w0;
        }
}

/* ---- the output process (H.264 C.4.5.3; include/p264parse.h has the rule) ----
 * the member of W that is due first: the smallest order count, of equal ones (a broken stream) the one decoded first; -1: W is empty */
static int wait_first(const wait_t *w, int n)
{
    int at = -1;
    for (int i = 0; i < n; i++)
        if (w[i].waiting && (at < 0 || w[i].poc < w[at].poc || (w[i].poc == w[at].poc && w[i].index < w[at].index))) at = i;
    return at;
}
static void wait_emit(wait_t *w, int slot, p264parse_output_t *out, int *n_out)
{
    p264parse_output_t *o = &out[(*n_out)++];
    o->slot = slot; o->poc = w[slot].poc; o->decode_index = w[slot].index; o->flags = w[slot].flags;
    w[slot].waiting = 0;
}
/* steps 1 - 3 for the picture completed in `slot` (n slots; *n_wait = |W|): everything is due in front of an IDR picture or one with
 * operation 5, the picture joins W, and W shrinks to `depth` */
static void output_steps(wait_t *w, int n, int *n_wait, int slot, int poc, int index, int flags, int depth, p264parse_output_t *out, int *n_out)
{
    if (flags & (P264PARSE_OUT_IDR | P264PARSE_OUT_MMCO5)) for (int i; (i = wait_first(w, n)) >= 0; (*n_wait)--) wait_emit(w, i, out, n_out);
    w[slot].waiting = 1; w[slot].poc = poc; w[slot].index = index; w[slot].flags = flags;
    for (++*n_wait; *n_wait > depth; (*n_wait)--) wait_emit(w, wait_first(w, n), out, n_out);
}
/* the picture in cur_slot is complete and marked: p->outs becomes what is due with it (steps 1 - 4), and the return the slot of
 * the next picture (step 5), -1 where every slot holds a reference */
static int output_process(p264parse *p, int had_mmco5)
{
    int n_wait = 0;
    for (int i = 0; i < p->slots; i++) n_wait += p->wait[i].waiting;
    p->n_outs = 0;
    output_steps(p->wait, p->slots, &n_wait, p->cur_slot, p->dpb[p->cur_slot].poc, p->decode_index,
                 (p->pic.is_idr ? P264PARSE_OUT_IDR : 0) | (had_mmco5 ? P264PARSE_OUT_MMCO5 : 0), p->reorder, p->outs, &p->n_outs);
    for (;;) {
        for (int i = 0; i < p->slots; i++) if (!p->dpb[i].used && !p->wait[i].waiting) return i;
        const int first = wait_first(p->wait, p->slots);        /* C.4.5.3 "bumping": no empty frame buffer */
        if (first < 0) return -1;
        wait_emit(p->wait, first, p->outs, &p->n_outs);
    }
}

/* Reference picture marking (H.264 8.2.5; the reference implements the sliding window only, decoder/lists.c:152-228) and
 * the choice of the next slot. */
static void finish_picture_marking(p264parse *p)
{
    const sps_t *sps = &p->sps[p->active_sps];
    const slice_t *first = &p->pic.first;
    int max_fn = 1 << sps->log2_max_frame_num;
    dpb_frame_t *cur = &p->dpb[p->cur_slot];
    int cur_long = 0, cur_long_idx = 0, had_mmco5 = 0;
    if (p->pic.is_idr) {
        for (int i = 0; i < p->slots; i++) if (i != p->cur_slot) p->dpb[i].used = 0;
        if (first->long_term_flag) { cur_long = 1; cur_long_idx = 0; }
    } else if (p->pic.ref_idc && first->adaptive_marking) {
        /* 8.2.5.4: the commands in order; PicNum relative to the current picture's frame_num */
        for (int k = 0; k < first->n_mmco; k++) {
            const int op = first->mmco[k].op, a = first->mmco[k].a, b = first->mmco[k].b;
            if (op == 1 || op == 3) {
                const int want = first->frame_num - (a + 1);
                for (int i = 0; i < p->slots; i++) {
                    dpb_frame_t *f = &p->dpb[i];
                    if (!f->used || f->is_long || i == p->cur_slot) continue;
                    if (pic_num_of(f->frame_num, first->frame_num, max_fn) != want) continue;
                    if (op == 1) f->used = 0;
                    else {                                  /* 3: the index is taken away from whoever holds it, then assigned */
                        for (int j = 0; j < p->slots; j++) if (j != i && p->dpb[j].used && p->dpb[j].is_long && p->dpb[j].long_idx == b) p->dpb[j].used = 0;
                        f->is_long = 1; f->long_idx = b;
                    }
                }
            } else if (op == 2) {
                for (int i = 0; i < p->slots; i++) if (p->dpb[i].used && p->dpb[i].is_long && p->dpb[i].long_idx == a && i != p->cur_slot) p->dpb[i].used = 0;
            } else if (op == 4) {
                for (int i = 0; i < p->slots; i++) if (p->dpb[i].used && p->dpb[i].is_long && p->dpb[i].long_idx >= a && i != p->cur_slot) p->dpb[i].used = 0;
            } else if (op == 5) {
                for (int i = 0; i < p->slots; i++) if (i != p->cur_slot) p->dpb[i].used = 0;
                had_mmco5 = 1;
            } else if (op == 6) {
                for (int j = 0; j < p->slots; j++) if (j != p->cur_slot && p->dpb[j].used && p->dpb[j].is_long && p->dpb[j].long_idx == b) p->dpb[j].used = 0;
                cur_long = 1; cur_long_idx = b;
            }
        }
    } else if (p->pic.ref_idc) {
        /* 8.2.5.3 sliding window: when short-term + long-term pictures fill num_ref_frames, the oldest short-term one goes */
        int cnt = 0, oldest = -1, oldest_num = 0;
        for (int i = 0; i < p->slots; i++) {
            if (!p->dpb[i].used || i == p->cur_slot) continue;
            cnt++;
            if (p->dpb[i].is_long) continue;
            const int num = pic_num_of(p->dpb[i].frame_num, first->frame_num, max_fn);
            if (oldest < 0 || num < oldest_num) { oldest = i; oldest_num = num; }
        }
        int cap = sps->num_ref_frames > 0 ? sps->num_ref_frames : 1;
        if (cnt >= cap && oldest >= 0) p->dpb[oldest].used = 0;
    }
    /* after memory_management_control_operation 5 the picture is inferred to have had frame_num 0 (H.264 7.4.3, 8.2.1): the
     * pictures that follow compute their PicNums against that */
    if (p->pic.ref_idc) { cur->used = 1; cur->frame_num = had_mmco5 ? 0 : first->frame_num; cur->is_long = cur_long; cur->long_idx = cur_long_idx; }
    /* picture order count: what the pictures behind this one measure theirs against (8.2.1; after operation 5 the picture
     * counts as POC 0 - frames, bottom not below top) */
    cur->poc = had_mmco5 ? 0 : p->pic.poc; cur->uid = p->pic.uid;
    if (sps->poc_type == 0 && p->pic.ref_idc) {
        p->prev_poc_msb = had_mmco5 ? 0 : poc_msb_of(p, sps, first, p->pic.is_idr);
        p->prev_poc_lsb = had_mmco5 ? 0 : first->poc_lsb;
    }
    if (sps->poc_type == 2) { p->frame_num_offset = had_mmco5 ? 0 : frame_num_offset_of(p, sps, first, p->pic.is_idr); p->prev_frame_num = had_mmco5 ? 0 : first->frame_num; }
    /* next picture goes into a slot that holds no reference - nor, with output order on, a picture that waits */
    int next = -1;
    if (p->out_on) next = output_process(p, had_mmco5);
    else for (int i = 0; i < p->slots; i++) if (!p->dpb[i].used) { next = i; break; }
    p->decode_index++;
    if (next < 0) {                               /* a stream that keeps more pictures than num_ref_frames: drop the oldest short-term one */
        int oldest = -1, oldest_num = 0;
        for (int i = 0; i < p->slots; i++) {
            if (p->dpb[i].is_long) continue;
            const int num = pic_num_of(p->dpb[i].frame_num, first->frame_num, max_fn);
            if (oldest < 0 || num < oldest_num) { oldest = i; oldest_num = num; }
        }
        next = oldest >= 0 ? oldest : p->cur_slot;
        p->dpb[next].used = 0;
    }
    p->cur_slot = next;
}

/* ---------------------------------------------------------------- neighbours ------------ */
typedef struct { int ref, mvx, mvy; } nbmv_t;      /* ref: -2 unavailable, -1 intra */

/* motion data of the 4x4 block at picture position (x4,y4), as a predictor for the current MB */
static nbmv_t nb_motion(const p264parse *p, int x4, int y4, int list)
{
    nbmv_t r = { -2, 0, 0 };
    /* where the block lies relative to the current macroblock decides everything: inside it - decoded so far or not; in the
     * left / top / top-right / top-left neighbour - that macroblock's availability (begin_mb); anywhere else - not decoded yet */
    const int dx = x4 - p->mbx * 4, dy = y4 - p->mby * 4, sub = (y4 & 3) * 4 + (x4 & 3);
    int i;
    if (dy >= 0) {
        if (dx >= 0) { if (dx >= 4 || dy >= 4 || !((p->mv_done[list] >> sub) & 1)) return r; i = p->mbi; }
        else { if (dy >= 4 || !(p->cur_avail & P264_AVAIL_LEFT)) return r; i = p->mbi - 1; }
    } else {
        if (dx < 0)      { if (!(p->cur_avail & P264_AVAIL_TOPLEFT)) return r;  i = p->mbi - p->mb_w - 1; }
        else if (dx < 4) { if (!(p->cur_avail & P264_AVAIL_TOP)) return r;      i = p->mbi - p->mb_w; }
        else             { if (dx >= 8 || !(p->cur_avail & P264_AVAIL_TOPRIGHT)) return r; i = p->mbi - p->mb_w + 1; }
    }
    const picbuf_t *q = &p->buf[p->cur];
    const int8_t *ref = q->ref[list]; const int16_t *mv = q->mv[list];
    r.ref = ref[i * 4 + ((y4 & 2) | ((x4 >> 1) & 1))];     /* -1: intra, or (B pictures) this list is not used there */
    r.mvx = mv[(i * 16 + sub) * 2]; r.mvy = mv[(i * 16 + sub) * 2 + 1];
    return r;
}

/* H.264 8.4.1.3 (core/macroblock.c:87-175).  (bx,by,bw) in 4x4 units inside the MB;
 * dir: 0 none, 1 = 16x8 upper, 2 = 16x8 lower, 3 = 8x16 left, 4 = 8x16 right. */
/* the block `sub` of macroblock i (which exists and is decoded) as a predictor */
static inline nbmv_t nb_of_mb(const p264parse *p, int i, int sub, int list)
{
    const picbuf_t *q = &p->buf[p->cur];
    const int8_t *ref = q->ref[list]; const int16_t *mv = q->mv[list];
    nbmv_t r;
    r.ref = ref[i * 4 + (((sub >> 2) & 2) | ((sub >> 1) & 1))];
    r.mvx = mv[(i * 16 + sub) * 2]; r.mvy = mv[(i * 16 + sub) * 2 + 1];
    return r;
}
static void predict_mv(const p264parse *p, int bx, int by, int bw, int ref, int dir, int *px, int *py, int list)
{
    int x0 = p->mbx * 4 + bx, y0 = p->mby * 4 + by;
    nbmv_t a, b, c;
    if (bw == 4 && by == 0) {
        /* the whole macroblock or its upper half (P_L0_16x16, P_SKIP, B 16x16, spatial direct, 16x8 upper - most calls): the neighbours are block 3 of the
         * macroblock to the left, block 12 of the one above, block 12 of the one above to the right or else block 15 of the
         * one above to the left; nothing but the availability flags to ask */
        const nbmv_t none = { -2, 0, 0 };
        const unsigned av = p->cur_avail;
        a = (av & P264_AVAIL_LEFT) ? nb_of_mb(p, p->mbi - 1, 3, list) : none;
        b = (av & P264_AVAIL_TOP) ? nb_of_mb(p, p->mbi - p->mb_w, 12, list) : none;
        c = (av & P264_AVAIL_TOPRIGHT) ? nb_of_mb(p, p->mbi - p->mb_w + 1, 12, list)
          : (av & P264_AVAIL_TOPLEFT) ? nb_of_mb(p, p->mbi - p->mb_w - 1, 15, list) : none;
    } else {
        a = nb_motion(p, x0 - 1, y0, list); b = nb_motion(p, x0, y0 - 1, list); c = nb_motion(p, x0 + bw, y0 - 1, list);
        if (c.ref == -2) c = nb_motion(p, x0 - 1, y0 - 1, list);
    }
    if (dir == 1 && b.ref == ref) { *px = b.mvx; *py = b.mvy; return; }
    if (dir == 2 && a.ref == ref) { *px = a.mvx; *py = a.mvy; return; }
    if (dir == 3 && a.ref == ref) { *px = a.mvx; *py = a.mvy; return; }
    if (dir == 4 && c.ref == ref) { *px = c.mvx; *py = c.mvy; return; }
    int hits = (a.ref == ref) + (b.ref == ref) + (c.ref == ref);
    if (hits == 1) {
        const nbmv_t *s = a.ref == ref ? &a : b.ref == ref ? &b : &c;
        *px = s->mvx; *py = s->mvy; return;
    }
    if (hits == 0 && b.ref == -2 && c.ref == -2 && a.ref != -2) { *px = a.mvx; *py = a.mvy; return; }
    *px = median3(a.mvx, b.mvx, c.mvx); *py = median3(a.mvy, b.mvy, c.mvy);
}

static void set_motion(p264parse *p, int bx, int by, int bw, int bh, int mvx, int mvy, int list)
{
    picbuf_t *q = &p->buf[p->cur];
    int16_t *mv = q->mv[list];
    if (bw == 4 && bh == 4) {                                   /* the whole macroblock: sixteen equal vectors, eight 8-byte stores */
        const uint32_t one = (uint32_t)(uint16_t)mvx | (uint32_t)(uint16_t)mvy << 16;
        const uint64_t two = (uint64_t)one | (uint64_t)one << 32;
        int16_t *d = mv + (size_t)p->mbi * 32;
        for (int k = 0; k < 8; k++) memcpy(d + 4 * k, &two, 8);
        p->mv_done[list] = 0xffffu;
        return;
    }
    for (int y = by; y < by + bh; y++)
        for (int x = bx; x < bx + bw; x++) {
            mv[(p->mbi * 16 + y * 4 + x) * 2] = (int16_t)mvx;
            mv[(p->mbi * 16 + y * 4 + x) * 2 + 1] = (int16_t)mvy;
            p->mv_done[list] |= 1u << (y * 4 + x);
        }
}

/* Intra4x4PredMode predictor (H.264 8.3.1.1; core/macroblock.c:40-51).  Both entropy coders come through here.
 * dcPredModePredictedFlag: a neighbouring macroblock that is not available - or, with constrained_intra_pred_flag, is inter -
 * makes the prediction 2 whatever the other neighbour says (the reference reads the flag and drops it, decoder/set.c:241) */
static int predict_i4mode(const p264parse *p, int blk)
{
    const picbuf_t *q = &p->buf[p->cur];
    const int cip = p->pps[p->sh.pps_id].constrained_intra;
    int x = blk_x[blk], y = blk_y[blk], ma, mb;
    if (x > 0) ma = q->i4[p->mbi * 16 + blk_of_xy[y][x-1]];
    else if ((p->cur_avail & P264_AVAIL_LEFT) && !(cip && !P264_MB_IS_INTRA(q->mb[p->mbi - 1].mb_type)))
        ma = q->mb[p->mbi - 1].mb_type == P264_MB_I4x4 ? q->i4[(p->mbi - 1) * 16 + blk_of_xy[y][3]] : 2;
    else ma = -1;
    if (y > 0) mb = q->i4[p->mbi * 16 + blk_of_xy[y-1][x]];
    else if ((p->cur_avail & P264_AVAIL_TOP) && !(cip && !P264_MB_IS_INTRA(q->mb[p->mbi - p->mb_w].mb_type)))
        mb = q->mb[p->mbi - p->mb_w].mb_type == P264_MB_I4x4 ? q->i4[(p->mbi - p->mb_w) * 16 + blk_of_xy[3][x]] : 2;
    else mb = -1;
    int m = ma < mb ? ma : mb;
    return m < 0 ? 2 : m;
}
/* (An Intra 8x8 neighbour - an I4x4 record with P264_MB_I8X8 - gives Intra8x8PredMode[luma4x4BlkIdxN >> 2] (8.3.1.1): its record keeps
 * the mode of 8x8 block k at i4[4k .. 4k+3], and decode-order indices 4k .. 4k+3 are quadrant k, so the look-ups above read exactly
 * that.)
 * Intra8x8PredMode predictor (H.264 8.3.2.1) of 8x8 block k: the minimum over the neighbours A (left) and B (above); 2 where one is
 * not available or, under constrained_intra_pred_flag, inter; a neighbour that is neither I4x4 nor Intra 8x8 counts as 2; an Intra 8x8
 * neighbour gives its block's mode, an Intra4x4 one Intra4x4PredMode[8x8 block N * 4 + n] with n = 1 for A and n = 2 for B - one
 * look-up for both kinds, the storage being what it is */
static int predict_i8mode(const p264parse *p, int k)
{
    const picbuf_t *q = &p->buf[p->cur];
    const int cip = p->pps[p->sh.pps_id].constrained_intra;
    int ma, mb;
    if (k & 1) ma = q->i4[p->mbi * 16 + 4 * (k - 1)];
    else if ((p->cur_avail & P264_AVAIL_LEFT) && !(cip && !P264_MB_IS_INTRA(q->mb[p->mbi - 1].mb_type)))
        ma = q->mb[p->mbi - 1].mb_type == P264_MB_I4x4 ? q->i4[(p->mbi - 1) * 16 + 4 * (k + 1) + 1] : 2;
    else ma = -1;
    if (k & 2) mb = q->i4[p->mbi * 16 + 4 * (k - 2)];
    else if ((p->cur_avail & P264_AVAIL_TOP) && !(cip && !P264_MB_IS_INTRA(q->mb[p->mbi - p->mb_w].mb_type)))
        mb = q->mb[p->mbi - p->mb_w].mb_type == P264_MB_I4x4 ? q->i4[(p->mbi - p->mb_w) * 16 + 4 * (k + 2) + 2] : 2;
    else mb = -1;
    int m = ma < mb ? ma : mb;
    return m < 0 ? 2 : m;
}

/* ---------------------------------------------------------------- macroblock layer ------ */
typedef struct {
    int16_t dc_luma[16], dc_chroma[16], blk[24][16];
    uint32_t mask;
} mbcoef_t;

static int coef_reserve(picbuf_t *q, size_t more)
{
    if (q->coef_n + more <= q->coef_cap) return 0;
    size_t cap = q->coef_cap * 2 + more;
    int16_t *n = (int16_t *)q->alloc(cap * 16 * sizeof(int16_t));
    if (!n) return -1;
    memcpy(n, q->coef, q->coef_n * 16 * sizeof(int16_t));
    if (q->coef_own) q->release(q->coef);               /* (else: a section of q->block, which stays) */
    q->coef = n; q->coef_cap = cap; q->coef_own = 1;
    return 0;
}

#include "parser_cabac.h"

/* residual( ) - decoder/macroblock.c:410-486 */
/* total_coeff predictor nC (H.264 9.2.1; core/macroblock.c:53-65): the mean of the counts of the blocks to the left and above.
 * The coefficient counts around and inside the macroblock on an 8-wide grid (left neighbour of a block one to the left, upper one
 * eight back; 0x80 = no such neighbour): luma block (x, y) at 8 (1 + y) + 1 + x, Cb (x, y) at 8 (6 + y) + 1 + x, Cr at
 * 8 (6 + y) + 5 + x.  nC of 9.2.1 is then two loads and a rounded mean that an absent neighbour falls out of by itself
 * (predict_nc: two table look-ups and four branches per block). */
static const uint8_t nc_pos[24] = { 9, 10, 17, 18, 11, 12, 19, 20, 25, 26, 33, 34, 27, 28, 35, 36,  49, 50, 57, 58,  53, 54, 61, 62 };
static inline int nc_of(const uint8_t *nc, int at)
{
    int r = nc[at - 1] + nc[at - 8];
    if (r < 0x80) r = (r + 1) >> 1;
    return r & 0x7f;
}
static int parse_residual(p264parse *p, bitrd_t *b, p264hip_mb_t *m, mbcoef_t *cf)
{
    uint8_t *nnz = p->nnz + (size_t)p->mbi * 24;
    int cbp_l = m->cbp & 15, cbp_c = m->cbp >> 4, tc;
    uint8_t nc[64];
    {
        const uint8_t *left = nnz - 24, *top = nnz - 24 * (size_t)p->mb_w;
        if (p->cur_avail & P264_AVAIL_LEFT) {
            nc[8] = left[5]; nc[16] = left[7]; nc[24] = left[13]; nc[32] = left[15];
            nc[48] = left[17]; nc[56] = left[19]; nc[52] = left[21]; nc[60] = left[23];
        } else nc[8] = nc[16] = nc[24] = nc[32] = nc[48] = nc[56] = nc[52] = nc[60] = 0x80;
        if (p->cur_avail & P264_AVAIL_TOP) {
            nc[1] = top[10]; nc[2] = top[11]; nc[3] = top[14]; nc[4] = top[15];
            nc[41] = top[18]; nc[42] = top[19]; nc[45] = top[22]; nc[46] = top[23];
        } else nc[1] = nc[2] = nc[3] = nc[4] = nc[41] = nc[42] = nc[45] = nc[46] = 0x80;
    }
    if (m->mb_type == P264_MB_I16x16) {
        if ((tc = cavlc_read_block(b, nc_of(nc, nc_pos[0]), 16, cf->dc_luma)) < 0) return -1;
        if (tc) cf->mask |= P264_COEF_LUMA_DC;
    }
    int maxc = m->mb_type == P264_MB_I16x16 ? 15 : 16;
    const int t8 = m->intra_modes & (P264_MB_T8X8 | P264_MB_I8X8);
    for (int i = 0; i < 16; i++) {
        const int at = nc_pos[i];
        nnz[i] = 0; nc[at] = 0;
        if (!(cbp_l & (1 << (i >> 2)))) continue;
        if (t8) {
            /* 7.3.5.3.2: an 8x8 block travels as four 4x4 blocks, each with its own nC and total_coeff (kept for the neighbours' nC);
             * level k of block j is scan position 4 k + j of the 8x8 block, whose 64 levels fill the quadrant's four entries */
            int16_t lv[16], *l8 = cf->blk[i & ~3];
            memset(lv, 0, sizeof lv);
            if ((i & 3) == 0) memset(l8, 0, 128);
            if ((tc = cavlc_read_block(b, nc_of(nc, at), 16, lv)) < 0) return -1;
            for (int k = 0; k < 16; k++) l8[4 * k + (i & 3)] = lv[k];
            nnz[i] = (uint8_t)tc; nc[at] = (uint8_t)tc;
            if (tc) cf->mask |= 0xfu << (i & ~3);
            continue;
        }
        if ((tc = cavlc_read_block(b, nc_of(nc, at), maxc, cf->blk[i])) < 0) return -1;
        nnz[i] = (uint8_t)tc; nc[at] = (uint8_t)tc;
        if (tc) cf->mask |= 1u << i;
    }
    if (cbp_c) {
        memset(cf->dc_chroma, 0, sizeof cf->dc_chroma);
        int t0, t1;
        if ((t0 = cavlc_read_block(b, -1, 4, cf->dc_chroma)) < 0) return -1;
        if ((t1 = cavlc_read_block(b, -1, 4, cf->dc_chroma + 4)) < 0) return -1;
        if (t0 | t1) cf->mask |= P264_COEF_CHROMA_DC;
    }
    for (int i = 16; i < 24; i++) {
        const int at = nc_pos[i];
        nnz[i] = 0; nc[at] = 0;
        if (!(cbp_c & 2)) continue;
        if ((tc = cavlc_read_block(b, nc_of(nc, at), 15, cf->blk[i])) < 0) return -1;
        nnz[i] = (uint8_t)tc; nc[at] = (uint8_t)tc;
        if (tc) cf->mask |= 1u << i;
    }
    return 0;
}

static int rd_residual(p264parse *p, bitrd_t *b, p264hip_mb_t *m, mbcoef_t *cf)
{
    return p->cabac_on ? parse_residual_cabac(p, m, cf) : parse_residual(p, b, m, cf);
}

static int store_coefs(p264parse *p, p264hip_mb_t *m, const mbcoef_t *cf)
{
    picbuf_t *q = &p->buf[p->cur];
    m->coef_mask = cf->mask;
    m->coef_index = (uint32_t)q->coef_n;
    if (!cf->mask) return 0;
    if (coef_reserve(q, 26) < 0) return -1;
    int16_t *dst = q->coef + q->coef_n * 16;
    if (cf->mask & P264_COEF_LUMA_DC)   { memcpy(dst, cf->dc_luma, 32); dst += 16; }
    if (cf->mask & P264_COEF_CHROMA_DC) { memcpy(dst, cf->dc_chroma, 32); dst += 16; }
    for (uint32_t left = cf->mask & 0xffffffu; left; left &= left - 1) { memcpy(dst, cf->blk[__builtin_ctz(left)], 32); dst += 16; }
    q->coef_n = (size_t)(dst - q->coef) / 16;
    return 0;
}

/* the four neighbours: they all lie in front of this macroblock, so only the picture's borders and the slice they belong to are
 * left to ask */
static inline int mb_neighbours(p264parse *p)
{
    int a = 0;
    const int w = p->mb_w, i = p->mbi, x = p->mbx;
    const uint16_t sn = (uint16_t)p->pic.slice_no, *so = p->slice_of;
    if (x > 0 && so[i - 1] == sn) a |= P264_AVAIL_LEFT;
    if (p->mby > 0) {
        if (so[i - w] == sn) a |= P264_AVAIL_TOP;
        if (x + 1 < w && so[i - w + 1] == sn) a |= P264_AVAIL_TOPRIGHT;
        if (x > 0 && so[i - w - 1] == sn) a |= P264_AVAIL_TOPLEFT;
    }
    p->cur_avail = a;
    return a;
}
static void begin_mb(p264parse *p, p264hip_mb_t *m)
{
    memset(m, 0, sizeof *m);
    p->mv_done[0] = p->mv_done[1] = 0;
    if (p->cabac_on) { p->cinfo[p->mbi] = 0; memset(p->mvd_abs[0] + p->mbi * 32, 0, 32); memset(p->mvd_abs[1] + p->mbi * 32, 0, 32); }
    const int a = mb_neighbours(p);
    m->avail = (uint8_t)a;
    int e = 0;
    if (p->sh.disable_deblock != 1) {
        e = P264_EDGE_INNER;
        if (p->mbx > 0 && (p->sh.disable_deblock == 0 || (a & P264_AVAIL_LEFT))) e |= P264_EDGE_LEFT;
        if (p->mby > 0 && (p->sh.disable_deblock == 0 || (a & P264_AVAIL_TOP)))  e |= P264_EDGE_TOP;
    }
    m->edges = (uint8_t)e;
    m->flags = p->slice_flags;                /* (0 in a slice that does not filter) */
}

/* the record's `avail` of an INTRA macroblock (I_PCM included): what intra prediction may read.  With constrained_intra_pred_flag
 * a neighbour in the slice counts only if it is intra itself (H.264 8.3.1.2, 8.3.3, 8.3.4).  p->cur_avail - vector prediction, nC,
 * the CABAC context increments - stays what the slice gives (data partitioning, the one exception of 9.2.1, is not decoded). */
static int intra_avail(const p264parse *p)
{
    int a = p->cur_avail;
    if (!p->pps[p->sh.pps_id].constrained_intra) return a;
    const p264hip_mb_t *mb = p->buf[p->cur].mb;
    const int i = p->mbi, w = p->mb_w;
    if ((a & P264_AVAIL_LEFT) && !P264_MB_IS_INTRA(mb[i - 1].mb_type)) a &= ~P264_AVAIL_LEFT;
    if ((a & P264_AVAIL_TOP) && !P264_MB_IS_INTRA(mb[i - w].mb_type)) a &= ~P264_AVAIL_TOP;
    if ((a & P264_AVAIL_TOPRIGHT) && !P264_MB_IS_INTRA(mb[i - w + 1].mb_type)) a &= ~P264_AVAIL_TOPRIGHT;
    if ((a & P264_AVAIL_TOPLEFT) && !P264_MB_IS_INTRA(mb[i - w - 1].mb_type)) a &= ~P264_AVAIL_TOPLEFT;
    return a;
}

/* QP bookkeeping of core/macroblock.c:1247-1252 (or the conformant chain in strict mode) */
static void finish_mb_qp(p264parse *p, p264hip_mb_t *m, int has_residual_syntax, int qp)
{
    if (p->strict_qp) {
        if (!has_residual_syntax) qp = p->qp_pred;
        p->qp_pred = qp;
    } else {
        if (m->mb_type != P264_MB_I16x16 && m->cbp == 0) qp = p->last_qp;
        p->last_qp = qp;
    }
    m->qp = (uint8_t)clip3i(qp, 0, 51);
}

/* this macroblock has no motion (intra, or a B macroblock before its partitions are read): index -1 and zero vectors, in list 1
 * where the stream can have B pictures at all */
static void clear_motion(p264parse *p)
{
    picbuf_t *q = &p->buf[p->cur];
    for (int l = 0; l < 2 && q->mv[l]; l++) { memset(q->ref[l] + p->mbi * 4, -1, 4); memset(q->mv[l] + p->mbi * 32, 0, 64); }
}

/* I_PCM (H.264 7.3.5, 8.3.5): pcm_alignment_zero_bits, then 384 sample bytes that go into the macroblock's place in coefs[] in one
 * piece - twelve 32-byte blocks, luma, Cb, Cr as the stream has them (include/p264hip.h).  The reference stops here
 * (decoder/macroblock.c:510-514).  For later macroblocks it counts as coded everywhere: total_coeff 16 in all 24 blocks (9.2.1),
 * every coded_block_flag 1 and coded_block_pattern 0x2f (9.3.3.1.1.9 / .4: cb_cbp asks nb_cbp), no mb_qp_delta (the next one's
 * context sees a delta of 0) and the QP chain untouched.  Its record carries qp 0: what the loop filter takes for it (8.7.2.2).
 * CAVLC: the samples lie at the next byte boundary of the bit reader.  CABAC: the terminate bin in front of them came back 1 and
 * the encoder has flushed as at the end of a slice (9.3.4.5: ten bits, the last of them a 1).  Where a bit-serial decoder stands
 * then is pos * 8 - n (what p264cabac_bits_left counts with), and that is the bit BEHIND the flush's last one: measured at the
 * end of every CABAC slice of the golden and test streams, where the same flush ends in the rbsp_stop_one_bit - pos * 8 - n was
 * rbsp_stop_bit() + 1 in all of them.  So the alignment zeros start at pos * 8 - n, the samples at the next
 * byte boundary, and the engine starts again behind them (9.3.1.2) with every context state kept. */
static int parse_ipcm(p264parse *p, bitrd_t *b, p264hip_mb_t *m)
{
    picbuf_t *q = &p->buf[p->cur];
    const uint8_t *src;
    if (p->cabac_on) {
        p264cabac_t *c = &p->cb;
        const int64_t bit = (int64_t)c->pos * 8 - c->n;          /* the first bit behind the flush */
        if (bit < 0 || bit > (int64_t)c->size * 8) { ERR(p, "macroblock overruns the slice data"); return -1; }
        const size_t at = (size_t)((bit + 7) >> 3);
        for (int64_t k = bit; k < (int64_t)at * 8; k++)
            if ((c->data[k >> 3] >> (7 - (k & 7))) & 1) { ERR(p, "pcm_alignment_zero_bit is not zero"); return -1; }
        /* (behind the samples the engine needs something to start on: at least end_of_slice_flag follows) */
        if (at + 384 >= c->size) { ERR(p, "macroblock overruns the slice data"); return -1; }
        src = c->data + at;
        p264cabac_start(c, src + 384, c->size - at - 384);
        p->cinfo[p->mbi] |= CI_DC_Y | CI_DC_CB | CI_DC_CR;
    } else {
        const int pad = (int)((0 - br_consumed(b)) & 7);
        if (pad && br_u(b, pad)) { ERR(p, "pcm_alignment_zero_bit is not zero"); return -1; }
        const size_t at = br_consumed(b) >> 3;
        if (br_overrun(b) || at + 384 > b->size) { ERR(p, "macroblock overruns the slice data"); return -1; }
        src = b->buf + at;
        b->pos = at + 384; b->win = 0; b->avail = 0;            /* the bit reader goes on behind the samples */
        br_refill(b);
    }
    if (coef_reserve(q, P264_IPCM_BLOCKS) < 0) return -1;
    memcpy(q->coef + q->coef_n * 16, src, 384);
    m->mb_type = P264_MB_IPCM;                                   /* qp, cbp, intra_modes: 0; flags: the slice's deltas, like any macroblock (begin_mb) */
    m->coef_mask = P264_IPCM_COEF_MASK;
    m->coef_index = (uint32_t)q->coef_n;
    q->coef_n += P264_IPCM_BLOCKS;
    clear_motion(p);
    memset(q->i4 + p->mbi * 16, 2, 16);
    memset(p->nnz + (size_t)p->mbi * 24, 16, 24);
    p->last_dqp = 0;
    return 0;
}

/* ---------------------------------------------------------------- direct prediction ------ */
/* B macroblocks: the reference has none of this (decoder/macroblock.c:168-171 rejects B macroblock types; its encoder-side helpers
 * core/macroblock.c:254-429 are not reachable from the decoder): H.264 7.3.5, 7.4.5 (tables 7-14, 7-18), 8.4.1.2. */

/* Direct prediction of the current macroblock (B_Skip, B_Direct_16x16, and the direct 8x8 quadrants of B_8x8): reference
 * indices per 8x8 quadrant and vectors per 4x4 block for both lists, into dr[2][4] / dm[2][16][2].  Nothing is stored:
 * the caller copies the quadrants that are direct. */
typedef struct { int8_t ref[2][4]; int16_t mv[2][16][2]; } direct_t;

static int min_positive(int a, int b) { return (a >= 0 && b >= 0) ? (a < b ? a : b) : (a > b ? a : b); }

static void direct_spatial(const p264parse *p, direct_t *d)
{   /* 8.4.1.2.2: the reference indices from the neighbours A, B, C of the MACROBLOCK, the vectors from the ordinary 16x16
     * prediction with them, zero where the co-located block does not move */
    const int x0 = p->mbx * 4, y0 = p->mby * 4;
    int ref[2], mv[2][2] = { { 0, 0 }, { 0, 0 } };
    for (int l = 0; l < 2; l++) {
        nbmv_t a = nb_motion(p, x0 - 1, y0, l), b = nb_motion(p, x0, y0 - 1, l), c = nb_motion(p, x0 + 4, y0 - 1, l);
        if (c.ref == -2) c = nb_motion(p, x0 - 1, y0 - 1, l);
        ref[l] = min_positive(a.ref < 0 ? -1 : a.ref, min_positive(b.ref < 0 ? -1 : b.ref, c.ref < 0 ? -1 : c.ref));
    }
    const int zero_pred = ref[0] < 0 && ref[1] < 0;
    if (zero_pred) ref[0] = ref[1] = 0;
    else for (int l = 0; l < 2; l++) if (ref[l] >= 0) predict_mv(p, 0, 0, 4, ref[l], 0, &mv[l][0], &mv[l][1], l);
    /* colZeroFlag: RefPicList1[0] is a short-term picture and the co-located block used reference index 0 with a vector
     * inside +-1 (direct_8x8_inference: the corner block of the quadrant speaks for it) */
    const int col_slot = p->list[1][0];
    const int col_short = !p->dpb[col_slot].is_long;
    const int8_t *cr = p->col_ref[col_slot] + p->mbi * 4; const int16_t *cm = p->col_mv[col_slot] + p->mbi * 32;
    const int inf = p->sps[p->active_sps].direct_8x8_inference;
    for (int blk = 0; blk < 16; blk++) {
        const int bx = blk & 3, by = blk >> 2, q = (by >> 1) * 2 + (bx >> 1);
        const int cb = inf ? ((by >> 1) * 3) * 4 + (bx >> 1) * 3 : blk;                          /* corner 4x4 of the quadrant: (0|3, 0|3) */
        const int col_zero = col_short && cr[q] == 0 && cm[cb * 2] >= -1 && cm[cb * 2] <= 1 && cm[cb * 2 + 1] >= -1 && cm[cb * 2 + 1] <= 1;
        for (int l = 0; l < 2; l++) {
            d->ref[l][q] = (int8_t)ref[l];
            const int z = zero_pred || ref[l] < 0 || (ref[l] == 0 && col_zero);
            d->mv[l][blk][0] = (int16_t)(z ? 0 : mv[l][0]); d->mv[l][blk][1] = (int16_t)(z ? 0 : mv[l][1]);
        }
    }
}

static void direct_temporal(const p264parse *p, direct_t *d)
{   /* 8.4.1.2.3: list 0 points at the picture the co-located block referred to, list 1 at RefPicList1[0]; the co-located
     * vector split in proportion to the picture distances */
    const int col_slot = p->list[1][0];
    const int8_t *cr = p->col_ref[col_slot] + p->mbi * 4; const int32_t *cu = p->col_uid[col_slot] + p->mbi * 4;
    const int16_t *cm = p->col_mv[col_slot] + p->mbi * 32;
    const int inf = p->sps[p->active_sps].direct_8x8_inference;
    for (int q = 0; q < 4; q++) {
        int r0 = 0, scale = 0, use_col = 0;                       /* intra co-located block: both indices 0, zero vectors */
        if (cr[q] >= 0) {
            r0 = -1;
            for (int i = 0; i < p->n_list[0] && r0 < 0; i++) if ((int32_t)p->dpb[p->list[0][i]].uid == cu[q]) r0 = i;   /* lowest index that names that picture */
            if (r0 < 0) r0 = 0;                                   /* (a stream that dropped it from list 0: not conformant; stay defined) */
            const dpb_frame_t *f0 = &p->dpb[p->list[0][r0]], *f1 = &p->dpb[col_slot];
            const int tb = clip3i(p->pic.poc - f0->poc, -128, 127), td = clip3i(f1->poc - f0->poc, -128, 127);
            use_col = 1;
            if (f0->is_long || td == 0) scale = -1;               /* mvL0 = mvCol, mvL1 = 0 */
            else { const int tx = (16384 + (td < 0 ? -td : td) / 2) / td; scale = clip3i((tb * tx + 32) >> 6, -1024, 1023); }
        }
        d->ref[0][q] = (int8_t)r0; d->ref[1][q] = 0;
        for (int k = 0; k < 4; k++) {
            const int bx = (q & 1) * 2 + (k & 1), by = (q >> 1) * 2 + (k >> 1), blk = by * 4 + bx;
            const int cb = inf ? ((q >> 1) * 3) * 4 + (q & 1) * 3 : blk;
            const int cx = use_col ? cm[cb * 2] : 0, cy = use_col ? cm[cb * 2 + 1] : 0;
            int m0x = cx, m0y = cy, m1x = 0, m1y = 0;
            if (use_col && scale != -1) { m0x = (scale * cx + 128) >> 8; m0y = (scale * cy + 128) >> 8; m1x = m0x - cx; m1y = m0y - cy; }
            d->mv[0][blk][0] = (int16_t)m0x; d->mv[0][blk][1] = (int16_t)m0y;
            d->mv[1][blk][0] = (int16_t)m1x; d->mv[1][blk][1] = (int16_t)m1y;
        }
    }
}

static void direct_predict(const p264parse *p, direct_t *d)
{
    if (p->sh.direct_spatial) direct_spatial(p, d); else direct_temporal(p, d);
}
/* copy quadrant q of a direct prediction into the picture arrays (vectors of an unused list are zero, its index -1) */
static void store_direct_quadrant(p264parse *p, const direct_t *d, int q, int list)
{
    picbuf_t *b = &p->buf[p->cur];
    b->ref[list][p->mbi * 4 + q] = d->ref[list][q];
    for (int k = 0; k < 4; k++) {
        const int bx = (q & 1) * 2 + (k & 1), by = (q >> 1) * 2 + (k >> 1), blk = by * 4 + bx;
        const int used = d->ref[list][q] >= 0;
        set_motion(p, bx, by, 1, 1, used ? d->mv[list][blk][0] : 0, used ? d->mv[list][blk][1] : 0, list);
    }
}

/* the whole macroblock direct-predicted (B_Skip, B_Direct_16x16) */
static void store_direct_mb(p264parse *p)
{
    direct_t d;
    direct_predict(p, &d);
    for (int l = 0; l < 2; l++) for (int k = 0; k < 4; k++) store_direct_quadrant(p, &d, k, l);
    if (p->cabac_on) p->cinfo[p->mbi] |= CI_DIRECT16 | CI_D8(0) | CI_D8(1) | CI_D8(2) | CI_D8(3);
}

/* P_Skip (decoder/macroblock.c:895-934) and B_Skip: no syntax, inferred motion, no residual */
static void decode_skip(p264parse *p)
{
    picbuf_t *q = &p->buf[p->cur];
    p264hip_mb_t *m = &q->mb[p->mbi];
    begin_mb(p, m);
    memset(p->nnz + (size_t)p->mbi * 24, 0, 24);
    memset(q->i4 + p->mbi * 16, 2, 16);
    if (p->sh.type == P264_SLICE_B) {
        m->mb_type = P264_MB_B;
        store_direct_mb(p);
    } else {
        m->mb_type = P264_MB_P_SKIP;
        memset(q->ref[0] + p->mbi * 4, 0, 4);
        int mvx = 0, mvy = 0;
        /* (8.4.1.1: the zero vector without a left or an upper neighbour or next to one at rest on reference 0; else the 16x16 prediction) */
        if ((p->cur_avail & (P264_AVAIL_LEFT | P264_AVAIL_TOP)) == (P264_AVAIL_LEFT | P264_AVAIL_TOP)) {
            const nbmv_t a = nb_of_mb(p, p->mbi - 1, 3, 0), b = nb_of_mb(p, p->mbi - p->mb_w, 12, 0);
            if (!((a.ref == 0 && a.mvx == 0 && a.mvy == 0) || (b.ref == 0 && b.mvx == 0 && b.mvy == 0)))
                predict_mv(p, 0, 0, 4, 0, 0, &mvx, &mvy, 0);
        }
        set_motion(p, 0, 0, 4, 4, mvx, mvy, 0);
    }
    m->coef_index = (uint32_t)q->coef_n;
    finish_mb_qp(p, m, 0, p->sh.qp);
    p->last_dqp = 0;
    if (p->cabac_on) p->cinfo[p->mbi] |= CI_SKIP;
}

/* ---------------------------------------------------------------- inter prediction ------- */
/* The partitions of an inter macroblock, P (decoder/macroblock.c:140-167, 304-408) or B: one, two or four; a partition of an 8x8
 * macroblock splits into sub-partitions of (sw, sh), any other is its own only sub-partition. */

/* which lists a partition predicts from: bit 0 list 0, bit 1 list 1; 0: a direct quadrant of B_8x8 */
enum { PRED_L0 = 1, PRED_L1 = 2, PRED_BI = 3 };
typedef struct { uint8_t x, y, w, h, sw, sh, dir, pred; } part_t;     /* 4x4 units inside the macroblock; dir: see predict_mv */

/* 16x16, 16x8 or 8x16 (shape 0, 1, 2) with the prediction of each partition; returns their number */
static inline int mb_partitions(part_t *pt, int shape, const uint8_t *pred)
{
    static const uint8_t geo[3][2][5] = {   /* x, y, w, h, dir */
        { {0,0,4,4,0}, {0,0,0,0,0} }, { {0,0,4,2,1}, {0,2,4,2,2} }, { {0,0,2,4,3}, {2,0,2,4,4} } };
    const int n = shape == 0 ? 1 : 2;
    for (int k = 0; k < n; k++) {
        const uint8_t *g = geo[shape][k];
        pt[k] = (part_t){ g[0], g[1], g[2], g[3], g[2], g[3], g[4], pred[k] };
    }
    return n;
}
/* quadrant k of an 8x8 macroblock with sub-partitions of (sw, sh) */
static inline void sub_partition(part_t *pt, int k, int sw, int sh, int pred)
{
    pt[k] = (part_t){ (uint8_t)((k & 1) * 2), (uint8_t)((k >> 1) * 2), 2, 2, (uint8_t)sw, (uint8_t)sh, 0, (uint8_t)pred };
}

/* ref_idx and mvd of the partitions pt[0 .. np) for n_lists lists (P: 1, every partition PRED_L0; B: 2), in the order of the syntax:
 * all ref_idx_l0, all ref_idx_l1, all mvd_l0, all mvd_l1.  read_ref 0: the indices are not coded, all 0 (P_8x8ref0).  d: the
 * direct prediction of the macroblock where a partition is direct.  n_lists is a constant at both call sites: the compiler makes
 * two routines of this one, and the P one is the hottest host code there is. */
static inline __attribute__((always_inline)) int parse_inter_pred(p264parse *p, bitrd_t *b, const int n_lists, int np, const part_t *pt, int read_ref, const direct_t *d)
{
    picbuf_t *q = &p->buf[p->cur];
    int r[2][4];
    for (int l = 0; l < n_lists; l++) {
        const int nref = p->sh.num_ref_idx[l];
        int8_t *ref = q->ref[l] + p->mbi * 4;
        for (int k = 0; k < np; k++) {
            if (!(pt[k].pred & (1 << l))) continue;
            r[l][k] = read_ref ? rd_ref_idx(p, b, l, pt[k].x, pt[k].y, nref) : 0;
            if (r[l][k] < 0 || r[l][k] >= nref) { ERR(p, "ref_idx out of range"); return -1; }
            for (int y = pt[k].y >> 1; y < (pt[k].y + pt[k].h) >> 1; y++)                    /* (at once: the next partition's context looks at it) */
                for (int x = pt[k].x >> 1; x < (pt[k].x + pt[k].w) >> 1; x++) ref[y * 2 + x] = (int8_t)r[l][k];
        }
    }
    for (int l = 0; l < n_lists; l++)
        for (int k = 0; k < np; k++) {
            const part_t *t = &pt[k];
            if (t->pred == 0) { store_direct_quadrant(p, d, k, l); continue; }                /* its turn: the derived motion becomes visible */
            /* a partition that does not use the list still becomes "decoded" for it (index -1, zero vector) when its turn comes */
            if (!(t->pred & (1 << l))) { set_motion(p, t->x, t->y, t->w, t->h, 0, 0, l); continue; }
            for (int sy = 0; sy < t->h; sy += t->sh)
                for (int sx = 0; sx < t->w; sx += t->sw) {
                    int dx, dy, px, py;
                    if (rd_mvd(p, b, l, t->x + sx, t->y + sy, t->sw, t->sh, &dx, &dy) < 0) { ERR(p, "mvd out of range"); return -1; }
                    predict_mv(p, t->x + sx, t->y + sy, t->sw, r[l][k], t->dir, &px, &py, l);
                    set_motion(p, t->x + sx, t->y + sy, t->sw, t->sh, px + dx, py + dy, l);
                }
        }
    return 0;
}

/* ---------------------------------------------------------------- macroblocks ------------ */
/* What follows the prediction syntax in every macroblock but I_PCM: coded_block_pattern (Intra16x16 carries it in its type),
 * mb_qp_delta, residual (decoder/macroblock.c:540-587), then the levels and the QP into the record */
/* t8_ok: the macroblock's prediction lets transform_size_8x8_flag follow the pattern (7.3.5): inter, no sub-macroblock partition
 * below 8x8, direct-predicted quadrants (or B_Direct_16x16) only under direct_8x8_inference_flag */
static int parse_mb_tail(p264parse *p, bitrd_t *b, p264hip_mb_t *m, int t8_ok)
{
    mbcoef_t cf; cf.mask = 0;
    if (m->mb_type != P264_MB_I16x16) {
        const int c = rd_cbp(p, b, m->mb_type == P264_MB_I4x4);
        if (c < 0) { ERR(p, "invalid cbp"); return -1; }
        m->cbp = (uint8_t)c;
        if ((c & 15) && p->t8x8_mode && t8_ok && rd_t8x8_flag(p, b)) m->intra_modes |= P264_MB_T8X8;
    }
    int qp = p->sh.qp, has_res = (m->cbp != 0 || m->mb_type == P264_MB_I16x16);
    if (has_res) {
        int dqp = rd_mb_qp_delta(p, b);
        if (dqp < -52 || dqp > 52) { ERR(p, "mb_qp_delta out of range"); return -1; }
        if (p->strict_qp) qp = (p->qp_pred + dqp + 52) % 52;
        else qp = p->sh.qp + dqp;                 /* delta is NOT accumulated: decoder/macroblock.c:568 */
        if (rd_residual(p, b, m, &cf) < 0) { ERR(p, "read residual data failed"); return -1; }
    } else { memset(p->nnz + (size_t)p->mbi * 24, 0, 24); p->last_dqp = 0; }
    if (store_coefs(p, m, &cf) < 0) return -1;
    finish_mb_qp(p, m, has_res, qp);
    if (br_overrun(b)) { ERR(p, "macroblock overruns the slice data"); return -1; }
    return 0;
}

/* t: mb_type as read (P slices), intra_t >= 0: the macroblock is intra with that I-slice type (I slices; P / B slices after
 * their offset of 5 / 23) */
static int parse_mb_t(p264parse *p, bitrd_t *b, unsigned t, int intra_t)
{
    picbuf_t *q = &p->buf[p->cur];
    p264hip_mb_t *m = &q->mb[p->mbi];
    begin_mb(p, m);
    uint8_t *i4 = q->i4 + p->mbi * 16;
    int t8_ok = intra_t < 0;

    if (intra_t >= 0) {
        /* ---- intra (decoder/macroblock.c:117-139, 265-301) ---- */
        if (intra_t > 25) { ERR(p, "invalid mb type %d", intra_t); return -1; }
        m->avail = (uint8_t)intra_avail(p);
        if (intra_t == 25) return parse_ipcm(p, b, m);
        clear_motion(p);
        if (intra_t == 0) {
            m->mb_type = P264_MB_I4x4;
            /* I_NxN: transform_size_8x8_flag comes in front of the prediction modes; 1 = Intra 8x8 prediction, which only a backend that
             * knows P264_MB_I8X8 does (P264PARSE_OPT_INTRA8X8) */
            if (p->t8x8_mode && rd_t8x8_flag(p, b)) {
                if (!(p->opts & P264PARSE_OPT_INTRA8X8)) { ERR(p, "Intra 8x8 prediction unsupported"); return -1; }
                /* four prev_intra8x8_pred_mode_flag / rem_intra8x8_pred_mode pairs: the 4x4 elements' code and contexts (7.3.5.1) */
                m->intra_modes = P264_MB_I8X8;
                p->pic.i8x8 = 1;
                for (int k = 0; k < 4; k++) memset(i4 + 4 * k, rd_intra4x4_mode(p, b, predict_i8mode(p, k)), 4);
            } else
            for (int i = 0; i < 16; i++) i4[i] = (uint8_t)rd_intra4x4_mode(p, b, predict_i4mode(p, i));
        } else {
            m->mb_type = P264_MB_I16x16;
            m->intra_modes = (uint8_t)((intra_t - 1) & 3);
            m->cbp = (uint8_t)((((intra_t - 1) >> 2) % 3) << 4 | (intra_t > 12 ? 15 : 0));
            memset(i4, 2, 16);
        }
        unsigned cm = rd_chroma_pred_mode(p, b);
        if (cm > 3) { ERR(p, "invalid intra chroma pred mode %u", cm); return -1; }
        m->intra_modes |= (uint8_t)(cm << 4);
    } else {
        /* ---- inter: P_L0_16x16, P_L0_L0_16x8, P_L0_L0_8x16, P_8x8, P_8x8ref0 ---- */
        static const uint8_t all_l0[2] = { PRED_L0, PRED_L0 };
        static const uint8_t sub_w[4] = { 2, 2, 1, 1 }, sub_h[4] = { 2, 1, 2, 1 };    /* sub_mb_type 8x8, 8x4, 4x8, 4x4 in 4x4 units */
        memset(i4, 2, 16);
        part_t pt[4];
        int np = 4;
        if (t <= 2) {
            m->mb_type = P264_MB_P_L0;
            np = mb_partitions(pt, (int)t, all_l0);
        } else {
            m->mb_type = P264_MB_P_8x8;
            for (int k = 0; k < 4; k++) {
                const int sub = rd_sub_mb_type(p, b);
                if (sub < 0 || sub > 3) { ERR(p, "invalid i_sub_partition"); return -1; }   /* (< 0: a ue(v) past 2^31 in a damaged stream) */
                sub_partition(pt, k, sub_w[sub], sub_h[sub], PRED_L0);
                t8_ok &= sub == 0;
            }
        }
        if (parse_inter_pred(p, b, 1, np, pt, t != 4, NULL) < 0) return -1;
    }
    return parse_mb_tail(p, b, m, t8_ok);
}

/* table 7-14, mb_type 4..21: (type - 4) >> 1 -> prediction of the two partitions (even types 16x8, odd types 8x16) */
static const uint8_t b_pair[9][2] = {
    { PRED_L0, PRED_L0 }, { PRED_L1, PRED_L1 }, { PRED_L0, PRED_L1 }, { PRED_L1, PRED_L0 }, { PRED_L0, PRED_BI },
    { PRED_L1, PRED_BI }, { PRED_BI, PRED_L0 }, { PRED_BI, PRED_L1 }, { PRED_BI, PRED_BI } };
static const uint8_t b_sub_pred[13] = { 0, PRED_L0, PRED_L1, PRED_BI, PRED_L0, PRED_L0, PRED_L1, PRED_L1, PRED_BI, PRED_BI, PRED_L0, PRED_L1, PRED_BI };   /* table 7-18; 0 = direct */
static const uint8_t b_sub_w[13] = { 2, 2, 2, 2, 2, 1, 2, 1, 2, 1, 1, 1, 1 }, b_sub_h[13] = { 2, 2, 2, 2, 1, 2, 1, 2, 1, 2, 1, 1, 1 };    /* sub-partition size in 4x4 units */

static int parse_mb_b_t(p264parse *p, bitrd_t *b, unsigned t)
{
    picbuf_t *q = &p->buf[p->cur];
    p264hip_mb_t *m = &q->mb[p->mbi];
    if (t >= 23) {                                            /* intra macroblock in a B slice: the I-slice syntax with the type offset */
        return parse_mb_t(p, b, t, (int)t - 23);
    }
    begin_mb(p, m);
    m->mb_type = P264_MB_B;
    memset(q->i4 + p->mbi * 16, 2, 16);
    clear_motion(p);
    int t8_ok = 1;
    const int inf8 = p->sps[p->active_sps].direct_8x8_inference;
    if (t == 0) { store_direct_mb(p); t8_ok = inf8; }         /* B_Direct_16x16: like B_Skip, with a residual */
    else {
        part_t pt[4];
        direct_t d;
        int np = 4;
        if (t <= 3) {                                         /* B_L0_16x16, B_L1_16x16, B_Bi_16x16 */
            const uint8_t pred = t == 1 ? PRED_L0 : t == 2 ? PRED_L1 : PRED_BI;
            np = mb_partitions(pt, 0, &pred);
        } else if (t <= 21) np = mb_partitions(pt, (t & 1) ? 2 : 1, b_pair[(t - 4) >> 1]);
        else {                                                /* 22: B_8x8 */
            int any_direct = 0;
            for (int k = 0; k < 4; k++) {
                const int sub = rd_sub_mb_type(p, b);
                if (sub < 0 || sub > 12) { ERR(p, "invalid B sub_mb_type %d", sub); return -1; }   /* (< 0: as above; found by tests/tools/asan_slices.sh) */
                sub_partition(pt, k, b_sub_w[sub], b_sub_h[sub], b_sub_pred[sub]);
                any_direct |= sub == 0;
                t8_ok &= sub == 0 ? inf8 : sub <= 3;
                if (p->cabac_on && sub == 0) p->cinfo[p->mbi] |= CI_D8(k);
            }
            if (any_direct) direct_predict(p, &d);            /* from the macroblock's neighbours, before any of its own motion exists */
        }
        if (parse_inter_pred(p, b, 2, np, pt, 1, &d) < 0) return -1;
    }
    return parse_mb_tail(p, b, m, t8_ok);
}

/* one non-skipped macroblock of the current slice, whatever its slice type and entropy coder */
static int parse_mb(p264parse *p, bitrd_t *b)
{
    const int ti = p->cabac_on ? cb_mb_type(p) : (int)br_ue(b);
    if (ti < 0) return -1;
    const unsigned t = (unsigned)ti;
    if (p->sh.type == P264_SLICE_B) return parse_mb_b_t(p, b, t);
    int intra_t = -1;
    if (p->sh.type == P264_SLICE_I) intra_t = (int)t;
    else if (t >= 5) intra_t = (int)t - 5;
    return parse_mb_t(p, b, t, intra_t);
}

/* position of the rbsp_stop_one_bit, in bits from the start of the payload */
static long rbsp_stop_bit(const uint8_t *buf, int size)
{
    int n = size;
    while (n > 0 && buf[n-1] == 0) n--;
    if (n == 0) return 0;
    int tz = 0; while (!((buf[n-1] >> tz) & 1)) tz++;
    return (long)n * 8 - 1 - tz;
}

/* ---------------------------------------------------------------- slice ------------------ */
/* List X of the slice that starts (p->list[X], with the slice's weights in p->sh.wp_tab) onto the picture's canonical list:
 * the first P / B slice's list IS the canonical list, verbatim, with its length and its duplicates.  Every entry i of a later slice
 * maps to canonical entry i where that one names the same frame (slices that agree keep their indices: such a picture is what it
 * was with one list per picture), else to the first canonical entry with the same frame - and, under explicit weights, the same
 * (weight, offset) for Y, Cb and Cr; without a match the entry is appended, with its weights.  More than P264HIP_MAX_REFS entries
 * are refused (without explicit weights that cannot happen: at most 16 frames, and an entry is only appended for a new frame). */
static int map_slice_list(p264parse *p, int X)
{
    const int *loc = p->list[X], n_loc = p->n_list[X];
    int *can = p->pic.list[X], *n_can = &p->pic.n_list[X];
    const int wp = p->pic.wp;
    p->ref_map_used[X] = 0;
    if (*n_can == 0) {
        memcpy(can, loc, sizeof(int) * (size_t)n_loc); *n_can = n_loc;
        for (int i = 0; i < P264HIP_MAX_REFS; i++) p->ref_map[X][i] = (int8_t)i;
        return 0;
    }
    for (int i = 0; i < n_loc; i++) {
        int j = -1;
#define SAME_ENTRY(k) (can[k] == loc[i] && (!wp || !memcmp(p->pic.wp_tab[X][k], p->sh.wp_tab[X][i], sizeof p->sh.wp_tab[X][i])))
        if (i < *n_can && SAME_ENTRY(i)) j = i;
        for (int k = 0; k < *n_can && j < 0; k++) if (SAME_ENTRY(k)) j = k;
#undef SAME_ENTRY
        if (j < 0) {
            if (*n_can >= P264HIP_MAX_REFS) { ERR(p, "the slices of the picture need more than %d entries in reference list %d", P264HIP_MAX_REFS, X); return -1; }
            j = (*n_can)++;
            can[j] = loc[i];
            if (wp) memcpy(p->pic.wp_tab[X][j], p->sh.wp_tab[X][i], sizeof p->sh.wp_tab[X][i]);
        }
        p->ref_map[X][i] = (int8_t)j;
        if (j != i) p->ref_map_used[X] = 1;
    }
    for (int i = n_loc; i < P264HIP_MAX_REFS; i++) p->ref_map[X][i] = p->ref_map[X][0];     /* (past the list = entry 0) */
    return 0;
}

/* The slice [first, end) is parsed.  What outlives it must not name its own list indices:
 * - the motion of a reference picture, kept for the direct prediction of later B pictures (8.4.1.2): per 8x8 the PICTURE the
 *   index meant (uid) - through the slice's own lists, here, while they are at hand - and the index as the slice coded it, which is
 *   what colZeroFlag asks about (8.4.1.2.2: refIdxCol is 0);
 * - ref_idx[] / ref_idx_l1[] of its macroblocks: rewritten to the picture's canonical indices (negative ones stay). */
static void end_slice(p264parse *p, int first, int end)
{
    picbuf_t *q = &p->buf[p->cur];
    const int isB = p->sh.type == P264_SLICE_B;
    if (p->pic.ref_idc && p->has_col) {
        int16_t *cm = p->col_mv[p->cur_slot]; int8_t *cr = p->col_ref[p->cur_slot]; int32_t *cu = p->col_uid[p->cur_slot];
        for (int i = first * 4; i < end * 4; i++) {
            const int r0 = q->ref[0][i], r1 = isB ? q->ref[1][i] : -1;
            const int mbi = i >> 2, q8 = i & 3, b0 = (q8 >> 1) * 8 + (q8 & 1) * 2;
            const int l = r0 >= 0 || r1 < 0 ? 0 : 1;                                          /* the list-0 motion if there is one, else list 1 */
            const int16_t *src = q->mv[l];
            const int r = r0 >= 0 ? r0 : r1;
            cr[i] = (int8_t)r;
            cu[i] = r < 0 ? -1 : (int32_t)p->dpb[p->list[l][r < p->n_list[l] ? r : 0]].uid;
            for (int k = 0; k < 4; k++) {
                const int blk = b0 + (k >> 1) * 4 + (k & 1);
                cm[(mbi * 16 + blk) * 2] = r < 0 ? 0 : src[(mbi * 16 + blk) * 2]; cm[(mbi * 16 + blk) * 2 + 1] = r < 0 ? 0 : src[(mbi * 16 + blk) * 2 + 1];
            }
        }
    }
    if (p->sh.type == P264_SLICE_I) return;
    for (int X = 0; X < (isB ? 2 : 1); X++) {
        if (!p->ref_map_used[X]) continue;
        int8_t *ref = q->ref[X];
        for (int i = first * 4; i < end * 4; i++) if (ref[i] >= 0) ref[i] = p->ref_map[X][ref[i] & (P264HIP_MAX_REFS - 1)];
    }
}

/* the picture as the device gets it: the canonical lists and weights */
static void publish_picture(p264parse *p)
{
    picbuf_t *q = &p->buf[p->cur];
    p264hip_picture_t *d = &p->desc[p->cur];
    const pps_t *pps = &p->pps[p->active_pps];
    const curpic_t *c = &p->pic;
    memset(d, 0, sizeof *d);
    d->mb_w = p->mb_w; d->mb_h = p->mb_h;
    d->slice_type = c->type;
    d->chroma_qp_offset = pps->chroma_qp_offset;
    /* Cr's own offset as a delta on it, from the same PPS; the extension counts under a High SPS only (open_slice) */
    if ((p->opts & P264PARSE_OPT_CR_OFFSET) && p->sps[pps->sps_id].high && pps->ext) d->cr_qp_offset_delta = pps->second_chroma_qp_offset - pps->chroma_qp_offset;
    d->deblock = (!pps->deblock_ctrl || c->deblock) ? 1 : 0;         /* per-macroblock `edges` gate the slices that switch it off */
    d->alpha_c0_offset = c->alpha; d->beta_offset = c->beta;
    d->dst_slot = p->cur_slot;
    d->n_ref = c->n_list[0];
    for (int i = 0; i < c->n_list[0]; i++) d->ref_slot[i] = c->list[0][i];
    d->n_coef_blocks = (uint32_t)q->coef_n;
    d->frame_num = (uint32_t)c->first.frame_num;
    d->mb = q->mb; d->mv = q->mv[0]; d->ref_idx = q->ref[0]; d->i4modes = q->i4; d->coefs = q->coef;
    if (c->type == P264_SLICE_B) {
        d->mv_l1 = q->mv[1]; d->ref_idx_l1 = q->ref[1];
        d->n_ref_l1 = c->n_list[1];
        for (int i = 0; i < c->n_list[1]; i++) d->ref_slot_l1[i] = c->list[1][i];
        d->weighted_bipred = c->weighted_bipred;
        memcpy(d->bipred_weight, c->bipred_weight, sizeof d->bipred_weight);
    }
    d->transform_8x8 = c->t8x8 | (c->i8x8 ? P264_T8X8_INTRA : 0);
    if (c->cqm) {
        d->scaling_lists = 1;
        memcpy(d->scaling4x4, c->lists.l4, sizeof d->scaling4x4); memcpy(d->scaling8x8, c->lists.l8, sizeof d->scaling8x8);
    }
    if (c->wp_set && c->wp) {
        d->explicit_wp = 1;
        d->wp_log2_denom[0] = c->wp_denom[0]; d->wp_log2_denom[1] = c->wp_denom[1];
        memcpy(d->wp, c->wp_tab, sizeof d->wp);
    }
}

/* The steps of decode_slice return 0 or one of these.  A refused slice leaves the picture open: the next slice may still continue
 * it (DESIGN.md section 7 lists these exits; some of them leave state of the refused slice behind). */
enum { REFUSE_SLICE = -1, ABANDON_PICTURE = -2 };

/* Step 1: the slice header (> 0: a slice to ignore), and the parameter sets it names made the active ones.  A new context
 * (buffers, frame store) only when the picture geometry or the frame-store size changes; switching between parameter sets of the
 * same geometry just activates them (H.264 7.4.1.2.1: the frame store lives on.  The reference loops forever in its context
 * switch here, decoder/decoder.c:380-396, so there is nothing to match). */
static int slice_header_and_context(p264parse *p, bitrd_t *b, int nal_type, int nal_ref_idc, slice_t *sh)
{
    const int rc = parse_slice_header(p, b, nal_type, nal_ref_idc, sh);
    if (rc < 0) { ERR(p, "slice header decode failed"); return REFUSE_SLICE; }
    if (rc > 0) return rc;
    const pps_t *pps = &p->pps[sh->pps_id];
    const sps_t *sps = &p->sps[pps->sps_id];
    const int slots = sps_slots(p, sps);
    if (p->active_sps < 0 || !p->buf[0].mb || sps->mb_w != p->mb_w || sps->mb_h != p->mb_h || slots != p->slots) {
        if (init_context(p, pps->sps_id, sh->pps_id) < 0) { ERR(p, "out of memory"); return REFUSE_SLICE; }
    } else { p->active_sps = pps->sps_id; p->active_pps = sh->pps_id; }
    if (p->out_on) p->reorder = p->out_depth >= 0 ? p->out_depth : sps_reorder_depth(sps);
    return 0;
}

/* Step 2: the slice opens a new picture (decoder/decoder.c:502-593) or continues the open one */
static int open_picture(p264parse *p, const slice_t *sh, int nal_type, int nal_ref_idc)
{
    curpic_t *c = &p->pic;
    if (sh->first_mb != 0 && c->open) {
        if (sh->first_mb != c->next_mb) { ERR(p, "slice starts at MB %d, expected %d", sh->first_mb, c->next_mb); return REFUSE_SLICE; }
        c->slice_no++;
        return 0;
    }
    if (sh->first_mb != 0) { ERR(p, "slice starts at MB %d but no picture is open", sh->first_mb); return REFUSE_SLICE; }
    c->open = 1; c->next_mb = 0; c->slice_no = 0;
    c->is_idr = nal_type == NAL_SLICE_IDR; c->ref_idc = nal_ref_idc;
    if (c->is_idr) {                              /* p264_slice_idr, decoder/decoder.c:43-64 */
        for (int i = 0; i < p->slots; i++) p->dpb[i].used = 0;
        if (!p->out_on) p->cur_slot = 0;          /* (output order: pictures from before may still wait, slot 0 among them - cur_slot is free) */
    }
    c->first = *sh;
    c->type = sh->type;
    c->deblock = 0; c->alpha = c->beta = 0;
    c->n_list[0] = c->n_list[1] = 0; c->wp_set = 0; c->t8x8 = 0; c->i8x8 = 0;
    p->n_list[0] = p->n_list[1] = 0;
    p->buf[p->cur].coef_n = 0;
    memset(p->slice_of, 0xff, (size_t)p->n_mb * sizeof(uint16_t));
    c->poc = picture_order_count(p, sh, c->is_idr, nal_ref_idc);
    c->uid = ++p->next_uid;
    if (p->buf[p->cur].ref[1]) memset(p->buf[p->cur].ref[1], -1, (size_t)p->n_mb * 4);   /* nothing predicts from list 1 until a B macroblock says so */
    return 0;
}

/* Step 3: what the macroblocks of the slice are parsed with - the filter deltas, its lists mapped onto the picture's, the QP chain */
static int open_slice(p264parse *p, const slice_t *sh)
{
    curpic_t *c = &p->pic;
    const pps_t *pps = &p->pps[sh->pps_id];
    if (sh->disable_deblock != 1 && !c->deblock) {        /* the filter parameters are per picture on the device */
        c->deblock = 1; c->alpha = sh->alpha_off; c->beta = sh->beta_off;
    }
    /* the device adds every macroblock's deltas to the picture's offsets: this slice's minus those of the first slice that filters */
    /* the PPS extension counts under a High SPS (decided here, where the pair is known, not where the PPS was parsed) */
    p->t8x8_mode = 0;
    if (p->sps[pps->sps_id].high && pps->ext) {
        if (pps->scaling_matrix && !pps->cqm_read) { ERR(p, "pic_scaling_matrix_present_flag unsupported (flat scaling lists only)"); return REFUSE_SLICE; }
        if (pps->ext_short) { ERR(p, "PPS %d: its extension ends inside the scaling matrix", sh->pps_id); return REFUSE_SLICE; }
        if (pps->second_chroma_qp_offset != pps->chroma_qp_offset && !(p->opts & P264PARSE_OPT_CR_OFFSET)) {      /* (with the option: publish_picture hands the difference out) */
            ERR(p, "second_chroma_qp_index_offset %d differs from chroma_qp_index_offset %d: unsupported", pps->second_chroma_qp_offset, pps->chroma_qp_offset);
            return REFUSE_SLICE;
        }
        if (pps->second_chroma_qp_offset != pps->chroma_qp_offset && (pps->second_chroma_qp_offset < -12 || pps->second_chroma_qp_offset > 12)) {   /* (7.4.2.2) */
            ERR(p, "second_chroma_qp_index_offset %d out of range (-12 .. 12)", pps->second_chroma_qp_offset); return REFUSE_SLICE;
        }
        p->t8x8_mode = pps->t8x8_mode;
        c->t8x8 |= pps->t8x8_mode;
    }
    {
        /* the picture's scaling lists (table 7-2): the PPS's - resolved against the SPS's where it has a matrix (rule B), against the
         * defaults where not (rule A) -, else the SPS's, else flat.  One table per picture on the device, like the weights: the first
         * slice's, every other one must resolve to the same.  (Lists that spell out weight 16 everywhere: a flat picture.) */
        const sps_t *sps = &p->sps[pps->sps_id];
        cqm_t now;
        int cqm = 0;
        if (sps->high && pps->ext && pps->scaling_matrix) { cqm_resolve(pps->cqm, 6 + 2 * pps->t8x8_mode, sps->cqm ? &sps->lists : NULL, &now); cqm = 1; }
        else if (sps->high && sps->cqm) { now = sps->lists; cqm = 1; }
        if (cqm && cqm_is_flat(&now)) cqm = 0;
        if (c->slice_no == 0) { c->cqm = cqm; if (cqm) c->lists = now; }
        else if (cqm != c->cqm || (cqm && memcmp(&now, &c->lists, sizeof now))) {
            ERR(p, "slices of one picture with different scaling lists unsupported"); return REFUSE_SLICE;
        }
    }
    p->slice_flags = sh->disable_deblock == 1 ? 0 : (uint16_t)(((sh->alpha_off - c->alpha) & 255) | ((sh->beta_off - c->beta) & 255) << 8);
    p->sh = *sh;
    if (sh->type == P264_SLICE_P || sh->type == P264_SLICE_B) {
        /* the slice's own lists; reference indices are resolved through ONE list 0 (and one list 1) per picture on the device: the
         * canonical lists, onto which the slice's are mapped below */
        const int n_lists = sh->type == P264_SLICE_B ? 2 : 1;
        for (int X = 0; X < n_lists; X++) {
            if (X == 1 && !p->has_col) { ERR(p, "B slice without list-1 storage (Baseline parameter set)"); return REFUSE_SLICE; }
            if ((p->n_list[X] = build_list(p, sh, X, p->list[X])) < 0) { p->n_list[X] = 0; return REFUSE_SLICE; }
        }
        /* a picture with any B slice is reconstructed as B, one with any P slice as P */
        if (c->type != P264_SLICE_I && c->type != sh->type) { ERR(p, "P and B slices in one picture unsupported"); return REFUSE_SLICE; }
        c->type = sh->type;
        if (sh->type == P264_SLICE_B) c->weighted_bipred = pps->weighted_bipred == 2;    /* (the weights themselves: on the canonical lists, when the picture is complete) */
        /* explicit weights: ONE table per picture on the device (like the lists); the first P / B slice's, every other one must match */
        if (!c->wp_set) {
            c->wp_set = 1;
            c->wp = sh->wp; c->wp_denom[0] = sh->wp_denom[0]; c->wp_denom[1] = sh->wp_denom[1];
            memcpy(c->wp_tab, sh->wp_tab, sizeof c->wp_tab); memcpy(c->wp_coded, sh->wp_tab, sizeof c->wp_coded);
        } else if (sh->wp != c->wp || (sh->wp && (sh->wp_denom[0] != c->wp_denom[0] || sh->wp_denom[1] != c->wp_denom[1]
                                                   || memcmp(sh->wp_tab, c->wp_coded, sizeof sh->wp_tab)))) {
            ERR(p, "slices of one picture with different weight tables unsupported"); return REFUSE_SLICE;
        }
        for (int X = 0; X < n_lists; X++) if (map_slice_list(p, X) < 0) return ABANDON_PICTURE;
    }
    p->qp_pred = sh->qp;
    /* The reference's QP bookkeeping (delta added to the slice QP, last QP carried over residual-free macroblocks and across
     * pictures: SURVEY A-Q2) is kept for what the reference decodes - Baseline CAVLC I / P slices.  It decodes neither CABAC nor
     * B slices nor any other profile: there is no behaviour to match there, those streams get the standard's chain. */
    p->strict_qp = (p->opts & P264PARSE_OPT_STRICT) || pps->cabac || p->sps[pps->sps_id].profile_idc != 66 || sh->type == P264_SLICE_B;
    p->cabac_on = pps->cabac;
    p->last_dqp = 0;
    return 0;
}

/* Step 4, CAVLC: slice_data( ) (7.3.4) with mb_skip_run (decoder/decoder.c:598-664) */
static int slice_data_cavlc(p264parse *p, bitrd_t *b, const uint8_t *payload, int size)
{
    const int type = p->sh.type;
    const long stop = rbsp_stop_bit(payload, size);
    p->skip_run = -1;
    while (p->pic.next_mb < p->n_mb) {
        p->mbi = p->pic.next_mb; p->mbx = p->mbi % p->mb_w; p->mby = p->mbi / p->mb_w;
        if (p->skip_run <= 0 && (long)br_consumed(b) >= stop) break;    /* !more_rbsp_data(): the slice ends here */
        if (type != P264_SLICE_I && p->skip_run < 0) {
            p->skip_run = (int)br_ue(b);
            if (p->skip_run > p->n_mb - p->pic.next_mb) { ERR(p, "mb_skip_run %d runs past the picture", p->skip_run); return ABANDON_PICTURE; }
        }
        if (p->skip_run > 0) {
            decode_skip(p);
            p->skip_run--;
        } else {
            if ((long)br_consumed(b) >= stop) break;
            if (parse_mb(p, b) < 0) { ERR(p, "macroblock read failed [%d,%d]", p->mbx, p->mby); return ABANDON_PICTURE; }
            p->skip_run = -1;
        }
        p->slice_of[p->mbi] = (uint16_t)p->pic.slice_no;
        p->pic.next_mb++;
    }
    return 0;
}

/* Step 4, CABAC: slice_data( ) (7.3.4): alignment bits, the engine started on the next byte, contexts from the slice QP; per
 * macroblock mb_skip_flag (P / B), the macroblock, end_of_slice_flag */
static int slice_data_cabac(p264parse *p, bitrd_t *b, const uint8_t *payload, int size)
{
    const int type = p->sh.type;
    if (!p->cinfo) { ERR(p, "CABAC slice without its context storage (Baseline parameter set)"); return REFUSE_SLICE; }
    const size_t at = (size_t)((br_consumed(b) + 7) >> 3);
    if (at >= (size_t)size) { ERR(p, "CABAC slice without data"); return REFUSE_SLICE; }
    p264cabac_init_contexts(&p->cb, type == P264_SLICE_I, p->sh.cabac_init_idc, p->sh.qp);
    p264cabac_start(&p->cb, payload + at, (size_t)size - at);
    for (;;) {
        if (p->pic.next_mb >= p->n_mb) { ERR(p, "slice data runs past the picture"); return ABANDON_PICTURE; }
        p->mbi = p->pic.next_mb; p->mbx = p->mbi % p->mb_w; p->mby = p->mbi / p->mb_w;
        /* (the neighbour flags of the macroblock are needed before its first bin: begin_mb computes them again, identically) */
        mb_neighbours(p);
        if (type != P264_SLICE_I && cb_mb_skip_flag(p)) decode_skip(p);
        else if (parse_mb(p, b) < 0) { ERR(p, "macroblock read failed [%d,%d]", p->mbx, p->mby); return ABANDON_PICTURE; }
        if (p264cabac_bits_left(&p->cb) < -64) { ERR(p, "CABAC data overrun"); return ABANDON_PICTURE; }
        p->slice_of[p->mbi] = (uint16_t)p->pic.slice_no;
        p->pic.next_mb++;
        if (p264cabac_terminate(&p->cb)) break;                  /* end_of_slice_flag */
    }
    return 0;
}

/* Step 6: every macroblock of the picture is there */
static int close_picture(p264parse *p, const p264hip_picture_t **pic)
{
    curpic_t *c = &p->pic;
    if (c->type == P264_SLICE_B) implicit_weights(p);         /* a function of the picture pair: per canonical pair */
    if (c->type == P264_SLICE_B && c->wp_set && c->wp && bipred_sums_bad(p)) return ABANDON_PICTURE;
    publish_picture(p);
    *pic = &p->desc[p->cur];
    finish_picture_marking(p);
    p->cur ^= 1;
    c->open = 0;
    return 0;
}

/* One slice NAL: 1 = it completed a picture, 0 = it did not, -1 = refused.  Which refusals also abandon the open picture is
 * decided here and nowhere else. */
static int decode_slice(p264parse *p, int nal_type, int nal_ref_idc, const uint8_t *payload, int size,
                        const p264hip_picture_t **pic)
{
    bitrd_t b; br_init(&b, payload, (size_t)size);
    slice_t sh;
    int rc = slice_header_and_context(p, &b, nal_type, nal_ref_idc, &sh);
    if (rc > 0) return 0;                                     /* redundant picture: ignore the slice */
    if (rc == 0) rc = open_picture(p, &sh, nal_type, nal_ref_idc);
    if (rc == 0) rc = open_slice(p, &sh);
    if (rc == 0) rc = p->cabac_on ? slice_data_cabac(p, &b, payload, size) : slice_data_cavlc(p, &b, payload, size);
    if (rc == 0) {
        end_slice(p, sh.first_mb, p->pic.next_mb);
        if (p->pic.next_mb < p->n_mb) return 0;               /* wait for the next slice of this picture */
        rc = close_picture(p, pic);
    }
    if (rc == ABANDON_PICTURE) p->pic.open = 0;
    return rc < 0 ? -1 : 1;
}

/* ---------------------------------------------------------------- public ---------------- */
p264parse *p264parse_open(int options)
{
    if (p264amd_cpu_refuse("p264parse_open")) return NULL;     /* (cpu_check.c: the host objects are built for x86-64-v3) */
    if (cavlc_global_init() != 0) { fprintf(stderr, "p264amd: CAVLC tables are not prefix-free\n"); return NULL; }
    p264parse *p = (p264parse *)calloc(1, sizeof *p);
    if (!p) return NULL;
    p->opts = options;
    p->active_sps = p->active_pps = -1;
    return p;
}

void p264parse_set_allocator(p264parse *p, void *(*alloc)(size_t bytes), void (*release)(void *ptr))
{
    if (!p || p->n_mb) return;                              /* only before the first context is built */
    p->alloc = alloc; p->release = release;
}

int p264parse_set_output_order(p264parse *p, int on, int reorder_depth)
{
    if (!p || p->n_mb || reorder_depth > P264HIP_MAX_REFS) return -1;      /* only before the first context is built */
    p->out_on = on != 0; p->out_depth = reorder_depth < 0 ? -1 : reorder_depth;
    return 0;
}

int p264parse_outputs(const p264parse *p, p264parse_output_t *out, int max)
{
    if (!p || !p->out_on || (max > 0 && !out)) return 0;
    for (int i = 0; i < p->n_outs && i < max; i++) out[i] = p->outs[i];
    return p->n_outs;
}

int p264parse_flush(p264parse *p, p264parse_output_t *out, int max)
{
    if (!p || !p->out_on || (max > 0 && !out)) return 0;
    p->n_outs = 0;
    for (int i; (i = wait_first(p->wait, p->slots)) >= 0; ) wait_emit(p->wait, i, p->outs, &p->n_outs);
    return p264parse_outputs(p, out, max);
}

void p264parse_close(p264parse *p)
{
    if (!p) return;
    free_context(p, 1);
    free(p);
}

int p264parse_nal(p264parse *p, int nal_type, int nal_ref_idc, const uint8_t *payload, int size,
                  const p264hip_picture_t **pic)
{
    if (pic) *pic = NULL;
    if (!p || !payload || size < 0 || !pic) return -1;
    bitrd_t b;
    switch (nal_type) {
    case NAL_SPS: br_init(&b, payload, (size_t)size);
        if (parse_sps(p, &b) < 0) { ERR(p, "sps read failed"); return -1; }
        return 0;
    case NAL_PPS: br_init(&b, payload, (size_t)size);
        if (parse_pps(p, &b) < 0) { ERR(p, "pps read failed"); return -1; }
        return 0;
    case NAL_SLICE_IDR:
    case NAL_SLICE:
        return decode_slice(p, nal_type, nal_ref_idc, payload, size, pic);
    case NAL_SLICE_DPA: case NAL_SLICE_DPB: case NAL_SLICE_DPC:
        ERR(p, "partitioned stream unsupported"); return -1;
    default:
        return 0;                                            /* SEI, AUD, ...: ignored (decoder.c:797-799) */
    }
}

int p264parse_mb_width(const p264parse *p)   { return p ? p->mb_w : 0; }
int p264parse_mb_height(const p264parse *p)  { return p ? p->mb_h : 0; }
int p264parse_slots(const p264parse *p)      { return p ? p->slots : 0; }
int p264parse_generation(const p264parse *p) { return p ? p->generation : 0; }

/* the display window of the active SPS (H.264 7.4.2.1.1, 4:2:0 frame macroblocks: CropUnitX = CropUnitY = 2) */
int p264parse_crop(const p264parse *p, int *left, int *top, int *width, int *height)
{
    if (!p || p->active_sps < 0 || !p->mb_w) return -1;
    const sps_t *s = &p->sps[p->active_sps];
    int64_t c[4];
    for (int i = 0; i < 4; i++) c[i] = 2 * (int64_t)(uint32_t)s->crop[i];
    const int64_t w = (int64_t)s->mb_w * 16 - c[0] - c[1], h = (int64_t)s->mb_h * 16 - c[2] - c[3];
    if (w < 1 || h < 1) return -1;                  /* the offsets leave no sample */
    if (left) *left = (int)c[0];
    if (top) *top = (int)c[2];
    if (width) *width = (int)w;
    if (height) *height = (int)h;
    return 0;
}

/* first index >= from with buf[i..i+2] == 00 00 01, or an index with i + 3 > size; the scan hops between zero bytes */
static int64_t annexb_find(const uint8_t *buf, int64_t size, int64_t from)
{
    int64_t i = from;
    while (i + 3 <= size) {
        const uint8_t *z = (const uint8_t *)memchr(buf + i, 0, (size_t)(size - 2 - i));
        if (!z) return size;
        i = z - buf;
        if (buf[i + 1] == 0 && buf[i + 2] == 1) return i;
        i++;
    }
    return size;
}

int p264_annexb_next(const uint8_t *buf, int64_t size, int64_t *pos, int64_t *nal_off, int64_t *nal_len)
{
    int64_t i = annexb_find(buf, size, *pos);
    if (i + 3 > size) { *pos = size; return 0; }
    int64_t start = i + 3, j = annexb_find(buf, size, start);
    int64_t end = j + 3 <= size ? j : size;
    *pos = end;
    while (end > start && buf[end-1] == 0) end--;           /* zeros in front of a start code belong to it */
    *nal_off = start; *nal_len = end - start;
    return 1;
}

/* ---------------------------------------------------------------- known-answer surface ---- */
/* B-picture derivations on hand-made state (tests/test_direct_kat.py drives them with the vectors recorded from the reference's
 * encoder-side functions, tests/golden/kat_direct.npz): the same static functions the macroblock layer calls, on a parser whose
 * picture is 3 x 2 macroblocks with the current one at (1, 1). */
static p264parse *kat_state(void)
{
    p264parse *p = (p264parse *)calloc(1, sizeof *p);
    if (!p) return NULL;
    p->mb_w = 3; p->mb_h = 2; p->n_mb = 6; p->slots = P264HIP_MAX_REFS + 1;
    picbuf_t *q = &p->buf[0];
    for (int l = 0; l < 2; l++) { q->mv[l] = (int16_t *)calloc(6 * 32, sizeof(int16_t)); q->ref[l] = (int8_t *)malloc(6 * 4); }
    for (int i = 0; i <= P264HIP_MAX_REFS; i++) {
        p->col_mv[i] = (int16_t *)calloc(6 * 32, sizeof(int16_t)); p->col_ref[i] = (int8_t *)malloc(6 * 4); p->col_uid[i] = (int32_t *)malloc(6 * 4 * sizeof(int32_t));
    }
    p->has_col = 1; p->active_sps = 0;
    p->mbx = 1; p->mby = 1; p->mbi = 4;
    return p;
}
static void kat_free(p264parse *p)
{
    for (int l = 0; l < 2; l++) { free(p->buf[0].mv[l]); free(p->buf[0].ref[l]); }
    for (int i = 0; i <= P264HIP_MAX_REFS; i++) { free(p->col_mv[i]); free(p->col_ref[i]); free(p->col_uid[i]); }
    free(p);
}
/* lists of a B picture from picture order counts, into list / n_list (the picture's or the slice's: whichever the function under
 * test reads): slot i holds list-0 entry i, slot n0 + k list-1 entry k unless that picture (same order count) already sits in list 0 */
static void kat_lists(p264parse *p, int (*list)[P264HIP_MAX_REFS], int *n_list, int n0, const int *poc0, int n1, const int *poc1, int cur_poc)
{
    int n = 0;
    for (int i = 0; i < n0; i++) { p->dpb[n].used = 1; p->dpb[n].poc = poc0[i]; p->dpb[n].uid = (uint32_t)(poc0[i] + 4096); list[0][i] = n++; }
    for (int k = 0; k < n1; k++) {
        int s = -1;
        for (int i = 0; i < n0; i++) if (poc0[i] == poc1[k]) { s = list[0][i]; break; }
        if (s < 0) { p->dpb[n].used = 1; p->dpb[n].poc = poc1[k]; p->dpb[n].uid = (uint32_t)(poc1[k] + 4096); s = n++; }
        list[1][k] = s;
    }
    n_list[0] = n0; n_list[1] = n1; p->pic.poc = cur_poc;
}

int p264parse_kat_bipred(int n0, const int *poc0, int n1, const int *poc1, int cur_poc, int16_t *weights)
{
    if (n0 < 0 || n1 < 0 || n0 > 8 || n1 > 8) return -1;
    p264parse *p = kat_state();
    if (!p) return -1;
    kat_lists(p, p->pic.list, p->pic.n_list, n0, poc0, n1, poc1, cur_poc);
    p->pic.weighted_bipred = 1;
    implicit_weights(p);
    memcpy(weights, p->pic.bipred_weight, sizeof p->pic.bipred_weight);
    kat_free(p);
    return 0;
}

int p264parse_kat_direct(int spatial, const int8_t *nb_ref, const int16_t *nb_mv, int col_intra, const int8_t *col_ref, const int16_t *col_mv,
                         int n0, const int *poc0, int poc1_0, int cur_poc, int n_col_list, const int *col_list_poc,
                         int8_t *out_ref, int16_t *out_mv)
{
    if (n0 < 1 || n0 > 8 || n_col_list < 0 || n_col_list > 8) return -1;
    p264parse *p = kat_state();
    if (!p) return -1;
    kat_lists(p, p->list, p->n_list, n0, poc0, 1, &poc1_0, cur_poc);
    p->sh.direct_spatial = spatial;
    picbuf_t *q = &p->buf[0];
    memset(q->ref[0], -1, 24); memset(q->ref[1], -1, 24);
    /* neighbours A, B, C, D: the 4x4 block left of / above / above right of / above left of the macroblock's first block */
    static const int nb_mb[4] = { 3, 1, 2, 0 }, nb_quad[4] = { 1, 2, 2, 3 }, nb_sub[4] = { 3, 12, 12, 15 };
    static const int nb_flag[4] = { P264_AVAIL_LEFT, P264_AVAIL_TOP, P264_AVAIL_TOPRIGHT, P264_AVAIL_TOPLEFT };
    p->cur_avail = 0;
    for (int n = 0; n < 4; n++) {
        if (nb_ref[n] != -2) p->cur_avail |= nb_flag[n];        /* (availability is a property of the macroblock: both lists agree) */
        for (int l = 0; l < 2; l++) {
            q->ref[l][nb_mb[n] * 4 + nb_quad[n]] = nb_ref[l * 4 + n] < 0 ? -1 : nb_ref[l * 4 + n];
            int16_t *mv = q->mv[l] + (nb_mb[n] * 16 + nb_sub[n]) * 2;
            mv[0] = nb_mv[(l * 4 + n) * 2]; mv[1] = nb_mv[(l * 4 + n) * 2 + 1];
        }
    }
    /* the co-located macroblock as finish_picture_marking would have left it: the list-0 motion where there is one, else list 1 */
    const int cs = p->list[1][0];
    for (int q8 = 0; q8 < 4; q8++) {
        const int r0 = col_intra ? -1 : col_ref[q8], r1 = col_intra ? -1 : col_ref[4 + q8], r = r0 >= 0 ? r0 : r1;
        p->col_ref[cs][p->mbi * 4 + q8] = (int8_t)r;
        p->col_uid[cs][p->mbi * 4 + q8] = r < 0 || r >= n_col_list ? -1 : col_list_poc[r] + 4096;   /* (list 1 of the co-located picture: not modelled, see the test) */
        for (int k = 0; k < 4; k++) {
            const int blk = (q8 >> 1) * 8 + (q8 & 1) * 2 + (k >> 1) * 4 + (k & 1);
            const int16_t *src = col_mv + ((r0 >= 0 ? 0 : 16) + blk) * 2;
            p->col_mv[cs][(p->mbi * 16 + blk) * 2] = r < 0 ? 0 : src[0]; p->col_mv[cs][(p->mbi * 16 + blk) * 2 + 1] = r < 0 ? 0 : src[1];
        }
    }
    direct_t d;
    direct_predict(p, &d);
    memcpy(out_ref, d.ref, sizeof d.ref); memcpy(out_mv, d.mv, sizeof d.mv);
    kat_free(p);
    return 0;
}

int p264parse_kat_output_order(int depth, int n, const int *poc, const int *flags, int *order, int *due_after)
{
    if (depth < 0 || n < 0 || (n && (!poc || !flags || !order || !due_after))) return -1;
    wait_t *w = (wait_t *)calloc((size_t)n + 1, sizeof *w);
    p264parse_output_t *out = (p264parse_output_t *)malloc(((size_t)n + 1) * sizeof *out);
    if (!w || !out) { free(w); free(out); return -1; }
    int n_wait = 0, done = 0;
    for (int i = 0; i <= n; i++) {                              /* picture i in a slot of its own; i = n: the flush */
        int n_out = 0;
        if (i < n) output_steps(w, n, &n_wait, i, (flags[i] & P264PARSE_OUT_MMCO5) ? 0 : poc[i], i, flags[i], depth, out, &n_out);
        else for (int k; (k = wait_first(w, n)) >= 0; ) wait_emit(w, k, out, &n_out);
        for (int k = 0; k < n_out; k++, done++) { order[done] = out[k].decode_index; due_after[done] = i; }
    }
    free(w); free(out);
    return done == n ? 0 : -1;
}
