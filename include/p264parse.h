/* p264parse.h - C ABI of the host-side bitstream layer.
 *
 * The serial, branchy part of the decoder that stays on the CPU (north star): NAL
 * dispatch, SPS/PPS, slice header, reference-list / frame-store bookkeeping and the
 * CAVLC macroblock-layer parse with MV / intra-mode / nC prediction.  Its product is one
 * p264hip_picture_t per coded picture - exactly the buffers the GPU layer consumes.
 *
 * Stands in for, in the reference: decoder/decoder.c:70-301,368-593,745-806 (NAL switch,
 * slice header, MB loop), decoder/set.c:37-272, decoder/lists.c:72-228,
 * decoder/macroblock.c:72-592, decoder/dec_cavlc.c:1371-1524 and the neighbour cache of
 * core/macroblock.c:40-252,870-1398.
 */
#ifndef P264PARSE_H
#define P264PARSE_H
#include <stdint.h>
#include <stddef.h>
#include "p264hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct p264parse p264parse;

enum {
    P264PARSE_OPT_QUIET  = 1,   /* do not print SPS/PPS/size lines to stderr (the reference prints them) */
    P264PARSE_OPT_INTRA8X8 = 4, /* hand out Intra 8x8 macroblocks (I_NxN with transform_size_8x8_flag 1, High profile) as I4x4 records with
                                   P264_MB_I8X8, in pictures whose descriptor carries P264_T8X8_INTRA (include/p264hip.h).  Off by default:
                                   only the owner of the backend that takes the pictures can say whether it knows the record; without
                                   the option such a macroblock ends the slice with "Intra 8x8 prediction unsupported" */
    P264PARSE_OPT_SCALING = 8,  /* read the scaling matrices of High-profile parameter sets (seq_ / pic_scaling_matrix_present_flag) and hand
                                   out every picture's eight resolved lists in its descriptor (scaling_lists, scaling4x4, scaling8x8:
                                   include/p264hip.h; lists that are 16 everywhere give scaling_lists = 0).  Off by default, for the reason
                                   P264PARSE_OPT_INTRA8X8 is: only the owner of the backend knows whether it reads the table; without the
                                   option such a parameter set is refused ("flat scaling lists only") as it always was */
    P264PARSE_OPT_CR_OFFSET = 16, /* accept a High-profile PPS whose second_chroma_qp_index_offset differs from chroma_qp_index_offset and
                                   hand out the difference as the descriptor's cr_qp_offset_delta (include/p264hip.h), taken from the
                                   PPS that gives chroma_qp_offset.  Off by default, for the same reason: only the owner of the backend
                                   knows whether it reads the delta; without the option the slices of such a PPS are refused
                                   ("second_chroma_qp_index_offset ... unsupported") as they always were */
    P264PARSE_OPT_STRICT = 2    /* H.264-conformant QP accumulation also for Baseline CAVLC streams, where the default is the
                                   reference's rule (decoder/macroblock.c:568, core/macroblock.c:1247-1252; SURVEY A-Q2).
                                   CABAC, B slices and every profile but Baseline - none of which the reference decodes -
                                   always get the conformant chain */
};

p264parse *p264parse_open(int options);
/* Where the arrays of the picture descriptors live (default: malloc/free).  A pipeline passes pinned-memory
 * functions so that the parser writes straight into DMA-able staging.  Call before the first slice NAL. */
void       p264parse_set_allocator(p264parse *p, void *(*alloc)(size_t bytes), void (*release)(void *ptr));
void       p264parse_close(p264parse *p);

/* Feed one NAL unit (header byte already split off, emulation-prevention bytes already
 * removed - see p264_nal_decode).  Returns <0 on error, 0 if no picture was completed,
 * 1 if *pic now describes a complete picture.  The descriptor and its arrays stay valid
 * until the next call that completes a picture. */
int p264parse_nal(p264parse *p, int nal_type, int nal_ref_idc,
                  const uint8_t *payload, int size, const p264hip_picture_t **pic);

/* geometry / frame-store size of the active SPS (0 before the first slice) */
int p264parse_mb_width(const p264parse *p);
int p264parse_mb_height(const p264parse *p);
int p264parse_slots(const p264parse *p);          /* num_ref_frames + 1; with output order on: D + 1 (below) */
/* The display window of the active SPS in luma samples: its frame cropping offsets times 2 in both directions (4:2:0, frame
 * macroblocks only); without cropping the MB-aligned frame.  The parser itself never crops: its pictures, and every frame store
 * behind them, stay MB-aligned - the window is what a caller puts into a p264hip_export_t.  -1 before the first slice, or where
 * the offsets leave no sample. */
int p264parse_crop(const p264parse *p, int *left, int *top, int *width, int *height);
/* bumped every time a new SPS/PPS pair is activated (context re-init, decoder.c:304-343) */
int p264parse_generation(const p264parse *p);

/* ---- pictures in output (display) order: the output process of H.264 C.4, "bumping" (C.4.5.3).  Off by default ----
 * The parser's pictures come in decode order, and without this option a slot of the frame store is reused as soon as it holds no
 * reference.  With it, a completed picture joins the set W of pictures that wait for their output and keeps its slot until it is
 * due: no later picture's dst_slot names a slot that holds a reference or a member of W.
 *
 * Per active SPS: D, the frames the decoded picture buffer holds - max_dec_frame_buffering where the SPS carries a VUI with
 * bitstream_restriction_flag, else MaxDpbFrames = min(MaxDpbMbs(level_idc) / (mb_w * mb_h), 16) of table A-1 (16 for an unknown
 * level_idc), in both cases at least num_ref_frames (and 1) and at most 16; R, the reorder depth - num_reorder_frames of that
 * restriction, else 0 under pic_order_cnt_type 2 (output order is decode order, 8.2.1.3), else D.  A VUI that overruns its NAL
 * unit or holds num_reorder_frames > max_dec_frame_buffering or either above 16 counts as absent; it never refuses the SPS.
 *
 * The rule, applied when picture P is complete:
 *   1. if P is an IDR picture or carried memory_management_control_operation 5, every member of W is due, ascending by order count
 *      (no_output_of_prior_pics_flag is read and ignored: pictures are never discarded);
 *   2. P joins W, with the order count the frame store records for it (0 after operation 5);
 *   3. while |W| > R the member with the smallest order count is due (of equal counts - a broken stream - the one decoded first);
 *   4. while no slot is free of both a reference and a member of W, and W is not empty, the member with the smallest order count
 *      is due; only with W empty the oldest short-term reference is dropped, as without the option;
 *   5. the next picture's slot is chosen among the free ones.
 * A conforming stream's pictures come out with strictly ascending order counts between two flushes (step 1, p264parse_flush).  A
 * stream that is not, or a depth below the stream's real one, gets every picture all the same, exactly once, in the order the
 * rule gives: no error, no drop.
 *
 * A picture due with P may be P itself, and a slot named in P's output list may be the destination of the very next picture.
 * The caller's contract makes that safe: export P's outputs behind P's reconstruct and before the next one, on the same HIP stream.
 *
 * A change of picture size or of the frame-store size (p264parse_generation moves) starts a new frame store: what still waited in
 * the old one is not handed out. */
enum { P264PARSE_OUT_IDR = 1, P264PARSE_OUT_MMCO5 = 2 };     /* p264parse_output_t.flags */
#define P264PARSE_MAX_OUTPUTS (P264HIP_MAX_REFS + 1)        /* the most pictures one call hands out */
typedef struct {
    int slot;            /* of the stream's frame store: where the picture lies */
    int poc;             /* its picture order count, as the frame store records it */
    int decode_index;    /* which of the parser's completed pictures it is, from 0 */
    int flags;           /* P264PARSE_OUT_* */
} p264parse_output_t;
/* on != 0 switches the output process on.  reorder_depth < 0 takes R from the stream; 0 .. 16 overrides it (the caller's low-delay
 * switch: 0 hands every picture out with itself, in decode order).  Only before the first slice NAL, like
 * p264parse_set_allocator; -1 (and nothing changed) later, or for a depth above 16. */
int p264parse_set_output_order(p264parse *p, int on, int reorder_depth);
/* The pictures that became due with the picture just completed, in output order, into out[0 .. max): returns how many there are
 * (at most P264PARSE_MAX_OUTPUTS; 0 with the option off).  The list is valid until the next call that completes a picture. */
int p264parse_outputs(const p264parse *p, p264parse_output_t *out, int max);
/* All of W, ascending by order count, the same way; W is empty afterwards.  For the end of a stream. */
int p264parse_flush(p264parse *p, p264parse_output_t *out, int max);

/* Annex-B helper: find the next NAL unit in buf[*pos..size).  On success returns 1 and sets
 * *nal_off / *nal_len (start code and its leading zeros excluded, like p264decoder.c:259-325);
 * returns 0 at end of buffer. */
int p264_annexb_next(const uint8_t *buf, int64_t size, int64_t *pos, int64_t *nal_off, int64_t *nal_len);

/* The CABAC arithmetic decoding engine of the entropy layer, driven bin by bin (csrc/host/cabac.h; replaces
 * p264_cabac_context_init / _decode_init / _decode_decision / _decode_bypass / _decode_terminal, core/cabac.c:819-902).
 * Contexts are initialised for the slice (9.3.1.1), decoding starts at data[0] (9.3.1.2), then one bin per op:
 * op >= 0: a decision with context op (< 460); -1: a bypass bin; -2: a terminate bin.  bins[i] receives bin i.
 * Returns 0, 1 if the ops read past the end of the data (bins beyond it are then undefined), -1 on a bad argument.
 * This is what the known-answer test of the engine drives; the macroblock-layer binarisations are built on the same
 * inline functions. */
int p264cabac_decode_ops(const uint8_t *data, size_t bytes, int is_i_slice, int cabac_init_idc, int slice_qp,
                         const int16_t *ops, int n_ops, uint8_t *bins);

/* Known-answer surface of the B-picture derivations (the macroblock layer's own static functions, run on hand-made state;
 * tests/test_direct_kat.py drives them with vectors recorded from the reference's encoder-side
 * p264_macroblock_bipred_init / p264_mb_predict_mv_direct16x16, core/macroblock.c:1400-1430, 254-413).
 *
 * p264parse_kat_bipred: implicit weights (H.264 8.4.2.3.1) of every (list-0, list-1) index pair, weights[r0 * 16 + r1] = weight
 * of the list-0 prediction, from the picture order counts of the list entries (n0, n1 <= 8) and of the current picture.
 *
 * p264parse_kat_direct: direct prediction (8.4.1.2) of one macroblock.  nb_ref[l * 4 + n], nb_mv[(l * 4 + n) * 2 + c]: reference
 * index and vector of the macroblock's neighbours n = A (left), B (top), C (top right), D (top left) in list l (-2 = not
 * available, -1 = intra / list unused); col_*: the co-located macroblock of RefPicList1[0] - intra or not, col_ref[l * 4 + q]
 * per 8x8 quadrant, col_mv[(l * 16 + b) * 2 + c] per 4x4 block in raster order; poc0[n0]: order counts of the current list 0,
 * poc1_0 of RefPicList1[0], cur_poc of the current picture; col_list_poc[n_col_list]: order counts of the list 0 the co-located
 * picture was decoded with.  direct_8x8_inference off, no long-term pictures.  out_ref[l * 4 + q], out_mv[(l * 16 + b) * 2 + c].
 * Both return 0, or -1 on a bad argument. */
int p264parse_kat_bipred(int n0, const int *poc0, int n1, const int *poc1, int cur_poc, int16_t *weights);
int p264parse_kat_direct(int spatial, const int8_t *nb_ref, const int16_t *nb_mv, int col_intra, const int8_t *col_ref, const int16_t *col_mv,
                         int n0, const int *poc0, int poc1_0, int cur_poc, int n_col_list, const int *col_list_poc,
                         int8_t *out_ref, int16_t *out_mv);
/* p264parse_kat_output_order: steps 1 - 3 of the output process above (the parser's own static functions; slots without bound, so
 * step 4 never fires) on a hand-made sequence of n pictures in decode order with reorder depth `depth`: poc[i] the order count,
 * flags[i] P264PARSE_OUT_IDR / P264PARSE_OUT_MMCO5 (such a picture counts with order count 0).  order[k] receives the decode index
 * of the k-th picture handed out, due_after[k] the decode index of the picture it became due with, n for those of the final
 * flush; n entries each.  0, or -1 on a bad argument. */
int p264parse_kat_output_order(int depth, int n, const int *poc, const int *flags, int *order, int *due_after);

#ifdef __cplusplus
}
#endif
#endif
