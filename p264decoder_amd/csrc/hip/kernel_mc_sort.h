// kernel_mc_sort.h - the work lists of the motion-compensation stage (kernel_mc.h): keys, layout and entry format, the
// classification of a macroblock, and k_mc_sort*, the counting sort that writes the lists (one workgroup per picture).
#pragma once
#include "device_common.h"
#include "launch_shared.h"           // (the lists' layout and the sort's workgroup size)
#include "wavefront_sync.h"          // (MAX_MB_ROWS: the row field of a list entry)
#include "kernel_scaling.h"          // (ScaleDev: which pictures of the batch k_mc_sort_scaled files without residuals)

// ------------------------------------------------------------------------------------------
// work lists
// ------------------------------------------------------------------------------------------
enum { PC_COPY = 0, PC_H = 1, PC_V = 2, PC_DIAG = 3, PC_C = 4, PC_CH = 5, PC_CV = 6, PC_GEN = 7 };
// PC_GEN | MCY_CLAMP: the 4x4 blocks of the quadrant have different vectors (sub-8x8 partitions), every lane fetches its own
// window.  PC_GEN without MCY_CLAMP: the macroblock belongs to a B picture and predicts from list 1 somewhere: every lane
// looks up which lists its quadrant uses, predicts from each of them like the class above and combines the two
// (p264_mb_mc_1xywh / _01xywh, core/macroblock.c:525-583).
#define MCY_CLAMP   8               // luma key bits: phase class | window not inside the picture | item has coded luma blocks
#define MCY_RESID   16
#define MCC_CLAMP   1               // chroma key bits: window not inside the picture (quadrant items: or vectors differing inside) | residual
#define MCC_RESID   2
#define MCC_BI      4               // | macroblock of a B picture that predicts from list 1 somewhere (quadrant items only)
// (keys per band MCY_KEYS / MCC_KEYS, the lists ML_*, MC_MAX_BANDS, MC_SORT_THREADS, mc_chunk_items, mc_list_keys, mc_entry_words,
// McLayout and mc_layout - the per-picture scratch this sort writes: launch_shared.h, which the launch plan reads too)

// the list entry a reference index names: negative (list unused) or at / past the list's length = entry 0, on every road
// (prediction, implicit and explicit weights; the loop filter's pic_of_init reads the same, include/p264hip.h: ref_idx)
__device__ __forceinline__ int ref_entry(int r, int n) { return (r < 0 || r >= n) ? 0 : r; }
__device__ __forceinline__ int mv_x(int packed) { return (int)(int16_t)(packed & 0xffff); }
__device__ __forceinline__ int mv_y(int packed) { return packed >> 16; }

// phase class of a quarter-pel vector (which of the reference's planes core/mc.c:244-257 combines)
__device__ __forceinline__ int phase_class(int fx, int fy)
{
    if ((fx | fy) == 0) return PC_COPY;
    if (fy == 0) return PC_H;
    if (fx == 0) return PC_V;
    if (fx & fy & 1) return PC_DIAG;
    if (fx == 2) return fy == 2 ? PC_C : PC_CH;
    return PC_CV;
}


// What one inter macroblock contributes to one pass: either one macroblock item per plane kind (one vector, one reference)
// or its four quadrants.  Packed so that a thread can keep the classification of several macroblocks in registers between
// the counting and the scattering pass: key[q] = luma key | chroma key << 16, vec[q] = the entry's vector,
// info = inter | whole << 1 | reference indices (4 bits each) << 8 | list per quadrant << 24 | Z per quadrant << 28.
//
// B pictures take TWO passes (two list sets, two launches of the consumer): a block that predicts from both lists gets its
// list-0 prediction in the first pass (entry with an empty coded-block mask: Z) and the list-1 prediction in the second,
// which reads the first one back, combines the two (core/mc.c:76-155) and adds the residual.  Blocks with one list are
// finished in the first pass, whichever list it is.  In the second pass Z on a quadrant means "not mine": no luma entry,
// and a chroma entry that only carries the quadrant's samples through (the four chroma entries of a macroblock stay
// together: their lanes store whole rows).  Macroblocks of a B picture whose vectors differ inside a quadrant go to the
// generic two-list class, in the first pass, as a whole.
struct McMb { uint32_t info, key[4], vec[4]; };
#define MCMB_INTER 1u
#define MCMB_WHOLE 2u

// ---- list entries: every shift and mask of an entry word is in this block ----
// A first-pass entry is 8 bytes: x = reference index << 28 | flags | macroblock row << 13 | column << 2 | quadrant (low 28
// bits all ones = padding; no division in the consumers), y = the item's vector (packed) - all a wavefront needs to start
// fetching its windows; chunks with residual (a third of them in the bench's pictures) fetch the macroblock's record for QP,
// coded-block mask and place in the coefficient stream, one chunk ahead (round 4 carried the three in every entry: 16 bytes,
// written and read for all chunks, and the sort read the record a second time to fill them in).  Second-pass entries
// (B pictures) stay 16 bytes: z = coded-block mask | QP << 26, w = place in the coefficient stream | weight of the pair of
// references << 23.
enum { MCE_QUAD_BITS = 2, MCE_COL_SHIFT = 2, MCE_COL_BITS = 11, MCE_ROW_SHIFT = 13, MCE_ROW_BITS = 10, MCE_LIST1_BIT = 23, MCE_REF_SHIFT = 28, MCE_MASK_BITS = 26, MCE_W_SHIFT = 23 };
#define MCE_LIST1  (1u << MCE_LIST1_BIT)   // flag: the reference index counts in list 1
#define MCE_KEEP   (1u << 24)       // flag (second pass, chroma quadrant entries): pass the samples through
#define MCE_Z      (1u << 25)       // flag (first pass): no residual here - the second pass adds it
#define MC_ITEM_MASK 0x0fffffffu    // all ones below the reference index: a padding entry (the sort writes MCE_PADDING into its x)
#define MCE_PADDING  0xffffffffu
#define MCE_MAX_MB_W ((1 << MCE_COL_BITS) - 1)     // widest picture whose columns fit an entry (p264hip_create)
static_assert(MCE_COL_SHIFT == MCE_QUAD_BITS && MCE_ROW_SHIFT == MCE_COL_SHIFT + MCE_COL_BITS && MCE_ROW_SHIFT + MCE_ROW_BITS <= MCE_LIST1_BIT && MAX_MB_ROWS <= 1 << MCE_ROW_BITS,
              "entry: quadrant, column and row side by side below the flags, the row field holds every macroblock row");
static_assert(MCE_LIST1 < MCE_KEEP && MCE_KEEP < MCE_Z && MCE_Z < 1u << MCE_REF_SHIFT && MC_ITEM_MASK == (1u << MCE_REF_SHIFT) - 1u && MCE_REF_SHIFT + 4 == 32 && P264HIP_MAX_REFS == 16,
              "entry: three flags of their own between the row and the 4 bits of reference index; MCE_REF_SLOT: a table of 2 x 16");
__device__ __forceinline__ uint32_t mcmb_entry(const McMb &k, int mbx, int mby, int q, int pass)
{
    const uint32_t l1 = (k.info >> (24 + q)) & 1u, z = (k.info >> (28 + q)) & 1u;
    return ((k.info >> (8 + 4 * q)) & 15u) << MCE_REF_SHIFT | (l1 ? MCE_LIST1 : 0u) | (z ? (pass ? MCE_KEEP : MCE_Z) : 0u) | (uint32_t)mby << MCE_ROW_SHIFT | (uint32_t)mbx << MCE_COL_SHIFT | (uint32_t)q;
}
__device__ __forceinline__ bool mce_valid(uint32_t x) { return (x & MC_ITEM_MASK) != MC_ITEM_MASK; }              // not padding
__device__ __forceinline__ int mce_row(uint32_t x) { return (int)((x >> MCE_ROW_SHIFT) & ((1u << MCE_ROW_BITS) - 1u)); }
__device__ __forceinline__ int mce_col(uint32_t x) { return (int)((x >> MCE_COL_SHIFT) & ((1u << MCE_COL_BITS) - 1u)); }
__device__ __forceinline__ int mce_quad(uint32_t x) { return (int)(x & ((1u << MCE_QUAD_BITS) - 1u)); }
// place of the entry's reference frame in a table of list 0's sixteen frames, then list 1's (mc_roles: ref_tab).  (A macro: as
// a function - by value, by reference, operands either way round - the same expression moved instructions in k_mc, k_mc_wp
// and k_mc_second.)
#define MCE_REF_SLOT(x) (((x) >> MCE_REF_SHIFT) | (((x) >> (MCE_LIST1_BIT - 4)) & 16u))
// second pass: z and w of an entry from the macroblock's record (mask word, QP; place in the coefficient stream, weight), and back
__device__ __forceinline__ uint32_t mce2_z(uint32_t rec_mask, uint32_t qp) { return (rec_mask & ((1u << MCE_MASK_BITS) - 1u)) | qp << MCE_MASK_BITS; }
__device__ __forceinline__ uint32_t mce2_z_no_mask(uint32_t z) { return z & ~((1u << MCE_MASK_BITS) - 1u); }
__device__ __forceinline__ uint32_t mce2_mask(uint32_t z) { return z & ((1u << MCE_MASK_BITS) - 1u); }
__device__ __forceinline__ int mce2_qp(uint32_t z) { return (int)(z >> MCE_MASK_BITS); }
__device__ __forceinline__ uint32_t mce2_w(uint32_t cidx, int weight) { return (cidx & ((1u << MCE_W_SHIFT) - 1u)) | (uint32_t)weight << MCE_W_SHIFT; }
__device__ __forceinline__ uint32_t mce2_cidx(uint32_t w) { return w & ((1u << MCE_W_SHIFT) - 1u); }
__device__ __forceinline__ int mce2_weight(uint32_t w) { return (int)w >> MCE_W_SHIFT; }
__device__ __forceinline__ bool quad_uniform(const uint4 &m0, const uint4 &m1, const uint4 &m2, const uint4 &m3, int q, uint32_t &v)
{
    // vectors of the quadrant's four 4x4 blocks (raster inside the macroblock: b0, b0+1, b0+4, b0+5)
    const uint4 top = q < 2 ? m0 : m2, bot = q < 2 ? m1 : m3;
    const uint32_t va = (q & 1) ? top.z : top.x, vb = (q & 1) ? top.w : top.y, vc = (q & 1) ? bot.z : bot.x, vd = (q & 1) ? bot.w : bot.y;
    v = va;
    return va == vb && va == vc && va == vd;
}
// what the classification reads of a macroblock (once, whatever the number of passes)
struct McIn { uint4 rec, m0, m1, m2, m3, n0, n1, n2, n3; uint32_t refs, refs1; bool two_lists; };
template <bool BPIC>
__device__ __forceinline__ McIn mc_load(const PicDev *pd, int mbi)
{
    McIn in;
    in.rec = gload4(pd->mb + mbi);
    const int *mvp = pd->mv + mbi * 16;
    in.m0 = gload4(mvp); in.m1 = gload4(mvp + 4); in.m2 = gload4(mvp + 8); in.m3 = gload4(mvp + 12);
    in.refs = gload1(pd->ref_idx + mbi * 4);
    in.refs1 = 0xffffffffu; in.two_lists = false;
    in.n0 = in.n1 = in.n2 = in.n3 = make_uint4(0, 0, 0, 0);
    // B pictures: a macroblock that predicts from list 0 only is an ordinary P-type macroblock for this stage
    if (BPIC && pd->slice_type == P264_SLICE_B && !P264_MB_IS_INTRA(in.rec.x & 255)) {
        in.refs1 = gload1(pd->ref_idx_l1 + mbi * 4);
        in.two_lists = ((~in.refs1 | in.refs) & 0x80808080u) != 0;             // some list-1 index >= 0, or some list-0 index < 0
        if (in.two_lists) { const int *mvp1 = pd->mv_l1 + mbi * 16; in.n0 = gload4(mvp1); in.n1 = gload4(mvp1 + 4); in.n2 = gload4(mvp1 + 8); in.n3 = gload4(mvp1 + 12); }
    }
    return in;
}
// scaled (k_mc_sort_scaled only): the picture has scaling_lists - luma and chroma of its macroblocks are filed as "no residual", the
// motion-compensation kernels leave the clipped prediction and k_scaled_inter adds the residual behind them (kernel_scaling.h)
template <bool BPIC, bool WP>
__device__ __forceinline__ McMb mc_classify(const PicDev *pd, const Geom &g, const McIn &in, int mbi, uint32_t inv_mbw, int band_log2, int pass, const bool scaled = false)
{
    McMb k;
    const uint4 rec = in.rec;
    uint4 m0 = in.m0, m1 = in.m1, m2 = in.m2, m3 = in.m3;
    const uint32_t refs = in.refs;
    k.info = P264_MB_IS_INTRA(rec.x & 255) ? 0u : MCMB_INTER;
#pragma unroll
    for (int q = 0; q < 4; q++) { k.key[q] = 0; k.vec[q] = 0; }
    int mbx, mby;
    split_mb(mbi, g, inv_mbw, mbx, mby);
    const int band = mby >> band_log2;
    const unsigned cc = scaled ? 0u : rec.y & (0x00ff0000u | P264_COEF_CHROMA_DC);   // any chroma level present
    // (a macroblock with P264_MB_T8X8: its luma items are filed as "no residual" - k_t8x8 adds it behind this stage, kernel_t8x8.h)
    const unsigned mask = scaled ? 0u : ((rec.x >> 24) & P264_MB_T8X8) ? (rec.y & ~0xffffu) : rec.y;
    if (WP && pd->explicit_wp) {
        // explicit weighted prediction (wave-uniform: a picture per workgroup; compiled into the k_mc_sort*_wp instances only): every inter macroblock goes to the generic two-list
        // class, all four quadrants, first pass - its lanes look up their lists, indices and weights themselves (mc_luma_body /
        // mc_chroma_body: wp_combine4)
        if (pass || !(k.info & MCMB_INTER)) { k.info = 0; return k; }
        const int kc = band * MCC_KEYS + MCC_BI + (cc ? MCC_RESID : 0);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int ky = band * MCY_KEYS + (PC_GEN | (((mask >> (4 * q)) & 15) ? MCY_RESID : 0));
            k.key[q] = (uint32_t)ky | (uint32_t)kc << 16;
        }
        return k;
    }
    const int n_ref = pd->n_ref;
    int ri[4];
    bool zq[4] = { false, false, false, false };           // Z per quadrant
    const bool two_lists = in.two_lists;
    const uint32_t refs1 = in.refs1;
    if (!BPIC || !two_lists) {
        if (pass) { k.info = 0; return k; }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            ri[q] = (int)(int8_t)(refs >> (8 * q));
            ri[q] = ref_entry(ri[q], n_ref);                // negative or past the list: entry 0, as the reference's flat lists
            k.info |= (uint32_t)ri[q] << (8 + 4 * q);
        }
    } else {
        const uint4 n0 = in.n0, n1 = in.n1, n2 = in.n2, n3 = in.n3;
        bool ok = true, any = false;
        uint32_t lq = 0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int r0 = (int)(int8_t)(refs >> (8 * q)), r1 = (int)(int8_t)(refs1 >> (8 * q));
            const bool u1 = r1 >= 0, u0 = r0 >= 0 || !u1;  // (no list at all: list 0, entry 0)
            uint32_t v0, v1;
            const bool un0 = quad_uniform(m0, m1, m2, m3, q, v0), un1 = quad_uniform(n0, n1, n2, n3, q, v1);
            ok &= (!u0 || un0) && (!u1 || un1);
            const bool bi = u0 && u1;
            bool l1; int r;
            if (!pass) { l1 = !u0; zq[q] = bi; r = l1 ? r1 : r0; any = true; }
            else       { l1 = bi; zq[q] = !bi; r = bi ? r1 : 0; any |= bi; }
            r = ref_entry(r, l1 ? pd->n_ref_l1 : n_ref);
            // (list and index: what a whole macroblock has to agree on; second pass: the list-0 index too - the weight is per pair)
            ri[q] = r | (l1 ? 16 : 0) | ((pass && bi) ? (r0 & 15) << 5 : 0);
            k.info |= (uint32_t)r << (8 + 4 * q);
            lq |= (l1 ? 1u : 0u) << q;
            // this pass's vector of the quadrant takes the place of the list-0 vectors below
            const uint32_t v = (pass && !bi) ? 0u : l1 ? v1 : v0;
            if (q == 0) { m0.x = m0.y = m1.x = m1.y = v; } else if (q == 1) { m0.z = m0.w = m1.z = m1.w = v; }
            else if (q == 2) { m2.x = m2.y = m3.x = m3.y = v; } else { m2.z = m2.w = m3.z = m3.w = v; }
        }
        if (!ok) {
            // vectors differing inside a quadrant: the generic two-list class, all four quadrants, first pass
            if (pass) { k.info = 0; return k; }
            k.info = MCMB_INTER;
            const int kc = band * MCC_KEYS + MCC_BI + (cc ? MCC_RESID : 0);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int ky = band * MCY_KEYS + (PC_GEN | (((mask >> (4 * q)) & 15) ? MCY_RESID : 0));
                k.key[q] = (uint32_t)ky | (uint32_t)kc << 16;
            }
            return k;
        }
        if (!any) { k.info = 0; return k; }
        k.info |= lq << 24 | ((uint32_t)zq[0] | (uint32_t)zq[1] << 1 | (uint32_t)zq[2] << 2 | (uint32_t)zq[3] << 3) << 28;
    }
    const uint32_t v0 = m0.x;
    const uint32_t diff = (m0.y ^ v0) | (m0.z ^ v0) | (m0.w ^ v0) | (m1.x ^ v0) | (m1.y ^ v0) | (m1.z ^ v0) | (m1.w ^ v0) | (m2.x ^ v0) | (m2.y ^ v0)
                        | (m2.z ^ v0) | (m2.w ^ v0) | (m3.x ^ v0) | (m3.y ^ v0) | (m3.z ^ v0) | (m3.w ^ v0);
    const bool whole = diff == 0 && ri[0] == ri[1] && ri[0] == ri[2] && ri[0] == ri[3] && zq[0] == zq[1] && zq[0] == zq[2] && zq[0] == zq[3];
    if (whole) {
        k.info |= MCMB_WHOLE;
        const int mvx = mv_x((int)v0), mvy = mv_y((int)v0);
        const int wx = mbx * 16 + (mvx >> 2) - 2, wy = mby * 16 + (mvy >> 2) - 2;      // 21 x 21 samples
        const bool in_y = wx >= 0 && wx + 21 <= g.w && wy >= 0 && wy + 21 <= g.h;
        const int cx = mbx * 8 + (mvx >> 3), cy = mby * 8 + (mvy >> 3);                 // 9 x 9 samples
        const bool in_c = cx >= 0 && cx + 9 <= g.cw && cy >= 0 && cy + 9 <= g.ch;
        const int ky = band * MCY_KEYS + (phase_class(mvx & 3, mvy & 3) | (in_y ? 0 : MCY_CLAMP) | (((mask & 0xffffu) && !zq[0]) ? MCY_RESID : 0));
        const int kc = band * MCC_KEYS + (in_c ? 0 : MCC_CLAMP) + ((cc && !zq[0]) ? MCC_RESID : 0);
        k.key[0] = (uint32_t)ky | (uint32_t)kc << 16;
        k.vec[0] = v0;
        return k;
    }
    bool c_inside = true;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        uint32_t va;
        const bool uniform = quad_uniform(m0, m1, m2, m3, q, va);
        const int X0 = mbx * 16 + (q & 1) * 8, Y0 = mby * 16 + (q >> 1) * 8;
        const int mvx = mv_x((int)va), mvy = mv_y((int)va);
        const int wx = X0 + (mvx >> 2) - 2, wy = Y0 + (mvy >> 2) - 2;                   // 13 x 13 samples
        const bool in_y = wx >= 0 && wx + 13 <= g.w && wy >= 0 && wy + 13 <= g.h;
        const int cx = X0 / 2 + (mvx >> 3), cy = Y0 / 2 + (mvy >> 3);                   // 5 x 5 samples
        const bool in_c = cx >= 0 && cx + 5 <= g.cw && cy >= 0 && cy + 5 <= g.ch;
        int pc = phase_class(mvx & 3, mvy & 3), fl = in_y ? 0 : MCY_CLAMP;
        if (!uniform) { pc = PC_GEN; fl = MCY_CLAMP; }
        if (((mask >> (4 * q)) & 15) && !zq[q]) fl |= MCY_RESID;
        const int ky = band * MCY_KEYS + (pc | fl);
        c_inside &= in_c && uniform;
        k.key[q] = (uint32_t)ky;
        k.vec[q] = va;
    }
    // the chroma entries of a split macroblock stay together (four consecutive list entries, quadrant 0..3): one key for all
    const int kc = band * MCC_KEYS + (c_inside ? 0 : MCC_CLAMP) + (cc ? MCC_RESID : 0);
#pragma unroll
    for (int q = 0; q < 4; q++) k.key[q] |= (uint32_t)kc << 16;
    return k;
}

// One workgroup per picture, one thread per macroblock: count the keys of the four lists, lay the key segments out (each
// padded to whole chunks), scatter the entries.  Up to MC_SORT_KEEP macroblocks per thread (1080p: 8) the classification
// stays in registers between the two passes: the macroblock arrays are read once.
#define MC_KEY_SLOTS (2 * MC_MAX_BANDS * MCY_KEYS + 2 * MC_MAX_BANDS * MCC_KEYS)
#define MC_SORT_KEEP 8
struct McSortCtx { const PicDev *pd; uint32_t *cnt, *pos, *out; int b_ym, b_yq, b_cm, b_cq; uint32_t l_ym, l_yq, l_cm, l_cq; int pass; };
__device__ __forceinline__ bool mcmb_luma_quad(const McMb &k, int q, int pass) { return !(pass && ((k.info >> (28 + q)) & 1u)); }
__device__ __forceinline__ void mc_count(const McSortCtx &c, const McMb &k)
{
    if (!(k.info & MCMB_INTER)) return;
    if (k.info & MCMB_WHOLE) { atomicAdd(&c.cnt[c.b_ym + (k.key[0] & 0xffffu)], 1u); atomicAdd(&c.cnt[c.b_cm + (k.key[0] >> 16)], 1u); }
    else {
#pragma unroll
        for (int q = 0; q < 4; q++) if (mcmb_luma_quad(k, q, c.pass)) atomicAdd(&c.cnt[c.b_yq + (k.key[q] & 0xffffu)], 1u);
        atomicAdd(&c.cnt[c.b_cq + (k.key[0] >> 16)], 4u);
    }
}
// (split_mb with the row kept in the caller's variable while it is fixed up: the form this file's split_mb had.  Through
// device_common.h's split_mb the compiler merges this split with mc_classify's and all four sort kernels change.)
__device__ __forceinline__ void scatter_split_mb(int mbi, const Geom &g, uint32_t inv_mbw, int &mbx, int &mby)
{
    mby = (int)__umulhi((unsigned)mbi, inv_mbw);
    if (mbi - mby * g.mb_w >= g.mb_w) mby++;
    mbx = mbi - mby * g.mb_w;
}
__device__ __forceinline__ void mc_scatter(const McSortCtx &c, const McMb &k, int mbi, const Geom &g, uint32_t inv_mbw, const bool scaled = false)
{
    if (!(k.info & MCMB_INTER)) return;
    int mbx, mby;
    scatter_split_mb(mbi, g, inv_mbw, mbx, mby);
    if (!c.pass) {
        // first pass: 8-byte entries, nothing of the record in them
        if (k.info & MCMB_WHOLE) {
            const uint2 e = make_uint2(mcmb_entry(k, mbx, mby, 0, 0), k.vec[0]);
            gstore2(c.out + c.l_ym + 2u * atomicAdd(&c.pos[c.b_ym + (k.key[0] & 0xffffu)], 1u), e);
            gstore2(c.out + c.l_cm + 2u * atomicAdd(&c.pos[c.b_cm + (k.key[0] >> 16)], 1u), e);
        } else {
            const uint32_t cq = atomicAdd(&c.pos[c.b_cq + (k.key[0] >> 16)], 4u);     // (a multiple of 4: every segment starts on a chunk)
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const uint2 e = make_uint2(mcmb_entry(k, mbx, mby, q, 0), k.vec[q]);
                gstore2(c.out + c.l_yq + 2u * atomicAdd(&c.pos[c.b_yq + (k.key[q] & 0xffffu)], 1u), e);
                gstore2(c.out + c.l_cq + 2u * (cq + (uint32_t)q), e);
            }
        }
        return;
    }
    // second pass: the record's residual fields and the weight of the pair of references (the table the parser derived,
    // core/macroblock.c:525-583; 32 = plain average) ride in the entry
    const uint4 rec = gload4(c.pd->mb + mbi);              // (second look at the record: out of the cache)
    const uint32_t ez = mce2_z(scaled ? 0u : rec.y, (rec.x >> 8) & 63u);      // (a scaled picture: no residual field anywhere, as in the first pass's keys)
    // (luma entries of a P264_MB_T8X8 macroblock: no coded block; the chroma entries keep the bits - they count them to find their levels)
    const uint32_t ezy = ((rec.x >> 24) & P264_MB_T8X8) ? (ez & ~0xffffu) : ez;
    uint32_t ew[4];
    const uint32_t refs = gload1(c.pd->ref_idx + mbi * 4);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        int w = 32;
        if (c.pd->weighted) {
            const int r0 = ref_entry((int)(int8_t)(refs >> (8 * q)), c.pd->n_ref), r1 = (int)((k.info >> (8 + 4 * q)) & 15u);
            w = (int)glob(c.pd->bipred_w)[r0 * P264HIP_MAX_REFS + r1];
        }
        ew[q] = mce2_w(rec.z, w);
    }
    if (k.info & MCMB_WHOLE) {
        const bool z = (k.info >> 28) & 1u;
        const uint4 e = make_uint4(mcmb_entry(k, mbx, mby, 0, 1), k.vec[0], z ? mce2_z_no_mask(ez) : ez, ew[0]);
        gstore4(c.out + c.l_ym + 4u * atomicAdd(&c.pos[c.b_ym + (k.key[0] & 0xffffu)], 1u), make_uint4(e.x, e.y, z ? e.z : ezy, e.w));
        gstore4(c.out + c.l_cm + 4u * atomicAdd(&c.pos[c.b_cm + (k.key[0] >> 16)], 1u), e);
    } else {
        const uint32_t cq = atomicAdd(&c.pos[c.b_cq + (k.key[0] >> 16)], 4u);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const bool z = (k.info >> (28 + q)) & 1u;
            const uint4 e = make_uint4(mcmb_entry(k, mbx, mby, q, 1), k.vec[q], z ? mce2_z_no_mask(ez) : ez, ew[q]);
            if (mcmb_luma_quad(k, q, 1)) gstore4(c.out + c.l_yq + 4u * atomicAdd(&c.pos[c.b_yq + (k.key[q] & 0xffffu)], 1u), make_uint4(e.x, e.y, z ? e.z : ezy, e.w));
            gstore4(c.out + c.l_cq + 4u * (cq + (uint32_t)q), e);
        }
    }
}
// One picture: P pictures one pass (the classification of up to MC_SORT_KEEP macroblocks per thread stays in registers between
// counting and scattering: the macroblock arrays are read once); B pictures both passes in one sweep (the arrays are read
// twice - keeping two classifications of eight macroblocks does not fit the register file).
template <bool BPIC, bool WP>
__device__ __forceinline__ void mc_sort_picture(const PicDev *__restrict__ pics, uint32_t *__restrict__ mc_all, const Geom &g, const McLayout &ml, uint32_t inv_mbw,
                                                uint32_t *cnt, uint32_t *pos, uint8_t *__restrict__ is_intra_all, const bool scaled = false)
{
    // by-product for the intra stage (k_intra's collect pass): one byte per macroblock, 1 = intra
    AS1 uint8_t *is_intra = glob(is_intra_all + (size_t)blockIdx.x * g.n_mb);
    constexpr int NP = BPIC ? 2 : 1;
    const PicDev *pd = pics + blockIdx.x;
    uint32_t *out = mc_all + (size_t)blockIdx.x * ml.words;
    const int tid = threadIdx.x;
    const int n_pass = pd->slice_type == P264_SLICE_I ? 0 : (BPIC && pd->slice_type == P264_SLICE_B) ? 2 : 1;       // wave-uniform
    if (tid < ML_LISTS * 2 && tid >= ML_LISTS * n_pass) gstore1(out + tid, 0);                            // the passes not taken: empty lists
    if (n_pass == 0) return;
    const int nky = (int)ml.n_bands * MCY_KEYS, nkc = (int)ml.n_bands * MCC_KEYS;
    const int b_ym = 0, b_yq = nky, b_cm = 2 * nky, b_cq = 2 * nky + nkc, b_end = 2 * nky + 2 * nkc;     // key slots of the four lists
    McSortCtx ctx[NP];
#pragma unroll
    for (int ps = 0; ps < NP; ps++)
        ctx[ps] = McSortCtx{ pd, cnt + ps * MC_KEY_SLOTS, pos + ps * MC_KEY_SLOTS, out, b_ym, b_yq, b_cm, b_cq, ml.off_list[ps * ML_LISTS + ML_YM], ml.off_list[ps * ML_LISTS + ML_YQ],
                             ml.off_list[ps * ML_LISTS + ML_CM], ml.off_list[ps * ML_LISTS + ML_CQ], ps };
    for (int k = tid; k < NP * MC_KEY_SLOTS; k += MC_SORT_THREADS) cnt[k] = 0;
    __syncthreads();
    const bool keep = !BPIC && g.n_mb <= MC_SORT_KEEP * MC_SORT_THREADS;
    McMb kept[BPIC ? 1 : MC_SORT_KEEP];
    if (keep) {
#pragma unroll
        for (int j = 0; j < (BPIC ? 1 : MC_SORT_KEEP); j++) {
            const int mbi = tid + j * MC_SORT_THREADS;
            kept[j].info = 0;
            if (mbi < g.n_mb) {
                kept[j] = mc_classify<BPIC, WP>(pd, g, mc_load<BPIC>(pd, mbi), mbi, inv_mbw, (int)ml.band_log2, 0, scaled); mc_count(ctx[0], kept[j]);
                is_intra[mbi] = (uint8_t)!(kept[j].info & MCMB_INTER);
            }
        }
    } else {
        for (int mbi = tid; mbi < g.n_mb; mbi += MC_SORT_THREADS) {
            const McIn in = mc_load<BPIC>(pd, mbi);
            is_intra[mbi] = (uint8_t)(P264_MB_IS_INTRA(in.rec.x & 255) != 0);
#pragma unroll
            for (int ps = 0; ps < NP; ps++) if (ps < n_pass) mc_count(ctx[ps], mc_classify<BPIC, WP>(pd, g, in, mbi, inv_mbw, (int)ml.band_log2, ps, scaled));
        }
    }
    __syncthreads();
    // segment starts: every thread sums the padded counts in front of its key (a few hundred LDS reads at most), notes the
    // key's class bits for each of its chunks, and the thread of a list's last key writes the number of chunks in use
#pragma unroll
    for (int ps = 0; ps < NP; ps++) {
        if (ps >= n_pass) break;
        const uint32_t *cn = cnt + ps * MC_KEY_SLOTS;
        uint32_t *po = pos + ps * MC_KEY_SLOTS;
        const int L0 = ps * ML_LISTS;
        for (int k = tid; k < b_end; k += MC_SORT_THREADS) {
            const int l = k < b_yq ? ML_YM : k < b_cm ? ML_YQ : k < b_cq ? ML_CM : ML_CQ;
            const int first = l == ML_YM ? b_ym : l == ML_YQ ? b_yq : l == ML_CM ? b_cm : b_cq;
            const int kk = k - first, nk = l < ML_CM ? nky : nkc;
            const uint32_t per = (uint32_t)mc_chunk_items(l);
            uint32_t start = 0;
            for (int j = 0; j < kk; j++) start += (cn[first + j] + per - 1) / per;
            const uint32_t n = (cn[k] + per - 1) / per;                         // chunks of this key, from chunk `start`
            po[k] = start * per;
            AS1 uint8_t *cls = glob((uint8_t *)(out + (l == ML_YM ? ml.off_cls[L0 + ML_YM] : l == ML_YQ ? ml.off_cls[L0 + ML_YQ] : l == ML_CM ? ml.off_cls[L0 + ML_CM] : ml.off_cls[L0 + ML_CQ])));
            const uint8_t v = (uint8_t)(kk % mc_list_keys(l));
            for (uint32_t c = 0; c < n; c++) cls[start + c] = v;
            if (kk == nk - 1) gstore1(out + L0 + l, start + n);
        }
    }
    __syncthreads();
    if (keep) {
#pragma unroll
        for (int j = 0; j < (BPIC ? 1 : MC_SORT_KEEP); j++) mc_scatter(ctx[0], kept[j], tid + j * MC_SORT_THREADS, g, inv_mbw, scaled);
    } else {
        for (int mbi = tid; mbi < g.n_mb; mbi += MC_SORT_THREADS) {
            const McIn in = mc_load<BPIC>(pd, mbi);
#pragma unroll
            for (int ps = 0; ps < NP; ps++) if (ps < n_pass) mc_scatter(ctx[ps], mc_classify<BPIC, WP>(pd, g, in, mbi, inv_mbw, (int)ml.band_log2, ps, scaled), mbi, g, inv_mbw, scaled);
        }
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < NP; ps++) {
        if (ps >= n_pass) break;
        const uint32_t *po = pos + ps * MC_KEY_SLOTS;
        const int L0 = ps * ML_LISTS;
        for (int k = tid; k < b_end; k += MC_SORT_THREADS) {                  // padding entries behind every segment
            const int l = k < b_yq ? ML_YM : k < b_cm ? ML_YQ : k < b_cq ? ML_CM : ML_CQ;
            const uint32_t per = (uint32_t)mc_chunk_items(l), end = po[k];
            // (selects on k itself: as a chain on l the compiler builds a four-entry table in scratch memory and indexes it)
            uint32_t lo = ml.off_list[L0 + ML_CQ];
            if (k < b_cq) lo = ml.off_list[L0 + ML_CM];
            if (k < b_cm) lo = ml.off_list[L0 + ML_YQ];
            if (k < b_yq) lo = ml.off_list[L0 + ML_YM];
            for (uint32_t p = end; p < (end + per - 1) / per * per; p++) {
                if (ps) gstore4(out + lo + 4u * p, make_uint4(MCE_PADDING, 0, 0, 0));
                else gstore2(out + lo + 2u * p, make_uint2(MCE_PADDING, 0));
            }
        }
    }
}
// batches without B pictures (the two-list classification costs registers the sort of a P picture does not have to pay for)
__global__ __launch_bounds__(MC_SORT_THREADS)
void k_mc_sort(const PicDev *__restrict__ pics, uint32_t *__restrict__ mc_all, Geom g, McLayout ml, uint32_t inv_mbw, uint8_t *__restrict__ is_intra)
{
    __shared__ uint32_t cnt[MC_KEY_SLOTS], pos[MC_KEY_SLOTS];
    mc_sort_picture<false, false>(pics, mc_all, g, ml, inv_mbw, cnt, pos, is_intra);
}
// the same for batches with a picture of explicit weighted prediction (launched with k_mc_wp; k_mc_sort itself has no test for it)
__global__ __launch_bounds__(MC_SORT_THREADS)
void k_mc_sort_wp(const PicDev *__restrict__ pics, uint32_t *__restrict__ mc_all, Geom g, McLayout ml, uint32_t inv_mbw, uint8_t *__restrict__ is_intra)
{
    __shared__ uint32_t cnt[MC_KEY_SLOTS], pos[MC_KEY_SLOTS];
    mc_sort_picture<false, true>(pics, mc_all, g, ml, inv_mbw, cnt, pos, is_intra);
}
// batches with B pictures
#define MC_SORT_B_WAVES_PER_EU 4       // 78 registers, no scratch, one workgroup per CU (round 4 shipped 8: 64 registers of which 9 spilled, two workgroups
                                       // per CU - the MC stage of a B launch 5.44 -> 5.37 ms, scratch/r4_sortb_occ.sh; given back for a binary without scratch)
__global__ __launch_bounds__(MC_SORT_THREADS, MC_SORT_B_WAVES_PER_EU)
void k_mc_sort_b(const PicDev *__restrict__ pics, uint32_t *__restrict__ mc_all, Geom g, McLayout ml, uint32_t inv_mbw, uint8_t *__restrict__ is_intra)
{
    __shared__ uint32_t cnt[2 * MC_KEY_SLOTS], pos[2 * MC_KEY_SLOTS];
    mc_sort_picture<true, false>(pics, mc_all, g, ml, inv_mbw, cnt, pos, is_intra);
}
__global__ __launch_bounds__(MC_SORT_THREADS, MC_SORT_B_WAVES_PER_EU)
void k_mc_sort_b_wp(const PicDev *__restrict__ pics, uint32_t *__restrict__ mc_all, Geom g, McLayout ml, uint32_t inv_mbw, uint8_t *__restrict__ is_intra)
{
    __shared__ uint32_t cnt[2 * MC_KEY_SLOTS], pos[2 * MC_KEY_SLOTS];
    mc_sort_picture<true, true>(pics, mc_all, g, ml, inv_mbw, cnt, pos, is_intra);
}
// batches with a picture that has scaling_lists: the residuals of such a picture's inter macroblocks are left to k_scaled_inter.
// scale[picture].scaled is per workgroup.  Two instances: batches of unweighted P (and I) pictures - k_mc_sort's shape, the
// classification kept in registers -, and every other batch - the two-list, weighted instance.
__global__ __launch_bounds__(MC_SORT_THREADS)
void k_mc_sort_scaled_p(const PicDev *__restrict__ pics, uint32_t *__restrict__ mc_all, Geom g, McLayout ml, uint32_t inv_mbw, uint8_t *__restrict__ is_intra,
                        const ScaleDev *__restrict__ scale)
{
    __shared__ uint32_t cnt[MC_KEY_SLOTS], pos[MC_KEY_SLOTS];
    mc_sort_picture<false, false>(pics, mc_all, g, ml, inv_mbw, cnt, pos, is_intra, scale[blockIdx.x].scaled != 0);
}
__global__ __launch_bounds__(MC_SORT_THREADS, MC_SORT_B_WAVES_PER_EU)
void k_mc_sort_scaled(const PicDev *__restrict__ pics, uint32_t *__restrict__ mc_all, Geom g, McLayout ml, uint32_t inv_mbw, uint8_t *__restrict__ is_intra,
                      const ScaleDev *__restrict__ scale)
{
    __shared__ uint32_t cnt[2 * MC_KEY_SLOTS], pos[2 * MC_KEY_SLOTS];
    mc_sort_picture<true, true>(pics, mc_all, g, ml, inv_mbw, cnt, pos, is_intra, scale[blockIdx.x].scaled != 0);
}
