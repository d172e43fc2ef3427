// kernel_deblock_body.h - the text of k_deblock (DEBLOCK_CR 0) and k_deblock_cr (DEBLOCK_CR 1): kernel_deblock.h includes it once for
// each and says what the two are.  Everything it uses is declared there: compiled on its own (DEBLOCK_CR not defined) it is that header.
#ifndef DEBLOCK_CR
#include "kernel_deblock.h"
#else
__global__ __launch_bounds__(ROW_WAVES * 64)
#if DEBLOCK_CR
void k_deblock_cr(const PicDev *__restrict__ pics, Geom g_, const EdgeInfo *__restrict__ info, int *status, int n_pics, int rb_log2_, int pics_per_wg, int odd_single,
                  const uint32_t *__restrict__ cr_info)
#else
void k_deblock(const PicDev *__restrict__ pics, Geom g_, const EdgeInfo *__restrict__ info, int *status, int n_pics, int rb_log2_, int pics_per_wg, int odd_single)
#endif
{
    typedef OctLdsT<DEBLOCK_CR ? EDGE_DW_CR : EDGE_DW> OctLds;
    __shared__ int progress[MAX_PICS_PER_WG][MAX_BANDS];     // fully stored macroblocks of a band's last row
    __shared__ OctLds lds[ROW_WAVES][8];
    __shared__ EdgeTables tables;
    edge_tables_init(tables);
    const Geom g = g_;
    // (the wavefront number is a scalar: without readfirstlane the compiler takes the unit loop for divergent and keeps all of its
    // book-keeping - unit, band, picture pointers - in vector registers)
    const int wave = rfl((int)(threadIdx.x >> 6)), n_waves = blockDim.x >> 6, lane = threadIdx.x & 63;
    // A work unit = (band, group of pictures): `1 << rb_log2` rows of `8 >> rb_log2` pictures.  odd_single (with bands of 4 rows and
    // an odd number of pictures, round 5): the pictures go in pairs and the LAST one on its own in bands of 8 rows - a pair's
    // group with one picture missing would issue every instruction of its 17 units for half the lanes.
    const int n_bands_all = (g.mb_h + (1 << rb_log2_) - 1) >> rb_log2_;
    const int n_groups_all = (pics_per_wg + (8 >> rb_log2_) - 1) / (8 >> rb_log2_);
    const int n_pairs = pics_per_wg >> 1, n_bands8 = (g.mb_h + 7) >> 3, per_step = 2 * n_pairs + 1;     // odd_single: units per two pair bands + one single band
    const int n_units = !odd_single ? n_bands_all * n_groups_all : (n_bands8 - 1) * per_step + (n_bands_all - 2 * (n_bands8 - 1)) * n_pairs + 1;
    for (int k = threadIdx.x; k < MAX_PICS_PER_WG * MAX_BANDS; k += blockDim.x) (&progress[0][0])[k] = 0;
    __syncthreads();
    bool ok = true;

    // units in band-major order: a wavefront takes unit u only after u - n_waves, and band b of a group only waits for band
    // b - 1 of the same group, which is an earlier unit - nobody waits for a unit that has not been started
    for (int unit = wave; unit < n_units; unit += n_waves) {
        // the unit's shape, band and first picture (scalars).  odd_single: steps of {band 2s of every pair, band s of the single
        // picture, band 2s + 1 of every pair} - a band still only waits for the band above it of the same pictures, an earlier unit
        int rb_log2 = rb_log2_, band, pic0;
        if (!odd_single) { band = unit / n_groups_all; pic0 = (unit - band * n_groups_all) * (8 >> rb_log2_); }
        else {
            const int st = unit / per_step, r = unit - st * per_step;
            if (r < n_pairs) { band = 2 * st; pic0 = 2 * r; }
            else if (r == n_pairs) { rb_log2 = 3; band = st; pic0 = pics_per_wg - 1; }
            else { band = 2 * st + 1; pic0 = 2 * (r - n_pairs - 1); }
        }
        const int RB = 1 << rb_log2, PW = 8 >> rb_log2;         // rows of the band, pictures of the wavefront
        // Everything that follows from the lane number is derived again per unit (a few dozen instructions against ~100 000 of the
        // unit): hoisted out of this loop, the lane constants that only the unit's set-up needs (64-bit offsets of the lane's rows,
        // products with the strip sizes) stayed alive through the iteration loop - the kernel has no register to spare for them
        // and spilled 17.
        int lane_u = lane;
        asm volatile("" : "+v"(lane_u));
        const int o = lane_u >> 3, j = lane_u & 7;
        const int gr = o & (RB - 1), pi = o >> rb_log2;           // row inside the band, picture inside the wavefront
        OctLds &L = lds[wave][o];
        const int seg2 = (j >> 1) * 2, cseg2 = (j & 3) * 2;       // 2 x the bS segment of this lane's luma / chroma lines
        const int cp = j >> 2, cr = (j & 3) * 2;                  // chroma plane, first chroma line of this lane
        uint8_t *tile8 = (uint8_t *)L.tile;
        const int piw = pic0 + pi;                                // picture inside the workgroup
        const int pic = blockIdx.x * pics_per_wg + piw;
        const PicDev *pd = pics + min(pic, n_pics - 1);
        const bool pic_ok = pi < PW && piw < pics_per_wg && pic < n_pics && pd->deblock;
        uint8_t *F = pd->dst;                                     // strip frame layout (device_common.h)
        const EdgeInfo *pinfo = info + (size_t)min(pic, n_pics - 1) * g.n_mb;
        const int alpha_off = pd->alpha_off, beta_off = pd->beta_off;
        uint32_t last_qp = 0xffffffffu, last_avg = 0xffffffffu;   // QPs the octet's class parameters in LDS were expanded for
        const int R0 = band << rb_log2;
        const int nrows = min(RB, g.mb_h - R0), last = nrows - 1;
        const int row = R0 + gr;
        const bool have_row = pic_ok && gr < nrows;
        const bool below_in_band = gr < last;                  // the row below belongs to the next octet
        const bool top_exists = row > 0;
        const bool from_above = have_row && gr == 0 && band > 0;   // the rows above come from the band above, through memory
        const int rowc = min(row, g.mb_h - 1);
        // Strip layout: macroblock x of this row owns the 256 luma bytes at x*ystrip + row*256 and the 128 chroma bytes at
        // coff + x*cstrip + row*128 (rows of 8 bytes U, 8 bytes V).  This lane's two luma rows are the 32 bytes at +32j, its
        // two chroma rows 8 bytes each: an octet reads and writes whole cache lines.
        const uint32_t sY = g.ystrip, sC = g.cstrip;
        uint8_t *ownY = F + (size_t)rowc * MB_LUMA_BYTES + j * 32, *ownC = F + g.coff + (size_t)rowc * MB_CHROMA_BYTES + cr * 16 + cp * 8;
        // the rows above (valid if top_exists): lanes 0..3 luma rows 12..15 of the macroblock above, lanes 4..7 its chroma
        // rows 6,7 of plane (j>>1)&1
        const uint32_t sT = j < 4 ? sY : sC;
        uint8_t *topP = j < 4 ? F + (ptrdiff_t)(rowc - 1) * MB_LUMA_BYTES + 192 + j * 16
                              : F + g.coff + (ptrdiff_t)(rowc - 1) * MB_CHROMA_BYTES + (6 + (j & 1)) * 16 + ((j >> 1) & 1) * 8;
        // Addresses inside the iteration loop: macroblock x = t - 2 gr of the row.  The lane-constant part (- 2 gr strips) is folded
        // into the bases here, in 64-bit arithmetic, so that the loop adds only t x strip - a scalar - to one pointer per array
        // (as (uint32) x * strip the compiler cannot fold it and keeps one 64-bit constant per array alive: registers it does not have).
        const ptrdiff_t lag = -(ptrdiff_t)(DB_LAG * gr);
        uint8_t *ownY0 = ownY + lag * (ptrdiff_t)sY, *ownC0 = ownC + lag * (ptrdiff_t)sC, *topP0 = topP + lag * (ptrdiff_t)sT;
        const EdgeInfo *pinfo0 = pinfo + (ptrdiff_t)row * g.mb_w + lag;
        // (CR: the macroblock's side word, at the same index as its EdgeInfo)
#if DEBLOCK_CR
        const uint32_t *cinfo0 = cr_info + (pinfo0 - info);
        uint32_t fCr = 0, last_cr = 0xffffffffu;                  // in flight for the next iteration / what the Cr classes in LDS were expanded for
#endif
        int *my_progress = &progress[piw & (MAX_PICS_PER_WG - 1)][band];
        const bool publisher = have_row && gr == last && j == 0;
        OctLds &Lnext = lds[wave][min(o + 1, 7)];

        uint32_t ya0 = 0, yb0 = 0, ca0 = 0, cb0 = 0;                  // columns -4..-1: the previous macroblock's last four
        uint4 fYa = make_uint4(0, 0, 0, 0), fYb = fYa, fC = fYa, fT = fYa, fE = fYa;   // in flight for the next iteration
        const int n_iter = g.mb_w + 1 + DB_LAG * last;
        const int *wait_on = from_above ? my_progress - 1 : my_progress;
        // tile addresses of this lane's rows
        uint32_t *tYa = L.tile + (2 * j) * 4, *tYb = tYa + 4, *tCa = L.tile + 64 + cp * 16 + cr * 2, *tCb = tCa + 2;

        // loads for iteration t
        auto prefetch = [&](int t) {
            const int x = t - DB_LAG * gr;
            const bool actn = have_row && x >= 0 && x < g.mb_w;
            if (ok) {
                // macroblock x needs the band above to have stored x completely
                const bool need = from_above && actn;
                const int want = x + 1;
                int spins = 0;
                while (__ballot(need && __hip_atomic_load(wait_on, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < want)) {
                    __builtin_amdgcn_s_sleep(DEBLOCK_WAIT_SLEEP);
                    if (++spins > SPIN_LIMIT) { if (lane_u == 0) atomicOr(status, 1); ok = false; break; }
                }
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            }
            if (actn) {
                if (j == 0) fE = gload4(pinfo0 + t);
#if DEBLOCK_CR
                fCr = gload1(cinfo0 + t);                            // (all eight lanes the same dword: the "changed" test below needs it in each)
#endif
                const uint8_t *tp = topP0 + (ptrdiff_t)t * (ptrdiff_t)sT;
                if (from_above) {
                    if (j < 4) fT = gload4(tp);
                    else { uint2 v2 = gload2(tp); fT.x = v2.x; fT.y = v2.y; }
                }
                const uint8_t *yp = ownY0 + (ptrdiff_t)t * (ptrdiff_t)sY, *cp2 = ownC0 + (ptrdiff_t)t * (ptrdiff_t)sC;
                fYa = gload4(yp); fYb = gload4(yp + 16);
                const uint2 ca2 = gload2(cp2), cb2 = gload2(cp2 + 16);
                fC = make_uint4(ca2.x, ca2.y, cb2.x, cb2.y);
            }
        };

        prefetch(0);
        for (int t = 0; t < n_iter; t++) {
            const int x = t - DB_LAG * gr;
            const bool act = have_row && x >= 0 && x < g.mb_w;         // filter macroblock x
            const bool flush = have_row && x >= 1 && x <= g.mb_w;       // store macroblock x-1
            uint32_t *ring = L.ring[x & 3];
            // ---- land what was prefetched for this iteration: pixels stay in registers for the vertical pass ----
            uint32_t ya[5] = { ya0, fYa.x, fYa.y, fYa.z, fYa.w }, yb[5] = { yb0, fYb.x, fYb.y, fYb.z, fYb.w };
            uint32_t ca[3] = { ca0, fC.x, fC.y }, cb[3] = { cb0, fC.z, fC.w };
            if (act) {
                if (from_above) {
                    if (j < 4) *(uint4 *)(ring + j * 4) = fT;
                    else *(uint2 *)(ring + 16 + (j - 4) * 2) = make_uint2(fT.x, fT.y);
                }
                if (j == 0) *(uint4 *)L.edge = fE;
            }
            // Everything this wave has issued is complete here (the prefetch was issued before the previous
            // iteration's horizontal pass, its stores before that): macroblocks 0 .. x-2 of this row are in memory.
            // Publish with RELEASE semantics at workgroup scope: the band below reads these macroblocks' pixels through global
            // memory on the same CU.  (The explicit wait drains the WHOLE wave's stores - the publisher lane speaks for all
            // eight octets of its wave, and a release fence only orders the publishing lane's own view.)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (publisher) __hip_atomic_store(my_progress, min(max(x - 1, 0), g.mb_w), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            wave_lds_fence();
            // the rows above macroblock x-1 were finished by its horizontal pass in the previous iteration
            if (flush && top_exists) {
                const uint32_t *pr = L.ring[(x - 1) & 3];
                uint8_t *tp = topP0 + (ptrdiff_t)(t - 1) * (ptrdiff_t)sT;
                if (j < 4) gstore4(tp, *(const uint4 *)(pr + j * 4));
                else gstore2(tp, *(const uint2 *)(pr + 16 + (j - 4) * 2));
            }
            EdgeRegs E;
            {
                const uint4 v = act ? *(const uint4 *)L.edge : make_uint4(0, 0, 0, 0);
                E.e[0] = v.x; E.e[1] = v.y; E.lds = L.edge;
                // the class parameters of the octet's LDS copy follow the macroblock's QPs and offset deltas (v.z holds both): expanded
                // again only when those change
#if DEBLOCK_CR
                const bool changed = act && (v.z != last_qp || v.w != last_avg || fCr != last_cr);
#else
                const bool changed = act && (v.z != last_qp || v.w != last_avg);
#endif
                if (__ballot(changed)) {
                    if (act) {
#if DEBLOCK_CR
                        {
                            // nine classes on eight lanes: lane j class j (6, 7: Cr's left and top), then lane 0 Cr's inner class
                            const EdgeClass ec = edge_expand_cr(tables, v.z, v.w, fCr, j, alpha_off, beta_off);
                            *(uint4 *)(L.edge + 4 + 8 * j) = ec.ab; L.edge[8 + 8 * j] = ec.tc;
                            if (j == 0) { const EdgeClass ei = edge_expand_cr(tables, v.z, v.w, fCr, 8, alpha_off, beta_off); *(uint4 *)(L.edge + 4 + 8 * 8) = ei.ab; L.edge[8 + 8 * 8] = ei.tc; }
                            last_cr = fCr;
                        }
#else
                        if (j < 6) { const EdgeClass ec = edge_expand(tables, v.z, v.w, j, alpha_off, beta_off); *(uint4 *)(L.edge + 4 + 8 * j) = ec.ab; L.edge[8 + 8 * j] = ec.tc; }
#endif
                        last_qp = v.z; last_avg = v.w;
                    }
                    wave_lds_fence();
                }
            }
            // chroma edges read their classes through Ec: the same copy, in the Cr instance three classes (24 dwords) further for the lanes of plane 1
#if DEBLOCK_CR
            EdgeRegs Ec = E;
            Ec.lds = L.edge + 24 * cp;
#else
            const EdgeRegs &Ec = E;
#endif
            const bool any_edges = __ballot((E.e[0] | E.e[1]) != 0) != 0;

            if (any_edges) {
                // ---------- vertical edges, in registers ----------
#pragma unroll
                for (int ed = 0; ed < 4; ed++) {
                    const int b = E.code(0, ed, seg2), k = edge_class(0, ed);
                    if (__ballot(b != 0) == 0) continue;
                    pk16 p2 = pair_byte<1>(ya[ed], yb[ed]), p1 = pair_byte<2>(ya[ed], yb[ed]), p0 = pair_byte<3>(ya[ed], yb[ed]);
                    pk16 q0 = pair_byte<0>(ya[ed+1], yb[ed+1]), q1 = pair_byte<1>(ya[ed+1], yb[ed+1]), q2 = pair_byte<2>(ya[ed+1], yb[ed+1]);
                    const EdgeParams ep(E, k);
                    const pk16 A = as_pk(ep.alpha2()), B = as_pk(ep.beta2()), nA = as_pk(ep.nalpha2()), nB = as_pk(ep.nbeta2());
                    pk16 e;
                    const pk16 f = pk_edge_flag(p1, p0, q0, q1, A, nA, B, nB, e);
                    const pk16 ap = pk_sign(pk_within(p2 - p0, B, nB)), aq = pk_sign(pk_within(q2 - q0, B, nB));
                    const pk16 en = as_pk(mask_bs123(b, ed));
                    const pk16 op2 = p2, op1 = p1, op0 = p0, oq0 = q0, oq1 = q1, oq2 = q2;
                    pk_luma_normal(p2, p1, p0, q0, q1, q2, e, f & en, ap, aq, as_pk(ep.tc2(b)));
                    // bS 4 exists on macroblock edges only (k_deblock_bs), and the strong filter changes nothing where the
                    // sample flag is off
                    if (ed == 0 && __ballot((as_u(f) & mask_bs4(b)) != 0)) {
                        const pk16 str = as_pk(mask_bs4(b));
                        pk16 sp2 = op2, sp1 = op1, sp0 = op0, sq0 = oq0, sq1 = oq1, sq2 = oq2;
                        pk_luma_strong(pair_byte<0>(ya[ed], yb[ed]), sp2, sp1, sp0, sq0, sq1, sq2, pair_byte<3>(ya[ed+1], yb[ed+1]), f & str, ap, aq, A);
                        p1 = pk_sel(str, sp1, p1); p0 = pk_sel(str, sp0, p0); q0 = pk_sel(str, sq0, q0); q1 = pk_sel(str, sq1, q1);
                        ya[ed] = perm(as_u(sp2), ya[ed], 0x03020400u);   yb[ed] = perm(as_u(sp2), yb[ed], 0x03020600u);
                        ya[ed+1] = perm(as_u(sq2), ya[ed+1], 0x03040100u); yb[ed+1] = perm(as_u(sq2), yb[ed+1], 0x03060100u);
                    }
                    // p0 / q0 clipped into byte pairs (row 2j in byte 0, row 2j+1 in byte 1), merged with p1 / q1: bytes {p1 a, p0 a, p1 b, p0 b}
                    const uint32_t tp = perm(pk_clip_bytes(p0), as_u(p1), 0x05020400u), tq = perm(as_u(q1), pk_clip_bytes(q0), 0x06010400u);
                    ya[ed] = perm(tp, ya[ed], 0x05040100u);     yb[ed] = perm(tp, yb[ed], 0x07060100u);
                    ya[ed+1] = perm(tq, ya[ed+1], 0x03020504u); yb[ed+1] = perm(tq, yb[ed+1], 0x03020706u);
                }
#pragma unroll
                for (int ed = 0; ed < 4; ed += 2) {
                    const int b = E.code(0, ed, cseg2), k = edge_class(0, ed) + 3, c = ed >> 1;
                    if (__ballot(b != 0) == 0) continue;
                    pk16 p1 = pair_byte<2>(ca[c], cb[c]), p0 = pair_byte<3>(ca[c], cb[c]);
                    pk16 q0 = pair_byte<0>(ca[c+1], cb[c+1]), q1 = pair_byte<1>(ca[c+1], cb[c+1]);
                    const EdgeParams ep(Ec, k);
                    const pk16 A = as_pk(ep.alpha2()), B = as_pk(ep.beta2());
                    pk16 e;
                    const pk16 f = pk_edge_flag(p1, p0, q0, q1, A, as_pk(ep.nalpha2()), B, as_pk(ep.nbeta2()), e);
                    pk_chroma(p1, p0, q0, q1, e, f, as_pk(mask_bs123(b, ed)), as_pk(ed == 0 ? mask_bs4(b) : 0u), ed == 0 && __ballot(b == 3) != 0, as_pk(ep.tc2(b)));
                    const uint32_t P0 = pk_clip_bytes(p0), Q0 = pk_clip_bytes(q0);      // (row a in byte 0, row b in byte 1)
                    ca[c] = perm(P0, ca[c], 0x04020100u);     cb[c] = perm(P0, cb[c], 0x05020100u);
                    ca[c+1] = perm(Q0, ca[c+1], 0x03020104u); cb[c+1] = perm(Q0, cb[c+1], 0x03020105u);
                }
            }
            // ---- macroblock x-1 is final now: columns 0..11 still sit in the tile, its last four columns are ya[0]/yb[0].
            // Store it as whole rows; rows 12..15 go to the octet below instead, which stores them as its "rows above".
            if (flush) {
                uint4 sa = *(const uint4 *)tYa, sb = *(const uint4 *)tYb;
                uint2 ta = *(const uint2 *)tCa, tb = *(const uint2 *)tCb;
                sa.w = ya[0]; sb.w = yb[0]; ta.y = ca[0]; tb.y = cb[0];
                uint32_t *nr = Lnext.ring[(x - 1) & 3];
                uint8_t *yp = ownY0 + (ptrdiff_t)(t - 1) * (ptrdiff_t)sY, *cp2 = ownC0 + (ptrdiff_t)(t - 1) * (ptrdiff_t)sC;
                if (below_in_band && j >= 6) { *(uint4 *)(nr + (2 * j - 12) * 4) = sa; *(uint4 *)(nr + (2 * j - 11) * 4) = sb; }
                else { gstore4(yp, sa); gstore4(yp + 16, sb); }
                if (below_in_band && (j & 3) == 3) { *(uint2 *)(nr + 16 + cp * 4) = ta; *(uint2 *)(nr + 16 + cp * 4 + 2) = tb; }
                else { gstore2(cp2, ta); gstore2(cp2 + 16, tb); }
            }
            wave_lds_fence();
            // ---------- rows of macroblock x -> tile ----------
            if (act) {
                *(uint4 *)tYa = make_uint4(ya[1], ya[2], ya[3], ya[4]); *(uint4 *)tYb = make_uint4(yb[1], yb[2], yb[3], yb[4]);
                *(uint2 *)tCa = make_uint2(ca[1], ca[2]);               *(uint2 *)tCb = make_uint2(cb[1], cb[2]);
            }
            wave_lds_fence();
            if (t + 1 < n_iter) prefetch(t + 1);                      // the next iteration's loads travel during the horizontal pass
            // ---------- horizontal edges: column pairs out of the tile, filtered, back into the tile ----------
            const bool h_edges = __ballot(E.e[1] != 0) != 0;
            if (h_edges) {
                if (act) {
                    // luma: columns 2j, 2j+1
                    const uint8_t *top = (const uint8_t *)ring + 2 * j, *col = tile8 + 2 * j;
                    pk16 c[20];
#pragma unroll
                    for (int r = 0; r < 4; r++) { uint32_t v = *(const uint16_t *)(top + r * 16); c[r] = as_pk(perm(v, v, 0x0c010c00u)); }
#pragma unroll
                    for (int r = 0; r < 16; r++) { uint32_t v = *(const uint16_t *)(col + r * 16); c[4 + r] = as_pk(perm(v, v, 0x0c010c00u)); }
#pragma unroll
                    for (int ed = 0; ed < 4; ed++) {
                        const int b = E.code(1, ed, seg2), k = edge_class(1, ed);
                        if (__ballot(b != 0) == 0) continue;
                        pk16 &p3 = c[4*ed], &p2 = c[4*ed+1], &p1 = c[4*ed+2], &p0 = c[4*ed+3], &q0 = c[4*ed+4], &q1 = c[4*ed+5], &q2 = c[4*ed+6], &q3 = c[4*ed+7];
                        const EdgeParams ep(E, k);
                        const pk16 A = as_pk(ep.alpha2()), B = as_pk(ep.beta2()), nA = as_pk(ep.nalpha2()), nB = as_pk(ep.nbeta2());
                        pk16 e;
                        const pk16 f = pk_edge_flag(p1, p0, q0, q1, A, nA, B, nB, e);
                        const pk16 ap = pk_sign(pk_within(p2 - p0, B, nB)), aq = pk_sign(pk_within(q2 - q0, B, nB));
                        const pk16 en = as_pk(mask_bs123(b, ed));
                        pk16 sp2 = p2, sp1 = p1, sp0 = p0, sq0 = q0, sq1 = q1, sq2 = q2;
                        pk_luma_normal(p2, p1, p0, q0, q1, q2, e, f & en, ap, aq, as_pk(ep.tc2(b)));
                        if (ed == 0 && __ballot((as_u(f) & mask_bs4(b)) != 0)) {
                            const pk16 str = as_pk(mask_bs4(b));
                            pk_luma_strong(p3, sp2, sp1, sp0, sq0, sq1, sq2, q3, f & str, ap, aq, A);
                            p2 = pk_sel(str, sp2, p2); p1 = pk_sel(str, sp1, p1); p0 = pk_sel(str, sp0, p0);
                            q0 = pk_sel(str, sq0, q0); q1 = pk_sel(str, sq1, q1); q2 = pk_sel(str, sq2, q2);
                        }
                    }
                    // rows -3 .. 14 back (row -4 cannot change).  The rows either side of an edge (p0 / q0: -1 | 0, 3 | 4, 7 | 8, 11 | 12) may
                    // hold p0 + delta / q0 - delta not yet clipped: clipped into a byte pair here, one 16-bit store
                    {
                        uint8_t *topw = (uint8_t *)ring + 2 * j, *colw = tile8 + 2 * j;
                        lds_put_pair<1 * 16>(topw, c[1]); lds_put_pair<2 * 16>(topw, c[2]); lds_put_clipped<3 * 16>(topw, c[3]);
                        lds_put_clipped<0 * 16>(colw, c[4]);  lds_put_pair<1 * 16>(colw, c[5]);   lds_put_pair<2 * 16>(colw, c[6]);   lds_put_clipped<3 * 16>(colw, c[7]);
                        lds_put_clipped<4 * 16>(colw, c[8]);  lds_put_pair<5 * 16>(colw, c[9]);   lds_put_pair<6 * 16>(colw, c[10]);  lds_put_clipped<7 * 16>(colw, c[11]);
                        lds_put_clipped<8 * 16>(colw, c[12]); lds_put_pair<9 * 16>(colw, c[13]);  lds_put_pair<10 * 16>(colw, c[14]); lds_put_clipped<11 * 16>(colw, c[15]);
                        lds_put_clipped<12 * 16>(colw, c[16]); lds_put_pair<13 * 16>(colw, c[17]); lds_put_pair<14 * 16>(colw, c[18]);
                    }
                    // chroma: columns cr, cr+1 of plane cp; only rows -1, 0, 3, 4 can change
                    const uint8_t *ctop = (const uint8_t *)ring + 64 + cp * 16 + cr;
                    uint8_t *ccol = tile8 + 256 + cp * 64 + cr;
                    pk16 d[10];
#pragma unroll
                    for (int r = 0; r < 2; r++) { uint32_t v = *(const uint16_t *)(ctop + r * 8); d[r] = as_pk(perm(v, v, 0x0c010c00u)); }
#pragma unroll
                    for (int r = 0; r < 8; r++) { uint32_t v = *(const uint16_t *)(ccol + r * 8); d[2 + r] = as_pk(perm(v, v, 0x0c010c00u)); }
#pragma unroll
                    for (int ed = 0; ed < 4; ed += 2) {
                        const int b = E.code(1, ed, cseg2), k = edge_class(1, ed) + 3;
                        if (__ballot(b != 0) == 0) continue;
                        const EdgeParams ep(Ec, k);
                        const pk16 A = as_pk(ep.alpha2()), B = as_pk(ep.beta2());
                        pk16 e;
                        const pk16 f = pk_edge_flag(d[2*ed], d[2*ed+1], d[2*ed+2], d[2*ed+3], A, as_pk(ep.nalpha2()), B, as_pk(ep.nbeta2()), e);
                        pk_chroma(d[2*ed], d[2*ed+1], d[2*ed+2], d[2*ed+3], e, f, as_pk(mask_bs123(b, ed)), as_pk(ed == 0 ? mask_bs4(b) : 0u), ed == 0 && __ballot(b == 3) != 0, as_pk(ep.tc2(b)));
                    }
                    // (all four are p0 / q0 rows: clipped here)
                    lds_put_clipped<8>((uint8_t *)ring + 64 + cp * 16 + cr, d[1]);
                    lds_put_clipped<0>(ccol, d[2]);
                    lds_put_clipped<3 * 8>(ccol, d[5]);
                    lds_put_clipped<4 * 8>(ccol, d[6]);
                }
                wave_lds_fence();
            }
            // the last four columns of this macroblock are the next one's columns -4..-1
            if (act) { ya0 = tYa[3]; yb0 = tYb[3]; ca0 = tCa[1]; cb0 = tCb[1]; }
            wave_lds_fence();
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (publisher) __hip_atomic_store(my_progress, g.mb_w, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        wave_lds_fence();
    }
}
#endif   // DEBLOCK_CR
