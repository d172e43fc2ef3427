// launch_plan.h - what a batch launches, decided in one place: plan_launches() is a pure function of the device (geometry, compute
// units, work-list layout), the P264AMD_* knobs, what kinds of picture the batch holds and the batch size.  p264hip_reconstruct
// (p264hip.hip) fills a BatchKinds, asks for the plan and issues it: one switch per stage, nothing decided there.
// Plain C++, no HIP: tests/test_launch_plan_cpu.py runs it without a GPU against what the GPU recorded.
#pragma once
#include <stdlib.h>
#include "p264hip.h"                 // (p264hip_launch_info_t)
#include "launch_shared.h"

// What the batch holds - the kernel instances and launch shapes follow from it: any picture with inter macroblocks / any B picture /
// any I picture / any explicit weights / any unweighted P picture whose list 0 holds one frame at several indices / any picture
// whose inter macroblocks may use the 8x8 transform / any picture whose Intra4x4 records may carry P264_MB_I8X8; sc: how many
// pictures take the scaled road (scaling_lists, or a Cr QP offset of its own); cr: any picture with a non-zero cr_qp_offset_delta (sc
// counts it) and n_cr: how many.  (As batch_fill fills it, wp, dup and t8 come with p: only pictures with inter macroblocks set them.)
struct BatchKinds { bool p = false, b = false, i = false, wp = false, dup = false, t8 = false, i8 = false; int sc = 0; bool cr = false; int n_cr = 0; };

// tuning knobs, read from the environment ONCE per context (p264hip_create); 0 (bs_fused, odd_single, mc_band_log2: -1) = built-in
// choice.  The values are kept as read; the shapes ignore what is out of their range.
struct LaunchKnobs {
    int mc_wgs = 0, intra_waves = 0, rb_log2 = 0, pics_per_wg = 0, db_waves = 0, bs_fused = -1, odd_single = -1;
    int mc_band_log2 = -1;           // P264AMD_MC_BAND_LOG2: macroblock rows per locality band of the work lists, 0 .. 9
};
// get: getenv, or anything that answers like it
template <class Getenv>
static inline LaunchKnobs launch_knobs_read(Getenv get)
{
    LaunchKnobs k;
    if (const char *env = get("P264AMD_MC_BAND_LOG2")) k.mc_band_log2 = atoi(env);
    if (const char *env = get("P264AMD_MC_WGS_PER_PIC")) k.mc_wgs = atoi(env);
    if (const char *env = get("P264AMD_INTRA_WAVES")) k.intra_waves = atoi(env);
    if (const char *env = get("P264AMD_DEBLOCK_RB_LOG2")) k.rb_log2 = atoi(env);
    if (const char *env = get("P264AMD_DEBLOCK_ODD_SINGLE")) k.odd_single = atoi(env) != 0;   /* 0: never, 1: whenever the shape allows it */
    if (const char *env = get("P264AMD_DEBLOCK_PICS_PER_WG")) k.pics_per_wg = atoi(env);
    if (const char *env = get("P264AMD_DEBLOCK_WAVES")) k.db_waves = atoi(env);
    if (const char *env = get("P264AMD_BS_FUSED")) { k.bs_fused = atoi(env); if (k.bs_fused > 16) k.bs_fused = 16; }   // 0: own launch; n: n edge-info workgroups per picture in the k_intra_sparse launch
    return k;
}

struct LaunchDevice { int mb_w = 0, mb_h = 0, n_cu = 256; McLayout ml = {}; };
static inline LaunchDevice launch_device(int mb_w, int mb_h, int n_cu, const LaunchKnobs &knobs)
{
    LaunchDevice d;
    d.mb_w = mb_w; d.mb_h = mb_h; d.n_cu = n_cu;
    // locality band of the motion-compensation lists: 16 macroblock rows unless that makes more than MC_MAX_BANDS bands
    int band_log2 = 4;
    if (knobs.mc_band_log2 >= 0 && knobs.mc_band_log2 <= 9) band_log2 = knobs.mc_band_log2;
    while (((mb_h + (1 << band_log2) - 1) >> band_log2) > MC_MAX_BANDS) band_log2++;
    d.ml = mc_layout(mb_w, mb_h, band_log2);
    return d;
}

// The kernel instance of each stage (kernel_mc_sort.h; kernel_mc.h; kernel_t8x8.h, kernel_scaling.h; kernel_intra.h; kernel_deblock.h)
enum class SortKernel { none, plain, wp, b, b_wp, scaled, scaled_p };
enum class McKernel { none, plain, wp };
enum class ResidualKernel { none, t8x8, scaled_inter };                                       // the launch that adds residuals in place behind the inter launches
enum class IntraKernel { dense, sparse, dense_i8, sparse_i8, dense_scaled, sparse_scaled };   // dense: k_intra*, sparse: k_intra_sparse*
enum class EdgeInfoRoad { fused, bs_by_index, bs_by_picture };                                // inside the k_intra_sparse launch / k_deblock_bs<false> / k_deblock_bs<true>

struct LaunchShape { unsigned grid_x = 0, grid_y = 1, threads = 0; };       // workgroups (x, y) and threads per workgroup

struct LaunchPlan {
    SortKernel sort = SortKernel::none;             LaunchShape sort_shape;
    McKernel mc = McKernel::none; bool mc_second = false; LaunchShape mc_shape;       // (k_mc_second: the shape of the first pass)
    int mc_wgs_total = 0; uint32_t mc_inv_wgs = 0;  // k_mc's arguments beside info.mc_wgs_per_picture: workgroups in use, 2^32 / workgroups per picture
    ResidualKernel residual = ResidualKernel::none; LaunchShape residual_shape;
    IntraKernel intra = IntraKernel::sparse;        LaunchShape intra_shape;          // (dynamic LDS: info.intra_waves x sizeof(IntraLds))
    EdgeInfoRoad edge = EdgeInfoRoad::bs_by_index;  LaunchShape edge_shape;           // (fused: no launch of its own)
    LaunchShape deblock_shape;
    bool copy_scale_table = false;                  // the batch's ScaleDev array travels to the device
    p264hip_launch_info_t info = {};                // what p264hip_last_launch reports of the batch
    bool deblock_cr = false;                        // the Cr instances of the loop filter's two launches (k_deblock_bs_cr, k_deblock_cr: kernel_deblock.h, K4c)
};

// k_mc: every picture gets the same number of workgroups, which split into the four roles on the device.  Enough workgroups per
// picture to fill the chip a few times over, no more than there can be chunks (four wavefronts per workgroup, one chunk per
// wavefront pass).
static inline int mc_wgs_per_picture(const LaunchDevice &dev, const LaunchKnobs &knobs, int n)
{
    int wgs = (dev.n_cu * 48 + n - 1) / n;   // (a dozen rounds of workgroups on small batches.  Round 5, 256 pictures per launch: 48 / 64 / 96 / 128 / 192 / 256
                                       //  per picture -> 0.685 / 0.687 / 0.691 / 0.704 / 0.724 / 0.751 ms for the stage - a wavefront's first chunk has no prefetch)
    if (wgs < 48) wgs = 48;            // (2048 pictures: 24 / 32 / 48 / 64 / 96 per picture -> 5.34 / 5.31 / 5.24 / 5.31 / 5.34 ms; with 24 the stage's reads grew by half:
                                       //  a picture's roles drift apart and stop sharing reference lines in L2)
    int max_wgs = 0;
    for (int l = 0; l < ML_LISTS; l++) max_wgs += (int)(dev.ml.max_chunks[l] + 3) / 4;
    if (wgs > max_wgs) wgs = max_wgs;
    if (knobs.mc_wgs >= 4 && knobs.mc_wgs <= max_wgs) wgs = knobs.mc_wgs;
    return wgs < 4 ? 4 : wgs;
}

// k_intra / k_intra_sparse, one workgroup per picture and role: 16 wavefronts while every picture can have a CU to itself, else 8 or
// 4 so that two or four pictures share a CU (measured +19 % at 512 and +9 % at 1024 pictures; 2048: 2 / 4 / 8 / 16 -> 1.02 / 0.87 /
// 0.90 / 1.10 ms)
static inline int intra_waves(const LaunchDevice &dev, const LaunchKnobs &knobs, int n)
{
    if (knobs.intra_waves >= 1 && knobs.intra_waves <= INTRA_ROW_WAVES) return knobs.intra_waves;
    return n > 2 * dev.n_cu ? INTRA_ROW_WAVES / 4 : n > dev.n_cu ? INTRA_ROW_WAVES / 2 : INTRA_ROW_WAVES;
}

// edge-info workgroups per picture inside the k_intra_sparse launch (P pictures only, by index: no B picture, no explicit weights,
// no frame twice in a list, no 8x8 transform - the fused role is compiled without its edge mask), 0: the pass takes its own launch
// (k_deblock_bs)
static inline int edge_info_fused(const LaunchKnobs &knobs, const BatchKinds &k)
{
    if (k.i || k.b || k.wp || k.dup || k.t8 || k.i8 || k.sc || knobs.bs_fused == 0) return 0;
    return knobs.bs_fused > 0 ? knobs.bs_fused : INTRA_BS_WGS;
}

static inline void deblock_shape(const LaunchDevice &dev, const LaunchKnobs &knobs, int n, p264hip_launch_info_t *li)
{
    const int mb_w = dev.mb_w, mb_h = dev.mb_h;
    // pictures per workgroup = as many as it takes to cover the batch with one workgroup per CU (a second, half-empty round
    // of workgroups costs more than sharing a workgroup: 1280 pictures as 320 workgroups of 4 took 5.35 ms, as 256 of 5 ...)
    int per_wg = (n + dev.n_cu - 1) / dev.n_cu;
    if (per_wg < 1) per_wg = 1;
    if (per_wg > MAX_PICS_PER_WG) per_wg = MAX_PICS_PER_WG;
    // bands of 8 rows of one picture per wavefront while every picture has a CU to itself, else 4 rows of two pictures; a
    // workgroup with more pictures than a wavefront holds (8 >> rb_log2) works on them in groups (units = band x group).
    // (Round 4: 2 rows x 4 pictures ran as fast, 2.70 ms, but every second row's bottom lines cross a band - 0.4 GB more
    // through memory per launch.)
    // Which shape: the stage's time follows the wavefront-iterations it issues (round 5: 1.07 ms per 16 units of 127 iterations at
    // 2 ... 15 pictures per workgroup, half-empty units included - it is bound by vector-instruction issue).  Bands of 4 rows hold
    // two pictures per wavefront: an odd picture count leaves one unit in every band half empty; bands of 8 rows hold one picture,
    // but run 8 iterations longer and the last band of a 68-row picture is half empty.  Take the cheaper one.
    auto units_cost = [&](int lg) {
        const int rows = 1 << lg, pw = 8 >> lg;
        const long bands = (mb_h + rows - 1) / rows, groups = (per_wg + pw - 1) / pw;
        return bands * groups * (long)(mb_w + 1 + DB_LAG * (rows - 1));
    };
    int rb_log2 = units_cost(3) < units_cost(2) ? 3 : 2;
    // an odd number (>= 3) of pictures: the pairs in bands of 4 rows, the last picture alone in bands of 8 (k_deblock, odd_single)
    const long cost_mixed = (per_wg >= 3 && (per_wg & 1)) ? ((mb_h + 3) / 4) * (long)(per_wg / 2) * (mb_w + 1 + 3 * DB_LAG) + ((mb_h + 7) / 8) * (long)(mb_w + 1 + 7 * DB_LAG) : -1;
    int odd_single = cost_mixed >= 0 && cost_mixed < units_cost(rb_log2);
    if (odd_single) rb_log2 = 2;
    if (knobs.rb_log2 >= 1 && knobs.rb_log2 <= 3) { rb_log2 = knobs.rb_log2; odd_single = 0; }
    if (knobs.pics_per_wg >= 1 && knobs.pics_per_wg <= MAX_PICS_PER_WG) { per_wg = knobs.pics_per_wg; odd_single = 0; }
    if (knobs.odd_single >= 0) odd_single = knobs.odd_single && rb_log2 == 2 && per_wg >= 3 && (per_wg & 1);
    const int n_bands = (mb_h + (1 << rb_log2) - 1) >> rb_log2;
    const int n_units = !odd_single ? n_bands * ((per_wg + (8 >> rb_log2) - 1) / (8 >> rb_log2)) : n_bands * (per_wg / 2) + (mb_h + 7) / 8;
    int waves = n_units < ROW_WAVES ? n_units : ROW_WAVES;
    if (knobs.db_waves >= 1 && knobs.db_waves < waves) waves = knobs.db_waves;
    li->deblock_pics_per_wg = per_wg; li->deblock_rb_log2 = rb_log2; li->deblock_waves = waves; li->deblock_wgs = (n + per_wg - 1) / per_wg;
    li->deblock_odd_single = odd_single;
}

// The plan of a batch of n pictures.  Each instance rule is written here, once; the stages are in stream order.
static inline LaunchPlan plan_launches(const LaunchDevice &dev, const LaunchKnobs &knobs, const BatchKinds &k, int n)
{
    LaunchPlan pl;
    p264hip_launch_info_t &li = pl.info;
    const int n_mb = dev.mb_w * dev.mb_h;
    const bool scaled = k.sc != 0;     // a picture with scaling_lists: every stage runs the instances that know the table
    li.pictures = n; li.compute_units = dev.n_cu; li.scaled_pictures = k.sc;
    pl.copy_scale_table = scaled;

    // motion compensation + residual of all inter macroblocks: the sort, then one launch for luma / chroma, macroblock / quadrant items
    if (k.p) {
        // (a scaled batch: the instance that files a scaled picture's residuals as absent - two of them, k_mc_sort's shape for batches
        // of unweighted P and I pictures, the two-list weighted one for every other; explicit weighted prediction in the batch: the
        // instances that route such pictures to the weighted class, kernel_mc_sort.h)
        pl.sort = scaled ? ((k.b || k.wp) ? SortKernel::scaled : SortKernel::scaled_p)
                : k.b ? (k.wp ? SortKernel::b_wp : SortKernel::b) : (k.wp ? SortKernel::wp : SortKernel::plain);
        pl.sort_shape = LaunchShape{ (unsigned)n, 1, MC_SORT_THREADS };
        // (a batch with explicit weighted prediction somewhere: the instance with the weighted generic class, kernel_mc.h: k_mc_wp)
        pl.mc = k.wp ? McKernel::wp : McKernel::plain;
        // B pictures: the blocks that predict from both lists get their second prediction (and their residual) in a second pass
        pl.mc_second = k.b;
        const int wgs = li.mc_wgs_per_picture = mc_wgs_per_picture(dev, knobs, n);
        pl.mc_shape = LaunchShape{ (unsigned)(((size_t)wgs * n + 7) / 8 * 8), 1, 256 };
        pl.mc_wgs_total = wgs * n;
        pl.mc_inv_wgs = (uint32_t)(((1ull << 32) - 1) / (unsigned)wgs);
        // the residuals the sort filed as absent, added in place in front of the intra launch (whose macroblocks predict from their
        // inter neighbours' finished samples): a scaled batch's k_scaled_inter owns the 8x8 blocks of all its pictures - no k_t8x8 beside it
        if (scaled) {
            pl.residual = ResidualKernel::scaled_inter;
            pl.residual_shape = LaunchShape{ (unsigned)((n_mb + T8_MBS_PER_WG - 1) / T8_MBS_PER_WG), (unsigned)n, T8_THREADS };
        } else if (k.t8) {
            pl.residual = ResidualKernel::t8x8;
            pl.residual_shape = LaunchShape{ (unsigned)((n_mb + T8_MBS_PER_WG - 1) / T8_MBS_PER_WG), (unsigned)n, T8_THREADS };
            li.t8x8_wgs = (int32_t)pl.residual_shape.grid_x * n;
        }
    }

    // intra: luma and chroma of a picture are independent chains - as two workgroups they run side by side.  Dense (a batch with an
    // I picture): grid (picture, role); sparse (P / B pictures only): picture x role in one dimension.  The scaled instances know
    // Intra 8x8; only the plain sparse instance carries the loop filter's edge info, in bs_wgs extra workgroups per picture.
    const int waves = li.intra_waves = intra_waves(dev, knobs, n);
    const int bs_wgs = li.edge_info_fused = edge_info_fused(knobs, k);
    li.intra_i8 = k.i8 ? 1 : 0;
    pl.intra = scaled ? (k.i ? IntraKernel::dense_scaled : IntraKernel::sparse_scaled)
             : k.i8 ? (k.i ? IntraKernel::dense_i8 : IntraKernel::sparse_i8) : (k.i ? IntraKernel::dense : IntraKernel::sparse);
    pl.intra_shape = k.i ? LaunchShape{ (unsigned)n, 2, (unsigned)waves * 64 } : LaunchShape{ (unsigned)n * (2 + (unsigned)bs_wgs), 1, (unsigned)waves * 64 };

    // edge info (boundary strengths, averaged QPs per edge class): explicit weighted prediction, a P list with one frame twice, B
    // pictures: the two-list instance, which compares reference pictures rather than indices - kernel_deblock.h
    pl.edge = (k.b || k.wp || k.dup) ? EdgeInfoRoad::bs_by_picture : bs_wgs > 0 ? EdgeInfoRoad::fused : EdgeInfoRoad::bs_by_index;
    if (pl.edge != EdgeInfoRoad::fused) pl.edge_shape = LaunchShape{ (unsigned)((n_mb + 255) / 256), (unsigned)n, 256 };

    deblock_shape(dev, knobs, n, &li);
    pl.deblock_shape = LaunchShape{ (unsigned)li.deblock_wgs, 1, (unsigned)li.deblock_waves * 64 };
    // a picture whose Cr has a QP offset of its own: the instances that carry Cr's averaged QPs beside the EdgeInfo, same roads and
    // shapes (never fused: such a batch is a scaled one, edge_info_fused)
    pl.deblock_cr = k.cr;
    li.cr_pictures = k.n_cr;
    return pl;
}
