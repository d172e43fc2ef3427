// p264hip.hip - host side of the C ABI in include/p264hip.h: device context, frame stores,
// resident picture inputs, batch launch of the reconstruction kernels, timing hooks.
//
// One context = one GPU = one HIP stream.  The product has no CPU reconstruction path: when no
// device is usable every entry point fails with P264HIP_ENODEV.
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <stdarg.h>
#include <vector>
#include <mutex>
#include <unordered_map>
#include "p264hip.h"
#include "device_common.h"
#include "launch_plan.h"                    // (BatchKinds, LaunchKnobs, LaunchDevice with its McLayout, plan_launches: what a batch launches)
#define P264HIP_K_DEBLOCK_DECL_ONLY          // k_deblock lives in k_deblock.hip (its own compiler options: kernel_deblock.h)
#include "kernel_deblock.h"
#include "kernel_mc_sort.h"                 // (MCE_W_SHIFT, MCE_MAX_MB_W, the k_mc_sort* kernels)
#include "kernel_mc.h"
#include "kernel_intra.h"
#include "kernel_t8x8.h"
#include "kernel_scaling.h"
#include "kernel_expand.h"
#include "kernel_export.h"
#include "kernel_resize.h"
#include "kernel_resize_aa.h"
#include "kernel_roi.h"
#include "kernel_roi_aa.h"
#include "kernel_roi_dev.h"

static thread_local char g_err[512] = "";
static int fail(int code, const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap);
    return code;
}
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(P264HIP_EHIP, "%s: %s", #x, hipGetErrorString(e_)); } while (0)

extern "C" const char *p264hip_last_error(void) { return g_err; }

extern "C" int p264hip_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

extern "C" int p264hip_build_info(void)
{
    return 0;                              // (bit 0, P264HIP_BUILD_TIMING, is reserved: include/p264hip.h)
}

static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// What an input slot holds.  Every road into a slot leaves it in exactly one state (from -> to):
//   p264hip_upload / _upload_async / _upload_packed: any -> READY     p264hip_upload_compact: any -> STAGED (appended to c->pending)
//   expand_pending: STAGED -> READY, or EMPTY when the expansion could not be queued
//   p264hip_input_reserve: any -> RESERVED                            p264hip_input_commit: RESERVED -> UNCHECKED
//   p264hip_clone_picture (dst): any -> the source's READY / UNCHECKED   p264hip_reconstruct: UNCHECKED -> READY, or EMPTY for a bad block
// A road that fails once it has started to rewrite a slot leaves it EMPTY.  Reconstruct and clone read the slots that hold a
// picture, state >= STAGED (expand_pending turns every STAGED one READY first).
enum SlotState : uint8_t { EMPTY, RESERVED, STAGED, UNCHECKED, READY };

struct PicSlot {                       // one device-resident parsed picture
    uint8_t *dev = nullptr;
    size_t   cap = 0;                  // bytes allocated
    p264hip_input_layout_t L = {};     // where the arrays lie in dev, and the bytes in use
    p264hip_picture_t meta;            // scalar fields only; pointers unused
    SlotState state = EMPTY;
    uint8_t *stage = nullptr; size_t stage_cap = 0;   // p264hip_upload_compact: the compact block as it arrived (STAGED: its expansion into dev has not been launched yet)
    uint64_t last_use{};                         // epoch of the last work queued on the context's stream that reads or writes the block
};

#define BATCH_RING 4
#define COPY_STREAMS 4

// device frame layout (strips, device_common.h) <-> planar staging (host boundary only): one thread per dword of the frame
__global__ void k_tile_convert(uint8_t *frame, uint8_t *planar, Geom g, int to_planar)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.n_mb * 96) return;
    const int mb = i / 96, d = i - mb * 96;
    const int mx = mb % g.mb_w, my = mb / g.mb_w;
    size_t po, fo;
    if (d < 64) {
        po = (size_t)(my * 16 + (d >> 2)) * g.w + mx * 16 + (d & 3) * 4;
        fo = mb_luma_off(g, mx, my) + d * 4;
    } else {
        const int e = d - 64, p = e >> 4, r = (e >> 1) & 7, dd = e & 1;
        po = (size_t)g.w * g.h + (size_t)p * g.cw * g.ch + (size_t)(my * 8 + r) * g.cw + mx * 8 + dd * 4;
        fo = mb_chroma_off(g, mx, my) + r * 16 + p * 8 + dd * 4;
    }
    uint32_t *t = (uint32_t *)(frame + fo), *q = (uint32_t *)(planar + po);
    if (to_planar) *q = *t; else *t = *q;
}

// The device twin of p264hip_records_check (csrc/host/input_layout.c), for pictures that arrive in device memory
// (p264hip_input_reserve / _commit): every macroblock's packed blocks must lie inside coefs[] - the kernels index the coefficient
// stream without further checks (include/p264hip.h).  One flag per input slot.
__global__ void k_check_records(const p264hip_mb_t *mb, int n_mb, uint32_t n_coef_blocks, int t8x8, int *bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_mb) return;
    const uint4 r = gload4(mb + i);
    if (r.y && (uint64_t)r.z + (uint64_t)__popc(r.y & 0x3ffffffu) > (uint64_t)n_coef_blocks) atomicOr(bad, 1);
    if ((r.x & 255u) == P264_MB_IPCM && r.y != P264_IPCM_COEF_MASK) atomicOr(bad, 1);       // (the intra kernels read twelve blocks of samples)
    // P264_MB_T8X8: in pictures that say so, inter, whole luma nibbles (k_t8x8 reads four entries per set nibble)
    if ((r.x >> 24) & P264_MB_T8X8) { if (!(t8x8 & ~P264_T8X8_INTRA) || P264_MB_IS_INTRA(r.x & 255u) || (r.y & 0xffffu) != (r.y & 0x1111u) * 15u) atomicOr(bad, 1); }
    // P264_MB_I8X8: in pictures that say so, I4x4, whole luma nibbles, not beside P264_MB_T8X8 (the Intra 8x8 instances of the intra kernels read four entries per set nibble)
    if ((r.x >> 24) & P264_MB_I8X8) { if (!(t8x8 & P264_T8X8_INTRA) || (r.x & 255u) != P264_MB_I4x4 || ((r.x >> 24) & P264_MB_T8X8) || (r.y & 0xffffu) != (r.y & 0x1111u) * 15u) atomicOr(bad, 1); }
}

struct p264hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    Geom g;
    int n_streams = 0, slots = 0, max_pictures = 0;
    uint8_t *frames = nullptr;
    size_t frame_bytes = 0;
    std::vector<PicSlot> pics;
    PicDev *h_batch[BATCH_RING] = {}, *d_batch[BATCH_RING] = {};
    // pictures with scaling_lists or a cr_qp_offset_delta: one ScaleDev per picture of the batch beside its PicDev (copied only for batches that hold such a
    // picture), and the all-16 table the batch's flat pictures point to
    ScaleDev *h_scale[BATCH_RING] = {}, *d_scale[BATCH_RING] = {};
    uint8_t *d_flat16 = nullptr;
    hipEvent_t batch_free[BATCH_RING] = {};
    int batch_cap = 0, ring = 0;
    int *d_status = nullptr;
    int *d_slot_bad = nullptr;             // [max_pictures]: k_check_records' verdict per input slot
    std::vector<int> pending;              // the STAGED input slots, in upload order: k_expand_compact's jobs (launched in front of the next reconstruct / clone / sync)
    ExpandJob *h_jobs = nullptr, *d_jobs = nullptr; int jobs_cap = 0; hipEvent_t jobs_free = nullptr;
    // compact blocks travel on COPY_STREAMS side streams, slot % COPY_STREAMS (two copies into one staging area on two streams would
    // land in any order): a copy of ~0.5 MB costs ~18 us of fixed latency beside ~9 us of transfer (measured, round 6: 512 copies per
    // step on the context's one stream ran at 19.6 GB/s) - side by side the latencies overlap.
    // The expansion kernel (context's stream) waits for the side streams' copies; a side stream waits for the last expansion before it
    // overwrites a staging area.
    hipStream_t cstream[COPY_STREAMS] = {}; hipEvent_t cdone[COPY_STREAMS] = {}; bool cdirty[COPY_STREAMS] = {}, cwaited[COPY_STREAMS] = {};
    hipEvent_t expand_done = nullptr;
    uint64_t upload_copies = 0;            // host -> HBM copies queued by p264hip_upload / _upload_async (one per picture whose arrays lie like a slot)
    uint64_t epoch = 0, done_epoch = 0;    // work queued on the stream / known to have completed (a slot is free for a new producer once its last_use is done)
    EdgeInfo *d_edge = nullptr;            // [batch_cap][n_mb], scratch between k_deblock_bs and k_deblock
    uint32_t *d_edge_cr = nullptr;         // [batch_cap][n_mb], Cr's averaged QPs beside it (k_deblock_bs_cr -> k_deblock_cr); from the first batch with a cr_qp_offset_delta
    uint32_t *d_mc = nullptr;              // [batch_cap][dev.ml.words], motion-compensation work lists (k_mc_sort -> k_mc, k_mc_second)
    uint8_t *d_is_intra = nullptr;         // [batch_cap][n_mb], 1 = intra macroblock (k_mc_sort -> k_intra's collect pass; P / B pictures)
    // what the launch plan is a function of, beside the batch (launch_plan.h): the P264AMD_* tuning knobs, read from the environment
    // ONCE (p264hip_create), and geometry, compute units and work-list layout
    LaunchKnobs knobs;
    LaunchDevice dev;
    std::vector<int> stream_seen;          // p264hip_reconstruct: batch index + 1 that last named a stream in the current call
    uint8_t *d_planar = nullptr;           // planar staging for p264hip_read_frame / p264hip_write_frame
    std::vector<uint8_t *> planar_pool;    // p264hip_frame_planar_device: planar I420 frames that stay on the device
    // p264hip_export_frames: the frame index (stream * slots + slot) of every picture of a call, a ring like the batch's
    uint32_t *h_exp[BATCH_RING] = {}, *d_exp[BATCH_RING] = {}; hipEvent_t exp_free[BATCH_RING] = {}; int exp_cap = 0, exp_ring = 0;
    uint32_t *d_roi = nullptr; size_t roi_cap = 0;          // the tap scratch of p264hip_export_rois (kernel_roi.h), bytes
    // p264hip_export_rois_device: the descriptors k_roi_plan writes (kernel_roi_dev.h), bytes, and the events of its two stream orders
    RoiDev *d_roi_tab = nullptr; size_t roi_tab_cap = 0; hipEvent_t roi_after = nullptr, roi_before = nullptr;
    p264hip_launch_info_t last = {};       // what the last p264hip_reconstruct launched
    hipEvent_t markers[P264HIP_MARKERS] = {};
    int next_marker = 0;
    bool timing = false;
    struct Stamp { hipEvent_t a, b; int k; };
    std::vector<Stamp> stamps;
    std::vector<hipEvent_t> event_pool;
    double ms_sum[P264HIP_NKERNELS] = {};
    int64_t ms_cnt[P264HIP_NKERNELS] = {};
};

static uint8_t *frame_ptr(p264hip_ctx *c, int stream, int slot)
{
    return c->frames + ((size_t)stream * c->slots + slot) * c->frame_bytes;
}

extern "C" int p264hip_create(p264hip_ctx **out, int device, int mb_w, int mb_h, int n_streams, int slots, int max_pictures)
{
    if (!out || mb_w < 1 || mb_w > MCE_MAX_MB_W || mb_h < 1 || mb_h > MAX_MB_ROWS ||    /* (the column and row fields of a work-list entry, kernel_mc_sort.h) */
        n_streams < 1 || slots < 1 || slots > P264HIP_MAX_REFS + 1 || max_pictures < 1)
        return fail(P264HIP_EINVAL, "p264hip_create: bad argument (mb %dx%d, streams %d, slots %d, pictures %d)", mb_w, mb_h, n_streams, slots, max_pictures);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(P264HIP_ENODEV, "no HIP device available: the MI355X reconstruction path cannot run (there is no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(P264HIP_EINVAL, "device %d out of range (have %d)", device, ndev);
    HIPCHK(hipSetDevice(device));
    p264hip_ctx *c = new p264hip_ctx();
    c->device = device;
    c->n_streams = n_streams; c->slots = slots; c->max_pictures = max_pictures;
    Geom &g = c->g;
    g.mb_w = mb_w; g.mb_h = mb_h; g.n_mb = mb_w * mb_h;
    g.w = mb_w * 16; g.h = mb_h * 16; g.cw = g.w / 2; g.ch = g.h / 2;
    g.ystrip = (uint32_t)g.h * 16u; g.cstrip = (uint32_t)g.ch * 16u; g.coff = (uint32_t)g.n_mb * MB_LUMA_BYTES;
    c->frame_bytes = align_up((size_t)g.n_mb * (MB_LUMA_BYTES + MB_CHROMA_BYTES), 256);      // strip layout (device_common.h)
    // (one stream's store is addressed by 32-bit offsets through one buffer descriptor, and the kernels use MC_OOB as "an offset
    // beyond any store" for loads that must return zeros - kernel_mc.h: the store has to end at or below it)
    if (c->frame_bytes * (size_t)slots > (size_t)MC_OOB) { delete c; return fail(P264HIP_EINVAL, "frame store of one stream exceeds %u bytes (%d slots of %zu bytes)", MC_OOB, slots, c->frame_bytes); }
    c->stream_seen.assign((size_t)n_streams, 0);
    c->pics.resize((size_t)max_pictures);
    int n_cu = 256;
    { int v = 0; if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0) n_cu = v; }
    c->knobs = launch_knobs_read(getenv);
    c->dev = launch_device(mb_w, mb_h, n_cu, c->knobs);
    c->last.compute_units = n_cu;                           // (p264hip_last_launch before the first batch: the device's size)
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc((void **)&c->frames, c->frame_bytes * (size_t)n_streams * slots);
    if (e == hipSuccess) e = hipMemsetAsync(c->frames, 0, c->frame_bytes * (size_t)n_streams * slots, c->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_status, sizeof(int));
    if (e == hipSuccess) e = hipMemsetAsync(c->d_status, 0, sizeof(int), c->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_slot_bad, sizeof(int) * (size_t)max_pictures);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_slot_bad, 0, sizeof(int) * (size_t)max_pictures, c->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&c->d_flat16, 256);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_flat16, 16, 256, c->stream);                 // (Flat_4x4_16 / Flat_8x8_16: every weight 16)
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        int rc = fail(e == hipErrorOutOfMemory ? P264HIP_ENOMEM : P264HIP_EHIP, "p264hip_create: %s", hipGetErrorString(e));
        p264hip_destroy(c);
        return rc;
    }
    *out = c;
    return P264HIP_OK;
}

extern "C" void p264hip_destroy(p264hip_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    // (the side streams too, before any staging area goes: a compact block that was never expanded may still be on its way)
    for (int i = 0; i < COPY_STREAMS; i++) { if (c->cstream[i]) { (void)hipStreamSynchronize(c->cstream[i]); (void)hipStreamDestroy(c->cstream[i]); } if (c->cdone[i]) (void)hipEventDestroy(c->cdone[i]); }
    for (auto &p : c->pics) { if (p.dev) (void)hipFree(p.dev); if (p.stage) (void)hipFree(p.stage); }
    if (c->h_jobs) (void)hipHostFree(c->h_jobs);
    if (c->d_jobs) (void)hipFree(c->d_jobs);
    if (c->jobs_free) (void)hipEventDestroy(c->jobs_free);
    if (c->expand_done) (void)hipEventDestroy(c->expand_done);
    for (int i = 0; i < BATCH_RING; i++) {
        if (c->h_batch[i]) (void)hipHostFree(c->h_batch[i]);
        if (c->d_batch[i]) (void)hipFree(c->d_batch[i]);
        if (c->h_scale[i]) (void)hipHostFree(c->h_scale[i]);
        if (c->d_scale[i]) (void)hipFree(c->d_scale[i]);
        if (c->batch_free[i]) (void)hipEventDestroy(c->batch_free[i]);
    }
    for (int i = 0; i < BATCH_RING; i++) {
        if (c->h_exp[i]) (void)hipHostFree(c->h_exp[i]);
        if (c->d_exp[i]) (void)hipFree(c->d_exp[i]);
        if (c->exp_free[i]) (void)hipEventDestroy(c->exp_free[i]);
    }
    if (c->d_roi) (void)hipFree(c->d_roi);
    if (c->d_roi_tab) (void)hipFree(c->d_roi_tab);
    if (c->roi_after) (void)hipEventDestroy(c->roi_after);
    if (c->roi_before) (void)hipEventDestroy(c->roi_before);
    for (auto &s : c->stamps) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    if (c->frames) (void)hipFree(c->frames);
    if (c->d_edge) (void)hipFree(c->d_edge);
    if (c->d_edge_cr) (void)hipFree(c->d_edge_cr);
    if (c->d_mc) (void)hipFree(c->d_mc);
    if (c->d_is_intra) (void)hipFree(c->d_is_intra);
    if (c->d_planar) (void)hipFree(c->d_planar);
    for (uint8_t *p : c->planar_pool) if (p) (void)hipFree(p);
    for (auto &m : c->markers) if (m) (void)hipEventDestroy(m);
    if (c->d_status) (void)hipFree(c->d_status);
    if (c->d_slot_bad) (void)hipFree(c->d_slot_bad);
    if (c->d_flat16) (void)hipFree(c->d_flat16);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// arrays: the picture's host arrays are there to be checked too (false: only the descriptor - the arrays are already packed)
static int check_pic(p264hip_ctx *c, const p264hip_picture_t *p, bool arrays)
{
    if (p->mb_w != c->g.mb_w || p->mb_h != c->g.mb_h)
        return fail(P264HIP_EINVAL, "picture is %dx%d MBs, context is %dx%d", p->mb_w, p->mb_h, c->g.mb_w, c->g.mb_h);
    if (p->dst_slot < 0 || p->dst_slot >= c->slots) return fail(P264HIP_EINVAL, "dst_slot %d out of range", p->dst_slot);
    if (p->n_ref < 0 || p->n_ref > P264HIP_MAX_REFS) return fail(P264HIP_EINVAL, "n_ref %d out of range", p->n_ref);
    for (int i = 0; i < p->n_ref; i++)
        if (p->ref_slot[i] < 0 || p->ref_slot[i] >= c->slots) return fail(P264HIP_EINVAL, "ref_slot[%d]=%d out of range", i, p->ref_slot[i]);
    if (p->slice_type != P264_SLICE_P && p->slice_type != P264_SLICE_B && p->slice_type != P264_SLICE_I) return fail(P264HIP_EINVAL, "slice_type %d", p->slice_type);
    if (p->slice_type == P264_SLICE_P && p->n_ref < 1) return fail(P264HIP_EINVAL, "P picture without reference");
    if (p->slice_type == P264_SLICE_B) {
        if (p->n_ref < 1 || p->n_ref_l1 < 1 || p->n_ref_l1 > P264HIP_MAX_REFS) return fail(P264HIP_EINVAL, "B picture: list lengths %d / %d", p->n_ref, p->n_ref_l1);
        if (arrays && (!p->mv_l1 || !p->ref_idx_l1)) return fail(P264HIP_EINVAL, "B picture without list-1 arrays");
        if (p->n_coef_blocks >= (1u << MCE_W_SHIFT)) return fail(P264HIP_EINVAL, "B picture with %u coefficient blocks (limit %u: the second pass packs the weight beside the index)", p->n_coef_blocks, 1u << MCE_W_SHIFT);
        for (int i = 0; i < p->n_ref_l1; i++)
            if (p->ref_slot_l1[i] < 0 || p->ref_slot_l1[i] >= c->slots) return fail(P264HIP_EINVAL, "ref_slot_l1[%d]=%d out of range", i, p->ref_slot_l1[i]);
        if (p->weighted_bipred)
            for (int i = 0; i < P264HIP_MAX_REFS * P264HIP_MAX_REFS; i++)
                if (p->bipred_weight[i] < -64 || p->bipred_weight[i] > 128) return fail(P264HIP_EINVAL, "bipred_weight[%d]=%d out of range (-64 .. 128)", i, p->bipred_weight[i]);
    }
    if (p264hip_wp_check(p))
        return fail(P264HIP_EINVAL, "explicit weight table out of range (denominators %d / %d: 0 .. 7, weights -128 .. 128, offsets -128 .. 127, no implicit weights beside it, not in an I picture)",
                    p->wp_log2_denom[0], p->wp_log2_denom[1]);
    if (!arrays) return 0;
    if (!p->mb || !p->mv || !p->ref_idx || !p->i4modes || (p->n_coef_blocks && !p->coefs)) return fail(P264HIP_EINVAL, "null picture array");
    const int bad = (int)p264hip_records_check_pic(p, p->mb);
    if (bad < 0) return 0;
    const p264hip_mb_t &m = p->mb[bad];                       // which part of the rule the record breaks (the range first)
    const int blocks = __builtin_popcount(m.coef_mask & 0x3ffffffu);
    if (m.coef_mask && (uint64_t)m.coef_index + (uint64_t)blocks > p->n_coef_blocks)
        return fail(P264HIP_EINVAL, "macroblock %d: coefficient blocks [%u, +%d) outside coefs[%u]", bad, m.coef_index, blocks, p->n_coef_blocks);
    if (m.intra_modes & P264_MB_I8X8)
        return fail(P264HIP_EINVAL, "macroblock %d: P264_MB_I8X8 on a record of type %d with intra_modes 0x%x and coef_mask 0x%x in a picture with transform_8x8 = %d (I4x4 records with whole luma nibbles and without P264_MB_T8X8, in pictures that carry P264_T8X8_INTRA)",
                    bad, m.mb_type, m.intra_modes, m.coef_mask, p->transform_8x8);
    if (m.intra_modes & P264_MB_T8X8)
        return fail(P264HIP_EINVAL, "macroblock %d: P264_MB_T8X8 on a record of type %d with coef_mask 0x%x in a picture with transform_8x8 = %d (inter records with whole luma nibbles, in pictures that say so)",
                    bad, m.mb_type, m.coef_mask, p->transform_8x8);
    return fail(P264HIP_EINVAL, "macroblock %d: I_PCM with coef_mask 0x%x (its twelve sample blocks are 0x%x)", bad, m.coef_mask, P264_IPCM_COEF_MASK);
}

// The one way a context buffer grows (input slots, staging areas, clone destinations, job table, batch ring): the old buffer
// is freed after `wait` (what may still use it; WAIT_NONE: the caller has waited), then need + slack bytes of device memory -
// pinned: of host memory the device reads - replace it.  cap: the bytes held (nullptr: the caller has decided to grow).
enum Wait { WAIT_NONE, WAIT_STREAM, WAIT_DEVICE };
static int grow(p264hip_ctx *c, void **buf, size_t *cap, size_t need, size_t slack, bool pinned, Wait wait, const char *what)
{
    if (cap && need <= *cap) return 0;
    if (cap) *cap = 0;
    if (*buf) {
        HIPCHK(wait == WAIT_STREAM ? hipStreamSynchronize(c->stream) : wait == WAIT_DEVICE ? hipDeviceSynchronize() : hipSuccess);
        HIPCHK(pinned ? hipHostFree(*buf) : hipFree(*buf));
        *buf = nullptr;
    }
    const hipError_t e = pinned ? hipHostMalloc(buf, need + slack, hipHostMallocDefault) : hipMalloc(buf, need + slack);
    if (e != hipSuccess) { *buf = nullptr; return fail(P264HIP_ENOMEM, "%s(%zu) for %s: %s", pinned ? "hipHostMalloc" : "hipMalloc", need + slack, what, hipGetErrorString(e)); }
    if (cap) *cap = need + slack;
    return 0;
}

// Work that reads or writes slot s has been queued (or is about to be) under the context's current epoch: a later
// p264hip_input_reserve of the slot waits for the stream unless that epoch is known to be done.
static void stamp(p264hip_ctx *c, PicSlot &s) { s.last_use = c->epoch; }

// ---- the roads into a slot (include/p264hip.h) ----
// First step of every road with a new picture: argument, device, descriptor (arrays: its host arrays too), layout; the slot is untouched
static int slot_enter(p264hip_ctx *c, int id, const p264hip_picture_t *p, bool arrays, p264hip_input_layout_t *L, const char *who)
{
    if (!c || !p || id < 0 || id >= c->max_pictures) return fail(P264HIP_EINVAL, "%s: bad argument (slot %d)", who, id);
    HIPCHK(hipSetDevice(c->device));
    const int rc = check_pic(c, p, arrays);
    if (rc) return rc;
    return p264hip_input_layout(p, L) ? fail(P264HIP_EINVAL, "%s: picture layout", who) : 0;
}
// The slot starts to be rewritten: no picture until the road ends (a STAGED block drops out of c->pending); room for L + slack
static int slot_prepare(p264hip_ctx *c, int id, const p264hip_input_layout_t &L, size_t slack)
{
    PicSlot &s = c->pics[(size_t)id];
    if (s.state == STAGED)
        for (size_t i = 0; i < c->pending.size(); i++) if (c->pending[i] == id) { c->pending.erase(c->pending.begin() + (long)i); break; }
    s.state = EMPTY;
    s.L = L;
    return grow(c, (void **)&s.dev, &s.cap, L.bytes, slack, false, WAIT_STREAM, "picture input");
}
// Last step of every road: the picture's scalar fields, the slot's new state and the epoch of the work just queued on it.
static void slot_exit(p264hip_ctx *c, int id, const p264hip_picture_t &p, SlotState state)
{
    PicSlot &s = c->pics[(size_t)id];
    s.meta = p;
    s.meta.mb = nullptr; s.meta.mv = nullptr; s.meta.ref_idx = nullptr; s.meta.i4modes = nullptr; s.meta.coefs = nullptr; s.meta.mv_l1 = nullptr; s.meta.ref_idx_l1 = nullptr;
    if (state == STAGED) c->pending.push_back(id);
    s.state = state;
    ++c->epoch;
    stamp(c, s);
}

// ---- compact link format (include/p264hip.h, kernel_expand.h) ----
// ONE launch expands every compact block uploaded since the last one
static int expand_launch(p264hip_ctx *c)
{
    const int n = (int)c->pending.size();
    if (c->jobs_free) HIPCHK(hipEventSynchronize(c->jobs_free));        // the copy that last read h_jobs is done
    else HIPCHK(hipEventCreateWithFlags(&c->jobs_free, hipEventDisableTiming));
    if (n > c->jobs_cap) {
        const int cap = n + n / 2 + 16;
        c->jobs_cap = 0;
        int rc = grow(c, (void **)&c->h_jobs, nullptr, (size_t)cap * sizeof(ExpandJob), 0, true, WAIT_NONE, "the expansion jobs");
        if (rc || (rc = grow(c, (void **)&c->d_jobs, nullptr, (size_t)cap * sizeof(ExpandJob), 0, false, WAIT_NONE, "the expansion jobs"))) return rc;
        c->jobs_cap = cap;
    }
    // the kernel writes the slots' arrays: a later p264hip_input_reserve of one of them must wait for it
    ++c->epoch;
    for (int i = 0; i < n; i++) {
        PicSlot &s = c->pics[(size_t)c->pending[(size_t)i]];
        c->h_jobs[i] = ExpandJob{ s.stage, s.dev, (uint32_t)s.L.off_mv, (uint32_t)s.L.off_ref, (uint32_t)s.L.off_i4, (uint32_t)s.L.off_coef,
                                  (uint32_t)s.L.off_mv_l1, (uint32_t)s.L.off_ref_l1, (uint32_t)s.L.off_weights, (uint32_t)s.L.off_wp, (uint32_t)s.L.off_scaling };
        stamp(c, s);
    }
    for (int i = 0; i < COPY_STREAMS; i++) {                 // the blocks' copies (side streams) in front of the kernel that reads them
        if (!c->cdirty[i]) continue;
        HIPCHK(hipEventRecord(c->cdone[i], c->cstream[i]));
        HIPCHK(hipStreamWaitEvent(c->stream, c->cdone[i], 0));
        c->cdirty[i] = false;
    }
    HIPCHK(hipMemcpyAsync(c->d_jobs, c->h_jobs, (size_t)n * sizeof(ExpandJob), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->jobs_free, c->stream));
    hipLaunchKernelGGL(k_expand_compact, dim3((unsigned)n), dim3(EXPAND_THREADS), 0, c->stream, (const ExpandJob *)c->d_jobs);
    HIPCHK(hipGetLastError());
    if (!c->expand_done) HIPCHK(hipEventCreateWithFlags(&c->expand_done, hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->expand_done, c->stream));        // the staging areas may be overwritten behind this
    for (int i = 0; i < COPY_STREAMS; i++) c->cwaited[i] = false;
    return 0;
}
// STAGED -> READY once the expansion is queued; if it is not, the slots are EMPTY (a retried reconstruct reports them empty
// instead of decoding arrays that were never written)
static int expand_pending(p264hip_ctx *c)
{
    if (c->pending.empty()) return 0;
    const int rc = expand_launch(c);
    for (int id : c->pending) c->pics[(size_t)id].state = rc ? EMPTY : READY;
    c->pending.clear();
    return rc;
}

extern "C" int p264hip_upload_async(p264hip_ctx *c, int id, const p264hip_picture_t *p)
{
    p264hip_input_layout_t L;
    int rc = slot_enter(c, id, p, true, &L, "p264hip_upload_async");
    if (rc || (rc = slot_prepare(c, id, L, L.bytes / 4))) return rc;
    PicSlot &s = c->pics[(size_t)id];
    const size_t n = (size_t)c->g.n_mb;
    if (p->slice_type == P264_SLICE_B) {
        HIPCHK(hipMemcpyAsync(s.dev + L.off_mv_l1, p->mv_l1, n * 64, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s.dev + L.off_ref_l1, p->ref_idx_l1, n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s.dev + L.off_weights, p->bipred_weight, sizeof p->bipred_weight, hipMemcpyHostToDevice, c->stream));
    }
    // The caller's arrays already lie in host memory the way the slot is laid out (the parser builds its pictures like that since
    // round 6, csrc/host/parser.c: picbuf_t): ONE copy for records, vectors, indices, modes and levels instead of five - the
    // pipeline's uploads ran at 12 GB/s in pieces, a packed block goes at 35 (bench.py: extras.upload_inclusive).
    const uint8_t *hb = (const uint8_t *)p->mb;
    const bool as_slot = (const uint8_t *)p->mv == hb + L.off_mv && (const uint8_t *)p->ref_idx == hb + L.off_ref && (const uint8_t *)p->i4modes == hb + L.off_i4
                         && (p->n_coef_blocks == 0 || (const uint8_t *)p->coefs == hb + L.off_coef);
    if (as_slot) HIPCHK(hipMemcpyAsync(s.dev, hb, L.off_coef + (size_t)p->n_coef_blocks * 32, hipMemcpyHostToDevice, c->stream));
    else {
        HIPCHK(hipMemcpyAsync(s.dev, p->mb, n * sizeof(p264hip_mb_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s.dev + L.off_mv, p->mv, n * 64, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s.dev + L.off_ref, p->ref_idx, n * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s.dev + L.off_i4, p->i4modes, n * 16, hipMemcpyHostToDevice, c->stream));
        if (p->n_coef_blocks)
            HIPCHK(hipMemcpyAsync(s.dev + L.off_coef, p->coefs, (size_t)p->n_coef_blocks * 32, hipMemcpyHostToDevice, c->stream));
    }
    if (p->explicit_wp) HIPCHK(hipMemcpyAsync(s.dev + L.off_wp, p->wp, sizeof p->wp, hipMemcpyHostToDevice, c->stream));
    // (scaling4x4 and scaling8x8 lie back to back in the descriptor, as they do in the slot)
    static_assert(offsetof(p264hip_picture_t, scaling8x8) == offsetof(p264hip_picture_t, scaling4x4) + sizeof p->scaling4x4 && sizeof p->scaling4x4 + sizeof p->scaling8x8 == P264HIP_SCALING_BYTES, "the scaling table");
    if (p->scaling_lists) HIPCHK(hipMemcpyAsync(s.dev + L.off_scaling, p->scaling4x4, P264HIP_SCALING_BYTES, hipMemcpyHostToDevice, c->stream));
    c->upload_copies += (as_slot ? 1 : 5) + (p->explicit_wp ? 1 : 0) + (p->scaling_lists ? 1 : 0);
    slot_exit(c, id, *p, READY);
    return P264HIP_OK;
}

// ---- other ways into a slot (include/p264hip.h): a packed host block in one copy; a device producer (reserve / commit) ----
extern "C" int p264hip_upload_packed(p264hip_ctx *c, int slot, const p264hip_picture_t *desc, const void *packed, size_t bytes)
{
    if (!packed) return fail(P264HIP_EINVAL, "p264hip_upload_packed: null block");
    p264hip_input_layout_t L;
    int rc = slot_enter(c, slot, desc, false, &L, "p264hip_upload_packed");
    if (rc) return rc;
    if (bytes != L.bytes) return fail(P264HIP_EINVAL, "p264hip_upload_packed: %zu bytes, the layout has %zu", bytes, L.bytes);
    if (desc->explicit_wp) {                                 // the table the kernels will read is the block's: its ranges too
        p264hip_picture_t t = *desc;
        memcpy(t.wp, (const uint8_t *)packed + L.off_wp, sizeof t.wp);
        if (p264hip_wp_check(&t)) return fail(P264HIP_EINVAL, "p264hip_upload_packed: the block's explicit weight table is out of range");
    }
    if ((rc = slot_prepare(c, slot, L, L.bytes / 4))) return rc;
    HIPCHK(hipMemcpyAsync(c->pics[(size_t)slot].dev, packed, L.bytes, hipMemcpyHostToDevice, c->stream));
    slot_exit(c, slot, *desc, READY);
    return P264HIP_OK;
}

extern "C" int p264hip_upload_compact(p264hip_ctx *c, int slot, const p264hip_picture_t *desc, const void *compact, size_t bytes)
{
    if (!compact) return fail(P264HIP_EINVAL, "p264hip_upload_compact: null block");
    p264hip_input_layout_t L;
    int rc = slot_enter(c, slot, desc, false, &L, "p264hip_upload_compact");
    if (rc) return rc;
    if (!p264hip_compact_header_ok(desc, compact, bytes)) return fail(P264HIP_EINVAL, "p264hip_upload_compact: the block is not a consistent compact picture of %dx%d macroblocks with %u coefficient blocks", desc->mb_w, desc->mb_h, desc->n_coef_blocks);
    if ((rc = slot_prepare(c, slot, L, L.bytes / 4))) return rc;
    PicSlot &s = c->pics[(size_t)slot];
    if ((rc = grow(c, (void **)&s.stage, &s.stage_cap, bytes, bytes / 4, false, WAIT_DEVICE, "a compact picture"))) return rc;
    const int cs = slot % COPY_STREAMS;
    if (!c->cstream[cs]) {
        HIPCHK(hipStreamCreateWithFlags(&c->cstream[cs], hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->cdone[cs], hipEventDisableTiming));
    }
    if (!c->cwaited[cs]) {
        // the last expansion kernel (it read the staging areas) is in front of this side stream's copies; nothing else is - a
        // copy into a staging area never touches the slot's arrays, so step t + 1's blocks travel while step t is reconstructed
        if (c->expand_done) HIPCHK(hipStreamWaitEvent(c->cstream[cs], c->expand_done, 0));
        c->cwaited[cs] = true;
    }
    HIPCHK(hipMemcpyAsync(s.stage, compact, bytes, hipMemcpyHostToDevice, c->cstream[cs]));
    c->cdirty[cs] = true;
    c->upload_copies += 1;
    slot_exit(c, slot, *desc, STAGED);
    return P264HIP_OK;
}

extern "C" int p264hip_input_reserve(p264hip_ctx *c, int slot, const p264hip_picture_t *desc, void **dev, size_t *bytes)
{
    if (!dev || !bytes) return fail(P264HIP_EINVAL, "p264hip_input_reserve: null argument");
    p264hip_input_layout_t L;
    int rc = slot_enter(c, slot, desc, false, &L, "p264hip_input_reserve");
    if (rc) return rc;
    PicSlot &s = c->pics[(size_t)slot];
    // Whatever still reads or writes the slot's previous picture on the context's stream must be through before somebody else
    // writes it.  One wait covers everything queued so far: the first reserve of a round waits (if the last batch is still
    // running), the others find their slots' work already known to be done - not one hipStreamSynchronize per picture.
    if (s.last_use > c->done_epoch) { const uint64_t upto = c->epoch; HIPCHK(hipStreamSynchronize(c->stream)); c->done_epoch = upto; }
    if ((rc = slot_prepare(c, slot, L, L.bytes / 4))) return rc;
    slot_exit(c, slot, *desc, RESERVED);
    *dev = s.dev; *bytes = L.bytes;
    return P264HIP_OK;
}

extern "C" int p264hip_input_commit(p264hip_ctx *c, int slot)
{
    if (!c || slot < 0 || slot >= c->max_pictures || c->pics[(size_t)slot].state != RESERVED) return fail(P264HIP_EINVAL, "p264hip_input_commit: slot %d is not reserved", slot);
    PicSlot &s = c->pics[(size_t)slot];
    HIPCHK(hipSetDevice(c->device));
    // The producer wrote the arrays (it says they are complete on the device: include/p264hip.h); their records get the check
    // p264hip_upload runs on the host, on the device - a block from a peer that packed it wrongly must become an error, not
    // an out-of-bounds read.  The verdict is read once per batch, by p264hip_reconstruct.
    HIPCHK(hipMemsetAsync(c->d_slot_bad + slot, 0, sizeof(int), c->stream));
    const int n_mb = c->g.n_mb;
    hipLaunchKernelGGL(k_check_records, dim3((n_mb + 255) / 256), dim3(256), 0, c->stream, (const p264hip_mb_t *)s.dev, n_mb, s.meta.n_coef_blocks, s.meta.transform_8x8, c->d_slot_bad + slot);
    HIPCHK(hipGetLastError());
    slot_exit(c, slot, s.meta, UNCHECKED);
    return P264HIP_OK;
}

// ---- frames at the host boundary: the strip layout of the device <-> planar I420 ----
static size_t planar_bytes(const Geom &g) { return (size_t)g.w * g.h + 2 * (size_t)g.cw * g.ch; }
// frame (stream, slot) -> the planar device buffer (to_planar) or back, queued on the context's stream
static int tile_convert(p264hip_ctx *c, int stream, int slot, uint8_t *planar, bool to_planar)
{
    const int n_dw = c->g.n_mb * 96;
    hipLaunchKernelGGL(k_tile_convert, dim3((n_dw + 255) / 256), dim3(256), 0, c->stream, frame_ptr(c, stream, slot), planar, c->g, to_planar ? 1 : 0);
    HIPCHK(hipGetLastError());
    return 0;
}
// the context's one planar staging frame (p264hip_read_frame / _read_frame_async / _write_frame), allocated at its first use
static int planar_staging(p264hip_ctx *c)
{
    if (!c->d_planar) HIPCHK(hipMalloc((void **)&c->d_planar, planar_bytes(c->g)));
    return 0;
}

extern "C" int p264hip_frame_planar_device(p264hip_ctx *c, int stream, int slot, int index, void **dev, size_t *bytes)
{
    if (!c || !dev || !bytes || stream < 0 || stream >= c->n_streams || slot < 0 || slot >= c->slots || index < 0 || index >= 4096)
        return fail(P264HIP_EINVAL, "p264hip_frame_planar_device: bad argument (stream %d slot %d buffer %d)", stream, slot, index);
    HIPCHK(hipSetDevice(c->device));
    const size_t sz = planar_bytes(c->g);
    if ((size_t)index >= c->planar_pool.size()) c->planar_pool.resize((size_t)index + 1, nullptr);
    if (!c->planar_pool[(size_t)index]) {
        hipError_t e = hipMalloc((void **)&c->planar_pool[(size_t)index], sz);
        if (e != hipSuccess) { c->planar_pool[(size_t)index] = nullptr; return fail(P264HIP_ENOMEM, "hipMalloc(%zu) for a planar frame: %s", sz, hipGetErrorString(e)); }
    }
    const int rc = tile_convert(c, stream, slot, c->planar_pool[(size_t)index], true);
    if (rc) return rc;
    *dev = c->planar_pool[(size_t)index]; *bytes = sz;
    return P264HIP_OK;
}

// ---- frames handed on on the device (include/p264hip.h: p264hip_export_t; kernel_export.h) ----
extern "C" const char *p264hip_export_why_(const p264hip_export_t *e, int mb_w, int mb_h);     // csrc/host/export_layout.c

// room for the table of a call with n pictures (a resized export: n words, its tap tables among them) in every buffer of the ring
static int export_reserve(p264hip_ctx *c, int n)
{
    if (n <= c->exp_cap) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));              // (one wait for every buffer of the ring)
    const int cap = n + n / 2 + 16;
    c->exp_cap = 0;
    for (int i = 0; i < BATCH_RING; i++) {
        int rc = grow(c, (void **)&c->h_exp[i], nullptr, (size_t)cap * sizeof(uint32_t), 0, true, WAIT_NONE, "the export table");
        if (rc || (rc = grow(c, (void **)&c->d_exp[i], nullptr, (size_t)cap * sizeof(uint32_t), 0, false, WAIT_NONE, "the export table"))) return rc;
        if (!c->exp_free[i]) HIPCHK(hipEventCreateWithFlags(&c->exp_free[i], hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->exp_free[i], c->stream));
    }
    c->exp_cap = cap;
    return 0;
}

// ---- the steps the export roads share ----
// every picture of the call is a frame of the store
static int export_pictures_check(const char *fn, const p264hip_ctx *c, const int *streams, const int *slots, int n)
{
    for (int i = 0; i < n; i++)
        if (streams[i] < 0 || streams[i] >= c->n_streams || slots[i] < 0 || slots[i] >= c->slots)
            return fail(P264HIP_EINVAL, "%s: picture %d names stream %d slot %d (have %d x %d)", fn, i, streams[i], slots[i], c->n_streams, c->slots);
    return 0;
}

// where n pictures of `bytes` bytes, elements of `elem` bytes, lie in dst: the description's pitch and frame_stride, 0 being the
// tight ones, in bytes - or why dst cannot hold them
static int export_dst(const char *fn, int n, int64_t bytes, int elem, int pitch, int64_t frame_stride, int format, int width, const void *dst, size_t dst_bytes,
                      int64_t *pitch_bytes, int64_t *stride_bytes)
{
    if ((uintptr_t)dst % (uintptr_t)elem) return fail(P264HIP_EINVAL, "%s: dst is no multiple of the element size %d", fn, elem);
    const int64_t stride = frame_stride ? frame_stride : bytes;
    if (n > 1 && stride > (INT64_MAX - bytes) / (n - 1)) return fail(P264HIP_EINVAL, "%s: %d pictures %lld bytes apart", fn, n, (long long)stride);
    const uint64_t need = (uint64_t)(n - 1) * (uint64_t)stride + (uint64_t)bytes;
    if ((uint64_t)dst_bytes < need) return fail(P264HIP_EINVAL, "%s: %d pictures need %llu bytes, dst has %zu", fn, n, (unsigned long long)need, dst_bytes);
    *pitch_bytes = pitch ? pitch : (format == P264HIP_FMT_RGB24 ? 3 * (int64_t)width : (int64_t)width) * elem;
    *stride_bytes = stride;
    return 0;
}
static int elem_bytes(int dtype) { return dtype == P264HIP_DTYPE_U8 ? 1 : dtype == P264HIP_DTYPE_F16 ? 2 : 4; }

// The staging ring: a call's table is written into a pinned buffer and copied to its device twin on the context's stream; the event
// says when that copy is done and the pinned buffer may be written again.  export_stage: the ring's next buffer with room for
// `words` words, its last copy done (the ring advances once per call, also one that fails later); export_send: its first bytes out
struct ExportTable { uint32_t *host; const uint32_t *dev; hipEvent_t free; };
static int export_stage(p264hip_ctx *c, int words, ExportTable *t)
{
    const int rc = export_reserve(c, words);
    if (rc) return rc;
    const int r = c->exp_ring; c->exp_ring = (c->exp_ring + 1) % BATCH_RING;
    *t = ExportTable{ c->h_exp[r], c->d_exp[r], c->exp_free[r] };
    HIPCHK(hipEventSynchronize(t->free));
    return 0;
}
static int export_send(p264hip_ctx *c, const ExportTable &t, size_t bytes)
{
    HIPCHK(hipMemcpyAsync((void *)t.dev, t.host, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(t.free, c->stream));
    return 0;
}
// the frame index of every picture, then zeros up to the next multiple of 4 words, where a call's tap tables begin: returns it
static int export_indices(const p264hip_ctx *c, uint32_t *t, const int *streams, const int *slots, int n)
{
    const int first_word = (n + 3) & ~3;
    for (int i = 0; i < n; i++) t[i] = (uint32_t)(streams[i] * c->slots + slots[i]);
    for (int i = n; i < first_word; i++) t[i] = 0;
    return first_word;
}

// the colour conversion of the RGB formats (ExportParams and ResizeParams name the six fields alike)
template <typename P> static void export_colour(P &p, int matrix, int full_range)
{
    const int32_t *k = export_coefs[matrix][full_range];
    p.cy = k[0]; p.yo = full_range ? 0 : 16; p.r_cv = k[1]; p.g_cu = k[2]; p.g_cv = k[3]; p.b_cu = k[4];
}

// [first, first + count) in the slices one launch takes - a grid's second dimension ends at 65535: launch(base, rows) for each
template <typename F> static void for_grid_rows(int first, int count, F launch)
{
    for (int base = first; base < first + count; base += 65535) {
        const int left = first + count - base;
        launch(base, (unsigned)(left < 65535 ? left : 65535));
    }
}

// the tiles of a picture (kernel_export.h); the description has passed p264hip_export_check
static ExportParams export_params(const p264hip_export_t &e, int64_t pitch, int64_t stride)
{
    ExportParams p = {};
    p.x0 = e.crop_left; p.y0 = e.crop_top; p.w = e.width; p.h = e.height;
    const int s1 = (p.x0 + p.w - 1) >> 4;
    p.s0 = p.x0 >> 4; p.n_cols = s1 - p.s0 + 1;
    p.g0 = p.y0 >> 3; p.n_groups = ((p.y0 + p.h - 1) >> 3) - p.g0 + 1;
    p.cg0 = (p.y0 >> 1) >> 3; p.n_cgroups = ((((p.y0 + p.h) >> 1) - 1) >> 3) - p.cg0 + 1;
    p.ltx = (p.n_cols + 7) / 8; p.n_ltiles = p.ltx * ((p.n_groups + EXPORT_GROUPS - 1) / EXPORT_GROUPS);
    if (e.format == P264HIP_FMT_NV12) { p.c0 = p.s0; p.n_ccols = p.n_cols; }
    if (e.format == P264HIP_FMT_I420) { p.c0 = p.s0 >> 1; p.n_ccols = (s1 >> 1) - p.c0 + 1; }
    p.ctx = p.n_ccols ? (p.n_ccols + 7) / 8 : 1;
    p.n_tiles = p.n_ltiles + (p.n_ccols ? p.ctx * ((p.n_cgroups + EXPORT_GROUPS - 1) / EXPORT_GROUPS) : 0);
    p.pitch = pitch; p.frame_stride = stride;
    export_colour(p, e.matrix, e.full_range);
    return p;
}

extern "C" int p264hip_export_frames(p264hip_ctx *c, const int *streams, const int *slots, int n, const p264hip_export_t *e, void *dst, size_t dst_bytes)
{
    if (!c || !streams || !slots || !e || !dst || n < 1) return fail(P264HIP_EINVAL, "p264hip_export_frames: bad argument (n %d)", n);
    if (const char *why = p264hip_export_why_(e, c->g.mb_w, c->g.mb_h))
        return fail(P264HIP_EINVAL, "p264hip_export_frames: %s (format %d matrix %d full_range %d, window %d,%d %dx%d in a %dx%d frame, pitch %d, frame_stride %lld)", why,
                    e->format, e->matrix, e->full_range, e->crop_left, e->crop_top, e->width, e->height, c->g.w, c->g.h, e->pitch, (long long)e->frame_stride);
    int rc = export_pictures_check("p264hip_export_frames", c, streams, slots, n);
    if (rc) return rc;
    int64_t pitch, stride;              // (bytes only: an element size of 1)
    if ((rc = export_dst("p264hip_export_frames", n, p264hip_export_frame_bytes(e), 1, e->pitch, e->frame_stride, e->format, e->width, dst, dst_bytes, &pitch, &stride))) return rc;
    HIPCHK(hipSetDevice(c->device));
    ExportTable t;                      // the call's table: the frame indices
    if ((rc = export_stage(c, n, &t))) return rc;
    for (int i = 0; i < n; i++) t.host[i] = (uint32_t)(streams[i] * c->slots + slots[i]);
    if ((rc = export_send(c, t, (size_t)n * sizeof(uint32_t)))) return rc;
    const ExportParams p = export_params(*e, pitch, stride);
    const unsigned gx = (unsigned)((p.n_tiles + EXPORT_THREADS / WAVE - 1) / (EXPORT_THREADS / WAVE));
    static decltype(&k_export_i420) const kernels[] = { k_export_i420, k_export_nv12, k_export_rgb24, k_export_rgbp };     // by P264HIP_FMT_*
    static_assert(P264HIP_FMT_I420 == 0 && P264HIP_FMT_NV12 == 1 && P264HIP_FMT_RGB24 == 2 && P264HIP_FMT_RGBP == 3, "kernels[] is indexed by the format");
    for_grid_rows(0, n, [&](int base, unsigned rows) { hipLaunchKernelGGL(kernels[e->format], dim3(gx, rows), dim3(EXPORT_THREADS), 0, c->stream, (const uint8_t *)c->frames, c->frame_bytes, c->g, t.dev, base, (uint8_t *)dst, p); });
    HIPCHK(hipGetLastError());
    return P264HIP_OK;
}

// ---- the same with a resize (include/p264hip.h: p264hip_resize_t; kernel_resize.h) ----
extern "C" const char *p264hip_resize_why_(const p264hip_resize_t *r, int mb_w, int mb_h);     // csrc/host/resize_layout.c

// one tap table (kernel_resize.h): fraction | (i1 - i0) << 8 | i0 << 16 per destination index, i0 a coordinate of the frame; the
// entries behind dst_n up to the next multiple of 4 repeat the last one.  The positions are computed into the table itself and turned
// into its words in place.  (The counts have passed p264hip_resize_check: 1 .. 16384 destination samples of 1 .. 65535 source samples,
// which p264hip_resize_taps cannot refuse.)
static void resize_table(uint32_t *t, int first, int src_n, int dst_n)
{
    (void)p264hip_resize_taps(src_n, dst_n, (int32_t *)t);
    const int padded = (dst_n + 3) & ~3;
    const uint32_t last = t[dst_n - 1];
    for (int d = 0; d < padded; d++) {
        const uint32_t p = d < dst_n ? t[d] : last, i0 = p >> 8;
        t[d] = (p & 255u) | ((int)i0 < src_n - 1 ? 1u << 8 : 0u) | ((uint32_t)first + i0) << 16;
    }
}

// ---- the antialiased filter (kernel_resize_aa.h) ----
// the taps of one axis as p264hip_resize_aa_taps gives them (the counts have passed p264hip_resize_check, which it cannot refuse)
struct AaTaps {
    std::vector<int32_t> first, count;
    std::vector<uint16_t> w;
    int n, off, stride;             // destination samples; the window's offset in the frame; the largest count, rounded up to even
    void build(int offset, int src_n, int dst_n)
    {
        n = dst_n; off = offset;
        first.resize((size_t)n); count.resize((size_t)n); w.resize((size_t)n * P264HIP_AA_MAX_TAPS);
        (void)p264hip_resize_aa_taps(src_n, dst_n, first.data(), count.data(), w.data());
        int top = 1;
        for (int d = 0; d < n; d++) top = count[(size_t)d] > top ? count[(size_t)d] : top;
        stride = (top + 1) & ~1;
    }
    int pos_words() const { return (n + 3) & ~3; }
    int weight_words() const { return (n * (stride / 2) + 3) & ~3; }
    // strips (of 1 << sh samples) of the widest source span among the tiles of tw destination samples
    int span(int tw, int sh) const
    {
        int top = 1;
        for (int x0 = 0; x0 < n; x0 += tw) {
            const int x1 = (x0 + tw < n ? x0 + tw : n) - 1;
            const int s = ((off + first[(size_t)x1] + count[(size_t)x1] - 1) >> sh) - ((off + first[(size_t)x0]) >> sh) + 1;
            top = s > top ? s : top;
        }
        return top;
    }
    // the axis into the call's table from word `at` on; returns the word behind it
    int put(uint32_t *t, int at, AaAxis &ax) const
    {
        ax.pos = at; ax.wts = at + pos_words(); ax.stride = stride;
        for (int d = 0; d < pos_words(); d++) { const size_t k = (size_t)(d < n ? d : n - 1); t[at + d] = (uint32_t)(off + first[k]) | (uint32_t)count[k] << 16; }
        uint16_t *wt = (uint16_t *)(t + ax.wts);
        for (int d = 0; d < n; d++)
            for (int k = 0; k < stride; k++) wt[(size_t)d * stride + k] = w[(size_t)d * P264HIP_AA_MAX_TAPS + k];
        for (size_t k = (size_t)n * stride; k < (size_t)weight_words() * 2; k++) wt[k] = 0;
        return ax.wts + weight_words();
    }
};

// ---- what the resizing roads share: the kernels of an instance, and ResizeParams ----
// the four families' kernel pointers in the order of kernel_resize.h's EXPORT_INSTANCES, and the place of (format, dtype) in it
// (the description has passed p264hip_resize_check: a format and a dtype of the list)
#define INSTANCE_NAME(family, sfx, fmt, dt) family##sfx,
#define INSTANCE_CASE(family, sfx, fmt, dt) case fmt * 3 + dt: return family##sfx;
static decltype(&k_resize_i420) const resize_kernels[] = { EXPORT_INSTANCES(INSTANCE_NAME, k_resize_) };
static decltype(&k_resize_aa_i420) const resize_aa_kernels[] = { EXPORT_INSTANCES(INSTANCE_NAME, k_resize_aa_) };
static decltype(&k_roi_i420) const roi_kernels[] = { EXPORT_INSTANCES(INSTANCE_NAME, k_roi_) };
static decltype(&k_roi_aa_i420) const roi_aa_kernels[] = { EXPORT_INSTANCES(INSTANCE_NAME, k_roi_aa_) };
enum { EXPORT_INSTANCES(INSTANCE_NAME, instance_) n_instances };
static int instance_of(int format, int dtype)
{
    switch (format * 3 + dtype) { EXPORT_INSTANCES(INSTANCE_CASE, instance_) }
    return n_instances - 1;
}

// what every resizing kernel reads of ResizeParams: the output, where its pictures lie, colour conversion, scale and bias
static ResizeParams resize_params(const p264hip_resize_t &e, int64_t pitch, int64_t stride)
{
    ResizeParams p = {};
    p.w = e.width; p.h = e.height;
    p.pitch = pitch; p.frame_stride = stride;
    export_colour(p, e.matrix, e.full_range);
    for (int i = 0; i < 3; i++) { p.scale[i] = e.scale[i]; p.bias[i] = e.bias[i]; }
    return p;
}
// the tiles of resize_body / roi_body (a wavefront each), which split a tile index; returns the first dimension of their grid
static unsigned resize_tiles(ResizeParams &p, int format)
{
    const bool rgb = format == P264HIP_FMT_RGB24 || format == P264HIP_FMT_RGBP;
    const int cw = p.w / 2, ch = p.h / 2;
    p.ltx = (p.w + RESIZE_TILE_W - 1) / RESIZE_TILE_W; p.n_ltiles = p.ltx * (p.h / 2);
    p.ctx = (cw + RESIZE_TILE_W - 1) / RESIZE_TILE_W; p.n_tiles = p.n_ltiles + (rgb ? 0 : p.ctx * ch);
    p.inv_ltx = 0xffffffffu / (uint32_t)p.ltx; p.inv_ctx = 0xffffffffu / (uint32_t)p.ctx;
    return (unsigned)((p.n_tiles + RESIZE_THREADS / WAVE - 1) / (RESIZE_THREADS / WAVE));
}

// p264hip_export_resized with P264HIP_FILTER_BILINEAR_AA: everything has been checked
static int export_resized_aa(p264hip_ctx *c, const int *streams, const int *slots, int n, const p264hip_resize_t *e, void *dst, int64_t pitch, int64_t stride)
{
    const int W = e->width, H = e->height;
    AaTaps xl, yl, xc, yc;
    xl.build(e->crop_left, e->crop_width, W); yl.build(e->crop_top, e->crop_height, H);
    xc.build(e->crop_left / 2, e->crop_width / 2, W / 2); yc.build(e->crop_top / 2, e->crop_height / 2, H / 2);
    AaParams p = {};
    // the widest tile whose source columns fit the LDS, luma and chroma
    int tw = AA_TW;
    for (;; tw >>= 1) {
        p.ns_l = xl.span(tw, 4); p.ns_c = xc.span(tw / 2, 3);
        if (p.ns_l * 16 * AA_TH <= AA_T_CAP && p.ns_c * 16 * (AA_TH / 2) <= AA_T_CAP) break;
        if (tw == 8) return fail(P264HIP_EINVAL, "p264hip_export_resized: a tile of 8 samples spans %d luma and %d chroma strips", p.ns_l, p.ns_c);
    }
    for (p.tw_shift = 0; (4 << p.tw_shift) < tw; p.tw_shift++) ;
    p.inv_ns_l = 0xffffffffu / (uint32_t)p.ns_l; p.inv_ns_c = 0xffffffffu / (uint32_t)p.ns_c;
    p.ntx = (W + tw - 1) / tw; p.inv_ntx = 0xffffffffu / (uint32_t)p.ntx;
    const int first_word = (n + 3) & ~3;
    const int words = first_word + xl.pos_words() + xl.weight_words() + yl.pos_words() + yl.weight_words() + xc.pos_words() + xc.weight_words() + yc.pos_words() + yc.weight_words();
    ExportTable t;                      // the call's table: the frame indices, then the four axes' positions and weights
    int rc = export_stage(c, words, &t);
    if (rc) return rc;
    int at = xl.put(t.host, export_indices(c, t.host, streams, slots, n), p.xl);
    at = yl.put(t.host, at, p.yl); at = xc.put(t.host, at, p.xc); at = yc.put(t.host, at, p.yc);
    if ((rc = export_send(c, t, (size_t)words * sizeof(uint32_t)))) return rc;
    p.r = resize_params(*e, pitch, stride);                 // (the tile fields stay 0: AaParams has this filter's tiles)
    const unsigned gx = (unsigned)(p.ntx * ((H + AA_TH - 1) / AA_TH));
    const size_t lds = sizeof(uint16_t) * 16 * (size_t)(p.ns_l * AA_TH > p.ns_c * (AA_TH / 2) ? p.ns_l * AA_TH : p.ns_c * (AA_TH / 2));
    const auto kernel = resize_aa_kernels[instance_of(e->format, e->dtype)];
    for_grid_rows(0, n, [&](int base, unsigned rows) { hipLaunchKernelGGL(kernel, dim3(gx, rows), dim3(AA_THREADS), lds, c->stream, (const uint8_t *)c->frames, c->frame_bytes, c->g, t.dev, base, (uint8_t *)dst, p); });
    HIPCHK(hipGetLastError());
    return P264HIP_OK;
}

extern "C" int p264hip_export_resized(p264hip_ctx *c, const int *streams, const int *slots, int n, const p264hip_resize_t *e, void *dst, size_t dst_bytes)
{
    if (!c || !streams || !slots || !e || !dst || n < 1) return fail(P264HIP_EINVAL, "p264hip_export_resized: bad argument (n %d)", n);
    if (const char *why = p264hip_resize_why_(e, c->g.mb_w, c->g.mb_h))
        return fail(P264HIP_EINVAL, "p264hip_export_resized: %s (format %d dtype %d filter %d matrix %d full_range %d, window %d,%d %dx%d in a %dx%d frame to %dx%d, pitch %d, frame_stride %lld)", why,
                    e->format, e->dtype, e->filter, e->matrix, e->full_range, e->crop_left, e->crop_top, e->crop_width, e->crop_height, c->g.w, c->g.h, e->width, e->height, e->pitch, (long long)e->frame_stride);
    if (c->g.w > 65535 || c->g.h > 65535) return fail(P264HIP_EINVAL, "p264hip_export_resized: a frame of %dx%d samples (a tap holds a coordinate in 16 bits)", c->g.w, c->g.h);
    int rc = export_pictures_check("p264hip_export_resized", c, streams, slots, n);
    if (rc) return rc;
    int64_t pitch, stride;
    if ((rc = export_dst("p264hip_export_resized", n, p264hip_resize_frame_bytes(e), elem_bytes(e->dtype), e->pitch, e->frame_stride, e->format, e->width, dst, dst_bytes, &pitch, &stride))) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (e->filter == P264HIP_FILTER_BILINEAR_AA) return export_resized_aa(c, streams, slots, n, e, dst, pitch, stride);
    // the call's table: the frame indices, then the four tap tables, each from a multiple of 4 words
    const int W = e->width, H = e->height, cw = W / 2, ch = H / 2;
    ResizeParams p = resize_params(*e, pitch, stride);
    p.t_xl = (n + 3) & ~3; p.t_yl = p.t_xl + ((W + 3) & ~3); p.t_xc = p.t_yl + ((H + 3) & ~3); p.t_yc = p.t_xc + ((cw + 3) & ~3);
    const int words = p.t_yc + ((ch + 3) & ~3);
    ExportTable t;
    if ((rc = export_stage(c, words, &t))) return rc;
    export_indices(c, t.host, streams, slots, n);
    resize_table(t.host + p.t_xl, e->crop_left, e->crop_width, W); resize_table(t.host + p.t_yl, e->crop_top, e->crop_height, H);
    resize_table(t.host + p.t_xc, e->crop_left / 2, e->crop_width / 2, cw); resize_table(t.host + p.t_yc, e->crop_top / 2, e->crop_height / 2, ch);
    if ((rc = export_send(c, t, (size_t)words * sizeof(uint32_t)))) return rc;
    const unsigned gx = resize_tiles(p, e->format);
    const auto kernel = resize_kernels[instance_of(e->format, e->dtype)];
    for_grid_rows(0, n, [&](int base, unsigned rows) { hipLaunchKernelGGL(kernel, dim3(gx, rows), dim3(RESIZE_THREADS), 0, c->stream, (const uint8_t *)c->frames, c->frame_bytes, c->g, t.dev, base, (uint8_t *)dst, p); });
    HIPCHK(hipGetLastError());
    return P264HIP_OK;
}

// ---- a window per picture into a rectangle of the output (include/p264hip.h: p264hip_roi_t; kernel_roi.h) ----
extern "C" const char *p264hip_rois_aa_why_(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots, int *bad);
extern "C" const char *p264hip_rois_why_(const p264hip_roi_t *rois, int n, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots, int *bad);     // csrc/host/resize_layout.c

// p264hip_export_rois (aa false) and p264hip_export_rois_aa: the checks, the descriptors and the launch pairs are one text
static int export_rois(p264hip_ctx *c, const p264hip_roi_t *rois, int n, const p264hip_resize_t *e, uint32_t fill, void *dst, size_t dst_bytes, bool aa)
{
    const char *fn = aa ? "p264hip_export_rois_aa" : "p264hip_export_rois";
    if (!c || !dst) return fail(P264HIP_EINVAL, "%s: bad argument (n %d)", fn, n);
    int bad;
    if (const char *why = (aa ? p264hip_rois_aa_why_ : p264hip_rois_why_)(rois, n, e, fill, c->g.mb_w, c->g.mb_h, c->n_streams, c->slots, &bad)) {
        if (bad < 0) return fail(P264HIP_EINVAL, "%s: %s (n %d, fill 0x%x)", fn, why, n, fill);
        const p264hip_roi_t &o = rois[bad];
        return fail(P264HIP_EINVAL, "%s: ROI %d: %s (stream %d slot %d of %d x %d, window %d,%d %dx%d in a %dx%d frame, rectangle %d,%d %dx%d in %dx%d)", fn, bad, why,
                    o.stream, o.slot, c->n_streams, c->slots, o.left, o.top, o.width, o.height, c->g.w, c->g.h, o.dst_left, o.dst_top, o.dst_width, o.dst_height, e->width, e->height);
    }
    if (c->g.w > 65535 || c->g.h > 65535) return fail(P264HIP_EINVAL, "%s: a frame of %dx%d samples (a tap holds a coordinate in 16 bits)", fn, c->g.w, c->g.h);
    int64_t pitch, stride;
    int rc = export_dst(fn, n, aa ? p264hip_rois_aa_frame_bytes(e) : p264hip_rois_frame_bytes(e), elem_bytes(e->dtype), e->pitch, e->frame_stride, e->format, e->width, dst, dst_bytes, &pitch, &stride);
    if (rc) return rc;
    constexpr int desc_words = (int)(sizeof(RoiDev) / sizeof(uint32_t));
    if (n > INT32_MAX / desc_words - 16) return fail(P264HIP_ENOMEM, "%s: %d descriptors", fn, n);
    HIPCHK(hipSetDevice(c->device));
    ExportTable table;                  // the call's table: a descriptor per ROI
    if ((rc = export_stage(c, n * desc_words, &table))) return rc;
    // the descriptors, and the launch pairs: ROIs first .. first + count - 1 of a pair share the scratch, a segment each from word 0 on
    // (one segment is at most 49152 words - 300 000 with weights -, so every pair holds at least one ROI)
    constexpr size_t scratch_words = P264HIP_ROI_SCRATCH_BYTES / sizeof(uint32_t);
    struct Pair { int first, count, widest, tiles, lds; };   // (tiles, lds: the grid and the dynamic LDS of the pair's k_roi_aa_* launches)
    std::vector<Pair> pairs;
    RoiDev *t = (RoiDev *)table.host;
    const int W = e->width, H = e->height;
    size_t used = 0, most = 0;
    for (int i = 0; i < n; i++) {
        const p264hip_roi_t &o = rois[i];
        const bool whole = !(o.dst_left | o.dst_top | o.dst_width | o.dst_height);
        const int dl = whole ? 0 : o.dst_left, dt = whole ? 0 : o.dst_top, dw = whole ? W : o.dst_width, dh = whole ? H : o.dst_height;
        const int words = aa ? p264hip_roi_aa_words(o.width, o.height, dw, dh) : roi_seg_words(dw, dh);
        if (pairs.empty() || used + (size_t)words > scratch_words) { pairs.push_back({ i, 0, 0, 0, 0 }); used = 0; }
        Pair &pr = pairs.back();
        t[i] = RoiDev{ (uint32_t)(o.stream * c->slots + o.slot), (uint32_t)used, (uint32_t)dl | (uint32_t)dw << 16, (uint32_t)dt | (uint32_t)dh << 16,
                       (uint32_t)o.left | (uint32_t)o.width << 16, (uint32_t)o.top | (uint32_t)o.height << 16, { 0, 0 } };
        const int entries = roi_seg_words(dw, dh);          // (filter 0: a word each; the antialiased filter: an entry of p264hip_aa.h each)
        if (aa) {
            // the ROI's tile width and LDS rows, and its four weight strides (kernel_roi_aa.h)
            int ns_l, ns_c;
            const int tw_shift = p264hip_roi_aa_tile(o.width, dw, AA_T_CAP, &ns_l, &ns_c), tw = 4 << tw_shift;
            t[i].pad[0] = (uint32_t)tw_shift | (uint32_t)ns_l << 8 | (uint32_t)ns_c << 16;
            t[i].pad[1] = (uint32_t)p264hip_aa_stride(o.width, dw) | (uint32_t)p264hip_aa_stride(o.height, dh) << 8
                        | (uint32_t)p264hip_aa_stride(o.width >> 1, dw >> 1) << 16 | (uint32_t)p264hip_aa_stride(o.height >> 1, dh >> 1) << 24;
            const int tiles = ((W + tw - 1) / tw) * ((H + AA_TH - 1) / AA_TH), lds = 32 * (ns_l * AA_TH > ns_c * (AA_TH / 2) ? ns_l * AA_TH : ns_c * (AA_TH / 2));
            pr.tiles = tiles > pr.tiles ? tiles : pr.tiles; pr.lds = lds > pr.lds ? lds : pr.lds;
        }
        used += (size_t)words; pr.count++;
        pr.widest = entries > pr.widest ? entries : pr.widest;
        most = used > most ? used : most;
    }
    if ((rc = grow(c, (void **)&c->d_roi, &c->roi_cap, most * sizeof(uint32_t), 0, false, WAIT_STREAM, "the ROI taps"))) return rc;
    if ((rc = export_send(c, table, (size_t)n * sizeof(RoiDev)))) return rc;
    ResizeParams p = resize_params(*e, pitch, stride);      // (t_xl .. t_yc stay 0: the tables are the segments')
    const unsigned gx = resize_tiles(p, e->format);
    RoiAaParams pa = {};
    pa.r = p;
    pa.tile_rows = (H + AA_TH - 1) / AA_TH;
    for (int s = 1; s <= 4; s++) pa.inv_ntx[s - 1] = 0xffffffffu / (uint32_t)((W + (4 << s) - 1) / (4 << s));
    // what the filter chooses of a pair's two launches: the kernels, the body's block and its parameters (its ninth argument)
    const int instance = instance_of(e->format, e->dtype);
    const auto taps = aa ? k_roi_aa_taps : k_roi_taps;
    const void *body = aa ? (const void *)roi_aa_kernels[instance] : (const void *)roi_kernels[instance];
    const unsigned block = aa ? AA_THREADS : RESIZE_THREADS;
    const uint8_t *frames = c->frames; const RoiDev *d_rois = (const RoiDev *)table.dev; const uint32_t *scratch = c->d_roi; uint8_t *out = (uint8_t *)dst;
    for (const Pair &pr : pairs) {                          // (one stream: a pair's taps are read before the next pair's are written)
        const unsigned tx = (unsigned)((pr.widest + ROI_TAPS_THREADS - 1) / ROI_TAPS_THREADS);
        for_grid_rows(pr.first, pr.count, [&](int base, unsigned rows) { hipLaunchKernelGGL(taps, dim3(tx, rows), dim3(ROI_TAPS_THREADS), 0, c->stream, d_rois, base, c->d_roi); });
        for_grid_rows(pr.first, pr.count, [&](int base, unsigned rows) {
            void *args[] = { &frames, &c->frame_bytes, &c->g, &d_rois, &scratch, &base, &out, aa ? (void *)&pa : (void *)&p, &fill };
            (void)hipLaunchKernel(body, dim3(aa ? (unsigned)pr.tiles : gx, rows), dim3(block), args, (size_t)pr.lds, c->stream);
        });
    }
    HIPCHK(hipGetLastError());
    return P264HIP_OK;
}

extern "C" int p264hip_export_rois(p264hip_ctx *c, const p264hip_roi_t *rois, int n, const p264hip_resize_t *e, uint32_t fill, void *dst, size_t dst_bytes)
{
    return export_rois(c, rois, n, e, fill, dst, dst_bytes, false);
}
extern "C" int p264hip_export_rois_aa(p264hip_ctx *c, const p264hip_roi_t *rois, int n, const p264hip_resize_t *e, uint32_t fill, void *dst, size_t dst_bytes)
{
    return export_rois(c, rois, n, e, fill, dst, dst_bytes, true);
}

// ---- the same from an ROI list in device memory (include/p264hip.h: p264hip_rois_dev_t; kernel_roi_dev.h) ----
extern "C" const char *p264hip_rois_device_why_(const p264hip_rois_dev_t *l, const p264hip_resize_t *r, uint32_t fill, int mb_w, int mb_h, int n_streams, int slots);     // csrc/host/resize_layout.c

extern "C" int p264hip_export_rois_device(p264hip_ctx *c, const p264hip_rois_dev_t *l, const p264hip_resize_t *e, uint32_t fill, void *dst, size_t dst_bytes)
{
    const char *fn = "p264hip_export_rois_device";
    if (!c || !dst) return fail(P264HIP_EINVAL, "%s: bad argument", fn);
    if (const char *why = p264hip_rois_device_why_(l, e, fill, c->g.mb_w, c->g.mb_h, c->n_streams, c->slots))
        return fail(P264HIP_EINVAL, "%s: %s (n %d, max_reduction %d, flags 0x%x, fill 0x%x, a %dx%d frame)", fn, why, l ? l->n : 0, l ? l->max_reduction : 0, l ? l->flags : 0, fill, c->g.w, c->g.h);
    const bool aa = e->filter == P264HIP_FILTER_BILINEAR_AA;
    const int n = l->n;
    int64_t pitch, stride;
    int rc = export_dst(fn, n, aa ? p264hip_rois_aa_frame_bytes(e) : p264hip_rois_frame_bytes(e), elem_bytes(e->dtype), e->pitch, e->frame_stride, e->format, e->width, dst, dst_bytes, &pitch, &stride);
    if (rc) return rc;
    p264hip_rois_plan_t plan;
    if (p264hip_rois_device_plan(e, l->max_reduction, &plan)) return fail(P264HIP_EINVAL, "%s: no plan for this output", fn);
    if ((size_t)n > SIZE_MAX / sizeof(RoiDev) / 2) return fail(P264HIP_ENOMEM, "%s: %d descriptors", fn, n);
    HIPCHK(hipSetDevice(c->device));
    // the context's buffers: a descriptor per ROI, and the segments of one pair (every ROI has one of plan.seg_words)
    const int per_pair = plan.rois_per_pair < n ? plan.rois_per_pair : n;
    if ((rc = grow(c, (void **)&c->d_roi_tab, &c->roi_tab_cap, (size_t)n * sizeof(RoiDev), (size_t)n / 2 * sizeof(RoiDev), false, WAIT_STREAM, "the ROI descriptors"))) return rc;
    if ((rc = grow(c, (void **)&c->d_roi, &c->roi_cap, (size_t)per_pair * (size_t)plan.seg_words * sizeof(uint32_t), 0, false, WAIT_STREAM, "the ROI taps"))) return rc;
    if (l->flags & P264HIP_ROIS_AFTER) {                    // the list is what after_stream has queued so far
        if (!c->roi_after) HIPCHK(hipEventCreateWithFlags(&c->roi_after, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->roi_after, (hipStream_t)l->after_stream));
        HIPCHK(hipStreamWaitEvent(c->stream, c->roi_after, 0));
    }
    const int32_t *d_slots = nullptr;
    if (l->slot_of_stream) {                                // the one table the call stages: n_streams integers
        ExportTable t;
        if ((rc = export_stage(c, c->n_streams, &t))) return rc;
        memcpy(t.host, l->slot_of_stream, (size_t)c->n_streams * sizeof(int32_t));
        if ((rc = export_send(c, t, (size_t)c->n_streams * sizeof(int32_t)))) return rc;
        d_slots = (const int32_t *)t.dev;
    }
    const RoiPlanParams pp = { n, e->width, e->height, e->filter, c->g.w, c->g.h, c->n_streams, c->slots, l->max_reduction, plan.seg_words, plan.rois_per_pair, AA_T_CAP };
    hipLaunchKernelGGL(k_roi_plan, dim3((unsigned)((n + ROI_PLAN_THREADS - 1) / ROI_PLAN_THREADS)), dim3(ROI_PLAN_THREADS), 0, c->stream, l->rois_dev, l->count_dev, d_slots, pp, c->d_roi_tab, l->status_dev);
    const int W = e->width, H = e->height;
    ResizeParams p = resize_params(*e, pitch, stride);      // (t_xl .. t_yc stay 0: the tables are the segments')
    const unsigned gx = resize_tiles(p, e->format);
    RoiAaParams pa = {};
    pa.r = p;
    pa.tile_rows = (H + AA_TH - 1) / AA_TH;
    for (int s = 1; s <= 4; s++) pa.inv_ntx[s - 1] = 0xffffffffu / (uint32_t)((W + (4 << s) - 1) / (4 << s));
    const int instance = instance_of(e->format, e->dtype);
    const auto taps = aa ? k_roi_aa_taps : k_roi_taps;
    const void *body = aa ? (const void *)roi_aa_kernels[instance] : (const void *)roi_kernels[instance];
    const unsigned block = aa ? AA_THREADS : RESIZE_THREADS;
    const uint8_t *frames = c->frames; const RoiDev *d_rois = c->d_roi_tab; const uint32_t *scratch = c->d_roi; uint8_t *out = (uint8_t *)dst;
    // every rectangle is inside the output: no segment has more entries than the whole output's
    const unsigned tx = (unsigned)((roi_seg_words(W, H) + ROI_TAPS_THREADS - 1) / ROI_TAPS_THREADS);
    for (int first = 0; first < n; first += plan.rois_per_pair) {        // (one stream: a pair's taps are read before the next pair's are written)
        const int count = n - first < plan.rois_per_pair ? n - first : plan.rois_per_pair;
        for_grid_rows(first, count, [&](int base, unsigned rows) { hipLaunchKernelGGL(taps, dim3(tx, rows), dim3(ROI_TAPS_THREADS), 0, c->stream, d_rois, base, c->d_roi); });
        for_grid_rows(first, count, [&](int base, unsigned rows) {
            void *args[] = { &frames, &c->frame_bytes, &c->g, &d_rois, &scratch, &base, &out, aa ? (void *)&pa : (void *)&p, &fill };
            (void)hipLaunchKernel(body, dim3(aa ? (unsigned)plan.aa_tiles : gx, rows), dim3(block), args, (size_t)plan.aa_lds_bytes, c->stream);
        });
    }
    HIPCHK(hipGetLastError());
    if (l->flags & P264HIP_ROIS_BEFORE) {
        if (!c->roi_before) HIPCHK(hipEventCreateWithFlags(&c->roi_before, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->roi_before, c->stream));
        HIPCHK(hipStreamWaitEvent((hipStream_t)l->before_stream, c->roi_before, 0));
    }
    return P264HIP_OK;
}

extern "C" int p264hip_copy_to_device(void *dev, const void *host, size_t bytes)
{
    if (!dev || !host) return fail(P264HIP_EINVAL, "p264hip_copy_to_device: null argument");
    HIPCHK(hipMemcpy(dev, host, bytes, hipMemcpyHostToDevice));
    return P264HIP_OK;
}
extern "C" int p264hip_copy_from_device(void *host, const void *dev, size_t bytes)
{
    if (!dev || !host) return fail(P264HIP_EINVAL, "p264hip_copy_from_device: null argument");
    HIPCHK(hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
    return P264HIP_OK;
}

extern "C" int p264hip_upload(p264hip_ctx *c, int first, const p264hip_picture_t *pics, int n)
{
    if (!c || !pics || n < 0 || first < 0 || first + n > c->max_pictures) return fail(P264HIP_EINVAL, "p264hip_upload: bad range [%d,+%d)", first, n);
    HIPCHK(hipSetDevice(c->device));
    for (int i = 0; i < n; i++) { int rc = p264hip_upload_async(c, first + i, &pics[i]); if (rc) return rc; }
    // sources are pageable host memory owned by the caller: make sure they are consumed before returning
    HIPCHK(hipStreamSynchronize(c->stream));
    return P264HIP_OK;
}

// Host buffers the device reads by DMA (the parsers write their pictures into them: p264parse_set_allocator).  Ordinary pages,
// advised as huge pages where the buffer is large, touched and then pinned with hipHostRegister - NOT hipHostMalloc: round 5
// found the parser threads 36 % slower on hipHostMalloc'ed buffers with or without a device at work (7.0 s against 5.15 s per 3 072
// 1080p pictures on 16 threads; registered 4 KB pages 5.7 s, registered huge pages 5.55 s, scratch/r5_pipe2.sh / r5_pipe3.sh) - the
// parser reads its own output back all the time (neighbour vectors, coefficient counts) through 4 KB translations.  The
// end-to-end pipeline went from 6.5 - 6.9 k to 8.3 k frames/s.  P264AMD_HOST_ALLOC = 0 (hipHostMalloc, coherent) / 1
// (non-coherent) / 2 (registered 4 KB pages) / 3 (the default) stay as a knob for the experiment.
static std::mutex g_host_mu;
static std::unordered_map<void *, int> g_host_registered;     // pointers from posix_memalign + hipHostRegister
static int host_alloc_mode()
{
    static int mode = -1;
    if (mode < 0) { const char *e = getenv("P264AMD_HOST_ALLOC"); int m = e ? atoi(e) : 3; mode = (m < 0 || m > 3) ? 3 : m; }
    return mode;
}
extern "C" void *p264hip_host_alloc(size_t bytes)
{
    void *p = nullptr;
    const size_t n = bytes ? bytes : 1;
    const int mode = host_alloc_mode();
    if (mode >= 2) {
        const bool huge = mode == 3 && n >= ((size_t)256 << 10);
        const size_t al = huge ? ((size_t)2 << 20) : 4096, rounded = (n + al - 1) & ~(al - 1);
        if (posix_memalign(&p, al, rounded) == 0) {
            if (huge) (void)madvise(p, rounded, MADV_HUGEPAGE);
            for (size_t o = 0; o < rounded; o += 4096) ((volatile char *)p)[o] = 0;          // (faulted in before they are pinned)
            if (hipHostRegister(p, rounded, hipHostRegisterPortable) == hipSuccess) {
                std::lock_guard<std::mutex> lk(g_host_mu);
                g_host_registered[p] = 1;
                return p;
            }
            (void)hipGetLastError();
            free(p); p = nullptr;
        }
        // (could not be registered: pinned memory of the runtime's own)
    }
    if (hipHostMalloc(&p, n, hipHostMallocPortable | (mode == 1 ? hipHostMallocNonCoherent : 0)) != hipSuccess) return nullptr;
    return p;
}

extern "C" void p264hip_host_free(void *p)
{
    if (!p) return;
    bool registered;
    { std::lock_guard<std::mutex> lk(g_host_mu); registered = g_host_registered.erase(p) != 0; }
    if (registered) { (void)hipHostUnregister(p); free(p); }
    else (void)hipHostFree(p);
}

extern "C" int p264hip_marker(p264hip_ctx *c)
{
    if (!c) return fail(P264HIP_EINVAL, "null context");
    HIPCHK(hipSetDevice(c->device));
    const int m = c->next_marker; c->next_marker = (c->next_marker + 1) % P264HIP_MARKERS;
    if (!c->markers[m]) HIPCHK(hipEventCreateWithFlags(&c->markers[m], hipEventDisableTiming));
    HIPCHK(hipEventRecord(c->markers[m], c->stream));
    return m;
}

extern "C" int p264hip_marker_wait(p264hip_ctx *c, int marker)
{
    if (!c || marker < 0 || marker >= P264HIP_MARKERS || !c->markers[marker]) return fail(P264HIP_EINVAL, "p264hip_marker_wait: bad marker %d", marker);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(c->markers[marker]));
    return P264HIP_OK;
}

extern "C" int p264hip_clone_picture(p264hip_ctx *c, int dst, int src)
{
    if (!c || dst < 0 || src < 0 || dst >= c->max_pictures || src >= c->max_pictures || dst == src || c->pics[(size_t)src].state < STAGED)
        return fail(P264HIP_EINVAL, "p264hip_clone_picture: bad slots %d <- %d", dst, src);
    HIPCHK(hipSetDevice(c->device));
    PicSlot &d = c->pics[(size_t)dst], &s = c->pics[(size_t)src];
    int rc = slot_prepare(c, dst, s.L, 0);
    if (rc || (rc = expand_pending(c))) return rc;            // (src may still be a compact block)
    HIPCHK(hipMemcpyAsync(d.dev, s.dev, s.L.bytes, hipMemcpyDeviceToDevice, c->stream));
    // the verdict of the record check is kept per slot (k_check_records -> d_slot_bad[slot]): an unchecked block takes its
    // verdict along (behind the check on the same stream), any other clone clears what an earlier tenant of dst left there
    if (s.state == UNCHECKED) HIPCHK(hipMemcpyAsync(c->d_slot_bad + dst, c->d_slot_bad + src, sizeof(int), hipMemcpyDeviceToDevice, c->stream));
    else HIPCHK(hipMemsetAsync(c->d_slot_bad + dst, 0, sizeof(int), c->stream));
    slot_exit(c, dst, s.meta, s.state);
    stamp(c, s);
    return P264HIP_OK;
}

static hipEvent_t get_event(p264hip_ctx *c)
{
    if (!c->event_pool.empty()) { hipEvent_t e = c->event_pool.back(); c->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr; (void)hipEventCreate(&e); return e;
}

struct ScopedStamp {                   // HIP events on the context's own stream, around one launch
    p264hip_ctx *c; int k; hipEvent_t a = nullptr, b = nullptr;
    ScopedStamp(p264hip_ctx *c_, int k_) : c(c_), k(k_) { if (c->timing) { a = get_event(c); b = get_event(c); (void)hipEventRecord(a, c->stream); } }
    ~ScopedStamp() { if (c->timing) { (void)hipEventRecord(b, c->stream); c->stamps.push_back({ a, b, k }); } }
};

// ---- p264hip_reconstruct, step by step (in call order) ----
// room for a batch of n pictures: the ring of descriptor buffers and the per-picture scratch of the kernels
static int batch_reserve(p264hip_ctx *c, int n)
{
    if (n <= c->batch_cap) return 0;
    HIPCHK(hipStreamSynchronize(c->stream));              // (one wait for every buffer of the ring)
    c->batch_cap = 0;
    for (int i = 0; i < BATCH_RING; i++) {
        int rc = grow(c, (void **)&c->h_batch[i], nullptr, (size_t)n * sizeof(PicDev), 0, true, WAIT_NONE, "the batch");
        if (rc || (rc = grow(c, (void **)&c->d_batch[i], nullptr, (size_t)n * sizeof(PicDev), 0, false, WAIT_NONE, "the batch")) ||
            (rc = grow(c, (void **)&c->h_scale[i], nullptr, (size_t)n * sizeof(ScaleDev), 0, true, WAIT_NONE, "the batch")) ||
            (rc = grow(c, (void **)&c->d_scale[i], nullptr, (size_t)n * sizeof(ScaleDev), 0, false, WAIT_NONE, "the batch"))) return rc;
        if (!c->batch_free[i]) HIPCHK(hipEventCreateWithFlags(&c->batch_free[i], hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->batch_free[i], c->stream));
    }
    int rc = grow(c, (void **)&c->d_is_intra, nullptr, (size_t)n * c->g.n_mb, 0, false, WAIT_NONE, "the batch");
    if (rc || (rc = grow(c, (void **)&c->d_edge, nullptr, (size_t)n * c->g.n_mb * sizeof(EdgeInfo), 0, false, WAIT_NONE, "the batch")) ||
        (rc = grow(c, (void **)&c->d_mc, nullptr, (size_t)n * c->dev.ml.words * sizeof(uint32_t), 0, false, WAIT_NONE, "the batch"))) return rc;
    // (the Cr side array, if the context has one, grows with the others; the stream has been waited for above)
    if (c->d_edge_cr && (rc = grow(c, (void **)&c->d_edge_cr, nullptr, (size_t)n * c->g.n_mb * sizeof(uint32_t), 0, false, WAIT_NONE, "the batch"))) return rc;
    c->batch_cap = n;
    return 0;
}
// the first batch that holds a picture with a cr_qp_offset_delta: one dword per macroblock for every picture a batch can hold
static int edge_cr_reserve(p264hip_ctx *c)
{
    if (c->d_edge_cr) return 0;
    return grow(c, (void **)&c->d_edge_cr, nullptr, (size_t)c->batch_cap * c->g.n_mb * sizeof(uint32_t), 0, false, WAIT_NONE, "the batch");
}

// pictures that came through p264hip_input_commit: the verdicts of their record checks, one wait for the whole batch
static int settle_unchecked(p264hip_ctx *c, const int *pic_ids, int n)
{
    bool any_unchecked = false;
    for (int i = 0; i < n; i++) { const int id = pic_ids[i]; if (id >= 0 && id < c->max_pictures && c->pics[(size_t)id].state == UNCHECKED) any_unchecked = true; }
    if (!any_unchecked) return 0;
    std::vector<int> bad((size_t)c->max_pictures);
    const uint64_t upto = c->epoch;
    HIPCHK(hipMemcpyAsync(bad.data(), c->d_slot_bad, sizeof(int) * bad.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->done_epoch = upto;
    for (int i = 0; i < n; i++) {
        const int id = pic_ids[i];
        if (id < 0 || id >= c->max_pictures || c->pics[(size_t)id].state != UNCHECKED) continue;
        if (bad[(size_t)id]) { c->pics[(size_t)id].state = EMPTY; return fail(P264HIP_EINVAL, "picture slot %d: a macroblock's coefficient blocks lie outside coefs[], or a record is an I_PCM or 8x8-transform record of the wrong form (the block a device producer committed is inconsistent)", id); }
        c->pics[(size_t)id].state = READY;
    }
    return 0;
}

// what the kernels see of the picture in input slot s when it decodes into frame store `st`
static PicDev picdev_of(p264hip_ctx *c, const PicSlot &s, int st)
{
    PicDev d;
    memset(&d, 0, sizeof d);
    d.mb = (const p264hip_mb_t *)s.dev;
    d.mv = (const int *)(s.dev + s.L.off_mv);
    d.ref_idx = (const int8_t *)(s.dev + s.L.off_ref);
    d.i4modes = s.dev + s.L.off_i4;
    d.coefs = (const int16_t *)(s.dev + s.L.off_coef);
    d.dst = frame_ptr(c, st, s.meta.dst_slot);
    d.store = frame_ptr(c, st, 0);
    d.store_bytes = (uint32_t)(c->frame_bytes * (size_t)c->slots);
    d.dst_off = (uint32_t)(c->frame_bytes * (size_t)s.meta.dst_slot);
    for (int k = 0; k < P264HIP_MAX_REFS; k++)
        d.ref_off[k] = (uint32_t)(c->frame_bytes * (size_t)(k < s.meta.n_ref ? s.meta.ref_slot[k] : (s.meta.n_ref ? s.meta.ref_slot[0] : s.meta.dst_slot)));
    d.n_ref = s.meta.n_ref; d.slice_type = s.meta.slice_type;
    d.chroma_qp_offset = s.meta.chroma_qp_offset; d.deblock = s.meta.deblock;
    d.alpha_off = s.meta.alpha_c0_offset; d.beta_off = s.meta.beta_offset;
    if (s.meta.slice_type == P264_SLICE_B) {
        d.mv_l1 = (const int *)(s.dev + s.L.off_mv_l1);
        d.ref_idx_l1 = (const int8_t *)(s.dev + s.L.off_ref_l1);
        d.bipred_w = (const int16_t *)(s.dev + s.L.off_weights);
        d.n_ref_l1 = s.meta.n_ref_l1; d.weighted = s.meta.weighted_bipred;
        for (int k = 0; k < P264HIP_MAX_REFS; k++)
            d.ref_off_l1[k] = (uint32_t)(c->frame_bytes * (size_t)(k < s.meta.n_ref_l1 ? s.meta.ref_slot_l1[k] : s.meta.ref_slot_l1[0]));
    }
    if (s.meta.explicit_wp) {
        d.wp = (const int16_t *)(s.dev + s.L.off_wp);
        d.explicit_wp = 1; d.wp_denom_y = s.meta.wp_log2_denom[0]; d.wp_denom_c = s.meta.wp_log2_denom[1];
    }
    if (s.meta.slice_type == P264_SLICE_P && !s.meta.explicit_wp) {
        // one frame at two indices (reordering commands that name it twice, a list padded with its last frame): the loop filter
        // tells reference PICTURES apart (H.264 8.7.2.1), so such a picture takes the by-picture edge info, as weighted ones do
        for (int k = 1; k < s.meta.n_ref && k < P264HIP_MAX_REFS; k++)
            for (int j = 0; j < k; j++) if (s.meta.ref_slot[k] == s.meta.ref_slot[j]) d.dup_refs = 1;
    }
    return d;
}

// the batch's streams and slots checked (nothing is queued yet), one PicDev per picture in hb; kinds: what the batch holds (launch_plan.h)
static int batch_fill(p264hip_ctx *c, const int *pic_ids, const int *streams, int n, PicDev *hb, ScaleDev *hs, BatchKinds *kinds)
{
    for (int i = 0; i < n; i++) {                          // two pictures of one call must not share a stream: they would race on its frames
        const int st = streams[i];
        if (st < 0 || st >= c->n_streams) return fail(P264HIP_EINVAL, "stream %d out of range", st);
        c->stream_seen[(size_t)st] = 0;
    }
    BatchKinds k;
    for (int i = 0; i < n; i++) {
        int id = pic_ids[i], st = streams[i];
        if (id < 0 || id >= c->max_pictures || c->pics[(size_t)id].state < STAGED) return fail(P264HIP_EINVAL, "picture slot %d is empty", id);
        if (c->stream_seen[(size_t)st]) return fail(P264HIP_EINVAL, "stream %d is named twice in one batch (entries %d and %d)", st, c->stream_seen[(size_t)st] - 1, i);
        c->stream_seen[(size_t)st] = i + 1;
        const PicSlot &s = c->pics[(size_t)id];
        hb[i] = picdev_of(c, s, st);
        k.p |= s.meta.slice_type != P264_SLICE_I;
        k.b |= s.meta.slice_type == P264_SLICE_B;
        k.i |= s.meta.slice_type == P264_SLICE_I;
        k.wp |= s.meta.explicit_wp != 0;
        k.dup |= hb[i].dup_refs != 0;
        k.t8 |= (s.meta.transform_8x8 & ~P264_T8X8_INTRA) != 0 && s.meta.slice_type != P264_SLICE_I;
        k.i8 |= (s.meta.transform_8x8 & P264_T8X8_INTRA) != 0;
        // the picture's table in its slot; a flat picture: the all-16 table (what a batch with a scaled picture runs it through).  A
        // picture whose Cr has a QP offset of its own takes the scaled road too, with the all-16 table where it has no lists
        const int cr_delta = s.meta.cr_qp_offset_delta;
        const bool scaled = s.meta.scaling_lists != 0 || cr_delta != 0;
        hs[i] = ScaleDev{ s.meta.scaling_lists ? s.dev + s.L.off_scaling : c->d_flat16, scaled ? 1 : 0, cr_delta };
        k.sc += scaled;
        k.cr |= cr_delta != 0;
        k.n_cr += cr_delta != 0;
    }
    *kinds = k;
    return 0;
}

// The launches, in stream order: each issues its stage of the batch's plan (launch_plan.h: which instance, which shape and why) and
// decides nothing.  batch: the n PicDevs on the device, scale: their ScaleDevs (copied for scaled batches only); a failed launch is
// reported by p264hip_reconstruct's hipGetLastError behind the last of them.
static uint32_t inv_mb_w(const p264hip_ctx *c) { return (uint32_t)(((1ull << 32) - 1) / (unsigned)c->g.mb_w); }
static dim3 grid_of(const LaunchShape &s) { return dim3(s.grid_x, s.grid_y); }

// motion compensation + residual of all inter macroblocks: device-side counting sort of the work items by what the
// interpolation has to do, then the luma and chroma kernels over the sorted lists (kernel_mc.h), side by side
static void launch_inter(p264hip_ctx *c, const PicDev *batch, const ScaleDev *scale, const LaunchPlan &pl)
{
    if (pl.sort == SortKernel::none) return;
    ScopedStamp t(c, 0);
    const Geom g = c->g;
    const McLayout ml = c->dev.ml;
#define SORT(kernel, ...) hipLaunchKernelGGL(kernel, grid_of(pl.sort_shape), dim3(pl.sort_shape.threads), 0, c->stream, batch, c->d_mc, g, ml, inv_mb_w(c), c->d_is_intra, ##__VA_ARGS__)
    switch (pl.sort) {
    case SortKernel::none:     break;
    case SortKernel::plain:    SORT(k_mc_sort); break;
    case SortKernel::wp:       SORT(k_mc_sort_wp); break;
    case SortKernel::b:        SORT(k_mc_sort_b); break;
    case SortKernel::b_wp:     SORT(k_mc_sort_b_wp); break;
    case SortKernel::scaled:   SORT(k_mc_sort_scaled, scale); break;
    case SortKernel::scaled_p: SORT(k_mc_sort_scaled_p, scale); break;
    }
#undef SORT
    // one launch for luma / chroma, macroblock / quadrant items; B pictures: a second pass over the second list set
#define MC(kernel) hipLaunchKernelGGL(kernel, grid_of(pl.mc_shape), dim3(pl.mc_shape.threads), 0, c->stream, batch, (const uint32_t *)c->d_mc, g, ml, \
                                      pl.info.mc_wgs_per_picture, pl.mc_wgs_total, pl.mc_inv_wgs)
    switch (pl.mc) {
    case McKernel::none:  break;
    case McKernel::plain: MC(k_mc); break;
    case McKernel::wp:    MC(k_mc_wp); break;
    }
    if (pl.mc_second) MC(k_mc_second);
#undef MC
}

// the residuals the inter launches left out, added in place on top of the prediction in the frame store: the luma of the macroblocks
// with P264_MB_T8X8 (kernel_t8x8.h), or - scaled batches - everything of the scaled pictures' inter macroblocks and the 8x8 blocks of
// every picture (kernel_scaling.h).  Counts as inter time (timing index 0).
static void launch_residual(p264hip_ctx *c, const PicDev *batch, const ScaleDev *scale, const LaunchPlan &pl)
{
    if (pl.residual == ResidualKernel::none) return;
    ScopedStamp t(c, 0);
    const dim3 grid = grid_of(pl.residual_shape), block(pl.residual_shape.threads);
    switch (pl.residual) {
    case ResidualKernel::none:         break;
    case ResidualKernel::t8x8:         hipLaunchKernelGGL(k_t8x8, grid, block, 0, c->stream, batch, c->g); break;
    case ResidualKernel::scaled_inter: hipLaunchKernelGGL(k_scaled_inter, grid, block, 0, c->stream, batch, scale, c->g); break;
    }
}

static void launch_intra(p264hip_ctx *c, const PicDev *batch, const ScaleDev *scale, const LaunchPlan &pl)
{
    ScopedStamp t(c, 1);
    const uint8_t *is_intra = c->d_is_intra;
#define INTRA(kernel, ...) hipLaunchKernelGGL(kernel, grid_of(pl.intra_shape), dim3(pl.intra_shape.threads), (size_t)pl.info.intra_waves * sizeof(IntraLds), c->stream, \
                                              batch, c->g, c->d_status, is_intra, ##__VA_ARGS__)
    switch (pl.intra) {
    case IntraKernel::dense:         INTRA(k_intra); break;
    case IntraKernel::sparse:        INTRA(k_intra_sparse, c->d_edge, inv_mb_w(c), pl.info.edge_info_fused); break;      // (with the edge-info workgroups, if any)
    case IntraKernel::dense_i8:      INTRA(k_intra_i8); break;
    case IntraKernel::sparse_i8:     INTRA(k_intra_sparse_i8); break;
    case IntraKernel::dense_scaled:  INTRA(k_intra_scaled, scale); break;
    case IntraKernel::sparse_scaled: INTRA(k_intra_sparse_scaled, scale); break;
    }
#undef INTRA
}

// edge info (boundary strengths, averaged QPs per edge class: everything about an edge that does not depend on samples) where the
// intra launch did not carry it, then the loop filter
static void launch_deblock(p264hip_ctx *c, const PicDev *batch, const ScaleDev *scale, const LaunchPlan &pl)
{
    ScopedStamp t(c, 2);
    const Geom g = c->g;
    const dim3 grid = grid_of(pl.edge_shape), block(pl.edge_shape.threads);
    const p264hip_launch_info_t &li = pl.info;
    if (pl.deblock_cr) {                                     // (K4c: Cr's averaged QPs in the side array; such a batch is never fused)
        switch (pl.edge) {
        case EdgeInfoRoad::fused:         break;
        case EdgeInfoRoad::bs_by_picture: hipLaunchKernelGGL(k_deblock_bs_cr<true>, grid, block, 0, c->stream, batch, g, c->d_edge, inv_mb_w(c), scale, c->d_edge_cr); break;
        case EdgeInfoRoad::bs_by_index:   hipLaunchKernelGGL(k_deblock_bs_cr<false>, grid, block, 0, c->stream, batch, g, c->d_edge, inv_mb_w(c), scale, c->d_edge_cr); break;
        }
        hipLaunchKernelGGL(k_deblock_cr, grid_of(pl.deblock_shape), dim3(pl.deblock_shape.threads), 0, c->stream, batch, g,
                           (const EdgeInfo *)c->d_edge, c->d_status, li.pictures, li.deblock_rb_log2, li.deblock_pics_per_wg, li.deblock_odd_single, (const uint32_t *)c->d_edge_cr);
        return;
    }
    switch (pl.edge) {
    case EdgeInfoRoad::fused:         break;
    case EdgeInfoRoad::bs_by_picture: hipLaunchKernelGGL(k_deblock_bs<true>, grid, block, 0, c->stream, batch, g, c->d_edge, inv_mb_w(c)); break;
    case EdgeInfoRoad::bs_by_index:   hipLaunchKernelGGL(k_deblock_bs<false>, grid, block, 0, c->stream, batch, g, c->d_edge, inv_mb_w(c)); break;
    }
    hipLaunchKernelGGL(k_deblock, grid_of(pl.deblock_shape), dim3(pl.deblock_shape.threads), 0, c->stream, batch, g,
                       (const EdgeInfo *)c->d_edge, c->d_status, li.pictures, li.deblock_rb_log2, li.deblock_pics_per_wg, li.deblock_odd_single);
}

extern "C" int p264hip_reconstruct(p264hip_ctx *c, const int *pic_ids, const int *streams, int n)
{
    if (!c || !pic_ids || !streams || n < 1) return fail(P264HIP_EINVAL, "p264hip_reconstruct: bad argument");
    HIPCHK(hipSetDevice(c->device));
    int rc = expand_pending(c);                             // compact uploads since the last launch: one expansion kernel for all of them
    if (rc || (rc = batch_reserve(c, n)) || (rc = settle_unchecked(c, pic_ids, n))) return rc;
    const int r = c->ring; c->ring = (c->ring + 1) % BATCH_RING;
    HIPCHK(hipEventSynchronize(c->batch_free[r]));            // the copy that last used this staging buffer is done
    BatchKinds k;
    if ((rc = batch_fill(c, pic_ids, streams, n, c->h_batch[r], c->h_scale[r], &k))) return rc;
    const LaunchPlan plan = plan_launches(c->dev, c->knobs, k, n);
    if (plan.deblock_cr && (rc = edge_cr_reserve(c))) return rc;
    c->last = plan.info;
    // from here on work that reads the batch's input slots is (about to be) queued: the slots carry the new epoch BEFORE the first
    // launch, so that whichever way this function returns - a launch error half-way included - a later p264hip_input_reserve
    // of one of them waits for the stream instead of letting a peer overwrite a block under running kernels
    ++c->epoch;
    for (int i = 0; i < n; i++) stamp(c, c->pics[(size_t)pic_ids[i]]);
    ScopedStamp whole(c, 3);
    HIPCHK(hipMemcpyAsync(c->d_batch[r], c->h_batch[r], (size_t)n * sizeof(PicDev), hipMemcpyHostToDevice, c->stream));
    if (plan.copy_scale_table) HIPCHK(hipMemcpyAsync(c->d_scale[r], c->h_scale[r], (size_t)n * sizeof(ScaleDev), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->batch_free[r], c->stream));
    launch_inter(c, c->d_batch[r], c->d_scale[r], plan);
    launch_residual(c, c->d_batch[r], c->d_scale[r], plan);
    launch_intra(c, c->d_batch[r], c->d_scale[r], plan);
    launch_deblock(c, c->d_batch[r], c->d_scale[r], plan);
    HIPCHK(hipGetLastError());
    return P264HIP_OK;
}

extern "C" int64_t p264hip_upload_copies(p264hip_ctx *c) { return c ? (int64_t)c->upload_copies : -1; }

extern "C" int p264hip_last_launch(p264hip_ctx *c, p264hip_launch_info_t *out)
{
    if (!c || !out) return fail(P264HIP_EINVAL, "p264hip_last_launch: null argument");
    *out = c->last;
    return P264HIP_OK;
}

extern "C" int p264hip_submit(p264hip_ctx *c, int stream, const p264hip_picture_t *pic)
{
    if (!c || !pic || stream < 0 || stream >= c->n_streams || stream >= c->max_pictures)
        return fail(P264HIP_EINVAL, "p264hip_submit: bad argument (stream %d)", stream);
    int rc = p264hip_upload(c, stream, pic, 1);               // input slot `stream` is this stream's staging slot
    if (rc) return rc;
    return p264hip_reconstruct(c, &stream, &stream, 1);
}

extern "C" int p264hip_submit_async(p264hip_ctx *c, int stream, const p264hip_picture_t *pic)
{
    if (!c || !pic || stream < 0 || stream >= c->n_streams || stream >= c->max_pictures)
        return fail(P264HIP_EINVAL, "p264hip_submit_async: bad argument (stream %d)", stream);
    int rc = p264hip_upload_async(c, stream, pic);
    if (rc) return rc;
    return p264hip_reconstruct(c, &stream, &stream, 1);
}

static int drain_stamps(p264hip_ctx *c)
{
    for (auto &s : c->stamps) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { c->ms_sum[s.k] += ms; c->ms_cnt[s.k]++; }
        c->event_pool.push_back(s.a); c->event_pool.push_back(s.b);
    }
    c->stamps.clear();
    return 0;
}

extern "C" int p264hip_sync(p264hip_ctx *c)
{
    if (!c) return fail(P264HIP_EINVAL, "null context");
    HIPCHK(hipSetDevice(c->device));
    { const int rc = expand_pending(c); if (rc) return rc; }
    { const uint64_t upto = c->epoch; HIPCHK(hipStreamSynchronize(c->stream)); c->done_epoch = upto; }
    drain_stamps(c);
    int st = 0;
    HIPCHK(hipMemcpy(&st, c->d_status, sizeof st, hipMemcpyDeviceToHost));
    if (st) {
        (void)hipMemset(c->d_status, 0, sizeof(int));
        return fail(P264HIP_EHIP, "a macroblock-row dependency wait timed out on the device (status %d)", st);
    }
    return P264HIP_OK;
}

static int frame_io(p264hip_ctx *c, int stream, int slot, uint8_t *y, int ys, uint8_t *u, uint8_t *v, int cs, bool read)
{
    if (!c || stream < 0 || stream >= c->n_streams || slot < 0 || slot >= c->slots || !y || !u || !v || ys < c->g.w || cs < c->g.cw)
        return fail(P264HIP_EINVAL, "frame access: bad argument (stream %d slot %d strides %d/%d)", stream, slot, ys, cs);
    HIPCHK(hipSetDevice(c->device));
    int rc = p264hip_sync(c);
    // frames live in the strip layout on the device; the host sees planes, through a planar staging buffer
    if (rc || (rc = planar_staging(c))) return rc;
    const Geom &g = c->g;
    const size_t ysz = (size_t)g.w * g.h, csz = (size_t)g.cw * g.ch;
    uint8_t *s = c->d_planar;
    hipMemcpyKind k = read ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice;
    struct { uint8_t *host; int hs; uint8_t *dev; int w, h; } pl[3] = {
        { y, ys, s, g.w, g.h }, { u, cs, s + ysz, g.cw, g.ch }, { v, cs, s + ysz + csz, g.cw, g.ch } };
    if (read) {
        if ((rc = tile_convert(c, stream, slot, s, true))) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
        for (auto &p : pl) HIPCHK(hipMemcpy2D(p.host, (size_t)p.hs, p.dev, (size_t)p.w, (size_t)p.w, (size_t)p.h, k));
    } else {
        for (auto &p : pl) HIPCHK(hipMemcpy2D(p.dev, (size_t)p.w, p.host, (size_t)p.hs, (size_t)p.w, (size_t)p.h, k));
        if ((rc = tile_convert(c, stream, slot, s, false))) return rc;
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return P264HIP_OK;
}

extern "C" int p264hip_read_frame_async(p264hip_ctx *c, int stream, int slot, uint8_t *y, int ys, uint8_t *u, uint8_t *v, int cs)
{
    if (!c || stream < 0 || stream >= c->n_streams || slot < 0 || slot >= c->slots || !y || !u || !v || ys < c->g.w || cs < c->g.cw)
        return fail(P264HIP_EINVAL, "frame access: bad argument (stream %d slot %d strides %d/%d)", stream, slot, ys, cs);
    HIPCHK(hipSetDevice(c->device));
    int rc = planar_staging(c);
    if (rc || (rc = tile_convert(c, stream, slot, c->d_planar, true))) return rc;
    const Geom &g = c->g;
    const size_t ysz = (size_t)g.w * g.h, csz = (size_t)g.cw * g.ch;
    uint8_t *s = c->d_planar;
    HIPCHK(hipMemcpy2DAsync(y, (size_t)ys, s, (size_t)g.w, (size_t)g.w, (size_t)g.h, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpy2DAsync(u, (size_t)cs, s + ysz, (size_t)g.cw, (size_t)g.cw, (size_t)g.ch, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpy2DAsync(v, (size_t)cs, s + ysz + csz, (size_t)g.cw, (size_t)g.cw, (size_t)g.ch, hipMemcpyDeviceToHost, c->stream));
    return P264HIP_OK;
}

extern "C" int p264hip_read_frame(p264hip_ctx *c, int stream, int slot, uint8_t *y, int ys, uint8_t *u, uint8_t *v, int cs)
{ return frame_io(c, stream, slot, y, ys, u, v, cs, true); }

extern "C" int p264hip_write_frame(p264hip_ctx *c, int stream, int slot, const uint8_t *y, int ys, const uint8_t *u, const uint8_t *v, int cs)
{ return frame_io(c, stream, slot, (uint8_t *)y, ys, (uint8_t *)u, (uint8_t *)v, cs, false); }

extern "C" int p264hip_timing_enable(p264hip_ctx *c, int on)
{
    if (!c) return fail(P264HIP_EINVAL, "null context");
    int rc = p264hip_sync(c);
    c->timing = on != 0;
    return rc;
}

extern "C" int p264hip_timing_reset(p264hip_ctx *c)
{
    if (!c) return fail(P264HIP_EINVAL, "null context");
    int rc = p264hip_sync(c);
    for (int i = 0; i < P264HIP_NKERNELS; i++) { c->ms_sum[i] = 0; c->ms_cnt[i] = 0; }
    return rc;
}

extern "C" int p264hip_timing_read(p264hip_ctx *c, double ms_sum[P264HIP_NKERNELS], int64_t count[P264HIP_NKERNELS])
{
    if (!c || !ms_sum || !count) return fail(P264HIP_EINVAL, "null argument");
    int rc = p264hip_sync(c);
    for (int i = 0; i < P264HIP_NKERNELS; i++) { ms_sum[i] = c->ms_sum[i]; count[i] = c->ms_cnt[i]; }
    return rc;
}
