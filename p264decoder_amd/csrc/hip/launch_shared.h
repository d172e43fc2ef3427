// launch_shared.h - what the launch plan (launch_plan.h) and the kernels both have to know: workgroup sizes and caps, and the layout
// of the motion-compensation work lists.  Plain C++: it compiles without HIP, so the plan can be checked on a machine without a GPU.
// Each constant is defined here and nowhere else; the kernel header named beside it says what it means for the kernel.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define P264_HOST_DEVICE __host__ __device__
#else
#define P264_HOST_DEVICE
#endif

#define ROW_WAVES       16           // wavefronts per picture workgroup (1024 threads) (wavefront_sync.h, kernel_deblock.h)
#define INTRA_ROW_WAVES 16           // most wavefronts per picture workgroup (kernel_intra.h)
#define INTRA_BS_WGS    1            // edge-info workgroups per picture inside the k_intra_sparse launch (kernel_intra.h, with the measurements)
#define DB_LAG          1            // columns a row of a k_deblock band lags behind the row above it (kernel_deblock.h)
#define MAX_PICS_PER_WG 16           // pictures one k_deblock workgroup serves (in groups of as many as a wavefront holds)
#define T8_THREADS      256          // k_t8x8 (kernel_t8x8.h) and k_scaled_inter (kernel_scaling.h): one wavefront per two macroblocks
#define T8_MBS_PER_WG   (T8_THREADS / 32)
#define MC_SORT_THREADS 1024         // k_mc_sort* (kernel_mc_sort.h): one workgroup per picture

// ---- the work lists of the motion-compensation stage (kernel_mc_sort.h writes them, kernel_mc.h reads them) ----
#define MCY_KEYS    32               // luma keys per band: phase class | MCY_CLAMP | MCY_RESID (kernel_mc_sort.h)
#define MCC_KEYS    8                // chroma keys per band: MCC_CLAMP | MCC_RESID | MCC_BI
enum { ML_YM = 0, ML_YQ = 1, ML_CM = 2, ML_CQ = 3, ML_LISTS = 4 };      // luma macroblocks, luma quadrants, chroma macroblocks, chroma quadrants
#define MC_MAX_BANDS 32
P264_HOST_DEVICE static inline int mc_chunk_items(int l) { return l == ML_YM ? 4 : l == ML_YQ ? 16 : l == ML_CM ? 8 : 32; }   // items per wavefront
P264_HOST_DEVICE static inline int mc_list_keys(int l) { return l < ML_CM ? MCY_KEYS : MCC_KEYS; }

// Per-picture scratch written by k_mc_sort (32-bit words): [l] chunks in use of list l, then per list one class byte
// per chunk, then the lists (their entries: "list entries", kernel_mc_sort.h).  Same layout for every picture of a batch.
P264_HOST_DEVICE static inline uint32_t mc_entry_words(int pass) { return pass ? 4u : 2u; }
struct McLayout {
    uint32_t band_log2, n_bands;
    uint32_t max_chunks[2 * ML_LISTS], off_cls[2 * ML_LISTS], off_list[2 * ML_LISTS], words;     // [pass * ML_LISTS + list]
};
static inline McLayout mc_layout(int mb_w, int mb_h, int band_log2)
{
    McLayout L;
    L.band_log2 = (uint32_t)band_log2;
    L.n_bands = (uint32_t)((mb_h + (1 << band_log2) - 1) >> band_log2);
    const uint32_t n_mb = (uint32_t)(mb_w * mb_h);
    uint32_t at = 16;
    for (int l = 0; l < 2 * ML_LISTS; l++) {
        const int t = l % ML_LISTS;
        const uint32_t items = (t == ML_YM || t == ML_CM) ? n_mb : n_mb * 4u, per = (uint32_t)mc_chunk_items(t);
        L.max_chunks[l] = (items + L.n_bands * (uint32_t)mc_list_keys(t) * (per - 1)) / per + 1;
        L.off_cls[l] = at; at += (L.max_chunks[l] + 3) / 4;
    }
    at = (at + 15) & ~15u;
    for (int l = 0; l < 2 * ML_LISTS; l++) { L.off_list[l] = at; at += L.max_chunks[l] * (uint32_t)mc_chunk_items(l % ML_LISTS) * mc_entry_words(l / ML_LISTS); }
    L.words = (at + 63) & ~63u;
    return L;
}
