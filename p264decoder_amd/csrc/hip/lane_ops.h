// lane_ops.h - wavefront, buffer and byte plumbing shared by the kernels: packed 16-bit views, byte-parallel averages, raw buffer
// loads and stores through a descriptor, exchanges among the four lanes of a quad, the shift-saturate-pack of four samples.
// Nothing here knows about a stage.
#pragma once
#include "device_common.h"

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

__device__ __forceinline__ uint32_t alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbyte(hi, lo, sh); }
__device__ __forceinline__ s16x2 as_s16x2(uint32_t v) { return __builtin_bit_cast(s16x2, v); }
__device__ __forceinline__ uint32_t as_u32(s16x2 v) { return __builtin_bit_cast(uint32_t, v); }
// byte-parallel (a + b + 1) >> 1 (pixel_avg, core/mc.c:58-74)
__device__ __forceinline__ uint32_t avg4(uint32_t a, uint32_t b) { return (a | b) - (((a ^ b) & 0xfefefefeu) >> 1); }
__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int d) { return (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16) | ((uint32_t)d << 24); }
__device__ __forceinline__ uint32_t sel32(bool c, uint32_t a, uint32_t b) { return c ? a : b; }

__device__ __forceinline__ rsrc_t make_rsrc(const void *base, uint32_t bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void *)base, (short)0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ uint32_t bload(rsrc_t r, uint32_t off) { return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(r, (int)off, 0, 0); }
__device__ __forceinline__ void bstore(rsrc_t r, uint32_t off, uint32_t v) { __builtin_amdgcn_raw_buffer_store_b32((int)v, r, (int)off, 0, 0); }
__device__ __forceinline__ u32x4 bload4(rsrc_t r, uint32_t off) { return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0)); }
// reconstructed samples are written once and not read again by this stage: non-temporal stores keep them from pushing
// reference lines out of L2 (measured: -3 % on the stage)
#define MC_ST_AUX 2
__device__ __forceinline__ u32x2 bload2(rsrc_t r, uint32_t off) { return __builtin_bit_cast(u32x2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)off, 0, 0)); }
// (the 8-byte stores of quadrant items fill half a 16-byte row each: left to L2 to merge - non-temporal they cost 0.27 GB of
// extra HBM writes per launch)
#define MC_ST2_AUX 0
__device__ __forceinline__ void bstore2(rsrc_t r, uint32_t off, uint32_t a, uint32_t b)
{
    const u32x2 v = { a, b }; __builtin_amdgcn_raw_buffer_store_b64(v, r, (int)off, 0, MC_ST2_AUX);
}
// a reference-window load
__device__ __forceinline__ u32x4 wload4(rsrc_t r, uint32_t off) { return bload4(r, off); }
// the value of lane ^ 1 / lane ^ 2 (inside a group of four lanes: DPP quad_perm, no LDS traffic)
__device__ __forceinline__ uint32_t lane_xor1(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t lane_xor2(uint32_t v) { return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, true); }
// 4x4 dword transpose among the four lanes of a quad: t[k] of lane L = x[L] of lane k (two exchange steps)
__device__ __forceinline__ void quad_transpose(uint32_t (&t)[4], const uint32_t (&x)[4], int lane)
{
    const bool b0 = lane & 1, b1 = lane & 2;
    uint32_t a[4];
#pragma unroll
    for (int i = 0; i < 4; i += 2) {                       // with lane ^ 1: a[i + j] = x[i + b0] of lane (L & ~1) + j
        const uint32_t r = lane_xor1(b0 ? x[i] : x[i + 1]);
        a[i] = b0 ? r : x[i]; a[i + 1] = b0 ? x[i + 1] : r;
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {                          // with lane ^ 2
        const uint32_t r = lane_xor2(b1 ? a[j] : a[2 + j]);
        t[j] = b1 ? r : a[j]; t[2 + j] = b1 ? a[2 + j] : r;
    }
}
__device__ __forceinline__ void bstore4(rsrc_t r, uint32_t off, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const u32x4 v = { a, b, c, d }; __builtin_amdgcn_raw_buffer_store_b128(v, r, (int)off, 0, MC_ST_AUX);
}

// "all of these loads have been issued, and their data is used HERE": keeps the compiler from sinking a load into the conditional
// block that stores its data (behind the waits and the stores of the loads in front of it)
__device__ __forceinline__ void loads_land(u32x4 &v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// (t >> sh) clipped to a byte, four at once: gfx950's v_ashr_pk_u8_i32 shifts, saturates and packs two values per
// instruction (result bits 16..31 are not defined: only its low two bytes are used)
template <int SH> __device__ __forceinline__ uint32_t round_pack4(const int t[4])
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_ashr_pk_u8_i32(t[0], t[1], SH), hi = (uint32_t)__builtin_amdgcn_ashr_pk_u8_i32(t[2], t[3], SH);
    return perm(hi, lo, 0x05040100u);
}
