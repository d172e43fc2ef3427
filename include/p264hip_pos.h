/* p264hip_pos.h - the ONE definition of the bilinear filter's source position (include/p264hip.h: p264hip_resize_t, "Taps"), in
 * plain C so that the host (csrc/host/resize_layout.c: p264hip_resize_taps) and the device (csrc/hip/kernel_roi.h: k_roi_taps) compile
 * the same text: the CPU tests of p264hip_resize_taps pin the arithmetic the device runs.
 *
 *   pos(d) = clamp( floor(((2d+1)*S*256 + D) / (2D)) - 128,  0,  (S-1)*256 )
 *
 * for 1 <= S, D <= 2^20 and 0 <= d < D.  The dividend needs 64 bits (up to 2^50); where it fits 32 - every axis of 1080p to
 * 224 x 224 - the division is a 32-bit one, which a GPU runs several times faster than the 64-bit one.  Both give the same floor. */
#ifndef P264HIP_POS_H
#define P264HIP_POS_H
#include <stdint.h>

#ifdef __HIPCC__
#define P264HIP_POS_FN __host__ __device__ static inline
#else
#define P264HIP_POS_FN static inline
#endif

P264HIP_POS_FN int32_t p264hip_resize_pos(int32_t src_n, int32_t dst_n, int32_t d)
{
    const uint64_t num = (2 * (uint64_t)d + 1) * (uint64_t)src_n * 256 + (uint64_t)dst_n;
    const uint32_t den = 2 * (uint32_t)dst_n;
    const int64_t q = (num >> 32) ? (int64_t)(num / den) : (int64_t)((uint32_t)num / den);
    const int64_t p = q - 128, last = ((int64_t)src_n - 1) * 256;
    return (int32_t)(p < 0 ? 0 : p > last ? last : p);
}
#endif
