// conv_device.h -- device primitives shared by the conv*.hip units and plan.hip: what a kernel and the packed weights / arena agree on
// (wait counts, XCD-aware order, half-wave swap, hi + lo planes) lives here once.  Inline functions and typedefs only: no kernels, no
// __shared__ objects, no loads that the call sites do not issue themselves.  Everything is internal to the including unit.
#pragma once
#include <hip/hip_runtime.h>
#include "plan.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) void lds_void;
typedef const __attribute__((address_space(1))) void gbl_void;

// one LDS-DMA request: 16 bytes per lane from g (uniform base + per-lane offset) to the wave's 1 KiB at s (wave-uniform)
__device__ __forceinline__ void lds_dma16(const char* g, char* s)
{
    __builtin_amdgcn_global_load_lds((gbl_void*)g, (lds_void*)s, 16, 0, 0);
}

// s_waitcnt vmcnt(n) for a value that is a constant after unrolling (the switch folds away).  The table covers the whole six-bit
// field; anything else becomes vmcnt(0), which is correct and slow.
__device__ __forceinline__ void wait_vm(int n)
{
    switch (n) {
#define W_(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
#define W8_(a, b, c, d, e, f, g, h) W_(a) W_(b) W_(c) W_(d) W_(e) W_(f) W_(g) W_(h)
        W8_(0, 1, 2, 3, 4, 5, 6, 7) W8_(8, 9, 10, 11, 12, 13, 14, 15) W8_(16, 17, 18, 19, 20, 21, 22, 23) W8_(24, 25, 26, 27, 28, 29, 30, 31)
        W8_(32, 33, 34, 35, 36, 37, 38, 39) W8_(40, 41, 42, 43, 44, 45, 46, 47) W8_(48, 49, 50, 51, 52, 53, 54, 55) W8_(56, 57, 58, 59, 60, 61, 62, 63)
#undef W8_
#undef W_
        default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
}

// every LDS read of this wave has returned, then the workgroup barrier (raw: an LDS-DMA in flight must survive it).  Two forms, on purpose:
__device__ __forceinline__ void lds_barrier_asm()
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}
// the BUILTIN, not inline asm: hipcc's wait-count pass then knows that the fragment set read before the barrier has landed and puts no
// lgkmcnt(0) in front of the MFMAs that use it behind the barrier (gfx9 encoding: vmcnt = 63 and expcnt = 7 "don't wait", lgkmcnt = 0)
__device__ __forceinline__ void lds_reads_landed() { __builtin_amdgcn_s_waitcnt(0xC07F); }
__device__ __forceinline__ void lds_barrier_builtin()
{
    lds_reads_landed();
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// XCD-aware block order: blocks b, b+8, b+16.. run on one XCD; each XCD gets a contiguous range of logical tiles, so that
// neighbouring tiles (the N tiles of one M tile, which re-read the same activation rows) share an L2.
__device__ __forceinline__ int xcd_logical_block()
{
    const int nblk = gridDim.x, bid = blockIdx.x;
    const int q = nblk >> 3, r = nblk & 7, xcd = bid & 7, loc = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// ---- register epilogue.  With the weights as the first MFMA operand a lane holds channels 8*g + 4*lhi + e (e = 0..3) of one pixel in
//      acc[4*g + e]; swapping x = acc[8*j + e], y = acc[8*j + 4 + e] between the half-waves leaves acc[8*j .. 8*j + 7] = 8 consecutive
//      channels 16*j + 8*lhi .. +7: one 16-byte NHWC access per plane.
// Pass VALUES copied out of the accumulator: a bit_cast of a vector ELEMENT lvalue reads element 0.
__device__ __forceinline__ float2 halfwave_swap(float x, float y)
{
    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(y), false, false);
    const unsigned s0 = sw[0], s1 = sw[1];
    return make_float2(__uint_as_float(s0), __uint_as_float(s1));
}

__device__ __forceinline__ void relu16(f32x16& c)               // NaN stays NaN (torch's ReLU)
{
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = c[r] < 0.f ? 0.f : c[r];
}

// c[8*j .. 8*j + 7] += eight channels of a residual / skip tensor read as NPL planes (hi, or hi + lo: exact in fp32)
template <int NPL>
__device__ __forceinline__ void add_planes8(f32x16& c, int j, const half8 (&h)[NPL])
{
#pragma unroll
    for (int e = 0; e < 8; ++e) c[8 * j + e] += NPL == 2 ? (float)h[0][e] + (float)h[NPL - 1][e] : (float)h[0][e];
}

}  // namespace
