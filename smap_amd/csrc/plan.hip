// plan.hip -- static inference schedule executor for SMAP.forward (model/smap.py:403-419)
// plus the non-GEMM kernels of the backbone:
//   stem_kernel     ResNet_top conv 7x7 s2 p3 + folded BN + ReLU   (smap.py:83-84, 88-90)
//   maxpool_kernel  MaxPool2d(3, 2, 1)                              (smap.py:86)
//   upadd_kernel    relu(a + bilinear_align_corners(t))             (smap.py:213-217)
//   headsum_kernel  res4 + up(res3) + up(res2) -> fp32 NCHW         (smap.py:221-229, 417-419)
// The schedule itself (which op, which buffers) is built by the Python host
// (smap_amd/plan.py) and handed over as a flat array of smap_op; this file only
// launches it, op after op, on one HIP stream -- capturable into a hipGraph.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <new>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <climits>
#include <vector>
#include <type_traits>
#include "smap_hip.h"
#include "plan.h"
#include "plan_check.h"
#include "conv_device.h"
#include "hip_rc.h"

namespace {

// ------------------------------------------------------------------ stem --
// ResNet_top conv 7x7 s2 p3, 3 -> 64, + folded BN + ReLU, fp32 NCHW image -> NHWC fp16.
// Implicit GEMM on the matrix cores with the im2col done by the LDS read addresses:
//   K order = (kh, c, kw padded 7->8): one 8-wide K granule = 8 consecutive input columns of one
//   (kh, c) row of the patch, i.e. 16 contiguous bytes of the fp16 patch in LDS; 21 granules + 1
//   zero granule = 22 = 11 MFMA K-steps of 16.  Weights (A operand, [64][176] fp16) and the
//   37x38x3 input patch (B operand) both sit in LDS; D[n][pixel] puts 4 consecutive channels of
//   one pixel in a lane, so the NHWC store is 8 bytes per lane with no transposition.
// One 16x16 output tile per workgroup, 64 pixels x 64 channels per wave (4 accumulators).
#ifndef SMAP_STEM_STORE16
#define SMAP_STEM_STORE16 1
#endif
constexpr int ST_T = 16, ST_PH = ST_T * 2 + 5, ST_PW = 40;     // tile edge, patch rows, padded patch row (halves)
constexpr int ST_K = SMAP_STEM_K;                              // 22 granules x 8 = 176

// The images of a schedule may come as up to SMAP_MAX_INPUTS separate [frames_per,3,H,W] buffers (smap_plan_run_inputs: a
// launch that coalesces several of the caller's batches reads them where they are -- no gather copy in front of the stem).
struct StemIn {
    const float* p[SMAP_MAX_INPUTS];
    int frames_per;                     // frames per buffer; frame b lives in p[b / frames_per] at index b % frames_per
};
__device__ __forceinline__ const float* stem_frame(const StemIn& in, int b, int H, int W)
{
    const int k = b / in.frames_per;
    const float* base = in.p[0];        // compile-time indices only: a run-time index into a by-value kernel argument would
#pragma unroll                          // be promoted to scratch / LDS (EXPERIMENTS R3.6)
    for (int j = 1; j < SMAP_MAX_INPUTS; ++j) base = k == j ? in.p[j] : base;
    return base + (size_t)(b - k * in.frames_per) * 3 * H * W;
}

// X3 (smap_op.precision = 1): image and weights as fp16 hi/lo pairs, three MFMAs per K step, output pixel = [hi(64) | lo(64)]
// (see conv.hip).  The weight blob then holds [64][176] hi followed by [64][176] lo of (w * 2^s); acc_scale = 2^-s.
template <bool X3>
__global__ __launch_bounds__(256) void stem_kernel(const StemIn in, const _Float16* __restrict__ wk,
                                                   const float* __restrict__ bias, _Float16* __restrict__ out,
                                                   int H, int W, int Ho, int Wo, float acc_scale, int flip_from)
{
    constexpr int NPL = X3 ? 2 : 1;
    __shared__ __attribute__((aligned(16))) _Float16 s_w[NPL * 64 * ST_K];
    __shared__ __attribute__((aligned(16))) _Float16 s_p[NPL * 3 * ST_PH * ST_PW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, oy0 = blockIdx.y * ST_T, ox0 = blockIdx.x * ST_T;
    for (int i = tid; i < NPL * 64 * ST_K / 8; i += 256)
        reinterpret_cast<half8*>(s_w)[i] = reinterpret_cast<const half8*>(wk)[i];
    const int iy0 = oy0 * 2 - 3, ix0 = ox0 * 2 - 3;
    // flip-TTA: frames >= flip_from are the x-mirrored images of frames 0.. (the mirror lives in this index, not in memory)
    const bool mirror = flip_from > 0 && b >= flip_from;
    const int bsrc = mirror ? b - flip_from : b;
    const float* __restrict__ img = stem_frame(in, bsrc, H, W);
    for (int i = tid; i < 3 * ST_PH * ST_PW; i += 256) {
        const int c = i / (ST_PH * ST_PW), r = i - c * ST_PH * ST_PW;
        const int py = r / ST_PW, px = r - py * ST_PW;
        const int iy = iy0 + py, ix = ix0 + px;
        float v = 0.f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
            v = img[((size_t)c * H + iy) * W + (mirror ? W - 1 - ix : ix)];
        const _Float16 hi = (_Float16)v;
        s_p[i] = hi;
        if (X3) s_p[3 * ST_PH * ST_PW + i] = (_Float16)(v - (float)hi);
    }
    __syncthreads();
    const int l31 = lane & 31, lhi = lane >> 5;
    f32x16 acc[2][2];                                          // [channel tile][pixel tile]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // this lane's two pixels (B operand columns): pixel tile t covers output rows 4*wave+2t, +1
    int pbase[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int py = 4 * wave + 2 * t + (l31 >> 4), px = l31 & 15;
        pbase[t] = (py * 2) * ST_PW + px * 2;                  // halves; + (c*ST_PH + kh)*ST_PW per granule
    }
#pragma unroll
    for (int ks = 0; ks < ST_K / 16; ++ks) {
        int g = ks * 2 + lhi;                                  // K granule of this half-wave
        const int gg = g < 21 ? g : 20;                        // granule 21 has zero weights: any in-bounds read
        const int kh = gg / 3, c = gg - kh * 3;
        const int goff = (c * ST_PH + kh) * ST_PW;
        half8 wf[NPL][2], pf[NPL][2];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                wf[pl][nt] = *reinterpret_cast<const half8*>(s_w + pl * 64 * ST_K + (nt * 32 + l31) * ST_K + g * 8);
#pragma unroll
            for (int t = 0; t < 2; ++t) {                      // 8 consecutive columns, 4-byte aligned: 4 x b32
                const unsigned* q = reinterpret_cast<const unsigned*>(s_p + pl * 3 * ST_PH * ST_PW + pbase[t] + goff);
                union { unsigned u[4]; half8 h; } cv;
                cv.u[0] = q[0]; cv.u[1] = q[1]; cv.u[2] = q[2]; cv.u[3] = q[3] & 0xffffu;      // column 8 has weight 0: a NaN / inf there is not in the window
                pf[pl][t] = cv.h;
            }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (X3) {
                    acc[nt][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[NPL - 1][nt], pf[0][t], acc[nt][t], 0, 0, 0);
                    acc[nt][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[0][nt], pf[NPL - 1][t], acc[nt][t], 0, 0, 0);
                }
                acc[nt][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[0][nt], pf[0][t], acc[nt][t], 0, 0, 0);
            }
    }
    // D[n][pixel]: lane = pixel (col l31), reg r -> channel nt*32 + (r&3) + 8*(r>>2) + 4*lhi.  The half-wave swap of convp.hip's
    // register epilogue turns a lane's 4 + 4 channels (8 apart) into 8 consecutive ones: 16-byte NHWC stores instead of 8-byte ones
    // (SMAP_STEM_STORE16 = 0: the round-1 form).
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int oy = oy0 + 4 * wave + 2 * t + (l31 >> 4), ox = ox0 + (l31 & 15);
        const bool ok = oy < Ho && ox < Wo;
        _Float16* op = out + (((size_t)b * Ho + (ok ? oy : 0)) * Wo + (ok ? ox : 0)) * (NPL * 64);
#if SMAP_STEM_STORE16
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                float v[8];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float2 sw = halfwave_swap(acc[nt][t][8 * j + e], acc[nt][t][8 * j + 4 + e]);    // channels 16j + e + 4 lhi and + 8
                    v[e] = sw.x;
                    v[4 + e] = sw.y;
                }
                const int n0 = nt * 32 + 16 * j + 8 * lhi;     // this lane now holds channels n0 .. n0 + 7 of its pixel
                const float4 b0 = *reinterpret_cast<const float4*>(bias + n0), b1 = *reinterpret_cast<const float4*>(bias + n0 + 4);
                const float bb[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
                half8 h, l;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float x = X3 ? v[e] * acc_scale + bb[e] : v[e] + bb[e];
                    x = x < 0.f ? 0.f : x;                     // NaN stays NaN (torch's ReLU)
                    h[e] = (_Float16)x;
                    l[e] = (_Float16)(x - (float)h[e]);
                }
                if (!ok) continue;
                *reinterpret_cast<half8*>(op + n0) = h;
                if (X3) *reinterpret_cast<half8*>(op + 64 + n0) = l;
            }
#else
        if (!ok) continue;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n0 = nt * 32 + 8 * q + 4 * lhi;
                const float4 bv = *reinterpret_cast<const float4*>(bias + n0);
                const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
                half4 h, l;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = X3 ? acc[nt][t][4 * q + e] * acc_scale + bb[e] : acc[nt][t][4 * q + e] + bb[e];
                    v = v < 0.f ? 0.f : v;                 // NaN stays NaN (torch's ReLU)
                    h[e] = (_Float16)v;
                    l[e] = (_Float16)(v - (float)h[e]);
                }
                *reinterpret_cast<half4*>(op + n0) = h;
                if (X3) *reinterpret_cast<half4*>(op + 64 + n0) = l;
            }
#endif
    }
}

// ------------------------------------------------------- stem + max-pool --
// ResNet_top in one kernel (smap.py:83-86): the 7x7 s2 conv + BN + ReLU of stem_kernel, then the 3x3 s2 p1 max-pool
// straight from LDS.  stem_kernel is bound by its 109 MB (B = 8) output write and maxpool_kernel reads that tensor
// back; here only the pooled 27 MB leave the CU.  A workgroup owns 8 x 7 pooled pixels = 17 x 15 conv pixels (255 of
// the 256 MFMA pixel columns; the one-pixel halo is recomputed: +14 % conv work on a store-bound kernel).  Conv pixels
// outside the image take the value 0 in the LDS tile: every real value is >= 0 after the ReLU, so a 0 never changes a
// window maximum -- the same result as MaxPool2d's -inf padding.
constexpr int SP_PY = 8, SP_PX = 7, SP_SY = 2 * SP_PY + 1, SP_SX = 2 * SP_PX + 1;       // pooled tile, conv tile (17 x 15)
constexpr int SP_PH = (SP_SY - 1) * 2 + 7, SP_PW = 40;                                  // input patch rows (39), padded row
static_assert(SP_SY * SP_SX <= 256 && (SP_SX - 1) * 2 + 8 <= SP_PW, "stem+pool tile");

// X3 / flip_from: as in stem_kernel (hi/lo planes, three MFMAs per K step, mirrored read of frames >= flip_from); the conv
// tile then stays in LDS as fp32 (the maximum is taken over the exact value, then re-split).
template <bool X3>
__global__ __launch_bounds__(256) void stem_pool_kernel(const StemIn in, const _Float16* __restrict__ wk,
                                                        const float* __restrict__ bias, _Float16* __restrict__ out,
                                                        int H, int W, int Hs, int Ws, int Ho, int Wo, float acc_scale, int flip_from)
{
    constexpr int NPL = X3 ? 2 : 1;
    typedef typename std::conditional<X3, float, _Float16>::type tile_t;
    __shared__ __attribute__((aligned(16))) _Float16 s_w[NPL * 64 * ST_K];
    __shared__ __attribute__((aligned(16))) _Float16 s_p[NPL * 3 * SP_PH * SP_PW];
    __shared__ __attribute__((aligned(16))) tile_t s_t[256 * 64];                       // conv tile, [pixel slot][channel]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.z, py0 = blockIdx.y * SP_PY, px0 = blockIdx.x * SP_PX;
    const int sy0 = py0 * 2 - 1, sx0 = px0 * 2 - 1;                                     // first conv pixel of the tile
    for (int i = tid; i < NPL * 64 * ST_K / 8; i += 256)
        reinterpret_cast<half8*>(s_w)[i] = reinterpret_cast<const half8*>(wk)[i];
    const int iy0 = sy0 * 2 - 3, ix0 = sx0 * 2 - 3;
    const bool mirror = flip_from > 0 && b >= flip_from;
    const int bsrc = mirror ? b - flip_from : b;
    const float* __restrict__ img = stem_frame(in, bsrc, H, W);
    for (int i = tid; i < 3 * SP_PH * SP_PW; i += 256) {
        const int c = i / (SP_PH * SP_PW), r = i - c * SP_PH * SP_PW;
        const int py = r / SP_PW, px = r - py * SP_PW;
        const int iy = iy0 + py, ix = ix0 + px;
        float v = 0.f;
        if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
            v = img[((size_t)c * H + iy) * W + (mirror ? W - 1 - ix : ix)];
        const _Float16 hi = (_Float16)v;
        s_p[i] = hi;
        if (X3) s_p[3 * SP_PH * SP_PW + i] = (_Float16)(v - (float)hi);
    }
    __syncthreads();
    const int l31 = lane & 31, lhi = lane >> 5;
    f32x16 acc[2][2];                                          // [channel tile][pixel tile]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // pixel slot s = wave*64 + t*32 + l31 -> conv pixel (s / 15, s % 15) of the 17 x 15 tile (slot 255 is a spare)
    int pbase[2], slot[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int sl = wave * 64 + t * 32 + l31;
        const int sc = sl < SP_SY * SP_SX ? sl : 0;
        const int py = sc / SP_SX, px = sc - py * SP_SX;
        slot[t] = sl;
        pbase[t] = (py * 2) * SP_PW + px * 2;
    }
#pragma unroll
    for (int ks = 0; ks < ST_K / 16; ++ks) {
        int g = ks * 2 + lhi;
        const int gg = g < 21 ? g : 20;
        const int kh = gg / 3, c = gg - kh * 3;
        const int goff = (c * SP_PH + kh) * SP_PW;
        half8 wf[NPL][2], pf[NPL][2];
#pragma unroll
        for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
            for (int nt = 0; nt < 2; ++nt)
                wf[pl][nt] = *reinterpret_cast<const half8*>(s_w + pl * 64 * ST_K + (nt * 32 + l31) * ST_K + g * 8);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const unsigned* q = reinterpret_cast<const unsigned*>(s_p + pl * 3 * SP_PH * SP_PW + pbase[t] + goff);
                union { unsigned u[4]; half8 h; } cv;
                cv.u[0] = q[0]; cv.u[1] = q[1]; cv.u[2] = q[2]; cv.u[3] = q[3] & 0xffffu;      // column 8 has weight 0: a NaN / inf there is not in the window
                pf[pl][t] = cv.h;
            }
        }
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                if (X3) {
                    acc[nt][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[NPL - 1][nt], pf[0][t], acc[nt][t], 0, 0, 0);
                    acc[nt][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[0][nt], pf[NPL - 1][t], acc[nt][t], 0, 0, 0);
                }
                acc[nt][t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[0][nt], pf[0][t], acc[nt][t], 0, 0, 0);
            }
    }
    // bias + ReLU -> conv tile in LDS (zero where the conv pixel lies outside the image)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int sl = slot[t];
        const int py = sl / SP_SX, px = sl - py * SP_SX;
        const int sy = sy0 + py, sx = sx0 + px;
        const bool live = sl < SP_SY * SP_SX && (unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int n0 = nt * 32 + 8 * q + 4 * lhi;
                const float4 bv = *reinterpret_cast<const float4*>(bias + n0);
                const float bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float v = X3 ? acc[nt][t][4 * q + e] * acc_scale + bb[e] : acc[nt][t][4 * q + e] + bb[e];
                    v = (!live || v < 0.f) ? 0.f : v;          // NaN stays NaN
                    s_t[sl * 64 + n0 + e] = (tile_t)v;
                }
            }
    }
    __syncthreads();
    // 3x3 s2 max over the conv tile: pooled pixel (py, px) reads conv rows 2py..2py+2, cols 2px..2px+2 of the tile
    for (int i = tid; i < SP_PY * SP_PX * 8; i += 256) {
        const int cg = i & 7, pp = i >> 3;
        const int py = pp / SP_PX, px = pp - py * SP_PX;
        const int oy = py0 + py, ox = px0 + px;
        if (oy >= Ho || ox >= Wo) continue;
        float m[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = (float)s_t[((2 * py) * SP_SX + 2 * px) * 64 + cg * 8 + e];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                if (dy == 0 && dx == 0) continue;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float x = (float)s_t[((2 * py + dy) * SP_SX + 2 * px + dx) * 64 + cg * 8 + e];
                    m[e] = (x > m[e] || x != x) ? x : m[e];    // ATen's rule: NaN sticks
                }
            }
        half8 h;
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (_Float16)m[e];
        _Float16* op = out + (((size_t)b * Ho + oy) * Wo + ox) * (NPL * 64) + cg * 8;
        *reinterpret_cast<half8*>(op) = h;
        if (X3) {
            half8 l;
#pragma unroll
            for (int e = 0; e < 8; ++e) l[e] = (_Float16)(m[e] - (float)h[e]);
            *reinterpret_cast<half8*>(op + 64) = l;
        }
    }
}

// --------------------------------------------------------------- maxpool --
// NHWC fp16, 3x3 stride 2 pad 1 (padding never wins: only in-range taps are read).
// X3: pixel = [hi(C) | lo(C)]; the maximum is taken over hi + lo (exact in fp32) and the winner's own pair is stored (re-splitting the
// sum would turn (odd hi, lo = half an ulp of it) into (the even neighbour, -lo): the same value, another pair).
template <bool X3>
__global__ void maxpool_kernel(const _Float16* __restrict__ in, _Float16* __restrict__ out, int B, int H, int W,
                               int C, int Ho, int Wo)
{
    constexpr int NPL = X3 ? 2 : 1;
    const int cg_n = C / 8;
    const long long total = (long long)B * Ho * Wo * cg_n;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int cg = (int)(idx % cg_n);
        long long pix = idx / cg_n;
        const int ox = (int)(pix % Wo);
        pix /= Wo;
        const int oy = (int)(pix % Ho), b = (int)(pix / Ho);
        float m[8];
        half8 h, l;                                            // X3: the winner's pair
#pragma unroll
        for (int e = 0; e < 8; ++e) { m[e] = -INFINITY; h[e] = (_Float16)-INFINITY; l[e] = (_Float16)0.f; }
        for (int dy = 0; dy < 3; ++dy) {
            const int iy = oy * 2 - 1 + dy;
            if ((unsigned)iy >= (unsigned)H) continue;
            for (int dx = 0; dx < 3; ++dx) {
                const int ix = ox * 2 - 1 + dx;
                if ((unsigned)ix >= (unsigned)W) continue;
                const _Float16* ip = in + (((size_t)b * H + iy) * W + ix) * (NPL * C) + cg * 8;
                const half8 v = *reinterpret_cast<const half8*>(ip);
                if (X3) {
                    const half8 vl = *reinterpret_cast<const half8*>(ip + C);
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float x = (float)v[e] + (float)vl[e];
                        const bool take = x > m[e] || x != x;  // ATen's rule: NaN sticks
                        m[e] = take ? x : m[e];
                        h[e] = take ? v[e] : h[e];
                        l[e] = take ? vl[e] : l[e];
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { const float x = (float)v[e]; m[e] = (x > m[e] || x != x) ? x : m[e]; }
                }
            }
        }
        if (!X3) {
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (_Float16)m[e];
        }
        _Float16* op = out + (((size_t)b * Ho + oy) * Wo + ox) * (NPL * C) + cg * 8;
        *reinterpret_cast<half8*>(op) = h;
        if (X3) *reinterpret_cast<half8*>(op + C) = l;
    }
}

// bilinear align-corners index rule: lerp_index() in plan.h (shared with the conv epilogue)

// out = relu(a + up(t)); a/out [B,Ho,Wo,C] fp16, t [B,h,w,C] fp16; 8 channels per thread.
__global__ void upadd_kernel(const _Float16* __restrict__ a, const _Float16* __restrict__ t,
                             _Float16* __restrict__ out, int B, int Ho, int Wo, int C, int h, int w, int relu)
{
    const int cg_n = C / 8;
    const long long total = (long long)B * Ho * Wo * cg_n;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int cg = (int)(idx % cg_n);
        long long pix = idx / cg_n;
        const int ox = (int)(pix % Wo);
        pix /= Wo;
        const int oy = (int)(pix % Ho), b = (int)(pix / Ho);
        const Lerp ly = lerp_index(oy, h, Ho), lx = lerp_index(ox, w, Wo);
        const _Float16* tb = t + (size_t)b * h * w * C + cg * 8;
        const half8 v00 = *reinterpret_cast<const half8*>(tb + ((size_t)ly.i0 * w + lx.i0) * C);
        const half8 v01 = *reinterpret_cast<const half8*>(tb + ((size_t)ly.i0 * w + lx.i1) * C);
        const half8 v10 = *reinterpret_cast<const half8*>(tb + ((size_t)ly.i1 * w + lx.i0) * C);
        const half8 v11 = *reinterpret_cast<const half8*>(tb + ((size_t)ly.i1 * w + lx.i1) * C);
        const size_t o = (((size_t)b * Ho + oy) * Wo + ox) * C + cg * 8;
        const half8 av = *reinterpret_cast<const half8*>(a + o);
        half8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float up = ly.l0 * (lx.l0 * (float)v00[e] + lx.l1 * (float)v01[e]) +
                             ly.l1 * (lx.l0 * (float)v10[e] + lx.l1 * (float)v11[e]);
            float v = (float)av[e] + up;
            if (relu) v = v < 0.f ? 0.f : v;
            r[e] = (_Float16)v;
        }
        *reinterpret_cast<half8*>(out + o) = r;
    }
}

// fp32 NHWC heads (channel stride Cs) -> fp32 NCHW [B,C,Ho,Wo] = ((s0 + up(s1)) + up(s2)).
// One 32-pixel row segment per workgroup; LDS transposes pixel-major -> channel-major so
// that both the NHWC reads and the NCHW writes are coalesced.
struct HeadSrc { const float* p[3]; int h[3], w[3]; int n; };
constexpr int HS_PX = 32;

// ((s0 + up(s1)) + up(s2)) for four consecutive channels of pixel (b, y, x): the value the reference's
// `res4 + res3 + res2` (smap.py:417) has there.  A source at the output resolution is its own bilinear image.
// Written with the source index k as a COMPILE-TIME constant (unrolled, `k < s.n` as a predicate).  The round-1/2 version looped
// over k with a private `Lerp ly[3]`; the compiler promoted that array to LDS (indexed through the dispatch packet) and the kernel
// returned ~15 wrong values in 10-30 % of the launches that overlapped another stream's kernels -- never alone (EXPERIMENTS
// R3.6, tools/experiments/headsum_runtime_index_repro.hip).  No run-time-indexed private arrays in this library's kernels.
template <int K>
__device__ __forceinline__ float4 head_source4(const HeadSrc& s, const Lerp& ly, int b, int y, int x, int c, int Ho, int Wo, int Cs)
{
    const int sh = s.h[K], sw = s.w[K];
    const float* base = s.p[K] + (size_t)b * sh * sw * Cs + c;
    if (sh == Ho && sw == Wo) return *reinterpret_cast<const float4*>(base + ((size_t)y * Wo + x) * Cs);
    const Lerp lx = lerp_index(x, sw, Wo);
    const float4 v00 = *reinterpret_cast<const float4*>(base + ((size_t)ly.i0 * sw + lx.i0) * Cs);
    const float4 v01 = *reinterpret_cast<const float4*>(base + ((size_t)ly.i0 * sw + lx.i1) * Cs);
    const float4 v10 = *reinterpret_cast<const float4*>(base + ((size_t)ly.i1 * sw + lx.i0) * Cs);
    const float4 v11 = *reinterpret_cast<const float4*>(base + ((size_t)ly.i1 * sw + lx.i1) * Cs);
    float4 up;
    up.x = ly.l0 * (lx.l0 * v00.x + lx.l1 * v01.x) + ly.l1 * (lx.l0 * v10.x + lx.l1 * v11.x);
    up.y = ly.l0 * (lx.l0 * v00.y + lx.l1 * v01.y) + ly.l1 * (lx.l0 * v10.y + lx.l1 * v11.y);
    up.z = ly.l0 * (lx.l0 * v00.z + lx.l1 * v01.z) + ly.l1 * (lx.l0 * v10.z + lx.l1 * v11.z);
    up.w = ly.l0 * (lx.l0 * v00.w + lx.l1 * v01.w) + ly.l1 * (lx.l0 * v10.w + lx.l1 * v11.w);
    return up;
}

__device__ __forceinline__ float4 head_value4(const HeadSrc& s, const Lerp& ly0, const Lerp& ly1, const Lerp& ly2, int b, int y, int x,
                                              int c, int Ho, int Wo, int Cs)
{
    float4 v = head_source4<0>(s, ly0, b, y, x, c, Ho, Wo, Cs);
    if (s.n > 1) {
        const float4 u = head_source4<1>(s, ly1, b, y, x, c, Ho, Wo, Cs);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    if (s.n > 2) {
        const float4 u = head_source4<2>(s, ly2, b, y, x, c, Ho, Wo, Cs);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
    }
    return v;
}

// fp32 NHWC heads (channel stride Cs) -> fp32 NCHW [B,C,Ho,Wo] = ((s0 + up(s1)) + up(s2)).
// One 32-pixel row segment per workgroup; LDS transposes pixel-major -> channel-major so
// that both the NHWC reads and the NCHW writes are coalesced.
// FLIP (smap_op.flip_from > 0): the flip-TTA merge of test.py:55-70 in the same pass -- the workgroup also evaluates the
// maps of the mirrored frame b + flip_from at the mirrored pixels W-1-x and writes
//     out[b,c] = v[b,c] + s_c * v_mirror[pair[c]]   (s_c = -1 on PAF-x channels), halved for c >= n_kpt,
// the same fp32 operations, in the same order, as the reference's channel loop (and as smap_flip_merge).
// scale (smap_op.scale_hms): the value is stored as v / 255 (channels < n_kpt) or v / 127 -- test.py:111-112's in-place division of the maps
// before the association, the same fp32 IEEE division as smap_scale_hms (csrc/assoc.hip), fused into this store.
template <bool FLIP>
__global__ __launch_bounds__(256) void headsum_kernel(HeadSrc s, float* __restrict__ out, int Ho, int Wo, int C,
                                                      int Cs, int flip_from, const int* __restrict__ pair, int n_kpt,
                                                      int* __restrict__ status, int scale)
{
    __shared__ float tile[(FLIP ? 2 : 1) * 48 * (HS_PX + 1)];
    float* tile2 = tile + 48 * (HS_PX + 1);
    const int b = blockIdx.z, y = blockIdx.y, x0 = blockIdx.x * HS_PX, tid = threadIdx.x;
    const Lerp ly0 = lerp_index(y, s.h[0], Ho);
    const Lerp ly1 = lerp_index(y, s.n > 1 ? s.h[1] : Ho, Ho), ly2 = lerp_index(y, s.n > 2 ? s.h[2] : Ho, Ho);
    // four channels per thread (16-byte loads; Cs is a multiple of 4: plan_check.cpp)
    const int G = Cs >> 2;
    for (int idx = tid; idx < HS_PX * G; idx += 256) {
        const int px = idx / G, c = (idx - px * G) * 4;
        const int x = x0 + px;
        if (x >= Wo || c >= C) continue;
        const float4 v = head_value4(s, ly0, ly1, ly2, b, y, x, c, Ho, Wo, Cs);
        const float vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c + e < C) tile[(c + e) * (HS_PX + 1) + px] = vv[e];
        if (FLIP) {
            const float4 m = head_value4(s, ly0, ly1, ly2, b + flip_from, y, Wo - 1 - x, c, Ho, Wo, Cs);
            const float mm[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (c + e < C) tile2[(c + e) * (HS_PX + 1) + px] = mm[e];
        }
    }
    __syncthreads();
    for (int idx = tid; idx < C * HS_PX; idx += 256) {
        const int c = idx / HS_PX, px = idx - c * HS_PX;
        const int x = x0 + px;
        if (x >= Wo) continue;
        float v = tile[c * (HS_PX + 1) + px];
        if (FLIP) {
            const float f = tile2[pair[c] * (HS_PX + 1) + px];
            const bool neg = c >= n_kpt && ((c - n_kpt) & 1) == 0;
            v = v + (neg ? f * -1.f : f);
            if (c >= n_kpt) v = v * 0.5f;
        }
        if (scale) v = v / (c < n_kpt ? 255.f : 127.f);
        out[(((size_t)b * C + c) * Ho + y) * Wo + x] = v;
        // inf / NaN: an activation left the fp16 range upstream.  Status word b / 31: bit 0 = some frame of the word, bit 1 + b % 31 =
        // output frame b; word 0's bit 0 = some frame of the launch (include/smap_hip.h)
        if (status && !(fabsf(v) <= 3.4028234e38f)) {
            atomicOr(reinterpret_cast<unsigned*>(status) + b / 31, 1u | (2u << (b % 31)));
            if (b >= 31) atomicOr(reinterpret_cast<unsigned*>(status), 1u);
        }
    }
}

// SMAP_OP_TAPSUM: out[b,0,y,x] = bias + sum_{kh,kw} t[b, y+kh-1, x+kw-1][3 kh + kw] (zero outside the map): the stencil half of a 3x3 conv with
// one output channel whose per-pixel dot products came out of the producing conv launch (conv.hip TAPDOT).  Taps summed in the fixed order
// 0..8.  One thread per output pixel; the nine reads of a wave are nine coalesced 64-byte-strided gathers of neighbouring pixels.
__global__ __launch_bounds__(256) void tapsum_kernel(const float* __restrict__ t, const float* __restrict__ bias, float* __restrict__ out,
                                                     int B, int H, int W, int ts, int* __restrict__ status)
{
    const long long total = (long long)B * H * W;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int x = (int)(i % W), y = (int)((i / W) % H), b = (int)(i / ((long long)W * H));
    float v = bias[0];
#pragma unroll
    for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
            const int yy = y + kh - 1, xx = x + kw - 1;
            if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) v += t[(((size_t)b * H + yy) * W + xx) * ts + kh * 3 + kw];
        }
    out[i] = v;
    if (status && !(fabsf(v) <= 3.4028234e38f)) {
        atomicOr(reinterpret_cast<unsigned*>(status) + b / 31, 1u | (2u << (b % 31)));
        if (b >= 31) atomicOr(reinterpret_cast<unsigned*>(status), 1u);
    }
}

inline int grid_for(long long total, int block)
{
    long long g = (total + block - 1) / block;
    return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

}  // namespace

struct smap_plan : PlanCheck {                 // the checked schedule (csrc/plan_check.h) + what running it with lanes on needs
    // lanes (smap_op.lane): side streams 1 .. SMAP_MAX_LANES - 1 and one event per op some other lane waits for; created on first use
    bool lanes_on = false, lanes_ready = false;
    hipStream_t side[SMAP_MAX_LANES] = {};
    std::vector<hipEvent_t> ev;            // per op, null unless signalled
    hipEvent_t join_ev[SMAP_MAX_LANES] = {};
};

#ifdef SMAP_TIMELINE
// Diagnostics build (tools/build_ablate.py --timeline): every conv launch gets a slice of a caller-provided buffer
// (env SMAP_TIMELINE_PTR = device address, SMAP_TIMELINE_CAP = launches it holds) in which its workgroups leave their
// start / end times on the device-wide 100 MHz clock and the CU they ran on (csrc/plan.h).
constexpr long long TL_SLICE = 4LL * (1 + 16384);               // int64 per launch: metadata row + up to 16384 workgroups
static int tl_next = 0;
static long long* tl_base() { const char* e = getenv("SMAP_TIMELINE_PTR"); return e ? reinterpret_cast<long long*>(strtoull(e, nullptr, 0)) : nullptr; }
static int tl_cap() { const char* e = getenv("SMAP_TIMELINE_CAP"); return e ? atoi(e) : 0; }
extern "C" __attribute__((visibility("default"))) void smap_timeline_reset(void) { tl_next = 0; }
extern "C" __attribute__((visibility("default"))) int smap_timeline_count(void) { return tl_next; }
#endif

extern "C" {

// The two constructors: the checker (csrc/plan_check.cpp) fills the plan or refuses the schedule; nothing here touches the GPU.
int smap_plan_create(const smap_op* ops, int n_ops, smap_plan** plan)
{
    std::unique_ptr<smap_plan> p(new (std::nothrow) smap_plan());
    if (!plan || !p) return SMAP_E_ARG;
    if (int rc = plan_check(ops, n_ops, p.get())) return rc;
    *plan = p.release();
    return 0;
}

int smap_plan_create_from_blob(const void* blob, size_t blob_bytes, smap_plan** plan, smap_blob_info* info)
{
    std::unique_ptr<smap_plan> p(new (std::nothrow) smap_plan());
    if (!plan || !p) return SMAP_E_ARG;
    if (int rc = plan_check_blob(blob, blob_bytes, p.get(), info)) return rc;
    *plan = p.release();
    return 0;
}

static void lanes_release(smap_plan* p)
{
    for (hipEvent_t& e : p->ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    for (int l = 0; l < SMAP_MAX_LANES; ++l) {
        if (p->join_ev[l]) { (void)hipEventDestroy(p->join_ev[l]); p->join_ev[l] = nullptr; }
        if (p->side[l]) { (void)hipStreamDestroy(p->side[l]); p->side[l] = nullptr; }
    }
    p->lanes_ready = false;
}

void smap_plan_destroy(smap_plan* plan)
{
    if (!plan) return;
    lanes_release(plan);
    delete plan;
}

// side streams + events of a plan whose lanes are switched on (device = the current one).  All or nothing: a failure half way releases
// what was created, so that the next attempt starts clean (round 5 created them lazily inside the const run and leaked on failure).
static int lanes_setup(smap_plan* p)
{
    if (p->lanes_ready) return 0;
    hipError_t e = hipSuccess;
    for (int l = 1; l < p->n_lanes && e == hipSuccess; ++l) e = hipStreamCreateWithFlags(&p->side[l], hipStreamNonBlocking);
    for (int l = 0; l < p->n_lanes && e == hipSuccess; ++l) e = hipEventCreateWithFlags(&p->join_ev[l], hipEventDisableTiming);
    p->ev.assign(p->ops.size(), nullptr);
    for (size_t i = 0; i < p->ops.size() && e == hipSuccess; ++i)
        if (p->signalled[i]) e = hipEventCreateWithFlags(&p->ev[i], hipEventDisableTiming);
    if (e != hipSuccess) { lanes_release(p); return hip_rc(e); }
    p->lanes_ready = true;
    return 0;
}

// Lanes on / off.  Switching them ON creates the side streams and events HERE (on the current device), not inside a run: a first run inside
// a stream capture must not create streams, smap_plan_run stays const, and a failure is this call's return code.  A plan with lanes on has
// ONE caller at a time (its side streams and events are shared by whoever runs it: executors of one plan on several host threads are not
// supported with lanes; without lanes a plan is immutable and may be run concurrently).
int smap_plan_set_lanes(smap_plan* plan, int on)
{
    if (!plan) return SMAP_E_ARG;
    if (on && plan->n_lanes > 1)
        if (int rc = lanes_setup(plan)) return rc;
    plan->lanes_on = on != 0;
    return 0;
}

// a CONV op as the argument block of its launch
static ConvArgs conv_args(const smap_op& o, char* ar, const char* wb)
{
    auto A = [&](int64_t off) -> _Float16* { return off < 0 ? nullptr : reinterpret_cast<_Float16*>(ar + off); };
    const TileRow& t = *tile_find(o.tile);       // (a checked op names a tile)
    ConvArgs a;
    a.arena = ar + window_of(o.in_off);          // 64-bit base of the launch; lane offsets are 32-bit from here
    a.in_off = o.in_off - window_of(o.in_off);
    a.w = reinterpret_cast<const _Float16*>(wb + o.w_off);
    a.bias = reinterpret_cast<const float*>(wb + o.bias_off);
    a.out = ar + o.out_off;
    a.res = A(o.res_off);
    a.add1 = A(o.add1_off);
    a.add2 = A(o.add2_off);
    a.up = A(o.aux_off[0]);
    a.up_h = o.aux_h[0];
    a.up_w = o.aux_w[0];
    a.H = o.H; a.W = o.W; a.Cin = o.Cin; a.in_stride_c = o.in_stride_c; a.in_c_off = o.in_c_off;
    a.Ho = o.Ho; a.Wo = o.Wo; a.Cout8 = (o.Cout + 7) & ~7;
    a.ksize = o.ksize; a.stride = o.stride; a.pad = o.pad; a.relu = o.relu;
    a.out_stride_c = o.out_stride_c; a.out_c_off = o.out_c_off; a.out_fp32 = o.out_fp32;
    a.M = o.B * o.Ho * o.Wo;
    a.K = o.ksize * o.ksize * o.Cin + (o.in2_C > 0 ? o.in2_C : 0);      // (a second input extends K)
    a.Cin2 = o.in2_C > 0 ? o.in2_C : 0;
    a.in2_off = o.in2_C > 0 ? o.in2_off - window_of(o.in_off) : 0;       // same base as the first input (validate: same window)
    a.H2 = o.in2_H; a.W2 = o.in2_W; a.in2_stride_c = o.in2_stride_c; a.stride2 = o.in2_stride; a.in2_lo = o.in2_stride_c / 2;
    a.bias_b = (o.in2_C > 0 && o.in2_mode == 1) ? reinterpret_cast<const float*>(wb + o.in2_bias_off) : nullptr;
    a.acc_scale_b = o.in2_acc_scale;
    a.x3 = o.precision;
    a.in_lo = o.in_stride_c / 2;
    a.out_lo = o.out_stride_c / 2;
    a.w_lo = (long long)o.cout_pad * a.K * 2;
    a.acc_scale = o.acc_scale;
    a.w_pairs = o.w_pairs;
    a.w2 = o.tail_cout > 0 ? reinterpret_cast<const _Float16*>(wb + o.tail_w_off) : nullptr;
    a.bias2 = o.tail_cout > 0 ? reinterpret_cast<const float*>(wb + o.tail_bias_off) : nullptr;
    a.tail_cout8 = o.tail_cout;
    a.tail_chunks = o.tail_cout > 0 ? o.tail_cout_pad / t.tail_bn : 0;
    a.tail_acc_scale = o.tail_acc_scale;
    a.w0 = o.head_cin > 0 ? reinterpret_cast<const _Float16*>(wb + o.head_w_off) : nullptr;
    a.bias0 = o.head_cin > 0 ? reinterpret_cast<const float*>(wb + o.head_bias_off) : nullptr;
    a.head_cin = o.head_cin;
    a.acc_scale0 = o.head_acc_scale;
    a.wd = o.head_cin > 0 && o.short_acc_scale > 0.f ? reinterpret_cast<const _Float16*>(wb + o.short_w_off) : nullptr;
    a.acc_scale_d = o.short_acc_scale;
    a.tap_n = o.tap_n;
    a.tap_w = o.tap_n > 0 ? reinterpret_cast<const _Float16*>(wb + o.tap_w_off) : nullptr;
    a.tap_scale = o.tap_scale;
    a.ksplit = o.ksplit > 1 ? o.ksplit : 1;
    a.kpart = o.ksplit > 1 ? reinterpret_cast<float*>(ar + o.kpart_off) : nullptr;
    a.kcount = o.ksplit > 1 ? reinterpret_cast<unsigned*>(ar + o.kcount_off) : nullptr;
    a.seg_n1 = o.seg_n[0] > 0 ? o.seg_n[0] : INT32_MAX;
    a.seg_n2 = o.seg_n[1] > 0 ? o.seg_n[1] : INT32_MAX;
    a.seg_out1 = o.seg_n[0] > 0 ? ar + o.seg_out_off[0] : nullptr;
    a.seg_out2 = o.seg_n[1] > 0 ? ar + o.seg_out_off[1] : nullptr;
    a.seg_cout8_1 = o.seg_cout[0]; a.seg_cout8_2 = o.seg_cout[1];
    a.seg_stride1 = o.seg_out_stride_c[0]; a.seg_stride2 = o.seg_out_stride_c[1];
    a.seg_relu1 = o.seg_relu[0]; a.seg_relu2 = o.seg_relu[1];
    a.seg_scale1 = o.seg_acc_scale[0]; a.seg_scale2 = o.seg_acc_scale[1];
    a.m_tiles = (a.M + t.bm - 1) / t.bm;
    a.n_tiles = o.cout_pad / t.bn;
    return a;
}

static int run_ops(const smap_plan* plan, int first, int count, const float* const* inputs, int n_inputs, void* arena,
                   const void* weights, float* out, void* stream)
{
    if (!plan || !arena || !weights || first < 0 || count < 0 || first + count > (int)plan->ops.size())
        return SMAP_E_ARG;
    if (n_inputs < 0 || n_inputs > SMAP_MAX_INPUTS || (n_inputs > 0 && !inputs)) return SMAP_E_ARG;
    hipStream_t st = (hipStream_t)stream;
    char* ar = static_cast<char*>(arena);
    const char* wb = static_cast<const char*>(weights);
    auto A = [&](int64_t off) -> _Float16* { return off < 0 ? nullptr : reinterpret_cast<_Float16*>(ar + off); };
    StemIn sin;
    for (int j = 0; j < SMAP_MAX_INPUTS; ++j) sin.p[j] = j < n_inputs ? inputs[j] : nullptr;
    sin.frames_per = 1;
    const bool have_input = n_inputs > 0 && inputs[0];
    for (int64_t w : plan->windows)
        if (hipError_t e = hipMemsetAsync(ar + w, 0, SMAP_ZERO_PAGE, st); e != hipSuccess) return hip_rc(e);
    // split-K tickets: zero before the first op (the kernels leave them at zero; an aborted run may not) -- the slices of the ops THIS run
    // launches, one memset each when they are apart, one for the lot when the packer laid them end to end (engine.py does)
    for (size_t t = 0; t < plan->tickets.size();) {
        if (plan->tickets[t].op < first || plan->tickets[t].op >= first + count) { ++t; continue; }
        int64_t lo = plan->tickets[t].off, hi = lo + plan->tickets[t].bytes;
        size_t u = t + 1;
        while (u < plan->tickets.size() && plan->tickets[u].off == hi && plan->tickets[u].op < first + count) hi += plan->tickets[u++].bytes;
        if (hipError_t e = hipMemsetAsync(ar + lo, 0, (size_t)(hi - lo), st); e != hipSuccess) return hip_rc(e);
        t = u;
    }
    for (int i = first; i < first + count; ++i)          // the status word (one per schedule) starts every run at 0
        if ((plan->ops[i].kind == SMAP_OP_HEADSUM || plan->ops[i].kind == SMAP_OP_TAPSUM) && plan->ops[i].status_off > 0 && out) {
            if (hipError_t e = hipMemsetAsync(reinterpret_cast<char*>(out) + plan->ops[i].status_off, 0, 4 * (size_t)SMAP_STATUS_WORDS(plan->ops[i].B), st); e != hipSuccess) return hip_rc(e);
            break;
        }
    // lanes: only for whole-schedule runs (a partial range may start behind a fork)
    const bool lanes = plan->lanes_on && plan->lanes_ready && plan->n_lanes > 1 && first == 0 && count == (int)plan->ops.size();
    hipStream_t const st0 = st;
    // (error returns behind the fork go through `fail`: the side lanes are joined into the caller's stream first, so that nothing of this run
    //  is still in flight on a stream the caller does not know about)
    auto join = [&]() -> int {
        for (int l = 1; l < plan->n_lanes; ++l) {
            if (hipError_t e = hipEventRecord(plan->join_ev[l], plan->side[l]); e != hipSuccess) return hip_rc(e);
            if (hipError_t e = hipStreamWaitEvent(st0, plan->join_ev[l], 0); e != hipSuccess) return hip_rc(e);
        }
        return 0;
    };
    auto fail = [&](int rc) -> int { if (lanes) (void)join(); return rc; };
    if (lanes) {
        // the side lanes start behind what the caller's stream holds so far (its earlier work, the memsets above)
        if (hipError_t e = hipEventRecord(plan->join_ev[0], st0); e != hipSuccess) return hip_rc(e);
        for (int l = 1; l < plan->n_lanes; ++l)
            if (hipError_t e = hipStreamWaitEvent(plan->side[l], plan->join_ev[0], 0); e != hipSuccess) return hip_rc(e);
    }
    for (int i = first; i < first + count; ++i) {
        const smap_op& o = plan->ops[i];
        hipError_t e = hipSuccess;
        if (lanes) {
            st = o.lane > 0 ? plan->side[o.lane] : st0;
            for (int k = 0; k < o.n_wait; ++k)
                if (hipError_t e2 = hipStreamWaitEvent(st, plan->ev[o.wait_op[k]], 0); e2 != hipSuccess) return fail(hip_rc(e2));
        }
        switch (o.kind) {
            case SMAP_OP_CONV: {
                ConvArgs a = conv_args(o, ar, wb);
#ifdef SMAP_TIMELINE
                a.tl = nullptr;
                if (tl_base() && tl_next < tl_cap()) {
                    a.tl = tl_base() + (long long)tl_next++ * TL_SLICE;
                    a.tl_meta[0] = i; a.tl_meta[1] = 0; a.tl_meta[2] = (long long)(uintptr_t)stream; a.tl_meta[3] = o.tile;
                }
#endif
#ifdef SMAP_TRACE
                a.dbg = getenv("SMAP_TRACE_PTR") ? reinterpret_cast<long long*>(strtoull(getenv("SMAP_TRACE_PTR"), nullptr, 0)) : nullptr;
#endif
                e = smap_launch_conv(a, o.tile, st);
                break;
            }
            case SMAP_OP_STEM: {
                const int frames = o.flip_from > 0 ? o.flip_from : o.B;       // frames the input holds
                if (!have_input || frames % n_inputs) return fail(SMAP_E_ARG);
                for (int j = 0; j < n_inputs; ++j) if (!inputs[j]) return fail(SMAP_E_ARG);
                sin.frames_per = frames / n_inputs;
                dim3 grid((o.Wo + ST_T - 1) / ST_T, (o.Ho + ST_T - 1) / ST_T, o.B);
                if (o.precision)
                    hipLaunchKernelGGL(stem_kernel<true>, grid, dim3(256), 0, st, sin,
                                       reinterpret_cast<const _Float16*>(wb + o.w_off),
                                       reinterpret_cast<const float*>(wb + o.bias_off), A(o.out_off), o.H, o.W, o.Ho,
                                       o.Wo, o.acc_scale, o.flip_from);
                else
                    hipLaunchKernelGGL(stem_kernel<false>, grid, dim3(256), 0, st, sin,
                                       reinterpret_cast<const _Float16*>(wb + o.w_off),
                                       reinterpret_cast<const float*>(wb + o.bias_off), A(o.out_off), o.H, o.W, o.Ho,
                                       o.Wo, 1.f, o.flip_from);
                e = hipGetLastError();
                break;
            }
            case SMAP_OP_STEMPOOL: {
                const int frames = o.flip_from > 0 ? o.flip_from : o.B;
                if (!have_input || frames % n_inputs) return fail(SMAP_E_ARG);
                for (int j = 0; j < n_inputs; ++j) if (!inputs[j]) return fail(SMAP_E_ARG);
                sin.frames_per = frames / n_inputs;
                const int hs = (o.H + 6 - 7) / 2 + 1, ws = (o.W + 6 - 7) / 2 + 1;
                dim3 grid((o.Wo + SP_PX - 1) / SP_PX, (o.Ho + SP_PY - 1) / SP_PY, o.B);
                if (o.precision)
                    hipLaunchKernelGGL(stem_pool_kernel<true>, grid, dim3(256), 0, st, sin,
                                       reinterpret_cast<const _Float16*>(wb + o.w_off),
                                       reinterpret_cast<const float*>(wb + o.bias_off), A(o.out_off), o.H, o.W, hs, ws,
                                       o.Ho, o.Wo, o.acc_scale, o.flip_from);
                else
                    hipLaunchKernelGGL(stem_pool_kernel<false>, grid, dim3(256), 0, st, sin,
                                       reinterpret_cast<const _Float16*>(wb + o.w_off),
                                       reinterpret_cast<const float*>(wb + o.bias_off), A(o.out_off), o.H, o.W, hs, ws,
                                       o.Ho, o.Wo, 1.f, o.flip_from);
                e = hipGetLastError();
                break;
            }
            case SMAP_OP_MAXPOOL: {
                const long long total = (long long)o.B * o.Ho * o.Wo * (o.Cin / 8);
                if (o.precision)
                    hipLaunchKernelGGL(maxpool_kernel<true>, dim3(grid_for(total, 256)), dim3(256), 0, st, A(o.in_off),
                                       A(o.out_off), o.B, o.H, o.W, o.Cin, o.Ho, o.Wo);
                else
                    hipLaunchKernelGGL(maxpool_kernel<false>, dim3(grid_for(total, 256)), dim3(256), 0, st, A(o.in_off),
                                       A(o.out_off), o.B, o.H, o.W, o.Cin, o.Ho, o.Wo);
                e = hipGetLastError();
                break;
            }
            case SMAP_OP_UPADD: {
                const long long total = (long long)o.B * o.Ho * o.Wo * (o.Cout / 8);
                hipLaunchKernelGGL(upadd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, A(o.in_off),
                                   A(o.aux_off[0]), A(o.out_off), o.B, o.Ho, o.Wo, o.Cout, o.aux_h[0], o.aux_w[0],
                                   o.relu);
                e = hipGetLastError();
                break;
            }
            case SMAP_OP_TAPSUM: {
                if (!out) return fail(SMAP_E_ARG);
                const long long total = (long long)o.B * o.H * o.W;
                int* status = o.status_off > 0 ? reinterpret_cast<int*>(reinterpret_cast<char*>(out) + o.status_off) : nullptr;
                hipLaunchKernelGGL(tapsum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const float*>(ar + o.aux_off[0]),
                                   reinterpret_cast<const float*>(wb + o.bias_off), reinterpret_cast<float*>(reinterpret_cast<char*>(out) + o.ext_off),
                                   o.B, o.H, o.W, o.Cin, status);
                e = hipGetLastError();
                break;
            }
            case SMAP_OP_HEADSUM: {
                if (!out) return fail(SMAP_E_ARG);
                HeadSrc s;
                s.n = o.n_aux;
                for (int k = 0; k < 3; ++k) {
                    s.p[k] = k < o.n_aux ? reinterpret_cast<const float*>(ar + o.aux_off[k]) : nullptr;
                    s.h[k] = o.aux_h[k];
                    s.w[k] = o.aux_w[k];
                }
                dim3 grid((o.Wo + HS_PX - 1) / HS_PX, o.Ho, o.B);
                float* dst = reinterpret_cast<float*>(reinterpret_cast<char*>(out) + o.ext_off);
                int* status = o.status_off > 0 ? reinterpret_cast<int*>(reinterpret_cast<char*>(out) + o.status_off) : nullptr;
                if (o.flip_from > 0)
                    hipLaunchKernelGGL(headsum_kernel<true>, grid, dim3(256), 0, st, s, dst, o.Ho, o.Wo, o.Cout, o.Cin,
                                       o.flip_from, reinterpret_cast<const int*>(wb + o.w_off), o.in_c_off, status, o.scale_hms);
                else
                    hipLaunchKernelGGL(headsum_kernel<false>, grid, dim3(256), 0, st, s, dst, o.Ho, o.Wo, o.Cout, o.Cin,
                                       0, nullptr, o.in_c_off, status, o.scale_hms);
                e = hipGetLastError();
                break;
            }
            default:
                return fail(SMAP_E_ARG);
        }
        if (e != hipSuccess) return fail(hip_rc(e));
        if (lanes && plan->signalled[i])
            if (hipError_t e2 = hipEventRecord(plan->ev[i], st); e2 != hipSuccess) return fail(hip_rc(e2));
    }
    if (lanes) return join();                            // the caller's stream continues when every lane is done
    return 0;
}

int smap_workspace_bytes(const smap_plan* plan, int64_t* arena_bytes, int64_t* out_bytes)
{
    if (!plan) return SMAP_E_ARG;
    plan_workspace_bytes(plan->ops, arena_bytes, out_bytes);
    return 0;
}

int smap_plan_run_range(const smap_plan* plan, int first, int count, const float* input, void* arena,
                        const void* weights, float* out, void* stream)
{
    return run_ops(plan, first, count, &input, input ? 1 : 0, arena, weights, out, stream);
}

int smap_plan_run(const smap_plan* plan, const float* input, void* arena, const void* weights, float* out,
                  void* stream)
{
    if (!plan) return SMAP_E_ARG;
    return run_ops(plan, 0, (int)plan->ops.size(), &input, input ? 1 : 0, arena, weights, out, stream);
}

int smap_plan_run_inputs(const smap_plan* plan, const float* const* inputs, int n_inputs, void* arena, const void* weights,
                         float* out, void* stream)
{
    if (!plan || n_inputs < 1) return SMAP_E_ARG;
    return run_ops(plan, 0, (int)plan->ops.size(), inputs, n_inputs, arena, weights, out, stream);
}

}  // extern "C"
