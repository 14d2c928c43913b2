// gemm_f32_device.h -- the two fp32 MFMA GEMM kernels of the training path, their operand descriptors and their launch helpers: the one
// copy that heads.hip (the head arms) and trunk.hip (u_skip, up_conv) both include.
// Both kernels run on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: bit for bit a k-ordered fmaf chain), 256 threads = 4 waves, every
// wave 2 x 2 accumulator tiles of 32 x 32:
//   conv_gemm    rows = pixels, columns = output channels, k = (chunk of 16 input channels, tap, channel of the chunk) in that order.  The pixel operand is read through
//                a descriptor (dense fp32, fp16, fp16 hi|lo planes summed in registers, or a head tensor in either order) with zeros
//                outside the image; the weights through strides, so a weight matrix is read where torch keeps it (transposed or tap-
//                mirrored by the strides, never copied).  Epilogue: + bias, relu, or zero where a mask tensor is not positive.
//   reduce_gemm  k = pixels: part[slice][n][t][m] = sum over the slice's pixels of A[p, n] * B[p + t, m], and the column sums of A.
//                fold adds the slices in order.  No atomics anywhere: the same bits run to run.
// Both stage a [16][rows] and a [16][columns] tile in LDS per k step, the next step's loads in flight while the MFMAs of this one run.
// Nothing outside the described elements is written: columns beyond N exist inside the tile only.
// Everything sits in gemm_f32's unnamed namespace: each unit that includes this header has its own instances.
#ifndef SMAP_GEMM_F32_DEVICE_H
#define SMAP_GEMM_F32_DEVICE_H
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include "smap_hip.h"
#include "hip_rc.h"

namespace gemm_f32 {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int NT = 256, BK = 16, PAD = 4;
constexpr int SLICE_MIN = 256, SLICE_MAX_N = 64;

// a pixel-major operand: element (frame b, pixel q of the h x w image, channel c) is at ptr[b * frame_stride + q * pix_stride + c * ch_stride]
struct Pix {
    const void* ptr;
    long long frame_stride, pix_stride, ch_stride;      // in elements
    int kind;                                           // SMAP_HEADS_X_*: f32, f16, or f16 hi|lo (value = hi + lo, lo `lo_off` halfs behind hi)
    int lo_off;
    int C;                                              // channels that exist; the ones behind read as 0
    int vec;                                            // ch_stride == 1 and four channels from a multiple of 4 are one aligned load
};
// weights: element (tap t, k, n) at ptr[t * ts + k * ks + n * ns]; k >= K and n >= N read as 0
struct Wgt {
    const float* ptr;
    long long ts, ks, ns;
    int K, N;
};

__device__ __forceinline__ float pix_load1(const Pix& s, long long off)
{
    if (s.kind == SMAP_HEADS_X_F32) return ((const float*)s.ptr)[off];
    const __half* p = (const __half*)s.ptr;
    float v = __half2float(p[off]);
    if (s.kind == SMAP_HEADS_X_F16_HILO) v += __half2float(p[off + s.lo_off]);
    return v;
}
__device__ __forceinline__ float4 halfs4(uint2 u)
{
    const __half2 a = *(const __half2*)&u.x, b = *(const __half2*)&u.y;
    const float2 fa = __half22float2(a), fb = __half22float2(b);
    return make_float4(fa.x, fa.y, fb.x, fb.y);
}
// channels c0 .. c0 + 3 of pixel q of frame b
__device__ __forceinline__ float4 pix_load4(const Pix& s, int b, long long q, int c0)
{
    float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const long long base = (long long)b * s.frame_stride + q * s.pix_stride;
    if (s.vec && c0 + 4 <= s.C) {
        if (s.kind == SMAP_HEADS_X_F32) return *(const float4*)((const float*)s.ptr + base + c0);
        const __half* p = (const __half*)s.ptr + base + c0;
        v = halfs4(*(const uint2*)p);
        if (s.kind == SMAP_HEADS_X_F16_HILO) {
            const float4 l = halfs4(*(const uint2*)(p + s.lo_off));
            v.x += l.x, v.y += l.y, v.z += l.z, v.w += l.w;
        }
        return v;
    }
    float* e = &v.x;
    for (int j = 0; j < 4; ++j)
        if (c0 + j < s.C) e[j] = pix_load1(s, base + (long long)(c0 + j) * s.ch_stride);
    return v;
}

// one k step of a wave: its 2 x 2 accumulators += As[k][rows] x Bs[k][columns], k ascending.  do_n[j]: column tile j holds a real column
template <int LDA, int LDB>
__device__ __forceinline__ void mfma_step(const float (*As)[LDA], const float (*Bs)[LDB], int row0, int col0, int lane, const bool do_n[2],
                                          f32x16 acc[2][2])
{
    const int r = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int kk = 0; kk < BK / 2; ++kk) {
        const int k = 2 * kk + kh;
        const float a0 = As[k][row0 + r], a1 = As[k][row0 + 32 + r];
        const float b0 = Bs[k][col0 + r], b1 = Bs[k][col0 + 32 + r];
        if (do_n[0]) {
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        }
        if (do_n[1]) {
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
}
// row of accumulator register `reg` within its 32 x 32 tile (the column is lane & 31)
__device__ __forceinline__ int acc_row(int reg, int lane) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }

struct ConvArgs {
    Pix a;
    Wgt wt;
    float* out;                                  // element (b, q, n) at out[b * out_fs + q * out_ps + n * out_cs]
    long long out_fs, out_ps, out_cs;
    const float* bias;                           // [N] or null
    const float* mask;                           // null, or element (p, n) at mask[p * mask_ps + n]: the result is 0 where it is not > 0
    long long mask_ps;
    int relu, B, h, w, N, taps, mirror;          // mirror: the pixel operand is read at p - t instead of p + t
};

// tile (64 WM pixels) x (64 WN channels), WM * WN == 4 waves
template <int WM, int WN>
__global__ __launch_bounds__(NT) void conv_gemm_kernel(const ConvArgs g)
{
    constexpr int BM = 64 * WM, BN = 64 * WN, LDA = BM + PAD, LDB = BN + PAD;
    constexpr int AQ = BM * (BK / 4) / NT, BQ = BK * BN / NT;
    __shared__ float As[BK][LDA], Bs[BK][LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave % WM, wn = wave / WM;
    const int hw = g.h * g.w;
    const long long P = (long long)g.B * hw, p0 = (long long)blockIdx.x * BM;
    const int n0 = blockIdx.y * BN;
    // this thread's share of the pixel tile: AQ (pixel, channel quad) slots, four lanes per pixel
    int ab[AQ], ay[AQ], ax[AQ];
#pragma unroll
    for (int i = 0; i < AQ; ++i) {
        const long long p = p0 + (tid + i * NT) / 4;
        ab[i] = -1, ay[i] = 0, ax[i] = 0;
        if (p < P) {
            ab[i] = (int)(p / hw);
            const int r = (int)(p - (long long)ab[i] * hw);
            ay[i] = r / g.w, ax[i] = r - ay[i] * g.w;
        }
    }
    const int nck = (g.wt.K + BK - 1) / BK, steps = g.taps * nck;
    float4 ra[AQ];
    float rb[BQ];
    auto fetch = [&](int s) {
        const int ck = s / g.taps, t = s - ck * g.taps, c0 = ck * BK;      // the taps of one channel chunk back to back: its lines stay in L1
        int dy = 0, dx = 0;
        if (g.taps == 9) dy = t / 3 - 1, dx = t % 3 - 1;
        if (g.mirror) dy = -dy, dx = -dx;
#pragma unroll
        for (int i = 0; i < AQ; ++i) {
            const int y = ay[i] + dy, x = ax[i] + dx;
            ra[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (ab[i] >= 0 && y >= 0 && y < g.h && x >= 0 && x < g.w) ra[i] = pix_load4(g.a, ab[i], (long long)y * g.w + x, c0 + 4 * (tid & 3));
        }
#pragma unroll
        for (int i = 0; i < BQ; ++i) {
            const int idx = tid + i * NT, k = c0 + idx / BN, n = n0 + idx % BN;
            rb[i] = (k < g.wt.K && n < g.wt.N) ? g.wt.ptr[t * g.wt.ts + k * g.wt.ks + n * g.wt.ns] : 0.0f;
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    const int col0 = wn * 64;
    const bool do_n[2] = {n0 + col0 < g.N, n0 + col0 + 32 < g.N};
    fetch(0);
    for (int s = 0; s < steps; ++s) {
#pragma unroll
        for (int i = 0; i < AQ; ++i) {
            // lane l of a wave: word (4 (l & 3) + j) * LDA + (l >> 2) + const; LDA = 4 mod 64, so bank = 16 (l & 3) + (l >> 2) + const -- the 64
            // lanes of each of the four stores hit 64 different banks
            const int m = (tid + i * NT) / 4, k = 4 * (tid & 3);
            As[k][m] = ra[i].x, As[k + 1][m] = ra[i].y, As[k + 2][m] = ra[i].z, As[k + 3][m] = ra[i].w;
        }
#pragma unroll
        for (int i = 0; i < BQ; ++i) {
            const int idx = tid + i * NT;
            Bs[idx / BN][idx % BN] = rb[i];
        }
        __syncthreads();
        if (s + 1 < steps) fetch(s + 1);
        mfma_step<LDA, LDB>(As, Bs, wm * 64, col0, lane, do_n, acc);
        __syncthreads();
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int n = n0 + col0 + 32 * ni + (lane & 31);
            if (n >= g.N) continue;
            const float bias = g.bias ? g.bias[n] : 0.0f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const long long p = p0 + wm * 64 + 32 * mi + acc_row(reg, lane);
                if (p >= P) continue;
                float v = acc[mi][ni][reg] + bias;
                if (g.relu) v = fmaxf(v, 0.0f);
                if (g.mask && !(g.mask[p * g.mask_ps + n] > 0.0f)) v = 0.0f;
                const int b = (int)(p / hw);
                const long long q = p - (long long)b * hw;
                g.out[b * g.out_fs + q * g.out_ps + n * g.out_cs] = v;
            }
        }
}

struct RedArgs {
    Pix a, b;                   // rows n = channels of a, columns m = channels of b, both summed over the pixels
    float* part;                // [slices][N][taps][Md]
    float* colpart;             // [slices][N]: the slice's sum of a over its pixels
    int B, h, w, N, Md, taps, slice_len;
};

// tile (64 WR channels of a) x (64 WC channels of b), WR * WC == 4 waves; grid (row tiles, column tiles * taps, slices)
template <int WR, int WC>
__global__ __launch_bounds__(NT) void reduce_gemm_kernel(const RedArgs g)
{
    constexpr int BR = 64 * WR, BC = 64 * WC, LDA = BR + PAD, LDB = BC + PAD;
    constexpr int AQ = BK * BR / 4 / NT, BQ = BK * BC / 4 / NT;
    __shared__ __attribute__((aligned(16))) float As[BK][LDA];
    __shared__ __attribute__((aligned(16))) float Bs[BK][LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave % WR, wc = wave / WR;
    const int hw = g.h * g.w;
    const long long P = (long long)g.B * hw;
    const int mtiles = (g.Md + BC - 1) / BC, t = blockIdx.y / mtiles;
    const int n0 = blockIdx.x * BR, m0 = (blockIdx.y - t * mtiles) * BC, slice = blockIdx.z;
    const long long pbeg = (long long)slice * g.slice_len, pend = min(P, pbeg + g.slice_len);
    int dy = 0, dx = 0;
    if (g.taps == 9) dy = t / 3 - 1, dx = t % 3 - 1;
    const int steps = (int)((pend - pbeg + BK - 1) / BK);
    float4 ra[AQ], rb[BQ];
    auto fetch = [&](int s) {
#pragma unroll
        for (int i = 0; i < AQ; ++i) {
            const int slot = tid + i * NT;
            const long long p = pbeg + (long long)s * BK + slot / (BR / 4);
            ra[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (p < pend) {
                const int b = (int)(p / hw);
                ra[i] = pix_load4(g.a, b, p - (long long)b * hw, n0 + 4 * (slot % (BR / 4)));
            }
        }
#pragma unroll
        for (int i = 0; i < BQ; ++i) {
            const int slot = tid + i * NT;
            const long long p = pbeg + (long long)s * BK + slot / (BC / 4);
            rb[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (p < pend) {
                const int b = (int)(p / hw), r = (int)(p - (long long)b * hw);
                const int y = r / g.w + dy, x = r % g.w + dx;
                if (y >= 0 && y < g.h && x >= 0 && x < g.w) rb[i] = pix_load4(g.b, b, (long long)y * g.w + x, m0 + 4 * (slot % (BC / 4)));
            }
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    const int col0 = wc * 64;
    const bool do_n[2] = {m0 + col0 < g.Md, m0 + col0 + 32 < g.Md};
    const bool colsum = blockIdx.y == 0 && tid < BR;           // one workgroup per (row tile, slice) also sums its rows of a
    float csum = 0.0f;
    if (steps > 0) fetch(0);
    for (int s = 0; s < steps; ++s) {
#pragma unroll
        for (int i = 0; i < AQ; ++i) {
            const int slot = tid + i * NT;
            *(float4*)&As[slot / (BR / 4)][4 * (slot % (BR / 4))] = ra[i];
        }
#pragma unroll
        for (int i = 0; i < BQ; ++i) {
            const int slot = tid + i * NT;
            *(float4*)&Bs[slot / (BC / 4)][4 * (slot % (BC / 4))] = rb[i];
        }
        __syncthreads();
        if (s + 1 < steps) fetch(s + 1);
        if (colsum)
#pragma unroll
            for (int k = 0; k < BK; ++k) csum += As[k][tid];
        mfma_step<LDA, LDB>(As, Bs, wr * 64, col0, lane, do_n, acc);
        __syncthreads();
    }
    if (colsum && n0 + tid < g.N) g.colpart[(long long)slice * g.N + n0 + tid] = csum;
#pragma unroll
    for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int ni = 0; ni < 2; ++ni) {
            const int m = m0 + col0 + 32 * ni + (lane & 31);
            if (m >= g.Md) continue;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int n = n0 + wr * 64 + 32 * mi + acc_row(reg, lane);
                if (n < g.N) g.part[(((long long)slice * g.N + n) * g.taps + t) * g.Md + m] = acc[mi][ni][reg];
            }
        }
}

// out[n * ons + t * ots + m * oms] = the slices' parts added in order; colout[n] alike
__global__ __launch_bounds__(NT) void reduce_fold_kernel(const float* part, const float* colpart, int slices, int N, int taps, int Md, float* out,
                                                         long long ons, long long ots, long long oms, float* colout)
{
    const long long per = (long long)N * taps * Md, e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e < per) {
        float v = 0.0f;
        for (int s = 0; s < slices; ++s) v += part[s * per + e];
        const int n = (int)(e / ((long long)taps * Md)), r = (int)(e - (long long)n * taps * Md), t = r / Md, m = r - t * Md;
        out[n * ons + t * ots + m * oms] = v;
    }
    if (e < N) {
        float v = 0.0f;
        for (int s = 0; s < slices; ++s) v += colpart[(long long)s * N + e];
        colout[e] = v;
    }
}

// ---- host ----
int64_t round64(int64_t floats) { return (floats + 63) / 64 * 64; }
int slice_len_of(int64_t P)
{
    if (P <= (int64_t)SLICE_MIN * SLICE_MAX_N) return SLICE_MIN;
    return (int)(((P + SLICE_MAX_N - 1) / SLICE_MAX_N + BK - 1) / BK * BK);
}
int slices_of(int64_t P) { return (int)((P + slice_len_of(P) - 1) / slice_len_of(P)); }
// where a reduction keeps its slices' parts: part [slices][N * taps * Md] | colpart [slices][N]
struct RedWs {
    float* part;
    float* colpart;
    int slices, slice_len;
};
// a smap_heads_x of h x w pixels of C channels; 0 or SMAP_E_ARG
int take_x(const smap_heads_x* x, int h, int w, int C, Pix& out)
{
    if (!x || !x->ptr) return SMAP_E_ARG;
    const bool f32 = x->layout == SMAP_HEADS_X_F32, hilo = x->layout == SMAP_HEADS_X_F16_HILO;
    if (!f32 && !hilo && x->layout != SMAP_HEADS_X_F16) return SMAP_E_ARG;
    if (x->pix_stride < (hilo ? 2 * C : C) || x->pix_stride % 4 || ((uintptr_t)x->ptr & (f32 ? 15 : 7))) return SMAP_E_ARG;
    out = Pix{x->ptr, (long long)h * w * x->pix_stride, x->pix_stride, 1, x->layout, C, C, 1};
    return 0;
}
bool bad_f32(const void* p) { return !p || ((uintptr_t)p & 3); }
bool bad_image(int B, int h, int w) { return B < 1 || B > 65535 || h < 1 || w < 1 || (int64_t)h * w > (1 << 24) || (int64_t)B * h * w > (1 << 26); }
// a workspace of `floats` floats: 256-byte aligned, ws_bytes long at least
bool bad_ws(const void* ws, int64_t ws_bytes, int64_t floats) { return !ws || ((uintptr_t)ws & 255) || ws_bytes < floats * 4; }

Pix dense(const float* p, int hw, int pix_stride, int C)
{
    return Pix{p, (long long)hw * pix_stride, pix_stride, 1, SMAP_HEADS_X_F32, 0, C, 1};
}

int launch_conv(const ConvArgs& g, hipStream_t st)
{
    const long long P = (long long)g.B * g.h * g.w;
    if (g.N > 64)
        hipLaunchKernelGGL((conv_gemm_kernel<2, 2>), dim3((unsigned)((P + 127) / 128), (unsigned)((g.N + 127) / 128)), dim3(NT), 0, st, g);
    else
        hipLaunchKernelGGL((conv_gemm_kernel<4, 1>), dim3((unsigned)((P + 255) / 256), 1), dim3(NT), 0, st, g);
    return hip_rc(hipGetLastError());
}
// out[n][t][m] by the given strides = sum_p a[p, n] * b[p + t, m]; colout[n] = sum_p a[p, n]
int launch_reduce(RedArgs g, const RedWs& r, float* out, long long ons, long long ots, long long oms, float* colout, hipStream_t st)
{
    g.part = r.part, g.colpart = r.colpart, g.slice_len = r.slice_len;
    if (g.N > 64)
        hipLaunchKernelGGL((reduce_gemm_kernel<2, 2>), dim3((unsigned)((g.N + 127) / 128), (unsigned)((g.Md + 127) / 128 * g.taps), (unsigned)r.slices),
                           dim3(NT), 0, st, g);
    else
        hipLaunchKernelGGL((reduce_gemm_kernel<1, 4>), dim3(1, (unsigned)((g.Md + 255) / 256 * g.taps), (unsigned)r.slices), dim3(NT), 0, st, g);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    const long long per = (long long)g.N * g.taps * g.Md;
    hipLaunchKernelGGL(reduce_fold_kernel, dim3((unsigned)((per + NT - 1) / NT)), dim3(NT), 0, st, g.part, g.colpart, r.slices, g.N, g.taps, g.Md, out,
                       ons, ots, oms, colout);
    return hip_rc(hipGetLastError());
}

}  // namespace
}  // namespace gemm_f32
#endif
