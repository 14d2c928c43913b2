// loss.hip -- the training loss of the network on gfx950: value and gradient of SMAP._calculate_loss (model/smap.py:355-401) with
// JointsL2Loss / DepthLoss (lib/utils/loss_h.py), over all 4 * stage_num heads in two launches forward and one backward.
//
//   reduce    one workgroup per (channel of 57, frame, head): d = out - label in fp32 (one correctly rounded subtraction), the sum of
//             double(d) * double(d) in a FIXED order -- every thread walks the plane with the workgroup's stride, lanes fold with
//             shuffles, waves through LDS -- so a value depends on its plane alone and is the same bits run to run.  No atomics.
//             One more workgroup per (frame, head) finds the cells of the frame's root-depth rows and reads root_d there.
//   finish    one workgroup: csrc/loss_core.h (the same text the host runs), a phase per barrier.
//   backward  one workgroup per (channel of 58, frame, head): grad = (out - label) * fp32(coef * upstream); a channel whose factor is
//             zero is written as zeros without reading anything.  The root_d plane is zeroed, then ONE thread adds its frame's rows in
//             order, so two persons on one cell add up the same way every time.
// The 3 * n_heads tensor pointers travel by value in the kernel arguments (HeadPtrs), as smap_preprocess_batch passes its frames.
// Compiled with -ffp-contract=off: every operation rounds once, in the order written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "smap_hip.h"
#include "hip_rc.h"
#include "loss_core.h"

namespace {

using namespace loss_core;

constexpr int NT = 256, FINISH_NT = 1024;

struct HeadPtrs {
    const float* p[3 * MAX_HEADS];        // [3 * h + 0 / 1 / 2] = heatmap_2d [B, 43, H, W], det_d [B, 14, H, W], root_d [B, 1, H, W]
};

// the plane of output channel c (0..56) of frame b in its head, and the label plane it is compared with
__device__ __forceinline__ const float* out_plane(const HeadPtrs& hp, int h, int b, int c, int HW)
{
    const float* t = c < N2D ? hp.p[3 * h] : hp.p[3 * h + 1];
    if (!t) return nullptr;
    return t + ((int64_t)b * (c < N2D ? N2D : NDD) + (c < N2D ? c : c - N2D)) * HW;
}
__device__ __forceinline__ const float* label_plane(const float* labels, const Params& p, int h, int b, int c, int HW)
{
    return labels + (((int64_t)b * p.S + head_scale(p, h)) * NC + label_channel(c)) * HW;
}

// ---- launch A ------------------------------------------------------------------------------------------------------------------
// grid (58, B, n_heads).  VEC: H * W % 4 == 0 and every tensor 16-byte aligned, so every plane is.
template <bool VEC>
__global__ __launch_bounds__(NT) void loss_reduce_kernel(HeadPtrs hp, const float* __restrict__ labels, const float* __restrict__ rdepth,
                                                          Params p, double* __restrict__ sums, float* __restrict__ rd_at,
                                                          int32_t* __restrict__ root_cell)
{
    __shared__ double s_part[NT / 64];
    const int c = blockIdx.x, b = blockIdx.y, h = blockIdx.z, t = threadIdx.x;
    const int HW = p.H * p.W;
    if (c == NC) {                                             // root_d at the frame's rows; a row outside the map is never dereferenced
        const float* rd = hp.p[3 * h + 2];
        for (int r = t; r < p.R; r += NT) {
            const int64_t row = (int64_t)b * p.R + r;
            const int cell = root_row_cell(p, rdepth + row * 3);           // ROW_SKIPPED throughout when the head has no root_d
            rd_at[(int64_t)h * p.B * p.R + row] = cell >= 0 ? rd[(int64_t)b * HW + cell] : 0.0f;
            root_cell[(int64_t)h * p.B * p.R + row] = cell;
        }
        return;
    }
    const float* out = out_plane(hp, h, b, c, HW);
    double acc = 0.0;
    if (out) {
        const float* lab = label_plane(labels, p, h, b, c, HW);
        if (VEC) {
            const float4* o4 = (const float4*)out;
            const float4* l4 = (const float4*)lab;
            const int n4 = HW >> 2;
#pragma unroll 4
            for (int i = t; i < n4; i += NT) {
                const float4 o = o4[i], l = l4[i];
                const float d0 = o.x - l.x, d1 = o.y - l.y, d2 = o.z - l.z, d3 = o.w - l.w;
                acc += (double)d0 * (double)d0;
                acc += (double)d1 * (double)d1;
                acc += (double)d2 * (double)d2;
                acc += (double)d3 * (double)d3;
            }
        } else {
#pragma unroll 4
            for (int i = t; i < HW; i += NT) {
                const float d = out[i] - lab[i];
                acc += (double)d * (double)d;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((t & 63) == 0) s_part[t >> 6] = acc;
    __syncthreads();
    if (t == 0) sums[((int64_t)h * p.B + b) * NC + c] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// ---- finish: csrc/loss_core.h, one workgroup ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(FINISH_NT) void loss_finish_kernel(Params p, const float* __restrict__ valids, const float* __restrict__ rdepth,
                                                                 char* ws, float* result)
{
    const int t = threadIdx.x;
    const int64_t frames = (int64_t)p.n_heads * p.B, n = frames * NC;
    const Workspace w = workspace_layout(p.n_heads, p.B, p.R);
    double* m = (double*)(ws + w.m);
    float* sel = (float*)(ws + w.sel);
    const float* rd_at = (const float*)(ws + w.rd_at);
    const int32_t* root_cell = (const int32_t*)(ws + w.root_cell);
    double* part = (double*)(ws + w.part);
    double* headloss = (double*)(ws + w.headloss);
    for (int64_t i = t; i < n; i += FINISH_NT) channel_mean(p, i, (const double*)(ws + w.sums), valids, m);
    __syncthreads();
    for (int64_t i = t; i < n; i += FINISH_NT) channel_select(p, i, m, valids, sel, (float*)(ws + w.coef));
    __syncthreads();
    for (int64_t i = t; i < frames; i += FINISH_NT) frame_partials(p, i, m, sel, rdepth, rd_at, root_cell, part);
    __syncthreads();
    if (t < p.n_heads) head_losses(p, t, part, headloss);
    __syncthreads();
    for (int64_t i = t; i < frames * p.R; i += FINISH_NT) root_factor(p, i, rdepth, rd_at, root_cell, headloss, (float*)(ws + w.root_fac));
    if (t == 0) totals(p, headloss, result);
}

// ---- launch B ------------------------------------------------------------------------------------------------------------------
// grid (58, B, n_heads).  grad: [n_heads] x ([B, 43, H, W] | [B, 14, H, W] | [B, 1, H, W]).
template <bool VEC>
__global__ __launch_bounds__(NT) void loss_backward_kernel(HeadPtrs hp, const float* __restrict__ labels, Params p,
                                                            const float* __restrict__ coef, const int32_t* __restrict__ root_cell,
                                                            const float* __restrict__ root_fac, const float* __restrict__ upstream,
                                                            float* __restrict__ grad)
{
    const int c = blockIdx.x, b = blockIdx.y, h = blockIdx.z, t = threadIdx.x;
    const int HW = p.H * p.W;
    const float up = upstream[0];
    float* gh = grad + (int64_t)h * p.B * GRAD_C * HW;
    if (c == NC) {
        if (!hp.p[3 * h + 2]) return;
        float* g = gh + ((int64_t)p.B * NC + b) * HW;
        if (VEC) {
            float4* g4 = (float4*)g;
            for (int i = t; i < (HW >> 2); i += NT) g4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            for (int i = t; i < HW; i += NT) g[i] = 0.0f;
        }
        __syncthreads();                                       // the workgroup's own stores: visible to its thread 0 behind the barrier
        if (t == 0) {
            const int64_t base = ((int64_t)h * p.B + b) * p.R;
            for (int r = 0; r < p.R; ++r) {
                const int cell = root_cell[base + r];
                if (cell >= 0 && cell < HW) g[cell] += root_fac[base + r] * up;
            }
        }
        return;
    }
    const float* out = out_plane(hp, h, b, c, HW);
    if (!out) return;
    float* g = gh + (c < N2D ? (int64_t)b * N2D + c : (int64_t)p.B * N2D + (int64_t)b * NDD + (c - N2D)) * HW;
    const float f = coef[((int64_t)h * p.B + b) * NC + c] * up;
    if (f == 0.0f) {                                           // zero weight or not selected: exactly zero, nothing read
        if (VEC) {
            float4* g4 = (float4*)g;
            for (int i = t; i < (HW >> 2); i += NT) g4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            for (int i = t; i < HW; i += NT) g[i] = 0.0f;
        }
        return;
    }
    const float* lab = label_plane(labels, p, h, b, c, HW);
    if (VEC) {
        const float4* o4 = (const float4*)out;
        const float4* l4 = (const float4*)lab;
        float4* g4 = (float4*)g;
#pragma unroll 4
        for (int i = t; i < (HW >> 2); i += NT) {
            const float4 o = o4[i], l = l4[i];
            g4[i] = make_float4((o.x - l.x) * f, (o.y - l.y) * f, (o.z - l.z) * f, (o.w - l.w) * f);
        }
    } else {
#pragma unroll 4
        for (int i = t; i < HW; i += NT) g[i] = (out[i] - lab[i]) * f;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
Params make_params(int stage_num, int ohkm, int topk, int ctf, int single, int B, int S, int R, int H, int W)
{
    Params p{};
    p.stage_num = stage_num;
    p.n_heads = single ? 1 : 4 * stage_num;
    p.ohkm = ohkm ? 1 : 0;
    p.topk = topk;
    p.ctf = ctf ? 1 : 0;
    p.single = single ? 1 : 0;
    p.B = B;
    p.S = S;
    p.R = R;
    p.H = H;
    p.W = W;
    p.has_hm = p.has_dd = p.has_rd = 1;
    return p;
}

// the heads of a launch: all three tensors of every head, or in single-head mode at least one; labels where a map is compared with them
int take_heads(const void* const* heads, Params& p, HeadPtrs& hp, const float* labels, bool& aligned)
{
    if (!heads) return SMAP_E_ARG;
    aligned = !((uintptr_t)labels & 15);
    for (int i = 0; i < 3 * MAX_HEADS; ++i) hp.p[i] = nullptr;
    for (int i = 0; i < 3 * p.n_heads; ++i) {
        hp.p[i] = (const float*)heads[i];
        if (!heads[i] && !p.single) return SMAP_E_ARG;
        if ((uintptr_t)heads[i] & 15) aligned = false;
    }
    p.has_hm = hp.p[0] != nullptr;
    p.has_dd = hp.p[1] != nullptr;
    p.has_rd = hp.p[2] != nullptr;
    if (!p.has_hm && !p.has_dd && !p.has_rd) return SMAP_E_ARG;
    if ((p.has_hm || p.has_dd) && !labels) return SMAP_E_ARG;
    return 0;
}

}  // namespace

extern "C" {

int64_t smap_loss_workspace_bytes(int n_heads, int B, int R)
{
    if (n_heads < 1 || n_heads > MAX_HEADS || B < 1 || B > 65535 || R < 1 || R > 65535) return SMAP_E_ARG;
    return workspace_layout(n_heads, B, R).bytes;
}

int smap_loss_forward(const void* const* heads, const float* labels, const float* valids, const float* rdepth, int stage_num, int ohkm,
                      int topk, int ctf, int single, int B, int S, int R, int H, int W, void* workspace, int64_t workspace_bytes,
                      float* result, void* stream)
{
    Params p = make_params(stage_num, ohkm, topk, ctf, single, B, S, R, H, W);
    if (check_params(p) || !workspace || !result || ((uintptr_t)workspace & 7)) return SMAP_E_ARG;
    HeadPtrs hp;
    bool aligned;
    if (take_heads(heads, p, hp, labels, aligned)) return SMAP_E_ARG;
    if (((p.has_hm || p.has_dd) && !valids) || !rdepth) return SMAP_E_ARG;       // the forward pass alone reads these two
    const Workspace w = workspace_layout(p.n_heads, B, R);
    if (workspace_bytes < w.bytes) return SMAP_E_ARG;
    char* ws = (char*)workspace;
    const dim3 grid(NC + 1, (unsigned)B, (unsigned)p.n_heads);
    if (aligned && (H * W) % 4 == 0)
        hipLaunchKernelGGL(loss_reduce_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, hp, labels, rdepth, p, (double*)(ws + w.sums),
                           (float*)(ws + w.rd_at), (int32_t*)(ws + w.root_cell));
    else
        hipLaunchKernelGGL(loss_reduce_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, hp, labels, rdepth, p, (double*)(ws + w.sums),
                           (float*)(ws + w.rd_at), (int32_t*)(ws + w.root_cell));
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(FINISH_NT), 0, (hipStream_t)stream, p, valids, rdepth, ws, result);
    return hip_rc(hipGetLastError());
}

int smap_loss_backward(const void* const* heads, const float* labels, int stage_num, int ohkm, int topk, int ctf, int single, int B, int S,
                       int R, int H, int W, const void* workspace, int64_t workspace_bytes, const float* upstream, float* grad, void* stream)
{
    Params p = make_params(stage_num, ohkm, topk, ctf, single, B, S, R, H, W);
    if (check_params(p) || !workspace || !upstream || !grad || ((uintptr_t)workspace & 7)) return SMAP_E_ARG;
    HeadPtrs hp;
    bool aligned;
    if (take_heads(heads, p, hp, labels, aligned)) return SMAP_E_ARG;            // valids and rdepth: the workspace's tables hold them
    if ((uintptr_t)grad & 15) aligned = false;
    const Workspace w = workspace_layout(p.n_heads, B, R);
    if (workspace_bytes < w.bytes) return SMAP_E_ARG;
    const char* ws = (const char*)workspace;
    const dim3 grid(GRAD_C, (unsigned)B, (unsigned)p.n_heads);
    if (aligned && (H * W) % 4 == 0)
        hipLaunchKernelGGL(loss_backward_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, hp, labels, p, (const float*)(ws + w.coef),
                           (const int32_t*)(ws + w.root_cell), (const float*)(ws + w.root_fac), upstream, grad);
    else
        hipLaunchKernelGGL(loss_backward_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, hp, labels, p, (const float*)(ws + w.coef),
                           (const int32_t*)(ws + w.root_cell), (const float*)(ws + w.root_fac), upstream, grad);
    return hip_rc(hipGetLastError());
}

int smap_loss_finish_host(const double* sums, const float* valids, const float* rdepth, const float* rd_at_rows, int stage_num, int ohkm,
                          int topk, int ctf, int single, int B, int R, int H, int W, double* result, double* m, double* sel, double* coef,
                          int32_t* root_cell, double* root_fac, double* part)
{
    Params p = make_params(stage_num, ohkm, topk, ctf, single, B, 8, R, H, W);      // S plays no part behind the reduction
    if (check_params(p) || !sums || !valids || !rdepth || !rd_at_rows || !result || !m || !sel || !coef || !root_cell || !root_fac || !part)
        return SMAP_E_ARG;
    double headloss[MAX_HEADS * HEADLOSS] = {};
    finish_serial<double>(p, sums, valids, rdepth, rd_at_rows, m, sel, coef, root_cell, root_fac, part, headloss, result);
    return 0;
}

}  // extern "C"
