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
//
// smap_loss_forward_src: the same value with every head read where the engine left it (SrcTable: pointer, size and strides per tensor, by
// value too), at its own resolution, interpolated to H x W on the fly -- three launches:
//   reduce_src  one workgroup per (chunk of 256 output pixels, frame, head), all 57 channels: 64 pixels at a time, the source values (16-byte
//               reads of four channels where the source is pixel-major, the tap expression of plan.hip's head_source4) go through an LDS
//               transpose, then wave w owns channels w, w + 4, ... and lane l pixel l, so a label row is read 256 bytes at a time; fifteen
//               double accumulators per lane, folded over the lanes once at the end -> partial [head][frame][chunk][57].
//   fold_src    one workgroup per (frame, head): the chunks' partials added in chunk order -> sums; root_d at the frame's rows.
//   finish      as above.
// smap_loss_backward_src: the gradient of that value at the heads' own resolution, the adjoint of the upsampling -- two launches:
//   part        one thread per (interval between source cells, channel, frame, head): its output pixels once, four partial sums to scratch;
//               the heads of H x W element-wise; root_d zeroed, then one thread per (frame, head) adds the rows' taps in order.
//   fold        one thread per (source cell, channel, frame, head): the up to nine partial sums of its cell in a fixed order.
// Compiled with -ffp-contract=off: every operation rounds once, in the order written.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "smap_hip.h"
#include "hip_rc.h"
#include "loss_core.h"
#include "plan.h"            // lerp_index: the bilinear align-corners index rule the engine's kernels use

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

// ---- the reduction from head sources ---------------------------------------------------------------------------------------------
struct Src {
    const float* p;          // element (frame b, pixel y, x, channel c) = p[b * frame + (y * w + x) * pix + c * ch]
    int h, w, pix, ch;
    long long frame;
};
struct SrcTable { Src s[3 * MAX_HEADS]; };      // [3 * h + 0 / 1 / 2] = heatmap_2d, det_d, root_d of head h

constexpr int SRC_SUB = 64, SRC_CHUNK = 256, SRC_ROWS = (NC + 3) / 4, SRC_LD = SRC_SUB + 1;

// 16-byte reads of four channels: channel-contiguous, every pixel 16-byte aligned, the pixel wide enough for the last group
__device__ __forceinline__ bool src_vec(const Src& s, int c)
{
    return s.ch == 1 && !(s.pix & 3) && s.pix >= ((c + 3) & ~3) && !(s.frame & 3) && !((uintptr_t)s.p & 15);
}

// the source's bilinear (align_corners) image at output pixel (y, x), channel c: ATen's index rule (lerp_index) and the tap expression of
// head_source4 (csrc/plan.hip); a source at the output's size is read as it is, one of height or width 1 has all its taps at index 0
__device__ __forceinline__ float src_value1(const Src& s, int b, int y, int x, int c, int H, int W)
{
    const float* base = s.p + (int64_t)b * s.frame + (int64_t)c * s.ch;
    if (s.h == H && s.w == W) return base[((int64_t)y * W + x) * s.pix];
    const Lerp ly = lerp_index(y, s.h, H), lx = lerp_index(x, s.w, W);
    const float v00 = base[((int64_t)ly.i0 * s.w + lx.i0) * s.pix], v01 = base[((int64_t)ly.i0 * s.w + lx.i1) * s.pix];
    const float v10 = base[((int64_t)ly.i1 * s.w + lx.i0) * s.pix], v11 = base[((int64_t)ly.i1 * s.w + lx.i1) * s.pix];
    return ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
}
__device__ __forceinline__ float4 src_value4(const Src& s, int b, int y, int x, int c, int H, int W)
{
    const float* base = s.p + (int64_t)b * s.frame + c;
    if (s.h == H && s.w == W) return *reinterpret_cast<const float4*>(base + ((int64_t)y * W + x) * s.pix);
    const Lerp ly = lerp_index(y, s.h, H), lx = lerp_index(x, s.w, W);
    const float4 v00 = *reinterpret_cast<const float4*>(base + ((int64_t)ly.i0 * s.w + lx.i0) * s.pix);
    const float4 v01 = *reinterpret_cast<const float4*>(base + ((int64_t)ly.i0 * s.w + lx.i1) * s.pix);
    const float4 v10 = *reinterpret_cast<const float4*>(base + ((int64_t)ly.i1 * s.w + lx.i0) * s.pix);
    const float4 v11 = *reinterpret_cast<const float4*>(base + ((int64_t)ly.i1 * s.w + lx.i1) * s.pix);
    float4 up;
    up.x = ly.l0 * (lx.l0 * v00.x + lx.l1 * v01.x) + ly.l1 * (lx.l0 * v10.x + lx.l1 * v11.x);
    up.y = ly.l0 * (lx.l0 * v00.y + lx.l1 * v01.y) + ly.l1 * (lx.l0 * v10.y + lx.l1 * v11.y);
    up.z = ly.l0 * (lx.l0 * v00.z + lx.l1 * v01.z) + ly.l1 * (lx.l0 * v10.z + lx.l1 * v11.z);
    up.w = ly.l0 * (lx.l0 * v00.w + lx.l1 * v01.w) + ly.l1 * (lx.l0 * v10.w + lx.l1 * v11.w);
    return up;
}

// grid (chunks, B, n_heads).  partial [n_heads][B][chunks][57].  acc[] is indexed by unrolled loops only: registers, no private array
// with a run-time index (EXPERIMENTS R3.6).
__global__ __launch_bounds__(NT) void loss_reduce_src_kernel(SrcTable tab, const float* __restrict__ labels, Params p,
                                                              double* __restrict__ partial)
{
    __shared__ float tile[NC * SRC_LD];
    const int chunk = blockIdx.x, chunks = gridDim.x, b = blockIdx.y, h = blockIdx.z, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int HW = p.H * p.W;
    const Src s2 = tab.s[3 * h], sd = tab.s[3 * h + 1];
    const bool vec = src_vec(s2, N2D) && src_vec(sd, NDD);                       // uniform over the workgroup
    const float* lab = labels + ((int64_t)b * p.S + head_scale(p, h)) * NC * HW;
    double acc[SRC_ROWS];
#pragma unroll
    for (int k = 0; k < SRC_ROWS; ++k) acc[k] = 0.0;
    const int last = min(HW, (chunk + 1) * SRC_CHUNK);
    for (int pix0 = chunk * SRC_CHUNK; pix0 < last; pix0 += SRC_SUB) {
        if (vec) {                                                               // item = (pixel, group of four channels): 12 + 4 groups
            for (int idx = t; idx < SRC_SUB * 16; idx += NT) {
                const int px = idx >> 4, g = idx & 15, pix = pix0 + px;
                if (pix >= HW) continue;
                const int y = pix / p.W, x = pix - y * p.W;
                const bool flat = g < 12;
                const int c = flat ? 4 * g : 4 * (g - 12), n = flat ? N2D : NDD, row = flat ? c : N2D + c;
                if (c >= n) continue;                                            // (the twelfth group of the 43 channels)
                const float4 v = flat ? src_value4(s2, b, y, x, c, p.H, p.W) : src_value4(sd, b, y, x, c, p.H, p.W);
                tile[row * SRC_LD + px] = v.x;
                if (c + 1 < n) tile[(row + 1) * SRC_LD + px] = v.y;
                if (c + 2 < n) tile[(row + 2) * SRC_LD + px] = v.z;
                if (c + 3 < n) tile[(row + 3) * SRC_LD + px] = v.w;
            }
        } else {                                                                 // item = (channel, pixel), pixels fastest
            for (int idx = t; idx < NC * SRC_SUB; idx += NT) {
                const int c = idx >> 6, px = idx & 63, pix = pix0 + px;
                if (pix >= HW) continue;
                const int y = pix / p.W, x = pix - y * p.W;
                tile[c * SRC_LD + px] = c < N2D ? src_value1(s2, b, y, x, c, p.H, p.W) : src_value1(sd, b, y, x, c - N2D, p.H, p.W);
            }
        }
        __syncthreads();
        const int pix = pix0 + lane;
        if (pix < HW) {
#pragma unroll
            for (int k = 0; k < SRC_ROWS; ++k) {
                const int c = wave + 4 * k;
                if (c < NC) {
                    const float d = tile[c * SRC_LD + lane] - lab[(int64_t)label_channel(c) * HW + pix];
                    acc[k] += (double)d * (double)d;
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < SRC_ROWS; ++k) {
        double a = acc[k];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
        const int c = wave + 4 * k;
        if (lane == 0 && c < NC) partial[((((int64_t)h * p.B + b) * chunks) + chunk) * NC + c] = a;
    }
}

// grid (B, n_heads), 64 threads: the chunks in order; root_d at the frame's rows (a row outside the map is never dereferenced)
__global__ __launch_bounds__(64) void loss_fold_src_kernel(SrcTable tab, const float* __restrict__ rdepth, Params p,
                                                           const double* __restrict__ partial, int chunks, double* __restrict__ sums,
                                                           float* __restrict__ rd_at, int32_t* __restrict__ root_cell)
{
    const int b = blockIdx.x, h = blockIdx.y, t = threadIdx.x;
    const int64_t frame = (int64_t)h * p.B + b;
    if (t < NC) {
        const double* q = partial + frame * chunks * NC + t;
        double s = 0.0;
        for (int i = 0; i < chunks; ++i) s += q[(int64_t)i * NC];
        sums[frame * NC + t] = s;
    }
    const Src sr = tab.s[3 * h + 2];
    for (int r = t; r < p.R; r += 64) {
        const int cell = root_row_cell(p, rdepth + ((int64_t)b * p.R + r) * 3);
        rd_at[frame * p.R + r] = cell >= 0 ? src_value1(sr, b, cell / p.W, cell % p.W, 0, p.H, p.W) : 0.0f;
        root_cell[frame * p.R + r] = cell;
    }
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

// ---- the gradient at the head sources: the adjoint of the on-the-fly upsampling ----------------------------------------------------
// Every output pixel (y, x) has its taps i0 / i1 (lerp_index); the pixels that share (i0(y), i0(x)) = (a, b) form the INTERVAL (a, b)
// of a source, and all of them read the same four source cells.  part: one thread per (interval, channel, frame, head) walks its
// pixels row by row, x ascending -- e = (up - label) * f with src_value1's tap expression -- and leaves the four sums
//     P[ry][rx] = sum_y l_ry(y) * sum_x l_rx(x) * e[y, x]           (r = 0: the pixel's weight on its first tap, 1: on its second)
// in `scratch`; each label is read by exactly one thread.  fold: one thread per (cell, channel, frame, head) adds the up to nine
// partial sums that name its cell -- intervals a = i - 1, i, within each b = j - 1, j, the second-tap sum before the first-tap one --
// and stores the gradient.  The order depends on (h, w, H, W) alone and the addressing of a layout never enters the arithmetic.  A source of H x W is one
// element-wise pass inside the first launch, which also owns root_d: zero-fill, then one thread walks the frame's rows.
struct GradDst {
    float* p;                // element (frame b, cell i, j, channel c) = p[b * frame + (i * w + j) * pix + c * ch]; null: not wanted
    int pix, ch;
    long long frame;
};
struct GradTable {
    GradDst g[3 * MAX_HEADS];
    long long part[2 * MAX_HEADS];      // [2 * h + 0 / 1]: where the partial sums of heatmap_2d / det_d of head h begin in scratch (floats)
};

// lerp_index's i1 for every pixel whose i0 is a
__device__ __forceinline__ int second_tap(int a, int in_size, int out_size)
{
    return in_size == out_size ? a : a + (a < in_size - 1 ? 1 : 0);
}
// the first dst in [0, out_size] whose i0 is at least a (i0 never decreases with dst); out_size when there is none
__device__ __forceinline__ int first_at_least(int a, int in_size, int out_size)
{
    int lo = 0, hi = out_size;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lerp_index(mid, in_size, out_size).i0 >= a) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// grid (58 * nblk, B, n_heads): block = (channel, slice of the tensor's intervals | pixels).
__global__ __launch_bounds__(NT) void loss_backward_src_part_kernel(SrcTable tab, GradTable gt, const float* __restrict__ labels, Params p,
                                                                     const float* __restrict__ coef, const int32_t* __restrict__ root_cell,
                                                                     const float* __restrict__ root_fac, const float* __restrict__ upstream,
                                                                     float* __restrict__ scratch, int nblk)
{
    const int c = blockIdx.x / nblk, blk = blockIdx.x % nblk, b = blockIdx.y, h = blockIdx.z, t = threadIdx.x;
    const int HW = p.H * p.W;
    const float up = upstream[0];
    if (c == NC) {                                             // root_d: zeros, then ONE thread adds the frame's rows in order
        const Src s = tab.s[3 * h + 2];
        const GradDst gd = gt.g[3 * h + 2];
        if (blk != 0 || !gd.p) return;
        float* g = gd.p + (int64_t)b * gd.frame;
        const int cells = s.h * s.w;
        for (int i = t; i < cells; i += NT) g[(int64_t)i * gd.pix] = 0.0f;
        __syncthreads();                                       // the workgroup's own stores: visible to its thread 0 behind the barrier
        if (t == 0) {
            const int64_t base = ((int64_t)h * p.B + b) * p.R;
            const bool same = s.h == p.H && s.w == p.W;
            for (int r = 0; r < p.R; ++r) {
                const int cell = root_cell[base + r];
                if (cell < 0 || cell >= HW) continue;          // skipped, or outside the map: never dereferenced
                const float v = root_fac[base + r] * up;
                if (same) {
                    g[(int64_t)cell * gd.pix] += v;
                    continue;
                }
                const Lerp ly = lerp_index(cell / p.W, s.h, p.H), lx = lerp_index(cell % p.W, s.w, p.W);
                g[((int64_t)ly.i0 * s.w + lx.i0) * gd.pix] += v * (ly.l0 * lx.l0);
                g[((int64_t)ly.i0 * s.w + lx.i1) * gd.pix] += v * (ly.l0 * lx.l1);
                g[((int64_t)ly.i1 * s.w + lx.i0) * gd.pix] += v * (ly.l1 * lx.l0);
                g[((int64_t)ly.i1 * s.w + lx.i1) * gd.pix] += v * (ly.l1 * lx.l1);
            }
        }
        return;
    }
    const int k = c < N2D ? 0 : 1, cc = k ? c - N2D : c, cn = k ? NDD : N2D;
    const Src s = tab.s[3 * h + k];
    const GradDst gd = gt.g[3 * h + k];
    if (!gd.p) return;
    const float f = coef[((int64_t)h * p.B + b) * NC + c] * up;
    const float* lab = label_plane(labels, p, h, b, c, HW);
    const float* src = s.p + (int64_t)b * s.frame + (int64_t)cc * s.ch;
    if (s.h == p.H && s.w == p.W) {                            // the identity: g = e; zero weight or not selected: zeros, nothing read
        float* g = gd.p + (int64_t)b * gd.frame + (int64_t)cc * gd.ch;
        for (int i = blk * NT + t; i < HW; i += nblk * NT) g[(int64_t)i * gd.pix] = f == 0.0f ? 0.0f : (src[(int64_t)i * s.pix] - lab[i]) * f;
        return;
    }
    const int idx = blk * NT + t;
    if (f == 0.0f || idx >= s.h * s.w) return;                 // (the fold writes a zero-factor channel's zeros)
    const int a = idx / s.w, bc = idx - a * s.w;
    const int a1 = second_tap(a, s.h, p.H), b1 = second_tap(bc, s.w, p.W);
    const float v00 = src[((int64_t)a * s.w + bc) * s.pix], v01 = src[((int64_t)a * s.w + b1) * s.pix];
    const float v10 = src[((int64_t)a1 * s.w + bc) * s.pix], v11 = src[((int64_t)a1 * s.w + b1) * s.pix];
    const int y0 = first_at_least(a, s.h, p.H), y1 = first_at_least(a + 1, s.h, p.H);
    const int x0 = first_at_least(bc, s.w, p.W), x1 = first_at_least(bc + 1, s.w, p.W);
    float p00 = 0.0f, p01 = 0.0f, p10 = 0.0f, p11 = 0.0f;
    for (int y = y0; y < y1; ++y) {
        const Lerp ly = lerp_index(y, s.h, p.H);
        const float* row = lab + (int64_t)y * p.W;
        float r0 = 0.0f, r1 = 0.0f;
        for (int x = x0; x < x1; ++x) {
            const Lerp lx = lerp_index(x, s.w, p.W);
            const float u = ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);      // src_value1's expression
            const float e = (u - row[x]) * f;
            r0 += lx.l0 * e;
            r1 += lx.l1 * e;
        }
        p00 += ly.l0 * r0;
        p01 += ly.l0 * r1;
        p10 += ly.l1 * r0;
        p11 += ly.l1 * r1;
    }
    float4* out = reinterpret_cast<float4*>(scratch + gt.part[2 * h + k]) + (((int64_t)b * cn + cc) * s.h + a) * s.w + bc;
    *out = make_float4(p00, p01, p10, p11);
}

// grid (57 * nblk, B, n_heads): block = (channel, slice of the tensor's cells); sources of H x W were finished by the first launch.
__global__ __launch_bounds__(NT) void loss_backward_src_fold_kernel(SrcTable tab, GradTable gt, Params p, const float* __restrict__ coef,
                                                                     const float* __restrict__ upstream, const float* __restrict__ scratch,
                                                                     int nblk)
{
    const int c = blockIdx.x / nblk, blk = blockIdx.x % nblk, b = blockIdx.y, h = blockIdx.z, t = threadIdx.x;
    const int k = c < N2D ? 0 : 1, cc = k ? c - N2D : c, cn = k ? NDD : N2D;
    const Src s = tab.s[3 * h + k];
    const GradDst gd = gt.g[3 * h + k];
    const int idx = blk * NT + t;
    if (!gd.p || (s.h == p.H && s.w == p.W) || idx >= s.h * s.w) return;
    const int i = idx / s.w, j = idx - i * s.w;
    const float f = coef[((int64_t)h * p.B + b) * NC + c] * upstream[0];
    float acc = 0.0f;
    if (f != 0.0f) {
        const float* part = scratch + gt.part[2 * h + k] + (((int64_t)b * cn + cc) * s.h) * s.w * 4;
        for (int a = max(i - 1, 0); a <= i; ++a)
            for (int ry = 1; ry >= 0; --ry) {                  // interval a names cell row i with its second tap, then with its first
                if (ry ? second_tap(a, s.h, p.H) != i : a != i) continue;
                for (int bc = max(j - 1, 0); bc <= j; ++bc)
                    for (int rx = 1; rx >= 0; --rx) {
                        if (rx ? second_tap(bc, s.w, p.W) != j : bc != j) continue;
                        acc += part[((int64_t)a * s.w + bc) * 4 + 2 * ry + rx];
                    }
            }
    }
    gd.p[(int64_t)b * gd.frame + (int64_t)idx * gd.pix + (int64_t)cc * gd.ch] = acc;
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

// smap_loss_forward_src's workspace: the layout above, then partial [n_heads][B][chunks][57] f64
int src_chunks(int H, int W) { return (H * W + SRC_CHUNK - 1) / SRC_CHUNK; }
int64_t src_partial_offset(int n_heads, int B, int R) { return workspace_layout(n_heads, B, R).bytes; }

// a descriptor of c channels under an H x W output, as the kernels take it; 0 or SMAP_E_ARG
int take_src(const smap_head_src& s, int c, int H, int W, Src& out)
{
    if (!s.ptr || ((uintptr_t)s.ptr & 3) || s.h < 1 || s.w < 1 || s.h > H || s.w > W || s.c != c || s.pix_stride < 1 || s.ch_stride < 1 ||
        s.frame_stride < 1)
        return SMAP_E_ARG;
    // the strides describe a tensor that does not fold onto itself: channel-minor (NHWC, padded or not) or pixel-minor (NCHW) order
    const int64_t px = (int64_t)s.h * s.w;
    const bool nhwc = s.ch_stride == 1 && s.pix_stride >= c && s.frame_stride >= px * s.pix_stride;
    const bool nchw = s.pix_stride == 1 && s.ch_stride >= px && s.frame_stride >= (int64_t)c * s.ch_stride;
    if (!nhwc && !nchw) return SMAP_E_ARG;
    out = Src{s.ptr, s.h, s.w, s.pix_stride, s.ch_stride, (long long)s.frame_stride};
    return 0;
}

// smap_loss_backward_src's scratch: per tensor the four partial sums of every interval, f32 [B][c][h][w][4]
int64_t part_floats(int h, int w, int c, int B) { return (int64_t)B * c * h * w * 4; }

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

int smap_sizeof_head_src(void) { return (int)sizeof(smap_head_src); }

int64_t smap_loss_src_workspace_bytes(int n_heads, int B, int R, int H, int W)
{
    if (n_heads < 1 || n_heads > MAX_HEADS || B < 1 || B > 65535 || R < 1 || R > 65535 || H < 1 || W < 1 || (int64_t)H * W > (1 << 24))
        return SMAP_E_ARG;
    return src_partial_offset(n_heads, B, R) + (int64_t)n_heads * B * src_chunks(H, W) * NC * 8;
}

int smap_loss_forward_src(const smap_head_src* sources, const float* labels, const float* valids, const float* rdepth, int stage_num,
                          int ohkm, int topk, int ctf, int B, int S, int R, int H, int W, void* workspace, int64_t workspace_bytes,
                          float* result, void* stream)
{
    Params p = make_params(stage_num, ohkm, topk, ctf, 0, B, S, R, H, W);
    if (check_params(p) || !sources || !labels || !valids || !rdepth || !workspace || !result || ((uintptr_t)workspace & 7))
        return SMAP_E_ARG;
    SrcTable tab{};
    for (int i = 0; i < 3 * p.n_heads; ++i)
        if (take_src(sources[i], i % 3 == 0 ? N2D : (i % 3 == 1 ? NDD : 1), H, W, tab.s[i])) return SMAP_E_ARG;
    const Workspace w = workspace_layout(p.n_heads, B, R);
    const int chunks = src_chunks(H, W);
    if (workspace_bytes < smap_loss_src_workspace_bytes(p.n_heads, B, R, H, W)) return SMAP_E_ARG;
    char* ws = (char*)workspace;
    double* partial = (double*)(ws + src_partial_offset(p.n_heads, B, R));
    hipLaunchKernelGGL(loss_reduce_src_kernel, dim3((unsigned)chunks, (unsigned)B, (unsigned)p.n_heads), dim3(NT), 0, (hipStream_t)stream, tab,
                       labels, p, partial);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    hipLaunchKernelGGL(loss_fold_src_kernel, dim3((unsigned)B, (unsigned)p.n_heads), dim3(64), 0, (hipStream_t)stream, tab, rdepth, p, partial,
                       chunks, (double*)(ws + w.sums), (float*)(ws + w.rd_at), (int32_t*)(ws + w.root_cell));
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

int64_t smap_loss_backward_src_scratch_bytes(const smap_head_src* sources, int n_heads, int B)
{
    if (!sources || n_heads < 1 || n_heads > MAX_HEADS || B < 1 || B > 65535) return SMAP_E_ARG;
    int64_t floats = 0;
    for (int i = 0; i < 3 * n_heads; ++i) {
        const smap_head_src& s = sources[i];
        if (s.h < 1 || s.w < 1 || (int64_t)s.h * s.w > (1 << 24)) return SMAP_E_ARG;
        if (i % 3 < 2) floats += part_floats(s.h, s.w, i % 3 ? NDD : N2D, B);
    }
    return floats * 4;
}

int smap_loss_backward_src(const smap_head_src* sources, const smap_head_src* grads, const float* labels, int stage_num, int ohkm, int topk,
                           int ctf, int B, int S, int R, int H, int W, const void* workspace, int64_t workspace_bytes, void* scratch,
                           int64_t scratch_bytes, const float* upstream, void* stream)
{
    Params p = make_params(stage_num, ohkm, topk, ctf, 0, B, S, R, H, W);
    if (check_params(p) || !sources || !grads || !labels || !workspace || !upstream || ((uintptr_t)workspace & 7) || ((uintptr_t)scratch & 15))
        return SMAP_E_ARG;
    if (workspace_bytes < workspace_layout(p.n_heads, B, R).bytes) return SMAP_E_ARG;
    SrcTable tab{};
    GradTable gt{};
    int64_t floats = 0;
    int nblk_part = 1, nblk_fold = 0;
    for (int i = 0; i < 3 * p.n_heads; ++i) {
        const int c = i % 3 == 0 ? N2D : (i % 3 == 1 ? NDD : 1);
        if (take_src(sources[i], c, H, W, tab.s[i])) return SMAP_E_ARG;
        const smap_head_src& g = grads[i];
        if (!g.ptr) continue;                                   // not wanted: gt.g[i].p stays null
        Src dst;
        if (g.h != sources[i].h || g.w != sources[i].w || take_src(g, c, H, W, dst)) return SMAP_E_ARG;
        gt.g[i] = GradDst{const_cast<float*>(g.ptr), g.pix_stride, g.ch_stride, (long long)g.frame_stride};
        if (i % 3 == 2) continue;
        const int64_t cells = (int64_t)g.h * g.w;
        if (g.h == H && g.w == W) {
            nblk_part = max(nblk_part, (int)((cells + 4 * NT - 1) / (4 * NT)));
        } else {
            gt.part[2 * (i / 3) + i % 3] = floats;
            floats += part_floats(g.h, g.w, c, B);
            nblk_part = max(nblk_part, (int)((cells + NT - 1) / NT));
            nblk_fold = max(nblk_fold, (int)((cells + NT - 1) / NT));
        }
    }
    if (floats && (!scratch || scratch_bytes < floats * 4)) return SMAP_E_ARG;
    const Workspace w = workspace_layout(p.n_heads, B, R);
    const char* ws = (const char*)workspace;
    const float* coef = (const float*)(ws + w.coef);
    hipLaunchKernelGGL(loss_backward_src_part_kernel, dim3((unsigned)(GRAD_C * nblk_part), (unsigned)B, (unsigned)p.n_heads), dim3(NT), 0,
                       (hipStream_t)stream, tab, gt, labels, p, coef, (const int32_t*)(ws + w.root_cell), (const float*)(ws + w.root_fac),
                       upstream, (float*)scratch, nblk_part);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    if (!nblk_fold) return 0;
    hipLaunchKernelGGL(loss_backward_src_fold_kernel, dim3((unsigned)(NC * nblk_fold), (unsigned)B, (unsigned)p.n_heads), dim3(NT), 0,
                       (hipStream_t)stream, tab, gt, p, coef, upstream, (const float*)scratch, nblk_fold);
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
