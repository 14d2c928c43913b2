// loss.hip -- the training loss of the network on gfx950: value and gradient of SMAP._calculate_loss (model/smap.py:355-401) with
// JointsL2Loss / DepthLoss (lib/utils/loss_h.py), over all 4 * stage_num heads.  Two routes, dense heads of H x W (HeadPtrs) and heads
// read where the engine left them (SrcTable: pointer, size and strides per tensor), both passed by value in the kernel arguments; they
// stay apart because their reductions add in different orders, and share the steps below.
//
// smap_loss_forward: reduce, finish.  smap_loss_backward: backward.
//   reduce    one workgroup per (channel of 57, frame, head): d = out - label in fp32 (one correctly rounded subtraction), the sum of
//             double(d) * double(d) in a FIXED order -- every thread walks the plane with the workgroup's stride, lanes fold with
//             wave_sum, waves through LDS -- so a value depends on its plane alone and is the same bits run to run.  No atomics.
//             One more workgroup per (frame, head) is root_rows: the cells of the frame's root-depth rows and root_d there.
//   finish    one workgroup: csrc/loss_core.h (the same text the host runs), a phase per barrier.
//   backward  one workgroup per (channel of 58, frame, head): grad = (out - label) * fp32(coef * upstream); a channel whose factor is
//             zero is zero_plane, nothing read.  The root_d plane is root_grad_plane: zeroed, then ONE thread adds its frame's rows in
//             order, so two persons on one cell add up the same way every time.
// smap_loss_forward_src: the same value, every head at its own resolution, interpolated to H x W on the fly (src_value1 / src_value4:
// lerp_index and the tap expression `tap`, as plan.hip's head_source4) -- reduce_src, fold_src, finish:
//   reduce_src  one workgroup per (chunk of 256 output pixels, frame, head), all 57 channels: 64 pixels at a time, the source values (16-byte
//               reads of four channels where the source is pixel-major) go through an LDS transpose, then wave w owns channels w, w + 4, ...
//               and lane l pixel l, so a label row is read 256 bytes at a time; fifteen double accumulators per lane, folded over the
//               lanes once at the end -> partial [head][frame][chunk][57].
//   fold_src    one workgroup per (frame, head): the chunks' partials added in chunk order -> sums; root_rows through src_value1.
// smap_loss_backward_src: the gradient of that value at the heads' own resolution, the adjoint of the upsampling -- part, fold:
//   part        one thread per (interval between source cells, channel, frame, head): its output pixels once, four partial sums to scratch;
//               the heads of H x W element-wise; root_d is root_grad_plane with the destination's stride and the four taps of a row.
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

struct Chan { int k, cc, cn; };          // of output channel c (0..56): its tensor within the head (0 / 1), its channel there, the tensor's channels
__device__ __forceinline__ Chan channel_of(int c) { return c < N2D ? Chan{0, c, N2D} : Chan{1, c - N2D, NDD}; }
// the plane of output channel c of frame b in its head, and the label plane it is compared with
__device__ __forceinline__ const float* out_plane(const HeadPtrs& hp, int h, int b, int c, int HW)
{
    const Chan ch = channel_of(c);
    const float* t = hp.p[3 * h + ch.k];
    if (!t) return nullptr;
    return t + ((int64_t)b * ch.cn + ch.cc) * HW;
}
__device__ __forceinline__ const float* label_plane(const float* labels, const Params& p, int h, int b, int c, int HW)
{
    return labels + (((int64_t)b * p.S + head_scale(p, h)) * NC + label_channel(c)) * HW;
}

__device__ __forceinline__ double wave_sum(double a)                   // lane 0 ends with the wave's sum, lanes added in a fixed order
{
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o, 64);
    return a;
}

// this thread's share (first, first + step, ...) of n zeros `stride` floats apart.  VEC: stride 1, n % 4 == 0, g 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void zero_plane(float* g, int n, int stride, int first, int step)
{
    if (VEC) {
        float4* g4 = (float4*)g;
        for (int i = first; i < (n >> 2); i += step) g4[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        for (int i = first; i < n; i += step) g[(int64_t)i * stride] = 0.0f;
    }
}

// the root-depth rows of frame b for head h, by nt threads: the cell of each and root_d there, rd(cell).  A row outside the map is never
// dereferenced, and root_row_cell is ROW_SKIPPED throughout when the head has no root_d
template <class ReadRd>
__device__ __forceinline__ void root_rows(const Params& p, const float* rdepth, int b, int h, int t, int nt, float* rd_at,
                                          int32_t* root_cell, ReadRd rd)
{
    const int64_t base = ((int64_t)h * p.B + b) * p.R;
    for (int r = t; r < p.R; r += nt) {
        const int cell = root_row_cell(p, rdepth + ((int64_t)b * p.R + r) * 3);
        rd_at[base + r] = cell >= 0 ? rd(cell) : 0.0f;
        root_cell[base + r] = cell;
    }
}

// the bilinear tap expression (head_source4's, csrc/plan.hip)
__device__ __forceinline__ float tap(const Lerp& ly, const Lerp& lx, float v00, float v01, float v10, float v11)
{
    return ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11);
}

// the root_d gradient plane of frame b, head h -- g: sh x sw cells `stride` floats apart -- by a workgroup of NT: zeros, then ONE thread
// adds the frame's rows in order, each at its cell (a plane of H x W) or spread over the cell's four taps
template <bool VEC>
__device__ __forceinline__ void root_grad_plane(float* g, int sh, int sw, int stride, const Params& p, int h, int b,
                                                const int32_t* root_cell, const float* root_fac, float up, int t)
{
    zero_plane<VEC>(g, sh * sw, stride, t, NT);
    __syncthreads();                                           // the workgroup's own stores: visible to its thread 0 behind the barrier
    if (t != 0) return;
    const int64_t base = ((int64_t)h * p.B + b) * p.R;
    const bool same = sh == p.H && sw == p.W;
    for (int r = 0; r < p.R; ++r) {
        const int cell = root_cell[base + r];
        if (cell < 0 || cell >= p.H * p.W) continue;           // skipped, or outside the map: never dereferenced
        const float v = root_fac[base + r] * up;
        if (same) { g[(int64_t)cell * stride] += v; continue; }
        const Lerp ly = lerp_index(cell / p.W, sh, p.H), lx = lerp_index(cell % p.W, sw, p.W);
        g[((int64_t)ly.i0 * sw + lx.i0) * stride] += v * (ly.l0 * lx.l0);
        g[((int64_t)ly.i0 * sw + lx.i1) * stride] += v * (ly.l0 * lx.l1);
        g[((int64_t)ly.i1 * sw + lx.i0) * stride] += v * (ly.l1 * lx.l0);
        g[((int64_t)ly.i1 * sw + lx.i1) * stride] += v * (ly.l1 * lx.l1);
    }
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
    if (c == NC) return root_rows(p, rdepth, b, h, t, NT, rd_at, root_cell, [&](int cell) { return hp.p[3 * h + 2][(int64_t)b * HW + cell]; });
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
    acc = wave_sum(acc);
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

// the source's bilinear (align_corners) image at output pixel (y, x), channel c: ATen's index rule (lerp_index) and `tap`; a source at the output's size is read as it is, one of height or width 1 has all its taps at index 0
__device__ __forceinline__ float src_value1(const Src& s, int b, int y, int x, int c, int H, int W)
{
    const float* base = s.p + (int64_t)b * s.frame + (int64_t)c * s.ch;
    if (s.h == H && s.w == W) return base[((int64_t)y * W + x) * s.pix];
    const Lerp ly = lerp_index(y, s.h, H), lx = lerp_index(x, s.w, W);
    const float v00 = base[((int64_t)ly.i0 * s.w + lx.i0) * s.pix], v01 = base[((int64_t)ly.i0 * s.w + lx.i1) * s.pix];
    const float v10 = base[((int64_t)ly.i1 * s.w + lx.i0) * s.pix], v11 = base[((int64_t)ly.i1 * s.w + lx.i1) * s.pix];
    return tap(ly, lx, v00, v01, v10, v11);
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
    return make_float4(tap(ly, lx, v00.x, v01.x, v10.x, v11.x), tap(ly, lx, v00.y, v01.y, v10.y, v11.y),
                       tap(ly, lx, v00.z, v01.z, v10.z, v11.z), tap(ly, lx, v00.w, v01.w, v10.w, v11.w));
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
        const double a = wave_sum(acc[k]);
        const int c = wave + 4 * k;
        if (lane == 0 && c < NC) partial[((((int64_t)h * p.B + b) * chunks) + chunk) * NC + c] = a;
    }
}

// grid (B, n_heads), 64 threads: the chunks in order; root_d at the frame's rows
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
    root_rows(p, rdepth, b, h, t, 64, rd_at, root_cell, [&](int cell) { return src_value1(sr, b, cell / p.W, cell % p.W, 0, p.H, p.W); });
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
        if (hp.p[3 * h + 2]) root_grad_plane<VEC>(gh + ((int64_t)p.B * NC + b) * HW, p.H, p.W, 1, p, h, b, root_cell, root_fac, up, t);
        return;
    }
    const float* out = out_plane(hp, h, b, c, HW);
    if (!out) return;
    float* g = gh + (c < N2D ? (int64_t)b * N2D + c : (int64_t)p.B * N2D + (int64_t)b * NDD + (c - N2D)) * HW;
    const float f = coef[((int64_t)h * p.B + b) * NC + c] * up;
    if (f == 0.0f) return zero_plane<VEC>(g, HW, 1, t, NT);    // zero weight or not selected: exactly zero, nothing read
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
// pixels row by row, x ascending -- e = (tap - label) * f -- and leaves the four sums
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
    if (c == NC) {
        const GradDst gd = gt.g[3 * h + 2];
        if (blk == 0 && gd.p)
            root_grad_plane<false>(gd.p + (int64_t)b * gd.frame, tab.s[3 * h + 2].h, tab.s[3 * h + 2].w, gd.pix, p, h, b, root_cell, root_fac, up, t);
        return;
    }
    const auto [k, cc, cn] = channel_of(c);
    const Src s = tab.s[3 * h + k];
    const GradDst gd = gt.g[3 * h + k];
    if (!gd.p) return;
    const float f = coef[((int64_t)h * p.B + b) * NC + c] * up;
    const float* lab = label_plane(labels, p, h, b, c, HW);
    const float* src = s.p + (int64_t)b * s.frame + (int64_t)cc * s.ch;
    if (s.h == p.H && s.w == p.W) {                            // the identity: g = e; zero weight or not selected: zeros, nothing read
        float* g = gd.p + (int64_t)b * gd.frame + (int64_t)cc * gd.ch;
        if (f == 0.0f) zero_plane<false>(g, HW, gd.pix, blk * NT + t, nblk * NT);
        else for (int i = blk * NT + t; i < HW; i += nblk * NT) g[(int64_t)i * gd.pix] = (src[(int64_t)i * s.pix] - lab[i]) * f;
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
            const float e = (tap(ly, lx, v00, v01, v10, v11) - row[x]) * f;
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
    const auto [k, cc, cn] = channel_of(c);
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
    return Params{single ? 1 : 4 * stage_num, stage_num, ohkm ? 1 : 0, topk, ctf ? 1 : 0, single ? 1 : 0, B, S, R, H, W, 1, 1, 1};
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
int64_t src_partial_bytes(int n_heads, int B, int H, int W) { return (int64_t)n_heads * B * src_chunks(H, W) * NC * 8; }

// what every launching entry point begins with: the parameters, and the workspace -- given, 8-byte aligned, the layout (and the
// partial sums behind it) in size
struct Call { Params p; Workspace w; char* ws; };
int begin_call(Call& c, int stage_num, int ohkm, int topk, int ctf, int single, int B, int S, int R, int H, int W, const void* workspace,
               int64_t workspace_bytes, bool partials = false)
{
    c.p = make_params(stage_num, ohkm, topk, ctf, single, B, S, R, H, W);
    if (check_params(c.p) || !workspace || ((uintptr_t)workspace & 7)) return SMAP_E_ARG;
    c.w = workspace_layout(c.p.n_heads, B, R);
    c.ws = (char*)workspace;
    return workspace_bytes < c.w.bytes + (partials ? src_partial_bytes(c.p.n_heads, B, H, W) : 0) ? SMAP_E_ARG : 0;
}

// the VEC instantiation of a kernel where every plane is 16-byte aligned and a multiple of four floats, its scalar twin otherwise
template <class... P, class... A>
void launch_planes(bool vec, void (*vec_kernel)(P...), void (*scalar_kernel)(P...), dim3 grid, void* stream, A... args)
{
    hipLaunchKernelGGL(vec ? vec_kernel : scalar_kernel, grid, dim3(NT), 0, (hipStream_t)stream, args...);
}

int launch_finish(const Call& c, const float* valids, const float* rdepth, float* result, void* stream)
{
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);     // of the reduction launched just before
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(FINISH_NT), 0, (hipStream_t)stream, c.p, valids, rdepth, c.ws, result);
    return hip_rc(hipGetLastError());
}

int tensor_channels(int i) { return i % 3 == 0 ? N2D : (i % 3 == 1 ? NDD : 1); }      // of tensor i of the 3 * n_heads

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
// smap_head_src[3 * n_heads] as the kernels take it; 0 or SMAP_E_ARG
int take_sources(const smap_head_src* sources, const Params& p, SrcTable& tab)
{
    if (!sources) return SMAP_E_ARG;
    for (int i = 0; i < 3 * p.n_heads; ++i)
        if (take_src(sources[i], tensor_channels(i), p.H, p.W, tab.s[i])) return SMAP_E_ARG;
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
    Call c;
    if (begin_call(c, stage_num, ohkm, topk, ctf, single, B, S, R, H, W, workspace, workspace_bytes) || !result) return SMAP_E_ARG;
    Params& p = c.p;
    HeadPtrs hp;
    bool aligned;
    if (take_heads(heads, p, hp, labels, aligned)) return SMAP_E_ARG;
    if (((p.has_hm || p.has_dd) && !valids) || !rdepth) return SMAP_E_ARG;       // the forward pass alone reads these two
    launch_planes(aligned && (H * W) % 4 == 0, loss_reduce_kernel<true>, loss_reduce_kernel<false>,
                  dim3(NC + 1, (unsigned)B, (unsigned)p.n_heads), stream, hp, labels, rdepth, p, (double*)(c.ws + c.w.sums),
                  (float*)(c.ws + c.w.rd_at), (int32_t*)(c.ws + c.w.root_cell));
    return launch_finish(c, valids, rdepth, result, stream);
}

int smap_sizeof_head_src(void) { return (int)sizeof(smap_head_src); }

int64_t smap_loss_src_workspace_bytes(int n_heads, int B, int R, int H, int W)
{
    const int64_t layout = smap_loss_workspace_bytes(n_heads, B, R);
    if (layout < 0 || H < 1 || W < 1 || (int64_t)H * W > (1 << 24)) return SMAP_E_ARG;
    return layout + src_partial_bytes(n_heads, B, H, W);
}

int smap_loss_forward_src(const smap_head_src* sources, const float* labels, const float* valids, const float* rdepth, int stage_num,
                          int ohkm, int topk, int ctf, int B, int S, int R, int H, int W, void* workspace, int64_t workspace_bytes,
                          float* result, void* stream)
{
    Call c;
    if (begin_call(c, stage_num, ohkm, topk, ctf, 0, B, S, R, H, W, workspace, workspace_bytes, true) || !labels || !valids || !rdepth || !result)
        return SMAP_E_ARG;
    const Params& p = c.p;
    SrcTable tab{};
    if (take_sources(sources, p, tab)) return SMAP_E_ARG;
    const int chunks = src_chunks(H, W);
    double* partial = (double*)(c.ws + c.w.bytes);
    hipLaunchKernelGGL(loss_reduce_src_kernel, dim3((unsigned)chunks, (unsigned)B, (unsigned)p.n_heads), dim3(NT), 0, (hipStream_t)stream, tab,
                       labels, p, partial);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    hipLaunchKernelGGL(loss_fold_src_kernel, dim3((unsigned)B, (unsigned)p.n_heads), dim3(64), 0, (hipStream_t)stream, tab, rdepth, p, partial,
                       chunks, (double*)(c.ws + c.w.sums), (float*)(c.ws + c.w.rd_at), (int32_t*)(c.ws + c.w.root_cell));
    return launch_finish(c, valids, rdepth, result, stream);
}

int smap_loss_backward(const void* const* heads, const float* labels, int stage_num, int ohkm, int topk, int ctf, int single, int B, int S,
                       int R, int H, int W, const void* workspace, int64_t workspace_bytes, const float* upstream, float* grad, void* stream)
{
    Call c;
    if (begin_call(c, stage_num, ohkm, topk, ctf, single, B, S, R, H, W, workspace, workspace_bytes) || !upstream || !grad) return SMAP_E_ARG;
    HeadPtrs hp;
    bool aligned;
    if (take_heads(heads, c.p, hp, labels, aligned)) return SMAP_E_ARG;          // valids and rdepth: the workspace's tables hold them
    launch_planes(aligned && !((uintptr_t)grad & 15) && (H * W) % 4 == 0, loss_backward_kernel<true>, loss_backward_kernel<false>,
                  dim3(GRAD_C, (unsigned)B, (unsigned)c.p.n_heads), stream, hp, labels, c.p, (const float*)(c.ws + c.w.coef),
                  (const int32_t*)(c.ws + c.w.root_cell), (const float*)(c.ws + c.w.root_fac), upstream, grad);
    return hip_rc(hipGetLastError());
}

int64_t smap_loss_backward_src_scratch_bytes(const smap_head_src* sources, int n_heads, int B)
{
    if (!sources || n_heads < 1 || n_heads > MAX_HEADS || B < 1 || B > 65535) return SMAP_E_ARG;
    int64_t floats = 0;
    for (int i = 0; i < 3 * n_heads; ++i) {
        const smap_head_src& s = sources[i];
        if (s.h < 1 || s.w < 1 || (int64_t)s.h * s.w > (1 << 24)) return SMAP_E_ARG;
        if (i % 3 < 2) floats += part_floats(s.h, s.w, tensor_channels(i), B);
    }
    return floats * 4;
}

int smap_loss_backward_src(const smap_head_src* sources, const smap_head_src* grads, const float* labels, int stage_num, int ohkm, int topk,
                           int ctf, int B, int S, int R, int H, int W, const void* workspace, int64_t workspace_bytes, void* scratch,
                           int64_t scratch_bytes, const float* upstream, void* stream)
{
    Call call;
    if (begin_call(call, stage_num, ohkm, topk, ctf, 0, B, S, R, H, W, workspace, workspace_bytes) || !grads || !labels || !upstream ||
        ((uintptr_t)scratch & 15))
        return SMAP_E_ARG;
    const Params& p = call.p;
    SrcTable tab{};
    if (take_sources(sources, p, tab)) return SMAP_E_ARG;
    GradTable gt{};
    int64_t floats = 0;
    int nblk_part = 1, nblk_fold = 0;
    for (int i = 0; i < 3 * p.n_heads; ++i) {
        const smap_head_src& g = grads[i];
        if (!g.ptr) continue;                                   // not wanted: gt.g[i].p stays null
        Src dst;
        if (g.h != sources[i].h || g.w != sources[i].w || take_src(g, tensor_channels(i), H, W, dst)) return SMAP_E_ARG;
        gt.g[i] = GradDst{const_cast<float*>(g.ptr), g.pix_stride, g.ch_stride, (long long)g.frame_stride};
        if (i % 3 == 2) continue;
        const int64_t cells = (int64_t)g.h * g.w;
        if (g.h == H && g.w == W) {
            nblk_part = max(nblk_part, (int)((cells + 4 * NT - 1) / (4 * NT)));
        } else {
            gt.part[2 * (i / 3) + i % 3] = floats;
            floats += part_floats(g.h, g.w, tensor_channels(i), B);
            nblk_part = max(nblk_part, (int)((cells + NT - 1) / NT));
            nblk_fold = max(nblk_fold, (int)((cells + NT - 1) / NT));
        }
    }
    if (floats && (!scratch || scratch_bytes < floats * 4)) return SMAP_E_ARG;
    const float* coef = (const float*)(call.ws + call.w.coef);
    hipLaunchKernelGGL(loss_backward_src_part_kernel, dim3((unsigned)(GRAD_C * nblk_part), (unsigned)B, (unsigned)p.n_heads), dim3(NT), 0,
                       (hipStream_t)stream, tab, gt, labels, p, coef, (const int32_t*)(call.ws + call.w.root_cell),
                       (const float*)(call.ws + call.w.root_fac), upstream, (float*)scratch, nblk_part);
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
