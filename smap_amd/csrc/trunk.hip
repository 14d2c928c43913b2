// trunk.hip -- the trunk of one Upsample_unit (model/smap.py: out = relu(u_skip(x) + up_conv(interpolate(out_prev)))) with BN folded,
// in fp32: forward, and the exact gradient of that forward.  P = B * h * w pixels, X [P, Cin]; O_prev [P', chl] at h' x w' (absent for
// the coarsest unit); I = bilinear align_corners interpolation h' x w' -> h x w by ATen's index and weight rule (csrc/plan.h lerp_index).
// The rows of I sum to 1, so the 1x1 commutes with it: nothing of size [P, chl] is interpolated before a GEMM in either direction.
//   forward   S = X Wu^T        U = O_prev Wc^T (at LOW resolution)       O = relu(S + I(U) + b),  b = bu + bc
//   backward  gPre = gO where O > 0, else 0       gb = sum_p gPre  (the gradient of bu and of bc alike)
//             gWu = gPre^T X    gX = gPre Wu  (optional)
//             gU = I^T gPre  [P', chl]            gWc = gU^T O_prev            gO_prev = gU Wc
// The five GEMMs are conv_gemm and reduce_gemm of csrc/gemm_f32_device.h (shared with heads.hip).  Three small kernels here, all fp32,
// NHWC, one thread per four channels, 16-byte accesses:
//   upadd_forward   O = relu((S + tap(U)) + b), the tap expression ly0 (lx0 v00 + lx1 v01) + ly1 (lx0 v10 + lx1 v11) of ATen's kernel.
//   relu_mask       gPre = gO where O > 0, stored once: the gWu | gb reduction, the adjoint and (where wanted) the gX GEMM read it.
//   upadd_adjoint   gather form: one thread per (low-resolution cell, channel quad) adds (wy * wx) * gPre over the high-resolution pixels
//                   whose taps name its cell, (y, x) ascending, within a pixel the first tap before the second: an fmaf chain from 0.
//                   No atomics: the same bits run to run.
// The coarsest unit has no up path: its forward is ONE conv_gemm launch with the bias and the ReLU in its epilogue.
// Compiled with -ffp-contract=off: every operation rounds once, in the order written.
#include "gemm_f32_device.h"
#include "plan.h"            // lerp_index: the bilinear align-corners index rule the engine's kernels use

namespace {

namespace G = gemm_f32;
using G::Pix;
using G::Wgt;

constexpr int NT = G::NT;

struct Up {
    int B, h, w, hp, wp, chl;       // high h x w, low hp x wp
};

// O[p, c] = relu((S[p, c] + tap(U)[p, c]) + b[c]); one thread per (pixel, channel quad)
__global__ __launch_bounds__(NT) void upadd_forward_kernel(const float* __restrict__ S, const float* __restrict__ U, const float* __restrict__ bias,
                                                           float* __restrict__ O, Up d)
{
    const int q4 = d.chl / 4;
    const long long e = (long long)blockIdx.x * NT + threadIdx.x, total = (long long)d.B * d.h * d.w * q4;
    if (e >= total) return;
    const int c = (int)(e % q4) * 4;
    const long long p = e / q4;
    const int hw = d.h * d.w, b = (int)(p / hw), r = (int)(p - (long long)b * hw), y = r / d.w, x = r - y * d.w;
    const Lerp ly = lerp_index(y, d.hp, d.h), lx = lerp_index(x, d.wp, d.w);
    const float* base = U + (long long)b * d.hp * d.wp * d.chl + c;
    const float4 v00 = *(const float4*)(base + ((long long)ly.i0 * d.wp + lx.i0) * d.chl);
    const float4 v01 = *(const float4*)(base + ((long long)ly.i0 * d.wp + lx.i1) * d.chl);
    const float4 v10 = *(const float4*)(base + ((long long)ly.i1 * d.wp + lx.i0) * d.chl);
    const float4 v11 = *(const float4*)(base + ((long long)ly.i1 * d.wp + lx.i1) * d.chl);
    const float4 s = *(const float4*)(S + p * d.chl + c), bb = *(const float4*)(bias + c);
    auto one = [&](float sv, float a00, float a01, float a10, float a11, float bv) {
        const float t = ly.l0 * (lx.l0 * a00 + lx.l1 * a01) + ly.l1 * (lx.l0 * a10 + lx.l1 * a11);
        return fmaxf((sv + t) + bv, 0.0f);
    };
    *(float4*)(O + p * d.chl + c) = make_float4(one(s.x, v00.x, v01.x, v10.x, v11.x, bb.x), one(s.y, v00.y, v01.y, v10.y, v11.y, bb.y),
                                                one(s.z, v00.z, v01.z, v10.z, v11.z, bb.z), one(s.w, v00.w, v01.w, v10.w, v11.w, bb.w));
}

// gPre = gO where O > 0, else 0; n4 float4s
__global__ __launch_bounds__(NT) void relu_mask_kernel(const float4* __restrict__ gO, const float4* __restrict__ O, float4* __restrict__ gPre, long long n4)
{
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= n4) return;
    const float4 g = gO[e], o = O[e];
    gPre[e] = make_float4(o.x > 0.0f ? g.x : 0.0f, o.y > 0.0f ? g.y : 0.0f, o.z > 0.0f ? g.z : 0.0f, o.w > 0.0f ? g.w : 0.0f);
}

// the first dst in [0, out_size] whose first tap is at least a (it never decreases with dst); out_size when there is none
__device__ __forceinline__ int first_at_least(int a, int in_size, int out_size)
{
    int lo = 0, hi = out_size;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (lerp_index(mid, in_size, out_size).i0 >= a) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// gU[cell, c] = sum over the pixels (y, x) and their taps (ry, rx) that name the cell of (l_ry(y) * l_rx(x)) * gPre[y, x, c].  A pixel's taps are
// i0 and i1 >= i0 with i1 <= i0 + 1, so the rows that can name cell row i are those whose i0 is i - 1 or i: one contiguous range.
__global__ __launch_bounds__(NT) void upadd_adjoint_kernel(const float* __restrict__ gPre, float* __restrict__ gU, Up d)
{
    const int q4 = d.chl / 4;
    const long long e = (long long)blockIdx.x * NT + threadIdx.x, total = (long long)d.B * d.hp * d.wp * q4;
    if (e >= total) return;
    const int c = (int)(e % q4) * 4;
    const long long cell = e / q4;
    const int hwp = d.hp * d.wp, b = (int)(cell / hwp), r = (int)(cell - (long long)b * hwp), i = r / d.wp, j = r - i * d.wp;
    const int y0 = first_at_least(i - 1, d.hp, d.h), y1 = first_at_least(i + 1, d.hp, d.h);
    const int x0 = first_at_least(j - 1, d.wp, d.w), x1 = first_at_least(j + 1, d.wp, d.w);
    const float* base = gPre + (long long)b * d.h * d.w * d.chl + c;
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int y = y0; y < y1; ++y) {
        const Lerp ly = lerp_index(y, d.hp, d.h);
        for (int ry = 0; ry < 2; ++ry) {
            if ((ry ? ly.i1 : ly.i0) != i) continue;
            const float wy = ry ? ly.l1 : ly.l0;
            for (int x = x0; x < x1; ++x) {
                const Lerp lx = lerp_index(x, d.wp, d.w);
                const float4 g = *(const float4*)(base + ((long long)y * d.w + x) * d.chl);
                for (int rx = 0; rx < 2; ++rx) {
                    if ((rx ? lx.i1 : lx.i0) != j) continue;
                    const float wt = wy * (rx ? lx.l1 : lx.l0);
                    acc.x = fmaf(wt, g.x, acc.x), acc.y = fmaf(wt, g.y, acc.y), acc.z = fmaf(wt, g.z, acc.z), acc.w = fmaf(wt, g.w, acc.w);
                }
            }
        }
    }
    *(float4*)(gU + cell * d.chl + c) = acc;
}

// ---- host ----
struct Layout {
    int64_t s, u, part, colpart, junk, floats;      // offsets in floats; s | u hold S | U (forward) or gPre | gU (backward)
    int slices, slice_len, slices_lo, slice_len_lo;
};
// forward: S [P][chl] | U [P'][chl].  backward: gPre [P][chl] | gU [P'][chl] | part [max(slices chl Cin, slices' chl chl)] |
// colpart [max(slices, slices')][chl] | colsum [chl] (the column sums of gU, which nothing reads).  No up path: P' = 0.
Layout layout_of(int64_t P, int64_t Pl, int cin, int chl, int backward)
{
    Layout l{};
    l.slice_len = G::slice_len_of(P), l.slices = G::slices_of(P);
    if (Pl) l.slice_len_lo = G::slice_len_of(Pl), l.slices_lo = G::slices_of(Pl);
    l.s = 0;
    l.floats = G::round64(P * chl);
    l.u = l.floats;
    l.floats += G::round64(Pl * chl);
    if (!backward) return l;
    l.part = l.floats;
    const int64_t hi = (int64_t)l.slices * chl * cin, lo = (int64_t)l.slices_lo * chl * chl;
    l.floats += G::round64(hi > lo ? hi : lo);
    l.colpart = l.floats;
    l.floats += G::round64((int64_t)(l.slices > l.slices_lo ? l.slices : l.slices_lo) * chl);
    l.junk = l.floats;
    l.floats += G::round64(chl);
    return l;
}
// hp == 0 and wp == 0: no up path
bool bad_dims(int B, int h, int w, int hp, int wp, int cin, int chl)
{
    if (G::bad_image(B, h, w) || chl < 64 || chl > 1024 || chl % 64 || cin < 64 || cin > 4096 || cin % 64) return true;
    if (hp == 0 && wp == 0) return false;
    return G::bad_image(B, hp, wp);
}
bool bad_f32x4(const void* p) { return !p || ((uintptr_t)p & 15); }
unsigned blocks_of(long long threads) { return (unsigned)((threads + NT - 1) / NT); }

// out [P][out_ps] (N channels written) = a W (+ bias, relu), W element (k, n) at w[k * ks + n * ns]
int launch_1x1(const Pix& a, const float* w, long long ks, long long ns, int K, int N, const float* bias, int relu, float* out, int out_ps, int B, int h,
               int wd, hipStream_t st)
{
    G::ConvArgs g{};
    g.a = a, g.wt = Wgt{w, 0, ks, ns, K, N};
    g.out = out, g.out_fs = (long long)h * wd * out_ps, g.out_ps = out_ps, g.out_cs = 1;
    g.bias = bias, g.relu = relu, g.B = B, g.h = h, g.w = wd, g.N = N, g.taps = 1;
    return G::launch_conv(g, st);
}

}  // namespace

extern "C" {

int64_t smap_trunk_ws_bytes(int B, int h, int w, int hp, int wp, int cin, int chl, int backward)
{
    if (bad_dims(B, h, w, hp, wp, cin, chl)) return SMAP_E_ARG;
    return layout_of((int64_t)B * h * w, (int64_t)B * hp * wp, cin, chl, backward).floats * 4;
}

int smap_trunk_forward(const smap_heads_x* x, const smap_heads_x* o_prev, const float* wu, const float* wc, const float* b, float* o, int B, int h,
                       int w, int hp, int wp, int cin, int chl, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (bad_dims(B, h, w, hp, wp, cin, chl) || G::bad_f32(wu) || bad_f32x4(b) || bad_f32x4(o)) return SMAP_E_ARG;
    const bool up = o_prev != nullptr;
    if (up != (hp > 0) || up != (wc != nullptr) || (up && G::bad_f32(wc))) return SMAP_E_ARG;
    Pix px, pl;
    if (G::take_x(x, h, w, cin, px) || (up && G::take_x(o_prev, hp, wp, chl, pl))) return SMAP_E_ARG;
    const Layout l = layout_of((int64_t)B * h * w, (int64_t)B * hp * wp, cin, chl, 0);
    if (G::bad_ws(workspace, workspace_bytes, l.floats)) return SMAP_E_ARG;
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (!up) return launch_1x1(px, wu, 1, cin, cin, chl, b, 1, o, chl, B, h, w, st);             // O = relu(X Wu^T + b)
    if (int rc = launch_1x1(px, wu, 1, cin, cin, chl, nullptr, 0, ws + l.s, chl, B, h, w, st)) return rc;        // S
    if (int rc = launch_1x1(pl, wc, 1, chl, chl, chl, nullptr, 0, ws + l.u, chl, B, hp, wp, st)) return rc;      // U, at low resolution
    const Up d{B, h, w, hp, wp, chl};
    hipLaunchKernelGGL(upadd_forward_kernel, dim3(blocks_of((long long)B * h * w * (chl / 4))), dim3(NT), 0, st, ws + l.s, ws + l.u, b, o, d);
    return hip_rc(hipGetLastError());
}

int smap_trunk_backward(const smap_heads_x* x, const smap_heads_x* o_prev, const float* o, const float* wu, const float* wc, const float* g_o,
                        float* gwu, float* gwc, float* gb, float* g_o_prev, float* gx, int gx_pix_stride, int B, int h, int w, int hp, int wp,
                        int cin, int chl, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (bad_dims(B, h, w, hp, wp, cin, chl) || G::bad_f32(wu) || bad_f32x4(o) || bad_f32x4(g_o) || G::bad_f32(gwu) || G::bad_f32(gb)) return SMAP_E_ARG;
    const bool up = o_prev != nullptr;
    if (up != (hp > 0) || up != (wc != nullptr) || up != (gwc != nullptr) || up != (g_o_prev != nullptr)) return SMAP_E_ARG;
    if (up && (G::bad_f32(wc) || G::bad_f32(gwc) || G::bad_f32(g_o_prev))) return SMAP_E_ARG;
    if (gx && (((uintptr_t)gx & 3) || gx_pix_stride < cin)) return SMAP_E_ARG;                  // gx null: that gradient is not wanted
    Pix px, pl;
    if (G::take_x(x, h, w, cin, px) || (up && G::take_x(o_prev, hp, wp, chl, pl))) return SMAP_E_ARG;
    const Layout l = layout_of((int64_t)B * h * w, (int64_t)B * hp * wp, cin, chl, 1);
    if (G::bad_ws(workspace, workspace_bytes, l.floats)) return SMAP_E_ARG;
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const long long P = (long long)B * h * w;
    hipLaunchKernelGGL(relu_mask_kernel, dim3(blocks_of(P * (chl / 4))), dim3(NT), 0, st, (const float4*)g_o, (const float4*)o, (float4*)(ws + l.s),
                       P * (chl / 4));
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    const Pix gpre = G::dense(ws + l.s, h * w, chl, chl);
    G::RedArgs r{};                                              // gWu [chl][Cin] | gb
    r.a = gpre, r.b = px, r.B = B, r.h = h, r.w = w, r.N = chl, r.Md = cin, r.taps = 1;
    if (int rc = G::launch_reduce(r, G::RedWs{ws + l.part, ws + l.colpart, l.slices, l.slice_len}, gwu, cin, 0, 1, gb, st)) return rc;
    if (gx)                                                      // gX = gPre Wu
        if (int rc = launch_1x1(gpre, wu, cin, 1, chl, cin, nullptr, 0, gx, gx_pix_stride, B, h, w, st)) return rc;
    if (!up) return 0;
    const Up d{B, h, w, hp, wp, chl};
    hipLaunchKernelGGL(upadd_adjoint_kernel, dim3(blocks_of((long long)B * hp * wp * (chl / 4))), dim3(NT), 0, st, ws + l.s, ws + l.u, d);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    const Pix gu = G::dense(ws + l.u, hp * wp, chl, chl);
    G::RedArgs q{};                                              // gWc [chl][chl]
    q.a = gu, q.b = pl, q.B = B, q.h = hp, q.w = wp, q.N = chl, q.Md = chl, q.taps = 1;
    if (int rc = G::launch_reduce(q, G::RedWs{ws + l.part, ws + l.colpart, l.slices_lo, l.slice_len_lo}, gwc, chl, 0, 1, ws + l.junk, st)) return rc;
    return launch_1x1(gu, wc, chl, 1, chl, chl, nullptr, 0, g_o_prev, chl, B, hp, wp, st);      // gO_prev = gU Wc
}

}  // extern "C"
