// heads.hip -- the three head arms of one Upsample_unit (model/smap.py: res*_conv1 1x1 chl -> chl, BN, ReLU; res*_conv2 3x3 chl -> C_a, BN)
// with BN folded, in fp32: forward, and the exact gradient of that forward.  One unit: P = B * h * w pixels, X = out [P, chl], arms a = 0, 1, 2.
//   forward   Z_a = X W1_a^T + b1_a      M_a = relu(Z_a)      Y_a = conv3x3(M_a, W2_a, pad 1) + b2_a
//   backward  gb2_a = sum_p G_a          gW2_a[c, ci, t] = sum_p G_a[p, c] M_a[p + t, ci]   (p + t inside the image)
//             gM_a = conv3x3^T(G_a, W2_a)   gZ_a = gM_a where Z_a > 0   gb1_a = sum_p gZ_a   gW1_a = gZ_a^T X   gX = sum_a gZ_a W1_a
// The two kernels behind every launch, conv_gemm and reduce_gemm, and their descriptors and launch helpers are csrc/gemm_f32_device.h
// (shared with trunk.hip).  conv_gemm serves Z|M (1 tap, N = 3 chl), Y_a (9 taps), gM_a -> gZ_a (9 taps mirrored, mask M_a) and gX (1 tap,
// K = 3 chl); reduce_gemm serves gW2_a | gb2_a and gW1 | gb1.
#include "gemm_f32_device.h"

namespace {

using namespace gemm_f32;

constexpr int MAX_ARM_C = 64;            // channels of one arm's head tensor (43 | 14 | 1 in the network)

// ---- host ----
struct Layout {
    int64_t m, gz, part, colpart, floats;     // offsets in floats
    int slices, slice_len;
};
// M [P][3 chl] | gZ [P][3 chl] | part [slices][max(3 chl * chl, 64 * 9 * chl)] | colpart [slices][3 chl]; the forward pass needs M alone
Layout layout_of(int64_t P, int chl, int backward)
{
    Layout l{};
    l.slice_len = slice_len_of(P);
    l.slices = slices_of(P);
    l.m = 0;
    l.floats = round64(P * 3 * chl);
    if (!backward) return l;
    l.gz = l.floats;
    l.floats += round64(P * 3 * chl);
    l.part = l.floats;
    l.floats += round64((int64_t)l.slices * chl * (3 * chl > 9 * MAX_ARM_C ? 3 * chl : 9 * MAX_ARM_C));
    l.colpart = l.floats;
    l.floats += round64((int64_t)l.slices * 3 * chl);
    return l;
}
bool bad_dims(int B, int h, int w, int chl)
{
    return bad_image(B, h, w) || chl < 64 || chl > 1024 || chl % 64;
}
// the three head tensors of a unit (c = 1 .. 64 each, h x w); 0 or SMAP_E_ARG
int take_heads(const smap_head_src* s, int h, int w, Pix out[3])
{
    if (!s) return SMAP_E_ARG;
    for (int a = 0; a < 3; ++a) {
        const smap_head_src& d = s[a];
        if (!d.ptr || ((uintptr_t)d.ptr & 3) || d.h != h || d.w != w || d.c < 1 || d.c > MAX_ARM_C || d.pix_stride < 1 || d.ch_stride < 1) return SMAP_E_ARG;
        const int64_t px = (int64_t)h * w;
        const bool nhwc = d.ch_stride == 1 && d.pix_stride >= d.c && d.frame_stride >= px * d.pix_stride;
        const bool nchw = d.pix_stride == 1 && d.ch_stride >= px && d.frame_stride >= (int64_t)d.c * d.ch_stride;
        if (!nhwc && !nchw) return SMAP_E_ARG;
        const int vec = d.ch_stride == 1 && d.pix_stride % 4 == 0 && d.frame_stride % 4 == 0 && !((uintptr_t)d.ptr & 15);
        out[a] = Pix{d.ptr, (long long)d.frame_stride, d.pix_stride, d.ch_stride, SMAP_HEADS_X_F32, 0, d.c, vec};
    }
    return 0;
}

RedWs red_ws(const Layout& l, float* ws) { return RedWs{ws + l.part, ws + l.colpart, l.slices, l.slice_len}; }
// M = relu(X W1cat^T + b1cat) into the workspace
int launch_m(const Pix& x, const float* w1cat, const float* b1cat, int B, int h, int w, int chl, float* m, hipStream_t st)
{
    ConvArgs g{};
    g.a = x, g.wt = Wgt{w1cat, 0, 1, chl, chl, 3 * chl};
    g.out = m, g.out_fs = (long long)h * w * 3 * chl, g.out_ps = 3 * chl, g.out_cs = 1;
    g.bias = b1cat, g.relu = 1, g.B = B, g.h = h, g.w = w, g.N = 3 * chl, g.taps = 1;
    return launch_conv(g, st);
}

}  // namespace

extern "C" {

int smap_sizeof_heads_x(void) { return (int)sizeof(smap_heads_x); }

int64_t smap_heads_ws_bytes(int B, int h, int w, int chl, int backward)
{
    if (bad_dims(B, h, w, chl)) return SMAP_E_ARG;
    return layout_of((int64_t)B * h * w, chl, backward).floats * 4;
}

int smap_heads_forward(const smap_heads_x* x, const float* w1cat, const float* b1cat, const float* const* w2, const float* const* b2,
                       const smap_head_src* y, int B, int h, int w, int chl, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (bad_dims(B, h, w, chl) || bad_f32(w1cat) || bad_f32(b1cat) || !w2 || !b2) return SMAP_E_ARG;
    Pix px, py[3];
    if (take_x(x, h, w, chl, px) || take_heads(y, h, w, py)) return SMAP_E_ARG;
    for (int a = 0; a < 3; ++a)
        if (bad_f32(w2[a]) || bad_f32(b2[a])) return SMAP_E_ARG;
    const Layout l = layout_of((int64_t)B * h * w, chl, 0);
    if (bad_ws(workspace, workspace_bytes, l.floats)) return SMAP_E_ARG;
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_m(px, w1cat, b1cat, B, h, w, chl, ws + l.m, st)) return rc;
    for (int a = 0; a < 3; ++a) {
        ConvArgs g{};
        g.a = dense(ws + l.m + a * chl, h * w, 3 * chl, chl);
        g.wt = Wgt{w2[a], 1, 9, (long long)chl * 9, chl, py[a].C};
        g.out = (float*)py[a].ptr, g.out_fs = py[a].frame_stride, g.out_ps = py[a].pix_stride, g.out_cs = py[a].ch_stride;
        g.bias = b2[a], g.B = B, g.h = h, g.w = w, g.N = py[a].C, g.taps = 9;
        if (int rc = launch_conv(g, st)) return rc;
    }
    return 0;
}

int smap_heads_backward(const smap_heads_x* x, const float* w1cat, const float* b1cat, const float* const* w2, const smap_head_src* g_heads,
                        int B, int h, int w, int chl, float* gw1cat, float* gb1cat, float* const* gw2, float* const* gb2, float* gx,
                        int gx_pix_stride, void* workspace, int64_t workspace_bytes, void* stream)
{
    if (bad_dims(B, h, w, chl) || bad_f32(w1cat) || bad_f32(b1cat) || !w2 || bad_f32(gw1cat) || bad_f32(gb1cat) || !gw2 || !gb2) return SMAP_E_ARG;
    Pix px, pg[3];
    if (take_x(x, h, w, chl, px) || take_heads(g_heads, h, w, pg)) return SMAP_E_ARG;
    for (int a = 0; a < 3; ++a)
        if (bad_f32(w2[a]) || bad_f32(gw2[a]) || bad_f32(gb2[a])) return SMAP_E_ARG;
    if (gx && (((uintptr_t)gx & 3) || gx_pix_stride < chl)) return SMAP_E_ARG;          // gx null: that gradient is not wanted
    const Layout l = layout_of((int64_t)B * h * w, chl, 1);
    if (bad_ws(workspace, workspace_bytes, l.floats)) return SMAP_E_ARG;
    float* ws = (float*)workspace;
    hipStream_t st = (hipStream_t)stream;
    const int hw = h * w;
    if (int rc = launch_m(px, w1cat, b1cat, B, h, w, chl, ws + l.m, st)) return rc;
    for (int a = 0; a < 3; ++a) {
        const Pix m = dense(ws + l.m + a * chl, hw, 3 * chl, chl);
        RedArgs r{};                                             // gW2_a [C_a][chl][3][3] | gb2_a
        r.a = pg[a], r.b = m, r.B = B, r.h = h, r.w = w, r.N = pg[a].C, r.Md = chl, r.taps = 9;
        if (int rc = launch_reduce(r, red_ws(l, ws), gw2[a], (long long)chl * 9, 1, 9, gb2[a], st)) return rc;
        ConvArgs g{};                                            // gZ_a = conv3x3^T(G_a, W2_a) where M_a > 0
        g.a = pg[a], g.wt = Wgt{w2[a], 1, (long long)chl * 9, 9, pg[a].C, chl};
        g.out = ws + l.gz + a * chl, g.out_fs = (long long)hw * 3 * chl, g.out_ps = 3 * chl, g.out_cs = 1;
        g.mask = ws + l.m + a * chl, g.mask_ps = 3 * chl;
        g.B = B, g.h = h, g.w = w, g.N = chl, g.taps = 9, g.mirror = 1;
        if (int rc = launch_conv(g, st)) return rc;
    }
    const Pix gz = dense(ws + l.gz, hw, 3 * chl, 3 * chl);
    RedArgs r{};                                                 // gW1cat [3 chl][chl] | gb1cat
    r.a = gz, r.b = px, r.B = B, r.h = h, r.w = w, r.N = 3 * chl, r.Md = chl, r.taps = 1;
    if (int rc = launch_reduce(r, red_ws(l, ws), gw1cat, chl, 0, 1, gb1cat, st)) return rc;
    if (!gx) return 0;
    ConvArgs g{};                                                // gX = gZ W1cat
    g.a = gz, g.wt = Wgt{w1cat, 0, chl, 1, 3 * chl, chl};
    g.out = gx, g.out_fs = (long long)hw * gx_pix_stride, g.out_ps = gx_pix_stride, g.out_cs = 1;
    g.B = B, g.h = h, g.w = w, g.N = chl, g.taps = 1;
    return launch_conv(g, st);
}

}  // extern "C"
