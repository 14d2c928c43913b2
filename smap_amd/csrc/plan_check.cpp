// plan_check.cpp -- which schedules the library runs: the guard between a foreign host (include/smap_hip.h) or a cached plan blob and the
// ~150 kernel launches of smap_plan_run.  Host only: no HIP header, builds with a plain C++17 compiler (tests/c/plan_check_main.cpp runs
// it under AddressSanitizer / UBSan).  Everything here that depends on WHERE an op reads or writes goes through one walk, for_each_span.
#include <algorithm>
#include <climits>
#include <cstring>
#include <initializer_list>
#include "plan_check.h"
#include "tiles.h"

namespace {

// ---- sizes: products of op fields, in int64.  A negative factor or a product beyond int64 makes the op invalid.
bool product(int64_t* r, std::initializer_list<int64_t> factors)
{
    int64_t n = 1;
    for (int64_t x : factors)
        if (x < 0 || __builtin_mul_overflow(n, x, &n)) return false;
    *r = n;
    return true;
}
bool within(int64_t limit, std::initializer_list<int64_t> factors)
{
    int64_t n;
    return product(&n, factors) && n <= limit;
}
inline int64_t cout8(const smap_op& o) { return (o.Cout + 7LL) & ~7LL; }      // channels a conv writes: Cout rounded up to 8

// ---- the walk: every byte range an op touches
enum SpanBuf { ARENA, OUTPUT, WEIGHTS };                      // the activation arena, the fp32 output buffer, the weight section
enum SpanRole { READ, WRITTEN, PARTIALS, TICKETS };           // PARTIALS / TICKETS: a split-K op's scratch and its uint32 per tile
struct Span { SpanBuf buf; SpanRole role; int64_t off, bytes; };

// Calls f(Span) for each; false when a size is not computable (see `product`) or the op is of no known kind / tile.  Operands that
// include/smap_hip.h makes OPTIONAL (res, add1, add2 and aux[0] of a CONV: -1 = absent; segments and the second input by their
// counts) are left out when absent; every other offset is reported as it is, valid or not.
template <class F>
bool for_each_span(const smap_op& o, F&& f)
{
    bool ok = true;
    auto span = [&](SpanBuf buf, SpanRole role, int64_t off, std::initializer_list<int64_t> factors) {
        int64_t bytes;
        if (product(&bytes, factors)) f(Span{buf, role, off, bytes});
        else ok = false;
    };
    const int64_t pl = o.precision == 1 ? 2 : 1;             // planes of an fp16 tensor / weight matrix
    int64_t M;                                                // output pixels
    if (!product(&M, {o.B, o.Ho, o.Wo})) return false;
    auto status = [&] { if (o.status_off > 0) span(OUTPUT, WRITTEN, o.status_off, {SMAP_STATUS_WORDS((int64_t)o.B), 4}); };
    switch (o.kind) {
        case SMAP_OP_CONV: {
            const TileRow* t = tile_find(o.tile);
            int64_t K;                                        // (a second input extends K)
            if (!t || !product(&K, {o.ksize, o.ksize, o.Cin}) || __builtin_add_overflow(K, o.in2_C > 0 ? o.in2_C : 0, &K)) return false;
            const int64_t c8 = o.tail_cout > 0 ? o.tail_cout : cout8(o);      // channels of the dense res / add / low-res tensors
            span(ARENA, READ, o.in_off, {o.B, o.H, o.W, o.in_stride_c, 2});
            if (o.in2_C > 0) span(ARENA, READ, o.in2_off, {o.B, o.in2_H, o.in2_W, o.in2_stride_c, 2});
            span(ARENA, WRITTEN, o.out_off, {M, o.out_stride_c, o.out_fp32 ? 4 : 2});
            for (int64_t off : {o.res_off, o.add1_off, o.add2_off})
                if (off >= 0) span(ARENA, READ, off, {M, c8, 2, pl});
            if (o.aux_off[0] >= 0) span(ARENA, READ, o.aux_off[0], {o.B, o.aux_h[0], o.aux_w[0], c8, 2, pl});
            for (int j = 0; j < 2; ++j)
                if (o.seg_n[j] > 0) span(ARENA, WRITTEN, o.seg_out_off[j], {M, o.seg_out_stride_c[j], 2});
            if (o.ksplit > 1) {
                const int64_t m_tiles = M / t->bm + (M % t->bm != 0), n_tiles = o.cout_pad / t->bn;
                span(ARENA, PARTIALS, o.kpart_off, {m_tiles, n_tiles, o.ksplit, t->bm, t->bn, 4});
                span(ARENA, TICKETS, o.kcount_off, {m_tiles, n_tiles, 4});
            }
            span(WEIGHTS, READ, o.w_off, {o.cout_pad, K, 2, pl});              // packed sizes: include/smap_hip.h
            span(WEIGHTS, READ, o.bias_off, {o.cout_pad, 4});
            if (o.tail_cout > 0) {
                span(WEIGHTS, READ, o.tail_w_off, {o.tail_cout_pad, o.Cout, 2, pl});
                span(WEIGHTS, READ, o.tail_bias_off, {o.tail_cout_pad, 4});
            }
            if (o.head_cin > 0) {
                span(WEIGHTS, READ, o.head_w_off, {o.head_cin, o.Cin, 2, pl});
                span(WEIGHTS, READ, o.head_bias_off, {o.Cin, 4});
                if (o.short_acc_scale > 0.f) span(WEIGHTS, READ, o.short_w_off, {o.tail_cout, o.head_cin, 2, pl});
            }
            if (o.in2_C > 0 && o.in2_mode == 1) span(WEIGHTS, READ, o.in2_bias_off, {o.cout_pad, 4});
            if (o.tap_n > 0) span(WEIGHTS, READ, o.tap_w_off, {o.cout_pad / 32, 2 * 64 * 8 * 2});
            break;
        }
        case SMAP_OP_STEM: case SMAP_OP_STEMPOOL:             // (the images are the caller's pointers, not arena ranges)
            span(ARENA, WRITTEN, o.out_off, {M, 64, 2, pl});
            span(WEIGHTS, READ, o.w_off, {64, SMAP_STEM_K, 2, pl});
            span(WEIGHTS, READ, o.bias_off, {64, 4});
            break;
        case SMAP_OP_MAXPOOL:
            span(ARENA, READ, o.in_off, {o.B, o.H, o.W, o.Cin, 2, pl});
            span(ARENA, WRITTEN, o.out_off, {M, o.Cout, 2, pl});
            break;
        case SMAP_OP_UPADD:                                   // a and out at the output's geometry, t at its own
            span(ARENA, READ, o.in_off, {M, o.Cout, 2});
            span(ARENA, READ, o.aux_off[0], {o.B, o.aux_h[0], o.aux_w[0], o.Cout, 2});
            span(ARENA, WRITTEN, o.out_off, {M, o.Cout, 2});
            break;
        case SMAP_OP_TAPSUM:
            span(ARENA, READ, o.aux_off[0], {M, o.Cin, 4});
            span(WEIGHTS, READ, o.bias_off, {4});
            span(OUTPUT, WRITTEN, o.ext_off, {M, 4});
            status();
            break;
        case SMAP_OP_HEADSUM:
            for (int k = 0; k < o.n_aux && k < 3; ++k)        // with flip_from the sources hold the mirrored half too
                span(ARENA, READ, o.aux_off[k], {o.flip_from > 0 ? 2 : 1, o.B, o.aux_h[k], o.aux_w[k], o.Cin, 4});
            if (o.flip_from > 0) span(WEIGHTS, READ, o.w_off, {o.Cout, 4});
            span(OUTPUT, WRITTEN, o.ext_off, {M, o.Cout, 4});
            status();
            break;
        default:
            return false;
    }
    return ok;
}

// [off, off + bytes) lies inside one window and off its zero page (no sum that could wrap)
inline bool clear_of_zero_pages(int64_t off, int64_t bytes)
{
    const int64_t in_window = off & (SMAP_WINDOW - 1);
    return off >= 0 && in_window >= SMAP_ZERO_PAGE && bytes <= SMAP_WINDOW - in_window;
}

// every (offset, size) pair of a blob is checked as `off <= total - size` with total - size >= 0: no sum that could wrap
inline bool inside(int64_t off, int64_t size, int64_t total) { return off >= 0 && size >= 0 && size <= total && off <= total - size; }

// ---- one op: what the kernels of its kind can compute.  Sums and products of fields are taken in int64 (2LL, `within`): any field may
// hold any value here.
int geometry(const smap_op& o)
{
    if (o.B <= 0 || o.H <= 0 || o.W <= 0 || o.Ho <= 0 || o.Wo <= 0 || o.Cout <= 0) return SMAP_E_ARG;
    if (o.precision != 0 && o.precision != 1) return SMAP_E_ARG;
    if (o.precision == 1 && o.kind == SMAP_OP_UPADD) return SMAP_E_ARG;       // UPADD has no split-precision instance
    const int64_t pl = 1 + o.precision, i31 = ((int64_t)1 << 31) - 1, i32 = (int64_t)1 << 32;
    switch (o.kind) {
        case SMAP_OP_CONV: {
            const TileRow* t = tile_find(o.tile);          // csrc/tiles.h: what the id's kernel is and which instances it has
            if (!t || !tile_has(*t, o.precision == 1)) return SMAP_E_ARG;      // unknown id, or no instance in this precision
            const int bn = t->bn;
            if (o.Cin <= 0 || o.Cin % 64 || o.Cin * 2LL + 16 > SMAP_ZERO_PAGE || o.cout_pad % bn || o.cout_pad < o.Cout) return SMAP_E_ARG;
            if (o.precision == 1) {
                if (o.in_stride_c % 16 || (!o.out_fp32 && o.out_stride_c % 16)) return SMAP_E_ARG;
                if (o.Cin * 2LL + o.in_stride_c + 16 > SMAP_ZERO_PAGE || !(o.acc_scale > 0.f)) return SMAP_E_ARG;
                if ((int64_t)o.in_c_off + o.Cin > o.in_stride_c / 2) return SMAP_E_ARG;
            }
            if ((o.ksize != 1 && o.ksize != 3) || o.stride < 1) return SMAP_E_ARG;
            if (o.w_pairs != 0 && o.w_pairs != 1) return SMAP_E_ARG;
            if (t->family == TF_HALO && (o.ksize != 3 || o.stride != 1 || o.pad != 1 || o.res_off >= 0 || o.add1_off >= 0 ||
                                 o.add2_off >= 0 || o.aux_off[0] >= 0))
                return SMAP_E_ARG;                       // halo-tiled kernel: plain 3x3 stride-1 convs only
            if ((t->tail_bn > 0) != (o.tail_cout > 0)) return SMAP_E_ARG;
            if ((t->family == TF_BLOCK) != (o.head_cin > 0)) return SMAP_E_ARG;
            if (t->family == TF_BLOCK) {                 // whole Bottleneck (convb.hip / convc.hip): `planes` planes, 4 x planes output channels
                const bool first = t->first;             // a layer's FIRST block: `planes` input channels, 1x1 shortcut conv instead of + x
                if (o.ksize != 3 || o.stride != 1 || o.pad != 1 || o.out_fp32 || o.aux_off[0] >= 0) return SMAP_E_ARG;
                const int planes = t->planes;
                if (o.Cin != planes || o.Cout != planes || o.cout_pad != planes || o.head_cin != (first ? planes : 4 * planes) || o.tail_cout != 4 * planes ||
                    o.tail_cout_pad != 4 * planes)
                    return SMAP_E_ARG;
                if (o.in_stride_c != 2 * o.head_cin || o.in_c_off != 0) return SMAP_E_ARG;
                if (first ? (o.res_off >= 0 || o.add1_off >= 0 || o.add2_off >= 0 || !(o.short_acc_scale > 0.f))
                          : (o.res_off != o.in_off || o.short_acc_scale != 0.f))     // identity block: the residual IS the input
                    return SMAP_E_ARG;
                if (!(o.head_acc_scale > 0.f) || !(o.tail_acc_scale > 0.f) || o.out_stride_c < o.tail_cout) return SMAP_E_ARG;
                if (!within(i31, {o.B, o.Ho, o.Wo, o.tail_cout, 2})) return SMAP_E_ARG;
            } else if (o.short_acc_scale != 0.f) return SMAP_E_ARG;      // (a zero-initialised op has no shortcut conv)
            if (t->family == TF_TAIL) {                  // 3x3 + fused 1x1 tail: the op's Cout is the tile's whole N extent
                const int bn2 = t->tail_bn;
                if (o.ksize != 3 || o.stride != 1 || o.pad != 1 || o.out_fp32 || o.aux_off[0] >= 0 || o.Cout != bn || o.cout_pad != bn)
                    return SMAP_E_ARG;
                if (o.tail_cout % 8 || o.tail_cout_pad % bn2 || o.tail_cout_pad < o.tail_cout) return SMAP_E_ARG;
                if (o.precision == 1 && !(o.tail_acc_scale > 0.f)) return SMAP_E_ARG;
                if (o.out_stride_c < o.tail_cout) return SMAP_E_ARG;
                if (!within(i31, {o.B, o.Ho, o.Wo, o.tail_cout, pl})) return SMAP_E_ARG;
            }
            if ((t->caps & TC_REGEPI) && (o.out_fp32 || o.aux_off[0] >= 0 || o.add1_off >= 0 || o.add2_off >= 0 || o.Cout % 8 || o.ksplit > 1))
                return SMAP_E_ARG;                       // register-epilogue tiles of conv.hip: fp16 outputs, residual + ReLU only
            if (t->family == TF_PERSIST && (o.out_fp32 || o.aux_off[0] >= 0 || o.Cout % 8 || o.cout_pad > 2048))
                return SMAP_E_ARG;                       // persistent kernel: register epilogue, fp16 outputs, no fused bilinear add, bias table of 2048 channels in LDS
            if (o.in_stride_c % 8 || o.in_c_off % 8 || o.out_stride_c % 8 || o.out_c_off % 8) return SMAP_E_ARG;
            if (o.out_stride_c < cout8(o) && o.tap_n == 0) return SMAP_E_ARG;      // (tap-dot: `out` is the [M][16] tap tensor)
            if ((o.res_off >= 0 || o.add1_off >= 0 || o.add2_off >= 0 || o.aux_off[0] >= 0) && o.Cout % 8) return SMAP_E_ARG;
            if (o.aux_off[0] >= 0 && (o.aux_h[0] <= 0 || o.aux_w[0] <= 0)) return SMAP_E_ARG;
            // (conv A-operand addresses are 32-bit byte offsets from the input's window base: the input lies inside its window, `validate`)
            if (!within(i32, {o.cout_pad, o.ksize, o.ksize, o.Cin, 2, pl})) return SMAP_E_ARG;
            if (o.ksplit < 0 || o.ksplit > 16) return SMAP_E_ARG;
            if (o.ksplit > 1 && (!(t->caps & TC_SPLITK) || o.ksplit > o.ksize * o.ksize * o.Cin / tile_bk(*t, o.precision == 1)))
                return SMAP_E_ARG;                       // split K: conv.hip's tiles, at most one part per K tile
            if (o.tap_n != 0) {                          // tap-dot epilogue: one N tile of 256 channels, t = fp32 [M][16]
                if (o.tap_n != 9 || !(t->caps & TC_TAPDOT) || o.cout_pad != 256 || o.Cout != 256 || o.ksize != 1 || o.stride != 1 || !o.out_fp32 || o.out_stride_c != 16 ||
                    o.out_c_off != 0 || o.res_off >= 0 || o.add1_off >= 0 || o.add2_off >= 0 || o.aux_off[0] >= 0 || o.seg_n[0] != 0 || o.ksplit > 1 || o.in2_C != 0 ||
                    !(o.tap_scale > 0.f))
                    return SMAP_E_ARG;
            }
            if (o.in2_C < 0) return SMAP_E_ARG;
            if (o.in2_C > 0) {                           // second input along K: 1x1 stride 1 on the first input, plain epilogue
                if (!(t->caps & TC_DUAL) || o.ksize != 1 || o.stride != 1 || o.pad != 0 || o.ksplit > 1 || o.seg_n[0] != 0 || o.aux_off[0] >= 0 ||
                    o.add1_off >= 0 || o.add2_off >= 0 || o.out_fp32 || o.in_c_off != 0)
                    return SMAP_E_ARG;
                if (o.in2_C % 64 || o.in2_stride < 1 || o.in2_stride > 2 || o.in2_H <= 0 || o.in2_W <= 0) return SMAP_E_ARG;
                if (o.Ho != (o.in2_H - 1) / o.in2_stride + 1 || o.Wo != (o.in2_W - 1) / o.in2_stride + 1) return SMAP_E_ARG;
                if (o.in2_stride_c % 8 || o.in2_stride_c < o.in2_C * pl || (o.precision == 1 && o.in2_stride_c % 16)) return SMAP_E_ARG;
                if (o.in2_C * 2LL + (o.precision ? o.in2_stride_c : 0) + 16 > SMAP_ZERO_PAGE) return SMAP_E_ARG;      // padding rows read the zero page (both planes)
                if (window_of(o.in2_off) != window_of(o.in_off)) return SMAP_E_ARG;      // one 64-bit base per launch
                if (!within(i32, {o.cout_pad, (int64_t)o.Cin + o.in2_C, 2, pl})) return SMAP_E_ARG;
                if (o.in2_mode != 0 && o.in2_mode != 1) return SMAP_E_ARG;
                if (o.in2_mode == 1 && (!(t->caps & TC_RELUSUM) || o.in2_stride != 1 || o.res_off >= 0 || o.relu != 0 || (o.precision == 1 && !(o.in2_acc_scale > 0.f))))
                    return SMAP_E_ARG;               // relu(W1 x + b1) + relu(W2 x2 + b2): its own activations, no residual
            } else if (o.in2_mode != 0) return SMAP_E_ARG;
            if (o.seg_n[0] == 0 && o.seg_n[1] != 0) return SMAP_E_ARG;
            if (o.seg_n[0] != 0) {                       // N segments: conv.hip's tiles, 1x1, fp16 outputs; every segment starts on an N tile
                if (t->family != TF_IGEMM || o.ksize != 1 || o.out_fp32 || o.out_c_off != 0) return SMAP_E_ARG;
                int prev = 0;
                for (int j = 0; j < 2 && o.seg_n[j] != 0; ++j) {
                    if (o.seg_n[j] <= prev || o.seg_n[j] % bn || o.seg_n[j] >= o.cout_pad) return SMAP_E_ARG;
                    const int end = (j == 0 && o.seg_n[1] != 0) ? o.seg_n[1] : o.cout_pad;
                    if (o.seg_cout[j] <= 0 || o.seg_cout[j] % 8 || (int64_t)o.seg_n[j] + o.seg_cout[j] > end) return SMAP_E_ARG;
                    if (o.seg_out_stride_c[j] % 8 || (o.precision == 1 && o.seg_out_stride_c[j] % 16)) return SMAP_E_ARG;
                    if (o.seg_out_stride_c[j] < o.seg_cout[j] * pl) return SMAP_E_ARG;
                    if (o.precision == 1 && !(o.seg_acc_scale[j] > 0.f)) return SMAP_E_ARG;
                    if (!within(i31, {o.B, o.Ho, o.Wo, o.seg_out_stride_c[j]})) return SMAP_E_ARG;
                    prev = o.seg_n[j];
                }
                if (cout8(o) > o.seg_n[0]) return SMAP_E_ARG;
            }
            // epilogues address outputs / residuals / addends / the low-res tensor with 32-bit ELEMENT offsets from their bases
            if (!within(i31, {o.B, o.Ho, o.Wo, o.out_stride_c}) || !within(i31, {o.B, o.Ho, o.Wo, cout8(o), pl})) return SMAP_E_ARG;
            if (o.Ho != (o.H + 2LL * o.pad - o.ksize) / o.stride + 1 || o.Wo != (o.W + 2LL * o.pad - o.ksize) / o.stride + 1) return SMAP_E_ARG;
            return 0;
        }
        case SMAP_OP_STEM: case SMAP_OP_STEMPOOL: {
            int64_t h = (o.H + 6LL - 7) / 2 + 1, w = (o.W + 6LL - 7) / 2 + 1;      // the 7x7 s2 p3 conv, then (STEMPOOL) the 3x3 s2 p1 pool
            if (o.kind == SMAP_OP_STEMPOOL) h = (h + 2 - 3) / 2 + 1, w = (w + 2 - 3) / 2 + 1;
            if (o.Cin != 3 || o.Cout != 64 || o.Ho != h || o.Wo != w) return SMAP_E_ARG;
            if (o.flip_from < 0 || (o.flip_from > 0 && o.B != 2LL * o.flip_from)) return SMAP_E_ARG;
            return 0;
        }
        case SMAP_OP_MAXPOOL:
            if (o.Cin % 8 || o.Cin != o.Cout || o.Ho != (o.H + 2LL - 3) / 2 + 1 || o.Wo != (o.W + 2LL - 3) / 2 + 1)
                return SMAP_E_ARG;
            return 0;
        case SMAP_OP_UPADD:
            if (o.Cout % 8 || o.aux_h[0] <= 0 || o.aux_w[0] <= 0) return SMAP_E_ARG;
            return 0;
        case SMAP_OP_TAPSUM:
            if (o.Cout != 1 || o.Cin < 9 || o.Cin % 4 || o.Ho != o.H || o.Wo != o.W) return SMAP_E_ARG;
            if (o.status_off < 0 || o.status_off % 4) return SMAP_E_ARG;
            return 0;
        case SMAP_OP_HEADSUM:
            if (o.n_aux < 1 || o.n_aux > 3 || o.Cout > 48 || o.Cin < o.Cout || o.Cin % 4) return SMAP_E_ARG;      // (float4 loads of the sources)
            for (int k = 0; k < o.n_aux; ++k)
                if (o.aux_h[k] <= 0 || o.aux_w[k] <= 0) return SMAP_E_ARG;
            if (o.flip_from < 0 || (o.flip_from > 0 && (o.in_c_off < 0 || o.in_c_off > o.Cout))) return SMAP_E_ARG;
            if (o.flip_from > 0 && o.flip_from != o.B) return SMAP_E_ARG;      // the mirrored frame of b is b + B: the sources hold 2 B frames
            if (o.status_off < 0 || o.status_off % 4) return SMAP_E_ARG;
            if ((o.scale_hms != 0 && o.scale_hms != 1) || (o.scale_hms && (o.in_c_off < 0 || o.in_c_off > o.Cout))) return SMAP_E_ARG;
            return 0;
        default:
            return SMAP_E_ARG;
    }
}

// ---- one op: its geometry, and the same rule for every range it touches.  ARENA: at or past the first zero page's end, inside one
// window and off that window's zero page (so a conv input is within 32 bits of its window base), split-K partials 16-byte and tickets
// 4-byte aligned.  Output buffer and weight section: a present offset and an end that int64 holds.
int validate(const smap_op& o)
{
    if (int rc = geometry(o)) return rc;
    bool bad = false;
    const bool sized = for_each_span(o, [&](const Span& s) {
        if (s.buf == ARENA)
            bad = bad || !clear_of_zero_pages(s.off, s.bytes) || (s.role == PARTIALS && s.off % 16) || (s.role == TICKETS && s.off % 4);
        else
            bad = bad || s.off < 0 || s.off > INT64_MAX - s.bytes;
    });
    return sized && !bad ? 0 : SMAP_E_ARG;
}

}  // namespace

int plan_check(const smap_op* ops, int n_ops, PlanCheck* out)
{
    if (!ops || !out || n_ops <= 0 || n_ops > 4096) return SMAP_E_ARG;
    for (int i = 0; i < n_ops; ++i)
        if (int rc = validate(ops[i])) return rc;
    *out = PlanCheck();
    out->ops.assign(ops, ops + n_ops);
    out->signalled.assign(n_ops, 0);
    for (int i = 0; i < n_ops; ++i) {                    // lanes: every wait names an EARLIER op of ANOTHER lane
        const smap_op& o = ops[i];
        if (o.lane < 0 || o.lane >= SMAP_MAX_LANES || o.n_wait < 0 || o.n_wait > 4) return SMAP_E_ARG;
        if (o.lane + 1 > out->n_lanes) out->n_lanes = o.lane + 1;
        for (int k = 0; k < o.n_wait; ++k) {
            const int w = o.wait_op[k];
            if (w < 0 || w >= i || ops[w].lane == o.lane) return SMAP_E_ARG;
            out->signalled[w] = 1;
        }
    }
    out->windows.assign(1, 0);
    for (int i = 0; i < n_ops; ++i) {
        const int64_t w = window_of(ops[i].in_off);      // the window each conv launch addresses through
        if (ops[i].kind == SMAP_OP_CONV && std::find(out->windows.begin(), out->windows.end(), w) == out->windows.end()) out->windows.push_back(w);
        for_each_span(ops[i], [&](const Span& s) { if (s.role == TICKETS) out->tickets.push_back({s.off, s.bytes, i}); });
    }
    // Split-K tickets: smap_plan_run zeroes EACH op's own slice (not a span from the lowest to the highest ticket: a foreign blob may put
    // tensors in between), and a slice overlaps no other range of the arena that any op of the schedule touches, another op's slice
    // included -- the tickets live for the whole schedule, whatever the packer reuses around them.
    for (int i = 0; i < n_ops; ++i) {
        bool hit = false;
        for_each_span(ops[i], [&](const Span& s) {
            for (const PlanCheck::Ticket& t : out->tickets)
                hit = hit || (s.buf == ARENA && !(s.role == TICKETS && i == t.op) && s.off < t.off + t.bytes && t.off < s.off + s.bytes);
        });
        if (hit) return SMAP_E_ARG;
    }
    return 0;
}

// arena / output bytes the schedule touches, from the ops alone (a host that did not build the schedule sizes its buffers with it)
void plan_workspace_bytes(const std::vector<smap_op>& ops, int64_t* arena_bytes, int64_t* out_bytes)
{
    int64_t ar = SMAP_ZERO_PAGE, ob = 0;
    for (const smap_op& o : ops)
        for_each_span(o, [&](const Span& s) {
            int64_t& m = s.buf == ARENA ? ar : ob;
            if (s.buf != WEIGHTS && s.off + s.bytes > m) m = s.off + s.bytes;
        });
    if (arena_bytes) *arena_bytes = ar;
    if (out_bytes) *out_bytes = ob;
}

// ---- serialised plans: include/smap_hip.h "plan blob"
int plan_check_blob(const void* blob, size_t blob_bytes, PlanCheck* out, smap_blob_info* info)
{
    if (!blob || !out || blob_bytes < sizeof(smap_blob_header)) return SMAP_E_ARG;
    smap_blob_header h;
    memcpy(&h, blob, sizeof(h));
    if (memcmp(h.magic, "SMAPPLN1", 8) || h.version != SMAP_BLOB_VERSION || h.sizeof_op != sizeof(smap_op) || h.header_bytes != sizeof(smap_blob_header))
        return SMAP_E_ARG;
    const int64_t total = (int64_t)blob_bytes;
    if (h.n_ops <= 0 || h.n_ops > 4096 || h.ops_offset < (int64_t)sizeof(h)) return SMAP_E_ARG;
    if (!inside(h.ops_offset, (int64_t)h.n_ops * (int64_t)sizeof(smap_op), total) || !inside(h.weights_offset, h.weights_bytes, total)) return SMAP_E_ARG;
    std::vector<smap_op> ops(h.n_ops);
    memcpy(ops.data(), static_cast<const char*>(blob) + h.ops_offset, (size_t)h.n_ops * sizeof(smap_op));
    if (int rc = plan_check(ops.data(), h.n_ops, out)) return rc;
    bool held = true;                   // the blob's weight section must hold EVERY byte the ops point at
    for (const smap_op& o : ops)
        for_each_span(o, [&](const Span& s) { held = held && (s.buf != WEIGHTS || inside(s.off, s.bytes, h.weights_bytes)); });
    int64_t ar = 0, ob = 0;
    plan_workspace_bytes(ops, &ar, &ob);
    // the sizes a host allocates from (header AND info) must cover what the ops touch
    if (!held || ar > h.arena_bytes || ob > h.out_bytes || ar > h.info.arena_bytes || ob > h.info.out_bytes ||
        h.info.weights_offset != h.weights_offset || h.info.weights_bytes != h.weights_bytes)
        return SMAP_E_ARG;
    if (info) *info = h.info;
    return 0;
}

extern "C" {

int smap_sizeof_op(void) { return (int)sizeof(smap_op); }

// The three tile lookups of the ABI: rows of csrc/tiles.h.
int smap_conv_tile_dims(int tile, int* bm, int* bn)
{
    const TileRow* t = tile_find(tile);
    if (t) { *bm = t->bm; *bn = t->bn; }
    return t ? 0 : -1;
}
int smap_conv_tile_bk(int tile, int precision) { const TileRow* t = tile_find(tile); return t ? tile_bk(*t, precision != 0) : 0; }
int smap_conv_tile_tail_bn(int tile) { const TileRow* t = tile_find(tile); return t ? t->tail_bn : 0; }

}  // extern "C"
