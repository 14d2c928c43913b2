// loss_core.h -- the "finish" of the training loss (SMAP._calculate_loss, model/smap.py:355-401; lib/utils/loss_h.py) as plain C++ that
// compiles for the host and for the device alike (the csrc/jpeg_huff.h pattern): csrc/loss.hip runs it in one workgroup behind the
// reduction, smap_loss_finish_host and tests/c/loss_finish_main.cpp run it on the CPU.  Everything here is double arithmetic on the
// per-channel sums of squares the reduction wrote; no HIP header, no allocation.
//
// The work is cut into per-item functions with no dependency inside a phase, so that the device runs a phase with one item per thread
// and a barrier after it, and the host runs the same items in a plain loop -- the same operations in the same order either way:
//   root_row_cell   item (head, frame, row): the map cell of a root-depth row (on the device the reduction's launch does this, where it
//                   reads root_d at that cell)
//   channel_mean    item (head, frame, channel): m = sum / (H * W) * (valid > 0)
//   channel_select  item (head, frame, channel): the 0 / 1 selection (top-k of the channel's group, ties to the LOWER channel index) and
//                   coef, the factor g with d total / d out = g * (out - label)
//   frame_partials  item (head, frame): the sums of the kept m of every group in channel order, the frame's root-depth rows in order
//   head_losses     item head: the frames' partial sums added in frame order, the means, the root-depth loss
//   root_factor     item (head, frame, row): the signed factor of the backward pass's root table
//   totals          once: the weighted sum over the heads, the three logging terms, bad_rows
// Channels are in OUTPUT order throughout: 0..42 the 2D head (15 key points, 28 PAF x / y), 43..56 the relative-depth head.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LOSS_HD __host__ __device__
#else
#define LOSS_HD
#endif
#if defined(__clang__)
#define LOSS_UNROLL _Pragma("unroll")          // constant trip counts: the loads of a loop go out together
#define LOSS_UNROLL4 _Pragma("unroll 4")
#define LOSS_UNROLL8 _Pragma("unroll 8")
#else
#define LOSS_UNROLL
#define LOSS_UNROLL4
#define LOSS_UNROLL8
#endif

namespace loss_core {

constexpr int NKP = 15, NPAF = 28, N2D = 43, NDD = 14, NC = 57, MAX_HEADS = 16, GRAD_C = 58;

struct Params {
    int n_heads, stage_num, ohkm, topk, ctf, single;
    int B, S, R, H, W;
    int has_hm, has_dd, has_rd;          // single-head mode only: which of the three tensors was given (all three otherwise)
};

// ---- what a head is ------------------------------------------------------------------------------------------------------------
LOSS_HD inline bool head_fine(const Params& p, int h) { return p.single || (h & 3) == 3; }                  // j == 3 (:378,390)
LOSS_HD inline int head_scale(const Params& p, int h)                                                      // :367-369
{
    if (p.single) return 0;
    return (h & 3) + ((h >> 2) == p.stage_num - 1 && p.ctf ? 1 : 0);
}
LOSS_HD inline double head_factor(const Params& p, int h) { return head_fine(p, h) ? 1.0 : 0.25; }        // :396-397
LOSS_HD inline double weight_2d(const Params& p) { return p.single ? 1.0 : 0.1; }                         // :395
LOSS_HD inline double weight_3d(const Params& p) { return p.single ? 1.0 : 5.0; }
LOSS_HD inline double weight_root(const Params& p) { return p.single ? 1.0 : 10.0; }
// label channel an output channel is compared with (:371-376)
LOSS_HD inline int label_channel(int c)
{
    if (c < NKP) return c;
    if (c < N2D) return NKP + 3 * ((c - NKP) / 2) + (c - NKP) % 2;
    return NKP + 3 * (c - N2D) + 2;
}
// the group of channels a top-k (or the plain mean) runs over, and how many of it are kept
struct Group { int first, n, keep; };
LOSS_HD inline Group channel_group(const Params& p, int h, int c)
{
    const bool hard = p.ohkm && head_fine(p, h);
    if (c >= N2D) return Group{N2D, NDD, hard ? p.topk : NDD};
    if (!hard) return Group{0, N2D, N2D};
    return c < NKP ? Group{0, NKP, p.topk} : Group{NKP, NPAF, 2 * p.topk};
}
// the map cell of a root-depth row (y, x, Z), or -1: int() truncates toward zero, so (-1, 0) still lands on 0 (loss_h.py:22)
LOSS_HD inline int root_cell_of(const float* row, int H, int W)
{
    const float y = row[0], x = row[1];
    if (!(y > -1.0f && y < (float)H && x > -1.0f && x < (float)W)) return -1;
    return (int)y * W + (int)x;
}
// what the root table holds of a row: its cell; ROW_SKIPPED where Z <= 0 (not a row at all); ROW_OUTSIDE where it counts but lies off the map
constexpr int ROW_SKIPPED = -1, ROW_OUTSIDE = -2;
LOSS_HD inline int root_row_cell(const Params& p, const float* row)
{
    if (!p.has_rd || !(row[2] > 0.0f)) return ROW_SKIPPED;
    const int cell = root_cell_of(row, p.H, p.W);
    return cell < 0 ? ROW_OUTSIDE : cell;
}

// ---- the workspace of smap_loss_forward / smap_loss_backward (smap_amd/loss.py workspace_layout mirrors it) -----------------------
struct Workspace {
    int64_t sums, m, part, headloss, coef, sel, rd_at, root_fac, root_cell, bytes;
};
LOSS_HD inline Workspace workspace_layout(int n_heads, int B, int R)
{
    const int64_t n = (int64_t)n_heads * B * NC, rows = (int64_t)n_heads * B * R;
    Workspace w;
    w.sums = 0;                                  // f64 [n_heads][B][57]
    w.m = w.sums + n * 8;                        // f64 [n_heads][B][57]
    w.part = w.m + n * 8;                        // f64 [n_heads][B][6]: the frames' partial sums (frame_partials)
    w.headloss = w.part + (int64_t)n_heads * B * 6 * 8;      // f64 [MAX_HEADS][5]: 2D, depth, root, bad rows, counted rows
    w.coef = w.headloss + MAX_HEADS * 5 * 8;     // f32 [n_heads][B][57]
    w.sel = w.coef + n * 4;                      // f32 [n_heads][B][57]
    w.rd_at = w.sel + n * 4;                     // f32 [n_heads][B][R]: root_d at the rows' cells
    w.root_fac = w.rd_at + rows * 4;             // f32 [n_heads][B][R]
    w.root_cell = w.root_fac + rows * 4;         // i32 [n_heads][B][R]
    w.bytes = (w.root_cell + rows * 4 + 7) / 8 * 8;
    return w;
}

// ---- argument rules shared by every entry point (0 or -1 = SMAP_E_ARG) -----------------------------------------------------------
inline int check_params(const Params& p)
{
    if (p.stage_num < 1 || p.stage_num > 4) return -1;
    if (p.single ? (p.stage_num != 1 || p.ctf) : false) return -1;
    if (p.n_heads != (p.single ? 1 : 4 * p.stage_num)) return -1;
    if (p.S < (p.single ? 1 : 4 + (p.ctf ? 1 : 0))) return -1;
    if (p.ohkm && (p.topk < 1 || p.topk > NDD)) return -1;
    if (p.H < 1 || p.W < 1 || (int64_t)p.H * p.W > (1 << 24)) return -1;
    if (p.B < 1 || p.B > 65535 || p.R < 1 || p.R > 65535) return -1;
    return 0;
}

// ---- phase 1: per (head, frame, channel) ---------------------------------------------------------------------------------------
LOSS_HD inline void channel_mean(const Params& p, int64_t item, const double* sums, const float* valids, double* m)
{
    const int it = (int)item, c = it % NC, b = it / NC % p.B;         // n_heads * B * 57 < 2^31
    if (c < N2D ? !p.has_hm : !p.has_dd) {
        m[item] = 0.0;
        return;
    }
    const double w = valids[(int64_t)b * NC + c] > 0.0f ? 1.0 : 0.0;                   // torch.gt(valid, 0).float() (loss_h.py:45)
    m[item] = sums[item] / ((double)p.H * (double)p.W) * w;                             // .mean(dim=[2, 3]) * weight (:44,46)
}

// ---- phase 2: per (head, frame, channel) ---------------------------------------------------------------------------------------
// how many of row[0..N) come before row[me] in "larger value first, lower index first"
template <int N>
LOSS_HD inline int rank_before(const double* row, int me)
{
    const double v = row[me];
    int rank = 0;
    LOSS_UNROLL
    for (int k = 0; k < N; ++k) rank += (row[k] > v || (row[k] == v && k < me)) ? 1 : 0;
    return rank;
}

template <class T>
LOSS_HD inline void channel_select(const Params& p, int64_t item, const double* m, const float* valids, T* sel, T* coef)
{
    const int it = (int)item, c = it % NC, b = it / NC % p.B, h = it / NC / p.B;
    if (c < N2D ? !p.has_hm : !p.has_dd) {
        sel[item] = (T)0;
        coef[item] = (T)0;
        return;
    }
    const Group g = channel_group(p, h, c);
    int keep = 1;
    if (g.keep < g.n) {
        // rank = how many channels of the group come before c in "descending value, ascending index"; NaN compares false both ways
        const double* row = m + (item - c) + g.first;
        const int me = c - g.first;
        const int rank = g.n == NKP ? rank_before<NKP>(row, me) : (g.n == NPAF ? rank_before<NPAF>(row, me) : rank_before<NDD>(row, me));
        keep = rank < g.keep ? 1 : 0;
    }
    sel[item] = (T)keep;
    const double w = valids[(int64_t)b * NC + c] > 0.0f ? 1.0 : 0.0;
    const double part = c < N2D ? weight_2d(p) : weight_3d(p);
    const double mean = (double)p.B * (double)g.keep;                                   // .mean() of the kept [B, keep] values
    coef[item] = (T)(head_factor(p, h) * part * 2.0 / ((double)p.H * (double)p.W * mean) * w * (double)keep);
}

// ---- phase 3: per (head, frame) -------------------------------------------------------------------------------------------------
// part [n_heads][B][PART]: the frame's sums of the kept m of the key-point | 2D, the PAF and the depth group, each in channel order;
// then of its root-depth rows, in order: sum |root_d - Z|, rows counted, rows outside the map.
constexpr int PART = 6;

template <int N, class T>
LOSS_HD inline double kept_sum(const double* m, const T* sel)
{
    double s = 0.0;
    LOSS_UNROLL8
    for (int k = 0; k < N; ++k) s += sel[k] != (T)0 ? m[k] : 0.0;
    return s;
}

template <class T>
LOSS_HD inline void frame_partials(const Params& p, int64_t item, const double* m, const T* sel, const float* rdepth, const float* rd_at,
                                   const int32_t* root_cell, double* part)
{
    const int b = (int)item % p.B, h = (int)item / p.B;
    const bool hard = p.ohkm && head_fine(p, h);
    const double* mf = m + item * NC;
    const T* sf = sel + item * NC;
    double* out = part + item * PART;
    out[0] = hard ? kept_sum<NKP>(mf, sf) : kept_sum<N2D>(mf, sf);
    out[1] = hard ? kept_sum<NPAF>(mf + NKP, sf + NKP) : 0.0;
    out[2] = kept_sum<NDD>(mf + N2D, sf + N2D);
    // DepthLoss (loss_h.py:14-28): the rows with Z > 0, in order; every load is unconditional
    double loss = 0.0;
    int count = 0, bad = 0;
    const float* z = rdepth + (int64_t)b * p.R * 3 + 2;
    LOSS_UNROLL4
    for (int r = 0; r < p.R; ++r) {
        const int cell = root_cell[item * p.R + r];
        const double d = fabs((double)rd_at[item * p.R + r] - (double)z[3 * r]);
        count += cell != ROW_SKIPPED ? 1 : 0;
        bad += cell == ROW_OUTSIDE ? 1 : 0;
        loss += cell >= 0 ? d : 0.0;
    }
    out[3] = loss;
    out[4] = (double)count;
    out[5] = (double)bad;
}

// ---- phase 4: per head ---------------------------------------------------------------------------------------------------------
// headloss [MAX_HEADS][HEADLOSS]: 2D, depth, root, rows outside the map, rows counted
constexpr int HEADLOSS = 5;

LOSS_HD inline void head_losses(const Params& p, int h, const double* part, double* headloss)
{
    const bool hard = p.ohkm && head_fine(p, h);
    double s[PART] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < p.B; ++b)                          // the frames in order
        for (int k = 0; k < PART; ++k) s[k] += part[((int64_t)h * p.B + b) * PART + k];
    double l2d = 0.0, l3d = 0.0;
    if (p.has_hm) l2d = hard ? s[0] / ((double)p.B * p.topk) + s[1] / ((double)p.B * 2 * p.topk) : s[0] / ((double)p.B * N2D);
    if (p.has_dd) l3d = s[2] / ((double)p.B * (hard ? p.topk : NDD));
    headloss[h * HEADLOSS + 0] = l2d;
    headloss[h * HEADLOSS + 1] = l3d;
    headloss[h * HEADLOSS + 2] = s[4] > 0.0 ? s[3] / s[4] : 0.0;
    headloss[h * HEADLOSS + 3] = s[5];
    headloss[h * HEADLOSS + 4] = s[4];
}

// ---- phase 5: per (head, frame, row): the root table's factor ------------------------------------------------------------------
template <class T>
LOSS_HD inline void root_factor(const Params& p, int64_t item, const float* rdepth, const float* rd_at, const int32_t* root_cell,
                                const double* headloss, T* root_fac)
{
    const int64_t rows = (int64_t)p.B * p.R;
    const int h = (int)(item / rows);
    const double count = headloss[h * HEADLOSS + 4];
    double f = 0.0;
    if (root_cell[item] >= 0 && count > 0.0) {
        const double d = (double)rd_at[item] - (double)rdepth[(item % rows) * 3 + 2];
        const double scale = weight_root(p) * head_factor(p, h) / count;
        f = d > 0.0 ? scale : (d < 0.0 ? -scale : 0.0);    // torch.abs's gradient: sign(0) = 0
    }
    root_fac[item] = (T)f;
}

// ---- phase 6: once -------------------------------------------------------------------------------------------------------------
// result[8]: total, 2D, bone, root, bad_rows, 0, 0, 0
template <class T>
LOSS_HD inline void totals(const Params& p, const double* headloss, T* result)
{
    double total = 0.0, l2d = 0.0, l3d = 0.0, lroot = 0.0;
    for (int h = 0; h < p.n_heads; ++h) {
        const double* hl = headloss + h * HEADLOSS;
        double t = weight_2d(p) * hl[0] + weight_3d(p) * hl[1] + weight_root(p) * hl[2];
        if (head_fine(p, h)) {
            l2d += hl[0];
            l3d += hl[1];
            lroot += hl[2];
        } else {
            t = t / 4.0;
        }
        total += t;
    }
    const double bad = headloss[3];                      // the same rows for every head
    if (bad > 0.0) total = (double)NAN;                  // a row outside the map: the reference wraps or raises
    result[0] = (T)total;
    result[1] = (T)l2d;
    result[2] = (T)l3d;
    result[3] = (T)lroot;
    result[4] = (T)bad;
    result[5] = result[6] = result[7] = (T)0;
}

// ---- the whole finish, serially (the host's driver) --------------------------------------------------------------------------------
template <class T>
inline void finish_serial(const Params& p, const double* sums, const float* valids, const float* rdepth, const float* rd_at, double* m,
                          T* sel, T* coef, int32_t* root_cell, T* root_fac, double* part, double* headloss, T* result)
{
    const int64_t frames = (int64_t)p.n_heads * p.B, n = frames * NC;
    for (int64_t i = 0; i < frames * p.R; ++i) root_cell[i] = root_row_cell(p, rdepth + (i % ((int64_t)p.B * p.R)) * 3);    // on the device: the reduction's launch
    for (int64_t i = 0; i < n; ++i) channel_mean(p, i, sums, valids, m);
    for (int64_t i = 0; i < n; ++i) channel_select(p, i, m, valids, sel, coef);
    for (int64_t i = 0; i < frames; ++i) frame_partials(p, i, m, sel, rdepth, rd_at, root_cell, part);
    for (int h = 0; h < p.n_heads; ++h) head_losses(p, h, part, headloss);
    for (int64_t i = 0; i < frames * p.R; ++i) root_factor(p, i, rdepth, rd_at, root_cell, headloss, root_fac);
    totals(p, headloss, result);
}

}  // namespace loss_core
