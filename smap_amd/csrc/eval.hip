// eval.hip -- MPJPE / PCK / ordinal scoring of generate_result runs on gfx950, and the scoring of the network's maps: 2D keypoint
// error / recall and per-bone relative-depth error.
//
// Reference semantics (zju3dv/SMAP): lib/eval/test_util_panoptic.py eval_3d (:273-307), initialization (:332-355); for the maps
// eval_one_image (:88-113) and the `eval` part of generate_rootZ (:145-156).
// Compiled with -ffp-contract=off like assoc.hip: every float64 op below rounds once, in the order written, and
// sqrt(double) is the correctly rounded one group_kernel already relies on -- so the sums are numpy's, bit for bit.
//
// Two parts (include/smap_hip.h):
//   terms  one thread per (frame, person, slot): slots 0..14 = the joint's five addends, slot 15 = the person's five counters.
//          A term row is laid out like the accumulator, so the fold needs no decoding.
//   fold   one thread per accumulator field walks frames and persons IN ORDER: acc[f] += row[f].  The rows of eight persons are
//          requested before the first of the eight additions, so the add chain never waits on a load it just issued.
//          The maps' scorer sums a frame's persons into a zero-initialised vector first and adds that to the running total
//          (:93,110-112 and :121,154-156): the same fold with PARTIAL = true associates the additions that way.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "smap_hip.h"
#include "hip_rc.h"

namespace {

constexpr int NJ = SMAP_NJ, MAXP = SMAP_MAXP, ROOT = 2;
constexpr int NF = SMAP_EVAL_ACC_DOUBLES;            // fields of the accumulator == doubles of a term row
constexpr int SLOTS = 16;                            // threads per person in the terms part
constexpr int F_REAL = 0, F_ROOT = 15, F_POINT = 30, F_REAL_PCK = 45, F_ROOT_PCK = 60;
constexpr int F_PEOPLE = 75, F_PEOPLE_GT = 76, F_PAIRS = 77, F_REVERSED = 78, F_LESS15 = 79;
constexpr int FUSED_NT = 1024, FUSED_MAX_PERSONS = 1024;
constexpr int FOLD_AHEAD = 8;
static_assert(SMAP_EVAL_TERM_DOUBLES == NF && F_LESS15 == NF - 1, "a term row is laid out like the accumulator");

__device__ __forceinline__ int clamp_count(int n, int G) { return n < 0 ? 0 : (n > G ? G : n); }

// np.linalg.norm(np.abs(a - b), axis=1) of one row: sqrt(add.reduce(d * d)) = sqrt((d0*d0 + d1*d1) + d2*d2)
__device__ __forceinline__ double norm3(double d0, double d1, double d2) { return sqrt((d0 * d0 + d1 * d1) + d2 * d2); }

// error_i[j] after `error_i[pred_body[:, 3] == 0] = 0` (:285-286)
__device__ __forceinline__ double real_error(const double* __restrict__ p, const double* __restrict__ q, int j)
{
    if (p[4 * j + 3] == 0.0) return 0.0;
    return norm3(p[4 * j] - q[4 * j], p[4 * j + 1] - q[4 * j + 1], p[4 * j + 2] - q[4 * j + 2]);
}

// One (person, slot) of the terms part.  idx = person * 16 + slot over the B * G person rows.
__device__ __forceinline__ void eval_term(const double* __restrict__ pred_3d, const int* __restrict__ counts,
                                          const double* __restrict__ gt, int G, long long idx, double* terms)
{
    const long long person = idx / SLOTS;
    const int slot = (int)(idx - person * SLOTS);
    const int b = (int)(person / G), g = (int)(person - (long long)b * G);
    const int n = clamp_count(counts[b], G);
    if (g >= n) return;                                        // rows beyond the frame's persons: not read, not written
    const double* p = pred_3d + ((size_t)b * MAXP + g) * NJ * 4;
    const double* q = gt + ((size_t)b * G + g) * NJ * 4;
    double* t = terms + ((size_t)b * G + g) * NF;
    const bool counted = !(q[4 * ROOT + 3] < 2.0);             // :275  (a NaN score is not < 2)
    const bool found = counted && !(p[4 * ROOT + 3] == 0.0);   // :278
    if (slot < NJ) {
        const int j = slot;
        double e = 0.0, r = 0.0, point = 0.0, e_pck = 0.0, r_pck = 0.0;
        if (found && !(p[4 * j + 3] == 0.0)) {
            e = real_error(p, q, j);
            // root_gt_body - root_pred_body, each side minus its own joint 2 first (:281-284,291)
            r = norm3((q[4 * j] - q[4 * ROOT]) - (p[4 * j] - p[4 * ROOT]),
                      (q[4 * j + 1] - q[4 * ROOT + 1]) - (p[4 * j + 1] - p[4 * ROOT + 1]),
                      (q[4 * j + 2] - q[4 * ROOT + 2]) - (p[4 * j + 2] - p[4 * ROOT + 2]));
            point = 1.0;
            e_pck = e < 15.0 ? 1.0 : 0.0;                      // strict; false for NaN
            r_pck = r < 15.0 ? 1.0 : 0.0;
        }
        t[F_REAL + j] = e;
        t[F_ROOT + j] = r;
        t[F_POINT + j] = point;
        t[F_REAL_PCK + j] = e_pck;
        t[F_ROOT_PCK + j] = r_pck;
    } else if (slot == NJ) {
        double pairs = 0.0, reversed = 0.0, less15 = 0.0;
        if (found) {
            less15 = real_error(p, q, 0) < 15.0 ? 1.0 : 0.0;   // :289 after the zeroing: a missing joint 0 counts
            if (g + 1 < n && p[NJ * 4 + 4 * ROOT] != 0.0) {     // :297 the next person's predicted root x
                pairs = 1.0;
                const double dz_gt = q[4 * ROOT + 2] - q[NJ * 4 + 4 * ROOT + 2];
                const double dz_pred = p[4 * ROOT + 2] - p[NJ * 4 + 4 * ROOT + 2];
                reversed = dz_gt * dz_pred < 0.0 ? 1.0 : 0.0;  // :299 strict: a zero product is not reversed
            }
        }
        t[F_PEOPLE] = found ? 1.0 : 0.0;
        t[F_PEOPLE_GT] = counted ? 1.0 : 0.0;
        t[F_PAIRS] = pairs;
        t[F_REVERSED] = reversed;
        t[F_LESS15] = less15;
    }
}

// acc[f] += terms[b][g][f], frames then persons in order; f = this thread's field of the NF a row holds.
// PARTIAL: per frame, partial = 0.0; partial += terms[b][g][f] for its persons in order; then acc[f] += partial.
template <int NF, bool PARTIAL>
__device__ __forceinline__ void eval_fold(const double* terms, const int* __restrict__ counts, int B, int G,
                                          double* __restrict__ acc, int f)
{
    double total = acc[f];
    int n_next = clamp_count(counts[0], G);
    for (int b = 0; b < B; ++b) {
        const int n = n_next;
        if (b + 1 < B) n_next = clamp_count(counts[b + 1], G);   // the next frame's count is on its way while this frame is added
        const double* row = terms + (size_t)b * G * NF + f;
        double a = PARTIAL ? 0.0 : total;
        for (int g0 = 0; g0 < n; g0 += FOLD_AHEAD) {
            double v[FOLD_AHEAD];
#pragma unroll
            for (int k = 0; k < FOLD_AHEAD; ++k) v[k] = g0 + k < n ? row[(size_t)(g0 + k) * NF] : 0.0;
#pragma unroll
            for (int k = 0; k < FOLD_AHEAD; ++k)
                if (g0 + k < n) a = a + v[k];
        }
        total = PARTIAL ? total + a : a;
    }
    acc[f] = total;
}

__global__ __launch_bounds__(128) void eval3d_acc_init_kernel(double* __restrict__ acc)
{
    const int f = threadIdx.x;
    if (f < NF) acc[f] = f == F_PAIRS ? 1e-8 : 0.0;
}

__global__ __launch_bounds__(256) void eval3d_terms_kernel(const double* __restrict__ pred_3d, const int* __restrict__ counts,
                                                           const double* __restrict__ gt, int G, long long total,
                                                           double* __restrict__ terms)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < total) eval_term(pred_3d, counts, gt, G, idx, terms);
}

__global__ __launch_bounds__(128) void eval3d_fold_kernel(const double* __restrict__ terms, const int* __restrict__ counts, int B,
                                                          int G, double* __restrict__ acc)
{
    if (threadIdx.x < NF) eval_fold<NF, false>(terms, counts, B, G, acc, threadIdx.x);
}

// Both parts in ONE workgroup: the term rows go through global memory (B * G * 640 bytes do not fit LDS at G = 64), the
// barrier orders this workgroup's stores before its own loads.
__global__ __launch_bounds__(FUSED_NT) void eval3d_update_kernel(const double* __restrict__ pred_3d, const int* __restrict__ counts,
                                                                 const double* __restrict__ gt, int B, int G,
                                                                 double* terms, double* __restrict__ acc)
{
    const int total = B * G * SLOTS;                            // <= 1024 * 16
    for (int idx = threadIdx.x; idx < total; idx += FUSED_NT) eval_term(pred_3d, counts, gt, G, idx, terms);
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x < NF) eval_fold<NF, false>(terms, counts, B, G, acc, threadIdx.x);
}

// ------------------------------------------------------------------- maps --
// eval_one_image (:99-108) and generate_rootZ's `eval` part (:145-150) of one person, on the rows as smap_register_gt and
// smap_lift_gt_bones left them.  A term row: count_gt[15] | count_pred[15] | distance_e[15] | distance_d[14] | reverse_count[14] |
// count_pred_bone[14], the accumulator's layout.  32 slots per person: 0..14 = joints, 15..28 = limbs.
constexpr int NL = 14, NFM = SMAP_EVALMAPS_ACC_DOUBLES, MSLOTS = 32;
constexpr int M_GT = 0, M_PRED = 15, M_DIST_E = 30, M_DIST_D = 45, M_REVERSE = 59, M_BONE = 73;
static_assert(M_BONE + NL == NFM, "a term row is laid out like the accumulator");
// cfg.DATASET.PAF.VECTOR (src, dst), the table lift_kernel samples the limbs with (assoc.hip c_pairs)
__constant__ int c_limbs[2 * NL] = {0, 1, 0, 2, 0, 9, 9, 10, 10, 11, 0, 3, 3, 4, 4, 5, 2, 12, 12, 13, 13, 14, 2, 6, 6, 7, 7, 8};

// distance() (:28-29) with multiply and sqrt for its ** 2 and ** 0.5
__device__ __forceinline__ double dist2(double ax, double ay, double bx, double by)
{
    const double dx = ax - bx, dy = ay - by;
    return sqrt(dx * dx + dy * dy);
}

__device__ __forceinline__ void maps_term(const double* __restrict__ pred_2d, const double* __restrict__ depth_v,
                                          const int* __restrict__ bone_mask, const int* __restrict__ counts,
                                          const double* __restrict__ gt, int G, long long idx, double* terms)
{
    const long long person = idx / MSLOTS;
    const int slot = (int)(idx - person * MSLOTS);
    const int b = (int)(person / G), g = (int)(person - (long long)b * G);
    const int n = clamp_count(counts[b], G);
    if (g >= n) return;                                        // rows beyond the frame's persons: not read, not written
    const double* p = pred_2d + ((size_t)b * MAXP + g) * NJ * 4;
    const double* q = gt + ((size_t)b * G + g) * NJ * 4;
    double* t = terms + ((size_t)b * G + g) * NFM;
    if (slot < NJ) {
        const int j = slot;
        double c_gt = 0.0, c_pred = 0.0, e = 0.0;
        if (p[4 * ROOT] > 0.0 && p[4 * ROOT + 1] > 0.0 && q[4 * j + 3] > 1.0) {          // :100,103
            const double head = dist2(q[4], q[5], q[0], q[1]) / 3.0;                      // norm_head_size (:60): head = joint 1, neck = joint 0
            const double dis = dist2(q[4 * j], q[4 * j + 1], p[4 * j], p[4 * j + 1]);
            if (dis < head) {                                                             // strict; false for a head size of 0 and for NaN
                e = dis / head;
                c_pred = 1.0;
            }
            c_gt = 1.0;
        }
        t[M_GT + j] = c_gt;
        t[M_PRED + j] = c_pred;
        t[M_DIST_E + j] = e;
    } else if (slot < NJ + NL) {
        const int k = slot - NJ;
        double d = 0.0, rev = 0.0, c = 0.0;
        if ((bone_mask[(size_t)b * MAXP + g] >> k) & 1) {                                 // lift_kernel sampled the limb (:125,130)
            const double real = q[4 * c_limbs[2 * k + 1] + 2] - q[4 * c_limbs[2 * k] + 2];
            const double mean_val = depth_v[((size_t)b * MAXP + g) * NL + k];
            d = fabs(mean_val - real);
            rev = mean_val * real < -1.0 ? 1.0 : 0.0;                                     // strict
            c = 1.0;
        }
        t[M_DIST_D + k] = d;
        t[M_REVERSE + k] = rev;
        t[M_BONE + k] = c;
    }
}

__global__ __launch_bounds__(128) void evalmaps_acc_init_kernel(double* __restrict__ acc)
{
    if (threadIdx.x < NFM) acc[threadIdx.x] = 0.0;
}

__global__ __launch_bounds__(256) void evalmaps_terms_kernel(const double* __restrict__ pred_2d, const double* __restrict__ depth_v,
                                                             const int* __restrict__ bone_mask, const int* __restrict__ counts,
                                                             const double* __restrict__ gt, int G, long long total,
                                                             double* __restrict__ terms)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx < total) maps_term(pred_2d, depth_v, bone_mask, counts, gt, G, idx, terms);
}

__global__ __launch_bounds__(128) void evalmaps_fold_kernel(const double* __restrict__ terms, const int* __restrict__ counts, int B,
                                                            int G, double* __restrict__ acc)
{
    if (threadIdx.x < NFM) eval_fold<NFM, true>(terms, counts, B, G, acc, threadIdx.x);
}

// One workgroup, as eval3d_update_kernel: B * G * 696 bytes of term rows through global memory.
__global__ __launch_bounds__(FUSED_NT) void evalmaps_update_kernel(const double* __restrict__ pred_2d, const double* __restrict__ depth_v,
                                                                   const int* __restrict__ bone_mask, const int* __restrict__ counts,
                                                                   const double* __restrict__ gt, int B, int G, double* terms,
                                                                   double* __restrict__ acc)
{
    const int total = B * G * MSLOTS;                           // <= 1024 * 32
    for (int idx = threadIdx.x; idx < total; idx += FUSED_NT) maps_term(pred_2d, depth_v, bone_mask, counts, gt, G, idx, terms);
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x < NFM) eval_fold<NFM, true>(terms, counts, B, G, acc, threadIdx.x);
}

bool bad_shape(int B, int G) { return B <= 0 || G <= 0 || G > SMAP_EVAL_MAXG || B > (1 << 20); }

}  // namespace

extern "C" {

int smap_eval3d_acc_init(double* acc, void* stream)
{
    if (!acc) return SMAP_E_ARG;
    hipLaunchKernelGGL(eval3d_acc_init_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, acc);
    return hip_rc(hipGetLastError());
}

int smap_eval3d_terms(const double* pred_3d, const int32_t* counts, const double* gt, int B, int G, double* terms, void* stream)
{
    if (!pred_3d || !counts || !gt || !terms || bad_shape(B, G)) return SMAP_E_ARG;
    const long long total = (long long)B * G * SLOTS;
    hipLaunchKernelGGL(eval3d_terms_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred_3d,
                       counts, gt, G, total, terms);
    return hip_rc(hipGetLastError());
}

int smap_eval3d_fold(const double* terms, const int32_t* counts, int B, int G, double* acc, void* stream)
{
    if (!terms || !counts || !acc || bad_shape(B, G)) return SMAP_E_ARG;
    hipLaunchKernelGGL(eval3d_fold_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, terms, counts, B, G, acc);
    return hip_rc(hipGetLastError());
}

int smap_eval3d_update(const double* pred_3d, const int32_t* counts, const double* gt, int B, int G, double* terms, double* acc,
                       void* stream)
{
    if (!pred_3d || !counts || !gt || !terms || !acc || bad_shape(B, G)) return SMAP_E_ARG;
    if ((long long)B * G > FUSED_MAX_PERSONS) {
        const int rc = smap_eval3d_terms(pred_3d, counts, gt, B, G, terms, stream);
        return rc ? rc : smap_eval3d_fold(terms, counts, B, G, acc, stream);
    }
    hipLaunchKernelGGL(eval3d_update_kernel, dim3(1), dim3(FUSED_NT), 0, (hipStream_t)stream, pred_3d, counts, gt, B, G, terms, acc);
    return hip_rc(hipGetLastError());
}

int smap_evalmaps_acc_init(double* acc, void* stream)
{
    if (!acc) return SMAP_E_ARG;
    hipLaunchKernelGGL(evalmaps_acc_init_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, acc);
    return hip_rc(hipGetLastError());
}

int smap_evalmaps_update(const double* pred_2d, const double* depth_v, const int32_t* bone_mask, const int32_t* counts,
                         const double* gt_2d, int B, int G, double* terms, double* acc, void* stream)
{
    if (!pred_2d || !depth_v || !bone_mask || !counts || !gt_2d || !terms || !acc || bad_shape(B, G)) return SMAP_E_ARG;
    if ((long long)B * G > FUSED_MAX_PERSONS) {
        const long long total = (long long)B * G * MSLOTS;
        hipLaunchKernelGGL(evalmaps_terms_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred_2d,
                           depth_v, bone_mask, counts, gt_2d, G, total, terms);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
        hipLaunchKernelGGL(evalmaps_fold_kernel, dim3(1), dim3(128), 0, (hipStream_t)stream, terms, counts, B, G, acc);
        return hip_rc(hipGetLastError());
    }
    hipLaunchKernelGGL(evalmaps_update_kernel, dim3(1), dim3(FUSED_NT), 0, (hipStream_t)stream, pred_2d, depth_v, bone_mask, counts,
                       gt_2d, B, G, terms, acc);
    return hip_rc(hipGetLastError());
}

}  // extern "C"
