// mupots.hip -- the MuPoTS-3D protocol (3DPCK, AUC, MPJPE, ordinal rate of root depths) on gfx950.
//
// Reference semantics (zju3dv/SMAP): lib/eval/mupots_smap.m with lib/eval/util_smap/.  The arithmetic of one element -- a matching
// score, a mapped joint, an error, an ordinal test, one accumulator field -- is csrc/mupots_core.h, which the host compiles too.
// Compiled with -ffp-contract=off like eval.hip: every float64 operation rounds once, in the order written.
//
// Two launches (include/smap_hip.h):
//   frames  one wavefront per frame.  Matching: the ground-truth persons are taken in order (the protocol is greedy, so this loop is
//           serial); lane l scores predictions l and l + 64 against the person, the arg-max over the wavefront is a butterfly of
//           __shfl_xor on one integer key (score first, then the LOWER index), and the lane that owns the winner marks it in a
//           register -- no array of flags, no scratch.  The winners go through 16 ints of LDS; then lane = (person, joint) for the
//           bone mapping and the error.  A joint's chain to the pelvis is at most four bones, each a function of the unmapped
//           prediction, so a lane recomputes its chain rather than wait for its parent's lane.
//   fold    one thread per (sequence, accumulator field) walks that sequence's rows, frames then persons in order.  No atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "smap_hip.h"
#include "hip_rc.h"
#include "mupots_core.h"

namespace {

using namespace mupots_core;
static_assert(MAXG == SMAP_MUPOTS_MAXG && MAXP == SMAP_MUPOTS_MAXP && ACC == SMAP_MUPOTS_ACC_DOUBLES, "include/smap_hip.h");
static_assert(MAXP <= 128, "two predictions per lane");
constexpr int WAVE = 64;

__global__ __launch_bounds__(WAVE) void mupots_frames_kernel(const double* __restrict__ gt2d, const double* __restrict__ gt3d,
                                                             const int32_t* __restrict__ gt_count, const double* __restrict__ pred2d,
                                                             const double* __restrict__ pred3d, const int32_t* __restrict__ pred_offset,
                                                             int G, int sumP, int relative, int use_skel, int matched_only,
                                                             int32_t* __restrict__ match, int32_t* __restrict__ considered,
                                                             double* __restrict__ err, double* __restrict__ rootz)
{
    __shared__ int s_match[MAXG];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int n = clamp_count(gt_count[f], G);                 // wave-uniform
    const long long p0 = pred_offset[f], p1 = pred_offset[f + 1];
    int P = 0;
    if (p0 >= 0 && p1 >= p0 && p1 <= sumP) P = (int)(p1 - p0 > MAXP ? MAXP : p1 - p0);
    const size_t row = (size_t)f * G;

    bool used0 = false, used1 = false;                         // this lane's predictions lane and lane + 64: matched already
    for (int k = 0; k < n; ++k) {
        const double* g2 = gt2d + (row + k) * NJ * 2;
        int key = -1;
        if (lane < P && !used0) key = match_key(match_score(g2, pred2d + (size_t)(p0 + lane) * NJ * 2), lane);
        if (lane + WAVE < P && !used1) {
            const int key1 = match_key(match_score(g2, pred2d + (size_t)(p0 + lane + WAVE) * NJ * 2), lane + WAVE);
            key = key1 > key ? key1 : key;
        }
#pragma unroll
        for (int off = WAVE / 2; off >= 1; off >>= 1) {
            const int other = __shfl_xor(key, off, WAVE);
            key = other > key ? other : key;
        }
        const int m = key_index(key);                          // the same in every lane
        if (m == lane) used0 = true;
        if (m == lane + WAVE) used1 = true;
        if (lane == 0) s_match[k] = m;
    }
    __syncthreads();

    for (int idx = lane; idx < n * NJ; idx += WAVE) {
        const int g = idx / NJ, j = idx - g * NJ;
        const int m = s_match[g];
        const double* g3 = gt3d + (row + g) * NJ * 3;
        const double* p3 = m >= 0 ? pred3d + (size_t)(p0 + m) * NJ * 4 : nullptr;
        err[(row + g) * NJ + j] = joint_error(p3, g3, relative, use_skel, j);
        if (j == ROOT) {
            match[row + g] = m;
            considered[row + g] = is_considered(m >= 0, matched_only);
            rootz[2 * (row + g)] = final_at(p3, g3, relative, use_skel, ROOT, 2);     // pred_p(3,15), mupots_smap.m:196
            rootz[2 * (row + g) + 1] = gt_at(g3, relative, ROOT, 2);                   // P(3,15), :197
        }
    }
}

__global__ __launch_bounds__(WAVE) void mupots_fold_kernel(const int32_t* __restrict__ seq_offset, const int32_t* __restrict__ gt_count,
                                                           int F, int G, const int32_t* __restrict__ match,
                                                           const int32_t* __restrict__ considered, const double* __restrict__ err,
                                                           const double* __restrict__ rootz, const double* __restrict__ occ,
                                                           int relative, double* __restrict__ acc)
{
    const int field = blockIdx.x * WAVE + threadIdx.x, s = blockIdx.y;
    if (field >= ACC) return;
    int f0 = seq_offset[s], f1 = seq_offset[s + 1];
    f0 = f0 < 0 ? 0 : (f0 > F ? F : f0);
    f1 = f1 < f0 ? f0 : (f1 > F ? F : f1);
    acc[(size_t)s * ACC + field] = fold_field(field, f0, f1, gt_count, G, match, considered, err, rootz, occ, relative);
}

bool bad_shape(int F, int G) { return F <= 0 || G <= 0 || G > MAXG || F > (1 << 20); }

}  // namespace

extern "C" {

int smap_mupots_frames(const double* gt2d, const double* gt3d, const int32_t* gt_count, const double* pred2d, const double* pred3d,
                       const int32_t* pred_offset, int F, int G, int sumP, int relative, int use_skel, int matched_only, int32_t* match,
                       int32_t* considered, double* err, double* rootz, void* stream)
{
    if (!gt2d || !gt3d || !gt_count || !pred2d || !pred3d || !pred_offset || !match || !considered || !err || !rootz || bad_shape(F, G) ||
        sumP < 0)
        return SMAP_E_ARG;
    hipLaunchKernelGGL(mupots_frames_kernel, dim3((unsigned)F), dim3(WAVE), 0, (hipStream_t)stream, gt2d, gt3d, gt_count, pred2d, pred3d,
                       pred_offset, G, sumP, relative != 0, use_skel != 0, matched_only != 0, match, considered, err, rootz);
    return hip_rc(hipGetLastError());
}

int smap_mupots_fold(const int32_t* seq_offset, int S, const int32_t* gt_count, int F, int G, const int32_t* match,
                     const int32_t* considered, const double* err, const double* rootz, const double* occ, int relative, double* acc,
                     void* stream)
{
    if (!seq_offset || !gt_count || !match || !considered || !err || !rootz || !occ || !acc || bad_shape(F, G) || S <= 0 || S > 65535)
        return SMAP_E_ARG;
    hipLaunchKernelGGL(mupots_fold_kernel, dim3((ACC + WAVE - 1) / WAVE, (unsigned)S), dim3(WAVE), 0, (hipStream_t)stream, seq_offset,
                       gt_count, F, G, match, considered, err, rootz, occ, relative != 0, acc);
    return hip_rc(hipGetLastError());
}

}  // extern "C"
