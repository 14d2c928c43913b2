// mupots_core.h -- the per-element arithmetic of the MuPoTS-3D protocol (zju3dv/SMAP lib/eval/mupots_smap.m and its helpers under
// lib/eval/util_smap/) as plain C++ that compiles for the host and for the device alike (the csrc/loss_core.h pattern): csrc/mupots.hip
// runs it with one wavefront per frame and one thread per accumulator field, tests/c/mupots_main.cpp runs the same expressions in
// serial loops on the CPU.  Everything is float64, one rounding per operation in the order written (-ffp-contract=off), with the
// correctly rounded sqrt.  No HIP header, no allocation, no array that is indexed at run time: the two skeleton tables are 4-bit
// fields of 64-bit literals, so they live in registers / immediates on the device and cost no scratch.
//
// Joints are 0-based here, in the protocol's (MPI) order: 0 head top, 1 neck, 2-4 right arm, 5-7 left arm, 8-10 right leg,
// 11-13 left leg, 14 pelvis.  The .m files count from 1; the comments cite them as they are written there.
//
// Layouts (all dense, row-major):
//   gt2d  [F][G][15][2]   annot2(:, 1:15)' of the frame's VALID persons in annotation order (mupots_smap.m:53,102-104)
//   gt3d  [F][G][15][3]   univ_annot3(:, 1:15)'                                             (:55,105)
//   occ   [F][G][15]      occlusion_labels{i,k}(1:15)                                       (:60,107)
//   pred2d [sumP][15][2], pred3d [sumP][15][4]: the predictions of all frames one after the other, in SMAP joint order (the order of
//          pose2d.mat / pose3d.mat); frame f owns rows pred_offset[f] .. pred_offset[f + 1] - 1.  Column 3 of pred3d is not read (:124-125).
// Rows (what the frames part leaves per (frame, valid person)): match [F][G] = index of the matched prediction inside the frame or -1,
// considered [F][G], err [F][G][15], rootz [F][G][2] = (pred_p(3,15), P(3,15)).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MUPOTS_HD __host__ __device__
#else
#define MUPOTS_HD
#endif

namespace mupots_core {

constexpr int NJ = 15, ROOT = 14, MAXG = 16, MAXP = 127, NT = 31;
constexpr double MATCH_THRESHOLD = 40.0, PCK_THRESHOLD = 150.0, ORDINAL_THRESHOLD = 300.0, UNMATCHED = 100000.0, NAN_ERROR = 160.0;

// ---- the per-sequence accumulator (include/smap_hip.h SMAP_MUPOTS_ACC_DOUBLES) --------------------------------------------------
constexpr int F_CONSIDERED = 0, F_ANNOTATED = 1, F_UNDETECTED = 2, F_ORD_CORRECT = 3, F_ORD_TOTAL = 4;
constexpr int F_JOINT = 5, JOINT_W = 2 + NT;              // per joint: error sum | NT counts of err < 5 * t | count of err <= 150
constexpr int F_MASK = F_JOINT + NJ * JOINT_W;            // per mask (0 visible, 1 occluded), per joint: mask sum | masked error sum | count > 150
constexpr int MASK_W = 3, ACC = F_MASK + 2 * NJ * MASK_W;
static_assert(F_MASK == 500 && ACC == 590, "the layout include/smap_hip.h documents");

// o1 of mupots_smap.m:15-17 (mpii_get_joints 'relevant', first 15, o1(2) = 15), 0-based, 4 bits per joint; the pelvis is its own parent
// here so that a walk towards the root stops there.
constexpr uint64_t pack15(int a0, int a1, int a2, int a3, int a4, int a5, int a6, int a7, int a8, int a9, int a10, int a11, int a12, int a13,
                          int a14)
{
    return (uint64_t)a0 | (uint64_t)a1 << 4 | (uint64_t)a2 << 8 | (uint64_t)a3 << 12 | (uint64_t)a4 << 16 | (uint64_t)a5 << 20 |
           (uint64_t)a6 << 24 | (uint64_t)a7 << 28 | (uint64_t)a8 << 32 | (uint64_t)a9 << 36 | (uint64_t)a10 << 40 | (uint64_t)a11 << 44 |
           (uint64_t)a12 << 48 | (uint64_t)a13 << 52 | (uint64_t)a14 << 56;
}
constexpr uint64_t PARENTS = pack15(1, 14, 1, 2, 3, 1, 5, 6, 14, 8, 9, 14, 11, 12, 14);
MUPOTS_HD inline int parent(int j) { return (int)((PARENTS >> (4 * j)) & 15); }
// the re-ordering of mupots_smap.m:122-123, 0-based: protocol joint j is SMAP joint smap_joint(j)
constexpr uint64_t SMAP_JOINT = pack15(1, 0, 9, 10, 11, 3, 4, 5, 12, 13, 14, 6, 7, 8, 2);
MUPOTS_HD inline int smap_joint(int j) { return (int)((SMAP_JOINT >> (4 * j)) & 15); }

// ---- matching: mpii_multiperson_get_identity_matching.m:12-15 for one (ground-truth person, prediction) pair ---------------------
// g2 = gt2d of the person [15][2], p2 = pred2d of the prediction [15][2] (SMAP order).  Joints 2..14 of the .m (matching_joints,
// mupots_smap.m:98): both differences strictly below the threshold, and the prediction's joint not at exactly (0, 0) (:143).
MUPOTS_HD inline int match_score(const double* g2, const double* p2)
{
    int score = 0;
    for (int j = 1; j <= 13; ++j) {
        const int s = smap_joint(j);
        const double px = p2[2 * s], py = p2[2 * s + 1];
        const bool near = fabs(g2[2 * j] - px) < MATCH_THRESHOLD && fabs(g2[2 * j + 1] - py) < MATCH_THRESHOLD;   // false for NaN
        const bool visible = !(px == 0.0 && py == 0.0);
        score += near && visible ? 1 : 0;
    }
    return score;
}
// The key the arg-max runs on: the larger score wins, then the LOWER prediction index (MATLAB's max returns the first maximum,
// :17).  key < KEY_MIN_MATCH: nothing matched (score 0, :18).  i <= 126.
constexpr int KEY_MIN_MATCH = 128;
MUPOTS_HD inline int match_key(int score, int i) { return score * 128 + (127 - i); }
MUPOTS_HD inline int key_index(int key) { return key >= KEY_MIN_MATCH ? 127 - (key & 127) : -1; }

// ---- poses ---------------------------------------------------------------------------------------------------------------------
// pred_pose_3d{k}(c, j) (mupots_smap.m:146,153-157) and P(c, j) (:172-176): minus the pelvis in relative mode
MUPOTS_HD inline double pred_at(const double* p3, int relative, int j, int c)
{
    const double v = p3[4 * smap_joint(j) + c];
    return relative ? v - p3[4 * smap_joint(ROOT) + c] : v;
}
MUPOTS_HD inline double gt_at(const double* g3, int relative, int j, int c)
{
    const double v = g3[3 * j + c];
    return relative ? v - g3[3 * ROOT + c] : v;
}
// norm() of a 3-vector as this project defines it: sqrt((x*x + y*y) + z*z).  MATLAB does not specify its own.
MUPOTS_HD inline double norm3(double x, double y, double z) { return sqrt((x * x + y * y) + z * z); }

// mpii_map_to_gt_bone_lengths.m:6-8 for joint j, coordinate c: the bone of the UNMAPPED prediction scaled to the ground truth's length,
// (v * gt_len) / norm(v).  A zero bone gives 0 / 0 = NaN.
MUPOTS_HD inline double scaled_bone(const double* p3, const double* g3, int relative, int j, int c)
{
    const int pa = parent(j);
    const double gt_len = norm3(gt_at(g3, relative, j, 0) - gt_at(g3, relative, pa, 0), gt_at(g3, relative, j, 1) - gt_at(g3, relative, pa, 1),
                                gt_at(g3, relative, j, 2) - gt_at(g3, relative, pa, 2));
    const double vx = pred_at(p3, relative, j, 0) - pred_at(p3, relative, pa, 0);
    const double vy = pred_at(p3, relative, j, 1) - pred_at(p3, relative, pa, 1);
    const double vz = pred_at(p3, relative, j, 2) - pred_at(p3, relative, pa, 2);
    const double v = c == 0 ? vx : (c == 1 ? vy : vz);
    return (v * gt_len) / norm3(vx, vy, vz);
}
// mapped_pose(c, j) of mpii_map_to_gt_bone_lengths.m:9: mapped(parent) + scaled bone, along the chain from the pelvis (which the
// traversal [2,1,3,...,14] of mupots_smap.m:29,183 never moves).  The chain is at most four bones long (wrist - elbow - shoulder -
// neck); each of its bones depends on the unmapped prediction only, so a joint is computed on its own: the additions are the
// traversal's, in its order.
MUPOTS_HD inline double mapped_at(const double* p3, const double* g3, int relative, int use_skel, int j, int c)
{
    if (!use_skel || j == ROOT) return pred_at(p3, relative, j, c);
    const int a0 = j, a1 = parent(a0), a2 = parent(a1), a3 = parent(a2);
    double m = pred_at(p3, relative, ROOT, c);
    if (a3 != ROOT) m = m + scaled_bone(p3, g3, relative, a3, c);
    if (a2 != ROOT) m = m + scaled_bone(p3, g3, relative, a2, c);
    if (a1 != ROOT) m = m + scaled_bone(p3, g3, relative, a1, c);
    return m + scaled_bone(p3, g3, relative, a0, c);
}
// pred_p(c, j) of mupots_smap.m:180-188: the matched prediction (p3 != null), or 100000 everywhere
MUPOTS_HD inline double final_at(const double* p3, const double* g3, int relative, int use_skel, int j, int c)
{
    return p3 ? mapped_at(p3, g3, relative, use_skel, j, c) : UNMATCHED;
}
// error_p(j) of mupots_smap.m:199-200
MUPOTS_HD inline double joint_error(const double* p3, const double* g3, int relative, int use_skel, int j)
{
    const double dx = final_at(p3, g3, relative, use_skel, j, 0) - gt_at(g3, relative, j, 0);
    const double dy = final_at(p3, g3, relative, use_skel, j, 1) - gt_at(g3, relative, j, 1);
    const double dz = final_at(p3, g3, relative, use_skel, j, 2) - gt_at(g3, relative, j, 2);
    return sqrt(((dx * dx) + (dy * dy)) + (dz * dz));
}
// pred_considered of mupots_smap.m:178-192
MUPOTS_HD inline int is_considered(int matched, int matched_only) { return matched || !matched_only ? 1 : 0; }

// cal_ordinal.m:52-60 (threshold 300) -> the `ordi >= 0` of mupots_smap.m:215
MUPOTS_HD inline int ordinal_correct(double pd1, double pd2, double gt1, double gt2)
{
    if ((gt1 - gt2) * (pd1 - pd2) > 0.0) return 1;
    return fabs(gt1 - gt2) < ORDINAL_THRESHOLD && fabs(pd1 - pd2) < ORDINAL_THRESHOLD ? 1 : 0;
}

// ---- the fold: one accumulator field of one sequence, its frames f0 .. f1 - 1 then their persons IN ORDER ------------------------
MUPOTS_HD inline int clamp_count(int n, int G) { return n < 0 ? 0 : (n > G ? G : n); }

MUPOTS_HD inline double fold_field(int field, int f0, int f1, const int32_t* gt_count, int G, const int32_t* match,
                                   const int32_t* considered, const double* err, const double* rootz, const double* occ, int relative)
{
    double total = 0.0;
    int j = 0, k = 0, mask = 0;
    if (field >= F_MASK) {
        mask = (field - F_MASK) / (NJ * MASK_W);
        j = ((field - F_MASK) % (NJ * MASK_W)) / MASK_W;
        k = (field - F_MASK) % MASK_W;
    } else if (field >= F_JOINT) {
        j = (field - F_JOINT) / JOINT_W;
        k = (field - F_JOINT) % JOINT_W;
    }
    for (int f = f0; f < f1; ++f) {
        const int n = clamp_count(gt_count[f], G);
        const size_t row = (size_t)f * G;
        if (field == F_ANNOTATED) {                                   // mupots_smap.m:86
            total = total + (double)n;
            continue;
        }
        if (field == F_ORD_CORRECT || field == F_ORD_TOTAL) {         // :210-221, absolute mode only (:195-198)
            if (relative) continue;
            for (int a = 0; a + 1 < n; ++a) {
                if (!considered[row + a]) continue;
                for (int b = a + 1; b < n; ++b) {
                    if (!considered[row + b]) continue;
                    const int ok = ordinal_correct(rootz[2 * (row + b)], rootz[2 * (row + a)], rootz[2 * (row + b) + 1], rootz[2 * (row + a) + 1]);
                    total = total + (field == F_ORD_TOTAL ? 1.0 : (double)ok);
                }
            }
            continue;
        }
        for (int g = 0; g < n; ++g) {
            if (field == F_UNDETECTED) {                              // :167
                total = total + (match[row + g] < 0 ? 1.0 : 0.0);
                continue;
            }
            if (!considered[row + g]) continue;                       // :194
            if (field == F_CONSIDERED) {
                total = total + 1.0;
                continue;
            }
            const double e = err[(row + g) * NJ + j];
            if (field < F_MASK) {
                if (k == 0) total = total + e;                                                   // the sum behind mean(..., 3), mpii_evaluate_multiperson_errors.m:27
                else if (k <= NT) total = total + (e < 5.0 * (double)(k - 1) ? 1.0 : 0.0);       // mpii_compute_3d_pck.m:20,30 (false for NaN)
                else total = total + (e <= PCK_THRESHOLD ? 1.0 : 0.0);                           // mupots_smap.m:250
            } else {
                // mpii_evaluate_multiperson_errors_visibility_mask.m:13-16: NaN -> 160, then times the mask (mupots_smap.m:107-108,202-203)
                const double o = occ[(row + g) * NJ + j];
                const double m = mask ? o : 1.0 - o;
                const double me = (e != e ? NAN_ERROR : e) * m;
                if (k == 0) total = total + m;
                else if (k == 1) total = total + me;
                else total = total + (me > PCK_THRESHOLD ? 1.0 : 0.0);
            }
        }
    }
    return total;
}

}  // namespace mupots_core
