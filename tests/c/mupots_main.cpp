/* mupots_main.cpp -- the host twin of smap_amd/csrc/mupots.hip: the per-element functions of smap_amd/csrc/mupots_core.h in plain serial
 * loops, for a CPU build under AddressSanitizer / UBSan (tests/test_mupots_cpu.py builds and runs it; no HIP, no Python in the process).
 *
 *     mupots_main scene.bin rows.bin
 *
 * scene.bin: int32 [8] = F, G, S, sumP, relative, use_skel, matched_only, 0; then gt2d f64 [F*G*15*2], gt3d f64 [F*G*15*3],
 * occ f64 [F*G*15], gt_count i32 [F], seq_offset i32 [S+1], pred_offset i32 [F+1], pred2d f64 [sumP*15*2], pred3d f64 [sumP*15*4].
 * rows.bin (written): match i32 [F*G], considered i32 [F*G], err f64 [F*G*15], rootz f64 [F*G*2], acc f64 [S*590]; rows beyond a frame's
 * persons are zero.  Every buffer lives in a heap block of exactly its size, so an access past an end is reported.  exit 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mupots_core.h"

using namespace mupots_core;

template <class T>
static T* take(FILE* f, size_t n)
{
    T* p = (T*)malloc(n ? n * sizeof(T) : 1);
    if (!p || fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return p;
}

template <class T>
static T* zeros(size_t n)
{
    T* p = (T*)calloc(n ? n : 1, sizeof(T));
    if (!p) exit(2);
    return p;
}

int main(int argc, char** argv)
{
    if (argc < 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t* hdr = take<int32_t>(f, 8);
    const int F = hdr[0], G = hdr[1], S = hdr[2], sumP = hdr[3], relative = hdr[4], use_skel = hdr[5], matched_only = hdr[6];
    if (F < 1 || G < 1 || G > MAXG || S < 1 || sumP < 0) return 2;
    const size_t FG = (size_t)F * G;
    double* gt2d = take<double>(f, FG * NJ * 2);
    double* gt3d = take<double>(f, FG * NJ * 3);
    double* occ = take<double>(f, FG * NJ);
    int32_t* gt_count = take<int32_t>(f, F);
    int32_t* seq_offset = take<int32_t>(f, (size_t)S + 1);
    int32_t* pred_offset = take<int32_t>(f, (size_t)F + 1);
    double* pred2d = take<double>(f, (size_t)sumP * NJ * 2);
    double* pred3d = take<double>(f, (size_t)sumP * NJ * 4);
    fclose(f);

    int32_t* match = zeros<int32_t>(FG);
    int32_t* considered = zeros<int32_t>(FG);
    double* err = zeros<double>(FG * NJ);
    double* rootz = zeros<double>(FG * 2);
    double* acc = zeros<double>((size_t)S * ACC);

    for (int fr = 0; fr < F; ++fr) {                            /* the frames part: what one wavefront does */
        const int n = clamp_count(gt_count[fr], G);
        const long long p0 = pred_offset[fr], p1 = pred_offset[fr + 1];
        int P = 0;
        if (p0 >= 0 && p1 >= p0 && p1 <= sumP) P = (int)(p1 - p0 > MAXP ? MAXP : p1 - p0);
        const size_t row = (size_t)fr * G;
        bool used[MAXP] = {};
        for (int k = 0; k < n; ++k) {
            int key = -1;
            for (int i = 0; i < P; ++i) {
                if (used[i]) continue;
                const int ki = match_key(match_score(gt2d + (row + k) * NJ * 2, pred2d + (size_t)(p0 + i) * NJ * 2), i);
                key = ki > key ? ki : key;
            }
            const int m = key_index(key);
            if (m >= 0) used[m] = true;
            match[row + k] = m;
        }
        for (int g = 0; g < n; ++g) {
            const int m = match[row + g];
            const double* g3 = gt3d + (row + g) * NJ * 3;
            const double* p3 = m >= 0 ? pred3d + (size_t)(p0 + m) * NJ * 4 : nullptr;
            for (int j = 0; j < NJ; ++j) err[(row + g) * NJ + j] = joint_error(p3, g3, relative, use_skel, j);
            considered[row + g] = is_considered(m >= 0, matched_only);
            rootz[2 * (row + g)] = final_at(p3, g3, relative, use_skel, ROOT, 2);
            rootz[2 * (row + g) + 1] = gt_at(g3, relative, ROOT, 2);
        }
    }
    for (int s = 0; s < S; ++s) {                               /* the fold: what one thread per field does */
        int f0 = seq_offset[s], f1 = seq_offset[s + 1];
        f0 = f0 < 0 ? 0 : (f0 > F ? F : f0);
        f1 = f1 < f0 ? f0 : (f1 > F ? F : f1);
        for (int field = 0; field < ACC; ++field)
            acc[(size_t)s * ACC + field] = fold_field(field, f0, f1, gt_count, G, match, considered, err, rootz, occ, relative);
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    bool ok = fwrite(match, sizeof(int32_t), FG, o) == FG && fwrite(considered, sizeof(int32_t), FG, o) == FG &&
              fwrite(err, sizeof(double), FG * NJ, o) == FG * NJ && fwrite(rootz, sizeof(double), FG * 2, o) == FG * 2 &&
              fwrite(acc, sizeof(double), (size_t)S * ACC, o) == (size_t)S * ACC;
    ok = fclose(o) == 0 && ok;
    free(hdr); free(gt2d); free(gt3d); free(occ); free(gt_count); free(seq_offset); free(pred_offset); free(pred2d); free(pred3d);
    free(match); free(considered); free(err); free(rootz); free(acc);
    return ok ? 0 : 2;
}
