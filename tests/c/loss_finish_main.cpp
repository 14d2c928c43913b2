/* loss_finish_main.cpp -- the finish of the training loss (smap_amd/csrc/loss_core.h) alone, for a CPU build under AddressSanitizer /
 * UBSan (tests/test_loss_cpu.py builds and runs it; no HIP, no Python in the process).
 *
 *     loss_finish_main scene.bin [nan]
 *
 * scene.bin: int32 [9] = stage_num, ohkm, topk, ctf, single, B, R, H, W; then sums f64 [n_heads * B * 57], valids f32 [B * 57],
 * rdepth f32 [B * R * 3], rd_at f32 [n_heads * B * R].  With `nan` every sum is replaced by NaN first.  Every buffer lives in a heap
 * block of exactly its size, so an access past an end is reported.  Prints "result <i> <value>" (8 lines), then "coef", "sel", "m"
 * (n_heads * B * 57 lines each) and "cell", "fac" (n_heads * B * R lines each), values as %.17g; exit 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "loss_core.h"

template <class T>
static T* take(FILE* f, size_t n)
{
    T* p = (T*)malloc(n * sizeof(T));
    if (!p || fread(p, sizeof(T), n, f) != n) {
        fprintf(stderr, "short file\n");
        exit(2);
    }
    return p;
}

int main(int argc, char** argv)
{
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t* hdr = take<int32_t>(f, 9);
    loss_core::Params p{};
    p.stage_num = hdr[0];
    p.ohkm = hdr[1];
    p.topk = hdr[2];
    p.ctf = hdr[3];
    p.single = hdr[4];
    p.B = hdr[5];
    p.R = hdr[6];
    p.H = hdr[7];
    p.W = hdr[8];
    p.S = 8;
    p.n_heads = p.single ? 1 : 4 * p.stage_num;
    p.has_hm = p.has_dd = p.has_rd = 1;
    free(hdr);
    if (loss_core::check_params(p)) {
        printf("rejected\n");
        return 0;
    }
    const size_t n = (size_t)p.n_heads * p.B * loss_core::NC, rows = (size_t)p.n_heads * p.B * p.R;
    double* sums = take<double>(f, n);
    float* valids = take<float>(f, (size_t)p.B * loss_core::NC);
    float* rdepth = take<float>(f, (size_t)p.B * p.R * 3);
    float* rd_at = take<float>(f, rows);
    fclose(f);
    if (argc > 2 && !strcmp(argv[2], "nan"))
        for (size_t i = 0; i < n; ++i) sums[i] = strtod("nan", nullptr);
    double* m = (double*)malloc(n * sizeof(double));
    double* sel = (double*)malloc(n * sizeof(double));
    double* coef = (double*)malloc(n * sizeof(double));
    int32_t* cell = (int32_t*)malloc(rows * sizeof(int32_t));
    double* fac = (double*)malloc(rows * sizeof(double));
    double* headloss = (double*)malloc(loss_core::MAX_HEADS * loss_core::HEADLOSS * sizeof(double));
    double* part = (double*)malloc((size_t)p.n_heads * p.B * loss_core::PART * sizeof(double));
    double* result = (double*)malloc(8 * sizeof(double));
    if (!m || !sel || !coef || !cell || !fac || !headloss || !part || !result) return 2;
    loss_core::finish_serial<double>(p, sums, valids, rdepth, rd_at, m, sel, coef, cell, fac, part, headloss, result);
    for (int i = 0; i < 8; ++i) printf("result %d %.17g\n", i, result[i]);
    for (size_t i = 0; i < n; ++i) printf("coef %.17g\n", coef[i]);
    for (size_t i = 0; i < n; ++i) printf("sel %.17g\n", sel[i]);
    for (size_t i = 0; i < n; ++i) printf("m %.17g\n", m[i]);
    for (size_t i = 0; i < rows; ++i) printf("cell %d\n", (int)cell[i]);
    for (size_t i = 0; i < rows; ++i) printf("fac %.17g\n", fac[i]);
    free(sums);
    free(valids);
    free(rdepth);
    free(rd_at);
    free(m);
    free(sel);
    free(coef);
    free(cell);
    free(fac);
    free(headloss);
    free(part);
    free(result);
    return 0;
}
