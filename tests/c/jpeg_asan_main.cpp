/* jpeg_asan_main.cpp -- the host half of the JPEG decode (smap_amd/csrc/jpeg_host.cpp) alone, for a CPU build under AddressSanitizer /
 * UBSan (tests/test_jpeg_cpu.py builds and runs it; no HIP, no Python in the process).
 *
 *     jpeg_asan_main file.jpg [mutations]
 *
 * Decodes the file, then every truncation of it and `mutations` copies with one to four random bytes replaced (a fixed LCG: the same
 * run every time).  Every input lives in a heap block of exactly its size and every coefficient buffer is exactly info.coef_bytes,
 * so a read or write past either is reported.  Prints "<rc of the file> <ok> <unsupported> <error>" over all variants; exit 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "smap_hip.h"

static int run(const uint8_t* src, size_t n) {
    uint8_t* d = (uint8_t*)malloc(n ? n : 1);
    memcpy(d, src, n);
    smap_jpeg_info info;
    int rc = smap_jpeg_probe(d, n, &info);
    if (rc == 0) {
        int16_t* co = (int16_t*)malloc((size_t)info.coef_bytes);
        rc = smap_jpeg_decode_coefficients(d, n, &info, co);
        free(co);
    }
    free(d);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    size_t n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t* buf = (uint8_t*)malloc(n);
    if (fread(buf, 1, n, f) != n) return 2;
    fclose(f);
    long muts = argc > 2 ? atol(argv[2]) : 0;
    int first = run(buf, n);
    long counts[3] = {0, 0, 0};
    for (size_t k = 0; k < n; ++k) {
        int rc = run(buf, k);
        ++counts[rc == 0 ? 0 : rc == SMAP_JPEG_UNSUPPORTED ? 1 : 2];
    }
    uint8_t* m = (uint8_t*)malloc(n);
    uint64_t s = 0x9E3779B97F4A7C15ull;
    for (long i = 0; i < muts; ++i) {
        memcpy(m, buf, n);
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        int nb = 1 + (int)((s >> 60) & 3);
        for (int j = 0; j < nb; ++j) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            m[(s >> 33) % n] = (uint8_t)(s >> 13);
        }
        int rc = run(m, n);
        ++counts[rc == 0 ? 0 : rc == SMAP_JPEG_UNSUPPORTED ? 1 : 2];
    }
    printf("%d %ld %ld %ld\n", first, counts[0], counts[1], counts[2]);
    free(m);
    free(buf);
    return 0;
}
