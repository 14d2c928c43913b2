// Stand-alone driver of csrc/cubic_table.cpp for the sanitizer build (tests/test_augment_cpu.py): the table is written into a heap
// block of EXACTLY 1024 * 16 int16, so a write past either end is an AddressSanitizer report; prints every entry's sum and a checksum.
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "smap_hip.h"

int main()
{
    if (smap_cubic_table(nullptr) != SMAP_E_ARG) {
        printf("null accepted\n");
        return 1;
    }
    std::vector<int16_t> tab(1024 * 16);
    if (smap_cubic_table(tab.data()) != 0) return 1;
    uint64_t digest = 1469598103934665603ull;            // FNV-1a over the int16 values
    int bad = 0;
    for (int e = 0; e < 1024; ++e) {
        int sum = 0;
        for (int k = 0; k < 16; ++k) {
            sum += tab[e * 16 + k];
            digest = (digest ^ (uint16_t)tab[e * 16 + k]) * 1099511628211ull;
        }
        bad += sum != 32768;
    }
    printf("entries with a wrong sum: %d\n", bad);
    printf("digest %llu\n", (unsigned long long)digest);
    return bad != 0;
}
