/* jpeg_huff_twin_main.cpp -- the CPU twin of smap_jpeg_decode_coefficients_device (smap_amd/csrc/jpeg_huff.hip): the same phases over
 * the same per-subsequence functions (smap_amd/csrc/jpeg_huff.h, included here as plain host C++), with loops in place of lanes and
 * workgroups.  For a CPU build under AddressSanitizer / UBSan (tests/test_jpeg_huff_cpu.py builds and runs it; no HIP, no Python).
 *
 *     jpeg_huff_twin [--lanes=L] [--subseq=S] [--rounds=R] file.jpg [mutations] [more files ...]
 *
 * L: subsequences per group (default 256, the kernels'); S: bytes per subsequence (0 = the shipped default); R: cross-group rounds
 * (0 = the shipped default, -1 = the number of groups, which is provably enough).  One line per file:
 *     "<status> <equal> <host rc> <rounds that changed a state> <groups> <file>"
 * equal = 1 when the coefficients are smap_jpeg_decode_coefficients'.  With a mutation count after the first file: every truncation of
 * it and that many copies with one to four random bytes of the entropy-coded data replaced (a fixed LCG), then one line
 *     "<variants> <status 0> <violations>"
 * where a violation is a variant with status 0 whose coefficients are not the host decoder's (or that the host decoder refuses).
 * Every input and every array lives in a heap block of exactly its size, so a read or write past one is reported.  Exit 0. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../smap_amd/csrc/jpeg_huff.h"

using namespace smap_huff;

struct Run {
    int status, equal, host_rc, rounds_used, groups;
};

template <class T>
static T* alloc(size_t count) { return (T*)malloc((count ? count : 1) * sizeof(T)); }

// inclusive sums inside each chunk, exclusive sums of the chunk totals (the kernels' scan_chunks + scan_totals)
static void scan(int32_t* x, int32_t* tot, int32_t count) {
    uint32_t run = 0;
    for (int32_t c = 0; c * kChunk < count; ++c) {
        uint32_t s = 0;
        for (int32_t i = c * kChunk; i < count && i < (c + 1) * kChunk; ++i) x[i] = int32_t(s += uint32_t(x[i]));
        tot[c] = int32_t(run);
        run += s;
    }
}

static Run run(const uint8_t* file, size_t n, int L, int S, int rounds) {
    Run out = {-1, 0, 0, 0, 0};
    uint8_t* d = alloc<uint8_t>(n);
    memcpy(d, file, n);
    smap_jpeg_info info;
    smap_jpeg_scan* scan_tab = alloc<smap_jpeg_scan>(1);
    Geo g;
    out.host_rc = smap_jpeg_probe(d, n, &info);
    if (out.host_rc == 0) out.host_rc = smap_jpeg_scan_tables(d, n, &info, scan_tab);
    if (out.host_rc != 0 || !geo_init(&g, info, n, S)) {
        free(scan_tab);
        free(d);
        return out;                                                 // the markers already refuse it: nothing for the device
    }
    int16_t* want = alloc<int16_t>(size_t(info.coef_bytes / 2));
    out.host_rc = smap_jpeg_decode_coefficients(d, n, &info, want);
    const int nsub = g.nsub, ngroups = (nsub + L - 1) / L;
    out.groups = ngroups;
    if (rounds == 0) rounds = SMAP_JPEG_ROUNDS;
    if (rounds < 0 || rounds > ngroups) rounds = ngroups;
    uint64_t* entry = alloc<uint64_t>(size_t(nsub));
    uint64_t* exit_ = alloc<uint64_t>(size_t(nsub));
    uint64_t* wantst = alloc<uint64_t>(size_t(L));
    uint64_t* gexit = alloc<uint64_t>(size_t(2 * ngroups));
    const int nchunk = (nsub + kChunk - 1) / kChunk, dchunk = (g.total + kChunk - 1) / kChunk;
    int32_t* nblk = alloc<int32_t>(size_t(nsub));
    int32_t* ntot = alloc<int32_t>(size_t(nchunk));
    int32_t* dcd = alloc<int32_t>(size_t(g.total));
    int32_t* dctot = alloc<int32_t>(size_t(dchunk));
    int16_t* co = alloc<int16_t>(size_t(info.coef_bytes / 2));
    const Src src = {d, nullptr, uint32_t(n), 0, 0};
    const smap_jpeg_huff* tab = scan_tab->table;
    const Out none = {nullptr, nullptr};

    auto decode = [&](int i) {
        const Result r = decode_subseq<false>(src, tab, g, i, entry[i], 0, none);
        exit_[i] = r.exit;
        nblk[i] = r.nblk;
    };
    // a group's sweeps: every lane whose left neighbour's exit is not its entry takes it and decodes again, until none changes
    auto sweeps = [&](int grp) {
        const int first = grp * L, cnt = nsub - first < L ? nsub - first : L;
        for (int sweep = 0; sweep <= cnt; ++sweep) {
            bool any = false;
            for (int t = 0; t < cnt; ++t) wantst[t] = t ? exit_[first + t - 1] : entry[first];
            for (int t = 0; t < cnt; ++t)
                if (wantst[t] != entry[first + t]) {
                    entry[first + t] = wantst[t];
                    decode(first + t);
                    any = true;
                }
            if (!any) break;
        }
    };
    for (int grp = 0; grp < ngroups; ++grp) {                       // speculate, synchronise inside the group
        for (int i = grp * L; i < nsub && i < (grp + 1) * L; ++i) {
            entry[i] = fresh_state(src, g, i);
            decode(i);
        }
        sweeps(grp);
        const int last = (grp + 1) * L < nsub ? (grp + 1) * L - 1 : nsub - 1;
        gexit[grp] = exit_[last];
    }
    for (int r = 1; r <= rounds; ++r) {                             // synchronise across groups: r further passes
        const uint64_t* prev = gexit + ((r - 1) & 1) * ngroups;
        uint64_t* cur = gexit + (r & 1) * ngroups;
        if (out.rounds_used < r - 1) break;                         // a round that changed nothing: every later one is the same no-op
        for (int grp = 0; grp < ngroups; ++grp) {
            cur[grp] = prev[grp];
            if (grp == 0 || prev[grp - 1] == entry[grp * L]) continue;
            entry[grp * L] = prev[grp - 1];
            decode(grp * L);
            sweeps(grp);
            const int last = (grp + 1) * L < nsub ? (grp + 1) * L - 1 : nsub - 1;
            cur[grp] = exit_[last];
            out.rounds_used = r;
        }
    }
    scan(nblk, ntot, nsub);                                         // count: each subsequence's first block number
    memset(co, 0, size_t(info.coef_bytes));
    memset(dcd, 0, size_t(g.total) * 4);
    int status = 0;
    const Out o = {co, dcd};
    for (int i = 0; i < nsub; ++i) {                                // the exact pass, and the proof that the chain closes
        const int32_t n0 = sum_upto(nblk, ntot, i - 1);
        const Result r = decode_subseq<true>(src, tab, g, i, entry[i], n0, o);
        status |= r.flags;
        if (n0 + r.nblk != sum_upto(nblk, ntot, i)) status |= kNotConv;
        if (i + 1 < nsub) {
            if (r.exit != entry[i + 1]) status |= kNotConv;
        } else if (r.exit != kEnd) {
            status |= kEData;
        }
    }
    scan(dcd, dctot, g.total);                                      // DC: sums, then predictors per restart interval
    for (int32_t e = 0; e < g.total; ++e) dc_store(g, dcd, dctot, e, co);
    out.status = status;
    out.equal = out.host_rc == 0 && memcmp(co, want, size_t(info.coef_bytes)) == 0;
    free(co); free(dctot); free(dcd); free(ntot); free(nblk); free(gexit); free(wantst); free(exit_); free(entry); free(want);
    free(scan_tab);
    free(d);
    return out;
}

int main(int argc, char** argv) {
    int L = kLanes, S = 0, rounds = 0, a = 1;
    for (; a < argc && argv[a][0] == '-' && argv[a][1] == '-'; ++a) {
        if (!strncmp(argv[a], "--lanes=", 8)) L = atoi(argv[a] + 8);
        else if (!strncmp(argv[a], "--subseq=", 9)) S = atoi(argv[a] + 9);
        else if (!strncmp(argv[a], "--rounds=", 9)) rounds = atoi(argv[a] + 9);
        else return 2;
    }
    if (a >= argc || L < 1) return 2;
    bool first = true;
    for (; a < argc; ++a, first = false) {
        FILE* f = fopen(argv[a], "rb");
        if (!f) return 2;
        fseek(f, 0, SEEK_END);
        const size_t n = (size_t)ftell(f);
        fseek(f, 0, SEEK_SET);
        uint8_t* buf = alloc<uint8_t>(n);
        if (fread(buf, 1, n, f) != n) return 2;
        fclose(f);
        const Run r = run(buf, n, L, S, rounds);
        printf("%d %d %d %d %d %s\n", r.status, r.equal, r.host_rc, r.rounds_used, r.groups, argv[a]);
        char* endp = nullptr;
        const long muts = (first && a + 1 < argc) ? strtol(argv[a + 1], &endp, 10) : 0;
        if (first && a + 1 < argc && endp && *endp == 0 && endp != argv[a + 1]) {
            ++a;
            long variants = 0, ok = 0, violations = 0;
            auto tally = [&](const Run& v) {
                ++variants;
                if (v.status == 0) {
                    ++ok;
                    if (!v.equal) ++violations;
                }
            };
            for (size_t k = 0; k < n; ++k) tally(run(buf, k, L, S, rounds));
            smap_jpeg_info info;
            const size_t s0 = smap_jpeg_probe(buf, n, &info) == 0 ? size_t(info.scan_offset) : 0;
            uint8_t* m = alloc<uint8_t>(n);
            uint64_t s = 0x9E3779B97F4A7C15ull;
            for (long i = 0; i < muts && s0 < n; ++i) {
                memcpy(m, buf, n);
                s = s * 6364136223846793005ull + 1442695040888963407ull;
                const int nb = 1 + (int)((s >> 60) & 3);
                for (int j = 0; j < nb; ++j) {
                    s = s * 6364136223846793005ull + 1442695040888963407ull;
                    m[s0 + (s >> 33) % (n - s0)] = (uint8_t)(s >> 13);
                }
                tally(run(m, n, L, S, rounds));
            }
            printf("%ld %ld %ld\n", variants, ok, violations);
            free(m);
        }
        free(buf);
    }
    return 0;
}
