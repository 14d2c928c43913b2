/* plan_check_main.cpp -- the host-side guard of the schedule executor (smap_amd/csrc/plan_check.cpp) alone, for a CPU build under
 * AddressSanitizer / UBSan (tests/test_abi_cpu.py builds and runs it; no HIP, no Python in the process).
 *
 *     plan_check_main plan.blob
 *
 * Runs the checker on the blob, on every truncation of its header and ops section, and on the blob with every int32 / int64 / float
 * field of every op overwritten in turn with -1, 0, 1, INT32_MAX, INT32_MIN (64-bit fields: also INT64_MAX and 2^32 - 8); an accepted
 * schedule is also sized.  The blob and every truncation live in a heap block of exactly their size, so a read past the end is
 * reported.  Prints "accepted" / "rejected" per case (first line: the blob itself) and the totals; exit 0. */
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "plan_check.h"

struct Field { size_t off; int count; char type; };       /* 'i' int32, 'l' int64, 'f' float */
#define F(type, name) {offsetof(smap_op, name), (int)(sizeof(((smap_op*)0)->name) / ((type) == 'l' ? 8 : 4)), type}
static const Field FIELDS[] = {
    F('i', kind), F('i', B), F('i', H), F('i', W), F('i', Cin), F('i', in_stride_c), F('i', in_c_off), F('i', Ho), F('i', Wo), F('i', Cout),
    F('i', ksize), F('i', stride), F('i', pad), F('i', relu), F('i', cout_pad), F('i', out_stride_c), F('i', out_c_off), F('i', out_fp32),
    F('i', tile), F('i', n_aux), F('l', in_off), F('l', out_off), F('l', w_off), F('l', bias_off), F('l', res_off), F('l', add1_off),
    F('l', add2_off), F('l', aux_off), F('i', aux_h), F('i', aux_w), F('l', ext_off), F('i', precision), F('f', acc_scale), F('i', flip_from),
    F('i', w_pairs), F('i', status_off), F('i', tail_cout), F('i', tail_cout_pad), F('f', tail_acc_scale), F('l', tail_w_off),
    F('l', tail_bias_off), F('i', head_cin), F('f', head_acc_scale), F('l', head_w_off), F('l', head_bias_off), F('l', short_w_off),
    F('f', short_acc_scale), F('i', scale_hms), F('i', seg_n), F('i', seg_cout), F('i', seg_relu), F('i', seg_out_stride_c),
    F('f', seg_acc_scale), F('l', seg_out_off), F('i', ksplit), F('i', reserved1), F('l', kpart_off), F('l', kcount_off), F('i', lane),
    F('i', n_wait), F('i', wait_op), F('l', in2_off), F('i', in2_H), F('i', in2_W), F('i', in2_C), F('i', in2_stride_c), F('i', in2_stride),
    F('i', in2_mode), F('f', in2_acc_scale), F('l', in2_bias_off), F('i', tap_n), F('f', tap_scale), F('l', tap_w_off),
};
static const int N_FIELDS = (int)(sizeof(FIELDS) / sizeof(FIELDS[0]));

static long counts[2];

static int run(const void* blob, size_t n, const char* what) {
    PlanCheck c;
    smap_blob_info info;
    const int rc = plan_check_blob(blob, n, &c, &info);
    if (rc == 0) {
        int64_t ar = 0, ob = 0;
        plan_workspace_bytes(c.ops, &ar, &ob);
        if (ar > info.arena_bytes || ob > info.out_bytes) { printf("%s: sizes beyond the header's\n", what); exit(3); }
    }
    ++counts[rc != 0];
    printf("%s %s\n", what, rc == 0 ? "accepted" : "rejected");
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const size_t n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    char* buf = (char*)malloc(n);
    if (!buf || fread(buf, 1, n, f) != n) return 2;
    fclose(f);
    size_t covered = 4;                                     /* the table names every byte of smap_op but its only padding, the 4 in front of in2_bias_off */
    for (int k = 0; k < N_FIELDS; ++k) covered += (size_t)FIELDS[k].count * (FIELDS[k].type == 'l' ? 8 : 4);
    if (covered != sizeof(smap_op) || offsetof(smap_op, in2_bias_off) != offsetof(smap_op, in2_acc_scale) + 8) { printf("field table covers %zu of %zu bytes\n", covered, sizeof(smap_op)); return 2; }
    char what[96];
    if (run(buf, n, "blob") != 0) return 1;
    smap_blob_header h;
    memcpy(&h, buf, sizeof(h));
    const size_t ops_end = (size_t)h.ops_offset + (size_t)h.n_ops * sizeof(smap_op);
    for (size_t k = 0; k < ops_end; ++k) {                  /* a block of exactly k bytes each */
        char* cut = (char*)malloc(k ? k : 1);
        memcpy(cut, buf, k);
        snprintf(what, sizeof(what), "truncated %zu", k);
        run(cut, k, what);
        free(cut);
    }
    static const int64_t VALUES[] = {-1, 0, 1, INT32_MAX, INT32_MIN, INT64_MAX, ((int64_t)1 << 32) - 8};
    for (int i = 0; i < h.n_ops; ++i)
        for (int k = 0; k < N_FIELDS; ++k)
            for (int e = 0; e < FIELDS[k].count; ++e) {
                const int wide = FIELDS[k].type == 'l';
                char* p = buf + h.ops_offset + (size_t)i * sizeof(smap_op) + FIELDS[k].off + (size_t)e * (wide ? 8 : 4);
                char saved[8];
                memcpy(saved, p, wide ? 8 : 4);
                for (int v = 0; v < (wide ? 7 : 5); ++v) {
                    const int32_t v32 = (int32_t)VALUES[v];
                    const float vf = (float)VALUES[v];
                    if (wide) memcpy(p, &VALUES[v], 8);
                    else if (FIELDS[k].type == 'f') memcpy(p, &vf, 4);
                    else memcpy(p, &v32, 4);
                    snprintf(what, sizeof(what), "op %d +%zu[%d] = %lld", i, FIELDS[k].off, e, (long long)VALUES[v]);
                    run(buf, n, what);
                }
                memcpy(p, saved, wide ? 8 : 4);
            }
    printf("total accepted %ld rejected %ld\n", counts[0], counts[1]);
    free(buf);
    return 0;
}
