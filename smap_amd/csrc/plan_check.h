// plan_check.h -- the host-side guard of the schedule executor (internal, not part of the C ABI; no HIP types): which smap_op arrays and
// plan blobs the library runs.  plan_check.cpp holds the rules, plan.hip the kernels and the launches.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "smap_hip.h"

// ZERO PAGES and WINDOWS.  The conv kernels address their input with (64-bit uniform base in SGPRs) + (32-bit byte offset per
// lane); offset 0..SMAP_ZERO_PAGE of that base must read as zeros (padding taps and rows past M fetch their 16 bytes there).
// The base of a launch is the WINDOW of its input: the arena offset in_off rounded down to a multiple of SMAP_WINDOW (4 GiB); as
// no tensor crosses a window boundary, an input tensor anywhere in an arena of any size is within 32 bits of its base.  Arena contract: bytes
// [k * SMAP_WINDOW, k * SMAP_WINDOW + SMAP_ZERO_PAGE) are reserved for every k >= 0 (no range any op touches overlaps them); smap_plan_run
// clears the ones its launches use on the stream before the first op.
constexpr int64_t SMAP_ZERO_PAGE = 16384;  // >= max Cin * 2 bytes + 16 (+ the lo-plane offset, <= 4096, in split precision):
                                           // a padding tap reads zero page + chunk*128 (+ lo offset)
constexpr int64_t SMAP_WINDOW = (int64_t)1 << 32;
inline int64_t window_of(int64_t off) { return off & ~(SMAP_WINDOW - 1); }

constexpr int SMAP_STEM_K = 176;           // halves per output channel of the packed stem weights (plan.hip ST_K: 22 granules x 8)

// What the checker hands to smap_plan_create: the schedule and what smap_plan_run needs besides the ops.
struct PlanCheck {
    std::vector<smap_op> ops;
    std::vector<int64_t> windows;          // arena offsets of the zero pages this schedule's conv launches address through
    struct Ticket { int64_t off, bytes; int op; };
    std::vector<Ticket> tickets;           // arena byte range of every split-K op's ticket slice (zeroed per op by smap_plan_run)
    std::vector<char> signalled;           // per op: some op of another lane waits for it (smap_op.wait_op)
    int n_lanes = 1;
};

// 0 and *out filled, or SMAP_E_ARG: every rule of smap_plan_create (include/smap_hip.h)
int plan_check(const smap_op* ops, int n_ops, PlanCheck* out);
// the same for a plan blob: header, every op, the weight section and the sizes the header states; info may be null
int plan_check_blob(const void* blob, size_t blob_bytes, PlanCheck* out, smap_blob_info* info);
// arena / output bytes checked ops touch
void plan_workspace_bytes(const std::vector<smap_op>& ops, int64_t* arena_bytes, int64_t* out_bytes);
