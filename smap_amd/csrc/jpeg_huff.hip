// jpeg_huff.hip -- the Huffman decode of a baseline JPEG scan on gfx950 (include/smap_hip.h "Huffman decode on the device"): the launches
// around csrc/jpeg_huff.h, which states the algorithm per subsequence.  One frame is a fixed sequence on the caller's stream:
//   memset of the coefficients, the DC differences and the status word
//   huff_sync_kernel round 0      every lane decodes its subsequence from (block 0, zig-zag 0); then, inside the workgroup, every lane
//                                 whose left neighbour's exit state is not its entry state takes it and decodes again, until none changes
//   huff_sync_kernel round 1..R   workgroup g takes workgroup g-1's last exit state OF THE ROUND BEFORE (two buffers by round parity: no
//                                 launch reads what it writes) and propagates again; a workgroup whose entry is unchanged returns at once
//   scan_chunks / scan_totals     blocks completed per subsequence -> the number of each subsequence's first block
//   huff_exact_kernel             the exact pass from the final entry states: writes the coefficients and the DC differences, repeats
//                                 the host decoder's checks, and verifies that its exit state is the next lane's entry state and that the
//                                 block counts are the ones the numbering used.  Only this pass decides the status word.
//   scan_chunks / scan_totals / dc_store_kernel   DC predictors: running sums of the differences per restart interval
// No kernel waits on another workgroup; nothing is read back.  Per workgroup the file span of its 256 subsequences and the scan's
// Huffman tables are staged in LDS; a lane that runs past the span reads global memory.  Every file read is below file_bytes (Src::at's
// callers), every coefficient write inside the planes geo_init checked, every loop bounded by a size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "hip_rc.h"
#include "jpeg_huff.h"
#include "smap_hip.h"

namespace {

using namespace smap_huff;

constexpr int kTabWords = int(sizeof(smap_jpeg_huff) / 4);
static_assert(sizeof(smap_jpeg_huff) % 4 == 0 && sizeof(smap_jpeg_scan) % 8 == 0, "tables are copied as 32-bit words");

struct Ws {
    uint64_t* entry;
    uint64_t* exit;
    uint64_t* gexit;
    int32_t* nblk;
    int32_t* ntot;
    int32_t* dcd;
    int32_t* dctot;
};

// the scan's tables and the workgroup's span of the file into LDS; -> the byte source of the workgroup's lanes
__device__ inline Src stage(const uint8_t* __restrict__ file, const smap_jpeg_scan* __restrict__ scan, const Geo& g, int grp,
                            smap_jpeg_huff* s_tab, uint8_t* s_stage, bool aligned16) {
    const int t = threadIdx.x;
    const uint32_t* tw = reinterpret_cast<const uint32_t*>(scan->table);
    uint32_t* sw = reinterpret_cast<uint32_t*>(s_tab);
    for (int k = t; k < 2 * g.ncomp * kTabWords; k += kLanes) sw[k] = tw[k];
    const uint32_t lo = (g.scan_off + uint32_t(grp) * uint32_t(kLanes * g.S)) & ~15u;
    const uint32_t want = uint32_t(kLanes * g.S) + 16u;
    const uint32_t len = g.n - lo < want ? g.n - lo : want;
    const uint32_t vec = aligned16 ? len / 16u : 0u;
    for (uint32_t k = t; k < vec; k += kLanes)                     // coalesced 16-byte loads (file + lo is 16-byte aligned)
        reinterpret_cast<uint4*>(s_stage)[k] = reinterpret_cast<const uint4*>(file + lo)[k];
    for (uint32_t k = vec * 16u + t; k < len; k += kLanes) s_stage[k] = file[lo + k];
    Src s;
    s.file = file;
    s.stage = s_stage;
    s.n = g.n;
    s.lo = lo;
    s.len = len;
    return s;
}

__global__ __launch_bounds__(kLanes) void huff_sync_kernel(const uint8_t* __restrict__ file, const smap_jpeg_scan* __restrict__ scan,
                                                           Geo garg, Ws w, int round, int aligned16) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_stage[];
    __shared__ smap_jpeg_huff s_tab[6];
    __shared__ uint64_t s_exit[kLanes];
    __shared__ Geo s_g;
    const int t = threadIdx.x, grp = blockIdx.x, i = grp * kLanes + t;
    const uint64_t* prev = w.gexit + ((round - 1) & 1) * garg.ngroups;
    uint64_t* cur = w.gexit + (round & 1) * garg.ngroups;
    if (round > 0 && (grp == 0 || prev[grp - 1] == w.entry[grp * kLanes])) {    // entry unchanged (uniform): nothing to propagate
        if (t == 0) cur[grp] = prev[grp];
        return;
    }
    if (t == 0) s_g = garg;
    const Src src = stage(file, scan, garg, grp, s_tab, s_stage, aligned16 != 0);
    __syncthreads();
    const Geo& g = s_g;
    const bool live = i < g.nsub;
    const Out none = {nullptr, nullptr};
    uint64_t my_entry = kEnd, my_exit = kEnd;
    int32_t my_nblk = 0;
    bool redo = false;
    if (round == 0) {
        if (live) my_entry = fresh_state(src, g, i);
        redo = live;
    } else if (live) {
        my_entry = w.entry[i];
        my_exit = w.exit[i];
        my_nblk = w.nblk[i];
        if (t == 0) {
            my_entry = prev[grp - 1];
            redo = true;
        }
    }
    for (int sweep = 0; sweep <= kLanes + 1; ++sweep) {            // (one body for the first decode and the sweeps: predicated, uniform trip count)
        if (redo) {
            const Result r = decode_subseq<false>(src, s_tab, g, i, my_entry, 0, none);
            my_exit = r.exit;
            my_nblk = r.nblk;
        }
        s_exit[t] = my_exit;
        __syncthreads();
        const uint64_t want = t ? s_exit[t - 1] : my_entry;
        redo = live && want != my_entry;
        if (!__syncthreads_or(redo)) break;                        // (also the barrier between this read of s_exit and the next write)
        if (redo) my_entry = want;
    }
    if (live) {
        w.entry[i] = my_entry;
        w.exit[i] = my_exit;
        w.nblk[i] = my_nblk;
        if (t == kLanes - 1 || i == g.nsub - 1) cur[grp] = my_exit;
    }
}

__global__ __launch_bounds__(kLanes) void huff_exact_kernel(const uint8_t* __restrict__ file, const smap_jpeg_scan* __restrict__ scan,
                                                            Geo garg, Ws w, int16_t* __restrict__ coeffs, int32_t* __restrict__ status,
                                                            int aligned16) {
    extern __shared__ __attribute__((aligned(16))) uint8_t s_stage[];
    __shared__ smap_jpeg_huff s_tab[6];
    __shared__ Geo s_g;
    const int t = threadIdx.x, grp = blockIdx.x, i = grp * kLanes + t;
    if (t == 0) s_g = garg;
    const Src src = stage(file, scan, garg, grp, s_tab, s_stage, aligned16 != 0);
    __syncthreads();
    const Geo& g = s_g;
    if (i >= g.nsub) return;
    const int32_t n0 = sum_upto(w.nblk, w.ntot, i - 1);
    const Out out = {coeffs, w.dcd};
    const Result r = decode_subseq<true>(src, s_tab, g, i, w.entry[i], n0, out);
    int flags = r.flags;
    if (n0 + r.nblk != sum_upto(w.nblk, w.ntot, i)) flags |= kNotConv;          // the numbering rests on these counts
    if (i + 1 < g.nsub) {
        if (r.exit != w.entry[i + 1]) flags |= kNotConv;                        // the chain of states closes
    } else if (r.exit != kEnd) {
        flags |= kEData;                                                        // every block, then EOI
    }
    if (flags) atomicOr(status, flags);
}

// inclusive sums of 256 values, one per thread, through LDS
__device__ inline uint32_t group_inclusive(uint32_t v, uint32_t* s) {
    const int t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (int d = 1; d < kLanes; d <<= 1) {
        const uint32_t add = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    return s[t];
}

// x[chunk * kChunk ...] -> its inclusive sums; tot[chunk] = the chunk's total
__global__ __launch_bounds__(kLanes) void scan_chunks_kernel(int32_t* __restrict__ x, int32_t* __restrict__ tot, int32_t count) {
    __shared__ uint32_t s[kLanes];
    constexpr int kPer = kChunk / kLanes;
    const int32_t base = int32_t(blockIdx.x) * kChunk + int32_t(threadIdx.x) * kPer;
    uint32_t v[kPer], sum = 0;
#pragma unroll
    for (int k = 0; k < kPer; ++k) {
        sum += base + k < count ? uint32_t(x[base + k]) : 0u;
        v[k] = sum;
    }
    const uint32_t before = group_inclusive(sum, s) - sum;
#pragma unroll
    for (int k = 0; k < kPer; ++k)
        if (base + k < count) x[base + k] = int32_t(v[k] + before);
    if (threadIdx.x == kLanes - 1) tot[blockIdx.x] = int32_t(before + sum);
}

// tot[0 .. nchunks) -> its exclusive sums (one workgroup, 256 chunks a turn)
__global__ __launch_bounds__(kLanes) void scan_totals_kernel(int32_t* __restrict__ tot, int32_t nchunks) {
    __shared__ uint32_t s[kLanes];
    uint32_t carry = 0;
    for (int32_t base = 0; base < nchunks; base += kLanes) {
        const int32_t k = base + int32_t(threadIdx.x);
        const uint32_t v = k < nchunks ? uint32_t(tot[k]) : 0u;
        const uint32_t inc = group_inclusive(v, s);
        if (k < nchunks) tot[k] = int32_t(carry + inc - v);
        carry += s[kLanes - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kLanes) void dc_store_kernel(Geo g, const int32_t* __restrict__ x, const int32_t* __restrict__ tot,
                                                          int16_t* __restrict__ coeffs) {
    const int32_t e = int32_t(blockIdx.x) * kLanes + int32_t(threadIdx.x);
    if (e < g.total) dc_store(g, x, tot, e, coeffs);
}

int run_scan(int32_t* x, int32_t* tot, int32_t count, hipStream_t st) {
    const int32_t nchunks = (count + kChunk - 1) / kChunk;
    hipLaunchKernelGGL(scan_chunks_kernel, dim3(unsigned(nchunks)), dim3(kLanes), 0, st, x, tot, count);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    hipLaunchKernelGGL(scan_totals_kernel, dim3(1), dim3(kLanes), 0, st, tot, nchunks);
    return hip_rc(hipGetLastError());
}

}  // namespace

extern "C" int64_t smap_jpeg_huff_workspace_bytes(const smap_jpeg_info* info, size_t file_bytes, int subseq_bytes) {
    Geo g;
    if (!info || !geo_init(&g, *info, file_bytes, subseq_bytes)) return 0;
    return workspace_layout(g).bytes;
}

extern "C" int smap_jpeg_decode_coefficients_device(const uint8_t* d_file, size_t file_bytes, const smap_jpeg_info* info,
                                                    const smap_jpeg_scan* d_scan, int subseq_bytes, int rounds, void* workspace,
                                                    int64_t workspace_bytes, int16_t* d_coeffs, int32_t* d_status, void* stream) {
    Geo g;
    if (!d_file || !info || !d_scan || !workspace || !d_coeffs || !d_status || rounds < 0) return SMAP_E_ARG;
    if (!geo_init(&g, *info, file_bytes, subseq_bytes)) return SMAP_E_ARG;
    const Workspace L = workspace_layout(g);
    if (workspace_bytes < L.bytes || (uintptr_t(workspace) & 7) || (uintptr_t(d_scan) & 7)) return SMAP_E_ARG;
    if (rounds == 0) rounds = SMAP_JPEG_ROUNDS;
    if (rounds > g.ngroups) rounds = g.ngroups;                    // the number of workgroups is provably enough
    hipStream_t st = (hipStream_t)stream;
    char* base = static_cast<char*>(workspace);
    Ws w;
    w.entry = reinterpret_cast<uint64_t*>(base + L.entry);
    w.exit = reinterpret_cast<uint64_t*>(base + L.exit);
    w.gexit = reinterpret_cast<uint64_t*>(base + L.gexit);
    w.nblk = reinterpret_cast<int32_t*>(base + L.nblk);
    w.ntot = reinterpret_cast<int32_t*>(base + L.ntot);
    w.dcd = reinterpret_cast<int32_t*>(base + L.dcd);
    w.dctot = reinterpret_cast<int32_t*>(base + L.dctot);
    const int aligned16 = (uintptr_t(d_file) & 15) == 0;
    const size_t lds = size_t(kLanes) * size_t(g.S) + 16;

    if (hipError_t e = hipMemsetAsync(d_coeffs, 0, size_t(info->coef_bytes), st); e != hipSuccess) return hip_rc(e);
    if (hipError_t e = hipMemsetAsync(w.dcd, 0, size_t(g.total) * 4, st); e != hipSuccess) return hip_rc(e);
    if (hipError_t e = hipMemsetAsync(d_status, 0, 4, st); e != hipSuccess) return hip_rc(e);
    for (int r = 0; r <= rounds; ++r) {
        hipLaunchKernelGGL(huff_sync_kernel, dim3(unsigned(g.ngroups)), dim3(kLanes), lds, st, d_file, d_scan, g, w, r, aligned16);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    }
    if (int rc = run_scan(w.nblk, w.ntot, g.nsub, st)) return rc;
    hipLaunchKernelGGL(huff_exact_kernel, dim3(unsigned(g.ngroups)), dim3(kLanes), lds, st, d_file, d_scan, g, w, d_coeffs, d_status,
                       aligned16);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    if (int rc = run_scan(w.dcd, w.dctot, g.total, st)) return rc;
    hipLaunchKernelGGL(dc_store_kernel, dim3(unsigned((g.total + kLanes - 1) / kLanes)), dim3(kLanes), 0, st, g, w.dcd, w.dctot, d_coeffs);
    return hip_rc(hipGetLastError());
}
