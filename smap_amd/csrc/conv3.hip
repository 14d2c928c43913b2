// conv3.hip -- 3x3 stride-1 pad-1 conv_bn_relu (model/smap.py:13-45, the Bottleneck 3x3s and the
// res_* heads) as a HALO-TILED implicit GEMM for gfx950.
//
// Why a second 3x3 path: the im2col view of conv.hip fetches every input element nine times, once
// per tap, through the L2 -> LDS stream that bounds these layers (loads alone are
// 70-90 % of their time).  Here a workgroup owns a 2-D tile of TH x TW = 128 output pixels; per
// 64-channel chunk it brings the (TH+2) x (TW+2) input patch into LDS ONCE and serves all nine taps
// from it (1.4-1.6x the tile instead of 9x); only the 8-16 KB weight tile changes per tap.
//
//   K order   : channel chunk cc (outer), tap (kh,kw) (inner) -- weights stay [cout][kh][kw][cin]
//   LDS       : A patch  2 x PROWS rows x 128 B (row = patch pixel, 16-B slot s holds granule
//               s ^ ((row>>1)&7), written by LDS-DMA exactly like conv.hip's tile rows)
//               B tile   NB x BN rows x 128 B
//   MFMA      : v_mfma_f32_32x32x16_f16; the A fragment of tap (kh,kw) for tile pixel (py,px) is
//               patch row (py+kh)*(TW+2) + px+kw -- a shifted view, no data movement
//   pipeline  : iteration = (cc, tap); NB-1 weight tiles and, from tap 0 of a chunk, the next patch are
//               in flight while the current tap is multiplied (counted vmcnt + raw s_barrier)
//   epilogue  : fp32 LDS tile -> bias, ReLU -> 16-byte NHWC stores (fp16, or fp32 for the heads)
//
// X3 (smap_op.precision = 1, see conv.hip): a chunk is 32 channels and an LDS row holds [hi(32) | lo(32)] of them --
// the same 128 bytes, the same swizzle, the same LDS footprint; the eight 16-byte slots of a row are logical granules
// 0..3 of the hi plane and 0..3 of the lo plane, fetched from the two planes of the pixel / the two weight matrices.
// A tap iteration then covers 32 channels with 2 K steps of three MFMAs (hi*hi + hi*lo + lo*hi).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "smap_hip.h"
#include "plan.h"
#include "conv_device.h"

#ifndef SMAP_STAG_DMA_IN_MFMA
#define SMAP_STAG_DMA_IN_MFMA 0   // staggered schedule: LDS-DMA requests issued from inside the MFMA burst instead of the read phase
#endif
#ifndef SMAP_STAG_DMA_POS
#define SMAP_STAG_DMA_POS 3       // ... in front of the MFMAs of accumulator POS (0..3) of the burst's first K step; 10 + POS: weight half there, patch piece before accumulator 3
#endif
#ifndef SMAP_ABLATE
#define SMAP_ABLATE 0      // diagnostics builds only (tools/build_ablate.py [--conv3]): 1 no LDS-DMA, 2 no MFMA, 8 no epilogue, 16 no ds_read, 32 no barriers in the staggered loop
#endif

namespace {

// ONE = the layer has a single 64-channel chunk (Cin = 64: the layer1 3x3s): no second patch buffer, which takes the
// workgroup from 80 to 52 KB of LDS (three per CU instead of two; residency is what these kernels are short of).
// BM = TH x TW output pixels per workgroup (128, or 256 with eight waves), NWV = 4 or 8 waves in a WM x WN grid.  The eight-wave
// shapes are for the 64x104 / 32x52 levels (round 4): a wave is blocked ~240 cycles per LDS-DMA instruction it issues, so what a wave
// can multiply between two barriers is bounded by the bytes it has to request for it.  256 pixels x 128 channels halves the weight
// bytes per MFMA (one workgroup per CU, two waves per SIMD); 128 x 128 with eight waves halves the requests per wave (two
// workgroups per CU, four waves per SIMD).
//
// STAG (eight waves, one workgroup per CU): the two waves of a SIMD (w and w + 4) run HALF AN ITERATION APART.  An iteration is two
// phases {fragment reads (+ LDS-DMA issue / vmcnt wait) ; barrier ; MFMAs ; barrier}; waves 4..7 pass one extra barrier before the
// loop (waves 0..3 one after it), so in every barrier interval one wave of each SIMD multiplies while the other reads -- in lockstep
// both waves expose every LDS and barrier latency to an idle matrix pipe (measured: 40 % of the pipe at best).  Order rules that
// make it safe (intervals I_k between consecutive barriers; tile T = weight tile of iteration T):
//   reads of T    : group 0 in I_{4T-1}, I_{4T+1}; group 1 in I_{4T}, I_{4T+2}; each retired (lgkmcnt(0)) BEFORE the reader's next barrier
//   publish  T    : every wave waits for its slice of T in phase 1 of iteration T-1, before that phase's first barrier (group 1: #4T-1)
//   refill        : the buffer of T is free from I_{4T+3}; B(T+D+1) = B(it+D) goes into it in phase 0 of it = T+1 (I_{4T+3} / I_{4T+4})
//   patches       : the same with chunk granularity (issued in phase 0 of tap 0, awaited in phase 1 of tap 8)
template <int BM, int BN, int TW, int NB, int NWV, int WN, int WPE, bool ONE, bool X3, bool STAG = false>
__global__ __launch_bounds__(NWV * 64, WPE) void conv3x3_halo_kernel(const ConvArgs a, int tiles_x, int tiles_y)
{
    static_assert(!STAG || (NWV == 8 && !ONE), "staggered schedule: eight waves");
    static_assert(!STAG || (BN / (NWV * 8)) % 2 == 0, "staggered schedule: a weight tile is requested in two halves");
    constexpr int CH = X3 ? 32 : 64;                            // channels per chunk
    constexpr int NPL = X3 ? 2 : 1;
    static_assert(!(ONE && X3), "split precision: Cin = 64 is two chunks");
    static_assert(NWV == 4 || NWV == 8, "4 or 8 waves");
    constexpr int NT = NWV * 64, RND = NWV * 8;                 // threads; rows one round of wave-wide LDS-DMA instructions covers
    constexpr int TH = BM / TW, PW = TW + 2, PH = TH + 2;
    static_assert(TH * TW == BM, "pixel tile");
    constexpr int PROWS = ((PH * PW + RND - 1) / RND) * RND;    // patch rows rounded to a DMA round
    constexpr int LA = PROWS / RND, LB = BN / RND;
    static_assert(LB >= 1 && LB * RND == BN, "BN is a multiple of the DMA round");
    constexpr int ROWB = 128;
    constexpr int A_BYTES = PROWS * ROWB, B_BYTES = BN * ROWB;
    constexpr int D = NB - 1;                                   // weight tiles in flight ahead of the one being multiplied
    static_assert(D >= 1 && D <= 8 && (D - 1) * LB + LA <= 24, "wait_vm covers 0..24");
    constexpr int NA = ONE ? 1 : 2;                              // patch buffers
    constexpr int PIPE = NA * A_BYTES + NB * B_BYTES;
    constexpr int LDS_BYTES = PIPE > BM * BN * 4 ? PIPE : BM * BN * 4;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
    constexpr int WM = NWV / WN;                                // 2 x 2 waves (wave tile 64 px x BN/2), 4 x 1 for BN = 32, 4 x 2 / 2 x 4 of eight
    static_assert(WM * WN == NWV, "wave grid");
    constexpr int MI = BM / WM / 32, NI = BN / WN / 32;
    static_assert(NI >= 1 && MI >= 1 && MI * 32 * WM == BM && NI * 32 * WN == BN, "wave tile");
    __shared__ __attribute__((aligned(16))) char smem[LDS_BYTES];

    SMAP_TL_BEGIN
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    const int logical = xcd_logical_block();                    // XCD-aware order, n tile fastest
    const int n_tile = logical % a.n_tiles;
    int t = logical / a.n_tiles;
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y, b = t / tiles_y;
    const int oy0 = ty * TH, ox0 = tx * TW, n0 = n_tile * BN;

    // ---- staging offsets (uniform base + 32-bit lane offset; 0 = zero page of the arena)
    const int lrow = lane >> 3, lslot = lane & 7;
    const int srow = wave * 8 + lrow;
    const int gl = lslot ^ ((srow >> 1) & 7);                   // (prow>>1)&7 == (srow>>1)&7: rounds are 32 / 64 rows
    const int gch = X3 ? (gl & 3) : gl;                         // channel granule inside the chunk ...
    const int gpl = X3 ? (gl >> 2) : 0;                         // ... of plane 0 (hi) / 1 (lo)
    const char* __restrict__ arena = reinterpret_cast<const char*>(a.arena);
    const char* __restrict__ wt = reinterpret_cast<const char*>(a.w);

    // weight tiles: one contiguous, pre-swizzled block per (n tile, chunk, tap) (smap_amd/engine.py::pack_conv_weights)
    const int w_chunks = a.Cin / CH;
    const char* __restrict__ wt_tile = wt + (long long)n_tile * w_chunks * 9 * B_BYTES;           // wave-uniform
    unsigned w_off[LB];                                         // per-lane 32-bit offsets inside a block
#pragma unroll
    for (int i = 0; i < LB; ++i) w_off[i] = (unsigned)((i * RND + wave * 8) * ROWB + lane * 16);
    auto issue_b = [&](int buf, int blk) {                      // blk = cc * 9 + tap
        char* sB = smem + NA * A_BYTES + buf * B_BYTES;
        const char* gB = wt_tile + (long long)blk * B_BYTES;
        if (SMAP_ABLATE & 1) return;
#pragma unroll
        for (int i = 0; i < LB; ++i)
            __builtin_amdgcn_global_load_lds((gbl_void*)(gB + w_off[i]), (lds_void*)(sB + (i * RND + wave * 8) * ROWB), 16, 0, 0);
    };
    issue_b(0, 0);                                              // weights of (cc 0, tap 0): no pixel math needed

    unsigned a_off[LA];                                         // patch pixel -> byte offset of its channel granule gch
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        const int prow = i * RND + srow;
        const int py = prow / PW, px = prow - py * PW;
        const int iy = oy0 - 1 + py, ix = ox0 - 1 + px;
        a_off[i] = 0;
        if (prow < PH * PW && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
            const long long e = ((long long)(b * a.H + iy) * a.W + ix) * a.in_stride_c + a.in_c_off + gch * 8 +
                                (X3 ? gpl * a.in_lo : 0);
            a_off[i] = (unsigned)(a.in_off + e * 2);
        }
    }
    auto issue_a = [&](int buf, int cc) {
        char* sA = smem + buf * A_BYTES;
        const char* gA = arena + (unsigned)(cc * CH * 2);       // invalid pixels: zero page + chunk offset
        if (SMAP_ABLATE & 1) return;
#pragma unroll
        for (int i = 0; i < LA; ++i)
            __builtin_amdgcn_global_load_lds((gbl_void*)(gA + a_off[i]), (lds_void*)(sA + (i * RND + wave * 8) * ROWB), 16, 0, 0);
    };
    issue_a(0, 0);
    auto issue_b_half = [&](int buf, int blk, int half) {       // staggered schedule: pieces [half * LB / 2, (half + 1) * LB / 2) of a weight tile
        char* sB = smem + NA * A_BYTES + buf * B_BYTES;
        const char* gB = wt_tile + (long long)blk * B_BYTES;
        if (SMAP_ABLATE & 1) return;
#pragma unroll
        for (int i = 0; i < LB; ++i)
            if (i / ((LB + 1) / 2) == half)
                __builtin_amdgcn_global_load_lds((gbl_void*)(gB + w_off[i]), (lds_void*)(sB + (i * RND + wave * 8) * ROWB), 16, 0, 0);
    };
    auto issue_a_piece = [&](int buf, int cc, int i) {
        char* sA = smem + buf * A_BYTES;
        const char* gA = arena + (unsigned)(cc * CH * 2);
        if (SMAP_ABLATE & 1) return;
        __builtin_amdgcn_global_load_lds((gbl_void*)(gA + a_off[i]), (lds_void*)(sA + (i * RND + wave * 8) * ROWB), 16, 0, 0);
    };

    f32x16 acc[MI][NI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mi][ni][r] = 0.f;

    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lhi = lane >> 5;
    // tile pixel of this lane's A fragment rows: p = wm*64 + mi*32 + l31 -> (py, px)
    int prow0[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int p = wm * (MI * 32) + mi * 32 + l31;
        prow0[mi] = (p / TW) * PW + (p % TW);                   // + kh*PW + kw per tap
    }
    const int b_row0 = wn * (BN / WN) + l31;
    const int bswz = (l31 >> 1) & 7;

    // ---- pipeline.  Flat iteration it = cc*9 + tap needs weight tile it (stage it % NB) and patch cc (stage
    //      cc & 1).  Weight tiles it+1 .. it+D-1 and, during taps 1..D, the next patch stay in flight across the
    //      barrier (counted vmcnt: loads retire in issue order).  Issue order per iteration: B(it+D), then at
    //      tap 0 A(cc+1) -- so A(cc+1) is younger than B(it) exactly while tap <= D.
    const int cchunks = a.Cin / CH;
    const int n_iter = cchunks * 9;
#pragma unroll
    for (int d = 1; d < D; ++d) issue_b(d, d);                              // taps 1..D-1 of chunk 0 (D <= 9)
    if constexpr (STAG) {
        constexpr int KPP = CH / 32;                                        // k16 steps per phase (two phases per iteration)
        const int grp = wave >> 2;
        wait_vm((D - 1) * LB);                                              // B(0), A(0) (issued before B(1..D-1))
        __builtin_amdgcn_s_barrier();
        if (grp) __builtin_amdgcn_s_barrier();                              // waves 4..7: half an iteration behind
        asm volatile("" ::: "memory");
        for (int cc = 0; cc < cchunks; ++cc) {
            const bool last = cc + 1 == cchunks;
            const char* sA = smem + (cc & 1) * A_BYTES;
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int it = cc * 9 + tap;
                const char* sB = smem + NA * A_BYTES + (it % NB) * B_BYTES;
                const int shift = (tap / 3) * PW + (tap % 3);
#pragma unroll
                for (int ph = 0; ph < 2; ++ph) {
                    half8 af[KPP][NPL][MI], bf[KPP][NPL][NI];
#pragma unroll
                    for (int kq = 0; kq < KPP; ++kq) {
                        const int g = (ph * KPP + kq) * 2 + lhi;
#pragma unroll
                        for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
                            for (int mi = 0; mi < MI; ++mi) {
                                const int prow = prow0[mi] + shift;
                                if (SMAP_ABLATE & 16) { for (int e = 0; e < 8; ++e) af[kq][pl][mi][e] = (_Float16)(float)(lane + g); continue; }
                                af[kq][pl][mi] = *reinterpret_cast<const half8*>(sA + prow * ROWB + (((g + 4 * pl) ^ ((prow >> 1) & 7)) << 4));
                            }
#pragma unroll
                            for (int ni = 0; ni < NI; ++ni) {
                                if (SMAP_ABLATE & 16) { for (int e = 0; e < 8; ++e) bf[kq][pl][ni][e] = (_Float16)(float)(tap + g); continue; }
                                bf[kq][pl][ni] = *reinterpret_cast<const half8*>(sB + (b_row0 + ni * 32) * ROWB + (((g + 4 * pl) ^ bswz) << 4));
                            }
                        }
                    }
                    // LDS-DMA requests: half of weight tile it+D per phase (buffer of tile it-1: free, see above), and piece
                    // i = 2 * tap + ph of the next patch in the first LA phases of a chunk.  Loads retire in issue order.
                    auto requests = [&](int what = 3) {                     // 1: the weight half, 2: the patch piece
                        const int nt = tap + D;
                        const int ncc = cc + nt / 9, ntap = nt % 9;
                        if ((what & 1) && ncc < cchunks) issue_b_half((it + D) % NB, ncc * 9 + ntap, ph);
                        if ((what & 2) && 2 * tap + ph < LA && !last) issue_a_piece((cc + 1) & 1, cc + 1, 2 * tap + ph);
                    };
                    if (!SMAP_STAG_DMA_IN_MFMA) requests();                 // in the read phase (a wave is held ~240 cycles per request there)
                    if (ph == 1) {                                          // publish tile it+1 (tap 8: the next patch is older than it)
                        if (SMAP_STAG_DMA_IN_MFMA) {
                            // D = 2, requests of phase (it, ph) issued inside that phase's MFMA burst: younger than the last piece of
                            // B(it+1) (burst of (it-1, 1)) are the patch piece of that burst, and B(it+2)'s first half + patch piece of burst (it, 0)
                            static_assert(!SMAP_STAG_DMA_IN_MFMA || D == 2, "derived for two weight tiles in flight");
                            const int na = ((2 * tap - 1 >= 0 && 2 * tap - 1 < LA) ? 1 : 0) + ((2 * tap < LA) ? 1 : 0);
                            if (last) wait_vm(tap + 2 <= 8 ? LB / 2 : 0);
                            else wait_vm(LB / 2 + na);
                        } else {
                            // requests younger than the last piece of B(it+1) (issued in phase 1 of iteration it+1-D): D-1 whole tiles and
                            // the patch pieces of phases 2*(tap+1-D)+1 .. 2*tap+1
                            const int lo_ = 2 * (tap + 1 - D) + 1, hi_ = 2 * tap + 1;
                            const int na = (hi_ < LA - 1 ? hi_ : LA - 1) - (lo_ > 0 ? lo_ : 0) + 1;
                            if (last) wait_vm((D - 1 < 7 - tap ? D - 1 : (7 - tap > 0 ? 7 - tap : 0)) * LB);
                            else wait_vm((D - 1) * LB + (na > 0 ? na : 0));
                        }
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // this phase's reads are done before anyone refills
                    if (!(SMAP_ABLATE & 32)) __builtin_amdgcn_s_barrier();
                    __builtin_amdgcn_sched_barrier(0);
                    __builtin_amdgcn_s_setprio(1);
#pragma unroll
                    for (int kq = 0; kq < KPP; ++kq)
#pragma unroll
                        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                            for (int ni = 0; ni < NI; ++ni) {
                                if (SMAP_STAG_DMA_IN_MFMA && kq == 0) {
                                    constexpr int pos = SMAP_STAG_DMA_POS % 10, split = SMAP_STAG_DMA_POS >= 10;
                                    const int idx = mi * NI + ni;
                                    if (idx == pos || (split && idx == MI * NI - 1)) {
                                        __builtin_amdgcn_sched_barrier(0);
                                        requests(!split ? 3 : idx == pos ? 1 : 2);
                                        __builtin_amdgcn_sched_barrier(0);
                                    }
                                }
                                if (SMAP_ABLATE & 2) { acc[mi][ni][kq + ph] += (float)af[kq][0][mi][0] + (float)bf[kq][0][ni][1] + (float)af[kq][NPL - 1][mi][2] + (float)bf[kq][NPL - 1][ni][3]; continue; }
                                if (X3) {
                                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[kq][NPL - 1][mi], bf[kq][0][ni], acc[mi][ni], 0, 0, 0);
                                    acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[kq][0][mi], bf[kq][NPL - 1][ni], acc[mi][ni], 0, 0, 0);
                                }
                                acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[kq][0][mi], bf[kq][0][ni], acc[mi][ni], 0, 0, 0);
                            }
                    __builtin_amdgcn_s_setprio(0);
                    __builtin_amdgcn_sched_barrier(0);
                    if (!(SMAP_ABLATE & 32)) __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                }
            }
        }
        if (!grp) __builtin_amdgcn_s_barrier();
    } else
    for (int cc = 0; cc < cchunks; ++cc) {
        const bool last = cc + 1 == cchunks;
        const char* sA = smem + (cc & 1) * A_BYTES;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int it = cc * 9 + tap;
            if (last) {
                if (tap + D - 1 >= 9) wait_vm(0);                           // tail: fewer tiles were issued
                else wait_vm((D - 1) * LB);
            } else {
                wait_vm((D - 1) * LB + ((tap >= 1 && tap <= D) ? LA : 0));
            }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            {
                const int nt = tap + D;                                     // tap index of iteration it+D
                const int ncc = cc + nt / 9, ntap = nt % 9;
                if (ncc < cchunks) issue_b((it + D) % NB, ncc * 9 + ntap);
                if (tap == 0 && !last) issue_a((cc + 1) & 1, cc + 1);
            }
            const char* sB = smem + NA * A_BYTES + (it % NB) * B_BYTES;
            const int shift = (tap / 3) * PW + (tap % 3);
#pragma unroll
            for (int kk = 0; kk < CH / 16; ++kk) {
                const int g = kk * 2 + lhi;
                half8 af[NPL][MI], bf[NPL][NI];
#pragma unroll
                for (int pl = 0; pl < NPL; ++pl) {
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi) {
                        const int prow = prow0[mi] + shift;
                        if (SMAP_ABLATE & 16) { for (int e = 0; e < 8; ++e) af[pl][mi][e] = (_Float16)(float)(lane + kk); continue; }
                        af[pl][mi] = *reinterpret_cast<const half8*>(sA + prow * ROWB + (((g + 4 * pl) ^ ((prow >> 1) & 7)) << 4));
                    }
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) {
                        if (SMAP_ABLATE & 16) { for (int e = 0; e < 8; ++e) bf[pl][ni][e] = (_Float16)(float)(tap + kk); continue; }
                        bf[pl][ni] = *reinterpret_cast<const half8*>(sB + (b_row0 + ni * 32) * ROWB + (((g + 4 * pl) ^ bswz) << 4));
                    }
                }
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                    for (int ni = 0; ni < NI; ++ni) {
                        if (SMAP_ABLATE & 2) { acc[mi][ni][kk] += (float)af[0][mi][0] + (float)bf[0][ni][1]; continue; }
                        if (X3) {
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[NPL - 1][mi], bf[0][ni], acc[mi][ni], 0, 0, 0);
                            acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0][mi], bf[NPL - 1][ni], acc[mi][ni], 0, 0, 0);
                        }
                        acc[mi][ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(af[0][mi], bf[0][ni], acc[mi][ni], 0, 0, 0);
                    }
            }
        }
    }
    (void)n_iter;
    __syncthreads();
    if (SMAP_ABLATE & 8) {
        if (acc[0][0][0] == 12345.678f) reinterpret_cast<float*>(a.out)[tid] = acc[MI - 1][NI - 1][1];   // keep acc live
        return;
    }

    // ---- epilogue: acc + bias -> fp32 [128][BN] LDS tile -> ReLU -> 16-byte NHWC stores
    float* Cs = reinterpret_cast<float*>(smem);
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) {
        const int col = wn * (BN / WN) + ni * 32 + l31;
        const float bias = a.bias[n0 + col];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = wm * (MI * 32) + mi * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                Cs[row * BN + col] = X3 ? acc[mi][ni][r] * a.acc_scale + bias : acc[mi][ni][r] + bias;
            }
    }
    __syncthreads();
    constexpr int CG = BN / 8, PASSES = BM * CG / NT;
    static_assert(PASSES * NT == BM * CG, "tile / thread mismatch");
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
        const int idx = p * NT + tid;
        const int row = idx / CG, cg = idx - row * CG;
        const int oy = oy0 + row / TW, ox = ox0 + row % TW, n = n0 + cg * 8;
        if (oy >= a.Ho || ox >= a.Wo || n >= a.Cout8) continue;
        const float4 lo = *reinterpret_cast<const float4*>(Cs + row * BN + cg * 8);
        const float4 hi = *reinterpret_cast<const float4*>(Cs + row * BN + cg * 8 + 4);
        float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        if (a.relu) {
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = v[e] < 0.f ? 0.f : v[e];       // NaN stays NaN, as torch's ReLU: an overflow must reach the head-sum guard
        }
        const long long m = ((long long)b * a.Ho + oy) * a.Wo + ox;
        const long long o = m * a.out_stride_c + a.out_c_off + n;
        if (a.out_fp32) {
            float* op = reinterpret_cast<float*>(a.out) + o;
            *reinterpret_cast<float4*>(op) = make_float4(v[0], v[1], v[2], v[3]);
            *reinterpret_cast<float4*>(op + 4) = make_float4(v[4], v[5], v[6], v[7]);
        } else {
            half8 h;
#pragma unroll
            for (int e = 0; e < 8; ++e) h[e] = (_Float16)v[e];
            *reinterpret_cast<half8*>(reinterpret_cast<_Float16*>(a.out) + o) = h;
            if (X3) {
                half8 l;
#pragma unroll
                for (int e = 0; e < 8; ++e) l[e] = (_Float16)(v[e] - (float)h[e]);
                *reinterpret_cast<half8*>(reinterpret_cast<_Float16*>(a.out) + o + a.out_lo) = l;
            }
        }
    }
    SMAP_TL_END(a)
}

// TILE: the row of csrc/tiles.h that BM and BN come from; the kernel's own arguments (TW = width of the pixel patch, NB = weight buffers,
// NWV waves of which WN along N, WPE = waves per SIMD of __launch_bounds__, STAG) stay on the dispatch line
template <int TILE, int TW, int NB, int NWV = 4, int WN = (tile_row(TILE).bn >= 64 ? 2 : 1), int WPE = 1, bool STAG = false>
hipError_t launch3(const ConvArgs& a, hipStream_t st)
{
    constexpr TileRow t = tile_row(TILE);
    static_assert(t.family == TF_HALO, "csrc/tiles.h: not a halo tile id");
    constexpr int BM = t.bm, BN = t.bn, TH = BM / TW;
    const int B = a.M / (a.Ho * a.Wo);
    const int tiles_x = (a.Wo + TW - 1) / TW, tiles_y = (a.Ho + TH - 1) / TH;
    const dim3 grid(tiles_x * tiles_y * B * a.n_tiles), block(NWV * 64);
    if (a.x3)
        hipLaunchKernelGGL((conv3x3_halo_kernel<BM, BN, TW, NB, NWV, WN, WPE, false, true, STAG>), grid, block, 0, st, a, tiles_x, tiles_y);
    else if constexpr (NWV == 4) {
        if (a.Cin == 64)
            hipLaunchKernelGGL((conv3x3_halo_kernel<BM, BN, TW, NB, NWV, WN, WPE, true, false>), grid, block, 0, st, a, tiles_x, tiles_y);
        else
            hipLaunchKernelGGL((conv3x3_halo_kernel<BM, BN, TW, NB, NWV, WN, WPE, false, false>), grid, block, 0, st, a, tiles_x, tiles_y);
    } else
        hipLaunchKernelGGL((conv3x3_halo_kernel<BM, BN, TW, NB, NWV, WN, WPE, false, false, STAG>), grid, block, 0, st, a, tiles_x, tiles_y);
    return hipGetLastError();
}

}  // namespace

// Only plain 3x3 stride-1 convs qualify (no residual / addends / bilinear add): the schedule's Bottleneck
// 3x3s and head convs.  Returns hipErrorInvalidValue otherwise (plan validation rejects such ops earlier).
hipError_t smap_launch_conv3(const ConvArgs& a, int tile, hipStream_t st)
{
    if (a.ksize != 3 || a.stride != 1 || a.pad != 1 || a.res || a.add1 || a.add2 || a.up) return hipErrorInvalidValue;
    switch (tile) {                                     // <tile id, TW, NB, NWV, WN, WPE, STAG>
        case 30: return launch3<30, 16, 2>(a, st);
        case 31: return launch3<31, 16, 2>(a, st);
        case 32: return launch3<32, 32, 2>(a, st);
        case 33: return launch3<33, 32, 2>(a, st);
        case 34: return launch3<34, 16, 4>(a, st);
        case 35: return launch3<35, 16, 3>(a, st);
        case 36: return launch3<36, 32, 3>(a, st);
        case 37: return launch3<37, 32, 3>(a, st);
        case 38: return launch3<38, 16, 4>(a, st);
        case 39: return launch3<39, 32, 4>(a, st);
        case 40: return launch3<40, 16, 2, 8, 2, 4>(a, st);
        case 41: return launch3<41, 16, 3, 8, 2, 2>(a, st);
        case 42: return launch3<42, 16, 4, 8, 2, 2>(a, st);
        case 43: return launch3<43, 32, 3, 8, 2, 2>(a, st);
        case 44: return launch3<44, 16, 3, 8, 2, 2, true>(a, st);
        case 45: return launch3<45, 32, 3, 8, 2, 2, true>(a, st);
        default: return hipErrorInvalidValue;
    }
}
