// block_device.h -- the phases the whole-Bottleneck kernels share (convb.hip: bottleneck_kernel, bottleneck_first_kernel; the LDS write-backs
// also serve convc.hip), each written once.  Like conv_device.h: inline templates only, no kernels, no __shared__ objects -- every function
// works on the ONE array its kernel declares.  ConvArgs always arrives by const reference and its fields are read where they are used: handed
// over by value, the kernel-argument loads move to the call site and cost up to 57 VGPRs in kernels that sit 9 below the limit of two waves
// per SIMD.  Every loop over accumulators and fragments is fully unrolled with compile-time indices (EXPERIMENTS R3.6).
#pragma once
#include "conv_device.h"

#ifndef SMAP_CONVB_LDS_KB
#define SMAP_CONVB_LDS_KB 80     // LDS per workgroup of convb.hip's kernels (two per CU); experiments: 64
#endif
#ifndef SMAP_CONVB_ABLATE
#define SMAP_CONVB_ABLATE 0      // diagnostics builds only (tools/build_ablate.py --convb N): 1 no x loads (identity kernel), and in both
#endif                           // kernels' shared phases 2 no MFMA, 4 no global stores, 8 no weight loads (W1 stages and the slot ring)

namespace {

// ================================================================= pieces that do not depend on the 64-plane geometry (convc.hip uses them too)

// acc[4*q + e] = b[8*q + e] / scale: a bias enters through the ACCUMULATORS (the power-of-two scale makes that exact).  b = the bias of the
// lane's first channel (chunk * 32 + 4 * lhi); an MFMA with the weights first leaves channels 8*q + 4*lhi + e in acc[4*q + e].
__device__ __forceinline__ void load_bias16(float4 (&raw)[4], const float* b)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) raw[q] = *reinterpret_cast<const float4*>(b + 8 * q);
}
__device__ __forceinline__ void acc_from_bias(f32x16& acc, const float4 (&raw)[4], float inv)
{
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        acc[4 * q + 0] = raw[q].x * inv; acc[4 * q + 1] = raw[q].y * inv;
        acc[4 * q + 2] = raw[q].z * inv; acc[4 * q + 3] = raw[q].w * inv;
    }
}

// row `prow` of the (PH x PW) halo patch whose centre tile starts at (oy0, ox0) lies inside the image (outside: the 3x3's zero padding)
template <int PW, int PH>
__device__ __forceinline__ bool patch_row_live(const ConvArgs& a, int prow, int oy0, int ox0)
{
    const int py = prow / PW, px = prow - py * PW;
    const int iy = oy0 - 1 + py, ix = ox0 - 1 + px;
    return prow < PH * PW && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
}

// The LDS write-back of y1 and y2: accumulators -> scale (+ bias) -> ReLU -> (live ? x : 0) -> hi | lo fp16 -> row r of a 32-channel chunk
// in conv3.hip's format (128-byte rows [hi32 | lo32], slot s = logical granule s ^ ((r >> 1) & 7)).  acc[4*q + e] = channel 8*q + 4*lhi + e
// of the chunk.  BIAS: bias points at the lane's first channel in a float table; otherwise the bias is already inside the accumulators.
template <bool BIAS>
__device__ __forceinline__ void put_row_hilo(char* chunk, int r, int lhi, const f32x16& acc, const float& scale, bool live, const float* bias)
{
    const int sw = (r >> 1) & 7;
    char* row = chunk + r * 128 + lhi * 8;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float bb[4] = {0.f, 0.f, 0.f, 0.f};
        if (BIAS) {
            const float4 b4 = *reinterpret_cast<const float4*>(bias + 8 * q);
            bb[0] = b4.x; bb[1] = b4.y; bb[2] = b4.z; bb[3] = b4.w;
        }
        half4 h, l;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = BIAS ? acc[4 * q + e] * scale + bb[e] : acc[4 * q + e] * scale;
            x = x < 0.f ? 0.f : x;                              // NaN stays NaN (torch's ReLU)
            x = live ? x : 0.f;
            h[e] = (_Float16)x;
            l[e] = (_Float16)(x - (float)h[e]);
        }
        *reinterpret_cast<half4*>(row + ((q ^ sw) << 4)) = h;
        *reinterpret_cast<half4*>(row + (((q + 4) ^ sw) << 4)) = l;
    }
}

// pixel -> output offsets of this lane's MI columns: pixel p0 + mi*32 of the tile (TW pixels wide) that starts at (oy0, ox0) in image b.
// dense = offset in a [pixels][hi C | lo C] residual / skip tensor, out = offset in a.out; both 0-based for pixels outside the image.
template <int MI, int TW>
__device__ __forceinline__ void pixel_offsets(bool (&m_ok)[MI], unsigned (&m_dense)[MI], unsigned (&m_out)[MI], const ConvArgs& a, int b, int oy0,
                                              int ox0, int p0)
{
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) {
        const int p = p0 + mi * 32;
        const int oy = oy0 + p / TW, ox = ox0 + p % TW;
        m_ok[mi] = oy < a.Ho && ox < a.Wo;
        const unsigned m = m_ok[mi] ? (unsigned)((b * a.Ho + oy) * a.Wo + ox) : 0u;
        m_dense[mi] = m * (unsigned)(2 * a.tail_cout8);
        m_out[mi] = m * (unsigned)a.out_stride_c + (unsigned)a.out_c_off;
    }
}

// ================================================================= the 64-plane block (convb.hip): TH x 16 output pixels, 4 waves

// (diagnostics: an MFMA that can be compiled out, keeping its operands alive)
__device__ __forceinline__ f32x16 block_mfma(half8 x, half8 y, f32x16 c)
{
#if SMAP_CONVB_ABLATE & 2
    c[0] += (float)x[0] + (float)y[1];
    return c;
#else
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, c, 0, 0, 0);
#endif
}

template <int TH>
struct BlockGeom {
    static constexpr int P = 64, C = 4 * P, TW = 16, CH = 32, ROWB = 128;
    static constexpr int PW = TW + 2, PH = TH + 2;
    static constexpr int PROWS = ((PH * PW + 31) / 32) * 32;    // patch rows rounded to MFMA blocks: 128 | 192
    static constexpr int MB1 = PROWS / 32;                      // M blocks of phase 1: 4 | 6
    static constexpr int NB1 = MB1 == 6 ? 3 : 2;                // 32 x 32 blocks of y1 per wave: (mb = wave, n = 0 | 1) [+ one of M blocks 4, 5]
    static constexpr int BM = TH * TW;                          // output pixels of the tile: 64 | 128
    static constexpr int MI = BM / 64;                          // 32-pixel blocks per wave in phases 2, 3 (2 x 2 waves): 1 | 2
    static constexpr int KC2 = P / CH;                          // 32-channel chunks of the 3x3's and the tail's K: 2
    static constexpr int Y1_BYTES = KC2 * PROWS * ROWB;         // 32 | 48 KiB
    static constexpr int Y2_BYTES = KC2 * BM * ROWB;            // 16 | 32 KiB: y2 takes over the start of y1's region
    static constexpr int LDS_BYTES = SMAP_CONVB_LDS_KB * 1024;
    static constexpr int SLOT = P * ROWB;                       // 8 KiB weight slot: 64 rows x one 32-channel chunk
    static constexpr int NS = (LDS_BYTES - Y1_BYTES) / SLOT;    // ring slots behind y1: 6 | 4
    static constexpr int LS = SLOT / 4096;                      // LDS-DMA instructions per thread and slot: 2
    static constexpr int NTAP = 9, NCH3 = C / 64;
    static constexpr int NS2 = NTAP * KC2, NS3 = NCH3 * KC2;    // 18 (tap, chunk) slots of the 3x3, 8 (tail chunk, k chunk) slots
    static_assert(MB1 == 4 || MB1 == 6, "TH = 4 or 8");
    static_assert(Y2_BYTES + C * 4 + P * 4 <= Y1_BYTES && C == 256, "room for the bias tables (tail [C], b2 [P]); one tail-bias value per thread");
    static_assert(NS >= 2 && Y1_BYTES + NS * SLOT <= LDS_BYTES, "LDS plan");
};

// tile decode and per-lane indices
template <int TH>
struct BlockLane {
    int tid, lane, wave;                                        // wave: uniform (a scalar register)
    int b, oy0, ox0;                                            // image and first output pixel of the tile
    int l31, lhi;
    int wm, wn;                                                 // phases 2, 3: pixel half / channel half of the wave
    int xmb, xnb;                                               // the extra y1 block (TH = 8): patch rows 128..191, channel half wave & 1
    int fswz;                                                   // (row >> 1) & 7 of every 128-byte fragment row = multiple of 32 + l31
    int crow[BlockGeom<TH>::MI];                                // centre pixels p = wm*(MI*32) + mi*32 + l31 -> patch row of the pixel itself
};
template <int TH>
__device__ __forceinline__ BlockLane<TH> block_lane(int tiles_x, int tiles_y)
{
    using G = BlockGeom<TH>;
    BlockLane<TH> L;
    L.tid = threadIdx.x, L.lane = L.tid & 63;
    L.wave = __builtin_amdgcn_readfirstlane(L.tid >> 6);
    int t = xcd_logical_block();                                // XCD-aware order (conv.hip): neighbouring tiles share an L2
    const int tx = t % tiles_x;
    t /= tiles_x;
    const int ty = t % tiles_y;
    L.b = t / tiles_y;
    L.oy0 = ty * TH, L.ox0 = tx * G::TW;
    L.l31 = L.lane & 31, L.lhi = L.lane >> 5;
    L.wm = L.wave >> 1, L.wn = L.wave & 1;
    L.xmb = 4 + (L.wave >> 1), L.xnb = L.wave & 1;
    L.fswz = (L.l31 >> 1) & 7;
#pragma unroll
    for (int mi = 0; mi < G::MI; ++mi) {
        const int p = L.wm * (G::MI * 32) + mi * 32 + L.l31;
        L.crow[mi] = (p / G::TW + 1) * G::PW + (p % G::TW) + 1;
    }
    return L;
}

// ---- phase stamps of -DSMAP_TRACE builds (tools/trace_convb.py): start, set-up, phase 1, y1 written, phase 2, last store issued, stores retired
#ifdef SMAP_TRACE
struct BlockTrace { long long t[7]; };
#define TRB(tr, i) (tr).t[i] = __builtin_amdgcn_s_memtime()
#else
struct BlockTrace {};
#define TRB(tr, i)
#endif
__device__ __forceinline__ void block_trace_end(BlockTrace& tr, const ConvArgs& a, int tid)
{
#ifdef SMAP_TRACE
    TRB(tr, 5);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    TRB(tr, 6);
    if (a.dbg && tid == 0) {                                    // stamps of wave 0, and where it ran
        long long* d = a.dbg + (long long)blockIdx.x * 8;
        unsigned hwid;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
#pragma unroll
        for (int i = 0; i < 7; ++i) d[i] = tr.t[i];
        d[7] = hwid;
    }
#endif
}

// ---- ONE ring of 8 KiB weight slots behind y1, filled by LDS-DMA.  Slots 0 .. SB-1 are the kernel's own (none in the identity kernel), then
// the 18 of the 3x3 and the 8 of the tail.  src(s) = where slot s lies in global memory: the only per-kernel part.
// Protocol.  Slot s: [barrier: slot s is published, slot s-1's buffer is free] -> issue slot s + NS - 1 -> multiply -> WAIT for the next
// slot(s); younger ones stay in flight.  In phase 3 a chunk's two slots are waited for together at the end of the PREVIOUS chunk's
// multiplications, i.e. BEFORE that chunk's stores: a counted vmcnt also counts stores, and a wait that covers stores issued a moment ago
// costs a store round trip (csrc/convf.hip pays that once per chunk).
template <int TH, int SB_, class Src>
struct SlotRing {
    using G = BlockGeom<TH>;
    static constexpr int SB = SB_, NSLOT = SB + G::NS2 + G::NS3;
    char* base;                                                 // smem + Y1_BYTES
    int wave;
    unsigned wlane;                                             // this lane's 16 bytes of a wave's 1 KiB
    const Src& src;

    __device__ __forceinline__ void issue(int s) const
    {
        char* dst = base + (s % G::NS) * G::SLOT + wave * 1024;
        const char* g = src(s) + wlane;
#pragma unroll
        for (int i = 0; i < ((SMAP_CONVB_ABLATE & 8) ? 0 : G::LS); ++i) lds_dma16(g + i * 4096, dst + i * 4096);
    }
    __device__ __forceinline__ void prime() const
    {
#pragma unroll
        for (int s = 0; s < G::NS - 1; ++s) issue(s);
    }
    // the head of slot s's interval; returns the byte offset of the slot's 64 rows from `base`.  Readers add it LAST (base + row + granule +
    // offset): a compile-time constant at the end of the sum lands in the immediate field of ds_read_b128; folded into the base first, the
    // slots at 64 KiB and above cost an address instruction per read (24 - 40 of them per tile)
    __device__ __forceinline__ int enter(int s) const
    {
        lds_barrier_asm();
        if (s + G::NS - 1 < NSLOT) issue(s + G::NS - 1);
        return (s % G::NS) * G::SLOT;
    }
    // in slot `cur` (its issue done): slots <= upto have landed
    __device__ __forceinline__ void wait(int cur, int upto) const
    {
        if (upto >= NSLOT) upto = NSLOT - 1;
        const int issued = cur + G::NS - 1 < NSLOT ? cur + G::NS - 1 : NSLOT - 1;
        wait_vm((issued > upto ? issued - upto : 0) * G::LS);
    }
};
template <int TH, int SB, class Src>
__device__ __forceinline__ SlotRing<TH, SB, Src> slot_ring(char* smem, const BlockLane<TH>& L, const Src& src)
{
    return {smem + BlockGeom<TH>::Y1_BYTES, L.wave, (unsigned)(L.wave * 1024 + L.lane * 16), src};
}
// slot t2 of the 3x3 and the tail, counted from the first tap: tap t2 / 2, chunk t2 % 2 of W2 (conv3.hip's blocks are ordered
// [chunk][tap]); then W3's [tail chunk][k chunk]
template <int TH>
__device__ __forceinline__ const char* block_w23_slot(const ConvArgs& a, int t2)
{
    using G = BlockGeom<TH>;
    return t2 < G::NS2 ? reinterpret_cast<const char*>(a.w) + (long long)((t2 % G::KC2) * G::NTAP + t2 / G::KC2) * G::SLOT
                       : reinterpret_cast<const char*>(a.w2) + (long long)(t2 - G::NS2) * G::SLOT;
}

// ---- the leading 1x1.  b1 enters through the accumulators: an ordinary global load in the middle of the LDS-DMA pipeline would make hipcc
// drain the whole queue (vmcnt(0)) at its use, and these loads are the oldest of the kernel.
template <int TH>
__device__ __forceinline__ void block_b1_load(float4 (&b1raw)[BlockGeom<TH>::NB1][4], const ConvArgs& a, const BlockLane<TH>& L)
{
#pragma unroll
    for (int j = 0; j < BlockGeom<TH>::NB1; ++j) load_bias16(b1raw[j], a.bias0 + (j < 2 ? j : L.xnb) * 32 + 4 * L.lhi);
}
template <int TH>
__device__ __forceinline__ void block_acc1_start(f32x16 (&acc1)[BlockGeom<TH>::NB1], const float4 (&b1raw)[BlockGeom<TH>::NB1][4], const ConvArgs& a)
{
    const float inv0 = 1.f / a.acc_scale0;
#pragma unroll
    for (int j = 0; j < BlockGeom<TH>::NB1; ++j) acc_from_bias(acc1[j], b1raw[j], inv0);
}
// one 16-channel K step: sW = 64 weight rows, sX = the patch rows, both with a pitch of PITCH bytes; slot[plane] = byte offset of this
// lane's hi / lo granule in its rows.  Per block three MFMAs: small cross terms first, then hi*hi (conv3.hip's order).
template <int TH, int PITCH>
__device__ __forceinline__ void block_c1_step(f32x16 (&acc1)[BlockGeom<TH>::NB1], const char* sW, const char* sX, const int (&slot)[2],
                                              const BlockLane<TH>& L)
{
    constexpr int MB1 = BlockGeom<TH>::MB1, NB1 = BlockGeom<TH>::NB1;
    half8 wf[2][2], xf[2], xe[2];
#pragma unroll
    for (int pl = 0; pl < 2; ++pl) {
        wf[pl][0] = *reinterpret_cast<const half8*>(sW + L.l31 * PITCH + slot[pl]);
        wf[pl][1] = *reinterpret_cast<const half8*>(sW + (32 + L.l31) * PITCH + slot[pl]);
        xf[pl] = *reinterpret_cast<const half8*>(sX + (L.wave * 32 + L.l31) * PITCH + slot[pl]);
        if (MB1 == 6) xe[pl] = *reinterpret_cast<const half8*>(sX + (L.xmb * 32 + L.l31) * PITCH + slot[pl]);
    }
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
        acc1[nb] = block_mfma(wf[0][nb], xf[1], acc1[nb]);
        acc1[nb] = block_mfma(wf[1][nb], xf[0], acc1[nb]);
        acc1[nb] = block_mfma(wf[0][nb], xf[0], acc1[nb]);
    }
    if (MB1 == 6) {                                             // the extra block's channel half is wave-uniform: a scalar branch, no copy
        if (L.xnb) {
            acc1[NB1 - 1] = block_mfma(wf[0][1], xe[1], acc1[NB1 - 1]);
            acc1[NB1 - 1] = block_mfma(wf[1][1], xe[0], acc1[NB1 - 1]);
            acc1[NB1 - 1] = block_mfma(wf[0][1], xe[0], acc1[NB1 - 1]);
        } else {
            acc1[NB1 - 1] = block_mfma(wf[0][0], xe[1], acc1[NB1 - 1]);
            acc1[NB1 - 1] = block_mfma(wf[1][0], xe[0], acc1[NB1 - 1]);
            acc1[NB1 - 1] = block_mfma(wf[0][0], xe[0], acc1[NB1 - 1]);
        }
    }
}
// accumulators -> y1 [KC2][PROWS][128 B] at the start of the LDS (rows = patch pixels): acc1[j] = channel block nb of patch rows mb*32 + l31;
// rows outside the image are the 3x3's zero padding (the 3x3 pads y1, not x)
template <int TH>
__device__ __forceinline__ void block_put_y1(char* smem, const f32x16 (&acc1)[BlockGeom<TH>::NB1], const ConvArgs& a, const BlockLane<TH>& L)
{
    using G = BlockGeom<TH>;
#pragma unroll
    for (int j = 0; j < G::NB1; ++j) {
        const int nb = j < 2 ? j : L.xnb, prow = (j < 2 ? L.wave : L.xmb) * 32 + L.l31;
        put_row_hilo<false>(smem + nb * G::PROWS * G::ROWB, prow, L.lhi, acc1[j], a.acc_scale0, patch_row_live<G::PW, G::PH>(a, prow, L.oy0, L.ox0), nullptr);
    }
}

// ---- phase 2: the 3x3 as nine shifted views of y1, one ring slot per (tap, chunk); acc2[mi] = 32 output channels wn of pixel block mi
template <int TH, class Ring>
__device__ __forceinline__ void block_conv3x3(f32x16 (&acc2)[BlockGeom<TH>::MI], const char* smem, const Ring& ring, const BlockLane<TH>& L)
{
    using G = BlockGeom<TH>;
    constexpr int MI = G::MI;
    int prow0[MI];                                              // patch row of tap (0,0) of this lane's pixels
#pragma unroll
    for (int mi = 0; mi < MI; ++mi) prow0[mi] = L.crow[mi] - G::PW - 1;
    const int b_row0 = L.wn * (G::P / 2) + L.l31;               // this wave's 32 output channels of the 3x3
#pragma unroll
    for (int t2 = 0; t2 < G::NS2; ++t2) {
        const int s = Ring::SB + t2;
        const int sB = ring.enter(s);                           // slot s landed for every wave; y1 complete (first tap); slot s-1's buffer is free
        const int tap = t2 / G::KC2, cc = t2 % G::KC2;
        const int shift = (tap / 3) * G::PW + (tap % 3);
#pragma unroll
        for (int kk = 0; kk < G::CH / 16; ++kk) {
            const int g = kk * 2 + L.lhi;
            half8 af[2][MI], bf[2];
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    const int prow = prow0[mi] + shift;
                    af[pl][mi] = *reinterpret_cast<const half8*>(smem + (cc * G::PROWS + prow) * G::ROWB + (((g + 4 * pl) ^ ((prow >> 1) & 7)) << 4));
                }
                bf[pl] = *reinterpret_cast<const half8*>(ring.base + b_row0 * G::ROWB + (((g + 4 * pl) ^ L.fswz) << 4) + sB);
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                acc2[mi] = block_mfma(bf[0], af[1][mi], acc2[mi]);
                acc2[mi] = block_mfma(bf[1], af[0][mi], acc2[mi]);
                acc2[mi] = block_mfma(bf[0], af[0][mi], acc2[mi]);
            }
        }
        ring.wait(s, t2 + 1 < G::NS2 ? s + 1 : s + 2);          // the last tap also waits for both slots of the first tail chunk
    }
}
// accumulators -> y2 [KC2][BM][128 B] over y1 (rows = tile pixels).  acc2[mi][4*q + e] = channel wn*32 + 8*q + 4*lhi + e.  BIAS: b2 comes
// from the float table sB2 [P]; otherwise it entered through the accumulators.
template <int TH, bool BIAS>
__device__ __forceinline__ void block_put_y2(char* smem, const f32x16 (&acc2)[BlockGeom<TH>::MI], const ConvArgs& a, const BlockLane<TH>& L, const float* sB2)
{
    using G = BlockGeom<TH>;
#pragma unroll
    for (int mi = 0; mi < G::MI; ++mi)
        put_row_hilo<BIAS>(smem + L.wn * G::BM * G::ROWB, L.wm * (G::MI * 32) + mi * 32 + L.l31, L.lhi, acc2[mi], a.acc_scale, true,
                           BIAS ? sB2 + L.wn * 32 + 4 * L.lhi : nullptr);
}
// [C] tail bias / tail scale, one value per thread: the part of y1's region that y2 leaves free
template <int TH>
__device__ __forceinline__ float* block_b3_table(char* smem) { return reinterpret_cast<float*>(smem + BlockGeom<TH>::Y2_BYTES); }

// ---- phase 3, in three pieces; between them each kernel adds its own residual
// (a) tail chunk nc (64 output channels): acc3 starts at b3 / scale from the table, K = y2's two chunks, one ring slot each; ends with the
//     wait for the next chunk's slots, BEFORE this chunk's stores.  Rows = channels nc*64 + wn*32 + 8*q + 4*lhi + e.
template <int TH, class Ring>
__device__ __forceinline__ void block_tail_chunk(f32x16 (&acc3)[BlockGeom<TH>::MI], int nc, char* smem, const Ring& ring, const BlockLane<TH>& L)
{
    using G = BlockGeom<TH>;
    constexpr int MI = G::MI;
    const float* sB3 = block_b3_table<TH>(smem);
    const int p_row0 = L.wm * (MI * 32) + L.l31;                // + mi*32: pixel rows of y2
    const int c_row0 = L.wn * 32 + L.l31;                       // channel rows of a tail chunk
#pragma unroll
    for (int kc = 0; kc < G::KC2; ++kc) {
        const int s = Ring::SB + G::NS2 + nc * G::KC2 + kc;
        const int sW = ring.enter(s);                           // slot s landed for every wave; y2 + bias table complete (first slot); slot s-1's buffer is free
        if (kc == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 b4 = *reinterpret_cast<const float4*>(sB3 + nc * 64 + L.wn * 32 + 8 * q + 4 * L.lhi);
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    acc3[mi][4 * q + 0] = b4.x; acc3[mi][4 * q + 1] = b4.y; acc3[mi][4 * q + 2] = b4.z; acc3[mi][4 * q + 3] = b4.w;
                }
            }
        }
#pragma unroll
        for (int kk = 0; kk < G::CH / 16; ++kk) {
            const int g = kk * 2 + L.lhi;
            half8 pf[2][MI], wf[2];
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
                for (int mi = 0; mi < MI; ++mi)
                    pf[pl][mi] = *reinterpret_cast<const half8*>(smem + (kc * G::BM + p_row0 + mi * 32) * G::ROWB + (((g + 4 * pl) ^ L.fswz) << 4));
                wf[pl] = *reinterpret_cast<const half8*>(ring.base + c_row0 * G::ROWB + (((g + 4 * pl) ^ L.fswz) << 4) + sW);
            }
#pragma unroll
            for (int mi = 0; mi < MI; ++mi) {
                acc3[mi] = block_mfma(wf[0], pf[1][mi], acc3[mi]);
                acc3[mi] = block_mfma(wf[1], pf[0][mi], acc3[mi]);
                acc3[mi] = block_mfma(wf[0], pf[0][mi], acc3[mi]);
            }
        }
        if (kc == G::KC2 - 1) ring.wait(s, s + 2);              // both slots of the next chunk, BEFORE this chunk's stores
    }
}
// (b) register epilogue (convp.hip): half-wave swap -> acc3[mi][8*j .. 8*j+7] = channels nc*64 + wn*32 + 8*lhi + 16*j .. +7 of the pixel,
//     in output units (the bias is inside)
template <int TH>
__device__ __forceinline__ void block_swap_scale(f32x16 (&acc3)[BlockGeom<TH>::MI], const ConvArgs& a)
{
#pragma unroll
    for (int mi = 0; mi < BlockGeom<TH>::MI; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float2 sw = halfwave_swap(acc3[mi][8 * j + e], acc3[mi][8 * j + 4 + e]);
                acc3[mi][8 * j + e] = a.tail_acc_scale * sw.x;
                acc3[mi][8 * j + 4 + e] = a.tail_acc_scale * sw.y;
            }
}
// (c) ReLU, the post-ReLU skip adds of the last block of a layer, 16-byte NHWC stores of both planes
template <int TH>
__device__ __forceinline__ void block_store_chunk(f32x16 (&acc3)[BlockGeom<TH>::MI], int nc, const ConvArgs& a, const BlockLane<TH>& L,
                                                  const bool (&m_ok)[BlockGeom<TH>::MI], const unsigned (&m_dense)[BlockGeom<TH>::MI],
                                                  const unsigned (&m_out)[BlockGeom<TH>::MI])
{
    constexpr int MI = BlockGeom<TH>::MI;
    const int n_lane = nc * 64 + L.wn * 32 + 8 * L.lhi;
    if (a.relu) {
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) relu16(acc3[mi]);
    }
    auto add_tensor = [&](const _Float16* __restrict__ tsr) {
        half8 h[MI][2][2];
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    h[mi][j][pl] = *reinterpret_cast<const half8*>(tsr + m_dense[mi] + (unsigned)(n_lane + 16 * j) + pl * a.tail_cout8);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int j = 0; j < 2; ++j) add_planes8(acc3[mi], j, h[mi][j]);
    };
    if (a.add1) add_tensor(a.add1);
    if (a.add2) add_tensor(a.add2);
    _Float16* __restrict__ outp = reinterpret_cast<_Float16*>(a.out);
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (!m_ok[mi]) continue;
            _Float16* op = outp + (m_out[mi] + (unsigned)(n_lane + 16 * j));
            half8 h, l;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                h[e] = (_Float16)acc3[mi][8 * j + e];
                l[e] = (_Float16)(acc3[mi][8 * j + e] - (float)h[e]);
            }
            if (SMAP_CONVB_ABLATE & 4) { if (h[0] == (_Float16)123.25f && l[1] == (_Float16)77.5f) *reinterpret_cast<half8*>(op) = h; continue; }   // keep the values live
            *reinterpret_cast<half8*>(op) = h;
            *reinterpret_cast<half8*>(op + a.out_lo) = l;
        }
}

}  // namespace
