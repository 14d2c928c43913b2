// convb.hip -- a whole stride-1 Bottleneck of 64 planes (model/smap.py:48-77) in ONE launch, split precision:
//     y1 = relu(W1 x + b1)            1x1, C_in -> P        (conv_bn_relu1)
//     y2 = relu(W2 * y1 + b2)         3x3 pad 1, P -> P     (conv_bn_relu2)
//     out = relu(W3 y2 + b3 + r)      1x1, P -> C = 4P, + the residual r (+ the two skip adds of smap.py:142-153)
// Two kernels: bottleneck_kernel runs the identity blocks (C_in = C, r = x, the block's input), bottleneck_first_kernel a layer's first block
// (C_in = P, r = Wd x + bd, the shortcut conv).
//
// Why: as three launches the identity block moves 4096 bytes per pixel through the fabric (x read by c1, y1 written and read, y2 written
// and read, x read again as the residual, out written) and every launch of these layers sits on the HBM read+write roof
// (DESIGN.md section 6).  Here x is read ONCE and out written once: 2048 bytes per pixel.  y1 and y2 never leave the CU, and the
// residual never leaves it either: while the K chunks of x pass through the LDS staging buffers of the leading 1x1, every wave
// copies the centre pixels' values it will need in the last epilogue into registers (the register file holds the 64 KB / 128 KB
// an LDS that is full of y1 cannot).
//
// Work per workgroup (4 waves, 80 KiB of LDS, two workgroups per CU so that one streams x while the other multiplies):
// a TH x 16 tile of output pixels (TH = 4 | 8).
//   phase 1  c1 on the (TH+2) x 18 halo patch (rows of the patch = GEMM rows, rounded up to PROWS = 128 | 192); accumulators -> relu ->
//            hi/lo -> y1 in conv3.hip's patch layout, rows outside the image forced to 0 (the 3x3 pads y1, not x).  The halo is recomputed:
//            +41 % (+69 %) of c1 = +10 % (+16 %) MFMA work.
//            Identity kernel: K = C in 16-channel stages, each staged as [PROWS][hi16 | lo16] (x) + [P][hi16 | lo16] (W1) by LDS-DMA in a
//            ring of 6 | 5 stages over the WHOLE 80 KiB (y1 does not exist yet; x comes from HBM: depth is what this phase lives on).
//            First-block kernel: K = 64, the x patch is loaded once into the region y1 will take over, W1 and the shortcut conv's
//            weights come through the slot ring; the shortcut conv runs on the tile's own pixels and stays in accumulators.
//   phase 2  the 3x3 as nine shifted views of y1 (conv3.hip), one 8 KiB weight slot per (tap, 32-channel chunk) in a ring
//            behind y1; accumulators -> relu -> hi/lo -> y2, written over y1 once every wave is done with it.
//   phase 3  the tail 1x1 in four chunks of 64 output channels (weight slots in the same ring) with convp.hip's register
//            epilogue: permlane32_swap -> 8 consecutive channels per lane, + the residual held since phase 1, ReLU, skip adds,
//            16-byte NHWC stores of both planes.
// MFMA operand order is weights FIRST everywhere (D rows = channels, columns = pixels): a lane then owns 4 consecutive
// channels of one pixel, which is what the hi/lo writes into LDS and the register epilogue want.
//
// Where the code is: everything the two kernels have in common -- geometry (BlockGeom), tile decode (BlockLane), the slot ring, the K step
// of the leading 1x1, the y1 / y2 write-backs, phase 2, the three pieces of phase 3, the trace stamps, and the SMAP_CONVB_LDS_KB /
// SMAP_CONVB_ABLATE switches -- is csrc/block_device.h, once.  This file keeps what differs: how x reaches the LDS, the phase-1 loops, the
// residual, where b2 enters, and which weights the ring's slots hold.
//
// Weights (smap_amd/engine.py::Graph.conv_block, all three in pack_halo_rows' format: 128-byte rows = [hi32 | lo32] of one
// 32-channel chunk, slot s of row r = logical granule s ^ ((r >> 1) & 7)):
//   W2  [2 chunks][9 taps][64 rows]            W3  [4 n chunks][2 chunks][64 rows]
// and W1 of the identity kernel in 16-channel stages (engine.pack_rows16): [16 stages][64 rows][64 B = hi16 | lo16], slot s of row r =
// granule s ^ ((r >> 2) & 3).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "smap_hip.h"
#include "plan.h"
#include "block_device.h"

namespace {

template <int TH>
__global__ __launch_bounds__(256, 2) void bottleneck_kernel(const ConvArgs a, int tiles_x, int tiles_y)
{
    using G = BlockGeom<TH>;
    constexpr int P = G::P, C = G::C, PW = G::PW, PH = G::PH, PROWS = G::PROWS, NB1 = G::NB1, MI = G::MI, NCH3 = G::NCH3;
    // phase 1 stages 16 channels at a time (64-byte rows [hi16 | lo16], one MFMA K step per stage): a 12 | 16 KiB stage, so that
    // 5 | 4 of them are in flight behind the one being multiplied -- x comes from HBM, and with 32-channel stages (3 | 2 of them in
    // 80 KiB) a workgroup waited a full memory latency per stage (profiles/r4_v2_*: 172 us per block)
    constexpr int CH1 = 16, ROW1 = 64, KS1 = C / CH1;           // 16 stages
    constexpr int XS = PROWS * ROW1, WS1 = P * ROW1;            // phase-1 stage = x rows (8 | 12 KiB) + W1 rows (4 KiB)
    constexpr int ST1 = XS + WS1;
    constexpr int NS1 = G::LDS_BYTES / ST1;                     // stages: 6 | 5
    constexpr int LA = XS / 4096, LB1 = WS1 / 4096, LPT1 = LA + LB1;   // LDS-DMA instructions per thread and stage: 2 | 3, + 1
    static_assert(NS1 >= 2 && NS1 * ST1 <= G::LDS_BYTES, "LDS plan of phase 1");
    __shared__ __attribute__((aligned(16))) char smem[G::LDS_BYTES];   // ONE array: a second __shared__ object makes hipcc drain vmcnt

    SMAP_TL_BEGIN
    BlockTrace tr;
    TRB(tr, 0);
    const BlockLane<TH> L = block_lane<TH>(tiles_x, tiles_y);
    const int tid = L.tid, lane = L.lane, wave = L.wave, l31 = L.l31, lhi = L.lhi, wn = L.wn;

    // ================================================================= phase 1: y1 = relu(W1 x + b1) on the halo patch
    const char* __restrict__ arena = reinterpret_cast<const char*>(a.arena);
    const char* __restrict__ w1g = reinterpret_cast<const char*>(a.w0);
    // a wave-wide LDS-DMA covers 16 rows x 64 B: lane -> row lane / 4, 16-byte slot lane % 4; slot s of row r holds logical granule
    // s ^ ((r >> 2) & 3) (0, 1 = hi channels 0..7, 8..15 of the stage; 2, 3 = lo): conflict-free ds_read_b128 (conv.hip, BK = 32)
    const int srow = wave * 16 + (lane >> 2);
    const int gl = (lane & 3) ^ ((srow >> 2) & 3);
    unsigned a_off[LA];                                         // patch row -> byte offset of its granule (0 = zero page)
#pragma unroll
    for (int i = 0; i < LA; ++i) {
        const int prow = i * 64 + srow;
        const int py = prow / PW, px = prow - py * PW;
        const int iy = L.oy0 - 1 + py, ix = L.ox0 - 1 + px;
        a_off[i] = 0;
        if (prow < PH * PW && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
            const long long e = ((long long)(L.b * a.H + iy) * a.W + ix) * a.in_stride_c + (gl & 1) * 8 + (gl >> 1) * a.in_lo;
            a_off[i] = (unsigned)(a.in_off + e * 2);
        }
    }
    auto issue1 = [&](int st, int ks) {                         // stage st <- channels 16 ks .. +15 of x and of W1
        char* sX = smem + st * ST1;
        const char* gA = arena + (unsigned)(ks * CH1 * 2);      // invalid rows: zero page + stage offset
#pragma unroll
        for (int i = 0; i < ((SMAP_CONVB_ABLATE & 1) ? 0 : LA); ++i)
            lds_dma16(gA + a_off[i], sX + (i * 64 + wave * 16) * ROW1);
        const char* gW = w1g + (long long)ks * WS1 + (unsigned)(wave * 1024 + lane * 16);
#pragma unroll
        for (int i = 0; i < ((SMAP_CONVB_ABLATE & 8) ? 0 : LB1); ++i)
            lds_dma16(gW + i * 4096, sX + XS + i * 4096 + wave * 1024);
    };
    // the residual of the last epilogue, collected while x passes through LDS: rs[nc][mi][j][plane] = channels
    // nc*64 + wn*32 + 16*j + 8*lhi .. +7 of pixel (mi, l31) -- the layout the register epilogue of phase 3 ends in
    half8 rs[NCH3][MI][2][2];

    // Biases enter through the ACCUMULATORS (block_device.h): b1 here, b2 during the last K chunk, b3 via a 1 KiB table in LDS.
    float4 b1raw[NB1][4];
    block_b1_load<TH>(b1raw, a, L);
    const float b3_mine = a.bias2[tid];                         // tail bias: one value per thread, parked until the table can be written
#pragma unroll
    for (int st = 0; st < NS1 - 1; ++st) issue1(st, st);        // the first stages go out behind the bias loads
    f32x16 acc1[NB1];
    block_acc1_start<TH>(acc1, b1raw, a);
    TRB(tr, 1);

    const int fs4 = (l31 >> 2) & 3;                             // (row >> 2) & 3 of every phase-1 fragment row = multiple of 32 + l31
    const int slot1[2] = {(lhi ^ fs4) << 4, ((lhi + 2) ^ fs4) << 4};   // hi | lo granule of this lane's K half
#pragma unroll
    for (int ks = 0; ks < KS1; ++ks) {
        if (ks + NS1 - 1 <= KS1) wait_vm((NS1 - 2) * LPT1);     // stage ks has landed; younger stages stay in flight
        else wait_vm((KS1 - 1 - ks) * LPT1);
        lds_barrier_asm();
        if (ks + NS1 - 1 < KS1) issue1((ks + NS1 - 1) % NS1, ks + NS1 - 1);     // into the buffer stage ks-1 was read from
        const char* sX = smem + (ks % NS1) * ST1;
        if (((ks >> 1) & 1) == wn) {                            // this wave's residual channels: nc*64 + wn*32 + 16*j + 8*lhi .. = stage 4 nc + 2 wn + j
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl)
                    rs[ks >> 2][mi][ks & 1][pl] = *reinterpret_cast<const half8*>(
                        sX + L.crow[mi] * ROW1 + (((lhi + 2 * pl) ^ ((L.crow[mi] >> 2) & 3)) << 4));
        }
        block_c1_step<TH, ROW1>(acc1, sX + XS, sX, slot1, L);
    }
    lds_barrier_asm();                                          // every wave is done with the staging buffers (all DMA has landed)
    TRB(tr, 2);
    // phase 2's accumulators start at b2 / scale: the loads go out now, ahead of the first weight slots, and are consumed after
    // y1 has been written (the wait hipcc puts there covers slot 0, which is needed then anyway)
    float4 b2v[4];
    load_bias16(b2v, a.bias + wn * 32 + 4 * lhi);

    const auto slot_src = [&](int s) { return block_w23_slot<TH>(a, s); };     // the 3x3's slots, then the tail's: no slots of its own
    const auto ring = slot_ring<TH, 0>(smem, L, slot_src);
    ring.prime();
    block_put_y1<TH>(smem, acc1, a, L);
    f32x16 acc2[MI];
    {
        const float inv = 1.f / a.acc_scale;
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) acc_from_bias(acc2[mi], b2v, inv);
    }
    wait_vm((G::NS - 2) * G::LS);                               // slot 0 (only slots 0 .. NS-2 are issued)
    TRB(tr, 3);

    // ================================================================= phase 2: the 3x3 on y1
    block_conv3x3<TH>(acc2, smem, ring, L);
    lds_barrier_asm();                                          // every wave is done with y1: y2 may overwrite it
    TRB(tr, 4);
    block_put_y2<TH, false>(smem, acc2, a, L, nullptr);         // (b2 inside)
    block_b3_table<TH>(smem)[tid] = b3_mine * (1.f / a.tail_acc_scale);

    // ================================================================= phase 3: the tail 1x1 + residual + ReLU (+ skip adds)
    unsigned m_dense[MI], m_out[MI];
    bool m_ok[MI];
    pixel_offsets<MI, G::TW>(m_ok, m_dense, m_out, a, L.b, L.oy0, L.ox0, L.wm * (MI * 32) + l31);
#pragma unroll
    for (int nc = 0; nc < NCH3; ++nc) {
        f32x16 acc3[MI];
        block_tail_chunk<TH>(acc3, nc, smem, ring, L);
        block_swap_scale<TH>(acc3, a);
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)                         // + x, from the registers filled in phase 1
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc3[mi][8 * j + e] += (float)rs[nc][mi][j][0][e] + (float)rs[nc][mi][j][1][e];
        block_store_chunk<TH>(acc3, nc, a, L, m_ok, m_dense, m_out);
    }
    block_trace_end(tr, a, tid);
    SMAP_TL_END(a)
}

template <int TH>
__global__ __launch_bounds__(256, 2) void bottleneck_first_kernel(const ConvArgs a, int tiles_x, int tiles_y)
{
    using G = BlockGeom<TH>;
    constexpr int P = G::P, C = G::C, CH = G::CH, ROWB = G::ROWB, PW = G::PW, PH = G::PH, PROWS = G::PROWS, NB1 = G::NB1, MI = G::MI;
    constexpr int KC2 = G::KC2, NCH3 = G::NCH3, SLOT = G::SLOT;
    constexpr int S1 = KC2, SD = NCH3 * KC2, SB = S1 + SD;      // in front of the 3x3's slots: 2 chunks of W1, 8 (chunk, k chunk) slots of the shortcut conv
    constexpr int LX = PROWS / 32;                              // LDS-DMA instructions per thread and 32-channel chunk of the x patch
    __shared__ __attribute__((aligned(16))) char smem[G::LDS_BYTES];   // ONE array: a second __shared__ object makes hipcc drain vmcnt

    SMAP_TL_BEGIN
    BlockTrace tr;
    TRB(tr, 0);
    const BlockLane<TH> L = block_lane<TH>(tiles_x, tiles_y);
    const int tid = L.tid, lane = L.lane, wave = L.wave, l31 = L.l31, lhi = L.lhi, wn = L.wn;

    // ================================================================= the x patch: C_in = 64 channels = two 32-channel chunks, loaded ONCE
    // into the region y1 will take over: [KC2][PROWS][128 B], conv3.hip's patch format (slot s of row r = granule s ^ ((r >> 1) & 7))
    const char* __restrict__ arena = reinterpret_cast<const char*>(a.arena);
    char* sX = smem;
    {
        const int lrow = lane >> 3, lslot = lane & 7;
        const int srow = wave * 8 + lrow;
        const int gl = lslot ^ ((srow >> 1) & 7);               // logical granule this lane fetches: 0..3 hi, 4..7 lo
#pragma unroll
        for (int i = 0; i < LX; ++i) {
            const int prow = i * 32 + srow;
            const int py = prow / PW, px = prow - py * PW;
            const int iy = L.oy0 - 1 + py, ix = L.ox0 - 1 + px;
            unsigned off = 0;                                   // 0 = zero page
            if (prow < PH * PW && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
                const long long e = ((long long)(L.b * a.H + iy) * a.W + ix) * a.in_stride_c + (gl & 3) * 8 + (gl >> 2) * a.in_lo;
                off = (unsigned)(a.in_off + e * 2);
            }
#pragma unroll
            for (int cc = 0; cc < KC2; ++cc)
                lds_dma16(arena + (unsigned)(cc * CH * 2) + off, sX + (cc * PROWS + i * 32 + wave * 8) * ROWB);
        }
    }
    // biases: b1 through the accumulators (its loads are the oldest of the kernel); b2 and the tail bias (b3 + the shortcut's)
    // one value per thread, parked in a register until a table in LDS can take them (after phase 2)
    float4 b1raw[NB1][4];
    block_b1_load<TH>(b1raw, a, L);
    const float b3_mine = a.bias2[tid];
    const float b2_mine = a.bias[tid & (P - 1)];
    // ---- the slot ring runs through the whole kernel, started before anything else.  Its own slots: W1 chunk s | shortcut [n chunk][k chunk]
    const auto slot_src = [&](int s) {
        return s < S1 ? reinterpret_cast<const char*>(a.w0) + (long long)s * SLOT
             : s < SB ? reinterpret_cast<const char*>(a.wd) + (long long)(s - S1) * SLOT : block_w23_slot<TH>(a, s - SB);
    };
    const auto ring = slot_ring<TH, SB>(smem, L, slot_src);
    ring.prime();
    f32x16 acc1[NB1];
    block_acc1_start<TH>(acc1, b1raw, a);
    wait_vm((G::NS - 2) * G::LS);                               // the x patch and slot 0 (older than slots 1 .. NS-2)
    TRB(tr, 1);
    // ================================================================= phase 1a: y1 = relu(W1 x + b1) on the halo patch (K = 64: two slots)
#pragma unroll
    for (int s = 0; s < S1; ++s) {
        const char* sW = ring.base + ring.enter(s);
#pragma unroll
        for (int kk = 0; kk < CH / 16; ++kk) {
            const int slot[2] = {((kk * 2 + lhi) ^ L.fswz) << 4, ((kk * 2 + lhi + 4) ^ L.fswz) << 4};
            block_c1_step<TH, ROWB>(acc1, sW, sX + s * PROWS * ROWB, slot, L);
        }
        ring.wait(s, s + 1);
    }
    // ================================================================= phase 1b: the shortcut conv Wd x on the tile's own pixels (1x1, 64 -> 256,
    // no ReLU): kept in the accumulators until the last epilogue -- where an identity block keeps x itself (its residual)
    const int c_row0 = wn * 32 + l31;                           // channel rows of a 64-channel chunk
    f32x16 accd[NCH3][MI];
#pragma unroll
    for (int nc = 0; nc < NCH3; ++nc)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi)
#pragma unroll
            for (int r = 0; r < 16; ++r) accd[nc][mi][r] = 0.f;
#pragma unroll
    for (int nc = 0; nc < NCH3; ++nc)
#pragma unroll
        for (int kc = 0; kc < KC2; ++kc) {
            const int s = S1 + nc * KC2 + kc;
            const int sW = ring.enter(s);                       // (the slot's offset goes last: SlotRing::enter)
#pragma unroll
            for (int kk = 0; kk < CH / 16; ++kk) {
                const int g = kk * 2 + lhi;
                half8 pf[2][MI], wf[2];
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
                    for (int mi = 0; mi < MI; ++mi)
                        pf[pl][mi] = *reinterpret_cast<const half8*>(sX + (kc * PROWS + L.crow[mi]) * ROWB + (((g + 4 * pl) ^ ((L.crow[mi] >> 1) & 7)) << 4));
                    wf[pl] = *reinterpret_cast<const half8*>(ring.base + c_row0 * ROWB + (((g + 4 * pl) ^ L.fswz) << 4) + sW);
                }
#pragma unroll
                for (int mi = 0; mi < MI; ++mi) {
                    accd[nc][mi] = block_mfma(wf[0], pf[1][mi], accd[nc][mi]);
                    accd[nc][mi] = block_mfma(wf[1], pf[0][mi], accd[nc][mi]);
                    accd[nc][mi] = block_mfma(wf[0], pf[0][mi], accd[nc][mi]);
                }
            }
            ring.wait(s, s + 1);
        }
    lds_barrier_asm();                                          // every wave is done with the x patch: y1 takes its place
    TRB(tr, 2);
    block_put_y1<TH>(smem, acc1, a, L);
    f32x16 acc2[MI];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[mi][r] = 0.f;
    TRB(tr, 3);

    // ================================================================= phase 2: the 3x3 on y1
    block_conv3x3<TH>(acc2, smem, ring, L);
    lds_barrier_asm();                                          // every wave is done with y1: y2 may overwrite it
    TRB(tr, 4);

    // ---- bias tables in the part of y1's region that y2 leaves free: [C] (b3 + shortcut bias) / tail scale, [P] b2
    float* sB3 = block_b3_table<TH>(smem);
    float* sB2 = sB3 + C;
    sB3[tid] = b3_mine * (1.f / a.tail_acc_scale);
    if (tid < P) sB2[tid] = b2_mine;
    lds_barrier_asm();
    block_put_y2<TH, true>(smem, acc2, a, L, sB2);

    // ================================================================= phase 3: the tail 1x1 + residual + ReLU (+ skip adds)
    unsigned m_dense[MI], m_out[MI];
    bool m_ok[MI];
    pixel_offsets<MI, G::TW>(m_ok, m_dense, m_out, a, L.b, L.oy0, L.ox0, L.wm * (MI * 32) + l31);
#pragma unroll
    for (int nc = 0; nc < NCH3; ++nc) {
        f32x16 acc3[MI];
        block_tail_chunk<TH>(acc3, nc, smem, ring, L);
        {                                                       // + the shortcut conv's accumulators (same lane layout), in units of the tail's scale
            const float rsd = a.acc_scale_d / a.tail_acc_scale;
#pragma unroll
            for (int mi = 0; mi < MI; ++mi)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc3[mi][r] += rsd * accd[nc][mi][r];
        }
        block_swap_scale<TH>(acc3, a);
        block_store_chunk<TH>(acc3, nc, a, L, m_ok, m_dense, m_out);
    }
    block_trace_end(tr, a, tid);
    SMAP_TL_END(a)
}

// TILE: the row of csrc/tiles.h; its BM = TH rows of 16 pixels, `first` selects the kernel with the shortcut conv
template <int TILE>
hipError_t launchb(const ConvArgs& a, hipStream_t st)
{
    constexpr TileRow t = tile_row(TILE);
    static_assert(t.family == TF_BLOCK && t.planes == 64 && t.tail_bn == 64 && t.bm % 16 == 0, "csrc/tiles.h: not a 64-plane whole-block tile id");
    constexpr int TH = t.bm / 16;
    if (!a.x3 || a.ksize != 3 || a.stride != 1 || a.pad != 1 || a.up || a.out_fp32 || !a.w0 || !a.w2 || a.Cin != t.planes ||
        a.tail_cout8 != 4 * t.planes || a.H != a.Ho || a.W != a.Wo)
        return hipErrorInvalidValue;
    if (t.first ? (a.head_cin != t.planes || !a.wd || a.res || a.add1 || a.add2) : (a.head_cin != 4 * t.planes || a.wd)) return hipErrorInvalidValue;
    const int B = a.M / (a.Ho * a.Wo);
    const int tiles_x = (a.Wo + 15) / 16, tiles_y = (a.Ho + TH - 1) / TH;
    if (t.first) hipLaunchKernelGGL((bottleneck_first_kernel<TH>), dim3(tiles_x * tiles_y * B), dim3(256), 0, st, a, tiles_x, tiles_y);
    else hipLaunchKernelGGL((bottleneck_kernel<TH>), dim3(tiles_x * tiles_y * B), dim3(256), 0, st, a, tiles_x, tiles_y);
    return hipGetLastError();
}

}  // namespace

// tools only (not part of include/smap_hip.h; exported from diagnostics builds with -DSMAP_DEBUG_EXPORTS, tools/build_ablate.py): resident
// workgroups per CU the runtime reports for a tile id's kernel
extern "C" __attribute__((visibility("default"))) int smap_debug_convb_occupancy(int tile);
#ifdef SMAP_DEBUG_EXPORTS
extern "C" int smap_debug_convb_occupancy(int tile)
{
    int n = -1;
    hipError_t e = hipErrorInvalidValue;
    switch (tile) {
        case 90: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, bottleneck_kernel<4>, 256, 0); break;
        case 91: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, bottleneck_kernel<8>, 256, 0); break;
        case 92: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, bottleneck_first_kernel<4>, 256, 0); break;
        case 93: e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, bottleneck_first_kernel<8>, 256, 0); break;
        default: break;
    }
    return e == hipSuccess ? n : -1000 - (int)e;
}
#endif

hipError_t smap_launch_convb(const ConvArgs& a, int tile, hipStream_t st)
{
    switch (tile) {
        case 90: return launchb<90>(a, st);
        case 91: return launchb<91>(a, st);
        case 92: return launchb<92>(a, st);
        case 93: return launchb<93>(a, st);
        case 94: return smap_launch_convc(a, st);       // 128 planes: csrc/convc.hip
        default: return hipErrorInvalidValue;
    }
}
