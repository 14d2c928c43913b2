// jpeg.hip -- the per-pixel half of the JPEG decode on gfx950 (include/smap_hip.h "JPEG decode"; the host half is csrc/jpeg_host.cpp).
//
// Launch (a) idct_kernel: dequantise + libjpeg's ISLOW inverse DCT (jidctint.c), one 8x8 block per wavefront, one lane per sample.
//   jidctint's two passes are the same 1-D butterfly of integer multiplies and adds followed by ONE rounding shift (11 bits after the
//   columns, 18 after the rows).  Before that shift a pass is therefore an exact integer matrix product, whatever the evaluation order:
//   c_idct below is the butterfly applied to the unit vectors (computed at compile time from the butterfly itself), and each lane takes
//   an 8-term dot product per pass through LDS.  int32 throughout, as libjpeg-turbo's SIMD path (dequantised values that overflow
//   int16 make libjpeg-turbo's own C and SIMD paths disagree: crafted files only, not followed here).
// Launch (b) color_kernel: one thread per output pixel -- libjpeg's "fancy" chroma upsampling (jdsample.c h2v1 / h2v2, triangle
//   filters, replicating the first / last real chroma row and column; planes at most 2 samples wide take the replicating path, as
//   libjpeg-turbo does), YCbCr -> RGB of jdcolor.c (SCALEBITS 16, arithmetic shifts, clamp), stored B, G, R with the EXIF orientation
//   applied as PIL's exif_transpose does.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "smap_hip.h"
#include "hip_rc.h"

namespace {

struct IdctMatrix { int32_t m[8][8]; };

// jidctint.c's 1-D butterfly (pass 1 and pass 2 are the same), everything before the descale
constexpr void butterfly(const int64_t* in, int64_t* out) {
    int64_t z2 = in[2], z3 = in[6];
    int64_t z1 = (z2 + z3) * 4433;                       // FIX_0_541196100
    int64_t tmp2 = z1 + z3 * -15137;                     // FIX_1_847759065
    int64_t tmp3 = z1 + z2 * 6270;                       // FIX_0_765366865
    z2 = in[0];
    z3 = in[4];
    int64_t tmp0 = (z2 + z3) * 8192, tmp1 = (z2 - z3) * 8192;          // << CONST_BITS
    int64_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = in[7]; tmp1 = in[5]; tmp2 = in[3]; tmp3 = in[1];
    z1 = tmp0 + tmp3;
    z2 = tmp1 + tmp2;
    z3 = tmp0 + tmp2;
    int64_t z4 = tmp1 + tmp3;
    int64_t z5 = (z3 + z4) * 9633;                       // FIX_1_175875602
    tmp0 *= 2446;                                        // FIX_0_298631336
    tmp1 *= 16819;                                       // FIX_2_053119869
    tmp2 *= 25172;                                       // FIX_3_072711026
    tmp3 *= 12299;                                       // FIX_1_501321110
    z1 *= -7373;                                         // FIX_0_899976223
    z2 *= -20995;                                        // FIX_2_562915447
    z3 *= -16069;                                        // FIX_1_961570560
    z4 *= -3196;                                         // FIX_0_390180644
    z3 += z5;
    z4 += z5;
    tmp0 += z1 + z3;
    tmp1 += z2 + z4;
    tmp2 += z2 + z3;
    tmp3 += z1 + z4;
    out[0] = tmp10 + tmp3; out[7] = tmp10 - tmp3;
    out[1] = tmp11 + tmp2; out[6] = tmp11 - tmp2;
    out[2] = tmp12 + tmp1; out[5] = tmp12 - tmp1;
    out[3] = tmp13 + tmp0; out[4] = tmp13 - tmp0;
}

constexpr IdctMatrix make_idct() {
    IdctMatrix r{};
    for (int j = 0; j < 8; ++j) {
        int64_t in[8] = {0, 0, 0, 0, 0, 0, 0, 0}, out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        in[j] = 1;
        butterfly(in, out);
        for (int k = 0; k < 8; ++k) r.m[k][j] = int32_t(out[k]);
    }
    return r;
}

__constant__ IdctMatrix c_idct = make_idct();

struct IdctArgs {
    int32_t ncomp;
    int32_t blocks_w[3];
    int64_t first_block[3];          // global block index of each component's first block
    int64_t n_blocks;
    uint16_t quant[3][64];
};

constexpr int kBlocksPerGroup = 4;   // 256 threads: 4 wavefronts, one block each

// rounding right shift of an int32 held as uint32 (wrap-around arithmetic: no signed overflow for crafted data)
__device__ inline int32_t descale(uint32_t x, int n) { return int32_t(x + (1u << (n - 1))) >> n; }

__global__ __launch_bounds__(256) void idct_kernel(const int16_t* __restrict__ coeffs, uint8_t* __restrict__ planes, IdctArgs a) {
    __shared__ int32_t s_in[kBlocksPerGroup][64];
    __shared__ int32_t s_ws[kBlocksPerGroup][64];
    const int w = threadIdx.x >> 6, t = threadIdx.x & 63, r = t >> 3, c = t & 7;
    const int64_t g = int64_t(blockIdx.x) * kBlocksPerGroup + w;
    const bool live = g < a.n_blocks;
    int comp = 0;
    if (live) {
        comp = (a.ncomp > 1 && g >= a.first_block[1]) + (a.ncomp > 2 && g >= a.first_block[2]);
        s_in[w][t] = int32_t(uint32_t(int32_t(coeffs[g * 64 + t])) * a.quant[comp][t]);     // natural order: t = row * 8 + column
    }
    __syncthreads();
    if (live) {                                          // pass 1: columns (vertical frequencies), descale by CONST_BITS - PASS1_BITS
        uint32_t acc = 0;
#pragma unroll
        for (int v = 0; v < 8; ++v) acc += uint32_t(c_idct.m[r][v]) * uint32_t(s_in[w][v * 8 + c]);
        s_ws[w][t] = descale(acc, 11);
    }
    __syncthreads();
    if (live) {                                          // pass 2: rows, descale by CONST_BITS + PASS1_BITS + 3, + 128, clamp
        uint32_t acc = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += uint32_t(c_idct.m[c][u]) * uint32_t(s_ws[w][r * 8 + u]);
        int v = descale(acc, 18) + 128;
        v = v < 0 ? 0 : v > 255 ? 255 : v;
        const int64_t lb = g - a.first_block[comp];
        const int bw = a.blocks_w[comp];
        const int64_t by = lb / bw, bx = lb - by * bw;
        // planes are laid out like the coefficients: component c's plane starts at byte first_block[c] * 64, row pitch bw * 8
        planes[a.first_block[comp] * 64 + (by * 8 + r) * (int64_t(bw) * 8) + bx * 8 + c] = uint8_t(v);
    }
}

struct ColorArgs {
    int32_t width, height;           // stored image
    int32_t out_w, out_h;            // after the orientation
    int32_t orientation;
    int32_t mode;                    // 0 grey, 1 4:4:4, 2 4:2:2 (h2v1), 3 4:2:0 (h2v2)
    int32_t fancy;                   // chroma wider than 2 samples: triangle filter; else replication
    int32_t cw, ch;                  // real chroma width / height (ceil of the luma's over the sampling factors)
    int64_t plane_off[3];
    int32_t pitch[3];
};

__device__ inline int chroma_h2v1(const uint8_t* row, int sx, int cw, bool fancy) {
    const int j = sx >> 1;
    const int v = row[j];
    if (!fancy) return v;
    if ((sx & 1) == 0) return j == 0 ? v : (3 * v + row[j - 1] + 1) >> 2;
    return j == cw - 1 ? v : (3 * v + row[j + 1] + 2) >> 2;
}

__device__ inline int chroma_h2v2(const uint8_t* plane, int pitch, int sy, int sx, int cw, int ch, bool fancy) {
    const int i = sy >> 1, j = sx >> 1;
    if (!fancy) return plane[int64_t(i) * pitch + j];
    int f = (sy & 1) ? i + 1 : i - 1;                    // the farther chroma row, the real edge rows replicated
    f = f < 0 ? 0 : f > ch - 1 ? ch - 1 : f;
    const uint8_t* near = plane + int64_t(i) * pitch;
    const uint8_t* far = plane + int64_t(f) * pitch;
    const int cs = 3 * near[j] + far[j];
    if ((sx & 1) == 0) return j == 0 ? (4 * cs + 8) >> 4 : (3 * cs + 3 * near[j - 1] + far[j - 1] + 8) >> 4;
    return j == cw - 1 ? (4 * cs + 7) >> 4 : (3 * cs + 3 * near[j + 1] + far[j + 1] + 7) >> 4;
}

__device__ inline uint8_t clamp255(int v) { return uint8_t(v < 0 ? 0 : v > 255 ? 255 : v); }

__global__ __launch_bounds__(256) void color_kernel(const uint8_t* __restrict__ planes, uint8_t* __restrict__ bgr, ColorArgs a) {
    const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
    if (ox >= a.out_w) return;
    int sy, sx;                                          // PIL's Image.Transpose per EXIF orientation: output pixel -> stored pixel
    switch (a.orientation) {
        case 2: sy = oy; sx = a.width - 1 - ox; break;                       // FLIP_LEFT_RIGHT
        case 3: sy = a.height - 1 - oy; sx = a.width - 1 - ox; break;        // ROTATE_180
        case 4: sy = a.height - 1 - oy; sx = ox; break;                      // FLIP_TOP_BOTTOM
        case 5: sy = ox; sx = oy; break;                                     // TRANSPOSE
        case 6: sy = a.height - 1 - ox; sx = oy; break;                      // ROTATE_270
        case 7: sy = a.height - 1 - ox; sx = a.width - 1 - oy; break;        // TRANSVERSE
        case 8: sy = ox; sx = a.width - 1 - oy; break;                       // ROTATE_90
        default: sy = oy; sx = ox; break;
    }
    const int y = planes[a.plane_off[0] + int64_t(sy) * a.pitch[0] + sx];
    uint8_t* o = bgr + (int64_t(oy) * a.out_w + ox) * 3;
    if (a.mode == 0) {
        o[0] = o[1] = o[2] = uint8_t(y);
        return;
    }
    const uint8_t* pb = planes + a.plane_off[1];
    const uint8_t* pr = planes + a.plane_off[2];
    int cb, cr;
    if (a.mode == 1) {
        cb = pb[int64_t(sy) * a.pitch[1] + sx];
        cr = pr[int64_t(sy) * a.pitch[2] + sx];
    } else if (a.mode == 2) {
        cb = chroma_h2v1(pb + int64_t(sy) * a.pitch[1], sx, a.cw, a.fancy);
        cr = chroma_h2v1(pr + int64_t(sy) * a.pitch[2], sx, a.cw, a.fancy);
    } else {
        cb = chroma_h2v2(pb, a.pitch[1], sy, sx, a.cw, a.ch, a.fancy);
        cr = chroma_h2v2(pr, a.pitch[2], sy, sx, a.cw, a.ch, a.fancy);
    }
    const int x = cr - 128, xb = cb - 128;               // jdcolor.c build_ycc_rgb_table, SCALEBITS 16
    o[2] = clamp255(y + ((91881 * x + 32768) >> 16));                    // R: FIX(1.40200)
    o[1] = clamp255(y + ((-46802 * x - 22554 * xb + 32768) >> 16));      // G: FIX(0.71414), FIX(0.34414)
    o[0] = clamp255(y + ((116130 * xb + 32768) >> 16));                  // B: FIX(1.77200)
}

// the block layout the host decoder writes for this image and sampling (an info that disagrees is refused: it sizes the buffers)
bool layout_ok(const smap_jpeg_info& I) {
    if (I.width <= 0 || I.height <= 0 || (I.ncomp != 1 && I.ncomp != 3)) return false;
    const int hmax = I.h_samp[0], vmax = I.v_samp[0];
    if (!((hmax == 1 && vmax == 1) || (hmax == 2 && vmax == 1) || (hmax == 2 && vmax == 2))) return false;
    if (I.ncomp == 1 && (hmax != 1 || vmax != 1)) return false;
    const int64_t mcux = (I.width + 8 * hmax - 1) / (8 * hmax), mcuy = (I.height + 8 * vmax - 1) / (8 * vmax);
    int64_t off = 0;
    for (int c = 0; c < I.ncomp; ++c) {
        const int hs = c ? 1 : hmax, vs = c ? 1 : vmax;
        if (I.h_samp[c] != hs || I.v_samp[c] != vs || I.blocks_w[c] != mcux * hs || I.blocks_h[c] != mcuy * vs || I.coef_offset[c] != off)
            return false;
        off += int64_t(I.blocks_w[c]) * I.blocks_h[c] * 128;
    }
    return off == I.coef_bytes && I.orientation >= 1 && I.orientation <= 8;
}

}  // namespace

extern "C" int smap_jpeg_reconstruct(const int16_t* coeffs, const smap_jpeg_info* info, uint8_t* planes, uint8_t* bgr, void* stream) {
    if (!coeffs || !info || !planes || !bgr || !layout_ok(*info)) return SMAP_E_ARG;
    const smap_jpeg_info& I = *info;
    hipStream_t st = (hipStream_t)stream;
    IdctArgs a{};
    a.ncomp = I.ncomp;
    for (int c = 0; c < I.ncomp; ++c) {
        a.blocks_w[c] = I.blocks_w[c];
        a.first_block[c] = I.coef_offset[c] / 128;
        for (int k = 0; k < 64; ++k) a.quant[c][k] = I.quant[c][k];
    }
    for (int c = I.ncomp; c < 3; ++c) a.first_block[c] = INT64_MAX;
    a.n_blocks = I.coef_bytes / 128;
    const int64_t groups = (a.n_blocks + kBlocksPerGroup - 1) / kBlocksPerGroup;
    if (groups > INT32_MAX) return SMAP_E_ARG;
    hipLaunchKernelGGL(idct_kernel, dim3(unsigned(groups)), dim3(256), 0, st, coeffs, planes, a);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);

    ColorArgs b{};
    b.width = I.width;
    b.height = I.height;
    b.orientation = I.orientation;
    const bool swap = I.orientation >= 5;
    b.out_w = swap ? I.height : I.width;
    b.out_h = swap ? I.width : I.height;
    b.mode = I.ncomp == 1 ? 0 : I.h_samp[0] == 1 ? 1 : I.v_samp[0] == 1 ? 2 : 3;
    b.cw = (I.width + I.h_samp[0] - 1) / I.h_samp[0];
    b.ch = (I.height + I.v_samp[0] - 1) / I.v_samp[0];
    b.fancy = b.cw > 2;                                  // jdsample.c jinit_upsampler: fancy only when downsampled_width > 2
    for (int c = 0; c < I.ncomp; ++c) {
        b.plane_off[c] = I.coef_offset[c] / 2;
        b.pitch[c] = I.blocks_w[c] * 8;
    }
    hipLaunchKernelGGL(color_kernel, dim3((b.out_w + 255) / 256, b.out_h), dim3(256), 0, st, planes, bgr, b);
    return hip_rc(hipGetLastError());
}
