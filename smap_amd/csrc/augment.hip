// augment.hip -- smap_augment_batch: one training sample per frame, rotate + resize + crop/pad + flip + normalise in ONE launch,
// straight from the uploaded uint8 frames (reference: dataset/ImageAugmentation.py aug_rotate / aug_croppad / aug_flip, then
// ToTensor + Normalize).  Compiled with -ffp-contract=off: the doubles of the coordinate map round once, in the order written.
//
// The bits are those of the STAGED pipeline -- cv2.warpAffine (INTER_CUBIC, constant border 128) rounded to uint8, then cv2.resize
// (INTER_LINEAR) of that image -- but the rotated image is never written: the linear resize of csrc/prep_device.h asks a pixel source
// for its 2 x 2 taps, and the source here (WarpFetch) computes each tap as the 8-bit result of OpenCV's generic bicubic remap:
//   cv::warpAffine     inverts the matrix, X0 = cvRound((M1*y + M2) * 1024) + 16, adelta[x] = cvRound(M0 * x * 1024) (AB_BITS = 10),
//                      X = (X0 + adelta[x]) >> 5: 5 fractional bits (INTER_BITS), the integer part saturated to 16 bits
//   remapBicubic       source column (X >> 5) - 1 for four taps, weights = entry (Y & 31) * 32 + (X & 31) of the fixed-point table
//                      (smap_cubic_table), result saturate_u8((sum + (1 << 14)) >> 15); a tap outside the frame contributes the
//                      border value 128, a footprint wholly outside is 128
// A thread owns four adjacent output x of one row (one 16-byte store per plane, as preprocess_batch_kernel) where net_w % 4 == 0.
// Work per output pixel with rotation: 4 taps x (2 x 16 B of weights + 4 rows x 12 B of source); rows of an interior footprint are read
// as three 4-byte words (the frame is byte aligned: the loads are unaligned, inside the frame by the interior test).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
#include "smap_hip.h"
#include "hip_rc.h"
#include "prep_device.h"

namespace {

constexpr int kBorder = 128;

// One frame: the stored image, the inverted matrix (ignored unless rotate), the resize window over the rotated image.
struct AugFrame { const unsigned char* src; int h, w, rotate, flip; double im[6]; PrepWindow win; };
struct AugTable { AugFrame f[SMAP_PREP_MAX_FRAMES]; };         // by value in the kernel arguments: 112 bytes per frame

__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// Pixel (y, x) of the rotated image, 8 bit: OpenCV's fixed-point bicubic remap of the stored frame.
struct WarpFetch {
    const unsigned char* __restrict__ src;
    int h, w;
    double m0, m1, m2, m3, m4, m5;                       // the inverted matrix
    const int16_t* __restrict__ tab;
    __device__ __forceinline__ void operator()(int y, int x, int p[3]) const
    {
        const int X0 = (int)rint((m1 * y + m2) * 1024.0) + 16, Y0 = (int)rint((m4 * y + m5) * 1024.0) + 16;
        const int X = (X0 + (int)rint(m0 * x * 1024.0)) >> 5, Y = (Y0 + (int)rint(m3 * x * 1024.0)) >> 5;
        const int sx = sat16(X >> 5) - 1, sy = sat16(Y >> 5) - 1;
        if (sx >= w || sx + 4 <= 0 || sy >= h || sy + 4 <= 0) {          // the 4 x 4 footprint is wholly outside
            p[0] = p[1] = p[2] = kBorder;
            return;
        }
        const uint4* wq = reinterpret_cast<const uint4*>(tab + (size_t)((Y & 31) * 32 + (X & 31)) * 16);
        const uint4 w0 = wq[0], w1 = wq[1];
        const unsigned wr[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};     // (indexed by constants only: registers)
        int sum[3] = {0, 0, 0};
        const int wi = w - 3 > 0 ? w - 3 : 0, hi = h - 3 > 0 ? h - 3 : 0;
        if ((unsigned)sx < (unsigned)wi && (unsigned)sy < (unsigned)hi) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned q[3];
                memcpy(q, src + ((size_t)(sy + i) * w + sx) * 3, 12);      // pixels sx .. sx + 3 of row sy + i: all inside
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = i * 4 + j;
                    const int wt = (int)(short)(wr[k >> 1] >> ((k & 1) * 16));
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const int b = j * 3 + c;
                        sum[c] += (int)((q[b >> 2] >> ((b & 3) * 8)) & 255u) * wt;
                    }
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int yy = sy + i;
                const bool yin = yy >= 0 && yy < h;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int k = i * 4 + j, xx = sx + j;
                    const int wt = (int)(short)(wr[k >> 1] >> ((k & 1) * 16));
                    const bool in = yin && xx >= 0 && xx < w;
                    const unsigned char* q = src + ((size_t)(in ? yy : 0) * w + (in ? xx : 0)) * 3;
#pragma unroll
                    for (int c = 0; c < 3; ++c) sum[c] += (in ? (int)q[c] : kBorder) * wt;
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int t = (sum[c] + (1 << 14)) >> 15;
            p[c] = t < 0 ? 0 : (t > 255 ? 255 : t);
        }
    }
};

// grid (x tiles, rows, frames), as preprocess_batch_kernel: PX = 4 needs net_w % 4 == 0 and a 16-byte aligned dst.  The output pixel x
// reads the canvas pixel net_w - 1 - x when the frame is flipped.  `rotate` is uniform over a block (one frame per blockIdx.z).
template <int PX>
__global__ void __launch_bounds__(256) augment_batch_kernel(AugTable t, float* __restrict__ dst, PrepCanvas cv, const int16_t* __restrict__ tab)
{
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * PX, y = blockIdx.y;
    if (x0 >= cv.net_w) return;
    const AugFrame& f = t.f[blockIdx.z];
    float pad[3], o[3][PX];
#pragma unroll
    for (int c = 0; c < 3; ++c) pad[c] = prep_norm(128.f, cv.mean[c], cv.stdv[c]);
#pragma unroll
    for (int i = 0; i < PX; ++i) {
        float v[3];
        const int x = f.flip ? cv.net_w - 1 - (x0 + i) : x0 + i;
        const bool in = f.rotate ? prep_pixel(f.win, WarpFetch{f.src, f.h, f.w, f.im[0], f.im[1], f.im[2], f.im[3], f.im[4], f.im[5], tab}, x, y, v)
                                 : prep_pixel(f.win, MemFetch{f.src, f.w}, x, y, v);
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c][i] = in ? prep_norm(v[c], cv.mean[c], cv.stdv[c]) : pad[c];
    }
    const size_t plane = (size_t)cv.net_h * cv.net_w;
    float* row = dst + (size_t)blockIdx.z * 3 * plane + (size_t)y * cv.net_w + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (PX == 4) *reinterpret_cast<float4*>(row + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        else row[c * plane] = o[c][0];
    }
}

// cv::warpAffine's inversion of the forward matrix (WARP_INVERSE_MAP not set), in double, operation by operation.
void invert_affine(const double* m, double* im)
{
    double M[6] = {m[0], m[1], m[2], m[3], m[4], m[5]};
    double D = M[0] * M[4] - M[1] * M[3];
    D = D != 0 ? 1. / D : 0;
    const double A11 = M[4] * D, A22 = M[0] * D;
    M[0] = A11; M[1] *= -D;
    M[3] *= -D; M[4] = A22;
    const double b1 = -M[0] * M[2] - M[1] * M[5];
    const double b2 = -M[3] * M[2] - M[4] * M[5];
    M[2] = b1; M[5] = b2;
    for (int k = 0; k < 6; ++k) im[k] = M[k];
}

}  // namespace

extern "C" int smap_sizeof_aug_frame(void) { return (int)sizeof(smap_aug_frame); }

extern "C" int smap_augment_batch(const smap_aug_frame* frames, int B, float* dst, int net_h, int net_w, const float* mean3,
                                  const float* std3, const int16_t* cubic_tab, void* stream)
{
    if (!frames || !dst || !mean3 || !std3 || B <= 0 || net_h <= 0 || net_w <= 0) return SMAP_E_ARG;
    if ((uintptr_t)cubic_tab & 15) return SMAP_E_ARG;
    for (int b = 0; b < B; ++b) {                        // every frame is checked before the first launch: all of the batch or nothing
        const smap_aug_frame& s = frames[b];
        if (!s.src || s.h <= 0 || s.w <= 0 || s.rh <= 0 || s.rw <= 0 || s.nh <= 0 || s.nw <= 0 || !(s.fx > 0) || !(s.fy > 0)) return SMAP_E_ARG;
        if (s.h > SMAP_AUG_MAX_SIDE || s.w > SMAP_AUG_MAX_SIDE || s.rh > SMAP_AUG_MAX_SIDE || s.rw > SMAP_AUG_MAX_SIDE) return SMAP_E_ARG;
        if (s.rotate) {
            if (!cubic_tab) return SMAP_E_ARG;
            for (int k = 0; k < 6; ++k)
                if (!isfinite(s.m[k])) return SMAP_E_ARG;
        }
    }
    const PrepCanvas cv{net_h, net_w, {mean3[0], mean3[1], mean3[2]}, {std3[0], std3[1], std3[2]}};
    const bool vec = net_w % 4 == 0 && ((uintptr_t)dst & 15) == 0;
    const int px = vec ? 4 : 1;
    const size_t frame_floats = (size_t)3 * net_h * net_w;                 // (a multiple of 4 floats when vec: every frame stays aligned)
    for (int b0 = 0; b0 < B; b0 += SMAP_PREP_MAX_FRAMES) {
        const int n = B - b0 < SMAP_PREP_MAX_FRAMES ? B - b0 : SMAP_PREP_MAX_FRAMES;
        AugTable t;
        for (int i = 0; i < SMAP_PREP_MAX_FRAMES; ++i) {                    // unused entries repeat the last frame: never read (grid.z = n)
            const smap_aug_frame& s = frames[b0 + (i < n ? i : n - 1)];
            AugFrame& a = t.f[i];
            a.src = s.src; a.h = s.h; a.w = s.w; a.rotate = s.rotate != 0; a.flip = s.flip != 0;
            for (int k = 0; k < 6; ++k) a.im[k] = 0;
            if (s.rotate) invert_affine(s.m, a.im);
            // the resize reads the rotated image (rh x rw) when the frame rotates, else the stored frame
            a.win = PrepWindow{s.rotate ? s.rh : s.h, s.rotate ? s.rw : s.w, s.nh, s.nw, s.top, s.left, 1.0 / s.fx, 1.0 / s.fy};
        }
        const dim3 grid((net_w + 256 * px - 1) / (256 * px), net_h, n);
        float* out = dst + (size_t)b0 * frame_floats;
        if (vec) hipLaunchKernelGGL(augment_batch_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, t, out, cv, cubic_tab);
        else hipLaunchKernelGGL(augment_batch_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, t, out, cv, cubic_tab);
        const int rc = hip_rc(hipGetLastError());
        if (rc) return rc;
    }
    return 0;
}
