// prep_device.h -- the ONE copy of the 8-bit INTER_LINEAR resize + crop/pad + ToTensor/Normalize arithmetic, shared by the kernels of
// assoc.hip (smap_preprocess, smap_preprocess_batch: the source is the stored frame) and augment.hip (smap_augment_batch: the source is
// the bicubic warp of the stored frame, computed per tap and never written to memory).  Units that include it are built with
// -ffp-contract=off: every float op rounds once, in the order written.
//
// dataset/custom_dataset.py:41-68 (aug_croppad) and dataset/base_dataset.py (the annotated sets' crop-and-pad) + ToTensor + Normalize on
// the device: OpenCV's 8-bit INTER_LINEAR resize, paste into the net_h x net_w canvas padded with 128, /255, (x - mean) / std, in ATen's
// operation order so that it matches the host path bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace {

// The resize window of one frame: the SOURCE image of the resize (h x w: the stored frame, or the rotated image), the window (nh x nw at
// (top, left), which may stick out of the canvas on any side) and 1 / fx, 1 / fy.
struct PrepWindow { int h, w, nh, nw, top, left; double scale_x, scale_y; };
struct PrepCanvas { int net_h, net_w; float mean[3], stdv[3]; };

// One axis of OpenCV's 8-bit INTER_LINEAR (modules/imgproc/src/resize.cpp, cv::resize -> resizeGeneric_ set-up):
//   fx = (float)((d + 0.5) * scale - 0.5) with scale = 1 / fx_arg (double); s = floor(fx); fx -= s;
//   s < 0 -> (0, 0);  s >= n - 1 -> (n - 1, 0);  coefficients = cvRound(c * 2048) as shorts (INTER_RESIZE_COEF_BITS = 11).
struct CvTap { int s0, s1; int c0, c1; };
__device__ __forceinline__ CvTap cv_tap(int d, double scale, int n)
{
    float f = (float)(((double)d + 0.5) * scale - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n - 1) { f = 0.f; s = n - 1; }
    CvTap t;
    t.s0 = s;
    t.s1 = s + 1 < n ? s + 1 : s;                        // its coefficient is 0 whenever the clamp applies
    t.c0 = (int)rintf((1.f - f) * 2048.f);               // saturate_cast<short>(float) = cvRound: half to even
    t.c1 = (int)rintf(f * 2048.f);
    return t;
}

// ToTensor + Normalize of one 8-bit value, in that order.
__device__ __forceinline__ float prep_norm(float v, float mean, float stdv) { return (v / 255.0f - mean) / stdv; }

// The plain pixel source: pixel (y, x) of a stored uint8 [h][w][3] frame.
struct MemFetch {
    const unsigned char* __restrict__ src;
    int w;
    __device__ __forceinline__ void operator()(int y, int x, int p[3]) const
    {
        const unsigned char* q = src + ((size_t)y * w + x) * 3;
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
    }
};

// Canvas pixel (x, y) of one frame as three 8-bit values: cv2.resize(img, (0,0), fx=s, fy=s) [INTER_LINEAR, 8-bit fixed point] where the
// window covers the pixel, else false (padding).  `fetch(y, x, p)` hands out pixel (y, x) of the h x w source, 0 <= y < h, 0 <= x < w.
// The window test is the paste's clip: a pixel of the canvas is the resized image's (y - top, x - left) if that exists, whatever the sign
// of top / left and however far the window overhangs (64-bit: no int overflow).
// The resize follows OpenCV's published algorithm operation by operation: horizontal pass in 11-bit fixed point (int32), vertical pass
// ((b0*(S0>>4))>>16) + ((b1*(S1>>4))>>16) + 2) >> 2 (VResizeLinear<uchar,int,short,FixedPtCast<int,uchar,22>>), and the exact 2x shrink
// as the 2x2 box mean (cv::resize switches INTER_LINEAR to INTER_AREA there).  cv2 is not in this image: parity unpinned by execution.
// Every tap is clamped to the source (h, w), so no read leaves it even when nh / nw were derived from another size.
template <class Fetch>
__device__ __forceinline__ bool prep_pixel(const PrepWindow& p, const Fetch& fetch, int x, int y, float v[3])
{
    const long long ry64 = (long long)y - p.top, rx64 = (long long)x - p.left;
    if (ry64 < 0 || ry64 >= p.nh || rx64 < 0 || rx64 >= p.nw) return false;
    const int ry = (int)ry64, rx = (int)rx64;
    int p00[3], p01[3], p10[3], p11[3];
    if (p.scale_x == 2.0 && p.scale_y == 2.0) {          // INTER_AREA fast path: (a + b + c + d + 2) >> 2
        const int y0 = ry * 2 < p.h ? ry * 2 : p.h - 1, y1 = ry * 2 + 1 < p.h ? ry * 2 + 1 : p.h - 1;
        const int x0 = rx * 2 < p.w ? rx * 2 : p.w - 1, x1 = rx * 2 + 1 < p.w ? rx * 2 + 1 : p.w - 1;
        fetch(y0, x0, p00); fetch(y0, x1, p01); fetch(y1, x0, p10); fetch(y1, x1, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = (float)((p00[c] + p01[c] + p10[c] + p11[c] + 2) >> 2);
    } else {
        const CvTap ty = cv_tap(ry, p.scale_y, p.h), tx = cv_tap(rx, p.scale_x, p.w);
        fetch(ty.s0, tx.s0, p00); fetch(ty.s0, tx.s1, p01); fetch(ty.s1, tx.s0, p10); fetch(ty.s1, tx.s1, p11);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int h0 = p00[c] * tx.c0 + p01[c] * tx.c1;
            const int h1 = p10[c] * tx.c0 + p11[c] * tx.c1;
            const int t = (((ty.c0 * (h0 >> 4)) >> 16) + ((ty.c1 * (h1 >> 4)) >> 16) + 2) >> 2;
            v[c] = (float)(t < 0 ? 0 : (t > 255 ? 255 : t));
        }
    }
    return true;
}

}  // namespace
