// labels.hip -- ground-truth label maps on gfx950: the 15 Gaussian heat-maps and the 14 x (x, y, z) part-affinity / relative-depth
// fields a training sample is made of, at every label scale of a batch.
//
// Reference semantics (zju3dv/SMAP): dataset/representation.py generate_heatmap (:5-21), generate_paf / putVecMaps3D (:36-113), laid out
// as JointDataset.__getitem__ does (dataset/base_dataset.py:177-185): labels [B, S, 15 + 3 * 14, H, W] fp32.
// Compiled with -ffp-contract=off like assoc.hip and eval.hip: every operation below rounds once, in the order written; the fp32
// divisions are the correctly rounded ones (hipcc's default).
//
// Who computes what (include/smap_hip.h, smap_amd/labels.py):
//   host    everything that is per (frame, scale, limb, person): validity, the int truncations, / stride, np.linalg.norm, the unit
//           vector, limb_z, the rounded and clipped box -- float64 numpy with the reference's own expressions -- and per
//           (frame, joint) the SET of impulse cells, plus the blur taps of every scale.  One table, one upload.
//   fields  one thread per pixel of one (limb, frame, scale): walks the frame's valid persons IN ORDER and repeats, on every pixel,
//           what putVecMaps3D does to the whole map: acc *= cnt; acc += vec; cnt += (vec_x != 0 || vec_y != 0); acc /= max(cnt, 1).
//           The multiply and the divide also run outside the person's box ((a * 3) / 3 is not always a).
//   heat    one workgroup per (joint, frame, scale): the separable blur of a 0 / 1 source restricted to the terms that are not zero
//           (every term is >= 0, so leaving a +0 out changes no bit), row pass inside the column pass, taps in ascending order;
//           then the map's maximum and the division by fp32(max / 255).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "smap_hip.h"
#include "hip_rc.h"

namespace {

constexpr int NJ = SMAP_NJ, NL = SMAP_NL, NC = SMAP_LABEL_C;
constexpr int MAX_HW = 32768;                        // one bit per pixel of the source in LDS: 4 KiB
constexpr int HEAT_NT = 1024, FIELD_NT = 256;

// Byte offsets of the table's sections (the layout include/smap_hip.h documents; smap_amd/labels.py table_layout mirrors it).
struct Layout {
    int64_t limb_f, limb_box, limb_n, imp, imp_n, taps, bytes;
};

inline int64_t align8(int64_t v) { return (v + 7) / 8 * 8; }

inline Layout table_layout(int B, int S, int P)
{
    const int64_t groups = (int64_t)B * S * NL;
    Layout t;
    t.limb_f = 0;
    t.limb_box = t.limb_f + groups * P * 6 * 8;
    t.limb_n = t.limb_box + groups * P * 4 * 4;
    t.imp = align8(t.limb_n + groups * 4);
    t.imp_n = t.imp + (int64_t)B * NJ * P * 4;
    t.taps = align8(t.imp_n + (int64_t)B * NJ * 4);
    t.bytes = align8(t.taps + (int64_t)S * 2 * SMAP_LABEL_MAX_TAPS * 4);
    return t;
}

struct Ksizes {
    int x[SMAP_LABEL_MAX_SCALES], y[SMAP_LABEL_MAX_SCALES];      // taps of the row pass (along x) and of the column pass
};

// ---- part-affinity + relative-depth fields -------------------------------------------------------------------------------------
// grid (pixel blocks, limb, frame * S + scale).  limb_f [group][P][6] = centerA_x, centerA_y, unit_x, unit_y, limb_z, thre (all as the
// reference holds them in float64); limb_box [group][P][4] = min_x, max_x, min_y, max_y (half open, already clipped to the map).
__global__ __launch_bounds__(FIELD_NT) void label_fields_kernel(const double* __restrict__ limb_f, const int32_t* __restrict__ limb_box,
                                                                 const int32_t* __restrict__ limb_n, int P, int H, int W,
                                                                 float* __restrict__ labels)
{
    const int pix = blockIdx.x * FIELD_NT + threadIdx.x;
    const int limb = blockIdx.y;
    const int64_t group = (int64_t)blockIdx.z * NL + limb;
    if (pix >= H * W) return;
    const int y = pix / W, x = pix - y * W;
    int n = limb_n[group];
    n = n < 0 ? 0 : (n > P ? P : n);
    const double* f = limb_f + group * P * 6;
    const int32_t* box = limb_box + group * P * 4;
    float ax = 0.0f, ay = 0.0f, az = 0.0f, cnt = 0.0f;
    for (int p = 0; p < n; ++p, f += 6, box += 4) {
        // np.multiply(accumulate_vec_map, count) (:100-101)
        ax *= cnt;
        ay *= cnt;
        az *= cnt;
        // mask = |ba_x * u_y - ba_y * u_x| < thre inside the box (:88-91), 0 elsewhere; vec_map = fp32(mask * u) (:93-96)
        double m = 0.0;
        if (x >= box[0] && x < box[1] && y >= box[2] && y < box[3]) {
            const double ba_x = (double)x - f[0], ba_y = (double)y - f[1];
            m = fabs(ba_x * f[3] - ba_y * f[2]) < f[5] ? 1.0 : 0.0;
        }
        const float vx = (float)(m * f[2]), vy = (float)(m * f[3]), vz = (float)(m * f[4]);
        ax += vx;                                              // :102
        ay += vy;
        az += vz;
        if (vx != 0.0f || vy != 0.0f) cnt += 1.0f;             // :97-98,104
        const float d = cnt == 0.0f ? 1.0f : cnt;              // :106-111
        ax /= d;
        ay /= d;
        az /= d;
    }
    float* out = labels + ((int64_t)blockIdx.z * NC + NJ + 3 * limb) * H * W + pix;
    out[0] = ax * 127.0f;                                      // :50-51
    out[(int64_t)H * W] = ay * 127.0f;
    out[(int64_t)2 * H * W] = az;
}

// ---- heat-maps -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

// grid (joint, frame * S + scale), HEAT_NT threads.  imp [B][15][P]: y * W + x of the distinct cells that hold an impulse.
__global__ __launch_bounds__(HEAT_NT) void label_heat_kernel(const int32_t* __restrict__ imp, const int32_t* __restrict__ imp_n,
                                                              const float* __restrict__ taps, Ksizes ks, int S, int P, int H, int W,
                                                              float* __restrict__ labels)
{
    __shared__ uint32_t s_src[MAX_HW / 32];                    // the 0 / 1 source map
    __shared__ uint32_t s_row[MAX_HW / 8 / 32];                // rows that hold an impulse (W >= 8, so H <= 4096)
    __shared__ float s_kx[SMAP_LABEL_MAX_TAPS], s_ky[SMAP_LABEL_MAX_TAPS];
    __shared__ float s_max[HEAT_NT / 64];
    const int joint = blockIdx.x, b = blockIdx.y / S, s = blockIdx.y - b * S;
    const int t = threadIdx.x, HW = H * W;
    const int nx = ks.x[s], ny = ks.y[s], rx = nx / 2, ry = ny / 2;
    for (int i = t; i < MAX_HW / 32; i += HEAT_NT) s_src[i] = 0u;
    if (t < MAX_HW / 8 / 32) s_row[t] = 0u;
    if (t < SMAP_LABEL_MAX_TAPS) {
        s_kx[t] = t < nx ? taps[(s * 2 + 0) * SMAP_LABEL_MAX_TAPS + t] : 0.0f;
        s_ky[t] = t < ny ? taps[(s * 2 + 1) * SMAP_LABEL_MAX_TAPS + t] : 0.0f;
    }
    __syncthreads();
    int n = imp_n[b * NJ + joint];
    n = n < 0 ? 0 : (n > P ? P : n);
    for (int i = t; i < n; i += HEAT_NT) {
        const int idx = imp[((int64_t)b * NJ + joint) * P + i];
        if (idx >= 0 && idx < HW) {
            atomicOr(&s_src[idx >> 5], 1u << (idx & 31));
            const int row = idx / W;
            atomicOr(&s_row[row >> 5], 1u << (row & 31));
        }
    }
    __syncthreads();
    float* out = labels + ((int64_t)blockIdx.y * NC + joint) * HW;
    float mx = 0.0f;
    for (int pix = t; pix < HW; pix += HEAT_NT) {
        const int y = pix / W, x = pix - y * W;
        float acc = 0.0f;
        for (int j = 0; j < ny; ++j) {                         // column pass over the row pass's output, taps ascending
            const int yy = reflect101(y + j - ry, H);
            if (!((s_row[yy >> 5] >> (yy & 31)) & 1u)) continue;          // a row without impulses blurs to +0: acc + k * 0 == acc
            float row = 0.0f;
            for (int i = 0; i < nx; ++i) {                     // row pass at (yy, x), taps ascending; k * 1 == k, k * 0 adds +0
                const int idx = yy * W + reflect101(x + i - rx, W);
                if ((s_src[idx >> 5] >> (idx & 31)) & 1u) row += s_kx[i];
            }
            acc += s_ky[j] * row;
        }
        out[pix] = acc;
        mx = fmaxf(mx, acc);
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_down(mx, o, 64));
    if ((t & 63) == 0) s_max[t >> 6] = mx;
    __syncthreads();
    mx = s_max[0];
    for (int i = 1; i < HEAT_NT / 64; ++i) mx = fmaxf(mx, s_max[i]);
    if ((double)mx <= 1e-8) return;                            // :17-18
    const float d = mx / 255.0f;                               // :19  heatmaps[i] /= maxi / 255
    for (int pix = t; pix < HW; pix += HEAT_NT) out[pix] = out[pix] / d;   // this thread's own stores: no fence needed
}

}  // namespace

extern "C" {

int smap_render_labels(const void* table, int64_t table_bytes, const int32_t* ksizes, int B, int S, int P, int H, int W, float* labels,
                       void* stream)
{
    if (!table || !ksizes || !labels || B < 1 || S < 1 || S > SMAP_LABEL_MAX_SCALES || P < 1 || P > SMAP_LABEL_MAX_PERSONS || H < 8 ||
        W < 8 || (int64_t)H * W > MAX_HW || (int64_t)B * S > 65535 || ((uintptr_t)table & 7))
        return SMAP_E_ARG;
    Ksizes ks{};
    for (int s = 0; s < 2 * S; ++s) {
        // odd, and a radius that ONE reflection brings back into the smallest map (8 cells)
        if (ksizes[s] < 1 || ksizes[s] >= SMAP_LABEL_MAX_TAPS || !(ksizes[s] & 1)) return SMAP_E_ARG;
        (s & 1 ? ks.y : ks.x)[s >> 1] = ksizes[s];
    }
    const Layout t = table_layout(B, S, P);
    if (table_bytes != t.bytes) return SMAP_E_ARG;
    const char* base = (const char*)table;
    const int HW = H * W;
    hipLaunchKernelGGL(label_fields_kernel, dim3((unsigned)((HW + FIELD_NT - 1) / FIELD_NT), NL, (unsigned)(B * S)), dim3(FIELD_NT), 0,
                       (hipStream_t)stream, (const double*)(base + t.limb_f), (const int32_t*)(base + t.limb_box),
                       (const int32_t*)(base + t.limb_n), P, H, W, labels);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return hip_rc(e);
    hipLaunchKernelGGL(label_heat_kernel, dim3(NJ, (unsigned)(B * S)), dim3(HEAT_NT), 0, (hipStream_t)stream,
                       (const int32_t*)(base + t.imp), (const int32_t*)(base + t.imp_n), (const float*)(base + t.taps), ks, S, P, H, W,
                       labels);
    return hip_rc(hipGetLastError());
}

}  // extern "C"
