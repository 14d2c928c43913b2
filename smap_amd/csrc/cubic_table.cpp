// cubic_table.cpp -- smap_cubic_table: the fixed-point weight table of OpenCV's 8-bit bicubic remap (modules/imgproc/src/imgwarp.cpp:
// interpolateCubic, initInterTab1D, initInterTab2D), restated operation by operation in float32.  Host-only C++, no HIP: also built
// alone under sanitizers (tests/c/cubic_table_main.cpp).  Built with -ffp-contract=off: every float op rounds once, in the order written.
#include <math.h>
#include <stdint.h>
#include "smap_hip.h"

namespace {

constexpr int kTab = 32, kTaps = 4, kScale = 32768;      // INTER_TAB_SIZE, the cubic's taps, INTER_REMAP_COEF_SCALE

void cubic_1d(float x, float* c)
{
    const float A = -0.75f;
    c[0] = ((A * (x + 1) - 5 * A) * (x + 1) + 8 * A) * (x + 1) - 4 * A;
    c[1] = ((A + 2) * x - (A + 3)) * x * x + 1;
    c[2] = ((A + 2) * (1 - x) - (A + 3)) * (1 - x) * (1 - x) + 1;
    c[3] = 1.f - c[0] - c[1] - c[2];
}

short saturate_short(float v)                            // saturate_cast<short>(float): cvRound (half to even), then the clamp
{
    const long r = lrintf(v);
    return (short)(r < -32768 ? -32768 : (r > 32767 ? 32767 : r));
}

}  // namespace

extern "C" int smap_cubic_table(int16_t* out)
{
    if (!out) return SMAP_E_ARG;
    float tab1[kTab * kTaps];
    const float scale = 1.f / kTab;
    for (int i = 0; i < kTab; ++i) cubic_1d(i * scale, tab1 + i * kTaps);
    for (int i = 0; i < kTab; ++i)
        for (int j = 0; j < kTab; ++j) {
            int16_t* itab = out + (i * kTab + j) * kTaps * kTaps;
            int isum = 0;
            for (int k1 = 0; k1 < kTaps; ++k1) {
                const float vy = tab1[i * kTaps + k1];
                for (int k2 = 0; k2 < kTaps; ++k2) {
                    const float v = vy * tab1[j * kTaps + k2];
                    isum += itab[k1 * kTaps + k2] = saturate_short(v * kScale);
                }
            }
            if (isum != kScale) {
                // initInterTab2D's fix-up: the difference goes to the largest (sum short) or the smallest (sum over) of the 2 x 2 entries
                // it scans -- rows and columns ksize / 2 and ksize / 2 + 1, i.e. indices 2 and 3 of the 4 x 4, ties to the first met
                const int diff = isum - kScale, k0 = kTaps / 2;
                int Mk1 = k0, Mk2 = k0, mk1 = k0, mk2 = k0;
                for (int k1 = k0; k1 < k0 + 2; ++k1)
                    for (int k2 = k0; k2 < k0 + 2; ++k2) {
                        if (itab[k1 * kTaps + k2] < itab[mk1 * kTaps + mk2]) mk1 = k1, mk2 = k2;
                        else if (itab[k1 * kTaps + k2] > itab[Mk1 * kTaps + Mk2]) Mk1 = k1, Mk2 = k2;
                    }
                if (diff < 0) itab[Mk1 * kTaps + Mk2] = (int16_t)(itab[Mk1 * kTaps + Mk2] - diff);
                else itab[mk1 * kTaps + mk2] = (int16_t)(itab[mk1 * kTaps + mk2] - diff);
            }
        }
    return 0;
}
