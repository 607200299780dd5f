// The 4x interpolator of the true-peak detector (include/ttsamd.h states the arithmetic): phases 1 .. 3 of the resampler's own
// Hann-windowed sinc table at o = 1, n = 4, lowpass_filter_width = 12, rolloff = 1 (25 taps per phase), as float64 chains over fp32
// values.  The product of two fp32 values is exact in float64, so a chain has the same bits with fma as with multiply-then-add, on the
// GPU and in numpy.  Shared by csrc/loudness.hip (ttsamd_true_peak) and csrc/limiter.hip (the detector of ttsamd_wave_limit_true_peak).
#pragma once
#include <cmath>

#include "common.hpp"

namespace ttsamd {

constexpr int TP_W = 12;                      // samples the filter reaches to either side
constexpr int TP_J = 2 * TP_W + 1;            // taps per phase
constexpr int TP_P = 3;                       // phases 1 .. 3; phase 0 is the sample itself

struct TpTaps {
    double h[TP_P][TP_J];                     // the fp32 table, widened: a kernel argument, so the taps are wave-uniform
};

// ttsamd/resample.py's formula in its order of operations, float64, rounded once to fp32
inline const TpTaps& tp_taps() {
    static const TpTaps taps = [] {
        TpTaps t;
        const double pi = 3.141592653589793;
        for (int p = 1; p <= TP_P; ++p)
            for (int j = 0; j < TP_J; ++j) {
                double x = (double)(j - TP_W) - (double)p / 4.0;
                x = x < -(double)TP_W ? -(double)TP_W : (x > (double)TP_W ? (double)TP_W : x);
                const double c = std::cos(x * pi / (double)TP_W / 2.0), xp = x * pi;
                const double sinc = xp == 0.0 ? 1.0 : std::sin(xp) / xp;
                t.h[p - 1][j] = (double)(float)(sinc * (c * c));
            }
        return t;
    }();
    return taps;
}

#if defined(__HIPCC__)
// xs[k] = the row's sample p0 + k for k < cnt, zero outside [0, n), times g when SCALE (fl32(x g), the limiter's u); p0 and cnt are
// multiples of 4 and xs is 16-byte aligned.  16-byte loads where the row is aligned and the four samples lie inside it; nothing at or
// past n is read.
template <bool SCALE>
__device__ __forceinline__ void tp_stage(const float* __restrict__ wb, const int64_t p0, const int cnt, const int64_t n, const float g,
                                         float* __restrict__ xs) {
    const bool aligned = (((uintptr_t)wb) & 15) == 0;
    for (int k = 4 * threadIdx.x; k < cnt; k += 4 * blockDim.x) {
        const int64_t p = p0 + k;
        float v[4];
        if (aligned && p >= 0 && p + 4 <= n) {
            const float4 q = *(const float4*)(wb + p);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = p + e >= 0 && p + e < n ? wb[p + e] : 0.f;
        }
        if (SCALE) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (p + e >= 0 && p + e < n) v[e] = __fmul_rn(v[e], g);
        }
        *(float4*)(xs + k) = make_float4(v[0], v[1], v[2], v[3]);
    }
}

// NS consecutive samples: xs[e + j] is the signal at (sample e) + j - 12.  vm[e] = max over p of |v[e][p]|,
// v[e][p] = sum over j ascending of h[p][j] (double)xs[e + j] from +0.0: 3 NS chains that run side by side, each in its own order.
template <int NS>
__device__ __forceinline__ void tp_chains(const float* __restrict__ xs, const TpTaps& t, double* __restrict__ vm) {
    double x[NS + TP_J - 1], acc[NS][TP_P];
#pragma unroll
    for (int k = 0; k < NS + TP_J - 1; ++k) x[k] = (double)xs[k];
#pragma unroll
    for (int e = 0; e < NS; ++e)
#pragma unroll
        for (int p = 0; p < TP_P; ++p) acc[e][p] = 0.0;
#pragma unroll
    for (int j = 0; j < TP_J; ++j)
#pragma unroll
        for (int p = 0; p < TP_P; ++p)
#pragma unroll
            for (int e = 0; e < NS; ++e) acc[e][p] = fma(t.h[p][j], x[e + j], acc[e][p]);
#pragma unroll
    for (int e = 0; e < NS; ++e) vm[e] = fmax(fmax(fabs(acc[e][0]), fabs(acc[e][1])), fabs(acc[e][2]));
}
#endif

}  // namespace ttsamd
