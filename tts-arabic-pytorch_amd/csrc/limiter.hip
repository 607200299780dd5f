// Look-ahead limiter (include/ttsamd.h states the arithmetic): a row gain and a gain-reduction curve in Q30
// integers, so that a LUFS target is reached where ttsamd_wave_level's cap on the gain would have stopped short of it, and so that a
// row alone, a row of a ragged batch and a row cut into stream windows leave with the same bits (minimum and integer sum are exact and
// order-free).
//   1. limit_q_kernel: u = fl32(x g), q = Q where |u| <= c, else floor(c / |u| 2^30) (float64 division), to the workspace; block 0 of a
//      row writes its gain, whether the row is written at all, and Q as the start of its reduction minimum.
//   2. limit_apply_kernel: a block owns a tile of LM_T samples.  It stages q over [t0 - A - R, t0 + T + 2A) in LDS (Q outside the row),
//      turns it in place into minima over 2^k samples by doubling (2^k <= R + A + 1 < 2^(k+1)), takes m = the minimum over
//      [i - R, i + A] from two overlapping windows of 2^k, adds m over [i - A, i + A] (int64; sums of eight first, then a sliding sum over a
//      thread's eight samples) and writes y = fl32(u s 2^-30) over its own tile.
// Two launches: the call works in place, and a tile's halo covers samples that another tile writes.
// ttsamd_wave_limit_true_peak: launch 1 is limit_q_tp_kernel, whose d is the larger of |u| and the 4x interpolator's values to either side
// of the sample (true_peak.hpp); launch 2 is the same kernel.
#include <cmath>

#include "common.hpp"
#include "true_peak.hpp"

namespace ttsamd {

constexpr int LM_T = 2048;                    // samples per tile (ttsamd.engine.LIMITER_TILE)
constexpr int LM_NT = 256;                    // threads per block: eight samples each
constexpr int LM_AMAX = 1024, LM_RMAX = 4096;
constexpr int LM_QN = LM_T + 3 * LM_AMAX + LM_RMAX;    // 9216 staged q
constexpr int LM_MN = LM_T + 2 * LM_AMAX;              // 4096 m
constexpr int LM_QPT = LM_QN / LM_NT;                  // 36 staged q per thread
constexpr int32_t LM_Q = 1 << 30;
static_assert(LM_QN % LM_NT == 0 && LM_T == 8 * LM_NT && LM_AMAX <= LM_T, "limiter tiling");
static_assert(LM_QN * 4 + LM_MN * 4 + LM_MN / 8 * 8 <= 65536, "limiter LDS");

__device__ __forceinline__ int64_t limit_len(const int64_t* __restrict__ ns, const int b, const int64_t stride) {
    return max((int64_t)0, min(ns[b], stride));
}

// the row's gain; false: the row keeps its samples
__device__ __forceinline__ bool limit_gain(const int md, const float tg, const float max_gain, const double* __restrict__ loudness, const int b,
                                           float& g) {
    g = 1.f;
    double g64;
    if (md == 2) {
        if (loudness == nullptr) return false;
        const double L = loudness[b];
        if (!isfinite(L)) return false;
        g64 = pow(10.0, ((double)tg - L) / 20.0);
    } else if (md == 3) {
        g64 = pow(10.0, (double)tg / 20.0);
    } else {
        return false;
    }
    g = (float)fmin(g64, (double)max_gain);
    return true;
}

__device__ __forceinline__ int32_t limit_q(const float u, const float c) {
    const float d = fabsf(u);
    return d > c ? (int32_t)floor((double)c / (double)d * 1073741824.0) : LM_Q;      // a NaN compares false: Q
}

__global__ __launch_bounds__(LM_NT) void limit_q_kernel(const float* __restrict__ wave, int64_t stride, const int64_t* __restrict__ ns,
                                                        const int32_t* __restrict__ mode, const float* __restrict__ target, float ceiling,
                                                        float max_gain, const double* __restrict__ loudness, float* __restrict__ gain_out,
                                                        int32_t* __restrict__ reduction_out, int32_t* __restrict__ live_out,
                                                        int32_t* __restrict__ qp) {
    const int b = blockIdx.y;
    const int64_t n = limit_len(ns, b, stride);
    float g;
    const bool live = limit_gain(mode[b], target[b], max_gain, loudness, b, g);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        gain_out[b] = g;
        reduction_out[b] = LM_Q;
        live_out[b] = live ? 1 : 0;
    }
    if (!live) return;
    const float* wb = wave + (int64_t)b * stride;
    int32_t* qb = qp + (int64_t)b * stride;
    const int64_t t0 = (int64_t)blockIdx.x * LM_T;
#pragma unroll
    for (int j = 0; j < LM_T / LM_NT; ++j) {
        const int64_t i = t0 + j * LM_NT + threadIdx.x;
        if (i < n) qb[i] = limit_q(__fmul_rn(wb[i], g), ceiling);
    }
}

// limit_q_kernel with the true-peak detector (ttsamd_wave_limit_true_peak): the block stages u for its tile and LM_TPH samples to either
// side (13 are needed: 12 taps and the sample in front; 16 keeps the 16-byte loads), every thread runs the interpolator's chains for
// the sample in front of its eight and for the eight, and d[i] = max(|u[i]|, max_p |v[i][p]|, max_p |v[i - 1][p]|) in float64.
constexpr int LM_TPH = 16;
constexpr int LM_UN = LM_T + 2 * LM_TPH;
static_assert(LM_TPH >= TP_W + 1 && LM_TPH % 4 == 0, "true-peak halo of the limiter");

__global__ __launch_bounds__(LM_NT) void limit_q_tp_kernel(const float* __restrict__ wave, int64_t stride, const int64_t* __restrict__ ns,
                                                           const int32_t* __restrict__ mode, const float* __restrict__ target, float ceiling,
                                                           float max_gain, const double* __restrict__ loudness, const TpTaps taps,
                                                           float* __restrict__ gain_out, int32_t* __restrict__ reduction_out,
                                                           int32_t* __restrict__ live_out, int32_t* __restrict__ qp) {
    __shared__ __align__(16) float us[LM_UN];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t n = limit_len(ns, b, stride);
    float g;
    const bool live = limit_gain(mode[b], target[b], max_gain, loudness, b, g);
    if (blockIdx.x == 0 && tid == 0) {
        gain_out[b] = g;
        reduction_out[b] = LM_Q;
        live_out[b] = live ? 1 : 0;
    }
    const int64_t t0 = (int64_t)blockIdx.x * LM_T;
    if (!live || t0 >= n) return;                              // the whole block
    tp_stage<true>(wave + (int64_t)b * stride, t0 - LM_TPH, LM_UN, n, g, us);
    __syncthreads();
    const int64_t i0 = t0 + 8 * tid;
    if (i0 >= n) return;
    double vm[9];                                              // samples i0 - 1 .. i0 + 7; us[8 tid + LM_TPH] is u[i0]
    tp_chains<9>(us + 8 * tid + LM_TPH - 1 - TP_W, taps, vm);
    int32_t* qb = qp + (int64_t)b * stride;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int64_t i = i0 + e;
        if (i < n) {
            double d = fmax(fabs((double)us[8 * tid + LM_TPH + e]), vm[e + 1]);
            if (i > 0) d = fmax(d, vm[e]);
            qb[i] = d > (double)ceiling ? (int32_t)floor((double)ceiling / d * 1073741824.0) : LM_Q;
        }
    }
}

__global__ __launch_bounds__(LM_NT) void limit_apply_kernel(float* __restrict__ wave, int64_t stride, const int64_t* __restrict__ ns,
                                                            int A, int R, int K2, const float* __restrict__ gain, const int32_t* __restrict__ live,
                                                            const int32_t* __restrict__ qp, int32_t* __restrict__ reduction_out) {
    __shared__ int32_t qs[LM_QN];
    __shared__ int32_t ms[LM_MN];
    __shared__ int64_t p8[LM_MN / 8];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t n = limit_len(ns, b, stride), t0 = (int64_t)blockIdx.x * LM_T;
    if (!live[b] || t0 >= n) return;                           // the whole block
    const float g = gain[b];
    const int32_t* qb = qp + (int64_t)b * stride;
    const int Ln = LM_T + 3 * A + R, Mn = LM_T + 2 * A;        // <= LM_QN, LM_MN: the host checks A and R
    const int64_t q0 = t0 - A - R;                             // the row position of qs[0]
    for (int j = tid; j < Ln; j += LM_NT) {
        const int64_t p = q0 + j;
        qs[j] = p >= 0 && p < n ? qb[p] : LM_Q;
    }
    __syncthreads();
    // qs[j] <- min qs[j .. j + 2^k - 1] by doubling; entries whose window runs past Ln keep a shorter one and are not read below
    for (int step = 1; step < K2; step <<= 1) {
        int32_t v[LM_QPT];
#pragma unroll
        for (int j = 0; j < LM_QPT; ++j) {
            const int i = tid + j * LM_NT;
            if (i < Ln) v[j] = i + step < Ln ? min(qs[i], qs[i + step]) : qs[i];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < LM_QPT; ++j) {
            const int i = tid + j * LM_NT;
            if (i < Ln) qs[i] = v[j];
        }
        __syncthreads();
    }
    // ms[j] = m at row position clamp(t0 - A + j, 0, n - 1): the minimum of q over [p - R, p + A], two windows of K2 <= R + A + 1
    for (int j = tid; j < Mn; j += LM_NT) {
        const int64_t p = min(max(t0 - A + j, (int64_t)0), n - 1);
        const int o = (int)(p - q0);                           // in [R, Ln - A)
        ms[j] = min(qs[o - R], qs[o + A - K2 + 1]);
    }
    __syncthreads();
    for (int j = tid; j < Mn / 8; j += LM_NT) {
        int64_t t = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) t += ms[8 * j + r];
        p8[j] = t;
    }
    __syncthreads();
    // samples t0 + 8 tid + (0 .. 7): the sum over ms[8 tid + e .. 8 tid + e + 2A]
    const int W = 2 * A + 1, nb = W >> 3, i0 = 8 * tid;
    int64_t sum = 0;
    for (int j = 0; j < nb; ++j) sum += p8[tid + j];
    for (int j = 8 * nb; j < W; ++j) sum += ms[i0 + j];
    int32_t s[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        s[e] = (int32_t)(sum / W);
        if (e < 7) sum += (int64_t)ms[i0 + e + W] - (int64_t)ms[i0 + e];      // i0 + e + W <= 2046 + 2A + 1 < Mn
    }
    float* wb = wave + (int64_t)b * stride;
    const int64_t i = t0 + i0;
    int32_t smin = LM_Q;
    if (i + 8 <= n && (((uintptr_t)(wb + i)) & 15) == 0) {
        float4 x[2] = {*(const float4*)(wb + i), *(const float4*)(wb + i + 4)};
        float* xv = (float*)x;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            xv[e] = (float)((double)__fmul_rn(xv[e], g) * (double)s[e] * (1.0 / 1073741824.0));
            smin = min(smin, s[e]);
        }
        *(float4*)(wb + i) = x[0];
        *(float4*)(wb + i + 4) = x[1];
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (i + e < n) {
                wb[i + e] = (float)((double)__fmul_rn(wb[i + e], g) * (double)s[e] * (1.0 / 1073741824.0));
                smin = min(smin, s[e]);
            }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) smin = min(smin, __shfl_xor(smin, d, 64));
    if ((tid & 63) == 0 && smin < LM_Q) atomicMin(reduction_out + b, smin);    // an integer minimum: order-free
}

struct LimitWs {
    int32_t *q, *live;                        // [B][stride] q plane, [B] row is written
    int64_t bytes;
};

static void limit_carve(void* base, int64_t B, int64_t stride, LimitWs& w) {
    Arena a(base, (int64_t)1 << 62);
    w.q = a.take<int32_t>(B * stride);
    w.live = a.take<int32_t>(B);
    w.bytes = a.off;
}

static int32_t wave_limit(float* wave, int64_t stride, const int64_t* nsamples, int32_t B, const int32_t* mode, const float* target,
                          float ceiling, float max_gain, int32_t A, int32_t R, const double* loudness, float* gain_out,
                          int32_t* reduction_out, void* workspace, int64_t workspace_bytes, bool true_peak, hipStream_t s) {
    TTS_REQUIRE(nsamples && mode && target && gain_out && reduction_out && workspace && (wave || stride == 0), "wave_limit: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && stride >= 0 && stride < ((int64_t)1 << 40), "wave_limit: bad batch %d / stride", B);
    TTS_REQUIRE(ceiling > 0.f && ceiling <= 1.f, "wave_limit: ceiling %g is not in (0, 1]", (double)ceiling);
    TTS_REQUIRE(max_gain > 0.f && std::isfinite(max_gain), "wave_limit: max_gain %g is not a finite gain above 0", (double)max_gain);
    TTS_REQUIRE(A >= 0 && A <= R && A <= LM_AMAX && R <= LM_RMAX, "wave_limit: attack %d / hold %d: 0 <= attack <= hold, attack <= %d, hold <= %d",
                A, R, LM_AMAX, LM_RMAX);
    LimitWs w;
    limit_carve(nullptr, B, stride, w);
    TTS_REQUIRE(workspace_bytes >= w.bytes, "wave_limit: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)w.bytes);
    limit_carve(workspace, B, stride, w);
    int64_t nt = (stride + LM_T - 1) / LM_T;
    nt = nt < 1 ? 1 : nt;
    TTS_REQUIRE(nt <= 0x7fffffff, "wave_limit: stride too large");
    int K2 = 1;
    while (2 * K2 <= R + A + 1) K2 *= 2;
    const dim3 grid((unsigned)nt, B);
    if (true_peak)
        hipLaunchKernelGGL(limit_q_tp_kernel, grid, dim3(LM_NT), 0, s, wave, stride, nsamples, mode, target, ceiling, max_gain, loudness,
                           tp_taps(), gain_out, reduction_out, w.live, w.q);
    else
        hipLaunchKernelGGL(limit_q_kernel, grid, dim3(LM_NT), 0, s, wave, stride, nsamples, mode, target, ceiling, max_gain, loudness, gain_out,
                           reduction_out, w.live, w.q);
    TTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(limit_apply_kernel, grid, dim3(LM_NT), 0, s, wave, stride, nsamples, (int)A, (int)R, K2, gain_out, w.live, w.q,
                       reduction_out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd

using namespace ttsamd;

extern "C" {

int64_t ttsamd_wave_limit_workspace_bytes(int32_t batch, int64_t wave_stride) {
    if (batch < 1 || wave_stride < 0 || wave_stride >= ((int64_t)1 << 40)) return -1;
    LimitWs w;
    limit_carve(nullptr, batch, wave_stride, w);
    return w.bytes;
}

int32_t ttsamd_wave_limit(float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, const int32_t* mode, const float* target,
                          float ceiling, float max_gain, int32_t attack, int32_t hold, const double* loudness, float* gain_out,
                          int32_t* reduction_out, void* workspace, int64_t workspace_bytes, void* stream) {
    return wave_limit(wave, wave_stride, nsamples, batch, mode, target, ceiling, max_gain, attack, hold, loudness, gain_out, reduction_out,
                      workspace, workspace_bytes, false, (hipStream_t)stream);
}

int32_t ttsamd_wave_limit_true_peak(float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, const int32_t* mode,
                                    const float* target, float ceiling, float max_gain, int32_t attack, int32_t hold, const double* loudness,
                                    float* gain_out, int32_t* reduction_out, void* workspace, int64_t workspace_bytes, void* stream) {
    return wave_limit(wave, wave_stride, nsamples, batch, mode, target, ceiling, max_gain, attack, hold, loudness, gain_out, reduction_out,
                      workspace, workspace_bytes, true, (hipStream_t)stream);
}

}  // extern "C"
