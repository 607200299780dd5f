// Objective evaluation on the device: the scores a TTS evaluation reports between a prediction and a recording, along a DTW path.
// The reference has no such module; the arithmetic is stated in include/ttsamd.h and DESIGN.md section 4 and restated in float64 by
// tests/objective_ref.py.
//
//   mel_cepstrum      logmel [B][n_mels][T] -> cep [B][n_coef][T]: the orthonormal DCT-II across the bands of every frame.  A block owns
//                     64 frames, one lane per frame (loads along t are coalesced for each band); its four waves split the coefficients
//                     (wave w: k = w, w + 4, ...), at most 16 float64 accumulators per lane.  The basis is ONE table of cos(pi r / 2M),
//                     r < 4M, in LDS, built in float64 by cospi; the argument k (2m + 1) is reduced mod 4M in integers, so every entry
//                     is good to the cosine's own ulp.  Products and sums are float64 over m ascending, the result is rounded once.
//   dtw_aligned_eval  one block per pair: step p of the path goes to thread p mod 256, which adds its steps in ascending order; the
//                     block sum is a fixed tree in LDS.  The order depends on the pair alone, so a row of a batch equals the call on
//                     that pair, bit for bit.  Pass 1: the cepstral distance, |mel difference|, voicing counts, the f0 errors and sums;
//                     pass 2: the centred sums of the correlation about the means of pass 1.  Every input is widened to float64 first.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "kernels.hpp"

namespace ttsamd {

constexpr int OBJ_MAXMEL = 128, OBJ_MAXCOEF = 64, OBJ_FPB = 64, OBJ_WAVES = 4, OBJ_CPW = OBJ_MAXCOEF / OBJ_WAVES;
constexpr int OBJ_NT = 256;

// ------------------------------------------------------------------------------------------------------------------- mel cepstrum ----
__global__ __launch_bounds__(OBJ_FPB * OBJ_WAVES) void mel_cepstrum_kernel(const float* __restrict__ logmel, const int64_t* __restrict__ lens,
                                                                           int n_mels, int t_max, int n_coef, float* __restrict__ cep) {
    __shared__ double tab[4 * OBJ_MAXMEL];                       // cos(pi r / (2 n_mels)), r < 4 n_mels
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & (OBJ_FPB - 1), w = tid / OBJ_FPB;
    const int t = blockIdx.x * OBJ_FPB + lane, period = 4 * n_mels;
    const int n = (int)max((int64_t)0, min(lens[b], (int64_t)t_max));
    for (int r = tid; r < period; r += OBJ_FPB * OBJ_WAVES) tab[r] = cospi((double)r / (double)(2 * n_mels));
    __syncthreads();
    const bool live = t < n;                                     // frames at or past the row's end are never read
    const float* xb = logmel + (int64_t)b * n_mels * t_max + t;
    double acc[OBJ_CPW];
    int r[OBJ_CPW];                                              // k (2m + 1) mod 4 n_mels of coefficient k = w + 4 c, advanced by 2k per band
#pragma unroll
    for (int c = 0; c < OBJ_CPW; ++c) {
        acc[c] = 0.0;
        r[c] = w + OBJ_WAVES * c;                                // k < n_mels <= period
    }
    for (int m = 0; m < n_mels; ++m) {
        const double x = live ? (double)xb[(int64_t)m * t_max] : 0.0;
#pragma unroll
        for (int c = 0; c < OBJ_CPW; ++c) {
            const int k = w + OBJ_WAVES * c;
            if (k < n_coef) {                                    // (wave-uniform)
                acc[c] += x * tab[r[c]];
                r[c] += 2 * k;
                if (r[c] >= period) r[c] -= period;
            }
        }
    }
    if (t < t_max) {
        float* cb = cep + (int64_t)b * n_coef * t_max + t;
        const double s0 = sqrt(1.0 / n_mels), s1 = sqrt(2.0 / n_mels);
#pragma unroll
        for (int c = 0; c < OBJ_CPW; ++c) {
            const int k = w + OBJ_WAVES * c;
            if (k < n_coef) cb[(int64_t)k * t_max] = live ? (float)((k ? s1 : s0) * acc[c]) : 0.f;
        }
    }
}

int32_t mel_cepstrum(const float* logmel, const int64_t* lens, int32_t B, int32_t n_mels, int32_t t_max, int32_t n_coef, float* cep,
                     hipStream_t s) {
    TTS_REQUIRE(lens && (t_max == 0 || (logmel && cep)), "mel_cepstrum: null argument");
    TTS_REQUIRE(n_mels >= 1 && n_mels <= OBJ_MAXMEL, "mel_cepstrum: n_mels = %d outside [1, %d]", n_mels, OBJ_MAXMEL);
    TTS_REQUIRE(n_coef >= 1 && n_coef <= std::min(n_mels, OBJ_MAXCOEF), "mel_cepstrum: n_coef = %d outside [1, min(n_mels = %d, %d)]", n_coef,
                n_mels, OBJ_MAXCOEF);
    TTS_REQUIRE(B >= 1 && B <= 65535 && t_max >= 0, "mel_cepstrum: bad batch %d / t_max %d", B, t_max);
    if (t_max == 0) return 0;
    hipLaunchKernelGGL(mel_cepstrum_kernel, dim3((t_max + OBJ_FPB - 1) / OBJ_FPB, B), dim3(OBJ_FPB * OBJ_WAVES), 0, s, logmel, lens, n_mels,
                       t_max, n_coef, cep);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------------- evaluation along a path ----
template <int NV>
__device__ void block_sum(double (&v)[NV], double (*red)[OBJ_NT], int tid) {   // fixed tree: the same value for the same pair, batch or alone
    __syncthreads();
#pragma unroll
    for (int q = 0; q < NV; ++q) red[q][tid] = v[q];
    __syncthreads();
    for (int s = OBJ_NT / 2; s > 0; s >>= 1) {
        if (tid < s) {
#pragma unroll
            for (int q = 0; q < NV; ++q) red[q][tid] = red[q][tid] + red[q][tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NV; ++q) v[q] = red[q][0];
}

__device__ __forceinline__ bool voiced_hz(float f) { return isfinite(f) && f > 0.f; }

__global__ __launch_bounds__(OBJ_NT) void aligned_eval_kernel(const float* __restrict__ cep_a, const float* __restrict__ cep_b, int n_coef,
                                                              int first_coef, const float* __restrict__ mel_a,
                                                              const float* __restrict__ mel_b, int n_mels, const float* __restrict__ f0_a,
                                                              const float* __restrict__ f0_b, int ta_max, int tb_max,
                                                              const int* __restrict__ path, const int* __restrict__ path_len, double scale,
                                                              double* __restrict__ stats) {
    __shared__ double red[8][OBJ_NT];
    const int bi = blockIdx.x, tid = threadIdx.x, pmax = ta_max + tb_max;
    const int L = (ta_max > 0 && tb_max > 0) ? max(0, min(path_len[bi], pmax)) : 0;
    const int* pb = path + (int64_t)bi * pmax * 2;
    const float* ca = cep_a + (int64_t)bi * n_coef * ta_max;
    const float* cb = cep_b + (int64_t)bi * n_coef * tb_max;
    const float* ma = mel_a ? mel_a + (int64_t)bi * n_mels * ta_max : nullptr;
    const float* mb = mel_b ? mel_b + (int64_t)bi * n_mels * tb_max : nullptr;
    const float* fa = f0_a ? f0_a + (int64_t)bi * ta_max : nullptr;
    const float* fb = f0_b ? f0_b + (int64_t)bi * tb_max : nullptr;
    // 0 sum of cepstral distances, 1 sum |mel difference|, 2 both voiced, 3 voicing differs, 4 sum cents^2, 5 sum Hz^2, 6 sum f0_a, 7 sum f0_b
    double v[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int p = tid; p < L; p += OBJ_NT) {
        const int i = min(max(pb[2 * p], 0), ta_max - 1), j = min(max(pb[2 * p + 1], 0), tb_max - 1);
        double d2 = 0.0;
        for (int c = first_coef; c < n_coef; ++c) {
            const double d = (double)ca[(int64_t)c * ta_max + i] - (double)cb[(int64_t)c * tb_max + j];
            d2 += d * d;
        }
        v[0] += sqrt(d2);
        if (ma) {
            double s = 0.0;
            for (int m = 0; m < n_mels; ++m) s += fabs((double)ma[(int64_t)m * ta_max + i] - (double)mb[(int64_t)m * tb_max + j]);
            v[1] += s;
        }
        if (fa) {
            const float x = fa[i], y = fb[j];
            const bool va = voiced_hz(x), vb = voiced_hz(y);
            if (va != vb) v[3] += 1.0;
            if (va && vb) {
                const double xd = (double)x, yd = (double)y, ce = 1200.0 * log2(xd / yd), dh = xd - yd;
                v[2] += 1.0;
                v[4] += ce * ce;
                v[5] += dh * dh;
                v[6] += xd;
                v[7] += yd;
            }
        }
    }
    block_sum<8>(v, red, tid);
    const double nvv = v[2];
    double cs[3] = {0.0, 0.0, 0.0};                                // centred sums: xx, yy, xy
    if (fa && nvv >= 2.0) {                                       // (block-uniform)
        const double mx = v[6] / nvv, my = v[7] / nvv;
        for (int p = tid; p < L; p += OBJ_NT) {
            const int i = min(max(pb[2 * p], 0), ta_max - 1), j = min(max(pb[2 * p + 1], 0), tb_max - 1);
            const float x = fa[i], y = fb[j];
            if (voiced_hz(x) && voiced_hz(y)) {
                const double dx = (double)x - mx, dy = (double)y - my;
                cs[0] += dx * dx;
                cs[1] += dy * dy;
                cs[2] += dx * dy;
            }
        }
        block_sum<3>(cs, red, tid);
    }
    if (tid == 0) {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double* st = stats + (int64_t)bi * TTSAMD_EVAL_STATS;
        st[0] = (double)L;
        st[1] = L ? scale * (v[0] / L) : nan;
        st[2] = (ma && L) ? v[1] / ((double)L * n_mels) : nan;
        st[3] = fa ? nvv : nan;
        st[4] = (fa && nvv > 0.0) ? sqrt(v[4] / nvv) : nan;
        st[5] = (fa && nvv > 0.0) ? sqrt(v[5] / nvv) : nan;
        st[6] = (fa && nvv >= 2.0 && cs[0] > 0.0 && cs[1] > 0.0) ? cs[2] / sqrt(cs[0] * cs[1]) : nan;
        st[7] = (fa && L) ? v[3] / L : nan;
    }
}

int32_t dtw_aligned_eval(const float* cep_a, const float* cep_b, int32_t n_coef, int32_t first_coef, const float* mel_a, const float* mel_b,
                         int32_t n_mels, const float* f0_a, const float* f0_b, int32_t B, int32_t ta_max, int32_t tb_max,
                         const int32_t* path, const int32_t* path_len, double scale, double* stats, hipStream_t s) {
    TTS_REQUIRE(path_len && stats && (ta_max == 0 || cep_a) && (tb_max == 0 || cep_b) && (ta_max + tb_max == 0 || path),
                "dtw_aligned_eval: null argument");
    TTS_REQUIRE(B >= 1 && ta_max >= 0 && tb_max >= 0, "dtw_aligned_eval: bad batch %d / lengths %d, %d", B, ta_max, tb_max);
    TTS_REQUIRE(n_coef >= 1 && first_coef >= 0 && first_coef < n_coef, "dtw_aligned_eval: first_coef = %d outside [0, n_coef = %d)", first_coef,
                n_coef);
    TTS_REQUIRE((mel_a == nullptr) == (mel_b == nullptr) && (f0_a == nullptr) == (f0_b == nullptr),
                "dtw_aligned_eval: mel_a / mel_b (and f0_a / f0_b) come as a pair or not at all");
    TTS_REQUIRE(!mel_a || n_mels >= 1, "dtw_aligned_eval: n_mels = %d with mels given", n_mels);
    hipLaunchKernelGGL(aligned_eval_kernel, dim3(B), dim3(OBJ_NT), 0, s, cep_a, cep_b, n_coef, first_coef, mel_a, mel_b, n_mels, f0_a, f0_b,
                       ta_max, tb_max, path, path_len, scale, stats);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
