// Oversmoothing analysis on the device: replaces the arithmetic of the reference's utils/oversmoothing.py (and its older twin
// utils/metrics.py): per-frame cepstral series, their summary / standardisation, DTW, and the error along the DTW path.
//
//   cepstral_series   mel [B][n_mels][T] -> series [B][4][T] (HQER, CSlope, CCentroid, CRoll95; oversmoothing.py:306-521).  A block owns
//                     16 frames; the DFT across the bands (n_mels = 80 / 100: no power of two) is a direct sum against a twiddle table
//                     in LDS.  Everything up to the final rounding is float64 (the window is np.hanning rounded ONCE to fp32, as the
//                     reference holds it): 6.5 kFLOP per frame is nothing for the fp64 pipes, and the result sits within an fp32 ulp of
//                     the exact value instead of a summation order away from it.
//   series_summary    one block per series: count / mean / median of the finite values (bitonic sort in LDS), and the copy the alignment
//                     uses: NaNs interpolated as np.interp does, z-scored with mean / population std from float64 rounded to fp32, the
//                     division itself in fp32 (oversmoothing.py:69-105).
//   dtw               one block per alignment, anti-diagonal wavefront (oversmoothing.py:110-200).  Thread t owns rows 4t .. 4t + 3: it
//                     keeps their cells of the last two anti-diagonals in registers, gets row 4t - 1 from its neighbour through LDS (one
//                     barrier per diagonal), computes the local costs of four diagonals at a time (4 a-values and 7 b-values per
//                     channel serve 16 cells) and stores the backpointers of its 4 rows x 4 diagonals as ONE 32-bit word, diagonal-major: the workspace
//                     is about half a byte per cell and no accumulated-cost matrix exists anywhere.  All arithmetic is single IEEE fp32
//                     operations in the reference's order (contraction off, correctly rounded sqrt and division, the sum over channels
//                     in order), so path and cost are reproducible bit for bit and independent of the block shape.  The backtrack walks
//                     windows of 64 diagonals staged in LDS by the whole block and leaves the path in ascending time.
//   aligned_mae       mean |pred[path_i] - ref[path_j]| (oversmoothing.py:268-302), differences in fp32, the sum in float64.
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "kernels.hpp"

#pragma clang fp contract(off)

namespace ttsamd {

constexpr int OS_MAXMEL = 128, OS_MAXQ = OS_MAXMEL / 2 + 1, OS_FPB = 16;
constexpr int OS_MAX_T = 4096;          // series_summary: frames per series;  dtw: frames per side  (TTSAMD_OVERSMOOTH_MAX_FRAMES)
constexpr float DTW_INF = 1e30f;        // what an unwritten cell of D reads as (finite, as in the reference)

// ---------------------------------------------------------------------------------------------------------------- cepstral series ----
__global__ __launch_bounds__(256) void cepstral_series_kernel(const float* __restrict__ mel, const int64_t* __restrict__ lens, int n_mels,
                                                              int t_max, int center, int hann, int from_power, int q_c, int q1, int q2,
                                                              double eps, double roll_p, float hqer_scale,
                                                              float* __restrict__ power_out, float* __restrict__ series) {
    __shared__ double xs[OS_MAXMEL][OS_FPB + 1];
    __shared__ double pw[OS_MAXQ][OS_FPB + 1];
    __shared__ double tc[OS_MAXMEL], tsn[OS_MAXMEL], wn[OS_MAXMEL], mu[OS_FPB];
    const int b = blockIdx.y, t0 = blockIdx.x * OS_FPB, tid = threadIdx.x;
    const int n = (int)max((int64_t)0, min(lens[b], (int64_t)t_max));
    float* sb = series + (int64_t)b * 4 * t_max;
    const int Q = from_power ? n_mels : n_mels / 2 + 1;         // from_power: `mel` is the power itself, [B][Q][t_max]
    if (t0 >= n) {                                              // past the row's end: zeros
        for (int idx = tid; idx < 4 * OS_FPB; idx += 256) {
            const int k = idx / OS_FPB, tt = idx % OS_FPB;
            if (t0 + tt < t_max) sb[(int64_t)k * t_max + t0 + tt] = 0.f;
        }
        if (power_out) {
            for (int idx = tid; idx < Q * OS_FPB; idx += 256) {
                const int q = idx / OS_FPB, tt = idx % OS_FPB;
                if (t0 + tt < t_max) power_out[((int64_t)b * Q + q) * t_max + t0 + tt] = 0.f;
            }
        }
        return;
    }
    const float* mb = mel + (int64_t)b * n_mels * t_max;
    if (from_power) {
        for (int idx = tid; idx < Q * OS_FPB; idx += 256) {
            const int q = idx / OS_FPB, tt = idx % OS_FPB;
            pw[q][tt] = t0 + tt < n ? (double)mb[(int64_t)q * t_max + t0 + tt] : 0.0;
        }
    } else {
    for (int idx = tid; idx < n_mels * OS_FPB; idx += 256) {
        const int m = idx / OS_FPB, tt = idx % OS_FPB;
        xs[m][tt] = t0 + tt < n ? (double)mb[(int64_t)m * t_max + t0 + tt] : 0.0;
    }
    if (tid < n_mels) {
        tc[tid] = cospi(2.0 * tid / n_mels);
        tsn[tid] = sinpi(2.0 * tid / n_mels);
        // np.hanning(n): 0.5 - 0.5 cos(2 pi i / (n - 1)), [1] for n = 1; held in fp32 by the reference
        wn[tid] = hann ? (double)(float)(n_mels > 1 ? 0.5 - 0.5 * cospi(2.0 * tid / (n_mels - 1)) : 1.0) : 1.0;
    }
    __syncthreads();
    if (tid < OS_FPB) {
        double s = 0.0;
        for (int m = 0; m < n_mels; ++m) s += xs[m][tid];
        mu[tid] = center ? s / n_mels : 0.0;
    }
    __syncthreads();
    for (int idx = tid; idx < n_mels * OS_FPB; idx += 256) {
        const int m = idx / OS_FPB, tt = idx % OS_FPB;
        xs[m][tt] = (xs[m][tt] - mu[tt]) * wn[m];
    }
    __syncthreads();
    for (int idx = tid; idx < Q * OS_FPB; idx += 256) {
        const int q = idx / OS_FPB, tt = idx % OS_FPB;
        double re = 0.0, im = 0.0;
        int r = 0;
        for (int m = 0; m < n_mels; ++m) {
            const double x = xs[m][tt];
            re += x * tc[r];
            im += x * tsn[r];
            r += q;
            if (r >= n_mels) r -= n_mels;
        }
        pw[q][tt] = re * re + im * im;
    }
    }
    __syncthreads();
    if (power_out) {
        float* po = power_out + (int64_t)b * Q * t_max;
        for (int idx = tid; idx < Q * OS_FPB; idx += 256) {
            const int q = idx / OS_FPB, tt = idx % OS_FPB;
            if (t0 + tt < t_max) po[(int64_t)q * t_max + t0 + tt] = t0 + tt < n ? (float)pw[q][tt] : 0.f;
        }
    }
    if (tid < OS_FPB && t0 + tid < t_max) {
        const int tt = tid;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (t0 + tt < n) {
            const int qc = q_c >= 0 ? q_c : max(1, min((int)floor(0.25 * Q), Q - 1));
            double tot = 0.0, hi = 0.0, qp = 0.0, ysum = 0.0;
            for (int q = 1; q < Q; ++q) {
                const double p = pw[q][tt];
                tot += p;
                qp += q * p;
            }
            for (int q = q1; q <= q2; ++q) ysum += 10.0 * log10(pw[q][tt] + eps);
            for (int q = qc; q < Q; ++q) hi += pw[q][tt];
            o[0] = (float)((double)hqer_scale * (hi / (tot + 1e-12)));
            const int np_ = q2 - q1 + 1;
            if (np_ < 2) {
                o[1] = nanf("");
            } else {
                const double qm = 0.5 * (q1 + q2), ym = ysum / np_;
                double qv = 0.0, cov = 0.0;
                for (int q = q1; q <= q2; ++q) {
                    qv += (q - qm) * (q - qm);
                    cov += (q - qm) * (10.0 * log10(pw[q][tt] + eps) - ym);
                }
                o[1] = (float)((cov / np_) / (qv / np_ + 1e-12));
            }
            o[2] = (float)(qp / (tot + 1e-12));
            const double target = roll_p * (tot + 1e-12);
            double cum = 0.0;
            int roll = 1;
            for (int q = 1; q < Q; ++q) {
                cum += pw[q][tt];
                if (cum >= target) {
                    roll = q;
                    break;
                }
            }
            o[3] = (float)roll;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) sb[(int64_t)k * t_max + t0 + tt] = o[k];
    }
}

int32_t cepstral_series(const float* mel, const int64_t* lens, int32_t B, int32_t n_mels, int32_t t_max, int32_t center, int32_t hann,
                        int32_t q_c, float hqer_scale, float* power, float* series, hipStream_t s) {
    TTS_REQUIRE(lens && (t_max == 0 || (mel && series)), "cepstral_series: null argument");
    TTS_REQUIRE(n_mels >= 1 && n_mels <= OS_MAXMEL, "cepstral_series: n_mels = %d outside [1, %d]", n_mels, OS_MAXMEL);
    TTS_REQUIRE(B >= 1 && B <= 65535 && t_max >= 0, "cepstral_series: bad batch %d / t_max %d", B, t_max);
    const int Q = n_mels / 2 + 1;
    TTS_REQUIRE(q_c >= -1 && q_c <= Q, "cepstral_series: q_c = %d outside [0, Q = %d] (-1 = the default floor(0.25 Q))", q_c, Q);
    if (t_max == 0) return 0;
    hipLaunchKernelGGL(cepstral_series_kernel, dim3((t_max + OS_FPB - 1) / OS_FPB, B), dim3(256), 0, s, mel, lens, n_mels, t_max, center,
                       hann, 0, q_c, 1, Q - 1, 1e-8, 0.95, hqer_scale, power, series);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

int32_t cepstral_series_from_power(const float* power, const int64_t* lens, int32_t B, int32_t Q, int32_t t_max, int32_t q_c, int32_t q1,
                                   int32_t q2, double eps, double roll_p, float hqer_scale, float* series, hipStream_t s) {
    TTS_REQUIRE(lens && (t_max == 0 || (power && series)), "cepstral_series_from_power: null argument");
    TTS_REQUIRE(Q >= 1 && Q <= OS_MAXQ, "cepstral_series_from_power: Q = %d outside [1, %d]", Q, OS_MAXQ);
    TTS_REQUIRE(B >= 1 && B <= 65535 && t_max >= 0, "cepstral_series_from_power: bad batch %d / t_max %d", B, t_max);
    TTS_REQUIRE(q_c >= -1 && q_c <= Q, "cepstral_series_from_power: q_c = %d outside [0, Q = %d] (-1 = the default floor(0.25 Q))", q_c, Q);
    TTS_REQUIRE(q1 >= 0 && q2 <= Q - 1 && q2 >= q1 - 1, "cepstral_series_from_power: slope range [%d, %d] outside [0, Q - 1 = %d]", q1, q2, Q - 1);
    if (t_max == 0) return 0;
    hipLaunchKernelGGL(cepstral_series_kernel, dim3((t_max + OS_FPB - 1) / OS_FPB, B), dim3(256), 0, s, power, lens, Q, t_max, 0, 0, 1, q_c, q1,
                       q2, eps, roll_p, hqer_scale, (float*)nullptr, series);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// ----------------------------------------------------------------------------------------------------------------- series summary ----
template <typename T>
__device__ T block_sum_256(T v, T* red, int tid) {               // fixed tree: the same value for the same series, batch or alone
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void series_summary_kernel(const float* __restrict__ series, const int64_t* __restrict__ lens,
                                                             int n_series, int t_max, float* __restrict__ stats,
                                                             float* __restrict__ feat) {
    __shared__ float x[OS_MAX_T], key[OS_MAX_T];
    __shared__ short prv[OS_MAX_T], nxt[OS_MAX_T];
    __shared__ double red[256];
    __shared__ int cl[256], cf[256];
    const int row = blockIdx.x, b = row / n_series, tid = threadIdx.x;
    const int n = (int)max((int64_t)0, min(lens[b], (int64_t)t_max));
    const float* sr = series + (int64_t)row * t_max;
    float* fr = feat + (int64_t)row * t_max;
    int np2 = 2;
    while (np2 < n) np2 <<= 1;
    double fsum = 0.0;
    int fcnt = 0, ninf = 0;
    for (int i = tid; i < np2; i += 256) {
        const float v = i < n ? sr[i] : nanf("");
        if (i < n) x[i] = v;
        const bool fin = isfinite(v);
        key[i] = fin ? v : INFINITY;
        if (fin) {
            fsum += (double)v;
            ++fcnt;
        }
        if (i < n && isinf(v)) ++ninf;
    }
    const double tsum = block_sum_256<double>(fsum, red, tid);
    const int cnt = (int)block_sum_256<double>((double)fcnt, red, tid);
    const bool has_inf = block_sum_256<double>((double)ninf, red, tid) > 0.0;
    // bitonic sort of the finite values (the rest sorts to the end as +inf)
    for (int k = 2; k <= np2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = tid; i < np2; i += 256) {
                const int l = i ^ j;
                if (l > i) {
                    const float u = key[i], v = key[l];
                    if (((i & k) == 0) ? (u > v) : (u < v)) {
                        key[i] = v;
                        key[l] = u;
                    }
                }
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        float* st = stats + (int64_t)row * 3;
        st[0] = (float)cnt;
        st[1] = cnt ? (float)(tsum / cnt) : nanf("");
        st[2] = cnt ? ((cnt & 1) ? key[cnt / 2] : (key[cnt / 2 - 1] + key[cnt / 2]) * 0.5f) : nanf("");
    }
    __syncthreads();
    // nearest non-NaN neighbour on each side: chunks of 16 per thread, the carries across chunks by thread 0
    const int c0 = tid * 16;
    int last = -1, first = -1;
    for (int i = c0; i < min(c0 + 16, n); ++i) {
        if (!isnan(x[i])) last = i;
        prv[i] = (short)last;
    }
    for (int i = min(c0 + 16, n) - 1; i >= c0; --i) {
        if (!isnan(x[i])) first = i;
        nxt[i] = (short)first;
    }
    cl[tid] = last;
    cf[tid] = first;
    __syncthreads();
    if (tid == 0) {
        int carry = -1;
        for (int c = 0; c < 256; ++c) {
            const int own = cl[c];
            cl[c] = carry;                                      // the last non-NaN index before chunk c
            if (own >= 0) carry = own;
        }
        carry = -1;
        for (int c = 255; c >= 0; --c) {
            const int own = cf[c];
            cf[c] = carry;
            if (own >= 0) carry = own;
        }
    }
    __syncthreads();
    float* xi = key;                                            // the interpolated copy (the sorted keys are no longer needed)
    double isum = 0.0;
    for (int i = c0; i < min(c0 + 16, n); ++i) {
        float v = x[i];
        if (isnan(v)) {
            const int l = prv[i] >= 0 ? prv[i] : cl[tid], r = nxt[i] >= 0 ? nxt[i] : cf[tid];
            if (l < 0 && r < 0) {
                v = 0.f;                                        // all NaN
            } else if (l < 0) {
                v = x[r];
            } else if (r < 0) {
                v = x[l];
            } else {                                            // np.interp: float64 slope * (x - x0) + y0, rounded when stored
                const double slope = ((double)x[r] - (double)x[l]) / ((double)r - (double)l);
                v = (float)(slope * ((double)i - (double)l) + (double)x[l]);
            }
        }
        xi[i] = v;
        isum += (double)v;
    }
    const double m = n ? block_sum_256<double>(isum, red, tid) / n : 0.0;
    double vs = 0.0;
    for (int i = c0; i < min(c0 + 16, n); ++i) {
        const double d = (double)xi[i] - m;
        vs += d * d;
    }
    const double sd = n ? sqrt(block_sum_256<double>(vs, red, tid) / n) : 0.0;
    const float mf = (float)m, sf = (float)sd;
    const bool flat = has_inf || !isfinite(mf) || !isfinite(sf) || sf == 0.f;
    for (int i = tid; i < t_max; i += 256) fr[i] = (i < n && !flat) ? (xi[i] - mf) / sf : 0.f;
}

int32_t series_summary(const float* series, const int64_t* lens, int32_t B, int32_t n_series, int32_t t_max, float* stats, float* feat,
                       hipStream_t s) {
    TTS_REQUIRE(lens && stats && (t_max == 0 || (series && feat)), "series_summary: null argument");
    TTS_REQUIRE(B >= 1 && n_series >= 1 && (int64_t)B * n_series <= 0x7fffffff && t_max >= 0, "series_summary: bad batch %d x %d / t_max %d", B,
                n_series, t_max);
    TTS_REQUIRE(t_max <= OS_MAX_T, "series_summary: t_max = %d above the %d frames a block sorts in LDS", t_max, OS_MAX_T);
    hipLaunchKernelGGL(series_summary_kernel, dim3(B * n_series), dim3(256), 0, s, series, lens, n_series, t_max, stats, feat);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------- DTW ----
constexpr int DTW_WIN_D = 64, DTW_WIN_B = 24;                   // backtrack window: diagonals x bytes (= 96 rows)

static int dtw_row_words(int ta_max) { return (ta_max + 3) / 4; }   // one 32-bit word per thread: its 4 rows x 4 diagonals x 2 bits

int64_t dtw_workspace_bytes(int32_t B, int32_t ta_max, int32_t tb_max, int32_t M) {
    if (B < 1 || M < 1 || ta_max < 0 || tb_max < 0 || ta_max > OS_MAX_T || tb_max > OS_MAX_T) return -1;
    if (ta_max == 0 || tb_max == 0) return 0;
    return (int64_t)B * ((ta_max + tb_max - 1 + 3) / 4) * dtw_row_words(ta_max) * 4;
}

__global__ __launch_bounds__(1024) void dtw_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                   const int64_t* __restrict__ lens_a, const int64_t* __restrict__ lens_b, int M,
                                                   int ta_max, int tb_max, int metric, int window, int S, float* __restrict__ cost,
                                                   int* __restrict__ path, int* __restrict__ path_len, unsigned* ws) {
    __shared__ float edge[2][1024];
    __shared__ float bs[OS_MAX_T];                               // M = 1: the whole of b
    __shared__ ushort2 pathl[2 * OS_MAX_T];
    __shared__ unsigned char win[DTW_WIN_D][DTW_WIN_B];
    __shared__ int st[4];
    const int bi = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
    const int Ta = (int)max((int64_t)0, min(lens_a[bi], (int64_t)ta_max)), Tb = (int)max((int64_t)0, min(lens_b[bi], (int64_t)tb_max));
    const int pmax = ta_max + tb_max;
    int* pb = path + (int64_t)bi * pmax * 2;
    if (Ta == 0 || Tb == 0) {                                    // D[Ta][Tb] as the recurrence leaves it; no path
        if (t == 0) {
            cost[bi] = (Ta == 0 && Tb == 0) ? 0.f : DTW_INF;
            path_len[bi] = 0;
        }
        for (int k = t; k < 2 * pmax; k += nt) pb[k] = 0;
        return;
    }
    const float* ab = a + (int64_t)bi * M * ta_max;
    const float* bb = b + (int64_t)bi * M * tb_max;
    unsigned* wb = ws + (int64_t)bi * ((ta_max + tb_max - 1 + 3) / 4) * S;
    const int nd = Ta + Tb - 1, i0 = 4 * t;
    float p1[4], p2[4], e1 = DTW_INF, e2 = t ? DTW_INF : 0.f;      // thread 0's first diagonal predecessor is D[0][0] = 0
#pragma unroll
    for (int r = 0; r < 4; ++r) p1[r] = p2[r] = DTW_INF;
    int ia[4], jmin[4];
    unsigned jspan[4];                                           // row r is written for jmin <= j <= jmin + jspan (none: jmin past Tb)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = i0 + r, lo = window >= 0 ? max(0, i - window) : 0, hi = window >= 0 ? min(Tb - 1, i + window) : Tb - 1;
        ia[r] = min(i, Ta - 1);
        jmin[r] = (i < Ta && hi >= lo) ? lo : 0x40000000;
        jspan[r] = (i < Ta && hi >= lo) ? (unsigned)(hi - lo) : 0u;
    }
    float a1[4];                                                 // M = 1: this thread's rows of a, and b in LDS -- no load in the loop
    if (M == 1) {
#pragma unroll
        for (int r = 0; r < 4; ++r) a1[r] = ab[ia[r]];
        for (int j = t; j < Tb; j += nt) bs[j] = bb[j];
        __syncthreads();
    }
    for (int d0 = 0; d0 < nd; d0 += 4) {
        // local costs of rows i0 .. i0 + 3 on diagonals d0 .. d0 + 3: cell (r, dd) has j = jl + 3 - r + dd
        float c[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) c[r][dd] = 0.f;
        bool any = i0 < Ta && d0 + 3 - i0 >= 0 && d0 - (i0 + 3) < Tb;
        if (window >= 0) any = any && 2 * i0 - (d0 + 3) <= window && 2 * (i0 + 3) - d0 >= -window;
        if (any) {
            const int jl = d0 - i0 - 3;
            int jb[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) jb[q] = min(max(jl + q, 0), Tb - 1);
            if (M == 1) {
                float bv[7];
#pragma unroll
                for (int q = 0; q < 7; ++q) bv[q] = bs[jb[q]];
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int dd = 0; dd < 4; ++dd) {
                        const float x = a1[r], y = bv[3 - r + dd];
                        if (metric == 0) {
                            // sqrt(fl(d * d)) == |d| in binary floating point unless d * d leaves the normal range: the correctly
                            // rounded sqrt (15 instructions) only runs for such a d
                            const float df = x - y, sq = df * df;
                            c[r][dd] = (sq >= 1.17549435e-38f && sq <= 3.40282347e38f) ? fabsf(df) : sqrtf(sq);
                        } else {
                            const float den = sqrtf(0.f + x * x) * sqrtf(0.f + y * y) + 1e-12f;
                            float sim = (0.f + x * y) / den;
                            if (sim > 1.f) sim = 1.f;
                            else if (sim < -1.f) sim = -1.f;
                            c[r][dd] = 1.f - sim;
                        }
                    }
            } else if (metric == 0) {
                for (int k = 0; k < M; ++k) {
                    float av[4], bv[7];
#pragma unroll
                    for (int r = 0; r < 4; ++r) av[r] = ab[(int64_t)k * ta_max + ia[r]];
#pragma unroll
                    for (int q = 0; q < 7; ++q) bv[q] = bb[(int64_t)k * tb_max + jb[q]];
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int dd = 0; dd < 4; ++dd) {
                            const float df = av[r] - bv[3 - r + dd];
                            c[r][dd] = c[r][dd] + df * df;
                        }
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int dd = 0; dd < 4; ++dd) c[r][dd] = sqrtf(c[r][dd]);
            } else {
                float na[4], nb[7];
#pragma unroll
                for (int r = 0; r < 4; ++r) na[r] = 0.f;
#pragma unroll
                for (int q = 0; q < 7; ++q) nb[q] = 0.f;
                for (int k = 0; k < M; ++k) {
                    float av[4], bv[7];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        av[r] = ab[(int64_t)k * ta_max + ia[r]];
                        na[r] = na[r] + av[r] * av[r];
                    }
#pragma unroll
                    for (int q = 0; q < 7; ++q) {
                        bv[q] = bb[(int64_t)k * tb_max + jb[q]];
                        nb[q] = nb[q] + bv[q] * bv[q];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int dd = 0; dd < 4; ++dd) c[r][dd] = c[r][dd] + av[r] * bv[3 - r + dd];
                }
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int dd = 0; dd < 4; ++dd) {
                        const float den = sqrtf(na[r]) * sqrtf(nb[3 - r + dd]) + 1e-12f;
                        float sim = c[r][dd] / den;
                        if (sim > 1.f) sim = 1.f;
                        else if (sim < -1.f) sim = -1.f;
                        c[r][dd] = 1.f - sim;
                    }
            }
        }
        unsigned word = 0;
#pragma unroll
        for (int dd = 0; dd < 4; ++dd) {
            const int d = d0 + dd;
            if (d < nd) {                                        // (block-uniform)
                float nw[4];
                unsigned bits = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool act = (unsigned)(d - i0 - r - jmin[r]) <= jspan[r];
                    const float up = r ? p1[r ? r - 1 : 0] : e1, left = p1[r], dg = r ? p2[r ? r - 1 : 0] : e2;
                    float best = up;                             // strict <, in the order up, left, diag
                    unsigned bp = 0;
                    if (left < best) {
                        best = left;
                        bp = 1;
                    }
                    if (dg < best) {
                        best = dg;
                        bp = 2;
                    }
                    nw[r] = act ? c[r][dd] + best : DTW_INF;
                    bits |= (act ? bp : 3u) << (2 * r);
                }
                word |= bits << (8 * dd);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p2[r] = p1[r];
                    p1[r] = nw[r];
                }
                edge[d & 1][t] = nw[3];
                __syncthreads();
                e2 = e1;
                e1 = t ? edge[d & 1][t - 1] : DTW_INF;
            }
        }
        if (i0 < Ta) wb[(int64_t)(d0 >> 2) * S + t] = word;       // one store per four diagonals
    }
    if (t == (Ta - 1) / 4) {                                      // D[Ta][Tb]: the last diagonal's only cell
        float total = p1[0];
#pragma unroll
        for (int r = 1; r < 4; ++r) total = ((Ta - 1) & 3) == r ? p1[r] : total;
        cost[bi] = total;
    }
    // ---- backtrack from (Ta - 1, Tb - 1): windows of 16 diagonal groups (64 diagonals) x 24 bytes in LDS, walked by thread 0
    if (t == 0) {
        st[0] = Ta - 1;
        st[1] = Tb - 1;
        st[2] = 0;
        st[3] = 0;
    }
    __syncthreads();                                             // (also orders the block's backpointer stores before the loads below)
    while (true) {
        const int iw = st[0], jw = st[1];
        if (st[3]) break;
        const int dw = iw + jw, cb = ((iw >> 2) & ~7) - 16, dlo = ((dw >> 2) - (DTW_WIN_D / 4 - 1)) * 4;   // diagonals dlo .. dlo + 63
        for (int idx = t; idx < (DTW_WIN_D / 4) * DTW_WIN_B; idx += nt) {
            const int gq = idx / DTW_WIN_B, cc = idx % DTW_WIN_B, grp = (dlo >> 2) + gq, col = cb + cc;
            unsigned v = 0xffffffffu;
            if (dlo + 4 * gq >= 0 && col >= 0 && col < S) v = wb[(int64_t)grp * S + col];
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) win[4 * gq + dd][cc] = (unsigned char)(v >> (8 * dd));
        }
        __syncthreads();
        if (t == 0) {
            int i = iw, j = jw, L = st[2], done = 0;
            while (true) {
                if (i < 0 || j < 0) {
                    done = 1;
                    break;
                }
                const int k = i + j - dlo;
                if (k < 0) break;                                // next window
                const unsigned code = (win[k][(i >> 2) - cb] >> (2 * (i & 3))) & 3u;
                pathl[L] = make_ushort2((unsigned short)i, (unsigned short)j);
                if (code == 3u) {                                // a cell never written: stop without counting it
                    done = 1;
                    break;
                }
                ++L;
                if (code == 2u) {
                    --i;
                    --j;
                } else if (code == 0u) {
                    --i;
                } else {
                    --j;
                }
            }
            st[0] = i;
            st[1] = j;
            st[2] = L;
            st[3] = done;
        }
        __syncthreads();
    }
    const int L = st[2];
    if (t == 0) path_len[bi] = L;
    for (int k = t; k < pmax; k += nt) {
        const ushort2 p = k < L ? pathl[L - 1 - k] : make_ushort2(0, 0);
        pb[2 * k] = p.x;
        pb[2 * k + 1] = p.y;
    }
}

int32_t dtw(const float* a, const int64_t* lens_a, const float* b, const int64_t* lens_b, int32_t B, int32_t M, int32_t ta_max,
            int32_t tb_max, int32_t metric, int32_t window, float* cost, int32_t* path, int32_t* path_len, void* workspace,
            int64_t workspace_bytes, hipStream_t s) {
    TTS_REQUIRE(lens_a && lens_b && cost && path_len, "dtw: null argument");
    TTS_REQUIRE(B >= 1 && M >= 1 && ta_max >= 0 && tb_max >= 0, "dtw: bad batch %d / channels %d / lengths %d, %d", B, M, ta_max, tb_max);
    TTS_REQUIRE(ta_max <= OS_MAX_T && tb_max <= OS_MAX_T, "dtw: %d x %d frames, at most %d per side are built", ta_max, tb_max, OS_MAX_T);
    TTS_REQUIRE(metric == 0 || metric == 1, "dtw: metric %d (0 = L2, 1 = cosine)", metric);
    TTS_REQUIRE(window >= -1, "dtw: window %d (-1 = none, else the Sakoe-Chiba radius)", window);
    TTS_REQUIRE((ta_max == 0 || a) && (tb_max == 0 || b) && (ta_max + tb_max == 0 || path), "dtw: null argument");
    const int64_t need = dtw_workspace_bytes(B, ta_max, tb_max, M);
    TTS_REQUIRE(workspace_bytes >= need && (need == 0 || workspace), "dtw: workspace of %lld bytes, %lld needed (ttsamd_dtw_workspace_bytes)",
                (long long)workspace_bytes, (long long)need);
    TTS_REQUIRE(((uintptr_t)workspace & 3) == 0, "dtw: the workspace must be 4-byte aligned");
    const int nt = std::max(64, (((ta_max + 3) / 4) + 63) & ~63);
    hipLaunchKernelGGL(dtw_kernel, dim3(B), dim3(nt), 0, s, a, b, lens_a, lens_b, M, ta_max, tb_max, metric, window, dtw_row_words(ta_max),
                       cost, path, path_len, (unsigned*)workspace);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// -------------------------------------------------------------------------------------------------------------------- aligned MAE ----
__global__ __launch_bounds__(256) void aligned_mae_kernel(const float* __restrict__ pred, const float* __restrict__ ref, int ta_max,
                                                          int tb_max, const int* __restrict__ path, const int* __restrict__ path_len,
                                                          float* __restrict__ mae) {
    __shared__ double red[256];
    const int bi = blockIdx.x, tid = threadIdx.x, pmax = ta_max + tb_max;
    const int L = max(0, min(path_len[bi], pmax));
    const int* pb = path + (int64_t)bi * pmax * 2;
    double s = 0.0;
    for (int k = tid; k < L; k += 256) {
        const int i = min(max(pb[2 * k], 0), ta_max - 1), j = min(max(pb[2 * k + 1], 0), tb_max - 1);
        s += (double)fabsf(pred[(int64_t)bi * ta_max + i] - ref[(int64_t)bi * tb_max + j]);
    }
    const double tot = block_sum_256<double>(s, red, tid);
    if (tid == 0) mae[bi] = L ? (float)(tot / L) : nanf("");     // np.mean of nothing
}

int32_t dtw_aligned_mae(const float* pred, const float* ref, int32_t B, int32_t ta_max, int32_t tb_max, const int32_t* path,
                        const int32_t* path_len, float* mae, hipStream_t s) {
    TTS_REQUIRE(path_len && mae && (ta_max == 0 || pred) && (tb_max == 0 || ref) && (ta_max + tb_max == 0 || path),
                "dtw_aligned_mae: null argument");
    TTS_REQUIRE(B >= 1 && ta_max >= 0 && tb_max >= 0, "dtw_aligned_mae: bad batch %d / lengths %d, %d", B, ta_max, tb_max);
    hipLaunchKernelGGL(aligned_mae_kernel, dim3(B), dim3(256), 0, s, pred, ref, ta_max, tb_max, path, path_len, mae);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
