// The alignment prior and the two alignment scores of the reference's aligner training, forward only, on the device:
//
//   prior           beta_binomial_prior_distribution and BetaBinomialInterpolator.__call__ (models/fastpitch/fastpitch/data_function.py:45-78),
//                   one cell per thread.  With integer a and b the beta-binomial pmf is a quotient of factorials: lf[n] = log n! is built once
//                   on the host in float64 (std::lgamma) and uploaded; a cell is nine table reads, one float64 exp and one rounding.
//                   mode 0 (exact): out[i-1][k] = betabinom(n = P, a = i, b = M + 1 - i).pmf(k), P = in_len, M = mel_len (n = P, not P - 1: the
//                   row does not add up to 1, as in the reference).  mode 1 (interpolated): the bank betabinom(n = bw, a = y + 1, b = bh - y)
//                   .pmf(x) of the rounded sizes (bw from the mel length, bh from the text length: the reference passes the rounded MEL
//                   length as the phoneme count, reproduced) sampled bilinearly as scipy.ndimage.zoom(order=1) does: output cell (o, p) at
//                   x = o (bw - 1) / (w - 1), y = p (bh - 1) / (h - 1).  The four bank values are computed in the cell; no bank is stored.
//   forward-sum     AttentionCTCLoss (attn_loss_function.py:20-61) = the CTC negative log-likelihood of the tokens 0 .. n_in - 1 in order
//                   under [blank_logprob, attn_logprob[t][:n_in]] log-softmaxed per frame.  Every label is distinct, so the skip transition
//                   is always allowed and the lattice is   tok'[l] = x[l + 1] + LSE(tok[l], blank before l, tok[l - 1]),
//                   blank' = x[0] + LSE(blank, token before it).  Two launches: the per-frame normaliser (a wave per frame, fully parallel)
//                   into the workspace, then the chain, one block per utterance as mas_kernel (aligner.hip) runs it: a lane owns up to four
//                   tokens (token l together with the blank AFTER it) in registers, the left neighbour comes by a cross-lane move and across
//                   waves through one double-buffered LDS word, the rows are loaded eight frames ahead.  The alphas stay in the log domain
//                   in float64: a rescaled linear chain loses the cells that are far below the frame's largest alpha, and with n_out close
//                   to n_in those are the only cells that can still reach the end.  With w[l] = LSE(tok[l], blank after l) a frame is
//                   tok'[l] = x[l + 1] + LSE(tok[l], w[l - 1]),  blank after l' = x[0] + w[l]:  two two-term LSEs per token (float64 exp and
//                   log1p are software polynomials, dozens of instructions each: they are the cost of the chain), one value moved per frame.
//                   The blank before token 0 has no second source: it is the running sum of x[0].  Tokens are dealt so that the waves share
//                   them evenly: R = ceil(L / 256) tokens per lane, ceil(L / 64 R) waves.
//   binarization    AttentionBinarizationLoss (attn_loss_function.py:64-71): per utterance the sum of log(max(soft, eps)) over the cells with
//                   hard == 1 and their count, float64, summed in a fixed order (one block per utterance, lane partials, a butterfly per wave,
//                   the waves in order).
//
// No gradient: these are the evaluation side.  ttsamd_set_precision does not reach this file.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <vector>

#include "kernels.hpp"

#pragma clang fp contract(off)                                   // a cell's value must not depend on the template instance that computes it

namespace ttsamd {

constexpr int AP_MAX_TABLE = 1 << 24;                            // log-factorial table: most entries (128 MB)
constexpr int CTC_MAX_L = TTSAMD_MAS_MAX_TOKENS;                 // 4 waves x 64 lanes x 4 tokens
constexpr int CTC_PF = 8;                                        // chain: frames in flight per lane
constexpr int BIN_THREADS = 1024;

// ---------------------------------------------------------------------------------------------------------------------------- prior ----
int32_t attn_prior_tables_host(int32_t n, double* lf) {
    TTS_REQUIRE(n >= 1 && n <= AP_MAX_TABLE && lf, "attn_prior_tables: n = %d outside [1, %d] or a null table", n, AP_MAX_TABLE);
    static std::mutex mu;                                        // std::lgamma writes the global signgam
    std::lock_guard<std::mutex> lk(mu);
    for (int k = 0; k < n; ++k) lf[k] = k < 2 ? 0.0 : std::lgamma((double)k + 1.0);
    return 0;
}

namespace {
struct PriorTable {
    double* dev = nullptr;
    int n = 0;
};
std::mutex g_prior_mu;
PriorTable g_prior[64];

// lf[0 .. need) on the current device; built and uploaded on first use and when a call needs more than is there
int32_t prior_table(int need, const double** out) {
    int dev = 0;
    TTS_CHECK_HIP(hipGetDevice(&dev));
    TTS_REQUIRE(dev >= 0 && dev < 64, "attn_prior: device %d (64 devices are tracked)", dev);
    std::lock_guard<std::mutex> lk(g_prior_mu);
    PriorTable& t = g_prior[dev];
    if (need > t.n) {
        int n = 8192;
        while (n < need) n *= 2;
        std::vector<double> host((size_t)n);
        TTS_TRY(attn_prior_tables_host(n, host.data()));
        double* p = nullptr;
        TTS_CHECK_HIP(hipMalloc((void**)&p, (size_t)n * sizeof(double)));
        hipError_t e = hipMemcpy(p, host.data(), (size_t)n * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(p);
            TTS_CHECK_HIP(e);
        }
        if (t.dev) (void)hipFree(t.dev);                         // (hipFree waits for the launches that still read the smaller table)
        t.dev = p;
        t.n = n;
    }
    *out = t.dev;
    return 0;
}
}  // namespace

// betabinom(n, a, b).pmf(k) for integers a, b >= 1 and 0 <= k < n
__device__ __forceinline__ double betabinom_pmf(const double* __restrict__ lf, int n, int a, int b, int k) {
    return exp((lf[n] - lf[k] - lf[n - k]) + (lf[k + a - 1] + lf[n - k + b - 1] - lf[n + a + b - 1]) - (lf[a - 1] + lf[b - 1] - lf[a + b - 1]));
}

// BetaBinomialInterpolator.round: max(1, np.round((val + 1) / to)) * to, halves to even
__device__ __forceinline__ int prior_round(int val, int to) { return max(1, (int)rint((double)(val + 1) / (double)to)) * to; }

template <typename T>
__global__ __launch_bounds__(256) void attn_prior_kernel(const double* __restrict__ lf, const int64_t* __restrict__ in_lens,
                                                         const int64_t* __restrict__ mel_lens, int n_tokens, int n_frames, int mode,
                                                         T* __restrict__ out) {
    const int b = blockIdx.y;
    const int64_t cell = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (cell >= (int64_t)n_frames * n_tokens) return;
    const int t = (int)(cell / n_tokens), l = (int)(cell - (int64_t)t * n_tokens);
    const int P = (int)max((int64_t)0, min(in_lens[b], (int64_t)n_tokens)), M = (int)max((int64_t)0, min(mel_lens[b], (int64_t)n_frames));
    double v = 0.0;
    if (t < M && l < P) {
        if (mode == 0) {
            v = betabinom_pmf(lf, P, t + 1, M - t, l);
        } else {
            const int bw = prior_round(M, 100), bh = prior_round(P, 20);
            const double x = M > 1 ? (double)t * ((double)(bw - 1) / (double)(M - 1)) : 0.0;
            const double y = P > 1 ? (double)l * ((double)(bh - 1) / (double)(P - 1)) : 0.0;
            const int x0 = min((int)floor(x), bw - 1), y0 = min((int)floor(y), bh - 1);
            const int x1 = min(x0 + 1, bw - 1), y1 = min(y0 + 1, bh - 1);
            const double fx = x - (double)x0, fy = y - (double)y0;
            const double v00 = betabinom_pmf(lf, bw, y0 + 1, bh - y0, x0), v01 = betabinom_pmf(lf, bw, y1 + 1, bh - y1, x0);
            const double v10 = betabinom_pmf(lf, bw, y0 + 1, bh - y0, x1), v11 = betabinom_pmf(lf, bw, y1 + 1, bh - y1, x1);
            v = (1.0 - fx) * ((1.0 - fy) * v00 + fy * v01) + fx * ((1.0 - fy) * v10 + fy * v11);
        }
    }
    out[(int64_t)b * n_frames * n_tokens + cell] = (T)v;
}

int32_t attn_prior(const int64_t* in_lens, const int64_t* mel_lens, int32_t B, int32_t L, int32_t T, int32_t mode, double scaling, void* out,
                   hipStream_t s) {
    TTS_REQUIRE(B >= 1 && B <= 65535 && L >= 0 && T >= 0, "attn_prior: bad batch %d / tokens %d / frames %d", B, L, T);
    TTS_REQUIRE((mode & ~TTSAMD_ATTN_PRIOR_F64) == 0 || (mode & ~TTSAMD_ATTN_PRIOR_F64) == 1,
                "attn_prior: mode %d (0 = exact, 1 = interpolated, + TTSAMD_ATTN_PRIOR_F64 for a float64 output)", mode);
    TTS_REQUIRE(scaling == 1.0, "attn_prior: scaling = %g: only scaling = 1 is built (the pmf in closed form needs integer Beta parameters)",
                scaling);
    if (L == 0 || T == 0) return 0;
    TTS_REQUIRE(in_lens && mel_lens && out, "attn_prior: null argument");
    TTS_REQUIRE((int64_t)T * L < ((int64_t)1 << 31) && (int64_t)T + L + 256 <= AP_MAX_TABLE, "attn_prior: %d x %d cells per utterance", T, L);
    const double* lf = nullptr;
    TTS_TRY(prior_table(T + L + 256, &lf));                      // exact: indices <= P + M; interpolated: <= bw + bh <= (M + 51) + (P + 11)
    const dim3 grid((unsigned)(((int64_t)T * L + 255) / 256), B);
    if (mode & TTSAMD_ATTN_PRIOR_F64)
        hipLaunchKernelGGL(attn_prior_kernel<double>, grid, dim3(256), 0, s, lf, in_lens, mel_lens, L, T, mode & 1, (double*)out);
    else
        hipLaunchKernelGGL(attn_prior_kernel<float>, grid, dim3(256), 0, s, lf, in_lens, mel_lens, L, T, mode & 1, (float*)out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------- forward-sum ----
__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

// log(exp(a) + exp(b)); -inf when both are
__device__ __forceinline__ double lse2(double a, double b) {
    const double m = fmax(a, b), n = fmin(a, b);
    const double ms = m == -INFINITY ? 0.0 : m;
    return m + log1p(exp(n - ms));
}

// lse[b][t] = log(exp(blank) + sum_{l < n_in} exp(lp[b][t][l])) for t < n_out: a wave per frame
__global__ __launch_bounds__(256) void attn_ctc_lse_kernel(const float* __restrict__ lp, const int64_t* __restrict__ in_lens,
                                                           const int64_t* __restrict__ out_lens, int T, int L, double blank,
                                                           double* __restrict__ lse) {
    const int b = blockIdx.y, lane = threadIdx.x & 63, t = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_in = (int)max((int64_t)0, min(in_lens[b], (int64_t)L)), n_out = (int)max((int64_t)0, min(out_lens[b], (int64_t)T));
    if (t >= n_out) return;                                      // (wave-uniform)
    const float* row = lp + ((int64_t)b * T + t) * L;
    double m = lane == 0 ? blank : -INFINITY;
    for (int l = lane; l < n_in; l += 64) m = fmax(m, (double)row[l]);
    m = wave_max_f64(m);
    double sum = lane == 0 ? exp(blank - m) : 0.0;
    for (int l = lane; l < n_in; l += 64) sum = sum + exp((double)row[l] - m);
    sum = wave_sum_f64(sum);
    if (lane == 0) lse[(int64_t)b * T + t] = m + log(sum);
}

// One block of ceil(L / 64 R) waves per utterance; lane `lane` of wave `wv` owns tokens 64 R wv + 64 r + lane, r = 0 .. R - 1.
template <int R>
__global__ __launch_bounds__(256) void attn_ctc_kernel(const float* __restrict__ lp, const int64_t* __restrict__ in_lens,
                                                       const int64_t* __restrict__ out_lens, int T, int L, double blank,
                                                       const double* __restrict__ lse, double* __restrict__ nll) {
    __shared__ double edge[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6;
    const int n_in = (int)max((int64_t)0, min(in_lens[b], (int64_t)L)), n_out = (int)max((int64_t)0, min(out_lens[b], (int64_t)T));
    if (n_in == 0 || n_out < n_in) {                             // (block-uniform) no token: the all-blank path, whose frames are certain;
        if (tid == 0) nll[b] = n_in == 0 ? 0.0 : (double)INFINITY;   // fewer frames than tokens: no path
        return;
    }
    const double NEG = -INFINITY;
    const float* ab = lp + (int64_t)b * T * L;
    const double* lb = lse + (int64_t)b * T;
    int tok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) tok[r] = 64 * R * wv + 64 * r + lane;
    // frame 0: the blank before token 0, or token 0
    const double lse0 = lb[0];
    double lead = blank - lse0;                                  // the blank before token 0: the running sum of x[t][0]
    double tk[R], af[R];                                         // token l, and the blank after it
#pragma unroll
    for (int r = 0; r < R; ++r) {
        tk[r] = tok[r] == 0 ? (double)ab[0] - lse0 : NEG;
        af[r] = NEG;
    }
    float ring[CTC_PF][R];
    double lring[CTC_PF];
    auto load_row = [&](int i, float* o, double& ls) {
#pragma unroll
        for (int r = 0; r < R; ++r) o[r] = (i < n_out && tok[r] < n_in) ? ab[(int64_t)i * L + tok[r]] : -INFINITY;
        ls = i < n_out ? lb[i] : 0.0;
    };
#pragma unroll
    for (int k = 0; k < CTC_PF; ++k) load_row(1 + k, ring[k], lring[k]);
    for (int i0 = 1; i0 < n_out; i0 += CTC_PF) {
#pragma unroll
        for (int k = 0; k < CTC_PF; ++k) {
            const int i = i0 + k;
            if (i >= n_out) break;                               // (block-uniform)
            double cur[R];
            const double ls = lring[k];
#pragma unroll
            for (int r = 0; r < R; ++r) cur[r] = (double)ring[k][r] - ls;
            load_row(i + CTC_PF, ring[k], lring[k]);             // refill the slot: frame i + CTC_PF is in flight while frames i .. are added
            double w[R], left[R];
#pragma unroll
            for (int r = 0; r < R; ++r) w[r] = lse2(tk[r], af[r]);
            if (nw > 1) {
                if (lane == 63) edge[i & 1][wv] = w[R - 1];
                __syncthreads();
            }
#pragma unroll
            for (int r = 0; r < R; ++r) left[r] = __shfl_up(w[r], 1, 64);
            {                                                    // token 64 q's left neighbour is lane 63 of q - 1
                double l0 = lead;
                if (nw > 1 && wv > 0) l0 = edge[i & 1][wv - 1];
                double first[R];
                first[0] = l0;
#pragma unroll
                for (int r = 1; r < R; ++r) first[r] = __shfl(w[r - 1], 63, 64);
                if (lane == 0) {
#pragma unroll
                    for (int r = 0; r < R; ++r) left[r] = first[r];
                }
            }
            const double xb = blank - ls;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                tk[r] = cur[r] + lse2(tk[r], left[r]);
                af[r] = xb + w[r];
            }
            lead = lead + xb;
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (tok[r] == n_in - 1) nll[b] = -lse2(tk[r], af[r]);
}

static int ctc_tokens_per_lane(int L) { return std::max(1, (L + 255) / 256); }

int64_t attn_ctc_workspace_bytes(int32_t B, int32_t T, int32_t L) {
    if (B < 1 || T < 0 || L < 0 || L > CTC_MAX_L) return -1;
    return align_up((int64_t)B * T * (int64_t)sizeof(double), 256);
}

int32_t attn_ctc_loss(const float* lp, const int64_t* in_lens, const int64_t* out_lens, int32_t B, int32_t T, int32_t L, double blank,
                      double* nll, void* ws, int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(in_lens && out_lens && nll && B >= 1 && B <= 65535 && T >= 0 && L >= 0,
                "attn_ctc_loss: bad argument (batch %d, frames %d, tokens %d)", B, T, L);
    TTS_REQUIRE(L <= CTC_MAX_L, "attn_ctc_loss: %d tokens, at most TTSAMD_MAS_MAX_TOKENS = %d are built", L, CTC_MAX_L);
    TTS_REQUIRE(T == 0 || L == 0 || lp, "attn_ctc_loss: null argument");
    TTS_REQUIRE((int64_t)T * L < ((int64_t)1 << 31), "attn_ctc_loss: %d x %d cells per utterance", T, L);
    TTS_REQUIRE(std::isfinite(blank), "attn_ctc_loss: blank_logprob = %g", blank);
    const int64_t need = attn_ctc_workspace_bytes(B, T, L);
    TTS_REQUIRE(ws_bytes >= need && (need == 0 || ws), "attn_ctc_loss: workspace of %lld bytes, %lld needed (ttsamd_attn_ctc_loss_workspace_bytes)",
                (long long)ws_bytes, (long long)need);
    TTS_REQUIRE(need == 0 || ((uintptr_t)ws & 7) == 0, "attn_ctc_loss: the workspace must be 8-byte aligned");
    double* lse = (double*)ws;
    if (T > 0) {
        hipLaunchKernelGGL(attn_ctc_lse_kernel, dim3((T + 3) / 4, B), dim3(256), 0, s, lp, in_lens, out_lens, T, L, blank, lse);
        TTS_CHECK_HIP(hipGetLastError());
    }
    const int R = ctc_tokens_per_lane(L), nw = std::max(1, (L + 64 * R - 1) / (64 * R));
    const dim3 grid(B), block(64 * nw);
    switch (R) {
        case 1: hipLaunchKernelGGL(attn_ctc_kernel<1>, grid, block, 0, s, lp, in_lens, out_lens, T, L, blank, lse, nll); break;
        case 2: hipLaunchKernelGGL(attn_ctc_kernel<2>, grid, block, 0, s, lp, in_lens, out_lens, T, L, blank, lse, nll); break;
        case 3: hipLaunchKernelGGL(attn_ctc_kernel<3>, grid, block, 0, s, lp, in_lens, out_lens, T, L, blank, lse, nll); break;
        default: hipLaunchKernelGGL(attn_ctc_kernel<4>, grid, block, 0, s, lp, in_lens, out_lens, T, L, blank, lse, nll); break;
    }
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// --------------------------------------------------------------------------------------------------------------------- binarization ----
__global__ __launch_bounds__(BIN_THREADS) void attn_bin_kernel(const float* __restrict__ hard, const float* __restrict__ soft, int64_t n,
                                                               double eps, double* __restrict__ sum_log, double* __restrict__ count) {
    __shared__ double ps[BIN_THREADS / 64], pc[BIN_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* hb = hard + (int64_t)b * n;
    const float* sb = soft + (int64_t)b * n;
    double s = 0.0, c = 0.0;
    for (int64_t e = tid; e < n; e += BIN_THREADS) {
        if (hb[e] == 1.f) {
            s = s + log(fmax((double)sb[e], eps));
            c = c + 1.0;
        }
    }
    s = wave_sum_f64(s);
    c = wave_sum_f64(c);
    if (lane == 0) {
        ps[wv] = s;
        pc[wv] = c;
    }
    __syncthreads();
    if (tid == 0) {
        double ts = 0.0, tc = 0.0;
        for (int w = 0; w < BIN_THREADS / 64; ++w) {
            ts = ts + ps[w];
            tc = tc + pc[w];
        }
        sum_log[b] = ts;
        count[b] = tc;
    }
}

int32_t attn_bin_loss(const float* hard, const float* soft, int32_t B, int32_t T, int32_t L, double eps, double* sum_log, double* count,
                      hipStream_t s) {
    TTS_REQUIRE(sum_log && count && B >= 1 && T >= 0 && L >= 0, "attn_bin_loss: bad argument (batch %d, frames %d, tokens %d)", B, T, L);
    TTS_REQUIRE((T == 0 || L == 0) || (hard && soft), "attn_bin_loss: null argument");
    TTS_REQUIRE(eps > 0.0 && std::isfinite(eps), "attn_bin_loss: eps = %g (a positive number)", eps);
    hipLaunchKernelGGL(attn_bin_kernel, dim3(B), dim3(BIN_THREADS), 0, s, hard, soft, (int64_t)T * L, eps, sum_log, count);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
