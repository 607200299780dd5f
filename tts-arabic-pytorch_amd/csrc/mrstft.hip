// Multi-resolution STFT distance between the rows of two sample-aligned ragged mono batches (include/ttsamd.h states the arithmetic;
// DESIGN.md section 4): per resolution (N = n_fft, H = hop, W = win_length) the spectral convergence and the log-magnitude distance of
// the magnitudes of torch.stft's framing (periodic Hann of W centred in a frame of N, reflect padding by N / 2, 1 + n / H frames).
// The samples are fp32; everything after the load is float64.  No floating-point atomics; every reduction has a fixed order that
// depends on the row's own length only, so row b of a batch has the bits it has alone and two runs agree bit for bit.
//
// R + 1 launches for R resolutions:
//   1 .. R. mr_stft_kernel<N>, N / 4 threads, a block per MR_FPB consecutive frames of a row (grid: chunks of the widest possible row x
//      batch; a block past its row's frames leaves at once).  The block builds the twiddle table once, keeps the window at its four
//      samples of a frame in registers, and walks its frames in order: ref, then est through ws_fft<N> (ws_fft.hpp; the two signals
//      are transformed one after the other and not as the two halves of one complex transform, so that an identical pair gives
//      identical magnitudes and exactly 0).  The next transform's samples travel while this one runs.  Thread i owns bins i and
//      i + N / 4, thread 0 bin N / 2 as well; it adds its terms of (dS^2, S_ref^2, |d ln S|) frame after frame, and the block sums the
//      threads once at the end: a butterfly over the lanes of each wave, then the waves in ascending order.  Three doubles per chunk
//      go to the workspace.
//   R + 1. mr_stft_finish_kernel, one block per row: thread 3 r + q adds sum q of resolution r over the row's chunks in ascending order;
//      thread r forms (sc, mag) and the frame count, NaN / NaN / 0 for a row of N / 2 samples or fewer.
#include <atomic>

#include "ws_fft.hpp"

namespace ttsamd {

constexpr int MR_FPB = 16;                   // frames per block
constexpr int MR_MAX_RES = 8;
constexpr double MR_FLOOR = 1e-7;            // under the square root

struct MrPlan {
    int32_t R;
    int32_t N[MR_MAX_RES], H[MR_MAX_RES], W[MR_MAX_RES];
    int64_t Cm[MR_MAX_RES];                  // chunks of a row as long as the stride (>= 1: the arrays are never empty)
    int64_t off[MR_MAX_RES];                 // of the resolution's partial sums [B][Cm][3] in the workspace, in doubles
    int64_t bytes;
};

// false: refused (a batch outside 1 .. 65535, a stride that is negative or gives 2^31 frames or more, R outside 1 .. 8, a NULL array,
// N not 512 / 1024 / 2048, W outside 1 .. N, H < 1)
static bool mr_plan(int32_t B, int64_t stride, const int32_t* n_fft, const int32_t* hop, const int32_t* win, int32_t R, MrPlan& p) {
    if (B < 1 || B > 65535 || stride < 0 || stride >= ((int64_t)1 << 31)) return false;
    if (R < 1 || R > MR_MAX_RES || !n_fft || !hop || !win) return false;
    p.R = R;
    int64_t off = 0;
    for (int r = 0; r < R; ++r) {
        const int32_t N = n_fft[r], H = hop[r], W = win[r];
        if ((N != 512 && N != 1024 && N != 2048) || W < 1 || W > N || H < 1) return false;
        const int64_t Fm = stride > N / 2 ? 1 + stride / H : 0;
        if (Fm > 0x7fffffff) return false;
        p.N[r] = N;
        p.H[r] = H;
        p.W[r] = W;
        p.Cm[r] = Fm > 0 ? (Fm + MR_FPB - 1) / MR_FPB : 1;
        p.off[r] = off;
        off += align_up((int64_t)B * p.Cm[r] * 3, 32);          // 256 bytes
    }
    p.bytes = off * (int64_t)sizeof(double);
    return true;
}

// sample t of frame f: padded[f H + t] with padded[p] = x[reflect(p - N / 2)]; n > N / 2 keeps every index inside [0, n)
template <int N>
__device__ __forceinline__ void mr_load(const float* __restrict__ x, const int64_t n, const int64_t f, const int H, const int i,
                                        const double (&w)[4], float (&v)[4]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int64_t j = f * H + (i + (N / 4) * q) - N / 2;
        if (j < 0) j = -j;
        else if (j >= n) j = 2 * (n - 1) - j;
        v[q] = w[q] != 0.0 ? x[j] : 0.f;                       // outside the window nothing is read
    }
}

template <int N>
__global__ __launch_bounds__(N / 4) void mr_stft_kernel(const float* __restrict__ ref, const float* __restrict__ est, int64_t stride,
                                                        const int64_t* __restrict__ ns, int H, int W, int64_t Cm,
                                                        double* __restrict__ part) {
    constexpr int Q = N / 4, P = N / 2, NW = Q / 64;
    extern __shared__ __attribute__((aligned(16))) char mr_smem[];
    __shared__ double red[3][NW];
    double* buf = reinterpret_cast<double*>(mr_smem);          // 4 N doubles: (re | im) x 2
    double *twr = buf + 4 * N, *twi = buf + 5 * N;
    const int b = blockIdx.y, i = threadIdx.x;
    const int64_t n = ws_len(ns, b, stride);
    if (n <= P) return;                                        // uniform over the block: the finishing launch writes the NaNs
    const int64_t F = 1 + n / H, f0 = (int64_t)blockIdx.x * MR_FPB;
    if (f0 >= F) return;
    const int nf = (int)min((int64_t)MR_FPB, F - f0);
    ws_twiddles<N>(twr, twi);
    const int woff = (N - W) / 2;
    double w[4];                                               // the periodic Hann window of W, centred, at the thread's four samples
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int t = i + Q * q - woff;
        w[q] = (t >= 0 && t < W) ? 0.5 - 0.5 * cospi(2.0 * (double)t / (double)W) : 0.0;
    }
    const float* xr = ref + (int64_t)b * stride;
    const float* xe = est + (int64_t)b * stride;
    float cur[4], nxt[4] = {0.f, 0.f, 0.f, 0.f};
    mr_load<N>(xr, n, f0, H, i, w, cur);
    __syncthreads();                                           // the twiddles
    double sref[3] = {0.0, 0.0, 0.0}, lref[3] = {0.0, 0.0, 0.0};
    double acc[3] = {0.0, 0.0, 0.0};                            // dS^2, S_ref^2, |d ln S|
    for (int fi = 0; fi < nf; ++fi) {
        for (int sig = 0; sig < 2; ++sig) {
            double *ar = buf, *ai = buf + N, *br = buf + 2 * N, *bi = buf + 3 * N;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ar[i + Q * q] = w[q] * (double)cur[q];
                ai[i + Q * q] = 0.0;
            }
            if (sig == 0) mr_load<N>(xe, n, f0 + fi, H, i, w, nxt);
            else if (fi + 1 < nf) mr_load<N>(xr, n, f0 + fi + 1, H, i, w, nxt);
            __syncthreads();
            ws_fft<N, Q>(ar, ai, br, bi, twr, twi, i);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                if (q < 2 || i == 0) {                         // bins i, i + N / 4; thread 0: N / 2 too
                    const int k = q < 2 ? i + Q * q : P;
                    const double re = ar[k], im = ai[k];
                    const double S = sqrt(fmax(re * re + im * im, MR_FLOOR));
                    const double l = log(S);
                    if (sig == 0) {
                        sref[q] = S;
                        lref[q] = l;
                    } else {
                        const double d = sref[q] - S;
                        acc[0] += d * d;
                        acc[1] += sref[q] * sref[q];
                        acc[2] += fabs(lref[q] - l);
                    }
                }
            }
            __syncthreads();                                   // the result has been read: the buffers are free
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
        }
    }
    block_sum_fixed<NW, 3>(acc, red);
    if (i < 3) part[((int64_t)b * Cm + blockIdx.x) * 3 + i] = i == 0 ? acc[0] : i == 1 ? acc[1] : acc[2];
}

__global__ __launch_bounds__(64) void mr_stft_finish_kernel(MrPlan p, int64_t stride, const int64_t* __restrict__ ns,
                                                            const double* __restrict__ ws, double* __restrict__ out,
                                                            int32_t* __restrict__ frames) {
    __shared__ double sum[3 * MR_MAX_RES];
    const int b = blockIdx.x, t = threadIdx.x;
    const int64_t n = ws_len(ns, b, stride);
    if (t < 3 * p.R) {
        const int r = t / 3, q = t - 3 * r;
        double s = 0.0;
        if (n > p.N[r] / 2) {
            const int64_t F = 1 + n / p.H[r], C = (F + MR_FPB - 1) / MR_FPB;
            const double* part = ws + p.off[r] + (int64_t)b * p.Cm[r] * 3;
            for (int64_t c = 0; c < C; ++c) s += part[3 * c + q];
        }
        sum[t] = s;
    }
    __syncthreads();
    if (t < p.R) {
        const int64_t o = (int64_t)b * p.R + t;
        if (n > p.N[t] / 2) {
            const int64_t F = 1 + n / p.H[t];
            out[2 * o] = sqrt(sum[3 * t]) / sqrt(sum[3 * t + 1]);
            out[2 * o + 1] = sum[3 * t + 2] / ((double)F * (double)(p.N[t] / 2 + 1));
            frames[o] = (int32_t)F;
        } else {
            out[2 * o] = NAN;
            out[2 * o + 1] = NAN;
            frames[o] = 0;
        }
    }
}

template <int N>
static int32_t mr_launch(const float* ref, const float* est, int64_t stride, const int64_t* nsamples, int32_t B, int H, int W, int64_t Cm,
                         double* part, hipStream_t s) {
    static std::atomic<uint64_t> lds{0};
    constexpr int bytes = 6 * N * (int)sizeof(double);         // 24 / 48 / 96 KB
    TTS_CHECK_HIP(lds_opt_in((const void*)mr_stft_kernel<N>, bytes, lds));
    hipLaunchKernelGGL(mr_stft_kernel<N>, dim3((unsigned)Cm, B), dim3(N / 4), bytes, s, ref, est, stride, nsamples, H, W, Cm, part);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

static int32_t mr_stft(const float* ref, const float* est, int64_t stride, const int64_t* nsamples, int32_t B, const int32_t* n_fft,
                       const int32_t* hop, const int32_t* win, int32_t R, double* out, int32_t* frames, void* workspace,
                       int64_t workspace_bytes, hipStream_t s) {
    TTS_REQUIRE(nsamples && out && frames && workspace && n_fft && hop && win && ((ref && est) || stride == 0), "mr_stft: null argument");
    MrPlan p;
    TTS_REQUIRE(mr_plan(B, stride, n_fft, hop, win, R, p),
                "mr_stft: bad batch %d / stride / resolutions (1 .. 8 of n_fft 512 / 1024 / 2048, 1 <= win <= n_fft, hop >= 1)", B);
    TTS_REQUIRE(workspace_bytes >= p.bytes, "mr_stft: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)p.bytes);
    double* ws = (double*)workspace;
    for (int r = 0; r < R; ++r) {
        double* part = ws + p.off[r];
        if (p.N[r] == 512) TTS_TRY(mr_launch<512>(ref, est, stride, nsamples, B, p.H[r], p.W[r], p.Cm[r], part, s));
        else if (p.N[r] == 1024) TTS_TRY(mr_launch<1024>(ref, est, stride, nsamples, B, p.H[r], p.W[r], p.Cm[r], part, s));
        else TTS_TRY(mr_launch<2048>(ref, est, stride, nsamples, B, p.H[r], p.W[r], p.Cm[r], part, s));
    }
    hipLaunchKernelGGL(mr_stft_finish_kernel, dim3(B), dim3(64), 0, s, p, stride, nsamples, ws, out, frames);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd

using namespace ttsamd;

extern "C" {

int64_t ttsamd_mr_stft_workspace_bytes(int32_t batch, int64_t wave_stride, const int32_t* n_fft, const int32_t* hop, const int32_t* win,
                                       int32_t n_res) {
    MrPlan p;
    return mr_plan(batch, wave_stride, n_fft, hop, win, n_res, p) ? p.bytes : -1;
}

int32_t ttsamd_mr_stft(const float* ref, const float* est, int64_t wave_stride, const int64_t* nsamples, int32_t batch, const int32_t* n_fft,
                       const int32_t* hop, const int32_t* win, int32_t n_res, double* out, int32_t* frames, void* workspace,
                       int64_t workspace_bytes, void* stream) {
    return mr_stft(ref, est, wave_stride, nsamples, batch, n_fft, hop, win, n_res, out, frames, workspace, workspace_bytes,
                   (hipStream_t)stream);
}

}  // extern "C"
