// Wave-against-wave scores (include/ttsamd.h states the arithmetic): STOI / ESTOI at 10 kHz, SI-SDR / SNR and a
// log-spectral distance between the rows of two sample-aligned ragged mono batches.  The samples are fp32; everything after the load is
// float64.  No floating-point atomics; every reduction has a fixed order that depends on the row's own length only, so row b of a batch
// has the bits it has alone and two runs agree bit for bit.
//
// The transform is ws_fft<N> of ws_fft.hpp (float64 Stockham passes in LDS): N = 512 serves STOI (the 256-sample frame zero-padded),
// N = 1024 the log-spectral distance.
//
// STOI in three launches:
//   1. stoi_select_kernel, one block per row: a wave per frame takes the windowed energy of the clean signal (lane l adds samples
//      l, l + 64, l + 128, l + 192 in that order, then a fixed butterfly over the lanes), the block takes the maximum, keeps the frames
//      within 40 dB of it and writes their indices in order (ballot + prefix counts) with (F, K).
//   2. stoi_band_kernel, a block per ST_FPB kept frames of a row: forms frame k of the overlap-added signal on the fly from kept frames
//      k - 1, k, k + 1, windows it again, transforms it and sums the fifteen bands; both signals, one after the other.
//   3. stoi_score_kernel, one block per row: STOI gives the (segment, band) pair (m', j) to thread (15 m' + j) mod 256, a thread's pairs
//      in ascending order; ESTOI gives segment m' to the group of 32 threads m' mod 8 (rows by 15 threads, then columns by 30).
// SI-SDR / SNR and the log-spectral distance are one block per row (the latter walks its row's frames: the entry takes no workspace).
// Block sums: a butterfly over the lanes of each wave, then the four waves' sums in a fixed order (ws_block_sum).
#include "ws_fft.hpp"

namespace ttsamd {

constexpr int ST_WIN = 256, ST_HOP = 128, ST_NFFT = 512, ST_BANDS = 15, ST_SEG = 30;
constexpr int ST_FPB = 4;                    // kept frames per block of the band kernel
constexpr int LSD_WIN = 1024, LSD_HOP = 256, LSD_BINS = 513;
constexpr int WS_T = 256;                    // threads of the one-block-per-row kernels
constexpr double WS_EPS = 2.220446049250313e-16;   // 2^-52

__constant__ int ST_LO[ST_BANDS] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174};
__constant__ int ST_HI[ST_BANDS] = {9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// sum over the block's WS_T threads in a fixed order: a butterfly over the lanes of each wave, then the four waves' sums as
// (0 + 1) + (2 + 3); every thread gets the sum.  red: WS_T / 64 doubles of LDS
__device__ __forceinline__ double ws_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    __syncthreads();                                           // red[] of the call before has been read
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// w = numpy.hanning(258)[1:-1]: 0.5 + 0.5 cos(pi (2 (i + 1) - 257) / 257)
__device__ __forceinline__ double stoi_window(const int i) {
    return 0.5 + 0.5 * cos(3.141592653589793 * (double)(2 * (i + 1) - 257) / 257.0);
}

struct StoiWs {
    int64_t Fm;                       // frames of a full stride (>= 1: the arrays are never empty)
    int32_t *kidx, *kcnt;             // [B][Fm] kept frames in order, [B] their count
    double *e, *tx, *ty;              // [B][Fm] frame energies in dB, [B][15][Fm] band magnitudes of the two signals
    int64_t bytes;
};

static void stoi_carve(void* base, int64_t B, int64_t stride, StoiWs& w) {
    w.Fm = stride >= ST_WIN ? (stride - ST_WIN) / ST_HOP + 1 : 1;
    Arena a(base, (int64_t)1 << 62);
    w.kidx = a.take<int32_t>(B * w.Fm);
    w.kcnt = a.take<int32_t>(B);
    w.e = a.take<double>(B * w.Fm);
    w.tx = a.take<double>(B * ST_BANDS * w.Fm);
    w.ty = a.take<double>(B * ST_BANDS * w.Fm);
    w.bytes = a.off;
}

__global__ __launch_bounds__(WS_T) void stoi_select_kernel(const float* __restrict__ ref, int64_t stride, const int64_t* __restrict__ ns,
                                                           int64_t Fm, double* __restrict__ e, int32_t* __restrict__ kidx,
                                                           int32_t* __restrict__ kcnt, int32_t* __restrict__ frames) {
    __shared__ double w[ST_WIN];
    __shared__ double wmax[WS_T / 64];
    __shared__ int wcnt[WS_T / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n = ws_len(ns, b, stride);
    const int F = n >= ST_WIN ? (int)((n - ST_WIN) / ST_HOP + 1) : 0;
    const float* x = ref + (int64_t)b * stride;
    double* eb = e + (int64_t)b * Fm;
    int32_t* kb = kidx + (int64_t)b * Fm;
    w[tid] = stoi_window(tid);
    __syncthreads();
    double m = -INFINITY;
    for (int f = wv; f < F; f += WS_T / 64) {
        const float* xf = x + (int64_t)f * ST_HOP;
        double s = 0.0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double v = w[lane + 64 * q] * (double)xf[lane + 64 * q];
            s += v * v;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        const double ef = 20.0 * log10(sqrt(s) + WS_EPS);
        if (lane == 0) eb[f] = ef;
        m = fmax(m, ef);
    }
    if (lane == 0) wmax[wv] = m;
    __syncthreads();                                           // eb[] of this block's own writes and the four maxima
    m = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    int run = 0;
    for (int base = 0; base < F; base += WS_T) {
        const int f = base + tid;
        const bool keep = f < F && (m - 40.0 - eb[f] < 0.0);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wcnt[wv] = __popcll(mask);
        __syncthreads();
        int off = run;
        for (int q = 0; q < wv; ++q) off += wcnt[q];
        if (keep) kb[off + __popcll(mask & ((1ull << lane) - 1ull))] = f;
        run += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
    if (tid == 0) {
        kcnt[b] = run;
        frames[2 * b] = F;
        frames[2 * b + 1] = run;
    }
}

__global__ __launch_bounds__(ST_WIN) void stoi_band_kernel(const float* __restrict__ ref, const float* __restrict__ deg, int64_t stride,
                                                           int64_t Fm, const int32_t* __restrict__ kidx, const int32_t* __restrict__ kcnt,
                                                           double* __restrict__ tx, double* __restrict__ ty, double* __restrict__ out_x,
                                                           double* __restrict__ out_y, int f_max) {
    __shared__ double buf[4 * ST_NFFT];
    __shared__ double tw[2 * ST_NFFT];
    __shared__ double w[ST_WIN];
    const int b = blockIdx.y, i = threadIdx.x;
    const int K = kcnt[b];
    const int32_t* kb = kidx + (int64_t)b * Fm;
    double *twr = tw, *twi = tw + ST_NFFT;
    ws_twiddles<ST_NFFT>(twr, twi);
    w[i] = stoi_window(i);
    __syncthreads();
    for (int q = 0; q < ST_FPB; ++q) {
        const int k = blockIdx.x * ST_FPB + q;                 // uniform over the block
        if (k >= K) {                                          // past the row's kept frames: zeros for the caller, nothing else
            if (i < ST_BANDS && k < f_max) {
                if (out_x) out_x[((int64_t)b * ST_BANDS + i) * f_max + k] = 0.0;
                if (out_y) out_y[((int64_t)b * ST_BANDS + i) * f_max + k] = 0.0;
            }
            continue;
        }
        const int64_t cur = (int64_t)kb[k] * ST_HOP;
        const int64_t prev = k > 0 ? (int64_t)kb[k - 1] * ST_HOP : -1, next = k + 1 < K ? (int64_t)kb[k + 1] * ST_HOP : -1;
        for (int sig = 0; sig < 2; ++sig) {
            const float* x = (sig ? deg : ref) + (int64_t)b * stride;
            double *ar = buf, *ai = buf + ST_NFFT, *br = buf + 2 * ST_NFFT, *bi = buf + 3 * ST_NFFT;
            double z = w[i] * (double)x[cur + i];              // the overlap-added signal at 128 k + i: this frame's term ...
            if (i < ST_HOP) {
                if (prev >= 0) z += w[i + ST_HOP] * (double)x[prev + ST_HOP + i];   // ... and the second half of the kept frame before it
            } else if (next >= 0) {
                z += w[i - ST_HOP] * (double)x[next + i - ST_HOP];                 // ... or the first half of the one behind
            }
            ar[i] = w[i] * z;
            ai[i] = 0.0;
            ar[i + ST_WIN] = 0.0;
            ai[i + ST_WIN] = 0.0;
            __syncthreads();
            ws_fft<ST_NFFT>(ar, ai, br, bi, twr, twi, i);
            const double re = ar[i], im = ai[i];               // bins 0 .. 255; the bands end at 218
            __syncthreads();
            br[i] = re * re + im * im;
            __syncthreads();
            if (i < ST_BANDS) {
                double s = 0.0;
                for (int c = ST_LO[i]; c < ST_HI[i]; ++c) s += br[c];
                const double t = sqrt(s);
                (sig ? ty : tx)[((int64_t)b * ST_BANDS + i) * Fm + k] = t;
                double* o = sig ? out_y : out_x;
                if (o && k < f_max) o[((int64_t)b * ST_BANDS + i) * f_max + k] = t;
            }
            __syncthreads();
        }
    }
}

// one (segment, band) pair of STOI: rows x, y of 30 frames (stride 1)
__device__ __forceinline__ double stoi_pair(const double* __restrict__ x, const double* __restrict__ y) {
    const double clip = 1.0 + pow(10.0, 15.0 / 20.0);
    double sx = 0.0, sy = 0.0;
    for (int t = 0; t < ST_SEG; ++t) {
        sx += x[t] * x[t];
        sy += y[t] * y[t];
    }
    const double c = sqrt(sx) / (sqrt(sy) + WS_EPS);
    double mx = 0.0, my = 0.0;
    for (int t = 0; t < ST_SEG; ++t) {
        mx += x[t];
        my += fmin(c * y[t], x[t] * clip);
    }
    mx /= (double)ST_SEG;
    my /= (double)ST_SEG;
    double vx = 0.0, vy = 0.0;
    for (int t = 0; t < ST_SEG; ++t) {
        const double a = x[t] - mx, d = fmin(c * y[t], x[t] * clip) - my;
        vx += a * a;
        vy += d * d;
    }
    const double nx = sqrt(vx) + WS_EPS, ny = sqrt(vy) + WS_EPS;
    double s = 0.0;
    for (int t = 0; t < ST_SEG; ++t) s += ((x[t] - mx) / nx) * ((fmin(c * y[t], x[t] * clip) - my) / ny);
    return s;
}

// column t of one ESTOI segment of one signal: rows normalised with (mean, norm + EPS) from st[0 .. 14], st[15 .. 29], then the column
// centred over the bands and divided by (norm + EPS), into v[15]
__device__ __forceinline__ void estoi_column(const double* __restrict__ tb, const int64_t Fm, const int64_t col, const double* st, double* v) {
    double m = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) {
        v[j] = (tb[j * Fm + col] - st[j]) / st[ST_BANDS + j];
        m += v[j];
    }
    m /= (double)ST_BANDS;
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) {
        v[j] -= m;
        s += v[j] * v[j];
    }
    const double nrm = sqrt(s) + WS_EPS;
#pragma unroll
    for (int j = 0; j < ST_BANDS; ++j) v[j] /= nrm;
}

__global__ __launch_bounds__(WS_T) void stoi_score_kernel(int64_t Fm, const int32_t* __restrict__ kcnt, const double* __restrict__ tx,
                                                          const double* __restrict__ ty, int extended, double* __restrict__ score) {
    __shared__ double red[WS_T / 64];
    __shared__ double st[WS_T / 32][4 * ST_BANDS];             // per group: mean and norm + EPS of the 15 rows, of x and of y
    __shared__ double colv[WS_T / 32][32];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int K = kcnt[b];
    if (K < ST_SEG) {                                          // uniform over the block
        if (tid == 0) score[b] = 1e-5;
        return;
    }
    const int M = K - ST_SEG + 1;
    const double* xb = tx + (int64_t)b * ST_BANDS * Fm;
    const double* yb = ty + (int64_t)b * ST_BANDS * Fm;
    double acc = 0.0;
    if (!extended) {
        for (int64_t q = tid; q < (int64_t)M * ST_BANDS; q += WS_T) {
            const int m = (int)(q / ST_BANDS), j = (int)(q - (int64_t)m * ST_BANDS);
            acc += stoi_pair(xb + j * Fm + m, yb + j * Fm + m);
        }
        const double total = ws_block_sum(acc, red);
        if (tid == 0) score[b] = total / (15.0 * (double)M);
        return;
    }
    const int g = tid >> 5, l = tid & 31;
    for (int m0 = 0; m0 < M; m0 += WS_T / 32) {                // the same trip count for every thread: the barriers are the block's
        const int m = m0 + g;
        if (m < M && l < ST_BANDS) {
            for (int sig = 0; sig < 2; ++sig) {
                const double* r = (sig ? yb : xb) + l * Fm + m;
                double mu = 0.0;
                for (int t = 0; t < ST_SEG; ++t) mu += r[t];
                mu /= (double)ST_SEG;
                double s = 0.0;
                for (int t = 0; t < ST_SEG; ++t) s += (r[t] - mu) * (r[t] - mu);
                st[g][2 * ST_BANDS * sig + l] = mu;
                st[g][2 * ST_BANDS * sig + ST_BANDS + l] = sqrt(s) + WS_EPS;
            }
        }
        __syncthreads();
        if (m < M && l < ST_SEG) {
            double vx[ST_BANDS], vy[ST_BANDS];
            estoi_column(xb, Fm, m + l, st[g], vx);
            estoi_column(yb, Fm, m + l, st[g] + 2 * ST_BANDS, vy);
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < ST_BANDS; ++j) s += vx[j] * vy[j];
            colv[g][l] = s;
        }
        __syncthreads();
        if (m < M && l == 0) {
            double s = 0.0;
            for (int t = 0; t < ST_SEG; ++t) s += colv[g][t];
            acc += s;
        }
    }
    const double total = ws_block_sum(acc, red);
    if (tid == 0) score[b] = total / (double)ST_SEG / (double)M;
}

static int32_t stoi(const float* ref, const float* deg, int64_t stride, const int64_t* nsamples, int32_t B, int32_t extended, double* score,
                    int32_t* frames, double* tob_ref, double* tob_deg, int32_t f_max, void* workspace, int64_t workspace_bytes,
                    hipStream_t s) {
    TTS_REQUIRE(nsamples && score && frames && workspace && ((ref && deg) || stride == 0), "stoi: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && stride >= 0 && stride < ((int64_t)1 << 31), "stoi: bad batch %d / stride", B);
    TTS_REQUIRE(f_max >= 0, "stoi: f_max = %d", f_max);
    StoiWs w;
    stoi_carve(nullptr, B, stride, w);
    TTS_REQUIRE(workspace_bytes >= w.bytes, "stoi: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)w.bytes);
    stoi_carve(workspace, B, stride, w);
    hipLaunchKernelGGL(stoi_select_kernel, dim3(B), dim3(WS_T), 0, s, ref, stride, nsamples, w.Fm, w.e, w.kidx, w.kcnt, frames);
    TTS_CHECK_HIP(hipGetLastError());
    const int64_t cover = (tob_ref || tob_deg) && f_max > w.Fm ? (int64_t)f_max : w.Fm;   // the zeros behind K reach f_max
    hipLaunchKernelGGL(stoi_band_kernel, dim3((unsigned)((cover + ST_FPB - 1) / ST_FPB), B), dim3(ST_WIN), 0, s, ref, deg, stride, w.Fm,
                       w.kidx, w.kcnt, w.tx, w.ty, tob_ref, tob_deg, f_max);
    TTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(stoi_score_kernel, dim3(B), dim3(WS_T), 0, s, w.Fm, w.kcnt, w.tx, w.ty, extended, score);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(WS_T) void wave_sdr_kernel(const float* __restrict__ ref, const float* __restrict__ est, int64_t stride,
                                                        const int64_t* __restrict__ ns, int zero_mean, double* __restrict__ out) {
    __shared__ double red[WS_T / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t n = ws_len(ns, b, stride);
    const float* r = ref + (int64_t)b * stride;
    const float* e = est + (int64_t)b * stride;
    double mr = 0.0, me = 0.0;
    if (zero_mean) {
        double sr = 0.0, se = 0.0;
        for (int64_t i = tid; i < n; i += WS_T) {
            sr += (double)r[i];
            se += (double)e[i];
        }
        mr = ws_block_sum(sr, red) / (double)n;
        me = ws_block_sum(se, red) / (double)n;
    }
    double rr = 0.0, re = 0.0, dd = 0.0;
    for (int64_t i = tid; i < n; i += WS_T) {
        const double x = (double)r[i] - mr, y = (double)e[i] - me;
        rr += x * x;
        re += y * x;
        dd += (x - y) * (x - y);
    }
    rr = ws_block_sum(rr, red);
    re = ws_block_sum(re, red);
    dd = ws_block_sum(dd, red);
    const double alpha = re / rr;
    double tt = 0.0, nn = 0.0;
    for (int64_t i = tid; i < n; i += WS_T) {
        const double x = alpha * ((double)r[i] - mr), y = (double)e[i] - me;
        tt += x * x;
        nn += (x - y) * (x - y);
    }
    tt = ws_block_sum(tt, red);
    nn = ws_block_sum(nn, red);
    if (tid == 0) {
        out[2 * b] = 10.0 * log10(tt / nn);
        out[2 * b + 1] = 10.0 * log10(rr / dd);
    }
}

static int32_t wave_sdr(const float* ref, const float* est, int64_t stride, const int64_t* nsamples, int32_t B, int32_t zero_mean,
                        double* out, hipStream_t s) {
    TTS_REQUIRE(nsamples && out && ((ref && est) || stride == 0), "wave_sdr: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && stride >= 0, "wave_sdr: bad batch %d / stride", B);
    hipLaunchKernelGGL(wave_sdr_kernel, dim3(B), dim3(WS_T), 0, s, ref, est, stride, nsamples, zero_mean, out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(WS_T) void lsd_kernel(const float* __restrict__ ref, const float* __restrict__ est, int64_t stride,
                                                   const int64_t* __restrict__ ns, double* __restrict__ out) {
    static_assert(LSD_WIN == 4 * WS_T, "a thread of lsd_kernel owns four samples of a frame");
    __shared__ double buf[4 * LSD_WIN];
    __shared__ double tw[2 * LSD_WIN];
    __shared__ double lref[LSD_BINS];
    __shared__ double red[WS_T / 64];
    const int b = blockIdx.x, i = threadIdx.x;
    const int64_t n = ws_len(ns, b, stride);
    const int64_t F = n >= LSD_WIN ? (n - LSD_WIN) / LSD_HOP + 1 : 0;
    double *twr = tw, *twi = tw + LSD_WIN;
    ws_twiddles<LSD_WIN>(twr, twi);
    double w[4];                                               // the periodic Hann window at the thread's four samples
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = 0.5 - 0.5 * cospi((double)(i + WS_T * q) / (double)(LSD_WIN / 2));
    __syncthreads();
    double total = 0.0;                                        // the frames in order (the same value in every thread)
    const float* xr = ref + (int64_t)b * stride;
    const float* xe = est + (int64_t)b * stride;
    float cur[4], nxt[4] = {0.f, 0.f, 0.f, 0.f};               // the thread's samples of this transform and of the one behind it
    if (F > 0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) cur[q] = xr[i + WS_T * q];
    }
    for (int64_t f = 0; f < F; ++f) {
        double d = 0.0;
        for (int sig = 0; sig < 2; ++sig) {
            double *ar = buf, *ai = buf + LSD_WIN, *br = buf + 2 * LSD_WIN, *bi = buf + 3 * LSD_WIN;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ar[i + WS_T * q] = w[q] * (double)cur[q];
                ai[i + WS_T * q] = 0.0;
            }
            // the next transform's samples travel while this one runs: est of this frame, then ref of the next (f + 1 < F: inside the row)
            if (sig == 0 || f + 1 < F) {
                const float* x = sig == 0 ? xe + f * LSD_HOP : xr + (f + 1) * LSD_HOP;
#pragma unroll
                for (int q = 0; q < 4; ++q) nxt[q] = x[i + WS_T * q];
            }
            __syncthreads();
            ws_fft<LSD_WIN>(ar, ai, br, bi, twr, twi, i);
            for (int k = i; k < LSD_BINS; k += WS_T) {         // thread 0 takes bins 0, 256 and 512
                const double re = ar[k], im = ai[k];
                const double l = 10.0 * log10(fmax(re * re + im * im, 1e-10));
                if (sig == 0) {
                    lref[k] = l;                               // read back by the same thread
                } else {
                    const double t = lref[k] - l;
                    d += t * t;
                }
            }
            __syncthreads();                                   // the result has been read: the buffers are free
#pragma unroll
            for (int q = 0; q < 4; ++q) cur[q] = nxt[q];
        }
        total += sqrt(ws_block_sum(d, red) / (double)LSD_BINS);
    }
    if (i == 0) {
        out[2 * b] = total / (double)F;                        // 0 / 0 = NaN for a row without a frame
        out[2 * b + 1] = (double)F;
    }
}

static int32_t log_spectral_distance(const float* ref, const float* est, int64_t stride, const int64_t* nsamples, int32_t B, double* out,
                                     hipStream_t s) {
    TTS_REQUIRE(nsamples && out && ((ref && est) || stride == 0), "log_spectral_distance: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && stride >= 0, "log_spectral_distance: bad batch %d / stride", B);
    hipLaunchKernelGGL(lsd_kernel, dim3(B), dim3(WS_T), 0, s, ref, est, stride, nsamples, out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd

using namespace ttsamd;

extern "C" {

int64_t ttsamd_stoi_workspace_bytes(int32_t batch, int64_t wave_stride) {
    if (batch < 1 || wave_stride < 0 || wave_stride >= ((int64_t)1 << 31)) return -1;
    StoiWs w;
    stoi_carve(nullptr, batch, wave_stride, w);
    return w.bytes;
}

int32_t ttsamd_stoi(const float* ref, const float* deg, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t extended,
                    double* score, int32_t* frames, double* tob_ref, double* tob_deg, int32_t f_max, void* workspace,
                    int64_t workspace_bytes, void* stream) {
    return stoi(ref, deg, wave_stride, nsamples, batch, extended, score, frames, tob_ref, tob_deg, f_max, workspace, workspace_bytes,
                (hipStream_t)stream);
}

int32_t ttsamd_wave_sdr(const float* ref, const float* est, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t zero_mean,
                        double* out, void* stream) {
    return wave_sdr(ref, est, wave_stride, nsamples, batch, zero_mean, out, (hipStream_t)stream);
}

int32_t ttsamd_log_spectral_distance(const float* ref, const float* est, int64_t wave_stride, const int64_t* nsamples, int32_t batch,
                                     double* out, void* stream) {
    return log_spectral_distance(ref, est, wave_stride, nsamples, batch, out, (hipStream_t)stream);
}

}  // extern "C"
