// Output levelling (include/ttsamd.h states the arithmetic): ITU-R BS.1770-4 integrated loudness and the peak per row
// of a ragged mono batch, and one gain per row towards a target -- what the reference's server does with `wave /= wave.abs().max();
// wave *= 0.99` (utils/app_utils.py:70-71), on the device and per row.
//
// K-weighting is a 4th-order recursive filter: a thread that walked a row would take 110 000 dependent steps per 5 s.  The filter is
// linear, so a row is cut into segments of S samples (S divides `step`, S <= 64) and filtered as a scan, in float64 throughout:
//   1. loud_zero_state_kernel: a thread per segment filters its S samples from a ZERO state and keeps the final state (4 doubles);
//      the block also takes max |x| over its tile.  The tile of 128 segments goes through LDS (coalesced loads, conflict-free reads:
//      the row stride of 65 words is odd).
//   2. loud_scan_kernel: one wave per row carries the state along the row, state_k = M state_(k-1) + zero_k with M = A^S (4 x 4, from
//      the host), 64 segments per step as a Kogge-Stone scan with M, M^2 .. M^32 (squared in LDS by the wave itself).
//   3. loud_energy_kernel: the thread of segment k filters it again from the true state after segment k - 1 and sums y^2.
//   4. loud_gate_kernel: one block per row adds the segment sums to block energies, applies the two gates and writes L and the peak.
// Four launches whatever the lengths.  Every sum has a fixed order that depends on the row's own length only (a thread's samples in
// order, a block's segments in order, strided partial sums and an LDS tree over the blocks), so row b of a batch has the bits it has alone.
// wave_level_kernel: every block works its row's gain out again from L, peak, mode and target (a few float64 operations) and scales
// its share of the row in place.
// true_peak_kernel (ttsamd_true_peak): the peak of the 4x interpolated row from the chains of true_peak.hpp; its result can stand in for
// `peak` in wave_level_kernel, which makes the ceiling a true-peak ceiling.
#include <cmath>

#include "common.hpp"
#include "true_peak.hpp"

namespace ttsamd {

constexpr int LD_T = 128;             // segments (= threads) per block of the two filter passes
constexpr int LD_SMAX = 64;           // longest segment
constexpr int LD_SP = LD_SMAX + 1;    // LDS words per segment
constexpr int LD_GT = 256;            // threads of the gate kernel
constexpr int32_t LD_FS_MIN = 8000, LD_FS_MAX = 192000;

struct LoudCoef {
    double b1[3], a1[2], b2[3], a2[2];
};
struct LoudPlan {
    LoudCoef c;
    double M[16];                     // state after one segment of zero input = M * state before it (row-major)
    int32_t step, S, Q;               // samples per step, per segment, segments per step
};

// one sample through both biquads (transposed direct form II); s = (s1, s2 of stage 1, s1, s2 of stage 2)
__host__ __device__ __forceinline__ double loud_sample(const LoudCoef& c, const double x, double* s) {
    const double y1 = c.b1[0] * x + s[0];
    s[0] = c.b1[1] * x - c.a1[0] * y1 + s[1];
    s[1] = c.b1[2] * x - c.a1[1] * y1;
    const double y2 = c.b2[0] * y1 + s[2];
    s[2] = c.b2[1] * y1 - c.a2[0] * y2 + s[3];
    s[3] = c.b2[2] * y1 - c.a2[1] * y2;
    return y2;
}

static void loud_coefficients(int32_t fs, LoudCoef& c) {
    const double pi = 3.14159265358979323846;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        c.b1[0] = (Vh + Vb * K / Q + K * K) / a0;
        c.b1[1] = 2.0 * (K * K - Vh) / a0;
        c.b1[2] = (Vh - Vb * K / Q + K * K) / a0;
        c.a1[0] = 2.0 * (K * K - 1.0) / a0;
        c.a1[1] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        c.b2[0] = 1.0;
        c.b2[1] = -2.0;
        c.b2[2] = 1.0;
        c.a2[0] = 2.0 * (K * K - 1.0) / a0;
        c.a2[1] = (1.0 - K / Q + K * K) / a0;
    }
}

static void loud_plan(int32_t fs, LoudPlan& p) {
    loud_coefficients(fs, p.c);
    p.step = (fs + 5) / 10;
    p.S = 1;
    for (int d = LD_SMAX; d > 1; --d)
        if (p.step % d == 0) {
            p.S = d;
            break;
        }
    p.Q = p.step / p.S;
    for (int col = 0; col < 4; ++col) {                        // column `col` of M: S samples of zero input from the unit state
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[col] = 1.0;
        for (int j = 0; j < p.S; ++j) loud_sample(p.c, 0.0, s);
        for (int r = 0; r < 4; ++r) p.M[4 * r + col] = s[r];
    }
}

struct LoudWs {
    int64_t K, NB, J;                 // per row of the stride: segments, blocks of the filter passes, gating blocks
    double *st, *seg, *zb;            // [B][K][4] states, [B][K] segment sums of y^2, [B][J] block energies
    float* pk;                        // [B][NB] partial peaks
    int64_t bytes;
};

static void loud_carve(void* base, int64_t B, int64_t stride, const LoudPlan& p, LoudWs& w) {
    w.K = (stride + p.S - 1) / p.S;
    w.K = w.K < 1 ? 1 : w.K;
    w.NB = (w.K + LD_T - 1) / LD_T;
    const int64_t block = 4 * (int64_t)p.step;
    w.J = stride >= block ? (stride - block) / p.step + 1 : 1;
    Arena a(base, (int64_t)1 << 62);
    w.st = a.take<double>(B * w.K * 4);
    w.seg = a.take<double>(B * w.K);
    w.zb = a.take<double>(B * w.J);
    w.pk = a.take<float>(B * w.NB);
    w.bytes = a.off;
}

__device__ __forceinline__ int64_t loud_len(const int64_t* __restrict__ ns, const int b, const int64_t stride) {
    return max((int64_t)0, min(ns[b], stride));
}

// the block's tile (LD_T segments of S samples from sample `base`) into LDS, zeros at and past n; returns the thread's max |x|
__device__ __forceinline__ float loud_load_tile(const float* __restrict__ wb, const int64_t base, const int64_t n, const int S,
                                                float* __restrict__ xs) {
    float m = 0.f;
    for (int idx = threadIdx.x; idx < LD_T * S; idx += LD_T) {
        const int sg = idx / S, j = idx - sg * S;
        const int64_t g = base + idx;
        const float v = g < n ? wb[g] : 0.f;
        m = fmaxf(m, fabsf(v));
        xs[sg * LD_SP + j] = v;
    }
    return m;
}

__global__ __launch_bounds__(LD_T) void loud_zero_state_kernel(const float* __restrict__ wave, int64_t stride, const int64_t* __restrict__ ns,
                                                               LoudPlan p, int64_t K, int64_t NB, double* __restrict__ st,
                                                               float* __restrict__ pk) {
    __shared__ float xs[LD_T * LD_SP];
    __shared__ float red[LD_T / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t n = loud_len(ns, b, stride), base = (int64_t)blockIdx.x * LD_T * p.S;
    if (base >= n) return;                                     // the whole block: nothing of the row is here
    float m = loud_load_tile(wave + (int64_t)b * stride, base, n, p.S, xs);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) pk[(int64_t)b * NB + blockIdx.x] = fmaxf(red[0], red[1]);
    const int64_t k = (int64_t)blockIdx.x * LD_T + tid;
    if (k * p.S >= n) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const float* xr = xs + tid * LD_SP;
    for (int j = 0; j < p.S; ++j) loud_sample(p.c, (double)xr[j], s);   // a last, partial segment runs on into zeros: its state is not used
    double* o = st + ((int64_t)b * K + k) * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = s[i];
}

__global__ __launch_bounds__(64) void loud_scan_kernel(const int64_t* __restrict__ ns, int64_t stride, LoudPlan p, int64_t K,
                                                       double* __restrict__ st) {
    __shared__ double P[6][16];                                // M^(2^d)
    const int b = blockIdx.x, lane = threadIdx.x;
    const int64_t n = loud_len(ns, b, stride), Kr = (n + p.S - 1) / p.S;
    if (Kr < 2) return;                                        // one segment: nothing to carry
    if (lane < 16) P[0][lane] = p.M[lane];
    __syncthreads();
    for (int d = 1; d < 6; ++d) {
        if (lane < 16) {
            const int r = lane >> 2, c = lane & 3;
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) acc += P[d - 1][4 * r + i] * P[d - 1][4 * i + c];
            P[d][lane] = acc;
        }
        __syncthreads();
    }
    double* sb = st + (int64_t)b * K * 4;
    double carry[4] = {0.0, 0.0, 0.0, 0.0};                    // the state in front of this run of 64 segments
    for (int64_t k0 = 0; k0 < Kr; k0 += 64) {
        const int64_t k = k0 + lane;
        double v[4] = {0.0, 0.0, 0.0, 0.0};
        if (k < Kr) {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = sb[k * 4 + i];
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double acc = v[r];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc += P[0][4 * r + i] * carry[i];
                v[r] = acc;
            }
        }
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            double u[4], w[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) u[i] = __shfl_up(v[i], 1u << d, 64);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double acc = v[r];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc += P[d][4 * r + i] * u[i];
                w[r] = acc;
            }
            if (lane >= (1 << d)) {
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = w[i];
            }
        }
        if (k < Kr) {
#pragma unroll
            for (int i = 0; i < 4; ++i) sb[k * 4 + i] = v[i];  // now the state BEHIND segment k
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) carry[i] = __shfl(v[i], 63, 64);
    }
}

__global__ __launch_bounds__(LD_T) void loud_energy_kernel(const float* __restrict__ wave, int64_t stride, const int64_t* __restrict__ ns,
                                                           LoudPlan p, int64_t K, const double* __restrict__ st, double* __restrict__ seg) {
    __shared__ float xs[LD_T * LD_SP];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t n = loud_len(ns, b, stride), base = (int64_t)blockIdx.x * LD_T * p.S;
    if (base >= n) return;
    loud_load_tile(wave + (int64_t)b * stride, base, n, p.S, xs);
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * LD_T + tid;
    if (k * p.S >= n) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (k > 0) {
        const double* i0 = st + ((int64_t)b * K + k - 1) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = i0[i];
    }
    const int m = (int)min((int64_t)p.S, n - k * p.S);         // the last segment of the row may be short
    const float* xr = xs + tid * LD_SP;
    double e = 0.0;
    for (int j = 0; j < m; ++j) {
        const double y = loud_sample(p.c, (double)xr[j], s);
        e += y * y;
    }
    seg[(int64_t)b * K + k] = e;
}

// sum and count over the block in a fixed order: the threads' own values through an LDS tree
__device__ __forceinline__ void loud_block_sum(double& v, int& c, double* rs, int* rc) {
    const int tid = threadIdx.x;
    __syncthreads();
    rs[tid] = v;
    rc[tid] = c;
    __syncthreads();
    for (int d = LD_GT / 2; d >= 1; d >>= 1) {
        if (tid < d) {
            rs[tid] += rs[tid + d];
            rc[tid] += rc[tid + d];
        }
        __syncthreads();
    }
    v = rs[0];
    c = rc[0];
}

__global__ __launch_bounds__(LD_GT) void loud_gate_kernel(const int64_t* __restrict__ ns, int64_t stride, int step, int S, int Q, int64_t K,
                                                          int64_t NB, int64_t J, const double* __restrict__ seg, const float* __restrict__ pk,
                                                          double* __restrict__ zb, double* __restrict__ loudness, float* __restrict__ peak) {
    __shared__ double rs[LD_GT];
    __shared__ int rc[LD_GT];
    __shared__ float rm[LD_GT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t n = loud_len(ns, b, stride), Kr = (n + S - 1) / S, block = 4 * (int64_t)step;
    const double* sg = seg + (int64_t)b * K;
    double* z = zb + (int64_t)b * J;
    float m = 0.f;
    for (int64_t i = tid; i < (Kr + LD_T - 1) / LD_T; i += LD_GT) m = fmaxf(m, pk[(int64_t)b * NB + i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if ((tid & 63) == 0) rm[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) peak[b] = fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3]));
    if (n == 0) {
        if (tid == 0) loudness[b] = -INFINITY;
        return;
    }
    int64_t Jr = 1;
    if (n < block) {                                           // a short row: one block, the mean over its n samples
        double e = 0.0;
        int c = 0;
        for (int64_t k = tid; k < Kr; k += LD_GT) e += sg[k];
        loud_block_sum(e, c, rs, rc);
        if (tid == 0) z[0] = e / (double)n;
    } else {
        Jr = (n - block) / step + 1;
        for (int64_t j = tid; j < Jr; j += LD_GT) {
            double e = 0.0;
            for (int q = 0; q < 4; ++q) {                      // four steps, each the sum of its Q segments in order
                double t = 0.0;
                const double* s0 = sg + (j + q) * Q;
                for (int i = 0; i < Q; ++i) t += s0[i];
                e += t;
            }
            z[j] = e / (double)block;
        }
    }
    __syncthreads();                                           // z[0] of a short row is read by every thread (a block's own writes)
    double sa = 0.0;
    int ca = 0;
    for (int64_t j = tid; j < Jr; j += LD_GT) {
        const double zj = z[j];
        if (-0.691 + 10.0 * log10(zj) > -70.0) {
            sa += zj;
            ++ca;
        }
    }
    loud_block_sum(sa, ca, rs, rc);
    if (ca == 0) {
        if (tid == 0) loudness[b] = -INFINITY;
        return;
    }
    const double gamma = -0.691 + 10.0 * log10(sa / (double)ca) - 10.0;
    double sr = 0.0;
    int cr = 0;
    for (int64_t j = tid; j < Jr; j += LD_GT) {
        const double zj = z[j], l = -0.691 + 10.0 * log10(zj);
        if (l > -70.0 && l > gamma) {
            sr += zj;
            ++cr;
        }
    }
    loud_block_sum(sr, cr, rs, rc);
    if (tid == 0) loudness[b] = cr > 0 ? -0.691 + 10.0 * log10(sr / (double)cr) : -INFINITY;
}

static int32_t loud_check_rate(int32_t fs, const char* what) {
    TTS_REQUIRE(fs >= LD_FS_MIN && fs <= LD_FS_MAX, "%s: sample rate %d outside [%d, %d]", what, fs, LD_FS_MIN, LD_FS_MAX);
    return 0;
}

static int32_t loudness_measure(const float* wave, int64_t stride, const int64_t* nsamples, int32_t B, int32_t fs, double* loudness,
                                float* peak, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    TTS_REQUIRE(nsamples && loudness && peak && workspace && (wave || stride == 0), "loudness_measure: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && stride >= 0 && stride < ((int64_t)1 << 40), "loudness_measure: bad batch %d / stride", B);
    TTS_TRY(loud_check_rate(fs, "loudness_measure"));
    LoudPlan p;
    loud_plan(fs, p);
    LoudWs w;
    loud_carve(nullptr, B, stride, p, w);
    TTS_REQUIRE(workspace_bytes >= w.bytes, "loudness_measure: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)w.bytes);
    TTS_REQUIRE(w.NB <= 0x7fffffff, "loudness_measure: stride too large");
    loud_carve(workspace, B, stride, p, w);
    const dim3 grid((unsigned)w.NB, B);
    hipLaunchKernelGGL(loud_zero_state_kernel, grid, dim3(LD_T), 0, s, wave, stride, nsamples, p, w.K, w.NB, w.st, w.pk);
    TTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loud_scan_kernel, dim3(B), dim3(64), 0, s, nsamples, stride, p, w.K, w.st);
    TTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loud_energy_kernel, grid, dim3(LD_T), 0, s, wave, stride, nsamples, p, w.K, w.st, w.seg);
    TTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loud_gate_kernel, dim3(B), dim3(LD_GT), 0, s, nsamples, stride, p.step, p.S, p.Q, w.K, w.NB, w.J, w.seg, w.pk, w.zb,
                       loudness, peak);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// True peak (include/ttsamd.h): a block owns a tile of TPK_T samples of one row, stages the tile and 12 samples to either side in LDS,
// and every thread runs the three float64 chains of its eight samples.  max |x|, |v| over the block in float64, rounded UPWARD to fp32;
// non-negative IEEE floats order as their bit patterns, so one unsigned atomic max per block on the (zeroed) result is exact and
// order-free.  The 4x signal lives in registers only.
constexpr int TPK_T = 2048, TPK_NT = 256;
constexpr int TPK_XN = TPK_T + 2 * TP_W;
static_assert(TPK_T == 8 * TPK_NT && TPK_XN % 4 == 0 && TP_W % 4 == 0, "true-peak tiling");

__global__ __launch_bounds__(TPK_NT) void true_peak_kernel(const float* __restrict__ wave, int64_t stride, const int64_t* __restrict__ ns,
                                                           const TpTaps taps, float* __restrict__ out) {
    __shared__ __align__(16) float xs[TPK_XN];
    __shared__ float red[TPK_NT / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t n = loud_len(ns, b, stride), t0 = (int64_t)blockIdx.x * TPK_T;
    if (t0 >= n) return;                                       // the whole block: an empty row keeps its zero
    tp_stage<false>(wave + (int64_t)b * stride, t0 - TP_W, TPK_XN, n, 1.f, xs);
    __syncthreads();
    const int64_t i0 = t0 + 8 * tid;
    double m = 0.0;
    if (i0 < n) {
        double vm[8];
        tp_chains<8>(xs + 8 * tid, taps, vm);
#pragma unroll
        for (int e = 0; e < 8; ++e)
            if (i0 + e < n) m = fmax(m, fmax(fabs((double)xs[8 * tid + TP_W + e]), vm[e]));
    }
    float f = (float)m;
    if ((double)f < m) f = nextafterf(f, INFINITY);            // the smallest fp32 >= m
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) f = fmaxf(f, __shfl_xor(f, d, 64));
    if ((tid & 63) == 0) red[tid >> 6] = f;
    __syncthreads();
    if (tid == 0) {
        f = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (f > 0.f) atomicMax((unsigned int*)out + b, __float_as_uint(f));
    }
}

static int32_t true_peak(const float* wave, int64_t stride, const int64_t* nsamples, int32_t B, float* out, hipStream_t s) {
    TTS_REQUIRE(nsamples && out && (wave || stride == 0), "true_peak: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && stride >= 0 && stride < ((int64_t)1 << 40), "true_peak: bad batch %d / stride", B);
    int64_t nt = (stride + TPK_T - 1) / TPK_T;
    nt = nt < 1 ? 1 : nt;
    TTS_REQUIRE(nt <= 0x7fffffff, "true_peak: stride too large");
    TTS_CHECK_HIP(hipMemsetAsync(out, 0, (size_t)B * sizeof(float), s));
    hipLaunchKernelGGL(true_peak_kernel, dim3((unsigned)nt, B), dim3(TPK_NT), 0, s, wave, stride, nsamples, tp_taps(), out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void wave_level_kernel(float* __restrict__ wave, int64_t stride, const int64_t* __restrict__ ns,
                                                         const int32_t* __restrict__ mode, const float* __restrict__ target, float ceiling,
                                                         const double* __restrict__ loudness, const float* __restrict__ peak,
                                                         float* __restrict__ gain_out) {
    const int b = blockIdx.y;
    const int64_t n = loud_len(ns, b, stride);
    const int md = mode[b];
    const float pk = peak[b], tg = target[b];
    float g = 1.f;
    bool live = false;
    if (md == 1 && pk > 0.f) {
        g = __fdiv_rn(tg, pk);
        live = true;
    } else if (md == 2 && pk > 0.f) {
        const double L = loudness[b];
        if (isfinite(L)) {
            double g64 = pow(10.0, ((double)tg - L) / 20.0);
            if ((double)pk * g64 > (double)ceiling) g64 = (double)ceiling / (double)pk;
            g = (float)g64;
            if (__fmul_rn(pk, g) > ceiling) g = nextafterf(g, 0.f);   // the rounding of g or of the product may lift the peak one ulp above
            live = true;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) gain_out[b] = g;
    if (!live) return;                                         // the row keeps its samples bit for bit
    float* wb = wave + (int64_t)b * stride;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = wb[i];
        wb[i] = md == 1 ? __fmul_rn(__fdiv_rn(v, pk), tg) : __fmul_rn(v, g);
    }
}

static int32_t wave_level(float* wave, int64_t stride, const int64_t* nsamples, int32_t B, const int32_t* mode, const float* target,
                          float ceiling, const double* loudness, const float* peak, float* gain_out, hipStream_t s) {
    TTS_REQUIRE(nsamples && mode && target && loudness && peak && gain_out && (wave || stride == 0), "wave_level: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && stride >= 0, "wave_level: bad batch %d / stride", B);
    TTS_REQUIRE(ceiling > 0.f && ceiling <= 1.f, "wave_level: ceiling %g is not in (0, 1]", (double)ceiling);
    int64_t nb = (stride + 2047) / 2048;                       // eight samples per thread of a full row
    nb = nb < 1 ? 1 : (nb > 4096 ? 4096 : nb);
    hipLaunchKernelGGL(wave_level_kernel, dim3((unsigned)nb, B), dim3(256), 0, s, wave, stride, nsamples, mode, target, ceiling, loudness,
                       peak, gain_out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd

using namespace ttsamd;

extern "C" {

int32_t ttsamd_loudness_coefficients(int32_t sample_rate, double* out) {
    TTS_REQUIRE(out, "loudness_coefficients: out is null");
    TTS_TRY(loud_check_rate(sample_rate, "loudness_coefficients"));
    LoudCoef c;
    loud_coefficients(sample_rate, c);
    const double v[10] = {c.b1[0], c.b1[1], c.b1[2], c.a1[0], c.a1[1], c.b2[0], c.b2[1], c.b2[2], c.a2[0], c.a2[1]};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return 0;
}

int64_t ttsamd_loudness_workspace_bytes(int32_t batch, int64_t wave_stride, int32_t sample_rate) {
    if (batch < 1 || wave_stride < 0 || wave_stride >= ((int64_t)1 << 40) || sample_rate < LD_FS_MIN || sample_rate > LD_FS_MAX) return -1;
    LoudPlan p;
    loud_plan(sample_rate, p);
    LoudWs w;
    loud_carve(nullptr, batch, wave_stride, p, w);
    return w.bytes;
}

int32_t ttsamd_loudness_measure(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t sample_rate,
                                double* loudness, float* peak, void* workspace, int64_t workspace_bytes, void* stream) {
    return loudness_measure(wave, wave_stride, nsamples, batch, sample_rate, loudness, peak, workspace, workspace_bytes, (hipStream_t)stream);
}

int32_t ttsamd_wave_level(float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, const int32_t* mode,
                          const float* target, float ceiling, const double* loudness, const float* peak, float* gain_out, void* stream) {
    return wave_level(wave, wave_stride, nsamples, batch, mode, target, ceiling, loudness, peak, gain_out, (hipStream_t)stream);
}

int32_t ttsamd_true_peak_taps(double* out) {
    TTS_REQUIRE(out, "true_peak_taps: out is null");
    const TpTaps& t = tp_taps();
    for (int p = 0; p < TP_P; ++p)
        for (int j = 0; j < TP_J; ++j) out[p * TP_J + j] = t.h[p][j];
    return 0;
}

int32_t ttsamd_true_peak(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, float* true_peak_out, void* stream) {
    return true_peak(wave, wave_stride, nsamples, batch, true_peak_out, (hipStream_t)stream);
}

}  // extern "C"
