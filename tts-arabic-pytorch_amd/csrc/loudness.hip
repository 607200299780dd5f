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
// The meter (ttsamd_loudness_meter): launches 1 - 3, then loud_meter_kernel, one block per row: step energies, momentary and short-term
// series with their maxima, the integrated loudness by the gates loud_gate_kernel uses (the same bits), the loudness range by rank
// counting.  The stream meter (ttsamd_meter_*) keeps a slot per stream (MeterHead and its planes); a push runs launches 1 - 3 as their
// <true> instantiations over "the slot's unfinished segment, then the chunk" from the slot's filter state, then meter_push_kernel.
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

// Stream meter (ttsamd_meter_*): what a slot carries from push to push.  The three filter kernels below run a push as the row
// "pending samples, then the chunk" from the carried filter state (their <true> instantiations); <false> is the whole-wave path.
struct MeterHead {
    double fst[4];                    // the filter state behind the last whole segment
    double upart;                     // the finished segments of the unfinished step, added in order
    int64_t n;                        // samples so far: n / S whole segments, (n / S) / Q whole steps in u
    float peak;
    int32_t status;                   // bit 0: a push beyond max_samples was dropped
    float pend[LD_SMAX];              // the n % S samples of the unfinished segment
};
struct MeterStream {
    char* state;                      // [nslots][slot_bytes]: a MeterHead, then u, z / s scratch and key scratch, [ucap] doubles each
    const int32_t* slots;             // device [rows]
    int64_t slot_bytes, max_samples, ucap;
    int32_t nslots;
};
constexpr int64_t METER_HEAD_BYTES = 512;
static_assert(sizeof(MeterHead) <= METER_HEAD_BYTES, "meter head");

__device__ __forceinline__ MeterHead* meter_head(const MeterStream& ms, const int b) {
    const int32_t sl = ms.slots[b];
    return sl >= 0 && sl < ms.nslots ? (MeterHead*)(ms.state + (int64_t)sl * ms.slot_bytes) : nullptr;
}
__device__ __forceinline__ double* meter_plane(MeterHead* h, const MeterStream& ms, const int i) {
    return (double*)((char*)h + METER_HEAD_BYTES) + (int64_t)i * ms.ucap;
}
// the row a push filters: r pending samples and c new ones; a bad slot or a push beyond max_samples takes nothing in (c = 0)
__device__ __forceinline__ MeterHead* meter_row(const MeterStream& ms, const int64_t* __restrict__ ns, const int b, const int64_t stride,
                                                const int S, int& r, int64_t& c) {
    MeterHead* h = meter_head(ms, b);
    r = 0;
    c = 0;
    if (!h) return h;
    c = loud_len(ns, b, stride);
    if (h->n + c > ms.max_samples) c = 0;
    r = (int)(h->n % S);
    return h;
}

// the block's tile (LD_T segments of S samples from sample `base`) into LDS, zeros at and past n; returns the thread's max |x|
// (a push: the first r samples of the row are the slot's pending ones)
template <bool ST>
__device__ __forceinline__ float loud_load_tile(const float* __restrict__ wb, const int64_t base, const int64_t n, const int S,
                                                float* __restrict__ xs, const float* pend = nullptr, const int r = 0) {
    float m = 0.f;
    for (int idx = threadIdx.x; idx < LD_T * S; idx += LD_T) {
        const int sg = idx / S, j = idx - sg * S;
        const int64_t g = base + idx;
        float v;
        if constexpr (ST)
            v = g < n ? (g < r ? pend[g] : wb[g - r]) : 0.f;
        else
            v = g < n ? wb[g] : 0.f;
        m = fmaxf(m, fabsf(v));
        xs[sg * LD_SP + j] = v;
    }
    return m;
}

template <bool ST>
__global__ __launch_bounds__(LD_T) void loud_zero_state_kernel(const float* __restrict__ wave, int64_t stride, const int64_t* __restrict__ ns,
                                                               LoudPlan p, int64_t K, int64_t NB, double* __restrict__ st,
                                                               float* __restrict__ pk, MeterStream ms) {
    __shared__ float xs[LD_T * LD_SP];
    __shared__ float red[LD_T / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t n;
    int r = 0;
    const float* pend = nullptr;
    if constexpr (ST) {
        int64_t c;
        const MeterHead* h = meter_row(ms, ns, b, stride, p.S, r, c);
        n = r + c;
        if (h) pend = h->pend;
    } else {
        n = loud_len(ns, b, stride);
    }
    const int64_t base = (int64_t)blockIdx.x * LD_T * p.S;
    if (base >= n) return;                                     // the whole block: nothing of the row is here
    float m = loud_load_tile<ST>(wave + (int64_t)b * stride, base, n, p.S, xs, pend, r);
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

template <bool ST>
__global__ __launch_bounds__(64) void loud_scan_kernel(const int64_t* __restrict__ ns, int64_t stride, LoudPlan p, int64_t K,
                                                       double* __restrict__ st, MeterStream ms) {
    __shared__ double P[6][16];                                // M^(2^d)
    const int b = blockIdx.x, lane = threadIdx.x;
    int64_t n;
    double carry[4] = {0.0, 0.0, 0.0, 0.0};                    // the state in front of this run of 64 segments
    if constexpr (ST) {
        int r;
        int64_t c;
        const MeterHead* h = meter_row(ms, ns, b, stride, p.S, r, c);
        n = r + c;
        if (h) {
#pragma unroll
            for (int i = 0; i < 4; ++i) carry[i] = h->fst[i];
        }
    } else {
        n = loud_len(ns, b, stride);
    }
    const int64_t Kr = (n + p.S - 1) / p.S;
    if (Kr < (ST ? 1 : 2)) return;                             // one segment from a zero state: nothing to carry
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

template <bool ST>
__global__ __launch_bounds__(LD_T) void loud_energy_kernel(const float* __restrict__ wave, int64_t stride, const int64_t* __restrict__ ns,
                                                           LoudPlan p, int64_t K, const double* __restrict__ st, double* __restrict__ seg,
                                                           MeterStream ms) {
    __shared__ float xs[LD_T * LD_SP];
    const int b = blockIdx.y, tid = threadIdx.x;
    int64_t n;
    int r = 0;
    const MeterHead* h = nullptr;
    if constexpr (ST) {
        int64_t c;
        h = meter_row(ms, ns, b, stride, p.S, r, c);
        n = r + c;
    } else {
        n = loud_len(ns, b, stride);
    }
    const int64_t base = (int64_t)blockIdx.x * LD_T * p.S;
    if (base >= n) return;
    loud_load_tile<ST>(wave + (int64_t)b * stride, base, n, p.S, xs, h ? h->pend : nullptr, r);
    __syncthreads();
    const int64_t k = (int64_t)blockIdx.x * LD_T + tid;
    if (k * p.S >= n) return;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (k > 0) {
        const double* i0 = st + ((int64_t)b * K + k - 1) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = i0[i];
    } else if constexpr (ST) {
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = h->fst[i];          // n > 0 here, so the slot is a good one
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

// both gates over the block energies z[0 .. Jr) (written by this block, a barrier behind them): the integrated loudness, in every thread
__device__ __forceinline__ double loud_gates(const double* z, const int64_t Jr, double* rs, int* rc) {
    const int tid = threadIdx.x;
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
    if (ca == 0) return -INFINITY;
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
    return cr > 0 ? -0.691 + 10.0 * log10(sr / (double)cr) : -INFINITY;
}

// the largest of the threads' values, in every thread
__device__ __forceinline__ double loud_block_max(const double v, double* rs) {
    const int tid = threadIdx.x;
    __syncthreads();
    rs[tid] = v;
    __syncthreads();
    for (int d = LD_GT / 2; d >= 1; d >>= 1) {
        if (tid < d) rs[tid] = fmax(rs[tid], rs[tid + d]);
        __syncthreads();
    }
    return rs[0];
}

// the block's partial peaks of a row of Kr segments -> max |x|, in thread 0
__device__ __forceinline__ float loud_row_peak(const float* __restrict__ pkb, const int64_t Kr, float* rm) {
    const int tid = threadIdx.x;
    float m = 0.f;
    for (int64_t i = tid; i < (Kr + LD_T - 1) / LD_T; i += LD_GT) m = fmaxf(m, pkb[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = fmaxf(m, __shfl_xor(m, d, 64));
    if ((tid & 63) == 0) rm[tid >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(rm[0], rm[1]), fmaxf(rm[2], rm[3]));
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
    const float m = loud_row_peak(pk + (int64_t)b * NB, Kr, rm);
    if (tid == 0) peak[b] = m;
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
    const double L = loud_gates(z, Jr, rs, rc);
    if (tid == 0) loudness[b] = L;
}

// ---- the meter (include/ttsamd.h, "loudness meter"): what comes after the step energies ----
constexpr int MT_TILE = 1024;                                  // keys per LDS tile of the rank count
struct MeterLds {
    double rs[LD_GT], tile[MT_TILE], lohi[2];
    int rc[LD_GT];
    float rm[LD_GT / 64];
};
struct MeterOut {
    double L, lra, maxm, maxs;
    int64_t J, JS;
};

// One block, from the step energies u[0 .. U) of a row of n samples: momentary blocks z (z[0] of a short row is there already), both
// gates, the short-term series, its two gates and the two percentiles by rank counting.  z is scratch of max(J, JS) doubles (the
// short-term energies take the blocks' place once those are used up), key of JS.  Mrow / Srow may be null.  The results are in every thread.
__device__ __forceinline__ MeterOut meter_windows(const double* u, const int64_t U, const int64_t n, const int step, double* z, double* key,
                                                  double* Mrow, double* Srow, MeterLds& l) {
    const int tid = threadIdx.x;
    const int64_t block = 4 * (int64_t)step;
    MeterOut o;
    o.J = n == 0 ? 0 : (n < block ? 1 : U - 3);
    o.JS = U >= 30 ? U - 29 : 0;
    if (n >= block)
        for (int64_t j = tid; j < o.J; j += LD_GT) z[j] = (((u[j] + u[j + 1]) + u[j + 2]) + u[j + 3]) / (double)block;
    __syncthreads();
    o.L = loud_gates(z, o.J, l.rs, l.rc);
    double mx = -INFINITY;
    for (int64_t j = tid; j < o.J; j += LD_GT) {
        const double m = -0.691 + 10.0 * log10(z[j]);
        if (Mrow) Mrow[j] = m;
        mx = fmax(mx, m);
    }
    o.maxm = loud_block_max(mx, l.rs);                         // (its barriers: z is free from here)
    double* se = z;
    double sa = 0.0;
    int ca = 0;
    mx = -INFINITY;
    for (int64_t j = tid; j < o.JS; j += LD_GT) {
        double e = 0.0;
        for (int q = 0; q < 30; ++q) e += u[j + q];
        e /= 30.0 * (double)step;
        const double s = -0.691 + 10.0 * log10(e);
        se[j] = e;
        key[j] = s;
        if (Srow) Srow[j] = s;
        mx = fmax(mx, s);
        if (s > -70.0) {
            sa += e;
            ++ca;
        }
    }
    o.maxs = loud_block_max(mx, l.rs);
    loud_block_sum(sa, ca, l.rs, l.rc);
    o.lra = 0.0;
    if (ca == 0) return o;
    const double gamma = -0.691 + 10.0 * log10(sa / (double)ca) - 20.0;
    double unused = 0.0;
    int k = 0;
    for (int64_t j = tid; j < o.JS; j += LD_GT) {              // a thread's own entries: the key is the value, +inf for a gated one
        const double s = key[j];
        const bool keep = s > -70.0 && s > gamma;
        key[j] = keep ? s : INFINITY;
        k += keep;
    }
    loud_block_sum(unused, k, l.rs, l.rc);
    if (k == 0) return o;
    const int64_t ilo = ((int64_t)(k - 1) * 10 + 50) / 100, ihi = ((int64_t)(k - 1) * 95 + 50) / 100;
    for (int64_t j0 = 0; j0 < o.JS; j0 += LD_GT) {             // rank of key[j] = the keys below it, ties by index: unique ranks 0 .. k - 1
        const int64_t j = j0 + tid;
        const double kj = j < o.JS ? key[j] : INFINITY;
        int64_t rank = 0;
        for (int64_t t0 = 0; t0 < o.JS; t0 += MT_TILE) {
            const int cnt = (int)min((int64_t)MT_TILE, o.JS - t0);
            __syncthreads();
            for (int i = tid; i < cnt; i += LD_GT) l.tile[i] = key[t0 + i];
            __syncthreads();
            for (int i = 0; i < cnt; ++i) {
                const double ki = l.tile[i];
                rank += (ki < kj || (ki == kj && t0 + i < j)) ? 1 : 0;
            }
        }
        if (kj < INFINITY) {
            if (rank == ilo) l.lohi[0] = kj;
            if (rank == ihi) l.lohi[1] = kj;
        }
    }
    __syncthreads();
    o.lra = l.lohi[1] - l.lohi[0];
    return o;
}

__device__ __forceinline__ void meter_write(const MeterOut& o, const int b, double* loudness, double* range, double* maxm, double* maxs,
                                            int64_t* counts) {
    loudness[b] = o.L;
    range[b] = o.lra;
    maxm[b] = o.maxm;
    maxs[b] = o.maxs;
    counts[2 * b] = o.J;
    counts[2 * b + 1] = o.JS;
}

__global__ __launch_bounds__(LD_GT) void loud_meter_kernel(const int64_t* __restrict__ ns, int64_t stride, int step, int S, int Q, int64_t K,
                                                           int64_t NB, int64_t J, int64_t UM, const double* __restrict__ seg,
                                                           const float* __restrict__ pk, double* __restrict__ zb, double* __restrict__ ub,
                                                           double* __restrict__ kb, double* __restrict__ loudness, float* __restrict__ peak,
                                                           double* __restrict__ range, double* __restrict__ maxm, double* __restrict__ maxs,
                                                           int64_t* __restrict__ counts, double* __restrict__ Mout, int64_t mstride,
                                                           double* __restrict__ Sout, int64_t sstride) {
    __shared__ MeterLds l;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t n = loud_len(ns, b, stride), Kr = (n + S - 1) / S, U = n / step;
    const double* sg = seg + (int64_t)b * K;
    double *z = zb + (int64_t)b * J, *u = ub + (int64_t)b * UM;
    const float m = loud_row_peak(pk + (int64_t)b * NB, Kr, l.rm);
    if (tid == 0) peak[b] = m;
    for (int64_t i = tid; i < U; i += LD_GT) {                 // a step: its Q segments in order
        double t = 0.0;
        const double* s0 = sg + i * Q;
        for (int q = 0; q < Q; ++q) t += s0[q];
        u[i] = t;
    }
    if (n > 0 && n < 4 * (int64_t)step) {                      // a short row, as loud_gate_kernel takes it
        double e = 0.0;
        int c = 0;
        for (int64_t k = tid; k < Kr; k += LD_GT) e += sg[k];
        loud_block_sum(e, c, l.rs, l.rc);
        if (tid == 0) z[0] = e / (double)n;
    }
    __syncthreads();
    const MeterOut o = meter_windows(u, U, n, step, z, kb + (int64_t)b * max(UM - 29, (int64_t)0), Mout ? Mout + (int64_t)b * mstride : nullptr,
                                     Sout ? Sout + (int64_t)b * sstride : nullptr, l);
    if (tid == 0) meter_write(o, b, loudness, range, maxm, maxs, counts);
}

__global__ void meter_reset_kernel(MeterStream ms, int rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= rows) return;
    MeterHead* h = meter_head(ms, b);
    if (!h) return;
#pragma unroll
    for (int i = 0; i < 4; ++i) h->fst[i] = 0.0;
    h->upart = 0.0;
    h->n = 0;
    h->peak = 0.f;
    h->status = 0;
}

// The last launch of a push: one block per row takes the whole segments of "pending, then the chunk" into the slot (steps that end in
// them, the partial step, the filter state behind them, the samples behind them, the peak) and reads the meter.
__global__ __launch_bounds__(LD_GT) void meter_push_kernel(const float* __restrict__ chunks, int64_t stride, const int64_t* __restrict__ ns,
                                                           MeterStream ms, int step, int S, int Q, int64_t K, int64_t NB,
                                                           const double* __restrict__ st, const double* __restrict__ seg,
                                                           const float* __restrict__ pk, double* __restrict__ momentary,
                                                           double* __restrict__ short_term, double* __restrict__ integrated) {
    __shared__ MeterLds l;
    const int b = blockIdx.x, tid = threadIdx.x;
    int r;
    int64_t c;
    MeterHead* h = meter_row(ms, ns, b, stride, S, r, c);
    if (!h) {                                                  // a slot that does not exist: the row is left out
        if (tid == 0) momentary[b] = short_term[b] = integrated[b] = -INFINITY;
        return;
    }
    const int64_t n0 = h->n, nv = r + c, Kw = nv / S, Kr = (nv + S - 1) / S, nseg0 = n0 / S, U0 = nseg0 / Q;
    const int q0 = (int)(nseg0 % Q);
    const bool dropped = n0 + loud_len(ns, b, stride) > ms.max_samples;
    const double up0 = h->upart;
    const int64_t nU = (q0 + Kw) / Q, U1 = U0 + nU;
    const float m = loud_row_peak(pk + (int64_t)b * NB, Kr, l.rm);      // (its barrier: every thread has read the head)
    const double* sg = seg + (int64_t)b * K;
    double *u = meter_plane(h, ms, 0), *z = meter_plane(h, ms, 1);
    for (int64_t i = tid; i < nU; i += LD_GT) {                // the steps that end in this push, each its Q segments in order
        double t = i == 0 ? up0 : 0.0;
        const int64_t k0 = i == 0 ? 0 : i * Q - q0, k1 = (i + 1) * Q - q0;
        for (int64_t k = k0; k < k1; ++k) t += sg[k];
        u[U0 + i] = t;
    }
    const float* cb = chunks + (int64_t)b * stride;
    for (int64_t g = Kw * S + tid; g < nv; g += LD_GT) {       // the samples behind the last whole segment (fewer than S)
        const float v = g < r ? h->pend[g] : cb[g - r];        // g < r only with Kw = 0: the entry it is written to
        h->pend[g - Kw * S] = v;
    }
    if (tid == 0) {
        double t = nU == 0 ? up0 : 0.0;
        for (int64_t k = nU == 0 ? 0 : nU * Q - q0; k < Kw; ++k) t += sg[k];
        h->upart = t;
        if (Kw > 0) {
            const double* s1 = st + ((int64_t)b * K + Kw - 1) * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) h->fst[i] = s1[i];
        }
        h->n = n0 + c;
        h->peak = fmaxf(h->peak, m);
        if (dropped) h->status |= 1;
    }
    __syncthreads();
    const int64_t Jr = U1 >= 4 ? U1 - 3 : 0;
    for (int64_t j = tid; j < Jr; j += LD_GT) z[j] = (((u[j] + u[j + 1]) + u[j + 2]) + u[j + 3]) / (double)(4 * (int64_t)step);
    __syncthreads();
    const double L = loud_gates(z, Jr, l.rs, l.rc);
    if (tid == 0) {
        integrated[b] = L;
        momentary[b] = Jr > 0 ? -0.691 + 10.0 * log10(z[Jr - 1]) : -INFINITY;
        double e = 0.0;
        if (U1 >= 30)
            for (int q = 0; q < 30; ++q) e += u[U1 - 30 + q];
        short_term[b] = U1 >= 30 ? -0.691 + 10.0 * log10(e / (30.0 * (double)step)) : -INFINITY;
    }
}

__global__ __launch_bounds__(LD_GT) void meter_result_kernel(MeterStream ms, LoudPlan p, double* __restrict__ loudness,
                                                             double* __restrict__ range, double* __restrict__ maxm, double* __restrict__ maxs,
                                                             float* __restrict__ peak, int64_t* __restrict__ counts,
                                                             int32_t* __restrict__ status) {
    __shared__ MeterLds l;
    const int b = blockIdx.x, tid = threadIdx.x;
    MeterHead* h = meter_head(ms, b);
    if (!h) {
        if (tid == 0) {
            MeterOut o = {-INFINITY, 0.0, -INFINITY, -INFINITY, 0, 0};
            meter_write(o, b, loudness, range, maxm, maxs, counts);
            peak[b] = 0.f;
            status[b] = 2;                                     // no such slot
        }
        return;
    }
    const int64_t n = h->n, U = (n / p.S) / p.Q;
    double *u = meter_plane(h, ms, 0), *z = meter_plane(h, ms, 1);
    if (tid == 0 && n > 0 && n < 4 * (int64_t)p.step) {        // a short stream: one block over its n samples, the unfinished segment included
        double e = 0.0, s[4];
        for (int64_t i = 0; i < U; ++i) e += u[i];
        e += h->upart;
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] = h->fst[i];
        for (int j = 0; j < (int)(n % p.S); ++j) {
            const double y = loud_sample(p.c, (double)h->pend[j], s);
            e += y * y;
        }
        z[0] = e / (double)n;
    }
    __syncthreads();
    const MeterOut o = meter_windows(u, U, n, p.step, z, meter_plane(h, ms, 2), nullptr, nullptr, l);
    if (tid == 0) {
        meter_write(o, b, loudness, range, maxm, maxs, counts);
        peak[b] = h->peak;
        status[b] = h->status;
    }
}

static int32_t loud_check_rate(int32_t fs, const char* what) {
    TTS_REQUIRE(fs >= LD_FS_MIN && fs <= LD_FS_MAX, "%s: sample rate %d outside [%d, %d]", what, fs, LD_FS_MIN, LD_FS_MAX);
    return 0;
}

// the three filter launches: the K-weighted energy of every segment to w.seg, the states behind the segments to w.st, peaks to w.pk
template <bool ST>
static int32_t loud_filter(const float* wave, int64_t stride, const int64_t* nsamples, int32_t B, const LoudPlan& p, const LoudWs& w,
                           const MeterStream& ms, hipStream_t s) {
    const dim3 grid((unsigned)w.NB, B);
    hipLaunchKernelGGL(loud_zero_state_kernel<ST>, grid, dim3(LD_T), 0, s, wave, stride, nsamples, p, w.K, w.NB, w.st, w.pk, ms);
    TTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loud_scan_kernel<ST>, dim3(B), dim3(64), 0, s, nsamples, stride, p, w.K, w.st, ms);
    TTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loud_energy_kernel<ST>, grid, dim3(LD_T), 0, s, wave, stride, nsamples, p, w.K, w.st, w.seg, ms);
    TTS_CHECK_HIP(hipGetLastError());
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
    TTS_TRY(loud_filter<false>(wave, stride, nsamples, B, p, w, MeterStream{}, s));
    hipLaunchKernelGGL(loud_gate_kernel, dim3(B), dim3(LD_GT), 0, s, nsamples, stride, p.step, p.S, p.Q, w.K, w.NB, w.J, w.seg, w.pk, w.zb,
                       loudness, peak);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

struct MeterWs {
    LoudWs w;
    int64_t UM, JSM;                  // per row of the stride: whole steps, short-term values
    double *ub, *kb;                  // [B][UM] step energies, [B][JSM] keys of the rank count
    int64_t bytes;
};

static void meter_carve(void* base, int64_t B, int64_t stride, const LoudPlan& p, MeterWs& m) {
    loud_carve(base, B, stride, p, m.w);
    m.UM = stride / p.step;
    m.JSM = m.UM >= 30 ? m.UM - 29 : 0;
    Arena a(base ? (char*)base + m.w.bytes : nullptr, (int64_t)1 << 62);
    m.ub = a.take<double>(B * m.UM);
    m.kb = a.take<double>(B * m.JSM);
    m.bytes = m.w.bytes + a.off;
}

static int32_t loudness_meter(const float* wave, int64_t stride, const int64_t* nsamples, int32_t B, int32_t fs, double* loudness, float* peak,
                              double* range, double* maxm, double* maxs, int64_t* counts, double* Mout, int64_t mstride, double* Sout,
                              int64_t sstride, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    TTS_REQUIRE(nsamples && loudness && peak && range && maxm && maxs && counts && workspace && (wave || stride == 0),
                "loudness_meter: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && stride >= 0 && stride < ((int64_t)1 << 40), "loudness_meter: bad batch %d / stride", B);
    TTS_TRY(loud_check_rate(fs, "loudness_meter"));
    LoudPlan p;
    loud_plan(fs, p);
    MeterWs m;
    meter_carve(nullptr, B, stride, p, m);
    TTS_REQUIRE(workspace_bytes >= m.bytes, "loudness_meter: workspace of %lld bytes, %lld needed", (long long)workspace_bytes,
                (long long)m.bytes);
    TTS_REQUIRE(m.w.NB <= 0x7fffffff, "loudness_meter: stride too large");
    TTS_REQUIRE((!Mout || mstride >= m.w.J) && (!Sout || sstride >= m.JSM), "loudness_meter: series strides %lld / %lld, %lld / %lld needed",
                (long long)mstride, (long long)sstride, (long long)m.w.J, (long long)m.JSM);
    meter_carve(workspace, B, stride, p, m);
    TTS_TRY(loud_filter<false>(wave, stride, nsamples, B, p, m.w, MeterStream{}, s));
    hipLaunchKernelGGL(loud_meter_kernel, dim3(B), dim3(LD_GT), 0, s, nsamples, stride, p.step, p.S, p.Q, m.w.K, m.w.NB, m.w.J, m.UM, m.w.seg,
                       m.w.pk, m.w.zb, m.ub, m.kb, loudness, peak, range, maxm, maxs, counts, Mout, mstride, Sout, sstride);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// ---- stream meter: the host side.  A state is [nslots] slots of meter_slot_bytes each.
static int64_t meter_ucap(int64_t max_samples, const LoudPlan& p) { return max_samples / p.step + 1; }
static int64_t meter_slot_bytes(int64_t max_samples, const LoudPlan& p) {
    return METER_HEAD_BYTES + align_up(3 * meter_ucap(max_samples, p) * (int64_t)sizeof(double), 256);
}

static int32_t meter_stream(void* state, int64_t state_bytes, int32_t nslots, int64_t max_samples, int32_t fs, const int32_t* slots,
                            int32_t rows, const char* what, LoudPlan& p, MeterStream& ms) {
    TTS_REQUIRE(state && slots, "%s: null argument", what);
    TTS_REQUIRE(nslots >= 1 && nslots <= 65535 && rows >= 1 && rows <= 65535 && max_samples >= 1 && max_samples < ((int64_t)1 << 40),
                "%s: %d slots, %d rows, max_samples %lld", what, nslots, rows, (long long)max_samples);
    TTS_TRY(loud_check_rate(fs, what));
    loud_plan(fs, p);
    ms.state = (char*)state;
    ms.slots = slots;
    ms.slot_bytes = meter_slot_bytes(max_samples, p);
    ms.max_samples = max_samples;
    ms.ucap = meter_ucap(max_samples, p);
    ms.nslots = nslots;
    TTS_REQUIRE(state_bytes >= nslots * ms.slot_bytes, "%s: state of %lld bytes, %lld needed", what, (long long)state_bytes,
                (long long)(nslots * ms.slot_bytes));
    return 0;
}

static int32_t meter_push(void* state, int64_t state_bytes, int32_t nslots, int64_t max_samples, int32_t fs, const float* chunks, int64_t stride,
                          const int64_t* nsamples, const int32_t* slots, int32_t rows, double* momentary, double* short_term,
                          double* integrated, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    LoudPlan p;
    MeterStream ms;
    TTS_TRY(meter_stream(state, state_bytes, nslots, max_samples, fs, slots, rows, "meter_push", p, ms));
    TTS_REQUIRE(nsamples && momentary && short_term && integrated && workspace && (chunks || stride == 0), "meter_push: null argument");
    TTS_REQUIRE(stride >= 0 && stride < ((int64_t)1 << 40), "meter_push: bad stride");
    LoudWs w;
    loud_carve(nullptr, rows, stride + LD_SMAX, p, w);         // the row a push filters: up to S - 1 pending samples, then the chunk
    TTS_REQUIRE(workspace_bytes >= w.bytes, "meter_push: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)w.bytes);
    TTS_REQUIRE(w.NB <= 0x7fffffff, "meter_push: stride too large");
    loud_carve(workspace, rows, stride + LD_SMAX, p, w);
    TTS_TRY(loud_filter<true>(chunks, stride, nsamples, rows, p, w, ms, s));
    hipLaunchKernelGGL(meter_push_kernel, dim3(rows), dim3(LD_GT), 0, s, chunks, stride, nsamples, ms, p.step, p.S, p.Q, w.K, w.NB, w.st, w.seg,
                       w.pk, momentary, short_term, integrated);
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

int64_t ttsamd_loudness_meter_workspace_bytes(int32_t batch, int64_t wave_stride, int32_t sample_rate) {
    if (batch < 1 || wave_stride < 0 || wave_stride >= ((int64_t)1 << 40) || sample_rate < LD_FS_MIN || sample_rate > LD_FS_MAX) return -1;
    LoudPlan p;
    loud_plan(sample_rate, p);
    MeterWs m;
    meter_carve(nullptr, batch, wave_stride, p, m);
    return m.bytes;
}

int32_t ttsamd_loudness_meter(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t sample_rate,
                              double* loudness, float* peak, double* loudness_range, double* max_momentary, double* max_short_term,
                              int64_t* counts, double* momentary, int64_t momentary_stride, double* short_term, int64_t short_term_stride,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    return loudness_meter(wave, wave_stride, nsamples, batch, sample_rate, loudness, peak, loudness_range, max_momentary, max_short_term, counts,
                          momentary, momentary_stride, short_term, short_term_stride, workspace, workspace_bytes, (hipStream_t)stream);
}

int64_t ttsamd_meter_state_bytes(int32_t slots, int64_t max_samples, int32_t sample_rate) {
    if (slots < 1 || slots > 65535 || max_samples < 1 || max_samples >= ((int64_t)1 << 40) || sample_rate < LD_FS_MIN || sample_rate > LD_FS_MAX)
        return -1;
    LoudPlan p;
    loud_plan(sample_rate, p);
    return slots * meter_slot_bytes(max_samples, p);
}

int32_t ttsamd_meter_reset(void* state, int64_t state_bytes, int32_t slots, int64_t max_samples, int32_t sample_rate, const int32_t* slot,
                           int32_t rows, void* stream) {
    LoudPlan p;
    MeterStream ms;
    TTS_TRY(meter_stream(state, state_bytes, slots, max_samples, sample_rate, slot, rows, "meter_reset", p, ms));
    hipLaunchKernelGGL(meter_reset_kernel, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, ms, rows);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

int64_t ttsamd_meter_push_workspace_bytes(int32_t rows, int64_t chunk_stride, int32_t sample_rate) {
    if (chunk_stride < 0 || chunk_stride >= ((int64_t)1 << 40)) return -1;
    return ttsamd_loudness_workspace_bytes(rows, chunk_stride + LD_SMAX, sample_rate);
}

int32_t ttsamd_meter_push(void* state, int64_t state_bytes, int32_t slots, int64_t max_samples, int32_t sample_rate, const float* chunks,
                          int64_t chunk_stride, const int64_t* nsamples, const int32_t* slot, int32_t rows, double* momentary,
                          double* short_term, double* integrated, void* workspace, int64_t workspace_bytes, void* stream) {
    return meter_push(state, state_bytes, slots, max_samples, sample_rate, chunks, chunk_stride, nsamples, slot, rows, momentary, short_term,
                      integrated, workspace, workspace_bytes, (hipStream_t)stream);
}

int32_t ttsamd_meter_result(void* state, int64_t state_bytes, int32_t slots, int64_t max_samples, int32_t sample_rate, const int32_t* slot,
                            int32_t rows, double* loudness, double* loudness_range, double* max_momentary, double* max_short_term, float* peak,
                            int64_t* counts, int32_t* status, void* stream) {
    LoudPlan p;
    MeterStream ms;
    TTS_TRY(meter_stream(state, state_bytes, slots, max_samples, sample_rate, slot, rows, "meter_result", p, ms));
    TTS_REQUIRE(loudness && loudness_range && max_momentary && max_short_term && peak && counts && status, "meter_result: null argument");
    hipLaunchKernelGGL(meter_result_kernel, dim3(rows), dim3(LD_GT), 0, (hipStream_t)stream, ms, p, loudness, loudness_range, max_momentary,
                       max_short_term, peak, counts, status);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
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
