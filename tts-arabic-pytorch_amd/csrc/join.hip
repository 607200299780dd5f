// Paragraph join (include/ttsamd.h states the arithmetic): the rows of a ragged batch of waves become ONE row, each
// cut to its speech bounds (ttsamd_trim_bounds' output, widened by `keep`), faded at both edges, with an exact run of zeros behind it or
// overlap-added onto the next row where the gap is negative.  Nothing leaves the device.
//
// wave_join, two launches: join_scan_kernel (one block: every row's source range and length in parallel, the effective gaps from the
// neighbouring lengths, then one block-wide prefix sum of length + gap: 256 threads each own a run of consecutive rows) writes `segs`
// and `total`; join_gather_kernel walks the output four samples a thread: a binary search in the rows' output starts (segs, 32 bytes a
// row: L2) finds the last row that starts at or before the first sample, the next three only step forward.  At most that row and the one
// before it cover a sample (the halves in the effective gap), so a sample is 0, one faded source sample or the rounded sum of two.
// Source loads are plain dwords (the offset into a row is arbitrary); stores are float4 where out + j is 16-byte aligned, the up to three
// samples in front of the first aligned one and behind the last whole quad go out one by one from the threads behind the quads.
#include <algorithm>

#include "kernels.hpp"

namespace ttsamd {

constexpr int JN_MAXB = 4096, JN_MAXF = 4096, JN_THREADS = 256;
constexpr long long JN_MAXGAP = 1ll << 40;

__global__ __launch_bounds__(JN_THREADS) void join_scan_kernel(const int64_t* __restrict__ ns, const int64_t* __restrict__ bounds,
                                                               const int64_t* __restrict__ gap, int B, int64_t wave_bs, int F, int64_t keep,
                                                               int64_t lead, int64_t* __restrict__ segs, int64_t* __restrict__ total) {
    __shared__ long long sm[JN_MAXB];
    __shared__ long long part[2][JN_THREADS];
    const int tid = threadIdx.x;
    for (int b = tid; b < B; b += JN_THREADS) {
        const int64_t n = max((int64_t)0, min(ns[b], wave_bs));
        int64_t s = 0, e = n;
        if (bounds) {
            s = min(max(bounds[2 * b], (int64_t)0), n);
            e = min(max(bounds[2 * b + 1], s), n);
        }
        if (e > s) {
            s = max((int64_t)0, s - keep);
            e = min(n, e + keep);
        }
        sm[b] = e - s;
        segs[4 * b + 2] = s;
        segs[4 * b + 3] = e;
    }
    __syncthreads();
    // length + effective gap of row b: what the next row's start adds to this row's
    auto step = [&](const int b) -> long long {
        const long long m = sm[b], g = gap[b];
        if (g >= 0) return m + min(g, JN_MAXGAP);
        if (b == B - 1) return m;
        const long long want = g < -(long long)F ? (long long)F : -g;
        return m - min(want, min(m / 2, sm[b + 1] / 2));
    };
    const int R = (B + JN_THREADS - 1) / JN_THREADS, b0 = min(tid * R, B), b1 = min(b0 + R, B);
    long long sum = 0;
    for (int b = b0; b < b1; ++b) sum += step(b);
    part[0][tid] = sum;
    __syncthreads();
    int cur = 0;
    for (int d = 1; d < JN_THREADS; d <<= 1) {                     // inclusive prefix sum of the 256 partial sums
        part[cur ^ 1][tid] = part[cur][tid] + (tid >= d ? part[cur][tid - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    long long p = lead + (tid ? part[cur][tid - 1] : 0);
    for (int b = b0; b < b1; ++b) {
        segs[4 * b] = p;
        segs[4 * b + 1] = p + sm[b];
        p += step(b);
    }
    if (b1 == B && b0 < B) total[0] = p;                           // the thread that owns the last row: p_{B-1} + m_{B-1} + max(g_{B-1}, 0)
}

// the value of output sample j given r = the last row with out_start <= j (-1: none)
__device__ __forceinline__ float join_sample(const float* __restrict__ wave, int64_t wave_bs, const int64_t* __restrict__ segs,
                                             const float* __restrict__ fade, int F, int64_t j, int r) {
    float v[2] = {0.f, 0.f};
    int n = 0;
    for (int q = r; q >= 0 && q >= r - 1; --q) {
        const int64_t p = segs[4 * q], m = segs[4 * q + 1] - p, i = j - p;
        if (i < m) {
            const int64_t back = m - 1 - i;
            const float x = wave[(int64_t)q * wave_bs + segs[4 * q + 2] + i];
            v[n++] = __fmul_rn(__fmul_rn(x, i < F ? fade[i] : 1.f), back < F ? fade[back] : 1.f);
        }
    }
    return n == 2 ? __fadd_rn(v[0], v[1]) : v[0];
}

__global__ __launch_bounds__(JN_THREADS) void join_gather_kernel(const float* __restrict__ wave, int64_t wave_bs,
                                                                 const int64_t* __restrict__ segs, const int64_t* __restrict__ total, int B,
                                                                 const float* __restrict__ fade, int F, float* __restrict__ out,
                                                                 int64_t out_bs, int64_t head, int64_t nquad) {
    const int64_t t = (int64_t)blockIdx.x * JN_THREADS + threadIdx.x;
    int64_t j0;
    int cnt;
    if (t < nquad) {
        j0 = head + 4 * t;
        cnt = 4;
    } else {                                                        // the loose samples: `head` in front, the rest behind the quads
        const int64_t k = t - nquad;
        j0 = k < head ? k : head + 4 * nquad + (k - head);
        cnt = j0 < out_bs ? 1 : 0;
    }
    if (cnt == 0) return;
    const int64_t tot = total[0];
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (j0 < tot) {
        int lo = -1, hi = B - 1;                                    // the last row with out_start <= j0 (starts never decrease)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (segs[4 * mid] <= j0) lo = mid; else hi = mid - 1;
        }
        int r = lo;
        for (int k = 0; k < cnt; ++k) {
            const int64_t j = j0 + k;
            if (j >= tot) break;
            while (r + 1 < B && segs[4 * (r + 1)] <= j) ++r;
            v[k] = join_sample(wave, wave_bs, segs, fade, F, j, r);
        }
    }
    if (cnt == 4)
        *reinterpret_cast<float4*>(out + j0) = make_float4(v[0], v[1], v[2], v[3]);
    else
        out[j0] = v[0];
}

int32_t wave_join(const float* wave, int64_t wave_stride, const int64_t* nsamples, const int64_t* bounds, const int64_t* gap, int32_t B,
                  const float* fade, int32_t F, int64_t keep, int64_t lead, float* out, int64_t out_stride, int64_t* segs, int64_t* total,
                  hipStream_t s) {
    TTS_REQUIRE(wave && nsamples && gap && out && segs && total, "wave_join: null argument");
    TTS_REQUIRE(((uintptr_t)out & 3) == 0, "wave_join: out is not aligned to a float");
    TTS_REQUIRE(B >= 1 && B <= JN_MAXB, "wave_join: %d rows outside [1, %d]", B, JN_MAXB);
    TTS_REQUIRE(F >= 0 && F <= JN_MAXF && (fade || F == 0), "wave_join: a fade table of %d entries (0 .. %d, not NULL unless 0)", F, JN_MAXF);
    TTS_REQUIRE(wave_stride >= 0 && wave_stride < ((int64_t)1 << 40) && out_stride >= 0 && out_stride < ((int64_t)1 << 40),
                "wave_join: bad stride %lld / %lld", (long long)wave_stride, (long long)out_stride);
    TTS_REQUIRE(keep >= 0 && keep < ((int64_t)1 << 40) && lead >= 0 && lead < ((int64_t)1 << 40), "wave_join: keep %lld / lead %lld",
                (long long)keep, (long long)lead);
    hipLaunchKernelGGL(join_scan_kernel, dim3(1), dim3(JN_THREADS), 0, s, nsamples, bounds, gap, B, wave_stride, F, keep, lead, segs, total);
    TTS_CHECK_HIP(hipGetLastError());
    if (out_stride == 0) return 0;
    const int64_t mis = (int64_t)(((uintptr_t)out >> 2) & 3), head = std::min((4 - mis) & 3, out_stride), nquad = (out_stride - head) / 4;
    const int64_t items = nquad + (out_stride - 4 * nquad), nb = (items + JN_THREADS - 1) / JN_THREADS;
    hipLaunchKernelGGL(join_gather_kernel, dim3((unsigned)nb), dim3(JN_THREADS), 0, s, wave, wave_stride, segs, total, B, fade, F, out,
                       out_stride, head, nquad);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
