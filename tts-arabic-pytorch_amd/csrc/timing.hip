// Token and word spans (include/ttsamd.h: ttsamd_token_spans states the arithmetic; DESIGN.md sections 4 and 7): per-token repeat counts
// -> where every token, and every group of tokens (a word), lies in the audio that is delivered.  The counts (FastPitch's reps, the MAS
// durations) and the map of a row (the trim / join table, the resampler's ratio) are already on the device, so the spans are made there
// and ride one small copy; the synthesis calls gain no synchronisation point.
//
// One launch, one block of 256 threads per row.  Pass 1: the exclusive prefix sums c[0..n] of max(reps, 0) into LDS -- 256 tokens a tile,
// a wave64 shuffle scan per 64 tokens, the four wave totals through LDS, the carry across tiles in a register.  Pass 2: token i reads
// c[i], c[i + 1], group g reads c[t0], c[t1], each position goes through the row's map m() and leaves as one 16-byte store.  Bound by
// launch latency: at the cap (8192 tokens) a row reads 64 KB and writes 128 KB.
#include <atomic>

#include "kernels.hpp"

namespace ttsamd {

constexpr int TS_THREADS = 256, TS_WAVES = TS_THREADS / 64, TS_MAXL = 8192;
constexpr long long TS_MAXRATIO = 1ll << 20;
constexpr long long TS_I64MAX = 0x7fffffffffffffffll;

struct SpanMap { long long lo, hi, off, num, den; };

// m(p) = off + ceil((min(max(p hop, lo), hi) - lo) num / den): d = q den + r, so d num / den = q num + r num / den with r num < 2^40
__device__ __forceinline__ long long span_pos(const long long p, const long long hop, const SpanMap& m) {
    long long x = p > TS_I64MAX / hop ? TS_I64MAX : p * hop;                 // p >= 0; saturates instead of wrapping
    x = min(max(x, m.lo), m.hi);
    const unsigned long long d = (unsigned long long)x - (unsigned long long)m.lo, den = (unsigned long long)m.den,
                             num = (unsigned long long)m.num;
    const unsigned long long q = d / den, r = d - q * den;
    return m.off + (long long)(q * num + (r * num + den - 1) / den);
}

__global__ __launch_bounds__(TS_THREADS) void token_spans_kernel(const int64_t* __restrict__ reps, int64_t reps_stride,
                                                                 const int64_t* __restrict__ n_tokens, int L,
                                                                 const int32_t* __restrict__ groups, const int32_t* __restrict__ n_groups,
                                                                 int G, long long hop, const int64_t* __restrict__ map,
                                                                 int64_t* __restrict__ tok, int64_t* __restrict__ grp) {
    extern __shared__ long long ts_lds[];                 // c[0 .. L], then the TS_WAVES wave totals of a tile
    long long* c = ts_lds;
    long long* wsum = ts_lds + L + 1;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = n_tokens ? (int)min(max(n_tokens[b], (int64_t)0), (int64_t)L) : L;
    const int64_t* rb = reps + (int64_t)b * reps_stride;
    long long carry = 0;
    if (tid == 0) c[0] = 0;
    for (int base = 0; base < n; base += TS_THREADS) {    // n is uniform over the block: every thread takes the barriers
        const int i = base + tid;
        long long v = i < n ? max((long long)rb[i], 0ll) : 0ll;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {                // wave64 inclusive scan
            const long long u = __shfl_up(v, o, 64);
            if (lane >= o) v += u;
        }
        if (lane == 63) wsum[wave] = v;
        __syncthreads();
        long long before = carry, all = 0;
#pragma unroll
        for (int w = 0; w < TS_WAVES; ++w) {
            const long long t = wsum[w];
            if (w < wave) before += t;
            all += t;
        }
        if (i < n) c[i + 1] = before + v;
        carry += all;
        __syncthreads();                                  // wsum is rewritten by the next tile; c is read below
    }
    if (n == 0) __syncthreads();                          // c[0]
    SpanMap m = {0, TS_I64MAX, 0, 1, 1};
    if (map) m = {map[5 * b], map[5 * b + 1], map[5 * b + 2], map[5 * b + 3], map[5 * b + 4]};
    const bool bad = m.num < 1 || m.num > TS_MAXRATIO || m.den < 1 || m.den > TS_MAXRATIO || m.hi < m.lo;
    longlong2* tb = reinterpret_cast<longlong2*>(tok) + (int64_t)b * L;
    for (int i = tid; i < L; i += TS_THREADS) {
        longlong2 o = make_longlong2(-1, -1);
        if (!bad) {
            o.x = span_pos(c[min(i, n)], hop, m);
            o.y = span_pos(c[min(i + 1, n)], hop, m);
        }
        tb[i] = o;
    }
    if (!grp) return;
    const int ng = n_groups ? min(max((int)n_groups[b], 0), G) : G;
    const int32_t* gb = groups + (int64_t)b * G * 2;
    longlong2* ob = reinterpret_cast<longlong2*>(grp) + (int64_t)b * G;
    for (int g = tid; g < G; g += TS_THREADS) {
        longlong2 o = make_longlong2(-1, -1);
        if (!bad) {
            int t0 = n, t1 = n;
            if (g < ng) {
                t0 = min(max(gb[2 * g], 0), n);
                t1 = max(min(max(gb[2 * g + 1], 0), n), t0);
            }
            o.x = span_pos(c[t0], hop, m);
            o.y = span_pos(c[t1], hop, m);
        }
        ob[g] = o;
    }
}

int32_t token_spans(const int64_t* reps, int64_t reps_stride, const int64_t* n_tokens, int32_t B, int32_t L, const int32_t* groups,
                    const int32_t* n_groups, int32_t G, int64_t hop, const int64_t* map, int64_t* tok, int64_t* grp, hipStream_t s) {
    TTS_REQUIRE(reps && tok, "token_spans: null reps / tok");
    TTS_REQUIRE(B >= 1 && B <= 65535, "token_spans: %d rows outside [1, 65535]", B);
    TTS_REQUIRE(L >= 1 && L <= TS_MAXL, "token_spans: %d tokens per row outside [1, %d]", L, TS_MAXL);
    TTS_REQUIRE(reps_stride >= L, "token_spans: reps_stride %lld < %d tokens", (long long)reps_stride, L);
    TTS_REQUIRE(G >= 0 && G <= (1 << 20), "token_spans: %d groups per row outside [0, 2^20]", G);
    TTS_REQUIRE(hop >= 1 && hop < ((int64_t)1 << 31), "token_spans: hop %lld outside [1, 2^31)", (long long)hop);
    TTS_REQUIRE(!groups || grp, "token_spans: groups without grp");
    TTS_REQUIRE(!grp || groups, "token_spans: grp without groups");
    TTS_REQUIRE(((uintptr_t)tok & 15) == 0 && ((uintptr_t)grp & 15) == 0, "token_spans: tok / grp are not 16-byte aligned");
    if (G == 0) grp = nullptr;
    const int lds = (int)((L + 1 + TS_WAVES) * sizeof(long long));
    if (lds > 48 * 1024) {
        static std::atomic<uint64_t> done{0};
        TTS_CHECK_HIP(lds_opt_in((const void*)token_spans_kernel, lds, done));
    }
    hipLaunchKernelGGL(token_spans_kernel, dim3(B), dim3(TS_THREADS), lds, s, reps, reps_stride, n_tokens, L, groups, n_groups, G,
                       (long long)hop, map, tok, grp);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
