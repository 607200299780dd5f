// Host side of ttsamd_stream_emit_resampled (stream.hip; include/ttsamd.h states the contract): the checks of the window descriptors, the
// interval arithmetic and the by-value table of the launch.  Plain C++ with no HIP call, so that tools/stream_plan_check.cpp can run
// it under the host sanitizers.  Every product with n is taken in int64.
#pragma once
#include <stdint.h>

#include "../../include/ttsamd.h"

namespace ttsamd {

void set_error(const char* fmt, ...);

// the resampler of a handle as the kernels index it; tapsT == nullptr: rate unchanged (o = n = 1, width = 0, one tap of 1.0)
struct ResampleView {
    const float* tapsT;     // [JP][NP], device
    int o, n, width, J, NP;
};

// window w: its outputs are k in [k0, k0 + nout); the row's sample 0 is utterance sample start; the kernel reads the utterance samples
// [lo, hi) and nothing else of the row
struct EmitTable {
    int64_t k0[TTSAMD_STREAM_MAX_WINDOWS];
    int32_t start[TTSAMD_STREAM_MAX_WINDOWS], lo[TTSAMD_STREAM_MAX_WINDOWS], hi[TTSAMD_STREAM_MAX_WINDOWS], nout[TTSAMD_STREAM_MAX_WINDOWS];
};

// the tiling of resample_general_kernel (resample.hip), which the emit kernel shares: a block of 256 threads owns FR frames x PC phases
constexpr int EMIT_LDS = 8192, EMIT_THREADS = 256;
struct EmitTiling {
    int PC, PCH, FR, JC;
};
inline EmitTiling emit_tiling(int o, int n) {
    EmitTiling t;
    t.PC = n < EMIT_THREADS ? n : EMIT_THREADS;
    t.PCH = (n + t.PC - 1) / t.PC;
    t.FR = EMIT_THREADS / t.PC;
    const int frmax = 1 + (EMIT_LDS - 256) / o;
    t.FR = t.FR > frmax ? frmax : t.FR;
    t.JC = EMIT_LDS - (t.FR - 1) * o;
    return t;
}

#define TTS_PLAN_REQUIRE(cond, ...)         \
    do {                                    \
        if (!(cond)) {                      \
            ttsamd::set_error(__VA_ARGS__); \
            return TTSAMD_EINVAL;           \
        }                                   \
    } while (0)

// Fills tab and nout_host (may be NULL) or returns TTSAMD_EINVAL with a message; nothing is written to nout_host on a refusal.
inline int32_t stream_emit_plan(const ResampleView& rv, int32_t W, int32_t w_max, int32_t hop, const int32_t* win_start, const int32_t* win_len,
                                const int32_t* utt_len, const int32_t* core_start, const int32_t* core_end, int32_t c_max, int32_t format,
                                EmitTable* tab, int32_t* nout_host) {
    TTS_PLAN_REQUIRE(win_start && win_len && utt_len && core_start && core_end && tab, "stream_emit_resampled: null argument");
    TTS_PLAN_REQUIRE(W >= 1 && W <= TTSAMD_STREAM_MAX_WINDOWS, "stream_emit_resampled: %d windows (1 .. %d)", W, TTSAMD_STREAM_MAX_WINDOWS);
    TTS_PLAN_REQUIRE(format >= 0 && format <= 3, "stream_emit_resampled: format %d (0 = float32, 1 = int16 PCM, 2 = mu-law, 3 = A-law)", format);
    TTS_PLAN_REQUIRE(hop >= 1 && w_max >= 1 && (int64_t)hop * w_max < (1ll << 31) && c_max >= 1 && (int64_t)W * c_max < (1ll << 31),
                     "stream_emit_resampled: bad sizes (hop %d, w_max %d, c_max %d)", hop, w_max, c_max);
    TTS_PLAN_REQUIRE(rv.o >= 1 && rv.n >= 1 && rv.width >= 0 && rv.J == 2 * rv.width + rv.o, "stream_emit_resampled: bad resampler handle");
    const int64_t o = rv.o, n = rv.n, row = (int64_t)hop * w_max;
    for (int w = 0; w < W; ++w) {
        const int64_t ws = win_start[w], wl = win_len[w], L = utt_len[w], s0 = core_start[w], s1 = core_end[w];
        TTS_PLAN_REQUIRE(wl >= 1 && wl <= row, "stream_emit_resampled: window %d: %lld samples do not fit the window wave of %lld", w,
                         (long long)wl, (long long)row);
        TTS_PLAN_REQUIRE(ws >= 0 && ws <= s0 && s0 < s1 && s1 <= L && s1 <= ws + wl,
                         "stream_emit_resampled: window %d: core [%lld, %lld) outside the window [%lld, %lld + %lld) or the utterance of %lld "
                         "samples", w, (long long)s0, (long long)s1, (long long)ws, (long long)ws, (long long)wl, (long long)L);
        const int64_t k0 = (n * s0 + o - 1) / o, k1 = (n * s1 + o - 1) / o, no = k1 - k0;
        TTS_PLAN_REQUIRE(no <= c_max, "stream_emit_resampled: window %d: %lld outputs, the chunk row holds c_max = %d", w, (long long)no, c_max);
        int64_t lo = 0, hi = 0;
        if (no > 0) {
            const int64_t f0 = k0 / n, f1 = (k1 - 1) / n;
            lo = f0 * o - rv.width;
            hi = f1 * o - rv.width + rv.J;
            lo = lo < 0 ? 0 : lo;
            hi = hi > L ? L : hi;
            TTS_PLAN_REQUIRE(lo >= ws && hi <= ws + wl,
                             "stream_emit_resampled: window %d: its outputs read the samples [%lld, %lld), the window holds [%lld, %lld)", w,
                             (long long)lo, (long long)hi, (long long)ws, (long long)(ws + wl));
        }
        tab->k0[w] = k0;
        tab->start[w] = (int32_t)ws;
        tab->lo[w] = (int32_t)lo;
        tab->hi[w] = (int32_t)hi;
        tab->nout[w] = (int32_t)no;
    }
    if (nout_host)
        for (int w = 0; w < W; ++w) nout_host[w] = tab->nout[w];
    return 0;
}

}  // namespace ttsamd
