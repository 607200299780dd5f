// Streaming synthesis (include/ttsamd.h states the contracts; ttsamd/stream.py is the scheduler): the receptive
// field of a HiFi-GAN handle in mel frames, and the two copies around the vocoder call of one streaming step.
//
// stream_gather: windows of mel frames of many open utterances, out of their slots of a pool, into the packed ragged batch the
// generator takes.  One launch, a block per (window, group of SG_ROWS mel bins), threads along time (coalesced; a window starts at any
// frame, so the source rows are unaligned: dword loads).  stream_emit: the cores of the window waves into the chunk buffer, as fp32 or
// as 16-bit PCM.  One launch, a thread per eight samples: offsets and lengths are multiples of the hop, so two 16-byte loads and one
// or two 16-byte stores.  The window descriptors are host values and travel as a by-value table in the launch arguments: no staging
// buffer, no copy, nothing to synchronise on.  They are checked on the host before the launch; the kernels index with them as given.
#include <cmath>

#include "kernels.hpp"

namespace ttsamd {

struct HifiGan;
const ttsamd_hifigan_cfg* hifigan_config(const HifiGan* h);

static inline int64_t floor_div(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }
static inline int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

// The samples of one frame, [0, hop - 1], walked back through the generator to the mel frames they depend on (ttsamd.h).  Every layer
// is translation-invariant by whole frames, so the two ends found for one frame are the halos of a core of any length.
int32_t hifigan_halo_frames(const HifiGan* h, int32_t* left, int32_t* right) {
    TTS_REQUIRE(h && left && right, "hifigan_halo_frames: null argument");
    const ttsamd_hifigan_cfg& cfg = *hifigan_config(h);
    int64_t hop = 1;
    for (int i = 0; i < cfg.n_ups; ++i) hop *= cfg.upsample_rates[i];
    int64_t lo = -3, hi = hop - 1 + 3;                                   // conv_post, k = 7
    for (int i = cfg.n_ups - 1; i >= 0; --i) {
        int64_t reach = 0;
        for (int j = 0; j < cfg.n_kernels; ++j) {
            const int64_t half = (cfg.resblock_kernel_sizes[j] - 1) / 2;
            int64_t r = 0;
            if (cfg.resblock == 2) r = half * (cfg.resblock_dilations[j][0] + cfg.resblock_dilations[j][1]);
            else for (int m = 0; m < cfg.n_dilations; ++m) r += half * (cfg.resblock_dilations[j][m] + 1);
            reach = r > reach ? r : reach;
        }
        lo -= reach;
        hi += reach;
        const int64_t u = cfg.upsample_rates[i], kt = cfg.upsample_kernel_sizes[i], p = (kt - u) / 2;
        lo = ceil_div(lo + p - kt + 1, u);
        hi = floor_div(hi + p, u);
    }
    *left = (int32_t)(3 - lo);                                           // conv_pre, k = 7
    *right = (int32_t)(hi + 3);
    return 0;
}

struct StreamTable {
    int32_t a[TTSAMD_STREAM_MAX_WINDOWS], b[TTSAMD_STREAM_MAX_WINDOWS], c[TTSAMD_STREAM_MAX_WINDOWS];
};

constexpr int SG_THREADS = 256, SG_ROWS = 8;

// tab.a / .b / .c = slot, start, len of window blockIdx.y
__global__ __launch_bounds__(SG_THREADS) void stream_gather_kernel(const float* __restrict__ pool, int num_mels, int t_cap,
                                                                   const StreamTable tab, int w_max, float* __restrict__ batch,
                                                                   int64_t* __restrict__ lens) {
    const int w = blockIdx.y, m0 = blockIdx.x * SG_ROWS;
    const int slot = tab.a[w], start = tab.b[w], len = tab.c[w];
    if (lens && blockIdx.x == 0 && threadIdx.x == 0) lens[w] = len;
    const float* src = pool + ((int64_t)slot * num_mels + m0) * t_cap + start;
    float* dst = batch + ((int64_t)w * num_mels + m0) * w_max;
    const int rows = min(SG_ROWS, num_mels - m0);
    for (int r = 0; r < rows; ++r)
        for (int t = threadIdx.x; t < w_max; t += SG_THREADS)
            dst[(int64_t)r * w_max + t] = t < len ? src[(int64_t)r * t_cap + t] : 0.f;
}

int32_t stream_gather(const float* pool, int32_t S, int32_t M, int32_t t_cap, const int32_t* slot, const int32_t* start,
                      const int32_t* len, int32_t W, int32_t w_max, float* batch, int64_t* lens, hipStream_t s) {
    TTS_REQUIRE(pool && slot && start && len && batch, "stream_gather: null argument");
    TTS_REQUIRE(S >= 1 && M >= 1 && t_cap >= 1 && w_max >= 1, "stream_gather: bad sizes (slots %d, mels %d, t_cap %d, w_max %d)", S, M, t_cap,
                w_max);
    TTS_REQUIRE(W >= 1 && W <= TTSAMD_STREAM_MAX_WINDOWS, "stream_gather: %d windows (1 .. %d)", W, TTSAMD_STREAM_MAX_WINDOWS);
    StreamTable tab = {};
    for (int w = 0; w < W; ++w) {
        TTS_REQUIRE(slot[w] >= 0 && slot[w] < S, "stream_gather: window %d: slot %d outside [0, %d)", w, slot[w], S);
        TTS_REQUIRE(start[w] >= 0 && len[w] >= 1 && len[w] <= w_max && (int64_t)start[w] + len[w] <= t_cap,
                    "stream_gather: window %d: frames [%d, %d + %d) do not fit w_max %d / t_cap %d", w, start[w], start[w], len[w], w_max,
                    t_cap);
        tab.a[w] = slot[w]; tab.b[w] = start[w]; tab.c[w] = len[w];
    }
    hipLaunchKernelGGL(stream_gather_kernel, dim3((M + SG_ROWS - 1) / SG_ROWS, W), dim3(SG_THREADS), 0, s, pool, M, t_cap, tab, w_max,
                       batch, lens);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// clip(rint(x * 32767), -32768, 32767) as numpy takes it on fp32 (one fp32 product, round half to even), NaN -> 0
__device__ __forceinline__ unsigned pcm16(float x) {
    const float v = rintf(__fmul_rn(x, 32767.0f));
    const int q = x != x ? 0 : (int)fminf(fmaxf(v, -32768.0f), 32767.0f);
    return (unsigned)q & 0xffffu;
}

// tab.a / .b = core_off, core_len of window blockIdx.y (samples, multiples of 8); thread = eight samples of the chunk row
template <int FORMAT>
__global__ __launch_bounds__(256) void stream_emit_kernel(const float* __restrict__ wave, int64_t wave_bs, const StreamTable tab, int c_max,
                                                          void* __restrict__ out) {
    const int w = blockIdx.y;
    const int i = (blockIdx.x * 256 + threadIdx.x) * 8;
    if (i >= c_max) return;
    float4 lo = make_float4(0.f, 0.f, 0.f, 0.f), hi = lo;
    if (i < tab.b[w]) {
        const float4* src = reinterpret_cast<const float4*>(wave + (int64_t)w * wave_bs + tab.a[w] + i);
        lo = src[0];
        hi = src[1];
    }
    if (FORMAT == 0) {
        float4* dst = reinterpret_cast<float4*>((float*)out + (int64_t)w * c_max + i);
        dst[0] = lo;
        dst[1] = hi;
    } else {
        uint4 v;
        v.x = pcm16(lo.x) | (pcm16(lo.y) << 16);
        v.y = pcm16(lo.z) | (pcm16(lo.w) << 16);
        v.z = pcm16(hi.x) | (pcm16(hi.y) << 16);
        v.w = pcm16(hi.z) | (pcm16(hi.w) << 16);
        *reinterpret_cast<uint4*>((int16_t*)out + (int64_t)w * c_max + i) = v;
    }
}

int32_t stream_emit(const float* wave, int32_t W, int32_t w_max, int32_t hop, const int32_t* core_off, const int32_t* core_len,
                    int32_t c_max, int32_t format, void* out, hipStream_t s) {
    TTS_REQUIRE(wave && core_off && core_len && out, "stream_emit: null argument");
    TTS_REQUIRE(W >= 1 && W <= TTSAMD_STREAM_MAX_WINDOWS, "stream_emit: %d windows (1 .. %d)", W, TTSAMD_STREAM_MAX_WINDOWS);
    TTS_REQUIRE(format == 0 || format == 1, "stream_emit: format %d (0 = float32, 1 = int16 PCM)", format);
    TTS_REQUIRE(hop >= 8 && hop % 8 == 0 && w_max >= 1 && c_max >= 8 && c_max % 8 == 0 && (int64_t)hop * w_max < (1ll << 31),
                "stream_emit: hop %d and c_max %d must be multiples of 8 (w_max %d)", hop, c_max, w_max);
    TTS_REQUIRE(((uintptr_t)wave & 15) == 0 && ((uintptr_t)out & 15) == 0, "stream_emit: wave and out must be 16-byte aligned");
    const int64_t n_max = (int64_t)hop * w_max;
    StreamTable tab = {};
    for (int w = 0; w < W; ++w) {
        TTS_REQUIRE(core_off[w] >= 0 && core_len[w] >= 0 && core_off[w] % hop == 0 && core_len[w] % hop == 0,
                    "stream_emit: window %d: offset %d / length %d are not non-negative multiples of the hop %d", w, core_off[w], core_len[w], hop);
        TTS_REQUIRE(core_len[w] <= c_max && (int64_t)core_off[w] + core_len[w] <= n_max,
                    "stream_emit: window %d: samples [%d, %d + %d) do not fit c_max %d / the window wave of %lld", w, core_off[w], core_off[w],
                    core_len[w], c_max, (long long)n_max);
        tab.a[w] = core_off[w]; tab.b[w] = core_len[w];
    }
    const dim3 grid((c_max / 8 + 255) / 256, W);
    if (format == 0) hipLaunchKernelGGL(stream_emit_kernel<0>, grid, dim3(256), 0, s, wave, n_max, tab, c_max, out);
    else hipLaunchKernelGGL(stream_emit_kernel<1>, grid, dim3(256), 0, s, wave, n_max, tab, c_max, out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
