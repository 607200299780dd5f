// Streaming synthesis (include/ttsamd.h states the contracts; ttsamd/stream.py is the scheduler): the receptive
// field of a HiFi-GAN handle in mel frames, and the copies around the vocoder call of one streaming step.
//
// stream_gather: windows of mel frames of many open utterances, out of their slots of a pool, into the packed ragged batch the
// generator takes.  One launch, a block per (window, group of SG_ROWS mel bins), threads along time (coalesced; a window starts at any
// frame, so the source rows are unaligned: dword loads).  stream_emit: the cores of the window waves into the chunk buffer, as fp32 or
// as 16-bit PCM.  One launch, a thread per eight samples: offsets and lengths are multiples of the hop, so two 16-byte loads and one
// or two 16-byte stores.  stream_emit_resampled: the same step with the polyphase resampler of resample.hip and an encoder (int16 PCM,
// G.711 mu-law / A-law) in between, for streams that leave at another rate: the tiling and the fma chain of resample_general_kernel over
// the window rows, so that a chunk holds the bits the whole-utterance resampler gives; wave_encode is its encoder alone, for finished
// waves.  The window descriptors are host values and travel as a by-value table in the launch arguments: no staging
// buffer, no copy, nothing to synchronise on.  They are checked on the host before the launch; the kernels index with them as given.
#include <cmath>

#include "kernels.hpp"
#include "stream_plan.hpp"

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
__device__ __forceinline__ int pcm16_value(float x) {
    const float v = rintf(__fmul_rn(x, 32767.0f));
    return x != x ? 0 : (int)fminf(fmaxf(v, -32768.0f), 32767.0f);
}
__device__ __forceinline__ unsigned pcm16(float x) { return (unsigned)pcm16_value(x) & 0xffffu; }

// G.711 from the 16-bit value s (include/ttsamd.h restates both; tests/golden/g711.npz holds every value).  mu-law: 14-bit magnitude
// plus the bias 33, clipped to 8191, as sign | exponent | 4 mantissa bits, complemented
__device__ __forceinline__ unsigned mulaw8(int s) {
    const int a = s >> 2, neg = a < 0;
    const int m = min((neg ? -a : a) + 33, 8191);
    const int e = 26 - __clz(m);                                         // floor(log2(m)) - 5, m >= 33
    return ~(unsigned)(neg << 7 | e << 4 | ((m >> (e + 1)) & 15)) & 0xffu;
}
// A-law: 13-bit value, one's complement magnitude, segment | 4 mantissa bits, even bits inverted
__device__ __forceinline__ unsigned alaw8(int s) {
    int a = s >> 3;
    const int pos = a >= 0;
    a = pos ? a : ~a;
    const int seg = a < 32 ? 0 : 27 - __clz(a);                          // floor(log2(a)) - 4
    const int mant = seg < 2 ? (a >> 1) & 15 : (a >> seg) & 15;
    return (unsigned)(pos << 7 | seg << 4 | mant) ^ 0x55u;
}
// formats of ttsamd_stream_emit_resampled / ttsamd_wave_encode: 0 fp32 (its bits), 1 int16 PCM, 2 mu-law, 3 A-law
template <int FORMAT>
__device__ __forceinline__ unsigned encode_sample(float x) {
    if (FORMAT == 0) return __float_as_uint(x);
    if (FORMAT == 1) return pcm16(x);
    return FORMAT == 2 ? mulaw8(pcm16_value(x)) : alaw8(pcm16_value(x));
}
template <int FORMAT>
struct FormatBytes {
    static constexpr int value = FORMAT == 0 ? 4 : FORMAT == 1 ? 2 : 1;
};

// Elements [e_a, e_b) of `out` (element = ES bytes, out 4-byte aligned) from vals[e - e_a]: the 32-bit words that lie wholly inside are
// stored packed, the elements of a word shared with a neighbour (another block, another row, the guard behind the buffer) one by one.
// Thread t of nthreads takes the words first + t, first + t + nthreads, ...
template <int ES, typename F>
__device__ __forceinline__ void store_packed(void* __restrict__ out, int64_t e_a, int64_t e_b, int t, int nthreads, F val) {
    constexpr int Q = 4 / ES;
    const int64_t wd0 = e_a / Q, nw = (e_b - 1) / Q - wd0 + 1;
    for (int64_t i = t; i < nw; i += nthreads) {
        const int64_t first = (wd0 + i) * Q;
        if (first >= e_a && first + Q <= e_b) {
            unsigned v = 0;
#pragma unroll
            for (int q = 0; q < Q; ++q) v |= val(first + q - e_a) << (8 * ES * q);
            reinterpret_cast<unsigned*>(out)[wd0 + i] = v;
        } else {
#pragma unroll
            for (int q = 0; q < Q; ++q) {
                const int64_t e = first + q;
                if (e >= e_a && e < e_b) {
                    if (ES == 2) reinterpret_cast<unsigned short*>(out)[e] = (unsigned short)val(e - e_a);
                    else reinterpret_cast<unsigned char*>(out)[e] = (unsigned char)val(e - e_a);
                }
            }
        }
    }
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

// stream_emit with the polyphase resampler and the encoder between the window waves and the chunk rows (ttsamd.h).  The tiling is
// resample_general_kernel's: block (run of FR frames, chunk of PC phases) of window blockIdx.y, one output per thread, the input strip of
// the run in LDS in chunks of JC taps, the same fp32 fma chain over j ascending from +0.  Frames count from the window's first one,
// K0 / n; of the strip only the utterance samples [lo, hi) of the table are read from the row, the others are zeros (outside the
// utterance: the resampler's own padding; inside: samples that only outputs outside [K0, K1) take, which are not stored).  A block's
// outputs are one run of k, slot tid of obuf = k_b + tid: they are encoded into LDS and leave through store_packed.
template <int FORMAT>
__global__ __launch_bounds__(EMIT_THREADS) void stream_emit_resampled_kernel(const float* __restrict__ wave, int64_t wave_bs, const EmitTable tab,
                                                                             const float* __restrict__ tapsT, int NP, int J, int o, int n,
                                                                             int width, int FR, int PC, int PCH, int JC, int c_max,
                                                                             void* __restrict__ out) {
    __shared__ float strip[EMIT_LDS];
    __shared__ unsigned obuf[EMIT_THREADS];
    const int w = blockIdx.y, tid = threadIdx.x;
    const int64_t run = blockIdx.x / PCH;
    const int pch = blockIdx.x % PCH;
    const int64_t K0 = tab.k0[w], K1 = K0 + tab.nout[w];
    const int64_t fb = K0 / n + run * FR;                        // the block's first frame
    const int64_t kb = fb * n + (int64_t)pch * PC;               // ... and first output
    const int seg = PCH == 1 ? FR * n : min(PC, n - pch * PC);
    const int64_t ka = max(kb, K0), ke = min(kb + seg, K0 + c_max);
    if (ka >= ke) return;                                        // (block-uniform) nothing of the chunk row
    float acc = 0.f;
    if (kb < K1) {                                               // (block-uniform) else zeros behind the row's outputs
        const int fl = tid / PC, p = pch * PC + tid % PC;
        const bool active = fl < FR && p < n;
        const int64_t lo = tab.lo[w], hi = tab.hi[w];
        const float* wb = wave + (int64_t)w * wave_bs;
        const int64_t ws = tab.start[w];
        const float* tp = tapsT + (active ? p : 0);
        const int so = fl < FR ? fl * o : 0;
        for (int j0 = 0; j0 < J; j0 += JC) {
            const int jn = min(JC, J - j0), span = (FR - 1) * o + jn;
            const int64_t g0 = fb * o - width + j0;
            __syncthreads();
            for (int s = tid; s < span; s += EMIT_THREADS) {
                const int64_t g = g0 + s;
                strip[s] = (g >= lo && g < hi) ? wb[g - ws] : 0.f;
            }
            __syncthreads();
            if (tapsT) {
                const float* tj = tp + (int64_t)j0 * NP;
#pragma unroll 8
                for (int jj = 0; jj < jn; ++jj) acc = fmaf(tj[(int64_t)jj * NP], strip[so + jj], acc);
            } else {
                acc = fmaf(1.0f, strip[so], acc);                // rate unchanged: J = 1
            }
        }
    }
    obuf[tid] = kb + tid < K1 ? encode_sample<FORMAT>(acc) : 0u;
    __syncthreads();
    const int64_t row = (int64_t)w * c_max - K0;                 // element of out = row + k
    const int skip = (int)(ka - kb);
    store_packed<FormatBytes<FORMAT>::value>(out, row + ka, row + ke, tid, EMIT_THREADS, [&](int64_t i) { return obuf[skip + i]; });
}

int32_t stream_emit_resampled(const Resample* h, const float* wave, int32_t W, int32_t w_max, int32_t hop, const int32_t* win_start,
                              const int32_t* win_len, const int32_t* utt_len, const int32_t* core_start, const int32_t* core_end,
                              int32_t c_max, int32_t format, void* out, int32_t* nout, hipStream_t s) {
    TTS_REQUIRE(wave && out, "stream_emit_resampled: null argument");
    TTS_REQUIRE(((uintptr_t)wave & 3) == 0 && ((uintptr_t)out & 3) == 0, "stream_emit_resampled: wave and out must be 4-byte aligned");
    const ResampleView rv = h ? resample_view(h) : ResampleView{nullptr, 1, 1, 0, 1, 1};
    EmitTable tab = {};
    TTS_TRY(stream_emit_plan(rv, W, w_max, hop, win_start, win_len, utt_len, core_start, core_end, c_max, format, &tab, nout));
    const EmitTiling t = emit_tiling(rv.o, rv.n);
    const int64_t frames = ((int64_t)c_max + rv.n - 2) / rv.n + 1;       // a row starts K0 mod n outputs into its first frame
    const int64_t runs = (frames + t.FR - 1) / t.FR;
    const dim3 grid((unsigned)(runs * t.PCH), W);
    const int64_t n_max = (int64_t)hop * w_max;
#define EMIT_CASE(F)                                                                                                                        \
    case F:                                                                                                                                 \
        hipLaunchKernelGGL(stream_emit_resampled_kernel<F>, grid, dim3(EMIT_THREADS), 0, s, wave, n_max, tab, rv.tapsT, rv.NP, rv.J, rv.o,   \
                           rv.n, rv.width, t.FR, t.PC, t.PCH, t.JC, c_max, out);                                                            \
        break;
    switch (format) { EMIT_CASE(0) EMIT_CASE(1) EMIT_CASE(2) EMIT_CASE(3) }
#undef EMIT_CASE
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// wave rows -> int16 PCM / mu-law / A-law rows, the encoder of the kernel above; thread t of a row takes the 32-bit words of out that
// the row touches, t-th first
template <int FORMAT>
__global__ __launch_bounds__(256) void wave_encode_kernel(const float* __restrict__ wave, int64_t wave_bs, const int64_t* __restrict__ ns,
                                                          int64_t cols, void* __restrict__ out, int64_t out_bs) {
    const int b = blockIdx.y;
    const int64_t L = ns ? max((int64_t)0, min(ns[b], wave_bs)) : wave_bs;
    const float* wb = wave + (int64_t)b * wave_bs;
    const int64_t e_a = (int64_t)b * out_bs;
    store_packed<FormatBytes<FORMAT>::value>(out, e_a, e_a + cols, (int)(blockIdx.x * 256 + threadIdx.x), (int)(gridDim.x * 256),
                                             [&](int64_t i) { return i < L ? encode_sample<FORMAT>(wb[i]) : 0u; });
}

int32_t wave_encode(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t B, int32_t format, void* out,
                    int64_t out_stride, hipStream_t s) {
    TTS_REQUIRE(wave && out, "wave_encode: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535, "wave_encode: batch %d outside [1, 65535]", B);
    TTS_REQUIRE(format >= 1 && format <= 3, "wave_encode: format %d (1 = int16 PCM, 2 = mu-law, 3 = A-law)", format);
    TTS_REQUIRE(wave_stride >= 0 && out_stride >= 0 && wave_stride < ((int64_t)1 << 40) && out_stride < ((int64_t)1 << 40),
                "wave_encode: bad stride");
    TTS_REQUIRE(((uintptr_t)wave & 3) == 0 && ((uintptr_t)out & 3) == 0, "wave_encode: wave and out must be 4-byte aligned");
    const int64_t cols = wave_stride < out_stride ? wave_stride : out_stride;
    if (cols == 0) return 0;
    const int64_t words = cols / (format == 1 ? 2 : 4) + 2;
    const int64_t blocks = (words + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096), B);
    if (format == 1) hipLaunchKernelGGL(wave_encode_kernel<1>, grid, dim3(256), 0, s, wave, wave_stride, nsamples, cols, out, out_stride);
    else if (format == 2) hipLaunchKernelGGL(wave_encode_kernel<2>, grid, dim3(256), 0, s, wave, wave_stride, nsamples, cols, out, out_stride);
    else hipLaunchKernelGGL(wave_encode_kernel<3>, grid, dim3(256), 0, s, wave, wave_stride, nsamples, cols, out, out_stride);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
