// Recording clean-up around the resampler (include/ttsamd.h states the arithmetic): what the reference does with
// librosa.effects.trim and numpy in scripts/preprocess_audio.py:33-47 and with remove_silence in utils/data.py:59-67,146-157,237-246.
//
// trim_bounds, two launches: trim_frames_kernel (a block of four waves owns 16 centred frames of one row: a wave sums the squares of a
// frame, lane-strided and then by xor shuffles -- a fixed order --, and the block takes max |x| over its own 16 hops of the row) writes
// the frame means and the partial peaks to the workspace; trim_decide_kernel (one block per row) takes the row's peak and the largest
// frame power, marks the frames above 10^(-top_db / 10) of it and writes (start, end).  With gain > 0 the decision is the one for the row
// scaled to that peak (x / peak * gain, what trim_apply writes): the scale only moves the 1e-5 floor of librosa's amplitude_to_db.
// trim_apply: out = fl32(fl32(x / peak) * gain) over [start, end), zeros behind it (correctly rounded division first, multiplication
// second, as numpy's float32 `x / m * 0.999`).
// frames_compact: one block per row; pass 1 finds the last frame whose channel mean is above the threshold, pass 2 walks the frames 256
// at a time, ranks the kept ones by ballot + popcount and a running base, and copies their columns (a plain float copy: bit-exact).
#include <cmath>
#include <vector>

#include "kernels.hpp"

namespace ttsamd {

constexpr int TR_MAXFL = 8192, TR_FPB = 16, TR_THREADS = 256;

__device__ __forceinline__ float tr_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ float tr_wave_max(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ long long tr_wave_max_i(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const long long u = __shfl_xor(v, d, 64);
        v = u > v ? u : v;
    }
    return v;
}

static inline int64_t trim_frames_max(int64_t wave_stride, int32_t hop) { return 1 + wave_stride / hop; }
static inline int64_t trim_blocks(int64_t wave_stride, int32_t hop) { return (trim_frames_max(wave_stride, hop) + TR_FPB - 1) / TR_FPB; }

int64_t trim_workspace_bytes(int32_t B, int64_t wave_stride, int32_t hop) {
    if (B < 1 || wave_stride < 0 || hop < 1) return -1;
    const int64_t nb = trim_blocks(wave_stride, hop);
    return align_up((int64_t)B * nb * TR_FPB * 4, 256) + align_up((int64_t)B * nb * 4, 256);
}

__global__ __launch_bounds__(TR_THREADS) void trim_frames_kernel(const float* __restrict__ wave, int64_t wave_bs,
                                                                 const int64_t* __restrict__ ns, int fl, int hop, int64_t nb,
                                                                 float* __restrict__ ms, float* __restrict__ pk) {
    __shared__ float red[4];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t L = max((int64_t)0, min(ns[b], wave_bs)), T = 1 + L / hop, t0 = (int64_t)blockIdx.x * TR_FPB;
    const float* wb = wave + (int64_t)b * wave_bs;
    float* mb = ms + ((int64_t)b * nb + blockIdx.x) * TR_FPB;
    for (int q = w; q < TR_FPB; q += 4) {
        const int64_t t = t0 + q, g0 = t * hop - fl / 2;
        float s = 0.f;
        if (t < T)
            for (int j = lane; j < fl; j += 64) {
                const int64_t g = g0 + j;
                const float v = (g >= 0 && g < L) ? wb[g] : 0.f;
                s = fmaf(v, v, s);
            }
        s = tr_wave_sum(s);
        if (lane == 0) mb[q] = s / (float)fl;
    }
    float m = 0.f;
    const int64_t e = min(L, (t0 + TR_FPB) * hop);
    for (int64_t g = t0 * hop + tid; g < e; g += TR_THREADS) m = fmaxf(m, fabsf(wb[g]));
    m = tr_wave_max(m);
    if (lane == 0) red[w] = m;
    __syncthreads();
    if (tid == 0) pk[(int64_t)b * nb + blockIdx.x] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

__global__ __launch_bounds__(TR_THREADS) void trim_decide_kernel(const int64_t* __restrict__ ns, int64_t wave_bs, int hop, int64_t nb,
                                                                 const float* __restrict__ ms, const float* __restrict__ pk, float fac,
                                                                 float gain, int64_t* __restrict__ bounds, float* __restrict__ peak) {
    __shared__ float redf[2][4];
    __shared__ long long redi[2][4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t L = max((int64_t)0, min(ns[b], wave_bs)), T = 1 + L / hop;
    const float* mb = ms + (int64_t)b * nb * TR_FPB;
    const float* pb = pk + (int64_t)b * nb;
    float p = 0.f;
    for (int64_t i = tid; i < (T + TR_FPB - 1) / TR_FPB; i += TR_THREADS) p = fmaxf(p, pb[i]);
    p = tr_wave_max(p);
    if (lane == 0) redf[0][w] = p;
    __syncthreads();
    p = fmaxf(fmaxf(redf[0][0], redf[0][1]), fmaxf(redf[0][2], redf[0][3]));
    const float sc = (gain > 0.f && p > 0.f) ? __fmul_rn(__fdiv_rn(1.f, p), gain) : 1.f, sc2 = sc * sc;
    float r = 0.f;
    for (int64_t t = tid; t < T; t += TR_THREADS) r = fmaxf(r, fmaxf(mb[t] * sc2, 1e-10f));
    r = tr_wave_max(r);
    if (lane == 0) redf[1][w] = r;
    __syncthreads();
    r = fmaxf(fmaxf(redf[1][0], redf[1][1]), fmaxf(redf[1][2], redf[1][3]));
    const float thr = fac * r;
    long long lo = -T, hi = -1;                                    // lo: max of -t over the non-silent frames
    for (int64_t t = tid; t < T; t += TR_THREADS)
        if (fmaxf(mb[t] * sc2, 1e-10f) > thr) {
            lo = -t > lo ? -t : lo;
            hi = t > hi ? t : hi;
        }
    lo = tr_wave_max_i(lo);
    hi = tr_wave_max_i(hi);
    if (lane == 0) { redi[0][w] = lo; redi[1][w] = hi; }
    __syncthreads();
    if (tid == 0) {
        for (int q = 1; q < 4; ++q) {
            lo = redi[0][q] > lo ? redi[0][q] : lo;
            hi = redi[1][q] > hi ? redi[1][q] : hi;
        }
        const bool any = hi >= 0;
        bounds[2 * b] = any ? -lo * hop : 0;
        bounds[2 * b + 1] = any ? min(L, (int64_t)((hi + 1) * hop)) : 0;
        if (peak) peak[b] = p;
    }
}

int32_t trim_bounds(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t B, float top_db, int32_t frame_length,
                    int32_t hop, float gain, int64_t* bounds, float* peak, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    TTS_REQUIRE(nsamples && bounds && workspace && (wave || wave_stride == 0), "trim_bounds: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && wave_stride >= 0 && wave_stride < ((int64_t)1 << 40), "trim_bounds: bad batch %d / stride", B);
    TTS_REQUIRE(frame_length >= 1 && frame_length <= TR_MAXFL, "trim_bounds: frame_length %d outside [1, %d]", frame_length, TR_MAXFL);
    TTS_REQUIRE(hop >= 1 && hop <= frame_length, "trim_bounds: hop_length %d outside [1, frame_length = %d]", hop, frame_length);
    TTS_REQUIRE(std::isfinite(top_db) && std::isfinite(gain) && gain >= 0.f, "trim_bounds: top_db %g / gain %g", top_db, gain);
    const int64_t nb = trim_blocks(wave_stride, hop), need = trim_workspace_bytes(B, wave_stride, hop);
    TTS_REQUIRE(nb <= 0x7fffffff, "trim_bounds: stride too large");
    if (workspace_bytes < need) {
        set_error("trim_bounds: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)need);
        return TTSAMD_ENOMEM;
    }
    float* ms = (float*)workspace;
    float* pk = (float*)((char*)workspace + align_up((int64_t)B * nb * TR_FPB * 4, 256));
    const float fac = (float)std::pow(10.0, -(double)top_db / 10.0);
    hipLaunchKernelGGL(trim_frames_kernel, dim3((unsigned)nb, B), dim3(TR_THREADS), 0, s, wave, wave_stride, nsamples, frame_length, hop, nb,
                       ms, pk);
    TTS_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(trim_decide_kernel, dim3(B), dim3(TR_THREADS), 0, s, nsamples, wave_stride, hop, nb, ms, pk, fac, gain, bounds, peak);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void trim_apply_kernel(const float* __restrict__ wave, int64_t wave_bs, const int64_t* __restrict__ bounds,
                                                         const float* __restrict__ peak, float gain, int64_t tail, float* __restrict__ out,
                                                         int64_t out_bs, int64_t* __restrict__ lens_out) {
    const int b = blockIdx.y;
    const int64_t st = min(max(bounds[2 * b], (int64_t)0), wave_bs), en = min(max(bounds[2 * b + 1], st), wave_bs);
    const int64_t len = min(en - st, out_bs);
    if (blockIdx.x == 0 && threadIdx.x == 0 && lens_out) lens_out[b] = min(len + tail, out_bs);
    const float pk = peak ? peak[b] : 0.f;
    const float* wb = wave + (int64_t)b * wave_bs + st;
    float* ob = out + (int64_t)b * out_bs;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < out_bs; i += (int64_t)gridDim.x * 256) {
        float v = 0.f;
        if (i < len) {
            v = wb[i];
            if (pk != 0.f) v = __fmul_rn(__fdiv_rn(v, pk), gain);
        }
        ob[i] = v;
    }
}

int32_t trim_apply(const float* wave, int64_t wave_stride, const int64_t* bounds, const float* peak, float gain, int64_t tail, int32_t B,
                   float* out, int64_t out_stride, int64_t* lens_out, hipStream_t s) {
    TTS_REQUIRE(bounds && (wave || wave_stride == 0) && (out || out_stride == 0), "trim_apply: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && wave_stride >= 0 && out_stride >= 0 && tail >= 0, "trim_apply: bad batch %d / stride / tail", B);
    int64_t nb = (out_stride + 255) / 256;
    nb = nb < 1 ? 1 : (nb > 4096 ? 4096 : nb);
    hipLaunchKernelGGL(trim_apply_kernel, dim3((unsigned)nb, B), dim3(256), 0, s, wave, wave_stride, bounds, peak, gain, tail, out, out_stride,
                       lens_out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

__global__ __launch_bounds__(256) void frames_compact_kernel(const float* __restrict__ mel, const float* __restrict__ extra,
                                                             const int64_t* __restrict__ lens, int C, int C2, int t_max, float thresh,
                                                             float* __restrict__ mel_out, float* __restrict__ extra_out,
                                                             int64_t* __restrict__ lens_out) {
    __shared__ int wcnt[4];
    __shared__ long long redi[4];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int T = (int)max((int64_t)0, min(lens[b], (int64_t)t_max));
    const float* mb = mel + (int64_t)b * C * t_max;
    const float* eb = extra ? extra + (int64_t)b * C2 * t_max : nullptr;
    float* mo = mel_out + (int64_t)b * C * t_max;
    float* eo = extra ? extra_out + (int64_t)b * C2 * t_max : nullptr;
    auto above = [&](const int t) {
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += mb[(int64_t)c * t_max + t];
        return s / (float)C > thresh;
    };
    long long last = -1;
    for (int t = tid; t < T; t += 256)
        if (above(t)) last = t;
    last = tr_wave_max_i(last);
    if (lane == 0) redi[w] = last;
    __syncthreads();
    for (int q = 0; q < 4; ++q) last = redi[q] > last ? redi[q] : last;
    int run = 0;
    for (int t0 = 0; t0 < T; t0 += 256) {
        const int t = t0 + tid;
        // the reference's loop marks every frame behind the last one above the threshold; with none above: frames 1 .. T - 1, not frame 0
        const bool keep = t < T && (last >= 0 ? (t > last || above(t)) : t >= 1);
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) wcnt[w] = __popcll(bal);
        __syncthreads();
        int base = run, total = 0;
        for (int q = 0; q < 4; ++q) {
            if (q < w) base += wcnt[q];
            total += wcnt[q];
        }
        if (keep) {
            const int dst = base + __popcll(bal & ((1ull << lane) - 1ull));
            for (int c = 0; c < C; ++c) mo[(int64_t)c * t_max + dst] = mb[(int64_t)c * t_max + t];
            for (int c = 0; c < C2 && eb; ++c) eo[(int64_t)c * t_max + dst] = eb[(int64_t)c * t_max + t];
        }
        run += total;
        __syncthreads();
    }
    for (int c = 0; c < C; ++c)
        for (int t = run + tid; t < t_max; t += 256) mo[(int64_t)c * t_max + t] = 0.f;
    for (int c = 0; c < C2 && eb; ++c)
        for (int t = run + tid; t < t_max; t += 256) eo[(int64_t)c * t_max + t] = 0.f;
    if (tid == 0) lens_out[b] = run;
}

int32_t frames_compact(const float* mel, const float* extra, const int64_t* lens, int32_t B, int32_t C, int32_t C2, int32_t t_max,
                       float thresh, float* mel_out, float* extra_out, int64_t* lens_out, hipStream_t s) {
    TTS_REQUIRE(lens && lens_out && ((mel && mel_out) || t_max == 0), "frames_compact: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && C >= 1 && t_max >= 0, "frames_compact: bad batch %d / channels %d / t_max %d", B, C, t_max);
    TTS_REQUIRE((extra == nullptr) == (extra_out == nullptr) && (extra == nullptr || C2 >= 1), "frames_compact: extra / extra_out / channels");
    TTS_REQUIRE(mel != mel_out && (extra == nullptr || extra != extra_out), "frames_compact: runs out of place");
    hipLaunchKernelGGL(frames_compact_kernel, dim3(B), dim3(256), 0, s, mel, extra, lens, C, extra ? C2 : 0, t_max, thresh, mel_out, extra_out,
                       lens_out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
