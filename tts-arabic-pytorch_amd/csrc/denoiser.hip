// HiFi-GAN bias denoiser (vocoder/hifigan/denoiser.py:32-72) on the GPU:
//   STFT(n_fft 1024, hop 256, hann, center/reflect)  ->  |X| - strength*bias, clamp >= 0, keep
//   phase  ->  ISTFT (window, overlap-add, divide by the window envelope).
// denoise() runs ONE kernel per call for STFT -> gain -> ISTFT frames (denoise_fft_kernel: a block per frame, two radix-4 Stockham
// FFTs of 1024 points in LDS, 0.1 MFLOP per frame) + the overlap-add; denoiser_bias_spec (one frame, once per model) is one block of
// the same transform (bias_frame0_kernel).  Framing, tables, reflection and the overlap-add sample are those of stft1024.hpp, shared
// with Vocos' ISTFT head, the mel analysis and Griffin-Lim.
// torchaudio itself is absent from the reference tree; semantics are those of
// torch.stft/istft(center=True, pad_mode='reflect', onesided, unnormalised).
#include <cmath>
#include <vector>

#include "kernels.hpp"
#include "stft1024.hpp"

namespace ttsamd {

struct Denoiser {
    float* dev = nullptr;           // window [1024] | twiddles [1024] x (cos, -sin)
    Stft1024Tables stft = {0, 0};
};

int32_t denoiser_create(Denoiser** out) {
    TTS_REQUIRE(out, "denoiser_create: null argument");
    auto* h = new Denoiser();
    std::vector<float> blob;
    h->stft = stft1024_append_tables(blob);
    hipError_t e = hipMalloc((void**)&h->dev, blob.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->dev, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("denoiser_create: upload failed: %s", hipGetErrorString(e));
        if (h->dev) (void)hipFree(h->dev);
        delete h;
        return TTSAMD_EHIP;
    }
    *out = h;
    return 0;
}

void denoiser_destroy(Denoiser* h) {
    if (!h) return;
    if (h->dev) (void)hipFree(h->dev);
    delete h;
}

// frames[b] = nsamples[b] / hop + 1   (center=True)
__global__ void frame_counts_kernel(const int64_t* __restrict__ ns, int B, int64_t* __restrict__ frames) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b < B) frames[b] = ns[b] / STFT_HOP + 1;
}

// out[b][m] = sum_t Y[b][t][m + pad - t*hop] / sum_t w^2[m + pad - t*hop] over the frame-major frames, m < hop*(frames[b] - 1) + 1024 - 2*pad.
// torch.istft(center) : pad = 512, n_out = hop*(frames-1); Vocos 'same' (spectral_ops.py:47-75): pad = 384, n_out = hop*frames.
__global__ __launch_bounds__(256) void overlap_add_kernel(const float* __restrict__ Y, const float* __restrict__ win,
                                                          const int64_t* __restrict__ frames, int pad, int F,
                                                          float* __restrict__ wave, int64_t wave_bs,
                                                          const float* __restrict__ keep_rows) {
    const int b = blockIdx.y;
    if (keep_rows && !(keep_rows[b] > 0.f)) return;            // denoise_rows: a row without denoising keeps its samples bit for bit
    const int m = blockIdx.x * 256 + threadIdx.x;
    const int fr = (int)frames[b];
    const int n_out = (fr - 1) * STFT_HOP + STFT_N - 2 * pad;
    if (m >= n_out) return;
    wave[(int64_t)b * wave_bs + m] = stft1024_ola_sample(Y + (int64_t)b * STFT_N * F, win, m + pad, fr);
}

int32_t launch_overlap_add(const float* Y, const float* win, const int64_t* frames, int32_t pad, int32_t B, int32_t F, int32_t n_max,
                           float* wave, int64_t wave_bs, hipStream_t s, const float* keep_rows) {
    if (n_max <= 0 || B <= 0) return 0;
    hipLaunchKernelGGL(overlap_add_kernel, dim3((n_max + 255) / 256, B), dim3(256), 0, s, Y, win, frames, pad, F, wave, wave_bs,
                       keep_rows);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// |STFT| of frame 0 of the centred framing (denoiser.py:60-64: bias_spec[:, :, 0]), one block: the frame reflects about sample 0 on its
// left half and, for the shortest wave (513 samples), ends on the row's last sample
__global__ __launch_bounds__(256) void bias_frame0_kernel(const float* __restrict__ wave, const int64_t* __restrict__ ns,
                                                          const float* __restrict__ win, const float2* __restrict__ tw_g,
                                                          float* __restrict__ out) {
    __shared__ float2 buf[2][STFT_N];
    __shared__ float2 tw[STFT_N];
    const int i = threadIdx.x;
    const int n = (int)ns[0];
    stft1024_load_twiddles(tw, tw_g, i);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = i + 256 * r;
        const int m = stft1024_reflect(k - stft1024_pad(1), n);
        buf[0][k] = make_float2(n > 0 ? wave[m] * win[k] : 0.f, 0.f);
    }
    __syncthreads();
    fft1024_stockham(buf[0], buf[1], tw, i);                    // X in buf[1]
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int k = i + 256 * r;                              // bins 0..511, and 512 by thread 0
        if (r == 2 && i != 0) break;
        const float2 x = buf[1][k];
        out[k] = sqrtf(x.x * x.x + x.y * x.y);
    }
}

// ---- denoise(): one block per frame.  x_w = window * reflect-padded frame -> X = FFT(x_w) -> X' = X * max(|X| - strength * bias, 0) / |X|
// (denoiser.py:68-71; the gain is real and depends on |X[k]| = |X[1024 - k]| only, so the Hermitian symmetry of a real signal's spectrum
// survives and the complex inverse transform of X' is real: exactly irfft of its one-sided half, whose DC / Nyquist bins are real already)
// -> y = Re(FFT(conj X')) / 1024 * window -> Y[b][t][k], frame-major for the overlap-add.  FFT = five radix-4 Stockham autosort passes
// over two LDS buffers of 1024 complex (thread i: inputs a[i + 256 r], twiddles tw[r k 256 / p], outputs b[4 (i - k) + k + p r], k = i % p;
// checked against numpy.fft in double before it was written: 4e-14).
__global__ __launch_bounds__(256) void denoise_fft_kernel(const float* __restrict__ wave, int64_t wave_bs, const int64_t* __restrict__ ns,
                                                          const float* __restrict__ bias, float strength,
                                                          const float* __restrict__ strength_rows,
                                                          const float* __restrict__ win, const float2* __restrict__ tw_g, int F,
                                                          float* __restrict__ Y) {
    __shared__ float2 buf[2][STFT_N];
    __shared__ float2 tw[STFT_N];
    const int b = blockIdx.y, t = blockIdx.x, i = threadIdx.x;
    const int n = (int)ns[b];
    if (t >= n / STFT_HOP + 1) return;                          // frames the overlap-add never reads
    if (strength_rows) {
        strength = strength_rows[b];
        if (!(strength > 0.f)) return;                          // ... and a row the overlap-add leaves as it is (no denoising)
    }
    const float* wb = wave + (int64_t)b * wave_bs;
    stft1024_load_twiddles(tw, tw_g, i);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = i + 256 * r;
        const int m = stft1024_reflect(t * STFT_HOP + k - stft1024_pad(1), n);   // centred frame, reflect padding
        buf[0][k] = make_float2(n > 0 ? wb[m] * win[k] : 0.f, 0.f);
    }
    __syncthreads();
    fft1024_stockham(buf[0], buf[1], tw, i);                    // X in buf[1]
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = i + 256 * r;
        const float2 x = buf[1][k];
        const float mag = sqrtf(x.x * x.x + x.y * x.y);
        const float md = fmaxf(mag - bias[k <= STFT_N / 2 ? k : STFT_N - k] * strength, 0.f);
        float2 o;
        if (mag > 0.f) {
            const float g = md / mag;
            o = make_float2(x.x * g, -(x.y * g));               // conj(X'): the inverse transform as a forward one
        } else {
            o = make_float2(md, 0.f);                           // angle(0) = 0
        }
        buf[0][k] = o;
    }
    __syncthreads();
    fft1024_stockham(buf[0], buf[1], tw, i);
    stft1024_store_inverse_frame(buf[1], win, Y + ((int64_t)b * F + t) * STFT_N, i);
}

struct DnWs {
    float* X;               // the time-domain frames [B][F][1024]
    int64_t* frames;
};

static void carve(Arena& a, int B, int F, DnWs& w) {
    w.X = a.take<float>((int64_t)B * STFT_N * F);
    w.frames = a.take<int64_t>(B);
}

int64_t denoiser_workspace_bytes(int32_t B, int32_t n_max) {
    Arena a(nullptr, 0);
    DnWs w;
    carve(a, B, n_max / STFT_HOP + 1, w);
    return a.off;
}

// one launch, no workspace (ws / ws_bytes: unused)
int32_t denoiser_bias_spec(const Denoiser* h, const float* audio, const int64_t* n_dev, int32_t n, float* bias_out,
                           void* ws, int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(h && audio && n_dev && bias_out, "denoiser_bias_spec: null argument");
    TTS_REQUIRE(n > STFT_N / 2, "denoiser: reflect padding needs more than %d samples (got %d)", STFT_N / 2, n);
    (void)ws; (void)ws_bytes;
    hipLaunchKernelGGL(bias_frame0_kernel, dim3(1), dim3(256), 0, s, audio, n_dev, h->dev + h->stft.window,
                       reinterpret_cast<const float2*>(h->dev + h->stft.twiddle), bias_out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// strength_rows: device [B] in place of the scalar (ttsamd_denoise_rows), nullptr: the scalar (ttsamd_denoise).  A row whose strength is
// not > 0 is left untouched bit for bit -- an STFT -> ISTFT round trip is no identity in bits -- which is what the wrappers' `if denoise >
// 0` does per call
int32_t denoise(const Denoiser* h, float* wave, int64_t wave_bs, const int64_t* nsamples, int32_t B, int32_t n_max,
                const float* bias_spec, float strength, const float* strength_rows, void* ws, int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(h && wave && nsamples && bias_spec, "denoise: null argument");
    TTS_REQUIRE(B >= 1 && n_max > STFT_N / 2, "denoise: needs more than %d samples per utterance", STFT_N / 2);
    const int F = n_max / STFT_HOP + 1;
    Arena a(ws, ws_bytes);
    DnWs w;
    carve(a, B, F, w);
    if (!ws || !a.ok) {
        set_error("denoise: workspace of %lld bytes needed, %lld given", (long long)a.off, (long long)ws_bytes);
        return TTSAMD_ENOMEM;
    }
    hipLaunchKernelGGL(frame_counts_kernel, dim3((B + 63) / 64), dim3(64), 0, s, nsamples, B, w.frames);
    // STFT -> gain -> ISTFT frames, one block per frame, time-domain frames into X as [b][frame][k]
    hipLaunchKernelGGL(denoise_fft_kernel, dim3(F, B), dim3(256), 0, s, wave, wave_bs, nsamples, bias_spec, strength, strength_rows,
                       h->dev + h->stft.window, reinterpret_cast<const float2*>(h->dev + h->stft.twiddle), F, w.X);
    TTS_CHECK_HIP(hipGetLastError());
    // center=True: frames = n/hop + 1 (w.frames), pad = 1024/2, n_out = hop*(frames-1)
    return launch_overlap_add(w.X, h->dev + h->stft.window, w.frames, stft1024_pad(1), B, F, n_max, wave, wave_bs, s, strength_rows);
}

}  // namespace ttsamd
