// What the fp32 STFT-1024 kernels share (denoiser.hip, vocos.hip, melspec.hip, griffinlim.hip) around the transform of fft1024.hpp:
// n_fft = win = 1024, hop 256, periodic hann, reflect padding at the row's own ends, framings "same" (pad 384 per side) and "center"
// (pad 512).  The engines agree with each other because each of these pieces is written once, here.  No kernel and no __shared__ in
// this header: the LDS buffers belong to the kernels.
#pragma once
#include "fft1024.hpp"

namespace ttsamd {

constexpr int STFT_N = 1024, STFT_HOP = 256, STFT_NBIN = STFT_N / 2 + 1;      // 513 bins
constexpr int stft1024_pad(const int center) { return center ? STFT_N / 2 : (STFT_N - STFT_HOP) / 2; }

// the periodic hann window, double cos rounded once
inline void hann_window_1024(std::vector<float>& window) {
    const double two_pi = 6.283185307179586476925286766559;
    window.resize(STFT_N);
    for (int k = 0; k < STFT_N; ++k) window[k] = (float)(0.5 - 0.5 * std::cos(two_pi * k / STFT_N));
}

// offsets, in floats, of the window [1024] and the twiddles [1024] x (cos, -sin) in a handle's blob
struct Stft1024Tables {
    int64_t window, twiddle;
};
inline Stft1024Tables stft1024_append_tables(std::vector<float>& blob) {
    std::vector<float> wnd;
    hann_window_1024(wnd);
    Stft1024Tables t;
    t.window = (int64_t)blob.size();
    blob.insert(blob.end(), wnd.begin(), wnd.end());
    t.twiddle = fft1024_append_twiddles(blob);
    return t;
}

#ifdef __HIPCC__
// sample s of the reflect-padded axis of a row of n samples -> its index in the row.  A row no longer than the padding would reflect
// past its other end (torch's reflect pad raises there and so do the Python wrappers): the index is only kept inside [0, n - 1].
// n = 0 gives -1: the caller reads nothing then.
__device__ __forceinline__ int stft1024_reflect(int s, const int n) {
    if (s < 0) s = -s;
    if (s >= n) s = 2 * (n - 1) - s;
    return min(max(s, 0), n - 1);
}

// the block's 256 threads copy the twiddle table into LDS; the caller synchronises
__device__ __forceinline__ void stft1024_load_twiddles(float2* tw, const float2* __restrict__ tw_g, const int i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) tw[i + 256 * r] = tw_g[i + 256 * r];
}

// two real frames in one complex transform (frame t in .x, t + 1 in .y): with z = Z[k] and cz = Z[1024 - k],
// X_t[k] = (z + conj cz) / 2 and X_t+1[k] = (z - conj cz) / 2i
__device__ __forceinline__ void stft1024_unpack_pair(const float2 z, const float2 cz, float2& xa, float2& xb) {
    xa = make_float2(0.5f * (z.x + cz.x), 0.5f * (z.y - cz.y));
    xb = make_float2(0.5f * (z.y + cz.y), 0.5f * (cz.x - z.x));
}

// a sample of an inverse frame: re = the real part Re(FFT(conj X))[k] leaves as re / 1024 * window[k]
__device__ __forceinline__ float stft1024_inverse_sample(const float re, const float w) { return re * (1.0f / STFT_N) * w; }

// the inverse frame in y (LDS, the transform's output) -> row [1024] of a frame-major matrix, by the block's 256 threads
__device__ __forceinline__ void stft1024_store_inverse_frame(const float2* y, const float* __restrict__ win, float* __restrict__ row,
                                                             const int i) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = i + 256 * r;
        row[k] = stft1024_inverse_sample(y[k].x, win[k]);
    }
}

// the overlap-add at position mp of the padded axis of a row of fr frame-major frames Y [fr][1024]: the frames that reach mp, added
// over t ascending, over the sum of their squared windows (torch.istft's envelope)
__device__ __forceinline__ float stft1024_ola_sample(const float* __restrict__ Y, const float* __restrict__ win, const int mp, const int fr) {
    const int t_hi = min(fr - 1, mp / STFT_HOP);
    const int t_lo = mp >= STFT_N ? (mp - STFT_N) / STFT_HOP + 1 : 0;   // first frame with mp - t * hop < 1024
    float acc = 0.f, env = 0.f;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int k = mp - t * STFT_HOP;
        if (k < 0 || k >= STFT_N) continue;
        acc += Y[(int64_t)t * STFT_N + k];
        env += win[k] * win[k];
    }
    return acc / env;
}
#endif

}  // namespace ttsamd
