// Mel analysis, wave -> (log-)mel, in ONE launch: replaces utils/audio.py:35-46 (MelSpectrogram.forward) and
// vocoder/vocos/feature_extractors.py:58-64 (MelSpectrogramFeatures.forward over torchaudio's MelSpectrogram, power = 1).
// n_fft = win = 1024, hop = 256, periodic hann, reflect padding at the utterance's own ends; two framings:
//   same   (pad 384 per side, stft(center=False)):  frames = n / 256      (n >= 385)
//   center (pad 512 per side, stft(center=True)):   frames = n / 256 + 1  (n >= 513)
// A block of 256 threads owns MS_FPB = 16 consecutive frames of one utterance.  Two real frames share one complex 1024-point FFT in LDS
// (fft1024.hpp: frame t in .x, frame t + 1 in .y, t even; the two spectra unpacked by bin k and 1024 - k, stft1024.hpp),
// the magnitudes of bins 0..512 go to an LDS strip, thread (j, m) sums band m of frame t + j over the band's non-zero bin range
// [lo, hi) (found at create from the matrix itself: a dense matrix has the range [0, 513) and is summed in full), its weights read once
// per block from the filterbank stored TRANSPOSED ([513][128]: the lanes of a wave read consecutive floats) when the band has at most 32
// bins, and the block's [n_mels][16] tile leaves through LDS so that the stores run along t (64 bytes per row) in the project's
// [B][n_mels][T_max] layout.  No spectrum and no frame matrix in HBM.  Latency-bound: seven barriers per pair of frames, about 3 us per
// pair for a block alone; HBM (5 % of its peak) and LDS (about an eighth of its rate) are mostly idle (profiles/r8/NOTES.md).
// __launch_bounds__(256, 4): 127 VGPRs without spills, so that four blocks share a CU and the 992 blocks of a B = 32 batch of 496
// frames are resident at once (unbounded the compiler takes 135-143 VGPRs = three blocks per CU: two residency rounds, +10 %).
// Frames at or past the row's own count are written as zero; every value of row b depends on row b's samples only and on t's parity
// pairing, which is the same in a batch and alone: a ragged row equals the call on that row alone bit for bit.
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.hpp"
#include "stft1024.hpp"

namespace ttsamd {

constexpr int MS_MAXMEL = 128, MS_FPB = 16, MS_WREG = 32;

struct MelSpec {
    float* dev = nullptr;     // fbT [513][128] | window [1024] | twiddles [1024] x (cos, -sin)
    int2* range = nullptr;    // [128] (lo, hi): bins of band m outside [lo, hi) are zero
    Stft1024Tables stft = {0, 0};
    int n_mels = 0, center = 0, mag_mode = 0;
    float log_clip = 0.f;
};

int32_t melspec_create(const float* fbank, int32_t n_mels, int32_t n_fft, int32_t hop, int32_t framing, int32_t mag_mode,
                       float log_clip, MelSpec** out) {
    TTS_REQUIRE(fbank && out, "melspec_create: null argument");
    TTS_REQUIRE(n_fft == STFT_N && hop == STFT_HOP, "melspec_create: only n_fft = win = %d, hop = %d is built (got %d / %d)", STFT_N,
                STFT_HOP, n_fft, hop);
    TTS_REQUIRE(n_mels >= 1 && n_mels <= MS_MAXMEL, "melspec_create: n_mels = %d outside [1, %d]", n_mels, MS_MAXMEL);
    TTS_REQUIRE((framing == 0 || framing == 1) && (mag_mode == 0 || mag_mode == 1), "melspec_create: framing / mag_mode must be 0 or 1");
    std::vector<float> blob((size_t)STFT_NBIN * MS_MAXMEL, 0.f);
    std::vector<int2> range(MS_MAXMEL, make_int2(0, 0));
    for (int m = 0; m < n_mels; ++m) {
        int lo = STFT_NBIN, hi = 0;
        for (int f = 0; f < STFT_NBIN; ++f) {
            const float v = fbank[(size_t)m * STFT_NBIN + f];
            blob[(size_t)f * MS_MAXMEL + m] = v;
            if (v != 0.f) {                                     // (NaN != 0 too: a poisoned matrix poisons its band, as a matmul would)
                lo = f < lo ? f : lo;
                hi = f + 1;
            }
        }
        range[m] = hi > lo ? make_int2(lo, hi) : make_int2(0, 0);
    }
    auto* h = new MelSpec();
    h->n_mels = n_mels; h->center = framing; h->mag_mode = mag_mode; h->log_clip = log_clip;
    h->stft = stft1024_append_tables(blob);
    hipError_t e = hipMalloc((void**)&h->dev, blob.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->dev, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&h->range, range.size() * sizeof(int2));
    if (e == hipSuccess) e = hipMemcpy(h->range, range.data(), range.size() * sizeof(int2), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("melspec_create: upload failed: %s", hipGetErrorString(e));
        if (h->dev) (void)hipFree(h->dev);
        if (h->range) (void)hipFree(h->range);
        delete h;
        return TTSAMD_EHIP;
    }
    *out = h;
    return 0;
}

void melspec_destroy(MelSpec* h) {
    if (!h) return;
    if (h->dev) (void)hipFree(h->dev);
    if (h->range) (void)hipFree(h->range);
    delete h;
}

__global__ __launch_bounds__(256, 4) void melspec_kernel(const float* __restrict__ wave, int64_t wave_bs, const int64_t* __restrict__ ns,
                                                      const float* __restrict__ fbT, const int2* __restrict__ range,
                                                      const float* __restrict__ win, const float2* __restrict__ tw_g, int n_mels,
                                                      int center, int mag_mode, float log_clip, int T_max, float* __restrict__ mel,
                                                      int64_t* __restrict__ frames_out) {
    __shared__ float2 buf[2][STFT_N];
    __shared__ float2 tw[STFT_N];
    __shared__ float mag[2][STFT_NBIN + 3];
    __shared__ float tile[MS_MAXMEL][MS_FPB + 1];
    const int b = blockIdx.y, t0 = blockIdx.x * MS_FPB, i = threadIdx.x;
    const int n = (int)max((int64_t)0, min(ns[b], wave_bs));     // indices stay inside the row whatever the caller's lengths say
    const int fr = min(n / STFT_HOP + center, T_max);
    if (blockIdx.x == 0 && i == 0 && frames_out) frames_out[b] = fr;
    float* mb = mel + (int64_t)b * n_mels * T_max;
    if (t0 >= fr || n == 0) {                                    // past the utterance: zeros, coalesced along t
        for (int idx = i; idx < n_mels * MS_FPB; idx += 256) {
            const int m = idx / MS_FPB, tt = idx % MS_FPB;
            if (t0 + tt < T_max) mb[(int64_t)m * T_max + t0 + tt] = 0.f;
        }
        return;
    }
    const float* wb = wave + (int64_t)b * wave_bs;
    const int pad = stft1024_pad(center);
    stft1024_load_twiddles(tw, tw_g, i);
    float w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) w[r] = win[i + 256 * r];
    const int j = i >> 7, m = i & 127;                           // filterbank: thread = (frame of the pair, band)
    const int2 rg = m < n_mels ? range[m] : make_int2(0, 0);
    // a band of at most MS_WREG bins (every triangle of the built configurations: <= 31) keeps its weights in registers for the
    // block's eight pairs; a wider one (a dense user matrix) streams them from L2 per pair.  Both sum over f ascending.
    const int cnt = rg.y - rg.x;
    const bool in_reg = cnt <= MS_WREG;
    float wr[MS_WREG];
#pragma unroll
    for (int q = 0; q < MS_WREG; ++q) wr[q] = (in_reg && q < cnt) ? fbT[(rg.x + q) * MS_MAXMEL + m] : 0.f;
    float xa[4], xb[4];
    auto load_pair = [&](const int t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = t * STFT_HOP + i + 256 * r - pad;        // reflect padding at the utterance's own ends (n > 0 here)
            const int s0 = stft1024_reflect(s, n), s1 = stft1024_reflect(s + STFT_HOP, n);
            xa[r] = t < fr ? wb[s0] : 0.f;
            xb[r] = t + 1 < fr ? wb[s1] : 0.f;
        }
    };
    for (int p = 0; p < MS_FPB / 2; ++p) {
        const int t = t0 + 2 * p;
        if (t >= fr) {                                           // (block-uniform)
            if (m < n_mels) tile[m][2 * p + j] = 0.f;
            continue;
        }
        const bool two = t + 1 < fr;
        load_pair(t);
#pragma unroll
        for (int r = 0; r < 4; ++r) buf[0][i + 256 * r] = make_float2(xa[r] * w[r], xb[r] * w[r]);
        __syncthreads();
        fft1024_stockham(buf[0], buf[1], tw, i);                 // Z in buf[1]
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int k = i + 256 * r;                           // bins 0..511, and 512 by thread 0
            if (r == 2 && i != 0) break;
            const float2 z = buf[1][k], c = buf[1][(STFT_N - k) & (STFT_N - 1)];
            float2 xt, xu;                                       // X_t[k], X_t+1[k]
            stft1024_unpack_pair(z, c, xt, xu);
            float pa = xt.x * xt.x + xt.y * xt.y, pb = xu.x * xu.x + xu.y * xu.y;
            if (mag_mode) { pa += 1e-9f; pb += 1e-9f; }
            mag[0][k] = sqrtf(pa);
            mag[1][k] = sqrtf(pb);
        }
        __syncthreads();
        if (m < n_mels) {
            float acc = 0.f;
            if (j == 0 || two) {
                const float* mg = mag[j];
                if (in_reg) {
#pragma unroll
                    for (int c = 0; c < MS_WREG; c += 8) {       // chunks of 8 unconditional LDS reads (one wait each), the tail selected to 0 * 0:
                        if (c < cnt) {                           // a branch per read serialises on LDS latency, 32 reads for every band on LDS issue
#pragma unroll
                            for (int q = c; q < c + 8; ++q) {
                                // the select must stay on v, not on the product: past the band's end v is another bin's magnitude, which
                                // may be Inf / NaN for such an input, and 0 * v would poison a band the reference leaves finite
                                const float v = mg[min(rg.x + q, STFT_NBIN - 1)];
                                acc += wr[q] * (q < cnt ? v : 0.f);
                            }
                        }
                    }
                } else {
                    for (int f = rg.x; f < rg.y; ++f) acc += fbT[f * MS_MAXMEL + m] * mg[f];
                }
                if (log_clip > 0.f) acc = logf(fmaxf(acc, log_clip));
            }
            tile[m][2 * p + j] = acc;
        }
    }
    __syncthreads();
    for (int idx = i; idx < n_mels * MS_FPB; idx += 256) {
        const int mm = idx / MS_FPB, tt = idx % MS_FPB;
        if (t0 + tt < T_max) mb[(int64_t)mm * T_max + t0 + tt] = tile[mm][tt];
    }
}

int32_t melspec_forward(const MelSpec* h, const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t B, int32_t T_max,
                        float* mel, int64_t* frames_out, hipStream_t s) {
    TTS_REQUIRE(h && wave && nsamples && (mel || T_max == 0), "melspec_forward: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && T_max >= 0 && wave_stride >= 0, "melspec_forward: bad batch %d / t_max %d / stride", B, T_max);
    const int nblk = T_max > 0 ? (T_max + MS_FPB - 1) / MS_FPB : 1;     // t_max = 0: the frame counts only
    hipLaunchKernelGGL(melspec_kernel, dim3(nblk, B), dim3(256), 0, s, wave, wave_stride, nsamples, h->dev, h->range,
                       h->dev + h->stft.window, reinterpret_cast<const float2*>(h->dev + h->stft.twiddle), h->n_mels, h->center, h->mag_mode,
                       h->log_clip, T_max, mel, frames_out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
