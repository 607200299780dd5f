// HiFi-GAN ResBlock2 (the V3 generator's residual block) in exact fp32 MFMA (v_mfma_f32_32x32x2f32):
//     x1 = x  + conv1d(lrelu(x,  0.1), w1, dil d1) + b1
//     v  = x1 + conv1d(lrelu(x1, 0.1), w2, dil d2) + b2          (vocoder/hifigan/models.py:62-83)
// and the stage-sum epilogue of the engine: y = v | y + v | (y + v) / div (mode 0 | 1 | 2).
//
// Two forms, one source:
//   resblock2_conv  one conv, y = x + conv(lrelu(x), w, d) + b [+ stage sum].  The raw input window (C channels x NT + (K-1)d
//                   columns) is staged ONCE in LDS; the conv reads it through lrelu and the residual is read from the same window,
//                   so x crosses HBM once.  Block = 4 waves x (C rows x NT/4 columns); the window is sized per launch by (K, d).
//   resblock2_pair  both convs in one launch: phase A computes x1 over the NT outputs plus conv 2's halo (H d2 on each side) into
//                   registers, x1 (zero past the utterance edge: the reference convolves the exact-length utterance) replaces the
//                   dead input window in LDS, phase B convolves it.  Saves one HBM round trip of x1 and one launch per ResBlock2;
//                   costs the recomputation of conv 1 over the halo.
// Weights are the direct packing of conv_mfma.hip ([C/8][K][2][C][4]: one float4 = one lane's A operands of four MFMAs) and
// stream from L2 as A operands through a register ring PF steps deep (a step = one (octet, tap)); all waves of a block read the
// same weights.  LDS holds activations only: entry (o, kk, col) = channels 8o + kk + {0,2,4,6} at one position (B operands).
#include <cstring>

#include "conv_mfma_common.hpp"

namespace ttsamd {

struct Rb2Params {
    const float* x;        // [B][C][L] input = residual of conv 1
    float* y;              // [B][C][L]; must not alias x (blocks read x's halo)
    const float4* w1;      // packed [C/8][K][2][C][4]
    const float4* w2;      // (pair only)
    const float* b1;
    const float* b2;
    const int64_t* lens;   // valid length = lens[b] * len_mul (nullptr -> L)
    int32_t len_mul, L, d1, d2;
    int32_t mode;          // 0: y = v   1: y = y + v   2: y = (y + v) / div
    float div, slope;
};

constexpr int kRb2PF = 4;          // weight steps in flight (C / 8 * K steps per conv: a multiple of 4 since C % 32 == 0)
constexpr int kRb2DMax = 16;       // largest dilation either form takes
constexpr int kRb2LdsMax = 160 * 1024;

// Window / tile geometry of one instantiation.  NT outputs per block; the pair's phase A covers NA 32-column tiles
// (NA * 32 >= NT + (K - 1) d2), JA per wave at most.
template <int K, int C, bool PAIR> struct Rb2Geo {
    static constexpr int MT = C / 32;
    static constexpr int NT = PAIR ? (C == 32 ? 256 : 128) : (C == 32 ? 256 : 128);
    static constexpr int JB = NT / 128;                 // 32-column output tiles per wave (phase B / the single conv)
    static constexpr int JA = PAIR ? (C == 32 ? 4 : 3) : 1;
    static constexpr int H = (K - 1) / 2;
};

__device__ __forceinline__ float rb2_lrelu(float v, float s) { return v > 0.f ? v : v * s; }

// acc[mt][j] += conv over all C input channels of LDS window X ([C/8][2][WS] float4) at columns col[j] + t * dil (col[j] includes
// the lane's l31), weights w4 (packed, global).  J tiles share each A operand, MT row tiles share each B operand.
template <int K, int C, int J>
__device__ __forceinline__ void rb2_conv_tiles(f32x16 (&acc)[C / 32][J], const float4* __restrict__ w4, const float4* X, int WS,
                                               const int (&col)[J], int dil, float slope, int kk, int l31) {
    constexpr int MT = C / 32, PF = kRb2PF, NS = C / 8 * K;
    static_assert(NS % PF == 0, "steps per conv must be a multiple of the prefetch depth");
    const float4* __restrict__ wl = w4 + kk * C + l31;        // step s = o * K + t: + s * 2C + 32 mt
    float4 ring[PF][MT];
#pragma unroll
    for (int u = 0; u < PF; ++u)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) ring[u][mt] = wl[(int64_t)u * 2 * C + 32 * mt];
#pragma unroll 1
    for (int s0 = 0; s0 < NS; s0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int s = s0 + u;
            const int o = s / K, t = s - o * K;
            const float4* xs = X + (o * 2 + kk) * WS + t * dil;
            float b[J][4];
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const float4 v = xs[col[j]];
                b[j][0] = rb2_lrelu(v.x, slope); b[j][1] = rb2_lrelu(v.y, slope);
                b[j][2] = rb2_lrelu(v.z, slope); b[j][3] = rb2_lrelu(v.w, slope);
            }
            float a[MT][4];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                a[mt][0] = ring[u][mt].x; a[mt][1] = ring[u][mt].y; a[mt][2] = ring[u][mt].z; a[mt][3] = ring[u][mt].w;
            }
            if (s + PF < NS) {
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) ring[u][mt] = wl[(int64_t)(s + PF) * 2 * C + 32 * mt];
            }
#pragma unroll
            for (int pq = 0; pq < 4; ++pq)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                    for (int j = 0; j < J; ++j)
                        acc[mt][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mt][pq], b[j][pq], acc[mt][j], 0, 0, 0);
        }
    }
}

// acc[mt][j][r] holds channel 32 mt + (r & 3) + 8 (r >> 2) + 4 kk.  Registers (r, r + 2) with r & 3 in {0, 1} are components
// (2 kk, 2 kk + 1) of window entry (4 mt + (r >> 2), r & 1, col): one float2 each.
__device__ __forceinline__ int rb2_entry(int mt, int r, int WS) { return ((4 * mt + (r >> 2)) * 2 + (r & 1)) * WS; }

// Stage columns [x0, x0 + WS) of x[b] raw into X, zero outside [0, len)
template <int C>
__device__ __forceinline__ void rb2_stage(float4* X, const float* __restrict__ xb, int L, int len, int x0, int WS, int tid) {
#pragma unroll 1
    for (int row = 0; row < C / 4; ++row) {                    // row = o * 2 + kk: channels 8o + kk + {0, 2, 4, 6}
        const float* src = xb + (int64_t)((row >> 1) * 8 + (row & 1)) * L;
        for (int col = tid; col < WS; col += 256) {
            const int pos = x0 + col;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (pos >= 0 && pos < len) {
                v.x = src[pos]; v.y = src[(int64_t)2 * L + pos]; v.z = src[(int64_t)4 * L + pos]; v.w = src[(int64_t)6 * L + pos];
            }
            X[row * WS + col] = v;
        }
    }
}

template <int K, int C, bool PAIR>
__global__ __launch_bounds__(256) void resblock2_kernel(const Rb2Params p) {
    using G = Rb2Geo<K, C, PAIR>;
    constexpr int MT = G::MT, NT = G::NT, JB = G::JB, JA = G::JA, H = G::H;
    extern __shared__ __attribute__((aligned(16))) float4 smem4[];
    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kk = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.z;
    const int q0 = blockIdx.x * NT;
    const int L = p.L;
    int len = L;
    if (p.lens) len = min(len, (int)p.lens[b] * p.len_mul);
    if (q0 >= len) return;
    const float slope = p.slope;
    const float* __restrict__ xb = p.x + (int64_t)b * C * L;
    float4* X = smem4;

    // phase B (or the single conv): NT outputs [q0, q0 + NT), window column 0 at position q0 - H d
    const int dB = PAIR ? p.d2 : p.d1;
    const int NA = PAIR ? (NT + (K - 1) * p.d2 + 31) / 32 : 0;     // phase A tiles (x1 columns [q0 - H d2, + NA * 32))
    const int WSB = PAIR ? NA * 32 : NT + (K - 1) * dB;             // columns of the window phase B reads
    const int WS = PAIR ? NA * 32 + (K - 1) * p.d1 : WSB;           // staged columns
    const int x0 = q0 - H * dB - (PAIR ? H * p.d1 : 0);
    rb2_stage<C>(X, xb, L, len, x0, WS, tid);
    __syncthreads();

    if constexpr (PAIR) {
        // ---- phase A: x1 = x + conv(lrelu(x), w1, d1) + b1 over NA tiles, wave w takes tiles w, w + 4, ... ---------------------
        f32x16 accA[MT][JA];
#pragma unroll
        for (int ja = 0; ja < JA; ++ja) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) accA[mt][ja][r] = 0.f;
            const int ti = wid + 4 * ja;
            if (ti < NA) {
                f32x16 a1[MT][1];
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) a1[mt][0] = accA[mt][ja];
                const int col[1] = {ti * 32 + l31};
                rb2_conv_tiles<K, C, 1>(a1, p.w1, X, WS, col, p.d1, slope, kk, l31);
#pragma unroll
                for (int mt = 0; mt < MT; ++mt) accA[mt][ja] = a1[mt][0];
            }
        }
        // + b1 + residual (window column c + H d1); zero outside the utterance
        float x1v[MT][JA][16];
#pragma unroll
        for (int ja = 0; ja < JA; ++ja) {
            const int c = (wid + 4 * ja) * 32 + l31;
            const int pos = q0 - H * p.d2 + c;
            const bool live = (wid + 4 * ja) < NA && pos >= 0 && pos < len;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if ((r & 3) >= 2) continue;
                    float2 res = make_float2(0.f, 0.f);
                    if (live) res = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(X + rb2_entry(mt, r, WS) + c + H * p.d1) + 2 * kk);
                    const int ch = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * kk;
                    x1v[mt][ja][r] = live ? accA[mt][ja][r] + p.b1[ch] + res.x : 0.f;
                    x1v[mt][ja][r + 2] = live ? accA[mt][ja][r + 2] + p.b1[ch + 2] + res.y : 0.f;
                }
        }
        __syncthreads();                                          // every wave is done with the input window
#pragma unroll
        for (int ja = 0; ja < JA; ++ja) {
            if ((wid + 4 * ja) >= NA) continue;
            const int c = (wid + 4 * ja) * 32 + l31;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if ((r & 3) >= 2) continue;
                    *reinterpret_cast<float2*>(reinterpret_cast<float*>(X + rb2_entry(mt, r, WSB) + c) + 2 * kk) =
                        make_float2(x1v[mt][ja][r], x1v[mt][ja][r + 2]);
                }
        }
        __syncthreads();
    }

    // ---- phase B / the single conv: JB tiles per wave, columns wid * 32 JB + 32 j --------------------------------------------
    const float4* wB = PAIR ? p.w2 : p.w1;
    const float* bB = PAIR ? p.b2 : p.b1;
    f32x16 acc[MT][JB];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < JB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][j][r] = 0.f;
    int col[JB];
#pragma unroll
    for (int j = 0; j < JB; ++j) col[j] = (wid * JB + j) * 32 + l31;
    rb2_conv_tiles<K, C, JB>(acc, wB, X, WSB, col, dB, slope, kk, l31);

    // ---- epilogue: + b + residual (window column n + H d) [+ stage sum]; nothing past len is written --------------------------
    float* __restrict__ yb = p.y + (int64_t)b * C * L;
    const int mode = p.mode;
    const float div = p.div;
#pragma unroll
    for (int j = 0; j < JB; ++j) {
        const int n = col[j];
        const int q = q0 + n;
        if (q >= len) continue;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if ((r & 3) >= 2) continue;
                const float2 res = *reinterpret_cast<const float2*>(reinterpret_cast<const float*>(X + rb2_entry(mt, r, WSB) + n + H * dB) + 2 * kk);
                const int ch = 32 * mt + (r & 3) + 8 * (r >> 2) + 4 * kk;
                const float v0 = acc[mt][j][r] + bB[ch] + res.x;
                const float v1 = acc[mt][j][r + 2] + bB[ch + 2] + res.y;
                float* y0 = yb + (int64_t)ch * L + q;
                float* y1 = yb + (int64_t)(ch + 2) * L + q;
                if (mode == 0) {
                    *y0 = v0; *y1 = v1;
                } else if (mode == 1) {
                    *y0 = *y0 + v0; *y1 = *y1 + v1;
                } else {
                    *y0 = (*y0 + v0) / div; *y1 = (*y1 + v1) / div;
                }
            }
    }
}

// dynamic LDS of one launch (bytes)
template <int K, int C, bool PAIR>
static int64_t rb2_lds(int d1, int d2) {
    using G = Rb2Geo<K, C, PAIR>;
    const int64_t ws = PAIR ? (G::NT + (K - 1) * (int64_t)d2 + 31) / 32 * 32 + (K - 1) * (int64_t)d1 : G::NT + (K - 1) * (int64_t)d1;
    return (int64_t)C * ws * 4;
}

template <int K, int C, bool PAIR>
static int32_t rb2_launch_k(const Rb2Params& p, int32_t batch, hipStream_t stream) {
    using G = Rb2Geo<K, C, PAIR>;
    static std::atomic<uint64_t> lds_done{0};          // per instantiation (common.hpp: lds_opt_in); opted in for the largest window
    TTS_CHECK_HIP(lds_opt_in((const void*)resblock2_kernel<K, C, PAIR>, kRb2LdsMax, lds_done));
    const size_t lds = (size_t)rb2_lds<K, C, PAIR>(p.d1, p.d2);
    dim3 grid((p.L + G::NT - 1) / G::NT, 1, batch);
    hipLaunchKernelGGL((resblock2_kernel<K, C, PAIR>), grid, dim3(256), lds, stream, p);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

template <bool PAIR>
static int64_t rb2_lds_any(int32_t channels, int32_t k, int32_t d1, int32_t d2) {
#define RB2_C(KK)                                                                    \
    if (channels == 32) return rb2_lds<KK, 32, PAIR>(d1, d2);                        \
    if (channels == 64) return rb2_lds<KK, 64, PAIR>(d1, d2);                        \
    if (!PAIR && channels == 128) return rb2_lds<KK, 128, PAIR>(d1, d2);             \
    return -1;
    switch (k) {
        case 3: { RB2_C(3) }
        case 5: { RB2_C(5) }
        case 7: { RB2_C(7) }
        case 11: { RB2_C(11) }
        default: return -1;
    }
#undef RB2_C
}

bool resblock2_conv_supported(int32_t channels, int32_t k, int32_t dil, int32_t L, const float* x, const float* y) {
    if (dil < 1 || dil > kRb2DMax || L < 1 || x == y) return false;
    const int64_t lds = rb2_lds_any<false>(channels, k, dil, 1);
    return lds > 0 && lds <= kRb2LdsMax && (int64_t)channels * L < ((int64_t)1 << 31);
}

bool resblock2_pair_supported(int32_t channels, int32_t k, int32_t d1, int32_t d2, int32_t L, const float* x, const float* y) {
    if (d1 < 1 || d1 > kRb2DMax || d2 < 1 || d2 > kRb2DMax || L < 1 || x == y || (channels != 32 && channels != 64)) return false;
    const int nt = channels == 32 ? 256 : 128, ja = channels == 32 ? 4 : 3;
    const int na = (nt + (k - 1) * d2 + 31) / 32;
    const int64_t lds = rb2_lds_any<true>(channels, k, d1, d2);
    return na <= 4 * ja && lds > 0 && lds <= kRb2LdsMax && (int64_t)channels * L < ((int64_t)1 << 31);
}

template <bool PAIR>
static int32_t rb2_dispatch(int32_t channels, int32_t k, const Rb2Params& p, int32_t batch, hipStream_t s) {
#define RB2_C(KK)                                                                    \
    if (channels == 32) return rb2_launch_k<KK, 32, PAIR>(p, batch, s);              \
    if (channels == 64) return rb2_launch_k<KK, 64, PAIR>(p, batch, s);              \
    if constexpr (!PAIR) if (channels == 128) return rb2_launch_k<KK, 128, PAIR>(p, batch, s); \
    break;
    switch (k) {
        case 3: { RB2_C(3) }
        case 5: { RB2_C(5) }
        case 7: { RB2_C(7) }
        case 11: { RB2_C(11) }
        default: break;
    }
#undef RB2_C
    set_error("resblock2: no kernel for C = %d, k = %d", channels, k);
    return TTSAMD_EINVAL;
}

int32_t launch_resblock2_conv(int32_t channels, const float* x, float* y, const float* w, const float* b, int32_t k, int32_t dil,
                              const int64_t* lens, int32_t len_mul, int32_t L, int32_t batch, int32_t mode, float div, float slope,
                              hipStream_t stream) {
    TTS_REQUIRE(resblock2_conv_supported(channels, k, dil, L, x, y),
                "resblock2_conv: unsupported geometry (C=%d, k=%d, dil=%d, L=%d; built for C = 32 / 64 / 128, k = 3 / 5 / 7 / 11, "
                "dilation 1..%d, x != y)", channels, k, dil, L, kRb2DMax);
    TTS_REQUIRE(batch >= 1 && mode >= 0 && mode <= 2 && len_mul >= 1, "resblock2_conv: bad argument");
    conv_log("rb2_conv", k, channels, channels, L, batch, 1, mode, len_mul, lens != nullptr, 1);
    Rb2Params p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.y = y; p.w1 = reinterpret_cast<const float4*>(w); p.b1 = b;
    p.lens = lens; p.len_mul = len_mul; p.L = L; p.d1 = dil; p.d2 = 1; p.mode = mode; p.div = div; p.slope = slope;
    return rb2_dispatch<false>(channels, k, p, batch, stream);
}

int32_t launch_resblock2_pair(int32_t channels, const float* x, float* y, const float* w1, const float* b1, const float* w2,
                              const float* b2, int32_t k, int32_t d1, int32_t d2, const int64_t* lens, int32_t len_mul, int32_t L,
                              int32_t batch, int32_t mode, float div, float slope, hipStream_t stream) {
    TTS_REQUIRE(resblock2_pair_supported(channels, k, d1, d2, L, x, y),
                "resblock2_pair: unsupported geometry (C=%d, k=%d, dilations %d / %d, L=%d; built for C = 32 / 64, k = 3 / 5 / 7 / 11, "
                "dilations 1..%d with (k - 1) d2 <= 256 at C = 32 / 256 at C = 64, x != y)", channels, k, d1, d2, L, kRb2DMax);
    TTS_REQUIRE(batch >= 1 && mode >= 0 && mode <= 2 && len_mul >= 1, "resblock2_pair: bad argument");
    conv_log("rb2_pair", k, channels, channels, L, batch, 1, mode, len_mul, lens != nullptr, 1);
    Rb2Params p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.y = y; p.w1 = reinterpret_cast<const float4*>(w1); p.w2 = reinterpret_cast<const float4*>(w2); p.b1 = b1; p.b2 = b2;
    p.lens = lens; p.len_mul = len_mul; p.L = L; p.d1 = d1; p.d2 = d2; p.mode = mode; p.div = div; p.slope = slope;
    return rb2_dispatch<true>(channels, k, p, batch, stream);
}

}  // namespace ttsamd
