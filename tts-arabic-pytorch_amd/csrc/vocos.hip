// MelVocos('22k' / '24k') on the MI355X: ConvNeXt backbone + ISTFT head with "same" (22k) or "center" (24k) padding.
// Replaces vocoder/vocos/pretrained.py:34-93 (MelVocos.__init__/make_denoising_vector/forward),
// models.py:77-89 (VocosBackbone.forward), modules.py:43-60 (ConvNeXtBlock.forward),
// heads.py:41 (ISTFTHead.out) and spectral_ops.py:33-75 (ISTFT.forward, padding="same").
// embed / pwconv1 (+GELU) / pwconv2 (x gamma, + residual) / head.out run on the MFMA conv engine; the
// ISTFT is one 1024-point FFT per frame in LDS (vocos_istft_kernel, fft1024.hpp); depthwise conv,
// LayerNorm (eps 1e-6), exp/cos/sin (+ the transposition to frame-major) and the overlap-add are HBM-bound kernels.  Ragged batches: every layer reads positions >= lens[b]
// as zero, i.e. utterance b equals MelVocos.forward(mel[b:b+1, :, :lens[b]]).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "stft1024.hpp"

namespace ttsamd {

constexpr int V_SPEC_CP = 1152;   // head.out rows: 2 x 513 padded to 9 x 128 (co tiles)

struct VConv {
    int64_t w_off = 0, b_off = -1, w16_off = 0;
    int cin = 0, cout = 0, coutp = 0, k = 0;
};
struct VBlock {
    int64_t dw_w, dw_b, ln_g, ln_b, gamma;
    VConv pw1, pw2;
};
struct Vocos {
    float* dev = nullptr;
    uint16_t* dev16 = nullptr;
    int in_ch = 80, in_chp = 80, dim = 512, inter = 1536;     // in_chp: in_ch rounded up to the conv engine's 8-channel chunks (100 -> 104)
    int center = 0;                                           // ISTFT trimming: 0 "same" (pad 384, 256 T samples), 1 "center" (pad 512, 256 (T - 1))
    VConv embed, head;
    int64_t n0_g, n0_b, fl_g, fl_b;
    Stft1024Tables stft;                                       // vocos_istft_kernel, the overlap-add
    std::vector<VBlock> blocks;
};

using TensorMap = std::map<std::string, const ttsamd_tensor*>;

static int64_t vnumel(const ttsamd_tensor* t) {
    int64_t n = 1;
    for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
    return n;
}

struct VBuilder {
    const TensorMap& tm;
    std::vector<float> blob;
    std::vector<uint16_t> blob16;
    int32_t rc = 0;
    explicit VBuilder(const TensorMap& t) : tm(t) {}
    const ttsamd_tensor* get(const std::string& name, int64_t n) {
        if (rc) return nullptr;
        auto it = tm.find(name);
        if (it == tm.end() || vnumel(it->second) != n) {
            set_error("vocos: missing or mis-sized tensor '%s' (expected %lld elements)", name.c_str(), (long long)n);
            rc = TTSAMD_EINVAL;
            return nullptr;
        }
        return it->second;
    }
    int64_t raw(const std::string& name, int64_t n, int64_t pad_to = 0) {
        const ttsamd_tensor* t = get(name, n);
        if (!t) return 0;
        const int64_t off = (int64_t)blob.size();
        blob.insert(blob.end(), t->data, t->data + n);
        if (pad_to > n) blob.resize(off + pad_to, 0.f);
        blob.resize(align_up((int64_t)blob.size(), 64));
        return off;
    }
    // cin_w: input channels of the stored weight; the cin - cin_w channels the engine's chunking adds carry zero weights
    VConv conv(const std::string& base, int cin, int cout, int k, int coutp, int cin_w = 0) {
        VConv c;
        if (cin_w == 0) cin_w = cin;
        c.cin = cin; c.cout = cout; c.k = k; c.coutp = coutp;
        const ttsamd_tensor* w = get(base + ".weight", (int64_t)cin_w * cout * k);
        if (!w) return c;
        // pack with the padded channel counts: rows >= cout (and input channels >= cin_w) are zero weights
        std::vector<float> wp((size_t)coutp * cin * k, 0.f);
        if (cin_w == cin) {
            std::memcpy(wp.data(), w->data, (size_t)cout * cin * k * sizeof(float));
        } else {
            for (int co = 0; co < cout; ++co)
                std::memcpy(wp.data() + (size_t)co * cin * k, w->data + (size_t)co * cin_w * k, (size_t)cin_w * k * sizeof(float));
        }
        c.w_off = (int64_t)blob.size();
        blob.resize(blob.size() + (size_t)cin * k * coutp);
        pack_conv_weight(wp.data(), coutp, cin, k, blob.data() + c.w_off);
        {
            const int64_t nn = (int64_t)cin * k * coutp;
            c.w16_off = (int64_t)blob16.size();
            blob16.resize(blob16.size() + 2 * nn);
            split_packed_bf16(blob.data() + c.w_off, nn, blob16.data() + c.w16_off);
        }
        blob.resize(align_up((int64_t)blob.size(), 64));
        c.b_off = raw(base + ".bias", cout, coutp);
        return c;
    }
};

int32_t vocos_create(const ttsamd_tensor* weights, int32_t n, int32_t in_ch, int32_t dim, int32_t inter,
                     int32_t n_layers, Vocos** out) {
    TTS_REQUIRE(weights && out, "vocos_create: null argument");
    TTS_REQUIRE(dim % 128 == 0 && inter % 128 == 0 && in_ch >= 1 && n_layers >= 1, "vocos_create: bad dims");
    TensorMap tm;
    for (int i = 0; i < n; ++i) tm[weights[i].name] = &weights[i];
    VBuilder b(tm);
    auto* h = new Vocos();
    h->in_ch = in_ch; h->in_chp = (int)align_up(in_ch, 8); h->dim = dim; h->inter = inter;
    h->embed = b.conv("backbone.embed", h->in_chp, dim, 7, dim, in_ch);
    h->n0_g = b.raw("backbone.norm.weight", dim);
    h->n0_b = b.raw("backbone.norm.bias", dim);
    for (int i = 0; i < n_layers && b.rc == 0; ++i) {
        const std::string p = "backbone.convnext." + std::to_string(i) + ".";
        VBlock bl;
        bl.dw_w = b.raw(p + "dwconv.weight", (int64_t)dim * 7);
        bl.dw_b = b.raw(p + "dwconv.bias", dim);
        bl.ln_g = b.raw(p + "norm.weight", dim);
        bl.ln_b = b.raw(p + "norm.bias", dim);
        bl.pw1 = b.conv(p + "pwconv1", dim, inter, 1, inter);
        bl.pw2 = b.conv(p + "pwconv2", inter, dim, 1, dim);
        bl.gamma = b.raw(p + "gamma", dim);
        h->blocks.push_back(bl);
    }
    h->fl_g = b.raw("backbone.final_layer_norm.weight", dim);
    h->fl_b = b.raw("backbone.final_layer_norm.bias", dim);
    // head.out: Linear(dim -> n_fft + 2), rows padded to V_SPEC_CP so the spectrum buffer is [re | im | 0]
    h->head = b.conv("head.out", dim, STFT_N + 2, 1, V_SPEC_CP);
    int32_t rc = b.rc;
    if (rc == 0) {
        h->stft = stft1024_append_tables(b.blob);
        hipError_t e = hipMalloc((void**)&h->dev, b.blob.size() * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(h->dev, b.blob.data(), b.blob.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void**)&h->dev16, b.blob16.size() * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMemcpy(h->dev16, b.blob16.data(), b.blob16.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_error("vocos_create: upload failed: %s", hipGetErrorString(e));
            rc = TTSAMD_EHIP;
        }
    }
    if (rc) {
        if (h->dev) (void)hipFree(h->dev);
        delete h;
        return rc;
    }
    *out = h;
    return 0;
}

int32_t vocos_set_padding(Vocos* h, int32_t mode) {
    TTS_REQUIRE(h && (mode == 0 || mode == 1), "vocos_set_padding: mode must be 0 (same) or 1 (center)");
    h->center = mode;
    return 0;
}

void vocos_destroy(Vocos* h) {
    if (!h) return;
    if (h->dev) (void)hipFree(h->dev);
    if (h->dev16) (void)hipFree(h->dev16);
    delete h;
}

// ISTFT head (pretrained.py:79-90, spectral_ops.py:47-75) in two launches + the overlap-add.
// 1. S[b][t][f] = clamp(exp(O[f][t]) - dn * bias[f], 0, 100) * (cos, sin)(O[513 + f][t]): the head's channel-first output [1026][T] read along t,
//    the complex spectrum written FRAME-major (f contiguous) through a 32 x 33 LDS tile, so that
// 2. one block per frame reads its 513 bins contiguously, builds conj(X) of the Hermitian extension (X[k] = S[k], X[1024 - k] = conj S[k]; the
//    imaginary parts of DC and Nyquist dropped as irfft does), runs ONE 1024-point FFT in LDS (fft1024.hpp) and writes Re / 1024 * window as
//    Y[b][t][k].  Rounds 1-5 ran the inverse DFT as a [1152 -> 1024] GEMM on the conv engine: 300 us per B = 32 call (40x the FLOPs).
// one 32 x 32 tile of row b: bins f0 ..., frames t0 ... of which those in [t_lo, t_hi) are computed and written, no other
// o_bs: batch stride of O in floats (V_SPEC_CP * T for the backbone's own buffer, 1026 * T for a caller's features)
__device__ __forceinline__ void vocos_spec_tile(const float* __restrict__ O, int64_t o_bs, const float* __restrict__ bias, float dn, int b, int f0,
                                                int t0, int t_lo, int t_hi, int T, float2* __restrict__ S) {
    __shared__ float2 tile[32][33];
    const bool sub = bias != nullptr && dn != 0.f;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;      // 32 x 8
    const float* ob = O + (int64_t)b * o_bs;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int f = f0 + ty + 8 * r, t = t0 + tx;
        float2 v = make_float2(0.f, 0.f);
        if (f < STFT_NBIN && t >= t_lo && t < t_hi) {
            const float lm = ob[(int64_t)f * T + t], ph = ob[(int64_t)(STFT_NBIN + f) * T + t];
            float mag = expf(lm);
            if (sub) mag -= dn * bias[f];
            mag = fminf(fmaxf(mag, 0.f), 100.f);
            v = make_float2(mag * cosf(ph), mag * sinf(ph));
        }
        tile[ty + 8 * r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int t = t0 + ty + 8 * r, f = f0 + tx;
        if (t >= t_lo && t < t_hi && f < STFT_NBIN) S[((int64_t)b * T + t) * STFT_NBIN + f] = tile[tx][ty + 8 * r];
    }
}

__global__ __launch_bounds__(256) void vocos_spec_t_kernel(const float* __restrict__ O, int64_t o_bs, const float* __restrict__ bias, float denoise,
                                                           const float* __restrict__ denoise_rows, const int64_t* __restrict__ lens, int T, float2* __restrict__ S) {
    const int b = blockIdx.z, f0 = blockIdx.y * 32, t0 = blockIdx.x * 32;
    const int len = lens ? min((int)lens[b], T) : T;
    if (t0 >= len) return;
    // the row's strength; the scalar entry passes bias = nullptr for 0, so a row at 0 takes the same (no) subtraction
    vocos_spec_tile(O, o_bs, bias, denoise_rows ? denoise_rows[b] : denoise, b, f0, t0, 0, len, T, S);
}

// frame t of row b: its 513 bins -> 1024 windowed samples, by the block's 256 threads
__device__ __forceinline__ void vocos_istft_frame(const float2* __restrict__ S, const float* __restrict__ win, const float2* __restrict__ tw_g,
                                                  int b, int t, int T, float* __restrict__ Y) {
    __shared__ float2 buf[2][STFT_N];
    __shared__ float2 tw[STFT_N];
    const int i = threadIdx.x;
    const float2* sb = S + ((int64_t)b * T + t) * STFT_NBIN;
    stft1024_load_twiddles(tw, tw_g, i);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = i + 256 * r;
        float2 x = sb[k <= STFT_N / 2 ? k : STFT_N - k];         // conj(X)[k]: conj S[k] below Nyquist, S[1024 - k] above
        if (k <= STFT_N / 2) x.y = -x.y;
        if (k == 0 || k == STFT_N / 2) x.y = 0.f;
        buf[0][k] = x;
    }
    __syncthreads();
    fft1024_stockham(buf[0], buf[1], tw, i);
    stft1024_store_inverse_frame(buf[1], win, Y + ((int64_t)b * T + t) * STFT_N, i);
}

__global__ __launch_bounds__(256) void vocos_istft_kernel(const float2* __restrict__ S, const int64_t* __restrict__ lens,
                                                          const float* __restrict__ win, const float2* __restrict__ tw_g, int T,
                                                          float* __restrict__ Y) {
    const int b = blockIdx.y, t = blockIdx.x;
    if (lens && t >= (int)lens[b]) return;                       // frames the overlap-add never reads
    vocos_istft_frame(S, win, tw_g, b, t, T, Y);
}

// ---- the head of one streaming step (ttsamd_vocos_forward_windows): the three launches above on the frames and samples a window's
// needed range can see.  Window w needs the samples of its frames [start[w], start[w] + len[w]) (host values, by value in the launch
// arguments); lens[w] is read on the device, where gather wrote it.  A sample of frame c is the overlap-add of the frames c - r_l ...
// c + 2 (r_l = 2 "same", 1 "center"; ttsamd.h), so spectrum and inverse FFT run on [start - r_l, start + len + 2) clipped to the window
// and the overlap-add, a block per frame of samples, reads no other frame and writes no other sample.
struct VocosWinTable {
    int32_t start[TTSAMD_STREAM_MAX_WINDOWS], len[TTSAMD_STREAM_MAX_WINDOWS];
};
__device__ __forceinline__ void vocos_window_frames(const VocosWinTable& tab, int w, int len, int r_l, int& f_lo, int& f_hi) {
    f_lo = max(tab.start[w] - r_l, 0);
    f_hi = min(tab.start[w] + tab.len[w] + 2, len);
}

__global__ __launch_bounds__(256) void vocos_spec_t_windows_kernel(const float* __restrict__ O, const float* __restrict__ bias,
                                                                   const float* __restrict__ denoise_rows, const int64_t* __restrict__ lens,
                                                                   const VocosWinTable tab, int r_l, int T, float2* __restrict__ S) {
    const int w = blockIdx.z, f0 = blockIdx.y * 32;
    int f_lo, f_hi;
    vocos_window_frames(tab, w, min((int)lens[w], T), r_l, f_lo, f_hi);
    const int t0 = (f_lo & ~31) + blockIdx.x * 32;
    if (t0 >= f_hi) return;
    vocos_spec_tile(O, (int64_t)V_SPEC_CP * T, bias, denoise_rows ? denoise_rows[w] : 0.f, w, f0, t0, f_lo, f_hi, T, S);
}

__global__ __launch_bounds__(256) void vocos_istft_windows_kernel(const float2* __restrict__ S, const int64_t* __restrict__ lens,
                                                                  const VocosWinTable tab, int r_l, const float* __restrict__ win,
                                                                  const float2* __restrict__ tw_g, int T, float* __restrict__ Y) {
    const int w = blockIdx.y;
    int f_lo, f_hi;
    vocos_window_frames(tab, w, min((int)lens[w], T), r_l, f_lo, f_hi);
    const int t = f_lo + blockIdx.x;
    if (t >= f_hi) return;
    vocos_istft_frame(S, win, tw_g, w, t, T, Y);
}

// overlap_add_kernel (denoiser.hip) for the samples of frame start[w] + blockIdx.x alone: the same stft1024_ola_sample, so the same bits
__global__ __launch_bounds__(256) void vocos_overlap_add_windows_kernel(const float* __restrict__ Y, const float* __restrict__ win,
                                                                        const int64_t* __restrict__ lens, const VocosWinTable tab, int pad,
                                                                        int T, float* __restrict__ wave) {
    const int w = blockIdx.y;
    if ((int)blockIdx.x >= tab.len[w]) return;
    const int fr = min((int)lens[w], T);
    const int m = (tab.start[w] + blockIdx.x) * STFT_HOP + threadIdx.x;
    const int n_out = (fr - 1) * STFT_HOP + STFT_N - 2 * pad;
    if (m >= n_out) return;
    wave[(int64_t)w * STFT_HOP * T + m] = stft1024_ola_sample(Y + (int64_t)w * STFT_N * T, win, m + pad, fr);
}

// bias_vec[f] = min(exp(O[f][0]), 100)   (pretrained.py:65-69)
__global__ void vocos_bias_kernel(const float* __restrict__ O, int T, float* __restrict__ out) {
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f < STFT_NBIN) out[f] = fminf(expf(O[(int64_t)f * T]), 100.f);
}

// mel [B][in_ch][T] -> [B][in_chp][T], the added channel rows zero (in_ch = 100: the embed conv reads 8-channel chunks)
__global__ __launch_bounds__(256) void vocos_pad_channels_kernel(const float* __restrict__ mel, int in_ch, int in_chp, int T,
                                                                 float* __restrict__ out) {
    const int b = blockIdx.y;
    const int64_t n = (int64_t)in_chp * T, n_in = (int64_t)in_ch * T;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256)
        out[b * n + e] = e < n_in ? mel[b * n_in + e] : 0.f;
}

struct VWs {
    float *x, *d, *h, *o, *y, *m;
};
static void vcarve(const Vocos* h, Arena& a, int B, int T, VWs& w) {
    w.m = h->in_chp != h->in_ch ? a.take<float>((int64_t)B * h->in_chp * T) : nullptr;      // staged mel (24k only)
    w.x = a.take<float>((int64_t)B * h->dim * T);
    w.d = a.take<float>((int64_t)B * h->dim * T);
    w.h = a.take<float>((int64_t)B * h->inter * T);
    w.o = a.take<float>((int64_t)B * V_SPEC_CP * T);
    w.y = a.take<float>((int64_t)B * STFT_N * T);
}
int64_t vocos_workspace_bytes(const Vocos* h, int32_t B, int32_t T) {
    Arena a(nullptr, 0);
    VWs w;
    vcarve(h, a, B, T, w);
    return a.off;
}

static int32_t vconv(const Vocos* h, const VConv& c, const float* x, float* y, const float* res, const float* scale,
                     const int64_t* lens, int B, int T, int act, hipStream_t s) {
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.x_bs = (int64_t)c.cin * T; p.x_cs = T;
    p.w = h->dev + c.w_off; p.bias = h->dev + c.b_off;
    p.w_bf16 = h->dev16 + c.w16_off; p.precision = default_precision();
    p.y = y; p.y_bs = (int64_t)c.coutp * T; p.y_cs = T; p.y_ts = 1;
    p.res = res; p.r_bs = (int64_t)c.coutp * T; p.r_cs = T;
    p.scale = scale;
    p.lens_in = lens; p.lens_out = lens; p.len_in_mul = 1; p.len_out_mul = 1;
    p.Lin = T; p.Nout = T; p.Cin = c.cin; p.Cout = c.coutp; p.CoutP = c.coutp; p.K = c.k;
    p.dil = 1; p.pad = c.k / 2; p.n_phase = 1; p.in_slope = 1.f; p.relu_out = act; p.mode = 0; p.div = 1.f; p.batch = B;
    prof_begin(s, 2.0 * c.cout * c.cin * c.k);
    const int32_t rc = launch_conv(p, s);
    prof_end(s);
    return rc;
}

// backbone + head.out -> w.o [B][V_SPEC_CP][T] holding (log-magnitude | phase | 0); mel [B][in_chp][T]
static int32_t vocos_features(const Vocos* h, const float* mel, const int64_t* lens, int B, int T, const VWs& w,
                              hipStream_t s) {
    const int d = h->dim;
    TTS_TRY(vconv(h, h->embed, mel, w.x, nullptr, nullptr, lens, B, T, 0, s));
    TTS_TRY(launch_layernorm_cf(w.x, w.x, h->dev + h->n0_g, h->dev + h->n0_b, nullptr, 0, B, d, T, s, 1e-6f));
    for (const VBlock& bl : h->blocks) {
        TTS_TRY(launch_dwconv7(w.x, h->dev + bl.dw_w, h->dev + bl.dw_b, lens, B, d, T, w.d, s));
        TTS_TRY(launch_layernorm_cf(w.d, w.d, h->dev + bl.ln_g, h->dev + bl.ln_b, nullptr, 0, B, d, T, s, 1e-6f));
        TTS_TRY(vconv(h, bl.pw1, w.d, w.h, nullptr, nullptr, lens, B, T, 2, s));                   // + GELU
        TTS_TRY(vconv(h, bl.pw2, w.h, w.x, w.x, h->dev + bl.gamma, lens, B, T, 0, s));             // gamma*() + residual
    }
    TTS_TRY(launch_layernorm_cf(w.x, w.d, h->dev + h->fl_g, h->dev + h->fl_b, nullptr, 0, B, d, T, s, 1e-6f));
    return vconv(h, h->head, w.d, w.o, nullptr, nullptr, lens, B, T, 0, s);
}

int32_t vocos_bias_vec(const Vocos* h, float* out513, void* ws, int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(h && out513, "vocos_bias_vec: null argument");
    const int T = 88;   // pretrained.py:61
    Arena a(ws, ws_bytes);
    VWs w;
    vcarve(h, a, 1, T, w);
    float* zero_mel = a.take<float>((int64_t)h->in_chp * T);
    if (!ws || !a.ok) {
        set_error("vocos_bias_vec: workspace of %lld bytes needed, %lld given", (long long)a.off, (long long)ws_bytes);
        return TTSAMD_ENOMEM;
    }
    TTS_CHECK_HIP(hipMemsetAsync(zero_mel, 0, (size_t)h->in_chp * T * sizeof(float), s));
    TTS_TRY(vocos_features(h, zero_mel, nullptr, 1, T, w, s));
    hipLaunchKernelGGL(vocos_bias_kernel, dim3((STFT_NBIN + 63) / 64), dim3(64), 0, s, w.o, T, out513);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

int64_t vocos_bias_workspace_bytes(const Vocos* h) {
    Arena a(nullptr, 0);
    VWs w;
    vcarve(h, a, 1, 88, w);
    a.take<float>((int64_t)h->in_chp * 88);
    return a.off;
}

// the channel padding of '24k', then backbone + head.out
static int32_t vocos_padded_features(const Vocos* h, const float* mel, const int64_t* lens, int B, int T, const VWs& w, hipStream_t s) {
    if (w.m) {
        hipLaunchKernelGGL(vocos_pad_channels_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)h->in_chp * T + 255) / 256, 1024), B),
                           dim3(256), 0, s, mel, h->in_ch, h->in_chp, T, w.m);
        TTS_CHECK_HIP(hipGetLastError());
        mel = w.m;
    }
    return vocos_features(h, mel, lens, B, T, w, s);
}

// the ISTFT head on O [B][>= 1026 rows][T] with batch stride o_bs: spectrum -> inverse FFT -> overlap-add
static int32_t vocos_head_run(const Vocos* h, const float* O, int64_t o_bs, const int64_t* lens, int B, int T, float denoise,
                              const float* denoise_rows, const float* bias_vec, float* wave, const VWs& w, hipStream_t s) {
    float2* S = reinterpret_cast<float2*>(w.h);
    hipLaunchKernelGGL(vocos_spec_t_kernel, dim3((T + 31) / 32, (STFT_NBIN + 31) / 32, B), dim3(256), 0, s, O, o_bs,
                       (denoise != 0.f || denoise_rows) ? bias_vec : nullptr, denoise, denoise_rows, lens, T, S);
    hipLaunchKernelGGL(vocos_istft_kernel, dim3(T, B), dim3(256), 0, s, S, lens, h->dev + h->stft.window,
                       reinterpret_cast<const float2*>(h->dev + h->stft.twiddle), T, w.y);
    TTS_CHECK_HIP(hipGetLastError());
    // "center" (24k): torch.istft(center=True) trimming, pad = n_fft / 2, n_out = hop * (frames - 1) per utterance; rows keep the stride hop * T
    if (h->center)
        return launch_overlap_add(w.y, h->dev + h->stft.window, lens, stft1024_pad(1), B, T, STFT_HOP * (T - 1), wave, (int64_t)STFT_HOP * T, s);
    // overlap-add with "same" trimming (pad = (n_fft - hop) / 2, n_out = hop * frames) over the frame-major time-domain frames
    return launch_overlap_add(w.y, h->dev + h->stft.window, lens, stft1024_pad(0), B, T, STFT_HOP * T, wave, (int64_t)STFT_HOP * T, s);
}

// denoise_rows: device [B] in place of the scalar (ttsamd_vocos_forward_rows), nullptr: the scalar (ttsamd_vocos_forward)
int32_t vocos_forward(const Vocos* h, const float* mel, const int64_t* lens, int32_t B, int32_t T, float denoise,
                      const float* denoise_rows, const float* bias_vec, float* wave, void* ws, int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(h && mel && wave && lens && B >= 1 && T >= 1, "vocos_forward: bad argument");
    TTS_REQUIRE((denoise == 0.f && !denoise_rows) || bias_vec, "vocos_forward: denoise > 0 needs bias_vec");
    if (h->center && T == 1) return 0;       // the centred ISTFT of one frame has no sample left after trimming n_fft / 2 per side
    Arena a(ws, ws_bytes);
    VWs w;
    vcarve(h, a, B, T, w);
    if (!ws || !a.ok) {
        set_error("vocos_forward: workspace of %lld bytes needed, %lld given", (long long)a.off, (long long)ws_bytes);
        return TTSAMD_ENOMEM;
    }
    // complex spectrum frame-major into the (dead) hidden buffer of the backbone: 513 float2 per frame <= inter floats
    TTS_REQUIRE(2 * STFT_NBIN <= h->inter, "vocos_forward: the spectrum does not fit the hidden buffer (inter %d)", h->inter);
    TTS_TRY(vocos_padded_features(h, mel, lens, B, T, w, s));
    return vocos_head_run(h, w.o, (int64_t)V_SPEC_CP * T, lens, B, T, denoise, denoise_rows, bias_vec, wave, w, s);
}

// rows f < 1026 of the backbone's [B][V_SPEC_CP][T] buffer -> a caller's [B][1026][T]; frames t >= lens[b], which no conv writes, as zero
__global__ __launch_bounds__(256) void vocos_copy_features_kernel(const float* __restrict__ O, const int64_t* __restrict__ lens, int T,
                                                                  float* __restrict__ out) {
    const int b = blockIdx.y;
    const int len = min((int)lens[b], T);
    const int64_t n = (int64_t)(STFT_N + 2) * T;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256)
        out[b * n + e] = (int)(e % T) < len ? O[(int64_t)b * V_SPEC_CP * T + e] : 0.f;
}

// backbone + head.out alone (ttsamd_vocos_features): the launches of vocos_forward up to the spectrum, then the copy above
int32_t vocos_features_out(const Vocos* h, const float* mel, const int64_t* lens, int32_t B, int32_t T, float* out, void* ws,
                           int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(h && mel && out && lens && B >= 1 && T >= 1, "vocos_features: bad argument");
    Arena a(ws, ws_bytes);
    VWs w;
    vcarve(h, a, B, T, w);
    if (!ws || !a.ok) {
        set_error("vocos_features: workspace of %lld bytes needed, %lld given", (long long)a.off, (long long)ws_bytes);
        return TTSAMD_ENOMEM;
    }
    TTS_TRY(vocos_padded_features(h, mel, lens, B, T, w, s));
    hipLaunchKernelGGL(vocos_copy_features_kernel, dim3((unsigned)std::min<int64_t>(((int64_t)(STFT_N + 2) * T + 255) / 256, 1024), B),
                       dim3(256), 0, s, w.o, lens, T, out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// spectrum, inverse FFT and overlap-add alone (ttsamd_vocos_head) on a caller's [B][1026][T]: the launches of vocos_forward behind head.out
int32_t vocos_head(const Vocos* h, const float* feats, const int64_t* lens, int32_t B, int32_t T, const float* denoise_rows,
                   const float* bias_vec, float* wave, void* ws, int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(h && feats && wave && lens && B >= 1 && T >= 1, "vocos_head: bad argument");
    TTS_REQUIRE(!denoise_rows || bias_vec, "vocos_head: denoise_rows needs bias_vec");
    if (h->center && T == 1) return 0;       // as vocos_forward: no sample left
    Arena a(ws, ws_bytes);
    VWs w;
    vcarve(h, a, B, T, w);
    if (!ws || !a.ok) {
        set_error("vocos_head: workspace of %lld bytes needed, %lld given", (long long)a.off, (long long)ws_bytes);
        return TTSAMD_ENOMEM;
    }
    TTS_REQUIRE(2 * STFT_NBIN <= h->inter, "vocos_head: the spectrum does not fit the hidden buffer (inter %d)", h->inter);
    return vocos_head_run(h, feats, (int64_t)(STFT_N + 2) * T, lens, B, T, 0.f, denoise_rows, bias_vec, wave, w, s);
}

// 3 (embed, k = 7) + 3 per ConvNeXt block (depthwise k = 7; LayerNorm, the pointwise convs and head.out are per frame), then the ISTFT's
// reach in frames (ttsamd.h)
int32_t vocos_halo_frames(const Vocos* h, int32_t* left, int32_t* right) {
    TTS_REQUIRE(h && left && right, "vocos_halo_frames: null argument");
    const int32_t reach = 3 + 3 * (int32_t)h->blocks.size();
    *left = reach + (h->center ? 1 : 2);
    *right = reach + 2;
    return 0;
}

int32_t vocos_forward_windows(const Vocos* h, const float* mel, const int64_t* lens, int32_t W, int32_t T, const int32_t* need_start,
                              const int32_t* need_len, const float* denoise_rows, const float* bias_vec, float* wave, void* ws,
                              int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(h && mel && lens && wave && need_start && need_len, "vocos_forward_windows: null argument");
    TTS_REQUIRE(W >= 1 && W <= TTSAMD_STREAM_MAX_WINDOWS, "vocos_forward_windows: %d windows (1 .. %d)", W, TTSAMD_STREAM_MAX_WINDOWS);
    TTS_REQUIRE(T >= 1 && (int64_t)STFT_N * T * W < (1ll << 31), "vocos_forward_windows: bad w_max %d", T);
    TTS_REQUIRE(!denoise_rows || bias_vec, "vocos_forward_windows: denoise_rows needs bias_vec");
    TTS_REQUIRE(2 * STFT_NBIN <= h->inter, "vocos_forward_windows: the spectrum does not fit the hidden buffer (inter %d)", h->inter);
    VocosWinTable tab = {};
    int max_len = 0;
    for (int w = 0; w < W; ++w) {
        TTS_REQUIRE(need_start[w] >= 0 && need_len[w] >= 1 && (int64_t)need_start[w] + need_len[w] <= T,
                    "vocos_forward_windows: window %d: needed frames [%d, %d + %d) outside [0, w_max = %d)", w, need_start[w], need_start[w],
                    need_len[w], T);
        tab.start[w] = need_start[w]; tab.len[w] = need_len[w];
        max_len = std::max(max_len, (int)need_len[w]);
    }
    Arena a(ws, ws_bytes);
    VWs v;
    vcarve(h, a, W, T, v);
    if (!ws || !a.ok) {
        set_error("vocos_forward_windows: workspace of %lld bytes needed, %lld given", (long long)a.off, (long long)ws_bytes);
        return TTSAMD_ENOMEM;
    }
    if (h->center && T == 1) return 0;       // as vocos_forward: no sample left
    TTS_TRY(vocos_padded_features(h, mel, lens, W, T, v, s));
    float2* S = reinterpret_cast<float2*>(v.h);
    const int r_l = h->center ? 1 : 2, n_frames = std::min(max_len + r_l + 2, (int)T);
    // the tiles start at the 32-frame boundary at or below a window's first frame
    hipLaunchKernelGGL(vocos_spec_t_windows_kernel, dim3((n_frames + 31 + 31) / 32, (STFT_NBIN + 31) / 32, W), dim3(256), 0, s, v.o,
                       denoise_rows ? bias_vec : nullptr, denoise_rows, lens, tab, r_l, T, S);
    hipLaunchKernelGGL(vocos_istft_windows_kernel, dim3(n_frames, W), dim3(256), 0, s, S, lens, tab, r_l, h->dev + h->stft.window,
                       reinterpret_cast<const float2*>(h->dev + h->stft.twiddle), T, v.y);
    hipLaunchKernelGGL(vocos_overlap_add_windows_kernel, dim3(max_len, W), dim3(256), 0, s, v.y, h->dev + h->stft.window, lens, tab,
                       stft1024_pad(h->center), T, wave);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
