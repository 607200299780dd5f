// FastPitch forced alignment on the device: replaces the aligner path of the reference's FastPitch.forward
// (models/fastpitch/fastpitch/model.py:298-318,331-332): ConvAttention.forward (attention.py:174-223), binarize_attention with
// mas_width1 (alignment.py:46-72) and average_pitch (model.py:93-111).
//
//   encoders        keys  word_emb(ids) -> [B][d_text][L] -> conv k = 3 (d_text -> 2 d_text) + ReLU -> 1 x 1 (-> n_att)
//                   queries mel [B][n_mel][T] -> conv k = 3 (n_mel -> 2 n_mel) + ReLU -> 1 x 1 (-> n_mel) + ReLU -> 1 x 1 (-> n_att)
//                   over the padded batch without masks, as the reference runs them.  The hidden layers run on the fp32 MFMA conv engine
//                   (conv_mfma.hip; output channels padded to its 32-row tiles with zero weights).  The LAST 1 x 1 conv of each encoder is a
//                   plain kernel that accumulates in float64 and leaves q and k in float64: the logit multiplies differences of values of
//                   order 50 by each other, and q, k merely ROUNDED to fp32 already put attn_soft 2.4 - 3.3 x the reference's own
//                   fp32-vs-float64 distance away from float64 (an fp32 MFMA projection: 7.4 x, measured); this way it is about 1.5 x.
//   attention       one block per (utterance, 8 frames): logit = -0.0005 sum_c (q - k)^2 summed directly in channel order (float64, rounded
//                   once), key tiles of 32 tokens through LDS, the 8 x L logits of the block in LDS; [log-softmax over the padded L +
//                   log(prior + 1e-8)]; the value before masking is attn_logprob; tokens >= in_lens[b] masked, softmax (fp32).
//   mas             mas_width1 bit for bit, one block per utterance.  Lane `l` of wave `w` owns tokens 256 w + 64 r + l (r = 0 .. 3): a row's
//                   loads are coalesced and the ballot of decision r IS word 4 w + r of the row's plain bit mask.  A row is one fp32 max and
//                   one fp32 add per cell in the reference's order; log_p of the previous row lives in registers and nowhere else; the
//                   input is loaded eight rows ahead (a row's arithmetic is a fraction of a memory latency).  The left
//                   neighbour comes by a cross-lane move, across waves through one double-buffered LDS word per wave (one barrier per row;
//                   none with a single wave, L <= 256).  The decisions `log_p[i-1][j-1] >= log_p[i-1][j]` are kept at one bit per cell, in
//                   LDS when they fit and in the workspace otherwise.  The backtrack stages 64 rows' words at a time and walks them from LDS.
//                   L == 1: the reference indexes log_p[i-1][-1] there (Python wraps it to the same column; out of bounds in C); defined here
//                   as every frame assigned to token 0.
//   average_pitch   per token the mean of the non-zero values of its frame segment, the segment summed directly (float64, rounded once)
//                   instead of as the difference of two fp32 cumulative sums; bounds = cumsum(durs).long() as the reference takes them.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "kernels.hpp"

#pragma clang fp contract(off)

namespace ttsamd {

constexpr int AL_TQ = 8, AL_TK = 32, AL_MAXC = 96;               // attention: frames per block, tokens per key tile, most channels
constexpr int AL_MAX_L = TTSAMD_MAS_MAX_TOKENS;                  // attention: tokens per row (8 x L logits + a float64 key tile: 62 KB of LDS at most)
constexpr int AL_PCO = 8;                                        // float64 projection: output channels per thread
constexpr int MAS_MAX_L = TTSAMD_MAS_MAX_TOKENS;                 // 4 waves x 64 lanes x 4 tokens
constexpr int MAS_LDS_WORDS = 5120;                              // 40 KB of decision bits in LDS (64-bit words); more goes to the workspace
constexpr int MAS_WIN = 64;                                      // backtrack: rows staged per window
constexpr int MAS_PF = 8;                                        // forward: rows in flight per lane (4 values each)

struct AConv {
    int64_t w_off = 0, b_off = -1;
    int cin = 0, cout = 0, coutp = 0, k = 0;
};
struct Aligner {
    float* dev = nullptr;
    int n_mel = 80, d_text = 384, n_att = 80, n_symbols = 0, padding_idx = 0;
    int64_t emb = 0;
    AConv k1, q1, q2;                                            // hidden layers on the conv engine
    int64_t k2_w = 0, k2_b = 0, q3_w = 0, q3_b = 0;              // the last 1 x 1 convs as stored, [n_att][cin] (aligner_proj64_kernel)
};

namespace {
using ATensorMap = std::map<std::string, const ttsamd_tensor*>;

int64_t anumel(const ttsamd_tensor* t) {
    int64_t n = 1;
    for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
    return n;
}

struct ABuilder {
    const ATensorMap& tm;
    std::vector<float> blob;
    int32_t rc = 0;
    explicit ABuilder(const ATensorMap& t) : tm(t) {}
    const ttsamd_tensor* get(const std::string& name, int64_t n) {
        if (rc) return nullptr;
        auto it = tm.find(name);
        if (it == tm.end() || anumel(it->second) != n) {
            set_error("aligner: missing or mis-sized tensor '%s' (expected %lld elements)", name.c_str(), (long long)n);
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
    // stored weight [cout][cin_w][k] -> the engine's packing with cin >= cin_w input channels and coutp >= cout rows, the added ones zero
    AConv conv(const std::string& base, int cin, int cin_w, int cout, int k) {
        AConv c;
        c.cin = cin; c.cout = cout; c.k = k; c.coutp = cout_padded(cout);
        const ttsamd_tensor* w = get(base + ".weight", (int64_t)cin_w * cout * k);
        if (!w) return c;
        std::vector<float> wp((size_t)c.coutp * cin * k, 0.f);
        for (int co = 0; co < cout; ++co)
            std::memcpy(wp.data() + (size_t)co * cin * k, w->data + (size_t)co * cin_w * k, (size_t)cin_w * k * sizeof(float));
        c.w_off = (int64_t)blob.size();
        blob.resize(blob.size() + (size_t)cin * k * c.coutp);
        pack_conv_weight(wp.data(), c.coutp, cin, k, blob.data() + c.w_off);
        blob.resize(align_up((int64_t)blob.size(), 64));
        c.b_off = raw(base + ".bias", cout, c.coutp);
        return c;
    }
};
}  // namespace

int32_t aligner_create(const ttsamd_tensor* weights, int32_t n, const ttsamd_aligner_cfg* cfg, Aligner** out) {
    TTS_REQUIRE(weights && cfg && out && n >= 1, "aligner_create: null argument");
    TTS_REQUIRE(cfg->n_mel >= 8 && cfg->n_mel % 8 == 0 && cfg->d_text >= 8 && cfg->d_text % 16 == 0,
                "aligner_create: n_mel = %d / d_text = %d (multiples of 8 / 16: the conv engine's input chunks)", cfg->n_mel, cfg->d_text);
    TTS_REQUIRE(cfg->n_att >= 1 && cfg->n_att <= AL_MAXC, "aligner_create: n_att = %d outside [1, %d]", cfg->n_att, AL_MAXC);
    TTS_REQUIRE(cfg->n_symbols >= 1 && cfg->padding_idx >= 0 && cfg->padding_idx < cfg->n_symbols, "aligner_create: n_symbols = %d, padding_idx = %d",
                cfg->n_symbols, cfg->padding_idx);
    ATensorMap tm;
    for (int i = 0; i < n; ++i) tm[weights[i].name] = &weights[i];
    ABuilder b(tm);
    auto* h = new Aligner();
    h->n_mel = cfg->n_mel; h->d_text = cfg->d_text; h->n_att = cfg->n_att; h->n_symbols = cfg->n_symbols; h->padding_idx = cfg->padding_idx;
    h->emb = b.raw("encoder.word_emb.weight", (int64_t)cfg->n_symbols * cfg->d_text);
    // nn.Sequential indices of ConvAttention (attention.py:100-132): key_proj 0, 2; query_proj 0, 2, 4; each a ConvNorm holding `.conv`
    h->k1 = b.conv("attention.key_proj.0.conv", cfg->d_text, cfg->d_text, 2 * cfg->d_text, 3);
    h->k2_w = b.raw("attention.key_proj.2.conv.weight", (int64_t)cfg->n_att * 2 * cfg->d_text);
    h->k2_b = b.raw("attention.key_proj.2.conv.bias", cfg->n_att);
    h->q1 = b.conv("attention.query_proj.0.conv", cfg->n_mel, cfg->n_mel, 2 * cfg->n_mel, 3);
    h->q2 = b.conv("attention.query_proj.2.conv", h->q1.coutp, 2 * cfg->n_mel, cfg->n_mel, 1);
    h->q3_w = b.raw("attention.query_proj.4.conv.weight", (int64_t)cfg->n_att * cfg->n_mel);
    h->q3_b = b.raw("attention.query_proj.4.conv.bias", cfg->n_att);
    int32_t rc = b.rc;
    if (rc == 0) {
        hipError_t e = hipMalloc((void**)&h->dev, b.blob.size() * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(h->dev, b.blob.data(), b.blob.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_error("aligner_create: upload failed: %s", hipGetErrorString(e));
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

void aligner_destroy(Aligner* h) {
    if (!h) return;
    if (h->dev) (void)hipFree(h->dev);
    delete h;
}

// ------------------------------------------------------------------------------------------------------------------- key embedding ----
// x[b][c][l] = word_emb[ids[b][l]][c] (encoder.word_emb(inputs).permute(0, 2, 1), model.py:299,307); ids outside the table are clamped
__global__ __launch_bounds__(256) void aligner_embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ emb, int n_symbols,
                                                            int C, int L, float* __restrict__ x) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, c0 = blockIdx.y * 32, l0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int l = l0 + ty + 8 * r, c = c0 + tx;
        float v = 0.f;
        if (l < L && c < C) {
            const int64_t id = min(max(ids[(int64_t)b * L + l], (int64_t)0), (int64_t)n_symbols - 1);
            v = emb[id * C + c];
        }
        tile[ty + 8 * r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int c = c0 + ty + 8 * r, l = l0 + tx;
        if (c < C && l < L) x[((int64_t)b * C + c) * L + l] = tile[tx][ty + 8 * r];
    }
}

// ----------------------------------------------------------------------------------------------------------------------- attention ----
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

// The last 1 x 1 conv of an encoder in float64: y[b][co][s] = bias[co] + sum_ci w[co][ci] x[b][ci][s]; x fp32 [B][x_rows][S] (the first cin rows
// are read), w fp32 [cout][cin] as stored, y float64 [B][cout][S].  One wave per (64 positions, AL_PCO output channels): x loads are coalesced,
// the weights are block-uniform (scalar loads).
__global__ __launch_bounds__(64) void aligner_proj64_kernel(const float* __restrict__ x, int x_rows, const float* __restrict__ w,
                                                            const float* __restrict__ bias, int cin, int cout, int S,
                                                            double* __restrict__ y) {
    const int b = blockIdx.z, co0 = blockIdx.y * AL_PCO, sp = blockIdx.x * 64 + threadIdx.x;
    const bool live = sp < S;
    const float* xb = x + (int64_t)b * x_rows * S + (live ? sp : 0);
    double acc[AL_PCO];
#pragma unroll
    for (int j = 0; j < AL_PCO; ++j) acc[j] = 0.0;
    int ci = 0;
    for (; ci + 8 <= cin; ci += 8) {                             // eight loads in flight: one per step ran at a memory latency per channel
        float xv[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) xv[u] = xb[(int64_t)(ci + u) * S];
#pragma unroll
        for (int u = 0; u < 8; ++u)
#pragma unroll
            for (int j = 0; j < AL_PCO; ++j) {
                const int co = min(co0 + j, cout - 1);
                acc[j] += (double)w[(int64_t)co * cin + ci + u] * (double)xv[u];
            }
    }
    for (; ci < cin; ++ci) {
        const double xv = (double)xb[(int64_t)ci * S];
#pragma unroll
        for (int j = 0; j < AL_PCO; ++j) {
            const int co = min(co0 + j, cout - 1);
            acc[j] += (double)w[(int64_t)co * cin + ci] * xv;
        }
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < AL_PCO; ++j)
            if (co0 + j < cout) y[((int64_t)b * cout + co0 + j) * S + sp] = acc[j] + (double)bias[co0 + j];
    }
}

// q [B][C][T], k [B][C][L] float64.  Dynamic LDS: AL_TQ * L logits.
__global__ __launch_bounds__(256) void aligner_attention_kernel(const double* __restrict__ q, const double* __restrict__ k,
                                                                const int64_t* __restrict__ in_lens, const float* __restrict__ prior, int C,
                                                                int T, int L, float* __restrict__ soft, float* __restrict__ logprob) {
    extern __shared__ float lg[];                                // [AL_TQ][L]
    __shared__ double qs[AL_MAXC][AL_TQ];
    __shared__ double ks[AL_MAXC][AL_TK];
    const int b = blockIdx.y, t0 = blockIdx.x * AL_TQ, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int kl = tid & (AL_TK - 1), fr = tid / AL_TK;          // this thread's token of the key tile and its frame of the block
    const double* qb = q + (int64_t)b * C * T;
    const double* kb = k + (int64_t)b * C * L;
    for (int idx = tid; idx < C * AL_TQ; idx += 256) {
        const int c = idx / AL_TQ, tt = idx % AL_TQ;
        qs[c][tt] = t0 + tt < T ? qb[(int64_t)c * T + t0 + tt] : 0.0;
    }
    for (int l0 = 0; l0 < L; l0 += AL_TK) {
        __syncthreads();                                         // (first pass: qs written; later: the previous tile's readers are done)
        for (int idx = tid; idx < C * AL_TK; idx += 256) {
            const int c = idx / AL_TK, ll = idx % AL_TK;
            ks[c][ll] = l0 + ll < L ? kb[(int64_t)c * L + l0 + ll] : 0.0;
        }
        __syncthreads();
        double s0 = 0.0;
        for (int c = 0; c < C; ++c) {
            const double d0 = qs[c][fr] - ks[c][kl];
            s0 += d0 * d0;
        }
        if (l0 + kl < L) lg[fr * L + l0 + kl] = (float)(-0.0005 * s0);
    }
    __syncthreads();
    const int n_in = (int)max((int64_t)0, min(in_lens[b], (int64_t)L));
#pragma unroll
    for (int rr = 0; rr < 2; ++rr) {                             // a wave per row: rows wv and wv + 4
        const int tt = wv + 4 * rr, t = t0 + tt;
        if (t >= T) continue;                                    // (wave-uniform)
        float* row = lg + tt * L;
        const int64_t o = ((int64_t)b * T + t) * L;
        if (prior) {                                             // log_softmax over the padded L, + log(prior + 1e-8)
            float m = -INFINITY;
            for (int l = lane; l < L; l += 64) m = fmaxf(m, row[l]);
            m = wave_max(m);
            float s = 0.f;
            for (int l = lane; l < L; l += 64) s = s + expf(row[l] - m);
            const float ls = logf(wave_sum(s));
            for (int l = lane; l < L; l += 64) row[l] = ((row[l] - m) - ls) + logf(prior[o + l] + 1e-8f);
        }
        float m = -INFINITY;
        for (int l = lane; l < L; l += 64) {
            const float v = row[l];
            logprob[o + l] = v;
            if (l < n_in) m = fmaxf(m, v);
        }
        m = wave_max(m);
        float s = 0.f;
        for (int l = lane; l < n_in; l += 64) s = s + expf(row[l] - m);
        s = wave_sum(s);
        for (int l = lane; l < L; l += 64) soft[o + l] = l < n_in ? expf(row[l] - m) / s : 0.f;
    }
}

struct AWs {
    float *kx, *kh, *qh1, *qh2;
    double *ke, *qe;
};
static void acarve(const Aligner* h, Arena& a, int B, int L, int T, AWs& w) {
    w.kx = a.take<float>((int64_t)B * h->d_text * L);
    w.kh = a.take<float>((int64_t)B * h->k1.coutp * L);
    w.ke = a.take<double>((int64_t)B * h->n_att * L);
    w.qh1 = a.take<float>((int64_t)B * h->q1.coutp * T);
    w.qh2 = a.take<float>((int64_t)B * h->q2.coutp * T);
    w.qe = a.take<double>((int64_t)B * h->n_att * T);
}
int64_t aligner_workspace_bytes(const Aligner* h, int32_t B, int32_t L, int32_t T) {
    Arena a(nullptr, 0);
    AWs w;
    acarve(h, a, B, L, T, w);
    return a.off;
}

// x [B][>= c.cin][S] with batch stride x_rows * S -> y [B][c.coutp][S]; no masks: the reference convolves the padded batch as it is
static int32_t aconv(const Aligner* h, const AConv& c, const float* x, int x_rows, float* y, int B, int S, int relu, hipStream_t s) {
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.x_bs = (int64_t)x_rows * S; p.x_cs = S;
    p.w = h->dev + c.w_off; p.bias = h->dev + c.b_off;
    p.precision = 0;                                             // the aligner is fp32 whatever ttsamd_set_precision says
    p.y = y; p.y_bs = (int64_t)c.coutp * S; p.y_cs = S; p.y_ts = 1;
    p.len_in_mul = 1; p.len_out_mul = 1;
    p.Lin = S; p.Nout = S; p.Cin = c.cin; p.Cout = c.coutp; p.CoutP = c.coutp; p.K = c.k;
    p.dil = 1; p.pad = c.k / 2; p.n_phase = 1; p.in_slope = 1.f; p.relu_out = relu; p.mode = 0; p.div = 1.f; p.batch = B;
    return launch_conv(p, s);
}

int32_t aligner_forward(const Aligner* h, const int64_t* ids, const int64_t* in_lens, const float* mel, const int64_t* mel_lens,
                        const float* prior, int32_t B, int32_t L, int32_t T, float* soft, float* logprob, void* ws, int64_t ws_bytes,
                        hipStream_t s) {
    (void)mel_lens;                                              // rows t >= mel_lens[b] are computed like the others (attention.py never masks them)
    TTS_REQUIRE(h && ids && in_lens && mel && soft && logprob, "aligner_forward: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && L >= 1 && T >= 1, "aligner_forward: bad batch %d / tokens %d / frames %d", B, L, T);
    TTS_REQUIRE(L <= AL_MAX_L, "aligner_forward: %d tokens, at most %d are built", L, AL_MAX_L);
    TTS_REQUIRE((int64_t)B * T * L < ((int64_t)1 << 40), "aligner_forward: attention of %d x %d x %d cells", B, T, L);
    Arena a(ws, ws_bytes);
    AWs w;
    acarve(h, a, B, L, T, w);
    if (!ws || !a.ok) {
        set_error("aligner_forward: workspace of %lld bytes needed, %lld given (ttsamd_aligner_workspace_bytes)", (long long)a.off,
                  (long long)ws_bytes);
        return TTSAMD_ENOMEM;
    }
    hipLaunchKernelGGL(aligner_embed_kernel, dim3((L + 31) / 32, (h->d_text + 31) / 32, B), dim3(256), 0, s, ids, h->dev + h->emb,
                       h->n_symbols, h->d_text, L, w.kx);
    TTS_CHECK_HIP(hipGetLastError());
    TTS_TRY(aconv(h, h->k1, w.kx, h->d_text, w.kh, B, L, 1, s));
    hipLaunchKernelGGL(aligner_proj64_kernel, dim3((L + 63) / 64, (h->n_att + AL_PCO - 1) / AL_PCO, B), dim3(64), 0, s, w.kh, h->k1.coutp,
                       h->dev + h->k2_w, h->dev + h->k2_b, 2 * h->d_text, h->n_att, L, w.ke);
    TTS_CHECK_HIP(hipGetLastError());
    TTS_TRY(aconv(h, h->q1, mel, h->n_mel, w.qh1, B, T, 1, s));
    TTS_TRY(aconv(h, h->q2, w.qh1, h->q1.coutp, w.qh2, B, T, 1, s));
    hipLaunchKernelGGL(aligner_proj64_kernel, dim3((T + 63) / 64, (h->n_att + AL_PCO - 1) / AL_PCO, B), dim3(64), 0, s, w.qh2, h->q2.coutp,
                       h->dev + h->q3_w, h->dev + h->q3_b, h->n_mel, h->n_att, T, w.qe);
    hipLaunchKernelGGL(aligner_attention_kernel, dim3((T + AL_TQ - 1) / AL_TQ, B), dim3(256), (size_t)AL_TQ * L * sizeof(float), s, w.qe, w.ke,
                       in_lens, prior, h->n_att, T, L, soft, logprob);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// ----------------------------------------------------------------------------------------------------------------------------- MAS ----
static int mas_waves(int L) { return std::max(1, (L + 255) / 256); }
static bool mas_bits_in_lds(int T, int L) { return (int64_t)T * 4 * mas_waves(L) <= MAS_LDS_WORDS; }

int64_t mas_workspace_bytes(int32_t B, int32_t T, int32_t L) {
    if (B < 1 || T < 0 || L < 0 || L > MAS_MAX_L) return -1;
    if (T == 0 || L == 0 || mas_bits_in_lds(T, L)) return 0;
    return (int64_t)B * T * 4 * mas_waves(L) * 8;
}

__global__ __launch_bounds__(256) void mas_kernel(const float* __restrict__ attn, int is_log, const int64_t* __restrict__ in_lens,
                                                  const int64_t* __restrict__ out_lens, int T, int L, int bits_lds,
                                                  float* __restrict__ dur, float* __restrict__ hard, unsigned long long* ws) {
    __shared__ unsigned long long lbits[MAS_LDS_WORDS];
    __shared__ unsigned long long win[MAS_WIN][2];
    __shared__ float edge[2][4];
    __shared__ int cnt[MAS_MAX_L];
    __shared__ int col[MAS_WIN];
    __shared__ int st[2];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, nw = blockDim.x >> 6, LW = 4 * nw;
    const int n_in = (int)max((int64_t)0, min(in_lens[b], (int64_t)L)), n_out = (int)max((int64_t)0, min(out_lens[b], (int64_t)T));
    float* db = dur + (int64_t)b * L;
    float* hb = hard ? hard + (int64_t)b * T * L : nullptr;
    if (n_in == 0 || n_out == 0) {
        for (int l = tid; l < L; l += blockDim.x) db[l] = 0.f;
        if (hb)
            for (int64_t e = tid; e < (int64_t)T * L; e += blockDim.x) hb[e] = 0.f;
        return;
    }
    // generic pointer: the block's decision bits, row i at bits[i * LW .. ), bit j of the row = (log_p[i-1][j-1] >= log_p[i-1][j])
    unsigned long long* bits = bits_lds ? lbits : ws + (int64_t)b * T * LW;
    const float* ab = attn + (int64_t)b * T * L;
    const float NEG = -INFINITY;
    int tok[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) tok[r] = 256 * wv + 64 * r + lane;
    // ---- forward: row 0, then one max and one add per cell and row.  Rows are loaded MAS_PF rows ahead into a ring of registers (the slot
    //      index is static: the row loop is unrolled MAS_PF times): a row's arithmetic takes a fraction of a memory latency, so with one
    //      row in flight the chain would run at one latency per row (measured: 0.58 us per row).  logf (is_log == 0) is taken when a row
    //      is used, not when it is loaded, so that no load is waited for early.
    const float NONE = is_log ? NEG : 0.f;                       // what a cell outside the corner loads as: logf(0) = -inf
    float prev[4], ring[MAS_PF][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float v = NEG;
        if (tok[r] == 0) {
            v = ab[0];
            if (!is_log) v = logf(v);
        }
        prev[r] = v;                                             // log_p[0][1:] = -inf
    }
    auto load_row = [&](int i, float* o) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = (i < n_out && tok[r] < n_in) ? ab[(int64_t)i * L + tok[r]] : NONE;
    };
#pragma unroll
    for (int k = 0; k < MAS_PF; ++k) load_row(1 + k, ring[k]);
    if (nw > 1) {
        if (lane == 63) edge[0][wv] = prev[3];
        __syncthreads();
    }
    for (int i0 = 1; i0 < n_out; i0 += MAS_PF) {
#pragma unroll
        for (int k = 0; k < MAS_PF; ++k) {
            const int i = i0 + k;
            if (i >= n_out) break;                               // (block-uniform)
            float cur[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) cur[r] = is_log ? ring[k][r] : logf(ring[k][r]);
            load_row(i + MAS_PF, ring[k]);                       // refill the slot: row i + MAS_PF is in flight while rows i .. are added
            float left[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) left[r] = __shfl_up(prev[r], 1, 64);
            {                                                    // token 64 q's left neighbour is lane 63 of q - 1
                const float l1 = __shfl(prev[0], 63, 64), l2 = __shfl(prev[1], 63, 64), l3 = __shfl(prev[2], 63, 64);
                float l0 = NEG;
                if (nw > 1 && wv > 0) l0 = edge[(i - 1) & 1][wv - 1];
                if (lane == 0) {
                    left[0] = l0; left[1] = l1; left[2] = l2; left[3] = l3;
                }
            }
            unsigned long long m[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p1 = left[r], p2 = prev[r];
                m[r] = __ballot(p1 >= p2);                       // ties (two -inf among them) go to j - 1
                const float best = p2 > p1 ? p2 : p1;            // Python's max(prev_log1, prev_log2)
                prev[r] = cur[r] + best;
            }
            if (lane == 0) {
                if (bits_lds) {
                    unsigned long long* br = lbits + i * LW + 4 * wv;
                    br[0] = m[0]; br[1] = m[1]; br[2] = m[2]; br[3] = m[3];
                } else {
                    unsigned long long* br = ws + ((int64_t)b * T + i) * LW + 4 * wv;
                    br[0] = m[0]; br[1] = m[1]; br[2] = m[2]; br[3] = m[3];
                }
            }
            if (nw > 1) {
                if (lane == 63) edge[i & 1][wv] = prev[3];
                __syncthreads();
            }
        }
    }
    // ---- backtrack (alignment.py:60-71): windows of MAS_WIN rows; the column moves by at most one per row, so a window needs the word
    //      of its first column and the one below it
    for (int l = tid; l < n_in; l += blockDim.x) cnt[l] = 0;
    if (tid == 0) {
        st[0] = n_out - 1;
        st[1] = n_in - 1;
    }
    __syncthreads();                                             // (also orders the block's stores of the bits before the loads below)
    while (true) {
        const int iw = st[0], jw = st[1];
        if (iw < 0) break;
        const int w1 = jw >> 6;
        if (tid < MAS_WIN) {
            const int i = iw - tid;
            unsigned long long a = 0, c = 0;
            if (i >= 1) {
                a = bits[(int64_t)i * LW + w1];
                if (w1 > 0) c = bits[(int64_t)i * LW + w1 - 1];
            }
            win[tid][0] = a;
            win[tid][1] = c;
        }
        __syncthreads();
        if (tid == 0) {
            int j = jw;
            const int nrow = min(MAS_WIN, iw + 1);
            for (int kq = 0; kq < nrow; ++kq) {
                col[kq] = j;
                cnt[j] += 1;
                const unsigned long long word = (j >> 6) == w1 ? win[kq][0] : win[kq][1];
                if (j > 0 && ((word >> (j & 63)) & 1ull)) --j;   // row 0 holds no decision (zero words); j == 0: the early exit's opt[1:i, 0]
            }
            st[0] = iw - nrow;
            st[1] = j;
        }
        __syncthreads();
        if (hb) {
            const int nrow = min(MAS_WIN, iw + 1);
            for (int e = tid; e < nrow * L; e += blockDim.x) {
                const int kq = e / L, l = e - kq * L;
                hb[(int64_t)(iw - kq) * L + l] = l == col[kq] ? 1.f : 0.f;
            }
        }
        __syncthreads();
    }
    for (int l = tid; l < L; l += blockDim.x) db[l] = l < n_in ? (float)cnt[l] : 0.f;
    if (hb)
        for (int64_t e = (int64_t)n_out * L + tid; e < (int64_t)T * L; e += blockDim.x) hb[e] = 0.f;
}

int32_t mas(const float* attn, int32_t is_log, const int64_t* in_lens, const int64_t* out_lens, int32_t B, int32_t T, int32_t L, float* dur,
            float* hard, void* ws, int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(in_lens && out_lens && B >= 1 && T >= 0 && L >= 0, "mas: bad argument (batch %d, frames %d, tokens %d)", B, T, L);
    TTS_REQUIRE(L <= MAS_MAX_L, "mas: %d tokens, at most TTSAMD_MAS_MAX_TOKENS = %d are built", L, MAS_MAX_L);
    if (L == 0) return 0;
    TTS_REQUIRE(dur && (T == 0 || attn), "mas: null argument");
    TTS_REQUIRE((int64_t)T * L < ((int64_t)1 << 31), "mas: %d x %d cells per utterance", T, L);
    const int64_t need = mas_workspace_bytes(B, T, L);
    TTS_REQUIRE(ws_bytes >= need && (need == 0 || ws), "mas: workspace of %lld bytes, %lld needed (ttsamd_mas_workspace_bytes)",
                (long long)ws_bytes, (long long)need);
    TTS_REQUIRE(need == 0 || ((uintptr_t)ws & 7) == 0, "mas: the workspace must be 8-byte aligned");
    hipLaunchKernelGGL(mas_kernel, dim3(B), dim3(64 * mas_waves(L)), 0, s, attn, is_log, in_lens, out_lens, T, L, need == 0 ? 1 : 0, dur, hard,
                       (unsigned long long*)ws);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------- average_pitch ----
constexpr int AP_CHUNK = 1024;

__global__ __launch_bounds__(256) void average_pitch_kernel(const float* __restrict__ pitch, const float* __restrict__ dur, int F, int T,
                                                            int L, float* __restrict__ out) {
    __shared__ int64_t ends[AP_CHUNK + 1];
    __shared__ float carry;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* dbp = dur + (int64_t)b * L;
    if (tid == 0) {
        carry = 0.f;
        ends[0] = 0;
    }
    for (int l0 = 0; l0 < L; l0 += AP_CHUNK) {
        const int n = min(AP_CHUNK, L - l0);
        __syncthreads();
        if (tid == 0) {                                          // torch.cumsum(durs, dim=1).long(): the fp32 running sum, truncated
            float c = carry;
            ends[0] = ends[l0 ? AP_CHUNK : 0];
            for (int l = 0; l < n; ++l) {
                c = c + dbp[l0 + l];
                ends[l + 1] = (int64_t)c;
            }
            carry = c;
        }
        __syncthreads();
        for (int e = tid; e < n * F; e += 256) {
            const int f = e / n, l = e - f * n;
            const int64_t t1 = min(max(ends[l + 1], (int64_t)0), (int64_t)T), t0 = min(max(ends[l], (int64_t)0), t1);
            const float* pr = pitch + ((int64_t)b * F + f) * T;
            double sum = 0.0;
            int nz = 0;
            for (int64_t t = t0; t < t1; ++t) {
                const float v = pr[t];
                if (v != 0.f) {
                    sum += (double)v;
                    ++nz;
                }
            }
            out[((int64_t)b * F + f) * L + l0 + l] = nz ? (float)(sum / nz) : 0.f;
        }
    }
}

int32_t average_pitch(const float* pitch, const float* dur, int32_t B, int32_t F, int32_t T, int32_t L, float* out, hipStream_t s) {
    TTS_REQUIRE(B >= 1 && F >= 0 && T >= 0 && L >= 0, "average_pitch: bad shape (batch %d, formants %d, frames %d, tokens %d)", B, F, T, L);
    if (F == 0 || L == 0) return 0;
    TTS_REQUIRE(dur && out && (T == 0 || pitch), "average_pitch: null argument");
    hipLaunchKernelGGL(average_pitch_kernel, dim3(B), dim3(256), 0, s, pitch, dur, F, T, L, out);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
