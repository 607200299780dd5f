// pYIN pitch tracking, wave -> (f0, voiced_flag, voiced_prob) per frame, in TWO launches whatever the length (include/ttsamd.h states
// the arithmetic).  What the reference gets from librosa.pyin (scripts/extract_f0.py:34-39,
// fastpitch/data_function.py:81-114), with two deliberate deviations: the difference function is summed directly in float64 (no FFT
// route, no clamp of values below 1e-6), and byte parity with a particular librosa release is not pinned.
//
// (a) pyin_frame_kernel: one block of 256 threads per (row, frame).  The padded frame sits in LDS; thread tau sums
//     d(tau) = sum_j (x[j] - x[j + tau])^2 over j ascending in float64 with separate multiply and add (no contraction: the sum is the
//     same bits as a sequential float64 sum on the host), one thread runs the cumulative sum in lag order, d' is formed in parallel,
//     troughs are found with one ballot per 64 lags and compacted by popcount, the (threshold, trough) incidence is a bit matrix
//     (one ballot per threshold and 64 troughs) from which the thread of trough m reads its position among the troughs under
//     threshold k as a popcount, and the winners of each pitch bin leave as a sparse list (bin, log-probability) plus the frame's
//     unvoiced log-probability: a dense [T][2P] observation array would be 130 MB at B = 32 x 860 frames.
// (b) pyin_viterbi_kernel: one block per row, thread j owns pitch bin j (its voiced and its unvoiced state).  Per step: the in-band
//     candidates (2 x w sources per destination, the band table in LDS as (same, switch) pairs, interior rows sharing one row), one
//     block-wide (max, lowest index) of the previous values for the out-of-band candidate max + log(tiny), ONE barrier.  The two value
//     vectors and the two observation vectors are double-buffered in LDS; the observations of step t + 1 are prefetched into registers
//     at the top of step t and scattered before the barrier.  Back-pointers go to the workspace as uint16; the backtrack runs in the
//     same launch, sixteen pointer rows at a time through LDS.  Latency-bound by construction: B blocks on 256 CUs, T dependent steps.
#include <cmath>
#include <cfloat>
#include <cstring>
#include <vector>

#include "kernels.hpp"

namespace ttsamd {

constexpr int PY_MAXN = 2048, PY_MAXBINS = 1024, PY_MAXTHR = 128, PY_MAXTAB = 12288, PY_FT = 256, PY_BTROWS = 16;
constexpr int PY_FRAME_LDS_MAX = 72 * 1024, PY_VIT_LDS_MAX = 128 * 1024;     // the opt-in ceilings: the limits above stay under them

struct PyinPlan {
    int sr, N, W, hop, pmin, pmax, L, nb, P, K, w, h, kinds, E, MW, pad_mode, a, b;
    double fmin, fmax, lambda, ntp, sw;
};

static int32_t pyin_plan(const ttsamd_pyin_cfg* c, PyinPlan& p) {
    TTS_REQUIRE(c, "pyin: null cfg");
    TTS_REQUIRE(c->sample_rate >= 1 && c->hop_length >= 1 && c->hop_length <= 65536, "pyin: sample_rate %d / hop_length %d", c->sample_rate,
                c->hop_length);
    TTS_REQUIRE(c->frame_length >= 4 && c->frame_length <= PY_MAXN && c->frame_length % 2 == 0,
                "pyin: frame_length %d: an even length <= %d is built", c->frame_length, PY_MAXN);
    TTS_REQUIRE(c->win_length >= 1 && c->win_length < c->frame_length, "pyin: win_length %d must be in [1, frame_length = %d)", c->win_length,
                c->frame_length);
    TTS_REQUIRE(std::isfinite(c->fmin) && std::isfinite(c->fmax) && c->fmin > 0 && c->fmax > c->fmin, "pyin: need 0 < fmin < fmax (got %g, %g)",
                c->fmin, c->fmax);
    TTS_REQUIRE(c->n_thresholds >= 1 && c->n_thresholds <= PY_MAXTHR, "pyin: n_thresholds %d outside [1, %d]", c->n_thresholds, PY_MAXTHR);
    TTS_REQUIRE(c->beta_a >= 1 && c->beta_b >= 1 && c->beta_a <= 64 && c->beta_b <= 64,
                "pyin: beta parameters (%d, %d): positive integers <= 64 are built (closed-form CDF)", c->beta_a, c->beta_b);
    TTS_REQUIRE(c->boltzmann > 0 && std::isfinite(c->boltzmann), "pyin: boltzmann parameter %g must be positive", c->boltzmann);
    TTS_REQUIRE(c->resolution > 0 && c->resolution <= 1, "pyin: resolution %g outside (0, 1]", c->resolution);
    TTS_REQUIRE(c->max_transition_rate >= 0 && std::isfinite(c->max_transition_rate), "pyin: max_transition_rate %g", c->max_transition_rate);
    TTS_REQUIRE(c->switch_prob >= 0 && c->switch_prob <= 1 && c->no_trough_prob >= 0 && c->no_trough_prob <= 1,
                "pyin: switch_prob %g / no_trough_prob %g outside [0, 1]", c->switch_prob, c->no_trough_prob);
    TTS_REQUIRE(c->pad_mode == 0 || c->pad_mode == 1, "pyin: pad_mode %d (0 constant, 1 reflect)", c->pad_mode);
    p.sr = c->sample_rate; p.N = c->frame_length; p.W = c->win_length; p.hop = c->hop_length; p.pad_mode = c->pad_mode;
    p.fmin = c->fmin; p.fmax = c->fmax; p.lambda = c->boltzmann; p.ntp = c->no_trough_prob; p.sw = c->switch_prob;
    p.K = c->n_thresholds; p.a = c->beta_a; p.b = c->beta_b;
    const double lo = std::floor((double)p.sr / p.fmax), hi = std::ceil((double)p.sr / p.fmin);
    p.pmin = lo < 1 ? 1 : (lo > 1e6 ? 1000000 : (int)lo);
    p.pmax = hi > (double)(p.N - p.W - 1) ? p.N - p.W - 1 : (int)hi;
    p.L = p.pmax - p.pmin + 1;
    TTS_REQUIRE(p.L >= 3, "pyin: lags %d..%d: fewer than three fit frame_length %d with win_length %d", p.pmin, p.pmax, p.N, p.W);
    const double nbd = std::ceil(1.0 / c->resolution);
    TTS_REQUIRE(nbd <= 1000, "pyin: resolution %g is finer than 1/1000 semitone", c->resolution);
    p.nb = (int)nbd;
    const double pb = std::floor(12.0 * p.nb * std::log2(p.fmax / p.fmin)) + 1;
    TTS_REQUIRE(pb >= 1 && pb <= PY_MAXBINS, "pyin: %g pitch bins: at most %d are built", pb, PY_MAXBINS);
    p.P = (int)pb;
    const double wr = std::nearbyint(c->max_transition_rate * 12.0 * p.hop / p.sr);
    TTS_REQUIRE(wr * p.nb + 1 <= PY_MAXTAB, "pyin: transition width %g", wr * p.nb + 1);
    p.w = (int)wr * p.nb + 1;
    TTS_REQUIRE(p.w % 2 == 1, "pyin: transition width %d: an odd width is built", p.w);
    p.h = p.w / 2;
    p.kinds = p.P < p.w ? p.P : p.w;
    TTS_REQUIRE((int64_t)p.kinds * p.w <= PY_MAXTAB, "pyin: transition table of %d x %d entries: at most %d are built", p.kinds, p.w, PY_MAXTAB);
    p.E = (p.L + 1) / 2;
    p.MW = (p.E + 63) / 64;
    return 0;
}

struct PyinTables {
    std::vector<double> beta, theta, expn, norm, trans;
    std::vector<float> logtrans, f0;
};

static double beta_cdf(int a, int b, double x) {                // I_x(a, b) for positive integers: sum_{j=a}^{n} C(n, j) x^j (1 - x)^(n - j), n = a + b - 1
    const int n = a + b - 1;
    double s = 0.0;
    for (int j = a; j <= n; ++j) {
        double c = 1.0;
        for (int i = 1; i <= j; ++i) c = c * (double)(n - j + i) / (double)i;
        s += c * std::pow(x, (double)j) * std::pow(1.0 - x, (double)(n - j));
    }
    return s;
}

static inline int pyin_kind(const PyinPlan& p, int k) {
    if (p.P <= p.w) return k;
    if (k < p.h) return k;
    if (k >= p.P - p.h) return k - (p.P - p.w);
    return p.h;
}

static void pyin_tables(const PyinPlan& p, PyinTables& t) {
    const double tiny = DBL_MIN;
    t.beta.resize(p.K); t.theta.resize(p.K);
    for (int k = 0; k < p.K; ++k) {
        t.theta[k] = (double)(k + 1) / (double)p.K;
        t.beta[k] = beta_cdf(p.a, p.b, (double)(k + 1) / (double)p.K) - beta_cdf(p.a, p.b, (double)k / (double)p.K);
    }
    t.expn.resize(p.E + 1); t.norm.resize(p.E + 1);
    for (int i = 0; i <= p.E; ++i) {
        t.expn[i] = std::exp(-p.lambda * i);
        t.norm[i] = i == 0 ? 0.0 : (1.0 - std::exp(-p.lambda)) / (1.0 - std::exp(-p.lambda * i));
    }
    std::vector<double> tri(p.w);
    for (int d = 0; d < p.w; ++d) tri[d] = (double)(p.h + 1 - std::abs(d - p.h)) / (double)(p.h + 1);
    t.trans.assign((size_t)p.kinds * p.w * 2, 0.0);
    t.logtrans.assign((size_t)p.kinds * p.w * 2, 0.f);
    for (int k = 0; k < p.P; ++k) {                             // every source bin writes its kind's row (interior bins: the same numbers)
        const int kd = pyin_kind(p, k);
        double sum = 0.0;
        for (int d = 0; d < p.w; ++d) {
            const int j = k + d - p.h;
            if (j >= 0 && j < p.P) sum += tri[d];
        }
        for (int d = 0; d < p.w; ++d) {
            const int j = k + d - p.h;
            const double bkj = (j >= 0 && j < p.P) ? tri[d] / sum : 0.0;
            const size_t o = ((size_t)kd * p.w + d) * 2;
            t.trans[o] = (1.0 - p.sw) * bkj;
            t.trans[o + 1] = p.sw * bkj;
            t.logtrans[o] = (float)std::log(t.trans[o] + tiny);
            t.logtrans[o + 1] = (float)std::log(t.trans[o + 1] + tiny);
        }
    }
    t.f0.resize(p.P);
    for (int s = 0; s < p.P; ++s) t.f0[s] = (float)(p.fmin * std::exp2((double)s / (12.0 * p.nb)));
}

int32_t pyin_tables_host(const ttsamd_pyin_cfg* cfg, int32_t* dims, double* beta, double* expn, double* norm, double* trans, float* logtrans,
                         float* f0) {
    PyinPlan p;
    TTS_TRY(pyin_plan(cfg, p));
    if (dims) {
        const int32_t d[8] = {p.pmin, p.pmax, p.P, p.nb, p.w, p.E, p.kinds, 0};
        memcpy(dims, d, sizeof(d));
    }
    if (!(beta || expn || norm || trans || logtrans || f0)) return 0;
    PyinTables t;
    pyin_tables(p, t);
    if (beta) memcpy(beta, t.beta.data(), t.beta.size() * sizeof(double));
    if (expn) memcpy(expn, t.expn.data(), t.expn.size() * sizeof(double));
    if (norm) memcpy(norm, t.norm.data(), t.norm.size() * sizeof(double));
    if (trans) memcpy(trans, t.trans.data(), t.trans.size() * sizeof(double));
    if (logtrans) memcpy(logtrans, t.logtrans.data(), t.logtrans.size() * sizeof(float));
    if (f0) memcpy(f0, t.f0.data(), t.f0.size() * sizeof(float));
    return 0;
}

// what the kernels take by value
struct PyinK {
    int sr, N, W, hop, pmin, pmax, L, P, K, E, MW, w, h, kinds, pad_mode;
    double fmin, ntp, binscale, sr_d;
    const double *beta, *theta, *expn, *norm;
    const float2* ltab;
    const float* f0tab;
    float LT, linit;                                            // fp32 log(tiny), log(1 / (2 P) + tiny)
};

struct Pyin {
    PyinPlan plan;
    PyinK k;
    char* dev = nullptr;
};

int32_t pyin_create(const ttsamd_pyin_cfg* cfg, Pyin** out) {
    TTS_REQUIRE(out, "pyin_create: null handle");
    PyinPlan p;
    TTS_TRY(pyin_plan(cfg, p));
    PyinTables t;
    pyin_tables(p, t);
    // one blob: doubles first (beta, theta, expn, norm), then the float2 band table, then f0
    const size_t nd = t.beta.size() + t.theta.size() + t.expn.size() + t.norm.size();
    const size_t bytes = nd * sizeof(double) + t.logtrans.size() * sizeof(float) + t.f0.size() * sizeof(float);
    std::vector<char> blob(bytes);
    char* q = blob.data();
    size_t o_beta = 0, o_theta, o_expn, o_norm, o_tab, o_f0;
    memcpy(q, t.beta.data(), t.beta.size() * 8);
    o_theta = o_beta + t.beta.size() * 8;
    memcpy(q + o_theta, t.theta.data(), t.theta.size() * 8);
    o_expn = o_theta + t.theta.size() * 8;
    memcpy(q + o_expn, t.expn.data(), t.expn.size() * 8);
    o_norm = o_expn + t.expn.size() * 8;
    memcpy(q + o_norm, t.norm.data(), t.norm.size() * 8);
    o_tab = o_norm + t.norm.size() * 8;
    memcpy(q + o_tab, t.logtrans.data(), t.logtrans.size() * 4);
    o_f0 = o_tab + t.logtrans.size() * 4;
    memcpy(q + o_f0, t.f0.data(), t.f0.size() * 4);
    auto* h = new Pyin();
    h->plan = p;
    hipError_t e = hipMalloc((void**)&h->dev, bytes);
    if (e == hipSuccess) e = hipMemcpy(h->dev, blob.data(), bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("pyin_create: upload failed: %s", hipGetErrorString(e));
        if (h->dev) (void)hipFree(h->dev);
        delete h;
        return TTSAMD_EHIP;
    }
    PyinK& k = h->k;
    k.sr = p.sr; k.N = p.N; k.W = p.W; k.hop = p.hop; k.pmin = p.pmin; k.pmax = p.pmax; k.L = p.L; k.P = p.P; k.K = p.K; k.E = p.E;
    k.MW = p.MW; k.w = p.w; k.h = p.h; k.kinds = p.kinds; k.pad_mode = p.pad_mode;
    k.fmin = p.fmin; k.ntp = p.ntp; k.binscale = (double)(12 * p.nb); k.sr_d = (double)p.sr;
    k.beta = (const double*)(h->dev + o_beta); k.theta = (const double*)(h->dev + o_theta);
    k.expn = (const double*)(h->dev + o_expn); k.norm = (const double*)(h->dev + o_norm);
    k.ltab = (const float2*)(h->dev + o_tab); k.f0tab = (const float*)(h->dev + o_f0);
    k.LT = (float)std::log(DBL_MIN);
    k.linit = (float)std::log(1.0 / (2.0 * p.P) + DBL_MIN);
    *out = h;
    return 0;
}

void pyin_destroy(Pyin* h) {
    if (!h) return;
    if (h->dev) (void)hipFree(h->dev);
    delete h;
}

struct PyinWs { int64_t cnt, unv, lp, bin, ptr, total; };

static PyinWs pyin_ws(const PyinPlan& p, int64_t B, int64_t T) {
    PyinWs w;
    w.cnt = 0;
    w.unv = align_up(w.cnt + B * T * 4, 256);
    w.lp = align_up(w.unv + B * T * 4, 256);
    w.bin = align_up(w.lp + B * T * p.E * 4, 256);
    w.ptr = align_up(w.bin + B * T * p.E * 2, 256);
    w.total = align_up(w.ptr + B * T * 2 * p.P * 2, 256);
    return w;
}

int64_t pyin_workspace_bytes(const Pyin* h, int32_t B, int32_t T) {
    if (!h || B < 1 || B > 65535 || T < 1 || T > TTSAMD_PYIN_MAX_FRAMES) return -1;
    return pyin_ws(h->plan, B, T).total;
}

int32_t pyin_obs_offsets(const Pyin* h, int32_t B, int32_t T, int64_t* off) {
    TTS_REQUIRE(h && off && B >= 1 && B <= 65535 && T >= 1 && T <= TTSAMD_PYIN_MAX_FRAMES, "pyin_obs_offsets: bad argument");
    const PyinWs w = pyin_ws(h->plan, B, T);
    off[0] = w.cnt; off[1] = w.unv; off[2] = w.lp; off[3] = w.bin;
    return 0;
}

// LDS carve of the frame kernel (bytes, 8-byte aligned pieces): d' [pmax] | cumsum, later trough heights [pmax] | trough probabilities [E]
// | incidence bits [K][MW] | trough mask [32] | winner mask [16] | reduction scratch [8] || frame [N] fp32 | trough bins [E] | N_k [K]
static size_t pyin_frame_lds(const PyinPlan& p) {
    return (size_t)8 * (2 * p.pmax + p.E + (size_t)p.K * p.MW + 32 + 16 + 8) + (size_t)4 * (p.N + p.E + p.K + 8);
}

__global__ __launch_bounds__(PY_FT) void pyin_frame_kernel(const PyinK c, const float* __restrict__ wave, int64_t wave_bs,
                                                           const int64_t* __restrict__ ns, int T_max, double* __restrict__ vprob,
                                                           int32_t* __restrict__ ocnt, float* __restrict__ ounv, float* __restrict__ olp,
                                                           uint16_t* __restrict__ obin, int64_t* __restrict__ frames_out) {
    extern __shared__ __attribute__((aligned(16))) char py_smem[];
    double* dd = reinterpret_cast<double*>(py_smem);                       // d(tau), then d'(tau), index tau - 1
    double* cs = dd + c.pmax;                                              // cumulative sums; dead once d' stands: trough heights th[m]
    double* tprob = cs + c.pmax;
    unsigned long long* below = reinterpret_cast<unsigned long long*>(tprob + c.E);
    unsigned long long* tmask = below + (size_t)c.K * c.MW;
    unsigned long long* cmask = tmask + 32;
    double* red = reinterpret_cast<double*>(cmask + 16);
    float* x = reinterpret_cast<float*>(red + 8);
    int* tbin = reinterpret_cast<int*>(x + c.N);
    int* nk = tbin + c.E;
    int* redi = nk + c.K;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int64_t n = max((int64_t)0, min(ns[b], wave_bs));
    const int fr = (int)min(n / c.hop + 1, (int64_t)T_max);
    if (t == 0 && tid == 0 && frames_out) frames_out[b] = fr;
    const int64_t ft = (int64_t)b * T_max + t;
    if (t >= fr) {
        if (tid == 0) { vprob[ft] = 0.0; ocnt[ft] = 0; ounv[ft] = 0.f; }
        return;
    }
    const float* wb = wave + (int64_t)b * wave_bs;
    for (int i = tid; i < c.N; i += PY_FT) {
        int64_t s = (int64_t)t * c.hop + i - c.N / 2;
        float v = 0.f;
        if (c.pad_mode == 0) {
            if (s >= 0 && s < n) v = wb[s];
        } else if (n == 1) {
            v = wb[0];
        } else if (n > 1) {                                                // periodic reflection about the row's own ends (numpy 'reflect')
            const int64_t per = 2 * (n - 1);
            s %= per;
            if (s < 0) s += per;
            if (s >= n) s = per - s;
            v = wb[s];
        }
        x[i] = v;
    }
    __syncthreads();
    // difference function: j ascending, separate float64 multiply and add (no contraction): the host's sequential sum, bit for bit
    for (int tau = 1 + tid; tau <= c.pmax; tau += PY_FT) {
        double acc = 0.0;
        for (int j = 0; j < c.W; ++j) {
            const double df = (double)x[j] - (double)x[j + tau];           // j + tau <= W - 1 + pmax <= N - 2
            acc = __dadd_rn(acc, __dmul_rn(df, df));
        }
        dd[tau - 1] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        double run = 0.0;
        for (int u = 0; u < c.pmax; ++u) {
            run = __dadd_rn(run, dd[u]);
            cs[u] = run;
        }
    }
    __syncthreads();
    for (int u = tid; u < c.pmax; u += PY_FT) dd[u] = dd[u] / (__dadd_rn(cs[u] / (double)(u + 1), DBL_MIN));
    __syncthreads();
    const double* dp = dd + (c.pmin - 1);                                  // d'[i], i = tau - pmin, i < L
    const int nch = (c.L + 63) / 64;                                       // <= 32
    for (int ch = wv; ch < nch; ch += PY_FT / 64) {
        const int i = ch * 64 + lane;
        bool tr = false;
        if (i < c.L) {
            if (i == 0) tr = dp[0] < dp[1];
            else if (i == c.L - 1) tr = dp[i] < dp[i - 1];
            else tr = dp[i] < dp[i - 1] && dp[i] <= dp[i + 1];
        }
        const unsigned long long mk = __ballot(tr);
        if (lane == 0) tmask[ch] = mk;
    }
    __syncthreads();
    int M = 0;
    for (int ch = 0; ch < nch; ++ch) M += __popcll(tmask[ch]);
    double* th = cs;
    for (int ch = wv; ch < nch; ch += PY_FT / 64) {
        const int i = ch * 64 + lane;
        const unsigned long long mk = tmask[ch];
        if ((mk >> lane) & 1ull) {
            int m = __popcll(mk & ((1ull << lane) - 1ull));
            for (int q = 0; q < ch; ++q) m += __popcll(tmask[q]);
            double shift = 0.0;
            if (i > 0 && i < c.L - 1) {
                const double a = dp[i + 1] + dp[i - 1] - 2.0 * dp[i];
                const double bb = (dp[i + 1] - dp[i - 1]) / 2.0;
                if (fabs(bb) < fabs(a)) shift = -bb / a;
            }
            const double f = c.sr_d / ((double)(c.pmin + i) + shift);
            double bn = rint(c.binscale * log2(f / c.fmin));
            bn = bn < 0.0 ? 0.0 : (bn > (double)c.P ? (double)c.P : bn);   // (NaN compares false twice: it falls to bin P, dropped)
            th[m] = dp[i];
            tbin[m] = bn == bn ? (int)bn : c.P;
        }
    }
    __syncthreads();
    // the lowest trough, first on ties
    {
        double bv = INFINITY;
        int bi = 0x7fffffff;
        for (int m = tid; m < M; m += PY_FT) {
            const double v = th[m];
            if (v < bv) { bv = v; bi = m; }
        }
        for (int o = 32; o >= 1; o >>= 1) {
            const double ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { red[wv] = bv; redi[wv] = bi; }
    }
    // incidence bits: below[k][word] bit l = trough 64 word + l is lower than threshold (k + 1) / K
    const int mw = (M + 63) / 64;
    for (int q = wv; q < c.K * mw; q += PY_FT / 64) {
        const int k = q / mw, wd = q - k * mw, m = wd * 64 + lane;
        const unsigned long long mk = __ballot(m < M && th[m] < c.theta[k]);
        if (lane == 0) below[k * c.MW + wd] = mk;
    }
    __syncthreads();
    int lowest = 0x7fffffff;
    {
        double bv = INFINITY;
        for (int q = 0; q < PY_FT / 64; ++q)
            if (red[q] < bv || (red[q] == bv && redi[q] < lowest)) { bv = red[q]; lowest = redi[q]; }
    }
    for (int k = tid; k < c.K; k += PY_FT) {
        int cnt = 0;
        for (int q = 0; q < mw; ++q) cnt += __popcll(below[k * c.MW + q]);
        nk[k] = cnt;
    }
    __syncthreads();
    for (int m = tid; m < M; m += PY_FT) {
        const int wd = m >> 6;
        const unsigned long long low = (1ull << (m & 63)) - 1ull;
        double acc = 0.0, extra = 0.0;
        for (int k = 0; k < c.K; ++k) {
            const unsigned long long bits = below[k * c.MW + wd];
            if ((bits >> (m & 63)) & 1ull) {
                int pos = __popcll(bits & low);
                for (int q = 0; q < wd; ++q) pos += __popcll(below[k * c.MW + q]);
                acc += c.beta[k] * (c.expn[pos] * c.norm[nk[k]]);
            } else if (m == lowest) {
                extra += c.beta[k];
            }
        }
        tprob[m] = acc + c.ntp * extra;
    }
    __syncthreads();
    // winners: the largest lag of each bin (bins fall as the lag grows), bin P dropped; those with a positive probability leave
    double part = 0.0;
    for (int ch = wv; ch < mw; ch += PY_FT / 64) {
        const int m = ch * 64 + lane;
        bool win = false;
        if (m < M) {
            win = tbin[m] < c.P && (m == M - 1 || tbin[m + 1] != tbin[m]);
            if (win) part += tprob[m];
            win = win && tprob[m] > 0.0;
        }
        const unsigned long long mk = __ballot(win);
        if (lane == 0) cmask[ch] = mk;
    }
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
    __syncthreads();                                                       // (red / redi were last read before the barrier above)
    if (lane == 0) red[wv] = part;
    __syncthreads();
    for (int ch = wv; ch < mw; ch += PY_FT / 64) {
        const int m = ch * 64 + lane;
        const unsigned long long mk = cmask[ch];
        if ((mk >> lane) & 1ull) {
            int e = __popcll(mk & ((1ull << lane) - 1ull));
            for (int q = 0; q < ch; ++q) e += __popcll(cmask[q]);
            olp[ft * c.E + e] = (float)log(tprob[m] + DBL_MIN);
            obin[ft * c.E + e] = (uint16_t)tbin[m];
        }
    }
    if (tid == 0) {
        int cnt = 0;
        for (int q = 0; q < mw; ++q) cnt += __popcll(cmask[q]);
        double vp = ((red[0] + red[1]) + red[2]) + red[3];
        vp = vp < 0.0 ? 0.0 : (vp > 1.0 ? 1.0 : vp);
        ocnt[ft] = cnt;
        vprob[ft] = vp;
        ounv[ft] = (float)log((1.0 - vp) / (double)c.P + DBL_MIN);
    }
}

// LDS of the Viterbi kernel: values float2 [2][Pp] | observations fp32 [2][Pp] | wave maxima (float, int) [2][16] | band table float2
// [kinds * w], later the pointer rows of the backtrack uint16 [PY_BTROWS][2 P] and its states int [PY_BTROWS]
static size_t pyin_vit_region(const PyinPlan& p) {
    const size_t tab = (size_t)p.kinds * p.w * 8, bt = (size_t)PY_BTROWS * 2 * p.P * 2 + PY_BTROWS * 4 + 16;
    return (tab > bt ? tab : bt) + 16;
}
static size_t pyin_vit_lds(const PyinPlan& p, int threads) { return (size_t)threads * (16 + 8) + 2 * 16 * 8 + pyin_vit_region(p); }

__global__ __launch_bounds__(1024) void pyin_viterbi_kernel(const PyinK c, int64_t wave_bs, const int64_t* __restrict__ ns, int T_max,
                                                            const int32_t* __restrict__ ocnt, const float* __restrict__ ounv,
                                                            const float* __restrict__ olp, const uint16_t* __restrict__ obin,
                                                            uint16_t* __restrict__ ptr, float* __restrict__ f0, uint8_t* __restrict__ flag,
                                                            int32_t* __restrict__ states) {
    extern __shared__ __attribute__((aligned(16))) char py_smem[];
    const int Pp = blockDim.x, P = c.P, j = threadIdx.x, lane = j & 63, wv = j >> 6, nw = Pp >> 6, b = blockIdx.x;
    float2* V = reinterpret_cast<float2*>(py_smem);                        // [2][Pp]: (voiced, unvoiced) value of bin j
    float* O = reinterpret_cast<float*>(V + 2 * Pp);                       // [2][Pp]: voiced log-observation of bin j
    float* wmv = O + 2 * Pp;                                               // [2][16]
    int* wmi = reinterpret_cast<int*>(wmv + 32);                           // [2][16]
    float2* tab = reinterpret_cast<float2*>(wmi + 32);
    uint16_t* bt = reinterpret_cast<uint16_t*>(tab);
    const int64_t n = max((int64_t)0, min(ns[b], wave_bs));
    const int fr = (int)min(n / c.hop + 1, (int64_t)T_max);
    const int64_t fb = (int64_t)b * T_max;
    const float LT = c.LT;
    for (int i = j; i < c.kinds * c.w; i += Pp) tab[i] = c.ltab[i];
    O[j] = LT;
    O[Pp + j] = LT;
    __syncthreads();
    if (j < ocnt[fb]) O[obin[fb * c.E + j]] = olp[fb * c.E + j];           // counts <= E <= P <= Pp, bins < P
    __syncthreads();
    // the source window of bin j: k in [klo, khi], column d = j - k + h; interior = every source row is the shared one
    const int klo = max(0, j - c.h), khi = min(P - 1, j + c.h);
    const bool interior = P > c.w && klo >= c.h && khi < P - c.h;
    float gmax;
    int gidx;
    // wave-level (max, lowest index), then every thread merges the wave results after the barrier
    auto reduce_store = [&](float v, int idx, int buf) {
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(v, o, 64);
            const int oi = __shfl_xor(idx, o, 64);
            if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
        }
        if (lane == 0) { wmv[buf * 16 + wv] = v; wmi[buf * 16 + wv] = idx; }
    };
    auto reduce_load = [&](int buf) {
        gmax = wmv[buf * 16];
        gidx = wmi[buf * 16];
        for (int q = 1; q < nw; ++q) {
            const float ov = wmv[buf * 16 + q];
            const int oi = wmi[buf * 16 + q];
            if (ov > gmax || (ov == gmax && oi < gidx)) { gmax = ov; gidx = oi; }
        }
    };
    // prefetch of a frame's observations into registers (entry j of the list)
    // a frame's count and unvoiced log-probability are the same for the whole block: as plain loads they become scalar loads, which
    // every LDS wait of the step then waits for.  Instead lane l of each wave keeps frame 64 q + l of the two arrays (one vector load
    // per 64 steps) and a step reads its frame with a cross-lane move.
    int ccache = 0, pcnt = 0, pbin = 0;
    float ucache = 0.f, plp = 0.f;
    auto refill = [&](int q) {
        const int f = 64 * q + lane;
        ccache = f < fr ? ocnt[fb + f] : 0;
        ucache = f < fr ? ounv[fb + f] : 0.f;
    };
    auto prefetch = [&](int t) {                                             // (t in the cached 64-frame block, or past the row)
        pcnt = __shfl(ccache, t & 63, 64);
        if (t >= fr) pcnt = 0;
        if (j < pcnt) {
            plp = olp[(fb + t) * c.E + j];
            pbin = obin[(fb + t) * c.E + j];
        }
    };
    refill(0);
    prefetch(1);
    {
        float v0 = -INFINITY, v1 = -INFINITY;
        int idx = 0x7fffffff;
        if (j < P) {
            v0 = O[j] + c.linit;
            v1 = ounv[fb] + c.linit;
            O[j] = LT;
            V[j] = make_float2(v0, v1);
            idx = j;
            if (v1 > v0) { v0 = v1; idx = P + j; }
        }
        reduce_store(v0, idx, 0);
        if (j < pcnt) O[Pp + pbin] = plp;
        __syncthreads();
        reduce_load(0);
    }
    for (int t = 1; t < fr; ++t) {
        const int cur = t & 1, prv = cur ^ 1;
        const float2* Vp = V + prv * Pp;
        const float ou = __shfl(ucache, t & 63, 64);
        if (((t + 1) & 63) == 0) refill((t + 1) >> 6);                     // frame t + 1 opens the next block of 64
        prefetch(t + 1);                                                   // (frame t's list is already in O[cur])
        float m0 = -INFINITY;
        int i0 = 0x7fffffff, arg0 = 0, arg1 = 0;
        if (j < P) {
            float b0v = -INFINITY, b1v = -INFINITY, b0u = -INFINITY, b1u = -INFINITY;   // best into (voiced, unvoiced) from voiced / unvoiced
            int a0v = 0, a1v = 0, a0u = 0, a1u = 0;
            if (interior) {
                const float2* tr = tab + c.h * c.w + (j + c.h);            // tr[-k] = row h, column j - k + h
#pragma unroll 4
                for (int k = klo; k <= khi; ++k) {
                    const float2 v = Vp[k], l = tr[-k];
                    const float c0v = v.x + l.x, c1v = v.x + l.y, c0u = v.y + l.y, c1u = v.y + l.x;
                    if (c0v > b0v) { b0v = c0v; a0v = k; }
                    if (c1v > b1v) { b1v = c1v; a1v = k; }
                    if (c0u > b0u) { b0u = c0u; a0u = k; }
                    if (c1u > b1u) { b1u = c1u; a1u = k; }
                }
            } else {
                for (int k = klo; k <= khi; ++k) {
                    const int kd = P <= c.w ? k : (k < c.h ? k : (k >= P - c.h ? k - (P - c.w) : c.h));
                    const float2 v = Vp[k], l = tab[kd * c.w + (j - k + c.h)];
                    const float c0v = v.x + l.x, c1v = v.x + l.y, c0u = v.y + l.y, c1u = v.y + l.x;
                    if (c0v > b0v) { b0v = c0v; a0v = k; }
                    if (c1v > b1v) { b1v = c1v; a1v = k; }
                    if (c0u > b0u) { b0u = c0u; a0u = k; }
                    if (c1u > b1u) { b1u = c1u; a1u = k; }
                }
            }
            // voiced sources come first in the state order: an unvoiced source must be strictly better
            float best0 = b0v, best1 = b1v;
            arg0 = a0v; arg1 = a1v;
            if (b0u > best0) { best0 = b0u; arg0 = P + a0u; }
            if (b1u > best1) { best1 = b1u; arg1 = P + a1u; }
            const float cg = gmax + LT;                                    // the best out-of-band source (every one of them has log(tiny))
            if (cg > best0 || (cg == best0 && gidx < arg0)) { best0 = cg; arg0 = gidx; }
            if (cg > best1 || (cg == best1 && gidx < arg1)) { best1 = cg; arg1 = gidx; }
            const float nv0 = O[cur * Pp + j] + best0, nv1 = ou + best1;
            O[cur * Pp + j] = LT;
            V[cur * Pp + j] = make_float2(nv0, nv1);
            m0 = nv0; i0 = j;
            if (nv1 > nv0) { m0 = nv1; i0 = P + j; }
        }
        if (j < pcnt) O[prv * Pp + pbin] = plp;                            // frame t + 1's list (those cells were cleared in step t - 1)
        reduce_store(m0, i0, cur);
        if (j < P) {                                                       // the pointer stores last: nothing of the step waits for them
            uint16_t* pr = ptr + (fb + t) * 2 * P;
            pr[j] = (uint16_t)arg0;
            pr[P + j] = (uint16_t)arg1;
        }
        __syncthreads();
        reduce_load(cur);
    }
    // backtrack: PY_BTROWS pointer rows at a time through LDS (the band table is dead); thread 0 walks, every thread writes outputs
    __shared__ int s_state;
    int* stl = reinterpret_cast<int*>((reinterpret_cast<uintptr_t>(bt + (size_t)PY_BTROWS * 2 * P) + 15) & ~(uintptr_t)15);
    if (j == 0) s_state = gidx;
    __syncthreads();
    for (int hi = fr - 1; hi >= 1; hi -= PY_BTROWS) {
        const int lo = max(hi - PY_BTROWS + 1, 1), rows = hi - lo + 1;
        const uint32_t* src = reinterpret_cast<const uint32_t*>(ptr + (fb + lo) * 2 * P);   // 2 P uint16 per row = P words, 4-byte aligned
        uint32_t* dst = reinterpret_cast<uint32_t*>(bt);
        for (int i = j; i < rows * P; i += Pp) dst[i] = src[i];
        __syncthreads();
        if (j == 0) {
            int s = s_state;
            for (int t = hi; t >= lo; --t) {
                stl[t - lo] = s;
                s = bt[(t - lo) * 2 * P + s];
            }
            s_state = s;
        }
        __syncthreads();
        if (j < rows) {
            const int s = stl[j];
            f0[fb + lo + j] = s < P ? c.f0tab[s] : 0.f;
            flag[fb + lo + j] = s < P ? 1 : 0;
            if (states) states[fb + lo + j] = s;
        }
        __syncthreads();
    }
    if (j == 0) {
        const int s = s_state;
        f0[fb] = s < P ? c.f0tab[s] : 0.f;
        flag[fb] = s < P ? 1 : 0;
        if (states) states[fb] = s;
    }
    for (int t = fr + j; t < T_max; t += Pp) {
        f0[fb + t] = 0.f;
        flag[fb + t] = 0;
        if (states) states[fb + t] = -1;
    }
}

static std::atomic<uint64_t> g_pyin_frame_lds{0}, g_pyin_vit_lds{0};

int32_t pyin_forward(const Pyin* h, const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t B, int32_t T_max, float* f0,
                     uint8_t* flag, double* vprob, int32_t* states, int64_t* frames_out, void* ws, int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(h && wave && nsamples && f0 && flag && vprob && ws, "pyin_forward: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535 && wave_stride >= 0, "pyin_forward: bad batch %d / stride", B);
    TTS_REQUIRE(T_max >= 1 && T_max <= TTSAMD_PYIN_MAX_FRAMES, "pyin_forward: t_max = %d outside [1, TTSAMD_PYIN_MAX_FRAMES = %d]", T_max,
                TTSAMD_PYIN_MAX_FRAMES);
    const PyinPlan& p = h->plan;
    const PyinWs w = pyin_ws(p, B, T_max);
    TTS_REQUIRE(ws_bytes >= w.total, "pyin_forward: workspace of %lld bytes, %lld needed", (long long)ws_bytes, (long long)w.total);
    TTS_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "pyin_forward: the workspace must be 256-byte aligned");
    char* base = (char*)ws;
    int32_t* ocnt = (int32_t*)(base + w.cnt);
    float* ounv = (float*)(base + w.unv);
    float* olp = (float*)(base + w.lp);
    uint16_t* obin = (uint16_t*)(base + w.bin);
    uint16_t* ptr = (uint16_t*)(base + w.ptr);
    const size_t flds = pyin_frame_lds(p);
    TTS_CHECK_HIP(lds_opt_in((const void*)pyin_frame_kernel, PY_FRAME_LDS_MAX, g_pyin_frame_lds));
    hipLaunchKernelGGL(pyin_frame_kernel, dim3(T_max, B), dim3(PY_FT), flds, s, h->k, wave, wave_stride, nsamples, T_max, vprob, ocnt, ounv,
                       olp, obin, frames_out);
    TTS_CHECK_HIP(hipGetLastError());
    const int threads = ((p.P > p.E ? p.P : p.E) + 63) / 64 * 64;            // thread j: pitch bin j, and entry j of a frame's observation list
    const size_t vlds = pyin_vit_lds(p, threads);
    TTS_REQUIRE(flds <= (size_t)PY_FRAME_LDS_MAX && vlds <= (size_t)PY_VIT_LDS_MAX, "pyin_forward: LDS plan %zu / %zu bytes", flds, vlds);
    TTS_CHECK_HIP(lds_opt_in((const void*)pyin_viterbi_kernel, PY_VIT_LDS_MAX, g_pyin_vit_lds));
    hipLaunchKernelGGL(pyin_viterbi_kernel, dim3(B), dim3(threads), vlds, s, h->k, wave_stride, nsamples, T_max, ocnt, ounv, olp, obin, ptr, f0,
                       flag, states);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
