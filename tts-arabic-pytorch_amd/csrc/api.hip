// extern "C" surface of libttsamd.so (include/ttsamd.h): argument checks, error strings,
// the launch-timing hooks used by bench.py, and thin forwards into the model code.
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.hpp"

namespace ttsamd {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
}

static int g_precision = 0;
int32_t default_precision() { return g_precision; }

// ---- launch timing (HIP events on the launch stream) -------------------------------
struct Prof {
    std::mutex mu;
    bool on = false;
    std::vector<hipEvent_t> ev;   // pairs
    size_t used = 0;
    size_t launches = 0;
    double flops_per_frame = 0.0;
} g_prof;

// Opens an event pair on `s` (a single launch, or a fork..join section of concurrent launches on several streams: the
// pair then measures the wall time of the section on the stream that forks and joins, never a sum of overlapping spans).
void prof_section_begin(hipStream_t s) {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (g_prof.used + 2 > g_prof.ev.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
        g_prof.ev.push_back(a);
        g_prof.ev.push_back(b);
    }
    (void)hipEventRecord(g_prof.ev[g_prof.used], s);
}

void prof_section_end(hipStream_t s) {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    if (g_prof.used + 2 > g_prof.ev.size()) return;
    (void)hipEventRecord(g_prof.ev[g_prof.used + 1], s);
    g_prof.used += 2;
}

// Counts one conv launch (and its algorithmic FLOPs per frame) inside an open section.
void prof_add(double flops_per_frame) {
    if (!g_prof.on) return;
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.launches += 1;
    g_prof.flops_per_frame += flops_per_frame;
}

void prof_begin(hipStream_t s, double flops_per_frame) {
    prof_section_begin(s);
    prof_add(flops_per_frame);
}

void prof_end(hipStream_t s) { prof_section_end(s); }

struct HifiGan;
struct FastPitch;
struct Denoiser;
struct Vocos;
int32_t vocos_create(const ttsamd_tensor*, int32_t, int32_t, int32_t, int32_t, int32_t, Vocos**);
void vocos_destroy(Vocos*);
int64_t vocos_workspace_bytes(const Vocos*, int32_t, int32_t);
int64_t vocos_bias_workspace_bytes(const Vocos*);
int32_t vocos_bias_vec(const Vocos*, float*, void*, int64_t, hipStream_t);
int32_t vocos_forward(const Vocos*, const float*, const int64_t*, int32_t, int32_t, float, const float*, const float*, float*, void*,
                      int64_t, hipStream_t);
int32_t vocos_set_padding(Vocos*, int32_t);
int32_t vocos_halo_frames(const Vocos*, int32_t*, int32_t*);
int32_t vocos_features_out(const Vocos*, const float*, const int64_t*, int32_t, int32_t, float*, void*, int64_t, hipStream_t);
int32_t vocos_head(const Vocos*, const float*, const int64_t*, int32_t, int32_t, const float*, const float*, float*, void*, int64_t,
                   hipStream_t);
int32_t vocos_forward_windows(const Vocos*, const float*, const int64_t*, int32_t, int32_t, const int32_t*, const int32_t*, const float*,
                              const float*, float*, void*, int64_t, hipStream_t);
struct MelSpec;
int32_t melspec_create(const float*, int32_t, int32_t, int32_t, int32_t, int32_t, float, MelSpec**);
void melspec_destroy(MelSpec*);
int32_t melspec_forward(const MelSpec*, const float*, int64_t, const int64_t*, int32_t, int32_t, float*, int64_t*, hipStream_t);
int32_t cepstral_series(const float*, const int64_t*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, float, float*, float*, hipStream_t);
int32_t cepstral_series_from_power(const float*, const int64_t*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, double, double, float,
                                   float*, hipStream_t);
int32_t series_summary(const float*, const int64_t*, int32_t, int32_t, int32_t, float*, float*, hipStream_t);
int64_t dtw_workspace_bytes(int32_t, int32_t, int32_t, int32_t);
int32_t dtw(const float*, const int64_t*, const float*, const int64_t*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, float*,
            int32_t*, int32_t*, void*, int64_t, hipStream_t);
int32_t dtw_aligned_mae(const float*, const float*, int32_t, int32_t, int32_t, const int32_t*, const int32_t*, float*, hipStream_t);
int32_t mel_cepstrum(const float*, const int64_t*, int32_t, int32_t, int32_t, int32_t, float*, hipStream_t);
int32_t dtw_aligned_eval(const float*, const float*, int32_t, int32_t, const float*, const float*, int32_t, const float*, const float*, int32_t,
                         int32_t, int32_t, const int32_t*, const int32_t*, double, double*, hipStream_t);
struct Aligner;
int32_t aligner_create(const ttsamd_tensor*, int32_t, const ttsamd_aligner_cfg*, Aligner**);
void aligner_destroy(Aligner*);
int64_t aligner_workspace_bytes(const Aligner*, int32_t, int32_t, int32_t);
int32_t aligner_forward(const Aligner*, const int64_t*, const int64_t*, const float*, const int64_t*, const float*, int32_t, int32_t, int32_t,
                        float*, float*, void*, int64_t, hipStream_t);
int64_t mas_workspace_bytes(int32_t, int32_t, int32_t);
int32_t mas(const float*, int32_t, const int64_t*, const int64_t*, int32_t, int32_t, int32_t, float*, float*, void*, int64_t, hipStream_t);
int32_t average_pitch(const float*, const float*, int32_t, int32_t, int32_t, int32_t, float*, hipStream_t);
int32_t attn_prior(const int64_t*, const int64_t*, int32_t, int32_t, int32_t, int32_t, double, void*, hipStream_t);
int32_t attn_prior_tables_host(int32_t, double*);
int64_t attn_ctc_workspace_bytes(int32_t, int32_t, int32_t);
int32_t attn_ctc_loss(const float*, const int64_t*, const int64_t*, int32_t, int32_t, int32_t, double, double*, void*, int64_t, hipStream_t);
int32_t attn_bin_loss(const float*, const float*, int32_t, int32_t, int32_t, double, double*, double*, hipStream_t);
struct Pyin;
int32_t pyin_tables_host(const ttsamd_pyin_cfg*, int32_t*, double*, double*, double*, double*, float*, float*);
int32_t pyin_create(const ttsamd_pyin_cfg*, Pyin**);
void pyin_destroy(Pyin*);
int64_t pyin_workspace_bytes(const Pyin*, int32_t, int32_t);
int32_t pyin_obs_offsets(const Pyin*, int32_t, int32_t, int64_t*);
int32_t pyin_forward(const Pyin*, const float*, int64_t, const int64_t*, int32_t, int32_t, float*, uint8_t*, double*, int32_t*, int64_t*, void*,
                     int64_t, hipStream_t);
struct Taco2;
int32_t tacotron2_create(const ttsamd_tensor*, int32_t, const ttsamd_tacotron2_cfg*, Taco2**);
void tacotron2_destroy(Taco2*);
int64_t tacotron2_workspace_bytes(const Taco2*, int32_t, int32_t, int32_t);
int32_t tacotron2_infer(const Taco2*, const int64_t*, const int64_t*, const int64_t*, int32_t, int32_t, int32_t, int64_t,
                        float*, int32_t*, float*, float*, int32_t*, void*, int64_t, hipStream_t);
struct TacoStream;
int64_t tacotron2_stream_bytes(const Taco2*, int32_t, int32_t, int32_t, int32_t);
int32_t tacotron2_stream_begin(const Taco2*, const int64_t*, const int64_t*, const int64_t*, int32_t, int32_t, int32_t, int32_t, int64_t,
                               const int32_t*, int32_t, float*, int32_t*, float*, void*, int64_t, TacoStream**, hipStream_t);
int32_t tacotron2_stream_advance(TacoStream*, int32_t, int32_t*, int32_t*, int32_t*, hipStream_t);
void tacotron2_stream_end(TacoStream*);
int32_t tacotron2_postnet_halo(const Taco2*);
int64_t tacotron2_postnet_window_bytes(const Taco2*, int32_t, int32_t);
int32_t tacotron2_postnet_window(const Taco2*, const float*, float*, int32_t, int32_t, int32_t, int32_t, int32_t, int32_t, void*, int64_t,
                                 hipStream_t);
struct Tagger;
int32_t tagger_create(const ttsamd_tensor*, int32_t, const ttsamd_tagger_cfg*, Tagger**);
void tagger_destroy(Tagger*);
int64_t tagger_workspace_bytes(const Tagger*, int32_t, int32_t);
int32_t tagger_forward(const Tagger*, const int64_t*, int32_t, int32_t, float*, void*, int64_t, hipStream_t);
int32_t denoiser_create(Denoiser**);
void denoiser_destroy(Denoiser*);
int64_t denoiser_workspace_bytes(int32_t, int32_t);
int32_t denoiser_bias_spec(const Denoiser*, const float*, const int64_t*, int32_t, float*, void*, int64_t, hipStream_t);
int32_t denoise(const Denoiser*, float*, int64_t, const int64_t*, int32_t, int32_t, const float*, float, const float*, void*, int64_t,
                hipStream_t);
int32_t hifigan_halo_frames(const HifiGan*, int32_t*, int32_t*);
int32_t stream_gather(const float*, int32_t, int32_t, int32_t, const int32_t*, const int32_t*, const int32_t*, int32_t, int32_t, float*,
                      int64_t*, hipStream_t);
int32_t stream_emit(const float*, int32_t, int32_t, int32_t, const int32_t*, const int32_t*, int32_t, int32_t, void*, hipStream_t);
int32_t stream_emit_resampled(const Resample*, const float*, int32_t, int32_t, int32_t, const int32_t*, const int32_t*, const int32_t*,
                              const int32_t*, const int32_t*, int32_t, int32_t, void*, int32_t*, hipStream_t);
int32_t wave_encode(const float*, int64_t, const int64_t*, int32_t, int32_t, void*, int64_t, hipStream_t);
int32_t hifigan_create(const ttsamd_tensor*, int32_t, const ttsamd_hifigan_cfg*, HifiGan**);
void hifigan_destroy(HifiGan*);
int64_t hifigan_workspace_bytes(const HifiGan*, int32_t, int32_t);
int32_t hifigan_forward(const HifiGan*, const float*, const int64_t*, int32_t, int32_t, float*, void*, int64_t,
                        hipStream_t);
int32_t fastpitch_create(const ttsamd_tensor*, int32_t, const ttsamd_fastpitch_cfg*, int32_t, FastPitch**);
void fastpitch_destroy(FastPitch*);
int64_t fastpitch_encode_workspace_bytes(const FastPitch*, int32_t, int32_t);
int64_t fastpitch_decode_workspace_bytes(const FastPitch*, int32_t, int32_t);
int32_t fastpitch_encode(const FastPitch*, const int64_t*, int32_t, int32_t, int32_t, float, const float*,
                         const float*, const float*, float, float, float, float*, float*, float*, float*, int64_t*,
                         int64_t*, void*, int64_t, hipStream_t);
void fastpitch_set_batch_mode(const FastPitch*, int);
int32_t fastpitch_decode(const FastPitch*, float*, const int64_t*, int32_t, int32_t, float*, void*, int64_t,
                         hipStream_t);
int32_t fastpitch_encode_rows(const FastPitch*, const int64_t*, int32_t, int32_t, int32_t, float, const float*,
                              const float*, const float*, float, float, float, float*, float*, float*, float*, int64_t*,
                              int64_t*, void*, int64_t, const int32_t*, const float*, const float*, const float*, int32_t, hipStream_t);
int32_t fastpitch_decode_rows(const FastPitch*, float*, const int64_t*, int32_t, int32_t, float*, void*, int64_t, int32_t,
                              hipStream_t);

__global__ void pack_conv_weight_kernel(const float* __restrict__ w, int cout, int cin, int k, int cp,
                                        float* __restrict__ out) {
    // same layout as pack_conv_weight (conv_mfma.hip): [cin/8][k][2][cp][4]
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)cin * k * cp;
    if (i >= n) return;
    const int pq = (int)(i % 4);
    const int co = (int)((i / 4) % cp);
    const int kk = (int)((i / (4 * (int64_t)cp)) % 2);
    const int t = (int)((i / (8 * (int64_t)cp)) % k);
    const int o = (int)(i / (8 * (int64_t)cp * k));
    out[i] = co < cout ? w[((int64_t)co * cin + (8 * o + 2 * pq + kk)) * k + t] : 0.f;
}

// torch ConvTranspose1d weight [cin][cout][2u] (stride u, padding u / 2) -> the u polyphase 2-tap filters [u][cin/8][2][2][cp][4]
// (same layout and values as pack_convt_weight, conv_mfma.hip)
__global__ void pack_convt_weight_kernel(const float* __restrict__ w, int cin, int cout, int u, int cp, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)u * cin * 2 * cp;
    if (i >= n) return;
    const int pq = (int)(i % 4);
    const int co = (int)((i / 4) % cp);
    const int kk = (int)((i / (4 * (int64_t)cp)) % 2);
    const int t = (int)((i / (8 * (int64_t)cp)) % 2);
    const int o = (int)((i / (16 * (int64_t)cp)) % (cin / 8));
    const int rho = (int)(i / (16 * (int64_t)cp * (cin / 8)));
    const int kidx = (rho + u / 2) % u + t * u;
    out[i] = co < cout ? w[((int64_t)(8 * o + 2 * pq + kk) * cout + co) * (2 * u) + kidx] : 0.f;
}

// torch ConvTranspose1d weight [cin][cout][2u] -> the F(4,2) group filters of the (u cout)-row two-tap conv [cin/8][6][2][u cout][4], row =
// co u + j, taps (g0, g1) = (w[..][j + u], w[..][j]); the u cout floats behind them: the bias per row (same values as pack_convt_wino_weight,
// conv_wino4.hip)
__global__ void pack_convt_wino_kernel(const float* __restrict__ w, const float* __restrict__ bias, int cin, int cout, int u,
                                       float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int rows = u * cout;
    const int64_t n = (int64_t)6 * cin * rows;
    if (i >= n + rows) return;
    if (i >= n) {
        out[i] = bias ? bias[(i - n) / u] : 0.f;
        return;
    }
    const int pq = (int)(i & 3);
    const int64_t r = i >> 2;
    const int row = (int)(r % rows);
    const int64_t r2 = r / rows;
    const int kk = (int)(r2 & 1);
    const int64_t r3 = r2 >> 1;
    const int t = (int)(r3 % 6), o = (int)(r3 / 6);
    const int co = row / u, j = row % u;
    const float* g = w + ((int64_t)(8 * o + 2 * pq + kk) * cout + co) * 2 * u;
    const double g0 = g[j + u], g1 = g[j];
    out[i] = t == 0 ? (float)(g0 / 4) : (t == 1 ? (float)(-(g0 + g1) / 6) : (t == 2 ? (float)(-(g0 - g1) / 6) :
             (t == 3 ? (float)(g0 / 24 + g1 / 12) : (t == 4 ? (float)(g0 / 24 - g1 / 12) : 0.f))));
}

__global__ void split_bf16_kernel(const float* __restrict__ packed, int64_t n, unsigned short* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float f = packed[i];
    unsigned u = __float_as_uint(f);
    u += 0x7fffu + ((u >> 16) & 1u);
    const unsigned h = u >> 16;
    const float r = f - __uint_as_float(h << 16);
    unsigned v = __float_as_uint(r);
    v += 0x7fffu + ((v >> 16) & 1u);
    out[i] = (unsigned short)h;
    out[n + i] = (unsigned short)(v >> 16);
}

// ---- run-time routing options (common.hpp: TTS_OPTIONS) --------------------------------------------------------------------------------
namespace {
struct OptDesc { const char* name; int kind; long long lo, hi; };
const OptDesc kOpts[OPT_COUNT] = {
#define TTS_OPT_DESC(name, kind, lo, hi) {"TTSAMD_" #name, kind, lo, hi},
    TTS_OPTIONS(TTS_OPT_DESC)
#undef TTS_OPT_DESC
};
std::atomic<const char*> g_opt[OPT_COUNT];       // interned strings, never freed (a few bytes per ttsamd_set_option call)
std::once_flag g_opt_once;
std::string g_opt_env_error;                     // first malformed TTSAMD_<NAME> of the environment (ttsamd_options_check)

bool opt_valid(const OptDesc& d, const char* v) {
    if (!v || !*v) return false;
    char* end = nullptr;
    errno = 0;
    const long long x = std::strtoll(v, &end, d.kind == 1 ? 16 : 10);
    if (!(errno == 0 && end != v && *end == '\0' && x >= d.lo && x <= d.hi)) return false;
    // TTSAMD_WINO4 bits 5 / 6 say HOW the F(4,3) kernel runs k = 7 / 11 (seven-point groups): without bit 1 / 2 it does not run that k at
    // all and the mask contradicts itself -- an error like any malformed value, not a bit that is quietly ignored.  Bit 7 says how it runs
    // the dilated launches (packed tiles, register epilogue): the same without bit 3
    if (&d == &kOpts[OPT_WINO4] && (((x & 32) && !(x & 2)) || ((x & 64) && !(x & 4)) || ((x & 128) && !(x & 8)))) return false;
    return true;
}
void opt_init() {
    std::call_once(g_opt_once, [] {
        for (int i = 0; i < OPT_COUNT; ++i) {
            const char* e = std::getenv(kOpts[i].name);        // the ONE getenv per option and process
            if (!e || !*e) continue;
            if (!opt_valid(kOpts[i], e)) {
                if (g_opt_env_error.empty()) {
                    char buf[256];
                    std::snprintf(buf, sizeof buf, "%s='%s' in the environment is not a valid value (%s in [%llx, %llx])", kOpts[i].name, e,
                                  kOpts[i].kind == 1 ? "hex mask" : "integer", kOpts[i].lo, kOpts[i].hi);
                    g_opt_env_error = buf;
                }
                continue;
            }
            g_opt[i].store(strdup(e), std::memory_order_release);
        }
    });
}
int opt_find(const char* name) {
    if (!name) return -1;
    for (int i = 0; i < OPT_COUNT; ++i)
        if (std::strcmp(name, kOpts[i].name) == 0 || std::strcmp(name, kOpts[i].name + 7) == 0) return i;
    return -1;
}
}  // namespace

int64_t opt_int(Opt o, int64_t unset) {
    opt_init();
    const char* v = g_opt[o].load(std::memory_order_acquire);     // validated: parses whole and in range
    return v ? (int64_t)std::strtoll(v, nullptr, kOpts[o].kind == 1 ? 16 : 10) : unset;
}

}  // namespace ttsamd

using namespace ttsamd;

extern "C" {

const char* ttsamd_last_error(void) { return g_err.c_str(); }
int32_t ttsamd_version(void) { return TTSAMD_ABI_VERSION; }

int32_t ttsamd_set_option(const char* name, const char* value) {
    opt_init();
    const int i = opt_find(name);
    TTS_REQUIRE(i >= 0, "set_option: unknown option '%s' (ttsamd_option_name lists them)", name ? name : "(null)");
    if (!value || !*value) {
        g_opt[i].store(nullptr, std::memory_order_release);
        return 0;
    }
    TTS_REQUIRE(opt_valid(kOpts[i], value), "set_option: %s='%s' is not a valid value (%s in [%llx, %llx])", kOpts[i].name, value,
                kOpts[i].kind == 1 ? "hex mask" : "integer", kOpts[i].lo, kOpts[i].hi);
    g_opt[i].store(strdup(value), std::memory_order_release);
    return 0;
}
int32_t ttsamd_get_option(const char* name, char* value, int32_t capacity) {
    opt_init();
    const int i = opt_find(name);
    TTS_REQUIRE(i >= 0 && value && capacity > 0, "get_option: unknown option '%s' or no buffer", name ? name : "(null)");
    const char* v = g_opt[i].load(std::memory_order_acquire);
    std::snprintf(value, (size_t)capacity, "%s", v ? v : "");
    return 0;
}
const char* ttsamd_option_name(int32_t index) { return (index >= 0 && index < OPT_COUNT) ? kOpts[index].name : nullptr; }
int32_t ttsamd_options_check(void) {
    opt_init();
    TTS_REQUIRE(g_opt_env_error.empty(), "%s", g_opt_env_error.c_str());
    return 0;
}

int32_t ttsamd_device_ok(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, 0) != hipSuccess) return 0;
    return std::string(prop.gcnArchName).rfind("gfx950", 0) == 0 ? 1 : 0;
}

int32_t ttsamd_hifigan_create(const ttsamd_tensor* weights, int32_t n, const ttsamd_hifigan_cfg* cfg, void** handle) {
    HifiGan* h = nullptr;
    const int32_t rc = hifigan_create(weights, n, cfg, &h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_hifigan_destroy(void* handle) {
    hifigan_destroy((HifiGan*)handle);
    return 0;
}
int64_t ttsamd_hifigan_workspace_bytes(void* handle, int32_t batch, int32_t t_max) {
    if (!handle || batch < 1 || t_max < 1) return 0;
    return hifigan_workspace_bytes((HifiGan*)handle, batch, t_max);
}
int32_t ttsamd_hifigan_forward(void* handle, const float* mel, const int64_t* lens, int32_t batch, int32_t t_max,
                               float* wave, void* workspace, int64_t workspace_bytes, void* stream) {
    return hifigan_forward((HifiGan*)handle, mel, lens, batch, t_max, wave, workspace, workspace_bytes,
                           (hipStream_t)stream);
}

// streaming synthesis (stream.hip)
int32_t ttsamd_hifigan_halo_frames(void* handle, int32_t* left, int32_t* right) {
    return hifigan_halo_frames((HifiGan*)handle, left, right);
}
int32_t ttsamd_denoiser_halo_frames(void) { return 3; }   // (1024 / 2 + 1024 / 2 - 256) / 256: ttsamd.h
int32_t ttsamd_stream_gather(const float* pool, int32_t n_slots, int32_t num_mels, int32_t t_cap, const int32_t* slot, const int32_t* start,
                             const int32_t* len, int32_t n_windows, int32_t w_max, float* batch, int64_t* lens, void* stream) {
    return stream_gather(pool, n_slots, num_mels, t_cap, slot, start, len, n_windows, w_max, batch, lens, (hipStream_t)stream);
}
int32_t ttsamd_stream_emit(const float* wave, int32_t n_windows, int32_t w_max, int32_t hop, const int32_t* core_off, const int32_t* core_len,
                           int32_t c_max, int32_t format, void* out, void* stream) {
    return stream_emit(wave, n_windows, w_max, hop, core_off, core_len, c_max, format, out, (hipStream_t)stream);
}
int32_t ttsamd_stream_emit_resampled(void* resample_handle, const float* wave, int32_t n_windows, int32_t w_max, int32_t hop,
                                     const int32_t* win_start, const int32_t* win_len, const int32_t* utt_len, const int32_t* core_start,
                                     const int32_t* core_end, int32_t c_max, int32_t format, void* out, int32_t* nout, void* stream) {
    return stream_emit_resampled((const Resample*)resample_handle, wave, n_windows, w_max, hop, win_start, win_len, utt_len, core_start,
                                 core_end, c_max, format, out, nout, (hipStream_t)stream);
}
int32_t ttsamd_wave_encode(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t format, void* out,
                           int64_t out_stride, void* stream) {
    return wave_encode(wave, wave_stride, nsamples, batch, format, out, out_stride, (hipStream_t)stream);
}

int32_t ttsamd_fastpitch_create(const ttsamd_tensor* weights, int32_t n, const ttsamd_fastpitch_cfg* cfg,
                                void** handle) {
    FastPitch* h = nullptr;
    const int32_t rc = fastpitch_create(weights, n, cfg, /*pos_cap=*/16384, &h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_fastpitch_destroy(void* handle) {
    fastpitch_destroy((FastPitch*)handle);
    return 0;
}
int64_t ttsamd_fastpitch_encode_workspace_bytes(void* handle, int32_t batch, int32_t n_tokens) {
    if (!handle || batch < 1 || n_tokens < 1) return 0;
    return fastpitch_encode_workspace_bytes((FastPitch*)handle, batch, n_tokens);
}
int64_t ttsamd_fastpitch_decode_workspace_bytes(void* handle, int32_t batch, int32_t t_max) {
    if (!handle || batch < 1 || t_max < 1) return 0;
    return fastpitch_decode_workspace_bytes((FastPitch*)handle, batch, t_max);
}
int32_t ttsamd_fastpitch_encode(void* handle, const int64_t* ids, int32_t batch, int32_t n_tokens, int32_t speaker,
                                float pace, const float* dur_tgt, const float* pitch_tgt, const float* energy_tgt,
                                float pitch_mul, float pitch_add, float max_duration, float* enc_cond,
                                float* dur_pred, float* pitch_pred, float* energy_pred, int64_t* reps,
                                int64_t* dec_lens, void* workspace, int64_t workspace_bytes, void* stream) {
    return fastpitch_encode((FastPitch*)handle, ids, batch, n_tokens, speaker, pace, dur_tgt, pitch_tgt, energy_tgt,
                            pitch_mul, pitch_add, max_duration, enc_cond, dur_pred, pitch_pred, energy_pred, reps,
                            dec_lens, workspace, workspace_bytes, (hipStream_t)stream);
}
int32_t ttsamd_length_regulate(const float* enc, const int64_t* reps, int32_t batch, int32_t n_tokens,
                               int32_t channels, int32_t t_max, float* out, int32_t* idx, void* stream) {
    TTS_REQUIRE(enc && reps && out && batch >= 1 && n_tokens >= 1 && channels >= 1 && t_max >= 0,
                "length_regulate: bad argument");
    return launch_regulate_gather(enc, reps, nullptr, 0, batch, n_tokens, channels, t_max, out, idx,
                                  (hipStream_t)stream);
}
int32_t ttsamd_fastpitch_set_batch_mode(void* handle, int32_t mode) {
    TTS_REQUIRE(handle != nullptr, "fastpitch_set_batch_mode: null handle");
    TTS_REQUIRE(mode == 0 || mode == 1, "fastpitch_set_batch_mode: mode %d (0 = padded-batch arithmetic, 1 = every utterance alone)", mode);
    fastpitch_set_batch_mode((const FastPitch*)handle, mode);
    return 0;
}
int32_t ttsamd_fastpitch_decode(void* handle, float* x, const int64_t* dec_lens, int32_t batch, int32_t t_max,
                                float* mel, void* workspace, int64_t workspace_bytes, void* stream) {
    return fastpitch_decode((FastPitch*)handle, x, dec_lens, batch, t_max, mel, workspace, workspace_bytes,
                            (hipStream_t)stream);
}
int32_t ttsamd_fastpitch_encode_rows(void* handle, const int64_t* ids, int32_t batch, int32_t n_tokens, int32_t speaker,
                                     float pace, const float* dur_tgt, const float* pitch_tgt, const float* energy_tgt,
                                     float pitch_mul, float pitch_add, float max_duration, float* enc_cond,
                                     float* dur_pred, float* pitch_pred, float* energy_pred, int64_t* reps,
                                     int64_t* dec_lens, void* workspace, int64_t workspace_bytes,
                                     const int32_t* speaker_rows, const float* pace_rows, const float* pitch_mul_rows,
                                     const float* pitch_add_rows, int32_t flags, void* stream) {
    return fastpitch_encode_rows((FastPitch*)handle, ids, batch, n_tokens, speaker, pace, dur_tgt, pitch_tgt, energy_tgt,
                                 pitch_mul, pitch_add, max_duration, enc_cond, dur_pred, pitch_pred, energy_pred, reps,
                                 dec_lens, workspace, workspace_bytes, speaker_rows, pace_rows, pitch_mul_rows, pitch_add_rows,
                                 flags, (hipStream_t)stream);
}
int32_t ttsamd_fastpitch_decode_rows(void* handle, float* x, const int64_t* dec_lens, int32_t batch, int32_t t_max,
                                     float* mel, void* workspace, int64_t workspace_bytes, int32_t flags, void* stream) {
    return fastpitch_decode_rows((FastPitch*)handle, x, dec_lens, batch, t_max, mel, workspace, workspace_bytes, flags,
                                 (hipStream_t)stream);
}

int32_t ttsamd_denoiser_create(void** handle) {
    Denoiser* h = nullptr;
    const int32_t rc = denoiser_create(&h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_denoiser_destroy(void* handle) {
    denoiser_destroy((Denoiser*)handle);
    return 0;
}
int64_t ttsamd_denoiser_workspace_bytes(int32_t batch, int32_t n_max) {
    if (batch < 1 || n_max < 1) return 0;
    return denoiser_workspace_bytes(batch, n_max);
}
int32_t ttsamd_denoiser_bias_spec(void* handle, const float* audio, const int64_t* n_dev, int32_t n,
                                  float* bias_spec, void* workspace, int64_t workspace_bytes, void* stream) {
    return denoiser_bias_spec((Denoiser*)handle, audio, n_dev, n, bias_spec, workspace, workspace_bytes,
                              (hipStream_t)stream);
}
int32_t ttsamd_denoise(void* handle, float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch,
                       int32_t n_max, const float* bias_spec, float strength, void* workspace,
                       int64_t workspace_bytes, void* stream) {
    return denoise((Denoiser*)handle, wave, wave_stride, nsamples, batch, n_max, bias_spec, strength, nullptr, workspace,
                   workspace_bytes, (hipStream_t)stream);
}
int32_t ttsamd_denoise_rows(void* handle, float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch,
                            int32_t n_max, const float* bias_spec, const float* strength_rows, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    TTS_REQUIRE(strength_rows, "denoise_rows: strength_rows is null");
    return denoise((Denoiser*)handle, wave, wave_stride, nsamples, batch, n_max, bias_spec, 0.f, strength_rows, workspace,
                   workspace_bytes, (hipStream_t)stream);
}

int32_t ttsamd_vocos_create(const ttsamd_tensor* weights, int32_t n, int32_t input_channels, int32_t dim,
                            int32_t intermediate_dim, int32_t num_layers, void** handle) {
    Vocos* h = nullptr;
    const int32_t rc = vocos_create(weights, n, input_channels, dim, intermediate_dim, num_layers, &h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_vocos_destroy(void* handle) {
    vocos_destroy((Vocos*)handle);
    return 0;
}
int64_t ttsamd_vocos_workspace_bytes(void* handle, int32_t batch, int32_t t_max) {
    if (!handle || batch < 1 || t_max < 1) return 0;
    const int64_t a = vocos_workspace_bytes((Vocos*)handle, batch, t_max), b = vocos_bias_workspace_bytes((Vocos*)handle);
    return a > b ? a : b;
}
int32_t ttsamd_vocos_bias_vec(void* handle, float* bias_vec, void* workspace, int64_t workspace_bytes, void* stream) {
    return vocos_bias_vec((Vocos*)handle, bias_vec, workspace, workspace_bytes, (hipStream_t)stream);
}
int32_t ttsamd_vocos_forward(void* handle, const float* mel, const int64_t* lens, int32_t batch, int32_t t_max,
                             float denoise, const float* bias_vec, float* wave, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    return vocos_forward((Vocos*)handle, mel, lens, batch, t_max, denoise, nullptr, bias_vec, wave, workspace, workspace_bytes,
                         (hipStream_t)stream);
}
int32_t ttsamd_vocos_forward_rows(void* handle, const float* mel, const int64_t* lens, int32_t batch, int32_t t_max,
                                  const float* denoise_rows, const float* bias_vec, float* wave, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    TTS_REQUIRE(denoise_rows, "vocos_forward_rows: denoise_rows is null");
    return vocos_forward((Vocos*)handle, mel, lens, batch, t_max, 0.f, denoise_rows, bias_vec, wave, workspace, workspace_bytes,
                         (hipStream_t)stream);
}

int32_t ttsamd_vocos_features(void* handle, const float* mel, const int64_t* lens, int32_t batch, int32_t t_max, float* out,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    return vocos_features_out((Vocos*)handle, mel, lens, batch, t_max, out, workspace, workspace_bytes, (hipStream_t)stream);
}
int32_t ttsamd_vocos_head(void* handle, const float* feats, const int64_t* lens, int32_t batch, int32_t t_max, const float* denoise_rows,
                          const float* bias_vec, float* wave, void* workspace, int64_t workspace_bytes, void* stream) {
    return vocos_head((Vocos*)handle, feats, lens, batch, t_max, denoise_rows, bias_vec, wave, workspace, workspace_bytes,
                      (hipStream_t)stream);
}
int32_t ttsamd_vocos_set_padding(void* handle, int32_t mode) { return vocos_set_padding((Vocos*)handle, mode); }

int32_t ttsamd_vocos_halo_frames(void* handle, int32_t* left, int32_t* right) {
    return vocos_halo_frames((Vocos*)handle, left, right);
}
int32_t ttsamd_vocos_forward_windows(void* handle, const float* mel, const int64_t* lens, int32_t n_windows, int32_t w_max,
                                     const int32_t* need_start, const int32_t* need_len, const float* denoise_rows, const float* bias_vec,
                                     float* wave, void* workspace, int64_t workspace_bytes, void* stream) {
    return vocos_forward_windows((Vocos*)handle, mel, lens, n_windows, w_max, need_start, need_len, denoise_rows, bias_vec, wave, workspace,
                                 workspace_bytes, (hipStream_t)stream);
}

int32_t ttsamd_melspec_create(const float* fbank, int32_t n_mels, int32_t n_fft, int32_t hop_length, int32_t framing,
                              int32_t mag_mode, float log_clip, void** handle) {
    TTS_REQUIRE(handle, "melspec_create: null handle");
    MelSpec* h = nullptr;
    const int32_t rc = melspec_create(fbank, n_mels, n_fft, hop_length, framing, mag_mode, log_clip, &h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_melspec_destroy(void* handle) {
    melspec_destroy((MelSpec*)handle);
    return 0;
}
int32_t ttsamd_melspec_forward(void* handle, const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch,
                               int32_t t_max, float* mel, int64_t* frames_out, void* stream) {
    return melspec_forward((const MelSpec*)handle, wave, wave_stride, nsamples, batch, t_max, mel, frames_out, (hipStream_t)stream);
}

int32_t ttsamd_cepstral_series(const float* mel, const int64_t* lens, int32_t batch, int32_t n_mels, int32_t t_max, int32_t center,
                               int32_t hann, int32_t q_c, float hqer_scale, float* power, float* series, void* stream) {
    return cepstral_series(mel, lens, batch, n_mels, t_max, center, hann, q_c, hqer_scale, power, series, (hipStream_t)stream);
}
int32_t ttsamd_cepstral_series_from_power(const float* power, const int64_t* lens, int32_t batch, int32_t n_q, int32_t t_max, int32_t q_c,
                                          int32_t q1, int32_t q2, double eps, double roll_p, float hqer_scale, float* series,
                                          void* stream) {
    return cepstral_series_from_power(power, lens, batch, n_q, t_max, q_c, q1, q2, eps, roll_p, hqer_scale, series, (hipStream_t)stream);
}
int32_t ttsamd_series_summary(const float* series, const int64_t* lens, int32_t batch, int32_t n_series, int32_t t_max, float* stats,
                              float* feat, void* stream) {
    return series_summary(series, lens, batch, n_series, t_max, stats, feat, (hipStream_t)stream);
}
int64_t ttsamd_dtw_workspace_bytes(int32_t batch, int32_t ta_max, int32_t tb_max, int32_t channels) {
    return dtw_workspace_bytes(batch, ta_max, tb_max, channels);
}
int32_t ttsamd_dtw(const float* a, const int64_t* lens_a, const float* b, const int64_t* lens_b, int32_t batch, int32_t channels,
                   int32_t ta_max, int32_t tb_max, int32_t metric, int32_t window, float* cost, int32_t* path, int32_t* path_len,
                   void* workspace, int64_t workspace_bytes, void* stream) {
    return dtw(a, lens_a, b, lens_b, batch, channels, ta_max, tb_max, metric, window, cost, path, path_len, workspace, workspace_bytes,
               (hipStream_t)stream);
}
int32_t ttsamd_dtw_aligned_mae(const float* pred, const float* ref, int32_t batch, int32_t ta_max, int32_t tb_max, const int32_t* path,
                               const int32_t* path_len, float* mae, void* stream) {
    return dtw_aligned_mae(pred, ref, batch, ta_max, tb_max, path, path_len, mae, (hipStream_t)stream);
}

int32_t ttsamd_mel_cepstrum(const float* logmel, const int64_t* lens, int32_t batch, int32_t n_mels, int32_t t_max, int32_t n_coef, float* cep,
                            void* stream) {
    return mel_cepstrum(logmel, lens, batch, n_mels, t_max, n_coef, cep, (hipStream_t)stream);
}
int32_t ttsamd_dtw_aligned_eval(const float* cep_a, const float* cep_b, int32_t n_coef, int32_t first_coef, const float* mel_a,
                                const float* mel_b, int32_t n_mels, const float* f0_a, const float* f0_b, int32_t batch, int32_t ta_max,
                                int32_t tb_max, const int32_t* path, const int32_t* path_len, double scale, double* stats, void* stream) {
    return dtw_aligned_eval(cep_a, cep_b, n_coef, first_coef, mel_a, mel_b, n_mels, f0_a, f0_b, batch, ta_max, tb_max, path, path_len, scale,
                            stats, (hipStream_t)stream);
}

int32_t ttsamd_aligner_create(const ttsamd_tensor* weights, int32_t n, const ttsamd_aligner_cfg* cfg, void** handle) {
    TTS_REQUIRE(handle, "aligner_create: null handle");
    Aligner* h = nullptr;
    const int32_t rc = aligner_create(weights, n, cfg, &h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_aligner_destroy(void* handle) {
    aligner_destroy((Aligner*)handle);
    return 0;
}
int64_t ttsamd_aligner_workspace_bytes(void* handle, int32_t batch, int32_t n_tokens, int32_t n_frames) {
    if (!handle || batch < 1 || n_tokens < 1 || n_frames < 1) return 0;
    return aligner_workspace_bytes((const Aligner*)handle, batch, n_tokens, n_frames);
}
int32_t ttsamd_aligner_forward(void* handle, const int64_t* ids, const int64_t* in_lens, const float* mel, const int64_t* mel_lens,
                               const float* attn_prior, int32_t batch, int32_t n_tokens, int32_t n_frames, float* attn_soft,
                               float* attn_logprob, void* workspace, int64_t workspace_bytes, void* stream) {
    return aligner_forward((const Aligner*)handle, ids, in_lens, mel, mel_lens, attn_prior, batch, n_tokens, n_frames, attn_soft, attn_logprob,
                           workspace, workspace_bytes, (hipStream_t)stream);
}
int64_t ttsamd_mas_workspace_bytes(int32_t batch, int32_t n_frames, int32_t n_tokens) { return mas_workspace_bytes(batch, n_frames, n_tokens); }
int32_t ttsamd_mas(const float* attn, int32_t is_log, const int64_t* in_lens, const int64_t* out_lens, int32_t batch, int32_t n_frames,
                   int32_t n_tokens, float* dur, float* attn_hard, void* workspace, int64_t workspace_bytes, void* stream) {
    return mas(attn, is_log, in_lens, out_lens, batch, n_frames, n_tokens, dur, attn_hard, workspace, workspace_bytes, (hipStream_t)stream);
}
int32_t ttsamd_attn_prior(const int64_t* in_lens, const int64_t* mel_lens, int32_t batch, int32_t n_tokens, int32_t n_frames, int32_t mode,
                          double scaling, void* out, void* stream) {
    return attn_prior(in_lens, mel_lens, batch, n_tokens, n_frames, mode, scaling, out, (hipStream_t)stream);
}
int32_t ttsamd_attn_prior_tables(int32_t n, double* lf) { return attn_prior_tables_host(n, lf); }
int64_t ttsamd_attn_ctc_loss_workspace_bytes(int32_t batch, int32_t n_frames, int32_t n_tokens) {
    return attn_ctc_workspace_bytes(batch, n_frames, n_tokens);
}
int32_t ttsamd_attn_ctc_loss(const float* attn_logprob, const int64_t* in_lens, const int64_t* out_lens, int32_t batch, int32_t n_frames,
                             int32_t n_tokens, double blank_logprob, double* nll, void* workspace, int64_t workspace_bytes, void* stream) {
    return attn_ctc_loss(attn_logprob, in_lens, out_lens, batch, n_frames, n_tokens, blank_logprob, nll, workspace, workspace_bytes,
                         (hipStream_t)stream);
}
int32_t ttsamd_attn_bin_loss(const float* attn_hard, const float* attn_soft, int32_t batch, int32_t n_frames, int32_t n_tokens, double eps,
                             double* sum_log, double* count, void* stream) {
    return attn_bin_loss(attn_hard, attn_soft, batch, n_frames, n_tokens, eps, sum_log, count, (hipStream_t)stream);
}
int32_t ttsamd_pyin_tables(const ttsamd_pyin_cfg* cfg, int32_t* dims, double* beta, double* expn, double* norm, double* trans,
                           float* logtrans, float* f0) {
    return pyin_tables_host(cfg, dims, beta, expn, norm, trans, logtrans, f0);
}
int32_t ttsamd_pyin_create(const ttsamd_pyin_cfg* cfg, void** handle) {
    TTS_REQUIRE(handle, "pyin_create: null handle");
    Pyin* h = nullptr;
    const int32_t rc = pyin_create(cfg, &h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_pyin_destroy(void* handle) {
    pyin_destroy((Pyin*)handle);
    return 0;
}
int64_t ttsamd_pyin_workspace_bytes(void* handle, int32_t batch, int32_t n_frames) {
    return pyin_workspace_bytes((const Pyin*)handle, batch, n_frames);
}
int32_t ttsamd_pyin_obs_offsets(void* handle, int32_t batch, int32_t n_frames, int64_t* obs_offsets) {
    return pyin_obs_offsets((const Pyin*)handle, batch, n_frames, obs_offsets);
}
int32_t ttsamd_pyin_forward(void* handle, const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, int32_t t_max,
                            float* f0, uint8_t* voiced_flag, double* voiced_prob, int32_t* states, int64_t* frames_out, void* workspace,
                            int64_t workspace_bytes, void* stream) {
    return pyin_forward((const Pyin*)handle, wave, wave_stride, nsamples, batch, t_max, f0, voiced_flag, voiced_prob, states, frames_out,
                        workspace, workspace_bytes, (hipStream_t)stream);
}
int32_t ttsamd_resample_create(const float* taps, int32_t o, int32_t n, int32_t width, void** handle) {
    TTS_REQUIRE(handle, "resample_create: null handle");
    Resample* h = nullptr;
    const int32_t rc = resample_create(taps, o, n, width, &h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_resample_destroy(void* handle) {
    resample_destroy((Resample*)handle);
    return 0;
}
int64_t ttsamd_resample_out_len(void* handle, int64_t nsamples) { return resample_out_len((const Resample*)handle, nsamples); }
int32_t ttsamd_resample_mfma_eligible(void* handle) { return resample_mfma_eligible((const Resample*)handle); }
int32_t ttsamd_resample_forward(void* handle, const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, float* out,
                                int64_t out_stride, int64_t* nout, int32_t route, void* stream) {
    return resample_forward((const Resample*)handle, wave, wave_stride, nsamples, batch, out, out_stride, nout, route, (hipStream_t)stream);
}
int64_t ttsamd_trim_workspace_bytes(int32_t batch, int64_t wave_stride, int32_t hop_length) {
    return trim_workspace_bytes(batch, wave_stride, hop_length);
}
int32_t ttsamd_trim_bounds(const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t batch, float top_db,
                           int32_t frame_length, int32_t hop_length, float gain, int64_t* bounds, float* peak, void* workspace,
                           int64_t workspace_bytes, void* stream) {
    return trim_bounds(wave, wave_stride, nsamples, batch, top_db, frame_length, hop_length, gain, bounds, peak, workspace, workspace_bytes,
                       (hipStream_t)stream);
}
int32_t ttsamd_trim_apply(const float* wave, int64_t wave_stride, const int64_t* bounds, const float* peak, float gain, int64_t tail,
                          int32_t batch, float* out, int64_t out_stride, int64_t* lens_out, void* stream) {
    return trim_apply(wave, wave_stride, bounds, peak, gain, tail, batch, out, out_stride, lens_out, (hipStream_t)stream);
}
int32_t ttsamd_frames_compact(const float* mel, const float* extra, const int64_t* lens, int32_t batch, int32_t n_channels,
                              int32_t n_extra, int32_t t_max, float thresh, float* mel_out, float* extra_out, int64_t* lens_out,
                              void* stream) {
    return frames_compact(mel, extra, lens, batch, n_channels, n_extra, t_max, thresh, mel_out, extra_out, lens_out, (hipStream_t)stream);
}
int32_t ttsamd_wave_join(const float* wave, int64_t wave_stride, const int64_t* nsamples, const int64_t* bounds, const int64_t* gap,
                         int32_t batch, const float* fade, int32_t n_fade, int64_t keep, int64_t lead, float* out, int64_t out_stride,
                         int64_t* segs, int64_t* total, void* stream) {
    return wave_join(wave, wave_stride, nsamples, bounds, gap, batch, fade, n_fade, keep, lead, out, out_stride, segs, total,
                     (hipStream_t)stream);
}
int32_t ttsamd_token_spans(const int64_t* reps, int64_t reps_stride, const int64_t* n_tokens, int32_t batch, int32_t max_tokens,
                           const int32_t* groups, const int32_t* n_groups, int32_t max_groups, int64_t hop, const int64_t* map,
                           int64_t* tok, int64_t* grp, void* stream) {
    return token_spans(reps, reps_stride, n_tokens, batch, max_tokens, groups, n_groups, max_groups, hop, map, tok, grp,
                       (hipStream_t)stream);
}
int32_t ttsamd_average_pitch(const float* pitch, const float* dur, int32_t batch, int32_t n_formants, int32_t n_frames, int32_t n_tokens,
                             float* out, void* stream) {
    return average_pitch(pitch, dur, batch, n_formants, n_frames, n_tokens, out, (hipStream_t)stream);
}

int32_t ttsamd_tacotron2_create(const ttsamd_tensor* weights, int32_t n, const ttsamd_tacotron2_cfg* cfg, void** handle) {
    TTS_REQUIRE(handle, "tacotron2_create: null handle");
    Taco2* h = nullptr;
    const int32_t rc = tacotron2_create(weights, n, cfg, &h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_tacotron2_destroy(void* handle) {
    tacotron2_destroy((Taco2*)handle);
    return 0;
}
int64_t ttsamd_tacotron2_workspace_bytes(void* handle, int32_t batch, int32_t n_tokens, int32_t max_step) {
    if (!handle || batch < 1 || n_tokens < 1 || max_step < 1) return 0;
    return tacotron2_workspace_bytes((Taco2*)handle, batch, n_tokens, max_step);
}
int32_t ttsamd_tacotron2_infer(void* handle, const int64_t* tokens, const int64_t* lengths, const int64_t* speaker_ids,
                               int32_t batch, int32_t n_tokens, int32_t max_step, int64_t dropout_seed, float* mel_post,
                               int32_t* mel_lens, float* alignments, float* mel_raw, int32_t* n_steps, void* workspace,
                               int64_t workspace_bytes, void* stream) {
    return tacotron2_infer((Taco2*)handle, tokens, lengths, speaker_ids, batch, n_tokens, max_step, dropout_seed, mel_post,
                           mel_lens, alignments, mel_raw, n_steps, workspace, workspace_bytes, (hipStream_t)stream);
}
int64_t ttsamd_tacotron2_stream_bytes(void* handle, int32_t batch, int32_t n_tokens, int32_t max_step, int32_t max_chunk_steps) {
    if (!handle || batch < 1 || n_tokens < 1 || max_step < 1 || max_chunk_steps < 8 || max_chunk_steps % 8 != 0) return 0;
    return tacotron2_stream_bytes((Taco2*)handle, batch, n_tokens, max_step, max_chunk_steps);
}
int32_t ttsamd_tacotron2_stream_begin(void* handle, const int64_t* tokens, const int64_t* lengths, const int64_t* speaker_ids, int32_t batch,
                                      int32_t n_tokens, int32_t max_step, int32_t max_chunk_steps, int64_t dropout_seed,
                                      const int32_t* cut_columns, int32_t rows_to_batch_end, float* mel_raw, int32_t* mel_lens,
                                      float* alignments, void* workspace, int64_t workspace_bytes, void** session, void* stream) {
    TTS_REQUIRE(session, "tacotron2_stream_begin: null session");
    TacoStream* st = nullptr;
    const int32_t rc = tacotron2_stream_begin((Taco2*)handle, tokens, lengths, speaker_ids, batch, n_tokens, max_step, max_chunk_steps,
                                              dropout_seed, cut_columns, rows_to_batch_end, mel_raw, mel_lens, alignments, workspace,
                                              workspace_bytes, &st, (hipStream_t)stream);
    if (rc == 0) *session = st;
    return rc;
}
int32_t ttsamd_tacotron2_stream_advance(void* session, int32_t n_steps, int32_t* steps_done, int32_t* ended, int32_t* rows, void* stream) {
    return tacotron2_stream_advance((TacoStream*)session, n_steps, steps_done, ended, rows, (hipStream_t)stream);
}
int32_t ttsamd_tacotron2_stream_end(void* session) {
    tacotron2_stream_end((TacoStream*)session);
    return 0;
}
int32_t ttsamd_tacotron2_postnet_halo_frames(void* handle, int32_t* halo) {
    TTS_REQUIRE(handle && halo, "tacotron2_postnet_halo_frames: null argument");
    *halo = tacotron2_postnet_halo((Taco2*)handle);
    return 0;
}
int64_t ttsamd_tacotron2_postnet_window_bytes(void* handle, int32_t batch, int32_t n_frames) {
    if (!handle || batch < 1 || n_frames < 1) return 0;
    return tacotron2_postnet_window_bytes((Taco2*)handle, batch, n_frames);
}
int32_t ttsamd_tacotron2_postnet_window(void* handle, const float* mel_raw, float* mel_post, int32_t batch, int32_t t_cap, int32_t t_known,
                                        int32_t t0, int32_t t1, int32_t ended, void* workspace, int64_t workspace_bytes, void* stream) {
    return tacotron2_postnet_window((Taco2*)handle, mel_raw, mel_post, batch, t_cap, t_known, t0, t1, ended, workspace, workspace_bytes,
                                    (hipStream_t)stream);
}

int32_t ttsamd_tagger_create(const ttsamd_tensor* weights, int32_t n, const ttsamd_tagger_cfg* cfg, void** handle) {
    TTS_REQUIRE(handle, "tagger_create: null handle");
    Tagger* h = nullptr;
    const int32_t rc = tagger_create(weights, n, cfg, &h);
    if (rc == 0) *handle = h;
    return rc;
}
int32_t ttsamd_tagger_destroy(void* handle) {
    tagger_destroy((Tagger*)handle);
    return 0;
}
int64_t ttsamd_tagger_workspace_bytes(void* handle, int32_t batch, int32_t n_chars) {
    if (!handle || batch < 1 || n_chars < 1) return 0;
    return tagger_workspace_bytes((Tagger*)handle, batch, n_chars);
}
int32_t ttsamd_tagger_forward(void* handle, const int64_t* ids, int32_t batch, int32_t n_chars, float* probs,
                              void* workspace, int64_t workspace_bytes, void* stream) {
    return tagger_forward((Tagger*)handle, ids, batch, n_chars, probs, workspace, workspace_bytes, (hipStream_t)stream);
}

int64_t ttsamd_conv1d_packed_floats(int32_t cout, int32_t cin, int32_t k) {
    // fp32 packed + bf16 hi/lo planes (+ k = 3 / 7 / 11: the Winograd group filters, conv_wino.hip / conv_wino2.hip / conv_wino4.hip:
    // F(2,3), F(4,3) six-point and -- k = 7 / 11 -- seven-point)
    return 2 * (int64_t)cin * k * cout_padded(cout) +
           ((k == 3 || k == 7 || k == 11) ? (int64_t)cin * (wino2_groups(k) + wino4_groups(k) + wino44_groups(k)) * cout_padded(cout) : 0);
}

// [Cout][Cin][k] -> the F(4,3) group filters in the packed layout [cin/8][NGQ][2][cp][4] (same values as pack_wino4_weight, conv_wino4.hip)
__global__ void pack_wino4_weight_kernel(const float* __restrict__ w, int cout, int cin, int k, int cp, float* __restrict__ out) {
    const int ng = k == 3 ? 6 : (k == 7 ? 16 : 24), nsf = k == 3 ? 1 : (k == 7 ? 2 : 4);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)cin * ng * cp;
    if (i >= n) return;
    const int pq = (int)(i & 3);
    const int64_t r = i >> 2;
    const int co = (int)(r % cp);
    const int64_t r2 = r / cp;
    const int kk = (int)(r2 & 1);
    const int64_t r3 = r2 >> 1;
    const int t = (int)(r3 % ng), o = (int)(r3 / ng);
    float v = 0.f;
    if (co < cout) {
        const float* g = w + ((int64_t)co * cin + (8 * o + 2 * pq + kk)) * k;
        if (t < 6 * nsf) {
            const int s = t / 6, j = t % 6;
            const double g0 = g[3 * s], g1 = 3 * s + 1 < k ? g[3 * s + 1] : 0.0, g2 = 3 * s + 2 < k ? g[3 * s + 2] : 0.0;
            v = j == 0 ? (float)(g0 / 4) : (j == 1 ? (float)(-(g0 + g1 + g2) / 6) : (j == 2 ? (float)(-(g0 - g1 + g2) / 6) :
                (j == 3 ? (float)(g0 / 24 + g1 / 12 + g2 / 6) : (j == 4 ? (float)(g0 / 24 - g1 / 12 + g2 / 6) : (float)g2))));
        } else {
            v = g[6];                       // k = 7: the single tap, four copies (planes P0 / P6 / P7 / P5)
        }
    }
    out[i] = v;
}

// [Cout][Cin][k], k = 7 / 11 -> the seven-point group filters in the packed layout [cin/8][NG][2][cp][4] (same values as pack_wino44_weight,
// conv_wino4.hip: sub-filter s = taps 4 s .. 4 s + 3, the last one has three taps and no U6)
__global__ void pack_wino44_weight_kernel(const float* __restrict__ w, int cout, int cin, int k, int cp, float* __restrict__ out) {
    const int ng = k == 7 ? 13 : 20;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)cin * ng * cp;
    if (i >= n) return;
    const int pq = (int)(i & 3);
    const int64_t r = i >> 2;
    const int co = (int)(r % cp);
    const int64_t r2 = r / cp;
    const int kk = (int)(r2 & 1);
    const int64_t r3 = r2 >> 1;
    const int t = (int)(r3 % ng), o = (int)(r3 / ng);
    float v = 0.f;
    if (co < cout) {
        const float* g = w + ((int64_t)co * cin + (8 * o + 2 * pq + kk)) * k;
        const int s = t / 7, j = t % 7;
        const double g0 = g[4 * s], g1 = g[4 * s + 1], g2 = g[4 * s + 2], g3 = 4 * s + 3 < k ? g[4 * s + 3] : 0.0;
        v = j == 0 ? (float)(g0 / 4) : (j == 1 ? (float)((g0 + g1 + g2 + g3) / 6) : (j == 2 ? (float)((g0 - g1 + g2 - g3) / 18) :
            (j == 3 ? (float)((g0 + 2 * g1 + 4 * g2 + 8 * g3) / 72) : (j == 4 ? (float)((g0 - 2 * g1 + 4 * g2 - 8 * g3) / 120) :
            (j == 5 ? (float)((32 * g0 + 16 * g1 + 8 * g2 + 4 * g3) / 45) : (float)(g3 / 2))))));
    }
    out[i] = v;
}

// [Cout][Cin][k] -> the Winograd group filters in the packed NG-tap layout [cin/8][NG][2][cp][4] (same values as pack_wino2_weight:
// sub-filter s: g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2; single tap t: g_t, -g_t)
__global__ void pack_wino2_weight_kernel(const float* __restrict__ w, int cout, int cin, int k, int cp, float* __restrict__ out) {
    const int ns = k / 3, ng = 4 * ns + 2 * (k - 3 * ns);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = (int64_t)cin * ng * cp;
    if (i >= n) return;
    const int pq = (int)(i & 3);
    const int64_t r = i >> 2;
    const int co = (int)(r % cp);
    const int64_t r2 = r / cp;
    const int kk = (int)(r2 & 1);
    const int64_t r3 = r2 >> 1;
    const int t = (int)(r3 % ng), o = (int)(r3 / ng);
    float v = 0.f;
    if (co < cout) {
        const float* g = w + ((int64_t)co * cin + (8 * o + 2 * pq + kk)) * k;
        if (t < 4 * ns) {
            const int s = t >> 2, j = t & 3;
            const double g0 = g[3 * s], g1 = g[3 * s + 1], g2 = g[3 * s + 2];
            v = j == 0 ? (float)g0 : (j == 1 ? (float)((g0 + g1 + g2) * 0.5) : (j == 2 ? (float)((g0 - g1 + g2) * 0.5) : (float)g2));
        } else {
            const int l = (t - 4 * ns) >> 1;
            v = ((t - 4 * ns) & 1) ? -g[3 * ns + l] : g[3 * ns + l];
        }
    }
    out[i] = v;
}

int32_t ttsamd_conv1d_ex(const float* x, const float* w, const float* bias, const float* res, const int64_t* lens, int32_t batch,
                         int32_t cin, int32_t cout, int32_t k, int32_t dilation, int32_t lin, float in_slope,
                         int32_t relu_out, int32_t mode, float div, float* y, float* packed, void* stream) {
    return ttsamd_conv1d_splitk(x, w, bias, res, lens, batch, cin, cout, k, dilation, lin, in_slope, relu_out, mode, div, y, packed, nullptr,
                                0, stream);
}

// The ConvParams of a ttsamd_conv1d_splitk call, shared with ttsamd_conv1d_route so that both route the same launch.  The forms a launch
// carries sit in `packed` one behind the other (ttsamd_conv1d_packed_floats): direct | bf16 planes | F(2,3) | F(4,3) | seven-point groups.
static int32_t conv1d_params(ConvParams& p, const float* x, const float* bias, const float* res, const int64_t* lens, int32_t batch,
                             int32_t cin, int32_t cout, int32_t k, int32_t dilation, int32_t lin, float in_slope, int32_t relu_out,
                             int32_t mode, float div, float* y, float* packed, float* splitk_ws, int64_t splitk_floats) {
    TTS_REQUIRE(mode >= 0 && mode <= 2 && (mode != 2 || div != 0.f), "conv1d: bad mode / div");
    // the residual-preload epilogues apply the activation to y_prev + res + conv + b: only mode 0 has the documented meaning with relu_out
    TTS_REQUIRE(relu_out == 0 || mode == 0, "conv1d: relu_out with an accumulate mode (mode %d) is not defined", mode);
    const int cp = cout_padded(cout);
    const int64_t n = (int64_t)cin * k * cp;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.x_bs = (int64_t)cin * lin; p.x_cs = lin;
    p.w = packed; p.bias = bias;
    p.precision = default_precision();
    if (p.precision != 0) p.w_bf16 = packed + n;
    if ((k == 3 || k == 7 || k == 11) && p.precision == 0 && cin % 8 == 0) {
        p.w_wino = packed + 2 * n;
        p.w_wino4 = p.w_wino + (int64_t)cin * wino2_groups(k) * cp;
        if (wino44_groups(k) != 0) p.w_wino44 = p.w_wino4 + (int64_t)cin * wino4_groups(k) * cp;
    }
    p.y = y; p.y_bs = (int64_t)cout * lin; p.y_cs = lin; p.y_ts = 1;
    p.lens_in = lens; p.lens_out = lens; p.len_in_mul = 1; p.len_out_mul = 1;
    p.Lin = lin; p.Nout = lin; p.Cin = cin; p.Cout = cout; p.CoutP = cp; p.K = k;
    p.dil = dilation; p.pad = (k * dilation - dilation) / 2;
    p.res = res; p.r_bs = (int64_t)cout * lin; p.r_cs = lin;
    p.n_phase = 1; p.in_slope = in_slope; p.relu_out = relu_out; p.mode = mode; p.div = div; p.batch = batch;
    if (splitk_ws != nullptr && splitk_floats > 0) { p.splitk_ws = splitk_ws; p.splitk_floats = splitk_floats; }
    return 0;
}

int32_t ttsamd_conv1d_splitk(const float* x, const float* w, const float* bias, const float* res, const int64_t* lens, int32_t batch,
                             int32_t cin, int32_t cout, int32_t k, int32_t dilation, int32_t lin, float in_slope,
                             int32_t relu_out, int32_t mode, float div, float* y, float* packed, float* splitk_ws, int64_t splitk_floats,
                             void* stream) {
    TTS_REQUIRE(x && w && y && packed, "conv1d: null argument");
    TTS_REQUIRE(splitk_floats >= 0 && (splitk_ws != nullptr || splitk_floats == 0), "conv1d: %lld split-K floats without a workspace",
                (long long)splitk_floats);
    ConvParams p;
    TTS_TRY(conv1d_params(p, x, bias, res, lens, batch, cin, cout, k, dilation, lin, in_slope, relu_out, mode, div, y, packed, splitk_ws,
                          splitk_floats));
    hipStream_t s = (hipStream_t)stream;
    const int cp = p.CoutP;
    const int64_t n = (int64_t)cin * k * cp;
    const auto blocks = [](int64_t floats) { return dim3((unsigned)((floats + 255) / 256)); };
    hipLaunchKernelGGL(pack_conv_weight_kernel, blocks(n), dim3(256), 0, s, w, cout, cin, k, cp, packed);
    TTS_CHECK_HIP(hipGetLastError());
    if (p.w_bf16 != nullptr) {
        hipLaunchKernelGGL(split_bf16_kernel, blocks(n), dim3(256), 0, s, packed, n, reinterpret_cast<unsigned short*>(packed + n));
        TTS_CHECK_HIP(hipGetLastError());
    }
    if (p.w_wino != nullptr) {
        hipLaunchKernelGGL(pack_wino2_weight_kernel, blocks((int64_t)cin * wino2_groups(k) * cp), dim3(256), 0, s, w, cout, cin, k, cp,
                           const_cast<float*>(p.w_wino));
        TTS_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(pack_wino4_weight_kernel, blocks((int64_t)cin * wino4_groups(k) * cp), dim3(256), 0, s, w, cout, cin, k, cp,
                           const_cast<float*>(p.w_wino4));
        TTS_CHECK_HIP(hipGetLastError());
    }
    if (p.w_wino44 != nullptr) {
        hipLaunchKernelGGL(pack_wino44_weight_kernel, blocks((int64_t)cin * wino44_groups(k) * cp), dim3(256), 0, s, w, cout, cin, k, cp,
                           const_cast<float*>(p.w_wino44));
        TTS_CHECK_HIP(hipGetLastError());
    }
    prof_begin(s, 2.0 * cout * cin * k);
    const int32_t rc = launch_conv(p, s);
    prof_end(s);
    return rc;
}

int32_t ttsamd_conv1d_route(int32_t batch, int32_t cin, int32_t cout, int32_t k, int32_t dilation, int32_t lin, float in_slope,
                            int32_t relu_out, int32_t has_res, int32_t mode, int64_t splitk_floats, int32_t* route, int32_t* ksplit) {
    TTS_REQUIRE(route && ksplit, "conv1d_route: null argument");
    TTS_REQUIRE(batch >= 1 && cin >= 1 && cout >= 1 && k >= 1 && lin >= 1 && dilation >= 1 && dilation <= 5 && splitk_floats >= 0,
                "conv1d_route: bad shape");
    float* const any = reinterpret_cast<float*>((uintptr_t)256);   // stands for every buffer: 16-byte aligned, never followed
    ConvParams p;
    TTS_TRY(conv1d_params(p, any, any, has_res ? any : nullptr, nullptr, batch, cin, cout, k, dilation, lin, in_slope, relu_out, mode, 1.f, any,
                          any, any, splitk_floats));
    TTS_REQUIRE(p.precision == 0, "conv1d_route: the bf16 launchers keep their own choices (precision %d)", p.precision);
    const ConvRoute r = conv_route(p, conv_route_opts());
    TTS_REQUIRE(r.id >= 0 && (relu_out < 2 || k == 1 || k == 5), "conv1d_route: no fp32 kernel takes k = %d, Cin = %d, relu_out = %d", k, cin, relu_out);
    *route = r.id;
    *ksplit = r.ksplit;
    return 0;
}

int32_t ttsamd_conv1d(const float* x, const float* w, const float* bias, const int64_t* lens, int32_t batch,
                      int32_t cin, int32_t cout, int32_t k, int32_t dilation, int32_t lin, float in_slope,
                      int32_t relu_out, float* y, float* packed, void* stream) {
    return ttsamd_conv1d_ex(x, w, bias, nullptr, lens, batch, cin, cout, k, dilation, lin, in_slope, relu_out, 0, 1.f, y, packed, stream);
}

int32_t ttsamd_conv_last_launch(int32_t* route, int32_t* ksplit) {
    TTS_REQUIRE(route && ksplit, "conv_last_launch: null argument");
    last_conv_launch(route, ksplit);
    return 0;
}

int64_t ttsamd_convt_packed_floats(int32_t cin, int32_t cout, int32_t u) {
    // the u polyphase 2-tap filters in fp32 + their bf16 hi / lo planes
    // ... and, where the F(4,2) launch exists (convt_wino_packable), its six group filters per tap pair and the bias per row
    if (cin < 1 || cout < 1 || u < 1) return 0;
    return 2 * (int64_t)u * cin * 2 * cout_padded(cout) + (convt_wino_packable(cin, cout, u) ? (int64_t)(6 * cin + 1) * u * cout : 0);
}

int64_t ttsamd_convt_wino_packed_floats(int32_t cin, int32_t cout, int32_t u) {
    return convt_wino_packable(cin, cout, u) ? (int64_t)(6 * cin + 1) * u * cout : 0;
}

int32_t ttsamd_convt_wino_pack_weight(const float* w, const float* bias, int32_t cin, int32_t cout, int32_t u, float* out) {
    TTS_REQUIRE(w && out, "convt_wino_pack_weight: null argument");
    TTS_REQUIRE(convt_wino_packable(cin, cout, u), "convt_wino_pack_weight: cin %d (a multiple of 16), cout %d, u %d (2 / 8, u cout a multiple of 64)",
                cin, cout, u);
    pack_convt_wino_weight(w, bias, cin, cout, u, out, out + (int64_t)6 * cin * u * cout);
    return 0;
}

int32_t ttsamd_conv_transpose1d(const float* x, const float* w, const float* bias, const int64_t* lens, int32_t batch, int32_t cin,
                                int32_t cout, int32_t u, int32_t lin, float in_slope, float* y, float* packed, void* stream) {
    TTS_REQUIRE(x && w && y && packed, "conv_transpose1d: null argument");
    TTS_REQUIRE(batch >= 1 && cin >= 8 && cin % 8 == 0 && cout >= 1 && lin >= 1, "conv_transpose1d: batch %d, cin %d (a multiple of 8), cout %d, lin %d",
                batch, cin, cout, lin);
    TTS_REQUIRE(u >= 2 && u % 2 == 0, "conv_transpose1d: stride %d (kernel 2 u, padding u / 2: u even)", u);
    TTS_REQUIRE((int64_t)lin * u < ((int64_t)1 << 31) / 4 / cout, "conv_transpose1d: %d x %d x %d outputs per row", cout, lin, u);
    hipStream_t s = (hipStream_t)stream;
    const int cp = cout_padded(cout);
    const int64_t n = (int64_t)u * cin * 2 * cp;
    hipLaunchKernelGGL(pack_convt_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w, cin, cout, u, cp, packed);
    TTS_CHECK_HIP(hipGetLastError());
    unsigned short* planes = nullptr;
    if (default_precision() != 0) {
        planes = reinterpret_cast<unsigned short*>(packed + n);
        hipLaunchKernelGGL(split_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, packed, n, planes);
        TTS_CHECK_HIP(hipGetLastError());
    }
    float* wino = nullptr;
    if (default_precision() == 0 && convt_wino_packable(cin, cout, u) && opt_int(OPT_CONVT_WINO, 1) != 0) {
        wino = packed + 2 * n;
        const int64_t nw = (int64_t)(6 * cin + 1) * u * cout;
        hipLaunchKernelGGL(pack_convt_wino_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, w, bias, cin, cout, u, wino);
        TTS_CHECK_HIP(hipGetLastError());
    }
    ConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.batch = batch;
    p.lens_in = lens; p.lens_out = lens;
    prof_begin(s, 2.0 * cout * cin * 2 * u);
    const int32_t rc = launch_upsampler(p, x, packed, planes, bias, y, cin, cout, u, 2 * u, lin, 1, in_slope, opt_int(OPT_CONVT, 1) != 0, s, wino,
                                        wino ? wino + (int64_t)6 * cin * u * cout : nullptr);
    prof_end(s);
    return rc;
}

int64_t ttsamd_resblock_pair_packed_floats(int32_t channels, int32_t k, int32_t variant) {
    // the two direct packings + (variant 4: conv 2, variant 5: both convs) as Winograd F(2,3) groups
    if (channels < 1 || k < 1) return 0;
    const int64_t n = 2 * (int64_t)channels * k * channels;
    const int nwino = (variant == 4 ? 1 : (variant == 5 ? 2 : 0));
    if (variant == 6) return n + ((k == 3 || k == 7 || k == 11) ? 2 * (int64_t)channels * wino4_groups(k) * channels : 0);   // both convs as F(4,3) groups
    if (variant == 7) return n + 2 * (int64_t)channels * wino44_groups(k) * channels;                                         // ... as seven-point groups
    return n + ((k == 3 || k == 7 || k == 11) ? nwino * (int64_t)channels * wino2_groups(k) * channels : 0);
}

int32_t ttsamd_resblock_pair(const float* x, float* y, const float* w1, const float* b1, const float* w2, const float* b2,
                             int32_t channels, int32_t k, int32_t dil, const int64_t* lens, int32_t len_mul, int32_t L,
                             int32_t batch, int32_t mode, float div, float slope, int32_t variant, float* packed, int64_t packed_floats,
                             void* stream) {
    TTS_REQUIRE(x && y && w1 && b1 && w2 && b2 && packed && channels % 32 == 0 && k >= 1 && batch >= 1 && L >= 1 && len_mul >= 1 &&
                mode >= 0 && mode <= 2, "resblock_pair: bad argument");
    TTS_REQUIRE(packed_floats >= ttsamd_resblock_pair_packed_floats(channels, k, variant),
                "resblock_pair: `packed` holds %lld floats, variant %d at C = %d, k = %d needs %lld (ttsamd_resblock_pair_packed_floats)",
                (long long)packed_floats, variant, channels, k, (long long)ttsamd_resblock_pair_packed_floats(channels, k, variant));
    hipStream_t s = (hipStream_t)stream;
    // every form the variant reads, re-laid out on the device into `packed` one behind the other: the two direct packings, then the
    // variant's group filters; then its route through the dispatch hifigan_forward uses
    PairConv c[2] = {{nullptr, b1, nullptr, nullptr, nullptr}, {nullptr, b2, nullptr, nullptr, nullptr}};
    float* next = packed;
    const auto pack = [&](void (*kernel)(const float*, int, int, int, int, float*), int groups, const float* w, const float*& form) {
        const int64_t nw = (int64_t)channels * groups * channels;
        hipLaunchKernelGGL(kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, w, channels, channels, k, channels, next);
        form = next;
        next += nw;
        return hipGetLastError();
    };
    TTS_CHECK_HIP(pack(pack_conv_weight_kernel, k, w1, c[0].w));
    TTS_CHECK_HIP(pack(pack_conv_weight_kernel, k, w2, c[1].w));
    prof_begin(s, 2.0 * (2.0 * channels * channels * k));
    int32_t rc = 0;
    if (variant == 4 || variant == 5) {       // 256-column blocks with phase B (4) or both phases (5) on Winograd F(2,3): conv 2's groups, then conv 1's
        TTS_REQUIRE((k == 3 || k == 7 || k == 11) && (channels <= 64 || (variant == 5 && channels == 128)),
                    "resblock_pair: variants 4 / 5 are built for C = 32 / 64 (5: and 128), k = 3 / 7 / 11");
        TTS_CHECK_HIP(pack(pack_wino2_weight_kernel, wino2_groups(k), w2, c[1].w_wino2));
        if (variant == 5) TTS_CHECK_HIP(pack(pack_wino2_weight_kernel, wino2_groups(k), w1, c[0].w_wino2));
    } else if (variant == 6) {                // C = 32, both convs on Winograd F(4,3) (resblock_pair4.hip)
        TTS_REQUIRE(channels == 32 && (k == 3 || k == 7 || k == 11), "resblock_pair: variant 6 is built for C = 32, k = 3 / 7 / 11");
        TTS_CHECK_HIP(pack(pack_wino4_weight_kernel, wino4_groups(k), w1, c[0].w_wino4));
        TTS_CHECK_HIP(pack(pack_wino4_weight_kernel, wino4_groups(k), w2, c[1].w_wino4));
    } else if (variant == 7) {                // ... both convs on seven-point groups (13 / 20 products per quad)
        TTS_REQUIRE(channels == 32 && (k == 7 || k == 11), "resblock_pair: variant 7 is built for C = 32, k = 7 / 11");
        TTS_CHECK_HIP(pack(pack_wino44_weight_kernel, wino44_groups(k), w1, c[0].w_wino44));
        TTS_CHECK_HIP(pack(pack_wino44_weight_kernel, wino44_groups(k), w2, c[1].w_wino44));
    } else if (variant != -1 && (variant < 1 || variant > 3)) {
        set_error("resblock_pair: variant %d (1: first generation, 2 / 3: second generation with 256- / 128-column blocks, 4 / 5: 256 columns + Winograd phase B / both phases, 6: C = 32 with both phases on Winograd F(4,3), 7: ... on its seven-point groups, k = 7 / 11)", variant);
        rc = TTSAMD_EINVAL;
    }
    // (variant -1: the two weight re-layout launches only -- tools/fused_pair_bench.py subtracts them)
    if (rc == 0 && variant != -1)
        rc = launch_pair(pair_route_of_variant(variant, channels, dil),
                         PairArgs{channels, k, dil, x, y, c[0], c[1], lens, len_mul, L, batch, mode, div, slope}, s);
    prof_end(s);
    return rc;
}

int32_t ttsamd_resblock_pair_route(int32_t batch, int32_t channels, int32_t k, int32_t dilation, int32_t L, int32_t* kernel, int32_t* ntw,
                                   int32_t* wino_phases, int32_t* points, const char** name) {
    TTS_REQUIRE(kernel && ntw && wino_phases && points && name, "resblock_pair_route: null argument");
    TTS_REQUIRE(batch >= 1 && channels >= 1 && k >= 1 && dilation >= 1 && L >= 1, "resblock_pair_route: bad shape");
    float* const any = reinterpret_cast<float*>((uintptr_t)256);   // stand for the two buffers: 16-byte aligned, distinct, never followed
    const PairRoute r = pair_route(PairShape{channels, k, dilation, L, batch, true, any, any + 64, hifigan_conv_forms(channels, channels, k),
                                             default_precision()}, pair_route_opts());
    *kernel = r.kernel; *ntw = r.ntw; *wino_phases = r.wm; *points = r.points; *name = r.name;
    return 0;
}

int64_t ttsamd_resblock2_packed_floats(int32_t channels, int32_t k, int32_t variant) {
    // the two direct packings (both variants read the same layout)
    if (channels < 1 || k < 1 || (variant != 1 && variant != 2)) return 0;
    return 2 * (int64_t)channels * k * channels;
}

int32_t ttsamd_resblock2(const float* x, float* y, const float* w1, const float* b1, const float* w2, const float* b2, int32_t channels,
                         int32_t k, int32_t dil1, int32_t dil2, const int64_t* lens, int32_t len_mul, int32_t L, int32_t batch, int32_t mode,
                         float div, float slope, int32_t variant, float* packed, int64_t packed_floats, void* stream) {
    TTS_REQUIRE(x && y && w1 && b1 && w2 && b2 && packed && channels % 32 == 0 && channels >= 32 && k >= 1 && batch >= 1 && L >= 1 &&
                len_mul >= 1 && mode >= 0 && mode <= 2 && x != y, "resblock2: bad argument");
    TTS_REQUIRE(variant == 1 || variant == 2, "resblock2: variant %d (1: two single-conv launches, 2: both convs in one launch)", variant);
    TTS_REQUIRE(packed_floats >= ttsamd_resblock2_packed_floats(channels, k, variant),
                "resblock2: `packed` holds %lld floats, C = %d, k = %d needs %lld (ttsamd_resblock2_packed_floats)", (long long)packed_floats,
                channels, k, (long long)ttsamd_resblock2_packed_floats(channels, k, variant));
    if (variant == 1) {
        TTS_REQUIRE(resblock2_conv_supported(channels, k, dil1, L, x, y) && resblock2_conv_supported(channels, k, dil2, L, x, y),
                    "resblock2: variant 1 does not cover C = %d, k = %d, dilations %d / %d (C = 32 / 64 / 128, k = 3 / 5 / 7 / 11, "
                    "dilation 1..16)", channels, k, dil1, dil2);
    } else {
        TTS_REQUIRE(resblock2_pair_supported(channels, k, dil1, dil2, L, x, y),
                    "resblock2: variant 2 does not cover C = %d, k = %d, dilations %d / %d (C = 32 / 64, k = 3 / 5 / 7 / 11, dilation "
                    "1..16, (k - 1) * dil2 <= 256)", channels, k, dil1, dil2);
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t n = (int64_t)channels * k * channels;
    for (int i = 0; i < 2; ++i) {
        hipLaunchKernelGGL(pack_conv_weight_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, i == 0 ? w1 : w2, channels,
                           channels, k, channels, packed + i * n);
        TTS_CHECK_HIP(hipGetLastError());
    }
    prof_begin(s, 2.0 * (2.0 * channels * channels * k));
    int32_t rc;
    if (variant == 2) {
        rc = launch_resblock2_pair(channels, x, y, packed, b1, packed + n, b2, k, dil1, dil2, lens, len_mul, L, batch, mode, div, slope, s);
    } else {
        // x1 goes through a stream-ordered temporary of B * C * L floats
        float* x1 = nullptr;
        TTS_CHECK_HIP(hipMallocAsync((void**)&x1, (size_t)batch * channels * L * sizeof(float), s));
        rc = launch_resblock2_conv(channels, x, x1, packed, b1, k, dil1, lens, len_mul, L, batch, 0, 1.f, slope, s);
        if (rc == 0) rc = launch_resblock2_conv(channels, x1, y, packed + n, b2, k, dil2, lens, len_mul, L, batch, mode, div, slope, s);
        const hipError_t e = hipFreeAsync(x1, s);
        if (rc == 0 && e != hipSuccess) {
            set_error("resblock2: hipFreeAsync failed: %s", hipGetErrorString(e));
            rc = TTSAMD_EHIP;
        }
    }
    prof_end(s);
    return rc;
}

int32_t ttsamd_set_precision(int32_t precision) {
    TTS_REQUIRE(precision >= 0 && precision <= 2, "set_precision: 0 = fp32 MFMA, 1 = bf16 MFMA, 2 = split-bf16 MFMA");
    g_precision = precision;
    return 0;
}
int32_t ttsamd_get_precision(void) { return g_precision; }

int32_t ttsamd_profile_enable(int32_t on) {
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.on = on != 0;
    g_prof.used = 0;
    g_prof.launches = 0;
    g_prof.flops_per_frame = 0.0;
    return 0;
}

int32_t ttsamd_profile_read(double* out3) {
    TTS_REQUIRE(out3, "profile_read: null argument");
    std::lock_guard<std::mutex> lk(g_prof.mu);
    // busy time of the conv engine = length of the UNION of the sections' intervals: on one stream the sections follow each
    // other (union = sum); with the acoustic model of batch i + 1 on a second stream under the vocoder of batch i
    // (ttsamd.pipeline) they overlap, and a sum would count the shared time twice
    std::vector<std::pair<float, float>> iv;
    for (size_t i = 0; i + 1 < g_prof.used; i += 2) {
        TTS_CHECK_HIP(hipEventSynchronize(g_prof.ev[i + 1]));
        float t0 = 0.f, t1 = 0.f;
        if (i > 0) TTS_CHECK_HIP(hipEventElapsedTime(&t0, g_prof.ev[0], g_prof.ev[i]));
        TTS_CHECK_HIP(hipEventElapsedTime(&t1, g_prof.ev[0], g_prof.ev[i + 1]));
        iv.emplace_back(t0, std::max(t0, t1));
    }
    std::sort(iv.begin(), iv.end());
    double ms = 0.0;
    float lo = 0.f, hi = -1.f;
    for (const auto& v : iv) {
        if (hi < lo || v.first > hi) {
            if (hi >= lo) ms += hi - lo;
            lo = v.first;
            hi = v.second;
        } else {
            hi = std::max(hi, v.second);
        }
    }
    if (hi >= lo) ms += hi - lo;
    out3[0] = ms;
    out3[1] = (double)g_prof.launches;
    out3[2] = (double)(g_prof.used / 2);
    return 0;
}

}  // extern "C"
