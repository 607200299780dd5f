// HiFi-GAN generator on the MFMA conv engine: handle creation (weight-norm fold, weight
// re-layout, upload) and the batched ragged forward.
// Replaces vocoder.load_hifigan (vocoder/__init__.py:3-20) and Generator.forward
// (vocoder/hifigan/models.py:111-127) incl. ResBlock1.forward (:46-53) and, for V3 configs (resblock "2"),
// ResBlock2.forward (:62-83) on resblock2.hip (fp32 only).
#include <cmath>
#include <cstring>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "bfo.hpp"

namespace ttsamd {

// ResBlock2 (V3) routing: which (C, k) go out as ONE resblock2_pair launch instead of two resblock2_conv launches.  Bit 3 ci + ki,
// ci = 0 / 1 for C = 32 / 64, ki = 0 / 1 / 2 for k = 3 / 5 / 7; TTSAMD_RESBLOCK2_PAIR (hex) replaces the default, read per call.
// Default none: same-run A/B of the V3 vocoder (tools/hifigan_v3_bench.py, profiles/r7/hifigan_v3_bench.jsonl) with every pair fused
// (3f) against none (0): batch 1 0.975 vs 0.894 ms, batch 8 2.91 vs 2.58, batch 32 10.38 vs 8.82.  The fused launch writes the stage
// sum, so on three streams it waits for the previous branch as a whole, where two conv launches overlap conv 1 of all branches
// (per launch the fused kernel is the faster one).
constexpr unsigned kResblock2PairMask = 0x00;

static bool resblock2_pair_choice(unsigned mask, int32_t channels, int32_t k, int32_t d1, int32_t d2, int32_t L, const float* x,
                                  const float* y) {
    const int ci = channels == 32 ? 0 : (channels == 64 ? 1 : -1);
    const int ki = k == 3 ? 0 : (k == 5 ? 1 : (k == 7 ? 2 : -1));
    if (ci < 0 || ki < 0 || !(mask & (1u << (3 * ci + ki)))) return false;
    return resblock2_pair_supported(channels, k, d1, d2, L, x, y);
}

struct ConvW {
    int64_t w_off = 0, b_off = 0;  // float offsets into the device weight blob
    int64_t w16_off = 0, w_n = 0;  // bf16 planes (hi, lo) in the uint16 blob; packed element count
    BfoWeightOffs wo;              // bf16 octet engine (bfo.hpp), per mode: [Cin/16][K][2][CoutP][8] / [..][hi 8 | lo 8] in the same uint16 blob
    int64_t ww44_off = -1;         // ... k = 7 / 11, Cout >= 64: and as seven-point groups (conv_wino4.hip, TTSAMD_WINO4 bits 5 / 6 pick the form per launch);
                                   // C = 32: the routed fused pairs' seven-point groups (resblock_pair4.hip, TTSAMD_PAIR4)
    int64_t ww4_off = -1;          // ... and as Winograd F(4,3) groups (conv_wino4.hip: the un-fused convs, Cout >= 64; resblock_pair4.hip: the C = 32 pairs)
    int64_t wct_off = -1, bct_off = -1;   // upsamplers: the F(4,2) group filters of the (u Cout)-row two-tap conv and its per-row bias (pack_convt_wino_weight; -1: none)
    int64_t ww_off = -1;           // k = 3 / 7 / 11: Winograd F(2,3) (sub-)filters + single taps as an NG-tap conv in the fp32 blob (conv_wino2.hip; -1: none)
    int cin = 0, cout = 0, k = 0;
};

struct HifiGan {
    ttsamd_hifigan_cfg cfg;
    float* dev = nullptr;  // one blob with every packed weight and bias
    uint16_t* dev16 = nullptr;  // bf16 hi/lo planes of the same packed weights
    int64_t dev_n = 0, dev16_n = 0;  // element counts of the two blobs (ttsamd_dp_broadcast_weights)
    ConvW conv_pre, conv_post;
    std::vector<ConvW> ups;
    std::vector<ConvW> c1, c2;  // [stage*n_kernels + j][m]
    int hop = 1;
    bool rb2 = false;    // ResBlock2 generator (cfg.resblock == 2): c1[r] / c2[r] are convs.0 / convs.1 of resblocks.r
    int64_t max_cl = 0;  // max over stages of C * (L / T)
    bool bfo_ok = false; // every layer fits the bf16 octet engine (config 3 path, hifigan_forward_bfo)
    // the three ResBlocks of a stage run on three streams (created and first dispatched in hifigan_create; guarded by mu)
    mutable std::mutex mu;
    mutable hipStream_t side[2] = {nullptr, nullptr};
    mutable hipEvent_t ev_fork = nullptr, ev_done[3] = {nullptr, nullptr, nullptr};
};

// The ResBlocks of one stage are independent until their sum.  A launch is a few rounds of equally long blocks, so up to
// a third of the chip idles in its tail (stage 1 at batch 32: 3.5 rounds of 200 us blocks; batch 1..8: 1-3 rounds
// everywhere); the three branches are therefore issued on three streams and fill each other's tails.  Only the last conv
// of each branch, which accumulates into the stage output, is chained j = 0 -> 1 -> 2 by events, so the sum is formed in
// the reference's order (bit-identical results, test_hifigan_branch_streams_bit_identical).  Measured gain: +6 % at batch 1,
// +7 % at 8, +4-5 % at 12-16, +2 % at 32.  Profiling (ttsamd_profile_*) brackets each fork..join section with ONE event
// pair on the caller's stream -- wall time of the section, never a sum of overlapping launches.
// TTSAMD_HIFIGAN_STREAMS=0/1 forces either schedule.
static bool use_branch_streams(const HifiGan* h, int32_t B, int32_t T) {
    if (h->cfg.n_kernels != 3) return false;
    const int64_t streams = opt_int(OPT_HIFIGAN_STREAMS, -1);   // read per call: the tests flip it
    if (streams >= 0) return streams == 1;
    // bf16 octet engine: the launches are power-bound at batch 32 and latency-bound below; the fork / join events cost more than the
    // overlap returns under ~8 k frames (batch 1: 2.09 -> 1.92 ms, batch 8: 4.35 -> 4.26 on one stream; batch 32: 10.02 -> 9.88 ms with
    // three under the two-stream pipeline)
    // (split bf16, round 6: three streams win at every size -- batch 1 1.18 vs 1.25 ms, 2: 1.87 / 1.94, 4: 3.37 / 3.53, 8: 6.15 / 6.40,
    // tools/b1_parts.py -- so the rule below is the plain-bf16 engine's only)
    if (default_precision() == 1 && h->bfo_ok) {
        if (opt_int(OPT_BFO, 1) != 0) return (int64_t)B * T >= 8192;
    }
    return true;
}

using TensorMap = std::map<std::string, const ttsamd_tensor*>;

static int64_t numel(const ttsamd_tensor* t) {
    int64_t n = 1;
    for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
    return n;
}

// Folded weight of `<base>` : either `<base>.weight`, or g*v/||v|| from the weight-norm pair
// (norm over all dims but 0, as torch._weight_norm(v, g, 0); vocoder/hifigan/models.py:129-136).
static int32_t folded_weight(const TensorMap& tm, const std::string& base, int ndim_expected,
                             std::vector<float>& out, int64_t shape[3]) {
    const ttsamd_tensor *w = nullptr, *g = nullptr, *v = nullptr;
    auto it = tm.find(base + ".weight");
    if (it != tm.end()) w = it->second;
    if (!w) {
        auto ig = tm.find(base + ".parametrizations.weight.original0");
        auto iv = tm.find(base + ".parametrizations.weight.original1");
        if (ig == tm.end() || iv == tm.end()) {
            ig = tm.find(base + ".weight_g");
            iv = tm.find(base + ".weight_v");
        }
        TTS_REQUIRE(ig != tm.end() && iv != tm.end(), "hifigan: no weight for layer '%s'", base.c_str());
        g = ig->second;
        v = iv->second;
    }
    const ttsamd_tensor* src = w ? w : v;
    TTS_REQUIRE(src->ndim == ndim_expected, "hifigan: '%s' has ndim %d, expected %d", base.c_str(), src->ndim,
                ndim_expected);
    for (int i = 0; i < 3; ++i) shape[i] = src->shape[i];
    const int64_t n = numel(src);
    out.resize(n);
    if (w) {
        std::memcpy(out.data(), w->data, n * sizeof(float));
        return 0;
    }
    const int64_t d0 = v->shape[0], inner = n / d0;
    TTS_REQUIRE(numel(g) == d0, "hifigan: '%s' weight_g has %lld elements, expected %lld", base.c_str(),
                (long long)numel(g), (long long)d0);
    for (int64_t i = 0; i < d0; ++i) {
        double ss = 0.0;
        const float* vr = v->data + i * inner;
        for (int64_t j = 0; j < inner; ++j) ss += (double)vr[j] * vr[j];
        const float scale = g->data[i] / (float)std::sqrt(ss);
        for (int64_t j = 0; j < inner; ++j) out[i * inner + j] = vr[j] * scale;
    }
    return 0;
}

static int32_t get_bias(const TensorMap& tm, const std::string& base, int n, std::vector<float>& blob,
                        int64_t& off) {
    auto it = tm.find(base + ".bias");
    TTS_REQUIRE(it != tm.end() && numel(it->second) == n, "hifigan: missing/mis-sized '%s.bias'", base.c_str());
    off = (int64_t)blob.size();
    blob.insert(blob.end(), it->second->data, it->second->data + n);
    blob.resize(align_up((int64_t)blob.size(), 64));
    return 0;
}

static void add_bf16(std::vector<float>& blob, std::vector<uint16_t>& blob16, ConvW& cw, int64_t n) {
    cw.w_n = n;
    cw.w16_off = (int64_t)blob16.size();
    blob16.resize(blob16.size() + 2 * n);
    split_packed_bf16(blob.data() + cw.w_off, n, blob16.data() + cw.w16_off);
}

// direct_only: the direct packing and the bias only (the ResBlock2 convs: resblock2.hip reads nothing else)
static int32_t add_conv(const TensorMap& tm, const std::string& base, int cin, int cout, int k,
                        std::vector<float>& blob, std::vector<uint16_t>& blob16, ConvW& cw, bool direct_only = false) {
    std::vector<float> w;
    int64_t shp[3];
    TTS_TRY(folded_weight(tm, base, 3, w, shp));
    TTS_REQUIRE(shp[0] == cout && shp[1] == cin && shp[2] == k, "hifigan: '%s' has shape [%lld,%lld,%lld], expected [%d,%d,%d]",
                base.c_str(), (long long)shp[0], (long long)shp[1], (long long)shp[2], cout, cin, k);
    cw.cin = cin; cw.cout = cout; cw.k = k;
    cw.w_off = (int64_t)blob.size();
    blob.resize(blob.size() + (size_t)cin * k * cout_padded(cout));
    pack_conv_weight(w.data(), cout, cin, k, blob.data() + cw.w_off);
    if (direct_only) {
        blob.resize(align_up((int64_t)blob.size(), 64));
        return get_bias(tm, base, cout, blob, cw.b_off);
    }
    add_bf16(blob, blob16, cw, (int64_t)cin * k * cout_padded(cout));
    // the Winograd forms this conv carries (hifigan_conv_forms, conv_route.hip), one behind the other
    const auto add_form = [&](int groups, void (*pack)(const float*, int, int, int, float*), int64_t& off) {
        blob.resize(align_up((int64_t)blob.size(), 64));
        off = (int64_t)blob.size();
        blob.resize(blob.size() + (size_t)cin * groups * cout_padded(cout));
        pack(w.data(), cout, cin, k, blob.data() + off);
    };
    const ConvForms forms = hifigan_conv_forms(cin, cout, k);
    if (forms.wino2) add_form(wino2_groups(k), pack_wino2_weight, cw.ww_off);
    if (forms.wino4) add_form(wino4_groups(k), pack_wino4_weight, cw.ww4_off);
    if (forms.wino44) add_form(wino44_groups(k), pack_wino44_weight, cw.ww44_off);
    if (cin % 8 == 0 && cout % 32 == 0) cw.wo = bfo_append_weights(w.data(), cout, cin, k, 1, blob16);
    blob.resize(align_up((int64_t)blob.size(), 64));
    return get_bias(tm, base, cout, blob, cw.b_off);
}

void hifigan_destroy(HifiGan* h);

__global__ void hifigan_touch_kernel() {}   // first dispatch of a branch stream (hifigan_create)

int32_t hifigan_create(const ttsamd_tensor* weights, int32_t n, const ttsamd_hifigan_cfg* cfg, HifiGan** out) {
    TTS_REQUIRE(weights && cfg && out, "hifigan_create: null argument");
    TTS_REQUIRE(cfg->n_ups >= 1 && cfg->n_ups <= 8 && cfg->n_kernels >= 1 && cfg->n_kernels <= 8 &&
                cfg->n_dilations >= 1 && cfg->n_dilations <= 8, "hifigan_create: bad config counts");
    const int rb = cfg->resblock == 0 ? 1 : cfg->resblock;
    TTS_REQUIRE(rb == 1 || rb == 2, "hifigan_create: resblock %d (1 = ResBlock1, 2 = ResBlock2)", cfg->resblock);
    TTS_REQUIRE(rb == 1 || cfg->n_dilations >= 2, "hifigan_create: a ResBlock2 takes two dilations per kernel size, %d given",
                cfg->n_dilations);
    TensorMap tm;
    for (int i = 0; i < n; ++i) tm[weights[i].name] = &weights[i];
    auto* h = new HifiGan();
    h->cfg = *cfg;
    h->cfg.resblock = rb;
    h->rb2 = rb == 2;
    std::vector<float> blob;
    std::vector<uint16_t> blob16;
    const int c0 = cfg->upsample_initial_channel;
    int32_t rc = add_conv(tm, "conv_pre", cfg->num_mels, c0, 7, blob, blob16, h->conv_pre);
    int ch = c0, mul = 1;
    h->max_cl = c0;
    for (int i = 0; rc == 0 && i < cfg->n_ups; ++i) {
        const int u = cfg->upsample_rates[i], kt = cfg->upsample_kernel_sizes[i];
        const int cin = ch, cout = ch / 2;
        if (kt != 2 * u || (kt - u) % 2 != 0) {
            set_error("hifigan: upsample kernel %d / rate %d: only kernel = 2*rate is built", kt, u);
            rc = TTSAMD_EINVAL;
            break;
        }
        std::vector<float> w;
        int64_t shp[3];
        rc = folded_weight(tm, "ups." + std::to_string(i), 3, w, shp);
        if (rc) break;
        if (shp[0] != cin || shp[1] != cout || shp[2] != kt) {
            set_error("hifigan: ups.%d has shape [%lld,%lld,%lld], expected [%d,%d,%d]", i, (long long)shp[0],
                      (long long)shp[1], (long long)shp[2], cin, cout, kt);
            rc = TTSAMD_EINVAL;
            break;
        }
        ConvW cw;
        cw.cin = cin; cw.cout = cout; cw.k = kt;
        cw.w_off = (int64_t)blob.size();
        blob.resize(blob.size() + (size_t)u * cin * 2 * cout_padded(cout));
        pack_convt_weight(w.data(), cin, cout, kt, u, (kt - u) / 2, blob.data() + cw.w_off);
        add_bf16(blob, blob16, cw, (int64_t)u * cin * 2 * cout_padded(cout));
        if (cin % 16 == 0 && cout % 32 == 0 && (u == 8 || u == 2)) cw.wo = bfo_append_weights(w.data(), cout, cin, kt, u, blob16);
        blob.resize(align_up((int64_t)blob.size(), 64));
        rc = get_bias(tm, "ups." + std::to_string(i), cout, blob, cw.b_off);
        if (rc) break;
        if (convt_wino_packable(cin, cout, u)) {   // the same upsampler for the F(4,2) launch (conv_wino4.hip); the routing switch is read per launch
            cw.wct_off = (int64_t)blob.size();
            blob.resize(blob.size() + (size_t)6 * cin * u * cout);
            cw.bct_off = (int64_t)blob.size();
            blob.resize(align_up((int64_t)blob.size() + (int64_t)u * cout, 64));
            // (blob may have been reallocated: take the bias pointer after the resize)
            pack_convt_wino_weight(w.data(), blob.data() + cw.b_off, cin, cout, u, blob.data() + cw.wct_off, blob.data() + cw.bct_off);
        }
        h->ups.push_back(cw);
        ch = cout;
        mul *= u;
        h->max_cl = std::max<int64_t>(h->max_cl, (int64_t)ch * mul);
        for (int j = 0; rc == 0 && j < cfg->n_kernels; ++j) {
            const int r = i * cfg->n_kernels + j, kk = cfg->resblock_kernel_sizes[j];
            if (h->rb2) {
                // exactly two convs per ResBlock2, dilations [j][0] / [j][1] (further entries are ignored, as by the reference)
                if (!resblock2_conv_supported(ch, kk, cfg->resblock_dilations[j][0], 1, nullptr, blob.data()) ||
                    !resblock2_conv_supported(ch, kk, cfg->resblock_dilations[j][1], 1, nullptr, blob.data())) {
                    set_error("hifigan: ResBlock2 at C = %d, k = %d, dilations %d / %d is not built (C = 32 / 64 / 128, k = 3 / 5 / 7 / 11, "
                              "dilation 1..16)", ch, kk, cfg->resblock_dilations[j][0], cfg->resblock_dilations[j][1]);
                    rc = TTSAMD_EINVAL;
                    break;
                }
                ConvW a, b;
                rc = add_conv(tm, "resblocks." + std::to_string(r) + ".convs.0", ch, ch, kk, blob, blob16, a, true);
                if (rc == 0) rc = add_conv(tm, "resblocks." + std::to_string(r) + ".convs.1", ch, ch, kk, blob, blob16, b, true);
                h->c1.push_back(a);
                h->c2.push_back(b);
                continue;
            }
            for (int m = 0; rc == 0 && m < cfg->n_dilations; ++m) {
                ConvW a, b;
                rc = add_conv(tm, "resblocks." + std::to_string(r) + ".convs1." + std::to_string(m), ch, ch, kk, blob, blob16, a);
                if (rc) break;
                rc = add_conv(tm, "resblocks." + std::to_string(r) + ".convs2." + std::to_string(m), ch, ch, kk, blob, blob16, b);
                h->c1.push_back(a);
                h->c2.push_back(b);
            }
        }
    }
    h->hop = mul;
    if (rc == 0 && !h->rb2) {
        // the bf16 octet engine covers this generator if every layer was packed for it
        bool ok = h->conv_pre.wo.packed() && ch == 32 && cfg->num_mels % 8 == 0;
        for (const ConvW& cw : h->ups) ok = ok && cw.wo.packed();
        for (size_t i = 0; i < h->c1.size(); ++i) ok = ok && h->c1[i].wo.packed() && h->c2[i].wo.packed();
        for (int j = 0; j < cfg->n_kernels; ++j) {
            const int kk = cfg->resblock_kernel_sizes[j];
            ok = ok && (kk == 3 || kk == 7 || kk == 11);
            for (int m = 0; m < cfg->n_dilations; ++m) ok = ok && cfg->resblock_dilations[j][m] >= 1 && cfg->resblock_dilations[j][m] <= BFO_DMAX;
        }
        h->bfo_ok = ok;
    }
    if (rc == 0) {
        // conv_post: [1][C][7] -> plain [C][7]
        std::vector<float> w;
        int64_t shp[3];
        rc = folded_weight(tm, "conv_post", 3, w, shp);
        if (rc == 0 && (shp[0] != 1 || shp[1] != ch || shp[2] != 7)) {
            set_error("hifigan: conv_post has shape [%lld,%lld,%lld], expected [1,%d,7]", (long long)shp[0],
                      (long long)shp[1], (long long)shp[2], ch);
            rc = TTSAMD_EINVAL;
        }
        if (rc == 0) {
            h->conv_post.cin = ch; h->conv_post.cout = 1; h->conv_post.k = 7;
            h->conv_post.w_off = (int64_t)blob.size();
            blob.insert(blob.end(), w.begin(), w.end());
            blob.resize(align_up((int64_t)blob.size(), 64));
            rc = get_bias(tm, "conv_post", 1, blob, h->conv_post.b_off);
        }
    }
    if (rc == 0) {
        h->dev_n = (int64_t)blob.size();
        h->dev16_n = (int64_t)blob16.size();
        hipError_t e = hipMalloc((void**)&h->dev, blob.size() * sizeof(float));
        if (e == hipSuccess) e = hipMemcpy(h->dev, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void**)&h->dev16, blob16.size() * sizeof(uint16_t));
        if (e == hipSuccess) e = hipMemcpy(h->dev16, blob16.data(), blob16.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            set_error("hifigan_create: weight upload failed: %s", hipGetErrorString(e));
            rc = TTSAMD_EHIP;
        }
        // The two ResBlock branch streams exist and have dispatched once BEFORE the caller's own side streams do (the runtime
        // binds a stream to a hardware queue at its first dispatch).  Created lazily inside the first forward they were bound
        // after the two ttsamd.pipeline streams whenever that schedule ran first, and every later one-stream call paid 1.2-1.9 ms
        // for its fork / join events (batch 1: 3.3 instead of 2.1 ms, tools/pipe_debug2.py).
        if (e == hipSuccess && cfg->n_kernels == 3) {
            for (auto& st : h->side)
                if (e == hipSuccess) {
                    // highest stream priority: under the two-stream pipeline (ttsamd.pipeline: its vocoder stream is created the same way)
                    // the acoustic model of the next batch fills what the vocoder leaves instead of competing with it -- same-box A/B,
                    // three alternations: fp32 52.86 -> 52.59 ms per step, split bf16 25.40 -> 25.25
                    int lo = 0, hi = 0;
                    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
                    e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi);
                }
            if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
            for (auto& ev : h->ev_done)
                if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
            for (auto& st : h->side)
                if (e == hipSuccess) {
                    hipLaunchKernelGGL(hifigan_touch_kernel, dim3(1), dim3(64), 0, st);
                    e = hipGetLastError();
                }
            for (auto& st : h->side)
                if (e == hipSuccess && st) e = hipStreamSynchronize(st);
            if (e != hipSuccess) {
                set_error("hifigan_create: branch streams: %s", hipGetErrorString(e));
                rc = TTSAMD_EHIP;
            }
        }
    }
    if (rc != 0) {
        hifigan_destroy(h);            // blobs, branch streams and events alike
        return rc;
    }
    *out = h;
    return 0;
}

void hifigan_destroy(HifiGan* h) {
    if (!h) return;
    if (h->dev) (void)hipFree(h->dev);
    if (h->dev16) (void)hipFree(h->dev16);
    for (hipStream_t st : h->side) if (st) (void)hipStreamDestroy(st);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (hipEvent_t e : h->ev_done) if (e) (void)hipEventDestroy(e);
    delete h;
}

// The workspace of a forward, carved once for hifigan_workspace_bytes (null arena: it only counts) and hifigan_forward.  nb = branches
// with buffers of their own (3 on three streams, else 1: the others alias branch 0's)
struct HgWorkspace {
    float *cur, *ups_out;             // the stage sum and the upsampler's output
    float *Tb[3], *R[3], *splitk[3];  // per branch: the c1 -> c2 intermediate, the ResBlock's running output, split-K partial sums
    uint16_t* mel_o;                  // octet engine: the mel in its layout (x3: 4 bytes per element)
};
static HgWorkspace hg_carve(Arena& a, const HifiGan* h, int32_t B, int32_t T, int nb) {
    HgWorkspace w;
    const int64_t n = (int64_t)B * h->max_cl * T;
    w.cur = a.take<float>(n); w.ups_out = a.take<float>(n);
    for (int i = 0; i < nb; ++i) { w.Tb[i] = a.take<float>(n); w.R[i] = a.take<float>(n); }
    for (int i = 0; i < nb; ++i) w.splitk[i] = a.take<float>(kSplitKFloats);
    for (int i = nb; i < 3; ++i) { w.Tb[i] = w.Tb[0]; w.R[i] = w.R[0]; w.splitk[i] = w.splitk[0]; }
    w.mel_o = a.take<uint16_t>((int64_t)B * align_up(h->cfg.num_mels, 8) * T * 2);
    return w;
}

int64_t hifigan_workspace_bytes(const HifiGan* h, int32_t B, int32_t T) {
    Arena a(nullptr, 0);
    hg_carve(a, h, B, T, use_branch_streams(h, B, T) ? 3 : 1);
    return a.off;
}

// The accumulate mode of a launch that writes the stage sum: branch 0 stores (0), the middle branches add (1), the last one adds and
// divides by n_kernels (2).  Every launch that is not its branch's last stores, and so does a lone branch.
static int sum_mode(int j, int n_kernels, bool last) {
    return (!last || n_kernels == 1 || j == 0) ? 0 : (j + 1 < n_kernels ? 1 : 2);
}

// The schedule of a stage's ResBlocks, for all three engines: the only place that records or waits for an event, and the one
// profiling bracket.  A branch body asks for its stream (branch), says that its next launch accumulates into the stage sum
// (before_sum: the sum is formed in the order j = 0 -> 1 -> 2) and that it is done (done).  One stream: all of it is a no-op.
struct StageSchedule {
    const HifiGan* h;
    hipStream_t s;            // the caller's stream: branch 0 and everything outside the ResBlocks
    bool multi;
    hipStream_t bs[3];
    bool in_section = false;  // inside fork..join: profiling brackets the section once, per-launch spans would overlap
    bool failed = false;

    // a failure must not leave the side streams running on a workspace the caller is about to recycle
    ~StageSchedule() { if (multi && failed) { (void)hipStreamSynchronize(bs[1]); (void)hipStreamSynchronize(bs[2]); } }
    int32_t fail(int32_t rc) { failed = failed || rc != 0; return rc; }

    int32_t fork() {
        if (!multi) return 0;
        prof_section_begin(s);
        in_section = true;
        TTS_CHECK_HIP(hipEventRecord(h->ev_fork, s));
        return 0;
    }
    int32_t branch(int j, hipStream_t* st) {
        *st = bs[j % 3];
        if (multi && j > 0) TTS_CHECK_HIP(hipStreamWaitEvent(*st, h->ev_fork, 0));
        return 0;
    }
    int32_t before_sum(int j) {
        if (multi && j > 0) TTS_CHECK_HIP(hipStreamWaitEvent(bs[j % 3], h->ev_done[j - 1], 0));
        return 0;
    }
    int32_t done(int j) {
        if (multi) TTS_CHECK_HIP(hipEventRecord(h->ev_done[j], bs[j % 3]));
        return 0;
    }
    int32_t join(int n_kernels) {
        if (!multi) return 0;
        TTS_CHECK_HIP(hipStreamWaitEvent(s, h->ev_done[n_kernels - 1], 0));
        in_section = false;
        prof_section_end(s);
        return 0;
    }
    template <class F>
    int32_t timed(hipStream_t st, double flops, F&& launch) {
        if (in_section) prof_add(flops);
        else prof_begin(st, flops);
        const int32_t rc = launch();
        if (!in_section) prof_end(st);
        return rc;
    }
};

// what one forward hands to its branch bodies: read once, constant from there on
struct HgCall {
    const HifiGan* h;
    const int64_t* lens;
    int32_t B, prec;
    HgWorkspace w;
    StageSchedule& sch;
    // the launch_conv engines (exact fp32; TTSAMD_BFO=0: the round-2 bf16 engine) only:
    ConvParams base;        // what every launch_conv of the forward shares; each launch builds its own parameters from it
    bool pack_t;            // plain bf16 mode: the c1 -> c2 intermediate of a ResBlock only feeds c2, so it crosses HBM as packed bf16
                            // (ConvParams::y_packed / x_packed; same rounding point as the fp32 buffer + round-on-load, bit-identical)
    PairRouteOpts pair_opts;
    unsigned rb2_mask;
};
struct Stage { int i, L, mul; };   // upsampler index, positions per row and length multiplier behind it

// ---- config 3: plain bf16 (precision 1) and split bf16 (precision 2) run on the octet engine (bfo.hpp / bfo3.hpp):
// v_mfma_f32_32x32x16_bf16, activations in HBM as octet entries (bf16, or hi + lo) stored pre-activated for their consumer,
// fused c1 -> c2 pairs for C <= 128.  TTSAMD_BFO=0 keeps the round-2 bf16 engine (fp32 activations in HBM).
// One ResBlock1: a chained launch, or per dilation a pair launch or (C = 256) two conv launches.  `cp` is the forward's one conv
// parameter block (octet_forward); next_slope: what reads the stage sum applies it
static int32_t octet_branch(const HgCall& c, const BfoMode& M, BfoConvParams& cp, const Stage& g, int j, float next_slope) {
    const HifiGan* h = c.h;
    const ttsamd_hifigan_cfg& cfg = h->cfg;
    const uint16_t* W16 = h->dev16;
    const int L = g.L, mul = g.mul;
    void *curo = c.w.cur, *Tb = c.w.Tb[j % 3], *R = c.w.R[j % 3];
    hipStream_t st;
    TTS_TRY(c.sch.branch(j, &st));
    const void* src = c.w.ups_out;
    const int li0 = (g.i * cfg.n_kernels + j) * cfg.n_dilations;
    const float div = (float)cfg.n_kernels, sum_slope = j + 1 == cfg.n_kernels ? next_slope : 1.f;
    // a ResBlock whose three pairs fit the chained kernel (k = 3; k = 7 at C <= 64) goes out as ONE launch (bfo_chain.hip; bit-identical)
    int32_t dl[3] = {0, 0, 0};
    for (int m = 0; m < cfg.n_dilations && m < 3; ++m) dl[m] = cfg.resblock_dilations[j][m];
    // (TTSAMD_BFO_CHAIN=0: three pair launches per ResBlock; bit-identical, A/B and parity runs)
    if (M.chain_wanted(h->c1[li0].cin, h->c1[li0].k, dl, cfg.n_dilations, L, c.B)) {
        BfoChainParams cc;
        std::memset(&cc, 0, sizeof(cc));
        cc.x = src; cc.y = curo; cc.sum_in = curo;
        for (int m = 0; m < 3; ++m) {
            const ConvW &w1 = h->c1[li0 + m], &w2 = h->c2[li0 + m];
            cc.w1[m] = W16 + w1.wo.of(M); cc.w2[m] = W16 + w2.wo.of(M); cc.b1[m] = h->dev + w1.b_off; cc.b2[m] = h->dev + w2.b_off;
            cc.dil[m] = dl[m];
        }
        cc.lens = c.lens; cc.len_mul = mul; cc.L = L; cc.batch = c.B; cc.k = h->c1[li0].k;
        cc.mode = sum_mode(j, cfg.n_kernels, true);
        cc.div = div; cc.in_slope = 0.1f; cc.mid_slope = 0.1f; cc.out_slope = sum_slope;
        TTS_TRY(c.sch.before_sum(j));
        TTS_TRY(c.sch.timed(st, 3 * 2.0 * (2.0 * h->c1[li0].cin * h->c1[li0].cin * h->c1[li0].k) * mul,
                            [&] { return M.chain(h->c1[li0].cin, cc, st); }));
        return c.sch.done(j);
    }
    for (int m = 0; m < cfg.n_dilations; ++m) {
        const int d = cfg.resblock_dilations[j][m];
        const bool last = m + 1 == cfg.n_dilations;
        const ConvW &w1 = h->c1[li0 + m], &w2 = h->c2[li0 + m];
        void* dst = last ? curo : (src == R ? Tb : R);
        // running ResBlock sum in `cur`: raw bf16 until the last branch stores it activated for its consumer
        const int mode = sum_mode(j, cfg.n_kernels, last);
        const float out_slope = !last ? 0.1f : sum_slope;
        if (last) TTS_TRY(c.sch.before_sum(j));
        const double fl = 2.0 * (2.0 * w1.cin * w1.cin * w1.k) * mul;
        if (M.pair_supported(w1.cin, w1.k, d, L)) {
            BfoPairParams pp;
            std::memset(&pp, 0, sizeof(pp));
            pp.x = src; pp.y = dst; pp.sum_in = curo;
            pp.w1 = W16 + w1.wo.of(M); pp.w2 = W16 + w2.wo.of(M); pp.b1 = h->dev + w1.b_off; pp.b2 = h->dev + w2.b_off;
            pp.lens = c.lens; pp.len_mul = mul; pp.L = L; pp.dil = d; pp.batch = c.B;
            pp.mode = mode; pp.div = div; pp.in_slope = 0.1f; pp.mid_slope = 0.1f; pp.out_slope = out_slope;
            TTS_TRY(c.sch.timed(st, fl, [&] { return M.pair(w1.cin, w1.k, pp, st); }));
        } else {
            // C = 256 (stage 1): c1 and c2 as two launches, the intermediate stored activated for c2.  c2 reads its
            // residual only at its own output positions, so it may run in place (dst == src == R)
            if (!last) dst = R;
            TTS_TRY(c.sch.timed(st, fl, [&] {
                cp.x = src; cp.y = Tb; cp.w = W16 + w1.wo.of(M); cp.bias = h->dev + w1.b_off; cp.res = nullptr; cp.sum_in = nullptr;
                cp.len_mul = mul; cp.Lin = L; cp.Cin = w1.cin; cp.Cout = w1.cout; cp.K = w1.k; cp.dil = d; cp.up = 1;
                cp.mode = 0; cp.out_slope = 0.1f; cp.res_slope = 1.f;
                cp.splitk_ws = c.w.splitk[j % 3]; cp.splitk_floats = kSplitKFloats;     // batch 1: 30 blocks per stage-1 conv
                const int32_t rc = M.conv(cp, st);
                if (rc != 0) return rc;
                cp.x = Tb; cp.y = dst; cp.w = W16 + w2.wo.of(M); cp.bias = h->dev + w2.b_off; cp.res = src; cp.sum_in = curo;
                cp.dil = 1; cp.mode = mode; cp.div = div; cp.out_slope = out_slope; cp.res_slope = 0.1f;
                return M.conv(cp, st);
            }));
        }
        if (last) TTS_TRY(c.sch.done(j));
        src = dst;
    }
    return 0;
}

static int32_t octet_forward(const HgCall& c, const float* mel, int32_t T, float* wave) {
    const HifiGan* h = c.h;
    const ttsamd_hifigan_cfg& cfg = h->cfg;
    const BfoMode& M = bfo_mode(c.prec);
    const uint16_t* W16 = h->dev16;
    hipStream_t s = c.sch.s;
    void *curo = c.w.cur, *upso = c.w.ups_out;                 // the fp32-sized buffers hold bf16 / x3 tensors of the same element count
    TTS_TRY(M.pack(mel, c.B, cfg.num_mels, T, 1.f, c.w.mel_o, s));
    BfoConvParams cp;
    std::memset(&cp, 0, sizeof(cp));
    cp.batch = c.B; cp.lens = c.lens; cp.div = 1.f; cp.res_slope = 1.f;
    // conv_pre (models.py:112); its consumer, the first upsampler, applies leaky_relu(0.1) (models.py:114)
    cp.x = c.w.mel_o; cp.y = curo; cp.w = W16 + h->conv_pre.wo.of(M); cp.bias = h->dev + h->conv_pre.b_off;
    cp.len_mul = 1; cp.Lin = T; cp.Cin = h->conv_pre.cin; cp.Cout = h->conv_pre.cout; cp.K = 7; cp.dil = 1; cp.up = 1;
    cp.mode = 0; cp.out_slope = 0.1f;
    TTS_TRY(c.sch.timed(s, 2.0 * cp.Cout * cp.Cin * 7, [&] { return M.conv(cp, s); }));
    Stage g = {0, T, 1};
    for (g.i = 0; g.i < cfg.n_ups; ++g.i) {
        const int u = cfg.upsample_rates[g.i];
        const ConvW& uw = h->ups[g.i];
        // ConvTranspose1d on the activated stage input; the ResBlocks read its output through leaky_relu(0.1)
        cp.x = curo; cp.y = upso; cp.w = W16 + uw.wo.of(M); cp.bias = h->dev + uw.b_off; cp.res = nullptr; cp.sum_in = nullptr;
        cp.len_mul = g.mul; cp.Lin = g.L; cp.Cin = uw.cin; cp.Cout = uw.cout; cp.K = 2; cp.dil = 1; cp.up = u;
        cp.mode = 0; cp.out_slope = 0.1f;
        TTS_TRY(c.sch.timed(s, 2.0 * uw.cout * uw.cin * 2 * u * g.mul, [&] { return M.convt(cp, s); }));
        g.L *= u; g.mul *= u;
        // what reads the stage sum: the next upsampler through leaky_relu(0.1), conv_post through leaky_relu(0.01)
        const float next_slope = g.i + 1 < cfg.n_ups ? 0.1f : 0.01f;
        TTS_TRY(c.sch.fork());
        for (int j = 0; j < cfg.n_kernels; ++j) TTS_TRY(octet_branch(c, M, cp, g, j, next_slope));
        TTS_TRY(c.sch.join(cfg.n_kernels));
    }
    return M.conv_post(curo, h->dev + h->conv_post.w_off, h->dev + h->conv_post.b_off, c.lens, g.mul, c.B, h->conv_post.cin, g.L, wave,
                       (int64_t)g.L, s);
}

// ---- exact fp32 (and TTSAMD_BFO=0: the round-2 bf16 engine) on launch_conv and the fused fp32 kernels
// one launch_conv.  pack_io bit 0: x is packed, bit 1: write y packed
static int32_t hg_conv(const HgCall& c, const ConvW& cw, const float* x, hipStream_t st, float* y, const float* res,
                       const Stage& g, int dil, float slope, int mode, float div, float* splitk_ws, int pack_io) {
    const HifiGan* h = c.h;
    const int L = g.L;
    ConvParams p = c.base;
    p.x = x; p.x_bs = (int64_t)cw.cin * L; p.x_cs = L;
    p.w = h->dev + cw.w_off; p.bias = h->dev + cw.b_off;
    p.w_bf16 = h->dev16 + cw.w16_off; p.precision = c.prec;
    p.w_wino = cw.ww_off >= 0 ? h->dev + cw.ww_off : nullptr;
    p.w_wino4 = (cw.ww4_off >= 0 && cw.cout >= 64) ? h->dev + cw.ww4_off : nullptr;   // (C = 32: the fused pair's filters only)
    p.w_wino44 = (cw.ww44_off >= 0 && cw.cout >= 64) ? h->dev + cw.ww44_off : nullptr;   // (likewise: 32 rows are no launch of the 64-row kernel)
    p.y = y; p.y_bs = (int64_t)cw.cout * L; p.y_cs = L; p.y_ts = 1;
    p.res = res; p.r_bs = (int64_t)cw.cout * L; p.r_cs = L;
    p.len_in_mul = g.mul; p.len_out_mul = g.mul; p.Lin = L; p.Nout = L;
    p.Cin = cw.cin; p.Cout = cw.cout; p.CoutP = cout_padded(cw.cout); p.K = cw.k;
    p.dil = dil; p.pad = (cw.k * dil - dil) / 2;
    p.in_slope = slope; p.mode = mode; p.div = div;
    p.x_packed = (pack_io & 1) ? 1 : 0; p.y_packed = (pack_io & 2) ? 1 : 0;
    p.splitk_ws = splitk_ws;
    return c.sch.timed(st, 2.0 * cw.cout * cw.cin * cw.k * g.mul, [&] { return launch_conv(p, st); });
}

static PairConv pair_conv(const HifiGan* h, const ConvW& cw) {
    const auto form = [&](int64_t off) { return off >= 0 ? h->dev + off : (const float*)nullptr; };
    return {h->dev + cw.w_off, h->dev + cw.b_off, form(cw.ww_off), form(cw.ww4_off), form(cw.ww44_off)};
}

// One ResBlock1 (models.py:46-53): per dilation the c1 -> c2 pair as ONE fused launch where pair_route says so (x and y must differ
// -- halo reads -- so the pair outputs alternate between R and the unused c1 buffer), else c1 into Tb and c2, with the residual, into R
static int32_t resblock1_branch(const HgCall& c, const Stage& g, int j) {
    const HifiGan* h = c.h;
    const ttsamd_hifigan_cfg& cfg = h->cfg;
    float *cur = c.w.cur, *Tb = c.w.Tb[j % 3], *R = c.w.R[j % 3], *splitk = c.w.splitk[j % 3];
    hipStream_t st;
    TTS_TRY(c.sch.branch(j, &st));
    const float* src = c.w.ups_out;
    for (int m = 0; m < cfg.n_dilations; ++m) {
        const int li = (g.i * cfg.n_kernels + j) * cfg.n_dilations + m;
        const int d = cfg.resblock_dilations[j][m];
        const bool last = m + 1 == cfg.n_dilations;
        const ConvW &w1 = h->c1[li], &w2 = h->c2[li];
        const PairConv p1 = pair_conv(h, w1), p2 = pair_conv(h, w2);
        const int mode = sum_mode(j, cfg.n_kernels, last);
        float* dst = last ? cur : (src == R ? Tb : R);
        const bool square = w1.cin == w1.cout && w2.cin == w1.cin && w2.cout == w1.cin && w1.k == w2.k;
        const ConvForms forms = {p1.w_wino2 && p2.w_wino2, p1.w_wino4 && p2.w_wino4, p1.w_wino44 && p2.w_wino44};
        const PairRoute r = pair_route(PairShape{w1.cin, w1.k, d, g.L, c.B, square, src, dst, forms, c.prec}, c.pair_opts);
        if (r.kernel != PAIR_NONE) {
            if (last) TTS_TRY(c.sch.before_sum(j));
            const PairArgs a = {w1.cin, w1.k, d, src, dst, p1, p2, c.lens, g.mul, g.L, c.B, mode, (float)cfg.n_kernels, 0.1f};
            TTS_TRY(c.sch.timed(st, 2.0 * (2.0 * w1.cin * w1.cin * w1.k) * g.mul, [&] { return launch_pair(r, a, st); }));
        } else {
            dst = last ? cur : R;
            TTS_TRY(hg_conv(c, w1, src, st, Tb, nullptr, g, d, 0.1f, 0, 1.f, splitk, c.pack_t ? 2 : 0));
            if (last) TTS_TRY(c.sch.before_sum(j));
            TTS_TRY(hg_conv(c, w2, Tb, st, dst, src, g, 1, 0.1f, mode, last ? (float)cfg.n_kernels : 1.f, splitk, c.pack_t ? 1 : 0));
        }
        if (last) TTS_TRY(c.sch.done(j));
        src = dst;
    }
    return 0;
}

// One ResBlock2 (models.py:62-83): both convs as one resblock2_pair launch where routed, else two resblock2_conv launches through Tb
// (x != y: halo reads).  The second writes the stage sum into `cur` (mode / div as for ResBlock1)
static int32_t resblock2_branch(const HgCall& c, const Stage& g, int j) {
    const HifiGan* h = c.h;
    const ttsamd_hifigan_cfg& cfg = h->cfg;
    const float* x = c.w.ups_out;
    float *cur = c.w.cur, *Tb = c.w.Tb[j % 3];
    hipStream_t st;
    TTS_TRY(c.sch.branch(j, &st));
    const ConvW &w1 = h->c1[g.i * cfg.n_kernels + j], &w2 = h->c2[g.i * cfg.n_kernels + j];
    const float *W1 = h->dev + w1.w_off, *B1 = h->dev + w1.b_off, *W2 = h->dev + w2.w_off, *B2 = h->dev + w2.b_off;
    const int d1 = cfg.resblock_dilations[j][0], d2 = cfg.resblock_dilations[j][1];
    const int mode = sum_mode(j, cfg.n_kernels, true);
    const float div = (float)cfg.n_kernels;
    const double fl = 2.0 * w1.cout * w1.cin * w1.k * g.mul;      // per conv
    if (resblock2_pair_choice(c.rb2_mask, w1.cin, w1.k, d1, d2, g.L, x, cur)) {
        TTS_TRY(c.sch.before_sum(j));
        TTS_TRY(c.sch.timed(st, 2 * fl, [&] {
            return launch_resblock2_pair(w1.cin, x, cur, W1, B1, W2, B2, w1.k, d1, d2, c.lens, g.mul, g.L, c.B, mode, div, 0.1f, st);
        }));
    } else {
        TTS_TRY(c.sch.timed(st, fl, [&] {
            return launch_resblock2_conv(w1.cin, x, Tb, W1, B1, w1.k, d1, c.lens, g.mul, g.L, c.B, 0, 1.f, 0.1f, st);
        }));
        TTS_TRY(c.sch.before_sum(j));
        TTS_TRY(c.sch.timed(st, fl, [&] {
            return launch_resblock2_conv(w2.cin, Tb, cur, W2, B2, w2.k, d2, c.lens, g.mul, g.L, c.B, mode, div, 0.1f, st);
        }));
    }
    return c.sch.done(j);
}

static int32_t f32_forward(const HgCall& c, const float* mel, int32_t T, float* wave) {
    const HifiGan* h = c.h;
    const ttsamd_hifigan_cfg& cfg = h->cfg;
    hipStream_t s = c.sch.s;
    float *cur = c.w.cur, *ups_out = c.w.ups_out;
    const bool convt_ok = opt_int(OPT_CONVT, 1) != 0;   // all-phases-per-wave transposed conv (convt_mfma.hip)
    // conv_pre (models.py:112)
    Stage g = {0, T, 1};
    TTS_TRY(hg_conv(c, h->conv_pre, mel, s, cur, nullptr, g, 1, 1.0f, 0, 1.f, c.w.splitk[0], 0));
    for (g.i = 0; g.i < cfg.n_ups; ++g.i) {
        const int u = cfg.upsample_rates[g.i], kt = cfg.upsample_kernel_sizes[g.i];
        const ConvW& uw = h->ups[g.i];
        // leaky_relu(0.1) + ConvTranspose1d as u polyphase 2-tap convs (models.py:114-115)
        ConvParams pu = c.base;
        pu.splitk_ws = c.w.splitk[0];
        TTS_TRY(c.sch.timed(s, 2.0 * uw.cout * uw.cin * 2 * u * g.mul, [&] {
            return launch_upsampler(pu, cur, h->dev + uw.w_off, h->dev16 + uw.w16_off, h->dev + uw.b_off, ups_out, uw.cin, uw.cout, u, kt, g.L,
                                    g.mul, 0.1f, convt_ok, s, uw.wct_off >= 0 ? h->dev + uw.wct_off : nullptr,
                                    uw.bct_off >= 0 ? h->dev + uw.bct_off : nullptr);
        }));
        g.L *= u; g.mul *= u;
        // the ResBlocks on the same input, averaged (models.py:116-122)
        TTS_TRY(c.sch.fork());
        for (int j = 0; j < cfg.n_kernels; ++j) TTS_TRY(h->rb2 ? resblock2_branch(c, g, j) : resblock1_branch(c, g, j));
        TTS_TRY(c.sch.join(cfg.n_kernels));
    }
    // leaky_relu (default slope 0.01) + conv_post + tanh (models.py:123-125)
    return launch_conv_post(cur, (int64_t)h->conv_post.cin * g.L, g.L, h->dev + h->conv_post.w_off, h->dev + h->conv_post.b_off, c.lens, g.mul,
                            c.B, h->conv_post.cin, g.L, 0.01f, wave, (int64_t)g.L, s);
}

int32_t hifigan_forward(const HifiGan* h, const float* mel, const int64_t* lens, int32_t B, int32_t T, float* wave,
                        void* ws, int64_t ws_bytes, hipStream_t s) {
    TTS_REQUIRE(h && mel && wave && B >= 1 && T >= 1, "hifigan_forward: bad argument");
    const int prec = default_precision();
    TTS_REQUIRE(!h->rb2 || prec == 0, "hifigan_forward: a ResBlock2 generator is built for f32 only (precision %d "
                "requested; ttsamd_set_precision(0))", prec);
    Arena a(ws, ws_bytes);
    const bool multi = use_branch_streams(h, B, T);
    const HgWorkspace w = hg_carve(a, h, B, T, multi ? 3 : 1);
    if (!ws || !a.ok) {
        set_error("hifigan_forward: workspace of %lld bytes needed, %lld given", (long long)a.off, (long long)ws_bytes);
        return TTSAMD_ENOMEM;
    }
    std::unique_lock<std::mutex> lk(h->mu, std::defer_lock);
    if (multi) {
        lk.lock();
        TTS_REQUIRE(h->ev_fork && h->side[0] && h->side[1], "hifigan_forward: the branch streams were not created (hifigan_create)");
    }
    StageSchedule sch{h, s, multi, {s, multi ? h->side[0] : s, multi ? h->side[1] : s}};
    HgCall c = {h, lens, B, prec, w, sch};     // (the rest zeroed)
    c.base.batch = B; c.base.lens_in = lens; c.base.lens_out = lens;
    c.base.n_phase = 1; c.base.div = 1.f; c.base.pack_slope = 0.1f;
    c.base.splitk_floats = kSplitKFloats;     // batch 1: stage-1 launches have < 256 tiles
    c.pack_t = prec == 1 && opt_int(OPT_BF16_PACKED_T, 1) != 0;
    c.pair_opts = pair_route_opts();
    c.rb2_mask = (unsigned)opt_int(OPT_RESBLOCK2_PAIR, kResblock2PairMask);
    const bool octet = (prec == 1 || prec == 2) && h->bfo_ok && opt_int(OPT_BFO, 1) != 0;
    return sch.fail(octet ? octet_forward(c, mel, T, wave) : f32_forward(c, mel, T, wave));
}

// the config a handle was created with (resblock already 1 / 2): what stream.hip derives the receptive field from
const ttsamd_hifigan_cfg* hifigan_config(const HifiGan* h) { return &h->cfg; }

void hifigan_blobs(const void* hv, void** f32, int64_t* n_f32, void** b16, int64_t* n_b16) {
    const HifiGan* h = (const HifiGan*)hv;
    *f32 = h->dev; *n_f32 = h->dev_n; *b16 = h->dev16; *n_b16 = h->dev16_n;
}

}  // namespace ttsamd
