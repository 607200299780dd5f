// The two modes of the bf16 octet engine as one table (bfo.hpp: BfoMode) and the C ABI of their kernel-level entries
// (include/ttsamd.h "bf16 octet engine" / "split-bf16 (x3) mode"): the parity tests and the layer bench drive single layers through
// these; the model forwards (hifigan.hip, fastpitch.hip) call the launchers through the same table.  Every entry is written once
// against the table and emitted for both prefixes, ttsamd_bfo_* and ttsamd_bfo3_*.
#include <cstring>

#include "bfo3.hpp"
#include "kernels.hpp"

namespace ttsamd {

static bool bfo3_chain_wanted(int32_t channels, int32_t k, const int32_t* dil, int32_t n_pairs, int32_t L, int32_t) {
    return opt_int(OPT_BFO_CHAIN, 1) != 0 && bfo3_chain_supported(channels, k, dil, n_pairs, L);
}

static const BfoMode kBfoModes[2] = {
    {"bfo", 16, bfo_launch_pack, bfo_launch_unpack, bfo_launch_conv, bfo_launch_convt, bfo_launch_pair, bfo_pair_supported,
     bfo_launch_chain, bfo_chain_wanted, bfo_launch_conv_post, launch_layernorm_cf_octet},
    {"bfo3", 32, bfo3_launch_pack, bfo3_launch_unpack, bfo3_launch_conv, bfo3_launch_convt, bfo3_launch_pair, bfo3_pair_supported,
     bfo3_launch_chain, bfo3_chain_wanted, bfo3_launch_conv_post, launch_layernorm_cf_x3},
};

const BfoMode& bfo_mode(int precision) { return kBfoModes[precision == 2 ? 1 : 0]; }

static int32_t api_pack(const BfoMode& M, const float* x, int32_t batch, int32_t channels, int32_t len, float slope, void* out, void* stream) {
    TTS_REQUIRE(x && out && channels % 8 == 0 && slope > 0.f, "%s_pack: bad argument (channels %% 8 must be 0, slope > 0)", M.prefix);
    return M.pack(x, batch, channels, len, slope, out, (hipStream_t)stream);
}

static int32_t api_unpack(const BfoMode& M, const void* in, int32_t batch, int32_t channels, int32_t len, float slope, float* out, void* stream) {
    TTS_REQUIRE(in && out && channels % 8 == 0 && slope > 0.f, "%s_unpack: bad argument (channels %% 8 must be 0, slope > 0)", M.prefix);
    return M.unpack(in, batch, channels, len, slope, out, (hipStream_t)stream);
}

static int64_t api_weight_elems(const BfoMode& M, int32_t cout, int32_t cin, int32_t k, int32_t up) {
    if (cout < 1 || cin < 1 || k < 1 || up < 1) return 0;
    return up > 1 ? M.convt_elems(cin, cout, up) : M.conv_elems(cout, cin, k);
}

static int32_t api_pack_weight(const BfoMode& M, const float* w, int32_t cout, int32_t cin, int32_t k, int32_t up, uint16_t* out) {
    TTS_REQUIRE(w && out && cout >= 1 && cin >= 1 && k >= 1 && up >= 1, "%s_pack_weight: bad argument", M.prefix);
    if (up > 1) {
        TTS_REQUIRE(k == 2 * up && cin % 16 == 0, "%s_pack_weight: transposed convs need kernel = 2 * stride and Cin %% 16 == 0", M.prefix);
        M.pack_convt_weight(w, cin, cout, up, out);
    } else {
        M.pack_conv_weight(w, cout, cin, k, out);
    }
    return 0;
}

static int32_t api_conv1d(const BfoMode& M, const void* x, const void* w_packed, const float* bias, const void* res, const void* sum_in,
                          const int64_t* lens, int32_t len_mul, int32_t batch, int32_t cin, int32_t cout, int32_t k,
                          int32_t dilation, int32_t up, int32_t len_in, int32_t mode, float div, float res_slope,
                          float out_slope, void* y, float* y_f32, const float* res_f32, void* stream) {
    TTS_REQUIRE(x && w_packed && (y || y_f32) && batch >= 1, "%s_conv1d: null argument", M.prefix);
    TTS_REQUIRE(mode >= 0 && mode <= 2 && out_slope >= 0.f && (!res || res_slope > 0.f), "%s_conv1d: bad mode / slope", M.prefix);
    BfoConvParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.y = y; p.w = w_packed; p.bias = bias; p.res = res; p.sum_in = sum_in; p.lens = lens;
    p.len_mul = len_mul; p.Lin = len_in; p.batch = batch; p.Cin = cin; p.Cout = cout; p.K = k; p.dil = dilation; p.up = up;
    p.mode = mode; p.div = div; p.res_slope = res ? res_slope : 1.f; p.out_slope = out_slope;
    p.y_f32 = y_f32; p.res_f32 = res_f32;
    hipStream_t s = (hipStream_t)stream;
    prof_begin(s, 2.0 * cout * cin * k);
    const int32_t rc = up > 1 ? M.convt(p, s) : M.conv(p, s);
    prof_end(s);
    return rc;
}

static int32_t api_resblock_pair(const BfoMode& M, const void* x, const void* w1, const float* b1, const void* w2, const float* b2,
                                 const void* sum_in, const int64_t* lens, int32_t len_mul, int32_t batch, int32_t channels,
                                 int32_t k, int32_t dilation, int32_t len, int32_t mode, float div, float in_slope,
                                 float mid_slope, float out_slope, void* y, void* stream) {
    TTS_REQUIRE(x && w1 && b1 && w2 && b2 && y && batch >= 1, "%s_resblock_pair: null argument", M.prefix);
    TTS_REQUIRE(mode >= 0 && mode <= 2 && in_slope > 0.f && mid_slope > 0.f && out_slope > 0.f, "%s_resblock_pair: bad mode / slope", M.prefix);
    BfoPairParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.y = y; p.sum_in = sum_in; p.w1 = w1; p.w2 = w2; p.b1 = b1; p.b2 = b2; p.lens = lens;
    p.len_mul = len_mul; p.L = len; p.dil = dilation; p.batch = batch; p.mode = mode; p.div = div;
    p.in_slope = in_slope; p.mid_slope = mid_slope; p.out_slope = out_slope;
    hipStream_t s = (hipStream_t)stream;
    prof_begin(s, 2.0 * (2.0 * channels * channels * k));
    const int32_t rc = M.pair(channels, k, p, s);
    prof_end(s);
    return rc;
}

static int32_t api_resblock_chain(const BfoMode& M, const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                                  const float* const* b2, const int32_t* dilations, const void* sum_in, const int64_t* lens,
                                  int32_t len_mul, int32_t batch, int32_t channels, int32_t len, int32_t mode, float div,
                                  float in_slope, float mid_slope, float out_slope, void* y, void* stream, int32_t k) {
    TTS_REQUIRE(x && w1 && b1 && w2 && b2 && dilations && y && batch >= 1, "%s_resblock_chain: null argument", M.prefix);
    TTS_REQUIRE(mode >= 0 && mode <= 2 && in_slope > 0.f && mid_slope > 0.f && out_slope > 0.f, "%s_resblock_chain: bad mode / slope", M.prefix);
    BfoChainParams p;
    std::memset(&p, 0, sizeof(p));
    p.x = x; p.y = y; p.sum_in = sum_in; p.lens = lens;
    for (int m = 0; m < 3; ++m) {
        TTS_REQUIRE(w1[m] && b1[m] && w2[m] && b2[m], "%s_resblock_chain: null weight", M.prefix);
        p.w1[m] = w1[m]; p.w2[m] = w2[m]; p.b1[m] = b1[m]; p.b2[m] = b2[m]; p.dil[m] = dilations[m];
    }
    p.len_mul = len_mul; p.L = len; p.batch = batch; p.mode = mode; p.div = div; p.k = k;
    p.in_slope = in_slope; p.mid_slope = mid_slope; p.out_slope = out_slope;
    hipStream_t s = (hipStream_t)stream;
    prof_begin(s, 3 * 2.0 * (2.0 * channels * channels * k));
    const int32_t rc = M.chain(channels, p, s);
    prof_end(s);
    return rc;
}

static int32_t api_conv_post(const BfoMode& M, const void* x, const float* w, const float* bias, const int64_t* lens, int32_t len_mul,
                             int32_t batch, int32_t channels, int32_t len, float* wave, int64_t wave_stride, void* stream) {
    TTS_REQUIRE(x && w && wave && batch >= 1, "%s_conv_post: null argument", M.prefix);
    return M.conv_post(x, w, bias, lens, len_mul, batch, channels, len, wave, wave_stride, (hipStream_t)stream);
}

}  // namespace ttsamd

using namespace ttsamd;

// the seven entries whose signatures are the same in both families; the chain entries follow (the x3 one has no `k`)
#define BFO_C_API(P, M)                                                                                                                  \
    int32_t ttsamd_##P##_pack(const float* x, int32_t batch, int32_t channels, int32_t len, float slope, void* out, void* stream) {      \
        return api_pack(M, x, batch, channels, len, slope, out, stream);                                                                 \
    }                                                                                                                                    \
    int32_t ttsamd_##P##_unpack(const void* in, int32_t batch, int32_t channels, int32_t len, float slope, float* out, void* stream) {   \
        return api_unpack(M, in, batch, channels, len, slope, out, stream);                                                              \
    }                                                                                                                                    \
    int64_t ttsamd_##P##_weight_elems(int32_t cout, int32_t cin, int32_t k, int32_t up) { return api_weight_elems(M, cout, cin, k, up); } \
    int32_t ttsamd_##P##_pack_weight(const float* w, int32_t cout, int32_t cin, int32_t k, int32_t up, uint16_t* out) {                  \
        return api_pack_weight(M, w, cout, cin, k, up, out);                                                                             \
    }                                                                                                                                    \
    int32_t ttsamd_##P##_conv1d(const void* x, const void* w_packed, const float* bias, const void* res, const void* sum_in,             \
                                const int64_t* lens, int32_t len_mul, int32_t batch, int32_t cin, int32_t cout, int32_t k,               \
                                int32_t dilation, int32_t up, int32_t len_in, int32_t mode, float div, float res_slope,                  \
                                float out_slope, void* y, float* y_f32, const float* res_f32, void* stream) {                            \
        return api_conv1d(M, x, w_packed, bias, res, sum_in, lens, len_mul, batch, cin, cout, k, dilation, up, len_in, mode, div,        \
                          res_slope, out_slope, y, y_f32, res_f32, stream);                                                              \
    }                                                                                                                                    \
    int32_t ttsamd_##P##_resblock_pair(const void* x, const void* w1, const float* b1, const void* w2, const float* b2,                  \
                                       const void* sum_in, const int64_t* lens, int32_t len_mul, int32_t batch, int32_t channels,        \
                                       int32_t k, int32_t dilation, int32_t len, int32_t mode, float div, float in_slope,                \
                                       float mid_slope, float out_slope, void* y, void* stream) {                                        \
        return api_resblock_pair(M, x, w1, b1, w2, b2, sum_in, lens, len_mul, batch, channels, k, dilation, len, mode, div, in_slope,    \
                                 mid_slope, out_slope, y, stream);                                                                       \
    }                                                                                                                                    \
    int32_t ttsamd_##P##_conv_post(const void* x, const float* w, const float* bias, const int64_t* lens, int32_t len_mul,               \
                                   int32_t batch, int32_t channels, int32_t len, float* wave, int64_t wave_stride, void* stream) {       \
        return api_conv_post(M, x, w, bias, lens, len_mul, batch, channels, len, wave, wave_stride, stream);                             \
    }

extern "C" {

BFO_C_API(bfo, kBfoModes[0])
BFO_C_API(bfo3, kBfoModes[1])

int32_t ttsamd_bfo_resblock_chain(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                                  const float* const* b2, const int32_t* dilations, const void* sum_in, const int64_t* lens,
                                  int32_t len_mul, int32_t batch, int32_t channels, int32_t len, int32_t mode, float div,
                                  float in_slope, float mid_slope, float out_slope, void* y, void* stream, int32_t k) {
    return api_resblock_chain(kBfoModes[0], x, w1, b1, w2, b2, dilations, sum_in, lens, len_mul, batch, channels, len, mode, div, in_slope,
                              mid_slope, out_slope, y, stream, k);
}

int32_t ttsamd_bfo3_resblock_chain(const void* x, const void* const* w1, const float* const* b1, const void* const* w2,
                                   const float* const* b2, const int32_t* dilations, const void* sum_in, const int64_t* lens,
                                   int32_t len_mul, int32_t batch, int32_t channels, int32_t len, int32_t mode, float div,
                                   float in_slope, float mid_slope, float out_slope, void* y, void* stream) {
    return api_resblock_chain(kBfoModes[1], x, w1, b1, w2, b2, dilations, sum_in, lens, len_mul, batch, channels, len, mode, div, in_slope,
                              mid_slope, out_slope, y, stream, 3);
}

}  // extern "C"
