// Shared host-side helpers of libttsamd (error reporting, launch checks, workspace carving).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../../include/ttsamd.h"

namespace ttsamd {

void set_error(const char* fmt, ...);

#define TTS_CHECK_HIP(expr)                                                         \
    do {                                                                            \
        hipError_t e_ = (expr);                                                     \
        if (e_ != hipSuccess) {                                                     \
            ttsamd::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                              __FILE__, __LINE__);                                  \
            return TTSAMD_EHIP;                                                     \
        }                                                                           \
    } while (0)

#define TTS_REQUIRE(cond, ...)              \
    do {                                    \
        if (!(cond)) {                      \
            ttsamd::set_error(__VA_ARGS__); \
            return TTSAMD_EINVAL;           \
        }                                   \
    } while (0)

#define TTS_TRY(expr)               \
    do {                            \
        int32_t rc_ = (expr);       \
        if (rc_ != 0) return rc_;   \
    } while (0)

inline int64_t align_up(int64_t x, int64_t a) { return (x + a - 1) / a * a; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) once per (kernel instantiation, device).  `done` is the instantiation's bitmask of
// devices already opted in; two host threads racing on a first launch both set the attribute (idempotent), devices >= 64 set it on
// every launch.  (Rounds 2-4 kept an unsynchronised bool[16] indexed by device & 15: a data race, and device 16 aliased device 0.)
inline hipError_t lds_opt_in(const void* fn, int bytes, std::atomic<uint64_t>& done) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64 && ((done.load(std::memory_order_acquire) >> dev) & 1)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && dev >= 0 && dev < 64) done.fetch_or(1ull << dev, std::memory_order_release);
    return e;
}

// ---- run-time routing options (include/ttsamd.h: ttsamd_set_option / ttsamd_get_option) -----------------------------------------------
// Every switch that routes between kernels / schedules that BOTH ship.  One table (api.hip): the value is seeded ONCE from the
// environment variable TTSAMD_<NAME> when the library is first used, validated (a malformed value is an error of ttsamd_options_check and
// of every ttsamd_set_option call, never silently ignored), and changed afterwards only through ttsamd_set_option -- product code never calls
// getenv on a hot path (a forward used to make several hundred getenv calls, each racing with a concurrent setenv of the host).
// X(name, kind, lo, hi): kind 0 = decimal integer in [lo, hi], 1 = hex mask <= hi.
#define TTS_OPTIONS(X)                                                                                     \
    X(HIFIGAN_STREAMS, 0, 0, 1)   /* ResBlock branches of a HiFi-GAN stage on one / three streams (default: by size) */ \
    X(WINO, 0, 0, 1)              /* fp32 engine: 0 = direct kernels only */                                \
    X(WINO2, 0, 0, 31)            /* F(2,3) decomposition kernel: bit 0 / 1 / 2 = k 3 / 7 / 11, 3 = dilated, 4 = Cout 64 */ \
    X(WINO4, 0, 0, 255)           /* F(4,3) decomposition kernel: bit 0 / 1 / 2 = k 3 / 7 / 11, 3 = dilated, 4 = k 1, 5 / 6 = k 7 / 11 on seven-point groups, 7 = packed tiles + register epilogue of the dilated launches */ \
    X(FUSED_PAIR, 0, 0, 1)        /* fp32 fused c1 -> c2 pairs: 0 = every pair as two launches */           \
    X(FUSED2, 0, 0, 1)            /* second-generation fused pair off / on */                               \
    X(FUSED2_MASK, 1, 0, 0x1ff)   /* which (C, k) pairs it takes: bit 3 ci + ki (default 00f) */            \
    X(FUSED2_MASK_N1, 1, 0, 0x1ff) /* ... with 128-column direct-arithmetic blocks (default 000) */         \
    X(FUSED2_WB, 0, 0, 2)         /* its Winograd phases: 0 none, 1 phase B, 2 both (default) */            \
    X(PAIR4, 0, 0, 2)             /* C = 32 fused pairs with both convs on Winograd F(4,3) (resblock_pair4): 0 off, 1 on (seven-point groups where routed), 2 on six-point groups */ \
    X(CONVT, 0, 0, 1)             /* all-phase transposed conv (convt_mfma.hip) off / on */                 \
    X(CONVT_WINO, 0, 0, 2)        /* fp32 upsamplers on Winograd F(4,2) (conv_wino4.hip): 0 off, 1 default routing, 2 wherever supported */ \
    X(BFO, 0, 0, 1)               /* bf16 modes: 0 = the round-2 bf16 conv engine instead of the octet engine */ \
    X(BFO_CHAIN, 0, 0, 1)         /* whole k = 3 ResBlock in one launch (octet engines) */                  \
    X(BFO_CHAIN7, 0, 0, 1)        /* ... and k = 7 (default: small batches only) */                         \
    X(BFO_FF, 0, 0, 1)            /* FastPitch conv-FF / predictors on the octet engine */                  \
    X(BFO_SPLITK, 0, 0, 1)        /* split-K of the octet slab conv */                                      \
    X(BFO_SMALL_TILES, 0, 0, 1)   /* 128-column tiles of the bf16 pair (default: by block count) */         \
    X(BF16_ATTN, 0, 0, 1)         /* bf16 MFMA attention in the bf16 mode */                                \
    X(BF16_PACKED_T, 0, 0, 1)     /* round-2 bf16 engine: packed bf16 c1 -> c2 intermediate */              \
    X(ATT_RA, 0, 1, 4)            /* fp32 attention: 16 * RA queries per block (1, 2, 4) */                 \
    X(ATT_SPLIT, 0, 0, 1)         /* ... one block per (16 queries, key tile) + merge launch */             \
    X(XCD_W, 0, 0, 1)             /* XCD-aware block -> tile map of the direct conv kernel */               \
    X(XCD_WMAX_KB, 0, 0, 1 << 20) /* ... weight footprint per XCD that keeps co-tile classes together */    \
    X(DEEP_SPLITK, 0, 0, 1)       /* 128 x 64 tiles with split K for the deep conv-FF conv at batch 7..13 */ \
    X(TACO_PERSISTENT, 0, 0, 2)   /* Tacotron2 decoder: 0 graph replay, 1 grid-barrier kernel, 2 dataflow kernel */ \
    X(TACO_SEG, 0, 8, 1 << 20)    /* ... decoder steps per persistent launch (default 512) */ \
    X(RESBLOCK2_PAIR, 1, 0, 0x3f) /* ResBlock2 as one launch (resblock2.hip): bit 3 ci + ki, C = 32 / 64, k = 3 / 5 / 7 */
enum Opt : int {
#define TTS_OPT_ENUM(name, kind, lo, hi) OPT_##name,
    TTS_OPTIONS(TTS_OPT_ENUM)
#undef TTS_OPT_ENUM
    OPT_COUNT
};
// current value as a number (parsed with the table's base), or `unset` when the option is not set (the documented default applies)
int64_t opt_int(Opt o, int64_t unset);

// Bump allocator over the caller-provided workspace (no hidden hipMalloc on hot calls).
struct Arena {
    char* base;
    int64_t size;
    int64_t off = 0;
    bool ok = true;
    Arena(void* p, int64_t n) : base((char*)p), size(n) {}
    template <typename T>
    T* take(int64_t count) {
        int64_t bytes = align_up(count * (int64_t)sizeof(T), 256);
        if (base != nullptr && off + bytes > size) ok = false;
        T* r = base ? (T*)(base + off) : nullptr;
        off += bytes;
        return r;
    }
};

// ---- generic implicit-GEMM conv1d (conv_mfma.hip) -----------------------------------
struct ConvParams {
    const float* x;      // [B][Cin][*], element (b,c,t) at x + b*x_bs + c*x_cs + t
    int64_t x_bs;
    int32_t x_cs;
    const float* w;      // packed fp32 weights [n_phase][Cin/8][K][2][CoutP][4]
    const void* w_bf16;  // same element order as bf16: plane hi then plane lo (nullptr if not packed)
    const float* w_wino; // k = 3 / 7 / 11: the Winograd F(2,3) group filters [Cin/8][wino2_groups(k)][2][CoutP][4] (pack_wino2_weight, conv_wino2.hip; k = 3: four taps, also conv_wino.hip's; nullptr = none)
    const float* w_wino4; // k = 3 / 7 / 11: the Winograd F(4,3) group filters [Cin/8][wino4_groups(k)][2][CoutP][4] (conv_wino4.hip; nullptr = none)
    int32_t precision;   // 0 fp32 MFMA, 1 bf16 MFMA, 2 split bf16 (3 MFMAs per product)
    const float* bias;   // [>=Cout] or nullptr
    float* y;            // (b,co,q) at y + b*y_bs + co*y_cs + q*y_ts + phase
    int64_t y_bs;
    int32_t y_cs, y_ts;
    const float* res;    // residual, same indexing as y (nullptr = none)
    int64_t r_bs;
    int32_t r_cs;
    const int64_t* lens_in;   // per-utterance valid input length = lens_in[b]*len_in_mul (nullptr -> Lin)
    const int64_t* lens_out;  // per-utterance number of outputs  = lens_out[b]*len_out_mul (nullptr -> Nout)
    int32_t len_in_mul, len_out_mul;
    int32_t Lin, Nout;
    int32_t Cin, Cout, CoutP, K;
    int32_t dil, pad;    // input position of tap k for output q: q + k*dil - pad
    int32_t n_phase;     // >1: transposed conv as n_phase polyphase convs (K=2, dil=-1)
    int32_t phase_p;     // transposed conv padding p: delta = (phase+p)/n_phase, pad = -delta
    float in_slope;      // leaky-relu slope applied to the input on load (1 = identity)
    const float* scale;  // per-output-channel factor applied after the bias, before the residual (nullptr = 1)
    int32_t relu_out;    // output activation: 0 none, 1 ReLU, 2 GELU (erf), 3 tanh (after the residual)
    int32_t mode;        // 0: y=v   1: y=y+v   2: y=(y+v)/div
    float div;
    int32_t batch;
    // split-K for problems that cannot fill the chip (batch 1, encoder-side S = 64): when splitk_ws is set and
    // the tile grid is small (conv_route.hip: direct engine < 320 blocks, aiming at 640; F(4,3) < 192, aiming at 224), the Cin range is
    // cut into `ksplit` slices (extra grid factor) that write raw partial sums to splitk_ws[ks][b][Cout][Nout]; a second kernel sums
    // them and applies the epilogue.
    float* splitk_ws;         // >= splitk_floats floats of scratch, or nullptr (never split)
    int64_t splitk_floats;
    int32_t ksplit;           // set by the launcher
    // bf16 mode only (precision 1): activations that only feed the next conv can cross HBM as bf16 in the LDS entry
    // order [B][C/8][2 (kk)][L][4 bf16] (entry (o,kk,t) = channels 8o+kk+{0,2,4,6} at position t), already
    // leaky-relu'd with the consumer's slope and rounded RNE: the consumer's staging is then a plain 8-byte copy.
    int32_t y_packed;         // write y in that layout (requires Cout % 8 == 0, y_ts == 1, mode 0, no phases)
    float pack_slope;         // ... after applying leaky-relu with this slope
    int32_t x_packed;         // read x in that layout (x_cs = positions per row; in_slope is ignored)
    int32_t xcd_w;            // set by the launcher: gcd(n_co_tiles, 8) co-tile classes, one per XCD residue (weight locality; 0 = off)
    int32_t tile_major;       // 1: blockIdx.x = utterance slot, blockIdx.z = time tile (ragged batches); the launchers pass 0
    int32_t compact;          // set by the launcher (ragged batches): the (utterance, time tile) pair of a block is looked up in the
                              // utterance-major list of LIVE tiles (live_tile below), so every dead block sits at the end of the grid
    unsigned long long* timing;   // unused (nullptr); kept so the kernel argument layout is unchanged
    const float* w_wino44; // k = 7 / 11: the same conv as SEVEN-point groups [Cin/8][wino44_groups(k)][2][CoutP][4] (conv_wino4.hip, TTSAMD_WINO4 bits 5 / 6;
                           // nullptr = none: the launch stays on w_wino4).  Both forms travel with a launch, the switch picks one per launch
    int32_t res_late;      // direct kernels: 1 = add the residual behind the finished sum, never preload it into the accumulators.  A preloaded
                           // residual makes every rounding of the Cin * K sum as large as the residual's: fine where conv and residual are of
                           // one size (ResBlocks, FFT blocks), ten times the fp32 noise where the residual is the output and the conv a small
                           // correction to it (Tacotron2 postnet: mel + postnet(mel), 2560 terms)
};
constexpr int64_t kSplitKFloats = 4 << 20;   // 16 MB covers every case the launchers pick (direct kernel: < 320 blocks, ~640 blocks wanted; conv_wino4.hip: four C-in slices of a 1 x 256 x 3584 launch = 3.7 M floats)
constexpr int64_t kSplitKFloatsFp = 8 << 20; // FastPitch: 32 MB, the deep conv-FF conv (1536 -> 384) splits K at batch 4..13 too

void conv_log(const char* kind, int K, int cin, int cout, int nout, int batch, int has_res, int mode, int len_mul, int ragged,
              int n_phase);
// block order of a launch (conv_mfma.hip)
bool compact_order(const void* lens, int batch);
// Launches the kernel; returns 0 or a negative code.
int32_t launch_conv(const ConvParams& p, hipStream_t stream);
// Routing of an exact-fp32 launch_conv (conv_route.hip): decided once per launch, by a function that launches nothing.
struct ConvRouteOpts { int wino, wino2, wino4, deep_splitk; };   // the options a route depends on, snapshotted once per launch
struct ConvRoute {
    int id;       // what note_conv_launch records: 0 direct, 1 / 2 F(2,3), 3 / 4 F(4,3) six- / seven-point, 7 / 8 their packed strip form;
                  // -1: no kernel takes it (kernel size not built, C-in no multiple of the tile's chunk) -- the direct launcher reports it
    int ksplit;   // C-in slices (1 = none), direct and F(4,3) alike
    int epi;      // F(4,3): the epilogue kind of conv1d_wino4_f32, 0 / 3 / 4 / 7
    int co_blk, nt_blk;   // direct engine: rows x columns of the tile
};
ConvRouteOpts conv_route_opts();                                   // the only place the fp32 conv path calls opt_int for these four
ConvRoute conv_route(const ConvParams& p, const ConvRouteOpts& o);  // pure: no opt_int, no globals, no HIP call, no allocation
// rows of y (and of the residual) are 16-byte aligned: what every float4 row epilogue asks
inline bool conv_rows_aligned(const ConvParams& p) {
    return (p.y_cs & 3) == 0 && (p.y_bs & 3) == 0 && ((uintptr_t)p.y & 15) == 0 &&
           (!p.res || ((p.r_cs & 3) == 0 && (p.r_bs & 3) == 0 && ((uintptr_t)p.res & 15) == 0));
}
// input channels per chunk of the direct engine's co_blk x nt_blk tile (conv_mfma.hip: Geo::KC).  k = 3 on the 128 x 128 tile takes two
// octets: a one-octet chunk is 48 MFMAs per wave (1.3 us) between barriers; two halve the barriers and still leave two blocks per CU
// (FastPitch's 384 -> 1536 conv 121 -> 128 TFLOP/s, HiFi-GAN C = 128 k = 3 106 -> 108; the smaller k = 3 tiles lose 2-3 % with it)
constexpr int conv_chunk_channels(int k, int nt_blk, int co_blk) {
    return (k == 3 && nt_blk == 128 && co_blk == 128) ? 16 : (k == 1 ? 32 : (k == 2 ? 16 : 8));
}
// What the calling thread's last fp32 conv launch decided (ttsamd_conv_last_launch; conv_mfma.hip): two thread_local ints, written by
// launch_conv with its ConvRoute and by the transposed-conv launchers.  route 0: direct kernel, 1 / 2: the F(2,3) kernels (conv_wino.hip / conv_wino2.hip), 3 / 4: F(4,3)
// on six- / seven-point groups, 5: the all-phase transposed conv (convt_mfma.hip), 6: the transposed conv as a two-tap conv on F(4,2)
// (launch_convt_wino, conv_wino4.hip), 7 / 8: F(4,3) on six- / seven-point groups in the PACKED strip form (dilation 3 / 5, packed tiles and
// the register epilogue: conv_wino4.hip EPI 7, TTSAMD_WINO4 bit 7).  Host only, no atomics.
void note_conv_launch(int32_t route, int32_t ksplit);
void last_conv_launch(int32_t* route, int32_t* ksplit);
// ConvTranspose1d with all output phases per wave (convt_mfma.hip): takes the polyphase ConvParams of the generic engine
bool convt_supported(const ConvParams& p);
int32_t launch_convt(const ConvParams& p, hipStream_t stream);
// One HiFi-GAN upsampler, leaky_relu + ConvTranspose1d(stride u, kernel kt, padding (kt - u) / 2): fills the polyphase fields of `p`
// (the caller has set batch, lens_in / lens_out and whatever it shares between its launches) and launches the all-phase kernel where
// `convt_ok` and convt_supported(p) say so, else the generic engine.  x [B][cin][L], y [B][cout][L * u], w / w_bf16 packed by
// pack_convt_weight (and split_packed_bf16); valid lengths lens * len_mul in, lens * len_mul * u out.
// w_wino / bias_wino: the same upsampler packed by pack_convt_wino_weight (nullptr = not packed: never routed to the F(4,2) launch).
int32_t launch_upsampler(ConvParams& p, const float* x, const float* w, const void* w_bf16, const float* bias, float* y, int cin, int cout,
                         int u, int kt, int L, int len_mul, float in_slope, bool convt_ok, hipStream_t stream, const float* w_wino = nullptr,
                         const float* bias_wino = nullptr);
// ConvTranspose1d(stride u, kernel 2u, padding u/2) as a two-tap Conv1d with u Cout rows on the F(4,3) kernel's k = 3 form with a zero
// third tap = F(4,2), five products per output quad and phase instead of eight (conv_wino4.hip: launch_convt_wino; route 6).
// convt_wino_packable: the shapes the packing exists for (u = 2 / 8, Cin % 16 == 0, u Cout % 64 == 0).  pack_convt_wino_weight: torch
// [Cin][Cout][2u] -> the group filters U0..U4 + a zero group of the taps (W[..][j + u], W[..][j], 0), row = co u + j, in the layout
// [Cin/8][6][2][u Cout][4] (6 cin u cout floats), and the bias per ROW (bias[row / u]; u cout floats, zeros without a bias).
// convt_wino_supported takes the polyphase ConvParams that launch_upsampler fills.
bool convt_wino_packable(int cin, int cout, int u);
void pack_convt_wino_weight(const float* w, const float* bias, int cin, int cout, int u, float* out_w, float* out_bias);
bool convt_wino_supported(const ConvParams& p, const float* w_wino, const float* bias_wino);
int32_t launch_convt_wino(const ConvParams& p, const float* w_wino, const float* bias_wino, hipStream_t stream);
// Routing of an exact-fp32 c1 -> c2 pair of a ResBlock1 (conv_route.hip): which of the three fused kernels takes it as ONE launch with
// the intermediate in LDS, and in which form -- decided once per pair, by a function that launches nothing.  launch_pair executes the
// answer; hifigan_forward and ttsamd_resblock_pair both go through it, ttsamd_resblock_pair_route asks without launching.
struct PairRouteOpts { int fused_pair, fused2, fused2_mask, fused2_mask_n1, fused2_wb, pair4; };   // fused2_mask < 0: not forced (the default mask)
struct ConvForms { bool wino2, wino4, wino44; };   // the Winograd forms a conv carries: F(2,3) groups, F(4,3) six-point, seven-point
// The pair: L positions per row (after the stage's upsampling), batch rows; square: c1 and c2 are both C -> C convs of the same k; x / y
// for their alignment and distinctness only, never followed; forms: what BOTH convs carry
struct PairShape { int32_t channels, k, dil, L, batch; bool square; const float *x, *y; ConvForms forms; int32_t precision; };
enum PairKernel : int32_t { PAIR_NONE = 0, PAIR_GEN1 = 1, PAIR_GEN2 = 2, PAIR_F43 = 3 };   // two launch_conv calls / resblock_pair / resblock_pair2 / resblock_pair4
// ntw, wm (resblock_pair2): 2 / 1 = 256- / 128-column blocks; phases on Winograd F(2,3), 0 none, 1 phase B (conv 2), 2 both.  points
// (resblock_pair4): 6 / 7 = six- / seven-point groups.  name: what the launch is logged under (TTSAMD_CONV_LOG); "" for PAIR_NONE
struct PairRoute { int32_t kernel, ntw, wm, points; const char* name; };
PairRouteOpts pair_route_opts();                                   // the only place the pair path calls opt_int for these six
PairRoute pair_route(const PairShape& s, const PairRouteOpts& o);  // pure: no opt_int, no globals, no HIP call, no allocation
PairRoute pair_route_of_variant(int32_t variant, int32_t channels, int32_t dil);   // the forced routes of ttsamd_resblock_pair (variant 1..7)
bool pair2_phases_built(int32_t channels, int32_t dil, int32_t ntw, int32_t wm);   // resblock_pair2<.., ntw, wm> exists for this pair
ConvForms hifigan_conv_forms(int cin, int cout, int k);            // what hifigan_create packs for a conv besides the direct layout
// one conv of a pair in every form it was packed in (nullptr = not packed); the route says which ones the launch reads
struct PairConv { const float *w, *b, *w_wino2, *w_wino4, *w_wino44; };
// one pair launch: v = x + conv(lrelu(conv(lrelu(x), c1, dil) + b1), c2) + b2;  y = v | y + v | (y + v) / div by mode 0 | 1 | 2.  x != y
struct PairArgs { int32_t channels, k, dil; const float* x; float* y; PairConv c1, c2; const int64_t* lens; int32_t len_mul, L, batch, mode; float div, slope; };
int32_t launch_pair(const PairRoute& r, const PairArgs& a, hipStream_t stream);
// The three kernels: the geometry each is built for (pair_route and the launcher's own argument check ask), and the launcher.
// First generation (resblock_fused.hip): C = 32, k = 3 / 7 / 11 and C = 64, k = 3.
bool fused_pair_supported(int32_t channels, int32_t k, int32_t dil, int32_t L, const float* x, const float* y);
int32_t launch_fused_pair(const PairArgs& a, hipStream_t stream);
// Second generation (resblock_fused2.hip): weights from L2 into a register queue, raw window, 5 barriers per block; C = 32 / 64 / 128
// at k = 3 / 7 / 11.  r.ntw / r.wm pick the instantiation: conv 2 / conv 1 are read as Winograd F(2,3) groups (pack_wino2_weight)
// where r.wm >= 1 / == 2.
bool fused_pair2_supported(int32_t channels, int32_t k, int32_t dil, int32_t L, const float* x, const float* y, int32_t ntw);
int32_t launch_fused_pair2(const PairArgs& a, const PairRoute& r, hipStream_t stream);
// The C = 32 pair with both convs on Winograd F(4,3) (resblock_pair4.hip): k = 3 / 7 / 11, dilation 1 / 3 / 5; the weights are the
// F(4,3) group filters of both convs (r.points = 6: pack_wino4_weight; 7, k = 7 / 11 only: the seven-point groups of
// pack_wino44_weight at 32 x 32, [4][wino44_groups(k)][2][32][4])
bool fused_pair4_supported(int32_t channels, int32_t k, int32_t dil, int32_t L, const float* x, const float* y);
int32_t launch_fused_pair4(const PairArgs& a, const PairRoute& r, hipStream_t stream);
// HiFi-GAN ResBlock2 (resblock2.hip), exact fp32: one conv y = x + conv(lrelu(x), w, dil) + b with the stage-sum epilogue (C = 32 / 64 /
// 128, k = 3 / 5 / 7 / 11, dilation 1..16), and both convs of a ResBlock2 in one launch (C = 32 / 64).  Direct weight packing
// (pack_conv_weight); x != y.
bool resblock2_conv_supported(int32_t channels, int32_t k, int32_t dil, int32_t L, const float* x, const float* y);
int32_t launch_resblock2_conv(int32_t channels, const float* x, float* y, const float* w, const float* b, int32_t k, int32_t dil,
                              const int64_t* lens, int32_t len_mul, int32_t L, int32_t batch, int32_t mode, float div, float slope,
                              hipStream_t stream);
bool resblock2_pair_supported(int32_t channels, int32_t k, int32_t d1, int32_t d2, int32_t L, const float* x, const float* y);
int32_t launch_resblock2_pair(int32_t channels, const float* x, float* y, const float* w1, const float* b1, const float* w2,
                              const float* b2, int32_t k, int32_t d1, int32_t d2, const int64_t* lens, int32_t len_mul, int32_t L,
                              int32_t batch, int32_t mode, float div, float slope, hipStream_t stream);
// Winograd F(2,3) path of the k = 3, dilation-1 convs (conv_wino.hip): launcher, host-side filter transform + packing
int32_t launch_wino(const ConvParams& p, hipStream_t stream);
void pack_wino_weight(const float* w, int cout, int cin, float* out);   // out: cin * 4 * cout_padded(cout) floats
// ... and its generalisation to k = 7 / 11 as sums of F(2,3) sub-filters + single taps (conv_wino2.hip): NG = wino2_groups(k) operand
// groups per octet, weights [Cin/8][NG][2][CoutP][4] (k = 3: identical to pack_wino_weight)
int wino2_groups(int k);
// outputs per tile at dilation d (see the kernel): the largest multiple of 2 d and of 4 in 2 * npair
__device__ __host__ constexpr int wino2_tile(int d, int npair) { return (2 * npair / ((d & 1) ? 4 * d : 2 * d)) * ((d & 1) ? 4 * d : 2 * d); }
int32_t launch_wino2(const ConvParams& p, hipStream_t stream);
void pack_wino2_weight(const float* w, int cout, int cin, int k, float* out);   // out: cin * wino2_groups(k) * cout_padded(cout) floats
// ... and the F(4,3) decomposition (conv_wino4.hip: 6 / 16 / 23 products per output QUAD at k = 3 / 7 / 11): 64 rows x 64 quads per block
int wino4_groups(int k);                         // groups per octet in the packed weights: 6 / 16 / 24 (k = 11: 23 + one zero group)
int wino44_groups(int k);                        // ... of the seven-point form: 13 / 20 at k = 7 / 11 (0: no such form)
constexpr int kWino4Default = 255;               // TTSAMD_WINO4 when unset
// outputs per tile at dilation d: the largest multiple of 4 d in 4 * ntup
__device__ __host__ constexpr int wino4_tile(int d, int ntup) { return (4 * ntup / (4 * d)) * (4 * d); }
// PACKED tiles of the dilated F(4,3) launches (conv_wino4.hip, EPI 7).  A row of n outputs at dilation d is cut into G = ceil(n / 4d)
// groups of 4 d columns = T = d G tuples; tuple t holds the columns (t / d) 4d + t % d + j d, j = 0..3, and tile i the tuples
// [64 i, 64 i + 64): every tuple slot of every tile but a row's last is live (the plain tile -- the largest multiple of 4 d columns in
// 256 -- leaves 1 of 64 slots idle at d = 3 and 4 at d = 5).  A tile then starts at residue r0 = 64 i % d inside its first group, which
// begins at column q0 = (64 i / d) 4d, and slot pe of the tile sits at q0 + wino4_pk_col(r0 + pe, d).  The launcher (grid), the kernel
// (block -> tile) and live_tile below all count tiles with these; at d = 1 the map is the plain one.
__host__ __device__ constexpr int wino4_pk_tuples(int n, int d) { return d * ((n + 4 * d - 1) / (4 * d)); }
__host__ __device__ constexpr int wino4_pk_tiles(int n, int d) { return (wino4_pk_tuples(n, d) + 63) / 64; }
__host__ __device__ constexpr int wino4_pk_col(int t, int d) { return (t / d) * 4 * d + t % d; }      // first column of tuple t
__host__ __device__ constexpr int wino4_pk_q0(int tile, int d) { return (64 * tile / d) * 4 * d; }
__host__ __device__ constexpr int wino4_pk_r0(int tile, int d) { return 64 * tile % d; }
int32_t launch_splitk_reduce(const ConvParams& q, hipStream_t stream);   // conv_mfma.hip: y = epilogue(sum of the ksplit partial tensors)
int32_t launch_wino4(const ConvParams& p, const ConvRoute& r, hipStream_t stream);   // r.id 3 / 4 / 7 / 8
void wino4_filter_groups(const float* g, int k, float* o);                      // one (co, ci) filter -> its wino4_groups(k) group filters
void pack_wino4_weight(const float* w, int cout, int cin, int k, float* out);   // out: cin * wino4_groups(k) * cout_padded(cout) floats
void wino44_filter_groups(const float* g, int k, float* o);                     // k = 7 / 11: one filter -> its wino44_groups(k) seven-point group filters
void pack_wino44_weight(const float* w, int cout, int cin, int k, float* out);  // out: cin * wino44_groups(k) * cout_padded(cout) floats
// Host-side weight re-layout: torch Conv1d [Cout][Cin][K] -> [Cin][K][CoutP]
void pack_conv_weight(const float* w, int cout, int cin, int k, float* out);
// torch ConvTranspose1d [Cin][Cout][Kt] (Kt = 2u, stride u, padding p) -> [u][Cin][2][CoutP]
void pack_convt_weight(const float* w, int cin, int cout, int kt, int u, int p, float* out);
inline int cout_padded(int cout) { return (int)align_up(cout, 32); }
void split_packed_bf16(const float* packed, int64_t n, uint16_t* out);
// process-wide default MFMA precision of the model forwards (ttsamd_set_precision)
int32_t default_precision();

#ifdef __HIPCC__
// Ragged batches, dead blocks last.  A grid of (time tiles of the LONGEST utterance) x batch has a run of dead blocks
// (tiles past the utterance's own length) behind every utterance; a dead block still needs a free slot (LDS, four
// waves) to launch and exit, and the in-order workgroup dispatcher cannot place the live block queued behind it: with
// utterances 16 % shorter than the padded length on average a stand-alone C = 128 k = 11 launch runs at 124.5 TFLOP/s
// against 137 on a uniform batch.  Instead, block number `lin` of the utterance-major order takes the lin-th LIVE
// (utterance, tile) pair and all dead blocks sit at the end of the grid
// (133.8 TFLOP/s on that launch; C = 256 k = 11 119 -> 130, C = 64 k = 11 120 -> 126): every wave loads the lengths
// (64 per pass), takes a wave prefix sum of the tile counts and finds its utterance with one ballot -- a few dozen
// cycles next to the length load the kernel does anyway.  Returns false past the last live pair.
// (A persistent variant -- as many blocks as the chip holds, tiles handed out by a device counter -- measured 1-3 %
// BELOW this on the ragged launches and 3-4 % below the plain grid on uniform ones; not kept.)
// EXTRA = 1 (the transposed conv on the F(4,2) kernel, conv_wino4.hip): a row of length len > 0 has len + 1 positions, one of length 0 none.
// PK_DIL > 0 at run time (PACKED only: the packed tiles above at that dilation): a row has wino4_pk_tiles(len, PK_DIL) tiles; tile_w is unused.
template <int EXTRA = 0, bool PACKED = false>
__device__ __forceinline__ bool live_tile(const int64_t* __restrict__ lens, const int mul, const int n_max, const int tile_w,
                                          const int batch, const unsigned lin, int& b, int& tile, const int pk_dil = 0) {
    const int lane = threadIdx.x & 63;
    unsigned base = 0;
    for (int u0 = 0; u0 < batch; u0 += 64) {
        int n = 0;
        if constexpr (EXTRA != 0) {
            if (u0 + lane < batch) {
                const int len = (int)lens[u0 + lane] * mul;
                n = (max(min(n_max, len > 0 ? len + EXTRA : 0), 0) + tile_w - 1) / tile_w;
            }
        } else if constexpr (PACKED) {
            if (u0 + lane < batch) n = wino4_pk_tiles(max(min(n_max, (int)lens[u0 + lane] * mul), 0), pk_dil);
        } else {
            if (u0 + lane < batch) n = (max(min(n_max, (int)lens[u0 + lane] * mul), 0) + tile_w - 1) / tile_w;
        }
        int incl = n;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        const unsigned total = (unsigned)__shfl(incl, 63, 64);
        if (lin < base + total) {
            const unsigned long long m = __ballot(base + (unsigned)incl > lin);   // first lane whose inclusive sum passes lin
            const int l = __ffsll((long long)m) - 1;
            b = u0 + l;
            tile = (int)(lin - base) - (__shfl(incl, l, 64) - __shfl(n, l, 64));
            return true;
        }
        base += total;
    }
    return false;
}

// K float64 sums over a block of NW waves in a fixed order, so that two runs agree bit for bit: a butterfly over the lanes of each
// wave, then the waves in ascending order.  Every thread leaves with the K totals in v; red is the block's scratch in LDS.  Holds a
// __syncthreads(): the whole block calls it.
template <int NW, int K>
__device__ __forceinline__ void block_sum_fixed(double (&v)[K], double (&red)[K][NW]) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int q = 0; q < K; ++q) v[q] += __shfl_xor(v[q], d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) red[q][threadIdx.x >> 6] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) {
        v[q] = red[q][0];
#pragma unroll
        for (int u = 1; u < NW; ++u) v[q] += red[q][u];
    }
}
#endif

}  // namespace ttsamd
