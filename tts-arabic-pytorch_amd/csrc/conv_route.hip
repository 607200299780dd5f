// Routing of an exact-fp32 conv launch (launch_conv, conv_mfma.hip): which kernel, in which form, in how many C-in slices.  Host only, no
// kernel here: conv_route decides from the launch and ONE snapshot of the switches and launches nothing; the launchers (conv_mfma.hip,
// conv_wino.hip, conv_wino2.hip, conv_wino4.hip) execute what it returned, and ttsamd_conv1d_route (api.hip) asks without launching.
// Below it, the same for a c1 -> c2 pair of a ResBlock1: pair_route decides which fused kernel takes the pair (resblock_fused.hip,
// resblock_fused2.hip, resblock_pair4.hip) and in which form, launch_pair executes it for hifigan_forward and ttsamd_resblock_pair alike,
// and ttsamd_resblock_pair_route asks without launching.
//   TTSAMD_WINO=0        everything on the direct kernel
//   TTSAMD_WINO2=<mask>  what the F(2,3) decomposition kernel takes: bit 0 / 1 / 2 = k 3 / 7 / 11, bit 3 = their dilated (3 / 5) convs, bit 4
//                        = Cout = 64.  Default 31 (same-box A/B of the bench step, tools/ab_env.sh: 74.2 ms with none, 73.1 with k = 3,
//                        68.5 with k = 7 + 11, 67.5 with the three, 65.6 with dilations, 64.6-65.1 with Cout = 64)
//   TTSAMD_WINO4=<mask>  what the F(4,3) decomposition kernel takes: bit 0 / 1 / 2 = k 3 / 7 / 11, bit 3 = their dilated convs, bit 4 = k 1,
//                        bit 5 / 6 = what it takes of k = 7 / 11 runs on seven-point groups (13 / 20 products per quad instead of 16 / 23:
//                        same tile, same conditions), bit 7 = the packed strip form of the dilated launches; default 255.
//                        (k = 3 -- 6 instead of 8 products per quad -- did not pay with the kernel's first staging path: 414 / 330 vs
//                        392 / 315 us on FastPitch's conv-FF pair; with the aligned 16-byte window loads it does: same-box A/B of the step
//                        55.46 (mask 14) vs 54.68 ms.)
#include <algorithm>

#include "common.hpp"

namespace ttsamd {

ConvRouteOpts conv_route_opts() {
    return {(int)opt_int(OPT_WINO, 1), (int)opt_int(OPT_WINO2, 31), (int)opt_int(OPT_WINO4, kWino4Default), (int)opt_int(OPT_DEEP_SPLITK, 1)};
}

// F(4,3), 64 rows x 64 quads per block: C-in slices of a launch that cannot fill the chip by its `blocks` tiles alone (batch 1: HiFi-GAN's
// C = 256 stage is 56 blocks): enough for ~224 blocks, at least eight chunks per slice, partial sums within the caller's split-K
// workspace.  1 = no split.
static int wino4_ksplit(const ConvParams& p, int64_t blocks) {
    // (more slices / a higher block threshold were measured: no change at batch 1, 2.34-2.40 ms at every setting -- profiles/r6/NOTES.md)
    constexpr int sk_blocks = 192, sk_target = 224;
    if (blocks >= sk_blocks || p.splitk_ws == nullptr) return 1;
    const int n_chunks = p.Cin / (p.K == 1 ? 32 : (p.K == 3 ? 16 : 8));
    const int64_t per = (int64_t)p.batch * p.Cout * p.Nout;
    // at least 8 chunks per slice: a block of 4-5 chunks is mostly prologue and output transform (FastPitch's conv-FF at batch 1 -- 48 / 12
    // blocks x 24 / 96 chunks -- ran 30 % slower on 5 / 19 slices than on the direct kernel's split-K tiles)
    int64_t ks = std::min<int64_t>((sk_target + blocks - 1) / blocks, n_chunks / 8);
    ks = std::min<int64_t>(ks, p.splitk_floats / std::max<int64_t>(per, 1));
    return ks >= 2 ? (int)ks : 1;
}

// The direct engine (conv_mfma.hip).  Tile choice: the largest tile that still gives the chip >= 3 blocks per CU (768); small
// problems (batch 1, encoder-side S = 64) fall back to smaller tiles to fill the 256 CUs.  Then split K where even those do not.
// id -1: the kernel size is not built, or C-in is no multiple of the tile's chunk -- the launcher reports it.
static ConvRoute route_direct(const ConvParams& p, const ConvRouteOpts& o) {
    const int K = p.K;
    ConvRoute r = {0, 1, 0, 0, 0};
    if (K != 1 && K != 2 && K != 3 && K != 5 && K != 7 && K != 11) return ConvRoute{-1, 1, 0, 0, 0};
    auto blocks = [&](int co_blk, int nt_blk) -> int64_t {
        return (int64_t)((p.Nout + nt_blk - 1) / nt_blk) * (p.CoutP / co_blk) * p.n_phase * p.batch;
    };
    auto tile = [&](int co_blk, int nt_blk) { r.co_blk = co_blk, r.nt_blk = nt_blk; };
    // blocks a launch should have: 3 per CU -- unless the whole problem is about one round of the smallest tiles (batch 1: 914 tiles
    // of 64 x 64 for a stage-2 conv): then one block per CU of a LARGE tile (64 x 256: 230 blocks at 0.85 of the matrix peak) beats
    // four of the small one (0.62): batch 1 5.04 -> 4.86 ms per call (200 vs 768 blocks wanted)
    const int64_t want = blocks(64, 64) <= 1024 ? (int64_t)200 : (int64_t)768;
    const bool tiny = p.Nout <= 96;
    // (measured and not kept, round 4: a 96 co x 128 t tile for FastPitch's second conv-FF conv -- 1536 -> 384, exactly two blocks per CU
    // instead of 2.6-2.8 of the 128 x 64 tile -- runs the step in 77.83 vs 77.82 ms)
    if (p.CoutP % 128 == 0) {
        // deep-K layers on short sequences (HiFi-GAN stage 1: C = 256, 8 positions per frame) have few, long blocks;
        // a launch is then 2-4 rounds of blocks and its tail costs 15-19 %: finer tiles pay there
        const bool few_long = p.Cin >= 256 && p.CoutP <= p.Cin && !tiny && blocks(128, 128) < 4 * want;
        if (few_long && K == 3 && blocks(128, 64) >= want) tile(128, 64);
        else if (few_long && K >= 7 && blocks(64, 128) >= want) tile(64, 128);
        else if (K < 11 && !tiny && blocks(128, 128) >= want && (K != 3 || p.Cin % 16 == 0)) tile(128, 128);   // (k = 3: 16-channel chunks)
        else if (K == 11 && !tiny && blocks(64, 256) >= want) tile(64, 256);
        // deep K, a few hundred tiles (FastPitch's second conv-FF conv, 1536 -> 384, at batch 7..13): 128 x 64 tiles with K split
        // (below: < 320 tiles -> 2..4 slices) instead of twice as many 64 x 64 tiles that each walk all 96 chunks; TTSAMD_DEEP_SPLITK
        else if (p.splitk_ws && p.Cin >= 1024 && !tiny && blocks(128, 64) >= 160 && blocks(128, 64) < 320 &&
                 (int64_t)2 * p.batch * p.Cout * p.Nout <= p.splitk_floats && o.deep_splitk != 0) tile(128, 64);
        else if (blocks(128, 64) >= want || (tiny && blocks(64, 64) < 2 * want)) tile(128, 64);
        else tile(64, 64);
    } else if (p.CoutP % 64 == 0) tile(64, !tiny && blocks(64, 256) >= want ? 256 : 64);
    else tile(32, !tiny && blocks(32, 256) >= want ? 256 : 128);
    const int kc = conv_chunk_channels(K, r.nt_blk, r.co_blk);
    if (p.Cin % kc != 0) return ConvRoute{-1, 1, 0, r.co_blk, r.nt_blk};
    // split K: under 320 blocks of at least eight chunks, slices for ~640 blocks of at least four chunks each, within the workspace
    const int64_t nblk = blocks(r.co_blk, r.nt_blk), per = (int64_t)p.batch * p.Cout * p.Nout;
    const int n_chunks = p.Cin / kc;
    constexpr int sk_blocks = 320, sk_target = 640, sk_chunks = 8;
    if (p.splitk_ws && p.n_phase == 1 && p.y_ts == 1 && nblk < sk_blocks && n_chunks >= sk_chunks) {
        int64_t ks = std::min<int64_t>((sk_target + nblk - 1) / nblk, n_chunks / 4);
        ks = std::min<int64_t>(ks, p.splitk_floats / per);
        if (ks >= 2) r.ksplit = (int)ks;
    }
    return r;
}

// The Winograd kernels, F(4,3) before F(2,3); id 0 = none of them takes the launch
static ConvRoute route_wino(const ConvParams& p, const ConvRouteOpts& o) {
    constexpr ConvRoute direct = {0, 1, 0, 0, 0};
    if (o.wino == 0) return direct;
    // what all three Winograd kernels ask: one phase, unit stride of y, 64-row blocks, activation as max(x, slope x), and for the row
    // epilogue and the residual preload rows of y (and of the residual) that are 16-byte aligned and a row block within 2^31 bytes
    // (32-bit buffer offsets)
    const bool rows_vec_ok = conv_rows_aligned(p) && (int64_t)p.Cout * std::max(std::max(p.r_cs, p.y_cs), 1) * 4 < ((int64_t)1 << 31);
    if (p.n_phase != 1 || p.y_ts != 1 || p.CoutP % 64 != 0 || !(p.in_slope >= 0.f && p.in_slope <= 1.f) || !rows_vec_ok) return direct;
    if (p.K == 1) {
        // k = 1 (Vocos' pointwise convs and head, FastPitch's qkv / o_net projections) on the F(4,3) kernel's skeleton with nothing to transform
        // (conv_wino4.hip, Wino4Geo::WSHARE): the direct engine's packed weights as they are; TTSAMD_WINO4 bit 4.  Same tile as the F(4,3) launches.
        if (!((o.wino4 & 16) && p.w != nullptr && p.dil == 1 && p.pad == 0 && p.Cin % 32 == 0 && !p.x_packed && !p.y_packed)) return direct;
        // (k = 1 never splits K here: wino4_ksplit answers > 1 only under 192 blocks and then aims at 224, so blocks1 stays under the 512
        // this route asks for -- the two rules exclude each other, and the factor below is always 1 on a launch that passes)
        const int64_t tiles1 = (int64_t)((p.Nout + 255) / 256) * (p.CoutP / 64) * p.batch;
        const int ks1 = wino4_ksplit(p, tiles1);
        // one full round of the chip's 512 block slots or more: Vocos' GEMMs (512 ... 1536 blocks); FastPitch's qkv / o_net at batch 32 (192 / 384
        // blocks) stay on the direct kernel's smaller tiles -- same-box A/B of the step: 52.43 ms with them here, 52.33 without
        return (tiles1 * ks1 >= 512 && p.Nout >= 256) ? ConvRoute{3, ks1, 0, 0, 0} : direct;
    }
    // k = 3 / 7 / 11 with 'same' padding at dilation 1 / 3 / 5, bias / residual / ReLU epilogues only (the k = 3 chunks are 16 channels)
    if ((p.w_wino == nullptr && p.w_wino4 == nullptr) || (p.K != 3 && p.K != 7 && p.K != 11)) return direct;
    if ((p.dil != 1 && p.dil != 3 && p.dil != 5) || p.pad != p.dil * (p.K - 1) / 2 || p.Cin % 8 != 0 || p.scale != nullptr || p.relu_out >= 2)
        return direct;
    const int kbit = p.K == 3 ? 1 : (p.K == 7 ? 2 : 4);
    auto takes = [&](int mask) { return (mask & kbit) && (p.dil == 1 || (mask & 8)) && (p.K != 3 || p.Cin % 16 == 0); };
    if (p.w_wino4 != nullptr) {
        // F(4,3) decomposition (conv_wino4.hip): 64 rows x 64 quads per block, at least 192 blocks (below: the F(2,3) / direct routing that follows)
        if (takes(o.wino4)) {
            const int bo4 = wino4_tile(p.dil, 64);
            const int64_t tiles4 = (int64_t)((p.Nout + bo4 - 1) / bo4) * (p.CoutP / 64) * p.batch;
            const int ks4 = wino4_ksplit(p, tiles4);
            if (tiles4 * ks4 >= 192 && p.Nout >= 256) {
                // bit 5 / 6: k = 7 / 11 on seven-point groups (when the launch carries them: ConvParams::w_wino44)
                const bool seven = p.w_wino44 != nullptr && p.K != 3 && (o.wino4 & (p.K == 7 ? 32 : 64)) != 0;
                // dilation 1: the window as aligned 16-byte vectors.  One C-in slice: the register epilogue, with the residual's quads fetched
                // under the last step (EPI 3: every c2 conv of a ResBlock, the second conv-FF conv) or without a residual (EPI 4: conv_pre, c1
                // at d = 1, the first conv-FF conv).  C-in slices write raw partial sums through the row epilogue (EPI 0).
                // dilation 3 / 5: the window through the per-wave LDS strip.  Bit 7: a launch with one C-in slice, no residual and mode 0
                // (HiFi-GAN's c1 convs: bias and ReLU only) runs in the packed strip form (EPI 7); C-in slices, a residual and the accumulate
                // modes keep the row epilogue (EPI 0)
                const int epi = p.dil == 1 ? (ks4 != 1 ? 0 : (p.res != nullptr ? 3 : 4))
                                           : (((o.wino4 & 128) && p.res == nullptr && p.mode == 0 && ks4 == 1) ? 7 : 0);
                return ConvRoute{(epi == 7 ? 7 : 3) + (seven ? 1 : 0), ks4, epi, 0, 0};
            }
        }
        if (p.w_wino == nullptr) return direct;
    }
    // F(2,3): 1 = conv1d_wino_f32 (conv_wino.hip: k = 3, dilation 1, 128-row tiles), 2 = conv1d_wino2_f32 (conv_wino2.hip: k = 3 / 7 / 11,
    // dilation 1 / 3 / 5, 128 rows x 64 pairs or, at Cout = 64, 64 rows x 128 pairs)
    const bool rows64 = p.CoutP % 128 != 0;
    const bool w2 = takes(o.wino2) && (!rows64 || (o.wino2 & 16));
    const bool w1 = p.K == 3 && p.dil == 1 && !rows64;
    if (!w2 && !w1) return direct;
    const int bo = wino2_tile(p.dil, rows64 ? 128 : 64);
    const int64_t blocks = (int64_t)((p.Nout + bo - 1) / bo) * (p.CoutP / (rows64 ? 64 : 128)) * p.batch;
    // under ~3/4 of a block per CU the direct kernel's 64 x 64 tiles with split K fill the chip better (batch 1: 3.68 ms per step with
    // the limit at 200, 3.74 at 100, 3.9-4.0 at 50 / 1 and with the Winograd kernels off; batch 4: 10.0 vs 10.5-11.0: tools/ab_small.sh);
    // short sequences (FastPitch's 64-token encoder) would leave half of a 128-output tile empty
    if (blocks < 192 || p.Nout < 256) return direct;
    return ConvRoute{w2 ? 2 : 1, 1, 0, 0, 0};
}

ConvRoute conv_route(const ConvParams& p, const ConvRouteOpts& o) {
    const ConvRoute r = route_wino(p, o);
    return r.id != 0 ? r : route_direct(p, o);
}

// ---- the c1 -> c2 pairs of a ResBlock1, exact fp32: one fused launch, or two launch_conv calls routed above ----
//   TTSAMD_FUSED_PAIR=0      no fused pair at all
//   TTSAMD_FUSED2=0          no second-generation kernel (resblock_fused2.hip) and none of its F(4,3) successor
//   TTSAMD_FUSED2_MASK / _MASK_N1 (hex)  replace kFused2Mask / kFused2MaskN1 (A/B runs and the forced-kernel parity tests); a forced
//                            MASK also lifts the small-problem rule
//   TTSAMD_FUSED2_WB         phases of the second-generation pair on Winograd F(2,3): 2 (default) both, 1 phase B only, 0 both direct
//   TTSAMD_PAIR4             1 (default) the routed C = 32 pairs on resblock_pair4.hip, seven-point groups at the k of kPair44Mask;
//                            2 six-point groups at every k; 0 they stay on resblock_pair2
// Bit 3 * ci + ki of the masks, ci = 0 / 1 / 2 for C = 32 / 64 / 128, ki = 0 / 1 / 2 for k = 3 / 7 / 11.
// default routing of the second-generation fused pair, set from same-box A/B runs of the bench workload
constexpr unsigned kFused2Mask = 0x00F;       // C = 32: k = 3 / 7 / 11; C = 64: k = 3.  Both convs of these pairs run on Winograd F(2,3) inside the launch
                                              // (resblock_pair2<..., WM = 2>).  Round 6: every other pair runs un-fused on the F(4,3) kernel (conv_wino4.hip,
                                              // 64-row blocks): same-box A/B of the bench step (tools/ab_env.sh) 56.72 (07f, k = 7 / 11 only on F(4,3)) / 56.15
                                              // (06f) / 55.00 (05f) / 54.81 ms (04f); then with k = 3 on F(4,3) too: 54.68 (04f) / 55.11 (047: C = 64 k = 3
                                              // un-fused) / 54.59 (007) / 54.10 ms (00f: C = 128 k = 3 un-fused).  Round 5 on F(2,3): C = 64 k = 11 fused 61.93 vs
                                              // 62.45; C = 128 k = 3 fused 63.90 vs 64.06
// Of those, the C = 32 k = 7 / 11 pairs run with both convs on Winograd F(4,3) (resblock_pair4.hip: 16 / 23 products per output quad
// against 20 / 32 on F(2,3)) when the pair takes the 256-column kernel and TTSAMD_FUSED2_WB asks for both phases on Winograd.
// Since round 28 the launch runs on SEVEN-point groups (13 / 20 products per quad, the arithmetic of the un-fused k = 7 / 11 convs) at
// the k of kPair44Mask (bit 0: k = 7, bit 1: k = 11; both: 749 / 712 / 707 -> 665 / 629 / 630 us and 972 / 920 / 894 -> 905 / 869 / 842 us
// per launch at batch 32, step 47.74 -> 47.15 ms, profiles/r28/NOTES.md).
// One-stream kernel table at batch 32 (profiles/r7/NOTES.md): k = 11 3.61 -> 2.75 ms per step, k = 7 2.43 -> 2.12, but k = 3 1.22 -> 1.32
// (memory-bound: 6 products per quad do not pay for the larger window and the extra LDS traffic), so k = 3 stays on resblock_pair2.
// C = 64 k = 3 stays there too (resblock_pair4 is built for C = 32 only: MT = 1, one 32-row tile per wave).
constexpr int kPair4MinK = 7;
constexpr unsigned kPair44Mask = 0x3;
constexpr unsigned kFused2MaskN1 = 0x000;     // 128-column blocks (the direct-arithmetic kernels only): none by default
constexpr int64_t kFused2SmallColumns = 2 * 256 * 252;   // batch x positions under which a stage counts as a small problem

PairRouteOpts pair_route_opts() {
    return {(int)opt_int(OPT_FUSED_PAIR, 1), (int)opt_int(OPT_FUSED2, 1), (int)opt_int(OPT_FUSED2_MASK, -1),
            (int)opt_int(OPT_FUSED2_MASK_N1, kFused2MaskN1), (int)opt_int(OPT_FUSED2_WB, 2), (int)opt_int(OPT_PAIR4, 1)};
}

// k = 3 / 7 / 11 convs carry their F(2,3) groups (Cout = 32: the fused pairs' Winograd phases); the un-fused ResBlock convs (Cout >= 64)
// and the C = 32 pairs that resblock_pair4.hip takes carry the F(4,3) groups too, in both forms where k has a seven-point one: the
// switches are read per launch (Cout >= 64) / per forward (the C = 32 pairs)
ConvForms hifigan_conv_forms(int cin, int cout, int k) {
    const bool wino2 = (k == 3 || k == 7 || k == 11) && cin % 8 == 0 && cout % 32 == 0;
    const bool wino4 = wino2 && (cout >= 64 || (cout == 32 && cin == 32 && k >= kPair4MinK));
    return {wino2, wino4, wino4 && wino44_groups(k) != 0};
}

// resblock_pair2<K, C, NTW, WM> is instantiated with Winograd phases for 256-column blocks only: phase B alone (WM 1) at C = 32 / 64,
// both phases (WM 2) at dilation 1 / 3 / 5 (256 / 252 / 250 intermediate columns per block) -- so C = 128 (8 waves) only with both
bool pair2_phases_built(int32_t channels, int32_t dil, int32_t ntw, int32_t wm) {
    if (wm == 0) return true;
    if (ntw != 2) return false;
    return wm == 1 ? channels <= 64 : (wm == 2 && (dil == 1 || dil == 3 || dil == 5));
}

// the most phases on Winograd that the forms at hand (conv 2's groups: phase B, conv 1's too: phase A) and the instantiations allow
static int pair2_phases(int32_t channels, int32_t dil, int32_t ntw, bool have_b, bool have_a) {
    if (have_b && have_a && pair2_phases_built(channels, dil, ntw, 2)) return 2;
    return (have_b && pair2_phases_built(channels, dil, ntw, 1)) ? 1 : 0;
}

static PairRoute make_pair_route(int32_t kernel, int32_t ntw, int32_t wm, int32_t points) {
    if (kernel == PAIR_GEN1) return {PAIR_GEN1, 0, 0, 0, "fused_pair"};
    if (kernel == PAIR_GEN2) return {PAIR_GEN2, ntw, wm, 0, wm == 2 ? "fused_pair2ww" : (wm == 1 ? "fused_pair2w" : (ntw == 2 ? "fused_pair2" : "fused_pair2n"))};
    if (kernel == PAIR_F43) return {PAIR_F43, 0, 0, points, points == 7 ? "fused_pair44" : "fused_pair4"};
    return {PAIR_NONE, 0, 0, 0, ""};
}

// The block width of the second-generation kernel for this pair: 2 = 256-column blocks, 1 = 128-column blocks, 0 = not this pair.
static int fused2_width(const PairShape& s, const PairRouteOpts& o) {
    if (o.fused2 == 0) return 0;
    const int ci = s.channels == 32 ? 0 : (s.channels == 64 ? 1 : (s.channels == 128 ? 2 : -1));
    const int ki = s.k == 3 ? 0 : (s.k == 7 ? 1 : (s.k == 11 ? 2 : -1));
    if (ci < 0 || ki < 0) return 0;
    const unsigned bit = 1u << (3 * ci + ki);
    // small problems (batch 1 ... 4: under two rounds of 256-column blocks).  Measured: every pair as ONE launch of 128-column blocks of
    // this kernel -- half the launches of the un-fused engine -- is SLOWER there (batch 1: 5.27 vs 5.04 ms per step, batch 4: 13.35 vs
    // 12.88; batch 8 equal): the un-fused engine's 64 x 64 tiles with split K put 3-4x more blocks on the chip.  So this kernel leaves
    // small problems alone (a forced TTSAMD_FUSED2_MASK overrides the rule: parity tests of the fused kernels on small inputs).  What
    // it leaves falls through to the first-generation kernel where that one is built (pair_route below), else to two launches.
    if ((int64_t)s.batch * s.L < kFused2SmallColumns && o.fused2_mask < 0) return 0;
    if (!((o.fused2_mask < 0 ? kFused2Mask : (unsigned)o.fused2_mask) & bit)) return 0;
    // the width the mask asks for; where the kernel's geometry refuses it, the other one
    const int ntw = ((unsigned)o.fused2_mask_n1 & bit) ? 1 : 2;
    const auto fits = [&](int n) { return fused_pair2_supported(s.channels, s.k, s.dil, s.L, s.x, s.y, n); };
    return fits(ntw) ? ntw : (fits(3 - ntw) ? 3 - ntw : 0);
}

PairRoute pair_route(const PairShape& s, const PairRouteOpts& o) {
    if (s.precision != 0 || o.fused_pair == 0 || !s.square) return make_pair_route(PAIR_NONE, 0, 0, 0);
    const int ntw = fused2_width(s, o);
    if (ntw == 0) {
        // What the second-generation kernel does not take -- a small problem, TTSAMD_FUSED2=0, a pair outside the mask -- goes to the
        // first-generation kernel wherever that is built (C = 32 at every k, C = 64 at k = 3): batch 1 runs those pairs on it by default
        return make_pair_route(fused_pair_supported(s.channels, s.k, s.dil, s.L, s.x, s.y) ? PAIR_GEN1 : PAIR_NONE, 0, 0, 0);
    }
    // the 256-column pair with both phases asked on Winograd -> its F(4,3) successor where it is built (C = 32) and packed (k = 7 / 11)
    if (ntw == 2 && o.pair4 != 0 && o.fused2_wb == 2 && s.k >= kPair4MinK && s.forms.wino4 &&
        fused_pair4_supported(s.channels, s.k, s.dil, s.L, s.x, s.y)) {
        const bool seven = o.pair4 == 1 && (kPair44Mask & (s.k == 7 ? 1u : (s.k == 11 ? 2u : 0u))) != 0 && s.forms.wino44;
        return make_pair_route(PAIR_F43, 0, 0, seven ? 7 : 6);
    }
    return make_pair_route(PAIR_GEN2, ntw, pair2_phases(s.channels, s.dil, ntw, o.fused2_wb != 0 && s.forms.wino2, o.fused2_wb == 2 && s.forms.wino2), 0);
}

// ttsamd_resblock_pair's variants: 1 first generation; 2 / 3 second generation with 256- / 128-column blocks; 4 / 5: 256 columns with
// phase B / both phases on Winograd where that is built; 6 / 7: F(4,3) on six- / seven-point groups
PairRoute pair_route_of_variant(int32_t variant, int32_t channels, int32_t dil) {
    if (variant == 2 || variant == 3) return make_pair_route(PAIR_GEN2, variant == 3 ? 1 : 2, 0, 0);
    if (variant == 4 || variant == 5) return make_pair_route(PAIR_GEN2, 2, pair2_phases(channels, dil, 2, true, variant == 5), 0);
    if (variant == 6 || variant == 7) return make_pair_route(PAIR_F43, 0, 0, variant);
    return make_pair_route(variant == 1 ? PAIR_GEN1 : PAIR_NONE, 0, 0, 0);
}

int32_t launch_pair(const PairRoute& r, const PairArgs& a, hipStream_t stream) {
    if (r.kernel == PAIR_GEN1) return launch_fused_pair(a, stream);
    if (r.kernel == PAIR_GEN2) return launch_fused_pair2(a, r, stream);
    if (r.kernel == PAIR_F43) return launch_fused_pair4(a, r, stream);
    set_error("launch_pair: no fused kernel takes this pair (C = %d, k = %d, dilation %d)", a.channels, a.k, a.dil);
    return TTSAMD_EINVAL;
}

}  // namespace ttsamd
