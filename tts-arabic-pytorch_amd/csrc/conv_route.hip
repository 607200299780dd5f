// Routing of an exact-fp32 conv launch (launch_conv, conv_mfma.hip): which kernel, in which form, in how many C-in slices.  Host only, no
// kernel here: conv_route decides from the launch and ONE snapshot of the switches and launches nothing; the launchers (conv_mfma.hip,
// conv_wino.hip, conv_wino2.hip, conv_wino4.hip) execute what it returned, and ttsamd_conv1d_route (api.hip) asks without launching.
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

}  // namespace ttsamd
