// The row epilogue of the fp32 / bf16 conv kernels (conv_mfma.hip, conv_mfma_bf16.hip, conv_wino.hip, conv_wino2.hip, conv_wino4.hip):
// device code only.
#pragma once
#include <type_traits>

#include "conv_mfma_common.hpp"

namespace ttsamd {

// where the per-row factor between conv and residual comes from
constexpr int kRowScaleNone = 0;     // the kernel has none: no multiply is compiled in
constexpr int kRowScaleLds = 1;      // scale_v = a vector in LDS beside the bias, index = row of the slab
constexpr int kRowScaleGlobal = 2;   // scale_v = p.scale (may be null), index = output channel

// A slab of ROWS rows x NT_BLK columns of the output tile sits in the dead LDS ring at `ep`, its bias vector at `epb` (one value per
// row of the slab), and the block is behind the barrier that made both visible.  Each wave walks rows of the slab -- RPI rows per wave
// instruction, CPL float4 column groups per lane -- and for every float4 of a row adds the bias, applies the per-row scale, the
// residual, ReLU / GELU / tanh and the accumulate modes 0 / 1 / 2 (y = v, y += v, y = (y + v) / div), and stores the quad; a quad the
// utterance end cuts is stored element by element.  co0 is the output channel of the slab's first row, `rows` (<= ROWS) how many of its
// rows belong to the tile, q0 the tile's first output position.  Everything that differs between the kernels is a compile-time parameter:
//   SCALE    kRowScale*
//   ACT      GELU (relu_out 2) and tanh (relu_out 3) are compiled in
//   PRELOAD  the residual (and, in the accumulate modes, the previous y) came in through the accumulators: nothing is read here
//   CLIP     columns >= nt_eff of the tile are not this block's (dilated Winograd tiles)
// No LDS of its own, no barrier.
// p arrives by value in the PRELOAD instantiations and by reference in the others.  Both compile to the same loops; the choice is there
// for the register allocator alone: by reference conv1d_mfma_bf16<5,2,2,1,4,2,3> needs 169 VGPRs instead of 167 (three waves per SIMD
// end at 168), by value conv1d_mfma_bf16<1,2,2,1,4,2,0> spills two registers it did not spill (profiles/r30/NOTES.md).
template <int NT_BLK, int ROWS, int SCALE, bool ACT, bool PRELOAD, bool CLIP>
__device__ __forceinline__ void conv_row_epilogue(std::conditional_t<PRELOAD, const ConvParams, const ConvParams&> p, const float* ep,
                                                  const float* epb, const float* scale_v, const int b, const int co0, const int rows,
                                                  const int q0, const int n_out, const int nt_eff) {
    constexpr int LPR = NT_BLK / 4;                                     // lanes per row (one float4 each)
    static_assert(64 % LPR == 0 || LPR % 64 == 0, "epilogue rows");
    constexpr int RPI = LPR >= 64 ? 1 : 64 / LPR;                       // rows per wave instruction
    constexpr int CPL = LPR >= 64 ? LPR / 64 : 1;                       // float4 column groups per lane
    constexpr int NR = (ROWS + 4 * RPI - 1) / (4 * RPI);                // row iterations per wave
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float* __restrict__ yb = p.y + (int64_t)b * p.y_bs;
    const float* __restrict__ rb = (p.res && !PRELOAD) ? p.res + (int64_t)b * p.r_bs : nullptr;
    // every field is read here, none inside the loops: with p.y_cs read through the reference inside them the compiler turns every
    // 16-byte store of both loops into a 12-byte and a 4-byte one (profiles/r30/NOTES.md)
    const int mode = p.mode, relu_out = p.relu_out, Cout = p.Cout, y_cs = p.y_cs, r_cs = p.r_cs;
    const float div = p.div;
    if (PRELOAD || (!rb && mode == 0 && (!ACT || relu_out < 2) && (SCALE != kRowScaleGlobal || scale_v == nullptr))) {
        // nothing to read from memory (no residual, or it came in through the accumulators): a loop without
        // a single vmcnt wait -- on this ISA a vmcnt wait also drains the wave's previous STORE, which made
        // every row iteration of the generic loop below one full memory round trip (~1.7 us)
        const float lo = relu_out == 1 ? 0.f : -__builtin_inff();
        const bool do_div = PRELOAD && mode == 2;                       // without the preload this loop runs in mode 0 only
#pragma unroll 4
        for (int it = 0; it < NR; ++it) {
            const int rl = wid * RPI + it * 4 * RPI + (LPR >= 64 ? 0 : lane / LPR);
            const int co = co0 + rl;
            if (rl >= rows || co >= Cout) continue;
            const float bsv = epb[rl];
            float scv = 1.f;
            if constexpr (SCALE == kRowScaleLds) scv = scale_v[rl];
#pragma unroll
            for (int cg = 0; cg < CPL; ++cg) {
                const int col = ((LPR >= 64 ? lane : lane % LPR) + 64 * cg) * 4;
                const int q = q0 + col;
                if (q >= n_out || (CLIP && col >= nt_eff)) continue;
                const float4 a4 = *reinterpret_cast<const float4*>(ep + rl * NT_BLK + col);
                float v[4] = {a4.x, a4.y, a4.z, a4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = v[e] + bsv;
                    if constexpr (SCALE == kRowScaleLds) x = x * scv;
                    x = fmaxf(x, lo);
                    if (do_div) x = x / div;
                    v[e] = x;
                }
                float* yp = yb + (int64_t)co * y_cs + q;
                if (q + 3 < n_out) {
                    *reinterpret_cast<float4*>(yp) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (q + e < n_out) yp[e] = v[e];
                }
            }
        }
        return;
    }
    if constexpr (!PRELOAD) {
#pragma unroll 2
        for (int it = 0; it < NR; ++it) {
            const int rl = wid * RPI + it * 4 * RPI + (LPR >= 64 ? 0 : lane / LPR);
            const int co = co0 + rl;
            if (rl >= rows || co >= Cout) continue;
            const float bsv = epb[rl];
            float scv = 1.f;
            if constexpr (SCALE == kRowScaleLds) scv = scale_v[rl];
#pragma unroll
            for (int cg = 0; cg < CPL; ++cg) {
                const int col = ((LPR >= 64 ? lane : lane % LPR) + 64 * cg) * 4;
                const int q = q0 + col;
                if (q >= n_out || (CLIP && col >= nt_eff)) continue;
                const float4 a4 = *reinterpret_cast<const float4*>(ep + rl * NT_BLK + col);
                float v[4] = {a4.x, a4.y, a4.z, a4.w};
                float* yp = yb + (int64_t)co * y_cs + q;
                const float* rp = rb ? rb + (int64_t)co * r_cs + q : nullptr;
                const bool full = q + 3 < n_out;
                float rr4[4] = {0.f, 0.f, 0.f, 0.f}, pp4[4] = {0.f, 0.f, 0.f, 0.f};
                if (full) {
                    if (rp) { const float4 t = *reinterpret_cast<const float4*>(rp); rr4[0] = t.x; rr4[1] = t.y; rr4[2] = t.z; rr4[3] = t.w; }
                    if (mode != 0) { const float4 t = *reinterpret_cast<const float4*>(yp); pp4[0] = t.x; pp4[1] = t.y; pp4[2] = t.z; pp4[3] = t.w; }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (q + e < n_out) {
                            if (rp) rr4[e] = rp[e];
                            if (mode != 0) pp4[e] = yp[e];
                        }
                }
                if constexpr (SCALE == kRowScaleGlobal) scv = scale_v ? scale_v[co] : 1.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float x = v[e] + bsv;
                    if constexpr (ACT) { if (relu_out == 2) x = 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f)); }   // nn.GELU()
                    if constexpr (SCALE != kRowScaleNone) x = x * scv;
                    x = x + rr4[e];
                    if (relu_out == 1) x = fmaxf(x, 0.f);
                    if constexpr (ACT) { if (relu_out == 3) x = tanhf(x); }
                    if (mode == 1) x = pp4[e] + x;
                    else if (mode == 2) x = (pp4[e] + x) / div;
                    v[e] = x;
                }
                if (full) {
                    *reinterpret_cast<float4*>(yp) = make_float4(v[0], v[1], v[2], v[3]);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (q + e < n_out) yp[e] = v[e];
                }
            }
        }
    }
}

}  // namespace ttsamd
