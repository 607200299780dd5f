// Polyphase sinc resampling, wave at orig_freq -> wave at new_freq (include/ttsamd.h states the arithmetic): what
// the reference gets from torchaudio.functional.resample in scripts/preprocess_audio.py:33-47 and utils/data.py:59-67.  With
// g = gcd(orig, new), o = orig / g, n = new / g a row is cut into frames of o input samples; frame f gives the n outputs
//     out[f * n + p] = sum_j taps[p][j] * xz[f * o + j - width],   j in [0, J),   xz = the row, zero outside [0, L)
// The table is built on the host (ttsamd/resample.py, float64, rounded once) and kept here TRANSPOSED, tapsT [JP][NP]: J padded with zero
// rows to a multiple of 16, n padded with zero columns to the phase tiling of the MFMA kernel, so that neither inner loop carries a guard.
// Both kernels sum over j ascending as one fp32 fma chain per output (a zero tap leaves the chain's value as it is): a row's result
// depends on the row alone, not on the batch, the grid or the route.
//
// (a) resample_general_kernel (VALU; any o, n <= 4096, J <= 65536, n = 1 = plain decimation included): a block of 256 threads owns FR
//     consecutive frames x PC consecutive phases of one row, one output per thread.  The input strip of the run sits in LDS, in chunks of
//     JC taps when (FR - 1) * o + J is more than the 32 KB buffer; thread (frame, phase) reads its strip value (a broadcast within a
//     frame) and its tap tapsT[j][p] (consecutive floats across a wave, from L2).
// (b) resample_mfma_kernel<NTW> (v_mfma_f32_16x16x4_f32: exact fp32, D[f][p] += A[f][k] * B[k][p] with A[f][k] = strip[f * o + k],
//     B = tapsT): a block of 512 threads owns 64 frames x NPB = 32 * NTW phases of one row (n > 256: several phase groups on grid.y).
//     Wave w takes frames 16 * (w & 3) .. + 16 and the 16-wide phase tiles NTW * (w >> 2) .. + NTW: one A fetch and NTW B fetches from LDS
//     per NTW MFMAs.  The whole strip, (64 - 1) * o + JP floats, stays in LDS for the block's life; B goes through a double-buffered LDS
//     tile of 16 taps x NPB phases, fetched from L2 into registers while the previous tile is multiplied (one barrier per 16 taps).
//     Bank hazard: the sixteen frames of an A operand are o floats apart, o = 320 = 0 (mod 64) for a 48 kHz source: one bank.  The strip
//     is SKEWED: sample s of the strip sits at s + (s / o) * pad with pad = (4 - o mod 8) mod 8, so that frames are o + pad = 4 (mod 8)
//     floats apart and the 16 frames x 4 taps of one fetch fall into 64 different banks; the B tile's rows are 16 (mod 64) floats apart
//     for the same reason.  (LDS-conflict counters were not collected.)
//     Eligible (route 2; route 0 picks from these): n >= 16, and strip + B tiles within 160 KB of LDS: (63 * o + JP) * (1 + pad / o)
//     + 2 * 16 * (NPB + 16 .. 79) floats.  Everything else runs on (a).
#include <cmath>
#include <cstring>
#include <vector>

#include "kernels.hpp"

namespace ttsamd {

constexpr int RS_MAXON = 4096, RS_MAXJ = 65536;
constexpr int RS_GEN_LDS = 8192, RS_GEN_THREADS = 256;                    // general kernel: strip buffer in floats
constexpr int RS_F = 64, RS_KC = 16, RS_THREADS = 512, RS_MAXNTW = 8;     // MFMA kernel: frames per block, taps per B tile
constexpr int RS_LDS_MAX = 160 * 1024;
constexpr int64_t RS_AUTO_MIN_BLOCKS = 48;                                // route 0: MFMA kernel from this many of its blocks on

struct Resample {
    float* tapsT = nullptr;     // [JP][NP]
    int o = 0, n = 0, width = 0, J = 0, JP = 0, NP = 0;
    int groups = 0, ntw = 0;    // MFMA tiling: NP = groups * 32 * ntw
    int pad = 0, bst = 0;       // strip skew per o samples; B tile row stride (floats)
    int64_t strip_floats = 0;   // skewed strip of a block
    int lds_bytes = 0;
    bool mfma_ok = false;
};

static inline int64_t rs_out_len(const Resample* h, int64_t L) { return L <= 0 ? 0 : ((int64_t)h->n * L + h->o - 1) / h->o; }

int32_t resample_create(const float* taps, int32_t o, int32_t n, int32_t width, Resample** out) {
    TTS_REQUIRE(taps && out, "resample_create: null argument");
    TTS_REQUIRE(o >= 1 && n >= 1 && o <= RS_MAXON && n <= RS_MAXON, "resample_create: o = %d / n = %d outside [1, %d]", o, n, RS_MAXON);
    TTS_REQUIRE(width >= 0 && 2 * (int64_t)width + o <= RS_MAXJ, "resample_create: width %d: J = 2 * width + o is at most %d", width, RS_MAXJ);
    auto* h = new Resample();
    h->o = o; h->n = n; h->width = width; h->J = 2 * width + o;
    h->JP = (int)align_up(h->J, RS_KC);
    h->groups = (n + 32 * RS_MAXNTW - 1) / (32 * RS_MAXNTW);
    h->ntw = (n + 32 * h->groups - 1) / (32 * h->groups);
    h->NP = h->groups * 32 * h->ntw;
    h->pad = (4 - o % 8 + 8) % 8;
    const int npb = 32 * h->ntw;
    h->bst = npb + ((16 - npb % 64) + 64) % 64;
    const int64_t sl = (int64_t)(RS_F - 1) * o + h->JP;
    h->strip_floats = align_up(sl + (sl / o + 1) * h->pad + 4, 4);
    const int64_t lds = (h->strip_floats + 2 * RS_KC * h->bst) * 4;
    h->lds_bytes = (int)(lds <= RS_LDS_MAX ? lds : 0);
    h->mfma_ok = n >= 16 && lds <= RS_LDS_MAX;
    std::vector<float> t((size_t)h->JP * h->NP, 0.f);
    for (int p = 0; p < n; ++p)
        for (int j = 0; j < h->J; ++j) t[(size_t)j * h->NP + p] = taps[(size_t)p * h->J + j];
    hipError_t e = hipMalloc((void**)&h->tapsT, t.size() * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(h->tapsT, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        set_error("resample_create: upload failed: %s", hipGetErrorString(e));
        if (h->tapsT) (void)hipFree(h->tapsT);
        delete h;
        return TTSAMD_EHIP;
    }
    *out = h;
    return 0;
}

void resample_destroy(Resample* h) {
    if (!h) return;
    if (h->tapsT) (void)hipFree(h->tapsT);
    delete h;
}

int64_t resample_out_len(const Resample* h, int64_t nsamples) { return h ? rs_out_len(h, nsamples) : -1; }

int32_t resample_mfma_eligible(const Resample* h) { return h && h->mfma_ok ? 1 : 0; }

ResampleView resample_view(const Resample* h) { return ResampleView{h->tapsT, h->o, h->n, h->width, h->J, h->NP}; }

// ---- (a) general kernel -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RS_GEN_THREADS) void resample_general_kernel(
    const float* __restrict__ wave, int64_t wave_bs, const int64_t* __restrict__ ns, const float* __restrict__ tapsT, int NP, int J, int o,
    int n, int width, int FR, int PC, int PCH, int JC, float* __restrict__ out, int64_t out_bs, int64_t* __restrict__ nout) {
    __shared__ float strip[RS_GEN_LDS];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int64_t run = blockIdx.x / PCH;
    const int pch = blockIdx.x % PCH;
    const int64_t L = max((int64_t)0, min(ns[b], wave_bs));
    const int64_t no = L <= 0 ? 0 : ((int64_t)n * L + o - 1) / o;
    if (blockIdx.x == 0 && tid == 0 && nout) nout[b] = no;
    const int fl = tid / PC, p = pch * PC + tid % PC;
    const bool active = fl < FR && p < n;
    const int64_t f0 = run * FR, m = (f0 + fl) * n + p;
    float* ob = out + (int64_t)b * out_bs;
    if (f0 * n >= no) {                                          // (block-uniform) past the row: zeros
        if (active && m < out_bs) ob[m] = 0.f;
        return;
    }
    const float* wb = wave + (int64_t)b * wave_bs;
    const float* tp = tapsT + (active ? p : 0);
    const int so = fl < FR ? fl * o : 0;
    float acc = 0.f;
    for (int j0 = 0; j0 < J; j0 += JC) {
        const int jn = min(JC, J - j0), span = (FR - 1) * o + jn;
        const int64_t g0 = f0 * o - width + j0;
        __syncthreads();
        for (int s = tid; s < span; s += RS_GEN_THREADS) {
            const int64_t g = g0 + s;
            strip[s] = (g >= 0 && g < L) ? wb[g] : 0.f;
        }
        __syncthreads();
        const float* tj = tp + (int64_t)j0 * NP;
#pragma unroll 8
        for (int jj = 0; jj < jn; ++jj) acc = fmaf(tj[(int64_t)jj * NP], strip[so + jj], acc);
    }
    if (active && m < out_bs) ob[m] = m < no ? acc : 0.f;
}

// ---- (b) MFMA kernel ----------------------------------------------------------------------------------------------------------------------
typedef float rs_f4 __attribute__((ext_vector_type(4)));

template <int NTW>
__global__ __launch_bounds__(RS_THREADS) void resample_mfma_kernel(
    const float* __restrict__ wave, int64_t wave_bs, const int64_t* __restrict__ ns, const float* __restrict__ tapsT, int NP, int JP, int o,
    int n, int width, int pad, int bst, int strip_floats, float* __restrict__ out, int64_t out_bs, int64_t* __restrict__ nout) {
    extern __shared__ float rs_lds[];
    constexpr int NPB = 32 * NTW, NV = RS_KC * NPB / 4, NLD = (NV + RS_THREADS - 1) / RS_THREADS;   // float4 of a B tile, per thread
    float* strip = rs_lds;
    float* bt = rs_lds + strip_floats;                           // [2][RS_KC][bst]
    const int b = blockIdx.z, pg = blockIdx.y, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t f0 = (int64_t)blockIdx.x * RS_F;
    const int64_t L = max((int64_t)0, min(ns[b], wave_bs));
    const int64_t no = L <= 0 ? 0 : ((int64_t)n * L + o - 1) / o;
    if (blockIdx.x == 0 && pg == 0 && tid == 0 && nout) nout[b] = no;
    float* ob = out + (int64_t)b * out_bs;
    const int li = lane & 15, lk = lane >> 4;
    const int fs = 16 * (w & 3), pt0 = NTW * (w >> 2);           // frames fs .. fs + 16 of the block, 16-wide phase tiles pt0 .. pt0 + NTW
    if (f0 * n >= no) {                                          // (block-uniform) past the row: zeros
        for (int t = 0; t < NTW; ++t) {
            const int p = pg * NPB + (pt0 + t) * 16 + li;
            for (int r = 0; r < 4; ++r) {
                const int64_t m = (f0 + fs + 4 * lk + r) * n + p;
                if (p < n && m < out_bs) ob[m] = 0.f;
            }
        }
        return;
    }
    // the strip: sample s (input index f0 * o - width + s) at s + (s / o) * pad
    const float* wb = wave + (int64_t)b * wave_bs;
    const int SL = (RS_F - 1) * o + JP;
    const int64_t g0 = f0 * o - width;
    for (int s = tid; s < SL; s += RS_THREADS) {
        const int64_t g = g0 + s;
        strip[s + (s / o) * pad] = (g >= 0 && g < L) ? wb[g] : 0.f;
    }
    // B tile c: rows 16 c .. 16 c + 16 of tapsT, columns pg * NPB .. + NPB
    const float* tb = tapsT + (int64_t)pg * NPB;
    rs_f4 breg[NLD];
    auto fetch = [&](const int c) {
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int e = tid + RS_THREADS * r;
            if (NV % RS_THREADS == 0 || e < NV) {
                const int row = e / (NPB / 4), col = e % (NPB / 4);
                breg[r] = *reinterpret_cast<const rs_f4*>(tb + (int64_t)(c * RS_KC + row) * NP + 4 * col);
            }
        }
    };
    auto stash = [&](float* dst) {
#pragma unroll
        for (int r = 0; r < NLD; ++r) {
            const int e = tid + RS_THREADS * r;
            if (NV % RS_THREADS == 0 || e < NV) {
                const int row = e / (NPB / 4), col = e % (NPB / 4);
                *reinterpret_cast<rs_f4*>(dst + row * bst + 4 * col) = breg[r];
            }
        }
    };
    rs_f4 acc[NTW];
#pragma unroll
    for (int t = 0; t < NTW; ++t) acc[t] = rs_f4{0.f, 0.f, 0.f, 0.f};
    const int nchunk = JP / RS_KC;
    fetch(0);
    stash(bt);
    __syncthreads();
    // this lane's A element of tap k: strip sample (fs + li) * o + k, k = 16 c + 4 s + lk; (kd, km) = (k / o, k % o) kept incrementally
    const int abase = (fs + li) * (o + pad);
    int kd = lk / o, km = lk % o;
    const int bofs = lk * bst + pt0 * 16 + li;
    for (int c = 0; c < nchunk; ++c) {
        const float* bc = bt + (c & 1) * RS_KC * bst;
        if (c + 1 < nchunk) fetch(c + 1);
#pragma unroll
        for (int s = 0; s < RS_KC / 4; ++s) {
            const float a = strip[abase + kd * (o + pad) + km];
            float bv[NTW];
#pragma unroll
            for (int t = 0; t < NTW; ++t) bv[t] = bc[bofs + 4 * s * bst + 16 * t];
#pragma unroll
            for (int t = 0; t < NTW; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bv[t], acc[t], 0, 0, 0);
            km += 4;
            while (km >= o) { km -= o; ++kd; }
        }
        if (c + 1 < nchunk) stash(bt + ((c + 1) & 1) * RS_KC * bst);   // the other buffer: last read before the barrier that ended chunk c - 1
        __syncthreads();
    }
    // D: column (phase) = lane & 15, row (frame) = 4 * (lane >> 4) + r
#pragma unroll
    for (int t = 0; t < NTW; ++t) {
        const int p = pg * NPB + (pt0 + t) * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = (f0 + fs + 4 * lk + r) * n + p;
            if (p < n && m < out_bs) ob[m] = m < no ? acc[t][r] : 0.f;
        }
    }
}

template <int NTW>
static int32_t launch_mfma(const Resample* h, const float* wave, int64_t wave_bs, const int64_t* ns, int B, float* out, int64_t out_bs,
                           int64_t* nout, int64_t tiles, hipStream_t s) {
    static std::atomic<uint64_t> done{0};
    TTS_CHECK_HIP(lds_opt_in((const void*)resample_mfma_kernel<NTW>, RS_LDS_MAX, done));
    hipLaunchKernelGGL(resample_mfma_kernel<NTW>, dim3((unsigned)tiles, h->groups, B), dim3(RS_THREADS), h->lds_bytes, s, wave, wave_bs, ns,
                       h->tapsT, h->NP, h->JP, h->o, h->n, h->width, h->pad, h->bst, (int)h->strip_floats, out, out_bs, nout);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

int32_t resample_forward(const Resample* h, const float* wave, int64_t wave_stride, const int64_t* nsamples, int32_t B, float* out,
                         int64_t out_stride, int64_t* nout, int32_t route, hipStream_t s) {
    TTS_REQUIRE(h && nsamples && (wave || wave_stride == 0) && (out || out_stride == 0), "resample_forward: null argument");
    TTS_REQUIRE(B >= 1 && B <= 65535, "resample_forward: batch %d outside [1, 65535]", B);
    TTS_REQUIRE(wave_stride >= 0 && out_stride >= 0 && wave_stride < ((int64_t)1 << 40) && out_stride < ((int64_t)1 << 40),
                "resample_forward: bad stride");
    TTS_REQUIRE(route >= 0 && route <= 2, "resample_forward: route %d (0 automatic, 1 general kernel, 2 MFMA kernel)", route);
    if (route == 2)
        TTS_REQUIRE(h->mfma_ok, "resample_forward: route 2 (MFMA kernel) needs n >= 16 and a strip of 63 * o + J floats plus the tap tiles "
                    "within %d KB of LDS; this handle has o = %d, n = %d, J = %d", RS_LDS_MAX / 1024, h->o, h->n, h->J);
    const int64_t frames = out_stride > 0 ? (out_stride + h->n - 1) / h->n : 1;    // out_stride = 0: the counts only
    const int64_t tiles = (frames + RS_F - 1) / RS_F;
    // automatic: the MFMA kernel where it is eligible and the launch has at least 48 of its blocks (profiles/r12/NOTES.md: measured at
    // 48 kHz -> 22 050 Hz, 24 blocks per 10 s row: from two rows on it wins by 1.5x to 8.6x; one row is a draw, +8 % at J = 602 and
    // -6 % at J = 4824 for the general kernel's 1 500 finer blocks)
    const bool mfma = route == 2 || (route == 0 && h->mfma_ok && tiles * h->groups * B >= RS_AUTO_MIN_BLOCKS);
    if (mfma) {
        TTS_REQUIRE(tiles <= 0x7fffffff, "resample_forward: out_stride too large");
        switch (h->ntw) {
#define RS_CASE(N) case N: return launch_mfma<N>(h, wave, wave_stride, nsamples, B, out, out_stride, nout, tiles, s);
            RS_CASE(1) RS_CASE(2) RS_CASE(3) RS_CASE(4) RS_CASE(5) RS_CASE(6) RS_CASE(7) RS_CASE(8)
#undef RS_CASE
        }
        set_error("resample_forward: internal: ntw %d", h->ntw);
        return TTSAMD_EINVAL;
    }
    const int PC = h->n < RS_GEN_THREADS ? h->n : RS_GEN_THREADS, PCH = (h->n + PC - 1) / PC;
    int FR = RS_GEN_THREADS / PC;
    const int frmax = 1 + (RS_GEN_LDS - 256) / h->o;
    FR = FR > frmax ? frmax : FR;
    const int JC = RS_GEN_LDS - (FR - 1) * h->o;
    const int64_t runs = (frames + FR - 1) / FR;
    TTS_REQUIRE(runs * PCH <= 0x7fffffff, "resample_forward: out_stride too large");
    hipLaunchKernelGGL(resample_general_kernel, dim3((unsigned)(runs * PCH), B), dim3(RS_GEN_THREADS), 0, s, wave, wave_stride, nsamples,
                       h->tapsT, h->NP, h->J, h->o, h->n, h->width, FR, PC, PCH, JC, out, out_stride, nout);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd
