// Griffin-Lim, magnitude -> wave, on the transform of melspec.hip (n_fft = win = 1024, hop 256, periodic hann; fft1024.hpp), and the mel
// inversion in front of it.  It is torchaudio.functional.griffinlim restated for a linear magnitude `mag` [513][T]:
//     c = momentum / (1 + momentum);  angles = init;  tprev = 0
//     n_iter times:  inv = istft(mag * angles);  rebuilt = stft(inv);  a = rebuilt - c * tprev;  angles = a / (|a| + 1e-16);  tprev = rebuilt
//     wave = istft(mag * angles)
// with the two framings of melspec.hip (reflect padding at the row's own ends):
//     center (pad 512 per side):  n = 256 (T - 1) samples, T >= 4        same (pad 384 per side):  n = 256 T samples, T >= 2
// istft = inverse real transform (the imaginary parts of bins 0 and 512 are dropped, as every c2r transform does), times the window,
// overlap-add over the padded length 256 (T - 1) + 1024, divided by the sum of the squared windows of the frames that exist at that
// sample (1.5 where four frames overlap, summed from the window table within 768 samples of either end), cropped by the padding.
//
// What crosses HBM between two iterations is the FRAME matrix, not a spectrum and not a wave: the windowed inverse frames [B][T][1024]
// of mag * angles, in a ping-pong pair.  Launches, whatever the batch and the lengths: n_iter + 3.
//   1.          gl_tables_kernel: the window and the 1024 twiddles into the workspace (double on the device, rounded once).
//   2.          gl_iter_kernel<true>: angles = init (zero phase, the hash, or the caller's `phase`), spectrum -> inverse frames.
//   3 .. n + 2. gl_iter_kernel<false>: a block of 256 threads owns ONE pair of consecutive frames of one row (t even in .x, t + 1 in .y
//               of one complex transform, as in melspec.hip: the pairing is the same in a batch and alone); it
//               a. builds the two time-domain frames from the previous frame matrix: sample s of the wave, read at the reflected index, is
//                  the sum of the up to four frames' entries (ascending) over the envelope; times the window;
//               b. forward transform in LDS, the two spectra unpacked by bin k and 1024 - k;
//               c. thread i takes bins i, i + 256 (thread 0: 512 too) of both frames: a = rebuilt - c * tprev, angles = a / (|a| + 1e-16),
//                  tprev = rebuilt ([B][T][513] complex in the workspace, only when momentum != 0); the last iteration also writes the
//                  angles to `phase` and adds (|rebuilt| - mag)^2 and mag^2 in float64;
//               d. mag * angles packed as conj(S_t + i S_t+1), transformed again (the inverse), windowed, stored frame-major.
//   n + 3.      gl_ola_kernel: the last frame matrix overlap-added into `wave`, zeros from the row's length to the stride; block 0 of a
//               row adds the row's per-block float64 partial sums (thread i those of the blocks i, i + 256, ... in ascending order, then
//               the same fixed tree as inside a block) -> inconsistency.
// fp32 throughout except those two sums.  No atomics: every reduction has a fixed order that depends on the row alone, so row b of a ragged
// batch has the bits of the call on row b alone and two runs agree.  Nothing at or past a row's frame count is read (mag, phase) --
// a NaN there stays where it is.  A row whose count is below the framing's minimum (device data: it cannot be refused) is an empty row.
// LDS: 16 KB transform buffers + 8 KB twiddles + 4 KB window = 28 KB; 62 VGPRs; five blocks per CU.  One pair per block, not melspec.hip's
// eight: the kernel is bound by the latency of its 13 barriers per pair, not by the 12 KB of tables a block loads first, and more blocks
// hide more of it -- 16 / 8 / 4 / 2 frames per block measured 1.71 / 0.91 / 0.53 / 0.37 ms for 32 iterations of one row of 450 frames and
// 4.38 / 4.32 / 4.04 / 3.33 ms for 32 rows (profiles/r39/NOTES.md).
#include <cmath>
#include <cstring>

#include "kernels.hpp"
#include "stft1024.hpp"

namespace ttsamd {

constexpr int GL_FPB = 2, GL_MAXMEL = 128;                // GL_FPB: frames per block, one pair
constexpr int GL_OLA = 1024;                              // samples per block of the overlap-add launch

struct GlPlan {
    int64_t frames_a, frames_b, tprev, part, window, twiddle, bytes;   // byte offsets into the workspace
    int32_t chunks;
};

static bool gl_plan(int32_t B, int32_t T, bool momentum, GlPlan& p) {
    if (B < 1 || B > 65535 || T < 1 || T > (1 << 22)) return false;
    Arena a(nullptr, 0);
    p.chunks = (T + GL_FPB - 1) / GL_FPB;
    p.window = a.off;  a.take<float>(STFT_N);
    p.twiddle = a.off; a.take<float2>(STFT_N);
    p.part = a.off;    a.take<double>((int64_t)B * p.chunks * 2);
    p.frames_a = a.off; a.take<float>((int64_t)B * T * STFT_N);
    p.frames_b = a.off; a.take<float>((int64_t)B * T * STFT_N);
    p.tprev = a.off;
    if (momentum) a.take<float2>((int64_t)B * T * STFT_NBIN);
    p.bytes = a.off;
    return true;
}

__global__ void gl_tables_kernel(float* __restrict__ win, float2* __restrict__ tw) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= STFT_N) return;
    const double x = (double)m / (STFT_N / 2);               // exp(-2 pi i m / 1024) = (cos, -sin)(pi x)
    win[m] = (float)(0.5 - 0.5 * cospi(x));
    tw[m] = make_float2((float)cospi(x), (float)(-sinpi(x)));
}

__device__ __forceinline__ uint32_t gl_fmix32(uint32_t h) {   // murmur3's finaliser
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}

// the hashed uniform phase of frame t, bin k under a row's 64-bit seed: (cos, sin) of 2 pi (h >> 8) 2^-24
__device__ __forceinline__ float2 gl_hash_phase(const uint32_t seed_lo, const uint32_t seed_hi, const int t, const int k) {
    const uint32_t h = gl_fmix32(gl_fmix32(seed_lo + 0x9E3779B9u * ((uint32_t)t * (uint32_t)STFT_NBIN + (uint32_t)k)) ^ seed_hi);
    float s, c;
    sincospif((float)(h >> 8) * (2.0f / 16777216.0f), &s, &c);   // the argument is exact in fp32
    return make_float2(c, s);
}

// frames of a row that the launches work on: the count clamped to the matrix, 0 below the framing's minimum
__device__ __forceinline__ int gl_row_frames(const int32_t* __restrict__ frames, const int b, const int T_max, const int center) {
    const int fr = min(max(frames[b], 0), T_max);
    return fr < (center ? 4 : 2) ? 0 : fr;
}

// the signal of the padded axis at position p (0 <= p < 256 (fr - 1) + 1024): the frames that exist at p, added in ascending order,
// over the sum of their squared windows.  fb: the row's windowed inverse frames [fr][1024]; win: the window in LDS.
__device__ __forceinline__ float gl_sample(const float* __restrict__ fb, const float* win, const int p, const int fr) {
    const int f_lo = p >= STFT_N ? (p - (STFT_N - STFT_HOP)) >> 8 : 0, f_hi = min(p >> 8, fr - 1);
    float v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int f = f_lo + q;
        v[q] = f <= f_hi ? fb[(int64_t)f * STFT_N + (p - STFT_HOP * f)] : 0.f;
    }
    float env = 1.5f;
    if (p < STFT_N - STFT_HOP || p >= STFT_HOP * fr) {           // within 768 samples of an end: fewer than four frames
        env = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = f_lo + q;
            const float w = win[min(max(p - STFT_HOP * f, 0), STFT_N - 1)];
            env += f <= f_hi ? w * w : 0.f;
        }
    }
    return (((v[0] + v[1]) + v[2]) + v[3]) / env;
}

struct GlArgs {
    const float* mag;            // [B][513][T_max]
    const int32_t* frames;       // [B]
    const float2* phase_in;      // FIRST, init 2: [B][T_max][513]
    float2* phase_out;           // where this launch leaves its angles, or nullptr
    const unsigned long long* seed_rows;   // FIRST, init 1: [B] or nullptr (seed for every row)
    unsigned long long seed;
    const float* prev;           // [B][T_max][1024]
    float* next;
    float2* tprev;               // [B][T_max][513] or nullptr (momentum 0)
    double* part;                // [B][chunks][2] or nullptr (not the last iteration)
    const float* win;
    const float2* tw;
    float coef;                  // momentum / (1 + momentum)
    int32_t T_max, center, init, tprev_valid, chunks;
};

template <bool FIRST>
__global__ __launch_bounds__(256, 4) void gl_iter_kernel(const GlArgs a) {
    __shared__ float2 buf[2][STFT_N];
    __shared__ float2 tw[STFT_N];
    __shared__ float wl[STFT_N];
    __shared__ double red[2][4];
    const int b = blockIdx.y, t0 = blockIdx.x * GL_FPB, i = threadIdx.x;
    const int T_max = a.T_max;
    const int fr = gl_row_frames(a.frames, b, T_max, a.center);
    if (t0 >= fr) return;                                        // (block-uniform)
    const int pad = stft1024_pad(a.center);
    const int n = a.center ? STFT_HOP * (fr - 1) : STFT_HOP * fr;
    stft1024_load_twiddles(tw, a.tw, i);
    float w[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        w[r] = a.win[i + 256 * r];
        wl[i + 256 * r] = w[r];
    }
    __syncthreads();
    const float* mg = a.mag + (int64_t)b * STFT_NBIN * T_max;
    const int64_t row = (int64_t)b * T_max;
    const float* fprev = a.prev + row * STFT_N;
    uint32_t seed_lo = 0, seed_hi = 0;
    if (FIRST && a.init == 1) {
        const unsigned long long sd = a.seed_rows ? a.seed_rows[b] : a.seed;
        seed_lo = (uint32_t)sd;
        seed_hi = (uint32_t)(sd >> 32);
    }
    const bool with_tprev = !FIRST && a.tprev != nullptr;
    double e[2] = {0.0, 0.0};                                    // (|rebuilt| - mag)^2, mag^2
    const int t = t0;                                            // the block's pair: frames t (even) and t + 1
    const bool two = t + 1 < fr;
    // bins of this thread: i, i + 256 and, for thread 0, 512
    const int nk = i == 0 ? 3 : 2;
    float ma[3], mb[3];
    float2 pa[3], pb[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        ma[r] = mb[r] = 0.f;
        pa[r] = pb[r] = make_float2(0.f, 0.f);
        if (r < nk) {
            const int k = i + 256 * r;
            ma[r] = mg[(int64_t)k * T_max + t];
            if (two) mb[r] = mg[(int64_t)k * T_max + t + 1];
            if (with_tprev && a.tprev_valid) {
                pa[r] = a.tprev[(row + t) * STFT_NBIN + k];
                if (two) pb[r] = a.tprev[(row + t + 1) * STFT_NBIN + k];
            }
        }
    }
    if (!FIRST) {
        // a. the two frames of the previous iterate's signal, windowed
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = i + 256 * r;
            const int sp = t * STFT_HOP + j - pad;
            const int s0 = stft1024_reflect(sp, n), s1 = stft1024_reflect(sp + STFT_HOP, n);
            const float xa = gl_sample(fprev, wl, s0 + pad, fr);
            const float xb = two ? gl_sample(fprev, wl, s1 + pad, fr) : 0.f;
            buf[0][j] = make_float2(xa * w[r], xb * w[r]);
        }
        __syncthreads();
        fft1024_stockham(buf[0], buf[1], tw, i);             // b. Z in buf[1]
    }
    // c. / d. per bin: the new angles, and conj(S_t + i S_t+1) into buf[0]
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        if (r < nk) {
            const int k = i + 256 * r;
            float2 ga, gb;                                   // angles of frame t, t + 1
            if (FIRST) {
                if (a.init == 1) {
                    ga = gl_hash_phase(seed_lo, seed_hi, t, k);
                    gb = gl_hash_phase(seed_lo, seed_hi, t + 1, k);
                } else if (a.init == 2) {
                    ga = a.phase_in[(row + t) * STFT_NBIN + k];
                    gb = two ? a.phase_in[(row + t + 1) * STFT_NBIN + k] : make_float2(0.f, 0.f);
                } else {
                    ga = gb = make_float2(1.f, 0.f);
                }
            } else {
                const float2 z = buf[1][k], cz = buf[1][(STFT_N - k) & (STFT_N - 1)];
                float2 ra, rb;                               // rebuilt, frames t and t + 1
                stft1024_unpack_pair(z, cz, ra, rb);
                // center framing, frame 0: reflected about sample 0 and windowed symmetrically, the frame is even about its middle,
                // so its spectrum is real (times (-1)^k); what the transform leaves in the imaginary part is rounding noise only, and
                // in a bin whose rebuilt magnitude is far below `mag` that noise would turn the angle (measured: 1e-5 of the frame's
                // largest magnitude against 1e-6 in the other frames, profiles/r39/NOTES.md)
                if (a.center && t == 0) ra.y = 0.f;
                float2 aa = ra, ab = rb;
                if (with_tprev) {
                    aa = make_float2(ra.x - a.coef * pa[r].x, ra.y - a.coef * pa[r].y);
                    ab = make_float2(rb.x - a.coef * pb[r].x, rb.y - a.coef * pb[r].y);
                    a.tprev[(row + t) * STFT_NBIN + k] = ra;
                    if (two) a.tprev[(row + t + 1) * STFT_NBIN + k] = rb;
                }
                const float da = sqrtf(aa.x * aa.x + aa.y * aa.y) + 1e-16f, db = sqrtf(ab.x * ab.x + ab.y * ab.y) + 1e-16f;
                ga = make_float2(aa.x / da, aa.y / da);
                gb = make_float2(ab.x / db, ab.y / db);
                if (a.part) {
                    const float ea = sqrtf(ra.x * ra.x + ra.y * ra.y) - ma[r];
                    e[0] += (double)ea * (double)ea;
                    e[1] += (double)ma[r] * (double)ma[r];
                    if (two) {
                        const float eb = sqrtf(rb.x * rb.x + rb.y * rb.y) - mb[r];
                        e[0] += (double)eb * (double)eb;
                        e[1] += (double)mb[r] * (double)mb[r];
                    }
                }
            }
            if (a.phase_out) {
                a.phase_out[(row + t) * STFT_NBIN + k] = ga;
                if (two) a.phase_out[(row + t + 1) * STFT_NBIN + k] = gb;
            }
            // (products rounded on their own, never contracted into the sums below: both instantiations of this kernel then give a
            // spectrum the same bits, which is what makes a run resumed through `phase` equal the uninterrupted one)
            float2 sa = make_float2(__fmul_rn(ma[r], ga.x), __fmul_rn(ma[r], ga.y));
            float2 sb = two ? make_float2(__fmul_rn(mb[r], gb.x), __fmul_rn(mb[r], gb.y)) : make_float2(0.f, 0.f);
            if (k == 0 || k == STFT_N / 2) sa.y = sb.y = 0.f;  // a real signal's bins 0 and 512 are real: c2r drops what is there
            buf[0][k] = make_float2(sa.x - sb.y, -(sa.y + sb.x));
            if (k != 0 && k != STFT_N / 2) buf[0][STFT_N - k] = make_float2(sa.x + sb.y, sa.y - sb.x);
        }
    }
    __syncthreads();
    fft1024_stockham(buf[0], buf[1], tw, i);                 // (1024 s_t, -1024 s_t+1) in buf[1]
    float* fa = a.next + (row + t) * STFT_N;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = i + 256 * r;
        const float2 y = buf[1][j];
        fa[j] = stft1024_inverse_sample(y.x, w[r]);
        if (two) fa[STFT_N + j] = stft1024_inverse_sample(-y.y, w[r]);
    }
    if (!FIRST && a.part) {
        block_sum_fixed<4, 2>(e, red);                       // the block's two sums, in a fixed order
        if (i < 2) a.part[((int64_t)b * a.chunks + blockIdx.x) * 2 + i] = i == 0 ? e[0] : e[1];
    }
}

__global__ __launch_bounds__(256) void gl_ola_kernel(const float* __restrict__ fin, const int32_t* __restrict__ frames, int T_max, int center,
                                                     const float* __restrict__ win, float* __restrict__ wave, int64_t wave_stride,
                                                     const double* __restrict__ part, int chunks, int have_part,
                                                     double* __restrict__ inconsistency) {
    __shared__ float wl[STFT_N];
    const int b = blockIdx.y, i = threadIdx.x;
    const int fr = gl_row_frames(frames, b, T_max, center);
    const int pad = stft1024_pad(center);
    const int64_t n = fr == 0 ? 0 : (center ? (int64_t)STFT_HOP * (fr - 1) : (int64_t)STFT_HOP * fr);
#pragma unroll
    for (int r = 0; r < 4; ++r) wl[i + 256 * r] = win[i + 256 * r];
    __syncthreads();
    const float* fb = fin + (int64_t)b * T_max * STFT_N;
    float* wb = wave + (int64_t)b * wave_stride;
#pragma unroll
    for (int r = 0; r < GL_OLA / 256; ++r) {
        const int64_t s = (int64_t)blockIdx.x * GL_OLA + i + 256 * r;
        if (s < wave_stride) wb[s] = s < n ? gl_sample(fb, wl, (int)s + pad, fr) : 0.f;
    }
    if (inconsistency && blockIdx.x == 0) {                          // (block-uniform)
        __shared__ double red[2][4];
        double e[2] = {0.0, 0.0};                                    // numerator, denominator
        const int C = (have_part && fr > 0) ? (fr + GL_FPB - 1) / GL_FPB : 0;
        for (int c = i; c < C; c += 256) {
            e[0] += part[((int64_t)b * chunks + c) * 2];
            e[1] += part[((int64_t)b * chunks + c) * 2 + 1];
        }
        block_sum_fixed<4, 2>(e, red);
        if (i == 0) inconsistency[b] = C > 0 ? sqrt(e[0]) / sqrt(e[1]) : (double)NAN;   // NaN: no iteration, or an empty row: nothing was rebuilt
    }
}

static int32_t griffinlim(const float* mag, const int32_t* frames, int32_t B, int32_t T, int32_t framing, int32_t n_iter, float momentum,
                          int32_t init, const uint64_t* seed_rows, uint64_t seed, float2* phase, float* wave, int64_t wave_stride,
                          double* inconsistency, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    TTS_REQUIRE(mag && frames && wave && workspace, "griffinlim: null argument");
    TTS_REQUIRE(framing == 0 || framing == 1, "griffinlim: framing %d (0 = same, 1 = center)", framing);
    const int t_min = framing ? 4 : 2;
    TTS_REQUIRE(T >= t_min, "griffinlim: t_max = %d frames, the %s framing needs at least %d (reflect padding of %d samples per side)", T,
                framing ? "center" : "same", t_min, framing ? 512 : 384);
    TTS_REQUIRE(n_iter >= 0 && n_iter <= (1 << 20), "griffinlim: n_iter = %d outside [0, 2^20]", n_iter);
    TTS_REQUIRE(momentum >= 0.f && momentum < 1.f, "griffinlim: momentum = %g outside [0, 1)", (double)momentum);
    TTS_REQUIRE(init >= 0 && init <= 2 && (init != 2 || phase), "griffinlim: init = %d (0 zero phase, 1 hash, 2 the caller's phase, which needs `phase`)", init);
    GlPlan p;
    TTS_REQUIRE(gl_plan(B, T, momentum != 0.f, p), "griffinlim: bad batch %d / t_max %d (1 .. 65535 rows, 1 .. 2^22 frames)", B, T);
    const int64_t n_max = framing ? (int64_t)STFT_HOP * (T - 1) : (int64_t)STFT_HOP * T;
    TTS_REQUIRE(wave_stride >= n_max && wave_stride < ((int64_t)1 << 31) - STFT_N, "griffinlim: wave_stride = %lld, %d frames give %lld samples",
                (long long)wave_stride, T, (long long)n_max);
    TTS_REQUIRE(workspace_bytes >= p.bytes, "griffinlim: workspace of %lld bytes, %lld needed", (long long)workspace_bytes, (long long)p.bytes);
    char* ws = (char*)workspace;
    float* win = (float*)(ws + p.window);
    float2* tw = (float2*)(ws + p.twiddle);
    float* fr_ab[2] = {(float*)(ws + p.frames_a), (float*)(ws + p.frames_b)};
    hipLaunchKernelGGL(gl_tables_kernel, dim3(STFT_N / 256), dim3(256), 0, s, win, tw);
    TTS_CHECK_HIP(hipGetLastError());
    GlArgs a;
    memset(&a, 0, sizeof(a));
    a.mag = mag; a.frames = frames; a.phase_in = phase; a.seed_rows = (const unsigned long long*)seed_rows; a.seed = seed;
    a.win = win; a.tw = tw; a.coef = momentum / (1.f + momentum); a.T_max = T; a.center = framing; a.init = init; a.chunks = p.chunks;
    a.tprev = momentum != 0.f ? (float2*)(ws + p.tprev) : nullptr;
    const dim3 grid(p.chunks, B);
    a.next = fr_ab[0];
    a.phase_out = (n_iter == 0 && init != 2) ? phase : nullptr;   // no iteration: the angles are the initial ones
    hipLaunchKernelGGL(gl_iter_kernel<true>, grid, dim3(256), 0, s, a);
    TTS_CHECK_HIP(hipGetLastError());
    int cur = 0;
    for (int it = 0; it < n_iter; ++it) {
        const bool last = it + 1 == n_iter;
        a.prev = fr_ab[cur];
        a.next = fr_ab[cur ^ 1];
        a.tprev_valid = it > 0;
        a.phase_out = last ? phase : nullptr;
        a.part = (last && inconsistency) ? (double*)(ws + p.part) : nullptr;
        hipLaunchKernelGGL(gl_iter_kernel<false>, grid, dim3(256), 0, s, a);
        TTS_CHECK_HIP(hipGetLastError());
        cur ^= 1;
    }
    const dim3 ogrid((unsigned)((wave_stride + GL_OLA - 1) / GL_OLA), B);
    hipLaunchKernelGGL(gl_ola_kernel, ogrid, dim3(256), 0, s, fr_ab[cur], frames, T, framing, win, wave, wave_stride,
                       (const double*)(ws + p.part), p.chunks, (int)(n_iter > 0), inconsistency);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

// mag[b][f][t] = max(sum_m pinv[f][m] * e(mel[b][m][t]), floor), e = exp for a log-mel: a block takes 64 frames x 64 bins of a row, the
// e tile [n_mels][64] in LDS, thread (f mod 4, t) walks its 16 bins with m ascending (pinv row entries are wave-uniform reads)
constexpr int ML_T = 64, ML_F = 64;

__global__ __launch_bounds__(256) void mel_to_linear_kernel(const float* __restrict__ mel, const int32_t* __restrict__ frames,
                                                            const float* __restrict__ pinv, int n_mels, int T_max, int log_input,
                                                            float floor_v, float* __restrict__ mag) {
    __shared__ float e[GL_MAXMEL][ML_T];
    const int b = blockIdx.z, t0 = blockIdx.x * ML_T, f0 = blockIdx.y * ML_F, i = threadIdx.x;
    const int fr = min(max(frames[b], 0), T_max);
    const int tx = i & (ML_T - 1), fy = i >> 6, t = t0 + tx;
    const bool live = t < fr;
    const float* mb = mel + (int64_t)b * n_mels * T_max;
    for (int m = fy; m < n_mels; m += 4) {
        float v = 0.f;
        if (live) {
            v = mb[(int64_t)m * T_max + t];
            if (log_input) v = expf(v);
        }
        e[m][tx] = v;
    }
    __syncthreads();
    if (t >= T_max) return;
    float* ob = mag + (int64_t)b * STFT_NBIN * T_max;
    for (int f = f0 + fy; f < min(f0 + ML_F, STFT_NBIN); f += 4) {
        float acc = 0.f;
        if (live) {
            const float* pr = pinv + (int64_t)f * n_mels;
            for (int m = 0; m < n_mels; ++m) acc += pr[m] * e[m][tx];
            acc = fmaxf(acc, floor_v);
        }
        ob[(int64_t)f * T_max + t] = acc;
    }
}

static int32_t mel_to_linear(const float* mel, const int32_t* frames, int32_t B, int32_t n_mels, int32_t T, const float* pinv,
                             int32_t log_input, float floor_v, float* mag, hipStream_t s) {
    TTS_REQUIRE(mel && frames && pinv && mag, "mel_to_linear: null argument");
    TTS_REQUIRE(n_mels >= 1 && n_mels <= GL_MAXMEL, "mel_to_linear: n_mels = %d outside [1, %d]", n_mels, GL_MAXMEL);
    TTS_REQUIRE(B >= 1 && B <= 65535 && T >= 1 && T <= (1 << 22), "mel_to_linear: bad batch %d / t_max %d (1 .. 65535 rows, 1 .. 2^22 frames)", B, T);
    hipLaunchKernelGGL(mel_to_linear_kernel, dim3((T + ML_T - 1) / ML_T, (STFT_NBIN + ML_F - 1) / ML_F, B), dim3(256), 0, s, mel, frames, pinv,
                       n_mels, T, log_input, floor_v, mag);
    TTS_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace ttsamd

using namespace ttsamd;

extern "C" {

int64_t ttsamd_griffinlim_workspace_bytes(int32_t batch, int32_t t_max, float momentum) {
    GlPlan p;
    return gl_plan(batch, t_max, momentum != 0.f, p) ? p.bytes : -1;
}

int32_t ttsamd_griffinlim(const float* mag, const int32_t* frames, int32_t batch, int32_t t_max, int32_t framing, int32_t n_iter,
                          float momentum, int32_t init, const uint64_t* seed_rows, uint64_t seed, void* phase, float* wave,
                          int64_t wave_stride, double* inconsistency, void* workspace, int64_t workspace_bytes, void* stream) {
    return griffinlim(mag, frames, batch, t_max, framing, n_iter, momentum, init, seed_rows, seed, (float2*)phase, wave, wave_stride,
                      inconsistency, workspace, workspace_bytes, (hipStream_t)stream);
}

int32_t ttsamd_mel_to_linear(const float* mel, const int32_t* frames, int32_t batch, int32_t n_mels, int32_t t_max, const float* pinv,
                             int32_t log_input, float floor, float* mag, void* stream) {
    return mel_to_linear(mel, frames, batch, n_mels, t_max, pinv, log_input, floor, mag, (hipStream_t)stream);
}

}  // extern "C"
