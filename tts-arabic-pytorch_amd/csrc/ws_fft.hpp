// The float64 transform of the wave-against-wave scores (wavescore.hip, mrstft.hip): ws_fft<N>, Stockham autosort passes over two split
// (re | im) buffers of N doubles each in LDS, radix 4 (N / 4 threads) and, for N = 2 * 4^a (512, 2048), one last radix-2 pass; twiddles
// exp(-2 pi i m / N) from a float64 table the block builds once in LDS (sincospi).  Thread i of the radix-4 pass p (p = 1, 4, 16 ..)
// takes a[i + r N / 4] * tw[r k N / (4 p)], r = 0 .. 3, k = i % p, and writes the butterfly to b[4 (i - k) + k + p r] (the scheme of
// fft1024.hpp); the result is in natural order (checked against numpy.fft in double before the kernels were written: 5e-14 on
// unit-variance complex input).  N = 512 serves STOI (the 256-sample frame zero-padded), N = 1024 the log-spectral distance, all three
// sizes the multi-resolution STFT distance.
//
// LDS traffic (64-bit accesses: a bank is (byte address / 4) mod 64 for the reads, mod 32 for the writes).  The data reads a[i + r N / 4]
// are consecutive doubles over the lanes: conflict-free.  The data writes b[4 (i - k) + k + p r] are stride-4 doubles over the lanes in
// pass p = 1 and runs of 4 doubles 16 apart in pass p = 4: 4 distinct addresses per bank in a group of 16 lanes (4-way); from p = 16 on
// a group writes 16 consecutive doubles and is conflict-free.  The twiddle reads tw[r k N / (4 p)] have stride r N / (4 p) doubles
// over k: one address (a broadcast) in pass 1, then p distinct addresses that share a bank as long as N / (4 p) is a multiple of 32
// doubles -- 4-way in pass 4, up to 16-way in pass 16 at N = 2048 -- and spread out in the later passes (2-way in the last radix-4 pass).
#pragma once
#include <cmath>

#include "common.hpp"

// the scores are specified by their arithmetic, operation for operation: a product and the sum behind it are rounded one after the other
// (no fused multiply-add), so that e.g. alpha ref - est is the difference of two rounded numbers here as it is in the restatement
#pragma clang fp contract(off)

namespace ttsamd {

__device__ __forceinline__ int64_t ws_len(const int64_t* __restrict__ ns, const int b, const int64_t stride) {
    return max((int64_t)0, min(ns[b], stride));
}

// tw[m] = exp(-2 pi i m / N) for m < N, by all threads of the block; the caller synchronises
template <int N>
__device__ __forceinline__ void ws_twiddles(double* twr, double* twi) {
    for (int m = threadIdx.x; m < N; m += blockDim.x) {
        double s, c;
        sincospi(2.0 * (double)m / (double)N, &s, &c);
        twr[m] = c;
        twi[m] = -s;
    }
}

__device__ __forceinline__ void ws_cmul(double& xr, double& xi, const double wr, const double wi) {
    const double r = xr * wr - xi * wi, im = xr * wi + xi * wr;
    xr = r;
    xi = im;
}

// in: (ar, ai) natural order, filled and synchronised by the caller; every thread of the block calls (the barriers are the block's):
// threads i < N / 4 work in the radix-4 passes; the last pass of N = 512 / 2048 is shared by T2 threads (N / 2: one butterfly each, as in
// the STOI kernel; N / 4: two each), the others only wait.  Returns through (ar, ai) the pointers of the buffer that holds the result;
// ends with a barrier.
template <int N, int T2 = N / 2>
__device__ __forceinline__ void ws_fft(double*& ar, double*& ai, double*& br, double*& bi, const double* twr, const double* twi,
                                       const int i) {
    constexpr int Q = N / 4, H = N / 2;
    int p = 1, tstep = Q;                                      // N / (4 p)
#pragma unroll 1
    for (; 4 * p <= N; p <<= 2, tstep >>= 2) {
        if (i < Q) {
            const int k = i & (p - 1), j = ((i - k) << 2) + k, m = k * tstep;
            const double u0r = ar[i], u0i = ai[i];
            double u1r = ar[i + Q], u1i = ai[i + Q], u2r = ar[i + 2 * Q], u2i = ai[i + 2 * Q], u3r = ar[i + 3 * Q], u3i = ai[i + 3 * Q];
            ws_cmul(u1r, u1i, twr[m], twi[m]);                 // the first pass multiplies by tw[0] = (1, -0): exact
            ws_cmul(u2r, u2i, twr[2 * m], twi[2 * m]);
            ws_cmul(u3r, u3i, twr[3 * m], twi[3 * m]);
            const double a0r = u0r + u2r, a0i = u0i + u2i, a1r = u0r - u2r, a1i = u0i - u2i;
            const double a2r = u1r + u3r, a2i = u1i + u3i;
            const double a3r = u1i - u3i, a3i = -(u1r - u3r);  // (u1 - u3) * (-i)
            br[j] = a0r + a2r;
            bi[j] = a0i + a2i;
            br[j + p] = a1r + a3r;
            bi[j + p] = a1i + a3i;
            br[j + 2 * p] = a0r - a2r;
            bi[j + 2 * p] = a0i - a2i;
            br[j + 3 * p] = a1r - a3r;
            bi[j + 3 * p] = a1i - a3i;
        }
        __syncthreads();
        double* t = ar; ar = br; br = t;
        t = ai; ai = bi; bi = t;
    }
    if (p < N) {                                               // N = 2 * 4^a: one radix-2 pass, p = N / 2, k = h
        if (i < T2) {
#pragma unroll
            for (int h = i; h < H; h += T2) {
                const double u0r = ar[h], u0i = ai[h];
                double u1r = ar[h + H], u1i = ai[h + H];
                ws_cmul(u1r, u1i, twr[h], twi[h]);
                br[h] = u0r + u1r;
                bi[h] = u0i + u1i;
                br[h + H] = u0r - u1r;
                bi[h + H] = u0i - u1i;
            }
        }
        __syncthreads();
        double* t = ar; ar = br; br = t;
        t = ai; ai = bi; bi = t;
    }
}

}  // namespace ttsamd
