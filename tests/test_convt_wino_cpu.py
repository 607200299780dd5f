"""CPU: the transposed conv of HiFi-GAN's upsamplers as a two-tap Conv1d on Winograd F(4,2) (csrc/conv_wino4.hip: launch_convt_wino),
restated in numpy step by step -- what the kernel computes, in the order of its stages:

    y[co][u tau + j - u/2] = b[co] + sum_ci W[ci][co][j] a[ci][tau] + W[ci][co][j + u] a[ci][tau - 1],  j = 0..u-1, tau = 0..len, a[-1] = a[len] = 0

  * row = co u + j of a (u Cout)-row conv with the taps (g0, g1, g2) = (W[..][j + u], W[..][j], 0) and pad 1;
  * U0..U4 of conv_wino4.hip's header with g2 = 0, formed in float64 and rounded once (U5 = g2 = 0 is never multiplied);
  * V0..V4 on the window x0..x4 = a[4 t - 1 .. 4 t + 3] of output quad t (x5 is never read), zeros outside [0, len);
  * five products per quad summed over C-in, the output transform without P5, the bias after the sum;
  * positions tau = 0 .. len INCLUSIVE, outputs stored for 0 <= n < u len only.

Exactness: with integer inputs and weights that are integer multiples of 24 every U, V, product and sum is an integer far below 2^53, so in
float64 the restatement must equal torch.conv_transpose1d bit for bit (any slip in an index, a sign or a coefficient shows).  In float32 on
randn data with tests/test_gpu_convt.py's weight scaling it is held against float64 to 5e-5, the bound tests/test_gpu_wino4_epilogue.py holds
the same six-point transforms to on the GPU.  The host packer behind ttsamd_convt_wino_pack_weight (pure host code) is compared with the
restated layout [Cin/8][6][2][u Cout][4] + the bias per row bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

LENS = (1, 2, 3, 4, 5, 255, 256, 257)


def group_filters(w, u):
    """torch ConvTranspose1d weight [Cin][Cout][2u] -> U[5][rows][Cin] in float64, row = co u + j."""
    cin, cout, _ = w.shape
    w = np.asarray(w, np.float64)
    g0 = w[:, :, u:].transpose(1, 2, 0).reshape(cout * u, cin)      # W[ci][co][j + u]: the tap on a[tau - 1]
    g1 = w[:, :, :u].transpose(1, 2, 0).reshape(cout * u, cin)      # W[ci][co][j]:     the tap on a[tau]
    return np.stack([g0 / 4, -(g0 + g1) / 6, -(g0 - g1) / 6, g0 / 24 + g1 / 12, g0 / 24 - g1 / 12])


def convt_wino(a, w, b, u, dtype):
    """a [Cin][len] (already activated), w [Cin][Cout][2u], b [Cout] -> y [Cout][u len], every stage in `dtype`."""
    cin, n = a.shape
    cout = w.shape[1]
    U = group_filters(w, u).astype(dtype)                            # one rounding
    nq = (n + 1 + 3) // 4                                            # quads that cover tau = 0 .. len
    xp = np.zeros((cin, 4 * nq + 4), dtype)                          # xp[:, 1 + t] = a[:, t]: a[-1] and a[len ..] are zeros
    xp[:, 1:1 + n] = a.astype(dtype)
    x = [xp[:, i:i + 4 * nq:4] for i in range(5)]                    # x0..x4 of quad t = a[4 t - 1 + i]
    four, five, two = dtype(4), dtype(5), dtype(2)
    V = [four * x[0] + (x[4] - five * x[2]),
         (x[4] - four * x[2]) + (x[3] - four * x[1]),
         (x[4] - four * x[2]) - (x[3] - four * x[1]),
         (x[4] - x[2]) + two * (x[3] - x[1]),
         (x[4] - x[2]) - two * (x[3] - x[1])]
    P = [U[k] @ V[k] for k in range(5)]                              # [rows][quads]
    assert P[0].dtype == dtype
    s12, d12, s34, d34 = P[1] + P[2], P[1] - P[2], P[3] + P[4], P[3] - P[4]
    yq = np.stack([P[0] + s12 + s34, d12 + two * d34, s12 + four * s34, d12 + dtype(8) * d34], axis=2)     # [rows][quads][4]
    ytau = yq.reshape(cout * u, 4 * nq) + np.repeat(np.asarray(b, dtype), u)[:, None]                         # [rows][tau], bias per row
    y = np.zeros((cout, u * n), dtype)
    for tau in range(n + 1):                                         # INCLUSIVE: tau = len gives the last u/2 outputs
        for j in range(u):
            k = u * tau + j - u // 2
            if 0 <= k < u * n:                                       # the store clip
                y[:, k] = ytau[j::u, tau]
    return y


@pytest.mark.parametrize('u', [2, 8])
def test_integer_data_equals_conv_transpose1d_exactly(u):
    rng = np.random.default_rng(u)
    cin, cout = 8, 3
    w = 24.0 * rng.integers(-4, 5, (cin, cout, 2 * u)).astype(np.float64)
    b = rng.integers(-9, 10, cout).astype(np.float64)
    for n in LENS:
        a = rng.integers(-7, 8, (cin, n)).astype(np.float64)
        ref = F.conv_transpose1d(torch.from_numpy(a)[None], torch.from_numpy(w), torch.from_numpy(b), stride=u, padding=u // 2)[0].numpy()
        got = convt_wino(a, w, b, u, np.float64)
        assert got.shape == ref.shape == (cout, u * n)
        assert np.array_equal(got, ref), f'u = {u}, len = {n}: max-abs {np.abs(got - ref).max()}'


@pytest.mark.parametrize('u', [2, 8])
def test_float32_against_float64(u):
    g = torch.Generator().manual_seed(40 + u)
    cin, cout = 128, 8
    w = (torch.randn(cin, cout, 2 * u, generator=g) / np.sqrt(2 * cin)).numpy()
    b = (torch.randn(cout, generator=g) * 0.3).numpy()
    worst = 0.0
    for n in LENS:
        a = F.leaky_relu(torch.randn(cin, n, generator=g), 0.1).numpy()
        ref = F.conv_transpose1d(torch.from_numpy(a).double()[None], torch.from_numpy(w).double(), torch.from_numpy(b).double(), stride=u,
                                 padding=u // 2)[0].numpy()
        got = convt_wino(a, w, b, u, np.float32)
        assert got.dtype == np.float32
        worst = max(worst, float(np.abs(got.astype(np.float64) - ref).max()))
    print(f'F(4,2) transposed conv in float32, u = {u}, Cin = {cin}: max-abs {worst:.2e} against float64')
    assert worst < 5e-5


@pytest.mark.parametrize('cin,cout,u', [(16, 8, 8), (32, 32, 2), (48, 24, 8)])
def test_host_packing_bit_for_bit(cin, cout, u):
    from ttsamd import lib as L
    lib = L.load()
    rng = np.random.default_rng(cin + u)
    w = rng.standard_normal((cin, cout, 2 * u)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    rows = u * cout
    n = int(lib.ttsamd_convt_wino_packed_floats(cin, cout, u))
    assert n == (6 * cin + 1) * rows
    out = np.full(n, np.nan, np.float32)
    L.check(lib.ttsamd_convt_wino_pack_weight(w.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), cin, cout, u,
                                              out.ctypes.data_as(C.c_void_p)), 'convt_wino_pack_weight')
    U = group_filters(w, u).astype(np.float32)                       # [5][rows][cin]
    want = np.zeros((cin // 8, 6, 2, rows, 4), np.float32)           # group 5: all zeros (fetched, never multiplied)
    for o in range(cin // 8):
        for kk in range(2):
            for pq in range(4):
                want[o, :5, kk, :, pq] = U[:, :, 8 * o + 2 * pq + kk]
    assert np.array_equal(out[:6 * cin * rows].view(np.uint32), want.reshape(-1).view(np.uint32))
    assert np.array_equal(out[6 * cin * rows:], np.repeat(b, u))
    # a shape the launch does not take: no packing, and the call says so
    assert lib.ttsamd_convt_wino_packed_floats(24, 8, 8) == 0 and lib.ttsamd_convt_wino_packed_floats(16, 8, 4) == 0
    assert lib.ttsamd_convt_wino_pack_weight(w.ctypes.data_as(C.c_void_p), None, 24, 8, 8, out.ctypes.data_as(C.c_void_p)) != 0
