"""Seven-point input transform of the F(4,3) kernel on SHARED PARTIAL SUMS (csrc/conv_wino4.hip, the PT7 branch of TTS_WRITE_JOB),
numerics on the CPU: the evaluation order that ships, emulated in float32 with one rounding per fma / add, next to the order it
replaces (every row written out term by term).

With f(i) = x[i+2] - 4 x[i], e(i) = f(i) - 2 f(i+1), d(i) = x[i] - x[i+2], h(i) = d(i) - 2 d(i+1) on the sub-filter's positions x0..x6:
    V0 = e(2) - e(0)     V1 = e(1) + e(2)     V2 = e(1) - e(2)     V6 = e(1) - e(3)
    V3 = 2 h(1) + h(2)   V4 = 2 h(1) - h(2)   V5 = f(3) - f(1)
Every multiplier is a power of two, so each line is ONE rounding whether or not the compiler fuses it: plain float32 arithmetic is the
exact emulation.  The three-tap sub-filter has no V6: f(4) and e(3) are not formed and x6 is not read.

The old rows have multipliers 3, 5, 7, 9, 10, 12 and are emulated as the compiler contracted them for gfx950 (read from the code of
the build this order replaces): of a sum or difference of two products one is fused and the other rounded -- 10 x3 - (5 x2), (5 x3) - 10 x4,
2 (x1 +- x5) + (3 | 5 (x4 - x2)).  The fused step goes through float64, whose double rounding shows in about one value in 2^29 -- it is
the baseline of a ratio, not the thing under test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_wino_f43_numerics_cpu import _lin
from test_wino44_numerics_cpu import AT44, BT44, G44

F32 = np.float32


def shared_rows(x, taps=4):
    """V0..V6 (three taps: V0..V5) of the windows x[7 or 6][...] in the order the kernel evaluates them; the dtype of x carries through
    (float32: the emulation, float64 / integers: the identities)."""
    c2, c4 = x[0].dtype.type(2), x[0].dtype.type(4)
    f = [x[i + 2] - c4 * x[i] for i in range(5 if taps == 4 else 4)]
    e0 = f[0] - c2 * f[1]
    e2 = f[2] - c2 * f[3]
    v0 = e2 - e0
    e1 = f[1] - c2 * f[2]
    v1 = e1 + e2
    v2 = e1 - e2
    v5 = f[3] - f[1]
    d = [None] + [x[i] - x[i + 2] for i in (1, 2, 3)]
    h1 = d[1] - c2 * d[2]
    h2 = d[2] - c2 * d[3]
    v3 = c2 * h1 + h2
    v4 = c2 * h1 - h2
    rows = [v0, v1, v2, v3, v4, v5]
    if taps == 4:
        e3 = f[3] - c2 * f[4]
        rows.append(e1 - e3)
    return rows


def _fma(a, b, c):
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(F32)


def term_by_term_rows(x, taps=4):
    """the rows as the kernel evaluated them before: five or six terms each, nothing shared (float32 windows)"""
    x0, x1, x2, x3, x4, x5 = x[:6]
    n = lambda c: F32(c)
    v0 = ((n(4) * x0 - n(8) * x1) + _fma(n(10), x3, -(n(5) * x2))) + (x4 - n(2) * x5)
    v1 = _fma(n(4), x2 - x1, _fma(n(9), x3, -x4)) - n(2) * x5
    v2 = _fma(n(-7), x3, _fma(n(12), x2, -(n(4) * x1)) + _fma(n(-3), x4, n(2) * x5))
    v3 = (n(2) * (x1 + x5) + n(3) * (x4 - x2)) - n(4) * x3
    v4 = n(2) * (x1 - x5) + n(5) * (x4 - x2)
    v5 = n(4) * x1 + _fma(n(-5), x3, x5)
    rows = [v0, v1, v2, v3, v4, v5]
    if taps == 4:
        rows.append(((n(8) * x2 - n(4) * x1) + _fma(n(-10), x4, n(5) * x3)) + (n(2) * x[6] - x5))
    return rows


@pytest.mark.parametrize('taps', [4, 3])
def test_shared_rows_are_the_matrix_exactly(taps):
    """On integer windows every operation of either form is exact in float64: the factorisation must give the rows of B^T bit for bit."""
    rng = np.random.default_rng(7)
    x = rng.integers(-(1 << 20), 1 << 20, size=(7, 4096)).astype(np.float64)
    if taps == 3:
        x[6] = 1e30                                                  # never read by the three-tap form
    got = shared_rows(list(x[:7 if taps == 4 else 6]), taps)
    nrow = 7 if taps == 4 else 6
    want = BT44[:nrow, :6] @ x[:6] if taps == 3 else BT44 @ x
    assert len(got) == nrow
    for i in range(nrow):
        assert np.array_equal(got[i], want[i]), f'V{i}'


@pytest.mark.parametrize('taps', [4, 3])
def test_shared_rows_round_no_worse_than_term_by_term(taps):
    """2^20 windows of leaky-ReLU(0.1)'d randn: per-row rms error against float64 of the shared-sum order at most 1.1x that of the
    term-by-term order, both measured here (it comes to 0.95 - 1.09x: V2 and V5 pass one more rounding than before, V0 and V6 fewer; the
    ratio moves by about 0.002 with the sample)."""
    g = torch.Generator().manual_seed(44)
    x = F.leaky_relu(torch.randn(7, 1 << 20, generator=g), 0.1).numpy()
    nrow = 7 if taps == 4 else 6
    npos = 7 if taps == 4 else 6
    exact = BT44[:nrow, :npos] @ x[:npos].astype(np.float64)
    new = shared_rows(list(x[:npos]), taps)
    old = term_by_term_rows(list(x[:npos]), taps)
    assert all(v.dtype == F32 for v in new) and all(v.dtype == F32 for v in old)
    for i in range(nrow):
        en, eo = new[i].astype(np.float64) - exact[i], old[i].astype(np.float64) - exact[i]
        rn, ro = float(np.sqrt((en ** 2).mean())), float(np.sqrt((eo ** 2).mean()))
        print(f'taps {taps} V{i}: rms shared {rn:.3e} term-by-term {ro:.3e} ({rn / ro:.3f}x), max {np.abs(en).max():.2e} / {np.abs(eo).max():.2e}')
        assert rn <= 1.1 * ro


def shared_rows_conv1d_fp32(x, w, bias, dilation):
    """'same' Conv1d in float32 through the seven-point groups (test_wino44_numerics_cpu.wino44_conv1d_fp32) with the input transform in the
    kernel's shared-sum order."""
    B, Ci, L = x.shape
    Co, _, k = w.shape
    nsf, half, m = (k + 3) // 4, (k - 1) // 2, 4
    w64 = np.zeros((Co, Ci, 4 * nsf))
    w64[:, :, :k] = w.double().numpy()
    Us = [[torch.from_numpy(np.einsum('t,oct->oc', G44[i], w64[:, :, 4 * s:4 * s + 4]).astype(np.float32)) for i in range(7)]
          for s in range(nsf)]
    y = torch.zeros(B, Co, L, dtype=torch.float32)
    for r in range(dilation):
        xr = x[:, :, r::dilation]
        Lr = xr.shape[2]
        J = -(-Lr // m)
        xp = F.pad(xr, (half, m * J + k - Lr))
        planes_U, planes_V = [[] for _ in range(7)], [[] for _ in range(7)]
        for s in range(nsf):
            taps = 4 if 4 * s + 3 < k else 3
            X = [xp[:, :, 4 * s + mm:4 * s + mm + m * J:m].numpy() for mm in range(7 if taps == 4 else 6)]
            for i, v in enumerate(shared_rows(X, taps)):
                assert v.dtype == F32
                planes_U[i].append(Us[s][i])
                planes_V[i].append(torch.from_numpy(np.ascontiguousarray(v)))
        P = [torch.matmul(torch.cat(planes_U[i], 1), torch.cat(planes_V[i], 1)) for i in range(7)]
        for o in range(m):
            yo = _lin(AT44[o], P)
            idx = torch.arange(o, m * J, m)
            keep = idx < Lr
            y[:, :, r::dilation][:, :, idx[keep]] = yo[:, :, :int(keep.sum())]
    return y + bias[None, :, None]


@pytest.mark.parametrize('k,d', [(7, 1), (11, 1), (7, 3), (11, 5)])
def test_whole_conv_on_shared_rows(k, d):
    """one conv (Cin 16, Cout 8, L 64) through transform, product and output transform: the bound of test_wino44_numerics_cpu.py"""
    g = torch.Generator().manual_seed(100 * k + d)
    x = F.leaky_relu(torch.randn(2, 16, 64, generator=g), 0.1)
    w = torch.randn(8, 16, k, generator=g) / (16 * k) ** 0.5
    b = torch.randn(8, generator=g)
    want = F.conv1d(x.double(), w.double(), b.double(), dilation=d, padding=d * (k - 1) // 2)
    e = float((shared_rows_conv1d_fp32(x, w, b, d).double() - want).abs().max())
    print(f'k={k} d={d}: shared-sum seven-point conv max-abs {e:.2e} against float64')
    assert e < 2e-5
