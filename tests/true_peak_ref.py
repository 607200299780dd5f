"""The true-peak arithmetic of include/ttsamd.h restated in numpy: the 4x interpolator's table, its float64 chains by a loop over the
taps, the true peak with its upward rounding to fp32, and the limiter with the true-peak detector (everything behind the detector is
tests/limiter_ref.py).  A checker for tests/test_true_peak_cpu.py and tests/test_gpu_true_peak.py; nothing here is fast."""
import numpy as np

import limiter_ref as LR

W, J, P = 12, 25, 3                     # reach to either side, taps per phase, phases 1 .. 3
REACH = W + 1                           # what the detector adds to the limiter's reach on each side


def _table():
    """h[p - 1][j] = sinc(t) cos^2(t pi / 24), t = clamp((j - 12) - p / 4, -12, 12), float64, rounded once to fp32 (the resampler's
    formula at o = 1, n = 4, lowpass_filter_width = 12, rolloff = 1, in ttsamd/resample.py's order of operations)"""
    j = np.arange(-W, W + 1, dtype=np.float64)[None, :]
    p = np.arange(1, P + 1, dtype=np.float64)[:, None] / 4.0
    t = np.clip(j - p, -float(W), float(W))
    win = np.cos(t * np.pi / W / 2.0) ** 2
    tpi = t * np.pi
    sinc = np.where(tpi == 0.0, 1.0, np.sin(tpi) / np.where(tpi == 0.0, 1.0, tpi))
    h = (sinc * win).astype(np.float32)
    h.setflags(write=False)
    return h


TAPS = _table()                                             # fp32 [3, 25]
H = float(np.abs(TAPS.astype(np.float64)).sum(axis=1).max())      # the interpolator's largest gain on a bounded signal


def interpolate(x):
    """x fp32 [n] -> v float64 [n, 3]: v[i][p] = sum over j ascending of (double)h[p][j] (double)xz[i + j - 12] from +0.0"""
    x = np.asarray(x, dtype=np.float32)
    n = len(x)
    xz = np.concatenate([np.zeros(W), x.astype(np.float64), np.zeros(W)])
    h = TAPS.astype(np.float64)
    v = np.zeros((n, P), dtype=np.float64)
    for j in range(J):
        v += xz[j:j + n, None] * h[None, :, j]              # a product of two fp32 values is exact in float64: one rounding per step
    return v


def ceil32(m):
    """the smallest fp32 >= the float64 m >= 0"""
    f = np.float32(m)
    return f if float(f) >= m else np.nextafter(f, np.float32(np.inf))


def true_peak64(x):
    x = np.asarray(x, dtype=np.float32)
    if len(x) == 0:
        return 0.0
    return max(float(np.abs(x).max()), float(np.abs(interpolate(x)).max()))


def true_peak(x):
    """-> fp32: max(max |x|, max |v|) in float64, rounded upward; 0 for an empty row"""
    return ceil32(true_peak64(x))


def true_peak_db(x):
    tp = float(true_peak(x))
    return 20.0 * np.log10(tp) if tp > 0 else -np.inf


def detector(u):
    """u fp32 [n] -> d float64 [n] = max(|u[i]|, max_p |v[i][p]|, max_p |v[i - 1][p]|), the last term omitted for i = 0"""
    u = np.asarray(u, dtype=np.float32)
    vm = np.abs(interpolate(u)).max(axis=1) if len(u) else np.zeros(0)
    d = np.maximum(np.abs(u.astype(np.float64)), vm)
    d[1:] = np.maximum(d[1:], vm[:-1])
    return d


def q_plane(d, c):
    """d float64 [n], c fp32 -> q int64 [n]: Q where not d > c, else floor(c / d * 2^30) in float64"""
    c64 = np.float64(np.float32(c))
    q = np.full(d.shape, LR.Q, dtype=np.int64)
    over = d > c64
    q[over] = np.floor(c64 / d[over] * float(LR.Q)).astype(np.int64)
    return q


def curves(x, g, c, A, R):
    """tests/limiter_ref.py's curves with the true-peak detector -> dict(u fp32, d float64, q, m, s int64, y fp32) of one row"""
    assert 0 <= A <= R and A <= LR.A_MAX and R <= LR.R_MAX
    x = np.asarray(x, dtype=np.float32)
    u = (x * np.float32(g)).astype(np.float32)
    d = detector(u)
    q = q_plane(d, c)
    m = LR.window_min(q, A, R)
    s = LR.box_floor(m, A)
    y = (u.astype(np.float64) * s.astype(np.float64) * 2.0 ** -30).astype(np.float32)
    return dict(u=u, d=d, q=q, m=m, s=s, y=y)


def limit(x, g, c, A, R):
    """-> (y fp32 [n], reduction = min s, Q for an empty row)"""
    r = curves(x, g, c, A, R)
    return r['y'], int(r['s'].min()) if len(r['s']) else LR.Q


def level_bound(ceiling):
    """the levelled row's true peak is at most this (include/ttsamd.h): ceiling (1 + H 2^-24)"""
    return float(np.float32(ceiling)) * (1.0 + H * 2.0 ** -24)
