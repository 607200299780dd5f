"""The look-ahead limiter of include/ttsamd.h restated in numpy: the gain-reduction curve in Q30 int64, everything else in the float
formats the header names.  A checker for tests/test_limiter_cpu.py and tests/test_gpu_limiter.py; nothing here is fast."""
import numpy as np

Q = 1 << 30
A_MAX, R_MAX = 1024, 4096


def row_gain(mode, target, max_gain, L=None):
    """the float64 formula of the row gain, before its one rounding to fp32 -> float64, or None for a row that is left alone"""
    if mode == 2:
        if L is None or not np.isfinite(L):
            return None
        g = 10.0 ** ((float(np.float32(target)) - float(L)) / 20.0)
    elif mode == 3:
        g = 10.0 ** (float(np.float32(target)) / 20.0)
    else:
        return None
    return min(g, float(np.float32(max_gain)))


def q_plane(u, c):
    """u fp32 [n], c fp32 -> q int64 [n]: Q where not |u| > c, else floor(c / |u| * 2^30) with the division in float64"""
    d = np.abs(u.astype(np.float32))
    q = np.full(d.shape, Q, dtype=np.int64)
    over = d > np.float32(c)
    with np.errstate(divide='ignore', invalid='ignore'):
        q[over] = np.floor(np.float64(np.float32(c)) / d[over].astype(np.float64) * float(Q)).astype(np.int64)
    return q


def window_min(q, A, R):
    """m[i] = min q[j] over j in [i - R, i + A] within the row"""
    n = len(q)
    m = np.empty(n, dtype=np.int64)
    for i in range(n):
        m[i] = q[max(i - R, 0):min(i + A, n - 1) + 1].min()
    return m


def box_floor(m, A):
    """s[i] = floor(sum of m[clamp(i + k, 0, n - 1)] over k = -A .. A / (2A + 1)), int64"""
    n = len(m)
    if n == 0:
        return m.copy()
    ext = np.concatenate([np.full(A, m[0], dtype=np.int64), m.astype(np.int64), np.full(A, m[-1], dtype=np.int64)])
    c = np.concatenate([np.zeros(1, dtype=np.int64), np.cumsum(ext, dtype=np.int64)])       # exact in int64: terms of at most 2^30
    return (c[2 * A + 1:] - c[:n]) // (2 * A + 1)


def curves(x, g, c, A, R):
    """-> dict(u fp32, q, m, s int64, y fp32) of one row"""
    assert 0 <= A <= R and A <= A_MAX and R <= R_MAX
    x = np.asarray(x, dtype=np.float32)
    u = (x * np.float32(g)).astype(np.float32)
    q = q_plane(u, c)
    m = window_min(q, A, R)
    s = box_floor(m, A)
    with np.errstate(invalid='ignore', over='ignore'):
        y = (u.astype(np.float64) * s.astype(np.float64) * 2.0 ** -30).astype(np.float32)
    return dict(u=u, q=q, m=m, s=s, y=y)


def limit(x, g, c, A, R):
    """-> (y fp32 [n], reduction = min s, Q for an empty row)"""
    r = curves(x, g, c, A, R)
    return r['y'], int(r['s'].min()) if len(r['s']) else Q


def attack_hold(attack_ms, hold_ms, fs):
    """(A, R) in samples as ttsamd.engine.LoudnessEngine.limit takes them from milliseconds"""
    A = int(round(attack_ms * fs / 1000.0))
    return A, max(int(round(hold_ms * fs / 1000.0)), A)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
