"""Shared by tests/test_oversmoothing_cpu.py, tests/test_gpu_oversmoothing.py and tools/gen_golden_oversmoothing.py (not a test module):
the fp32 restatement of the reference's DTW, the float64 restatement of its four cepstral series, numpy's summary of a series, and the
builders that make every test input from a seed (the golden file holds a digest of the inputs and the reference's outputs only).

The DTW contract (include/ttsamd.h: ttsamd_dtw) is what the reference's text computes when it runs as plain Python over NumPy 2 scalars:
every operation is one IEEE fp32 operation.  `dtw_fp32` does the same operations on whole anti-diagonals: numpy's elementwise fp32
add / sub / mul / div / sqrt are correctly rounded, so the result is the same bits."""
import hashlib

import numpy as np

KEYS = ('HQER', 'CSlope', 'CCentroid', 'CRoll95')
INF = np.float32(1e30)


# ---------------------------------------------------------------------------------------------------------------------------- DTW ----
def local_cost_fp32(A, B, metric):
    """A [Ta, M], B [Tb, M] float32 -> C [Ta, Tb] float32; the sums run over k in order, one fp32 operation at a time."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    Ta, M = A.shape
    Tb = B.shape[0]
    if metric == 0:
        s = np.zeros((Ta, Tb), np.float32)
        for k in range(M):
            d = A[:, k, None] - B[None, :, k]
            s = s + d * d
        return np.sqrt(s)
    num, na, nb = np.zeros((Ta, Tb), np.float32), np.zeros(Ta, np.float32), np.zeros(Tb, np.float32)
    for k in range(M):
        num = num + A[:, k, None] * B[None, :, k]
        na = na + A[:, k] * A[:, k]
        nb = nb + B[:, k] * B[:, k]
    den = np.sqrt(na)[:, None] * np.sqrt(nb)[None, :] + np.float32(1e-12)
    with np.errstate(invalid='ignore', divide='ignore'):
        sim = num / den
    sim = np.where(sim > 1, np.float32(1), np.where(sim < -1, np.float32(-1), sim)).astype(np.float32)
    return np.float32(1) - sim


def dtw_fp32(A, B, metric=0, window=-1):
    """A [Ta, M], B [Tb, M] (time-major, as the reference's core takes them) -> (cost float32, path int32 [L, 2])."""
    A, B = np.asarray(A, np.float32), np.asarray(B, np.float32)
    Ta, Tb = A.shape[0], B.shape[0]
    D = np.full((Ta + 1, Tb + 1), INF, np.float32)
    D[0, 0] = 0
    P = np.full((max(Ta, 1), max(Tb, 1)), -1, np.int8)
    if Ta and Tb:
        C = local_cost_fp32(A, B, metric)
        for d in range(Ta + Tb - 1):
            i = np.arange(max(0, d - Tb + 1), min(Ta - 1, d) + 1)
            j = d - i
            if window >= 0:
                keep = np.abs(i - j) <= window
                i, j = i[keep], j[keep]
                if not i.size:
                    continue
            up, left, diag = D[i, j + 1], D[i + 1, j], D[i, j]
            best, bp = up.copy(), np.zeros(i.size, np.int8)
            m = left < best
            best[m], bp[m] = left[m], 1
            m = diag < best
            best[m], bp[m] = diag[m], 2
            D[i + 1, j + 1] = C[i, j] + best
            P[i, j] = bp
    path = []
    i, j = Ta - 1, Tb - 1
    while i >= 0 and j >= 0:
        bp = P[i, j]
        if bp < 0:
            break
        path.append((i, j))
        if bp == 2:
            i, j = i - 1, j - 1
        elif bp == 0:
            i -= 1
        else:
            j -= 1
    return D[Ta, Tb], np.asarray(path[::-1], np.int32).reshape(-1, 2)


# ------------------------------------------------------------------------------------------------------------------------- series ----
def hann_fp32(n):
    """np.hanning(n) as the reference holds it: float64, rounded once to fp32."""
    return np.hanning(n).astype(np.float32)


def power_f64(mel, center=True, hann=True):
    """mel [n_mels, T] -> P [Q, T] float64: the frame's mean over the bands removed, the fp32 hann window, |rfft|^2."""
    X = np.asarray(mel, np.float32).astype(np.float64)
    if center:
        X = X - X.mean(axis=0, keepdims=True)
    if hann:
        X = X * hann_fp32(X.shape[0]).astype(np.float64)[:, None]
    C = np.fft.rfft(X, axis=0)
    return C.real ** 2 + C.imag ** 2


def series_from_power_f64(P, q_c=None, q1=1, q2=None, eps=1e-8, p=0.95, hqer_scale=100.0):
    """P [Q, T] -> [4, T] float64 in the order KEYS (CRoll95 as a float)."""
    P = np.asarray(P, np.float64)
    Q, T = P.shape
    if q_c is None:
        q_c = max(1, min(int(np.floor(0.25 * Q)), Q - 1))
    q2 = Q - 1 if q2 is None else q2
    tot = P[1:Q].sum(axis=0)
    hqer = hqer_scale * (P[q_c:Q].sum(axis=0) / (tot + 1e-12))
    q = np.arange(q1, q2 + 1, dtype=np.float64)
    if q.size < 2:
        slope = np.full(T, np.nan)
    else:
        y = 10.0 * np.log10(P[q1:q2 + 1] + eps)
        qm = q.mean()
        slope = ((q[:, None] - qm) * (y - y.mean(axis=0))).mean(axis=0) / (((q - qm) ** 2).mean() + 1e-12)
    cent = (np.arange(Q, dtype=np.float64)[1:, None] * P[1:Q]).sum(axis=0) / (tot + 1e-12)
    cum = np.cumsum(np.concatenate([np.zeros((1, T)), P[1:Q]]), axis=0)
    ge = cum >= (p * (cum[-1] + 1e-12))[None]
    roll = np.where(ge.any(axis=0), ge.argmax(axis=0), 1).astype(np.float64)
    return np.stack([hqer, slope, cent, roll])


def series_f64(mel, center=True, hann=True, q_c=None):
    return series_from_power_f64(power_f64(mel, center, hann), q_c)


def series_np32(mel, center=True, hann=True, q_c=None):
    """The same four series in numpy's fp32 arithmetic on the CPU (np.fft.rfft of a float32 array is single precision in NumPy 2; sums
    are numpy's pairwise fp32 sums): the reference's own precision, measured against series_f64 by the GPU test in the run that uses it."""
    X = np.asarray(mel, np.float32)
    if center:
        X = X - X.mean(axis=0, keepdims=True)
    if hann:
        X = X * hann_fp32(X.shape[0])[:, None]
    C = np.fft.rfft(X, axis=0)
    P = C.real ** 2 + C.imag ** 2
    assert P.dtype == np.float32
    Q, T = P.shape
    if q_c is None:
        q_c = max(1, min(int(np.floor(0.25 * Q)), Q - 1))
    tot = P[1:Q].sum(axis=0) + np.float32(1e-12)
    q = np.arange(1, Q, dtype=np.float32)
    y = np.float32(10) * np.log10(P[1:Q] + np.float32(1e-8))
    qm = q.mean()
    slope = ((q[:, None] - qm) * (y - y.mean(axis=0))).mean(axis=0) / (((q - qm) ** 2).mean() + np.float32(1e-12))
    cum = np.cumsum(np.concatenate([np.zeros((1, T), np.float32), P[1:Q]]), axis=0)
    ge = cum >= (np.float32(0.95) * (cum[-1] + np.float32(1e-12)))[None]
    roll = np.where(ge.any(axis=0), ge.argmax(axis=0), 1).astype(np.float32)
    return np.stack([np.float32(100) * (P[q_c:Q].sum(axis=0) / tot), slope, (q[:, None] * P[1:Q]).sum(axis=0) / tot, roll])


def roll_near_tie(P, p=0.95, rel=1e-5):
    """Frames whose float64 cumulative power comes within rel * total of the roll-off target: [T] bool.  There the index depends on
    rounding, in the reference's fp32 as much as anywhere, and is left out of exact comparisons (at most 2 % of a case's frames)."""
    P = np.asarray(P, np.float64)
    cum = np.cumsum(P[1:], axis=0)
    tot = cum[-1] + 1e-12
    return (np.abs(cum - p * tot) <= rel * tot).any(axis=0)


# ------------------------------------------------------------------------------------------------------------------------ summary ----
def nan_interp(x):
    x = np.asarray(x, np.float32).copy()
    nan = np.isnan(x)
    if not nan.any():
        return x
    if nan.all():
        return np.zeros_like(x)
    idx = np.arange(x.size, dtype=np.float32)
    x[nan] = np.interp(idx[nan], idx[~nan], x[~nan])
    return x


def zscore_numpy(x):
    """numpy's own fp32 route (nanmean / nanstd, then (x - m) / s): (z, m, s)."""
    with np.errstate(all='ignore'):
        m, s = np.nanmean(x), np.nanstd(x)
        if not np.isfinite(s) or s == 0:
            return np.zeros_like(x, dtype=np.float32), m, s
        return ((x - m) / s).astype(np.float32), m, s


# ------------------------------------------------------------------------------------------------------------------------- inputs ----
def warped_pair(seed, n_mels, ta, tb, noise=0.05, smooth=4):
    """A mel-like pair: a [n_mels, ta] = time-smoothed noise of sigma 2 over a slow ripple across the bands, around -4 (a log-mel's
    range; white across the bands, so that no cepstral bin is starved: the tests assert min P[q >= 1] >= 1e-4), b = a resampled in time
    to tb frames by a monotone random warp, plus noise."""
    rng = np.random.default_rng(seed)
    a = rng.normal(0, 1, (n_mels, ta + smooth))
    a = np.cumsum(a, axis=1)
    a = (a[:, smooth:] - a[:, :-smooth]) / np.sqrt(smooth)        # moving sum over time
    a = 2.0 * a + 1.5 * np.sin(np.arange(n_mels) / 5.0)[:, None] - 4.0
    a = a.astype(np.float32)
    steps = rng.uniform(0.5, 1.5, tb)
    pos = np.cumsum(steps)
    idx = np.round((pos - pos[0]) / (pos[-1] - pos[0]) * (ta - 1)).astype(int) if tb > 1 else np.zeros(1, int)
    b = (a[:, idx] + noise * rng.normal(0, 1, (n_mels, tb))).astype(np.float32)
    return a, b


def plateau_series(seed, n, levels=6, run=9):
    """An integer-valued series with long exact plateaus (as CRoll95 is): equal values everywhere, so the tie order decides the path."""
    rng = np.random.default_rng(seed)
    v = np.repeat(rng.integers(1, levels + 1, n // run + 1), run)[:n]
    return v.astype(np.float32)


GOLDEN_PAIRS = {'p80': (20, 80, 180, 160), 'p100': (17, 100, 176, 158)}        # seed, n_mels, Ta, Tb
NAN_FRAMES = (0, 1, 17, 60, 61, 62, 159)                                      # injected into CSlope of p80's second series
TIGHT_WINDOW = 10                                                             # narrower than |Ta - Tb| of both pairs


def golden_inputs():
    """{name: (a, b)} of the golden cases, rebuilt from the seeds."""
    return {k: warped_pair(*v) for k, v in GOLDEN_PAIRS.items()}


def inputs_digest(inputs):
    h = hashlib.sha256()
    for k in sorted(inputs):
        for x in inputs[k]:
            h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()
