"""Shared by tests/test_objective_cpu.py and tests/test_gpu_objective.py (not a test module): the float64 numpy restatement of the two
definitions of include/ttsamd.h (ttsamd_mel_cepstrum, ttsamd_dtw_aligned_eval), written from their text, and the random monotone paths
the tests walk.  The reference has no such module, so this restatement is the yardstick."""
import numpy as np

KEYS = ('n', 'mcd', 'mel_mae', 'n_vv', 'f0_rmse_cents', 'f0_rmse_hz', 'f0_corr', 'vuv_error')
MCD_SCALE = 10.0 * np.sqrt(2.0) / np.log(10.0)


def cepstrum(logmel, n_coef):
    """[M, T] -> [n_coef, T] float64: c_k = s_k sum_m x_m cos(pi k (2m + 1) / (2M)), the argument reduced mod 4M in integers."""
    x = np.asarray(logmel, np.float64)
    M = x.shape[0]
    k, m = np.arange(n_coef)[:, None], np.arange(M)[None, :]
    basis = np.cos(np.pi * ((k * (2 * m + 1)) % (4 * M)) / (2.0 * M))
    s = np.full(n_coef, np.sqrt(2.0 / M))
    s[0] = np.sqrt(1.0 / M)
    return s[:, None] * (basis @ x)


def voiced(f0):
    f0 = np.asarray(f0, np.float64)
    with np.errstate(invalid='ignore'):
        return np.isfinite(f0) & (f0 > 0)


def aligned_eval(cep_a, cep_b, path, mel_a=None, mel_b=None, f0_a=None, f0_b=None, first_coef=1, scale=MCD_SCALE):
    """cep_* [C, T*], path [n, 2] (the steps themselves) -> the eight stats as float64 [8]"""
    path = np.asarray(path, np.int64).reshape(-1, 2)
    n = path.shape[0]
    out = np.full(8, np.nan)
    out[0] = n
    if f0_a is not None:
        out[3] = 0
    if n == 0:
        return out
    i, j = path[:, 0], path[:, 1]
    d = np.asarray(cep_a, np.float64)[first_coef:, i] - np.asarray(cep_b, np.float64)[first_coef:, j]
    out[1] = scale * np.sqrt((d * d).sum(axis=0)).mean()
    if mel_a is not None:
        out[2] = np.abs(np.asarray(mel_a, np.float64)[:, i] - np.asarray(mel_b, np.float64)[:, j]).mean()
    if f0_a is None:
        return out
    x, y = np.asarray(f0_a, np.float64)[i], np.asarray(f0_b, np.float64)[j]
    vx, vy = voiced(x), voiced(y)
    vv = vx & vy
    out[3] = vv.sum()
    out[7] = (vx != vy).sum() / n
    if vv.any():
        x, y = x[vv], y[vv]
        out[4] = np.sqrt(((1200.0 * np.log2(x / y)) ** 2).mean())
        out[5] = np.sqrt(((x - y) ** 2).mean())
        if x.size >= 2:
            dx, dy = x - x.mean(), y - y.mean()
            sxx, syy = (dx * dx).sum(), (dy * dy).sum()
            if sxx > 0 and syy > 0:
                out[6] = (dx * dy).sum() / np.sqrt(sxx * syy)
    return out


def random_path(rng, ta, tb, n=None):
    """A monotone path from (0, 0) towards (ta - 1, tb - 1) with steps (1, 0), (0, 1), (1, 1), as DTW makes them; cut to n steps if given."""
    i = j = 0
    steps = [(0, 0)]
    while i < ta - 1 or j < tb - 1:
        move = rng.integers(0, 3)
        if i == ta - 1:
            move = 1
        elif j == tb - 1:
            move = 0
        i, j = i + (move != 1), j + (move != 0)
        steps.append((i, j))
    p = np.asarray(steps, np.int32)
    return p if n is None else p[:n]


def padded_paths(paths, ta_max, tb_max):
    """list of [n_b, 2] -> (int32 [B, ta_max + tb_max, 2] with zeros past each path, int32 [B]): ttsamd_dtw's layout"""
    out = np.zeros((len(paths), ta_max + tb_max, 2), np.int32)
    for b, p in enumerate(paths):
        out[b, :len(p)] = p
    return out, np.asarray([len(p) for p in paths], np.int32)
