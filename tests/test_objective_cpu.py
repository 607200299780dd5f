"""CPU: the float64 restatement tests/objective_ref.py (the yardstick of tests/test_gpu_objective.py; the reference has no objective
evaluation module) against scipy's DCT, numpy's corrcoef and hand-made tiny cases, and the surface of utils.objective."""
import inspect

import numpy as np
import pytest

import objective_ref as R


@pytest.mark.parametrize('M,n_coef', [(1, 1), (80, 13), (80, 80), (100, 13), (128, 64)])
def test_cepstrum_restatement_equals_scipy_dct(M, n_coef):
    from scipy.fft import dct
    x = np.random.default_rng(M + n_coef).normal(-4, 2, (M, 37))
    want = dct(x, type=2, norm='ortho', axis=0)[:n_coef]
    got = R.cepstrum(x, n_coef)
    err = float(np.abs(got - want).max())
    print(f'M = {M}, n_coef = {n_coef}: max |restatement - scipy| {err:.2e}')
    assert got.shape == (n_coef, 37) and err <= 1e-13


def _case(seed, ta=40, tb=50, C=13, M=8):
    rng = np.random.default_rng(seed)
    path = R.random_path(rng, ta, tb)
    ca, cb = rng.normal(0, 1, (C, ta)), rng.normal(0, 1, (C, tb))
    ma, mb = rng.normal(-4, 2, (M, ta)), rng.normal(-4, 2, (M, tb))
    fa, fb = rng.uniform(80, 400, ta), rng.uniform(80, 400, tb)
    return path, ca, cb, ma, mb, fa, fb


def test_stats_restatement_against_numpy():
    path, ca, cb, ma, mb, fa, fb = _case(0)
    fa[[3, 4, 20]] = np.nan
    fb[[0, 7]] = 0.0
    fb[9] = np.inf
    s = R.aligned_eval(ca, cb, path, ma, mb, fa, fb)
    i, j = path[:, 0], path[:, 1]
    assert s[0] == len(path) and len(path) >= 50
    d = ca[1:, i] - cb[1:, j]
    assert s[1] == pytest.approx(R.MCD_SCALE * np.mean(np.linalg.norm(d, axis=0)), rel=1e-14)
    assert s[2] == pytest.approx(np.mean(np.abs(ma[:, i] - mb[:, j])), rel=1e-14)
    va, vb = np.isfinite(fa[i]) & (np.nan_to_num(fa[i]) > 0), np.isfinite(fb[j]) & (np.nan_to_num(fb[j]) > 0)
    vv = va & vb
    assert s[3] == vv.sum() and 2 <= vv.sum() < len(path)
    x, y = fa[i][vv], fb[j][vv]
    assert s[4] == pytest.approx(np.sqrt(np.mean((1200 * np.log2(x / y)) ** 2)), rel=1e-14)
    assert s[5] == pytest.approx(np.sqrt(np.mean((x - y) ** 2)), rel=1e-14)
    assert abs(s[6] - np.corrcoef(x, y)[0, 1]) <= 1e-13
    assert s[7] == (va != vb).sum() / len(path) and s[7] > 0
    # first_coef and scale
    s0 = R.aligned_eval(ca, cb, path, first_coef=0, scale=1.0)
    assert s0[1] == pytest.approx(np.mean(np.linalg.norm(ca[:, i] - cb[:, j], axis=0)), rel=1e-14)
    assert np.isnan(s0[2:]).all()                                                  # no mels, no f0: NaN in 2 .. 7


def test_stats_restatement_tiny_cases():
    ca, cb = np.array([[9.0, 9.0, 9.0], [1.0, 2.0, 4.0]]), np.array([[0.0, 0.0], [1.0, 0.0]])
    # n = 0: n = 0, n_vv = 0 with f0 (NaN without), NaN elsewhere
    s = R.aligned_eval(ca, cb, np.zeros((0, 2)), f0_a=np.ones(3), f0_b=np.ones(2))
    assert s[0] == 0 and s[3] == 0 and np.isnan(s[[1, 2, 4, 5, 6, 7]]).all()
    assert np.isnan(R.aligned_eval(ca, cb, np.zeros((0, 2)))[1:]).all()
    path = np.array([[0, 0], [1, 0], [2, 1]])
    # distances over c >= 1: |1 - 1|, |2 - 1|, |4 - 0| -> mean 5 / 3; c0 (9 against 0) is left out
    assert R.aligned_eval(ca, cb, path, scale=1.0)[1] == pytest.approx(5.0 / 3.0, rel=1e-15)
    # n_vv = 0: both sides unvoiced on every step, or never together
    s = R.aligned_eval(ca, cb, path, f0_a=[np.nan, 0.0, 100.0], f0_b=[100.0, 0.0])
    assert s[3] == 0 and np.isnan(s[4:7]).all() and s[7] == pytest.approx(3.0 / 3.0)
    # n_vv = 1: the errors exist, the correlation does not
    s = R.aligned_eval(ca, cb, path, f0_a=[200.0, np.nan, 0.0], f0_b=[100.0, -5.0])
    assert s[3] == 1 and s[4] == pytest.approx(1200.0) and s[5] == pytest.approx(100.0) and np.isnan(s[6])
    assert s[7] == pytest.approx(1.0 / 3.0)                                        # step (1, 0): NaN against 100 Hz
    # n_vv = 2: two points correlate perfectly, one way or the other
    s = R.aligned_eval(ca, cb, path, f0_a=[100.0, np.nan, 200.0], f0_b=[100.0, 400.0])
    assert s[3] == 2 and s[6] == pytest.approx(1.0, abs=1e-15) and s[7] == pytest.approx(1.0 / 3.0)
    assert s[4] == pytest.approx(np.sqrt(0.5) * 1200.0) and s[5] == pytest.approx(np.sqrt(0.5 * 200.0 ** 2))
    s = R.aligned_eval(ca, cb, path, f0_a=[200.0, np.nan, 100.0], f0_b=[100.0, 400.0])
    assert s[6] == pytest.approx(-1.0, abs=1e-15)
    # a constant f0 on one side: a centred sum of squares is 0 -> NaN
    s = R.aligned_eval(ca, cb, path, f0_a=[100.0, 150.0, 200.0], f0_b=[120.0, 120.0])
    assert s[3] == 3 and np.isnan(s[6]) and np.isfinite(s[4:6]).all() and s[7] == 0.0


def test_random_path_is_a_dtw_path():
    rng = np.random.default_rng(5)
    for ta, tb in ((1, 1), (1, 9), (9, 1), (40, 50)):
        p = R.random_path(rng, ta, tb)
        step = np.diff(p, axis=0)
        assert tuple(p[0]) == (0, 0) and tuple(p[-1]) == (ta - 1, tb - 1)
        assert ((step >= 0) & (step <= 1)).all() and (step.sum(axis=1) >= 1).all()
    paths, lens = R.padded_paths([p, p[:0]], 40, 50)
    assert paths.shape == (2, 90, 2) and lens.tolist() == [len(p), 0] and not paths[1].any() and not paths[0, len(p):].any()


def test_utils_objective_surface():
    """the module imports without a GPU; names, argument names and defaults are the documented ones"""
    import torch
    from ttsamd import engine as E
    from ttsamd.lib import TtsAmdError
    from utils import objective as ob
    assert E.OBJECTIVE_KEYS == R.KEYS == ob.KEYS and len(R.KEYS) == 8
    assert E.MCD_SCALE == ob.MCD_SCALE == pytest.approx(10 * np.sqrt(2) / np.log(10), rel=1e-15) == pytest.approx(R.MCD_SCALE, rel=1e-15)

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}
    assert defaults(ob.mel_cepstrum) == dict(n_coef=13, lens=None)
    assert defaults(ob.mel_cepstral_distortion) == dict(n_coef=13, align='dtw', window=None, lens_pred=None, lens_ref=None)
    assert defaults(ob.f0_metrics) == dict(path=None, path_len=None, lens_pred=None, lens_ref=None)
    assert defaults(ob.objective_metrics) == dict(f0_pred=None, f0_ref=None, n_coef=13, align='dtw', window=None, lens_pred=None,
                                                  lens_ref=None)
    assert defaults(ob.evaluate_waves) == dict(n_coef=13, align='dtw', window=None, lens_pred=None, lens_ref=None)
    assert defaults(E.mel_cepstrum) == dict(lens=None, n_coef=13)
    assert defaults(E.dtw_aligned_eval) == dict(mel_a=None, mel_b=None, f0_a=None, f0_b=None, first_coef=1, scale=E.MCD_SCALE)
    assert defaults(E.objective_score) == dict(f0_pred=None, f0_ref=None, n_coef=13, align='dtw', window=None)
    from models.fastpitch.networks import FastPitch2Wave
    assert defaults(FastPitch2Wave.evaluate) == dict(teacher_forced=False, align='dtw', n_coef=13, window=None)
    if not torch.cuda.is_available():                                              # no device: every call raises, nothing falls back
        with pytest.raises(TtsAmdError):
            ob.mel_cepstrum(np.zeros((80, 4), np.float32))
        with pytest.raises(TtsAmdError):
            ob.f0_metrics(np.ones(4), np.ones(4))
        with pytest.raises(TtsAmdError):
            E.ObjectiveEngine()
