"""GPU: objective evaluation (csrc/objective.hip) through the C ABI, ttsamd.engine, utils.objective and FastPitch2Wave.evaluate.  The
reference has no such module: the yardstick is the float64 restatement tests/objective_ref.py (pinned to scipy and numpy by
tests/test_objective_cpu.py), and every bound below is derived from the arithmetic, not from what the kernels give.

  cepstrum   |got - want| <= 2^-23 |want| + 1e-12 sum_m |x_m|: one rounding to fp32 (doubled for double rounding), plus a float64
             accumulation of <= 128 products over a basis good to a few ulps, (M + 4) 2^-53 s_k sum|x| ~ 1.5e-14 sum|x|, with ~70 x left
             for the summation order and the device's cosine.  An fp32 accumulation (M 2^-24 |x|) or one wrong basis entry misses it by
             orders of magnitude.
  stats      1e-11 relative (f0_corr: 1e-11 absolute): (n_coef + n + 16) 2^-53 < 1e-12 for n <= 8192, relative to sums of non-negative
             terms (to sqrt(Sxx Syy) for the cross sum, by Cauchy-Schwarz), x 10 for the device's sqrt / log2 and the reduction order.
             Counts are exact and NaN sits exactly where the definition puts it."""
import json
import os

import numpy as np
import pytest
import torch

import melspec_ref as MR
import objective_ref as R
import oversmoothing_ref as OR
import pyin_ref as PR

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(DEV)


def _bits(t):
    """float tensor -> its bit patterns (NaN == NaN)"""
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


# ---------------------------------------------------------------------------------------------------------------------- cepstrum ----
@pytest.mark.parametrize('M,n_coef', [(1, 1), (80, 13), (80, 80), (100, 13), (128, 64)])
def test_cepstrum_against_float64(M, n_coef):
    from ttsamd import engine as E
    if n_coef > E.MEL_CEPSTRUM_MAX_COEF:                                             # (80, 80): beyond the 64 coefficients that are built
        with pytest.raises(E.L.TtsAmdError, match='n_coef'):
            E.mel_cepstrum(torch.zeros(1, M, 2, device=DEV), None, n_coef)
        n_coef = E.MEL_CEPSTRUM_MAX_COEF
    for T in (1, 2, 257):
        x = np.random.default_rng(1000 * M + T).normal(-4, 2, (2, M, T)).astype(np.float32)
        got = E.mel_cepstrum(_dev(x), None, n_coef).cpu().numpy().astype(np.float64)
        assert got.shape == (2, n_coef, T)
        for b in range(2):
            want = R.cepstrum(x[b], n_coef)
            bound = 2.0 ** -23 * np.abs(want) + 1e-12 * np.abs(x[b].astype(np.float64)).sum(axis=0)[None]
            err = np.abs(got[b] - want)
            print(f'M = {M}, n_coef = {n_coef}, T = {T}: max err / bound {float((err / bound).max()):.3f}, max err {float(err.max()):.2e}')
            assert (err <= bound).all(), (M, n_coef, T, float((err / bound).max()))


@pytest.mark.parametrize('M,n_coef', [(80, 13), (128, 64)])
def test_cepstrum_ragged_batch(M, n_coef):
    from ttsamd import engine as E
    T = 257
    lens = [T, T - 1, 1, 0]
    x = np.random.default_rng(M).normal(-4, 2, (4, M, T)).astype(np.float32)
    for b, n in enumerate(lens):
        x[b, :, n:] = np.nan                                                        # poison: nothing past a row's end is read into a result
    xd, ld = _dev(x), torch.tensor(lens, dtype=torch.int64, device=DEV)
    got = E.mel_cepstrum(xd, ld, n_coef)
    assert got.shape == (4, n_coef, T)
    for b, n in enumerate(lens):
        assert not got[b, :, n:].any() and bool(torch.isfinite(got[b]).all())       # zero past the end
        alone = E.mel_cepstrum(xd[b:b + 1], ld[b:b + 1], n_coef)
        assert np.array_equal(_bits(alone[0]), _bits(got[b])), b
        if n:
            trimmed = E.mel_cepstrum(xd[b:b + 1, :, :n].contiguous(), None, n_coef)
            assert np.array_equal(_bits(trimmed[0]), _bits(got[b, :, :n])), b
            want = R.cepstrum(x[b, :, :n], n_coef)
            assert np.abs(got[b, :, :n].cpu().numpy() - want).max() <= 2.0 ** -22 * np.abs(want).max() + 1e-9


# ------------------------------------------------------------------------------------------------------- evaluation along a path ----
def _pair(seed, ta, tb, C=13, M=80, n=None):
    """one pair of random features with a random monotone path: dict of numpy arrays (fp32, as the kernel takes them)"""
    rng = np.random.default_rng(seed)
    f0 = [np.where(rng.random(t) < 0.25, 0.0, rng.uniform(80, 400, t)).astype(np.float32) for t in (ta, tb)]
    return dict(path=R.random_path(rng, ta, tb, n), cep_a=rng.normal(0, 1, (C, ta)).astype(np.float32),
                cep_b=rng.normal(0, 1, (C, tb)).astype(np.float32), mel_a=rng.normal(-4, 2, (M, ta)).astype(np.float32),
                mel_b=rng.normal(-4, 2, (M, tb)).astype(np.float32), f0_a=f0[0], f0_b=f0[1])


def _run(pairs, mels=True, f0=True, ta_max=None, tb_max=None, **kw):
    """pairs -> stats float64 [B, 8] (a device tensor) of one ttsamd_dtw_aligned_eval call on the zero-padded batch"""
    from ttsamd import engine as E
    ta_max = ta_max or max(p['cep_a'].shape[1] for p in pairs)
    tb_max = tb_max or max(p['cep_b'].shape[1] for p in pairs)

    def stack(key, width):
        out = np.zeros((len(pairs),) + pairs[0][key].shape[:-1] + (width,), np.float32)
        for b, p in enumerate(pairs):
            out[b, ..., :p[key].shape[-1]] = p[key]
        return _dev(out)
    path, plen = R.padded_paths([p['path'] for p in pairs], ta_max, tb_max)
    return E.dtw_aligned_eval(stack('cep_a', ta_max), stack('cep_b', tb_max), _dev(path), _dev(plen),
                              stack('mel_a', ta_max) if mels else None, stack('mel_b', tb_max) if mels else None,
                              stack('f0_a', ta_max) if f0 else None, stack('f0_b', tb_max) if f0 else None, **kw)


def _check(got, p, mels=True, f0=True, **kw):
    want = R.aligned_eval(p['cep_a'], p['cep_b'], p['path'], p['mel_a'] if mels else None, p['mel_b'] if mels else None,
                          p['f0_a'] if f0 else None, p['f0_b'] if f0 else None, **kw)
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (8,)
    print('got ', got.tolist(), '\nwant', want.tolist())
    assert np.array_equal(np.isnan(got), np.isnan(want)), (got, want)                # NaN exactly where specified
    assert got[0] == want[0] and (np.isnan(want[3]) or got[3] == want[3])            # counts are exact
    for k in (1, 2, 4, 5, 7):
        if not np.isnan(want[k]):
            assert abs(got[k] - want[k]) <= 1e-11 * abs(want[k]), (R.KEYS[k], got[k], want[k])
    if not np.isnan(want[6]):
        assert abs(got[6] - want[6]) <= 1e-11, (got[6], want[6])
    return want


@pytest.mark.parametrize('n', [0, 1, 257])
def test_aligned_eval_against_the_restatement(n):
    p = _pair(10 + n, 200, 180, n=n)
    want = _check(_run([p])[0], p)
    assert want[0] == n and (n < 257 or (want[3] >= 2 and not np.isnan(want).any()))


def test_aligned_eval_long_pair_multi_pass():
    p = _pair(3, 4096, 4096)
    assert len(p['path']) > 4096
    want = _check(_run([p])[0], p)
    assert not np.isnan(want).any()


def test_aligned_eval_voicing_cases():
    from ttsamd import engine as E
    base = _pair(21, 60, 70)
    i, j = base['path'][:, 0], base['path'][:, 1]

    def with_f0(fa, fb):
        return dict(base, f0_a=np.asarray(fa, np.float32), f0_b=np.asarray(fb, np.float32))
    # n_vv = 0: one side silent; NaN and 0 (and a negative value, and inf) all count as unvoiced
    silent = np.zeros(70, np.float32)
    silent[::3], silent[1::3] = np.nan, -1.0
    silent[5] = np.inf
    w = _check(_run([with_f0(base['f0_a'], silent)])[0], with_f0(base['f0_a'], silent))
    assert w[3] == 0 and np.isnan(w[4:7]).all() and 0 < w[7] < 1
    # n_vv = 1 and 2: voiced together on the first one / two of five steps; step (4, 3) differs in voicing
    short = np.array([[0, 0], [1, 1], [2, 2], [3, 2], [4, 3]], np.int32)
    for nvv in (1, 2):
        fa, fb = np.full(60, np.nan, np.float32), np.zeros(70, np.float32)
        fa[:nvv], fb[:nvv], fb[3] = (200.0, 230.0)[:nvv], (180.0, 260.0)[:nvv], 150.0
        p = dict(with_f0(fa, fb), path=short)
        w = _check(_run([p])[0], p)
        assert w[0] == 5 and w[3] == nvv and np.isnan(w[6]) == (nvv < 2) and np.isfinite(w[4:6]).all() and w[7] == 0.2
    # a constant f0 on one side (200 Hz: its sums are exact, so the centred sum of squares is exactly 0): f0_corr is NaN
    fb = np.full(70, 200.0, np.float32)
    w = _check(_run([with_f0(np.abs(base['f0_a']) + 90.0, fb)])[0], with_f0(np.abs(base['f0_a']) + 90.0, fb))
    assert w[3] == len(i) and np.isnan(w[6]) and np.isfinite(w[4:6]).all() and w[7] == 0
    # mels NULL / f0 NULL / both; first_coef and scale
    _check(_run([base], mels=False)[0], base, mels=False)
    _check(_run([base], f0=False)[0], base, f0=False)
    w = _check(_run([base], mels=False, f0=False, first_coef=0, scale=1.0)[0], base, mels=False, f0=False, first_coef=0, scale=1.0)
    assert np.isnan(w[2:]).all()
    with pytest.raises(E.L.TtsAmdError, match='first_coef'):
        _run([base], first_coef=13)


def test_aligned_eval_ragged_batch_rows_equal_the_call_alone():
    shapes = [(200, 180, None), (64, 257, None), (1, 1, None), (90, 40, 0), (130, 129, 77)]     # (90, 40): an empty path
    pairs = [_pair(40 + b, ta, tb, n=n) for b, (ta, tb, n) in enumerate(shapes)]
    got = _run(pairs)
    assert got.shape == (5, 8) and got[3, 0] == 0 and got[3, 3] == 0 and bool(torch.isnan(got[3, [1, 2, 4, 5, 6, 7]]).all())
    for b, p in enumerate(pairs):
        _check(got[b], p)
        same = _run([p], ta_max=200, tb_max=257)                                     # alone at the batch's padded size
        assert np.array_equal(_bits(same[0]), _bits(got[b])), b
        trimmed = _run([p])                                                          # alone at its own size
        assert np.array_equal(_bits(trimmed[0]), _bits(got[b])), b


# ----------------------------------------------------------------------------------------------------------------- known answers ----
def test_known_answer_identical_pair():
    from ttsamd import engine as E
    a, _ = OR.warped_pair(7, 80, 120, 150)
    rng = np.random.default_rng(8)
    f0 = np.where(rng.random(120) < 0.3, 0.0, rng.uniform(80, 400, 120)).astype(np.float32)
    mel, f = _dev(a[None]), _dev(f0[None])
    out = E.objective_score(mel, None, mel, None, f, f, align='dtw')
    assert int(out['path_len'][0]) == 120 and float(out['dtw_cost'][0]) == 0.0
    assert np.array_equal(out['path'][0, :120].cpu().numpy(), np.repeat(np.arange(120)[:, None], 2, axis=1))
    for k in ('mcd', 'mel_mae', 'f0_rmse_cents', 'f0_rmse_hz', 'vuv_error'):
        assert float(out[k][0]) == 0.0, k
    assert float(out['n'][0]) == 120 and float(out['n_vv'][0]) == float((f0 > 0).sum())
    assert abs(float(out['f0_corr'][0]) - 1.0) <= 1e-12


def test_known_answer_level_shift():
    """x on the grid of 2^-10 in [-8, 0] and x + 2 are both exact in fp32: the mel error is 2 and only c0 differs beyond one rounding of
    each cepstrum (the DCT of a constant is zero for k >= 1)."""
    from ttsamd import engine as E
    n_coef = 13
    x = (np.random.default_rng(9).integers(-8192, 1, (1, 80, 100)) / 1024.0).astype(np.float32)
    y = x + np.float32(2.0)
    assert np.array_equal(y.astype(np.float64), x.astype(np.float64) + 2.0)
    out = E.objective_score(_dev(x), None, _dev(y), None, n_coef=n_coef, align='frames')
    assert float(out['n'][0]) == 100 and 'dtw_cost' not in out
    assert abs(float(out['mel_mae'][0]) - 2.0) <= 1e-12
    cmax = max(float(np.abs(R.cepstrum(v[0], n_coef)).max()) for v in (x, y))
    mcd = float(out['mcd'][0])
    print(f'mcd of a level shift {mcd:.3e}, bound {R.MCD_SCALE * np.sqrt(n_coef - 1) * 2.0 ** -23 * cmax:.3e}')
    assert 0.0 <= mcd <= R.MCD_SCALE * np.sqrt(n_coef - 1) * 2.0 ** -23 * cmax
    c0 = E.mel_cepstrum(_dev(y), None, n_coef)[0, 0] - E.mel_cepstrum(_dev(x), None, n_coef)[0, 0]
    assert np.abs(c0.cpu().numpy() - 2.0 * np.sqrt(80.0)).max() <= 1e-5              # the level went to c0: 2 sqrt(M)


# ------------------------------------------------------------------------------------------------------------- the composed call ----
@pytest.fixture(scope='module')
def ragged_mels():
    a0, b0 = OR.warped_pair(31, 80, 120, 150)
    a1, b1 = OR.warped_pair(32, 80, 70, 60)
    pred, ref = np.zeros((2, 80, 120), np.float32), np.zeros((2, 80, 150), np.float32)
    pred[0], ref[0], pred[1, :, :70], ref[1, :, :60] = a0, b0, a1, b1
    rng = np.random.default_rng(33)
    fp, fr = (np.where(rng.random((2, t)) < 0.3, 0.0, rng.uniform(80, 400, (2, t))).astype(np.float32) for t in (120, 150))
    lp, lr = torch.tensor([120, 70], device=DEV), torch.tensor([150, 60], device=DEV)
    return _dev(pred), lp, _dev(ref), lr, _dev(fp), _dev(fr)


def test_objective_score_equals_its_pieces(ragged_mels):
    from ttsamd import engine as E
    pred, lp, ref, lr, fp, fr = ragged_mels
    for window in (None, 40):
        out = E.objective_score(pred, lp, ref, lr, fp, fr, window=window)
        cp, cr = E.mel_cepstrum(pred, lp, 13), E.mel_cepstrum(ref, lr, 13)
        cost, path, plen = E.dtw(cp[:, 1:], cr[:, 1:], lp, lr, 'l2', window)
        stats = E.dtw_aligned_eval(cp, cr, path, plen, pred, ref, fp, fr)
        assert torch.equal(out['path'], path) and torch.equal(out['path_len'], plen) and np.array_equal(_bits(out['dtw_cost']), _bits(cost))
        for k, name in enumerate(E.OBJECTIVE_KEYS):
            assert np.array_equal(_bits(out[name]), _bits(stats[:, k])), name
        for b, (ta, tb) in enumerate(((120, 150), (70, 60))):                        # DTW is bit-exact: the path of the restatement
            wcost, wpath = OR.dtw_fp32(cp[b, 1:, :ta].cpu().numpy().T, cr[b, 1:, :tb].cpu().numpy().T, 0, -1 if window is None else window)
            n = int(plen[b])
            assert n == len(wpath) and np.array_equal(path[b, :n].cpu().numpy(), wpath.astype(np.int32))
            assert np.float32(wcost).view(np.uint32) == cost[b].cpu().numpy().view(np.uint32)
            if window is not None:
                assert np.abs(wpath[:, 0] - wpath[:, 1]).max() <= window
    frames = E.objective_score(pred, lp, ref, lr, fp, fr, align='frames')
    assert frames['n'].tolist() == [120.0, 60.0] and frames['path_len'].tolist() == [120, 60] and 'dtw_cost' not in frames
    ipath, ilen = E.identity_path(lp, lr, 120, 150)
    assert torch.equal(frames['path'], ipath) and ipath.shape == (2, 270, 2) and not ipath[1, 60:].any()
    assert np.array_equal(ipath[0, :120].cpu().numpy(), np.repeat(np.arange(120)[:, None], 2, axis=1))
    want = R.aligned_eval(R.cepstrum(pred[1, :, :70].cpu().numpy(), 13).astype(np.float32), R.cepstrum(ref[1, :, :60].cpu().numpy(), 13).astype(np.float32),
                          ipath[1, :60].cpu().numpy(), pred[1].cpu().numpy(), ref[1].cpu().numpy(), fp[1].cpu().numpy(), fr[1].cpu().numpy())
    assert abs(float(frames['mel_mae'][1]) - want[2]) <= 1e-11 * want[2] and float(frames['n_vv'][1]) == want[3]
    assert abs(float(frames['mcd'][1]) - want[1]) <= 1e-5 * want[1]                  # (the restated cepstra are rounded on the host here)


def test_argument_errors_name_what_is_built(ragged_mels):
    from ttsamd import engine as E
    from ttsamd.lib import TtsAmdError
    pred, lp, ref, lr, fp, fr = ragged_mels
    with pytest.raises(TtsAmdError, match='dimensions'):
        E.objective_score(pred[0], None, ref[0], None)                              # wrong rank
    with pytest.raises(TtsAmdError, match='batch or band count'):
        E.objective_score(pred[:1], None, ref, None)
    with pytest.raises(TtsAmdError, match='batch or band count'):
        E.objective_score(pred[:, :64].contiguous(), None, ref, None)
    for n_coef in (0, 65, 81):
        with pytest.raises(TtsAmdError, match='n_coef'):
            E.objective_score(pred, lp, ref, lr, n_coef=n_coef)
    with pytest.raises(TtsAmdError, match='n_coef'):
        E.mel_cepstrum(pred[:, :8].contiguous(), None, 9)
    with pytest.raises(TtsAmdError, match="'dtw' | 'frames'".replace('|', r'\|')):
        E.objective_score(pred, lp, ref, lr, align='linear')
    with pytest.raises(TtsAmdError, match='at most 4096'):
        E.objective_score(torch.zeros(1, 80, E.OVERSMOOTH_MAX_FRAMES + 1, device=DEV), None, ref[:1], None)
    with pytest.raises(TtsAmdError, match='ROCm device'):
        E.mel_cepstrum(torch.zeros(1, 80, 4), None)
    with pytest.raises(TtsAmdError, match='pair'):
        E.objective_score(pred, lp, ref, lr, f0_pred=fp)
    lib = E.L.load()                                                                # the C entries refuse the same, nothing is launched
    z = torch.zeros(1, 129, 4, device=DEV)
    ln = torch.tensor([4], dtype=torch.int64, device=DEV)
    assert lib.ttsamd_mel_cepstrum(E._ptr(z), E._ptr(ln), 1, 129, 4, 13, E._ptr(z), E._stream()) == -1
    assert lib.ttsamd_mel_cepstrum(E._ptr(z), E._ptr(ln), 1, 80, 4, 65, E._ptr(z), E._stream()) == -1
    assert lib.ttsamd_mel_cepstrum(E._ptr(z), E._ptr(ln), 1, 12, 4, 13, E._ptr(z), E._stream()) == -1


# ------------------------------------------------------------------------------------------------------------------ wave to score ----
def test_score_waves_without_a_host_sync():
    from ttsamd import engine as E
    from utils.pitch import note_to_hz
    n = np.array([[40 * 256, 45 * 256], [33 * 256 + 100, 30 * 256]])                 # [row][pred, ref]; row 0: two tones 100 cents apart
    wp, wr = np.zeros((2, n[:, 0].max()), np.float32), np.zeros((2, n[:, 1].max()), np.float32)
    wp[0], wr[0] = PR.harmonic_tone(220.0, n[0, 0]), PR.harmonic_tone(220.0 * 2.0 ** (100.0 / 1200.0), n[0, 1])
    wp[1, :n[1, 0]], wr[1, :n[1, 1]] = MR.voiced(int(n[1, 0]), 5), MR.voiced(int(n[1, 1]), 6)
    wp_d, wr_d, np_d, nr_d = _dev(wp), _dev(wr), _dev(n[:, 0]), _dev(n[:, 1])
    obj = E.ObjectiveEngine()
    ms = E.MelSpecEngine(MR.fbank('audio'), 'same', 'eps', 1e-5)
    py = E.PyinEngine(note_to_hz('C2'), note_to_hz('C7'), sr=22050, frame_length=1024, hop_length=256)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        out = obj.score_waves(wp_d, np_d, wr_d, nr_d)
        parts = []
        for w, ns in ((wp_d, np_d), (wr_d, nr_d)):
            mel, frames = ms.forward(w, ns)
            f0 = py.forward(w, ns)[0]
            parts += [mel, frames, torch.nn.functional.pad(f0, (0, mel.shape[2] - f0.shape[1]))]
        want = E.objective_score(parts[0], parts[1], parts[3], parts[4], parts[2], parts[5])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert out['lens_pred'].tolist() == [40, 33] and out['lens_ref'].tolist() == [45, 30]
    assert torch.equal(out['path'], want['path']) and torch.equal(out['path_len'], want['path_len'])
    for k in E.OBJECTIVE_KEYS + ('dtw_cost',):
        assert np.array_equal(_bits(out[k]), _bits(want[k])), k
    row = {k: float(out[k][0]) for k in E.OBJECTIVE_KEYS}
    print('tone pair:', row)
    assert row['n_vv'] >= row['n'] / 2 and row['n'] >= 45                            # a condition on the inputs: both tones are voiced
    assert 80.0 <= row['f0_rmse_cents'] <= 120.0                                     # 100 cents, each tone within pYIN's 10-cent bound
    assert all(np.isfinite(float(out[k][1])) for k in ('mcd', 'mel_mae')) and float(out['n'][1]) >= 33


# ------------------------------------------------------------------------------------------------------------------ the drop-ins ----
def test_utils_objective_dropins(ragged_mels):
    from ttsamd import engine as E
    from utils import objective as ob
    pred, lp, ref, lr, fp, fr = ragged_mels
    a, b = pred[1, :, :70].cpu().numpy(), ref[1, :, :60].cpu().numpy()
    fa, fb = fp[1, :70].cpu().numpy().astype(np.float64), fr[1, :60].cpu().numpy().astype(np.float64)
    fa[fa == 0] = np.nan                                                            # pyin's NaN fill: unvoiced as well
    batch = E.objective_score(pred, lp, ref, lr, fp, fr)
    one = ob.objective_metrics(a, b, fa, fb)                                         # numpy in, floats out; a single pair == its batch row
    assert list(one) == list(E.OBJECTIVE_KEYS) and all(isinstance(v, float) for v in one.values())
    for k in E.OBJECTIVE_KEYS:
        assert np.float64(one[k]).view(np.int64) == _bits(batch[k])[1], k
    assert ob.mel_cepstral_distortion(a, b) == one['mcd']
    assert ob.mel_cepstral_distortion(a, b, align='frames') == float(E.objective_score(pred, lp, ref, lr, align='frames')['mcd'][1])
    cep = ob.mel_cepstrum(a)
    assert isinstance(cep, np.ndarray) and cep.dtype == np.float32 and cep.shape == (13, 70)
    assert np.array_equal(cep, E.mel_cepstrum(pred, lp, 13)[1, :, :70].cpu().numpy())
    # f0_metrics: frame by frame, and along a path of one's own
    f = ob.f0_metrics(fa, fb)
    ident = np.repeat(np.arange(60)[:, None], 2, axis=1)
    want = R.aligned_eval(np.zeros((1, 70)), np.zeros((1, 60)), ident, f0_a=fa.astype(np.float32), f0_b=fb.astype(np.float32), first_coef=0)
    assert list(f) == ['n', 'n_vv', 'f0_rmse_cents', 'f0_rmse_hz', 'f0_corr', 'vuv_error'] and f['n'] == 60 and f['n_vv'] == want[3]
    for k in ('f0_rmse_cents', 'f0_rmse_hz', 'vuv_error'):
        assert abs(f[k] - want[R.KEYS.index(k)]) <= 1e-11 * abs(want[R.KEYS.index(k)]), k
    assert abs(f['f0_corr'] - want[6]) <= 1e-11
    path = batch['path'][1, :int(batch['path_len'][1])].cpu().numpy()
    along = ob.f0_metrics(fa, fb, path=path)
    for k in along:
        assert np.float64(along[k]).view(np.int64) == np.float64(one[k]).view(np.int64), k
    # tensors on the device stay there; a batch carries its leading dimension
    dev = ob.objective_metrics(pred, ref, fp, fr, lens_pred=lp, lens_ref=lr)
    assert all(v.device.type == 'cuda' and v.shape == (2,) for v in dev.values())
    for k in E.OBJECTIVE_KEYS:
        assert np.array_equal(_bits(dev[k]), _bits(batch[k])), k


@pytest.fixture(scope='module')
def tts_model(synth_weights, golden, tmp_path_factory):
    import text
    from conftest import GOLDEN
    from models.fastpitch import FastPitch2Wave
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
    d = tmp_path_factory.mktemp('objective')
    sd = dict(synth_weights['fastpitch'])
    sd.update(synth.fastpitch_aligner_state_dict(gain=float(golden('aligner')['gain'])))
    torch.save({'model': {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, 'config': dict(NET_CONFIG), 'symbols': list(text.symbols)},
               d / 'fp.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, d / 'hg.pth')
    with open(d / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        lines = json.load(f)[:3]
    model = FastPitch2Wave(str(d / 'fp.pth'), vocoder_sd=str(d / 'hg.pth'), vocoder_config=str(d / 'config.json')).to(DEV)
    recordings = model.tts(lines, speed=0.9, denoise=0, batch_size=3)               # 'recordings': the same lines, spoken more slowly
    return model, lines, recordings


def _same_floats(rows, score, keys):
    for b, row in enumerate(rows):
        assert all(isinstance(v, float) for v in row.values())
        for k in keys:
            assert np.float64(row[k]).view(np.int64) == _bits(score[k])[b], (b, k)


def test_fastpitch2wave_evaluate(tts_model):
    import text
    from ttsamd import engine as E
    from utils import objective as ob
    model, lines, recordings = tts_model
    obj = E.ObjectiveEngine()
    rec, n_rec = model._pad_waves(recordings, DEV)
    # default: tts, then score_waves
    rows = model.evaluate(lines, recordings, denoise=0, batch_size=3)
    wave, n = model._pad_waves(model.tts(lines, denoise=0, batch_size=3), DEV)
    want = obj.score_waves(wave, n, rec, n_rec)
    assert len(rows) == 3 and list(rows[0]) == list(E.OBJECTIVE_KEYS) + ['frames_pred', 'frames_ref']
    _same_floats(rows, want, E.OBJECTIVE_KEYS)
    assert all(np.isfinite(r['mcd']) and np.isfinite(r['mel_mae']) and r['mcd'] > 0 for r in rows)
    assert [r['frames_ref'] for r in rows] == [float(len(w) // 256) for w in recordings]
    assert all(r['frames_pred'] < r['frames_ref'] for r in rows)                     # the recordings were spoken at speed 0.9
    frames = model.evaluate(lines, recordings, align='frames', denoise=0, batch_size=3)
    assert [r['n'] for r in frames] == [min(r['frames_pred'], r['frames_ref']) for r in rows]
    # the drop-in on the same waves: numpy in, floats out
    one = ob.evaluate_waves(wave[0, :int(n[0])].cpu().numpy(), recordings[0].numpy())
    assert all(abs(one[k] - rows[0][k]) <= 1e-9 * abs(rows[0][k]) for k in ('mcd', 'mel_mae')) and one['n'] == rows[0]['n']
    # teacher forced: the recording's durations, pitch and energy through align -> infer -> vocoder
    tf = model.evaluate(lines, recordings, teacher_forced=True, denoise=0)
    m = model.model
    ids_rows = [text.tokens_to_ids(m._tokenize(line), m.phon_to_id) for line in lines]
    ids = torch.zeros(3, max(len(r) for r in ids_rows), dtype=torch.int64)
    for b, r in enumerate(ids_rows):
        ids[b, :len(r)] = torch.as_tensor(r)
    mel_rec, fr = obj.melspec.forward(rec, n_rec)
    tgt = m.align(ids, mel_rec, fr, pitch=m.pitch_track(rec, n_rec, mel_len=mel_rec.shape[2]), energy=torch.linalg.vector_norm(mel_rec, dim=1))
    mel, dec_lens, *_ = m.infer(ids, dur_tgt=tgt.dur_tgt, pitch_tgt=tgt.pitch_tgt, energy_tgt=tgt.energy_tgt)
    assert torch.equal(dec_lens.cpu(), fr.cpu())                                     # the prediction has the recording's length
    want = obj.score_waves(model.vocoder.engine().forward(mel, dec_lens), dec_lens * 256, rec, n_rec)
    _same_floats(tf, want, E.OBJECTIVE_KEYS)
    assert all(r['frames_pred'] == r['frames_ref'] and np.isfinite(r['mcd']) and np.isfinite(r['mel_mae']) for r in tf)
    one_line = model.evaluate(lines[0], recordings[0], denoise=0)
    assert len(one_line) == 1 and np.isfinite(one_line[0]['mcd'])
    with pytest.raises(E.L.TtsAmdError, match='3 lines against 2 recordings'):
        model.evaluate(lines, recordings[:2])
    with pytest.raises(E.L.TtsAmdError, match='speed'):
        model.evaluate(lines, recordings, teacher_forced=True, speed=1.2)
    with pytest.raises(E.L.TtsAmdError, match="'dtw' | 'frames'".replace('|', r'\|')):
        model.evaluate(lines, recordings, align='nearest', denoise=0, batch_size=3)
