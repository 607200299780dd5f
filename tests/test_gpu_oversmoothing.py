"""GPU: the oversmoothing kernels (csrc/oversmooth.hip) through the C ABI.  DTW is compared bit for bit with the fp32 restatement of the
reference (tests/oversmoothing_ref.py, which tests/test_oversmoothing_cpu.py pins to the reference's goldens), the series with float64
under the rule tests/test_gpu_melspec.py uses (at most 4x the error of the reference's own fp32 arithmetic, measured in the same run), the
summary with numpy, and the drop-in modules with the reference's goldens inside its own recorded noise floor."""
import numpy as np
import pytest
import torch

import oversmoothing_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP = 2.0 ** -23


def _dtw(a, b, metric=0, window=-1, **kw):
    """a [M, Ta], b [M, Tb] numpy -> (cost float32, path int32 [L, 2]) through ttsamd_dtw"""
    from ttsamd import engine as E
    cost, path, plen = E.dtw(torch.from_numpy(np.ascontiguousarray(a))[None].to(DEV), torch.from_numpy(np.ascontiguousarray(b))[None].to(DEV),
                             metric=('l2', 'cosine')[metric], window=None if window < 0 else window, **kw)
    L = int(plen[0])
    assert not path[0, L:].any()
    return cost.cpu().numpy()[0], path[0, :L].cpu().numpy()


def _same(got, want, what):
    assert got[1].shape == want[1].shape and np.array_equal(got[1], want[1]), (what, got[1].shape, want[1].shape)
    assert np.float32(got[0]).view(np.uint32) == np.float32(want[0]).view(np.uint32), (what, got[0], want[0])


def _feats(seed, M, ta, tb):
    if M == 1:
        rng = np.random.default_rng(seed)
        a = np.cumsum(rng.normal(0, 1, ta)).astype(np.float32)[None]
        idx = np.round(np.linspace(0, ta - 1, tb)).astype(int)
        return a, (a[:, idx] + 0.1 * rng.normal(0, 1, (1, tb))).astype(np.float32)
    return R.warped_pair(seed, M, ta, tb)


@pytest.mark.parametrize('M', [1, 80, 100])
def test_dtw_is_the_restatement_bit_for_bit(M):
    """Path, path_len and the cost's bits: both metrics, no band / radius 20 / a band narrower than |Ta - Tb| (as far as the lengths allow
    one), from one frame per side to the bench's utterances."""
    for ta, tb in ((1, 1), (1, 7), (7, 1), (64, 65), (449, 430)):
        a, b = _feats(100 + ta, M, ta, tb)
        for metric in (0, 1):
            for window in (-1, 20, max(abs(ta - tb) - 1, 0)):
                _same(_dtw(a, b, metric, window), R.dtw_fp32(a.T, b.T, metric, window), (M, ta, tb, metric, window))
    a, b = _feats(5, M, 449, 430)
    got = _dtw(a, b, 0, 18)                                        # |Ta - Tb| = 19: the end cell lies outside the band
    assert len(got[1]) == 0 and got[0] == np.float32(1e30)


def test_dtw_long_series_and_wide_mel():
    """2 291 x 2 100 at M = 1 (config 1's longest line) and a 1 000 x 900 alignment of 80-band mels."""
    a, b = _feats(7, 1, 2291, 2100)
    for metric, window in ((0, -1), (1, -1), (0, 200), (0, 20)):
        _same(_dtw(a, b, metric, window), R.dtw_fp32(a.T, b.T, metric, window), (2291, 2100, metric, window))
    a, b = R.warped_pair(8, 80, 1000, 900)
    for metric in (0, 1):
        _same(_dtw(a, b, metric), R.dtw_fp32(a.T, b.T, metric), (1000, 900, 80, metric))
    a, b = _feats(9, 1, 4096, 4001)                                # the largest supported side
    _same(_dtw(a, b), R.dtw_fp32(a.T, b.T), (4096, 4001))


def test_dtw_tie_order_on_plateaus():
    """Integer-valued series with long exact plateaus (as CRoll95 is): equal costs everywhere, the order up, left, diag with strict <
    decides the path."""
    for seed, ta, tb in ((1, 449, 430), (2, 200, 333), (3, 64, 64)):
        a, b = R.plateau_series(seed, ta)[None], R.plateau_series(seed + 50, tb)[None]
        for metric in (0, 1):
            _same(_dtw(a, b, metric), R.dtw_fp32(a.T, b.T, metric), (seed, metric))
    z = np.zeros((1, 90), np.float32)                              # all ties
    _same(_dtw(z, z[:, :70]), R.dtw_fp32(z.T, z[:, :70].T), 'zeros')


def test_dtw_ragged_batch_rows_equal_the_call_alone():
    """32 rows of ragged lengths, one of them empty, NaN poison past each row's end: two runs are bit-identical, and every row equals both
    the call on it alone and the restatement."""
    from ttsamd import engine as E
    rng = np.random.default_rng(3)
    B, ta_max, tb_max = 32, 300, 280
    la, lb = rng.integers(5, ta_max + 1, B), rng.integers(5, tb_max + 1, B)
    la[0], lb[0], la[5], la[9], lb[9] = ta_max, tb_max, 0, 0, 0
    A, Bm = np.full((B, 1, ta_max), np.nan, np.float32), np.full((B, 1, tb_max), np.nan, np.float32)
    rows = []
    for r in range(B):
        a, b = _feats(200 + r, 1, max(la[r], 1), max(lb[r], 1))
        A[r, :, :la[r]], Bm[r, :, :lb[r]] = a[:, :la[r]], b[:, :lb[r]]
        rows.append((a[:, :la[r]], b[:, :lb[r]]))
    args = (torch.from_numpy(A).to(DEV), torch.from_numpy(Bm).to(DEV), torch.from_numpy(la).to(DEV), torch.from_numpy(lb).to(DEV))
    runs = [tuple(t.cpu().numpy().copy() for t in E.dtw(*args)) for _ in range(2)]
    for x, y in zip(*runs):
        assert np.array_equal(x.view(np.uint32 if x.dtype == np.float32 else x.dtype), y.view(np.uint32 if y.dtype == np.float32 else y.dtype))
    cost, path, plen = runs[0]
    for r, (a, b) in enumerate(rows):
        want = R.dtw_fp32(a.T, b.T)
        _same((cost[r], path[r, :plen[r]]), want, ('row', r))
        assert not path[r, plen[r]:].any()
        if la[r] and lb[r]:
            _same(_dtw(a, b), want, ('alone', r))
    assert plen[5] == 0 and cost[5] == np.float32(1e30) and plen[9] == 0 and cost[9] == 0


SERIES_CASES = [(39, 80, True, True, None), (39, 80, False, False, None), (39, 80, True, False, 7), (39, 80, False, True, None),
                (30, 100, True, True, None), (30, 100, False, False, 12), (30, 100, True, False, None)]


def test_series_against_float64():
    """Per series the max-abs error relative to the largest value is at most 4x the largest such error of the reference's own fp32
    arithmetic (numpy on the CPU) over this module's cases, measured here and printed; CRoll95 is exact on every frame that is no
    near-tie (at most 2 % of a case's frames).  80 and 100 bands, center / hann on and off, an explicit q_c."""
    from ttsamd import engine as E
    ref_err, got_err = np.zeros(3), np.zeros(3)
    for seed, n_mels, center, hann, q_c in SERIES_CASES:
        a, _ = R.warped_pair(seed, n_mels, 449, 430)
        P = R.power_f64(a, center, hann)
        assert P[1:].min() >= 1e-4, (seed, n_mels, center, hann, P[1:].min())
        tie = R.roll_near_tie(P)
        assert tie.mean() <= 0.02
        want = R.series_f64(a, center, hann, q_c)
        got = E.cepstral_series(torch.from_numpy(a)[None].to(DEV), None, center, hann, q_c).cpu().numpy()[0].astype(np.float64)
        np32 = R.series_np32(a, center, hann, q_c).astype(np.float64)
        scale = np.abs(want[:3]).max(axis=1)
        ref_err = np.maximum(ref_err, np.abs(np32[:3] - want[:3]).max(axis=1) / scale)
        got_err = np.maximum(got_err, np.abs(got[:3] - want[:3]).max(axis=1) / scale)
        assert np.array_equal(got[3][~tie], want[3][~tie]), (seed, n_mels, center, hann)
    for k in range(3):
        print(f'{R.KEYS[k]}: kernel {got_err[k]:.2e} relative, numpy fp32 {ref_err[k]:.2e} (bound 4x = {4 * ref_err[k]:.2e})')
    assert (got_err <= 4 * ref_err).all(), (got_err, ref_err)


def test_series_ragged_rows_zero_past_the_end_and_equal_alone():
    from ttsamd import engine as E
    B, T = 5, 70
    lens = np.array([70, 33, 0, 16, 49])
    mel = np.full((B, 80, T), np.nan, np.float32)
    for r in range(B):
        mel[r, :, :lens[r]] = R.warped_pair(60 + r, 80, T, 8)[0][:, :lens[r]]
    out, power = E.cepstral_series(torch.from_numpy(mel).to(DEV), torch.from_numpy(lens).to(DEV), return_power=True)
    out, power = out.cpu().numpy(), power.cpu().numpy()
    for r in range(B):
        assert not out[r, :, lens[r]:].any() and not power[r, :, lens[r]:].any() and np.isfinite(out[r]).all()
        if lens[r]:
            alone = E.cepstral_series(torch.from_numpy(mel[r:r + 1, :, :lens[r]].copy()).to(DEV)).cpu().numpy()[0]
            assert np.array_equal(alone.view(np.uint32), out[r, :, :lens[r]].view(np.uint32)), r
            P = R.power_f64(mel[r, :, :lens[r]])
            assert np.abs(power[r, :, :lens[r]] - P).max() <= 2 * ULP * P.max()
    # the same series from the power the caller holds, with the reference's parameters
    fp = E.cepstral_series_from_power(torch.from_numpy(power[:1]).to(DEV), q_c=9, q1=2, q2=30, eps=1e-6, roll_p=0.9).cpu().numpy()[0]
    want = R.series_from_power_f64(power[0], 9, 2, 30, 1e-6, 0.9, 1.0)
    assert np.abs(fp[:3] - want[:3]).max() <= 4 * ULP * np.abs(want[:3]).max() and np.array_equal(fp[3], want[3])
    tiny = E.cepstral_series(torch.ones(1, 2, 4, device=DEV)).cpu().numpy()[0]          # Q = 2: one point, no slope
    assert np.isnan(tiny[1]).all() and not tiny[0].any() and (tiny[3] == 1).all()


def test_summary_against_numpy():
    """count / mean / median of the finite values and the standardised copy: the median is exact (a selection, or a mean of two), the
    mean is the float64 mean rounded, |z - z_numpy| <= 4 * 2^-23 * (|m| / s + |z|) elementwise (an absolute shift set by the rounding of
    the mean; numpy's own fp32 nanmean / nanstd sit up to 2 / 1 ulps from the float64 values); NaN frames are interpolated as np.interp
    does; an all-NaN and a constant series give zeros."""
    from ttsamd import engine as E
    rng = np.random.default_rng(5)
    T = 449
    a, _ = R.warped_pair(39, 80, T, 430)
    ser = np.zeros((3, 4, T), np.float32)
    lens = np.array([T, 300, 1])
    ser[0] = R.series_np32(a)
    ser[1] = ser[0] * np.float32(0.5) + rng.normal(0, 1, (4, T)).astype(np.float32)
    ser[1, 0, [0, 1, 2, 50, 51, 120, 298, 299]] = np.nan                                # both ends and inside
    ser[1, 1, :] = np.nan                                                               # all NaN
    ser[1, 2, :] = 3.0                                                                  # constant
    ser[1, 3, 7] = np.inf                                                               # not finite, not NaN: the feature is all zeros
    ser[1, :, 300:] = np.nan                                                            # poison past the end
    ser[2, :, 1:] = np.nan
    stats, feat = E.series_summary(torch.from_numpy(ser).to(DEV), torch.from_numpy(lens).to(DEV))
    stats, feat = stats.cpu().numpy(), feat.cpu().numpy()
    worst = 0.0
    for r in range(3):
        for k in range(4):
            x = ser[r, k, :lens[r]]
            fin = x[np.isfinite(x)]
            assert stats[r, k, 0] == fin.size
            if fin.size:
                assert stats[r, k, 2] == np.median(fin), (r, k)
                assert stats[r, k, 1] == np.float32(fin.astype(np.float64).mean()), (r, k)
            else:
                assert np.isnan(stats[r, k, 1]) and np.isnan(stats[r, k, 2])
            z, m, s = R.zscore_numpy(R.nan_interp(x))
            got = feat[r, k, :lens[r]]
            assert not feat[r, k, lens[r]:].any()
            if not z.any():
                assert not got.any(), (r, k)
                continue
            unit = ULP * (abs(float(m)) / float(s) + np.abs(z.astype(np.float64)))
            worst = max(worst, float((np.abs(got.astype(np.float64) - z) / unit).max()))
    print(f'z-score: worst |z - z_numpy| = {worst:.2f} units of 2^-23 (|m| / s + |z|) (bound 4)')
    assert worst <= 4.0
    assert feat[1, 0].any() and feat[0].any()
    with pytest.raises(E.L.TtsAmdError):
        E.series_summary(torch.zeros(1, 1, E.OVERSMOOTH_MAX_FRAMES + 1, device=DEV))


@pytest.fixture(scope='module')
def gold(golden):
    g = golden('oversmoothing')
    inputs = R.golden_inputs()
    assert R.inputs_digest(inputs) == str(g['inputs_sha256'])
    return g, inputs


def _check_aligned(got, g, name, what):
    """every mae_* / delta_u_* within 4x the key's recorded noise floor + 8 fp32 ulps of the series' median magnitude"""
    for i, k in enumerate(R.KEYS):
        med = max(abs(float(np.median(g[f'{name}_series_a'][i]))), abs(float(np.median(g[f'{name}_series_b'][i]))))
        for j, key in ((i, f'mae_{k}'), (4 + i, f'delta_u_{k}')):
            tol = 4 * g[f'{name}_floor'][j] + 8 * ULP * med
            v = float(got[key])
            print(f'{what} {name} {key}: {v:.8g} (reference {g[f"{name}_aligned"][j]:.8g}, floor {g[f"{name}_floor"][j]:.2e}, tol {tol:.2e})')
            assert abs(v - g[f'{name}_aligned'][j]) <= tol, (what, name, key)


def test_dropins_against_the_reference_goldens(gold):
    """utils.oversmoothing and utils.metrics on the golden inputs, numpy in and device tensors in."""
    from utils import metrics as mt, oversmoothing as ov
    g, inputs = gold
    for name, (a, b) in inputs.items():
        n_mels = a.shape[0]
        rel = (n_mels + n_mels // 2 + 1) * ULP
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        res = ov.oversmoothing_metrics_aligned(a, b)
        assert all(isinstance(v, float) for v in res.values()) and list(res)[:2] == ['mae_HQER', 'delta_u_HQER']
        _check_aligned(res, g, name, 'oversmoothing numpy')
        rt = ov.oversmoothing_metrics_aligned(ta, tb)
        assert all(isinstance(v, torch.Tensor) and v.is_cuda and v.dim() == 0 for v in rt.values())
        assert all(float(rt[k]) == res[k] for k in res)
        _check_aligned(mt.over_smoothing_metric_aligned(a, b), g, name, 'metrics numpy')
        for tag, kw in (('a', {}), ('a_raw_qc7', dict(center=False, hann=False, q_c=7))):
            m = ov.compute_mel_oversmoothing_metrics(a, **kw)
            assert m['Q'] == n_mels // 2 + 1 and m['CRoll95'].dtype == np.int64 and m['HQER'].dtype == np.float32
            want = g[f'{name}_series_{tag}']
            tie = R.roll_near_tie(R.power_f64(a, kw.get('center', True), kw.get('hann', True)))
            for i, k in enumerate(R.KEYS[:3]):
                assert np.abs(m[k] - want[i]).max() <= rel * np.abs(want[i]).max(), (name, tag, k)
            assert np.array_equal(m['CRoll95'][~tie], want[3][~tie].astype(np.int64))
        m2 = mt.compute_mel_over_smoothing_metrics(a.T.copy(), assume_BxT=False)
        m1 = ov.compute_mel_oversmoothing_metrics(a)
        assert all(np.array_equal(m1[k], m2[k]) for k in R.KEYS)
        for red in ('mean', 'median'):
            m = ov.compute_mel_oversmoothing_metrics(a, reduction=red)
            want = g[f'{name}_{red}_a']
            for i, k in enumerate(R.KEYS):
                assert isinstance(m[k], float)
                tol = rel * abs(want[i]) if i < 3 else (0.02 * m['Q'] if red == 'mean' else 0)
                assert abs(m[k] - want[i]) <= tol, (name, red, k, m[k], want[i])
            mt_ = ov.compute_mel_oversmoothing_metrics(ta, reduction=red)
            assert all(float(mt_[k]) == m[k] for k in R.KEYS)
        P = ov.framewise_rfft_power(a)
        assert P.shape == (n_mels // 2 + 1, a.shape[1]) and np.abs(P - R.power_f64(a)).max() <= 2 * ULP * P.max()
        h = ov.hqer_from_power(P)
        assert np.abs(100 * h - g[f'{name}_series_a'][0]).max() <= rel * 100
        assert ov.rolloff_from_power(P, reduction='median') == float(np.median(ov.rolloff_from_power(P)))
        assert np.isnan(ov.slope_from_power(P, q1=5, q2=5))
        for metric in ('l2', 'cosine'):
            for wname, w in (('none', None), ('w20', 20), ('tight', R.TIGHT_WINDOW)):
                cost, path, A_al, B_al = ov.dtw_align_mels(a, b, metric=metric, window=w, return_aligned=True)
                want = g[f'{name}_dtw_{metric}_{wname}_path'].astype(np.int32)
                assert isinstance(cost, float) and path.dtype == np.int32 and np.array_equal(path, want), (name, metric, wname)
                assert np.float32(cost).view(np.uint32) == g[f'{name}_dtw_{metric}_{wname}_cost'].view(np.uint32)
                assert np.array_equal(A_al, a.T[want[:, 0]]) and np.array_equal(B_al, b.T[want[:, 1]])
                c2, p2 = mt.dtw_align_mels(a.T.copy(), b, metric=metric, window=w, return_aligned=False)      # [T, M] and [M, T]
                assert c2 == cost and np.array_equal(p2, want)
                c3, p3 = ov.dtw_align_mels(ta, tb, metric=metric, window=w, return_aligned=False)
                assert float(c3) == cost and p3.is_cuda and np.array_equal(p3.cpu().numpy(), want)
    # a series with NaN frames, and a constant one
    sa, sb = g['p80_series_a'][1].copy(), g['p80_series_b'][1].copy()
    sb[list(R.NAN_FRAMES)] = np.nan
    assert np.isnan(ov.aligned_mae_distance(sa, sb)) and np.isnan(mt.aligned_distance(sa, sb))
    const = np.full(160, 3.0, np.float32)
    got = ov.aligned_mae_distance(sa, const)
    assert abs(got - float(g['const_mae'])) <= 8 * ULP * abs(float(g['const_mae'])), (got, float(g['const_mae']))


def test_batched_call_equals_the_pairs_and_error_paths(gold):
    from ttsamd import engine as E
    from ttsamd.lib import TtsAmdError
    from utils import oversmoothing as ov
    g, inputs = gold
    a0, b0 = inputs['p80']
    a1, b1 = R.warped_pair(77, 80, 120, 150)
    P, Rf = np.full((2, 80, 180), np.nan, np.float32), np.full((2, 80, 160), np.nan, np.float32)
    P[0], Rf[0], P[1, :, :120], Rf[1, :, :150] = a0, b0, a1, b1
    lp, lr = np.array([180, 120]), np.array([160, 150])
    res = ov.oversmoothing_metrics_aligned(P, Rf, lens_pred=lp, lens_ref=lr)
    for r, (a, b) in enumerate(((a0, b0), (a1, b1))):
        one = ov.oversmoothing_metrics_aligned(a, b)
        for k, v in one.items():
            assert np.float32(res[k][r]).view(np.uint32) == np.float32(v).view(np.uint32), (r, k)
    m = ov.compute_mel_oversmoothing_metrics(P, lens=lp, reduction='median')
    assert m['HQER'].shape == (2,) and m['HQER'][1] == ov.compute_mel_oversmoothing_metrics(a1, reduction='median')['HQER']
    cost, path, plen, A_al, B_al = ov.dtw_align_mels(P, Rf, metric='l2', lens_a=lp, lens_b=lr)
    c1, p1, A1, B1 = ov.dtw_align_mels(a1, b1, metric='l2')
    assert cost[1] == np.float32(c1) and np.array_equal(path[1, :plen[1]], p1) and np.array_equal(A_al[1, :plen[1]], A1)
    mel = torch.zeros(80, 20, device=DEV)
    with pytest.raises(TtsAmdError):
        ov.compute_mel_oversmoothing_metrics(torch.zeros(20, device=DEV))              # wrong rank
    with pytest.raises(TtsAmdError):
        ov.oversmoothing_metrics_aligned(mel, torch.zeros(100, 20, device=DEV))        # band counts differ
    with pytest.raises(TtsAmdError):
        ov.dtw_align_mels(mel, torch.zeros(100, 20, device=DEV))
    with pytest.raises(TtsAmdError):
        ov.compute_mel_oversmoothing_metrics(torch.zeros(129, 20, device=DEV))         # n_mels above 128
    long = torch.zeros(1, 1, E.OVERSMOOTH_MAX_FRAMES + 1, device=DEV)
    with pytest.raises(TtsAmdError):
        E.dtw(long, long[:, :, :10])                                                   # a length above the maximum
    with pytest.raises(TtsAmdError):
        ov.aligned_mae_distance(long[0, 0], long[0, 0, :10])
    with pytest.raises(TtsAmdError):
        E.dtw(mel[None], mel[None], metric='l1')
    lib = E.L.load()
    need = lib.ttsamd_dtw_workspace_bytes(1, 20, 20, 80)
    assert need > 0 and lib.ttsamd_dtw_workspace_bytes(1, 5000, 20, 1) == -1
    assert lib.ttsamd_dtw_workspace_bytes(32 * 4, 449, 430, 1) <= 32 * 4 * (449 * 430 + 8 * (449 + 430))   # <= 1 byte per cell + O(Ta + Tb)
    with pytest.raises(TtsAmdError, match='workspace'):
        E.dtw(mel[None], mel[None], workspace=torch.empty(need - 1, dtype=torch.uint8, device=DEV))


def test_pipeline_wave_to_scores_without_a_host_read():
    """MelSpecEngine on a batch of waves, the log-mels against a perturbed copy, scored by oversmoothing_score: the chain runs with
    torch's synchronisation check set to raise (any host read of a device value fails it) and equals the per-pair calls."""
    import melspec_ref as MR
    from ttsamd import engine as E
    from utils import oversmoothing as ov
    ms = E.MelSpecEngine(MR.fbank('audio'), 'same', 'eps', 1e-5)
    n = np.array([256 * 90, 256 * 61])
    wave = np.zeros((2, n.max()), np.float32)
    for r in range(2):
        wave[r, :n[r]] = MR.voiced(int(n[r]), 300 + r)
    wave_d, n_d = torch.from_numpy(wave).to(DEV), torch.from_numpy(n).to(DEV)
    noise = torch.from_numpy(np.random.default_rng(1).normal(0, 0.3, (2, 80, 90)).astype(np.float32)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        mel, frames = ms.forward(wave_d, n_d)
        pred = mel + noise
        sp, sr, score = E.oversmoothing_score(pred, frames, mel, frames)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    torch.cuda.synchronize()
    assert frames.tolist() == [90, 61] and sp.shape == (2, 4, 90) and not sp[1, :, 61:].any()
    for r in range(2):
        t = int(frames[r])
        one = ov.oversmoothing_metrics_aligned(pred[r, :, :t].cpu().numpy(), mel[r, :, :t].cpu().numpy())
        for k, v in one.items():
            assert np.float32(float(score[k][r])).view(np.uint32) == np.float32(v).view(np.uint32), (r, k)
        assert one['mae_HQER'] > 0 and np.isfinite(list(one.values())).all()
