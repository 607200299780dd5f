"""CPU: the restatements tests/oversmoothing_ref.py against the reference's goldens (tests/golden/oversmoothing.npz, written by
tools/gen_golden_oversmoothing.py from the reference's utils/oversmoothing.py and utils/metrics.py), the input conditions the series
comparisons rest on, and the drop-in modules' surface.  The GPU tests compare the kernels with these restatements."""
import inspect

import numpy as np
import pytest

import oversmoothing_ref as R

WINDOWS = {'none': -1, 'w20': 20, 'tight': R.TIGHT_WINDOW}


@pytest.fixture(scope='module')
def gold(golden):
    g = golden('oversmoothing')
    inputs = R.golden_inputs()
    assert R.inputs_digest(inputs) == str(g['inputs_sha256']), 'the seeded inputs differ from the ones the golden run used'
    return g, inputs


def test_dtw_restatement_equals_the_reference_bit_for_bit(gold):
    """Every DTW golden: array_equal on the path, == on the cost's bits; the too-tight band gives an empty path and cost 1e30f."""
    g, inputs = gold
    n = 0
    for name, (a, b) in inputs.items():
        for mi, metric in enumerate(('l2', 'cosine')):
            for wname, w in WINDOWS.items():
                cost, path = R.dtw_fp32(a.T, b.T, mi, w)
                want = g[f'{name}_dtw_{metric}_{wname}_path'].astype(np.int32)
                assert np.array_equal(path, want), (name, metric, wname)
                assert np.float32(cost).view(np.uint32) == g[f'{name}_dtw_{metric}_{wname}_cost'].view(np.uint32), (name, metric, wname)
                if wname == 'tight':
                    assert len(path) == 0 and cost == np.float32(1e30)
                n += 1
    # M = 1, on the standardised series: NaN frames interpolated, and a constant series (all features zero: ties everywhere)
    sa = g['p80_series_a'][1]
    fa = R.zscore_numpy(R.nan_interp(sa))[0]
    for case in ('nan', 'const'):
        cost, path = R.dtw_fp32(fa[:, None], g[f'{case}_feat'][:, None], 0, -1)
        assert np.array_equal(path, g[f'{case}_path'].astype(np.int32)), case
        n += 1
    assert n == 14


def test_summary_restatement_equals_the_reference(gold):
    g, _ = gold
    sb = g['p80_series_b'][1].copy()
    sb[list(R.NAN_FRAMES)] = np.nan
    assert np.array_equal(R.zscore_numpy(R.nan_interp(sb))[0], g['nan_feat'])
    assert not g['const_feat'].any() and np.array_equal(R.zscore_numpy(np.full(160, 3.0, np.float32))[0], g['const_feat'])
    assert np.isnan(g['nan_mae'])                    # the error is taken on the ORIGINAL series: its NaN frames are on the path


def test_series_restatement_agrees_with_the_reference_fp32(gold):
    """float64 restatement against the reference's fp32 series.  Bound: (n_mels + Q) * 2^-23 * max|series|, rounding growing linearly
    over the terms a frame accumulates (1.4e-5 relative at 80 bands; the reference's own fp32 error measured 3e-7 .. 3.6e-6 relative);
    a wrong formula is orders of magnitude outside it.  CRoll95 is an index: exact on every frame that is no near-tie."""
    g, inputs = gold
    for name, (a, b) in inputs.items():
        n_mels = a.shape[0]
        Q = n_mels // 2 + 1
        cases = [('a', a, True, True, None), ('b', b, True, True, None), ('a_raw_qc7', a, False, False, 7)]
        for tag, mel, center, hann, q_c in cases:
            P = R.power_f64(mel, center, hann)
            assert P[1:].min() >= 1e-4, (name, tag, P[1:].min())           # the 1e-8 inside the logarithm never decides
            tie = R.roll_near_tie(P)
            assert tie.mean() <= 0.02, (name, tag, tie.mean())
            want, got = g[f'{name}_series_{tag}'].astype(np.float64), R.series_f64(mel, center, hann, q_c)
            for k, key in enumerate(R.KEYS[:3]):
                err, bound = np.abs(got[k] - want[k]).max(), (n_mels + Q) * 2.0 ** -23 * np.abs(got[k]).max()
                print(f'{name} {tag} {key}: max-abs {err:.2e} (bound {bound:.2e}, values to {np.abs(got[k]).max():.3g})')
                assert err <= bound, (name, tag, key)
            assert np.array_equal(got[3][~tie], want[3][~tie]), (name, tag)
            print(f'{name} {tag} CRoll95: exact on {int((~tie).sum())} of {tie.size} frames, min P {P[1:].min():.2e}')
        for red, fn in (('mean', np.mean), ('median', np.median)):
            got = fn(R.series_f64(a), axis=1)
            want = g[f'{name}_{red}_a']
            assert np.allclose(got[:3], want[:3], rtol=(n_mels + Q) * 2.0 ** -23, atol=0), (name, red, got, want)
            assert abs(got[3] - want[3]) <= (0.02 * Q if red == 'mean' else 0), (name, red)


# the reference's public names with their parameters and defaults (utils/oversmoothing.py, utils/metrics.py)
SIGNATURES = {
    'oversmoothing': {
        'framewise_rfft_power': [('mel_BxT', inspect.Parameter.empty), ('center', True), ('hann', True)],
        'hqer_from_power': [('P_qT', inspect.Parameter.empty), ('q_c', None), ('reduction', 'none')],
        'slope_from_power': [('P_qT', inspect.Parameter.empty), ('q1', 1), ('q2', None), ('eps', 1e-8), ('reduction', 'none')],
        'centroid_from_power': [('P_qT', inspect.Parameter.empty), ('reduction', 'none')],
        'rolloff_from_power': [('P_qT', inspect.Parameter.empty), ('p', 0.95), ('reduction', 'none')],
        'compute_mel_oversmoothing_metrics': [('mel', inspect.Parameter.empty), ('center', True), ('hann', True), ('q_c', None),
                                              ('reduction', 'none')],
        'dtw_align_mels': [('mel_a', inspect.Parameter.empty), ('mel_b', inspect.Parameter.empty), ('metric', 'cosine'), ('window', None),
                           ('return_aligned', True)],
        'aligned_mae_distance': [('series_pred', inspect.Parameter.empty), ('series_ref', inspect.Parameter.empty)],
        'oversmoothing_metrics_aligned': [('mel_spec_pred', inspect.Parameter.empty), ('mel_spec_ref', inspect.Parameter.empty),
                                          ('center', True), ('hann', True)],
    },
    'metrics': {
        '_ensure_time_major': [('x', inspect.Parameter.empty)],
        'dtw_align_mels': [('mel_a', inspect.Parameter.empty), ('mel_b', inspect.Parameter.empty), ('metric', 'cosine'), ('window', None),
                           ('return_aligned', True)],
        'hqer_from_power': [('P_qT', inspect.Parameter.empty), ('q_c', None), ('reduction', 'none')],
        'slope_from_power': [('P_qT', inspect.Parameter.empty), ('q1', 1), ('q2', None), ('eps', 1e-8), ('reduction', 'none')],
        'centroid_from_power': [('P_qT', inspect.Parameter.empty), ('reduction', 'none')],
        'rolloff_from_power': [('P_qT', inspect.Parameter.empty), ('p', 0.95), ('reduction', 'none')],
        'compute_mel_over_smoothing_metrics': [('mel', inspect.Parameter.empty), ('assume_BxT', True), ('center', True), ('hann', True),
                                               ('q_c', None), ('reduction', 'none')],
        'aligned_distance': [('series_pred', inspect.Parameter.empty), ('series_ref', inspect.Parameter.empty)],
        'over_smoothing_metric_aligned': [('mel_spec_pred', inspect.Parameter.empty), ('mel_spec_ref', inspect.Parameter.empty),
                                          ('center', True)],
    },
}


def test_dropins_keep_the_reference_names_and_defaults_and_raise_without_a_device():
    """utils.oversmoothing / utils.metrics import on a CPU-only machine and expose the reference's names: its parameters lead each
    signature with its defaults (what follows them is this project's batch addition, `lens*`, always defaulted).  Without a gfx950
    device a call raises TtsAmdError: there is no CPU fallback."""
    import importlib
    import torch
    from ttsamd.lib import TtsAmdError
    for mod_name, table in SIGNATURES.items():
        mod = importlib.import_module(f'utils.{mod_name}')
        for fn_name, want in table.items():
            params = list(inspect.signature(getattr(mod, fn_name)).parameters.values())
            assert [(p.name, p.default) for p in params[:len(want)]] == want, (mod_name, fn_name)
            for extra in params[len(want):]:
                assert extra.name.startswith('lens') and extra.default is None, (mod_name, fn_name, extra.name)
    assert importlib.import_module('utils.metrics')._ensure_time_major(np.zeros((80, 200))).shape == (200, 80)
    if not torch.cuda.is_available():
        ov, mt = importlib.import_module('utils.oversmoothing'), importlib.import_module('utils.metrics')
        mel, ser = np.zeros((80, 20), np.float32), np.zeros(20, np.float32)
        calls = [lambda: ov.framewise_rfft_power(mel), lambda: ov.hqer_from_power(np.ones((41, 20), np.float32)),
                 lambda: ov.slope_from_power(np.ones((41, 20), np.float32)), lambda: ov.compute_mel_oversmoothing_metrics(mel),
                 lambda: ov.dtw_align_mels(mel, mel), lambda: ov.aligned_mae_distance(ser, ser),
                 lambda: ov.oversmoothing_metrics_aligned(mel, mel), lambda: mt.dtw_align_mels(mel.T, mel),
                 lambda: mt.compute_mel_over_smoothing_metrics(mel), lambda: mt.aligned_distance(ser, ser),
                 lambda: mt.over_smoothing_metric_aligned(mel, mel)]
        for call in calls:
            with pytest.raises(TtsAmdError):
                call()
