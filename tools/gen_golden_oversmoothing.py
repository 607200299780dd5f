"""Generate tests/golden/oversmoothing.npz with the REAL reference's utils/oversmoothing.py and utils/metrics.py.
Run manually where the reference tree is readable (oracle/_refstub.py: TTS_REFERENCE):  python tools/gen_golden_oversmoothing.py

What runs is the reference's own text, its numba decorators replaced by the identity (oracle/_refstub.py), so the DTW core runs as plain
Python over NumPy 2 scalars: every operation in it is one fp32 operation (parity unpinned at the numba boundary).  The inputs
are rebuilt from seeds by tests/oversmoothing_ref.py; the file holds their sha256 and the reference's OUTPUTS only: series, paths, costs,
metric dicts, and per metric key the reference's own noise floor: the largest change of oversmoothing_metrics_aligned's value over 16
repeats in which the per-frame series are multiplied by 1 + 4 * 2^-23 * N(0, 1) and the mean / std of each z-score are moved by a random
-2 .. +2 fp32 ulps (rounding-level noise at the two places where another implementation's rounding differs from numpy's)."""
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _load('oversmoothing_ref', os.path.join(REPO, 'tests', 'oversmoothing_ref.py'))
_refstub = _load('_refstub', os.path.join(REPO, 'oracle', '_refstub.py'))


def _ulps(v, k):
    v = np.float32(v)
    for _ in range(abs(int(k))):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


def noise_floor(ov, sp, sr, rng, repeats=16):
    """{key: (floor of mae, floor of delta_u)} for the series dicts sp / sr of the reference."""
    def feat(x, dm, ds):
        x = ov._nan_interp_1d(x)
        m, s = _ulps(np.nanmean(x), dm), _ulps(np.nanstd(x), ds)
        return ((x - m) / s).astype(np.float32)[:, None]

    def score(a, b, d):
        _, path = ov._dtw_path_numba(feat(a, d[0], d[1]), feat(b, d[2], d[3]), metric=0, window=-1)
        return (float(np.mean(np.abs(a[path[:, 0]] - b[path[:, 1]]))), ov._median_ignore_nan(a) - ov._median_ignore_nan(b))

    out = {}
    for k in R.KEYS:
        a, b = sp[k].astype(np.float32), sr[k].astype(np.float32)
        base = score(a, b, (0, 0, 0, 0))
        fl = [0.0, 0.0]
        for _ in range(repeats):
            an = (a * (1 + 4 * 2.0 ** -23 * rng.standard_normal(a.size))).astype(np.float32)
            bn = (b * (1 + 4 * 2.0 ** -23 * rng.standard_normal(b.size))).astype(np.float32)
            got = score(an, bn, rng.integers(-2, 3, 4))
            fl = [max(f, abs(g - v)) for f, g, v in zip(fl, got, base)]
        out[k] = fl
    return out


def main():
    inputs = R.golden_inputs()
    digest = R.inputs_digest(inputs)
    _refstub.install()
    ov = _load('ref_oversmoothing', os.path.join(_refstub.REF, 'utils', 'oversmoothing.py'))
    mt = _load('ref_metrics', os.path.join(_refstub.REF, 'utils', 'metrics.py'))
    rng = np.random.default_rng(2024)
    out = {'inputs_sha256': np.array(digest)}
    for name, (a, b) in inputs.items():
        sp, sr = ov.compute_mel_oversmoothing_metrics(a), ov.compute_mel_oversmoothing_metrics(b)
        assert sp['Q'] == a.shape[0] // 2 + 1
        out[f'{name}_series_a'] = np.stack([sp[k].astype(np.float32) for k in R.KEYS])
        out[f'{name}_series_b'] = np.stack([sr[k].astype(np.float32) for k in R.KEYS])
        for red in ('mean', 'median'):
            m = ov.compute_mel_oversmoothing_metrics(a, reduction=red)
            out[f'{name}_{red}_a'] = np.array([m[k] for k in R.KEYS], np.float64)
        m = ov.compute_mel_oversmoothing_metrics(a, center=False, hann=False, q_c=7)
        out[f'{name}_series_a_raw_qc7'] = np.stack([m[k].astype(np.float32) for k in R.KEYS])
        al = ov.oversmoothing_metrics_aligned(a, b)
        old = mt.over_smoothing_metric_aligned(a, b)
        assert al == old, 'utils/metrics.py and utils/oversmoothing.py disagree'
        out[f'{name}_aligned'] = np.array([al[f'mae_{k}'] for k in R.KEYS] + [al[f'delta_u_{k}'] for k in R.KEYS], np.float64)
        fl = noise_floor(ov, sp, sr, rng)
        out[f'{name}_floor'] = np.array([fl[k][0] for k in R.KEYS] + [fl[k][1] for k in R.KEYS], np.float64)
        print(name, 'aligned', out[f'{name}_aligned'], 'floor', out[f'{name}_floor'])
        for metric in ('l2', 'cosine'):
            for wname, w in (('none', None), ('w20', 20), ('tight', R.TIGHT_WINDOW)):
                assert w is None or w == 20 or w < abs(a.shape[1] - b.shape[1])
                cost, path, A_al, B_al = ov.dtw_align_mels(a, b, metric=metric, window=w, return_aligned=True)
                c2, p2 = mt.dtw_align_mels(a, b, metric=metric, window=w, return_aligned=False)
                assert np.array_equal(path, p2) and np.float32(cost) == np.float32(c2)
                assert np.array_equal(A_al, a.T[path[:, 0]]) and np.array_equal(B_al, b.T[path[:, 1]])
                out[f'{name}_dtw_{metric}_{wname}_cost'] = np.float32(cost)
                out[f'{name}_dtw_{metric}_{wname}_path'] = path.astype(np.int16)
                print(name, metric, wname, float(cost), path.shape)
    # a series with NaN frames and a constant one (zero standard deviation), against p80's CSlope series
    sa, sb = out['p80_series_a'][1].copy(), out['p80_series_b'][1].copy()
    sb[list(R.NAN_FRAMES)] = np.nan
    out['nan_feat'] = ov._zscore_1d(ov._nan_interp_1d(sb))
    ai, bi = ov._dtw_align_indices_1d(sa, sb)
    out['nan_path'] = np.stack([ai, bi], axis=1).astype(np.int16)
    out['nan_mae'] = np.float64(ov.aligned_mae_distance(sa, sb))
    const = np.full(160, 3.0, np.float32)
    out['const_feat'] = ov._zscore_1d(ov._nan_interp_1d(const))
    ai, bi = ov._dtw_align_indices_1d(sa, const)
    out['const_path'] = np.stack([ai, bi], axis=1).astype(np.int16)
    out['const_mae'] = np.float64(ov.aligned_mae_distance(sa, const))
    path = os.path.join(REPO, 'tests', 'golden', 'oversmoothing.npz')
    np.savez_compressed(path, **out)
    print(f'oversmoothing: {os.path.getsize(path) / 1024:.1f} kB')


if __name__ == '__main__':
    main()
