"""CPU: the restatements of tests/recording_ref.py against second formulations, the host-side tap table of ttsamd.resample against the
restatement, and the host drop-ins of utils.data.  No GPU, no library call."""
import math

import numpy as np
import pytest
import torch

import recording_ref as R
from conftest import WAVE_TOL
from melspec_ref import voiced


def test_resample_ref_agrees_with_a_plain_loop():
    x = voiced(700, 3, sr=48000)
    for orig, new, lfw in [(48000, 22050, 16), (44100, 22050, 8), (22050, 24000, 6), (8000, 22050, 5)]:
        a = R.resample_ref(x, orig, new, lfw).numpy()
        b = R.resample_direct(x, orig, new, lfw)
        assert a.shape == b.shape
        assert np.abs(a - b).max() < 1e-12, (orig, new)


@pytest.mark.parametrize('orig,new', [(48000, 22050), (44100, 22050), (22050, 24000)])
def test_resampled_sine_is_the_sine_at_the_new_rate(orig, new):
    x = np.sin(2 * np.pi * 440.0 * np.arange(6000) / orig)
    y = R.resample_ref(x, orig, new, 64).numpy()
    m = np.arange(y.size)
    want = np.sin(2 * np.pi * 440.0 * m / new)
    mid = slice(y.size // 4, y.size - y.size // 4)
    err = np.abs(y[mid] - want[mid]).max()
    print(f'{orig} -> {new}: middle half against the analytic sine {err:.2e}')
    assert err < 1e-5


@pytest.mark.parametrize('case', sorted(R.RATE_CASES))
def test_host_table_equals_the_restatement(case):
    from ttsamd.resample import resample_taps
    orig, new, lfw = case
    taps, width, o, n = resample_taps(orig, new, lowpass_filter_width=lfw)
    rt, rw, ro, rn = R.taps_ref(orig, new, lfw)
    assert (o, n, taps.shape[1]) == R.RATE_CASES[case] == (ro, rn, rt.shape[1])
    assert width == rw and taps.shape[1] == 2 * width + o
    assert taps.dtype == np.float32 and taps.shape == (n, 2 * width + o)
    assert np.array_equal(taps.view(np.uint32), rt.view(np.uint32))
    assert resample_taps(orig, new, lowpass_filter_width=lfw)[0] is taps           # cached per argument tuple


@pytest.mark.parametrize('case', sorted(R.RATE_CASES))
def test_output_length_rule(case):
    from ttsamd.resample import out_len
    o, n, _ = R.RATE_CASES[case]
    orig, new, lfw = case
    for L in sorted({1, max(o - 1, 1), o, o + 1, 6000, 6001}):
        want = math.ceil(n * L / o)
        assert out_len(L, o, n) == R.out_len(L, o, n) == want
        if lfw <= 64:
            assert R.resample_ref(np.zeros(L), orig, new, lfw).numel() == want
    assert out_len((1 << 40) + 1, 320, 147) == (147 * ((1 << 40) + 1) + 319) // 320      # exact past 2^31 and past float64's integers


def test_the_waveform_bar_sees_a_wrong_tap():
    x = voiced(6000, 5, sr=48000)
    taps, width, o, n = R.taps_ref(48000, 22050, 64)
    good = R.resample_ref(x, 48000, 22050, taps=(taps, width, o, n)).numpy()
    shifted = R.resample_ref(x, 48000, 22050, taps=(np.roll(taps, 1, axis=0), width, o, n)).numpy()
    holed = taps.copy()
    p, j = np.unravel_index(np.abs(taps).argmax(), taps.shape)
    holed[p, j] = 0.0
    hole = R.resample_ref(x, 48000, 22050, taps=(holed, width, o, n)).numpy()
    e1, e2 = np.abs(shifted - good).max(), np.abs(hole - good).max()
    print(f'phase index moved by one: {e1:.2e}; centre tap zeroed: {e2:.2e}; bar {WAVE_TOL:.0e}')
    assert e1 > 10 * WAVE_TOL and e2 > 10 * WAVE_TOL


def _trim_brute(x, top_db, fl, hop):
    x = np.asarray(x, dtype=np.float64)
    L = x.size
    r2 = []
    for t in range(1 + L // hop):
        s = 0.0
        for g in range(t * hop - fl // 2, t * hop - fl // 2 + fl):
            if 0 <= g < L:
                s += x[g] * x[g]
        r2.append(max(math.sqrt(s / fl), 1e-5) ** 2)
    top = max(r2)
    loud = [t for t, v in enumerate(r2) if v > 10.0 ** (-top_db / 10.0) * top]
    return (loud[0] * hop, min(L, (loud[-1] + 1) * hop)) if loud else (0, 0)


def test_trim_ref_against_a_frame_loop():
    rows = R.trim_rows()
    for i, x in enumerate(rows):
        (bounds, margin) = R.trim_ref(x, 23, 1024, 256)
        assert bounds == _trim_brute(x, 23, 1024, 256), i
        if i < len(R.TRIM_BOUNDS):
            assert bounds == R.TRIM_BOUNDS[i] and margin > 0.5, (i, bounds, margin)
    assert R.trim_ref(rows[4], 23, 1024, 256)[0] == (0, 3000)                      # all-zero row: every frame sits at the floor = the max
    assert R.trim_ref(voiced(4000, 1), 60, 2048, 512)[0] == _trim_brute(voiced(4000, 1), 60, 2048, 512)


def _remove_silence_loop(e, thresh):
    keep = [bool(v > thresh) for v in e]
    i = len(keep) - 1
    while not keep[i] and i > 0:
        keep[i] = True
        i -= 1
    return np.array(keep)


def test_remove_silence_ref_and_the_drop_in_against_the_loop():
    from utils.data import normalize_pitch, remove_silence
    rng = np.random.default_rng(2)
    cases = [rng.uniform(-14, -6, size=40), np.full(9, -11.0), np.full(9, -3.0), np.array([-11.0]), np.array([-3.0]),
             np.array([-11.0, -3.0, -11.0, -11.0]), np.array([-3.0, -11.0, -11.0, -3.0, -11.0])]
    for e in cases:
        want = _remove_silence_loop(e, -10.0)
        assert np.array_equal(R.remove_silence_ref(e, -10.0), want)
        assert np.array_equal(remove_silence(torch.from_numpy(e), -10.0).numpy(), want)
    assert not _remove_silence_loop(np.full(5, -11.0), -10.0)[0] and _remove_silence_loop(np.full(5, -11.0), -10.0)[1:].all()
    p = torch.tensor([0.0, 130.05478, 152.91745, 0.0])
    q = normalize_pitch(p)
    assert q is p and torch.allclose(p, torch.tensor([0.0, 0.0, 1.0, 0.0]), atol=1e-6)
