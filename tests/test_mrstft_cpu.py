"""CPU: pins tests/mrstft_ref.py, the float64 restatement of the multi-resolution STFT distance (include/ttsamd.h, csrc/mrstft.hip)
that tests/test_gpu_mrstft.py holds the kernels to: against an independent torch route (torch.stft in float64 with center=True and
reflect padding, then the two formulas written out in torch), its frame counts, the too-short rows and three closed-form cases.

Bounds of the torch comparison: 1e-11 relative on the spectral convergence and 1e-9 absolute on the log-magnitude distance, the
project's SDR_RTOL and LSD_TOL (tests/test_gpu_wavescore.py) for the same error classes.  The worst observed differences are printed:
they are the noise floor of this class of error (two float64 FFTs with different summation order)."""
import numpy as np
import pytest
import torch

import mrstft_ref as M
import wavescore_ref as R

SC_RTOL, MAG_TOL = 1e-11, 1e-9
RESOLUTIONS = M.DEFAULT + ((512, 128, 512), (1024, 77, 241))           # the last: N - W odd
SNRS = (30.0, 10.0, -5.0)


@pytest.fixture(scope='module')
def x():
    return R.speech_like()


def lengths(N):
    return (N // 2 + 1, N - 1, 3000, 20000)


def torch_route(ref, est, N, H, W):
    """-> (sc, mag, frames) through torch.stft in float64"""
    w = torch.hann_window(W, dtype=torch.float64)
    S = []
    for v in (ref, est):
        X = torch.stft(torch.from_numpy(np.asarray(v, dtype=np.float64)), n_fft=N, hop_length=H, win_length=W, window=w, center=True,
                       pad_mode='reflect', return_complex=True)
        S.append(torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=1e-7)))
    sc = torch.sqrt(((S[0] - S[1]) ** 2).sum()) / torch.sqrt((S[0] ** 2).sum())
    mag = (torch.log(S[0]) - torch.log(S[1])).abs().mean()
    return float(sc), float(mag), S[0].shape[1]


def test_restatement_agrees_with_torch_stft(x):
    worst_sc = worst_mag = 0.0
    for snr in SNRS:
        y = R.add_noise(x, snr)
        for N, H, W in RESOLUTIONS:
            for n in lengths(N):
                sc, mag, F = M.stft_distance(x[:n], y[:n], N, H, W)
                tsc, tmag, tF = torch_route(x[:n], y[:n], N, H, W)
                assert F == tF == 1 + n // H
                dsc, dmag = abs(sc - tsc) / abs(tsc), abs(mag - tmag)
                worst_sc, worst_mag = max(worst_sc, dsc), max(worst_mag, dmag)
                assert dsc <= SC_RTOL and dmag <= MAG_TOL, (snr, N, H, W, n, sc, tsc, mag, tmag)
    print(f'restatement against torch.stft: worst relative difference of sc {worst_sc:.3e} (bound {SC_RTOL:.0e}), worst absolute '
          f'difference of mag {worst_mag:.3e} (bound {MAG_TOL:.0e})')


def test_frames_are_torch_stft_frames(x):
    """steps 1 - 3 alone: the windowed frames' spectra against torch.stft's, relative to the largest bin"""
    for N, H, W in RESOLUTIONS:
        for n in lengths(N):
            X = np.fft.rfft(M.frames(x[:n], N, H, W), axis=1)
            T = torch.stft(torch.from_numpy(x[:n].astype(np.float64)), n_fft=N, hop_length=H, win_length=W,
                           window=torch.hann_window(W, dtype=torch.float64), center=True, pad_mode='reflect', return_complex=True).numpy().T
            assert X.shape == T.shape == (1 + n // H, N // 2 + 1)
            assert np.abs(X - T).max() <= 1e-12 * np.abs(T).max()


def test_frame_counts(x):
    for N, H, W in RESOLUTIONS:
        k = N // H + 2                                                  # k H - 1 and k H: the count steps
        for n in lengths(N) + (k * H - 1, k * H):
            assert M.stft_distance(x[:n], x[:n], N, H, W)[2] == 1 + n // H == M.frames(x[:n], N, H, W).shape[0]
    per, fr = M.mr_stft(x, x)
    assert per.shape == (3, 2) and fr.dtype == np.int32 and fr.tolist() == [1 + 20000 // 120, 1 + 20000 // 240, 1 + 20000 // 50]


def test_too_short_rows_give_nan_where_torch_raises(x):
    for N, H, W in RESOLUTIONS:
        for n in (1, N // 2):
            sc, mag, F = M.stft_distance(x[:n], x[:n], N, H, W)
            assert np.isnan(sc) and np.isnan(mag) and F == 0
            with pytest.raises(RuntimeError):
                torch_route(x[:n], x[:n], N, H, W)
        assert M.stft_distance(x[:N // 2 + 1], x[:N // 2 + 1], N, H, W)[2] == 1 + (N // 2 + 1) // H      # one sample more: valid
    per, fr = M.mr_stft(x[:600], x[:600])                              # valid at 512 and 1024, too short at 2048
    assert np.isnan(per[1]).all() and np.isfinite(per[[0, 2]]).all() and fr.tolist() == [6, 0, 13]


def test_identical_pair_is_exactly_zero(x):
    for N, H, W in RESOLUTIONS:
        for n in lengths(N):
            assert M.stft_distance(x[:n], x[:n], N, H, W)[:2] == (0.0, 0.0)


def test_zero_estimate_sits_on_the_floor(x):
    for N, H, W in RESOLUTIONS:
        Se = M.magnitudes(np.zeros(3000, dtype=np.float32), N, H, W)
        assert np.all(Se == np.sqrt(1e-7))
        Sr = M.magnitudes(x[:3000], N, H, W)
        sc, mag, _ = M.stft_distance(x[:3000], np.zeros(3000, dtype=np.float32), N, H, W)
        assert sc == np.sqrt(np.sum((Sr - np.sqrt(1e-7)) ** 2)) / np.sqrt(np.sum(Sr ** 2))
        assert abs(mag - np.mean(np.abs(np.log(Sr) - 0.5 * np.log(1e-7)))) <= 1e-12


def test_doubled_estimate_gives_one_and_ln_two():
    a = np.random.default_rng(21).standard_normal(6000).astype(np.float32)
    for N, H, W in RESOLUTIONS:
        X = np.fft.rfft(M.frames(a, N, H, W), axis=1)
        assert (X.real ** 2 + X.imag ** 2).min() > 1e-7               # every bin of both clears the floor
        sc, mag, _ = M.stft_distance(a, 2.0 * a, N, H, W)
        assert abs(sc - 1.0) <= 1e-12 and abs(mag - np.log(2.0)) <= 1e-12
