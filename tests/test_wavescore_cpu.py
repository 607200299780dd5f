"""CPU: pins tests/wavescore_ref.py, the float64 restatement of the wave-against-wave scores (include/ttsamd.h, csrc/wavescore.hip) that
tests/test_gpu_wavescore.py holds the kernels to: its tables against their construction, its transform against scipy, and the properties
the scores must have.  The last test needs no GPU either: the public functions refuse a CPU tensor."""
import numpy as np
import pytest

import wavescore_ref as R


@pytest.fixture(scope='module')
def x():
    return R.speech_like()


def test_band_table_is_the_argmin_construction_from_150_hz():
    lo, hi = R.band_edges(10000, 512, 15, 150.0)
    assert np.array_equal(lo, R.LO) and np.array_equal(hi, R.HI)
    assert np.array_equal(R.LO[1:], R.HI[:-1])                          # the bands tile bins 7 .. 218
    assert R.EPS == np.finfo(np.float64).eps


def test_window_is_hanning_258_without_its_zeros():
    assert np.array_equal(R.W, np.hanning(258)[1:-1]) and R.W.shape == (256,) and R.W.min() > 0
    assert not np.allclose(R.W, np.hanning(256))                        # not the symmetric 256-point window
    assert np.allclose(R.hann_periodic(1024), np.hanning(1025)[:-1], atol=1e-15)


def test_fft_stage_agrees_with_scipy_stft(x):
    from scipy.signal import stft
    sig = x.astype(np.float64)[:4000]
    # scipy scales by 1 / sum(window); boundary=None, padded=False: the same frames
    _, _, Z = stft(sig, fs=10000, window=R.W, nperseg=256, noverlap=128, nfft=512, boundary=None, padded=False, detrend=False)
    P = np.abs(Z.T * R.W.sum()) ** 2
    mine = R.spectra(sig)
    assert mine.shape == P.shape == (30, 257)
    assert np.abs(mine - P).max() <= 1e-12 * P.max()
    w = R.hann_periodic(1024)
    _, _, Z = stft(sig, fs=22050, window=w, nperseg=1024, noverlap=768, nfft=1024, boundary=None, padded=False, detrend=False)
    P = np.abs(Z.T * w.sum()) ** 2
    mine = R.spectra(sig, 1024, 256, 1024, w)
    assert mine.shape == P.shape == (12, 513) and np.abs(mine - P).max() <= 1e-12 * P.max()


def test_stoi_of_a_signal_with_itself_is_one(x):
    for ext in (False, True):
        assert abs(R.stoi_10k(x, x, ext) - 1.0) < 1e-12


def test_score_falls_with_the_snr(x):
    d = R.stoi_10k(x, R.add_noise(x, 10.0), details=True)
    assert d['frames'] == (155, 80)                                     # the compaction happens mid-row
    assert d['margin_db'] > 1.0 and d['cond'] > 1e-3
    for ext in (False, True):
        s = [R.stoi_10k(x, R.add_noise(x, snr), ext) for snr in (30.0, 10.0, 0.0, -5.0)]
        assert all(a > b for a, b in zip(s, s[1:])), s
        assert 0.0 < s[-1] and s[0] < 1.0


def test_29_kept_frames_are_too_short_and_30_give_one_segment():
    rng = np.random.default_rng(3)
    y = rng.standard_normal(4000)
    for n, F in ((0, 0), (255, 0), (256, 1), (3839, 28), (3840, 29)):
        d = R.stoi_10k(y[:n], y[:n], details=True)
        assert d['frames'] == (F, F) and d['score'] == 1e-5
    d = R.stoi_10k(y[:3968], y[:3968], details=True)
    assert d['frames'] == (30, 30) and d['tob_x'].shape == (15, 30) and abs(d['score'] - 1.0) < 1e-12
    dseg, _ = R.stoi_segments(d['tob_x'], d['tob_y'], False)
    assert dseg.shape == (1,)
    z = np.zeros(4000)
    assert R.stoi_10k(z, z, details=True)['frames'] == (30, 30) and R.stoi_10k(z, z) == 0.0 and R.stoi_10k(z, z, True) == 0.0


def test_silent_frames_go_by_the_clean_signal_alone(x):
    keep = R.kept_frames(x)
    xs, ys, F, K = R.remove_silent_frames(x, R.add_noise(x, 0.0))
    assert (F, K) == (155, len(keep)) and len(xs) == len(ys) == 128 * (K - 1) + 256
    # inside a run of kept neighbours the rebuilt signal is the signal times w[i] + w[i + 128] (the two frames that overlap a position)
    run = next(i for i in range(len(keep) - 2) if keep[i + 1] == keep[i] + 1 and keep[i + 2] == keep[i] + 2)
    got = xs[128 * (run + 1): 128 * (run + 1) + 128]
    want = x.astype(np.float64)[128 * keep[run + 1]: 128 * keep[run + 1] + 128] * (R.W[:128] + R.W[128:])
    assert np.allclose(got, want, rtol=0, atol=1e-15)


def test_si_sdr_is_scale_invariant_and_snr_is_not(x):
    y = R.add_noise(x, 10.0).astype(np.float64)
    si, sn = R.sdr(x, y)
    si3, sn3 = R.sdr(x, 3.0 * y)
    assert abs(si - si3) < 1e-10 and abs(sn - sn3) > 1.0
    assert abs(sn - 10.0) < 0.01 and abs(si - 10.0) < 0.05
    assert R.sdr(x, x) == (float('inf'), float('inf'))
    assert all(np.isnan(v) for v in R.sdr(np.zeros(0), np.zeros(0)))
    assert np.isnan(R.sdr(np.zeros(8), np.ones(8), zero_mean=False)[0])
    # zero_mean removes an offset (up to the rounding of the mean); without it the offset counts as distortion
    assert R.sdr(x, x.astype(np.float64) + 0.5)[0] > 200.0 and R.sdr(x, x.astype(np.float64) + 0.5, zero_mean=False)[0] < 0.0


def test_lsd_of_a_signal_with_itself_is_zero(x):
    assert R.lsd(x, x) == (0.0, 75)
    assert np.isnan(R.lsd(x[:1023], x[:1023])[0]) and R.lsd(x[:1023], x[:1023])[1] == 0
    assert R.lsd(x[:1024], x[:1024]) == (0.0, 1)
    d, F = R.lsd(x, R.add_noise(x, 10.0))
    assert F == 75 and d > 1.0
    d0, _ = R.lsd(x, np.zeros_like(x))                                  # est = 0: every bin of it sits on the 1e-10 floor (-100 dB)
    assert np.isfinite(d0) and d0 > d


def test_public_functions_refuse_a_cpu_tensor():
    import torch
    from ttsamd import engine as E
    from ttsamd.lib import TtsAmdError
    t = torch.zeros(1, 4000)
    for fn in (E.stoi_10k, E.wave_sdr, E.log_spectral_distance):
        with pytest.raises(TtsAmdError):
            fn(t, t)
    if torch.cuda.is_available():
        eng = E.WaveScoreEngine(22050)
        for fn in (eng.stoi, eng.metrics):
            with pytest.raises(TtsAmdError, match='no CPU fallback'):
                fn(t, t)
    else:
        with pytest.raises(TtsAmdError):
            E.WaveScoreEngine(22050)
