"""The numpy restatement of csrc/griffinlim.hip (tests/griffinlim_ref.py) pinned on the CPU, so that the GPU tests can trust it:
against a torch.stft / torch.istft loop in float64 (`center` framing), by perfect reconstruction (both framings), by the frame count
the mel analysis sees, by the Griffin-Lim theorem, and -- for the tolerance rule of tests/test_gpu_griffinlim.py -- by showing that
every structural mutant moves the wave by more than 100 x the float32 rounding noise from which that rule takes its bounds."""
import numpy as np
import pytest
import torch

import griffinlim_ref as G
import melspec_ref as MR


def _signal(T, framing, seed=0):
    return G.test_signal(G.samples(T, framing), seed=seed).astype(np.float64)


def _torch_loop(mag, angles, n_iter, momentum):
    """torchaudio.functional.griffinlim's loop on torch.stft / torch.istft (center=True), float64, from given angles; [T, 513] in and out"""
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    mag_t, ang = torch.from_numpy(mag).T, torch.from_numpy(angles).T
    n = 256 * (mag.shape[0] - 1)
    c = momentum / (1 + momentum)
    tprev = torch.zeros_like(ang)
    for _ in range(n_iter):
        inv = torch.istft(mag_t * ang, 1024, 256, 1024, win, center=True, length=n)
        rebuilt = torch.stft(inv, 1024, 256, 1024, win, center=True, pad_mode='reflect', normalized=False, onesided=True, return_complex=True)
        a = rebuilt - c * tprev if momentum else rebuilt
        ang = a / (a.abs() + 1e-16)
        tprev = rebuilt
    wave = torch.istft(mag_t * ang, 1024, 256, 1024, win, center=True, length=n)
    return wave.numpy(), ang.T.numpy()


@pytest.mark.parametrize('momentum', [0.0, 0.99])
@pytest.mark.parametrize('n_iter', [1, 2, 8])
def test_center_against_torch_loop(n_iter, momentum):
    T = 21
    mag = np.abs(G.stft(_signal(T, 'center'), 'center'))
    ang0 = G.hash_phase(T, seed=7)
    got = G.griffinlim(mag, n_iter, momentum, 'center', init=2, phase=ang0)
    wave, ang = _torch_loop(mag, ang0, n_iter, momentum)
    assert got['wave'].shape == wave.shape == (256 * (T - 1),)
    ew, ea = np.abs(got['wave'] - wave).max(), np.abs(got['angles'] - ang).max()
    print(f'n_iter {n_iter} momentum {momentum}: wave {ew:.2e}, angles {ea:.2e} (1e-10)')
    assert ew <= 1e-10 and ea <= 1e-10


def test_restatement_stft_is_torch_stft():
    x = _signal(12, 'center', seed=3)
    win = torch.hann_window(1024, periodic=True, dtype=torch.float64)
    ref = torch.stft(torch.from_numpy(x), 1024, 256, 1024, win, center=True, pad_mode='reflect', return_complex=True).T.numpy()
    assert np.abs(G.stft(x, 'center') - ref).max() <= 1e-11


@pytest.mark.parametrize('framing,T', [('same', 2), ('same', 17), ('center', 4), ('center', 18)])
def test_perfect_reconstruction(framing, T):
    x = _signal(T, framing, seed=5)
    X = G.stft(x, framing)
    assert X.shape == (T, G.NBIN)
    mag = np.abs(X)
    ang0 = X / mag                                                  # (the noise leaves no bin at exactly 0)
    got0 = G.griffinlim(mag, 0, 0.99, framing, init=2, phase=ang0)
    assert got0['wave'].shape == x.shape and np.isnan(got0['inconsistency'])
    assert np.abs(got0['wave'] - x).max() <= 1e-12
    got1 = G.griffinlim(mag, 1, 0.99, framing, init=2, phase=ang0)
    # the spectrum stays where it is; a raw angle moves by the float64 noise over the bin's own magnitude
    assert np.abs(mag * (got1['angles'] - ang0)).max() <= 1e-12 * mag.max() and np.abs(got1['angles'] - ang0).max() <= 1e-8
    assert got1['inconsistency'] <= 1e-12


def test_same_framing_output_has_the_frames_it_was_given():
    T = 9
    mag = np.abs(G.stft(_signal(T, 'same'), 'same'))
    wave = G.griffinlim(mag, 2, 0.99, 'same', init=1, seed=1)['wave']
    assert wave.shape == (256 * T,)
    assert MR.mel_ref(wave, MR.fbank('audio'), 'same', 1).shape[-1] == T
    wave_c = G.griffinlim(np.abs(G.stft(_signal(T, 'center'), 'center')), 2, 0.99, 'center', init=1, seed=1)['wave']
    assert MR.mel_ref(wave_c, MR.fbank('audio'), 'center', 0).shape[-1] == T


def _moved(a, b):
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return float('inf') if not np.isfinite(d).all() else float(d.max())


@pytest.mark.parametrize('framing', ['same', 'center'])
def test_every_mutant_moves_the_wave_past_the_float32_noise(framing):
    """the input has a stretch of exact silence (the 1e-16 of the angle update is what keeps it silent: 0 / 0 without it)"""
    T = 32
    x = _signal(T, framing, seed=2)
    x[256 * 8:256 * 24] = 0.0                                       # long enough that rebuilt frames are exactly 0 too
    mag = np.abs(G.stft(x, framing))
    ang0 = G.hash_phase(T, seed=11)
    ref64 = G.griffinlim(mag, 2, 0.99, framing, init=2, phase=ang0)['wave']
    ref32 = G.griffinlim(mag.astype(np.float32), 2, 0.99, framing, init=2, phase=ang0, dtype=np.float32)['wave']
    assert ref32.dtype == np.float32
    noise = _moved(ref32, ref64)
    assert 0.0 < noise < 1e-4 * np.abs(ref64).max()
    for mut in G.MUTANTS:
        moved = _moved(G.griffinlim(mag, 2, 0.99, framing, init=2, phase=ang0, mut=mut)['wave'], ref64)
        print(f'{framing} {mut}: moved {moved:.2e}, float32 noise {noise:.2e}')
        assert moved > 100.0 * noise, mut


@pytest.mark.parametrize('framing', ['same', 'center'])
def test_inconsistency_does_not_increase_without_momentum(framing):
    T = 20
    mag = np.abs(G.stft(_signal(T, framing, seed=4), framing))
    h = G.griffinlim(mag, 8, 0.0, framing, init=1, seed=3)['history']
    print(framing, ['%.4f' % v for v in h])
    assert len(h) == 8 and all(b <= a for a, b in zip(h, h[1:]))


def test_hash_init_is_uniform_and_keyed():
    u = G.hash_angle_units(40, seed=0)
    assert u.min() >= 0 and u.max() < 2 ** 24 and abs(u.mean() / 2 ** 24 - 0.5) < 0.01
    assert not np.array_equal(u, G.hash_angle_units(40, seed=1)) and not np.array_equal(u, G.hash_angle_units(40, seed=1 << 32))
    assert np.array_equal(u[:7], G.hash_angle_units(7, seed=0))     # a frame's phase does not depend on the row's length
    # fmix32 against murmur3's published test value: fmix32(1) = 0x514E28B7
    assert int(G._fmix32(np.array([1], dtype=np.uint64))[0]) == 0x514E28B7


def test_mel_to_linear_round_trip():
    fb = MR.fbank('audio')
    P = G.pinv_filterbank(fb)
    assert P.shape == (G.NBIN, 80) and P.dtype == np.float32
    mel = np.log(np.maximum(fb.astype(np.float64) @ np.abs(G.stft(_signal(12, 'same'), 'same')).T, 1e-5))
    mag, scale = G.mel_to_linear(mel, P)
    assert mag.shape == (G.NBIN, 12) and mag.min() >= 1e-10 and (scale >= 0).all()
    # P is a pseudo-inverse: the mel of the inverted magnitude (before the floor) is the mel
    back = fb.astype(np.float64) @ (P.astype(np.float64) @ np.exp(mel))
    assert np.abs(back - np.exp(mel)).max() <= 1e-5 * np.exp(mel).max()
