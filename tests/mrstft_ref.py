"""float64 numpy restatement of the multi-resolution STFT distance of include/ttsamd.h (csrc/mrstft.hip), built on np.fft.rfft.  Written
from the specification; it shares no code with the kernels.  tests/test_mrstft_cpu.py pins it on the CPU (against torch.stft),
tests/test_gpu_mrstft.py uses it as the GPU yardstick."""
import numpy as np

DEFAULT = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))         # (n_fft, hop, win_length)
FLOOR = 1e-7


def window(N, W):
    """the periodic Hann window of W points at offset (N - W) // 2 of a frame of N, zero elsewhere"""
    w = np.zeros(N)
    off = (N - W) // 2
    w[off:off + W] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(W) / W)
    return w


def reflect_pad(x, P):
    """x [n], n > P -> [n + 2 P]: padded index p maps to j = p - P, j < 0 -> -j, j >= n -> 2 (n - 1) - j"""
    n = len(x)
    j = np.arange(-P, n + P)
    j = np.where(j < 0, -j, j)
    j = np.where(j >= n, 2 * (n - 1) - j, j)
    return x[j]


def frames(x, N, H, W):
    """x [n], n > N / 2 -> the windowed frames [1 + n // H, N]"""
    x = np.asarray(x, dtype=np.float64)
    padded = reflect_pad(x, N // 2)
    F = 1 + len(x) // H
    w = window(N, W)
    return np.stack([padded[f * H: f * H + N] * w for f in range(F)])


def magnitudes(x, N, H, W):
    """-> S [F, N / 2 + 1] = sqrt(max(|X|^2, 1e-7))"""
    X = np.fft.rfft(frames(x, N, H, W), axis=1)
    return np.sqrt(np.maximum(X.real ** 2 + X.imag ** 2, FLOOR))


def stft_distance(ref, est, N, H, W):
    """-> (sc, mag, frames) of one resolution; (NaN, NaN, 0) for a row of N / 2 samples or fewer"""
    ref, est = np.asarray(ref, dtype=np.float64), np.asarray(est, dtype=np.float64)
    assert ref.shape == est.shape and ref.ndim == 1
    if len(ref) <= N // 2:
        return float('nan'), float('nan'), 0
    Sr, Se = magnitudes(ref, N, H, W), magnitudes(est, N, H, W)
    sc = np.sqrt(np.sum((Sr - Se) ** 2)) / np.sqrt(np.sum(Sr ** 2))
    mag = np.sum(np.abs(np.log(Sr) - np.log(Se))) / (Sr.shape[0] * (N // 2 + 1))
    return float(sc), float(mag), Sr.shape[0]


def mr_stft(ref, est, resolutions=DEFAULT):
    """-> (per [R, 2] = (sc, mag), frames [R]) over the resolutions"""
    got = [stft_distance(ref, est, *r) for r in resolutions]
    return np.array([g[:2] for g in got], dtype=np.float64).reshape(len(got), 2), np.array([g[2] for g in got], dtype=np.int32)
