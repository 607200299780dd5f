"""Shared by tests/test_griffinlim_cpu.py and tests/test_gpu_griffinlim.py (not a test module): the numpy restatement of
csrc/griffinlim.hip (include/ttsamd.h: ttsamd_griffinlim, ttsamd_mel_to_linear), parameterised by dtype -- float64 is the reference,
float32 (numpy's pocketfft runs in single precision for single input) measures the reference's own rounding noise, from which the GPU
tests take their bounds.

  c = momentum / (1 + momentum);  angles = init;  tprev = 0
  n_iter times:  inv = istft(mag * angles);  rebuilt = stft(inv);  a = rebuilt - c * tprev;  angles = a / (|a| + 1e-16);  tprev = rebuilt
  wave = istft(mag * angles)

Layouts here are frame-major: mag [T, 513] real, angles [T, 513] complex (the library's `phase` layout; its `mag` is [513, T]).
The mutants (MUTANTS) are the structural errors a kernel of this kind can make; the CPU test shows that each moves the wave by far more
than the tolerance the GPU test derives, so that the GPU test would see it."""
import numpy as np

N_FFT, HOP, NBIN = 1024, 256, 513
PAD = {'center': 512, 'same': 384}
MIN_FRAMES = {'center': 4, 'same': 2}
MUTANTS = ('no_momentum', 'no_envelope', 'zero_pad', 'symmetric_window', 'eps_missing', 'tprev_is_angles')


def samples(T, framing):
    return HOP * (T - 1) if framing == 'center' else HOP * T


def window(dtype=np.float64, mut=None):
    if mut == 'symmetric_window':
        return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / (N_FFT - 1))).astype(dtype)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)


def _cdtype(dtype):
    return np.complex64 if np.dtype(dtype) == np.float32 else np.complex128


def stft(x, framing, dtype=np.float64, mut=None):
    """x [n] -> [T, 513]: reflect padding at the row's own ends, frames of 1024 every 256, periodic hann"""
    x = np.asarray(x, dtype=dtype)
    pad = PAD[framing]
    assert x.size > pad, f'{framing}: {x.size} samples, the reflect padding needs more than {pad}'
    xp = np.pad(x, pad, mode='constant' if mut == 'zero_pad' else 'reflect')
    T = (xp.size - N_FFT) // HOP + 1
    idx = HOP * np.arange(T)[:, None] + np.arange(N_FFT)[None, :]
    out = np.fft.rfft(xp[idx] * window(dtype, mut)[None, :], axis=1)
    assert out.dtype == _cdtype(dtype)
    return out


def envelope(T, dtype=np.float64, mut=None):
    """sum of the squared windows of the frames that exist at each of the 256 (T - 1) + 1024 padded samples"""
    L = HOP * (T - 1) + N_FFT
    if mut == 'no_envelope':
        return np.full(L, 1.5, dtype=dtype)
    w2 = window(dtype, mut) ** 2
    env = np.zeros(L, dtype=dtype)
    for t in range(T):
        env[HOP * t:HOP * t + N_FFT] += w2
    return env


def istft(spec, framing, dtype=np.float64, mut=None):
    """spec [T, 513] complex -> [n]: c2r per frame (the imaginary parts of bins 0 and 512 are dropped), window, overlap-add in ascending
    frame order, over the envelope, cropped by the padding"""
    spec = np.asarray(spec, dtype=_cdtype(dtype))
    T = spec.shape[0]
    fr = np.fft.irfft(spec, n=N_FFT, axis=1).astype(dtype) * window(dtype, mut)[None, :]
    L = HOP * (T - 1) + N_FFT
    ola = np.zeros(L, dtype=dtype)
    for t in range(T):
        ola[HOP * t:HOP * t + N_FFT] += fr[t]
    pad, n = PAD[framing], samples(T, framing)
    env = envelope(T, dtype, mut)
    return (ola[pad:pad + n] / env[pad:pad + n]).astype(dtype)


def _fmix32(h):
    h = h.astype(np.uint64)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    return h


def hash_angle_units(T, seed):
    """(h >> 8) of every (t, k): the phase is 2 pi times this times 2^-24.  uint32 arithmetic carried in uint64."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    lo, hi = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    idx = (np.arange(T, dtype=np.uint64)[:, None] * np.uint64(NBIN) + np.arange(NBIN, dtype=np.uint64)[None, :]) & np.uint64(0xFFFFFFFF)
    h = (lo + ((np.uint64(0x9E3779B9) * idx) & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)
    h = _fmix32(_fmix32(h) ^ hi)
    return (h >> np.uint64(8)).astype(np.int64)


def hash_phase(T, seed, dtype=np.float64):
    ang = (2.0 * np.pi) * hash_angle_units(T, seed).astype(np.float64) * 2.0 ** -24
    return (np.cos(ang) + 1j * np.sin(ang)).astype(_cdtype(dtype))


def griffinlim(mag, n_iter, momentum, framing, init=0, seed=0, phase=None, dtype=np.float64, mut=None):
    """mag [T, 513] -> dict(wave [n], angles [T, 513] complex, inconsistency, history: the inconsistency of every iteration).
    init 0: zero phase, 1: the hash under `seed`, 2: `phase` [T, 513] complex."""
    cd = _cdtype(dtype)
    mag = np.asarray(mag, dtype=dtype)
    T = mag.shape[0]
    assert mag.shape == (T, NBIN) and T >= MIN_FRAMES[framing]
    if init == 0:
        angles = np.ones((T, NBIN), dtype=cd)
    elif init == 1:
        angles = hash_phase(T, seed, dtype)
    else:
        angles = np.asarray(phase, dtype=cd).copy()
    if mut == 'no_momentum':
        momentum = 0.0
    c = np.asarray(momentum / (1.0 + momentum), dtype=dtype)
    eps = np.asarray(0.0 if mut == 'eps_missing' else 1e-16, dtype=dtype)
    tprev = np.zeros((T, NBIN), dtype=cd)
    history = []
    for _ in range(n_iter):
        inv = istft(mag * angles, framing, dtype, mut)
        rebuilt = stft(inv, framing, dtype, mut)
        a = rebuilt - c * tprev if momentum else rebuilt
        with np.errstate(invalid='ignore', divide='ignore'):
            angles = (a / (np.abs(a) + eps)).astype(cd)
        tprev = angles if mut == 'tprev_is_angles' else rebuilt
        d = np.abs(rebuilt).astype(dtype) - mag
        history.append(float(np.sqrt(np.sum(d.astype(np.float64) ** 2)) / np.sqrt(np.sum(mag.astype(np.float64) ** 2))))
    wave = istft(mag * angles, framing, dtype, mut)
    return dict(wave=wave, angles=angles, inconsistency=history[-1] if history else float('nan'), history=history)


def pinv_filterbank(fb):
    """P [513, n_mels]: the float64 pseudo-inverse of the float32 filterbank [n_mels, 513], rounded once to float32 (what the kernel gets)"""
    return np.linalg.pinv(np.asarray(fb, dtype=np.float64)).astype(np.float32)


def mel_to_linear(mel, pinv, log=True, floor=1e-10, dtype=np.float64):
    """mel [n_mels, T] -> mag [513, T] = max(P exp(mel), floor); also |P| exp(mel), the scale of the fp32 rounding bound"""
    e = np.asarray(mel, dtype=dtype)
    e = np.exp(e) if log else e
    P = np.asarray(pinv, dtype=dtype)
    return np.maximum(P @ e, np.asarray(floor, dtype=dtype)), np.abs(P) @ np.abs(e)


def test_signal(n, seed=0, snr_db=20.0):
    """wavescore_ref.speech_like at 22 050 Hz plus white noise at 20 dB, so that the bins are not mostly empty"""
    import wavescore_ref as WR
    return WR.add_noise(WR.speech_like(n, fs=22050, seed=seed), snr_db, seed=seed + 1)
