"""Mel filterbanks [n_mels, n_fft // 2 + 1] from the published formulas, own code: computed in float64 and rounded once to float32.

Two scales, as `librosa.filters.mel` and torchaudio's `melscale_fbanks` define them:
  'slaney' (Slaney's Auditory Toolbox): linear below 1 kHz at 200/3 Hz per mel, logarithmic above with log(6.4) / 27 per mel;
  'htk':   mel = 2595 * log10(1 + f / 700).
Band m is the triangle over the edges f[m] < f[m + 1] < f[m + 2], f = mel^-1(linspace(mel(f_min), mel(f_max), n_mels + 2)), sampled at the
bin centres linspace(0, sr / 2, n_fft // 2 + 1); norm 'slaney' scales it by 2 / (f[m + 2] - f[m]) (unit area), None leaves the peak at 1.
Neither library is a dependency of this package: the values are pinned to the formulas, not to those libraries' own rounding."""
import numpy as np

_F_SP = 200.0 / 3.0
_MIN_LOG_HZ = 1000.0
_MIN_LOG_MEL = _MIN_LOG_HZ / _F_SP            # 15
_LOGSTEP = np.log(6.4) / 27.0


def hz_to_mel(f, mel_scale='htk'):
    f = np.asarray(f, dtype=np.float64)
    if mel_scale == 'htk':
        return 2595.0 * np.log10(1.0 + f / 700.0)
    if mel_scale != 'slaney':
        raise ValueError('mel_scale should be one of "htk" or "slaney"')
    return np.where(f >= _MIN_LOG_HZ, _MIN_LOG_MEL + np.log(np.maximum(f, _MIN_LOG_HZ) / _MIN_LOG_HZ) / _LOGSTEP, f / _F_SP)


def mel_to_hz(m, mel_scale='htk'):
    m = np.asarray(m, dtype=np.float64)
    if mel_scale == 'htk':
        return 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    if mel_scale != 'slaney':
        raise ValueError('mel_scale should be one of "htk" or "slaney"')
    return np.where(m >= _MIN_LOG_MEL, _MIN_LOG_HZ * np.exp(_LOGSTEP * (m - _MIN_LOG_MEL)), _F_SP * m)


def band_edges(sample_rate, n_mels, f_min=0.0, f_max=None, mel_scale='htk'):
    """The n_mels + 2 band edges in Hz (float64)."""
    f_max = sample_rate / 2.0 if f_max is None else float(f_max)
    m = np.linspace(hz_to_mel(float(f_min), mel_scale), hz_to_mel(f_max, mel_scale), n_mels + 2)
    return mel_to_hz(m, mel_scale)


def mel_filterbank(sample_rate, n_fft, n_mels, f_min=0.0, f_max=None, norm=None, mel_scale='htk', dtype=np.float32):
    """-> [n_mels, n_fft // 2 + 1]; norm None or 'slaney'."""
    if norm not in (None, 'slaney'):
        raise ValueError('norm must be one of None or "slaney"')
    freqs = np.linspace(0.0, sample_rate / 2.0, n_fft // 2 + 1)
    f = band_edges(sample_rate, n_mels, f_min, f_max, mel_scale)
    fdiff = np.diff(f)
    slopes = f[:, None] - freqs[None, :]                       # [n_mels + 2, bins]
    down = -slopes[:-2] / fdiff[:-1, None]                     # rises from f[m] to f[m + 1]
    up = slopes[2:] / fdiff[1:, None]                          # falls from f[m + 1] to f[m + 2]
    fb = np.maximum(0.0, np.minimum(down, up))
    if norm == 'slaney':
        fb *= (2.0 / (f[2:] - f[:-2]))[:, None]
    return fb.astype(dtype)
