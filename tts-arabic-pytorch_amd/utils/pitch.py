"""Pitch tracking on the device: `pyin` with librosa.pyin's names and defaults (what the reference calls in scripts/extract_f0.py:34-39
and models/fastpitch/fastpitch/data_function.py:81-114), run by csrc/pyin.hip in two launches, plus the two helpers of that script:
`note_to_hz` and the pooled `pitch_mean_std`.

Not librosa bit for bit, by design: the difference function is summed directly in float64 (librosa's FFT route and its clamp of values
below 1e-6 are not reproduced), and parity with a particular librosa release is not pinned; the arithmetic is stated in DESIGN.md
section 4 and restated in float64 by tests/pyin_ref.py.  A tensor on the device comes back as tensors on the device, a NumPy array as
NumPy (one copy each way).  No CPU fallback: without a gfx950 device every call raises."""
import math

import numpy as np
import torch

from ttsamd import engine as _engine
from ttsamd.lib import TtsAmdError

_NOTES = {'C': 0, 'D': 2, 'E': 4, 'F': 5, 'G': 7, 'A': 9, 'B': 11}
_engines = {}


def note_to_hz(note):
    """'C2' -> 65.406..., 'C7' -> 2093.004... (A4 = 440 Hz, twelve-tone equal temperament; '#' and 'b' accidentals)."""
    s = str(note).strip()
    if not s or s[0].upper() not in _NOTES:
        raise ValueError(f'note_to_hz: {note!r}')
    pitch, i = _NOTES[s[0].upper()], 1
    while i < len(s) and s[i] in '#b':
        pitch += 1 if s[i] == '#' else -1
        i += 1
    midi = 12 * (int(s[i:] or 0) + 1) + pitch
    return 440.0 * 2.0 ** ((midi - 69) / 12.0)


def _engine_for(device, fmin, fmax, **kw):
    key = (str(device), float(fmin), float(fmax)) + tuple(sorted((k, tuple(v) if isinstance(v, (tuple, list)) else v) for k, v in kw.items()))
    if key not in _engines:
        _engines[key] = _engine.PyinEngine(fmin, fmax, device=device, **kw)
    return _engines[key]


def pyin(y, *, fmin, fmax, sr=22050, frame_length=2048, win_length=None, hop_length=None, n_thresholds=100, beta_parameters=(2, 18),
         boltzmann_parameter=2, resolution=0.1, max_transition_rate=35.92, switch_prob=0.01, no_trough_prob=0.01, fill_na=np.nan,
         center=True, pad_mode='constant', lens=None):
    """y [..., n] -> (f0 [..., T], voiced_flag [..., T] bool, voiced_prob [..., T]), T = 1 + n // hop_length; f0 is float32 with `fill_na`
    on unvoiced frames.  `lens` (not in librosa): samples per row of a ragged batch; row b is then the call on y[b, :lens[b]] alone and
    its frames past 1 + lens[b] // hop_length are unvoiced with probability 0.  Built: center=True, pad_mode 'constant' / 'reflect',
    a number as fill_na, frame_length even and <= 2048, win_length < frame_length, at most 1024 pitch bins, 128 thresholds, 8192
    frames per row, integer beta_parameters; anything else raises TtsAmdError."""
    if not center:
        raise TtsAmdError('pyin(center=False): only center=True (frames centred on t * hop_length, padded by frame_length // 2) is built')
    if fill_na is None:
        raise TtsAmdError('pyin(fill_na=None): the best-guess fill is not built; pass a number (NaN is the default)')
    host = not isinstance(y, torch.Tensor)
    if host:
        _engine._require_gpu()
        x = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to('cuda:0')
    else:
        if y.device.type != 'cuda':
            raise TtsAmdError('pyin: a tensor must live on the ROCm device (NumPy arrays are copied there)')
        x = y
    lead = tuple(x.shape[:-1])
    eng = _engine_for(x.device, fmin, fmax, sr=sr, frame_length=frame_length, win_length=win_length, hop_length=hop_length,
                      n_thresholds=n_thresholds, beta_parameters=tuple(beta_parameters), boltzmann_parameter=boltzmann_parameter,
                      resolution=resolution, max_transition_rate=max_transition_rate, switch_prob=switch_prob,
                      no_trough_prob=no_trough_prob, pad_mode=pad_mode)
    if lens is not None and not isinstance(lens, torch.Tensor):
        lens = torch.as_tensor(np.asarray(lens), dtype=torch.int64)
    f0, flag, prob, _ = eng.forward(x.reshape(-1, x.shape[-1]), None if lens is None else lens.reshape(-1))
    f0 = torch.where(flag, f0, torch.full_like(f0, float(fill_na)))
    out = tuple(t.reshape(lead + (t.shape[-1],)) for t in (f0, flag, prob))
    return tuple(t.cpu().numpy() for t in out) if host else out


def pitch_mean_std(tracks):
    """Pooled mean and standard deviation of the voiced values (> 1 Hz; NaN counts as unvoiced) of an iterable of f0 tracks, by the
    running update of scripts/extract_f0.py:57-76 in float64: per track the mean m, the population variance v and the count n of its
    voiced values, then
        var  <- ((N - 1) var + (n - 1) v) / (N + n - 1) + N n (m - mean)^2 / ((N + n) (N + n - 1))
        mean <- (n m + N mean) / (n + N),  N <- N + n.
    A track without a voiced value is skipped.  -> (mean, std) as Python floats."""
    mean = var = 0.0
    count = 0
    for tr in tracks:
        a = tr.detach().cpu().numpy() if hasattr(tr, 'detach') else np.asarray(tr)
        a = np.asarray(a, dtype=np.float64).reshape(-1)
        a = a[np.nan_to_num(a, nan=0.0) > 1]
        n = a.size
        if n == 0:
            continue
        m, v = float(a.mean()), float(a.var())
        if count + n > 1:
            var = ((count - 1) * var + (n - 1) * v) / (count + n - 1) + count * n * (m - mean) ** 2 / ((count + n) * (count + n - 1))
        mean = (n * m + count * mean) / (n + count)
        count += n
    return mean, math.sqrt(var)
