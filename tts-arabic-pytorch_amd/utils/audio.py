"""Output side of the path: wav files and the peak normalisation of the web manager.
The reference calls torchaudio.save(path, wave[None], 22050) (inference.py:61-63, utils/app_utils.py:76-77);
torchaudio is not a dependency here, so the RIFF container is written directly.
Analysis side: `MelSpectrogram` (reference utils/audio.py:6-46), the 80-band mel the acoustic models and HiFi-GAN were trained on,
as one HIP launch (csrc/melspec.hip)."""
import struct

import numpy as np
import torch
import torch.nn as nn

from ttsamd import melfb
from ttsamd.engine import MelSpecEngine
from ttsamd.lib import TtsAmdError


def _host_min_len(x, lens):
    """Shortest utterance if it is known without reading the device, else None."""
    if lens is None:
        return int(x.shape[-1])
    if isinstance(lens, torch.Tensor):
        return int(lens.min()) if lens.device.type == 'cpu' and lens.numel() else None
    return int(min(lens)) if len(lens) else None


class _MelModule(nn.Module):
    """A filterbank buffer `mel_basis` [n_mels, 513] + one MelSpecEngine per (device, matrix): the engine is rebuilt when the buffer
    was replaced or written to (`_version`), so a caller's own matrix is the one the kernel uses.  A buffer that is an inference tensor
    (made under torch.inference_mode()) has no version counter: the engine is then rebuilt on every call."""
    _framing, _mag, _log_clip, _what = 'same', 'abs', None, 'MelSpectrogram'

    def _engine(self):
        fb = self.mel_basis
        if fb.device.type != 'cuda':
            raise TtsAmdError(f'{type(self).__name__} is on {fb.device}: the MI355X path has no CPU fallback; '
                              'move the module with .to("cuda")')
        try:
            key = (str(fb.device), fb.data_ptr(), fb._version, tuple(fb.shape))
        except RuntimeError:                # an inference tensor tracks no version: in-place writes are invisible, so rebuild on every call
            key = None
        if key is None or getattr(self, '_eng_key', None) != key:
            self._eng = MelSpecEngine(fb, self._framing, self._mag, self._log_clip, device=fb.device)
            self._eng_key = key
        return self._eng

    def extract(self, x, lens=None):
        """x [B, n] (or [n]) -> (mel [B, n_mels, frames], frames int64 [B] on the device); `lens` int64 [B]: samples per row (ragged)."""
        need = MelSpecEngine.MIN_SAMPLES[self._framing]
        n_min = _host_min_len(x, lens)
        if n_min is not None and x.numel() and n_min < need:
            raise ValueError(f'{self._what}: every utterance needs more than {need - 1} samples (reflect padding of {need - 1}); '
                             f'shortest has {n_min}')
        eng = self._engine()
        if lens is not None and not isinstance(lens, torch.Tensor):
            lens = torch.as_tensor(lens, dtype=torch.int64)
        return eng.forward(x.reshape(-1, x.shape[-1]), lens)


class MelSpectrogram(_MelModule):
    """Drop-in for utils.audio.MelSpectrogram (reference utils/audio.py:6-46): reflect pad (n_fft - hop) / 2, STFT, sqrt(|X|^2 + 1e-9),
    mel_basis @ . -> LINEAR mel [B, n_mels, n // 256].  Built: n_fft = win_length = 1024, hop_length = 256, center=False, n_mels <= 128;
    anything else raises TtsAmdError here.  `mel_basis` = ttsamd.melfb (the formulas librosa.filters.mel implements; htk=False)."""
    _framing, _mag, _log_clip, _what = 'same', 'eps', None, 'MelSpectrogram'

    def __init__(self, sample_rate: int = 22050, n_fft: int = 1024, win_length: int = 1024, hop_length: int = 256,
                 n_mels: int = 80, f_min: float = 0, f_max: float = 8000.0, norm: str = 'slaney', center: bool = False):
        super().__init__()
        if n_fft != 1024 or win_length != 1024 or hop_length != 256 or center or not 1 <= n_mels <= 128:
            raise TtsAmdError(f'MelSpectrogram(n_fft={n_fft}, win_length={win_length}, hop_length={hop_length}, n_mels={n_mels}, '
                              f'center={center}): only n_fft = win_length = 1024, hop_length = 256, center=False, n_mels <= 128 is built')
        self.sample_rate, self.n_fft, self.hop_length, self.win_length, self.center = sample_rate, n_fft, hop_length, win_length, center
        self.pad_length = int((n_fft - hop_length) / 2)
        self.register_buffer('mel_basis', torch.from_numpy(melfb.mel_filterbank(sample_rate, n_fft, n_mels, f_min, f_max, norm, 'slaney')))
        self.register_buffer('window_fn', torch.hann_window(win_length))      # the kernel's own window is this one (periodic hann)

    @torch.inference_mode()
    def forward(self, x, lens=None):
        mel, _ = self.extract(x, lens)
        return mel[0] if x.dim() == 1 else mel


def save_wav(path, wave, sample_rate=22_050, encoding='PCM_S', bits_per_sample=16):
    """wave: 1-D (or [1, n]) float tensor/array in [-1, 1].  'PCM_S' 16-bit (torchaudio.save's default for
    .wav from float32 is 32-bit float: pass encoding='PCM_F') -> little-endian RIFF/WAVE, mono."""
    a = wave.detach().cpu().numpy() if hasattr(wave, 'detach') else np.asarray(wave)
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    if encoding == 'PCM_F':
        fmt, bits, data = 3, 32, a.astype('<f4').tobytes()
    elif encoding == 'PCM_S' and bits_per_sample == 16:
        fmt, bits = 1, 16
        data = np.clip(np.round(a * 32767.0), -32768, 32767).astype('<i2').tobytes()
    else:
        raise ValueError(f'unsupported wav encoding {encoding}/{bits_per_sample}')
    block = bits // 8
    hdr = b'RIFF' + struct.pack('<I', 36 + len(data)) + b'WAVE' + b'fmt ' + struct.pack(
        '<IHHIIHH', 16, fmt, 1, sample_rate, sample_rate * block, block, bits) + b'data' + struct.pack('<I', len(data))
    with open(path, 'wb') as f:
        f.write(hdr)
        f.write(data)


def peak_normalise(wave, peak=0.99):
    """wave / max|wave| * 0.99 (utils/app_utils.py:73-74); returns a new tensor/array."""
    m = abs(wave).max()
    return wave / m * peak if float(m) > 0 else wave


def load_wav(path):
    """Little-endian RIFF/WAVE -> (float32 array [n] in [-1, 1], sample_rate): 16-bit PCM (x / 32768) and 32-bit float, what save_wav
    writes; several channels are averaged to one.  Anything else raises ValueError.  There is no resampler here."""
    with open(path, 'rb') as f:
        raw = f.read()
    if len(raw) < 12 or raw[:4] != b'RIFF' or raw[8:12] != b'WAVE':
        raise ValueError(f'{path}: not a RIFF/WAVE file')
    pos, fmt, data = 12, None, None
    while pos + 8 <= len(raw):
        tag, size = raw[pos:pos + 4], struct.unpack('<I', raw[pos + 4:pos + 8])[0]
        body = raw[pos + 8:pos + 8 + size]
        if tag == b'fmt ':
            fmt = struct.unpack('<HHIIHH', body[:16])
        elif tag == b'data':
            data = body
        pos += 8 + size + (size & 1)
    if fmt is None or data is None:
        raise ValueError(f'{path}: no fmt / data chunk')
    code, channels, rate, _, _, bits = fmt
    if code == 1 and bits == 16:
        a = np.frombuffer(data[:len(data) // 2 * 2], dtype='<i2').astype(np.float32) / 32768.0
    elif code == 3 and bits == 32:
        a = np.frombuffer(data[:len(data) // 4 * 4], dtype='<f4').astype(np.float32)
    else:
        raise ValueError(f'{path}: format {code} with {bits} bits: 16-bit PCM and 32-bit float are read')
    if channels > 1:
        a = a[:len(a) // channels * channels].reshape(-1, channels).mean(axis=1).astype(np.float32)
    return a, int(rate)
