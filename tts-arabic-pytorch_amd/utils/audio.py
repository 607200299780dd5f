"""Output side of the path: wav files and the peak normalisation of the web manager.
The reference calls torchaudio.save(path, wave[None], 22050) (inference.py:61-63, utils/app_utils.py:76-77);
torchaudio is not a dependency here, so the RIFF container is written directly.
Analysis side: `MelSpectrogram` (reference utils/audio.py:6-46), the 80-band mel the acoustic models and HiFi-GAN were trained on,
as one HIP launch (csrc/melspec.hip).
Synthesis without a vocoder: `GriffinLim` / `griffinlim` (torchaudio.transforms.GriffinLim's names) and `mel_to_linear`, on the device
(csrc/griffinlim.hip): specified by its arithmetic; `center` framing pinned against `torch.stft` / `torch.istft`; parity with a
torchaudio release unpinned (own random init).
Input side: `resample` / `Resample` (torchaudio.functional.resample's name and defaults), `trim` (librosa.effects.trim's) and
`prepare_recording` = the clean-up of the reference's scripts/preprocess_audio.py:33-47 (resample with lowpass_filter_width=1024,
peak 0.999, trim at 23 dB, 768 zeros appended), on the device (csrc/resample.hip, csrc/trim.hip).
Level: `loudness` (ITU-R BS.1770-4 integrated loudness per row), `normalize_loudness` and `peak_normalize`, on the device and per row
of a ragged batch (csrc/loudness.hip); `peak_normalise` is the host helper for one wave.
Joining: `join_waves`, several waves -> one with trimmed seams, faded edges and exact pauses, on the device (csrc/join.hip): what
`tts_long` of the models runs behind the vocoder."""
import struct

import numpy as np
import torch
import torch.nn as nn

from ttsamd import melfb
from ttsamd.engine import GriffinLimEngine, MelSpecEngine, ResampleEngine, TrimEngine
from ttsamd.engine import LIMITER_NO_MAX_GAIN, LIMITER_Q, check_finite, limiter_samples, limiter_spec, per_row, row_values
from ttsamd.engine import leveller as _leveller
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


_gl_engines = {}


def _gl_engine(device):
    device = torch.device(device)
    if device.type != 'cuda':
        raise TtsAmdError(f'griffinlim: the input is on {device}: the MI355X path has no CPU fallback; move it with .to("cuda")')
    key = str(device)
    if key not in _gl_engines:
        _gl_engines[key] = GriffinLimEngine(device=device)
    return _gl_engines[key]


def _gl_lens(lens, B, T, framing, what):
    """frames per row from `lens` in samples (what the framing gives back: 256 T or 256 (T - 1)); host values are checked"""
    if lens is None:
        return None
    if isinstance(lens, torch.Tensor) and lens.device.type != 'cpu':
        return (lens // 256 + (framing == 'center')).to(torch.int32)
    host = np.asarray(lens.numpy() if isinstance(lens, torch.Tensor) else lens, dtype=np.int64).reshape(-1)
    if host.size != B or (host % 256).any():
        raise TtsAmdError(f'{what}: lens={host.tolist()}: one length per row ({B}), each a multiple of hop_length = 256 '
                          f'(the {framing!r} framing gives {"256 (T - 1)" if framing == "center" else "256 T"} samples for T frames)')
    return host // 256 + (framing == 'center')


def griffinlim(specgram, window=None, n_fft=1024, hop_length=256, win_length=None, power=2.0, n_iter=32, momentum=0.99, length=None,
               rand_init=True, framing='center', seed=0, lens=None):
    """torchaudio.functional.griffinlim's names on the HIP path (csrc/griffinlim.hip): specgram [..., 513, T] on the device, a magnitude
    to the power `power` (any positive float; the root is taken here with torch) -> wave [..., n], n = 256 (T - 1) for framing='center'
    (torch.stft's center=True) or 256 T for 'same' (the HiFi-GAN mel's framing).  The project's additions: framing=, seed= (one int,
    or one per row: the random initial phase is a hash of (seed, frame, bin), so a row's audio depends on neither its batch nor its
    position) and lens= (samples per row of a ragged batch; what lies past a row's length is zero).  rand_init=False is zero phase.
    Refused by name: n_fft other than 1024, hop_length other than 256, win_length other than 1024, a window other than the periodic
    hann, a length other than the framing's n."""
    what = 'griffinlim'
    if n_fft != 1024:
        raise TtsAmdError(f'{what}: n_fft={n_fft}: only n_fft = 1024 is built')
    if hop_length not in (None, 256):
        raise TtsAmdError(f'{what}: hop_length={hop_length}: only hop_length = 256 is built')
    if win_length not in (None, 1024):
        raise TtsAmdError(f'{what}: win_length={win_length}: only win_length = n_fft = 1024 is built')
    if window is not None:
        w = torch.as_tensor(window).detach().cpu().double()
        if w.shape != (1024,) or float((w - torch.hann_window(1024, dtype=torch.float64)).abs().max()) > 1e-6:
            raise TtsAmdError(f'{what}: window: only the periodic hann window of 1024 samples (torch.hann_window(1024)) is built')
    if not (isinstance(power, (int, float)) and power > 0 and np.isfinite(power)):
        raise TtsAmdError(f'{what}: power={power!r} is not a positive number')
    if framing not in GriffinLimEngine.MIN_FRAMES:
        raise TtsAmdError(f"{what}: framing={framing!r}: only 'same' and 'center' are built")
    if not isinstance(specgram, torch.Tensor) or specgram.dim() < 2 or specgram.shape[-2] != 513:
        raise TtsAmdError(f'{what}: specgram of shape {tuple(getattr(specgram, "shape", ()))}, expected [..., 513, T] (n_fft = 1024)')
    T = specgram.shape[-1]
    n = GriffinLimEngine.samples(T, framing)
    if length is not None and length != n:
        raise TtsAmdError(f'{what}: length={length}: {T} frames in the {framing!r} framing give {n} samples, no other length is built')
    eng = _gl_engine(specgram.device)
    lead = specgram.shape[:-2]
    mag = specgram.reshape(-1, 513, T).float()
    if power != 1:
        mag = mag.pow(1.0 / power)
    frames = _gl_lens(lens, mag.shape[0], T, framing, what)
    wave = eng.forward(mag, frames, n_iter=n_iter, momentum=momentum, framing=framing, init='hash' if rand_init else 'zeros', seed=seed)
    return wave.reshape(*lead, n)


class GriffinLim(nn.Module):
    """torchaudio.transforms.GriffinLim's names (n_fft, n_iter, win_length, hop_length, power, momentum, length, rand_init) over
    `griffinlim` above; the project's additions are framing='center', seed=0 and, at the call, lens=.  No window_fn / wkwargs: the
    window is the periodic hann."""

    def __init__(self, n_fft: int = 1024, n_iter: int = 32, win_length=None, hop_length=None, power: float = 2.0, momentum: float = 0.99,
                 length=None, rand_init: bool = True, framing: str = 'center', seed: int = 0):
        super().__init__()
        if n_fft != 1024:
            raise TtsAmdError(f'GriffinLim: n_fft={n_fft}: only n_fft = 1024 is built')
        if hop_length not in (None, 256):
            raise TtsAmdError(f'GriffinLim: hop_length={hop_length}: only hop_length = 256 is built')
        if win_length not in (None, 1024):
            raise TtsAmdError(f'GriffinLim: win_length={win_length}: only win_length = n_fft = 1024 is built')
        if framing not in GriffinLimEngine.MIN_FRAMES:
            raise TtsAmdError(f"GriffinLim: framing={framing!r}: only 'same' and 'center' are built")
        if not 0.0 <= momentum < 1.0:
            raise TtsAmdError(f'GriffinLim: momentum={momentum!r} outside [0, 1)')
        if not (isinstance(power, (int, float)) and power > 0):
            raise TtsAmdError(f'GriffinLim: power={power!r} is not a positive number')
        self.n_fft, self.n_iter, self.win_length, self.hop_length = n_fft, n_iter, 1024, 256
        self.power, self.momentum, self.length, self.rand_init, self.framing, self.seed = power, momentum, length, rand_init, framing, seed

    @torch.inference_mode()
    def forward(self, specgram, lens=None, seed=None):
        return griffinlim(specgram, None, self.n_fft, self.hop_length, self.win_length, self.power, self.n_iter, self.momentum,
                          self.length, self.rand_init, self.framing, self.seed if seed is None else seed, lens)


def mel_to_linear(mel, log=True, lens=None, fbank=None):
    """mel [..., n_mels, T] on the device -> magnitude [..., 513, T] = max(pinv(fbank) exp(mel), 1e-10) (log=False: mel is linear);
    fbank None = `MelSpectrogram`'s 80-band matrix, else [n_mels <= 128, 513] (a Vocos scale: pass its filterbank).  lens: FRAMES per
    row; what lies at or past them is zero.  The plain pseudo-inverse (float64 on the host, once per matrix), no NNLS refinement."""
    if not isinstance(mel, torch.Tensor) or mel.dim() < 2:
        raise TtsAmdError(f'mel_to_linear: mel of shape {tuple(getattr(mel, "shape", ()))}, expected [..., n_mels, T]')
    eng = _gl_engine(mel.device)
    lead = mel.shape[:-2]
    m3 = mel.reshape(-1, mel.shape[-2], mel.shape[-1])
    return eng.mel_to_linear(m3, lens, log=log, fbank=fbank).reshape(*lead, 513, mel.shape[-1])


def save_wav(path, wave, sample_rate=22_050, encoding='PCM_S', bits_per_sample=16):
    """wave: 1-D (or [1, n]) float tensor/array in [-1, 1].  'PCM_S' 16-bit (torchaudio.save's default for
    .wav from float32 is 32-bit float: pass encoding='PCM_F') -> little-endian RIFF/WAVE, mono.
    'ULAW' / 'ALAW' with bits_per_sample=8 (torchaudio's names): G.711, WAVE format 7 / 6 with an 18-byte fmt chunk and a fact chunk;
    wave is then float samples (encoded as `encode` does: PCM16 first) or uint8 data that is already encoded."""
    a = wave.detach().cpu().numpy() if hasattr(wave, 'detach') else np.asarray(wave)
    if encoding in ('ULAW', 'ALAW') and bits_per_sample == 8:
        from ttsamd import g711
        from ttsamd.stream import pcm16
        a = a.reshape(-1)
        if a.dtype != np.uint8:
            a = (g711.lin2ulaw if encoding == 'ULAW' else g711.lin2alaw)(pcm16(a))
        data = a.tobytes()
        fmt = struct.pack('<IHHIIHHH', 18, 7 if encoding == 'ULAW' else 6, 1, sample_rate, sample_rate, 1, 8, 0)
        body = b'WAVE' + b'fmt ' + fmt + b'fact' + struct.pack('<II', 4, len(data)) + b'data' + struct.pack('<I', len(data)) + data
        with open(path, 'wb') as f:
            f.write(b'RIFF' + struct.pack('<I', len(body) + (len(data) & 1)) + body + b'\0' * (len(data) & 1))
        return
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
    """Little-endian RIFF/WAVE -> (float32 array [n] in [-1, 1], sample_rate): 16-bit PCM (x / 32768), 32-bit float and 8-bit G.711
    (format 7 mu-law, 6 A-law: decoded to 16 bits, then x / 32768), what save_wav writes; several channels are averaged to one.  Anything else raises ValueError.  The samples come back at the file's own rate:
`load_recording` adds the resampler."""
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
    elif code in (6, 7) and bits == 8:
        a = decode(np.frombuffer(data, dtype=np.uint8), 'mulaw' if code == 7 else 'alaw')
    else:
        raise ValueError(f'{path}: format {code} with {bits} bits: 16-bit PCM, 32-bit float and 8-bit G.711 are read')
    if channels > 1:
        a = a[:len(a) // channels * channels].reshape(-1, channels).mean(axis=1).astype(np.float32)
    return a, int(rate)


def encode(wave, encoding, lens=None):
    """Device tensor [..., n] of float samples -> int16 ('pcm16': clip(rint(x * 32767)), save_wav's arithmetic) or uint8 G.711 bytes
    ('mulaw' | 'alaw', from that PCM16 value) of the same shape, on the device (ttsamd_wave_encode: the encoder of the streaming emit).
    lens (int64 [rows]): samples per row of a ragged batch; a row is zero behind its length.  Nothing is read back to the host."""
    import ctypes as C
    from ttsamd import lib as L
    from ttsamd.stream import ENCODINGS
    _device_wave(wave, 'encode')
    if encoding not in ('pcm16', 'mulaw', 'alaw'):
        raise ValueError(f"encode: encoding {encoding!r}: one of 'pcm16', 'mulaw', 'alaw'")
    x = wave.to(torch.float32).contiguous()
    shape = x.shape
    rows, n = (x.numel() // shape[-1] if shape[-1] else 0), shape[-1]
    out = torch.zeros(shape, dtype=torch.int16 if encoding == 'pcm16' else torch.uint8, device=x.device)
    if rows and n:
        if lens is not None:
            lens = torch.as_tensor(lens).to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
            if lens.numel() != rows:
                raise ValueError(f'encode: {lens.numel()} lengths for {rows} rows')
        with torch.cuda.device(x.device):
            L.check(L.load().ttsamd_wave_encode(C.c_void_p(x.data_ptr()), n, C.c_void_p(lens.data_ptr()) if lens is not None else None, rows,
                                                ENCODINGS[encoding], C.c_void_p(out.data_ptr()), n,
                                                C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'wave_encode')
    return out


def decode(data, encoding):
    """Host array or tensor of 'pcm16' (int16) or 'mulaw' / 'alaw' (uint8) data -> float32 numpy array, value / 32768 (load_wav's
    convention); the G.711 decoders are the standard's (ttsamd/g711.py)."""
    from ttsamd import g711
    a = data.detach().cpu().numpy() if hasattr(data, 'detach') else np.asarray(data)
    if encoding == 'pcm16':
        pcm = a.astype(np.int16)
    elif encoding in g711.DECODERS:
        pcm = g711.DECODERS[encoding](a.astype(np.uint8))
    else:
        raise ValueError(f"decode: encoding {encoding!r}: one of 'pcm16', 'mulaw', 'alaw'")
    return pcm.astype(np.float32) / np.float32(32768.0)


_resamplers, _trimmers = {}, {}


def _device_wave(x, what):
    if not isinstance(x, torch.Tensor) or x.device.type != 'cuda':
        raise TtsAmdError(f'{what}: expected a tensor on the ROCm device; the MI355X path has no CPU fallback (move it with .to("cuda"))')
    return x


def _resampler(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, device):
    """Checks the arguments; -> the cached engine, or None when the two rates are equal."""
    if resampling_method != 'sinc_interp_hann':
        raise TtsAmdError(f"resample: resampling_method {resampling_method!r}: only 'sinc_interp_hann' is built")
    try:
        ok = int(orig_freq) == orig_freq and int(new_freq) == new_freq and orig_freq > 0 and new_freq > 0 and lowpass_filter_width > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise TtsAmdError(f'resample: positive integer rates and a positive lowpass_filter_width are built (got {orig_freq}, {new_freq}, '
                          f'{lowpass_filter_width})')
    if int(orig_freq) == int(new_freq):
        return None
    key = (int(orig_freq), int(new_freq), int(lowpass_filter_width), float(rolloff), str(device))
    if key not in _resamplers:
        _resamplers[key] = ResampleEngine(*key[:4], device=device)
    return _resamplers[key]


def _trimmer(device):
    if str(device) not in _trimmers:
        _trimmers[str(device)] = TrimEngine(device=device)
    return _trimmers[str(device)]


def _level_rows(wave, lens, what):
    """-> (rows [R, n] float32 contiguous, a COPY the levelling kernels may write; lens int64 [R] on the device or None)"""
    _device_wave(wave, what)
    x = wave.to(torch.float32).reshape(-1, wave.shape[-1]).contiguous()
    if lens is not None:
        lens = torch.as_tensor(lens).to(device=x.device, dtype=torch.int64).reshape(-1).contiguous()
        if lens.numel() != x.shape[0]:
            raise ValueError(f'{what}: {lens.numel()} lengths for {x.shape[0]} rows')
    return x, lens


@torch.inference_mode()
def loudness(wave, sample_rate=22050, lens=None):
    """Integrated loudness (ITU-R BS.1770-4 / EBU R 128: K-weighting, 400 ms blocks every 100 ms, the absolute gate at -70 LUFS and the
    relative gate 10 LU under the gated mean) of every row of wave [..., n] -> float64 tensor [rows] in LUFS on the device; -inf for a
    row with no block above -70 LUFS.  A row shorter than 400 ms is measured as one block over its samples.  lens (int64 [rows]):
    samples per row of a ragged batch; nothing behind a row's length is read.  No host synchronisation."""
    x, lens = _level_rows(wave, lens, 'loudness')
    return _leveller(sample_rate, x.device).measure(x, lens)[0]


@torch.inference_mode()
def true_peak(wave, lens=None):
    """True peak of every row of wave [..., n] -> fp32 tensor [rows] on the device, linear: the largest magnitude among the samples and
    the three points between each sample and the next (and behind the last) of a 4x interpolation with a 25-tap Hann-windowed sinc
    (include/ttsamd.h states the arithmetic), in float64, rounded upward to fp32; 0 for an empty row.  The interpolator needs no rate.
    Specified by its arithmetic; parity with libebur128 / pyloudnorm is not pinned.  lens (int64 [rows]): samples per row of a ragged
    batch; nothing behind a row's length is read.  No host synchronisation."""
    x, lens = _level_rows(wave, lens, 'true_peak')
    return _leveller(22050, x.device).true_peak(x, lens)


@torch.inference_mode()
def true_peak_db(wave, lens=None):
    """`true_peak` in dBTP: 20 log10 of it as float64 [rows] on the device, -inf for a row of zeros or an empty row"""
    return 20.0 * torch.log10(true_peak(wave, lens).to(torch.float64))


def _level(wave, lens, sample_rate, mode, target, ceiling, what, true_peak=False):
    x, lens = _level_rows(wave, lens, what)
    if x.data_ptr() == wave.data_ptr():
        x = x.clone()                           # the caller's tensor stays as it is
    out, _ = _leveller(sample_rate, x.device).level(x, lens, mode, target, ceiling, **(dict(true_peak=True) if true_peak else {}))
    return out.reshape(wave.shape)


def _meter_rows(wave, lens, what, device=None):
    """`_level_rows`, and a list of 1-D waves (what `tts` returns) zero-padded to one batch as FastPitch2Wave._pad_waves pads"""
    if not isinstance(wave, (list, tuple)):
        return _level_rows(wave, lens, what)
    if lens is not None:
        raise ValueError(f'{what}: a list of waves carries its own lengths')
    rows = [torch.as_tensor(np.asarray(w) if not isinstance(w, torch.Tensor) else w).reshape(-1).float() for w in wave]
    if device is None:
        device = next((r.device for r in rows if r.device.type == 'cuda'), torch.device('cuda:0'))
    n = [int(r.numel()) for r in rows]
    out = torch.zeros(len(rows), max(n, default=0), dtype=torch.float32, device=device)
    for b, r in enumerate(rows):
        out[b, :n[b]] = r.to(device)
    return out, torch.tensor(n, dtype=torch.int64).to(device)


@torch.inference_mode()
def loudness_stats(wave, sample_rate=22050, lens=None):
    """The EBU R 128 figures of every row of wave [..., n] (or of a list of waves) -> dict of device tensors [rows]: integrated (LUFS,
    the bits of `loudness`), loudness_range (LU, EBU Tech 3342 on short-term values every 100 ms), max_momentary (400 ms windows),
    max_short_term (3 s windows; both -inf for a row too short to have one), peak (max |x|, fp32).  include/ttsamd.h states the
    arithmetic; it is specified by its arithmetic, parity with libebur128 unpinned (libebur128 takes its short-term blocks for the
    range at another hop).  lens as in `loudness`.  No host synchronisation."""
    x, lens = _meter_rows(wave, lens, 'loudness_stats')
    m = _leveller(sample_rate, x.device).meter(x, lens)
    return {k: m[k] for k in ('integrated', 'loudness_range', 'max_momentary', 'max_short_term', 'peak')}


@torch.inference_mode()
def momentary_loudness(wave, sample_rate=22050, lens=None):
    """Momentary loudness M (400 ms windows every 100 ms; one window over a row shorter than 400 ms) -> (values float64 [rows, J] on the
    device, NaN behind a row's own count; counts int64 [rows])"""
    x, lens = _meter_rows(wave, lens, 'momentary_loudness')
    m = _leveller(sample_rate, x.device).meter(x, lens, series=True)
    return m['momentary'], m['counts'][:, 0]


@torch.inference_mode()
def short_term_loudness(wave, sample_rate=22050, lens=None):
    """Short-term loudness S (3 s windows every 100 ms; none for a row shorter than 3 s) -> (values float64 [rows, JS] on the device,
    NaN behind a row's own count; counts int64 [rows])"""
    x, lens = _meter_rows(wave, lens, 'short_term_loudness')
    m = _leveller(sample_rate, x.device).meter(x, lens, series=True)
    return m['short_term'], m['counts'][:, 1]


def loudness_range(wave, sample_rate=22050, lens=None):
    """Loudness range (LRA, EBU Tech 3342) of every row -> float64 [rows] in LU on the device: `loudness_stats`'s loudness_range"""
    return loudness_stats(wave, sample_rate, lens)['loudness_range']


class LoudnessMeter:
    """Loudness of streams while they arrive: `max_streams` slots on the device, each measuring one stream of at most `max_seconds`.
    push(chunks [rows, n] or one chunk [n], lens, slots) -> dict(momentary, short_term, integrated) of float64 device tensors [rows]: the
    latest 400 ms and 3 s values (-inf before the first) and the integrated loudness of the stream so far; result(slots) -> dict(integrated,
    loudness_range, max_momentary, max_short_term, peak, counts, status) over the stream so far; reset(slots) starts a slot again.
    A stream's figures do not depend on which other slots share a push.  Against `loudness_stats` on the whole wave they agree within
    1e-9 LU (the peak exactly) for any chunking.  A push that would pass max_seconds is left out and flagged in status (bit 0)."""

    def __init__(self, sample_rate=22050, max_streams=32, max_seconds=600.0, device='cuda'):
        from ttsamd.engine import LoudnessMeter as _Meter
        self._m = _Meter(sample_rate, max_streams, max_seconds, device=device)
        self.sample_rate, self.max_streams, self.max_seconds = self._m.sample_rate, self._m.max_streams, float(max_seconds)

    @torch.inference_mode()
    def push(self, chunks, lens=None, slots=None):
        return self._m.push(_device_wave(chunks, 'LoudnessMeter.push'), lens, slots)

    @torch.inference_mode()
    def result(self, slots):
        return self._m.result(slots)

    @torch.inference_mode()
    def reset(self, slots):
        self._m.reset(slots)


def _level_capped(wave, lens, sample_rate, target_lufs, peak_ceiling, max_short_term, spec, true_peak):
    """normalize_loudness with the short-term cap of EBU R 128 s1: the row's target becomes min(target, L + max_short_term - maxS),
    worked out on the device from the meter's figures, and goes to ttsamd_wave_level / ttsamd_wave_limit as their per-row target"""
    import ctypes as C
    from ttsamd import lib as L
    check_finite([max_short_term], 'normalize_loudness max_short_term')
    x, lens = _level_rows(wave, lens, 'normalize_loudness')
    if x.data_ptr() == wave.data_ptr():
        x = x.clone()
    B, n_max = x.shape
    if not B:
        return x.reshape(wave.shape)
    targets = row_values(target_lufs, B, 'normalize_loudness target_lufs') if per_row(target_lufs) else [target_lufs] * B
    check_finite(targets, 'normalize_loudness target_lufs')
    eng = _leveller(sample_rate, x.device)
    lens_d = torch.full((B,), n_max, dtype=torch.int64, device=x.device) if lens is None else lens
    m = eng.meter(x, lens_d)
    target = torch.tensor([float(t) for t in targets], dtype=torch.float64).to(x.device)
    cap = m['integrated'] + (float(max_short_term) - m['max_short_term'])
    target = torch.where(torch.isfinite(cap), torch.minimum(target, cap), target).to(torch.float32)
    mode = torch.full((B,), 2, dtype=torch.int32, device=x.device)
    if spec is not None:
        attack, hold = limiter_samples(spec['attack_ms'], spec['hold_ms'], sample_rate)
        eng.limit_samples(x, lens_d, mode, target, spec['ceiling'], 10.0 ** (float(spec['max_gain_db']) / 20.0), attack, hold, m['integrated'],
                          **(dict(true_peak=True) if true_peak else {}))
        return x.reshape(wave.shape)
    if not 0.0 < float(peak_ceiling) <= 1.0:
        raise TtsAmdError(f'level: ceiling {peak_ceiling!r} is not in (0, 1]')
    peak = eng.true_peak(x, lens_d) if true_peak else m['peak']
    gain = torch.ones(B, dtype=torch.float32, device=x.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(x.device):
        L.check(L.load().ttsamd_wave_level(p(x), n_max, p(lens_d), B, p(mode), p(target), float(peak_ceiling), p(m['integrated']), p(peak),
                                           p(gain), C.c_void_p(torch.cuda.current_stream().cuda_stream)), 'wave_level')
    return x.reshape(wave.shape)


@torch.inference_mode()
def normalize_loudness(wave, sample_rate=22050, target_lufs=-23.0, peak_ceiling=0.99, lens=None, limiter=False, true_peak=False,
                       max_short_term=None):
    """Every row of wave [..., n] scaled by ONE gain to target_lufs (a float or one per row); where that would lift the row's peak
    above peak_ceiling, the gain is ceiling / peak instead (a cap on the gain, no limiter).  A silent row is returned as it is.  A new
    tensor on the device; the samples behind lens[row] are copied unchanged.
    limiter (True, or a dict with any of ceiling, attack_ms, hold_ms, max_gain_db): the full gain towards the target instead, and the
    look-ahead limiter (`limit`) holds the peaks at the ceiling (peak_ceiling unless the dict names one), so the target is reached.
    true_peak: the ceiling is a true-peak ceiling (dBTP as a linear value): the cap uses `true_peak` of the row, and the levelled row's
    true peak stays within peak_ceiling (1 + H 2^-24), H = 2.31 (the fp32 rounding of the output: include/ttsamd.h); with a limiter, its detector is the true-peak one (no exact bound: see `limit`).
    max_short_term (LUFS, e.g. -18.0: EBU R 128 s1 for short-form content): a row whose maximum short-term loudness would end above it
    is levelled to min(target, L + max_short_term - maxS) instead, worked out on the device with no synchronisation; None: the call as
    it was, bit for bit."""
    spec = limiter_spec(limiter)
    if spec is not None and not (isinstance(limiter, dict) and 'ceiling' in limiter):
        spec['ceiling'] = peak_ceiling
    if max_short_term is not None:
        return _level_capped(wave, lens, sample_rate, target_lufs, peak_ceiling, max_short_term, spec, true_peak)
    if spec is None:
        return _level(wave, lens, sample_rate, 2, target_lufs, peak_ceiling, 'normalize_loudness', true_peak)
    x, lens = _level_rows(wave, lens, 'normalize_loudness')
    if x.data_ptr() == wave.data_ptr():
        x = x.clone()
    out, _, _ = _leveller(sample_rate, x.device).limit(x, lens, 2, target_lufs, **spec, **(dict(true_peak=True) if true_peak else {}))
    return out.reshape(wave.shape)


@torch.inference_mode()
def limit(wave, gain_db=0.0, ceiling=0.99, attack_ms=1.5, hold_ms=15.0, sample_rate=22050, lens=None, true_peak=False):
    """A fixed gain and the look-ahead limiter (include/ttsamd.h states the arithmetic): every row of wave [..., n] times 10^(gain_db /
    20) (a float or one per row), then a gain-reduction curve in Q30 integers that looks attack_ms ahead, holds hold_ms and keeps
    |y| <= ceiling exactly; samples that no peak reaches are fl32(x g) bit for bit.  -> (a new tensor on the device, reduction_db
    float64 [rows] on the device: the deepest gain reduction in dB, 0 where nothing was limited).  The samples behind lens[row] are copied
    unchanged.  This is what a stream with `limiter=` applies to its windows: the concatenated chunks have the bits of this call on the
    whole wave.
    true_peak: the detector is max(|u[i]|, the 4x interpolator's values between i - 1 and i + 1) instead of |u[i]|, so a peak between
    two samples pulls the gain down as one on a sample does.  |y| <= ceiling still holds exactly; the true peak of y lands close to the
    ceiling but has no exact bound (the gain curve varies under the interpolator's 25 taps: DESIGN.md section 4 has the measured
    overshoot)."""
    x, lens = _level_rows(wave, lens, 'limit')
    if x.data_ptr() == wave.data_ptr():
        x = x.clone()
    if not 0.0 < float(ceiling) <= 1.0:
        raise ValueError(f'limit: ceiling {ceiling!r} is not in (0, 1]')
    B = x.shape[0]
    gains = row_values(gain_db, B, 'limit gain_db') if per_row(gain_db) else [gain_db] * B
    check_finite(gains, 'limit gain_db')
    attack, hold = limiter_samples(attack_ms, hold_ms, sample_rate)
    eng = _leveller(sample_rate, x.device)
    lens_d = torch.full((B,), x.shape[1], dtype=torch.int64, device=x.device) if lens is None else lens
    mode = torch.full((B,), 3, dtype=torch.int32, device=x.device)
    target = torch.tensor([float(v) for v in gains], dtype=torch.float32).to(x.device)
    out, _, red = eng.limit_samples(x, lens_d, mode, target, ceiling, LIMITER_NO_MAX_GAIN, attack, hold,
                                    **(dict(true_peak=True) if true_peak else {}))
    return out.reshape(wave.shape), 20.0 * torch.log10(red.to(torch.float64) / float(LIMITER_Q))


@torch.inference_mode()
def peak_normalize(wave, peak=0.99, lens=None, true_peak=False):
    """`peak_normalise` for a batch on the device: every row of wave [..., n] becomes x / max|x| * peak over its own samples (the bits
    of peak_normalise on that row); an all-zero row is returned as it is.  A new tensor on the device.
    true_peak: x / TP * peak with TP = `true_peak` of the row, so `peak` is where the true peak lands."""
    return _level(wave, lens, 22050, 1, peak, 0.99, 'peak_normalize', true_peak)


def resample(waveform, orig_freq, new_freq, lowpass_filter_width=6, rolloff=0.99, resampling_method='sinc_interp_hann', beta=None,
             lens=None, route='auto'):
    """torchaudio.functional.resample on the device: waveform [..., n] -> [..., ceil(n * new_freq / orig_freq)].  With `lens` (int64
    [rows]: samples per row of a ragged batch) it returns (wave, new_lens), new_lens on the device; every row is then the call on its
    own samples alone and is zero behind its new length.  Equal rates return the input unchanged.  Only 'sinc_interp_hann' is built."""
    _device_wave(waveform, 'resample')
    eng = _resampler(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, waveform.device)
    if lens is not None:
        lens = torch.as_tensor(lens).to(device=waveform.device, dtype=torch.int64)
    if eng is None:
        return waveform if lens is None else (waveform, lens)
    shape = waveform.shape
    out, nout = eng.forward(waveform.reshape(-1, shape[-1]), None if lens is None else lens.reshape(-1), route=route)
    out = out.reshape(shape[:-1] + (out.shape[-1],))
    return out if lens is None else (out, nout.reshape(lens.shape))


class Resample(nn.Module):
    """torchaudio.transforms.Resample's name and defaults over one ResampleEngine (the table is built once, at the first call on a
    device)."""

    def __init__(self, orig_freq: int = 16000, new_freq: int = 16000, resampling_method: str = 'sinc_interp_hann',
                 lowpass_filter_width: int = 6, rolloff: float = 0.99, beta=None):
        super().__init__()
        if resampling_method != 'sinc_interp_hann':
            raise TtsAmdError(f"Resample: resampling_method {resampling_method!r}: only 'sinc_interp_hann' is built")
        self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff = orig_freq, new_freq, lowpass_filter_width, rolloff
        self.resampling_method = resampling_method

    @torch.inference_mode()
    def forward(self, waveform, lens=None):
        return resample(waveform, self.orig_freq, self.new_freq, self.lowpass_filter_width, self.rolloff, self.resampling_method, lens=lens)


def trim(y, top_db=60, frame_length=2048, hop_length=512, lens=None):
    """librosa.effects.trim (ref = max) on the device.  One row [n]: (y[start:end], (start, end)) -- two integers, read from the device.
    A batch [B, n] (+ lens int64 [B]): bounds int64 [B, 2] on the device, no host read."""
    _device_wave(y, 'trim')
    eng = _trimmer(y.device)
    if y.dim() == 1:
        bounds, _ = eng.bounds(y[None], None, top_db, frame_length, hop_length)
        start, end = (int(v) for v in bounds[0].tolist())
        return y[start:end], (start, end)
    bounds, _ = eng.bounds(y, lens, top_db, frame_length, hop_length)
    return bounds


@torch.inference_mode()
def join_waves(waves, lens=None, pause_ms=350.0, trim_db=40.0, keep_ms=10.0, fade_ms=5.0, sample_rate=22050):
    """Several waves -> one, on the device (csrc/join.hip; include/ttsamd.h states the arithmetic): every wave is cut to its speech
    bounds (librosa.effects.trim's at trim_db with frame 1024 / hop 256, widened by keep_ms on each side; trim_db=None: the waves whole),
    faded in and out over fade_ms by a raised cosine, and followed by its pause.  waves: a list of 1-D tensors / arrays (host or
    device, any lengths) or a tensor [B, n] with lens int64 [B].  pause_ms: one value = the pause BETWEEN two waves (none behind the
    last), or one value per wave (the last: trailing silence); a negative pause asks for that much overlap with the next wave, which
    is overlap-added over at most the fade's length and half of either wave.  -> (wave [N] float32 on the device, segs int64 [B, 4] on
    the host = (out_start, out_end, src_start, src_end) per wave).  One read-back: the total length and the segment table."""
    from ttsamd.join import fade_table, join_rows, ms_to_samples
    if isinstance(waves, (list, tuple)):
        if lens is not None:
            raise ValueError('join_waves: lens goes with a [B, n] tensor; a list of waves carries its own lengths')
        if not waves:
            raise ValueError('join_waves: no waves')
        rows = [(w if isinstance(w, torch.Tensor) else torch.as_tensor(np.asarray(w))).reshape(-1) for w in waves]
        dev = next((r.device for r in rows if r.device.type == 'cuda'), torch.device('cuda:0'))
        n = [int(r.numel()) for r in rows]
        x = torch.zeros(len(rows), max(max(n), 1), dtype=torch.float32, device=dev)
        for b, r in enumerate(rows):
            x[b, :n[b]] = r.to(device=dev, dtype=torch.float32)
        lens = torch.tensor(n, dtype=torch.int64).to(dev)
    else:
        x = _device_wave(waves, 'join_waves')
        if x.dim() != 2:
            raise ValueError(f'join_waves: a list of waves or a tensor [B, n] (+ lens), got shape {tuple(x.shape)}')
        x = x.to(torch.float32).contiguous()
    B = x.shape[0]
    pauses = row_values(pause_ms, B, 'pause_ms') if per_row(pause_ms) else [pause_ms] * (B - 1) + [0.0]
    check_finite(pauses, 'pause_ms')
    gaps = [ms_to_samples(p, sample_rate) for p in pauses]
    bounds = None
    if trim_db is not None:
        bounds, _ = _trimmer(x.device).bounds(x, lens, float(trim_db), 1024, 256, gain=0.0)
    out, segs = join_rows(x, lens, gaps, bounds, keep=ms_to_samples(keep_ms, sample_rate), fade=fade_table(ms_to_samples(fade_ms, sample_rate)))
    return out[0], segs


@torch.inference_mode()
def prepare_recording(wave, sample_rate, lens=None, sr_target=22050, lowpass_filter_width=1024, peak=0.999, top_db=23, frame_length=1024,
                      hop_length=256, tail_silence=768):
    """The reference's recording clean-up (scripts/preprocess_audio.py:33-47) for a batch on the device: resample to sr_target, scale
    each row to the peak `peak` (x / max|x| * peak), trim leading and trailing silence (librosa.effects.trim at top_db on the scaled
    row), append tail_silence zeros.  wave [B, n] (or [n]), lens int64 [B] -> (wave [B, width], lens int64 [B]) on the device, width =
    the resampled width + tail_silence; rows are zero behind their length.  No host synchronisation."""
    _device_wave(wave, 'prepare_recording')
    x = wave.reshape(-1, wave.shape[-1])
    if lens is None:
        lens = torch.full((x.shape[0],), x.shape[1], dtype=torch.int64, device=x.device)
    x, n = resample(x, sample_rate, sr_target, lowpass_filter_width, lens=lens)
    eng = _trimmer(x.device)
    bounds, pk = eng.bounds(x, n, top_db, frame_length, hop_length, gain=peak)
    return eng.apply(x, bounds, pk, gain=peak, tail=tail_silence, out_width=x.shape[1] + int(tail_silence))


def load_recording(path, sr_target=22050, device='cuda'):
    """load_wav + resample: a wav file at any rate -> float32 tensor [n] at sr_target on the device (torchaudio's default filter)."""
    a, rate = load_wav(path)
    return resample(torch.from_numpy(a).to(device), rate, sr_target)
