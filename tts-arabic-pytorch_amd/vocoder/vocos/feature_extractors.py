"""Drop-in for vocoder/vocos/feature_extractors.py:28-64 (`MelSpectrogramFeatures`): log-mel of a waveform, one HIP launch
(csrc/melspec.hip).  torchaudio's MelSpectrogram(power=1) is restated as |STFT| (periodic hann, reflect) times the ttsamd.melfb matrix."""
import torch

from ttsamd import melfb
from ttsamd.lib import TtsAmdError
from utils.audio import _MelModule


class FeatureExtractor(_MelModule):
    """Base class for feature extractors."""


class MelSpectrogramFeatures(FeatureExtractor):
    _mag, _what = 'abs', 'MelSpectrogramFeatures'

    def __init__(self, sample_rate=24000, n_fft=1024, hop_length=256, n_mels=100, padding="center",
                 f_min: float = 0, f_max: float = None, norm: str = None, mel_scale: str = "htk"):
        super().__init__()
        if padding not in ["center", "same"]:
            raise ValueError("Padding must be 'center' or 'same'.")
        if n_fft != 1024 or hop_length != 256 or not 1 <= n_mels <= 128:
            raise TtsAmdError(f'MelSpectrogramFeatures(n_fft={n_fft}, hop_length={hop_length}, n_mels={n_mels}): only n_fft = 1024, '
                              'hop_length = 256, n_mels <= 128 is built')
        self.padding = padding
        self._framing = padding
        self.clip_val = 1e-5
        self._log_clip = self.clip_val
        self.sample_rate, self.n_fft, self.hop_length, self.n_mels = sample_rate, n_fft, hop_length, n_mels
        self.register_buffer('mel_basis', torch.from_numpy(melfb.mel_filterbank(sample_rate, n_fft, n_mels, f_min, f_max, norm, mel_scale)))

    @torch.inference_mode()
    def forward(self, audio, lens=None, **kwargs):
        """audio [B, n] -> log(max(mel, 1e-5)) [B, n_mels, frames]: n // 256 ('same') or n // 256 + 1 ('center')."""
        mel, _ = self.extract(audio, lens)
        return mel[0] if audio.dim() == 1 else mel
