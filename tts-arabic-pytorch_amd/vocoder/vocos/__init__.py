"""Drop-in for the inference part of the reference's vendored Vocos
(vocoder/vocos/pretrained.py:34-97 `MelVocos`, configs '22k' and '24k' of vocoder/vocos/__init__.py:8-67):
mel -> waveform through the HIP ConvNeXt backbone + ISTFT head, and waveform -> log-mel through the HIP analysis kernel
(`feature_extractor`, `reconstruct`).  '22k': 80 slaney bands, "same" framing; '24k' (the published Vocos mel checkpoint's geometry):
100 HTK bands, "center" framing.  The reference never wires it to FastPitch; `FastPitch2Wave`-style use is:
`wave = vocos(mel_batch, denoise=0.)`.  The constructor default is '22k' here ('24k' in the reference): INTEGRATION.md."""
import numpy as np
import torch

from ttsamd.config import VOCOS_22K_CONFIG, VOCOS_24K_CONFIG
from ttsamd.engine import VocosEngine
from ttsamd.lib import TtsAmdError
from vocoder.hifigan.models import _HipModule
from vocoder.vocos.feature_extractors import MelSpectrogramFeatures

config_22k = dict(VOCOS_22K_CONFIG)
config_24k = dict(VOCOS_24K_CONFIG)


class MelVocos(_HipModule):
    def __init__(self, config_name='22k'):
        super().__init__()
        if config_name not in ('22k', '24k'):
            raise TtsAmdError(f"MelVocos({config_name!r}): only '22k' (80 mel bands, 22.05 kHz) and '24k' (100 bands, 24 kHz) are built")
        self.config = {'22k': config_22k, '24k': config_24k}[config_name]
        self.feature_extractor = MelSpectrogramFeatures(**self.config['feature_extractor'])
        self.n_mels = self.config['input_channels']
        # the rate of the wave: 22 050 / 24 000 Hz ('22k''s feature extractor keeps the reference's 24 000, which is not it)
        self.sampling_rate = self.config['sample_rate']
        self._sd = None

    def load_state_dict(self, state_dict, strict=True):
        self._sd = {k: (v.detach().cpu().float().numpy() if hasattr(v, 'detach') else np.asarray(v, np.float32))
                    for k, v in state_dict.items() if k.startswith(('backbone.', 'head.out.'))}
        self._engines.clear()

    def state_dict(self, *a, **k):
        return {k_: torch.from_numpy(v) for k_, v in (self._sd or {}).items()}

    def engine(self):
        if self._sd is None:
            raise TtsAmdError('MelVocos has no weights: call load_state_dict first')
        return self._engine(lambda dev: VocosEngine(self._sd, self.config, device=dev))

    @property
    def bias_vec(self):
        return self.engine().bias_vec()

    @torch.inference_mode()
    def forward(self, mel_spec, denoise=0., lens=None):
        """mel_spec [B, n_mels, frames] -> wave [B, 256*frames] ('22k'; pretrained.py:73-93) or [B, 256*(frames-1)] ('24k')."""
        eng = self.engine()
        if self.config['padding'] == 'center' and mel_spec.shape[-1] < 2:
            # torch.istft(center=True) of a single frame has no sample left after trimming n_fft / 2 per side and raises
            raise ValueError("MelVocos('24k'): the centred ISTFT needs at least 2 frames (got %d)" % mel_spec.shape[-1])
        return eng.forward(mel_spec, lens, denoise)

    def stream(self, mel, chunk_frames=64, first_chunk_frames=32, pcm16=False, denoise=0.0, sample_rate=None, encoding=None):
        """Extension (ttsamd.stream), as Generator.stream: mel [n_mels, T] -> a generator of device chunks whose concatenation is
        forward(mel, denoise)'s 256 T ('22k') or 256 (T - 1) ('24k') samples, the first after first_chunk_frames frames of work plus
        the halo instead of T.  sample_rate / encoding ('float32' | 'pcm16' | 'mulaw' | 'alaw'): the chunks leave resampled to that rate
        and encoded (StreamingVocoder).  A chunk stays valid until the one after next has been taken."""
        from ttsamd.stream import StreamingVocoder
        sv = StreamingVocoder(self, max_streams=1, max_frames=int(mel.shape[-1]), chunk_frames=chunk_frames,
                              first_chunk_frames=first_chunk_frames, pcm16=pcm16, sample_rate=sample_rate, encoding=encoding)
        sv.open(mel, denoise)
        while sv.open_streams:
            for _, chunk, _ in sv.step():
                yield chunk

    @torch.inference_mode()
    def reconstruct(self, wave, denoise=0., lens=None):
        """wave [B, n] -> forward(feature_extractor(wave), denoise) (pretrained.py:95-97).  `lens` int64 [B] (extension): samples per
        row of a ragged batch; the frame counts go from the analysis kernel to the vocoder on the device, no host read in between."""
        self.engine()                                   # (a module left on the CPU raises before any work)
        mel, frames = self.feature_extractor.extract(wave, lens)
        return self.forward(mel, denoise, frames)
