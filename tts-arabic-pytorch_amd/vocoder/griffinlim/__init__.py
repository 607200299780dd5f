"""A vocoder without weights: the log-mel of the HiFi-GAN analysis -> wave by the pseudo-inverse of the filterbank and Griffin-Lim
(csrc/griffinlim.hip).  It takes and returns what vocoder.hifigan.models.Generator takes and returns, so it stands wherever a Generator
does that needs no stream: `utils.objective.copy_synthesis(GriffinLimVocoder(), wave)` gives the Griffin-Lim row of a vocoder table,
and FastPitch2Wave / Tacotron2Wave(..., vocoder='griffin_lim') synthesise without a vocoder checkpoint.
Specified by its arithmetic; parity with a torchaudio release is not pinned (the random initial phase is the project's own hash)."""
import torch

from ttsamd.engine import GriffinLimEngine
from ttsamd.lib import TtsAmdError
from vocoder.hifigan.models import _HipModule


class _MelGriffinLim:
    """What GriffinLimVocoder.engine() returns: forward(mel [B, 80, T], lens) -> wave [B, 256 T], the call HifiGanEngine.forward answers"""

    hop = 256

    def __init__(self, device, n_iter, momentum, seed):
        self.gl = GriffinLimEngine(device=device)
        self.device, self.n_iter, self.momentum, self.seed = self.gl.device, n_iter, momentum, seed

    def forward(self, mel, lens=None):
        """mel: log-mel [B, 80, T] (`same` framing); lens: frames per row (any integer tensor / list) or None.  Rows as if alone; zeros
        at and past 256 * lens[b]."""
        if mel.dim() != 3 or mel.shape[1] != 80:
            raise TtsAmdError(f'GriffinLimVocoder: mel of shape {tuple(mel.shape)}, expected [B, 80, T]')
        if isinstance(lens, torch.Tensor):
            lens = lens.to(torch.int32)
        mag = self.gl.mel_to_linear(mel, lens, log=True)
        return self.gl.forward(mag, lens, n_iter=self.n_iter, momentum=self.momentum, framing='same', init='hash', seed=self.seed)


class NoDenoiser(torch.nn.Module):
    """Stands where vocoder.hifigan.denoiser.Denoiser stands in FastPitch2Wave / Tacotron2Wave(vocoder='griffin_lim'): the bias denoiser
    subtracts HiFi-GAN's own artefact (its output for a zero mel), which a Griffin-Lim wave does not have, so every strength is taken
    as 0 and the wave is handed back as it is."""

    def forward(self, wave, strength=0.0):
        return wave

    def forward_batch(self, wave, nsamples, strength=0.0, nsamples_min=None):
        return wave


class GriffinLimVocoder(_HipModule):
    def __init__(self, n_iter: int = 32, momentum: float = 0.99, seed: int = 0):
        super().__init__()
        if int(n_iter) != n_iter or n_iter < 0:
            raise TtsAmdError(f'GriffinLimVocoder: n_iter={n_iter!r} is not an integer >= 0')
        if not 0.0 <= momentum < 1.0:
            raise TtsAmdError(f'GriffinLimVocoder: momentum={momentum!r} outside [0, 1)')
        self.n_iter, self.momentum, self.seed = int(n_iter), float(momentum), int(seed)

    def remove_weight_norm(self):
        """No-op: there are no weights."""

    def engine(self):
        return self._engine(lambda dev: _MelGriffinLim(dev, self.n_iter, self.momentum, self.seed))

    @torch.inference_mode()
    def forward(self, x, lens=None):
        """x [80, T] -> [1, 256 T], or [B, 80, T] -> [B, 1, 256 T]; `lens` (frames per row) makes the batch ragged: Generator.forward's
        shapes."""
        eng = self.engine()
        if x.dim() == 2:
            return eng.forward(x[None])
        return eng.forward(x, lens)[:, None, :]

    def stream(self, *a, **k):
        raise ValueError('GriffinLimVocoder: streaming is out of scope (every iteration needs the whole utterance)')
