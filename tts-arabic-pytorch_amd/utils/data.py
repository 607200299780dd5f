"""Data-preparation helpers with the reference's names (utils/data.py:50-67): `remove_silence`, `normalize_pitch`, and the batched
device call `drop_silent_frames` = remove_silence(mel_log.mean(0)) followed by mel_log[:, keep] / pitch[:, keep] for every row of a
batch in one launch (csrc/trim.hip)."""
import torch

from ttsamd.engine import TrimEngine
from ttsamd.lib import TtsAmdError

_engines = {}


def remove_silence(energy_per_frame: torch.Tensor, thresh: float = -10.0):
    """1-D energies -> bool mask of the frames to keep: those above `thresh` and every frame behind the last of them; with no frame
    above the threshold all but frame 0 (what the reference's backward loop leaves)."""
    keep = energy_per_frame > thresh
    above = torch.nonzero(keep)
    keep[(int(above[-1]) + 1 if above.numel() else 1):] = True
    return keep


def normalize_pitch(pitch, mean: float = 130.05478, std: float = 22.86267):
    """In place: (pitch - mean) / std on the voiced frames, unvoiced ones (0) stay 0."""
    unvoiced = pitch == 0.0
    pitch.sub_(mean).div_(std)
    pitch[unvoiced] = 0.0
    return pitch


def drop_silent_frames(mel_log, lens=None, thresh=-10.0, extra=None):
    """mel_log [B, C, T] on the device (+ lens int64 [B], + extra [B, C2, T], e.g. the pitch track) -> (mel, lens) or (mel, extra, lens):
    per row the frames remove_silence(mel_log[b, :, :lens[b]].mean(0), thresh) keeps, moved to the front bit for bit, zeros behind the
    new length.  No host read."""
    if not isinstance(mel_log, torch.Tensor) or mel_log.device.type != 'cuda':
        raise TtsAmdError('drop_silent_frames: expected a tensor on the ROCm device; the MI355X path has no CPU fallback')
    key = str(mel_log.device)
    if key not in _engines:
        _engines[key] = TrimEngine(device=mel_log.device)
    mel, ext, new_lens = _engines[key].compact(mel_log, lens, thresh, extra)
    return (mel, new_lens) if extra is None else (mel, ext, new_lens)
