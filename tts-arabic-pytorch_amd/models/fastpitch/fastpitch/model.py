"""Drop-in for the reference's models/fastpitch/fastpitch/model.py -- for now `average_pitch(pitch, durs)` and `mask_from_lens` ONLY.
The FastPitch class of that file (forward's 12-tuple, losses, gradients) is not built here: inference and forced alignment are
models.fastpitch.networks.FastPitch (.infer / .align), regulate_len is ttsamd.engine.length_regulate.

average_pitch runs in ttsamd_average_pitch (csrc/aligner.hip): each token's frames are summed directly instead of as the difference of two
fp32 cumulative sums, so values agree with the reference within its own rounding noise, not bit for bit.  No CPU fallback."""
from typing import Optional

import torch

from ttsamd import engine as _engine


def mask_from_lens(lens, max_len: Optional[int] = None):
    """lens [B] -> bool [B, max_len] (max_len None: the longest row), True on each row's first lens[b] positions"""
    n = int(lens.max()) if max_len is None else max_len
    return torch.arange(n, device=lens.device, dtype=lens.dtype)[None, :] < lens[:, None]


def average_pitch(pitch, durs):
    """pitch [B, F, T], durs [B, L] on the device -> [B, F, L]: per token the mean of the non-zero values of its frames, 0 where none"""
    return _engine.average_pitch(pitch, durs)
