"""Vocoder loaders of the drop-in surface.

`load_hifigan(state_dict_path, config_file)` keeps the reference's signature
(vocoder/__init__.py:3): it returns a callable mel -> waveform module.  Here the module is
the HIP generator (vocoder.hifigan.models.Generator): the checkpoint's weight-normalised
tensors are handed to the C ABI as they are, which folds g*v/||v|| itself.
"""
import json


def _read_generator_checkpoint(path):
    import torch
    ckpt = torch.load(path, map_location='cpu')
    if 'generator' not in ckpt:
        raise KeyError(f"{path}: expected a HiFi-GAN checkpoint with a 'generator' entry")
    return ckpt['generator']


def load_hifigan(state_dict_path, config_file):
    from vocoder.hifigan.env import AttrDict
    from vocoder.hifigan.models import Generator

    with open(config_file, 'r') as fh:
        hparams = AttrDict(json.load(fh))
    vocoder = Generator(hparams, state_dict=_read_generator_checkpoint(state_dict_path))
    return vocoder.eval()


def load_griffinlim(n_iter=32, momentum=0.99, seed=0):
    """The vocoder that needs no checkpoint (vocoder.griffinlim.GriffinLimVocoder): the HiFi-GAN analysis's log-mel -> wave by the
    pseudo-inverse of the filterbank and `n_iter` Griffin-Lim iterations on the device."""
    from vocoder.griffinlim import GriffinLimVocoder
    return GriffinLimVocoder(n_iter=n_iter, momentum=momentum, seed=seed).eval()
