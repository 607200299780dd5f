"""Generate tests/golden/melspec.npz and tests/golden/vocos_24k.npz with the REAL reference's analysis modules and MelVocos('24k').
Run manually where the reference tree is readable (oracle/_refstub.py: TTS_REFERENCE):  python tools/gen_golden_melspec.py

What runs is the reference's own code: utils/audio.py MelSpectrogram.forward, vocoder/vocos/feature_extractors.py
MelSpectrogramFeatures.forward (both Vocos configs) and vocoder/vocos/pretrained.py MelVocos('24k') forward / bias_vec / reconstruct.
The two third-party pieces that are no dependency of this project are stand-ins, installed in sys.modules after oracle/_refstub.py:
  librosa.filters.mel                    -> ttsamd.melfb.mel_filterbank(..., mel_scale='slaney')   (librosa's htk=False default)
  torchaudio.transforms.MelSpectrogram   -> torch.stft with torchaudio's documented defaults (periodic hann, center -> reflect padding,
                                            onesided, unnormalised, power = 1) times ttsamd.melfb's matrix
so the filterbank VALUES are pinned to the published formulas only (parity unpinned).  The fixtures hold inputs and the
reference's outputs, plus the sha256 digest of the synthetic 24k weights; no weights and no code.
"""
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'oracle'))
import gen_golden as gg  # noqa: E402  (loads our synth / config by path and installs the reference, as for the other goldens)

melfb = gg._load_pkg_module('ttsamd.melfb', ('ttsamd', 'melfb.py'))

import torch  # noqa: E402


def _install_standins():
    librosa, filters = types.ModuleType('librosa'), types.ModuleType('librosa.filters')

    def mel(sr, n_fft, n_mels=128, fmin=0.0, fmax=None, htk=False, norm='slaney'):
        return melfb.mel_filterbank(sr, n_fft, n_mels, fmin, fmax, norm, 'htk' if htk else 'slaney')

    filters.mel = mel
    librosa.filters = filters
    sys.modules['librosa'], sys.modules['librosa.filters'] = librosa, filters

    class MelSpectrogram(torch.nn.Module):
        def __init__(self, sample_rate=16000, n_fft=400, win_length=None, hop_length=None, f_min=0.0, f_max=None, pad=0, n_mels=128,
                     power=2.0, normalized=False, center=True, pad_mode='reflect', norm=None, mel_scale='htk'):
            super().__init__()
            assert pad == 0 and not normalized
            self.n_fft, self.win_length = n_fft, win_length or n_fft
            self.hop_length = hop_length or self.win_length // 2
            self.power, self.center, self.pad_mode = power, center, pad_mode
            self.register_buffer('window', torch.hann_window(self.win_length))
            self.register_buffer('fb', torch.from_numpy(melfb.mel_filterbank(sample_rate, n_fft, n_mels, f_min, f_max, norm, mel_scale)))

        def forward(self, x):
            spec = torch.stft(x, self.n_fft, self.hop_length, self.win_length, self.window, center=self.center, pad_mode=self.pad_mode,
                              normalized=False, onesided=True, return_complex=True).abs().pow(self.power)
            return torch.matmul(self.fb, spec)

    sys.modules['torchaudio.transforms'].MelSpectrogram = MelSpectrogram


def voiced(n, seed, sr=22050):
    """A voiced-like test signal: harmonics of f0 in [100, 240] Hz up to 10 kHz with amplitudes U(0.3, 1) / h, peak 0.5, a 3 Hz
    tremolo, white noise of sigma 3e-3 (the family tests/test_gpu_melspec.py uses)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = rng.uniform(100.0, 240.0)
    x = np.zeros(n)
    for h in range(1, int(10000 // f0) + 1):
        x += rng.uniform(0.3, 1.0) / h * np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi))
    x *= 0.5 / np.abs(x).max()
    x *= 1.0 + 0.3 * np.sin(2 * np.pi * 3.0 * t)
    return (x + 3e-3 * rng.standard_normal(n)).astype(np.float32)


def main():
    _install_standins()
    from utils.audio import MelSpectrogram
    from vocoder.vocos import config_22k, config_24k
    from vocoder.vocos.feature_extractors import MelSpectrogramFeatures
    from vocoder.vocos.pretrained import MelVocos

    ms = MelSpectrogram()
    fe22 = MelSpectrogramFeatures(**config_22k['feature_extractor']['init_args'])
    fe24 = MelSpectrogramFeatures(**config_24k['feature_extractor']['init_args'])
    out = {}
    for i, (n, seed) in enumerate(((5000, 101), (3333, 102))):
        w = torch.from_numpy(voiced(n, seed))[None]
        out[f'wave_{i}'] = w[0].numpy()
        out[f'mel_audio_{i}'] = ms(w)[0].numpy()              # utils.audio.MelSpectrogram: linear mel, sqrt(|X|^2 + 1e-9)
        out[f'feat_22k_{i}'] = fe22(w)[0].numpy()             # MelSpectrogramFeatures: log(max(mel, 1e-5))
        out[f'feat_24k_{i}'] = fe24(w)[0].numpy()
        print(n, out[f'mel_audio_{i}'].shape, out[f'feat_22k_{i}'].shape, out[f'feat_24k_{i}'].shape,
              'min linear mel', float(out[f'mel_audio_{i}'].min()))
    path = os.path.join(REPO, 'tests', 'golden', 'melspec.npz')
    np.savez_compressed(path, **out)
    print(f'melspec: {os.path.getsize(path) / 1024:.1f} kB')

    cfg = gg.config.VOCOS_24K_CONFIG
    for k in ('input_channels', 'dim', 'intermediate_dim', 'num_layers'):
        assert config_24k['backbone']['init_args'][k] == cfg[k], k
    assert config_24k['head']['init_args']['padding'] == cfg['padding'] == 'center'
    assert {k: v for k, v in cfg['feature_extractor'].items()} == config_24k['feature_extractor']['init_args']
    assert gg.config.VOCOS_22K_CONFIG['feature_extractor'] == config_22k['feature_extractor']['init_args']
    with torch.enable_grad():
        mv = MelVocos('24k')
    vsd = gg.synth.vocos_state_dict(cfg)
    full = {k: v for k, v in mv.state_dict().items() if k not in vsd}      # window / feature-extractor buffers
    full.update(gg.t(vsd))
    mv.load_state_dict(full)                                               # post-hook recomputes bias_vec
    mv.eval()
    rng = np.random.default_rng(23)
    vg = {'digest': np.array(gg.sd_digest(vsd)), 'bias_vec': mv.bias_vec.numpy()}
    with torch.no_grad():
        for T in (2, 5, 24):
            mel = torch.from_numpy((rng.standard_normal((2, 100, T)) * 1.5 - 4.0).astype(np.float32))
            vg[f'mel_T{T}'] = mel.numpy()
            vg[f'wave_T{T}'] = mv(mel).numpy()
            vg[f'wave_dn_T{T}'] = mv(mel, denoise=0.3).numpy()
            print(T, tuple(vg[f'wave_T{T}'].shape), 'abs max', float(np.abs(vg[f'wave_T{T}']).max()))
        w = torch.from_numpy(voiced(3000, 103, sr=24000))[None]
        vg['recon_in'] = w.numpy()
        vg['recon_out'] = mv.reconstruct(w).numpy()
        vg['recon_dn_out'] = mv.reconstruct(w, denoise=0.3).numpy()
        print('reconstruct', tuple(vg['recon_out'].shape), 'bias max', float(mv.bias_vec.max()))
    path = os.path.join(REPO, 'tests', 'golden', 'vocos_24k.npz')
    np.savez_compressed(path, **vg)
    print(f'vocos_24k: {os.path.getsize(path) / 1024:.1f} kB')


if __name__ == '__main__':
    main()
