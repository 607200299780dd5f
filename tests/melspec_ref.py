"""Shared by tests/test_melspec_cpu.py and tests/test_gpu_melspec.py (not a test module): the float64 restatement of the reference's
mel analysis, the three built filterbank configurations and the voiced-like test signals."""
import numpy as np
import torch

MIN_SAMPLES = {'same': 385, 'center': 513}
# the three built configurations: utils.audio.MelSpectrogram, MelSpectrogramFeatures of config_22k (sample_rate 24000: the reference's quirk)
# and of config_24k
FB_ARGS = {
    'audio': dict(sample_rate=22050, n_fft=1024, n_mels=80, f_min=0, f_max=8000.0, norm='slaney', mel_scale='slaney'),
    'v22k': dict(sample_rate=24000, n_fft=1024, n_mels=80, f_min=0, f_max=8000, norm='slaney', mel_scale='slaney'),
    'v24k': dict(sample_rate=24000, n_fft=1024, n_mels=100, f_min=0, f_max=None, norm=None, mel_scale='htk'),
}


def fbank(name):
    from ttsamd import melfb
    return melfb.mel_filterbank(**FB_ARGS[name])


def mel_ref(wave, fb, framing, mag_mode, log_clip=None, dtype=torch.float64):
    """utils/audio.py:35-46 and feature_extractors.py:58-64 restated: reflect pad (384 per side, or torch.stft's own 512 with
    center=True), torch.stft with the periodic hann window, |X| (mag_mode 0) or sqrt(|X|^2 + 1e-9) (1), filterbank, log(max(., clip)).
    wave [n] or [B, n]; fb [n_mels, 513] float32 (the values the kernel gets), cast to `dtype`."""
    x = torch.as_tensor(np.asarray(wave)).to(dtype)
    x = x[None] if x.dim() == 1 else x
    win = torch.hann_window(1024, dtype=dtype)
    if framing == 'same':
        x = torch.nn.functional.pad(x[:, None], (384, 384), mode='reflect')[:, 0]
    spec = torch.stft(x, 1024, 256, 1024, win, center=framing == 'center', pad_mode='reflect', normalized=False, onesided=True,
                      return_complex=True)
    mag = spec.abs().pow(2).add(1e-9).sqrt() if mag_mode else spec.abs()
    mel = torch.matmul(torch.as_tensor(fb).to(dtype), mag)
    return torch.log(torch.clamp(mel, min=log_clip)) if log_clip else mel


def voiced(n, seed, sr=22050):
    """Voiced-like signal, so that no mel value sits near the log clip: harmonics of a random f0 in [100, 240] Hz up to 10 kHz with
    amplitudes U(0.3, 1) / h, peak-normalised to 0.5, a 3 Hz tremolo, white noise of sigma 3e-3."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr
    f0 = rng.uniform(100.0, 240.0)
    x = np.zeros(n)
    for h in range(1, int(10000 // f0) + 1):
        x += rng.uniform(0.3, 1.0) / h * np.sin(2 * np.pi * h * f0 * t + rng.uniform(0, 2 * np.pi))
    x *= 0.5 / np.abs(x).max()
    x *= 1.0 + 0.3 * np.sin(2 * np.pi * 3.0 * t)
    return (x + 3e-3 * rng.standard_normal(n)).astype(np.float32)


def vocos24_ref(w, mel, cfg, denoise=0.0, bias_vec=None, dtype=torch.float32):
    """MelVocos('24k').forward restated (pretrained.py:73-93 over spectral_ops.py:44-46): the oracle's backbone, then
    torch.istft(center=True).  mel [B, 100, T] -> wave [B, 256 (T - 1)]."""
    import tts_oracle as O
    import torch.nn.functional as F
    W = {k: torch.as_tensor(np.asarray(v)).to(dtype) for k, v in w.items()}
    feats = O._vocos_backbone(W, torch.as_tensor(np.asarray(mel)).to(dtype), cfg['num_layers'])
    xo = F.linear(feats, W['head.out.weight'], W['head.out.bias']).transpose(1, 2)
    mag, ph = xo.chunk(2, dim=1)
    mag = torch.exp(mag)
    if bias_vec is None:
        bias_vec = O.vocos_bias_vec(w, cfg, dtype)
    mag = torch.clamp(mag - denoise * torch.as_tensor(bias_vec).to(dtype), min=0., max=1e2)
    S = mag * (torch.cos(ph) + 1j * torch.sin(ph))
    return torch.istft(S, cfg['n_fft'], cfg['hop_length'], cfg['n_fft'], torch.hann_window(cfg['n_fft'], dtype=dtype), center=True)
