"""CPU: the mel analysis (utils.audio.MelSpectrogram, MelSpectrogramFeatures), the filterbanks of ttsamd.melfb and MelVocos('24k')
against the goldens made with the real reference (tools/gen_golden_melspec.py) and against the published formulas; no GPU work."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import MEL_TOL
import melspec_ref as R


def maxabs(a, b):
    a, b = (np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (a, b))
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


def test_float64_restatement_reproduces_the_reference_goldens(golden):
    """The yardstick of the GPU tests (melspec_ref.mel_ref in float64) against what the reference's own modules gave in fp32.
    Linear mel: max-abs error relative to the largest value <= 1e-6 (fp32 through a 1024-point FFT and a sum of <= 31 products: a few
    eps = 6e-8; the reference in fp32 measures 1.7e-7 on such signals).  Log-mel: the project's MEL_TOL."""
    g = golden('melspec')
    for i in (0, 1):
        w = g[f'wave_{i}']
        lin = R.mel_ref(w, R.fbank('audio'), 'same', 1)[0]
        assert lin.shape == g[f'mel_audio_{i}'].shape == (80, len(w) // 256)
        assert maxabs(lin, g[f'mel_audio_{i}']) <= 1e-6 * float(lin.max())
        f22 = R.mel_ref(w, R.fbank('v22k'), 'same', 0, 1e-5)[0]
        assert f22.shape == (80, len(w) // 256) and maxabs(f22, g[f'feat_22k_{i}']) < MEL_TOL
        f24 = R.mel_ref(w, R.fbank('v24k'), 'center', 0, 1e-5)[0]
        assert f24.shape == (100, len(w) // 256 + 1) and maxabs(f24, g[f'feat_24k_{i}']) < MEL_TOL


@pytest.mark.parametrize('name', ['audio', 'v22k', 'v24k'])
def test_filterbank_shape_and_triangles(name):
    a = R.FB_ARGS[name]
    fb = R.fbank(name)
    assert fb.shape == (a['n_mels'], 513) and fb.dtype == np.float32
    assert (fb >= 0).all() and np.isfinite(fb).all()
    assert (fb.sum(axis=1) > 0).all(), 'an empty band'
    for m, row in enumerate(fb):
        nz = np.flatnonzero(row)
        assert (np.diff(nz) == 1).all(), f'band {m}: support is not one interval'
        seg = row[nz[0]:nz[-1] + 1].astype(np.float64)
        k = int(seg.argmax())
        assert (np.diff(seg[:k + 1]) > 0).all() and (np.diff(seg[k:]) < 0).all(), f'band {m}: not a single triangle'


def test_band_edges_follow_the_published_scales():
    from ttsamd import melfb
    # HTK: f = 700 (10^(m / 2595) - 1), edges equally spaced in mel between 0 and sr / 2
    e = melfb.band_edges(24000, 100, 0, None, 'htk')
    m = np.linspace(0.0, 2595.0 * np.log10(1.0 + 12000.0 / 700.0), 102)
    assert np.allclose(e, 700.0 * (10.0 ** (m / 2595.0) - 1.0), rtol=1e-12, atol=1e-9)
    assert e[0] == 0.0 and abs(e[-1] - 12000.0) < 1e-8
    # Slaney: linear (200 / 3 Hz per mel) below 1 kHz, log(6.4) / 27 per mel above
    e = melfb.band_edges(22050, 80, 0, 8000.0, 'slaney')
    mel = np.linspace(0.0, 15.0 + np.log(8.0) / (np.log(6.4) / 27.0), 82)
    lo, hi = mel < 15.0, mel >= 15.0
    assert np.allclose(e[lo], mel[lo] * 200.0 / 3.0, rtol=1e-12)
    assert np.allclose(np.diff(np.log(e[hi])), (mel[1] - mel[0]) * np.log(6.4) / 27.0, rtol=1e-10)
    assert abs(e[-1] - 8000.0) < 1e-8
    # Slaney area norm: the un-normalised triangle (peak 1 at its centre edge) times 2 / (f[m + 2] - f[m])
    plain = melfb.mel_filterbank(22050, 1024, 80, 0, 8000.0, None, 'slaney', dtype=np.float64)
    normed = melfb.mel_filterbank(22050, 1024, 80, 0, 8000.0, 'slaney', 'slaney', dtype=np.float64)
    assert np.allclose(normed, plain * (2.0 / (e[2:] - e[:-2]))[:, None], rtol=1e-12, atol=0)
    freqs = np.linspace(0, 11025.0, 513)
    tri = np.maximum(0, np.minimum((freqs[None] - e[:-2, None]) / (e[1:-1] - e[:-2])[:, None],
                                   (e[2:, None] - freqs[None]) / (e[2:] - e[1:-1])[:, None]))
    assert np.allclose(plain, tri, rtol=1e-12, atol=1e-15)
    with pytest.raises(ValueError):
        melfb.mel_filterbank(22050, 1024, 80, mel_scale='bark')


def test_vocos_24k_restatement_matches_the_reference_golden(golden):
    """MelVocos('24k') of the reference vs the fp32 restatement (the oracle's backbone and bias vector, torch.istft(center=True)),
    within the bound test_vocos_22k holds the oracle to: 1e-6 on bias_vec and on the waves, with and without denoise."""
    import tts_oracle as O
    from ttsamd import synth
    from ttsamd.config import VOCOS_24K_CONFIG as cfg
    g = golden('vocos_24k')
    w = synth.vocos_state_dict(cfg)
    assert w['backbone.embed.weight'].shape == (512, 100, 7)
    h = hashlib.sha256()
    for k in sorted(w):
        h.update(k.encode())
        h.update(np.ascontiguousarray(w[k]).tobytes())
    assert h.hexdigest() == str(g['digest']), 'synthetic 24k Vocos weights differ from the golden run'
    bias = O.vocos_bias_vec(w, cfg)
    assert maxabs(bias, g['bias_vec']) < 1e-6
    for T in (2, 5, 24):
        assert g[f'wave_T{T}'].shape == (2, 256 * (T - 1))
        assert maxabs(R.vocos24_ref(w, g[f'mel_T{T}'], cfg, bias_vec=bias), g[f'wave_T{T}']) < 1e-6
        assert maxabs(R.vocos24_ref(w, g[f'mel_T{T}'], cfg, denoise=0.3, bias_vec=bias), g[f'wave_dn_T{T}']) < 1e-6
    # reconstruct = forward(feature_extractor(wave)): the analysis in fp32, as the reference ran it
    feat = R.mel_ref(g['recon_in'], R.fbank('v24k'), 'center', 0, 1e-5, dtype=torch.float32)
    assert maxabs(R.vocos24_ref(w, feat, cfg, bias_vec=bias), g['recon_out']) < 1e-6
    assert maxabs(R.vocos24_ref(w, feat, cfg, denoise=0.3, bias_vec=bias), g['recon_dn_out']) < 1e-6


def test_new_symbols_are_bound_and_the_abi_revision_stays():
    from ttsamd import lib
    for name in ('ttsamd_melspec_create', 'ttsamd_melspec_destroy', 'ttsamd_melspec_forward', 'ttsamd_vocos_set_padding'):
        assert name in lib.SYMBOLS
        assert getattr(lib.load(), name) is not None
    assert lib.ABI_VERSION == 8 == lib.load().ttsamd_version()


def test_configs_and_public_surface():
    from ttsamd.config import VOCOS_22K_CONFIG, VOCOS_24K_CONFIG
    from utils.audio import MelSpectrogram
    from vocoder.vocos import MelVocos, config_22k, config_24k
    from vocoder.vocos.feature_extractors import MelSpectrogramFeatures
    assert config_24k == VOCOS_24K_CONFIG and config_22k == VOCOS_22K_CONFIG
    assert VOCOS_24K_CONFIG['input_channels'] == 100 and VOCOS_24K_CONFIG['padding'] == 'center'
    assert VOCOS_22K_CONFIG['feature_extractor']['sample_rate'] == 24000          # the reference's quirk, kept
    ms = MelSpectrogram()
    assert ms.mel_basis.shape == (80, 513) and ms.window_fn.shape == (1024,) and ms.pad_length == 384
    assert np.array_equal(ms.mel_basis.numpy(), R.fbank('audio'))
    assert torch.equal(ms.window_fn, torch.hann_window(1024))
    for name, fbn, nm in (('22k', 'v22k', 80), ('24k', 'v24k', 100)):
        v = MelVocos(name)
        assert v.n_mels == nm and isinstance(v.feature_extractor, MelSpectrogramFeatures)
        assert np.array_equal(v.feature_extractor.mel_basis.numpy(), R.fbank(fbn))
    assert MelVocos().n_mels == 80                                                # the default stays '22k' 
    with pytest.raises(ValueError):
        MelSpectrogramFeatures(padding='valid')


def test_geometries_that_are_not_built_raise_at_construction():
    from ttsamd.lib import TtsAmdError
    from utils.audio import MelSpectrogram
    from vocoder.vocos import MelVocos
    from vocoder.vocos.feature_extractors import MelSpectrogramFeatures
    for kw in (dict(n_fft=2048), dict(n_fft=512, win_length=512), dict(hop_length=128), dict(center=True), dict(n_mels=129),
               dict(win_length=800)):
        with pytest.raises(TtsAmdError):
            MelSpectrogram(**kw)
    for kw in (dict(n_fft=2048), dict(hop_length=300), dict(n_mels=129)):
        with pytest.raises(TtsAmdError):
            MelSpectrogramFeatures(**kw)
    with pytest.raises(TtsAmdError):
        MelVocos('44k')


def test_modules_on_the_cpu_raise_instead_of_falling_back():
    """There is no CPU path: a module that was not moved to the GPU raises TtsAmdError, with or without a GPU in the box."""
    from ttsamd import synth
    from ttsamd.config import VOCOS_24K_CONFIG
    from ttsamd.lib import TtsAmdError
    from utils.audio import MelSpectrogram
    from vocoder.vocos import MelVocos
    x = torch.from_numpy(R.voiced(2000, 1))[None]
    with pytest.raises(TtsAmdError):
        MelSpectrogram()(x)
    v = MelVocos('24k')
    v.load_state_dict({k: torch.from_numpy(a) for k, a in synth.vocos_state_dict(VOCOS_24K_CONFIG).items()})
    with pytest.raises(TtsAmdError):
        v(torch.zeros(1, 100, 8))
    with pytest.raises(TtsAmdError):
        v.feature_extractor(x)
    with pytest.raises(TtsAmdError):
        v.reconstruct(x)
    # too-short inputs are refused on the host, before any device work, worded like the Denoiser's check
    with pytest.raises(ValueError, match='more than 384 samples'):
        MelSpectrogram()(torch.zeros(1, 384))
    with pytest.raises(ValueError, match='more than 512 samples'):
        v.feature_extractor(torch.zeros(2, 600), lens=torch.tensor([600, 512]))
