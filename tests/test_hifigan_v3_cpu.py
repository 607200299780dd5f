"""CPU: HiFi-GAN V3 (ResBlock2) -- a float64 restatement of the reference generator pinned to its golden
(tests/golden/hifigan_v3.npz, tools/gen_golden_hifigan_v3.py), the synthetic V3 weights, and the ABI 8 surface.
The GPU tests (test_gpu_hifigan_v3.py) compare the HIP generator against the same restatement."""
import hashlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

LRELU_SLOPE = 0.1


def digest(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


def fold(sd, base):
    """float64 weight of `base`: `<base>.weight`, or g * v / ||v|| (norm over all dims but 0)."""
    if base + '.weight' in sd:
        return torch.from_numpy(np.asarray(sd[base + '.weight'], np.float64))
    g = np.asarray(sd[base + '.parametrizations.weight.original0'], np.float64)
    v = np.asarray(sd[base + '.parametrizations.weight.original1'], np.float64)
    n = np.sqrt((v ** 2).sum(axis=tuple(range(1, v.ndim)), keepdims=True))
    return torch.from_numpy(g * v / n)


def bias(sd, base):
    return torch.from_numpy(np.asarray(sd[base + '.bias'], np.float64))


def resblock2_f64(x, w1, b1, w2, b2, d1, d2):
    """x [B, C, L] float64: the reference ResBlock2.forward (vocoder/hifigan/models.py:62-83) on one exact-length utterance."""
    for w, b, d in ((w1, b1, d1), (w2, b2, d2)):
        k = w.shape[2]
        x = F.conv1d(F.leaky_relu(x, LRELU_SLOPE), w, b, dilation=d, padding=(k * d - d) // 2) + x
    return x


def generator_f64(sd, h, mel):
    """mel [80, T] (one exact-length utterance) -> wave [256 T] in float64: Generator.forward with ResBlock2 blocks."""
    x = torch.as_tensor(np.asarray(mel, np.float64))[None]
    x = F.conv1d(x, fold(sd, 'conv_pre'), bias(sd, 'conv_pre'), padding=3)
    nk = len(h['resblock_kernel_sizes'])
    for i, (u, k) in enumerate(zip(h['upsample_rates'], h['upsample_kernel_sizes'])):
        x = F.leaky_relu(x, LRELU_SLOPE)
        x = F.conv_transpose1d(x, fold(sd, f'ups.{i}'), bias(sd, f'ups.{i}'), stride=u, padding=(k - u) // 2)
        xs = None
        for j in range(nk):
            r = i * nk + j
            d = h['resblock_dilation_sizes'][j]
            y = resblock2_f64(x, fold(sd, f'resblocks.{r}.convs.0'), bias(sd, f'resblocks.{r}.convs.0'),
                              fold(sd, f'resblocks.{r}.convs.1'), bias(sd, f'resblocks.{r}.convs.1'), d[0], d[1])
            xs = y if xs is None else xs + y
        x = xs / nk
    x = F.leaky_relu(x)                                 # default slope 0.01
    x = torch.tanh(F.conv1d(x, fold(sd, 'conv_post'), bias(sd, 'conv_post'), padding=3))
    return x[0, 0].numpy()


@pytest.fixture(scope='module')
def v3():
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_V3_CONFIG
    return HIFIGAN_V3_CONFIG, synth.hifigan_state_dict(HIFIGAN_V3_CONFIG, seed=0)


def test_v3_config_is_the_published_table():
    from ttsamd.config import HIFIGAN_V3_CONFIG as h
    assert h['resblock'] == '2' and h['upsample_initial_channel'] == 256
    assert h['upsample_rates'] == [8, 8, 4] and h['upsample_kernel_sizes'] == [16, 16, 8] and int(np.prod(h['upsample_rates'])) == 256
    assert h['resblock_kernel_sizes'] == [3, 5, 7] and h['resblock_dilation_sizes'] == [[1, 2], [2, 6], [3, 12]]
    assert (h['num_mels'], h['n_fft'], h['hop_size'], h['sampling_rate']) == (80, 1024, 256, 22050)


def test_v3_synthetic_weights_match_the_golden_digest(golden, v3):
    _, sd = v3
    assert digest(sd) == str(golden('hifigan_v3')['digest'])
    assert 'resblocks.8.convs.1.parametrizations.weight.original1' in sd and not any('convs1' in k for k in sd)
    # the folded form carries the same tensors as `.weight`
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_V3_CONFIG
    folded = synth.hifigan_state_dict(HIFIGAN_V3_CONFIG, seed=0, weight_norm=False)
    w = folded['resblocks.4.convs.0.weight']
    assert w.shape == (64, 64, 5)
    np.testing.assert_allclose(w, fold(sd, 'resblocks.4.convs.0').numpy(), rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize('T', [1, 7, 40])
def test_f64_restatement_matches_reference_golden(golden, v3, T):
    h, sd = v3
    g = golden('hifigan_v3')
    want = g[f'wave_T{T}'].reshape(-1)
    got = generator_f64(sd, h, g[f'mel_T{T}'])
    assert got.shape == want.shape == (256 * T,)
    assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()


def test_abi8_cfg_ends_with_resblock():
    from ttsamd import lib
    assert lib.ABI_VERSION == 8
    assert lib.HifiGanCfg._fields_[-1][0] == 'resblock'
    assert lib.SYMBOLS['ttsamd_resblock2'][1][6:10] == [lib._I32] * 4
    assert 'ttsamd_resblock2_packed_floats' in lib.SYMBOLS


def test_v3_generator_has_no_cpu_path(v3):
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    from ttsamd.lib import TtsAmdError
    from vocoder.hifigan.models import Generator
    h, sd = v3
    g = Generator(dict(h), state_dict={k: torch.from_numpy(v) for k, v in sd.items()})
    with pytest.raises(TtsAmdError):
        g(torch.zeros(80, 4))
