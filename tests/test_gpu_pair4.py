"""GPU (pytest -m gpu): the C = 32 fused c1 -> c2 ResBlock1 pair with both convs on Winograd F(4,3) (csrc/resblock_pair4.hip),
through the C ABI (ttsamd_resblock_pair variant 6) against the reference's ops (vocoder/hifigan/models.py:46-53) in float64, and inside
the whole generator at its default routing against the oracle and against the F(2,3) pair it replaces (TTSAMD_PAIR4=0)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import WAVE_TOL

pytestmark = pytest.mark.gpu


def _ref_pair(x, w1, b1, w2, b2, dil, lens, slope=0.1):
    """per utterance on its exact length, float64"""
    k = w1.shape[2]
    out = torch.zeros_like(x, dtype=torch.float64)
    for b, n in enumerate(lens):
        if n == 0:
            continue
        xb = x[b:b + 1, :, :n].double()
        t = F.conv1d(F.leaky_relu(xb, slope), w1.double(), b1.double(), dilation=dil, padding=(k * dil - dil) // 2)
        t = F.conv1d(F.leaky_relu(t, slope), w2.double(), b2.double(), padding=(k - 1) // 2)
        out[b, :, :n] = (xb + t)[0]
    return out


def _ts(k, d):
    """outputs per block: 128 quads at dilation d = whole groups of 4 d intermediate columns, minus the halo, a multiple of 4"""
    return (4 * (512 // (4 * d)) * d - (k - 1)) & ~3


@pytest.mark.parametrize('k', [3, 7, 11])
@pytest.mark.parametrize('dil', [1, 3, 5])
def test_pair4_kernel_vs_float64(k, dil):
    from ttsamd.engine import resblock_pair
    dev = torch.device('cuda:0')
    C = 32
    g = torch.Generator().manual_seed(7000 + 10 * k + dil)
    ts = _ts(k, dil)
    # around one and two blocks, one ending inside the halo of a block edge, one shorter than k, a length that is not a multiple of 4, empty
    lens = [2 * ts + 8, ts + 4, ts - 4, ts, ts + 2, 4, 2, 0, 3 * ts - 12]
    Lx = max(lens)
    x = torch.randn(len(lens), C, Lx, generator=g)
    w1 = torch.randn(C, C, k, generator=g) / np.sqrt(C * k)
    w2 = torch.randn(C, C, k, generator=g) / np.sqrt(C * k)
    b1, b2 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    ref = _ref_pair(x, w1, b1, w2, b2, dil, lens)
    xd, lens_d = x.to(dev), torch.tensor(lens, device=dev)
    args = (xd, w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev), dil)
    y = resblock_pair(*args, lens=lens_d, variant=6)
    torch.cuda.synchronize()
    y = y.cpu()
    for b, n in enumerate(lens):
        err = float((y[b, :, :n].double() - ref[b, :, :n]).abs().max()) if n else 0.0
        assert err < 2e-5, (k, dil, b, n, err)
        assert n == Lx or float(y[b, :, n:].abs().max()) == 0.0                 # nothing is written past the utterance
    prev = torch.randn(len(lens), C, Lx, generator=g)
    for mode, div in ((1, 1.0), (2, 3.0)):
        ya = resblock_pair(*args, lens=lens_d, y=prev.to(dev).clone(), mode=mode, div=div, variant=6).cpu()
        for b, n in enumerate(lens):
            want = (prev[b, :, :n].double() + ref[b, :, :n]) / div
            assert n == 0 or float((ya[b, :, :n].double() - want).abs().max()) < 2e-5, (mode, b)
            assert torch.equal(ya[b, :, n:], prev[b, :, n:])                     # untouched past the utterance
    assert torch.equal(resblock_pair(*args, lens=lens_d, variant=6).cpu(), y)     # run-to-run bit determinism


def test_pair4_len_mul_and_full_batch():
    """lens in mel frames with len_mul (how the generator calls it), and lens = NULL"""
    from ttsamd.engine import resblock_pair
    dev = torch.device('cuda:0')
    g = torch.Generator().manual_seed(31)
    C, k, dil = 32, 11, 3
    frames, mul = [5, 2, 7], 256
    Lx = max(frames) * mul
    x = torch.randn(3, C, Lx, generator=g)
    w1, w2 = torch.randn(C, C, k, generator=g) / np.sqrt(C * k), torch.randn(C, C, k, generator=g) / np.sqrt(C * k)
    b1, b2 = torch.randn(C, generator=g) * 0.1, torch.randn(C, generator=g) * 0.1
    args = (x.to(dev), w1.to(dev), b1.to(dev), w2.to(dev), b2.to(dev), dil)
    y = resblock_pair(*args, lens=torch.tensor(frames, device=dev), len_mul=mul, variant=6).cpu()
    assert float((y.double() - _ref_pair(x, w1, b1, w2, b2, dil, [f * mul for f in frames])).abs().max()) < 2e-5
    y = resblock_pair(*args, variant=6).cpu()
    assert float((y.double() - _ref_pair(x, w1, b1, w2, b2, dil, [Lx] * 3)).abs().max()) < 2e-5


def test_pair4_entry_rejects_what_it_cannot_run():
    from ttsamd.engine import resblock_pair
    from ttsamd.lib import TtsAmdError
    dev = torch.device('cuda:0')
    x = torch.randn(1, 64, 64, device=dev)
    w, b = torch.randn(64, 64, 3, device=dev), torch.zeros(64, device=dev)
    with pytest.raises(TtsAmdError, match='variant 6'):
        resblock_pair(x, w, b, w, b, 1, variant=6)                                                 # C = 64: not built
    x = torch.randn(1, 32, 64, device=dev)
    w, b = torch.randn(32, 32, 3, device=dev), torch.zeros(32, device=dev)
    with pytest.raises(TtsAmdError, match='unsupported geometry'):
        resblock_pair(x, w, b, w, b, 2, variant=6)                                                 # dilation 2
    with pytest.raises(TtsAmdError, match='unsupported geometry'):
        resblock_pair(x[:, :, :62].contiguous(), w, b, w, b, 1, variant=6)                         # L % 4 != 0


@pytest.fixture(scope='module')
def vocoder_case(synth_weights):
    """a ragged batch big enough for the default routing to take the fused pairs (B x L >= kFused2SmallColumns at the C = 32 stage)"""
    import tts_oracle as O
    from ttsamd.config import HIFIGAN_CONFIG
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(12)
    lens = [160, 151, 97, 133]
    mel = (rng.standard_normal((4, 80, 160)) * 1.5 - 4.0).astype(np.float32)
    hw = {k: v.to(dev) for k, v in O.fold_weight_norm(synth_weights['hifigan']).items()}
    with torch.backends.cudnn.flags(enabled=False), torch.inference_mode():
        ref = O.hifigan_forward_ragged(hw, torch.from_numpy(mel).to(dev), torch.tensor(lens).to(dev), HIFIGAN_CONFIG).cpu()
    return {'dev': dev, 'mel': mel, 'lens': lens, 'ref': ref}


def _vocode(synth_weights, case):
    from ttsamd.engine import HifiGanEngine
    dev = case['dev']
    wave = HifiGanEngine(synth_weights['hifigan'], device=dev).forward(torch.from_numpy(case['mel']).to(dev),
                                                                       torch.tensor(case['lens']).to(dev))
    torch.cuda.synchronize()
    return wave.cpu()


def test_hifigan_default_routing_with_pair4_vs_oracle(synth_weights, vocoder_case, ttsopt):
    """default routing (the C = 32 pairs on resblock_pair4) against the oracle, and against TTSAMD_PAIR4=0 (resblock_pair2)"""
    from ttsamd import lib
    assert lib.get_option('TTSAMD_PAIR4') in (None, '1')
    wave = _vocode(synth_weights, vocoder_case)
    ttsopt.set('TTSAMD_PAIR4', '0')
    wave23 = _vocode(synth_weights, vocoder_case)
    worst = worst23 = 0.0
    for b, n in enumerate(vocoder_case['lens']):
        ref = vocoder_case['ref'][b, :256 * n]
        worst = max(worst, float((wave[b, :256 * n] - ref).abs().max()))
        worst23 = max(worst23, float((wave23[b, :256 * n] - ref).abs().max()))
        assert 256 * n == wave.shape[1] or float(wave[b, 256 * n:].abs().max()) == 0.0
    diff = float((wave - wave23).abs().max())
    print(f'\nwave max-abs vs oracle: F(4,3) pairs {worst:.2e}, F(2,3) pairs {worst23:.2e}; between them {diff:.2e}')
    assert worst < WAVE_TOL and worst23 < WAVE_TOL
    assert diff > 0.0                # the switch really changes the kernel
    assert diff < 1e-5
