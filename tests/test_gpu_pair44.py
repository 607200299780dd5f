"""GPU (pytest -m gpu): the C = 32 fused c1 -> c2 ResBlock1 pair with both convs on the SEVEN-point groups of Winograd F(4,3)
(csrc/resblock_pair4.hip, PT_ = 7: 13 / 20 products per output quad at k = 7 / 11), through the C ABI (ttsamd_resblock_pair variant 7)
against the reference's ops (vocoder/hifigan/models.py:46-53) in float64 and beside the six-point launch (variant 6) on the same data, and
inside the whole generator under TTSAMD_PAIR4 = 1 (default) / 2 (six-point groups) / 0 (resblock_pair2) against the oracle.

Variant 7 packs its filters from the raw ones with the values and the layout of the host packing the generator uses
(pack_wino44_weight at 32 x 32: [4][NG][2][32][4]); a wrong layout in either shows as an error of order 1 here."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, WAVE_TOL
from test_gpu_pair4 import _ref_pair, _ts

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('k', [7, 11])
@pytest.mark.parametrize('dil', [1, 3, 5])
def test_pair44_kernel_vs_float64(k, dil):
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
    y = resblock_pair(*args, lens=lens_d, variant=7)
    y6 = resblock_pair(*args, lens=lens_d, variant=6)
    torch.cuda.synchronize()
    y, y6 = y.cpu(), y6.cpu()
    errs = [float((y[b, :, :n].double() - ref[b, :, :n]).abs().max()) if n else 0.0 for b, n in enumerate(lens)]
    errs6 = [float((y6[b, :, :n].double() - ref[b, :, :n]).abs().max()) if n else 0.0 for b, n in enumerate(lens)]
    print(f'\nk={k} d={dil}: worst max-abs vs float64: seven-point (variant 7) {max(errs):.2e}, six-point (variant 6) {max(errs6):.2e}')
    for b, n in enumerate(lens):
        assert errs[b] < 2e-5, (k, dil, b, n, errs[b])
        assert errs6[b] < 2e-5, (k, dil, b, n, errs6[b])
        assert n == Lx or float(y[b, :, n:].abs().max()) == 0.0                 # nothing is written past the utterance
    assert not torch.equal(y, y6)                                                # another arithmetic, not the same launch
    prev = torch.randn(len(lens), C, Lx, generator=g)
    for mode, div in ((1, 1.0), (2, 3.0)):
        ya = resblock_pair(*args, lens=lens_d, y=prev.to(dev).clone(), mode=mode, div=div, variant=7).cpu()
        for b, n in enumerate(lens):
            want = (prev[b, :, :n].double() + ref[b, :, :n]) / div
            assert n == 0 or float((ya[b, :, :n].double() - want).abs().max()) < 2e-5, (mode, b)
            assert torch.equal(ya[b, :, n:], prev[b, :, n:])                     # untouched past the utterance
    assert torch.equal(resblock_pair(*args, lens=lens_d, variant=7).cpu(), y)     # run-to-run bit determinism


def test_pair44_len_mul_and_full_batch():
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
    y = resblock_pair(*args, lens=torch.tensor(frames, device=dev), len_mul=mul, variant=7).cpu()
    assert float((y.double() - _ref_pair(x, w1, b1, w2, b2, dil, [f * mul for f in frames])).abs().max()) < 2e-5
    y = resblock_pair(*args, variant=7).cpu()
    assert float((y.double() - _ref_pair(x, w1, b1, w2, b2, dil, [Lx] * 3)).abs().max()) < 2e-5


def test_pair44_entry_rejects_what_it_cannot_run():
    from ttsamd.engine import resblock_pair
    from ttsamd.lib import TtsAmdError
    dev = torch.device('cuda:0')
    x = torch.randn(1, 64, 64, device=dev)
    w, b = torch.randn(64, 64, 7, device=dev), torch.zeros(64, device=dev)
    with pytest.raises(TtsAmdError, match='variant 7'):
        resblock_pair(x, w, b, w, b, 1, variant=7)                                                 # C = 64: not built
    x = torch.randn(1, 32, 64, device=dev)
    w, b = torch.randn(32, 32, 3, device=dev), torch.zeros(32, device=dev)
    with pytest.raises(TtsAmdError, match='variant 7'):
        resblock_pair(x, w, b, w, b, 1, variant=7)                                                 # k = 3: no seven-point form


@pytest.fixture(scope='module')
def vocoder_case(synth_weights):
    """the ragged batch of test_gpu_pair4.py: big enough for the default routing to take the fused pairs"""
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


def test_hifigan_pair4_routings_vs_oracle(synth_weights, vocoder_case, ttsopt):
    """TTSAMD_PAIR4 = 1 (default: seven-point groups where routed), 2 (six-point groups: the launch before them) and 0 (resblock_pair2)
    against the oracle; the default differs from = 2, and by rounding only"""
    from ttsamd import lib
    from ttsamd.engine import HifiGanEngine
    dev = vocoder_case['dev']
    assert lib.get_option('TTSAMD_PAIR4') in (None, '1')
    eng = HifiGanEngine(synth_weights['hifigan'], device=dev)
    mel, lens = torch.from_numpy(vocoder_case['mel']).to(dev), torch.tensor(vocoder_case['lens']).to(dev)
    waves = {}
    for opt in (None, '2', '0'):
        if opt is not None:
            ttsopt.set('TTSAMD_PAIR4', opt)
        waves[opt] = eng.forward(mel, lens).cpu()
    worst = {}
    for opt, wave in waves.items():
        worst[opt] = 0.0
        for b, n in enumerate(vocoder_case['lens']):
            worst[opt] = max(worst[opt], float((wave[b, :256 * n] - vocoder_case['ref'][b, :256 * n]).abs().max()))
            assert 256 * n == wave.shape[1] or float(wave[b, 256 * n:].abs().max()) == 0.0
    diff = float((waves[None] - waves['2']).abs().max())
    print(f"\nwave max-abs vs oracle: default {worst[None]:.2e}, TTSAMD_PAIR4=2 {worst['2']:.2e}, =0 {worst['0']:.2e}; "
          f'default against =2 {diff:.2e}')
    assert all(v < WAVE_TOL for v in worst.values())
    assert 0.0 < diff < 1e-5


_ROUTE_CHILD = r'''
import sys
sys.path[:0] = [%r, %r]
import numpy as np, torch
from ttsamd import lib, synth
from ttsamd.engine import HifiGanEngine
dev = torch.device('cuda:0')
rng = np.random.default_rng(12)
mel = torch.from_numpy((rng.standard_normal((4, 80, 160)) * 1.5 - 4.0).astype(np.float32)).to(dev)
lens = torch.tensor([160, 151, 97, 133]).to(dev)
eng = HifiGanEngine(synth.hifigan_state_dict(), device=dev)
for opt in (None, 2):
    if opt is not None:
        lib.set_option('TTSAMD_PAIR4', opt)
    with open(sys.argv[1], 'a') as f:
        f.write('# PAIR4=%%s\n' %% opt)
    eng.forward(mel, lens)
    torch.cuda.synchronize()
print('ROUTES OK')
'''


def test_route_log_names_the_pair_form(tmp_path):
    """TTSAMD_CONV_LOG (opened once per process, hence the child): under the default the C = 32 k = 7 / 11 pairs are logged as
    fused_pair44 (seven-point groups), under TTSAMD_PAIR4=2 as fused_pair4; six launches per forward either way"""
    log = tmp_path / 'conv_log.csv'
    code = _ROUTE_CHILD % (os.path.join(REPO, 'tts-arabic-pytorch_amd'), os.path.join(REPO, 'oracle'))
    p = subprocess.run([sys.executable, '-c', code, str(log)], capture_output=True, timeout=300,
                       env=dict(os.environ, TTSAMD_CONV_LOG=str(log)))
    assert p.returncode == 0 and b'ROUTES OK' in p.stdout, p.stderr.decode()[-3000:]
    runs, cur = {}, None
    for ln in log.read_text().splitlines():
        if ln.startswith('# PAIR4='):
            cur = runs.setdefault(ln[len('# PAIR4='):], [])
        elif cur is not None and ln.startswith('fused_pair4'):
            f = ln.split(',')
            cur.append((f[0], int(f[1]), int(f[2])))
    want_k = [7] * 3 + [11] * 3
    assert sorted(runs['None']) == [('fused_pair44', k, 32) for k in want_k], runs['None']
    assert sorted(runs['2']) == [('fused_pair4', k, 32) for k in want_k], runs['2']
