"""GPU parity of the seven-point groups of the F(4,3) kernel (csrc/conv_wino4.hip, Wino4Geo PT_ = 7; TTSAMD_WINO4 bits 5 / 6) through
the C ABI (pytest -m gpu): k = 7 as 7 + 6 = 13 products per output quad, k = 11 as 7 + 7 + 6 = 20, against 16 / 23 of the six-point groups.

Checker, lengths and epilogues are those of tests/test_gpu_wino.py::test_wino_decomposition_k3_k7_k11 (its k = 7 / 11 rows: the smallest
shapes that still reach this kernel): torch conv1d in float64 on the host (HiFi-GAN's ResBlock convs, vocoder/hifigan/models.py:30-53),
ragged lengths L, L - 1 (a quad cut by the utterance end), 131 (cut inside a quad) and 1,
positions past an utterance untouched.  Every case runs with TTSAMD_WINO4=111 (seven-point groups) and =15 (six-point groups, today's
kernel) on the same input:
    both within 5e-5 max-abs of float64 (the project's kernel bound);
    the seven-point error at most 2x the six-point one (CPU emulation, tests/test_wino44_numerics_cpu.py: 0.7-1.2x);
    different bits (the route took effect), and a repeated call gives the same bits."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


@pytest.mark.parametrize('k,d,cin,cout,L,B,mode', [
    (7, 1, 256, 256, 1032, 16, None), (7, 1, 256, 256, 1028, 16, 1), (7, 1, 128, 128, 2052, 16, 2),
    (11, 1, 256, 256, 1032, 16, None), (11, 1, 256, 256, 1028, 16, 2), (11, 1, 128, 128, 2052, 16, 1), (7, 1, 32, 128, 700, 48, None),
    (7, 3, 256, 256, 1028, 16, None), (7, 5, 128, 128, 2052, 16, 1),
    (11, 3, 128, 128, 2052, 16, None), (11, 5, 256, 256, 1032, 16, None), (11, 5, 256, 256, 1028, 16, 2),
    (7, 1, 64, 64, 4100, 12, 2), (7, 5, 64, 64, 4100, 12, None),
    (11, 1, 64, 64, 4100, 12, None), (11, 3, 64, 64, 4100, 12, 1), (11, 5, 64, 64, 4100, 12, 2), (11, 1, 128, 64, 4100, 12, 0),
])
def test_seven_point_groups_k7_k11(dev, k, d, cin, cout, L, B, mode, ttsopt):
    """dilation 1: the aligned-vector window (k = 7: 13 groups in one phase, the 13th in a queue slot of its own; k = 11: 20 groups in one
    phase), with the plain epilogue (mode None) and the residual preload into nine planes (mode 0 / 1 / 2); dilation 3 / 5: the per-wave
    strip (k = 11 in two phases of 8 + 12 groups), residual in the row epilogue."""
    from ttsamd.engine import conv1d
    g = torch.Generator().manual_seed(k * 1000 + cin + L + d)
    x = torch.randn(B, cin, L, generator=g)
    w = torch.randn(cout, cin, k, generator=g) / np.sqrt(cin * k)
    b = torch.randn(cout, generator=g) * 0.3
    res = torch.randn(B, cout, L, generator=g) if mode is not None else None
    y0 = torch.randn(B, cout, L, generator=g)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0], lens[1], lens[2], lens[3] = L, L - 1, 131, 1
    xd, wd, bd, ld = x.to(dev), w.to(dev), b.to(dev), lens.to(dev)
    rd = None if res is None else res.to(dev)

    def run():
        y = y0.clone().to(dev)
        conv1d(xd, wd, bd, lens=ld, dilation=d, in_slope=0.1, res=rd, mode=mode or 0, div=3.0, y=y)
        return y.cpu()
    ttsopt.set('TTSAMD_WINO', '1')
    ttsopt.set('TTSAMD_WINO2', '31')
    outs = {}
    for mask in ('111', '15'):
        ttsopt.set('TTSAMD_WINO4', mask)
        outs[mask] = run()
    ttsopt.set('TTSAMD_WINO4', '111')
    again = run()
    worst = {'111': 0.0, '15': 0.0}
    for i in range(B):
        n = int(lens[i])
        v = F.conv1d(F.leaky_relu(x[i:i + 1, :, :n].double(), 0.1), w.double(), b.double(), padding=d * (k - 1) // 2, dilation=d)[0]
        if res is not None:
            v = v + res[i, :, :n].double()
        ref = v if not mode else (y0[i, :, :n].double() + v if mode == 1 else (y0[i, :, :n].double() + v) / 3.0)
        for mask in worst:
            worst[mask] = max(worst[mask], float((outs[mask][i, :, :n].double() - ref).abs().max()))
            assert torch.equal(outs[mask][i, :, n:], y0[i, :, n:]), 'positions past the utterance must stay untouched'
    print(f'k={k} d={d} cin={cin} cout={cout} mode={mode}: seven-point max-abs {worst["111"]:.2e}, six-point {worst["15"]:.2e} '
          f'({worst["111"] / worst["15"]:.2f}x)')
    assert worst['111'] < 5e-5 and worst['15'] < 5e-5
    assert worst['111'] <= 2.0 * worst['15']
    assert not torch.equal(outs['111'], outs['15']), 'TTSAMD_WINO4 bits 5 / 6 must route these shapes to the seven-point groups'
    assert torch.equal(outs['111'], again), 'a repeated call must give the same bits'
