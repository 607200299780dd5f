"""GPU parity of the fp32 ConvTranspose1d launches -- HiFi-GAN's upsamplers -- through the C ABI (pytest -m gpu): the all-phase kernel
(csrc/convt_mfma.hip: every output phase of a tile in one wave, `rho >= u / 2` input shift, float4 / float2 stores of u consecutive outputs)
and the polyphase launch of the direct kernel (csrc/conv_mfma.hip with n_phase = u, K = 2, dil = -1, y_ts = u, per-lane epilogue), which
takes what the first does not: u = 4 (V3), launches under 100 blocks, unaligned rows, and everything under TTSAMD_CONVT=0.

ttsamd_conv_transpose1d fills the launch through the function the generator uses (launch_upsampler) and packs the torch weight
[Cin][Cout][2u] on the device; ttsamd_conv_last_launch says which kernel ran (5: all-phase, 0: direct).  Reference: torch
conv_transpose1d(leaky_relu(x, 0.1), stride u, padding u // 2) in float64 on the host, per row at its exact length.  Per shape, with
TTSAMD_CONVT=1 and =0: the expected route; max-abs < 3e-5 (the direct conv's bound, tests/test_gpu_parity.py: these sums have at most
2 x 512 = 1024 products of the same scaling, fewer than the 2816 of the C = 256, k = 11 conv that holds it); a repeated call gives the
same bits; the two routes agree to 5e-6 where both exist; outputs past lens * u -- the whole of a row of length 0 -- keep the prefill."""
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


# (cin, cout, u), L, B, route with TTSAMD_CONVT=1.  L: just enough for the u = 8 shapes to have the all-phase kernel's 100 blocks of 64 rows x
# 64 inputs at B = 4 (4 / 2 / 1 row blocks: 7 x 16, 13 x 8, 25 x 4)
@pytest.mark.parametrize('shape,L,B,route1', [
    ((512, 256, 8), 400, 4, 5), ((256, 128, 8), 800, 4, 5), ((128, 64, 2), 700, 4, 5), ((64, 32, 2), 700, 4, 5),     # V1
    ((128, 64, 8), 1600, 4, 5), ((64, 32, 4), 700, 4, 0),                                                            # V3 (u = 4: always direct)
    ((512, 256, 8), 150, 1, 0),            # 3 x 4 blocks: under min_blocks, the direct kernel even with TTSAMD_CONVT=1
    ((128, 64, 2), 701, 4, 0),             # odd L: rows of y are not 16-byte aligned
])
def test_conv_transpose1d(dev, shape, L, B, route1, ttsopt):
    """Measured on an MI355X: 4.94e-6 / 4.16e-6 / 2.79e-6 ((512, 256, 8), (256, 128, 8), (128, 64, 8)), 2.25e-6 / 1.44e-6 (u = 2), 1.90e-6
    (u = 4) against float64 on either route, and the two routes equal bit for bit: both run the same MFMA chain (octets, taps, channel
    pairs in one order) and add the bias after it.  With the all-phase kernel's accumulators started from the bias, as they were, the
    routes were up to 7.15e-6 apart at (512, 256, 8) and missed the 5e-6 below."""
    from ttsamd.engine import conv_transpose1d, last_conv_launch
    cin, cout, u = shape
    g = torch.Generator().manual_seed(cin + 10 * u + L)
    x = torch.randn(B, cin, L, generator=g)
    w = torch.randn(cin, cout, 2 * u, generator=g) / np.sqrt(2 * cin)
    b = torch.randn(cout, generator=g) * 0.3
    y0 = torch.randn(B, cout, L * u, generator=g)
    lens = torch.tensor([L, L - 41, 1, 0][:B], dtype=torch.int64)
    xd, wd, bd, ld = x.to(dev), w.to(dev), b.to(dev), lens.to(dev)

    def run():
        y = y0.clone().to(dev)
        conv_transpose1d(xd, wd, bd, lens=ld, in_slope=0.1, y=y)
        return y.cpu(), last_conv_launch()
    outs = {}
    for flag, route in (('1', route1), ('0', 0)):
        ttsopt.set('TTSAMD_CONVT', flag)
        outs[flag], rec = run()
        again, _ = run()
        assert rec == (route, 1), f'TTSAMD_CONVT={flag}: route / ksplit {rec}, expected ({route}, 1)'
        assert torch.equal(outs[flag], again), 'a repeated call must give the same bits'
    refs = [F.conv_transpose1d(F.leaky_relu(x[i:i + 1, :, :int(n)], 0.1).double(), w.double(), b.double(), stride=u, padding=u // 2)[0]
            for i, n in enumerate(lens) if int(n) > 0]
    worst = {'1': 0.0, '0': 0.0}
    for flag, out in outs.items():
        assert not torch.isnan(out).any()
        for i, n in enumerate(lens):
            m = int(n) * u
            if m:
                assert refs[i].shape[1] == m
                worst[flag] = max(worst[flag], float((out[i, :, :m].double() - refs[i]).abs().max()))
            assert torch.equal(out[i, :, m:], y0[i, :, m:]), f'TTSAMD_CONVT={flag}: outputs past lens * u must stay untouched (row {i})'
    both = float((outs['1'] - outs['0']).abs().max())
    print(f'convt {shape} L={L} B={B}: route {route1} max-abs {worst["1"]:.2e}, route 0 {worst["0"]:.2e}, between the two {both:.2e}')
    assert worst['1'] < 3e-5 and worst['0'] < 3e-5
    assert both <= 5e-6
    if route1 == 5:   # stronger than the band: the two kernels run one MFMA chain and add the bias after it, so a re-ordering of either shows
        assert torch.equal(outs['1'], outs['0']), 'the all-phase and the direct launch must give the same bits'
