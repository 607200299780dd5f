"""GPU parity of the fp32 upsamplers on Winograd F(4,2) (csrc/conv_wino4.hip: launch_convt_wino, route 6) through the C ABI
(pytest -m gpu): ConvTranspose1d(stride u, kernel 2u, padding u/2) as a two-tap Conv1d with u Cout rows, five products per output quad and
phase, interleaved stores straight from the output transform (tests/test_convt_wino_cpu.py restates the arithmetic).

ttsamd_conv_transpose1d under TTSAMD_CONVT_WINO=2 (wherever the launch is supported).  One ragged batch per shape: rows of lengths
{L, L - 41, 257, 256, 255, 5, 4, 1, 0}, L = 600 -- the launch covers positions tau = 0 .. len INCLUSIVE in tiles of 256, so 255 / 256 / 257 put
tau = len in the last tile, in a tile of its own and one past it; 5 / 4 / 1 cut the first quads; 0 has no tile at all.  Reference: torch
conv_transpose1d(leaky_relu(x, 0.1)) in float64 on the host, per row at its exact length, tests/test_gpu_convt.py's weight scaling.
Checks: max-abs < 5e-5 (the bound tests/test_gpu_wino4_epilogue.py holds the same six-point transforms to); route 6; a repeated call
gives the same bits; outputs past lens * u -- the whole of the row of length 0 -- keep the prefill; the result agrees with the
TTSAMD_CONVT_WINO=0 launch within the sum of both errors.  Default routing: route 6 at exactly the default's minimum batch x L of a class
it takes, route 5 just below."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

L_MAX = 600
LENS = (L_MAX, L_MAX - 41, 257, 256, 255, 5, 4, 1, 0)
MIN_POSITIONS = 8192            # kConvtWinoMinPositions, csrc/convt_mfma.hip


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


@pytest.mark.parametrize('shape', [(16, 8, 8), (32, 16, 8), (64, 32, 2), (128, 64, 2), (256, 128, 8)])
def test_conv_transpose1d_wino(dev, shape, ttsopt):
    """Measured on an MI355X, max-abs against float64, F(4,2) / the launch it replaces: (16, 8, 8) 1.05e-6 / 9.5e-7, (32, 16, 8) 2.26e-6 /
    1.32e-6, (64, 32, 2) 1.65e-6 / 1.31e-6, (128, 64, 2) 2.67e-6 / 2.00e-6, (256, 128, 8) 4.53e-6 / 3.34e-6; the two launches 1.4e-6 ... 4.5e-6
    apart (1.3-1.7x the direct arithmetic's error, as for the other six-point launches; bound 5e-5)."""
    from ttsamd.engine import conv_transpose1d, last_conv_launch
    cin, cout, u = shape
    B, L = len(LENS), L_MAX
    g = torch.Generator().manual_seed(cin + 10 * u + L)
    x = torch.randn(B, cin, L, generator=g)
    w = torch.randn(cin, cout, 2 * u, generator=g) / np.sqrt(2 * cin)
    b = torch.randn(cout, generator=g) * 0.3
    y0 = torch.randn(B, cout, L * u, generator=g)
    lens = torch.tensor(LENS, dtype=torch.int64)
    xd, wd, bd, ld = x.to(dev), w.to(dev), b.to(dev), lens.to(dev)

    def run():
        y = y0.clone().to(dev)
        conv_transpose1d(xd, wd, bd, lens=ld, in_slope=0.1, y=y)
        return y.cpu(), last_conv_launch()
    ttsopt.set('TTSAMD_CONVT', '1')
    ttsopt.set('TTSAMD_CONVT_WINO', 2)
    out, rec = run()
    again, _ = run()
    ttsopt.set('TTSAMD_CONVT_WINO', 0)
    base, rec0 = run()
    assert rec == (6, 1), f'TTSAMD_CONVT_WINO=2: route / ksplit {rec}, expected (6, 1)'
    assert rec0[0] in (0, 5), f'TTSAMD_CONVT_WINO=0: route {rec0}'
    assert torch.equal(out, again), 'a repeated call must give the same bits'
    assert not torch.isnan(out).any()
    worst, worst0 = 0.0, 0.0
    for i, n in enumerate(LENS):
        m = n * u
        if m:
            ref = F.conv_transpose1d(F.leaky_relu(x[i:i + 1, :, :n], 0.1).double(), w.double(), b.double(), stride=u, padding=u // 2)[0]
            assert ref.shape[1] == m
            worst = max(worst, float((out[i, :, :m].double() - ref).abs().max()))
            worst0 = max(worst0, float((base[i, :, :m].double() - ref).abs().max()))
        assert torch.equal(out[i, :, m:], y0[i, :, m:]), f'outputs past lens * u must stay untouched (row {i}, length {n})'
    both = float((out - base).abs().max())
    print(f'convt wino {shape} L={L} B={B}: route 6 max-abs {worst:.2e}, route {rec0[0]} {worst0:.2e}, between the two {both:.2e}')
    assert worst < 5e-5
    assert both <= worst + worst0


def test_default_routing_threshold(dev, ttsopt):
    """Default routing (TTSAMD_CONVT_WINO unset): a class it takes goes to the F(4,2) launch from batch x L = 8192 input positions, and stays
    on the all-phase kernel one row of quads below; the two launches agree."""
    from ttsamd.engine import conv_transpose1d, last_conv_launch
    cin, cout, u = ROUTED_CLASS
    B = 4
    g = torch.Generator().manual_seed(7)
    w = (torch.randn(cin, cout, 2 * u, generator=g) / np.sqrt(2 * cin)).to(dev)
    ttsopt.set('TTSAMD_CONVT', '1')
    ttsopt.set('TTSAMD_CONVT_WINO', None)
    for L, route in ((MIN_POSITIONS // B, 6), (MIN_POSITIONS // B - 4, 5)):
        x = torch.randn(B, cin, L, generator=g).to(dev)
        y = conv_transpose1d(x, w, None, in_slope=0.1)
        assert last_conv_launch() == (route, 1), f'batch x L = {B * L}: route {last_conv_launch()}, expected {route}'
        if route == 6:
            ttsopt.set('TTSAMD_CONVT_WINO', 0)
            y5 = conv_transpose1d(x, w, None, in_slope=0.1)
            assert last_conv_launch() == (5, 1)
            ttsopt.set('TTSAMD_CONVT_WINO', None)
            assert float((y - y5).abs().max()) < 1e-4       # each within 5e-5 of the exact result (the bound above)


ROUTED_CLASS = (128, 64, 2)     # a (Cin, Cout, u) the default routing takes (convt_wino_default, csrc/convt_mfma.hip)
