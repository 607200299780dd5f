"""GPU parity of the register epilogue of the F(4,3) kernel (csrc/conv_wino4.hip, EPI 3 / 4) through the C ABI (pytest -m gpu): every
dilation-1 launch of k = 3 / 7 / 11 with one C-in slice peels the last step of its loop, fetches the residual's quads and the bias in that
step's gaps and stores the rows from registers.  What can go wrong there, at the smallest launches that reach it:

    steps: k = 3 (16-channel chunks, three stages) with Cin 16 / 32 / 48 and k = 7 / 11 (8-channel chunks) with Cin 8 / 16 / 24 = one, two and
    three chunks: the peeled step alone, straight behind the prologue, then with one and two ordinary steps in front of it; k = 7 / 11 on the
    seven-point groups (TTSAMD_WINO4=127, route 4) and on the six-point ones (=31, route 3: k = 11 runs two phases per chunk on three stages);
    epilogues (HiFi-GAN's ResBlock convs, vocoder/hifigan/models.py:30-53; FastPitch's conv-FF, transformer.py:59-65): plain; ReLU; no bias;
    residual with mode 0 / 1 / 2 (div 3); the residual is y itself (in place);
    rows: Cout 64 (one row block) with every step count and epilogue; Cout 128 (two row blocks) at two chunks with the plain, the mode 2
    and the in-place epilogue.  (Cout 96 is not here: the route wants whole 64-row blocks and sends it to the direct kernel, route 0.)

The route takes a launch with L % 4 == 0, L >= 256 and at least 192 blocks of 64 rows x 256 outputs: L = 1028 (five tiles) and the smallest
batch that gives 192 blocks; no split-K workspace, so one C-in slice.  Checker as in tests/test_gpu_wino44_rows.py: torch conv1d in float64
on the host per row at its exact length -- computed once per shape, the epilogues applied to it in float64 -- ragged lengths L, L - 1 (a
quad cut by the utterance end), 131 (cut inside a quad), 1, the rest random; 5e-5 max-abs (the project's kernel bound); positions past a
row's length keep their values; no NaN; a repeated call gives the same bits; ttsamd_conv_last_launch must report route 3 / 4, one slice."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

L0 = 1028
DIV = 3.0
# name -> (bias, relu_out, residual, mode, in place)
EPILOGUES = {
    'plain': (True, False, False, 0, False),
    'relu': (True, True, False, 0, False),
    'nobias': (False, False, False, 0, False),
    'res0': (True, False, True, 0, False),
    'res1': (True, False, True, 1, False),
    'res2': (True, False, True, 2, False),
    'inplace': (True, False, True, 0, True),
}


def batch_for_route(L, cout):
    tiles = -(-L // 256) * (-(-cout // 64))
    return -(-192 // tiles)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _shape(k, cin, cout):
    """data of one shape and its float64 convolution per row (no bias), computed once and left unchanged"""
    B = batch_for_route(L0, cout)
    g = torch.Generator().manual_seed(k * 10000 + 10 * cin + cout)
    x = torch.randn(B, cin, L0, generator=g)
    w = torch.randn(cout, cin, k, generator=g) / np.sqrt(cin * k)
    b = torch.randn(cout, generator=g) * 0.3
    r = torch.randn(B, cout, L0, generator=g)
    y0 = torch.randn(B, cout, L0, generator=g)
    ln = torch.randint(1, L0 + 1, (B,), generator=g)
    ln[0], ln[1], ln[2], ln[3] = L0, L0 - 1, 131, 1
    convs = []
    for i in range(B):
        n = int(ln[i])
        convs.append(F.conv1d(F.leaky_relu(x[i:i + 1, :, :n].double(), 0.1), w.double(), None, padding=(k - 1) // 2)[0])
    return x, w, b, r, y0, ln, convs


def _reference(shape, i, bias, relu, res, mode, inplace):
    x, w, b, r, y0, ln, convs = shape
    n = int(ln[i])
    v = convs[i]
    if bias:
        v = v + b.double()[:, None]
    if res:
        v = v + (y0 if inplace else r)[i, :, :n].double()
    if relu:
        v = v.clamp_min(0.0)
    if mode == 1:
        v = y0[i, :, :n].double() + v
    elif mode == 2:
        v = (y0[i, :, :n].double() + v) / DIV
    return v


def _run_and_check(dev, ttsopt, k, cin, cout, mask, epi):
    from ttsamd.engine import conv1d, last_conv_launch
    bias, relu, res, mode, inplace = EPILOGUES[epi]
    shape = _shape(k, cin, cout)
    x, w, b, r, y0, ln, _ = shape
    ttsopt.set('TTSAMD_WINO', '1')
    ttsopt.set('TTSAMD_WINO2', '31')
    ttsopt.set('TTSAMD_WINO4', str(mask))
    xd, wd, ld = x.to(dev), w.to(dev), ln.to(dev)
    bd = b.to(dev) if bias else None
    rd = r.to(dev) if (res and not inplace) else None

    def run():
        y = y0.clone().to(dev)
        conv1d(xd, wd, bd, lens=ld, dilation=1, in_slope=0.1, relu_out=relu, res=(y if inplace else rd) if res else None, mode=mode,
               div=DIV, y=y)
        return y.cpu(), last_conv_launch()
    out, rec = run()
    again, _ = run()
    worst = 0.0
    for i in range(x.shape[0]):
        ref = _reference(shape, i, bias, relu, res, mode, inplace)
        n = ref.shape[1]
        worst = max(worst, float((out[i, :, :n].double() - ref).abs().max()))
        assert torch.equal(out[i, :, n:], y0[i, :, n:]), 'positions past the utterance must keep their values bit for bit'
    print(f'k={k} cin={cin} cout={cout} WINO4={mask} {epi} B={x.shape[0]}: route {rec[0]} ksplit {rec[1]}, max-abs {worst:.2e} against float64')
    want = 4 if (k != 3 and mask & (32 if k == 7 else 64)) else 3
    assert rec == (want, 1), f'route {rec[0]} in {rec[1]} slices: the launch must run on the F(4,3) kernel (route {want}) in one slice'
    assert not torch.isnan(out).any()
    assert worst < 5e-5
    assert torch.equal(out, again), 'a repeated call must give the same bits'


# (k, TTSAMD_WINO4, the Cin of one / two / three chunks)
KERNELS = [(3, 127, (16, 32, 48)), (7, 127, (8, 16, 24)), (11, 127, (8, 16, 24)), (7, 31, (8, 16, 24)), (11, 31, (8, 16, 24))]


@pytest.mark.parametrize('epi', list(EPILOGUES))
@pytest.mark.parametrize('steps', [1, 2, 3])
@pytest.mark.parametrize('k,mask,cins', KERNELS, ids=[f'k{k}-wino4_{m}' for k, m, _ in KERNELS])
def test_register_epilogue_one_to_three_chunks(dev, k, mask, cins, steps, epi, ttsopt):
    _run_and_check(dev, ttsopt, k, cins[steps - 1], 64, mask, epi)


@pytest.mark.parametrize('epi', ['plain', 'res2', 'inplace'])
@pytest.mark.parametrize('k,mask,cins', KERNELS, ids=[f'k{k}-wino4_{m}' for k, m, _ in KERNELS])
def test_register_epilogue_two_row_blocks(dev, k, mask, cins, epi, ttsopt):
    _run_and_check(dev, ttsopt, k, cins[1], 128, mask, epi)
