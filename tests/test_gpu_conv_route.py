"""GPU (pytest -m gpu): the launchers of the exact-fp32 conv execute what the routing function answers.  Every case launches one conv
through engine.conv1d and asserts last_conv_launch() == conv_route(...) (ttsamd_conv1d_route, csrc/conv_route.hip) and the route id the
case was chosen for: every id, C-in slices on the direct and on the F(4,3) kernel, and the three fall-backs to the direct kernel
(rows that are no multiple of four floats, an in-slope above 1, a kernel size without a Winograd form).  The shapes were chosen with the
query on the host: the smallest of this form that reach each id (F(4,3) and F(2,3) ask for 192 blocks; 12 x 17 tiles of 64 rows at
L = 4100).  The values are checked against torch's conv1d in float64 at the project's kernel bound, so an id that named a kernel
other than the one that ran would still have to compute the conv.  tests/test_gpu_splitk.py and tests/test_gpu_wino4_strip_packed.py
assert the same equality on every launch of theirs (slices on routes 0 / 3 / 4, the packed forms 7 / 8)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WS = 4 << 20                    # kSplitKFloats (csrc/common.hpp)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


# options, (B, cin, cout, k, dilation, L), in_slope, residual, mode, workspace floats, (route, slices; None: >= 2)
CASES = [
    ({'TTSAMD_WINO': '0'}, (12, 64, 64, 3, 1, 4100), 0.1, False, 0, None, (0, 1)),
    ({}, (1, 256, 256, 3, 1, 130), 0.1, False, 0, WS, (0, None)),                     # direct kernel, C-in slices
    ({'TTSAMD_WINO4': '0', 'TTSAMD_WINO2': '0'}, (6, 64, 128, 3, 1, 4100), 0.1, False, 0, None, (1, 1)),
    ({}, (6, 24, 128, 3, 1, 4100), 0.1, True, 0, None, (1, 1)),                       # Cin % 16 != 0: conv1d_wino_f32 under the defaults
    ({'TTSAMD_WINO4': '0'}, (12, 64, 64, 7, 1, 4100), 0.1, False, 0, None, (2, 1)),
    ({}, (12, 64, 64, 3, 1, 4100), 0.1, False, 0, None, (3, 1)),                      # F(4,3), register epilogue without a residual
    ({}, (12, 64, 64, 3, 1, 4100), 0.1, True, 2, None, (3, 1)),                       # ... with the residual, accumulate mode 2
    ({}, (1, 256, 64, 3, 1, 24576), 0.1, False, 0, WS, (3, None)),                    # F(4,3), C-in slices
    ({}, (12, 64, 64, 7, 1, 4100), 0.1, False, 0, None, (4, 1)),
    ({}, (12, 64, 64, 3, 3, 4100), 0.1, False, 0, None, (7, 1)),
    ({}, (12, 64, 64, 11, 5, 4100), 0.1, False, 0, None, (8, 1)),
    ({}, (12, 64, 64, 11, 5, 4100), 0.1, True, 0, None, (4, 1)),                      # a residual keeps the row epilogue
    ({}, (12, 64, 64, 3, 1, 4099), 0.1, False, 0, None, (0, 1)),                      # fall-backs: rows of 4099 floats,
    ({}, (12, 64, 64, 3, 1, 4100), 1.5, False, 0, None, (0, 1)),                      # an in-slope above 1,
    ({}, (12, 64, 64, 5, 1, 4100), 0.1, False, 0, None, (0, 1)),                      # k = 5
]


@pytest.mark.parametrize('options,shape,slope,res,mode,ws,want', CASES)
def test_launch_is_the_route_the_query_answers(dev, ttsopt, options, shape, slope, res, mode, ws, want):
    from ttsamd.engine import conv1d, conv_route, last_conv_launch
    B, cin, cout, k, d, L = shape
    g = torch.Generator().manual_seed(100 * k + d + cin)
    x = torch.randn(B, cin, L, generator=g)
    w = torch.randn(cout, cin, k, generator=g) / np.sqrt(cin * k)
    b = torch.randn(cout, generator=g) * 0.3
    r = torch.randn(B, cout, L, generator=g) if res else None
    y0 = torch.randn(B, cout, L, generator=g)
    for name, value in options.items():
        ttsopt.set(name, value)
    asked = conv_route(B, cin, cout, k, L, dilation=d, in_slope=slope, has_res=res, mode=mode, splitk_floats=ws)
    y = y0.clone().to(dev)
    conv1d(x.to(dev), w.to(dev), b.to(dev), dilation=d, in_slope=slope, res=None if r is None else r.to(dev), mode=mode, div=3.0, y=y,
           splitk_floats=ws)
    ran = last_conv_launch()
    assert ran == asked, f'launched {ran}, conv_route says {asked}'
    assert ran[0] == want[0] and (ran[1] >= 2 if want[1] is None else ran[1] == want[1]), f'{ran}: the case was chosen for {want}'
    v = F.conv1d(F.leaky_relu(x.double(), slope), w.double(), b.double(), padding=d * (k - 1) // 2, dilation=d)
    if r is not None:
        v = v + r.double()
    ref = v if mode == 0 else (y0.double() + v) / 3.0
    err = float((y.cpu().double() - ref).abs().max())
    print(f'{options} {shape} slope {slope} res {res} mode {mode}: route {ran[0]} ksplit {ran[1]}, max-abs {err:.2e} against float64')
    assert err < 5e-5
