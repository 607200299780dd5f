"""GPU parity of the split-K launches of the fp32 conv engine through the C ABI (pytest -m gpu): what every batch-1 conv of HiFi-GAN's
C = 256 stage and of FastPitch's conv-FF runs, and what ttsamd_conv1d_ex -- which hands the launchers no workspace -- never reaches.

ttsamd_conv1d_splitk carries the workspace the models carry (csrc/common.hpp: kSplitKFloats = 4 << 20 floats, NaN-filled here before every
call), ttsamd_conv_last_launch says which kernel ran and in how many input-channel slices, so a case cannot pass on another route.  Covered:
the slice bookkeeping of the direct kernel (csrc/conv_mfma.hip: c_beg / c_end, uneven slices, the (slice, row) partial layout, the partial
store with Cout < CoutP) and of the F(4,3) kernel (csrc/conv_wino4.hip, six- and seven-point groups, aligned window and strip), and
splitk_reduce_kernel, which re-implements the epilogue: bias, residual, ReLU, mode 0 / 1 / 2, ragged lengths.

Checker and data are those of tests/test_gpu_wino44.py: torch conv1d in float64 on the host per row at its exact length, positions past a
row's length untouched bit for bit.  Every case runs
    (a) with the workspace, (b) the same call again: the same bits,
    (c) the same kernel un-split on the same data: the direct kernel without a workspace; the F(4,3) kernel with the batch repeated until
        the launch has the 192 blocks that keep it on its route without a split (compared on the first copy),
and asserts the recorded route and slice count, (a) and (c) within the project's bound for that kernel (3e-5 the plain direct epilogue,
tests/test_gpu_parity.py; 5e-5 the Winograd routes and every case with a residual or an accumulate mode, tests/test_gpu_wino44.py),
err(a) <= 2 err(c) (slices only regroup the sum: about 1x), different bits between (a) and (c), and no NaN."""
import functools

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


@functools.lru_cache(maxsize=None)
def _case(cin, cout, k, d, L, B, lens, res, mode, relu):
    """Data of one case and its float64 reference per row (computed once, shared by the runs and routes of the case)."""
    g = torch.Generator().manual_seed(k * 1000 + cin + L + d)
    x = torch.randn(B, cin, L, generator=g)
    w = torch.randn(cout, cin, k, generator=g) / np.sqrt(cin * k)
    b = torch.randn(cout, generator=g) * 0.3
    r = torch.randn(B, cout, L, generator=g) if res else None
    y0 = torch.randn(B, cout, L, generator=g)
    ln = torch.tensor(lens, dtype=torch.int64) if lens is not None else None
    refs = []
    for i in range(B):
        n = L if lens is None else int(lens[i])
        if n == 0:
            refs.append(torch.zeros(cout, 0, dtype=torch.float64))
            continue
        v = F.conv1d(F.leaky_relu(x[i:i + 1, :, :n].double(), 0.1), w.double(), b.double(), padding=d * (k - 1) // 2, dilation=d)[0]
        if r is not None:
            v = v + r[i, :, :n].double()
        if relu:
            v = v.clamp_min(0.0)
        refs.append(v if not mode else (y0[i, :, :n].double() + v if mode == 1 else (y0[i, :, :n].double() + v) / 3.0))
    return x, w, b, r, y0, ln, refs


def _run(dev, case, d, mode, relu, splitk_floats=None, repeat=1):
    """One call on the case's data (the batch `repeat` times over) -> (y on the host, (route, ksplit))."""
    from ttsamd.engine import conv1d, conv_route, last_conv_launch
    x, w, b, r, y0, ln, _ = case
    rep = (lambda t: None if t is None else t.repeat(repeat, *([1] * (t.dim() - 1))).to(dev))
    y = rep(y0)
    conv1d(rep(x), w.to(dev), b.to(dev), lens=rep(ln), dilation=d, in_slope=0.1, relu_out=relu, res=rep(r), mode=mode or 0, div=3.0, y=y,
           splitk_floats=splitk_floats)
    rec = last_conv_launch()
    # ... and it is what the routing function answers for this launch without launching (ttsamd_conv1d_route)
    asked = conv_route(x.shape[0] * repeat, x.shape[1], w.shape[0], w.shape[2], x.shape[2], dilation=d, in_slope=0.1, relu_out=relu,
                       has_res=r is not None, mode=mode or 0, splitk_floats=splitk_floats)
    assert rec == asked, f'launched {rec}, conv_route says {asked}'
    return y.cpu(), rec


def _err(out, case):
    """max-abs against float64 over the rows of the case; the tail of every row must be the prefill, bit for bit."""
    _, _, _, _, y0, ln, refs = case
    worst = 0.0
    for i, ref in enumerate(refs):
        n = ref.shape[1]
        if n:
            worst = max(worst, float((out[i, :, :n].double() - ref).abs().max()))
        assert torch.equal(out[i, :, n:], y0[i, :, n:]), 'positions past the utterance must stay untouched'
    return worst


def _check(tag, rec_a, rec_c, a, again, c, case, bound, ksplit=None):
    B = case[4].shape[0]
    assert not torch.isnan(a).any() and not torch.isnan(c).any(), 'NaN: the reduce read a partial sum nobody wrote'
    ea, ec = _err(a, case), _err(c[:B], case)
    print(f'{tag}: route {rec_a[0]} ksplit {rec_a[1]}: split max-abs {ea:.2e}, un-split (route {rec_c[0]}, ksplit {rec_c[1]}) {ec:.2e} '
          f'({ea / ec if ec else float("nan"):.2f}x)')
    assert rec_c == (rec_a[0], 1), f'the un-split run took route / ksplit {rec_c}'
    assert rec_a[1] >= 2 if ksplit is None else rec_a[1] == ksplit, f'{rec_a[1]} slices'
    assert ea < bound and ec < bound
    assert ea <= 2.0 * ec
    assert not torch.equal(a, c[:B]), 'split and un-split runs must differ in bits (the sums are grouped differently)'
    assert torch.equal(a, again), 'a repeated call must give the same bits'


RAGGED8 = (448, 447, 131, 1, 300, 64, 448, 200)


# (cin, cout, k, dil, L, B), lens, residual, mode (None: plain), relu_out, workspace floats
@pytest.mark.parametrize('shape,lens,res,mode,relu,ws', [
    ((256, 256, 3, 1, 130, 1), None, False, None, False, WS),
    ((256, 256, 11, 5, 131, 2), (131, 64), True, 2, False, WS),                 # odd L: unaligned rows
    ((384, 1536, 3, 1, 64, 1), None, False, None, True, WS),                    # FastPitch conv-FF, `tiny` tiles
    ((1536, 384, 3, 1, 64, 1), None, True, 0, False, WS),
    ((384, 80, 1, 1, 200, 1), None, False, None, False, WS),                    # Cout 80 < CoutP 96
    ((128, 128, 7, 3, 300, 3), (300, 0, 1), False, 1, False, WS),
    ((1536, 384, 3, 1, 448, 8), RAGGED8, True, 0, False, 8 << 20),              # 128 x 64 deep-K tiles (TTSAMD_DEEP_SPLITK default)
])
def test_direct_kernel_splitk(dev, shape, lens, res, mode, relu, ws, ttsopt):
    cin, cout, k, d, L, B = shape
    case = _case(cin, cout, k, d, L, B, lens, res, mode, relu)
    ttsopt.set('TTSAMD_WINO', '0')
    a, rec_a = _run(dev, case, d, mode, relu, splitk_floats=ws)
    again, _ = _run(dev, case, d, mode, relu, splitk_floats=ws)
    c, rec_c = _run(dev, case, d, mode, relu)
    assert rec_a[0] == 0
    bound = 5e-5 if (res or mode) else 3e-5
    _check(f'direct {shape} lens={lens} res={res} mode={mode} relu={relu}', rec_a, rec_c, a, again, c, case, bound)


def test_direct_kernel_uneven_slices_and_workspace_limit(dev, ttsopt):
    """32 chunks of 8 channels in 3 slices (10 + 11 + 11) when the workspace holds exactly three partial tensors; one float short of two
    partial tensors: no split, and the bits of the call without a workspace."""
    cin, cout, k, d, L, B = 256, 256, 7, 1, 200, 1
    case = _case(cin, cout, k, d, L, B, None, False, None, False)
    per = B * cout * L
    ttsopt.set('TTSAMD_WINO', '0')
    a, rec_a = _run(dev, case, d, None, False, splitk_floats=3 * per)
    again, _ = _run(dev, case, d, None, False, splitk_floats=3 * per)
    c, rec_c = _run(dev, case, d, None, False)
    assert rec_a[0] == 0
    _check('direct (256, 256, 7, 1, 200, 1) workspace 3 x B Cout L', rec_a, rec_c, a, again, c, case, 3e-5, ksplit=3)
    small, rec_s = _run(dev, case, d, None, False, splitk_floats=2 * per - 1)
    assert rec_s == (0, 1), rec_s
    assert torch.equal(small, c), 'a workspace too small for two slices must give the bits of the call without one'


# (cin, cout, k, dil, L, B), lens, residual, mode, relu_out, expected slices (None: >= 2)
WINO4_CASES = [
    ((256, 256, 7, 1, 3584, 1), None, False, None, False, None),
    ((256, 256, 11, 1, 3584, 1), None, True, 2, False, None),        # the residual goes through the reduce kernel, not the nine-plane preload
    ((256, 256, 11, 5, 3584, 1), None, False, 1, False, None),       # the strip path (seven-point: two phases of 8 + 12 groups)
    ((256, 256, 7, 3, 1792, 2), (1792, 131), True, 0, False, None),
    ((256, 256, 11, 3, 1792, 2), (1791, 1), False, None, False, None),
]


def _wino4_case(dev, ttsopt, mask, route, shape, lens, res, mode, relu, ksplit):
    cin, cout, k, d, L, B = shape
    assert L % 4 == 0
    case = _case(cin, cout, k, d, L, B, lens, res, mode, relu)
    ttsopt.set('TTSAMD_WINO', '1')
    ttsopt.set('TTSAMD_WINO2', '31')
    ttsopt.set('TTSAMD_WINO4', mask)
    a, rec_a = _run(dev, case, d, mode, relu, splitk_floats=WS)
    again, _ = _run(dev, case, d, mode, relu, splitk_floats=WS)
    assert rec_a[0] == route, f'route {rec_a[0]} (ksplit {rec_a[1]}), expected {route}'
    # un-split: without a workspace a launch this small falls off the F(4,3) route (< 192 blocks): repeat the batch until it stays
    for rep in range(2, 17):
        c, rec_c = _run(dev, case, d, mode, relu, repeat=rep)
        if rec_c == (route, 1):
            break
    _check(f'F(4,3) mask {mask} {shape} lens={lens} res={res} mode={mode} relu={relu} (un-split: batch x {rep})', rec_a, rec_c, a, again, c,
           case, 5e-5, ksplit=ksplit)


@pytest.mark.parametrize('mask,route', [('127', 4), ('31', 3)])
@pytest.mark.parametrize('shape,lens,res,mode,relu,ksplit', WINO4_CASES)
def test_wino4_splitk_k7_k11(dev, mask, route, shape, lens, res, mode, relu, ksplit, ttsopt):
    """C = 256 at L = 3584 (B L = 3584 in the ragged cases) is the project's batch-1 shape: 56-60 blocks x 4 slices."""
    _wino4_case(dev, ttsopt, mask, route, shape, lens, res, mode, relu, ksplit)


@pytest.mark.parametrize('shape,lens,res,mode,relu,ksplit', [
    ((256, 256, 3, 1, 7168, 1), None, False, None, False, 2),
    ((384, 1536, 3, 1, 768, 1), None, False, None, True, 3),
    ((1536, 384, 3, 1, 768, 1), None, True, 0, False, 12),
])
def test_wino4_splitk_k3(dev, shape, lens, res, mode, relu, ksplit, ttsopt):
    """k = 3 (16-channel chunks, six-point groups only): HiFi-GAN's C = 256 stage and FastPitch's conv-FF pair; slice counts as
    wino4_ksplit (csrc/conv_route.hip) gives them: ~224 blocks wanted, at least 8 chunks per slice."""
    _wino4_case(dev, ttsopt, '127', 3, shape, lens, res, mode, relu, ksplit)
