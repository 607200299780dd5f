"""GPU parity of the seven-point groups of the F(4,3) kernel (csrc/conv_wino4.hip, Wino4Geo PT_ = 7) on the smallest launches at which
the partial sums its input transform shares between rows -- and carries from one sub-filter to the next -- can go wrong, through the C
ABI (pytest -m gpu).  tests/test_gpu_wino44.py starts at Cin 32; here:

    Cin 8 / 16 / 24 = one, two and three 8-channel chunks: with two stages the prologue stages the first chunk and the loop re-stages the
    last one into a dead stage (the tail), so at one chunk EVERY staged value comes from the prologue or the tail, at two chunks one
    step is an ordinary one; Cout 64 (one row block), k = 7 and 11;
    dilation 1 (aligned-vector window) plain and with the residual preloaded into the nine planes (mode 0 and 2); dilation 3 / 5 (the
    per-wave strip: k = 11 in two phases of 8 + 12 groups, phase 0 ends on V0 of the second sub-filter and phase 1 starts at its V1);
    one split-K launch (256 -> 256, k = 11, dilation 3, L = 1792, batch 2) with the workspace of tests/test_gpu_splitk.py: slices that
    start at a chunk other than 0 on the two-phase kernel.

The route takes a launch with L % 4 == 0, L >= 256 and at least 192 blocks of 64 rows x wino4_block_outputs(dilation) outputs: L = 1028
(five tiles at every dilation) and the smallest batch that gives 192 blocks.  Checker as in tests/test_gpu_wino44.py: torch conv1d in
float64 on the host per row at its exact length (HiFi-GAN's ResBlock convs, vocoder/hifigan/models.py:30-53), ragged lengths L, L - 1
(a quad cut by the utterance end), 131 (cut inside a quad), 1, the rest random; 5e-5 max-abs (the project's kernel bound); positions past
a row's length untouched; a repeated call gives the same bits; ttsamd_conv_last_launch must report route 4."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WS = 4 << 20                    # kSplitKFloats (csrc/common.hpp)
L0 = 1028


def block_outputs(d):
    """wino4_block_outputs (csrc/conv_wino4.hip): the largest multiple of 4 d in 256"""
    return (256 // (4 * d)) * (4 * d)


def batch_for_route(L, d, cout=64):
    tiles = -(-L // block_outputs(d)) * (-(-cout // 64))
    return -(-192 // tiles)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


@functools.lru_cache(maxsize=None)
def _case(cin, cout, k, d, L, B, lens, res, mode):
    """data of one case and its float64 reference per row, computed once"""
    g = torch.Generator().manual_seed(k * 1000 + 10 * cin + d + (7 if res else 0) + (mode or 0))
    x = torch.randn(B, cin, L, generator=g)
    w = torch.randn(cout, cin, k, generator=g) / np.sqrt(cin * k)
    b = torch.randn(cout, generator=g) * 0.3
    r = torch.randn(B, cout, L, generator=g) if res else None
    y0 = torch.randn(B, cout, L, generator=g)
    if lens is None:
        ln = torch.randint(1, L + 1, (B,), generator=g)
        ln[0], ln[1], ln[2], ln[3] = L, L - 1, 131, 1
    else:
        ln = torch.tensor(lens, dtype=torch.int64)
    refs = []
    for i in range(B):
        n = int(ln[i])
        v = F.conv1d(F.leaky_relu(x[i:i + 1, :, :n].double(), 0.1), w.double(), b.double(), padding=d * (k - 1) // 2, dilation=d)[0]
        if r is not None:
            v = v + r[i, :, :n].double()
        refs.append(v if not mode else (y0[i, :, :n].double() + v if mode == 1 else (y0[i, :, :n].double() + v) / 3.0))
    return x, w, b, r, y0, ln, refs


def _run_and_check(dev, ttsopt, tag, case, d, mode, splitk_floats=None):
    from ttsamd.engine import conv1d, last_conv_launch
    x, w, b, r, y0, ln, refs = case
    ttsopt.set('TTSAMD_WINO', '1')
    ttsopt.set('TTSAMD_WINO2', '31')
    ttsopt.set('TTSAMD_WINO4', '127')
    xd, wd, bd, ld = x.to(dev), w.to(dev), b.to(dev), ln.to(dev)
    rd = None if r is None else r.to(dev)

    def run():
        y = y0.clone().to(dev)
        conv1d(xd, wd, bd, lens=ld, dilation=d, in_slope=0.1, res=rd, mode=mode or 0, div=3.0, y=y, splitk_floats=splitk_floats)
        return y.cpu(), last_conv_launch()
    out, rec = run()
    again, _ = run()
    worst = 0.0
    for i, ref in enumerate(refs):
        n = ref.shape[1]
        worst = max(worst, float((out[i, :, :n].double() - ref).abs().max()))
        assert torch.equal(out[i, :, n:], y0[i, :, n:]), 'positions past the utterance must stay untouched'
    print(f'{tag}: route {rec[0]} ksplit {rec[1]}, max-abs {worst:.2e} against float64')
    assert rec[0] == 4, f'route {rec[0]} (ksplit {rec[1]}): the launch must run on the seven-point groups'
    assert not torch.isnan(out).any()
    assert worst < 5e-5
    assert torch.equal(out, again), 'a repeated call must give the same bits'
    return rec


# dilation, residual, mode (None: plain epilogue)
EPILOGUES = [(1, False, None), (1, True, 0), (1, True, 2), (3, False, None), (5, False, None)]


@pytest.mark.parametrize('d,res,mode', EPILOGUES)
@pytest.mark.parametrize('cin', [8, 16, 24])
@pytest.mark.parametrize('k', [7, 11])
def test_seven_point_rows_one_to_three_chunks(dev, k, cin, d, res, mode, ttsopt):
    B = batch_for_route(L0, d)
    case = _case(cin, 64, k, d, L0, B, None, res, mode)
    rec = _run_and_check(dev, ttsopt, f'k={k} cin={cin} d={d} res={res} mode={mode} B={B}', case, d, mode)
    assert rec[1] == 1


def test_seven_point_rows_splitk_two_phase_strip(dev, ttsopt):
    """C-in slices (c_beg != 0) on the strip path of k = 11: every slice's prologue and tail form the sums of their own chunks"""
    cin, cout, k, d, L, B = 256, 256, 11, 3, 1792, 2
    case = _case(cin, cout, k, d, L, B, (L - 1, 131), False, None)
    rec = _run_and_check(dev, ttsopt, f'split-K k={k} cin={cin} d={d} L={L} B={B}', case, d, None, splitk_floats=WS)
    assert rec[1] >= 2, f'{rec[1]} slices'
