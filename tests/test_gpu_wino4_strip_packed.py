"""GPU parity of the PACKED strip form of the F(4,3) kernel (csrc/conv_wino4.hip, EPI 7; TTSAMD_WINO4 bit 7) through the C ABI
(pytest -m gpu): the dilated launches with one C-in slice, no residual and mode 0 (HiFi-GAN's c1 convs) on packed tiles -- tile i of a
row = its tuples [64 i, 64 i + 64) of the d ceil(n / 4d) the row has (csrc/common.hpp: wino4_pk_*) -- with the last step peeled and the
rows stored from registers as dwords.

    k = 7 / 11 with Cin 8 / 16 / 24 (one to three 8-channel chunks: the prologue, the peeled step, one ordinary step), k = 3 with Cin
    16 / 32 (16-channel chunks), Cout 64 and one case with 128 (two row blocks), dilation 3 and 5;
    L = 1028: 260 tuples at d = 5 = five tiles that start at the residues 0, 4, 3, 2, 1 of their first group, the last of four tuples;
    258 tuples at d = 3 = all three residues; one case at L = 1284; the smallest batch that gives the route its 192 blocks;
    ragged lengths L, L - 1, 257, 256, 241, 240, 131, 21, 20, 19 (under one group at d = 5), 1, the rest random: the edges of the plain
    tiles (252 / 240 columns), of the packed ones and of a group.

Checker as in tests/test_gpu_wino44_rows.py: torch conv1d in float64 on the host per row at its exact length, 5e-5 max-abs (the
project's kernel bound), positions past a row's length untouched, a repeated call gives the same bits.  Every case runs with
TTSAMD_WINO4 = 255 and = 127 (the plain tiles and the row epilogue through LDS on every launch): both inside the bound and EQUAL BIT
FOR BIT -- the products of an output, their order, the output transform and the bias / ReLU order are the same, only which block
computes a quad differs.  ttsamd_conv_last_launch must report route 7 / 8 (six- / seven-point groups, packed form) under 255 and
3 / 4 under 127.  A residual, an accumulate mode and C-in slices keep the row epilogue under 255 too (route 3 / 4, the bits of 127)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

WS = 4 << 20                    # kSplitKFloats (csrc/common.hpp)
L0 = 1028
EDGES = (0, -1, 257, 256, 241, 240, 131, 21, 20, 19, 1)      # 0 / -1: L, L - 1


def block_outputs(d):
    """wino4_block_outputs (csrc/conv_wino4.hip): the largest multiple of 4 d in 256 -- the routing rule counts blocks of the PLAIN tile"""
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
def _case(cin, cout, k, d, L, B, lens, res, mode, relu):
    """data of one case and its float64 reference per row, computed once (both masks share it)"""
    g = torch.Generator().manual_seed(k * 1000 + 10 * cin + d + L + (7 if res else 0) + (mode or 0))
    x = torch.randn(B, cin, L, generator=g)
    w = torch.randn(cout, cin, k, generator=g) / np.sqrt(cin * k)
    b = torch.randn(cout, generator=g) * 0.3
    r = torch.randn(B, cout, L, generator=g) if res else None
    y0 = torch.randn(B, cout, L, generator=g)
    if lens is None:
        ln = torch.randint(1, L + 1, (B,), generator=g)
        for i, e in enumerate(EDGES[:B]):
            ln[i] = L + e if e <= 0 else e
    else:
        ln = torch.tensor(lens, dtype=torch.int64)
    refs = []
    for i in range(B):
        n = int(ln[i])
        v = F.conv1d(F.leaky_relu(x[i:i + 1, :, :n].double(), 0.1), w.double(), b.double(), padding=d * (k - 1) // 2, dilation=d)[0]
        if r is not None:
            v = v + r[i, :, :n].double()
        if relu:
            v = v.clamp_min(0.0)
        refs.append(v if not mode else (y0[i, :, :n].double() + v if mode == 1 else (y0[i, :, :n].double() + v) / 3.0))
    return x, w, b, r, y0, ln, refs


def _run_mask(dev, ttsopt, mask, case, d, mode, relu, splitk_floats=None):
    """two calls under one mask -> (y on the host, (route, ksplit), max-abs against float64); tails and repeatability asserted"""
    from ttsamd.engine import conv1d, conv_route, last_conv_launch
    x, w, b, r, y0, ln, refs = case
    ttsopt.set('TTSAMD_WINO', '1')
    ttsopt.set('TTSAMD_WINO2', '31')
    ttsopt.set('TTSAMD_WINO4', str(mask))
    xd, wd, bd, ld = x.to(dev), w.to(dev), b.to(dev), ln.to(dev)
    rd = None if r is None else r.to(dev)

    def run():
        y = y0.clone().to(dev)
        conv1d(xd, wd, bd, lens=ld, dilation=d, in_slope=0.1, relu_out=relu, res=rd, mode=mode or 0, div=3.0, y=y, splitk_floats=splitk_floats)
        return y.cpu(), last_conv_launch()
    out, rec = run()
    asked = conv_route(x.shape[0], x.shape[1], w.shape[0], w.shape[2], x.shape[2], dilation=d, in_slope=0.1, relu_out=relu, has_res=r is not None,
                       mode=mode or 0, splitk_floats=splitk_floats)
    assert rec == asked, f'mask {mask}: launched {rec}, conv_route (ttsamd_conv1d_route) says {asked}'
    again, _ = run()
    worst = 0.0
    for i, ref in enumerate(refs):
        n = ref.shape[1]
        worst = max(worst, float((out[i, :, :n].double() - ref).abs().max()))
        assert torch.equal(out[i, :, n:], y0[i, :, n:]), f'mask {mask}: positions past the utterance must stay untouched (row {i}, length {n})'
    assert not torch.isnan(out).any()
    assert torch.equal(out, again), f'mask {mask}: a repeated call must give the same bits'
    return out, rec, worst


def _both_masks(dev, ttsopt, tag, case, k, d, mode, relu, packed, splitk_floats=None):
    new, rec_new, e_new = _run_mask(dev, ttsopt, 255, case, d, mode, relu, splitk_floats)
    old, rec_old, e_old = _run_mask(dev, ttsopt, 127, case, d, mode, relu, splitk_floats)
    plain = 3 if k == 3 else 4
    print(f'{tag}: mask 255 route {rec_new[0]} ksplit {rec_new[1]} max-abs {e_new:.2e}; mask 127 route {rec_old[0]} ksplit {rec_old[1]} '
          f'max-abs {e_old:.2e} against float64')
    assert rec_old[0] == plain, f'mask 127: route {rec_old}'
    assert rec_new[0] == (plain + 4 if packed else plain), f'mask 255: route {rec_new}, packed form expected: {packed}'
    assert rec_new[1] == rec_old[1]
    assert e_new < 5e-5 and e_old < 5e-5
    assert torch.equal(new, old), 'the packed strip form must give the bits of the plain one'
    return rec_new


@pytest.mark.parametrize('d', [3, 5])
@pytest.mark.parametrize('cin', [8, 16, 24])
@pytest.mark.parametrize('k', [7, 11])
def test_packed_strip_k7_k11_one_to_three_chunks(dev, k, cin, d, ttsopt):
    B = batch_for_route(L0, d)
    relu = 1 if cin == 16 else 0
    case = _case(cin, 64, k, d, L0, B, None, False, None, relu)
    rec = _both_masks(dev, ttsopt, f'k={k} cin={cin} d={d} relu={relu} B={B}', case, k, d, None, relu, True)
    assert rec[1] == 1


@pytest.mark.parametrize('d', [3, 5])
@pytest.mark.parametrize('cin', [16, 32])
def test_packed_strip_k3(dev, cin, d, ttsopt):
    B = batch_for_route(L0, d)
    relu = 1 if cin == 32 else 0
    case = _case(cin, 64, 3, d, L0, B, None, False, None, relu)
    rec = _both_masks(dev, ttsopt, f'k=3 cin={cin} d={d} relu={relu} B={B}', case, 3, d, None, relu, True)
    assert rec[1] == 1


def test_packed_strip_two_row_blocks(dev, ttsopt):
    k, cin, cout, d = 7, 16, 128, 5
    B = batch_for_route(L0, d, cout)
    case = _case(cin, cout, k, d, L0, B, None, False, None, 0)
    _both_masks(dev, ttsopt, f'k={k} cin={cin} cout={cout} d={d} B={B}', case, k, d, None, 0, True)


def test_packed_strip_longer_rows(dev, ttsopt):
    """L = 1284: 325 tuples at d = 5 = six tiles, the last of five tuples"""
    k, cin, d, L = 11, 8, 5, 1284
    B = batch_for_route(L, d)
    case = _case(cin, 64, k, d, L, B, None, False, None, 1)
    _both_masks(dev, ttsopt, f'k={k} cin={cin} d={d} L={L} B={B}', case, k, d, None, 1, True)


@pytest.mark.parametrize('res,mode', [(True, None), (False, 2)])
def test_residual_and_accumulate_modes_keep_the_row_epilogue(dev, res, mode, ttsopt):
    k, cin, d = 7, 16, 3
    B = batch_for_route(L0, d)
    case = _case(cin, 64, k, d, L0, B, None, res, mode, 0)
    _both_masks(dev, ttsopt, f'k={k} cin={cin} d={d} res={res} mode={mode} B={B}', case, k, d, mode, 0, False)


def test_cin_slices_keep_the_row_epilogue(dev, ttsopt):
    """the split-K launch of tests/test_gpu_wino44_rows.py (256 -> 256, k = 11, dilation 3, L = 1792, batch 2) with the workspace of
    tests/test_gpu_splitk.py"""
    cin, cout, k, d, L, B = 256, 256, 11, 3, 1792, 2
    case = _case(cin, cout, k, d, L, B, (L - 1, 131), False, None, 0)
    rec = _both_masks(dev, ttsopt, f'split-K k={k} cin={cin} d={d} L={L} B={B}', case, k, d, None, 0, False, splitk_floats=WS)
    assert rec[1] >= 2, f'{rec[1]} slices'


def test_whole_generator_default_equals_plain_strip(dev, ttsopt):
    """HiFi-GAN on a small ragged batch: the default (bit 7 set) against TTSAMD_WINO4 = 127, bit for bit; and the batch is large enough
    that its C = 64 c1 convs at dilation 3 take the packed form (the same launch through conv1d: route 8)"""
    from ttsamd import lib, synth
    from ttsamd.engine import HifiGanEngine, conv1d, last_conv_launch
    ttsopt.set('TTSAMD_WINO4', None)                   # the default mask is under test
    assert lib.get_option('TTSAMD_WINO4') is None
    rng = np.random.default_rng(33)
    mel = torch.from_numpy((rng.standard_normal((4, 80, 160)) * 1.5 - 4.0).astype(np.float32)).to(dev)
    lens = torch.tensor([160, 151, 97, 133]).to(dev)
    eng = HifiGanEngine(synth.hifigan_state_dict(), device=dev)
    wave_new = eng.forward(mel, lens).cpu()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 64, 128 * 160, generator=g).to(dev)
    w = (torch.randn(64, 64, 7, generator=g) / 21.0).to(dev)
    conv1d(x, w, torch.zeros(64, device=dev), lens=128 * lens, dilation=3, in_slope=0.1)
    assert last_conv_launch() == (8, 1), last_conv_launch()
    ttsopt.set('TTSAMD_WINO4', '127')
    wave_old = eng.forward(mel, lens).cpu()
    assert not torch.isnan(wave_new).any() and float(wave_new.abs().max()) > 0
    assert torch.equal(wave_new, wave_old), 'HiFi-GAN under the default mask must give the bits of mask 127'
