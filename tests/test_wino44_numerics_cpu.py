"""Seven-point groups of the F(4,3) kernel (csrc/conv_wino4.hip, Wino4Geo PT_ = 7), numerics on the CPU in the emulation style of
test_wino_f43_numerics_cpu.py: filter transform in float64 rounded once, input transform / products / output transform in float32.

One more interpolation point (1/2) beside 0, +-1, +-2, inf turns the three-tap sub-filter of F(4,3) into a FOUR-tap one, F(4,4): seven
products per output quad for four taps.  A three-tap sub-filter on the same seven points has U6 = g3 / 2 = 0: six products, window
position x6 never read.  k = 7 = taps (0..3) + (4..6): 7 + 6 = 13 products per quad (six-point groups: 16), k = 11 = (0..3) + (4..7) +
(8..10): 20 (23).  The price is a transform with larger entries (12, 10, 1/120): measured here on single convs and on the whole vocoder
(vocoder/hifigan/models.py:30-53, the ResBlock1 convs), against the same network in float64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import tts_oracle as O
from ttsamd import synth
from ttsamd.config import NET_CONFIG, HIFIGAN_CONFIG

from test_wino_f43_numerics_cpu import _lin, wino_conv1d_fp32

# points 0, 1, -1, 2, -2, 1/2, inf: the matrices in csrc/conv_wino4.hip's header
BT44 = np.array([[4, -8, -5, 10, 1, -2, 0],
                 [0, -4, 4, 9, -1, -2, 0],
                 [0, -4, 12, -7, -3, 2, 0],
                 [0, 2, -3, -4, 3, 2, 0],
                 [0, 2, -5, 0, 5, -2, 0],
                 [0, 4, 0, -5, 0, 1, 0],
                 [0, -4, 8, 5, -10, -1, 2]], np.float64)
G44 = np.array([[1 / 4, 0, 0, 0],
                [1 / 6, 1 / 6, 1 / 6, 1 / 6],
                [1 / 18, -1 / 18, 1 / 18, -1 / 18],
                [1 / 72, 2 / 72, 4 / 72, 8 / 72],
                [1 / 120, -2 / 120, 4 / 120, -8 / 120],
                [32 / 45, 16 / 45, 8 / 45, 4 / 45],
                [0, 0, 0, 1 / 2]], np.float64)
AT44 = np.array([[1, 1, 1, 1, 1, 1, 0],
                 [0, 1, -1, 2, -2, 1 / 2, 0],
                 [0, 1, 1, 4, 4, 1 / 4, 0],
                 [0, 1, -1, 8, -8, 1 / 8, 1]], np.float64)


def test_seven_point_matrices_are_exact():
    """A^T [(G g) * (B^T x)] == the four-tap correlation in float64, and the three-tap one with g3 = 0 whose seventh product vanishes;
    x6 enters V6 only, P0 reaches y0 only and P6 reaches y3 only (what the kernel's window size and residual preload rely on)."""
    rng = np.random.default_rng(0)
    for taps in (4, 3):
        for _ in range(8):
            g, x = np.zeros(4), rng.standard_normal(7)
            g[:taps] = rng.standard_normal(taps)
            want = np.array([sum(g[t] * x[i + t] for t in range(4)) for i in range(4)])
            U = G44 @ g
            assert np.abs(AT44 @ (U * (BT44 @ x)) - want).max() < 1e-12
            if taps == 3:
                assert U[6] == 0.0
                x2 = x.copy()
                x2[6] = 1e6                                        # never read: the six issued products do not see it
                assert np.abs(AT44[:, :6] @ (U[:6] * (BT44 @ x2)[:6]) - want).max() < 1e-12
    assert (BT44[:6, 6] == 0).all()
    assert (AT44[1:, 0] == 0).all() and (AT44[:3, 6] == 0).all() and AT44[0, 0] == 1 and AT44[3, 6] == 1


def wino44_conv1d_fp32(x, w, bias, dilation, counts=None):
    """'same' Conv1d [B,Ci,L] x [Co,Ci,k] (k in 7 / 11) in float32 through the seven-point groups: four-tap sub-filters at the tap offsets
    0, 4 (, 8), the last one with three taps and six groups.  counts (a dict) receives the products per output quad of each k."""
    B, Ci, L = x.shape
    Co, _, k = w.shape
    assert k in (7, 11)
    nsf, half, m = (k + 3) // 4, (k - 1) // 2, 4
    w64 = np.zeros((Co, Ci, 4 * nsf))
    w64[:, :, :k] = w.double().numpy()
    # filter transform in float64, rounded once (pack_wino44_weight)
    Us = [[torch.from_numpy(np.einsum('t,oct->oc', G44[i], w64[:, :, 4 * s:4 * s + 4]).astype(np.float32)) for i in range(7)]
          for s in range(nsf)]
    ngrp = [7 if 4 * s + 3 < k else 6 for s in range(nsf)]
    if counts is not None:
        counts[k] = sum(ngrp)
    y = torch.zeros(B, Co, L, dtype=torch.float32)
    for r in range(dilation):
        xr = x[:, :, r::dilation]
        Lr = xr.shape[2]
        if Lr == 0:
            continue
        J = -(-Lr // m)
        xp = F.pad(xr, (half, m * J + k - Lr))
        planes_U = [[] for _ in range(7)]
        planes_V = [[] for _ in range(7)]
        for s in range(nsf):
            # the window of a quad has k + 3 positions: a three-tap sub-filter reads six of them, x6 (past the window) is never touched
            X = [xp[:, :, 4 * s + mm:4 * s + mm + m * J:m] for mm in range(ngrp[s])]
            for i in range(ngrp[s]):
                planes_U[i].append(Us[s][i])
                planes_V[i].append(_lin(BT44[i][:ngrp[s]], X))
        P = [torch.matmul(torch.cat(planes_U[i], 1), torch.cat(planes_V[i], 1)) for i in range(7)]
        for o in range(m):
            yo = _lin(AT44[o], P)
            idx = torch.arange(o, m * J, m)
            keep = idx < Lr
            y[:, :, r::dilation][:, :, idx[keep]] = yo[:, :, :int(keep.sum())]
    if bias is not None:
        y = y + bias[None, :, None]
    return y


@pytest.mark.parametrize('k,d', [(7, 1), (7, 3), (11, 1), (11, 5)])
def test_emulated_seven_point_conv_equals_the_direct_conv(k, d):
    """same shapes, seeds and bound as the F(4,3) cases of test_wino_f43_numerics_cpu.py"""
    g = torch.Generator().manual_seed(10 * k + d)
    x = torch.randn(2, 16, 67, generator=g)
    w = torch.randn(24, 16, k, generator=g) / (16 * k) ** 0.5
    b = torch.randn(24, generator=g)
    want = F.conv1d(x.double(), w.double(), b.double(), dilation=d, padding=d * (k - 1) // 2)
    got = wino44_conv1d_fp32(x, w, b, d)
    got43 = wino_conv1d_fp32(x, w, b, d, 'f43')
    e, e43 = float((got.double() - want).abs().max()), float((got43.double() - want).abs().max())
    print(f'\nk={k} d={d}: seven-point max-abs {e:.2e}, F(4,3) emulation {e43:.2e}')
    assert e < 2e-5


class _Patched:
    """F.conv1d of the oracle module replaced for the launches the fp32 engine routes to its Winograd kernels (the conditions of
    test_wino_f43_numerics_cpu._Patched).  scheme 'f43': all of them on F(4,3); 'w44': k = 7 / 11 with Cout >= 64 on the seven-point groups
    (what csrc/hifigan.hip packs them for), everything else on F(4,3)."""

    def __init__(self, scheme):
        self.scheme, self.n, self.n44, self.counts = scheme, 0, 0, {}

    def __enter__(self):
        self.orig = O.F.conv1d

        def conv1d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
            k = w.shape[2]
            if (x.dtype == torch.float32 and k in (3, 7, 11) and w.shape[1] % 8 == 0 and w.shape[0] % 32 == 0
                    and padding == dilation * (k - 1) // 2 and stride == 1 and groups == 1 and x.dim() == 3):
                self.n += 1
                if self.scheme == 'w44' and k in (7, 11) and w.shape[0] >= 64:
                    self.n44 += 1
                    return wino44_conv1d_fp32(x, w, b, dilation, self.counts)
                return wino_conv1d_fp32(x, w, b, dilation, 'f43')
            return self.orig(x, w, b, stride, padding, dilation, groups)
        O.F.conv1d = conv1d
        return self

    def __exit__(self, *a):
        O.F.conv1d = self.orig


@pytest.fixture(scope='module')
def study():
    """the utterance of test_wino_f43_numerics_cpu.py's study (20 tokens, 142 frames, 36 352 samples): the float64 mel, then the vocoder in
    float64, with every routed conv on F(4,3), and with the k = 7 / 11 convs of Cout >= 64 on the seven-point groups"""
    torch.manual_seed(0)
    fsd, hsd = synth.fastpitch_state_dict(), synth.hifigan_state_dict()
    ids = synth.synth_ids(1, 20)
    dur = synth.synth_durations(1, 20)
    with torch.inference_mode():
        hw = O.fold_weight_norm(hsd)
        mel64, lens, *_ = O.fastpitch_infer(O.to_torch(fsd, torch.float64), NET_CONFIG, ids, dur_tgt=dur, dtype=torch.float64)
        mel64 = mel64.double()
        wave64 = O.hifigan_forward(hw, mel64, HIFIGAN_CONFIG, dtype=torch.float64)
        res = {}
        for scheme in ('f43', 'w44'):
            with _Patched(scheme) as p:
                wave = O.hifigan_forward(hw, mel64.float(), HIFIGAN_CONFIG)
            err = wave.double() - wave64
            res[scheme] = {'wave': float(err.abs().max()), 'rms': float(err.pow(2).mean().sqrt()), 'routed': p.n, 'n44': p.n44,
                           'counts': dict(p.counts)}
    res['peak'] = float(wave64.abs().max())
    return res


def test_seven_point_whole_vocoder_error_study(study):
    """The whole vocoder with its k = 7 / 11 ResBlock convs of 64 channels and more on the seven-point groups: the wave stays under the
    project's review threshold (2e-5 max-abs against float64) and within 1.5x of the all-F(4,3) vocoder of the same run."""
    a, b = study['f43'], study['w44']
    print(f"\nwave vs float64 (|wave| peak {study['peak']:.3f}): F(4,3) max-abs {a['wave']:.2e} rms {a['rms']:.2e}; "
          f"seven-point groups max-abs {b['wave']:.2e} rms {b['rms']:.2e} ({b['wave'] / a['wave']:.2f}x)"
          f"\nconvs routed: {b['routed']}, of them on seven-point groups: {b['n44']}"
          f"\nproducts per output quad: k = 7: {b['counts'].get(7)}, k = 11: {b['counts'].get(11)} (six-point groups: 16 / 23)")
    assert a['routed'] == b['routed'] >= 72 and b['n44'] >= 36        # 3 stages x 2 kernel sizes x 6 convs
    assert b['wave'] < 2e-5
    assert b['wave'] <= 1.5 * a['wave']
    assert b['counts'] == {7: 13, 11: 20}

def test_mask_that_contradicts_itself_is_rejected():
    """bits 5 / 6 say how the F(4,3) kernel runs k = 7 / 11; without bit 1 / 2 it does not run that k: an error, not an ignored bit"""
    from ttsamd import lib
    for bad in (32, 64, 96, 32 + 4, 64 + 2):
        with pytest.raises(lib.TtsAmdError):
            lib.set_option('TTSAMD_WINO4', bad)
    assert lib.get_option('TTSAMD_WINO4') is None
