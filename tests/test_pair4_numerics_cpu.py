"""CPU: the C = 32 fused pairs on Winograd F(4,3) (csrc/resblock_pair4.hip) before any GPU run.

1. The whole vocoder (vocoder/hifigan/models.py) with every conv emulated in float32 the way the fp32 engine now routes it -- the
   C = 32 k = 7 / 11 pairs and every un-fused ResBlock conv on F(4,3), the C = 32 / 64 k = 3 pairs still on F(2,3) -- and with the
   k = 3 pairs on F(4,3) too (what variant 6 of the kernel-level entry computes), against float64: the error budget stays inside the
   wave tolerance (1e-4) with room to spare.
2. The block geometry of resblock_pair4 restated in Python: for every (k, dilation) the staged window, the phase-A reads, the
   intermediate and the phase-B reads stay inside the LDS rows the kernel allocates, and every stored output reads only intermediate
   columns phase A wrote."""
import pytest
import torch

import tts_oracle as O
from ttsamd import synth
from ttsamd.config import HIFIGAN_CONFIG

from test_wino_f43_numerics_cpu import wino_conv1d_fp32


class _Routed:
    """F.conv1d of the oracle replaced by the Winograd emulation for the convs the fp32 engine sends to its Winograd kernels, with the
    scheme the engine uses after this change: F(2,3) for the C <= 64 k = 3 pairs (resblock_pair2), F(4,3) for the rest
    (k3_f43: the C = 32 k = 3 pairs on F(4,3) as well)."""

    def __init__(self, k3_f43):
        self.k3_f43, self.n = k3_f43, {'f23': 0, 'f43': 0}

    def __enter__(self):
        self.orig = O.F.conv1d

        def conv1d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
            k = w.shape[2]
            if (x.dtype == torch.float32 and k in (3, 7, 11) and w.shape[1] % 8 == 0 and w.shape[0] % 32 == 0
                    and padding == dilation * (k - 1) // 2 and stride == 1 and groups == 1 and x.dim() == 3):
                pair_k3 = k == 3 and w.shape[0] == w.shape[1] and w.shape[0] in ((64,) if self.k3_f43 else (32, 64))
                scheme = 'f23' if pair_k3 else 'f43'
                self.n[scheme] += 1
                return wino_conv1d_fp32(x, w, b, dilation, scheme)
            return self.orig(x, w, b, stride, padding, dilation, groups)
        O.F.conv1d = conv1d
        return self

    def __exit__(self, *a):
        O.F.conv1d = self.orig


@pytest.mark.parametrize('k3_f43', [False, True])
def test_vocoder_with_f43_pairs_error_budget(k3_f43):
    torch.manual_seed(0)
    hw = O.fold_weight_norm(synth.hifigan_state_dict())
    g = torch.Generator().manual_seed(4)
    mel = torch.randn(1, 80, 96, generator=g, dtype=torch.float64) * 1.5 - 4.0
    with torch.inference_mode():
        wave64 = O.hifigan_forward(hw, mel, HIFIGAN_CONFIG, dtype=torch.float64)
        with _Routed(k3_f43) as r:
            wave = O.hifigan_forward(hw, mel.float(), HIFIGAN_CONFIG)
    err = float((wave.double() - wave64).abs().max())
    print(f'\nwave max-abs vs float64 with the C = 32 pairs on F(4,3): {err:.2e} (convs routed: {r.n})')
    # 4 stages x 3 ResBlocks x 3 pairs x 2 convs + conv_pre (k = 7); the k = 3 ResBlocks' 6 convs per stage on F(2,3) where routed so
    assert r.n == ({'f23': 6, 'f43': 67} if k3_f43 else {'f23': 12, 'f43': 61})
    assert err < 1e-5          # the wave tolerance is 1e-4 (test_wino_f43_numerics_cpu.py: F(2,3) / F(4,3) everywhere, another input)


# ---- resblock_pair4.hip: Pair4Geo restated
WQ, NQ = 145, 128


def _geo(k, d):
    h = (k - 1) // 2
    nqa = (4 * NQ // (4 * d)) * d
    ts = (4 * nqa - 2 * h) & ~3
    nvec = (3 + 4 * nqa + (k - 1) * d + 3) // 4
    return h, nqa, ts, nvec


@pytest.mark.parametrize('k', [3, 7, 11])
@pytest.mark.parametrize('d', [1, 3, 5])
def test_pair4_block_geometry(k, d):
    h, nqa, ts, nvec = _geo(k, d)
    npos = k + 3
    assert 2 * 4 * 4 * WQ * 16 * 2 <= 160 * 1024                     # two blocks per CU
    assert nvec <= WQ and ts % 4 == 0 and ts > 0
    for q0 in (0, ts, 7 * ts):
        xfirst = q0 - h - h * d
        off = xfirst - (xfirst & ~3)
        assert 0 <= off < 4
        cols_w = set()
        for jw in range(NQ):                                         # phase A: every slot (idle ones repeat the last quad)
            pa = min(jw, nqa - 1)
            na = (pa // d) * 4 * d + pa % d
            for m in range(npos):
                c = off + na + m * d
                assert (c >> 2) < nvec                               # inside the staged vectors of the row
            if jw < nqa:
                cols_w.update(na + hh * d for hh in range(4))
        assert cols_w == set(range(4 * nqa))                         # the quads tile the intermediate columns exactly
        for jw in range(NQ):                                         # phase B: quad jw -> outputs 4 jw .. 4 jw + 3
            for m in range(npos):
                c = 4 * jw + m
                assert (c & 3) * WQ + (c >> 2) < 4 * WQ
            if 4 * jw < ts:                                          # a stored quad reads only columns phase A wrote
                assert 4 * jw + npos - 1 < 4 * nqa
    # every output of an utterance is stored by exactly one block
    L = 5 * ts + 12
    owners = [0] * L
    for t in range((L + ts - 1) // ts):
        for n in range(0, ts, 4):
            for e in range(4):
                if t * ts + n + e < L:
                    owners[t * ts + n + e] += 1
    assert owners == [1] * L
