"""CPU: the C = 32 k = 7 / 11 fused pairs on the seven-point groups (csrc/resblock_pair4.hip, PT_ = 7) before any GPU run.

The whole vocoder (vocoder/hifigan/models.py:30-53, 111-127) on the study utterance of test_wino44_numerics_cpu.py with every routed conv
emulated in float32 the way the fp32 engine runs it, against the same network in float64:

  'before'  the routing of the parent: k = 7 / 11 with Cout >= 64 on seven-point groups, the C = 32 k = 7 / 11 pairs on six-point F(4,3)
  'after'   the C = 32 k = 7 / 11 pairs on seven-point groups as well (13 / 20 products per output quad in both of their convs)

In both runs the k = 3 pairs of C = 32 / 64 are on F(2,3) (resblock_pair2) and the un-fused k = 3 convs on F(4,3): each conv on the scheme
it runs on.  The host packing (pack_wino44_weight at 32 x 32) has no entry of its own in the C ABI, so its layout is checked on the GPU
(tests/test_gpu_pair44.py): by the whole generator at its default routing against the oracle, which runs on the host-packed filters,
and by variant 7 of ttsamd_resblock_pair, which packs the same values in the same layout on the device."""
import pytest
import torch

import tts_oracle as O
from ttsamd import synth
from ttsamd.config import NET_CONFIG, HIFIGAN_CONFIG

from test_wino_f43_numerics_cpu import wino_conv1d_fp32
from test_wino44_numerics_cpu import wino44_conv1d_fp32


class _Routed:
    """F.conv1d of the oracle replaced for the convs the fp32 engine sends to its Winograd kernels (the conditions of
    test_wino_f43_numerics_cpu._Patched), each on its scheme; pairs44: the C = 32 k = 7 / 11 pairs on seven-point groups."""

    def __init__(self, pairs44):
        self.pairs44, self.n, self.counts = pairs44, {'f23': 0, 'f43': 0, 'w44': 0}, {}

    def __enter__(self):
        self.orig = O.F.conv1d

        def conv1d(x, w, b=None, stride=1, padding=0, dilation=1, groups=1):
            k = w.shape[2]
            if (x.dtype == torch.float32 and k in (3, 7, 11) and w.shape[1] % 8 == 0 and w.shape[0] % 32 == 0
                    and padding == dilation * (k - 1) // 2 and stride == 1 and groups == 1 and x.dim() == 3):
                square = w.shape[0] == w.shape[1]
                if k == 3:
                    scheme = 'f23' if square and w.shape[0] in (32, 64) else 'f43'
                elif w.shape[0] >= 64 or (self.pairs44 and square and w.shape[0] == 32):
                    scheme = 'w44'
                else:
                    scheme = 'f43'
                self.n[scheme] += 1
                if scheme == 'w44':
                    return wino44_conv1d_fp32(x, w, b, dilation, self.counts)
                return wino_conv1d_fp32(x, w, b, dilation, scheme)
            return self.orig(x, w, b, stride, padding, dilation, groups)
        O.F.conv1d = conv1d
        return self

    def __exit__(self, *a):
        O.F.conv1d = self.orig


@pytest.fixture(scope='module')
def study():
    """one utterance of 20 tokens (142 frames, 36 352 samples): the float64 mel, the vocoder in float64 and under both routings"""
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
        for name, pairs44 in (('before', False), ('after', True)):
            with _Routed(pairs44) as r:
                wave = O.hifigan_forward(hw, mel64.float(), HIFIGAN_CONFIG)
            err = wave.double() - wave64
            res[name] = {'wave': float(err.abs().max()), 'rms': float(err.pow(2).mean().sqrt()), 'n': dict(r.n), 'counts': dict(r.counts),
                         'out': wave}
    res['peak'] = float(wave64.abs().max())
    return res


def test_seven_point_pairs_whole_vocoder_error_study(study):
    a, b = study['before'], study['after']
    between = float((a['out'] - b['out']).abs().max())
    print(f"\nwave vs float64 (|wave| peak {study['peak']:.3f}): as routed before max-abs {a['wave']:.2e} rms {a['rms']:.2e}; with the "
          f"C = 32 k = 7 / 11 pairs on seven-point groups max-abs {b['wave']:.2e} rms {b['rms']:.2e} ({b['wave'] / a['wave']:.2f}x); "
          f"between the two waves {between:.2e}\nconvs per scheme: before {a['n']}, after {b['n']}")
    # 4 stages x 3 ResBlocks x 3 pairs x 2 convs + conv_pre (k = 7, 512 rows): 73 routed convs.  k = 3 pairs of C = 32 / 64: 12 on F(2,3);
    # un-fused k = 3 (C = 256 / 128): 12 on F(4,3); k = 7 / 11 at C >= 64: 36 + conv_pre on seven-point groups; C = 32 k = 7 / 11: 12 convs
    assert a['n'] == {'f23': 12, 'f43': 24, 'w44': 37}
    assert b['n'] == {'f23': 12, 'f43': 12, 'w44': 49}
    assert b['counts'] == {7: 13, 11: 20}
    assert b['wave'] < 2e-5                         # the project's review threshold (test_wino44_numerics_cpu.py)
    assert b['wave'] <= 1.5 * a['wave']
    assert between > 0.0                            # the two routings really differ
