"""CPU: the restatement tests/aligner_ref.py against the reference's goldens (tests/golden/aligner.npz, written by tools/gen_golden_aligner.py
from the reference's ConvAttention, mas_width1 and average_pitch), the input condition the end-to-end comparison rests on, and the surface
of the drop-in modules.  The GPU tests (tests/test_gpu_aligner.py) compare the kernels with this restatement."""
import inspect

import numpy as np
import pytest

import aligner_ref as R


@pytest.fixture(scope='module')
def gold(golden, synth_weights):
    from ttsamd import synth
    g = golden('aligner')
    sd = dict(synth_weights['fastpitch'])
    sd.update(synth.fastpitch_aligner_state_dict(gain=float(g['gain'])))
    return g, sd


def test_hard_paths_and_durations_equal_the_reference_exactly(gold):
    g, _ = gold
    hard = R.b_mas(g['log_attn'], g['in_lens'], g['mel_lens'])
    assert hard.dtype == np.float32
    assert np.array_equal(hard, g['attn_hard'].astype(np.float32))
    dur = hard.sum(2)[:, 0, :]
    assert np.array_equal(dur, g['dur'])
    assert np.array_equal(dur.sum(1), g['mel_lens'].astype(np.float32))          # the reference's own assertion (model.py:315)
    for b, n in enumerate(g['in_lens']):
        assert not dur[b, n:].any()


@pytest.mark.parametrize('tag', ['', '_prior'])
def test_soft_values_within_the_reference_noise_floor(gold, tag):
    """float64 restatement vs the reference's fp32 output: the largest difference IS the stored floor (the generator measured it with this
    very restatement), so this pins the restatement, the weights and the stored inputs together; fp32 restatement within 4 floors."""
    g, sd = gold
    prior = g['prior'] if tag else None
    soft, logprob = R.attention(sd, g['ids'], g['mel'], g['in_lens'], prior, np.float64)
    for key, got in (('attn_soft', soft), ('attn_logprob', logprob)):
        floor = float(g['floor_' + key + tag])
        err = float(np.abs(got - g[key + tag]).max())
        print(f'{key}{tag}: float64 restatement vs reference {err:.3e}, stored floor {floor:.3e}')
        assert 0 < floor < 1e-4
        assert err <= floor * (1 + 1e-9)
    soft32, logprob32 = R.attention(sd, g['ids'], g['mel'], g['in_lens'], prior, np.float32)
    assert np.abs(soft32 - soft).max() <= 4 * float(g['floor_attn_soft' + tag])
    assert np.abs(logprob32 - logprob).max() <= 4 * float(g['floor_attn_logprob' + tag])
    # what the soft attention must be whatever the arithmetic
    masked = np.arange(g['ids'].shape[1])[None, None, None, :] >= g['in_lens'][:, None, None, None]
    assert not (g['attn_soft' + tag] * masked).any()
    assert np.abs(g['attn_soft' + tag].sum(-1) - 1).max() < 1e-6


def test_log_attn_is_the_fp32_log_of_attn_soft(gold):
    g, _ = gold
    with np.errstate(divide='ignore'):
        mine = np.log(g['attn_soft'])
    fin = np.isfinite(g['log_attn'])
    assert np.array_equal(fin, np.isfinite(mine))
    assert np.abs(mine[fin] - g['log_attn'][fin]).max() <= 2e-6 * np.abs(g['log_attn'][fin]).max()      # libm's logf vs torch's: an ulp or two


@pytest.mark.parametrize('tag', ['', '_prior'])
def test_the_reference_alone_is_unambiguous(gold, tag):
    """The two conditions the end-to-end test rests on, recomputed here and compared with what the generator stored: the fp32 path equals
    the float64 path, and the smallest |log_p[i-1, j-1] - log_p[i-1, j]| on the backtrack is >= 8 x the largest |log_p fp32 - float64|."""
    g, sd = gold
    assert bool(g['path_fp32_equals_fp64' + tag])
    soft64, _ = R.attention(sd, g['ids'], g['mel'], g['in_lens'], g['prior'] if tag else None, np.float64)
    with np.errstate(divide='ignore'):
        log64 = np.log(soft64)
        log32 = np.log(g['attn_soft' + tag]).astype(np.float32) if tag else g['log_attn']
    margin, err = np.inf, 0.0
    for b in range(g['ids'].shape[0]):
        t, n = int(g['mel_lens'][b]), int(g['in_lens'][b])
        p32, p64 = R.mas_forward(log32[b, 0, :t, :n]), R.mas_forward(log64[b, 0, :t, :n])
        opt32, m = R.mas_backtrack(p32)
        opt64, _ = R.mas_backtrack(p64)
        assert np.array_equal(opt32, opt64) and np.array_equal(opt32, g['attn_hard' + tag][b, 0, :t, :n])
        margin = min(margin, float(np.nanmin(m)))
        fin = np.isfinite(p32)
        assert np.array_equal(fin, np.isfinite(p64))
        err = max(err, float(np.abs(p32[fin].astype(np.float64) - p64[fin]).max()))
    print(f'aligner{tag}: smallest backtrack margin {margin:.3e}, largest table error {err:.3e}, ratio {margin / err:.1f}')
    assert margin >= 8 * err
    assert float(g['min_backtrack_margin' + tag]) >= 8 * float(g['max_table_err' + tag])
    if not tag:
        assert margin == float(g['min_backtrack_margin']) and err == float(g['max_table_err'])


def test_pitch_tgt_within_its_floor(gold):
    g, _ = gold
    floor = float(g['floor_pitch_tgt'])
    got = R.average_pitch(g['pitch'], g['dur'])
    assert 0 < floor < 1e-5
    assert np.abs(got - g['pitch_tgt']).max() <= floor * (1 + 1e-9)
    # the properties of average_pitch: zero for a token without frames or without a voiced frame
    assert not got[:, 0][g['dur'] == 0].any()


def test_mas_restatement_edge_cases():
    """the rule itself at the sizes where it changes: one token, one frame, fewer frames than tokens, all ties, -inf entries"""
    one = R.mas_width1(np.zeros((5, 1), np.float32))
    assert np.array_equal(one, np.ones((5, 1), np.float32))
    assert np.array_equal(R.mas_width1(np.zeros((1, 4), np.float32)), np.array([[0, 0, 0, 1]], np.float32))
    ties = R.mas_width1(np.zeros((4, 3), np.float32))                            # every decision a tie -> j - 1 at once, then token 0
    assert np.array_equal(ties.argmax(1), [0, 0, 1, 2])
    short = R.mas_width1(np.zeros((3, 6), np.float32))                           # T < L: -inf ties walk left, the first tokens get nothing
    assert np.array_equal(short.argmax(1), [3, 4, 5]) and short.sum() == 3
    x = np.zeros((4, 3), np.float32)
    x[2, 1] = -np.inf
    got = R.mas_width1(x)
    assert got.sum(1).tolist() == [1, 1, 1, 1] and got[2, 1] == 0


def test_dropin_modules_expose_the_reference_names():
    from models.fastpitch.fastpitch import alignment, model
    assert list(inspect.signature(alignment.mas_width1).parameters) == ['log_attn_map']
    sig = inspect.signature(alignment.b_mas)
    assert list(sig.parameters) == ['b_log_attn_map', 'in_lens', 'out_lens', 'width'] and sig.parameters['width'].default == 1
    assert list(inspect.signature(model.average_pitch).parameters) == ['pitch', 'durs']
    sig = inspect.signature(model.mask_from_lens)
    assert list(sig.parameters) == ['lens', 'max_len'] and sig.parameters['max_len'].default is None
    assert 'ONLY' in model.__doc__
    import torch
    lens = torch.tensor([3, 1, 0])
    assert model.mask_from_lens(lens).tolist() == [[True, True, True], [True, False, False], [False, False, False]]
    assert model.mask_from_lens(lens, max_len=2).shape == (3, 2)


def test_aligner_state_dict_has_the_reference_keys_and_shapes(gold, synth_weights):
    from ttsamd import synth
    from ttsamd.engine import ALIGNER_KEYS
    g, _ = gold
    sd = synth.fastpitch_aligner_state_dict()
    want = dict(zip(g['aligner_keys'].tolist(), g['aligner_shapes'].tolist()))   # the reference module's own state_dict()
    assert len(want) == 10
    assert {k: str(tuple(v.shape)) for k, v in sd.items()} == want
    assert all(v.dtype == np.float32 for v in sd.values())
    assert set(ALIGNER_KEYS) == set(want) | {'encoder.word_emb.weight'}
    assert not set(sd) & set(synth_weights['fastpitch'])                         # fastpitch_state_dict itself is unchanged (conftest pins it)
    # gain scales the last conv of both encoders and nothing else
    sd4 = synth.fastpitch_aligner_state_dict(gain=4.0)
    for k in sd:
        last = k.startswith('attention.key_proj.2.') or k.startswith('attention.query_proj.4.')
        assert np.array_equal(sd4[k], sd[k]) != last, k


def test_fastpitch_keeps_attention_tensors_apart(tmp_path, synth_weights):
    """FastPitch(checkpoint): `attention.*` in a dict of its own, state_dict() as before; without them align() names what is missing."""
    import torch
    import text
    from ttsamd import synth
    from ttsamd.config import NET_CONFIG
    from ttsamd.lib import TtsAmdError
    from models.fastpitch.networks import FastPitch
    full = dict(synth_weights['fastpitch'])
    full.update(synth.fastpitch_aligner_state_dict())
    for name, sd in (('with', full), ('without', synth_weights['fastpitch'])):
        torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in sd.items()}, 'config': dict(NET_CONFIG), 'symbols': list(text.symbols)},
                   tmp_path / f'{name}.pth')
    m = FastPitch(str(tmp_path / 'with.pth'))
    assert set(m.state_dict()) == set(synth_weights['fastpitch']) and len(m._attn_sd) == 10 and not m._aligners
    m0 = FastPitch(str(tmp_path / 'without.pth'))
    assert set(m0.state_dict()) == set(m.state_dict()) and not m0._attn_sd
    with pytest.raises(TtsAmdError):                                             # on the CPU: no fallback
        m.align(np.ones((1, 3), np.int64), np.zeros((1, 80, 5), np.float32))
