"""GPU: the forced-alignment kernels (csrc/aligner.hip) through the C ABI and the drop-ins.  MAS is compared element for element with the
fp32 restatement of the reference's mas_width1 (tests/aligner_ref.py, which tests/test_aligner_cpu.py pins to the reference's goldens); the
attention with the float64 restatement inside 4 x the reference's own recorded noise floor (the kernel sums the same 80 squares and the same
convs in another order: the same error class as the reference's own fp32); average_pitch with float64."""
import numpy as np
import pytest
import torch

import aligner_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _mas(x, in_lens=None, out_lens=None, **kw):
    """x [B, T, L] numpy -> (dur [B, L], hard [B, T, L]) numpy through ttsamd_mas"""
    from ttsamd import engine as E
    B, T, Lt = x.shape
    il = torch.tensor([Lt] * B if in_lens is None else in_lens, dtype=torch.int64)
    ol = torch.tensor([T] * B if out_lens is None else out_lens, dtype=torch.int64)
    dur, hard = E.mas(torch.from_numpy(np.ascontiguousarray(x)).to(DEV), il, ol, **kw)
    return dur.cpu().numpy(), hard.cpu().numpy()


def _log_attn(seed, T, Lt, sharp=3.0):
    """a log-attention with a noisy diagonal ridge: paths that wander, decisions of every size"""
    rng = np.random.default_rng(seed)
    t, l = np.arange(T)[:, None] / max(T - 1, 1), np.arange(Lt)[None, :] / max(Lt - 1, 1)
    a = rng.normal(0, 1.5, (T, Lt)) - sharp * np.abs(t - l) * np.sqrt(Lt)
    a = a - a.max(1, keepdims=True)
    return (a - np.log(np.exp(a).sum(1, keepdims=True))).astype(np.float32)


def _check(x, what):
    dur, hard = _mas(x[None])
    want = R.mas_width1(x)
    assert np.array_equal(hard[0], want), what
    assert np.array_equal(dur[0], want.sum(0)), what


# (T, L): the lane, wave and multi-wave hand-offs (63 / 64 / 65, 129, 257, 1024), one token, one frame, T == L, T < L, and decision bits
# that leave a single word (257), the LDS (1300 x 64 with one wave, 700 x 257 with two, 1100 x 1024 with four)
SHAPES = [(9, 1), (7, 2), (100, 63), (101, 64), (102, 65), (65, 65), (1, 65), (160, 129), (300, 257), (5, 9), (1, 1), (300, 300),
          (1300, 64), (700, 257), (1100, 1024), (40, 1024)]


@pytest.mark.parametrize('T,Lt', SHAPES)
def test_mas_equals_the_restatement(T, Lt):
    _check(_log_attn(1000 + T + Lt, T, Lt), (T, Lt, 'ridge'))


@pytest.mark.parametrize('T,Lt', [(5, 9), (70, 65), (300, 257), (700, 257)])
def test_mas_ties_and_minus_infinity(T, Lt):
    _check(np.zeros((T, Lt), np.float32), (T, Lt, 'all equal: every decision a tie'))
    x = _log_attn(7, T, Lt)
    x[np.random.default_rng(8).random((T, Lt)) < 0.15] = -np.inf
    _check(x, (T, Lt, '-inf entries'))
    x[:] = -np.inf
    _check(x, (T, Lt, 'all -inf'))


def test_mas_golden_equals_the_reference(golden):
    g = golden('aligner')
    dur, hard = _mas(g['log_attn'][:, 0], g['in_lens'], g['mel_lens'])
    assert np.array_equal(hard, g['attn_hard'][:, 0].astype(np.float32))
    assert np.array_equal(dur, g['dur'])
    # from the probabilities: the kernel takes logf of the stored fp32 value itself (model.py:248)
    dur2, hard2 = _mas(g['attn_soft'][:, 0], g['in_lens'], g['mel_lens'], is_log=False)
    assert np.array_equal(hard2, hard) and np.array_equal(dur2, dur)


def test_mas_ragged_batch_and_limits():
    from ttsamd import engine as E
    from ttsamd.lib import TtsAmdError
    T, Lt = 90, 70
    x = np.stack([_log_attn(20 + b, T, Lt) for b in range(4)])
    in_lens, out_lens = [70, 33, 1, 50], [90, 40, 17, 0]
    dur, hard = _mas(x, in_lens, out_lens)
    want = R.b_mas(x[:, None], in_lens, out_lens)[:, 0]
    assert np.array_equal(hard, want) and np.array_equal(dur, want.sum(1))
    assert not hard[3].any() and hard[2, :17, 0].all() and hard[2].sum() == 17       # no frames: zeros; one token: every frame to token 0
    dur_only, none = E.mas(torch.from_numpy(x).to(DEV), torch.tensor(in_lens), torch.tensor(out_lens), return_hard=False)
    assert none is None and np.array_equal(dur_only.cpu().numpy(), dur)
    with pytest.raises(TtsAmdError):
        E.mas(torch.zeros(1, 2, 1025, device=DEV), torch.tensor([1025]), torch.tensor([2]))
    assert E.L.load().ttsamd_mas_workspace_bytes(1, 2, 1025) == -1


@pytest.fixture(scope='module')
def gold(golden):
    from ttsamd import synth
    g = golden('aligner')
    sd = synth.fastpitch_state_dict()
    sd.update(synth.fastpitch_aligner_state_dict(gain=float(g['gain'])))
    return g, sd


@pytest.fixture(scope='module')
def yardstick(gold):
    """the float64 restatement of both attention cases, computed once"""
    g, sd = gold
    return {tag: R.attention(sd, g['ids'], g['mel'], g['in_lens'], g['prior'] if tag else None, np.float64) for tag in ('', '_prior')}


@pytest.mark.parametrize('tag', ['', '_prior'])
def test_attention_within_four_noise_floors_of_float64(gold, yardstick, tag):
    from ttsamd.engine import AlignerEngine
    g, sd = gold
    eng = AlignerEngine(sd)
    soft, logprob, in_lens = eng.attention(g['ids'], g['mel'], g['prior'] if tag else None)
    assert soft.shape == logprob.shape == g['attn_soft'].shape and np.array_equal(in_lens.cpu().numpy(), g['in_lens'])
    soft, logprob = soft.cpu().numpy(), logprob.cpu().numpy()
    for key, got, want in (('attn_soft', soft, yardstick[tag][0]), ('attn_logprob', logprob, yardstick[tag][1])):
        floor = float(g['floor_' + key + tag])
        err = float(np.abs(got - want).max())
        print(f'{key}{tag}: max |kernel - float64| {err:.3e} = {err / floor:.2f} x the reference\'s own floor {floor:.3e}')
        assert err <= 4 * floor, (key + tag, err, floor)
    masked = np.arange(g['ids'].shape[1])[None, None, None, :] >= g['in_lens'][:, None, None, None]
    assert not (soft * masked).any()                                                # exactly 0 past in_lens
    assert np.abs(soft.sum(-1, dtype=np.float64) - 1).max() < 1e-6


@pytest.fixture(scope='module')
def checkpoints(gold, tmp_path_factory):
    import text
    from ttsamd.config import NET_CONFIG
    g, sd = gold
    d = tmp_path_factory.mktemp('aligner')
    for name, keep in (('with', lambda k: True), ('without', lambda k: not k.startswith('attention.'))):
        torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in sd.items() if keep(k)}, 'config': dict(NET_CONFIG),
                    'symbols': list(text.symbols)}, d / f'{name}.pth')
    return d


def test_fastpitch_align_end_to_end(gold, checkpoints):
    from models.fastpitch.networks import FastPitch
    g, _ = gold
    m = FastPitch(str(checkpoints / 'with.pth')).to(DEV)
    res = m.align(g['ids'], g['mel'], g['mel_lens'], pitch=g['pitch'], energy=np.abs(g['pitch'][:, 0]), return_attn=True)
    assert np.array_equal(res.dur_tgt.cpu().numpy(), g['dur'])
    assert np.array_equal(res.dur_tgt.sum(1).cpu().numpy(), g['mel_lens'].astype(np.float32))
    assert np.array_equal(res.attn_hard.cpu().numpy(), g['attn_hard'].astype(np.float32))
    assert res.attn_soft.shape == res.attn_logprob.shape == g['attn_soft'].shape
    want = R.average_pitch(g['pitch'], g['dur'])
    err, floor = float(np.abs(res.pitch_tgt.cpu().numpy() - want).max()), float(g['floor_pitch_tgt'])
    print(f'pitch_tgt: max |kernel - float64| {err:.3e} = {err / floor:.2f} x the floor {floor:.3e}')
    assert res.pitch_tgt.shape == g['pitch_tgt'].shape and err <= 4 * floor
    e64 = np.log(1.0 + R.average_pitch(np.abs(g['pitch']), g['dur']))
    assert res.energy_tgt.shape == (3, 1, g['ids'].shape[1]) and np.abs(res.energy_tgt.cpu().numpy() - e64).max() < 1e-6
    # without the maps, and the targets feed infer() as they are
    plain = m.align(g['ids'], g['mel'], g['mel_lens'])
    assert plain.attn_soft is None and plain.pitch_tgt is None and torch.equal(plain.dur_tgt, res.dur_tgt)
    mel, dec_lens, *_ = m.infer(g['ids'], dur_tgt=res.dur_tgt, pitch_tgt=res.pitch_tgt)
    assert np.array_equal(dec_lens.cpu().numpy(), g['mel_lens']) and mel.shape[2] == int(g['mel_lens'].max())


def test_average_pitch_against_float64():
    from ttsamd import engine as E
    rng = np.random.default_rng(3)
    for F in (1, 3):
        B, T, Lt = 3, 57, 11
        pitch = rng.normal(0, 1, (B, F, T)).astype(np.float32)
        pitch[:, :, rng.random(T) < 0.3] = 0.0                                       # unvoiced frames
        dur = rng.integers(1, 6, (B, Lt)).astype(np.float32)
        dur[:, 4] = 0                                                                # a token without frames
        dur[1, 8:] = 0                                                               # a ragged batch: row 1 ends early, row 2 overruns T
        dur[2, -1] = 40
        s, e = int(dur[0, :6].sum()), int(dur[0, :7].sum())
        pitch[0, :, s:e] = 0.0                                                       # a token whose frames are all unvoiced
        got = E.average_pitch(torch.from_numpy(pitch).to(DEV), torch.from_numpy(dur).to(DEV)).cpu().numpy()
        want = R.average_pitch(pitch, dur)
        assert got.shape == (B, F, Lt)
        assert np.abs(got - want).max() <= 2.0 ** -23 * np.abs(want).max()           # float64 sum, rounded once
        assert not got[:, :, 4].any() and not got[0, :, 6].any() and not got[1, :, 8:].any()


def test_dropins(golden, checkpoints):
    from models.fastpitch.fastpitch import alignment, model
    from models.fastpitch.networks import FastPitch
    from ttsamd.lib import TtsAmdError
    g = golden('aligner')
    out = alignment.b_mas(g['log_attn'], g['in_lens'], g['mel_lens'], width=1)       # numpy in, numpy out, as in the reference
    assert isinstance(out, np.ndarray) and out.dtype == np.float32
    assert np.array_equal(out, g['attn_hard'].astype(np.float32))
    t, n = int(g['mel_lens'][1]), int(g['in_lens'][1])
    one = alignment.mas_width1(g['log_attn'][1, 0, :t, :n])
    assert isinstance(one, np.ndarray) and np.array_equal(one, out[1, 0, :t, :n])
    on_dev = alignment.b_mas(torch.from_numpy(g['log_attn']).to(DEV), torch.from_numpy(g['in_lens']), torch.from_numpy(g['mel_lens']))
    assert on_dev.device.type == 'cuda' and np.array_equal(on_dev.cpu().numpy(), out)
    pt = model.average_pitch(torch.from_numpy(g['pitch']).to(DEV), torch.from_numpy(g['dur']).to(DEV))
    assert np.abs(pt.cpu().numpy() - g['pitch_tgt']).max() <= 4 * float(g['floor_pitch_tgt'])
    m = FastPitch(str(checkpoints / 'without.pth')).to(DEV)
    with pytest.raises(TtsAmdError, match='attention.key_proj.0.conv.weight'):
        m.align(g['ids'], g['mel'], g['mel_lens'])
