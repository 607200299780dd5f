"""The look-ahead limiter on the GPU (pytest -m gpu): ttsamd_wave_limit (csrc/limiter.hip), LoudnessEngine.limit, utils.audio.limit,
`limiter=` of the tts wrappers and of the streams, against the numpy restatement tests/limiter_ref.py.

The gain-reduction curve is integer arithmetic and the rest is stated operation by operation in include/ttsamd.h, so y, gain and
reduction are compared BIT FOR BIT; the restatement is fed the kernel's own gain_out, which is held to one fp32 step of the float64
formula on its own (the device's 10^x may differ from numpy's in the last bits of float64, and the result is rounded once to fp32).

Sizes: the kernel's tile T = LIMITER_TILE samples at k T - 1, k T, k T + 1 for k = 1, 2, 3; lengths around the attack A and the hold R
(0, 1, 2, 3, A, A + 1, 2A + 1, R, R + A + 1); A = 0, A = R, R > n and the limits A = 1024, R = 4096.  Impulses at 0, n - 1, each tile
edge +- 1 and two impulses R apart."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import limiter_ref as R
import loudness_ref as LR
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

EINVAL = -1
Q = R.Q
T = 2048


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def eng(dev):
    from ttsamd.engine import LIMITER_TILE, leveller
    assert LIMITER_TILE == T
    return leveller(22050, dev)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _row(n, seed, Rh, sigma=0.05):
    """noise with impulses at 0, n - 1, every tile edge +- 1 and a pair R apart (where the row has room for them)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * sigma).astype(np.float32)
    spots = [0, n - 1] + [k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)] + [n // 3, n // 3 + Rh]
    for k, p in enumerate(spots):
        if 0 <= p < n:
            x[p] = np.float32((0.5 + 0.05 * (k % 9)) * (-1) ** k)
    return x


def _poisoned(xs, dev, stride=None):
    stride = stride or max(1, max(len(x) for x in xs))
    buf = np.full((len(xs), stride), np.nan, dtype=np.float32)
    for b, x in enumerate(xs):
        buf[b, :len(x)] = x
    return torch.from_numpy(buf).to(dev), torch.tensor([len(x) for x in xs], dtype=torch.int64, device=dev)


def _run(eng, xs, A, Rh, gains_db, c=0.99, max_gain=1e6, stride=None):
    """mode 3 on a NaN-poisoned ragged batch -> (rows of y, gain fp32 [B], reduction int32 [B], what lies behind the rows)"""
    dev = eng.device
    wave, lens = _poisoned(xs, dev, stride)
    B = len(xs)
    mode = torch.full((B,), 3, dtype=torch.int32, device=dev)
    target = torch.tensor(list(gains_db), dtype=torch.float32).to(dev)
    out, gain, red = eng.limit_samples(wave, lens, mode, target, c, max_gain, A, Rh)
    assert out.data_ptr() == wave.data_ptr() and gain.dtype == torch.float32 and red.dtype == torch.int32
    out = out.cpu().numpy()
    behind = np.concatenate([out[b, len(x):] for b, x in enumerate(xs)])
    return [out[b, :len(x)] for b, x in enumerate(xs)], gain.cpu().numpy(), red.cpu().numpy(), behind


def _check_rows(xs, ys, gain, red, A, Rh, c, what):
    hit = 0
    for b, (x, y) in enumerate(zip(xs, ys)):
        want, want_red = R.limit(x, gain[b], np.float32(c), A, Rh)
        assert np.array_equal(R.bits(y), R.bits(want)), (what, b, len(x), np.flatnonzero(R.bits(y) != R.bits(want))[:8])
        assert int(red[b]) == want_red, (what, b, len(x))
        assert len(x) == 0 or np.abs(y).max() <= np.float32(c)
        hit += want_red < Q
    return hit


GROUPS = {
    'small': (5, 40, [0, 1, 2, 3, 5, 6, 11, 40, 46, 333]),
    'tiles': (5, 40, [k * T + d for k in (1, 2, 3) for d in (-1, 0, 1)]),
    'default': (33, 331, [33, 34, 67, 331, 365, T + 1, 2 * T - 1]),
    'no_attack': (0, 0, [1, 2, 77, T + 1]),
    'no_attack_hold': (0, 7, [1, 7, 8, 2 * T]),
    'attack_is_hold': (33, 33, [33, 34, 67, 500, T + 1]),
    'hold_past_the_row': (5, 400, [1, 100, 399, 406]),
    'longest_attack': (1024, 1024, [1024, 1025, 2049, 2 * T + 1]),
    'limits': (1024, 4096, [3, 4096, 5121, 3 * T + 1]),
    'longest_hold': (7, 4096, [T - 1, 2 * T + 1]),
}


@pytest.mark.parametrize('name', list(GROUPS))
def test_rows_against_the_restatement(eng, name):
    """every length of the group alone and all of them in one NaN-poisoned ragged batch: the restatement's bits both times"""
    A, Rh, sizes = GROUPS[name]
    xs = [_row(n, 1000 + n, Rh) for n in sizes]
    db = [12.0 + (k % 3) for k in range(len(xs))]
    ys, gain, red, behind = _run(eng, xs, A, Rh, db)
    assert np.isnan(behind).all()                                        # nothing behind a row's length was written
    for b in range(len(xs)):
        assert gain[b] == np.float32(R.row_gain(3, db[b], 1e6)) or abs(float(gain[b]) / R.row_gain(3, db[b], 1e6) - 1) < 1.2e-7
    hit = _check_rows(xs, ys, gain, red, A, Rh, 0.99, name)
    assert hit == len([n for n in sizes if n > 0]), 'every row has an impulse that the gain lifts over the ceiling'
    for b, x in enumerate(xs):
        y1, g1, r1, _ = _run(eng, [x], A, Rh, [db[b]])
        assert g1[0] == gain[b] and r1[0] == red[b] and np.array_equal(R.bits(y1[0]), R.bits(ys[b])), (name, b)


def test_two_runs_and_other_ceilings(eng):
    xs = [_row(n, 7 + n, 331, sigma=0.2) for n in (3 * T + 5, T, 777)]
    for c in (0.5, 1.0, 0.25):
        a = _run(eng, xs, 33, 331, [6.0, 3.0, 20.0], c=c)
        b = _run(eng, xs, 33, 331, [6.0, 3.0, 20.0], c=c)
        assert all(np.array_equal(R.bits(u), R.bits(v)) for u, v in zip(a[0], b[0])) and np.array_equal(a[2], b[2])
        assert _check_rows(xs, a[0], a[1], a[2], 33, 331, c, f'ceiling {c}') == 3
    # a stride that is no multiple of four samples: the rows start off the 16-byte grid
    a = _run(eng, xs[1:], 33, 331, [6.0, 20.0], stride=T + 3)
    _check_rows(xs[1:], a[0], a[1], a[2], 33, 331, 0.99, 'odd stride')


def test_row_under_the_ceiling_is_the_plain_product(eng):
    x = (np.random.default_rng(5).uniform(-0.2, 0.2, 2 * T + 9)).astype(np.float32)
    ys, gain, red, _ = _run(eng, [x], 33, 331, [12.0])
    assert red[0] == Q and np.array_equal(R.bits(ys[0]), R.bits(x * gain[0]))


def test_gain_from_the_loudness_and_the_clamp(eng, dev):
    xs = [(np.random.default_rng(s).standard_normal(n) * a).astype(np.float32) for s, n, a in ((1, 22050, 0.02), (2, 9000, 0.1), (3, 30000, 0.002))]
    wave, lens = _poisoned(xs, dev)
    loud = eng.measure(wave, lens)[0].cpu().numpy()
    targets = [-16.0, -23.0, -14.0]
    out, gain, red = eng.limit(wave, lens, 2, targets, max_gain_db=30.0)
    gain = gain.cpu().numpy()
    for b in range(3):
        g64 = R.row_gain(2, targets[b], 10 ** 1.5, loud[b])
        gf = np.float32(g64)
        print(f'row {b}: L {loud[b]:.4f} LUFS, gain {gain[b]!r}, float64 formula {g64!r}')
        assert gain[b] in (np.nextafter(gf, np.float32(0)), gf, np.nextafter(gf, np.float32(np.inf))), b
        assert np.array_equal(R.bits(out[b, :len(xs[b])].cpu().numpy()), R.bits(R.limit(xs[b], gain[b], np.float32(0.99), 33, 331)[0]))
    assert 10 ** ((-14.0 - loud[2]) / 20) > 10 ** 1.5 and gain[2] == np.float32(10 ** 1.5)      # row 2 asks for more than 30 dB
    _, g2, _ = eng.limit(_poisoned(xs, dev)[0], lens, 2, targets, max_gain_db=6.0)
    assert g2.cpu().numpy().max() <= np.float32(10 ** 0.3) and g2[2] == np.float32(10 ** 0.3)
    _, g3, _ = eng.limit(_poisoned(xs, dev)[0], lens, ['gain', 'off', 3], [40.0, 40.0, -6.0], max_gain_db=20.0)
    assert float(g3[0]) == 10.0 and float(g3[1]) == 1.0 and abs(float(g3[2]) / 10 ** -0.3 - 1) < 1.2e-7      # 40 dB clamped to 20


def test_rows_that_are_left_alone(eng, dev):
    """silent and empty rows in mode 2, mode 0, a device mode outside the table and mode 2 without a loudness: gain 1, reduction Q,
    the samples untouched"""
    from ttsamd import lib
    h = lib.load()
    loud_row = (np.random.default_rng(4).standard_normal(9000) * 0.3).astype(np.float32)
    xs = [np.zeros(9000, np.float32), np.zeros(0, np.float32), loud_row, loud_row, loud_row]
    wave, lens = _poisoned(xs, dev)
    before = wave.clone()
    out, gain, red = eng.limit(wave, lens, [2, 2, 0, 2, 3], [-16.0, -16.0, -16.0, -6.0, 12.0])
    assert gain.cpu().tolist()[:3] == [1.0, 1.0, 1.0] and red.cpu().tolist()[:3] == [Q, Q, Q]
    assert torch.equal(out[:3].view(torch.int32), before[:3].view(torch.int32))
    assert float(gain[3]) > 1.0 and int(red[3]) < Q and int(red[4]) < Q
    assert not torch.equal(out[3], before[3]) and not torch.equal(out[4], before[4])
    # the C call with device modes 7 and -1, and mode 2 with loudness NULL
    wave = before.clone()
    mode = torch.tensor([7, -1, 2, 2, 1], dtype=torch.int32, device=dev)
    target = torch.full((5,), 12.0, dtype=torch.float32, device=dev)
    gain = torch.full((5,), 7.0, dtype=torch.float32, device=dev)
    red = torch.full((5,), 7, dtype=torch.int32, device=dev)
    nb = h.ttsamd_wave_limit_workspace_bytes(5, wave.shape[1])
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    assert h.ttsamd_wave_limit(_ptr(wave), wave.shape[1], _ptr(lens), 5, _ptr(mode), _ptr(target), 0.99, 31.6, 33, 331, None, _ptr(gain),
                               _ptr(red), _ptr(ws), nb, _stream()) == 0, h.ttsamd_last_error()
    assert gain.cpu().tolist() == [1.0] * 5 and red.cpu().tolist() == [Q] * 5
    assert torch.equal(wave.view(torch.int32), before.view(torch.int32))


def test_refusals(eng, dev):
    from ttsamd import lib
    from ttsamd.lib import TtsAmdError
    h = lib.load()
    x = _row(T + 7, 3, 331)
    wave, lens = _poisoned([x], dev)
    before = wave.clone()
    n = wave.shape[1]
    mode = torch.tensor([3], dtype=torch.int32, device=dev)
    target = torch.tensor([12.0], dtype=torch.float32, device=dev)
    gain = torch.full((1,), 7.0, dtype=torch.float32, device=dev)
    red = torch.full((1,), 7, dtype=torch.int32, device=dev)
    nb = h.ttsamd_wave_limit_workspace_bytes(1, n)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def call(wave_=wave, lens_=lens, B=1, mode_=mode, target_=target, c=0.99, mg=31.6, A=33, Rh=331, gain_=gain, red_=red, ws_=ws, nb_=nb):
        return h.ttsamd_wave_limit(_ptr(wave_), n, _ptr(lens_), B, _ptr(mode_), _ptr(target_), c, mg, A, Rh, None, _ptr(gain_), _ptr(red_),
                                   _ptr(ws_), nb_, _stream())
    for kw in (dict(wave_=None), dict(lens_=None), dict(mode_=None), dict(target_=None), dict(gain_=None), dict(red_=None), dict(ws_=None),
               dict(B=0), dict(B=-1), dict(c=0.0), dict(c=1.5), dict(c=float('nan')), dict(mg=0.0), dict(mg=-1.0), dict(mg=float('inf')),
               dict(A=-1), dict(A=332), dict(A=1025, Rh=1025), dict(Rh=4097), dict(nb_=nb - 1), dict(nb_=0)):
        assert call(**kw) == EINVAL, kw
        assert b'wave_limit' in h.ttsamd_last_error()
    torch.cuda.synchronize()
    assert float(gain[0]) == 7.0 and int(red[0]) == 7 and torch.equal(wave.view(torch.int32), before.view(torch.int32))      # nothing was launched
    assert call(A=1024, Rh=4096) == 0 and call(A=0, Rh=0, c=1.0) == 0
    for bad in (1, -1, 4, 'peak', 1.5, [0, 3], None, True):
        w2 = before.clone()
        with pytest.raises((TtsAmdError, ValueError)):
            eng.limit(w2, lens, bad, 0.0)
        assert torch.equal(w2.view(torch.int32), before.view(torch.int32))
    for bad in (dict(target=float('nan')), dict(ceiling=0.0), dict(ceiling=1.01), dict(attack_ms=50.0, hold_ms=60.0), dict(hold_ms=200.0),
                dict(max_gain_db=float('inf')), dict(attack_ms=-1.0)):
        with pytest.raises((TtsAmdError, ValueError)):
            eng.limit(before.clone(), lens, 3, **dict(dict(target=0.0), **bad))
    with pytest.raises(TtsAmdError):
        eng.limit(before.cpu(), lens, 3, 0.0)


def _speech_like(n, seed, amp):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / 22050.0
    return (rng.standard_normal(n) * amp * (0.55 + 0.45 * np.sin(2 * np.pi * 0.9 * t + seed))).astype(np.float32)


def test_row_under_the_ceiling_measures_at_the_target(eng, dev):
    x = _speech_like(3 * 22050 + 777, 11, 0.02)
    wave, lens = _poisoned([x], dev)
    out, gain, red = eng.limit(wave, lens, 2, -23.0)
    assert int(red[0]) == Q and float(gain[0]) * float(np.abs(x).max()) < 0.99
    again = eng.measure(out, lens)[0]
    print(f'limit towards -23 LUFS with nothing to limit: measures {float(again[0]):.7f}')
    assert abs(float(again[0]) + 23.0) < 1e-4


def test_spiky_row_gets_closer_to_the_target_than_the_cap(eng, dev):
    """a quiet row with a few large impulses: level() stops where the impulse meets the ceiling; limit() takes the full gain and
    reduces it around the impulses alone"""
    x = _speech_like(3 * 22050, 12, 0.01)
    for p in (5000, 30000, 30700, 61000):
        x[p] = 0.8
    target = -16.0
    L0 = LR.measure(x, 22050)['L']
    assert 0.8 * 10 ** ((target - L0) / 20) > 0.99
    wave, lens = _poisoned([x], dev)
    capped, _ = eng.level(wave.clone(), lens, 2, target)
    limited, gain, red = eng.limit(wave.clone(), lens, 2, target)
    Lc, Ll = float(eng.measure(capped, lens)[0][0]), float(eng.measure(limited, lens)[0][0])
    print(f'{L0:.2f} LUFS towards {target}: the cap ends at {Lc:.3f}, the limiter at {Ll:.3f} (reduction {int(red[0]) / Q:.4f})')
    assert abs(Lc - target) > 1.0 and abs(Ll - target) < abs(Lc - target) and int(red[0]) < Q
    assert float(limited[0, :len(x)].abs().max()) <= np.float32(0.99)


def test_audio_helpers(eng, dev):
    from utils import audio
    xs = [_row(T + 100, 21, 331, sigma=0.1), _row(900, 22, 331, sigma=0.1)]
    wave, lens = _poisoned(xs, dev)
    before = wave.clone()
    out, red_db = audio.limit(wave, gain_db=[6.0, 12.0], lens=lens)
    assert out.data_ptr() != wave.data_ptr() and torch.equal(wave.view(torch.int32), before.view(torch.int32))
    assert red_db.dtype == torch.float64 and red_db.shape == (2,) and float(red_db.max()) < 0.0
    for b, x in enumerate(xs):
        ys, gain, red, _ = _run(eng, [x], 33, 331, [[6.0, 12.0][b]])        # the engine call with the same gain in dB
        want, want_red = R.limit(x, gain[0], np.float32(0.99), 33, 331)
        got = out[b, :len(x)].cpu().numpy()
        assert np.array_equal(R.bits(got), R.bits(ys[0])) and np.array_equal(R.bits(got), R.bits(want)) and int(red[0]) == want_red
        assert abs(float(red_db[b]) - 20 * np.log10(want_red / Q)) < 1e-9
    one = torch.from_numpy(xs[1]).to(dev)
    y1, r1 = audio.limit(one, gain_db=12.0, ceiling=0.5, attack_ms=0.5, hold_ms=2.0)
    assert y1.shape == one.shape and float(y1.abs().max()) <= 0.5 and r1.shape == (1,)
    spiky = _speech_like(2 * 22050, 31, 0.01)
    spiky[7000] = 0.9
    w = torch.from_numpy(spiky).to(dev)
    a, b = audio.normalize_loudness(w, target_lufs=-16.0), audio.normalize_loudness(w, target_lufs=-16.0, limiter=True)
    La, Lb = float(audio.loudness(a)[0]), float(audio.loudness(b)[0])
    assert abs(Lb + 16.0) < abs(La + 16.0) and float(b.abs().max()) <= np.float32(0.99)
    c = audio.normalize_loudness(w, target_lufs=-16.0, peak_ceiling=0.5, limiter=dict(hold_ms=10.0))
    assert float(c.abs().max()) <= 0.5


# ---- through the models ----
@pytest.fixture(scope='module')
def model(tmp_path_factory, synth_weights, dev):
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
    d = tmp_path_factory.mktemp('ckpt_limit')
    torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['fastpitch'].items()}, 'config': dict(NET_CONFIG),
                'symbols': list(text.symbols)}, d / 'fp.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, d / 'hg.pth')
    with open(d / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    return FastPitch2Wave(str(d / 'fp.pth'), vocoder_sd=str(d / 'hg.pth'), vocoder_config=str(d / 'config.json')).to(dev)


@pytest.fixture(scope='module')
def lines():
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        every = json.load(f)
    return [every[i] for i in (68, 14, 92, 63, 35)]


@pytest.fixture(scope='module')
def plain(model, lines):
    return {bs: model.tts(lines, batch_size=bs) for bs in (1, 2, 32)}


OPTIONS = [-16.0, 'peak', None, 'lufs', -14.0]
HOT = [-3.0, 'peak', None, 0.0, -6.0]          # targets that lift the synthetic waves' peaks (crest factor about 13 dB) over the ceiling


@pytest.mark.parametrize('batch_size', [1, 2, 32])
def test_tts_with_a_limiter_is_the_manual_composition(model, lines, plain, batch_size, eng):
    """wave i = the plain wave of the same path, through LoudnessEngine.limit in mode 2 where its option is 'lufs' or a target and
    through today's level() where it is 'peak', bit for bit; one target for all lines and per-line lists, among them targets at which
    the limiter has work"""
    from ttsamd.engine import level_spec
    limited = 0
    for options in (-16.0, OPTIONS, HOT):
        waves = model.tts(lines, batch_size=batch_size, normalize=options, limiter=True)
        for i, (w, p) in enumerate(zip(waves, plain[batch_size])):
            opt = options[i] if isinstance(options, list) else options
            if opt is None:
                want = p
            else:
                mode, target = level_spec(opt)
                row = p.to(model.device)[None].contiguous()
                if mode == 2:
                    out, _, red = eng.limit(row, None, 2, target)
                    limited += int(red[0]) < Q
                    assert float(out.abs().max()) <= np.float32(0.99)
                else:
                    out, _ = eng.level(row, None, mode, target)
                want = out[0].cpu()
            assert w.shape == p.shape and torch.equal(w.view(torch.int32), want.view(torch.int32)), (batch_size, i, opt)
    print(f'batch_size {batch_size}: the limiter had work on {limited} waves')
    assert limited >= 3, 'the hot targets were to be limited: the comparison would be a plain gain'
    ceil = model.tts(lines, batch_size=batch_size, normalize=-10.0, limiter=dict(ceiling=0.5, hold_ms=10.0))
    for w, p in zip(ceil, plain[batch_size]):
        out, _, _ = eng.limit(p.to(model.device)[None].contiguous(), None, 2, -10.0, ceiling=0.5, hold_ms=10.0)
        assert torch.equal(w.view(torch.int32), out[0].cpu().view(torch.int32)) and float(w.abs().max()) <= 0.5


@pytest.mark.parametrize('batch_size', [1, 2, 32])
def test_tts_without_a_limiter_keeps_its_bits(model, lines, plain, batch_size):
    from ttsamd.engine import level_spec, leveller
    lv = leveller(22050, model.device)
    for kw in (dict(), dict(limiter=False), dict(limiter=None)):
        waves = model.tts(lines, batch_size=batch_size, normalize=OPTIONS, **kw)
        for w, p, opt in zip(waves, plain[batch_size], OPTIONS):
            want = p if opt is None else lv.level(p.to(model.device)[None].contiguous(), None, *level_spec(opt))[0][0].cpu()
            assert torch.equal(w.view(torch.int32), want.view(torch.int32))
    with pytest.raises(ValueError):
        model.tts(lines, batch_size=batch_size, limiter=True)
    wave, n = model.tts_batch_device(lines, denoise=0.005, normalize=OPTIONS, limiter=True)
    for b, w in enumerate(model.tts(lines, batch_size=32, normalize=OPTIONS, limiter=True)):
        assert int(n[b]) == w.numel() and torch.equal(wave[b, :w.numel()].cpu().view(torch.int32), w.view(torch.int32))


# ---- inside a stream ----
# The tiny generators of tests/test_gpu_stream.py and tests/test_gpu_vocos_stream.py, utterances of 1 .. 70 frames in one pool, first
# chunk 4 frames, then 8.  The vocoder's fp32 sums depend on where a sample lies in its window, so "the unlimited stream" is the same
# StreamingVocoder with `bypass` set: the same windows, the same launches, the samples the limiter works on.  Every utterance's gain
# lifts its peak to twice the ceiling, so the limiter has work on every utterance; max_gain_db is out of the way (utils.audio.limit
# has no such clamp).
TS = [1, 2, 3, 13, 14, 40, 70]
STRENGTHS = [0.0, 0.0, 0.01, 0.0, 0.01, 0.01, 0.0]
HOP = 256


def _mel(C_, T_, seed):
    return (np.random.default_rng(seed).standard_normal((C_, T_)) * 1.5 - 4.0).astype(np.float32)


def _stream_run(sv, mels, strengths, gains, tap=False):
    """open every mel, step until all have closed -> ({i: [chunks on the host]}, {i: [float cores of the window rows]} with tap,
    the smallest reduction over all steps).  tap reads the cores out of the window buffer the emit reads (the samples at the vocoder's
    rate behind the limiter, whatever rate and encoding the chunks leave in)."""
    sid_of = {sv.open(torch.from_numpy(m).to(sv.device), strengths[i], gains[i]): i for i, m in enumerate(mels)}
    got, cores, red_min, steps = {i: [] for i in range(len(mels))}, {i: [] for i in range(len(mels))}, Q, 0
    while sv.open_streams:
        rows = [(st.sid, st.plan[st.next]) for st in list(sv._open.values())[:sv._rows]]
        res = sv.step()
        steps += 1
        assert [sid for sid, _, _ in res] == [sid for sid, _ in rows] and steps < 200
        if sv.reduction is not None and not sv.bypass:
            red_min = min(red_min, int(sv.reduction.min()))
        w_max = (max(c[3] for _, c in rows) + 3) & ~3
        win = sv._wave[:len(rows) * HOP * w_max].view(len(rows), HOP * w_max).cpu() if tap else None
        for w, ((sid, chunk, _), (_, c)) in enumerate(zip(res, rows)):
            got[sid_of[sid]].append(chunk.cpu())
            if tap:
                cores[sid_of[sid]].append(win[w, HOP * (c[0] - c[2]):HOP * (c[0] - c[2] + c[1])].clone())
    return got, cores, red_min


def _gains_for(waves, ceiling=0.99):
    return [float(np.float32(20.0 * np.log10(2.0 * ceiling / float(w.abs().max())))) for w in waves]


def _check_stream(make_sv, mels, strengths, sample_rate=22050):
    from utils import audio
    sv = make_sv()
    sv.bypass = True
    plain, _, _ = _stream_run(sv, mels, strengths, [0.0] * len(mels))
    plain = [torch.cat(plain[i]) for i in range(len(mels))]
    gains = _gains_for(plain)
    sv.bypass = False
    got, _, red_min = _stream_run(sv, mels, strengths, gains)
    assert red_min < Q, 'no chunk was limited: the comparison would be vacuous'
    for i, u in enumerate(plain):
        want, red_db = audio.limit(u.to(sv.device), gain_db=gains[i], sample_rate=sample_rate, **{k: sv._lim[k] for k in ('ceiling', 'attack_ms', 'hold_ms')})
        y = torch.cat(got[i])
        assert float(red_db[0]) < 0.0 and y.shape == u.shape
        assert torch.equal(y.view(torch.int32), want.cpu().view(torch.int32)), (i, int((y != want.cpu()).sum()))
        assert float(y.abs().max()) <= np.float32(sv._lim['ceiling'])
    return plain


@pytest.fixture(scope='module')
def v1(dev, synth_weights):
    from ttsamd.config import HIFIGAN_CONFIG
    from vocoder.hifigan.denoiser import Denoiser
    from vocoder.hifigan.models import Generator
    gen = Generator(dict(HIFIGAN_CONFIG), state_dict={k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}).to(dev)
    return gen, Denoiser(gen)


SV_KW = dict(max_streams=8, max_frames=96, chunk_frames=8, first_chunk_frames=4)


def test_hifigan_stream_with_denoise_on_some_rows(v1):
    from conftest import WAVE_TOL
    from ttsamd.stream import StreamingVocoder, limiter_halo_frames
    mels = [_mel(80, T_, 100 + T_) for T_ in TS]
    lim = dict(max_gain_db=120.0)
    plain = _check_stream(lambda: StreamingVocoder(v1[0], v1[1], limiter=lim, **SV_KW), mels, STRENGTHS)
    assert limiter_halo_frames(33, 331, 256) == 2 and limiter_halo_frames(1024, 4096, 256) == 20 and limiter_halo_frames(0, 0, 256) == 0
    # the bypassed stream against the stream without a limiter: other windows, so fp32 summation order, each within WAVE_TOL of the oracle
    sv0 = StreamingVocoder(v1[0], v1[1], **SV_KW)
    base, _, _ = _stream_run(sv0, mels, STRENGTHS, [0.0] * len(mels))
    assert sv0.reduction is None
    assert max(float((torch.cat(base[i]) - plain[i]).abs().max()) for i in range(len(TS))) < 2 * WAVE_TOL
    with pytest.raises(ValueError):
        sv0.open(torch.from_numpy(mels[3]).to(sv0.device), 0.0, 6.0)          # a gain without a limiter
    with pytest.raises(ValueError):
        sv0.open(torch.from_numpy(mels[3]).to(sv0.device), 0.0, float('nan'))
    assert sv0.free_slots == sv0.max_streams
    with pytest.raises(ValueError):
        StreamingVocoder(v1[0], v1[1], limiter=dict(hold_ms=500.0), **SV_KW)


def test_vocos_22k_stream(dev):
    from ttsamd import synth
    from ttsamd.config import VOCOS_22K_CONFIG
    from ttsamd.stream import StreamingVocoder
    from vocoder.vocos import MelVocos
    voc = MelVocos('22k')
    voc.load_state_dict({k: torch.from_numpy(v) for k, v in synth.vocos_state_dict(VOCOS_22K_CONFIG).items()})
    voc = voc.to(dev)
    mels = [_mel(VOCOS_22K_CONFIG['input_channels'], T_, 200 + T_) for T_ in TS]
    lim = dict(max_gain_db=120.0, hold_ms=30.0, ceiling=0.9)
    _check_stream(lambda: StreamingVocoder(voc, limiter=lim, **SV_KW), mels, [0.0, 0.3, 0.0, 0.0, 0.3, 0.0, 0.3])


def test_hifigan_stream_as_8k_mulaw(v1):
    """the chunks leave at 8 kHz as G.711 mu-law: put together they are resample + encode of the whole limited wave, whose float samples
    at 22 050 Hz are read out of the window rows behind the limiter"""
    from ttsamd.stream import StreamingVocoder
    from utils import audio
    mels = [_mel(80, T_, 100 + T_) for T_ in TS]
    sv = StreamingVocoder(v1[0], v1[1], limiter=dict(max_gain_db=120.0), sample_rate=8000, encoding='mulaw', **SV_KW)
    sv.bypass = True
    _, cores, _ = _stream_run(sv, mels, STRENGTHS, [0.0] * len(mels), tap=True)
    plain = [torch.cat(cores[i]) for i in range(len(mels))]
    gains = _gains_for(plain)
    sv.bypass = False
    got, cores, red_min = _stream_run(sv, mels, STRENGTHS, gains, tap=True)
    assert red_min < Q
    for i, u in enumerate(plain):
        limited, _ = audio.limit(u.to(sv.device), gain_db=gains[i])
        assert torch.equal(torch.cat(cores[i]).view(torch.int32), limited.cpu().view(torch.int32)), i
        want = audio.encode(audio.resample(limited[None], 22050, 8000), 'mulaw')[0].cpu()
        y = torch.cat(got[i])
        assert y.dtype == torch.uint8 and y.shape == want.shape and torch.equal(y, want), i


def test_tts_stream_takes_gain_and_limiter(model, lines):
    from utils import audio
    kw = dict(chunk_frames=16, first_chunk_frames=8, denoise=0.0)
    with pytest.raises(ValueError):
        list(model.tts_stream(lines[0], gain_db=6.0, **kw))
    with pytest.raises(ValueError):
        list(model.tts_stream(lines[:2], gain_db=[6.0], limiter=True, **kw))
    sv_kw = dict(limiter=dict(max_gain_db=120.0), **kw)
    y0 = torch.cat(list(model.tts_stream(lines[0], gain_db=0.0, **sv_kw)))
    model._stream_voc.bypass = True
    u = torch.cat(list(model.tts_stream(lines[0], **sv_kw)))
    model._stream_voc.bypass = False
    g = _gains_for([u])[0]
    y = torch.cat(list(model.tts_stream(lines[0], gain_db=g, **sv_kw)))
    want, red_db = audio.limit(u.to(model.device), gain_db=g)
    assert float(red_db[0]) < 0.0 and torch.equal(y.view(torch.int32), want.cpu().view(torch.int32))
    assert torch.equal(y0.view(torch.int32), audio.limit(u.to(model.device))[0].cpu().view(torch.int32))
    parts = {}
    for i, chunk, last in model.tts_stream(lines[:3], gain_db=[g, 0.0, g + 3.0], **sv_kw):
        parts.setdefault(i, []).append(chunk)
    assert sorted(parts) == [0, 1, 2] and [torch.cat(parts[i]).numel() for i in (0,)] == [y.numel()]
    assert all(float(torch.cat(parts[i]).abs().max()) <= np.float32(0.99) for i in parts)
