"""CPU: the look-ahead limiter without a GPU -- the properties include/ttsamd.h claims for its arithmetic, on the numpy restatement
(tests/limiter_ref.py), and the host side of `limiter=` (parsing, the ValueErrors, attack and hold in samples, and the option's way
through the tts wrappers on the fake engines of tests/test_loudness_cpu.py)."""
import os

import numpy as np
import pytest
import torch

import limiter_ref as R

pytest.importorskip('ttsamd.lib')
from ttsamd import lib  # noqa: E402

if not os.path.exists(lib.LIB_PATH):
    pytest.skip('libttsamd.so not built', allow_module_level=True)

Q = R.Q
AR = [(A, R_) for A in (0, 1, 5) for R_ in sorted({A, A + 1, 40})]
CEILINGS = (0.99, 0.5, 1.0)


def _rows(seed, count=6):
    """random rows: speech-like noise with a few large impulses, lengths around the reach, gains up to 100"""
    rng = np.random.default_rng(seed)
    for k in range(count):
        n = int(rng.integers(1, 400))
        x = (rng.standard_normal(n) * 0.05).astype(np.float32)
        for _ in range(int(rng.integers(0, 4))):
            x[int(rng.integers(0, n))] = np.float32(rng.uniform(-1, 1))
        yield x, np.float32(rng.choice([0.5, 1.0, 3.0, 17.0, 100.0])), np.float32(CEILINGS[k % 3])


@pytest.mark.parametrize('A,Rh', AR)
def test_ceiling_holds_and_s_is_under_q(A, Rh):
    for x, g, c in _rows(100 * A + Rh):
        r = R.curves(x, g, c, A, Rh)
        assert (r['s'] <= r['q']).all() and (r['s'] >= 0).all() and (r['m'] <= r['q']).all()
        assert np.abs(r['y']).max() <= c, (A, Rh, float(g), float(c))
        assert r['y'].dtype == np.float32 and r['s'].dtype == np.int64


@pytest.mark.parametrize('A,Rh', AR)
def test_identity_when_nothing_exceeds_the_ceiling(A, Rh):
    rng = np.random.default_rng(7 + A + Rh)
    x = rng.uniform(-0.3, 0.3, 257).astype(np.float32)
    g = np.float32(3.0)
    y, red = R.limit(x, g, np.float32(0.99), A, Rh)
    assert red == Q and np.array_equal(R.bits(y), R.bits(x * g))
    # and away from a peak's reach [j - 2A, j + R + A]
    x[100] = 0.9
    r = R.curves(x, g, np.float32(0.99), A, Rh)
    far = np.ones(257, dtype=bool)
    far[max(100 - 2 * A, 0):100 + Rh + A + 1] = False
    assert np.array_equal(R.bits(r['y'][far]), R.bits(r['u'][far])) and (r['s'][far] == Q).all() and r['s'][100] < Q


@pytest.mark.parametrize('A,Rh', AR)
def test_single_impulse_dip_has_the_exact_integer_ramp(A, Rh):
    n, j = 400, 150
    x = np.zeros(n, dtype=np.float32)
    x[j] = 1.0
    g, c = np.float32(2.0), np.float32(0.5)
    r = R.curves(x, g, c, A, Rh)
    q0 = int(np.floor(0.5 / 2.0 * Q))
    assert r['q'][j] == q0 and (np.delete(r['q'], j) == Q).all()
    W = 2 * A + 1
    for i in range(n):
        # m is q0 on [j - A, j + R]; s[i] averages m over [i - A, i + A]: `low` of its W terms are q0
        low = max(0, min(i + A, j + Rh) - max(i - A, j - A) + 1)
        assert r['s'][i] == (low * q0 + (W - low) * Q) // W, i
    assert (r['s'][j:j + Rh - A + 1] == q0).all()                       # full reduction on [j, j + R - A]
    assert r['s'][j - 2 * A - 1] == Q and r['s'][j + Rh + A + 1] == Q   # nothing outside [j - 2A, j + R + A]
    if A:
        assert r['s'][j - 2 * A] < Q and r['s'][j + Rh + A] < Q
        assert (np.diff(r['s'][j - 2 * A - 1:j + 1]) <= 0).all() and (np.diff(r['s'][j + Rh - A:j + Rh + A + 2]) >= 0).all()


@pytest.mark.parametrize('A,Rh', AR)
def test_reach_invariance(A, Rh):
    """y[i] from x[i - A - R : i + 2A + 1] alone has the bits it has in the whole row (clamping at a cut edge is harmless)"""
    for x, g, c in _rows(900 + 10 * A + Rh, count=4):
        y = R.limit(x, g, c, A, Rh)[0]
        n = len(x)
        for i in sorted({0, 1, n // 3, n // 2, n - 2, n - 1} & set(range(n))):
            lo, hi = max(i - A - Rh, 0), min(i + 2 * A + 1, n)
            part = R.limit(x[lo:hi], g, c, A, Rh)[0]
            assert R.bits(part)[i - lo] == R.bits(y)[i], (i, n)


def test_non_finite_samples_stay_in_their_place():
    x = np.array([0.1, np.nan, 0.2, np.inf, 0.1, 0.1], dtype=np.float32)
    r = R.curves(x, np.float32(1.0), np.float32(0.99), 1, 2)
    assert r['q'][1] == Q and r['q'][3] == 0 and np.isnan(r['y'][1])


def test_gain_formula_and_modes():
    assert R.row_gain(0, -16.0, 31.6) is None and R.row_gain(1, 0.99, 31.6) is None and R.row_gain(2, -16.0, 31.6, None) is None
    assert R.row_gain(2, -16.0, 31.6, -np.inf) is None
    assert abs(R.row_gain(2, -16.0, 31.6, -26.0) - 10 ** 0.5) < 1e-12 and R.row_gain(2, -16.0, 2.0, -26.0) == 2.0
    assert abs(R.row_gain(3, 6.0, 31.6) - 10 ** 0.3) < 1e-12 and R.row_gain(3, 60.0, 31.6) == float(np.float32(31.6))


def test_attack_and_hold_in_samples():
    from ttsamd.engine import LIMITER_MAX_ATTACK, LIMITER_MAX_HOLD, LIMITER_Q, LIMITER_TILE, limiter_reach, limiter_samples
    assert (LIMITER_MAX_ATTACK, LIMITER_MAX_HOLD, LIMITER_Q) == (R.A_MAX, R.R_MAX, Q) and LIMITER_TILE >= LIMITER_MAX_ATTACK
    assert limiter_samples(1.5, 15.0, 22050) == (33, 331) == R.attack_hold(1.5, 15.0, 22050)
    assert limiter_samples(1.5, 15.0, 8000) == (12, 120) and limiter_samples(1.5, 15.0, 48000) == (72, 720)
    assert limiter_samples(5.0, 1.0, 22050) == (110, 110)                # hold is at least the attack
    assert limiter_samples(0, 0, 22050) == (0, 0)
    assert limiter_samples(1024 * 1000 / 22050, 4096 * 1000 / 22050, 22050) == (1024, 4096)
    for bad in ((50.0, 60.0), (1.5, 200.0), (-1.0, 15.0), (1.5, float('nan')), (True, 15.0), ('1', 15.0)):
        with pytest.raises(ValueError):
            limiter_samples(*bad, 22050)
    assert limiter_reach(33, 331) == (364, 66)


def test_limiter_option_parsing():
    from ttsamd.engine import LIMITER_DEFAULTS, check_limiter, limiter_spec
    assert limiter_spec(None) is None and limiter_spec(False) is None
    assert limiter_spec(True) == dict(ceiling=0.99, attack_ms=1.5, hold_ms=15.0, max_gain_db=30.0) == LIMITER_DEFAULTS
    assert limiter_spec({}) == LIMITER_DEFAULTS and limiter_spec(True) is not LIMITER_DEFAULTS
    assert limiter_spec(dict(ceiling=0.5, hold_ms=20)) == dict(ceiling=0.5, attack_ms=1.5, hold_ms=20.0, max_gain_db=30.0)
    for bad in (1, 'on', [True], dict(celing=0.9), dict(ceiling=0.0), dict(ceiling=1.5), dict(attack_ms=-1), dict(hold_ms=float('nan')),
                dict(max_gain_db='30'), dict(ceiling=True)):
        with pytest.raises(ValueError):
            limiter_spec(bad)
    assert check_limiter(False, None) is None and check_limiter(None, 'peak') is None
    assert check_limiter(True, -16.0) == LIMITER_DEFAULTS and check_limiter(True, [None, 'lufs'])['ceiling'] == 0.99
    for normalize in (None, [None, None]):
        with pytest.raises(ValueError):
            check_limiter(True, normalize)


LENGTHS = [3, 9, 1, 7, 5, 9, 2]
LINES = [str(i) for i in range(len(LENGTHS))]
NORM = [None, 'peak', -20.0, 'lufs', None, -16.0, 'peak']


def _fakes(monkeypatch):
    """the fakes of tests/test_loudness_cpu.py, with a recorder in place of level_waves that also takes `limiter`"""
    from models.fastpitch import networks as N
    from vocoder.hifigan.models import _HipModule
    monkeypatch.setattr(N.text, 'tokens_to_ids', lambda toks, table: toks)
    levelled = []

    class FakeFastPitch(N.FastPitch):
        def __init__(self):
            _HipModule.__init__(self)
            self.net_config = dict(n_speakers=4, padding_idx=0, n_symbols=100)
            self.phon_to_id, self.default_vowelizer = None, None

        def _tokenize(self, line, vowelizer=None):
            return [int(line) + 1] * LENGTHS[int(line)]

        def infer(self, ids, **kw):
            rows = [int(r[0]) - 1 for r in ids]
            lens = torch.tensor([LENGTHS[i] for i in rows])
            mel = torch.zeros(len(rows), 2, int(lens.max()))
            for b, i in enumerate(rows):
                mel[b, :, :LENGTHS[i]] = i
            return mel, lens, None, None, None

    class FakeVocoderEngine:
        hop = 4

        def forward(self, mel, lens):
            return mel[:, 0].repeat_interleave(4, dim=1)

    class FakeVocoder:
        def engine(self):
            return FakeVocoderEngine()

        def __call__(self, mel):
            return FakeVocoderEngine().forward(mel if mel.dim() == 3 else mel[None], None)

    class FakeDenoiser:
        def forward_batch(self, wave, n, strength, nsamples_min=None):
            return wave

        def __call__(self, wave, strength):
            return wave

    class FakeTts(N.FastPitch2Wave):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.model, self.vocoder, self.denoiser = FakeFastPitch(), FakeVocoder(), FakeDenoiser()

    def fake_level(wave, nsamples, normalize, sample_rate=22050, ceiling=0.99, **kw):
        levelled.append(([int(v) for v in wave[:, 0].tolist()], normalize, kw))
        return wave

    monkeypatch.setattr(N, 'level_waves', fake_level)
    return N, FakeTts(), levelled


def test_limiter_reaches_level_waves_with_its_lines(monkeypatch):
    from ttsamd.engine import LIMITER_DEFAULTS
    N, tts, levelled = _fakes(monkeypatch)
    spec = dict(LIMITER_DEFAULTS, ceiling=0.9)
    waves = tts.tts(LINES, batch_size=3, normalize=NORM, limiter=dict(ceiling=0.9))
    assert [int(w[0]) for w in waves] == list(range(7))
    assert [sorted(rows) for rows, *_ in levelled] == [[0, 1, 2], [3, 4, 5], [6]]
    for rows, options, kw in levelled:
        assert options == [NORM[i] for i in rows] and kw == dict(limiter=spec)
    # limiter=False (the default): level_waves gets exactly the arguments it got before
    levelled.clear()
    tts.tts(LINES, batch_size=3, normalize=NORM)
    tts.tts(LINES, batch_size=3, normalize=NORM, limiter=False)
    assert len(levelled) == 6 and all(kw == {} for *_, kw in levelled)
    # batch_size 1 on the one-stream path: a line without a level is not levelled, with or without a limiter
    levelled.clear()
    tts.tts(LINES, batch_size=1, normalize=NORM, limiter=True)
    assert [(rows, opt) for rows, opt, _ in levelled] == [([i], NORM[i]) for i in range(7) if NORM[i] is not None]
    assert all(kw == dict(limiter=LIMITER_DEFAULTS) for *_, kw in levelled)
    # a chunk whose lines ask for no level passes no limiter on
    levelled.clear()
    tts.tts(LINES[:4], batch_size=2, normalize=[None, None, -16.0, None], limiter=True)
    assert [(sorted(rows), kw) for rows, _, kw in levelled] == [([0, 1], {}), ([2, 3], dict(limiter=LIMITER_DEFAULTS))]
    levelled.clear()
    tts.tts_batch(LINES[:2], normalize=-16.0, limiter=True)
    tts.tts_single('3', normalize='lufs', limiter=True)
    assert [kw for *_, kw in levelled] == [dict(limiter=LIMITER_DEFAULTS)] * 2


def test_limiter_value_errors_come_before_any_work(monkeypatch):
    N, tts, levelled = _fakes(monkeypatch)
    for kw in (dict(limiter=True), dict(limiter=True, normalize=None), dict(limiter=True, normalize=[None] * 7),
               dict(limiter='yes', normalize=-16.0), dict(limiter=dict(knee=3), normalize=-16.0), dict(limiter=dict(ceiling=2.0), normalize='lufs')):
        with pytest.raises(ValueError):
            tts.tts(LINES, batch_size=3, **kw)
    with pytest.raises(ValueError):
        tts.tts_single('1', limiter=True)
    with pytest.raises(ValueError):
        tts.tts_batch(LINES[:2], limiter=True)
    with pytest.raises(ValueError):
        tts.tts('1', limiter=True)
    assert levelled == []


def test_tts_requests_takes_the_limiter_per_call(monkeypatch):
    N, tts, levelled = _fakes(monkeypatch)
    got = {}
    monkeypatch.setattr(tts, 'tts', lambda texts, **kw: got.update(texts=texts, **kw) or ['w'] * len(texts))
    reqs = [dict(text='3', normalize=-16.0), dict(text='0')]
    tts.tts_requests(reqs, limiter=dict(hold_ms=10.0))
    assert got['limiter'] == dict(hold_ms=10.0) and got['normalize'] == [-16.0, None]
    got.clear()
    tts.tts_requests(reqs)
    assert 'limiter' not in got
    with pytest.raises(ValueError):
        tts.tts_requests([dict(text='1', limiter=True)])               # not a request's option


def test_level_waves_and_helpers_refuse_before_the_device():
    from ttsamd.lib import TtsAmdError
    from utils import audio
    x = torch.zeros(2, 100)
    for call in (lambda: audio.limit(x), lambda: audio.normalize_loudness(x, limiter=True)):
        with pytest.raises(TtsAmdError):
            call()
    with pytest.raises(ValueError):
        audio.normalize_loudness(x, limiter=dict(knee=1))


def test_library_refuses_bad_limiter_arguments():
    """ttsamd_wave_limit checks its host arguments before it touches a pointer or launches: the refusals need no GPU"""
    import ctypes as C
    h = lib.load()
    assert h.ttsamd_wave_limit_workspace_bytes(0, 100) == -1 and h.ttsamd_wave_limit_workspace_bytes(1, -1) == -1
    assert h.ttsamd_wave_limit_workspace_bytes(1, 1 << 40) == -1
    assert h.ttsamd_wave_limit_workspace_bytes(2, 1000) >= 2 * 1000 * 4 and h.ttsamd_wave_limit_workspace_bytes(3, 0) > 0
    p = C.c_void_p(256)                                                  # never dereferenced: every call below is refused

    def call(batch=1, stride=100, ceiling=0.99, max_gain=31.6, attack=33, hold=331, ws=1 << 20, wave=p, gain=p):
        return h.ttsamd_wave_limit(wave, stride, p, batch, p, p, ceiling, max_gain, attack, hold, None, gain, p, p, ws, None)

    for kw in (dict(batch=0), dict(batch=65536), dict(stride=-1), dict(ceiling=0.0), dict(ceiling=1.01), dict(ceiling=float('nan')),
               dict(max_gain=0.0), dict(max_gain=float('inf')), dict(attack=-1), dict(attack=34, hold=33), dict(attack=1025, hold=2000),
               dict(attack=10, hold=4097), dict(ws=16), dict(wave=None), dict(gain=None)):
        assert call(**kw) == -1 and h.ttsamd_last_error(), kw
    assert b'attack' in (call(attack=1025, hold=2000), h.ttsamd_last_error())[1]
    assert b'workspace' in (call(ws=16), h.ttsamd_last_error())[1]


def test_the_two_symbols_are_in_the_table():
    for name in ('ttsamd_wave_limit_workspace_bytes', 'ttsamd_wave_limit'):
        assert name in lib.SYMBOLS and getattr(lib.load(), name) is not None
