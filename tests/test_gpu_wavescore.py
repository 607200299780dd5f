"""Wave-against-wave scores on the GPU (pytest -m gpu): ttsamd_stoi / ttsamd_wave_sdr / ttsamd_log_spectral_distance
(csrc/wavescore.hip), ttsamd.engine.WaveScoreEngine and the utils.objective wrappers, against the float64 restatement
tests/wavescore_ref.py (pinned on the CPU by tests/test_wavescore_cpu.py).

Bounds.  frames: exact.  Third-octave magnitudes: 1e-12 * sqrt(total power of the frame) per entry -- nine butterfly levels at 2^-53
and a sum of at most 212 powers leave about 1e-14 of the frame's norm, two orders under the bound.  STOI / ESTOI: 1e-10 absolute; the
tests assert on the restatement that no frame energy lies within 1e-9 dB of the silence threshold and that no centred segment row has
a norm under 1e-6 of its uncentred norm, so that a miss is a kernel error and not conditioning.  (A band edge off by one bin moves the
score by 1.6e-5, the symmetric hanning(256) by 5.5e-5, a missing clip by 5e-2.)  SI-SDR / SNR: 1e-11 relative, the `stats` bound of
tests/test_gpu_objective.py (float64 sums of up to 20 000 terms in another order: 1e-13).  LSD: 1e-9 dB absolute.  Rows of a ragged
batch, two runs, and the wrappers against the manual pipeline: bit for bit.

The signal: wavescore_ref.speech_like, 20 000 samples at 10 kHz, eight vibrato'd harmonics under a max(sin(2 pi 2.3 t), 0)^2 envelope
plus 1e-4 noise; the restatement keeps 80 of its 155 frames (the compaction happens mid-row), the nearest frame energy 6.3 dB from the
threshold.  Degraded copies add white noise at 30 / 10 / 0 / -5 dB."""
import numpy as np
import pytest
import torch

import wavescore_ref as R

pytestmark = pytest.mark.gpu

SNRS = (30.0, 10.0, 0.0, -5.0)
STOI_TOL, TOB_TOL, SDR_RTOL, LSD_TOL = 1e-10, 1e-12, 1e-11, 1e-9


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def x():
    return R.speech_like()


@pytest.fixture(scope='module')
def degraded(x):
    """{snr: (y, {extended: restatement details})}, computed once"""
    out = {}
    for snr in SNRS:
        y = R.add_noise(x, snr)
        out[snr] = (y, {ext: R.stoi_10k(x, y, ext, details=True) for ext in (False, True)})
    return out


def _poisoned(xs, dev, stride=None):
    """rows of different lengths in one buffer whose every entry behind a row's length is NaN -> (wave [B, stride], lens int64 [B])"""
    stride = max(len(v) for v in xs) if stride is None else stride
    buf = np.full((len(xs), stride), np.nan, dtype=np.float32)
    for b, v in enumerate(xs):
        buf[b, :len(v)] = v
    return torch.from_numpy(buf).to(dev), torch.tensor([len(v) for v in xs], dtype=torch.int64, device=dev)


def _stoi(xs, ys, dev, extended, stride=None):
    """-> (score [B], frames [B, 2], tob_x, tob_y [B, 15, F]) as numpy, from NaN-poisoned buffers"""
    from ttsamd.engine import stoi_10k
    wx, lens = _poisoned(xs, dev, stride)
    wy, _ = _poisoned(ys, dev, stride)
    score, frames, tx, ty = stoi_10k(wx, wy, lens, extended=extended, return_bands=True)
    assert score.dtype == torch.float64 and frames.dtype == torch.int32 and tx.dtype == torch.float64 and score.device == wx.device
    return score.cpu().numpy(), frames.cpu().numpy(), tx.cpu().numpy(), ty.cpu().numpy()


def _well_conditioned(d):
    assert d['margin_db'] > 1e-9, d['margin_db']
    assert d['cond'] > 1e-6, d['cond']


@pytest.mark.parametrize('snr', SNRS)
def test_stoi_stages_against_the_restatement(dev, x, degraded, snr):
    y, want = degraded[snr]
    for ext in (False, True):
        d = want[ext]
        _well_conditioned(d)
        score, frames, tx, ty = _stoi([x], [y], dev, ext)
        F, K = d['frames']
        assert (F, K) == (155, 80) and tuple(frames[0]) == (F, K)
        assert tx.shape == ty.shape == (1, 15, F)
        for name, got, ref, power in (('tob_ref', tx, d['tob_x'], d['power_x']), ('tob_deg', ty, d['tob_y'], d['power_y'])):
            err = np.abs(got[0, :, :K] - ref) / np.sqrt(power)[None, :]
            print(f'snr {snr} extended {ext} {name}: max error / sqrt(frame power) {err.max():.3e} (bound {TOB_TOL:.0e})')
            assert err.max() <= TOB_TOL
            assert not got[0, :, K:].any()                              # zero from frame K on
        print(f'snr {snr} extended {ext}: score {score[0]:.15f} restatement {d["score"]:.15f} diff {abs(score[0] - d["score"]):.3e}')
        assert abs(score[0] - d['score']) <= STOI_TOL


@pytest.mark.parametrize('n', [0, 255, 256, 3839, 3840, 3968, 4000])
def test_stoi_lengths_around_the_first_segment(dev, n):
    """29 frames and fewer give 1e-5; 3 968 samples are 30 frames and one segment"""
    rng = np.random.default_rng(11)
    a = (0.1 * rng.standard_normal(4000)).astype(np.float32)
    b = R.add_noise(a, 5.0, seed=12)
    F = (n - 256) // 128 + 1 if n >= 256 else 0
    for ext in (False, True):
        d = R.stoi_10k(a[:n], b[:n], ext, details=True)
        assert d['frames'] == (F, F)                                    # stationary noise: every frame is kept
        if F >= 30:
            _well_conditioned(d)
        score, frames, tx, _ = _stoi([a[:n]], [b[:n]], dev, ext, stride=4000)
        assert tuple(frames[0]) == (F, F) and tx.shape == (1, 15, 30)
        print(f'n {n} extended {ext}: score {score[0]!r} restatement {d["score"]!r}')
        if F < 30:
            assert score[0] == 1e-5 == d['score']
        else:
            assert abs(score[0] - d['score']) <= STOI_TOL
        assert not tx[0, :, F:].any()


def test_stoi_ragged_batch_rows_are_the_rows_alone(dev, x, degraded):
    y = degraded[10.0][0]
    lens = [20000, 3968, 255, 0]
    xs, ys = [x[:n] for n in lens], [y[:n] for n in lens]
    for ext in (False, True):
        score, frames, tx, ty = _stoi(xs, ys, dev, ext, stride=20096)
        again = _stoi(xs, ys, dev, ext, stride=20096)
        for got, rep in zip((score, frames, tx, ty), again):
            assert np.array_equal(got, rep)                             # two runs: the same bits
        assert np.isfinite(score).all() and np.isfinite(tx).all() and np.isfinite(ty).all()
        for b, n in enumerate(lens):
            d = R.stoi_10k(xs[b], ys[b], ext, details=True)
            assert tuple(frames[b]) == d['frames']
            assert abs(score[b] - d['score']) <= STOI_TOL
            for stride in (20096, n):                                   # alone in the batch's stride, and trimmed
                s1, f1, tx1, ty1 = _stoi(xs[b:b + 1], ys[b:b + 1], dev, ext, stride=stride)
                K = int(f1[0, 1])
                assert s1.tobytes() == score[b:b + 1].tobytes() and np.array_equal(f1[0], frames[b])
                assert np.array_equal(tx1[0, :, :K], tx[b, :, :K]) and np.array_equal(ty1[0, :, :K], ty[b, :, :K])
        assert score[2] == 1e-5 and score[3] == 1e-5 and tuple(frames[3]) == (0, 0)


def test_stoi_all_zero_pair_scores_zero_as_the_restatement(dev):
    z = np.zeros(4000, dtype=np.float32)
    for ext in (False, True):
        score, frames, tx, ty = _stoi([z], [z], dev, ext)
        assert R.stoi_10k(z, z, ext) == 0.0 and score[0] == 0.0 and tuple(frames[0]) == (30, 30)
        assert not tx.any() and not ty.any()


def _sdr(rs, es, dev, zero_mean, stride=None):
    from ttsamd.engine import wave_sdr
    wr, lens = _poisoned(rs, dev, stride)
    we, _ = _poisoned(es, dev, stride)
    out = wave_sdr(wr, we, lens, zero_mean=zero_mean)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(rs), 2)
    return out.cpu().numpy()


def _close_ieee(got, want, rtol):
    """equal where the restatement is not finite (inf with its sign, NaN), within rtol elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    return np.array_equal(got[~fin], want[~fin], equal_nan=True) and np.all(np.abs(got[fin] - want[fin]) <= rtol * np.abs(want[fin]))


@pytest.mark.parametrize('zero_mean', [True, False])
def test_sdr_and_snr_against_the_restatement(dev, x, degraded, zero_mean):
    y = degraded[10.0][0]
    lens = [1, 255, 256, 257, 20000]
    rs, es = [x[:n] for n in lens], [y[:n] for n in lens]
    got = _sdr(rs, es, dev, zero_mean)
    assert np.array_equal(got, _sdr(rs, es, dev, zero_mean), equal_nan=True)
    for b, n in enumerate(lens):
        want = R.sdr(rs[b], es[b], zero_mean)
        print(f'n {n} zero_mean {zero_mean}: (si_sdr, snr) {got[b].tolist()} restatement {want}')
        assert _close_ieee(got[b], want, SDR_RTOL), (n, got[b], want)
        for stride in (20000, n):                                       # the row alone, and trimmed: the same bits
            assert _sdr(rs[b:b + 1], es[b:b + 1], dev, zero_mean, stride=stride).tobytes() == got[b:b + 1].tobytes()
    same = _sdr([x], [x], dev, zero_mean)
    assert same[0, 0] == np.inf and same[0, 1] == np.inf               # identical rows
    zero = _sdr([np.zeros(300, dtype=np.float32)], [x[:300]], dev, zero_mean)
    assert np.isnan(zero[0, 0]) and _close_ieee(zero[0], R.sdr(np.zeros(300), x[:300], zero_mean), SDR_RTOL)   # a zero reference
    empty = _sdr([x[:0]], [x[:0]], dev, zero_mean, stride=8)
    assert np.isnan(empty).all()


def _lsd(rs, es, dev, stride=None):
    from ttsamd.engine import log_spectral_distance
    wr, lens = _poisoned(rs, dev, stride)
    we, _ = _poisoned(es, dev, stride)
    out = log_spectral_distance(wr, we, lens)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(rs), 2)
    return out.cpu().numpy()


def test_lsd_against_the_restatement(dev, x, degraded):
    y = degraded[10.0][0]
    lens = [1023, 1024, 20000, 20000]
    rs = [x[:n] for n in lens]
    es = [y[:1023], y[:1024], y, np.zeros(20000, dtype=np.float32)]    # the last: est = 0, every bin of it on the 1e-10 floor
    got = _lsd(rs, es, dev)
    assert np.array_equal(got, _lsd(rs, es, dev), equal_nan=True)
    for b, n in enumerate(lens):
        want, F = R.lsd(rs[b], es[b])
        print(f'n {n}: lsd {got[b, 0]!r} restatement {want!r}, frames {got[b, 1]} / {F}')
        assert got[b, 1] == F == ((n - 1024) // 256 + 1 if n >= 1024 else 0)
        if F == 0:
            assert np.isnan(got[b, 0]) and np.isnan(want)
        else:
            assert abs(got[b, 0] - want) <= LSD_TOL
        for stride in (20000, n):
            assert _lsd(rs[b:b + 1], es[b:b + 1], dev, stride=stride).tobytes() == got[b:b + 1].tobytes()
    assert _lsd([x], [x], dev)[0].tolist() == [0.0, 75.0]


@pytest.fixture(scope='module')
def pair22(dev):
    """one second at 22 050 Hz and a degraded copy, on the device"""
    a = R.speech_like(22050, fs=22050, seed=5)
    return torch.from_numpy(a).to(dev), torch.from_numpy(R.add_noise(a, 10.0, seed=6)).to(dev)


def test_stoi_wrapper_is_stoi_10k_on_the_resampled_rows(dev, pair22):
    from ttsamd.engine import stoi_10k
    from utils.audio import resample
    from utils.objective import stoi
    a, b = pair22
    a10, b10 = (resample(v[None], 22050, 10000, lowpass_filter_width=64) for v in (a, b))
    assert a10.shape == (1, 10000)
    for ext in (False, True):
        want = stoi_10k(a10, b10, extended=ext)[0]
        got = stoi(a, b, fs=22050, extended=ext)
        assert isinstance(got, torch.Tensor) and got.dtype == torch.float64 and got.dim() == 0
        assert torch.equal(got, want[0]) and 0.0 < float(got) < 1.0
        # a batch with lens, padded with NaN behind the rows: row 0 is the same call
        wave_a, lens = _poisoned([a.cpu().numpy(), a.cpu().numpy()[:9000]], dev, stride=22100)
        wave_b, _ = _poisoned([b.cpu().numpy(), b.cpu().numpy()[:9000]], dev, stride=22100)
        both = stoi(wave_a, wave_b, fs=22050, extended=ext, lens=lens)
        assert tuple(both.shape) == (2,) and torch.equal(both[0], got) and bool(torch.isfinite(both).all())
    assert torch.equal(stoi(a10[0], b10[0], fs=10000), stoi_10k(a10, b10)[0][0])     # at 10 kHz nothing is resampled


def test_wave_metrics_keys_shapes_and_numpy_conventions(dev, pair22):
    from utils.objective import WAVE_KEYS, log_spectral_distance, si_sdr, snr, stoi, wave_metrics
    a, b = pair22
    m = wave_metrics(b, a)
    assert tuple(m) == WAVE_KEYS == ('stoi', 'estoi', 'si_sdr', 'snr', 'lsd', 'frames', 'frames_kept')
    assert all(isinstance(v, torch.Tensor) and v.dim() == 0 and v.device.type == 'cuda' for v in m.values())
    assert all(m[k].dtype == torch.float64 for k in WAVE_KEYS[:5]) and m['frames'].dtype == torch.int32
    assert torch.equal(m['stoi'], stoi(a, b)) and torch.equal(m['estoi'], stoi(a, b, extended=True))
    assert torch.equal(m['si_sdr'], si_sdr(b, a)) and torch.equal(m['snr'], snr(b, a)) and torch.equal(m['lsd'], log_spectral_distance(b, a))
    assert int(m['frames']) == (10000 - 256) // 128 + 1 and 30 <= int(m['frames_kept']) <= int(m['frames'])
    assert abs(float(m['snr']) - 10.0) < 0.05 and float(m['lsd']) > 0.0
    an, bn = a.cpu().numpy(), b.cpu().numpy()
    mn = wave_metrics(bn, an)                                           # numpy in: floats out
    assert all(isinstance(mn[k], float) for k in WAVE_KEYS[:5]) and isinstance(mn['frames'], int)
    assert all(mn[k] == m[k].item() for k in WAVE_KEYS)
    mb = wave_metrics(np.stack([bn, bn]), np.stack([an, an[::-1].copy()]), lens=[22050, 12000])   # batched numpy in: arrays [B] out
    assert all(isinstance(mb[k], np.ndarray) and mb[k].shape == (2,) for k in WAVE_KEYS)
    assert all(mb[k][0] == mn[k] for k in WAVE_KEYS)
    wide = wave_metrics(torch.nn.functional.pad(b, (0, 50)), a)        # different padded widths: compared over the min of the two
    assert all(torch.equal(wide[k], m[k]) for k in WAVE_KEYS)


def test_copy_synthesis_is_the_manual_pipeline_and_bf16_is_measured(dev, pair22):
    from ttsamd import engine as E
    from ttsamd import synth
    from ttsamd.config import HIFIGAN_CONFIG
    from utils.objective import WAVE_KEYS, copy_synthesis, si_sdr
    from vocoder.hifigan.models import Generator
    a, _ = pair22
    hsd = synth.hifigan_state_dict()
    gen = Generator(dict(HIFIGAN_CONFIG), state_dict={k: torch.from_numpy(np.array(v)) for k, v in hsd.items()}).to(dev)
    score, out = copy_synthesis(gen, a)
    frames = 22050 // 256
    assert tuple(out.shape) == (256 * frames,) and tuple(score) == WAVE_KEYS
    print('copy synthesis (synthetic V1 weights, fp32):', {k: float(v) for k, v in score.items()})
    assert all(bool(torch.isfinite(score[k])) for k in WAVE_KEYS[:5])
    mel, fr = E.ObjectiveEngine(device=dev).melspec.forward(a[None], None)
    manual = gen.engine().forward(mel, fr)
    assert int(fr[0]) == frames and torch.equal(manual[0], out)
    want = E.wave_scorer(22050, dev).metrics(a[None, :256 * frames].contiguous(), manual, 256 * fr)
    assert all(torch.equal(want[k][0], score[k]) for k in WAVE_KEYS)
    assert float(si_sdr(out, out)) == float('inf')                      # fp32 against itself
    E.set_precision('bf16')
    try:
        score16, out16 = copy_synthesis(gen, a)
    finally:
        E.set_precision('f32')
    s16 = float(si_sdr(out16, out))
    print(f'plain bf16 resynthesis against the fp32 one: SI-SDR {s16:.2f} dB (a measurement; synthetic weights)')
    assert np.isfinite(s16) and s16 < float('inf')
    assert all(bool(torch.isfinite(score16[k])) for k in WAVE_KEYS[:5])
