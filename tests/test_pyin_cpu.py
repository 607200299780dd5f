"""CPU: the pYIN restatement (tests/pyin_ref.py) on signals whose f0 is known, its closed forms against scipy.stats, the tables the
library builds on the host (ttsamd_pyin_tables) against the restatement's, the fp32 kernel-form Viterbi against the dense float64 one,
and the host-side helpers of utils/pitch.py and the data_function drop-in against direct numpy."""
import math

import numpy as np
import pytest
import torch

import pyin_ref as R

C2, C7 = 65.40639132514966, 2093.004522404789
REF = dict(frame_length=1024, hop_length=256)
N60 = 60 * 256 - 1


@pytest.fixture(scope='module')
def p():
    return R.Params(C2, C7, **REF)


def test_geometry_of_the_reference_call(p):
    assert (p.pmin, p.pmax, p.P, p.nb, p.w, p.W) == (10, 338, 601, 10, 51, 512)
    from utils.pitch import note_to_hz
    assert note_to_hz('C2') == C2 and note_to_hz('C7') == C7 and note_to_hz('A4') == 440.0
    assert abs(note_to_hz('C#4') - 277.1826309768721) < 1e-9 and abs(note_to_hz('Bb3') - 233.08188075904496) < 1e-9


@pytest.mark.parametrize('f,noise', [(70.0, 0), (110.0, 0), (220.0, 0), (437.3, 0), (880.0, 0), (1500.0, 0), (180.0, 0.03)])
def test_steady_tones_within_one_bin(p, f, noise):
    f0, flag, vp, _ = R.pyin(R.harmonic_tone(f, N60, noise=noise, seed=5), p)
    assert len(f0) == 60 and flag[3:-3].all()
    c = R.cents(f0[3:-3], f)
    print(f'{f} Hz: max {c.max():.2f} cents')
    assert c.max() <= 10.0


def test_noise_and_silence_are_unvoiced(p):
    rng = np.random.default_rng(3)
    for y in (rng.normal(0, 0.1, 40 * 256).astype(np.float32), np.zeros(40 * 256, np.float32)):
        f0, flag, vp, _ = R.pyin(y, p)
        assert not flag.any() and np.isnan(f0).all()
    assert not vp.any()                                          # silence: d' is 0 everywhere, no trough at all


def test_flag_follows_a_silent_gap(p):
    y = R.harmonic_tone(200.0, 90 * 256 - 1)
    y[30 * 256: 60 * 256] = 0
    _, flag, _, _ = R.pyin(y, p)
    on = np.flatnonzero(np.diff(flag.astype(int)))
    assert flag[5:28].all() and not flag[33:58].any() and flag[63:85].all()
    assert len(on) == 2 + int(not flag[0]) + int(not flag[-1]) and np.abs(on[-2 - int(not flag[-1])] + 1 - 30).max() <= 2 \
        and abs(on[-1 - int(not flag[-1])] + 1 - 60) <= 2


def test_closed_forms_against_scipy(p):
    stats = pytest.importorskip('scipy.stats')
    th = np.linspace(0, 1, p.K + 1)
    assert np.abs(R.beta_weights(p) - np.diff(stats.beta.cdf(th, 2, 18))).max() < 1e-14
    x = np.linspace(0, 1, 41)
    assert np.abs(np.array([R.beta_cdf(2, 18, v) for v in x]) - (1 - (1 - x) ** 19 - 19 * x * (1 - x) ** 18)).max() < 1e-14
    assert np.abs(np.array([R.beta_cdf(3, 5, v) for v in x]) - stats.beta.cdf(x, 3, 5)).max() < 1e-14
    for n in (1, 2, 7, 40):
        assert np.abs(R.boltzmann_prior(2.0, np.arange(n), n) - stats.boltzmann.pmf(np.arange(n), 2.0, n)).max() < 1e-15


@pytest.mark.parametrize('kw', [dict(fmin=C2, fmax=C7, **REF), dict(fmin=100.0, fmax=400.0, **REF), dict(fmin=C2, fmax=C7, frame_length=2048),
                                dict(fmin=C2, fmax=C7, resolution=0.5, **REF), dict(fmin=C2, fmax=C7, max_transition_rate=1.0, **REF),
                                dict(fmin=300.0, fmax=400.0, beta_parameters=(3, 5), boltzmann_parameter=1.5, n_thresholds=37,
                                     switch_prob=0.05, **REF)],
                         ids=['default', 'P241', 'frame2048', 'res0.5', 'w1', 'P50_under_w'])
def test_library_tables_equal_the_restatement(kw):
    """ttsamd_pyin_tables: what csrc/pyin.hip uploads at create, built on the host in float64."""
    from ttsamd.engine import pyin_tables
    q, t = R.Params(**kw), pyin_tables(**kw)
    assert (t['pmin'], t['pmax'], t['n_bins'], t['bins_per_semitone'], t['width']) == (q.pmin, q.pmax, q.P, q.nb, q.w)
    E = t['max_obs']
    assert E == (q.pmax - q.pmin + 2) // 2 and t['n_kinds'] == min(q.P, q.w)
    assert np.abs(t['beta'] - R.beta_weights(q)).max() <= 1e-15
    for n in (1, 2, 3, E // 2, E):
        assert np.abs(t['expn'][:n] * t['norm'][n] - R.boltzmann_prior(q.lam, np.arange(n), n)).max() <= 1e-15
    A, P, w, h = R.transition(q), q.P, q.w, q.w // 2
    kind = lambda k: k if P <= w else (k if k < h else (k - (P - w) if k >= P - h else h))   # noqa: E731
    D = np.zeros_like(A)
    for a in range(2):
        for b in range(2):
            for k in range(P):
                j = np.arange(max(0, k - h), min(P - 1, k + h) + 1)
                D[a * P + k, b * P + j] = t['trans'][kind(k), j - k + h, int(a != b)]
    assert np.abs(D - A).max() <= 1e-15                           # every in-band entry, and nothing outside the band
    assert np.abs(A.sum(1) - 1).max() < 1e-12
    assert np.array_equal(t['logtrans'], np.log(t['trans'] + R.TINY).astype(np.float32))
    assert np.allclose(t['f0'], q.fmin * 2.0 ** (np.arange(P) / (12.0 * q.nb)), rtol=1e-7, atol=0)


def test_limits_are_refused_on_the_host():
    from ttsamd.engine import pyin_tables
    from ttsamd.lib import TtsAmdError
    for bad in (dict(frame_length=4096), dict(frame_length=1023), dict(frame_length=1024, win_length=1024), dict(resolution=0.01, **REF),
                dict(n_thresholds=129, **REF), dict(beta_parameters=(2.5, 18), **REF), dict(beta_parameters=(0, 18), **REF)):
        with pytest.raises(TtsAmdError):
            pyin_tables(C2, C7, **bad)


FIXTURES = [(11, 40, 0.0), (12, 80, 1e-3), (13, 120, 1e-2)]


def _reported(states, P):
    """what a call reports of a state: the flag on every frame, the bin on the voiced ones.  The bin an UNVOICED state carries is no
    output (f0 is the fill value there), and it is not determined: paths that cross an unvoiced stretch with the same steps in another
    order have the same cost in exact arithmetic, so rounding picks among them (seen here: fixture 13, frames 69-79, float64 walks
    904, 903, 902, ... where fp32, dense or kernel-form, walks 903, 901, 899, ...; both rejoin at 889)."""
    return np.where(states < P, states, -1)


def test_kernel_form_fp32_viterbi_equals_dense_float64(p):
    lt, S, tables = np.log(R.transition(p) + R.TINY), 2 * p.P, R.band_tables(p)
    total = 0
    for seed, frames, noise in FIXTURES:
        obs, _ = R.observations(R.speech_like(seed, frames, noise=noise), p)
        lo = np.log(obs + R.TINY)
        want = R.viterbi_dense(lo, lt, np.log(np.full(S, 1.0 / S) + R.TINY), np.float64)
        got = R.viterbi_kernel_form(lo.astype(np.float32), p, tables)
        assert np.array_equal(_reported(got, p.P), _reported(want, p.P)), np.flatnonzero(_reported(got, p.P) != _reported(want, p.P))
        assert np.array_equal(got, R.viterbi_dense(lo, lt, np.log(np.full(S, 1.0 / S) + R.TINY), np.float32))   # fp32 dense: state for state
        total += frames
    # ties: an all-silent signal, where the lowest index decides every step, in both forms and in dense fp32
    obs, _ = R.observations(np.zeros(20 * 256, np.float32), p)
    lo = np.log(obs + R.TINY)
    a = R.viterbi_dense(lo, lt, np.log(np.full(S, 1.0 / S) + R.TINY), np.float32)
    assert np.array_equal(R.viterbi_kernel_form(lo.astype(np.float32), p, tables), a)
    print(f'{total} frames: no difference')


def test_pitch_helpers_against_direct_numpy():
    from models.fastpitch.fastpitch.data_function import fit_to_mel_len, normalize_pitch
    from utils.pitch import pitch_mean_std
    rng = np.random.default_rng(0)
    tracks = [np.where(rng.random(n) < 0.3, 0.0, rng.uniform(80, 400, n)) for n in (50, 7, 120)]
    tracks[1][2] = np.nan
    tracks.append(np.zeros(5))
    mean, std = pitch_mean_std(tracks + [torch.from_numpy(tracks[0])])
    rmean = rvar = 0.0
    ndata = 0
    for tr in tracks[:3] + [tracks[0]]:                           # the update of the script, written out with Python floats
        v = [float(x) for x in tr if x == x and x > 1]
        n = len(v)
        m = math.fsum(v) / n
        var = math.fsum((x - m) ** 2 for x in v) / n
        rvar = ((ndata - 1) * rvar + (n - 1) * var) / (ndata + n - 1) + ndata * n * (m - rmean) ** 2 / ((ndata + n) * (ndata + n - 1))
        rmean = (n * m + ndata * rmean) / (n + ndata)
        ndata += n
    assert abs(mean - rmean) < 1e-10 and abs(std - math.sqrt(rvar)) < 1e-10
    one = np.array([0.0, 100.0, 300.0, 0.5])
    assert pitch_mean_std([one]) == (200.0, 100.0)                # one track: its mean and population std
    x = torch.tensor([[0.0, 100.0, 250.0, 0.0, 300.0]])
    got = normalize_pitch(x.clone(), torch.tensor([200.0]), torch.tensor([50.0]))
    assert torch.equal(got, torch.tensor([[0.0, -2.0, 1.0, 0.0, 2.0]]))
    assert torch.equal(fit_to_mel_len(x, 3), x[:, :3]) and torch.equal(fit_to_mel_len(x, 7), torch.cat([x, torch.zeros(1, 2)], 1))
    assert fit_to_mel_len(x, 5) is not None and fit_to_mel_len(x, 5).shape == (1, 5)


def test_wav_reader_round_trip(tmp_path):
    from utils.audio import load_wav, save_wav
    y = (np.sin(np.arange(3000) / 17.0) * 0.7).astype(np.float32)
    save_wav(str(tmp_path / 'a.wav'), y)
    a, sr = load_wav(str(tmp_path / 'a.wav'))
    assert sr == 22050 and a.dtype == np.float32 and np.array_equal(a, (np.round(y * 32767.0) / 32768.0).astype(np.float32))
    save_wav(str(tmp_path / 'f.wav'), y, sample_rate=16000, encoding='PCM_F')
    a, sr = load_wav(str(tmp_path / 'f.wav'))
    assert sr == 16000 and np.array_equal(a, y)
    (tmp_path / 'bad.wav').write_bytes(b'nope')
    with pytest.raises(ValueError):
        load_wav(str(tmp_path / 'bad.wav'))
