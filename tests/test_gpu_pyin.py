"""GPU: pYIN (csrc/pyin.hip) through the C ABI and the drop-ins, against tests/pyin_ref.py.

Stage 1 (the frame kernel): voiced_prob within 1e-12 of the float64 restatement on every frame -- the probabilities are sums of table
values, so a larger difference means a comparison went the other way; the sparse observations name the same bins.
Viterbi: the states equal, element for element, the restatement of the kernel's own fp32 recurrence run on the kernel's own observations.
Outcome: (f0, voiced_flag) of the whole call against the DENSE float64 restatement: the flag on every frame, the bin on every voiced
one (the bin an unvoiced state carries is no output; tests/test_pyin_cpu.py says why rounding decides it).  f0 is compared through
rtol 1e-6 (fp32 rounding of fmin 2^(bin / 120); a bin is 5.8e-3 away), never a wider bound."""
import functools

import numpy as np
import pytest
import torch

import pyin_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C2, C7 = 65.40639132514966, 2093.004522404789
REF = dict(frame_length=1024, hop_length=256)                  # the reference's two calls
FIXTURES = [(11, 40, 0.0), (12, 80, 1e-3), (13, 120, 1e-2), (14, 160, 0.0)]   # (seed, frames, noise)


@functools.lru_cache(maxsize=None)
def _engine(fmin=C2, fmax=C7, **kw):
    from ttsamd.engine import PyinEngine
    return PyinEngine(fmin, fmax, **kw)


def _batch(rows):
    n = max(max(len(r) for r in rows), 1)
    x = np.zeros((len(rows), n), np.float32)
    for b, r in enumerate(rows):
        x[b, :len(r)] = r
    return torch.from_numpy(x).to(DEV), torch.tensor([len(r) for r in rows], dtype=torch.int64)


def _run(eng, rows):
    x, lens = _batch(rows)
    f0, flag, prob, frames, states, obs = eng.forward(x, lens, return_states=True, return_obs=True)
    torch.cuda.synchronize()
    return (f0.cpu().numpy(), flag.cpu().numpy(), prob.cpu().numpy(), frames.cpu().numpy(), states.cpu().numpy(),
            {k: v.cpu().numpy() for k, v in obs.items()})


def _dense_logobs(obs, b, T, P):
    """the kernel's own observations of row b as the fp32 [T][2P] array its recurrence sees"""
    lo = np.full((T, 2 * P), np.float32(np.log(R.TINY)), dtype=np.float32)
    for t in range(T):
        c = int(obs['count'][b, t])
        lo[t, obs['bin'][b, t, :c]] = obs['logprob'][b, t, :c]
        lo[t, P:] = obs['unvoiced'][b, t]
    return lo


@pytest.fixture(scope='module')
def fixtures():
    """speech-like rows, their float64 restatement (observations, voiced_prob, dense float64 states) and the device's answer, once"""
    p = R.Params(C2, C7, **REF)
    rows = [R.speech_like(seed, frames, noise=noise) for seed, frames, noise in FIXTURES]
    ref = []
    lt, S = np.log(R.transition(p) + R.TINY), 2 * p.P
    for y in rows:
        obs, vp = R.observations(y, p)
        st = R.viterbi_dense(np.log(obs + R.TINY), lt, np.log(np.full(S, 1.0 / S) + R.TINY), np.float64)
        ref.append((obs, vp, st))
    return p, rows, ref, _run(_engine(**REF), rows)


def test_stage1_voiced_prob_and_observations(fixtures):
    p, rows, ref, (f0, flag, prob, frames, states, obs) = fixtures
    beta = R.beta_weights(p)
    for b, (y, (robs, rvp, _)) in enumerate(zip(rows, ref)):
        T = len(rvp)
        assert frames[b] == T == 1 + len(y) // 256
        err = np.abs(prob[b, :T] - rvp)
        print(f'row {b}: {T} frames, max |voiced_prob - float64| = {err.max():.3e}')
        for t in np.flatnonzero(err > 1e-12):
            _, _, dbg = R.frame_observation(R.frames_of(y, p)[t], p, beta)
            k = np.floor(dbg['heights'] * p.K)
            print(f'  frame {t}: device {prob[b, t]:.17g} float64 {rvp[t]:.17g}; trough heights {dbg["heights"]} next thresholds {(k + 1) / p.K}')
        assert err.max() <= 1e-12
        assert not prob[b, T:].any()
        for t in range(T):
            c = int(obs['count'][b, t])
            want = np.flatnonzero(robs[t, :p.P])[::-1]
            assert np.array_equal(obs['bin'][b, t, :c], want), (b, t)
            wl = np.log(robs[t, want] + R.TINY)
            assert np.all(np.abs(obs['logprob'][b, t, :c] - wl) <= 2.4e-7 * np.abs(wl) + 1e-30), (b, t)       # one fp32 rounding of a float64 log
            # (1 - voiced_prob) / P: where voiced_prob is one rounding from 1 the LOG is ill-conditioned, so compare the probability:
            # the 1e-12 allowed on voiced_prob, over P, plus the fp32 rounding of the stored log (relative 1.2e-7 |log|)
            wu = robs[t, p.P]
            assert abs(np.exp(np.float64(obs['unvoiced'][b, t])) - wu) <= 1e-12 / p.P + 2.4e-7 * abs(np.log(wu + R.TINY)) * wu, (b, t)


def test_outcome_equals_the_dense_float64_restatement(fixtures):
    p, rows, ref, (f0, flag, prob, frames, states, obs) = fixtures
    total = bad = 0
    for b, (_, _, st64) in enumerate(ref):
        T = len(st64)
        rf0, rflag = R.decode(st64, p, fill_na=0.0)
        assert np.array_equal(states[b, :T] < p.P, flag[b, :T])
        want = np.where(flag[b, :T], p.fmin * 2.0 ** ((states[b, :T] % p.P) / (12.0 * p.nb)), 0.0)
        assert np.allclose(f0[b, :T], want, rtol=1e-6, atol=0)              # f0 is the bin's frequency
        diff = np.flatnonzero((states[b, :T] != st64) & (flag[b, :T] | rflag))   # (the bin of an unvoiced state is no output)
        for t in diff:
            print(f'row {b} frame {t}: device state {states[b, t]} (f0 {f0[b, t]:.3f}) vs float64 state {st64[t]} (f0 {rf0[t]:.3f})')
        assert np.array_equal(flag[b, :T], rflag), 'a voiced flag differs'
        assert np.all(np.abs(states[b, :T] % p.P - st64 % p.P)[flag[b, :T]] <= 1), 'more than one bin apart'
        total += T
        bad += int(np.count_nonzero((states[b, :T] != st64) & flag[b, :T]))
    print(f'{bad} of {total} frames differ from the dense float64 Viterbi')
    assert bad <= 0.01 * total


# (name, Params keywords): the default geometry, P = 241, frame_length 2048 (hop 512: w = 101, two-octave window), resolution 0.5
# (P = 121, w = 11), and a transition rate that leaves w = 1 (no local move at all)
PARAM_SETS = [('default', dict(fmin=C2, fmax=C7, **REF)),
              ('P241', dict(fmin=100.0, fmax=400.0, **REF)),
              ('frame2048', dict(fmin=C2, fmax=C7, frame_length=2048)),
              ('res0.5', dict(fmin=C2, fmax=C7, resolution=0.5, **REF)),
              ('w1', dict(fmin=C2, fmax=C7, max_transition_rate=1.0, **REF))]


@pytest.mark.parametrize('name,kw', PARAM_SETS, ids=[n for n, _ in PARAM_SETS])
def test_viterbi_states_equal_the_kernel_form_restatement(name, kw):
    p = R.Params(**kw)
    assert p.w == {'default': 51, 'P241': 51, 'frame2048': 101, 'res0.5': 11, 'w1': 1}[name]
    hop = p.hop
    rows = [R.speech_like(21, 60, hop=hop, noise=1e-3),                   # voiced, silent and noisy segments
            R.harmonic_tone(150.0, 40 * hop - 1),                         # all voiced
            np.zeros(40 * hop - 1, np.float32),                           # all silent: every step a tie, the lowest index decides
            R.harmonic_tone(200.0, hop - 1),                              # n < hop: one frame
            R.harmonic_tone(200.0, 2 * hop - 1),                          # two frames
            R.harmonic_tone(300.0, p.N - 100)]                            # shorter than a frame
    if name == 'default':
        rows.append(R.speech_like(22, 257, noise=1e-2))                   # 257 frames: past 16 x 16 pointer rows of the backtrack
    eng = _engine(**kw)
    f0, flag, prob, frames, states, obs = _run(eng, rows)
    tables = R.band_tables(p)
    for b, y in enumerate(rows):
        T = 1 + len(y) // hop
        assert frames[b] == T
        want = R.viterbi_kernel_form(_dense_logobs(obs, b, T, p.P), p, tables)
        diff = np.flatnonzero(states[b, :T] != want)
        assert diff.size == 0, (name, b, diff[:8], states[b, diff[:8]], want[diff[:8]])
        assert np.all(states[b, T:] == -1) and not f0[b, T:].any() and not flag[b, T:].any()
    assert not flag[2].any()                                             # silence stays unvoiced
    if name != 'w1':                                                      # (w = 1 cannot move between bins: it may sit out a wrong start unvoiced)
        assert flag[1, 3:37].all()


def test_analytic_tones_within_ten_cents():
    tones = [70.0, 110.0, 220.0, 437.3, 880.0, 1500.0]
    rows = [R.harmonic_tone(f, 60 * 256 - 1) for f in tones] + [R.harmonic_tone(180.0, 60 * 256 - 1, noise=0.03, seed=5)]
    rng = np.random.default_rng(3)
    rows += [rng.normal(0, 0.1, 60 * 256 - 1).astype(np.float32), np.zeros(60 * 256 - 1, np.float32)]
    f0, flag, prob, frames, states, _ = _run(_engine(**REF), rows)
    for b, f in enumerate(tones + [180.0]):
        assert flag[b, 3:-3].all(), f
        c = R.cents(f0[b, 3:-3], f)
        print(f'{f} Hz: max {c.max():.2f} cents')
        assert c.max() <= 10.0, (f, c.max())
    assert not flag[7].any() and not flag[8].any()                        # white noise, digital silence


def test_ragged_batch_rows_equal_their_alone_runs_and_limits():
    from ttsamd.engine import PyinEngine, PYIN_MAX_FRAMES
    from ttsamd.lib import TtsAmdError
    from utils.pitch import pyin
    eng = _engine(**REF)
    rows = [R.speech_like(31, 40, noise=1e-3), R.speech_like(32, 30)[:5000], R.harmonic_tone(220.0, 255), np.zeros(0, np.float32)]
    f0, flag, prob, frames, states, _ = _run(eng, rows)
    assert frames.tolist() == [1 + len(r) // 256 for r in rows] == [40, 20, 1, 1]
    for b, r in enumerate(rows):
        a0, afl, apr, afr, ast, _ = _run(eng, [r])
        T = int(afr[0])
        assert np.array_equal(f0[b, :T].view(np.uint32), a0[0, :T].view(np.uint32)) and np.array_equal(flag[b, :T], afl[0, :T])
        assert np.array_equal(prob[b, :T].view(np.uint64), apr[0, :T].view(np.uint64)) and np.array_equal(states[b, :T], ast[0, :T])
        assert not f0[b, T:].any() and not flag[b, T:].any() and not prob[b, T:].any()
    # limits: each refused by name, and the workspace query says -1
    for bad in (dict(frame_length=4096), dict(frame_length=1023), dict(frame_length=1024, win_length=1024), dict(resolution=0.01, **REF),
                dict(n_thresholds=200, **REF), dict(beta_parameters=(2.5, 18), **REF), dict(pad_mode='edge', **REF)):
        with pytest.raises(TtsAmdError):
            PyinEngine(C2, C7, **bad)
    lib = eng.lib
    assert lib.ttsamd_pyin_workspace_bytes(eng.handle, 1, PYIN_MAX_FRAMES + 1) == -1
    assert lib.ttsamd_pyin_workspace_bytes(None, 1, 10) == -1 and lib.ttsamd_pyin_workspace_bytes(eng.handle, 0, 10) == -1
    assert eng.workspace_bytes(1, PYIN_MAX_FRAMES) > 0
    with pytest.raises(TtsAmdError):
        eng.forward(torch.zeros(1, 256 * PYIN_MAX_FRAMES, device=DEV))
    with pytest.raises(TtsAmdError):
        pyin(np.zeros(1000, np.float32), fmin=C2, fmax=C7, center=False)
    with pytest.raises(TtsAmdError):
        pyin(np.zeros(1000, np.float32), fmin=C2, fmax=C7, fill_na=None)


def test_reflect_padding_matches_the_restatement():
    p = R.Params(C2, C7, pad_mode='reflect', **REF)
    y = R.harmonic_tone(140.0, 20 * 256 - 7)
    f0, flag, prob, frames, states, _ = _run(_engine(pad_mode='reflect', **REF), [y, y[:300]])
    for b, r in enumerate((y, y[:300])):
        _, rvp = R.observations(r, p)
        assert np.abs(prob[b, :len(rvp)] - rvp).max() <= 1e-12


def test_dropins_numpy_wav_file_and_fastpitch(tmp_path, golden):
    import text
    from models.fastpitch.fastpitch.data_function import estimate_pitch, normalize_pitch
    from models.fastpitch.networks import FastPitch
    from ttsamd import synth
    from ttsamd.config import NET_CONFIG
    from utils.audio import save_wav
    from utils.pitch import note_to_hz, pyin
    y = np.concatenate([R.harmonic_tone(200.0, 30 * 256), np.zeros(20 * 256 - 1, np.float32)])
    f0, flag, prob = pyin(y, fmin=note_to_hz('C2'), fmax=note_to_hz('C7'), **REF)
    assert isinstance(f0, np.ndarray) and f0.shape == flag.shape == prob.shape == (50,) and flag.dtype == bool
    assert np.array_equal(np.isnan(f0), ~flag) and flag[3:27].all() and not flag[34:].any()
    assert R.cents(f0[3:27], 200.0).max() <= 10.0
    t0, tfl, _ = pyin(torch.from_numpy(y).to(DEV)[None], fmin=C2, fmax=C7, **REF)
    assert t0.is_cuda and t0.shape == (1, 50) and np.array_equal(tfl[0].cpu().numpy(), flag)
    # a wav file: 16-bit PCM quantises the samples, so the file's own samples are the input of the comparison
    path = str(tmp_path / 'tone.wav')
    save_wav(path, y)
    q = (np.clip(np.round(y * 32767.0), -32768, 32767) / 32768.0).astype(np.float32)
    qf0, _, _ = pyin(q, fmin=C2, fmax=C7, **REF)
    for mel_len in (49, 50, 51):
        got = estimate_pitch(path, mel_len)
        want = np.zeros(mel_len, np.float32)
        want[:min(mel_len, 50)] = np.nan_to_num(qf0)[:min(mel_len, 50)]
        assert got.shape == (1, mel_len) and got.dtype == torch.float32 and np.array_equal(got[0].numpy(), want)
    norm = estimate_pitch(path, 50, normalize_mean=200.0, normalize_std=50.0)[0].numpy()
    assert np.allclose(norm[flag], (np.nan_to_num(qf0)[flag] - 200.0) / 50.0, rtol=1e-6) and not norm[~flag].any()
    save_wav(str(tmp_path / 'r16k.wav'), y, sample_rate=16000)
    from ttsamd.lib import TtsAmdError
    with pytest.raises(TtsAmdError):
        estimate_pitch(str(tmp_path / 'r16k.wav'), 50)
    with pytest.raises(NotImplementedError):
        estimate_pitch(path, 50, n_formants=2)
    with pytest.raises(ValueError):
        estimate_pitch(path, 50, method='yin')
    # FastPitch.pitch_track -> align(pitch=) -> infer(dur_tgt, pitch_tgt)
    g = golden('aligner')
    sd = synth.fastpitch_state_dict()
    sd.update(synth.fastpitch_aligner_state_dict(gain=float(g['gain'])))
    torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in sd.items()}, 'config': dict(NET_CONFIG), 'symbols': list(text.symbols)},
               tmp_path / 'fp.pth')
    m = FastPitch(str(tmp_path / 'fp.pth')).to(DEV)
    B, T = g['mel'].shape[0], g['mel'].shape[2]
    lens = [int(v) * 256 - 1 for v in g['mel_lens']]
    wave = np.zeros((B, max(lens)), np.float32)
    for b, n in enumerate(lens):                                          # the first half of each recording is voiced, the rest silent
        wave[b, :n // 2] = R.harmonic_tone(120.0 + 40 * b, n // 2)
    track = m.pitch_track(wave, torch.tensor(lens), mel_len=T)
    assert track.shape == (B, 1, T) and track.is_cuda
    hz = m.pitch_track(wave, torch.tensor(lens), mel_len=T, normalize=False)
    voiced = (hz != 0)
    assert torch.equal(voiced, track != 0) and torch.allclose(track[voiced], (hz[voiced] - 218.14) / 67.24, rtol=1e-5)
    res = m.align(g['ids'], g['mel'], g['mel_lens'], pitch=track)
    dur = res.dur_tgt.cpu().numpy().astype(int)
    vf = voiced[:, 0].cpu().numpy()
    pt = res.pitch_tgt.cpu().numpy()
    seen = 0
    for b in range(B):
        e = np.concatenate([[0], np.cumsum(dur[b])])
        for l in range(dur.shape[1]):
            if dur[b, l] and not vf[b, e[l]:e[l + 1]].any():
                assert pt[b, 0, l] == 0.0
                seen += 1
    assert seen > 0
    mel, dec_lens, *_ = m.infer(g['ids'], dur_tgt=res.dur_tgt, pitch_tgt=res.pitch_tgt)
    assert np.array_equal(dec_lens.cpu().numpy(), g['mel_lens'])
