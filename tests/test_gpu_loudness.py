"""Output levelling on the GPU (pytest -m gpu): ttsamd_loudness_measure / ttsamd_wave_level (csrc/loudness.hip), LoudnessEngine, the
utils.audio helpers and `normalize=` of the tts wrappers, against the float64 restatement tests/loudness_ref.py.

Tolerances.  L: 1e-9 LU -- the float64 floor of the block energies is 3e-13 relative (1.3e-12 LU), so three orders are left for the
GPU's summation order; every input is checked (on the restatement) to keep all its blocks at least 1e-6 LU from both gates, so that no
gate can flip inside the tolerance.  Peak: exact.  gain_out: 1e-6 relative (fp32 rounding of g is 6e-8; a libm difference in 10^x a few
ulp of float64).  Levelled samples: numpy's float32 arithmetic on the kernel's own gain / peak, bit for bit.  Rows of a ragged batch:
the bits of the row alone.

Sizes at 22 050 Hz (step 2 205, block 8 820, segments of 63 samples, 128 segments = 8 064 samples per work-group of the filter passes,
64 segments = 4 032 samples per step of the scan): around one segment, one step, one block, one scan step and one work-group, and
8 820 + 4 * 2 205 +- 1 = 17 640 +- 1, which lies behind the second work-group boundary (16 128)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import loudness_ref as R
from conftest import GOLDEN, WAVE_TOL

pytestmark = pytest.mark.gpu

EINVAL = -1
SIZES = [1, 62, 63, 64, 2204, 2205, 4032, 4033, 8063, 8064, 8065, 8819, 8820, 8821, 11024, 11025, 17639, 17641, 3 * 22050 + 777]
L_TOL = 1e-9


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch.device('cuda:0')


def _signal(n, seed, fs=22050):
    """noise at sigma 0.1 under a slow envelope (0.1 .. 1), so that the blocks differ and the relative gate has work to do"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / fs
    return (rng.standard_normal(n) * 0.1 * (0.55 + 0.45 * np.sin(2 * np.pi * 0.9 * t + seed))).astype(np.float32)


@pytest.fixture(scope='module')
def rows():
    """{n: (samples, restatement)} at 22 050 Hz, computed once; every block at least 1e-6 LU from both gates"""
    out = {}
    for n in SIZES:
        x = _signal(n, n)
        m = R.measure(x, 22050)
        assert R.gate_margin(m) > 1e-6, (n, R.gate_margin(m))
        out[n] = (x, m)
    return out


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _poisoned(xs, dev, stride=None):
    """rows of different lengths in one buffer whose every entry behind a row's length is NaN -> (wave [B, stride], lens int64 [B])"""
    stride = stride or max(1, max(len(x) for x in xs))
    buf = np.full((len(xs), stride), np.nan, dtype=np.float32)
    for b, x in enumerate(xs):
        buf[b, :len(x)] = x
    return torch.from_numpy(buf).to(dev), torch.tensor([len(x) for x in xs], dtype=torch.int64, device=dev)


def _measure(xs, dev, fs=22050, stride=None):
    from ttsamd.engine import leveller
    wave, lens = _poisoned(xs, dev, stride)
    loud, peak = leveller(fs, dev).measure(wave, lens)
    assert loud.dtype == torch.float64 and peak.dtype == torch.float32 and loud.device == wave.device
    return loud.cpu().numpy(), peak.cpu().numpy()


def test_rows_alone_against_the_restatement(dev, rows):
    worst = 0.0
    for n, (x, m) in rows.items():
        loud, peak = _measure([x], dev)
        d = abs(loud[0] - m['L'])
        worst = max(worst, d)
        print(f'n = {n}: L {loud[0]:.9f} LUFS, restatement {m["L"]:.9f}, difference {d:.2e} LU, {len(m["z"])} blocks')
        assert d < L_TOL, n
        assert peak[0] == m['peak'], n
    print(f'largest difference over {len(rows)} rows: {worst:.2e} LU (tol {L_TOL})')


@pytest.mark.parametrize('fs', [8000, 24000, 48000])
def test_other_sample_rates(dev, fs):
    x = _signal(fs + 777, fs, fs)
    m = R.measure(x, fs)
    assert R.gate_margin(m) > 1e-6
    loud, peak = _measure([x], dev, fs)
    print(f'{fs} Hz: L {loud[0]:.9f}, restatement {m["L"]:.9f}, difference {abs(loud[0] - m["L"]):.2e} LU')
    assert abs(loud[0] - m['L']) < L_TOL and peak[0] == m['peak']


def test_calibration_sine_and_gating_case(dev):
    sine = np.sin(2 * np.pi * 997.0 * np.arange(48000) / 48000.0).astype(np.float32)
    loud, peak = _measure([sine], dev, 48000)
    assert abs(loud[0] + 3.01) < 0.01 and abs(loud[0] - R.loudness(sine, 48000)) < L_TOL and peak[0] == np.abs(sine).max()
    x = R.gating_case()
    m = R.measure(x, 22050)
    loud, peak = _measure([x], dev)
    print(f'gating case: L {loud[0]:.9f} LUFS, restatement {m["L"]:.9f}')
    assert abs(loud[0] - m['L']) < L_TOL and abs(loud[0] + 17.81) < 0.01 and peak[0] == m['peak']


def test_silent_and_empty_rows(dev):
    """an all-zero row, a row at amplitude 1e-5 (every block below -70 LUFS) and n = 0: L = -inf, gain 1, the samples untouched"""
    from ttsamd.engine import leveller
    quiet = (np.random.default_rng(3).uniform(-1, 1, 11025) * 1e-5).astype(np.float32)
    assert R.measure(quiet, 22050)['L'] == -np.inf
    xs = [np.zeros(9000, np.float32), quiet, np.zeros(0, np.float32)]
    loud, peak = _measure(xs, dev)
    assert np.all(loud == -np.inf) and peak[0] == 0 and peak[1] == np.abs(quiet).max() and peak[2] == 0
    for mode, target in ((2, -23.0), (1, 0.99)):
        wave, lens = _poisoned(xs, dev)
        before = wave.clone()
        out, gain = leveller(22050, dev).level(wave, lens, mode, target)
        if mode == 2:
            assert gain.tolist() == [1.0, 1.0, 1.0] and torch.equal(out.view(torch.int32), before.view(torch.int32))
        else:                                        # peak mode lifts the quiet row, leaves the zero and the empty one
            assert gain[0] == 1 and gain[2] == 1 and torch.equal(out[[0, 2]].view(torch.int32), before[[0, 2]].view(torch.int32))
            assert float(out[1, :11025].abs().max()) == pytest.approx(0.99, abs=1e-7)
    # alone, with a stride of one sample and a length of zero
    loud, peak = _measure([np.zeros(0, np.float32)], dev)
    assert loud[0] == -np.inf and peak[0] == 0


RAGGED = [3 * 22050 + 777, 1, 8821, 17641, 11025]
RAGGED_MODE = [2, 1, 2, 1, 2]
RAGGED_TARGET = [-23.0, 0.99, -30.0, 0.5, -16.0]


def test_ragged_batch_has_the_bits_of_the_rows_alone(dev, rows):
    from ttsamd.engine import leveller
    eng = leveller(22050, dev)
    xs = [rows[n][0] for n in RAGGED]
    wave, lens = _poisoned(xs, dev, stride=RAGGED[0] + 100)
    loud, peak = eng.measure(wave, lens)
    out, gain = eng.level(wave, lens, RAGGED_MODE, RAGGED_TARGET)
    assert out.data_ptr() == wave.data_ptr()
    for b, x in enumerate(xs):
        w1, l1 = _poisoned([x], dev)
        loud1, peak1 = eng.measure(w1, l1)
        out1, gain1 = eng.level(w1, l1, RAGGED_MODE[b], RAGGED_TARGET[b])
        assert torch.equal(loud[b:b + 1].view(torch.int64), loud1.view(torch.int64)), b
        assert torch.equal(peak[b:b + 1].view(torch.int32), peak1.view(torch.int32)) and torch.equal(gain[b:b + 1].view(torch.int32), gain1.view(torch.int32)), b
        assert torch.equal(out[b, :len(x)].view(torch.int32), out1[0, :len(x)].view(torch.int32)), b
        assert bool(torch.isnan(out[b, len(x):]).all()), b          # nothing behind the length was written
        assert not bool(torch.isnan(out[b, :len(x)]).any()), b      # ... or read
        assert abs(float(loud[b]) - rows[len(x)][1]['L']) < L_TOL


def test_apply_is_numpys_float32_arithmetic(dev, rows):
    from ttsamd.engine import leveller
    eng = leveller(22050, dev)
    ns = [11025, 17641, 8821, 8820]
    modes, targets = [1, 2, 0, 2], [0.99, -23.0, 0.0, -40.0]
    xs = [rows[n][0] for n in ns]
    wave, lens = _poisoned(xs, dev)
    loud, peak = eng.measure(wave, lens)
    out, gain = eng.level(wave, lens, modes, targets)
    out, gain, loud, peak = out.cpu().numpy(), gain.cpu().numpy(), loud.cpu().numpy(), peak.cpu().numpy()
    for b, x in enumerate(xs):
        m = rows[len(x)][1]
        want_gain = R.gain(m['L'], m['peak'], modes[b], targets[b])
        assert abs(gain[b] / want_gain - 1) < 1e-6, (b, gain[b], want_gain)
        want = R.apply(x, modes[b], targets[b], peak[b], gain[b], loud[b])
        assert np.array_equal(out[b, :len(x)].view(np.int32), want.view(np.int32)), b
        assert np.isnan(out[b, len(x):]).all()
    assert gain[2] == 1 and np.array_equal(out[2, :ns[2]].view(np.int32), xs[2].view(np.int32))        # mode 0: untouched
    assert gain[0] == np.float32(0.99) / peak[0]
    # peak mode has the bits of the host helper on the same samples
    from utils.audio import peak_normalise
    assert np.array_equal(out[0, :ns[0]], peak_normalise(torch.from_numpy(xs[0])).numpy())
    assert np.array_equal(out[0, :ns[0]], peak_normalise(xs[0], np.float32(0.99)))


def test_ceiling_binds_and_the_target_is_met(dev, rows):
    from ttsamd.engine import leveller
    eng = leveller(22050, dev)
    spiky = (np.random.default_rng(9).standard_normal(22050) * 1e-3).astype(np.float32)
    spiky[5000] = 0.9
    m = R.measure(spiky, 22050)
    assert np.isfinite(m['L']) and 0.9 * 10 ** ((-10.0 - m['L']) / 20) > 0.99          # the target would lift the spike above the ceiling
    wave, lens = _poisoned([spiky], dev)
    out, gain = eng.level(wave, lens, 2, -10.0, ceiling=0.99)
    assert float(gain[0]) == R.gain(m['L'], m['peak'], 2, -10.0) and abs(float(gain[0]) / 1.1 - 1) < 2e-7
    assert float(out[0].abs().max()) <= np.float32(0.99)
    out, gain = eng.level(_poisoned([spiky], dev)[0], lens, 2, -10.0, ceiling=0.5)
    assert float(out[0].abs().max()) <= 0.5 and float(gain[0]) == R.gain(m['L'], m['peak'], 2, -10.0, 0.5)
    # no cap: measuring again gives the target
    x, m = rows[3 * 22050 + 777]
    wave, lens = _poisoned([x], dev)
    out, gain = eng.level(wave, lens, 2, -23.0)
    assert float(gain[0]) * float(m['peak']) < 0.99
    again, _ = eng.measure(out, lens)
    print(f'levelled to -23 LUFS from {m["L"]:.4f}: measures {float(again[0]):.7f}')
    assert abs(float(again[0]) + 23.0) < 1e-4


def test_refusals(dev, rows):
    from ttsamd import lib
    from ttsamd.engine import leveller
    from ttsamd.lib import TtsAmdError
    h = lib.load()
    x = rows[8821][0]
    wave, lens = _poisoned([x], dev)
    before = wave.clone()
    n = wave.shape[1]
    loud = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    peak = torch.full((1,), 7.0, dtype=torch.float32, device=dev)
    nb = h.ttsamd_loudness_workspace_bytes(1, n, 22050)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)

    def measure(wave_=wave, lens_=lens, B=1, fs=22050, loud_=loud, peak_=peak, ws_=ws, nb_=nb):
        return h.ttsamd_loudness_measure(_ptr(wave_), n, _ptr(lens_), B, fs, _ptr(loud_), _ptr(peak_), _ptr(ws_), nb_, _stream())
    for kw in (dict(wave_=None), dict(lens_=None), dict(loud_=None), dict(peak_=None), dict(ws_=None), dict(B=0), dict(B=-1), dict(nb_=nb - 1),
               dict(nb_=0), dict(fs=7999), dict(fs=192001)):
        assert measure(**kw) == EINVAL, kw
        assert b'loudness_measure' in h.ttsamd_last_error()
    torch.cuda.synchronize()
    assert float(loud[0]) == 7.0 and float(peak[0]) == 7.0                  # nothing was launched
    assert measure() == 0
    mode = torch.tensor([2], dtype=torch.int32, device=dev)
    target = torch.tensor([-23.0], dtype=torch.float32, device=dev)
    gain = torch.full((1,), 7.0, dtype=torch.float32, device=dev)

    def level(wave_=wave, lens_=lens, B=1, mode_=mode, target_=target, ceiling=0.99, loud_=loud, peak_=peak, gain_=gain):
        return h.ttsamd_wave_level(_ptr(wave_), n, _ptr(lens_), B, _ptr(mode_), _ptr(target_), ceiling, _ptr(loud_), _ptr(peak_), _ptr(gain_), _stream())
    for kw in (dict(wave_=None), dict(lens_=None), dict(mode_=None), dict(target_=None), dict(loud_=None), dict(peak_=None), dict(gain_=None),
               dict(B=0), dict(ceiling=0.0), dict(ceiling=-0.5), dict(ceiling=1.5), dict(ceiling=float('nan'))):
        assert level(**kw) == EINVAL, kw
        assert b'wave_level' in h.ttsamd_last_error()
    torch.cuda.synchronize()
    assert float(gain[0]) == 7.0 and torch.equal(wave.view(torch.int32), before.view(torch.int32))
    assert level(ceiling=1.0) == 0
    # a mode outside 0 .. 2 is refused where it is still a host value, before anything is launched ...
    eng = leveller(22050, dev)
    for bad in (3, -1, 'rms', 1.5, [0, 3], None):
        w2 = before.clone()
        with pytest.raises((TtsAmdError, ValueError)):
            eng.level(w2, lens, bad, -23.0)
        assert torch.equal(w2.view(torch.int32), before.view(torch.int32))
    for bad in (dict(target=float('nan')), dict(ceiling=0.0), dict(ceiling=1.01)):
        with pytest.raises((TtsAmdError, ValueError)):
            eng.level(before.clone(), lens, 2, **dict(dict(target=-23.0), **bad))
    # ... and a device value outside 0 .. 2 leaves its row as mode 0 does
    w2 = before.clone()
    mode[0] = 5
    assert level(wave_=w2) == 0
    assert float(gain[0]) == 1.0 and torch.equal(w2.view(torch.int32), before.view(torch.int32))
    with pytest.raises(TtsAmdError):
        eng.measure(wave.cpu(), lens)
    with pytest.raises(TtsAmdError):
        leveller(7999, dev)


def test_audio_helpers(dev, rows):
    from utils import audio
    xs = [rows[n][0] for n in (11025, 8821)]
    wave, lens = _poisoned(xs, dev)
    before = wave.clone()
    L = audio.loudness(wave, lens=lens)
    assert L.dtype == torch.float64 and L.shape == (2,) and L.device.type == 'cuda'
    assert abs(float(L[0]) - rows[11025][1]['L']) < L_TOL and abs(float(L[1]) - rows[8821][1]['L']) < L_TOL
    out = audio.normalize_loudness(wave, target_lufs=-30.0, lens=lens)
    assert out.data_ptr() != wave.data_ptr() and torch.equal(wave.view(torch.int32), before.view(torch.int32))      # the caller's tensor stays
    again = audio.loudness(out, lens=lens)
    assert float((again + 30.0).abs().max()) < 1e-4
    one = torch.from_numpy(xs[0]).to(dev)
    pk = audio.peak_normalize(one, 0.5)
    assert pk.shape == one.shape and np.array_equal(pk.cpu().numpy(), xs[0] / np.abs(xs[0]).max() * np.float32(0.5))
    assert abs(float(audio.loudness(one)[0]) - rows[11025][1]['L']) < L_TOL


# ---- through the models ----
@pytest.fixture(scope='module')
def model(tmp_path_factory, synth_weights, dev):
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
    d = tmp_path_factory.mktemp('ckpt_level')
    torch.save({'model': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['fastpitch'].items()}, 'config': dict(NET_CONFIG),
                'symbols': list(text.symbols)}, d / 'fp.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, d / 'hg.pth')
    with open(d / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    return FastPitch2Wave(str(d / 'fp.pth'), vocoder_sd=str(d / 'hg.pth'), vocoder_config=str(d / 'config.json')).to(dev)


@pytest.fixture(scope='module')
def lines():
    """five of the shortest committed infer_text lines (35 - 42 tokens), unsorted"""
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        every = json.load(f)
    return [every[i] for i in (68, 14, 92, 63, 35)]


@pytest.fixture(scope='module')
def plain(model, lines):
    """{batch_size: tts(lines)}: the un-normalised waves of every path, made once"""
    return {bs: model.tts(lines, batch_size=bs) for bs in (1, 2, 32)}


@pytest.mark.parametrize('batch_size', [1, 2, 32])
def test_tts_peak_is_peak_normalise_of_the_plain_waves(model, lines, plain, batch_size):
    """batch_size 1 and 2: the pipelined list path (length-sorted alone groups / chunks with the collate sort); 32: one tts_batch call"""
    from utils.audio import peak_normalise
    waves = model.tts(lines, batch_size=batch_size, normalize='peak')
    for w, p in zip(waves, plain[batch_size]):
        assert w.device.type == 'cpu' and w.shape == p.shape
        assert torch.equal(w.view(torch.int32), peak_normalise(p).view(torch.int32))
        assert abs(float(w.abs().max()) - 0.99) < 1e-6


@pytest.mark.parametrize('batch_size', [1, 2, 32])
def test_tts_default_is_the_path_without_levelling(model, lines, plain, batch_size, monkeypatch):
    from models.fastpitch import networks as N
    monkeypatch.setattr(N, 'level_waves', lambda *a, **k: pytest.fail('normalize=None reached the levelling step'))
    for kw in (dict(normalize=None), dict(normalize=[None] * 5)):
        waves = model.tts(lines, batch_size=batch_size, **kw)
        for w, p in zip(waves, plain[batch_size]):
            assert torch.equal(w.view(torch.int32), p.view(torch.int32))


OPTIONS = [None, 'peak', -20.0, 'lufs', -30.0]


@pytest.mark.parametrize('batch_size', [1, 2, 32])
def test_tts_per_line_options(model, lines, plain, batch_size):
    """tts(lines, normalize=[None, 'peak', -20.0, 'lufs', -30.0]): wave i is (a) the plain wave of the same path levelled by ITS option,
    bit for bit (the option followed its line through the sort and the chunks), and (b) tts_single(line i, normalize=its option) within
    the tolerance the two un-normalised waves are held to (conftest.WAVE_TOL), times the gain, times 1 + 1.6 peak / rms: a difference
    d per sample moves a block's K-weighted rms (the weighting lifts by up to 4 dB = 1.6) by at most 1.6 d, so the gain by a share
    1.6 d / rms, which the peak sample multiplies.  For (b) the call also carries a per-line `speed` list: with scalars only, a chunk of
    batch_size > 1 is the reference's padded FastPitch batch, whose frame counts depend on the chunk's composition and are not
    tts_single's (tests/test_gpu_mixed_batch.py compares against tts_single under the same condition); a `normalize` list alone does
    not change that."""
    from ttsamd.engine import level_spec, leveller
    eng = leveller(22050, model.device)
    waves = model.tts(lines, batch_size=batch_size, normalize=OPTIONS)
    for i, (w, p, opt) in enumerate(zip(waves, plain[batch_size], OPTIONS)):
        assert w.shape == p.shape
        if opt is None:
            want, g = p, 1.0
        else:
            mode, target = level_spec(opt)
            out, gain = eng.level(p.to(model.device)[None].contiguous(), None, mode, target)
            want, g = out[0].cpu(), float(gain[0])
        assert torch.equal(w.view(torch.int32), want.view(torch.int32)), (i, opt)
    alone = model.tts(lines, batch_size=batch_size, normalize=OPTIONS, speed=[1.0] * len(lines))      # rows computed as if alone
    for i, (w, opt) in enumerate(zip(alone, OPTIONS)):
        single = model.tts_single(lines[i], denoise=0.005, normalize=opt)
        raw = model.tts_single(lines[i], denoise=0.005)
        peak_raw = float(raw.abs().max())
        g = float(single.abs().max()) / peak_raw if opt is not None and peak_raw > 0 else 1.0
        m = R.measure(raw.numpy(), 22050)
        rms = 10 ** ((m['L'] + 0.691) / 20) if np.isfinite(m['L']) else np.inf
        tol = WAVE_TOL * max(g, 1.0) * (1 + 1.6 * float(m['peak']) / rms)
        assert single.shape == w.shape, (i, single.shape, w.shape)
        err = float((w - single).abs().max())
        print(f'batch_size {batch_size}, line {i}, normalize={opt!r}: gain {g:.4f}, L {m["L"]:.2f} LUFS, against tts_single {err:.2e} (tol {tol:.2e})')
        assert single.shape == w.shape and err < tol
        if opt is None:
            assert torch.equal(single.view(torch.int32), raw.view(torch.int32))


def test_tts_batch_device_and_requests(model, lines, plain):
    wave, n = model.tts_batch_device(lines, denoise=0.005, normalize=OPTIONS)
    waves = model.tts(lines, batch_size=32, normalize=OPTIONS)
    for b, w in enumerate(waves):
        assert int(n[b]) == w.numel() and torch.equal(wave[b, :w.numel()].cpu().view(torch.int32), w.view(torch.int32))
        assert not bool(wave[b, w.numel():].any())
    reqs = [dict(text=t, **({} if o is None else dict(normalize=o))) for t, o in zip(lines, OPTIONS)]
    # tts_requests is tts with every option as a per-line list (the rows of FastPitch as if alone)
    lists = {k: [d] * len(lines) for k, d in type(model).REQUEST_DEFAULTS.items()}
    for w, v in zip(model.tts_requests(reqs, batch_size=32), model.tts(lines, batch_size=32, normalize=OPTIONS, **lists)):
        assert torch.equal(w.view(torch.int32), v.view(torch.int32))
    with pytest.raises(ValueError):
        model.tts(lines, normalize='rms')
    with pytest.raises(ValueError):
        model.tts_single(lines[0], normalize=float('nan'))
