"""CPU: output levelling without a GPU -- the float64 restatement (tests/loudness_ref.py) against the standard's own figures, the host entry
ttsamd_loudness_coefficients against the restatement, the segment scan against the sequential filter, and the host side of `normalize=`
(validation, and the option following its line through the collate sort and the chunks: fake engines as in tests/test_mixed_batch_cpu.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import loudness_ref as R

pytest.importorskip('ttsamd.lib')
from ttsamd import lib  # noqa: E402

if not os.path.exists(lib.LIB_PATH):
    pytest.skip('libttsamd.so not built', allow_module_level=True)

EINVAL = -1


def test_coefficients_at_48k_are_the_standards_table():
    for name, got in zip(('b1', 'a1', 'b2', 'a2'), R.coefficients(48000)):
        assert np.abs(got - np.array(R.TABLE_48K[name])).max() < 1e-13, name


@pytest.mark.parametrize('fs', [8000, 22050, 24000, 48000])
def test_library_coefficients_against_the_restatement(fs):
    out = (C.c_double * 10)()
    assert lib.load().ttsamd_loudness_coefficients(fs, out) == 0, lib.load().ttsamd_last_error()
    got, want = np.array(out), R.coefficient_vector(fs)
    rel = np.abs(got - want) / np.abs(want)
    print(f'{fs} Hz: largest relative difference {rel.max():.2e}')
    assert rel.max() < 1e-14
    if fs == 22050:                              # the poles of the high-pass
        assert abs(np.sqrt(want[9]) - 0.98920) < 5e-6


def test_library_refuses_rates_out_of_range():
    h, out = lib.load(), (C.c_double * 10)()
    for fs in (7999, 192001):
        assert h.ttsamd_loudness_coefficients(fs, out) == EINVAL and b'sample rate' in h.ttsamd_last_error()
        assert h.ttsamd_loudness_workspace_bytes(1, 1000, fs) == -1
    assert h.ttsamd_loudness_coefficients(8000, None) == EINVAL
    assert h.ttsamd_loudness_coefficients(8000, out) == 0 and h.ttsamd_loudness_coefficients(192000, out) == 0
    assert h.ttsamd_loudness_workspace_bytes(0, 1000, 22050) == -1 and h.ttsamd_loudness_workspace_bytes(1, -1, 22050) == -1
    assert h.ttsamd_loudness_workspace_bytes(2, 1000, 22050) > 0


def test_calibration_sine():
    """the standard's calibration: a 997 Hz full-scale sine reads -3.01 LUFS (mono)"""
    x = np.sin(2 * np.pi * 997.0 * np.arange(5 * 48000) / 48000.0).astype(np.float32)
    L = R.loudness(x, 48000)
    print(f'997 Hz full scale, 5 s at 48 kHz: {L:.4f} LUFS')
    assert abs(L + 3.01) < 0.01


def test_gating_case():
    m = R.measure(R.gating_case(), 22050)
    print(f'{len(m["z"])} blocks, L {m["L"]:.4f}, Gamma {m["gamma"]:.4f}, margin {R.gate_margin(m):.3f} LU')
    assert len(m['z']) == 27 and abs(m['L'] + 17.81) < 0.01 and abs(m['gamma'] + 27.81) < 0.01
    assert R.gate_margin(m) >= 1.2
    kept = m['l'] > m['gamma']
    assert 0 < kept.sum() < 27 and abs(m['L'] - (-0.691 + 10 * np.log10(m['z'][kept].mean()))) < 1e-12
    # without the gates the quiet second would pull the level down by 10 log10(27 / kept)
    assert abs((-0.691 + 10 * np.log10(m['z'].mean())) - (m['L'] + 10 * np.log10(kept.sum() / 27.0))) < 1e-3


def test_short_row_rule():
    step, block = R.step_block(22050)
    assert (step, block) == (2205, 8820) and R.step_block(48000) == (4800, 19200) and R.step_block(8000) == (800, 3200)
    x = (np.random.default_rng(1).standard_normal(block + step) * 0.2).astype(np.float32)
    for n in (1, block - 1):
        m = R.measure(x[:n], 22050)
        y = R.kweight(x[:n], 22050)
        assert len(m['z']) == 1 and m['z'][0] == (y ** 2).sum() / n and m['L'] == -0.691 + 10 * np.log10(m['z'][0])
    m = R.measure(x[:block], 22050)
    assert len(m['z']) == 1 and m['z'][0] == (R.kweight(x[:block], 22050) ** 2).sum() / block
    assert len(R.measure(x[:block + step - 1], 22050)['z']) == 1 and len(R.measure(x, 22050)['z']) == 2
    m0 = R.measure(x[:0], 22050)
    assert len(m0['z']) == 0 and m0['L'] == -np.inf and m0['peak'] == 0


@pytest.mark.parametrize('fs', [8000, 22050, 24000, 48000])
def test_segment_scan_against_the_sequential_filter(fs):
    step, _ = R.step_block(fs)
    S = R.segment_length(step)
    assert step % S == 0 and 32 <= S <= 64
    x = (np.random.default_rng(fs).standard_normal(fs + 777) * 0.2).astype(np.float32)
    y, yc = R.kweight(x, fs), R.kweight_chunked(x, fs)
    err = np.abs(y - yc).max() / np.abs(x).max()
    za, zb = R.block_energies(y, fs), R.block_energies(yc, fs)
    print(f'{fs} Hz, segments of {S}: scan against the sequential filter {err:.2e} of the peak, block energies {np.abs(za / zb - 1).max():.2e} relative')
    assert err < 1e-12 and np.abs(za / zb - 1).max() < 1e-11
    assert abs(R.measure(x, fs)['L'] - R.measure(x, fs, chunked=True)['L']) < 1e-10


def test_gain_rules():
    assert R.gain(-20.0, 0.5, 0, -23.0) == 1 and R.gain(-np.inf, 0.5, 2, -23.0) == 1 and R.gain(-20.0, 0.0, 2, -23.0) == 1 and R.gain(0, 0.0, 1, 0.99) == 1
    assert R.gain(-20.0, 0.5, 1, 0.99) == np.float32(0.99) / np.float32(0.5)
    assert abs(R.gain(-20.0, 0.1, 2, -23.0) - 10 ** (-3 / 20)) < 1e-7
    g = R.gain(-30.0, 0.5, 2, -10.0)                       # 10x would lift the peak to 5: capped
    assert abs(g / 1.98 - 1) < 2e-7 and np.float32(0.5) * g <= np.float32(0.99)
    assert all(np.float32(p) * R.gain(-30.0, p, 2, -10.0, c) <= np.float32(c) for p in (0.9, 0.7, 0.3, 0.11) for c in (0.99, 0.5, 1.0))


def test_check_line_controls_takes_normalize():
    from models.fastpitch.networks import check_line_controls
    from ttsamd.engine import level_spec
    for ok in (None, 'peak', 'lufs', -16.0, -23, np.float32(-19.0), [None, 'peak', -20.0], ('lufs', None, None), [None] * 3):
        check_line_controls(3, 1, normalize=ok)
    for bad in ('rms', 'PEAK', float('nan'), float('inf'), True, [None, 'peak'], [None, 'peak', 'loud'], [None, float('nan'), -20.0], [[-20.0]] * 3):
        with pytest.raises(ValueError):
            check_line_controls(3, 1, normalize=bad)
    assert level_spec(None) is None and level_spec('peak') == (1, 0.99) and level_spec('lufs') == (2, -23.0) and level_spec(-16) == (2, -16.0)


LENGTHS = [3, 9, 1, 7, 5, 9, 2]
LINES = [str(i) for i in range(len(LENGTHS))]
NORM = [None, 'peak', -20.0, 'lufs', None, -16.0, 'peak']


def _fakes(monkeypatch):
    """the fakes of tests/test_mixed_batch_cpu.py (a row of a batch names its line by its value) + a recorder in place of level_waves"""
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

    def fake_level(wave, nsamples, normalize, sample_rate=22050, ceiling=0.99):
        levelled.append(([int(v) for v in wave[:, 0].tolist()], normalize, None if nsamples is None else nsamples.tolist(), sample_rate))
        return wave

    monkeypatch.setattr(N, 'level_waves', fake_level)
    return N, FakeTts(), levelled


def test_normalize_follows_the_chunks_and_the_collate_sort(monkeypatch):
    N, tts, levelled = _fakes(monkeypatch)
    waves = tts.tts(LINES, batch_size=3, normalize=NORM)
    assert [int(w[0]) for w in waves] == list(range(7))
    assert [sorted(rows) for rows, *_ in levelled] == [[0, 1, 2], [3, 4, 5], [6]]
    for rows, options, n, rate in levelled:
        assert options == [NORM[i] for i in rows] and n == [4 * LENGTHS[i] for i in rows] and rate == 22050
        assert [LENGTHS[i] for i in rows] == sorted((LENGTHS[i] for i in rows), reverse=True)     # the collate order
    # one option for every line stays the scalar it was
    levelled.clear()
    tts.tts(LINES, batch_size=4, normalize='lufs')
    assert [opt for _, opt, *_ in levelled] == ['lufs', 'lufs']
    # None, or nothing but None: the levelling step is not reached at all
    levelled.clear()
    tts.tts(LINES, batch_size=3)
    tts.tts(LINES, batch_size=3, normalize=None)
    tts.tts(LINES, batch_size=3, normalize=[None] * 7)
    tts.tts(LINES, batch_size=1, normalize=[None] * 7)
    assert levelled == []
    # batch_size 1 on the one-stream path: every line with its own option
    tts.tts(LINES, batch_size=1, normalize=NORM)
    assert [(rows, opt) for rows, opt, *_ in levelled] == [([i], NORM[i]) for i in range(7) if NORM[i] is not None]
    # refused before any work
    levelled.clear()
    for bad in (NORM[:3], 'rms', [None] * 6 + [float('nan')], [None] * 8):
        with pytest.raises(ValueError):
            tts.tts(LINES, batch_size=3, normalize=bad)
    assert levelled == []


def test_tts_requests_passes_normalize_through(monkeypatch):
    N, tts, levelled = _fakes(monkeypatch)
    got = {}
    monkeypatch.setattr(tts, 'tts', lambda texts, **kw: got.update(texts=texts, **kw) or ['w'] * len(texts))
    reqs = [dict(text='3', normalize='peak'), dict(text='0'), dict(text='5', normalize=-16.0, denoise=0.0)]
    assert tts.tts_requests(reqs, batch_size=8) == ['w'] * 3
    assert got['normalize'] == ['peak', None, -16.0] and got['denoise'] == [0.005, 0.005, 0.0] and got['texts'] == ['3', '0', '5']
    got.clear()
    tts.tts_requests([dict(text='1'), dict(text='2', normalize=None)])
    assert 'normalize' not in got                         # no request asks for a level: today's call
    with pytest.raises(ValueError):
        tts.tts_requests([dict(text='1', normalise='peak')])


def test_device_helpers_refuse_a_cpu_tensor():
    from ttsamd.lib import TtsAmdError
    from utils import audio
    x = torch.zeros(2, 100)
    for call in (lambda: audio.loudness(x), lambda: audio.normalize_loudness(x), lambda: audio.peak_normalize(x)):
        with pytest.raises(TtsAmdError):
            call()


def test_the_four_symbols_are_in_the_table():
    for name in ('ttsamd_loudness_coefficients', 'ttsamd_loudness_workspace_bytes', 'ttsamd_loudness_measure', 'ttsamd_wave_level'):
        assert name in lib.SYMBOLS and getattr(lib.load(), name) is not None
    assert lib.ABI_VERSION == 8 == lib.load().ttsamd_version()
