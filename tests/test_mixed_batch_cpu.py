"""CPU: the host side of mixed requests in one batch -- per-line speed / speaker_id / pitch_mul / pitch_add / denoise lists follow their lines
through the collate sort and the chunking, the host-side validation, and the four new symbols in the ctypes table.  Fake engines stand in
for the GPU: they record which controls arrive with which row.  (The length-sorted groups of the batch_size = 1 pipeline run on HIP
streams: tests/test_gpu_mixed_batch.py covers them.)"""
import os

import pytest
import torch

pytest.importorskip('ttsamd.lib')
from ttsamd import lib  # noqa: E402

if not os.path.exists(lib.LIB_PATH):
    pytest.skip('libttsamd.so not built', allow_module_level=True)

# line i = (i + 1) repeated LENGTHS[i] times: a row of the padded batch names its line by its first token
LENGTHS = [3, 9, 1, 7, 5, 9, 2]
SPEED = [0.5, 0.6, 0.7, 0.8, 0.9, 1.0, 1.1]
SPK = [0, 1, 2, 3, 0, 1, 2]
MUL = [1.0, 1.1, 1.2, 1.3, 1.4, 1.5, 1.6]
ADD = [0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
DN = [0.0, 0.01, 0.0, 0.03, 0.04, 0.0, 0.06]
LINES = [str(i) for i in range(len(LENGTHS))]


def _fakes(monkeypatch):
    from models.fastpitch import networks as N
    from vocoder.hifigan.models import _HipModule
    monkeypatch.setattr(N.text, 'tokens_to_ids', lambda toks, table: toks)
    calls = []

    class FakeFastPitch(N.FastPitch):
        def __init__(self):
            _HipModule.__init__(self)
            self.net_config = dict(n_speakers=4, padding_idx=0, n_symbols=100)
            self.phon_to_id, self.default_vowelizer = None, None

        def _tokenize(self, line, vowelizer=None):
            i = int(line)
            return [i + 1] * LENGTHS[i]

        def infer(self, ids, pace=1.0, speaker=0, alone=False, pitch_transform=None, pitch_mul=None, pitch_add=None, **kw):
            rows = [int(r[0]) - 1 for r in ids]
            calls.append(dict(rows=rows, pace=pace, speaker=speaker, pitch_mul=pitch_mul, pitch_add=pitch_add,
                              pitch_transform=pitch_transform, alone=alone))
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

    class FakeDenoiser:
        def __init__(self):
            self.seen = []

        def forward_batch(self, wave, n, strength, nsamples_min=None):
            self.seen.append((wave[:, 0].tolist(), strength))
            return wave

    class FakeTts(N.FastPitch2Wave):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.model, self.vocoder, self.denoiser = FakeFastPitch(), FakeVocoder(), FakeDenoiser()

    return N, FakeTts(), calls


def _check_rows(call, speed=SPEED, spk=SPK, mul=MUL, add=ADD):
    for b, i in enumerate(call['rows']):
        assert call['pace'][b] == speed[i] and call['speaker'][b] == spk[i], (call, b)
        assert call['pitch_mul'][b] == mul[i] and call['pitch_add'][b] == add[i], (call, b)


def test_controls_follow_the_collate_sort(monkeypatch):
    """ttmel_batch sorts the lines by length (text_collate_fn); row b of the padded batch must arrive with the controls of ITS line, and
    the mels go back in the order of the lines."""
    N, tts, calls = _fakes(monkeypatch)
    mels = tts.model.ttmel_batch(LINES, speed=SPEED, speaker_id=SPK, pitch_mul=MUL, pitch_add=ADD)
    assert len(calls) == 1 and calls[0]['rows'] != list(range(7)) and sorted(calls[0]['rows']) == list(range(7))
    assert [LENGTHS[i] for i in calls[0]['rows']] == sorted(LENGTHS, reverse=True)
    _check_rows(calls[0])
    assert calls[0]['pitch_transform'] is None and calls[0]['alone'] is True     # mixed requests are independent: rows as if alone
    assert [int(m[0, 0]) for m in mels] == list(range(7)) and [m.shape[1] for m in mels] == LENGTHS
    # one list is enough; a scalar stays the scalar it was (and the pitch pair still goes through the tagged transform)
    calls.clear()
    tts.model.ttmel_batch(LINES, speed=SPEED, pitch_mul=1.5)
    c = calls[0]
    assert [c['pace'][b] for b in range(7)] == [SPEED[i] for i in c['rows']] and c['speaker'] == 0
    assert c['pitch_mul'] is None and c['pitch_transform'].affine == (1.5, 0.0)
    # all scalars: today's call, unchanged
    calls.clear()
    tts.model.ttmel_batch(LINES, speed=1.25, speaker_id=3)
    assert calls[0]['pace'] == 1.25 and calls[0]['speaker'] == 3 and calls[0]['pitch_transform'] is None and calls[0]['pitch_mul'] is None
    assert calls[0]['alone'] is False                    # ... in the reference's padded-batch arithmetic


def test_controls_follow_the_chunks_and_the_denoise_list_the_sort(monkeypatch):
    """tts(list, batch_size=3) on the one-stream path: chunk k gets the slices of every list, each chunk sorts on its own, the denoiser sees
    the strengths in the order of the rows it is given, and wave i answers line i."""
    N, tts, calls = _fakes(monkeypatch)
    waves = tts.tts(LINES, batch_size=3, speed=SPEED, speaker_id=SPK, pitch_mul=MUL, pitch_add=ADD, denoise=DN)
    assert [sorted(c['rows']) for c in calls] == [[0, 1, 2], [3, 4, 5], [6]]
    for c in calls:
        _check_rows(c)
    assert [int(w[0]) for w in waves] == list(range(7)) and [w.numel() for w in waves] == [4 * n for n in LENGTHS]
    seen = tts.denoiser.seen
    assert len(seen) == 3                                # every chunk has a line with denoise > 0
    for rows, strengths in seen:
        assert strengths == [DN[int(i)] for i in rows]
    # a chunk whose strengths are all zero is not denoised at all (what `if denoise > 0` does for a scalar)
    tts.denoiser.seen.clear()
    tts.tts(LINES, batch_size=3, denoise=[0, 0, 0, 0.1, 0, 0, 0])
    assert [len(s[0]) for s in tts.denoiser.seen] == [3]
    # ttmel chunks the same way; batch_size 1 takes the scalars of each line
    calls.clear()
    tts.model.ttmel(LINES, batch_size=2, speed=SPEED, speaker_id=SPK, pitch_mul=MUL, pitch_add=ADD)
    assert [sorted(c['rows']) for c in calls] == [[0, 1], [2, 3], [4, 5], [6]]
    for c in calls:
        _check_rows(c)


def test_tts_requests_builds_the_lists(monkeypatch):
    N, tts, calls = _fakes(monkeypatch)
    got = {}
    monkeypatch.setattr(tts, 'tts', lambda texts, **kw: got.update(texts=texts, **kw) or ['w'] * len(texts))
    reqs = [dict(text='3', speed=0.8, speaker_id=2), dict(text='0'), dict(text='5', denoise=0.0, pitch_mul=1.2, pitch_add=-0.1)]
    assert tts.tts_requests(reqs, batch_size=8) == ['w'] * 3
    assert got['texts'] == ['3', '0', '5'] and got['batch_size'] == 8
    assert got['speed'] == [0.8, 1.0, 1.0] and got['speaker_id'] == [2, 0, 0] and got['denoise'] == [0.005, 0.005, 0.0]
    assert got['pitch_mul'] == [1.0, 1.0, 1.2] and got['pitch_add'] == [0.0, 0.0, -0.1]
    for bad in ([dict(speed=1.0)], [dict(text='1', tempo=2)], [dict(text=7)]):
        with pytest.raises(ValueError):
            tts.tts_requests(bad)


def test_host_side_validation(monkeypatch):
    from ttsamd import engine as E
    N, tts, calls = _fakes(monkeypatch)
    assert E.per_row([1]) and E.per_row((1, 2)) and E.per_row(torch.zeros(2)) and not E.per_row(1.0) and not E.per_row(torch.tensor(1.0))
    assert E.row_values(torch.tensor([1.0, 2.0]), 2, 'x') == [1.0, 2.0]
    with pytest.raises(ValueError):
        E.row_values([1, 2, 3], 2, 'x')
    E.check_speakers([0, 3], 4)
    E.check_speakers([7], 1)                             # a single-speaker model ignores the index, as the scalar entry does
    for bad in ([4], [-1]):
        with pytest.raises(IndexError):
            E.check_speakers(bad, 4)
    with pytest.raises(ValueError):
        E.check_speakers([1.5], 4)
    E.check_finite([0.0, -1.0], 'pitch_add')
    for bad in ([0.0], [-0.5], [float('nan')], [float('inf')]):
        with pytest.raises(ValueError):
            E.check_finite(bad, 'pace', positive=True)
    with pytest.raises(ValueError):
        E.check_finite([float('nan')], 'pitch_mul')
    # the wrappers refuse before any work
    for kw, exc in ((dict(speed=SPEED[:3]), ValueError), (dict(speaker_id=[0, 1, 2, 3, 4, 1, 2]), IndexError), (dict(speed=[1] * 6 + [0]), ValueError),
                    (dict(speed=[1] * 6 + [-1]), ValueError), (dict(pitch_add=[0] * 6 + [float('nan')]), ValueError),
                    (dict(denoise=[0] * 6 + [float('nan')]), ValueError)):
        with pytest.raises(exc):
            tts.tts(LINES, batch_size=3, **kw)
    assert calls == []
    with pytest.raises(ValueError):                      # a custom transform cannot be applied per row
        tts.model.ttmel_batch(LINES, pitch_mul=MUL, pitch_transform=lambda p, *a: p)
    with pytest.raises(ValueError):
        N.FastPitch.infer(tts.model, torch.ones(2, 3, dtype=torch.long), pitch_add=[0.1, 0.2], pitch_transform=N.pitch_trf(2.0, 0.0))
    assert calls == []


def test_the_data_parallel_path_refuses_lists():
    from ttsamd.dp import tts_sharded
    with pytest.raises(ValueError, match='speed'):
        tts_sharded(object(), ['a', 'b'], speed=[1.0, 2.0], dp=object())
    with pytest.raises(ValueError, match='denoise'):
        tts_sharded(object(), ['a', 'b'], denoise=torch.tensor([0.0, 0.1]), dp=object())


def test_the_four_symbols_are_in_the_table():
    for name in ('ttsamd_fastpitch_encode_rows', 'ttsamd_fastpitch_decode_rows', 'ttsamd_denoise_rows', 'ttsamd_vocos_forward_rows'):
        assert name in lib.SYMBOLS and getattr(lib.load(), name) is not None
    enc, enc_rows = lib.SYMBOLS['ttsamd_fastpitch_encode'][1], lib.SYMBOLS['ttsamd_fastpitch_encode_rows'][1]
    assert enc_rows[:len(enc) - 1] == enc[:-1] and len(enc_rows) == len(enc) + 5          # + four row arrays and flags, the stream last
    dec, dec_rows = lib.SYMBOLS['ttsamd_fastpitch_decode'][1], lib.SYMBOLS['ttsamd_fastpitch_decode_rows'][1]
    assert dec_rows[:len(dec) - 1] == dec[:-1] and len(dec_rows) == len(dec) + 1
    assert len(lib.SYMBOLS['ttsamd_denoise_rows'][1]) == len(lib.SYMBOLS['ttsamd_denoise'][1])
    assert len(lib.SYMBOLS['ttsamd_vocos_forward_rows'][1]) == len(lib.SYMBOLS['ttsamd_vocos_forward'][1])
    assert lib.ABI_VERSION == 8 == lib.load().ttsamd_version()
