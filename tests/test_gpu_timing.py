"""GPU: token and word spans (csrc/timing.hip, ttsamd/timing.py) against their numpy statement (tests/timing_ref.py, pinned by
tests/test_timing_cpu.py): exact integer equality over the WHOLE output arrays; and the timestamps of the synthesis entry points on the
synthetic checkpoints."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch

import timing_ref as R
from conftest import GOLDEN, WAVE_TOL

pytestmark = pytest.mark.gpu

SENTINEL = -7777


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    from ttsamd import lib
    assert lib.load().ttsamd_device_ok() == 1
    return torch.device('cuda:0')


def _reps(B, L, stride, seed):
    """values 0 .. 75 with zeros, a run of zeros across every wave edge it can reach, one negative value per row; what lies behind L in a
    row of the wider stride is large (it must not be read)"""
    rng = np.random.default_rng(seed)
    reps = rng.integers(0, 76, size=(B, stride)).astype(np.int64)
    reps[rng.random((B, stride)) < 0.15] = 0
    for edge in (64, 256, 1024):
        if L > edge + 2:
            reps[:, edge - 2:edge + 3] = 0
    reps[:, L // 2] = -5
    reps[:, L:] = 1 << 40
    return reps


def _call(dev, reps, L, n_tokens=None, groups=None, n_groups=None, hop=256, maps=None, B=None, want_grp=None, G=None):
    """ttsamd_token_spans through the C ABI into buffers filled with a sentinel -> (rc, tok [B, L, 2], grp [B, G, 2] or None)"""
    from ttsamd import lib
    h = lib.load()
    B = reps.shape[0] if B is None else B
    up = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=dt))).to(dev)   # noqa: E731
    r, n, g, ng, m = up(reps, np.int64), up(n_tokens, np.int64), up(groups, np.int32), up(n_groups, np.int32), up(maps, np.int64)
    G = (0 if groups is None else np.asarray(groups).shape[1]) if G is None else G
    tok = torch.full((max(reps.shape[0], 1), max(L, 1), 2), SENTINEL, dtype=torch.int64, device=dev)
    want_grp = (groups is not None) if want_grp is None else want_grp
    grp = torch.full((max(reps.shape[0], 1), max(G, 1), 2), SENTINEL, dtype=torch.int64, device=dev) if want_grp else None
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)                # noqa: E731
    rc = h.ttsamd_token_spans(p(r), reps.shape[1], p(n), B, L, p(g), p(ng), G, hop, p(m), p(tok), p(grp),
                              C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, tok.cpu().numpy(), None if grp is None else grp.cpu().numpy()


def _groups(B, L, ns, G=7):
    """per row: a first range starting past token 0, ranges that touch, an empty range, one reaching past n (clamped), n_groups < G"""
    groups = np.zeros((B, G, 2), dtype=np.int32)
    n_groups = np.zeros(B, dtype=np.int32)
    for b in range(B):
        n = int(ns[b])
        a = min(1, n)
        q = [a, a + (n - a) // 4, a + (n - a) // 2, n]
        rows = [(q[0], q[1]), (q[1], q[2]), (q[2], q[2]), (q[2] + 1, q[3] - 1), (q[3] - 1, n + 9), (n + 3, n + 5)]
        groups[b, :len(rows)] = rows
        groups[b, len(rows):] = (1, 2)                                 # behind n_groups: not read as a range
        n_groups[b] = len(rows) - (b % 2)
    return groups, n_groups


MAPS = {
    'null': None,
    'cut': lambda c_end, hop: (hop // 2 + 3, max(c_end * hop - hop - 7, hop // 2 + 3), 0, 1, 1),       # into the first and last token
    'swallow': lambda c_end, hop: (min(200 * hop, c_end * hop), max(c_end * hop - 300 * hop, min(200 * hop, c_end * hop)), 1234, 1, 1),
    '8k': lambda c_end, hop: (0, R.INT64_MAX, 0, 160, 441),
    '37/40': lambda c_end, hop: (5, c_end * hop, 11, 37, 40),
}


@pytest.mark.parametrize('L', [1, 63, 64, 65, 255, 256, 257, 1025, 8192])
def test_token_spans_kernel_is_the_reference(dev, L):
    """B = 1 and B = 3 (ragged n_tokens with n = 0 and n = L, reps_stride > L; at the cap one row), every map, with and without groups"""
    for B in ((1,) if L == 8192 else (1, 3)):
        stride = L + (5 if B == 3 else 0)
        reps = _reps(B, L, stride, seed=L + B)
        ns = [L] if B == 1 else [L, 0, max(L - 3, 0)]
        groups, n_groups = _groups(B, L, ns)
        for name, fn in MAPS.items():
            maps = None
            if fn is not None:
                ends = [int(np.maximum(reps[b, :ns[b]], 0).sum()) for b in range(B)]
                maps = np.array([fn(ends[b], 256) for b in range(B)], dtype=np.int64)
            for with_groups in (True, False):
                kw = dict(n_tokens=None if B == 1 else ns, hop=256, maps=maps)
                if with_groups:
                    kw.update(groups=groups, n_groups=n_groups)
                want_tok, want_grp = R.token_spans(reps[:, :L], **kw)
                rc, tok, grp = _call(dev, reps, L, **kw)
                assert rc == 0, (name, B)
                assert np.array_equal(tok, want_tok), (name, B, with_groups, np.argwhere(tok != want_tok)[:3])
                if with_groups:
                    assert np.array_equal(grp, want_grp), (name, B, np.argwhere(grp != want_grp)[:3])
        # n_groups = NULL: all G ranges are read
        want_tok, want_grp = R.token_spans(reps[:, :L], n_tokens=ns, groups=groups, hop=3)
        rc, tok, grp = _call(dev, reps, L, n_tokens=ns, groups=groups, hop=3)
        assert rc == 0 and np.array_equal(tok, want_tok) and np.array_equal(grp, want_grp)


def test_token_spans_bad_map_row_is_minus_one_and_alone(dev):
    """den = 0, num past 2^20 and hi < lo each turn their own row to -1; the rows beside them are what they are without them"""
    L, B = 70, 4
    reps = _reps(B, L, L, seed=3)
    ns = [L, 5, L - 1, 64]
    groups, n_groups = _groups(B, L, ns)
    good = np.array([(3, 9000, 5, 160, 441)] * B, dtype=np.int64)
    want_tok, want_grp = R.token_spans(reps, ns, groups, n_groups, 256, good)
    for row, bad in ((1, (3, 9000, 5, 160, 0)), (0, (3, 9000, 5, (1 << 20) + 1, 441)), (3, (10, 9, 0, 1, 1)), (2, (0, 5, 0, -1, 1))):
        maps = good.copy()
        maps[row] = bad
        rc, tok, grp = _call(dev, reps, L, ns, groups, n_groups, 256, maps)
        ref_tok, ref_grp = R.token_spans(reps, ns, groups, n_groups, 256, maps)
        assert rc == 0 and np.array_equal(tok, ref_tok) and np.array_equal(grp, ref_grp)
        assert (tok[row] == -1).all() and (grp[row] == -1).all()
        keep = [b for b in range(B) if b != row]
        assert np.array_equal(tok[keep], want_tok[keep]) and np.array_equal(grp[keep], want_grp[keep])


def test_token_spans_refusals_leave_the_outputs_alone(dev):
    from ttsamd import lib
    reps = _reps(2, 16, 16, seed=1)
    groups, n_groups = _groups(2, 16, [16, 16])
    big = np.zeros((1, 8193), dtype=np.int64)
    cases = [dict(B=0), dict(L=0), dict(G=-1, groups=groups, n_groups=n_groups), dict(hop=0), dict(hop=-256),
             dict(groups=groups, n_groups=n_groups, want_grp=False)]
    for kw in cases:
        L = kw.pop('L', 16)
        rc, tok, grp = _call(dev, reps, L, **kw)
        assert rc == -1 and lib.load().ttsamd_last_error(), kw
        assert (tok == SENTINEL).all() and (grp is None or (grp == SENTINEL).all()), kw
    rc, tok, _ = _call(dev, big, 8193)
    assert rc == -1 and (tok == SENTINEL).all()


def test_token_spans_wrapper_checks_like_join_rows(dev):
    """ttsamd.timing.token_spans: device tensors in, device tensors out, the same numbers; host-checkable mistakes raise"""
    from ttsamd.lib import TtsAmdError
    from ttsamd.timing import token_spans
    reps = _reps(3, 65, 70, seed=9)
    ns = [65, 0, 33]
    groups, n_groups = _groups(3, 65, ns)
    maps = np.array([(0, R.INT64_MAX, 0, 160, 441)] * 3, dtype=np.int64)
    wide = torch.from_numpy(reps).to(dev)
    tok, grp = token_spans(wide[:, :65], torch.tensor(ns), torch.from_numpy(groups), torch.from_numpy(n_groups), 256, torch.from_numpy(maps))
    want_tok, want_grp = R.token_spans(reps[:, :65], ns, groups, n_groups, 256, maps)
    assert tok.device.type == 'cuda' and np.array_equal(tok.cpu().numpy(), want_tok) and np.array_equal(grp.cpu().numpy(), want_grp)
    tok, grp = token_spans(wide[:, :65])
    assert grp is None and np.array_equal(tok.cpu().numpy(), R.token_spans(reps[:, :65])[0])
    with pytest.raises(TtsAmdError):
        token_spans(torch.from_numpy(reps))                            # on the host
    with pytest.raises(TtsAmdError):
        token_spans(wide[:, :65], torch.tensor([1, 2]))                # n_tokens for two rows
    with pytest.raises(TtsAmdError):
        token_spans(wide[:, :65], groups=torch.zeros(3, 4, 3))
    with pytest.raises(TtsAmdError):
        token_spans(torch.zeros(1, 8193, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        token_spans(wide[:, :65], hop=0)


# ---- through the models (synthetic checkpoints, built as tests/test_gpu_join.py builds them) ----
@pytest.fixture(scope='module')
def model(tmp_path_factory, synth_weights, dev):
    import text
    from models.fastpitch import FastPitch2Wave
    from ttsamd.config import HIFIGAN_CONFIG, NET_CONFIG
    d = tmp_path_factory.mktemp('ckpt_timing')
    sd = dict(synth_weights['fastpitch'])
    from ttsamd import synth
    sd.update(synth.fastpitch_aligner_state_dict(gain=8.0))
    torch.save({'model': {k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, 'config': dict(NET_CONFIG),
                'symbols': list(text.symbols)}, d / 'fp.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, d / 'hg.pth')
    with open(d / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    return FastPitch2Wave(str(d / 'fp.pth'), vocoder_sd=str(d / 'hg.pth'), vocoder_config=str(d / 'config.json')).to(dev), d


@functools.lru_cache(maxsize=None)
def _corpus():
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        return json.load(f)


LINES = (9, 14, 92, 63, 35)          # short committed lines (the ones tests/test_gpu_join.py joins)


def _lines(n=5):
    return [_corpus()[i] for i in LINES[:n]]


def _consistent(timing, wave, line):
    """a timing against its own wave and line: the last token ends where the wave does, tokens tile [0, end], word k covers
    word_ranges' k-th range, and what lies between two words is exactly the separators' spans"""
    import text
    toks, words = timing['tokens'], timing['words']
    assert timing['sample_rate'] == 22050 and toks[-1]['end'] == wave.numel() and toks[0]['start'] == 0
    assert all(a['end'] == b['start'] for a, b in zip(toks, toks[1:])) and all(t['start'] <= t['end'] for t in toks)
    names = [t['token'] for t in toks]
    ranges = text.word_ranges(names)
    assert [w['tokens'] for w in words] == ranges and [w['word'] for w in words] == text.line_words(line)
    for w, (i0, i1) in zip(words, ranges):
        if i1 > i0:
            assert (w['start'], w['end']) == (toks[i0]['start'], toks[i1 - 1]['end'])
        assert w['t0'] == w['start'] / 22050 and w['t1'] == w['end'] / 22050
    for a, b in zip(words, words[1:]):
        between = toks[a['tokens'][1]:b['tokens'][0]]
        assert all(t['token'] == text.SEPARATOR_TOKEN for t in between)
        assert b['start'] - a['end'] == sum(t['end'] - t['start'] for t in between)


def test_fastpitch_spans_are_the_runs_of_the_frame_index(model):
    """infer(return_idx=True) names the source token of every frame: the token spans of the same call / hop are exactly its runs"""
    import text
    from ttsamd.timing import token_spans
    m, _ = model
    rows = [text.tokens_to_ids(m.model._tokenize(l), m.model.phon_to_id) for l in _lines(3)]
    ids = torch.zeros(3, max(len(r) for r in rows), dtype=torch.int64)
    for b, r in enumerate(rows):
        ids[b, :len(r)] = torch.as_tensor(r)
    mel, dec_lens, _, _, _, idx, reps = m.model.engine().infer(ids, alone=True, return_idx=True, return_reps=True)
    tok, _ = token_spans(reps, torch.tensor([len(r) for r in rows]), hop=256)
    tok, idx, dec_lens = tok.cpu().numpy(), idx.cpu().numpy(), dec_lens.cpu().tolist()
    for b, r in enumerate(rows):
        n = len(r)
        assert tok[b, n - 1, 1] == 256 * dec_lens[b] and (tok[b] % 256 == 0).all()
        frames = np.concatenate([np.full((tok[b, i, 1] - tok[b, i, 0]) // 256, i) for i in range(n)])
        assert np.array_equal(frames, idx[b, :dec_lens[b]])


def test_tts_string_with_timestamps(model):
    m, _ = model
    line = _lines(1)[0]
    for kw in (dict(denoise=0), dict(denoise=0.005, normalize='peak'), dict(denoise=0, speed=1.3)):
        wave, timing = m.tts(line, return_timestamps=True, **kw)
        assert torch.equal(wave, m.tts(line, **kw))
        _consistent(timing, wave, line)
    wave, mel, timing = m.tts(line, denoise=0, return_mel=True, return_timestamps=True)
    assert timing['tokens'][-1]['end'] == 256 * mel.shape[-1] == wave.numel()


@pytest.mark.parametrize('batch_size', [1, 2, 8])
def test_tts_list_with_timestamps(model, batch_size):
    """the chunked loop, the padded batches and both pipelines: waves as without the flag, every timing consistent with its own wave"""
    m, _ = model
    lines = _lines(5)
    waves, timings = m.tts(lines, batch_size=batch_size, denoise=0, return_timestamps=True)
    plain = m.tts(lines, batch_size=batch_size, denoise=0)
    assert len(waves) == len(timings) == 5 and all(torch.equal(a, b) for a, b in zip(waves, plain))
    for line, wave, timing in zip(lines, waves, timings):
        _consistent(timing, wave, line)
    # a per-line list: rows as if alone, so timing i is tts_single(line i, its options)'s exactly
    speeds = [1.0, 1.25, 0.8, 1.1, 1.0]
    waves, timings = m.tts(lines, batch_size=batch_size, denoise=0, speed=speeds, return_timestamps=True)
    plain = m.tts(lines, batch_size=batch_size, denoise=0, speed=speeds)
    assert all(torch.equal(a, b) for a, b in zip(waves, plain))
    for line, wave, timing, s in zip(lines, waves, timings, speeds):
        _consistent(timing, wave, line)
        assert timing == m.tts_single(line, speed=s, denoise=0, return_timestamps=True)[1]


def test_tts_requests_with_timestamps(model):
    m, _ = model
    lines = _lines(3)
    reqs = [dict(text=l, speed=s, denoise=0) for l, s in zip(lines, (1.0, 1.2, 0.9))]
    waves, timings = m.tts_requests(reqs, return_timestamps=True)
    assert all(torch.equal(a, b) for a, b in zip(waves, m.tts_requests(reqs)))
    for r, wave, timing in zip(reqs, waves, timings):
        _consistent(timing, wave, r['text'])
        assert timing == m.tts_single(r['text'], speed=r['speed'], denoise=0, return_timestamps=True)[1]
    assert m.tts_requests([], return_timestamps=True) == ([], [])


def test_griffin_lim_vocoder_has_the_same_hop(model):
    from models.fastpitch import FastPitch2Wave
    m, d = model
    gl = FastPitch2Wave(str(d / 'fp.pth'), vocoder='griffin_lim').to(m.device)
    line = _lines(1)[0]
    wave, timing = gl.tts(line, return_timestamps=True)
    _consistent(timing, wave, line)
    assert timing == m.tts(line, denoise=0, return_timestamps=True)[1]


@pytest.fixture(scope='module')
def paragraph():
    a, b, c, d, e, f6 = (_corpus()[i] for i in (9, 14, 92, 63, 35, 68))
    return f'{a}. {b}، {c}\n{d}. {e}؟ {f6}'


def test_tts_long_with_timestamps(model, paragraph):
    from text import spoken_text
    m, _ = model
    out, rows, timing = m.tts_long(paragraph, denoise=0, return_segments=True, return_timestamps=True)
    plain, plain_rows = m.tts_long(paragraph, denoise=0, return_segments=True)
    assert torch.equal(out, plain) and rows == plain_rows
    out_t, timing_t = m.tts_long(paragraph, denoise=0, return_timestamps=True)
    assert torch.equal(out_t, out) and timing_t == timing
    words = timing['words']
    assert [w['segment'] for w in words] == sorted(w['segment'] for w in words) and {w['segment'] for w in words} == set(range(len(rows)))
    flat = [v for w in words for v in (w['start'], w['end'])]
    assert flat == sorted(flat)                                                                 # monotone across the paragraph
    F = 110
    for k, r in enumerate(rows):
        mine = [w for w in words if w['segment'] == k]
        own, own_t = m.tts(spoken_text(r['text']), denoise=0, return_timestamps=True)
        assert [w['word'] for w in mine] == [w['word'] for w in own_t['words']]
        for w, o in zip(mine, own_t['words']):
            assert r['start'] <= w['start'] <= w['end'] <= r['end']
            # the segment's own mark, clamped to what the trim kept and moved to its place
            assert w['start'] == r['start'] + min(max(o['start'], r['src_start']), r['src_end']) - r['src_start']
            assert w['end'] == r['start'] + min(max(o['end'], r['src_start']), r['src_end']) - r['src_start']
            s, e = max(w['start'], r['start'] + F), min(w['end'], r['end'] - F)                 # away from the fades
            if e > s:
                err = float((out[s:e] - own[s - r['start'] + r['src_start']:e - r['start'] + r['src_start']]).abs().max())
                assert err < WAVE_TOL, (k, w['word'], err)
    for k in range(len(rows) - 1):                                                              # every pause lies between two segments' words
        last = [w for w in words if w['segment'] == k][-1]
        first = [w for w in words if w['segment'] == k + 1][0]
        assert last['end'] <= rows[k]['end'] <= rows[k + 1]['start'] <= first['start']
    # the grouping does not matter
    _, timing2 = m.tts_long(paragraph, denoise=0, batch_size=2, return_timestamps=True)
    assert timing2 == timing


@pytest.mark.parametrize('delivery', [dict(), dict(sample_rate=8000, encoding='mulaw')])
def test_tts_stream_marks(model, delivery):
    from ttsamd.timing import delivered_timing
    m, _ = model
    line = _lines(1)[0]
    kw = dict(chunk_frames=16, first_chunk_frames=8, denoise=0, **delivery)
    plain = list(m.tts_stream(line, **kw))
    got = list(m.tts_stream(line, marks=True, **kw))
    assert len(got) == len(plain) and all(torch.equal(c, p) for (c, _), p in zip(got, plain))
    want = delivered_timing(m.tts(line, denoise=0, return_timestamps=True)[1], delivery.get('sample_rate'))
    if delivery:
        ref = m.tts(line, denoise=0, return_timestamps=True)[1]
        assert [w['start'] for w in want['words']] == [-(-160 * w['start'] // 441) for w in ref['words']] and want['sample_rate'] == 8000
    assert [w for _, marks in got for w in marks] == want['words']
    pos = 0
    for k, (chunk, marks) in enumerate(got):
        for w in marks:                                       # with the chunk whose delivered range holds its start (the end: the last)
            assert pos <= w['start'] < pos + chunk.numel() or (k == len(got) - 1 and w['start'] == pos + chunk.numel())
        pos += chunk.numel()


def test_tts_stream_marks_follow_their_line(model):
    m, _ = model
    lines = _lines(3)
    kw = dict(chunk_frames=16, first_chunk_frames=8, denoise=0, max_streams=2)
    plain = list(m.tts_stream(lines, **kw))
    got = list(m.tts_stream(lines, marks=True, **kw))
    assert [(i, last) for i, _, last, _ in got] == [(i, last) for i, _, last in plain]
    assert all(torch.equal(a[1], b[1]) for a, b in zip(got, plain))
    for i, line in enumerate(lines):
        want = m.tts_single(line, denoise=0, return_timestamps=True)[1]['words']
        assert [w for j, _, _, marks in got if j == i for w in marks] == want
    with_meter = list(m.tts_stream(lines[0], marks=True, meter=True, chunk_frames=16, first_chunk_frames=8, denoise=0))
    assert all(len(item) == 3 and 'momentary' in item[1] and isinstance(item[2], list) for item in with_meter)


def test_fastpitch_timestamps_of_a_recording(model):
    """FastPitch.timestamps on a synthesised mel: the token spans' lengths in frames are align's durations"""
    m, _ = model
    lines = _lines(2)
    mels = m.model.ttmel(lines, batch_size=1)
    lens = [int(x.shape[-1]) for x in mels]
    mel = torch.zeros(2, mels[0].shape[0], max(lens), device=m.device)
    for b, x in enumerate(mels):
        mel[b, :, :lens[b]] = x
    timings = m.model.timestamps(lines, mel, torch.tensor(lens))
    dur = m.model.align(lines, mel, torch.tensor(lens)).dur_tgt.cpu().numpy()
    for b, t in enumerate(timings):
        got = [(k['end'] - k['start']) / 256 for k in t['tokens']]
        assert got == dur[b, :len(got)].tolist() and t['tokens'][-1]['end'] == 256 * lens[b]
        assert [w['word'] for w in t['words']] == __import__('text').line_words(lines[b])
    one = m.model.timestamps(lines[0], mel[:1, :, :lens[0]])
    assert one['tokens'][-1]['end'] == 256 * lens[0]


@pytest.mark.parametrize('long', [False, True])
def test_inference_cli_timestamps(model, tmp_path, long):
    """inference.py --timestamps srt: one .srt next to every wave, its last cue ending within a millisecond of the wave's length"""
    import inference
    from scipy.io import wavfile
    _, d = model
    c = _corpus()
    lst = tmp_path / 'lines.txt'
    lst.write_text(f'{c[9]}. {c[14]}\n{c[63]}\n' if long else f'{c[9]}\n{c[63]}\n', encoding='utf-8')
    inference.main(['--list', str(lst), '--model', 'fastpitch', '--checkpoint', str(d / 'fp.pth'), '--vocoder_sd', str(d / 'hg.pth'),
                    '--vocoder_config', str(d / 'config.json'), '--out_dir', str(tmp_path / 'out'), '--timestamps', 'srt']
                   + (['--long'] if long else []))
    for i in range(2):
        sr, data = wavfile.read(tmp_path / 'out' / 'wavs' / f'static{i}.wav')
        srt = (tmp_path / 'out' / 'wavs' / f'static{i}.srt').read_text(encoding='utf-8')
        stamp = srt.strip().split('\n\n')[-1].split('\n')[1].split(' --> ')[1]
        h, mnt, rest = stamp.split(':')
        ms = (int(h) * 60 + int(mnt)) * 60000 + int(rest.replace(',', ''))
        assert abs(ms - data.size * 1000 / sr) <= 1.0, (stamp, data.size)


# ---- Tacotron2 ----
@pytest.fixture(scope='module')
def taco(tmp_path_factory, synth_weights, dev):
    import text
    from models.tacotron2 import Tacotron2Wave
    from ttsamd.config import HIFIGAN_CONFIG, TACOTRON2_CONFIG
    from ttsamd.synth import tacotron2_state_dict
    d = tmp_path_factory.mktemp('ckpt_timing_taco')
    sd = tacotron2_state_dict(dict(TACOTRON2_CONFIG, num_speakers=40), seed=4, gate_bias=-0.5)
    torch.save({'model': {k: torch.from_numpy(np.asarray(v).copy()) for k, v in sd.items()}, 'symbols': list(text.symbols)}, d / 'taco.pth')
    torch.save({'generator': {k: torch.from_numpy(v.copy()) for k, v in synth_weights['hifigan'].items()}}, d / 'hg.pth')
    with open(d / 'config.json', 'w') as f:
        json.dump(HIFIGAN_CONFIG, f)
    m = Tacotron2Wave(str(d / 'taco.pth'), str(d / 'hg.pth'), str(d / 'config.json'), n_symbol=len(text.symbols)).to(dev)
    m.model.decoder_max_step = 40
    m.model.dropout_seed = 5
    return m


TACO_LINES = ['اَلسَّلامُ عَلَيكُم يَا صَدِيقِي', 'كِتَاب']


def test_tacotron2_timestamps(taco):
    import aligner_ref as A
    import text
    m = taco
    for line in TACO_LINES:
        for post in (True, False):
            wave, timing = m.tts(line, denoise=0, postprocess_mel=post, return_timestamps=True)
            assert torch.equal(wave, m.tts(line, denoise=0, postprocess_mel=post))
            toks = timing['tokens']
            assert [w['word'] for w in timing['words']] == text.line_words(line)
            assert all(a['end'] == b['start'] for a, b in zip(toks, toks[1:])) and toks[0]['start'] == 0
            # the durations behind the timing: b_mas on the SAME log-attention tensor, read back
            tokens, cut = m.model._tokens_for(line, None, post)
            ids = torch.LongTensor(text.tokens_to_ids(tokens, m.model.phon_to_id)).unsqueeze(0)
            mel, _, align = m.model.infer(ids, torch.LongTensor([0]))
            dur, log_attn = m.model.attention_durations(align, torch.tensor([len(tokens)]), torch.tensor([align.shape[1]]))
            hard = A.b_mas(log_attn.cpu().numpy()[:, None], np.array([len(tokens)]), np.array([align.shape[1]]))
            assert np.array_equal(dur.cpu().numpy(), hard[:, 0].sum(axis=1))
            c = np.concatenate([[0], np.cumsum(dur.cpu().numpy()[0])]).astype(np.int64) * 256
            n_end = wave.numel() // 256 - 3 if cut else None
            hi = n_end * 256 if cut else c[-1]
            assert [(t['start'], t['end']) for t in toks] == [(min(a, hi), min(b, hi)) for a, b in zip(c[:-1], c[1:])]
            assert toks[-1]['end'] <= wave.numel() and (not cut or toks[-1]['end'] <= n_end * 256)
            # speed: every position is the ceiling rule of the unscaled one at n_t_new / n_t
            fast, t_fast = m.tts(line, denoise=0, postprocess_mel=post, speed=1.25, return_timestamps=True)
            n_t, n_new = wave.numel() // 256, fast.numel() // 256
            assert n_new == int(1 / 1.25 * n_t)
            assert [(t['start'], t['end']) for t in t_fast['tokens']] == [(-(-t['start'] * n_new // n_t), -(-t['end'] * n_new // n_t)) for t in toks]
    waves, timings = m.tts(TACO_LINES, batch_size=2, denoise=0, return_timestamps=True)
    assert all(torch.equal(a, b) for a, b in zip(waves, m.tts(TACO_LINES, batch_size=2, denoise=0)))
    for line, wave, timing in zip(TACO_LINES, waves, timings):
        assert [w['word'] for w in timing['words']] == text.line_words(line) and timing['tokens'][-1]['end'] <= wave.numel()
    with pytest.raises(ValueError):
        next(m.tts_stream(TACO_LINES[0], marks=True))


def test_tacotron2_attention_with_exact_zeros(taco, dev):
    """an alignment with exact zeros goes through the clamp, the log and the search: no NaN, no -inf, durations that add up"""
    import aligner_ref as A
    align = torch.zeros(1, 12, 5, device=dev)
    align[0, torch.arange(12), torch.arange(12) * 5 // 12] = 1.0
    dur, log_attn = taco.model.attention_durations(align, torch.tensor([5]), torch.tensor([12]))
    assert bool(torch.isfinite(log_attn).all()) and bool(torch.isfinite(dur).all()) and float(dur.sum()) == 12.0
    assert dur[0].tolist() == np.bincount(np.arange(12) * 5 // 12, minlength=5).tolist()
    hard = A.b_mas(log_attn.cpu().numpy()[:, None], np.array([5]), np.array([12]))
    assert np.array_equal(dur.cpu().numpy(), hard[:, 0].sum(axis=1))


@pytest.mark.parametrize('speed', [None, 1.25, 0.8])
def test_tacotron2_tts_long_with_timestamps(taco, speed):
    """marks in the JOINED wave: each segment's own marks (tts of the same padded batch, with the same cut and speed), clamped to what the
    trim kept and moved -- exactly, also where a speed puts a ratio between the two clamps (two launches)"""
    import text
    from text import spoken_text
    m = taco
    para = '. '.join(TACO_LINES)
    out, rows, timing = m.tts_long(para, denoise=0, speed=speed, return_segments=True, return_timestamps=True)
    plain, plain_rows = m.tts_long(para, denoise=0, speed=speed, return_segments=True)
    assert torch.equal(out, plain) and rows == plain_rows and len(rows) == 2
    lines = [spoken_text(r['text']) for r in rows]
    _, own = m.tts(lines, batch_size=32, denoise=0, speed=speed, return_timestamps=True)   # the same padded batch as tts_long's group
    words = timing['words']
    flat = [v for w in words for v in (w['start'], w['end'])]
    assert flat == sorted(flat) and [w['segment'] for w in words] == [0] * len(text.line_words(lines[0])) + [1] * len(text.line_words(lines[1]))
    place = lambda v, r: r['start'] + min(max(v, r['src_start']), r['src_end']) - r['src_start']   # noqa: E731
    for k, r in enumerate(rows):
        mine = [w for w in words if w['segment'] == k]
        assert [w['word'] for w in mine] == [w['word'] for w in own[k]['words']]
        for w, o in zip(mine, own[k]['words']):
            assert r['start'] <= w['start'] <= w['end'] <= r['end']
            assert (w['start'], w['end']) == (place(o['start'], r), place(o['end'], r))
    n0 = len(own[0]['tokens'])
    for k, r in enumerate(rows):
        mine = timing['tokens'][:n0] if k == 0 else timing['tokens'][n0:]
        assert [(t['start'], t['end']) for t in mine] == [(place(t['start'], r), place(t['end'], r)) for t in own[k]['tokens']]


ODD_LINES = ['qaAla 12', 'qaAla marHabAF ;', 'qaAla marHabAF - 5', ' qaAla  marHabAF (', 'qaAla 7 marHabAF \u061f']


def test_a_timing_request_never_turns_a_call_into_an_error(model):
    """text with digits, brackets, free-standing marks the inventory lacks, double and leading spaces: whatever `tts` synthesises without
    the flag it synthesises with it, every timing consistent with its wave"""
    import text
    m, _ = model
    waves, timings = m.tts(ODD_LINES, batch_size=2, denoise=0, return_timestamps=True)
    assert all(torch.equal(a, b) for a, b in zip(waves, m.tts(ODD_LINES, batch_size=2, denoise=0)))
    for line, wave, timing in zip(ODD_LINES, waves, timings):
        _consistent(timing, wave, line)
    assert [w['word'] for w in timings[4]['words']] == ['qaAla', '7', 'marHabAF'] and timings[4]['words'][1]['start'] == timings[4]['words'][1]['end']
    wave, timing = m.tts_requests([dict(text=ODD_LINES[3], denoise=0)], return_timestamps=True)
    _consistent(timing[0], wave[0], ODD_LINES[3])
    got = list(m.tts_stream(ODD_LINES[:3], chunk_frames=16, first_chunk_frames=8, denoise=0, marks=True))
    for i, line in enumerate(ODD_LINES[:3]):
        assert [w['word'] for j, _, _, marks in got if j == i for w in marks] == text.line_words(line)
    # and should a caller's words not pair up with the token groups, the groups are named by their tokens instead of raising
    from ttsamd.timing import PendingTimings
    tokens = text.buckwalter_to_tokens('qaAla marHabAF', append_space=False)
    reps = torch.ones(1, len(tokens), dtype=torch.int64, device=m.device)
    t = PendingTimings([tokens], [['only one']], reps, 256, 22050).resolve()[0]
    assert [w['word'] for w in t['words']] == ['q aa l a', 'm a r H a b a n'] and t['tokens'][-1]['end'] == 256 * len(tokens)


class _Copies:
    """counts the device -> host reads of a block: .cpu(), .tolist() and .item() of tensors on the device"""

    def __enter__(self):
        self.n, self.saved = 0, {k: getattr(torch.Tensor, k) for k in ('cpu', 'tolist', 'item')}
        for name, fn in self.saved.items():
            def wrapped(t, *a, _fn=fn, **kw):
                self.n += t.device.type == 'cuda'
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, name, wrapped)
        return self

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(torch.Tensor, name, fn)


def test_timestamps_cost_one_copy_per_model_call(model, paragraph):
    """with the flag on: one more device -> host copy per FastPitch call, none per chunk of a stream"""
    m, _ = model
    lines = _lines(4)

    def copies(fn):
        with _Copies() as c:
            fn()
        return c.n
    for on, off in ((lambda: m.tts(lines[0], denoise=0, return_timestamps=True), lambda: m.tts(lines[0], denoise=0)),
                    (lambda: m.tts_batch(lines, denoise=0, return_timestamps=True), lambda: m.tts_batch(lines, denoise=0)),
                    (lambda: m.tts_long(paragraph, denoise=0, return_timestamps=True), lambda: m.tts_long(paragraph, denoise=0)),
                    (lambda: list(m.tts_stream(lines[0], chunk_frames=8, first_chunk_frames=8, denoise=0, marks=True)),
                     lambda: list(m.tts_stream(lines[0], chunk_frames=8, first_chunk_frames=8, denoise=0))),
                    (lambda: list(m.tts_stream(lines, chunk_frames=8, first_chunk_frames=8, denoise=0, marks=True)),
                     lambda: list(m.tts_stream(lines, chunk_frames=8, first_chunk_frames=8, denoise=0)))):
        assert copies(on) == copies(off) + 1
    # two FastPitch calls (batch_size 2 over four lines, the pipelined list path): two more copies
    assert copies(lambda: m.tts(lines, batch_size=2, denoise=0, return_timestamps=True)) == copies(lambda: m.tts(lines, batch_size=2, denoise=0)) + 2
