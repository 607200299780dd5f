"""CPU: the host side of the timestamps -- which tokens make which word (text.word_ranges / line_words), the numpy statement of
ttsamd_token_spans (tests/timing_ref.py) and its properties, the subtitle writers of utils.timing, and the exported symbol."""
import json
import os

import numpy as np
import pytest

import timing_ref as R
from conftest import GOLDEN


def _lines():
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        return json.load(f)


def test_word_ranges_count_the_words_of_every_corpus_line():
    import text
    lines = _lines()
    assert len(lines) == 100
    for line in lines:
        for append_space in (False, True):
            tokens = text.buckwalter_to_tokens(line, append_space=append_space)
            ranges = text.word_ranges(tokens)
            assert len(ranges) == len(line.split()) == len(text.line_words(line)), line
            # disjoint, increasing, and what they skip is exactly the separators and the EOS
            covered = [i for t0, t1 in ranges for i in range(t0, t1)]
            assert covered == sorted(set(covered)) and all(a[1] < b[0] or a[1] == b[0] - 1 for a, b in zip(ranges, ranges[1:]))
            skipped = [tokens[i] for i in range(len(tokens)) if i not in set(covered)]
            assert set(skipped) <= {text.SEPARATOR_TOKEN, text.EOS_TOKEN} and skipped.count(text.EOS_TOKEN) == 1
            assert not any(tokens[i] in (text.SEPARATOR_TOKEN, text.EOS_TOKEN) for i in covered)


@pytest.mark.parametrize('line, sizes, words', [
    ('qaAla - marHabAF', [4, 0, 8], ['qaAla', '-', 'marHabAF']),
    ('qaAla , marHabAF', [5, 8], ['qaAla ,', 'marHabAF']),
    ('qaAla , marHabAF ?', [5, 9], ['qaAla ,', 'marHabAF ?']),
    ('qaAla, marHabAF?', [5, 9], ['qaAla,', 'marHabAF?']),
    ('qaAla sil marHabAF -', [4, 0, 8], ['qaAla', 'sil', 'marHabAF']),
])
def test_word_ranges_hand_cases(line, sizes, words):
    import text
    for append_space in (False, True):
        tokens = text.buckwalter_to_tokens(line, append_space=append_space)
        assert [t1 - t0 for t0, t1 in text.word_ranges(tokens)] == sizes
    assert text.line_words(line) == words


@pytest.mark.parametrize('line, sizes, words', [
    ('qaAla 12', [4], ['qaAla']),                                        # a trailing piece without phones goes with the separators
    ('qaAla ;', [4], ['qaAla']),
    ('qaAla marHabAF (', [4, 8], ['qaAla', 'marHabAF']),
    ('qaAla marHabAF \u061f', [4, 8], ['qaAla', 'marHabAF']),
    ('qaAla marHabAF - 5', [4, 8], ['qaAla', 'marHabAF']),
    ('qaAla 12 marHabAF', [4, 0, 8], ['qaAla', '12', 'marHabAF']),        # ... in the middle it is a word without tokens
    ('qaAla ... marHabAF', [5, 0, 8], ['qaAla .', '..', 'marHabAF']),    # the tokeniser cuts one mark off: '.' joins, '..' is a piece
    (' qaAla  marHabAF ', [0, 4, 0, 8], ['', 'qaAla', '', 'marHabAF']),  # leading and double spaces are empty pieces
    ('. qaAla', [1, 4], ['.', 'qaAla']),                                 # a mark with nothing in front of it opens a word
    ('a.b', [1, 1], ['a', '.b']),                                        # a mark inside a piece cuts it
])
def test_line_words_follow_the_tokeniser(line, sizes, words):
    import text
    for to_tokens, arabic_in in ((text.arabic_to_tokens, True), (text.buckwalter_to_tokens, False)):
        for append_space in (False, True):
            tokens = to_tokens(line, append_space=append_space)
            assert [t1 - t0 for t0, t1 in text.word_ranges(tokens)] == sizes
        assert text.line_words(line, arabic_in) == words


def test_line_words_arabic_script():
    import text
    line = '\u0645\u064e\u0631\u0652\u062d\u064e\u0628\u0627\u064b \u060c \u0643\u064e\u064a\u0652\u0641\u064e \u062d\u064e\u0627\u0644\u064f\u0643\u064e \u061f'
    words = text.line_words(line)
    assert words == line.split(' ')[:4]                                  # the Arabic comma is a piece without phones, the closing mark is dropped
    sizes = [t1 - t0 for t0, t1 in text.word_ranges(text.arabic_to_tokens(line, append_space=False))]
    assert len(sizes) == 4 and sizes[1] == 0 and all(sizes[k] > 0 for k in (0, 2, 3))


def test_line_words_pair_with_word_ranges_on_any_text():
    """20 000 seeded random lines over letters, diacritics, marks, digits, brackets, `-`, `sil`, spaces and Arabic script, through both
    tokenisers: a timing request must never meet a line whose words and token groups do not pair up"""
    import random
    import text
    rng = random.Random(0)
    alphabet = list("qaAlmrHbFNKuio~>'<|Ypwy*$ -.,?!;(1") + ['sil', ' ', ' ', '\u0640', '\u0628', '\u064e', '\u060c', '\u061f', '\u0627']
    for _ in range(20000):
        line = ''.join(rng.choice(alphabet) for _ in range(rng.randint(0, 14)))
        for to_tokens, arabic_in in ((text.arabic_to_tokens, True), (text.buckwalter_to_tokens, False)):
            append_space = bool(rng.getrandbits(1))
            tokens = to_tokens(line, append_space=append_space)
            assert len(text.word_ranges(tokens)) == len(text.line_words(line, arabic_in)), repr(line)
            # the one-pass form a timing request tokenises with: the tokeniser's tokens, the same words
            assert text.tokens_and_words(line, arabic_in, append_space) == (tokens, text.line_words(line, arabic_in)), repr(line)
    for line in _lines():
        assert text.tokens_and_words(line, True, False)[0] == text.arabic_to_tokens(line, append_space=False)


def test_mark_feeder_hands_every_mark_to_the_chunk_that_holds_it():
    """ttsamd.timing.delivered_timing + MarkFeeder against ttsamd.stream.chunk_outputs: with the chunk sizes a stream at 8 kHz delivers,
    every word goes out once, in order, with the chunk whose range holds its start; one at the very end with the last chunk"""
    from ttsamd.stream import chunk_outputs
    from ttsamd.timing import MarkFeeder, delivered_timing
    total = 200 * 256
    starts = [0, 1, 8 * 256 - 1, 8 * 256, 8 * 256 + 1, 24 * 256, 24 * 256, 30000, total - 1, total]
    timing = dict(sample_rate=22050, words=[dict(word=str(k), start=s, end=min(s + 5, total), t0=s / 22050, t1=min(s + 5, total) / 22050,
                                                 tokens=(k, k + 1)) for k, s in enumerate(starts)], tokens=[dict(token='x', start=0, end=total)])
    assert delivered_timing(timing, None) is timing and delivered_timing(timing, 22050) is timing
    there = delivered_timing(timing, 8000)
    assert there['sample_rate'] == 8000 and [w['start'] for w in there['words']] == [chunk_outputs(s, s, 441, 160)[0] for s in starts]
    assert there['tokens'][0]['end'] == chunk_outputs(0, total, 441, 160)[1]
    cores = [(0, 8 * 256)] + [(8 * 256 + 16 * 256 * k, 8 * 256 + 16 * 256 * (k + 1)) for k in range(12)]
    ranges = [chunk_outputs(a, b, 441, 160) for a, b in cores]
    feed, got = MarkFeeder(there), []
    for k, (k0, k1) in enumerate(ranges):
        marks = feed.take(k1 - k0, last=k == len(ranges) - 1)
        assert all(k0 <= w['start'] < k1 or (k == len(ranges) - 1 and w['start'] == k1) for w in marks)
        got += marks
    assert got == there['words']


def test_word_ranges_leave_out_what_a_wrapper_appends():
    """Tacotron2's token list: the separator of append_space, an inserted separator in front of it, the EOS run"""
    import text
    tokens = text.buckwalter_to_tokens('qaAla marHabAF', append_space=True)
    want = text.word_ranges(text.buckwalter_to_tokens('qaAla marHabAF', append_space=False))
    assert text.word_ranges(tokens) == want == [(0, 4), (5, 13)]
    tokens.insert(-2, text.SEPARATOR_TOKEN)
    assert text.word_ranges(tokens) == want
    assert text.word_ranges([text.EOS_TOKEN]) == [] and text.word_ranges([]) == [] and text.line_words('') == []


def _case(seed=0, B=3, L=40):
    rng = np.random.default_rng(seed)
    reps = rng.integers(0, 20, size=(B, L))
    reps[:, 3] = -4
    reps[:, 10:13] = 0
    return reps, [L, 0, L - 7]


def test_ref_spans_partition_and_are_monotone():
    reps, ns = _case()
    for maps in (None, [(300, 40000, 17, 160, 441)] * 3, [(0, R.INT64_MAX, 0, 37, 40)] * 3, [(5000, 5000, 9, 1, 1)] * 3):
        tok, _ = R.token_spans(reps, ns, hop=256, maps=maps)
        for b, n in enumerate(ns):
            m = (0, R.INT64_MAX, 0, 1, 1) if maps is None else maps[b]
            c_end = int(np.maximum(reps[b, :n], 0).sum())
            flat = tok[b].reshape(-1)
            assert (np.diff(flat) >= 0).all()                                          # monotone
            assert (tok[b, 1:, 0] == tok[b, :-1, 1]).all()                             # each span starts where the last one ended
            assert tok[b, 0, 0] == R.span_pos(0, 256, m) and tok[b, -1, 1] == R.span_pos(c_end, 256, m)
            assert (tok[b, n:] == R.span_pos(c_end, 256, m)).all()


def test_ref_identity_map_is_the_prefix_sum_times_hop():
    reps, ns = _case(1)
    tok, grp = R.token_spans(reps, None, groups=[[(0, 5), (5, 5), (7, 99)]] * 3, hop=200)
    c = np.concatenate([np.zeros((3, 1), dtype=np.int64), np.cumsum(np.maximum(reps, 0), axis=1)], axis=1) * 200
    assert np.array_equal(tok[:, :, 0], c[:, :-1]) and np.array_equal(tok[:, :, 1], c[:, 1:])
    assert np.array_equal(grp[:, 0], np.stack([c[:, 0], c[:, 5]], 1)) and np.array_equal(grp[:, 1], np.stack([c[:, 5], c[:, 5]], 1))
    assert np.array_equal(grp[:, 2], np.stack([c[:, 7], c[:, -1]], 1))                  # t1 clamped to n


def test_ref_bad_rows_are_minus_one():
    reps, ns = _case(2)
    maps = [(0, 100, 0, 1, 0), (0, 100, 0, 1, 1), (9, 8, 0, 1, 1)]
    tok, grp = R.token_spans(reps, ns, groups=[[(0, 2)]] * 3, maps=maps)
    assert (tok[0] == -1).all() and (grp[0] == -1).all() and (tok[2] == -1).all() and (tok[1] >= 0).all()


@pytest.mark.parametrize('rate', [8000, 16000, 24000, 48000])
def test_ceiling_rule_is_chunk_outputs_rule(rate):
    """m(p) with num / den = n / o is ttsamd.stream.chunk_outputs on the same instant; over chunk cores that partition the samples, the
    chunk whose [K0, K1) holds ceil(n S / o) is unique for every S in a window"""
    from math import gcd
    from ttsamd.stream import chunk_outputs
    g = gcd(22050, rate)
    o, n = 22050 // g, rate // g
    cores = [(0, 32 * 256)] + [(32 * 256 + k * 64 * 256, 32 * 256 + (k + 1) * 64 * 256) for k in range(3)]
    ranges = [chunk_outputs(a, b, o, n) for a, b in cores]
    assert all(r[1] == q[0] for r, q in zip(ranges, ranges[1:]))
    for S in list(range(0, 3000)) + list(range(32 * 256 - 600, 32 * 256 + 600)) + list(range(cores[-1][1] - 1200, cores[-1][1])):
        pos = R.span_pos(S, 1, (0, R.INT64_MAX, 0, n, o))
        assert pos == chunk_outputs(S, S, o, n)[0]
        # exactly one chunk; an instant in the last fraction of an output sample maps to the very end (it goes with the last chunk)
        assert sum(k0 <= pos < k1 for k0, k1 in ranges) == (0 if pos == ranges[-1][1] else 1), (S, pos)


TIMING = dict(sample_rate=22050, words=[
    dict(word='wa*alika', start=0, end=11025, t0=0.0, t1=0.5, tokens=(0, 8)),
    dict(word='-', start=11025, end=11025, t0=0.5, t1=0.5, tokens=(9, 9)),
    dict(word='biHuDuwri', start=12000, end=22049, t0=12000 / 22050, t1=22049 / 22050, tokens=(10, 19)),
    dict(word='ra}yisi ,', start=22049, end=33075, t0=22049 / 22050, t1=1.5, tokens=(20, 28)),
    dict(word='lhay}api', start=44100, end=55125, t0=2.0, t1=2.5, tokens=(29, 37)),
    dict(word='l>aqal~i', start=55125, end=81144000, t0=2.5, t1=3680.0, tokens=(38, 46)),
], tokens=[dict(token='_eos_', start=81144000, end=81145261)])


def test_srt_and_vtt_exact_text():
    from utils.timing import to_json, to_srt, to_vtt
    # default: one break at the 0.5 s gap in front of lhay}api; 22049 samples floor to 999 ms; the last cue runs to the last token's end
    assert to_srt(TIMING) == ('1\n00:00:00,000 --> 00:00:01,500\nwa*alika biHuDuwri ra}yisi ,\n\n'
                              '2\n00:00:02,000 --> 01:01:20,057\nlhay}api l>aqal~i\n\n')
    # max_chars 18: 'wa*alika biHuDuwri' is exactly 18 and stays one cue; the next word opens a new one
    assert to_vtt(TIMING, max_chars=18, max_gap=10.0) == ('WEBVTT\n\n00:00:00.000 --> 00:00:00.999\nwa*alika biHuDuwri\n\n'
                                                          '00:00:00.999 --> 00:00:02.500\nra}yisi , lhay}api\n\n'
                                                          '00:00:02.500 --> 01:01:20.057\nl>aqal~i\n\n')
    assert json.loads(to_json(TIMING))['words'][1]['tokens'] == [9, 9]
    assert to_srt(dict(sample_rate=22050, words=[], tokens=[])) == '' and to_vtt(dict(sample_rate=22050, words=[], tokens=[])) == 'WEBVTT\n\n'


def test_map_timing_is_the_ceiling_rule():
    from ttsamd.timing import map_timing
    t = map_timing(TIMING, 160, 441, 8000)
    assert t['sample_rate'] == 8000 and [w['start'] for w in t['words']][:4] == [0, 4000, -(-160 * 12000 // 441), -(-160 * 22049 // 441)]
    assert t['words'][3]['t1'] == t['words'][3]['end'] / 8000 and t['tokens'][0]['end'] == -(-160 * 81145261 // 441)


def test_library_exports_token_spans():
    from ttsamd import lib
    assert 'ttsamd_token_spans' in lib.SYMBOLS and getattr(lib.load(), 'ttsamd_token_spans') is not None
    assert lib.load().ttsamd_version() == 8
