"""Token and word timestamps (csrc/timing.hip; include/ttsamd.h: ttsamd_token_spans states the arithmetic): per-token repeat counts
(FastPitch's reps, the MAS durations of an attention map) -> where every token and every word lies in the audio that is delivered.  The
spans are made on the device, beside the counts and the trim / join table they read, and come to the host in ONE small copy after the
audio's own; a synthesis call gains no synchronisation point.

A timing is a plain dict, one per line: sample_rate; words: dicts of word, start, end (samples of the returned wave), t0, t1 (the same
in seconds), tokens = (i0, i1) (the word's half-open token range); tokens: dicts of token, start, end."""
import numpy as np
import torch

from . import lib as L
from .engine import _ptr, _require_gpu, _stream

MAX_TOKENS, MAX_RATIO = 8192, 1 << 20


def _dev_int(t, dtype, shape, dev, what):
    """an integer input on the device, of that dtype and shape (None in a place of `shape`: any size); None stays None"""
    if t is None:
        return None
    t = torch.as_tensor(t).to(device=dev, dtype=dtype).contiguous()
    if t.dim() != len(shape) or any(s is not None and s != g for s, g in zip(shape, t.shape)):
        raise L.TtsAmdError(f'token_spans: {what} of shape {tuple(t.shape)}, expected {tuple("*" if s is None else s for s in shape)}')
    return t


def _spans(reps, n_tokens, groups, n_groups, hop, maps):
    """token_spans' launch -> (flat, tok, grp): tok and grp are views of `flat`, one int64 buffer, so that both ride one copy"""
    lib = _require_gpu()
    if not isinstance(reps, torch.Tensor) or reps.device.type != 'cuda' or reps.dim() != 2:
        raise L.TtsAmdError('token_spans: reps: expected a [B, L] tensor on the ROCm device (there is no CPU fallback)')
    dev = reps.device
    reps = reps.to(torch.int64)
    if reps.stride(1) != 1 or reps.stride(0) < reps.shape[1]:
        reps = reps.contiguous()
    B, Lt = reps.shape
    hop = int(hop)
    if not (B >= 1 and 1 <= Lt <= MAX_TOKENS):
        raise L.TtsAmdError(f'token_spans: reps of shape {(B, Lt)}: at least one row, 1 .. {MAX_TOKENS} tokens per row')
    if hop < 1:
        raise ValueError(f'token_spans: hop {hop} must be at least 1')
    n_tokens = _dev_int(n_tokens, torch.int64, (B,), dev, 'n_tokens')
    groups = _dev_int(groups, torch.int32, (B, None, 2), dev, 'groups')
    G = 0 if groups is None else int(groups.shape[1])
    if n_groups is not None and groups is None:
        raise L.TtsAmdError('token_spans: n_groups without groups')
    n_groups = _dev_int(n_groups, torch.int32, (B,), dev, 'n_groups')
    maps = _dev_int(maps, torch.int64, (B, 5), dev, 'maps')
    flat = torch.empty(2 * B * (Lt + G), dtype=torch.int64, device=dev)
    tok = flat[:2 * B * Lt].view(B, Lt, 2)
    grp = flat[2 * B * Lt:].view(B, G, 2) if G else None
    with torch.cuda.device(dev):
        L.check(lib.ttsamd_token_spans(_ptr(reps), reps.stride(0), _ptr(n_tokens), B, Lt, _ptr(groups if G else None),
                                       _ptr(n_groups if G else None), G, hop, _ptr(maps), _ptr(tok), _ptr(grp), _stream()), 'token_spans')
    return flat, tok, grp


def token_spans(reps, n_tokens=None, groups=None, n_groups=None, hop=256, maps=None):
    """reps int64 [B, L] on the device (repeat counts per token; a row may be a strided view), n_tokens int64 [B] (None: L each), groups
    int32 [B, G, 2] (half-open token ranges, e.g. text.word_ranges) + n_groups int32 [B] (None: G each), hop samples per repeat, maps
    int64 [B, 5] = (lo, hi, off, num, den) per row (None: the identity) -> (tok int64 [B, L, 2], grp int64 [B, G, 2] or None) on the
    device: (start, end) of every token and group, m(c[i]) with c the prefix sums of max(reps, 0) and
    m(p) = off + ceil((clamp(p hop, lo, hi) - lo) num / den).  One launch, nothing read back."""
    _, tok, grp = _spans(reps, n_tokens, groups, n_groups, hop, maps)
    return tok, grp


def pack_groups(ranges):
    """a list of rows of (t0, t1) ranges (text.word_ranges per line) -> (groups int32 [B, G, 2], n_groups int32 [B]) on the host, G at
    least 1, rows padded with (0, 0)"""
    G = max(1, max((len(r) for r in ranges), default=0))
    groups = np.zeros((len(ranges), G, 2), dtype=np.int32)
    for b, r in enumerate(ranges):
        if len(r):
            groups[b, :len(r)] = np.asarray(r, dtype=np.int32).reshape(-1, 2)
    return torch.from_numpy(groups), torch.tensor([len(r) for r in ranges], dtype=torch.int32)


def make_timing(tokens, words, ranges, tok, grp, sample_rate, segment=None):
    """one line's timing dict from its token strings, its words (text.line_words), their token ranges (text.word_ranges) and the host
    rows tok [>= n, 2], grp [>= len(words), 2] of token_spans; segment: the index tts_long's words carry"""
    sr = float(sample_rate)
    rows = []
    for k, (word, (i0, i1)) in enumerate(zip(words, ranges)):
        s, e = int(grp[k][0]), int(grp[k][1])
        row = dict(word=word, start=s, end=e, t0=s / sr, t1=e / sr, tokens=(int(i0), int(i1)))
        if segment is not None:
            row['segment'] = segment
        rows.append(row)
    return dict(sample_rate=int(sample_rate), words=rows,
                tokens=[dict(token=t, start=int(tok[i][0]), end=int(tok[i][1])) for i, t in enumerate(tokens)])


class PendingTimings:
    """The spans of the rows of one model call, launched and still on the device.  resolve() is the one copy to the host (call it behind
    the audio's own copy, so that the launch order of the synthesis is what it was) -> one timing dict per row, in the row order given."""

    def __init__(self, token_rows, word_rows, reps, hop, sample_rate, row_maps=None, launch=True):
        """row_maps int64 [B, 5] on the device: the map of each row into its OWN wave (Tacotron2: the cut of truncate_mel and the ratio of
        resize_mel; position 0 stays 0: lo = off = 0), None: the identity.  launch=False: held back until launch(maps) (tts_long: the join table is not there yet)."""
        import text
        self.token_rows = [list(t) for t in token_rows]
        self.ranges = [text.word_ranges(t) for t in self.token_rows]
        # a request for timestamps never turns a call that synthesises into one that raises: should a line's words ever not pair up
        # with its token groups, the groups are named by their tokens
        self.word_rows = [list(w) if len(w) == len(r) else [' '.join(t[t0:t1]) for t0, t1 in r]
                          for w, r, t in zip(word_rows, self.ranges, self.token_rows)]
        assert reps.shape[0] == len(self.token_rows), (reps.shape, len(self.token_rows))
        self.reps, self.hop, self.sample_rate, self.row_maps, self.segments = reps, hop, sample_rate, row_maps, None
        self.flat = self._done = None
        if launch:
            self.launch()

    def launch(self, maps=None, segments=None):
        """the launch, on the current stream; maps int64 [B, 5] on the device: where each row's wave goes from there (tts_long: the trim /
        join table, ttsamd.join.span_maps), segments: what the words of each row carry as `segment`.  With row_maps AND maps there are
        two launches, because two clamps with a ratio between them are not one map: the first puts every token into its row's wave;
        the lengths of those spans, at one sample a repeat, are the counts of the second, whose prefix sums are then exactly the
        first's positions."""
        groups, n_groups = pack_groups(self.ranges)
        n_tokens = torch.tensor([len(t) for t in self.token_rows], dtype=torch.int64)
        reps, hop = self.reps, self.hop
        if self.row_maps is not None and maps is not None:
            _, tok, _ = _spans(reps, n_tokens, None, None, hop, self.row_maps)
            reps, hop = (tok[:, :, 1] - tok[:, :, 0]).contiguous(), 1
        elif maps is None:
            maps = self.row_maps
        self.flat, self.tok, self.grp = _spans(reps, n_tokens, groups, n_groups, hop, maps)
        self.reps, self.segments = None, segments

    def resolve(self):
        if self._done is None:
            if self.flat is None:
                self.launch()
            B, Lt, G = self.tok.shape[0], self.tok.shape[1], self.grp.shape[1]
            host = self.flat.cpu().numpy()                             # the one copy
            tok, grp = host[:2 * B * Lt].reshape(B, Lt, 2), host[2 * B * Lt:].reshape(B, G, 2)
            self._done = [make_timing(self.token_rows[b], self.word_rows[b], self.ranges[b], tok[b], grp[b], self.sample_rate,
                                      None if self.segments is None else self.segments[b]) for b in range(B)]
            self.flat = self.tok = self.grp = None
        return self._done


def map_timing(timing, num, den, sample_rate):
    """a timing at another rate: every position s becomes ceil(num s / den) (the first sample of the new rate at or after the instant:
    the rule of the stream's chunk borders), seconds by the new sample_rate"""
    num, den, sr = int(num), int(den), float(sample_rate)

    def m(s):
        return -((-num * int(s)) // den)
    words = []
    for w in timing['words']:
        s, e = m(w['start']), m(w['end'])
        words.append(dict(w, start=s, end=e, t0=s / sr, t1=e / sr))
    return dict(sample_rate=int(sample_rate), words=words, tokens=[dict(t, start=m(t['start']), end=m(t['end'])) for t in timing['tokens']])


class MarkFeeder:
    """The word marks of one line of a stream, handed out with the chunks: take(n, last) -> the words whose start lies in the next n
    delivered samples (on the last chunk: all that are left, so a mark at the very end goes with it).  Host only: nothing runs per chunk
    on the device."""

    def __init__(self, timing):
        self.words, self.pos, self.k = timing['words'], 0, 0          # starts never decrease: one pointer

    def take(self, n, last=False):
        self.pos += int(n)
        k0 = self.k
        while self.k < len(self.words) and (last or self.words[self.k]['start'] < self.pos):
            self.k += 1
        return self.words[k0:self.k]


def delivered_timing(timing, sample_rate, source_rate=22050):
    """a timing of the vocoder's wave at the rate a stream delivers (None or the source rate: as it is): map_timing with num / den = the
    resampler's n / o, the two rates over their greatest common divisor"""
    from math import gcd
    if sample_rate is None or int(sample_rate) == int(source_rate):
        return timing
    g = gcd(int(sample_rate), int(source_rate))
    return map_timing(timing, int(sample_rate) // g, int(source_rate) // g, int(sample_rate))


def merge_timings(timings):
    """the timings of the segments of a paragraph (positions already in the joined wave) -> one timing"""
    return dict(sample_rate=timings[0]['sample_rate'] if timings else 22050, words=[w for t in timings for w in t['words']],
                tokens=[k for t in timings for k in t['tokens']])
