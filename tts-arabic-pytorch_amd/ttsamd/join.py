"""Paragraph join on the device (csrc/join.hip; include/ttsamd.h: ttsamd_wave_join states the arithmetic): the rows of a ragged batch of
waves -> ONE row with trimmed seams, exact pauses, faded edges and overlap-added seams where a gap is negative.  What `tts_long` of
the two models and `utils.audio.join_waves` run between the vocoder and the single copy to the host."""
import numpy as np
import torch

from . import lib as L
from .engine import _dev_f32, _dev_lens, _ptr, _require_gpu, _stream, row_values

MAX_ROWS, MAX_FADE = 4096, 4096
# pause behind a segment by the kind of boundary that ended it, in ms: choices, not measurements ('forced': None = -fade_ms, an
# overlap-added seam -- a cut in the middle of a phrase gets no silence)
DEFAULT_PAUSES = {'paragraph': 700.0, 'sentence': 350.0, 'clause': 250.0, 'comma': 150.0, 'forced': None, 'end': 0.0}


def ms_to_samples(ms, sample_rate=22050):
    """milliseconds -> samples, rounded half away from zero (a negative pause is an overlap of that many samples)"""
    v = float(ms) * float(sample_rate) / 1000.0
    if not np.isfinite(v):
        raise ValueError(f'{ms!r} ms is not finite')
    return int(v + 0.5) if v >= 0 else -int(-v + 0.5)


def fade_table(n):
    """The rising raised cosine over n samples, 0.5 - 0.5 cos(pi (i + 0.5) / n) in float64, rounded once to fp32 (numpy [n]); a table and
    its mirror add up to 1, so an overlap-added seam of equal material keeps its level."""
    n = int(n)
    if not 0 <= n <= MAX_FADE:
        raise ValueError(f'fade_table: {n} samples outside [0, {MAX_FADE}]')
    i = np.arange(n, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(np.pi * (i + 0.5) / max(n, 1))).astype(np.float32)


def pause_table(pauses, fade_ms):
    """DEFAULT_PAUSES overridden by `pauses` (a dict of boundary -> ms), 'forced' resolved to -fade_ms; ValueError for an unknown key or a
    value that is not finite"""
    table = dict(DEFAULT_PAUSES)
    for k, v in (pauses or {}).items():
        if k not in DEFAULT_PAUSES:
            raise ValueError(f'pauses: {k!r} is not one of {sorted(DEFAULT_PAUSES)}')
        table[k] = v
    if table['forced'] is None:
        table['forced'] = -float(fade_ms)
    for k, v in table.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(float(v)):
            raise ValueError(f'pauses[{k!r}]: {v!r} is not a finite number of milliseconds')
    return table


def join_rows(wave, lens, gaps, bounds=None, keep=0, lead=0, fade=None, return_device_table=False):
    """wave [B, n_max] fp32 on the device, lens int64 [B] (None: whole rows), gaps: B host integers (samples behind each row; negative:
    overlap with the next row), bounds int64 [B, 2] on the device (TrimEngine.bounds) or None, keep / lead in samples, fade: a rising
    table (numpy / tensor, at most 4096 entries) or None -> (out [1, N] fp32 on the device, segs int64 [B, 4] on the host =
    (out_start, out_end, src_start, src_end) per row).  `out` is cut from a buffer sized by a host-side upper bound (lead + B n_max +
    the positive gaps); the only read-back is total and segs, 8 (4 B + 1) bytes in one copy.  return_device_table: a third result, segs
    as int64 [B, 4] still on the device (the table the read-back copies), for work that goes on there: tts_long's timestamps."""
    lib = _require_gpu()
    wave = _dev_f32(wave, 2, 'join_rows: wave')
    B, n_max = wave.shape
    if not 1 <= B <= MAX_ROWS:
        raise L.TtsAmdError(f'join_rows: {B} rows outside [1, {MAX_ROWS}]')
    dev = wave.device
    lens = _dev_lens(lens, B, n_max, dev)
    gaps = [int(g) for g in row_values(gaps, B, 'join_rows: gaps')]
    keep, lead = int(keep), int(lead)
    if keep < 0 or lead < 0:
        raise ValueError(f'join_rows: keep {keep} / lead {lead} must not be negative')
    if bounds is not None:
        bounds = bounds.to(device=dev, dtype=torch.int64).contiguous()
        if bounds.shape != (B, 2):
            raise L.TtsAmdError(f'join_rows: bounds of shape {tuple(bounds.shape)} for {B} rows')
    F = 0
    if fade is not None:
        fade = torch.as_tensor(np.asarray(fade) if not isinstance(fade, torch.Tensor) else fade).to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        F = int(fade.numel())
        if F > MAX_FADE:
            raise L.TtsAmdError(f'join_rows: a fade table of {F} entries (at most {MAX_FADE})')
        if F == 0:
            fade = None
    width = lead + B * n_max + sum(g for g in gaps if g > 0)
    out = torch.empty(1, max(width, 1), dtype=torch.float32, device=dev)
    table = torch.empty(4 * B + 1, dtype=torch.int64, device=dev)            # segs [B][4], then total
    gap_d = torch.tensor(gaps, dtype=torch.int64).to(dev)
    with torch.cuda.device(dev):
        L.check(lib.ttsamd_wave_join(_ptr(wave), n_max, _ptr(lens), _ptr(bounds), _ptr(gap_d), B, _ptr(fade), F, keep, lead, _ptr(out),
                                     width, _ptr(table), _ptr(table[4 * B:]), _stream()), 'wave_join')
    table_d, table = table, table.cpu()
    total = int(table[4 * B])
    assert 0 <= total <= width, (total, width)
    if return_device_table:
        return out[:, :total], table[:4 * B].reshape(B, 4), table_d[:4 * B].view(B, 4)
    return out[:, :total], table[:4 * B].reshape(B, 4)


def span_maps(table):
    """join_rows' device table int64 [B, 4] = (out_start, out_end, src_start, src_end) -> token_spans' maps int64 [B, 5] on the device:
    (lo, hi, off, num, den) = (src_start, src_end, out_start, 1, 1): a position of the row's own wave, clamped to what the trim kept
    and moved to its place in the joined wave"""
    one = torch.ones_like(table[:, 0])
    return torch.stack([table[:, 2], table[:, 3], table[:, 0], one, one], dim=1).contiguous()


def paragraph_pieces(text_input, max_chars):
    """`tts_long`'s text argument -> (split_text's pieces, the line the model says for each: text.spoken_text, the segment without the
    marks that close it): a string as it is, a list of strings as paragraphs (joined by a newline, the paragraph boundary);
    ValueError when nothing is left to say"""
    from text import split_text, spoken_text
    if isinstance(text_input, (list, tuple)):
        if not all(isinstance(t, str) for t in text_input):
            raise TypeError('tts_long: a string or a list of strings')
        text_input = '\n'.join(text_input)
    pieces = split_text(text_input, max_chars)
    lines = [spoken_text(t) for t, _ in pieces]
    if not pieces or not all(lines):
        raise ValueError('tts_long: the text is empty')
    if len(pieces) > MAX_ROWS:
        raise ValueError(f'tts_long: {len(pieces)} segments (at most {MAX_ROWS} per call)')
    return pieces, lines


def join_paragraph(groups, pieces, pauses, trim_db, keep_ms, fade_ms, sample_rate, trimmer, normalize=None, limiter=None, true_peak=False,
                   spans=None):
    """What the two `tts_long` share behind the vocoder: groups = [(wave [b, w] on the device, samples int64 [b] on the device), ...] in
    the order of `pieces` -> the rows in one padded buffer, their trim bounds (trim_db None: whole rows), the join, the level of the
    JOINED wave as one row (level_waves: one gain for the paragraph), one copy to the host.  -> (wave [N] on the host, segment dicts).
    spans: one ttsamd.timing.PendingTimings per group, not launched yet: each is launched behind the join with its rows of the join
    table as maps (span_maps: clamped to what the trim kept, moved to the segment's place) and copied behind the wave -> a third result,
    the timing of the paragraph (positions in the joined wave; every word carries the index of its segment)."""
    from .engine import level_waves
    dev = groups[0][0].device
    width = max(int(w.shape[1]) for w, _ in groups)
    buf = torch.zeros(len(pieces), max(width, 1), dtype=torch.float32, device=dev)
    k = 0
    for w, _ in groups:
        buf[k:k + w.shape[0], :w.shape[1]] = w
        k += w.shape[0]
    assert k == len(pieces), (k, len(pieces))
    lens = torch.cat([n.to(device=dev, dtype=torch.int64).reshape(-1) for _, n in groups])
    bounds = None
    if trim_db is not None:
        bounds, _ = trimmer.bounds(buf, lens, float(trim_db), 1024, 256, gain=0.0)
    gaps = gaps_for([b for _, b in pieces], pauses, sample_rate)
    out, segs, *table = join_rows(buf, lens, gaps, bounds, keep=ms_to_samples(keep_ms, sample_rate),
                                  fade=fade_table(ms_to_samples(fade_ms, sample_rate)), **({'return_device_table': True} if spans else {}))
    k = 0
    for sp in spans or []:
        b = len(sp.token_rows)
        sp.launch(span_maps(table[0][k:k + b]), segments=list(range(k, k + b)))
        k += b
    if normalize is not None and out.shape[1]:
        out = level_waves(out, None, normalize, sample_rate, **({'limiter': limiter} if limiter else {}),
                          **({'true_peak': True} if true_peak else {}))
    if spans:
        from .timing import merge_timings
        return out[0].cpu(), segment_rows(pieces, segs), merge_timings([t for sp in spans for t in sp.resolve()])
    return out[0].cpu(), segment_rows(pieces, segs)


def gaps_for(boundaries, pauses, sample_rate=22050):
    """the gap in samples behind every segment, from its boundary kind and a pause_table"""
    return [ms_to_samples(pauses[b], sample_rate) for b in boundaries]


def segment_rows(pieces, segs):
    """split_text's pieces + join_rows' segs -> the list of dicts `tts_long(return_segments=True)` hands out"""
    return [dict(text=t, boundary=b, start=int(r[0]), end=int(r[1]), src_start=int(r[2]), src_end=int(r[3]))
            for (t, b), r in zip(pieces, segs.tolist())]
