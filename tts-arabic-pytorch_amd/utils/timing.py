"""What a caller does with a timing (ttsamd.timing: the dict `tts(..., return_timestamps=True)` hands out): JSON, SubRip and WebVTT cues.
Host code.  A cue runs until adding the next word would pass `max_chars` characters or until the silence in front of the next word is
longer than `max_gap` seconds; 42 characters and 0.35 s are choices (a subtitle line, the default sentence pause), not measurements.
The last cue stays until the last token ends (the closing tokens belong to no word), i.e. until the audio does.  Times are floored to
the millisecond.  Words stay in logical order, as typed: no bidi reordering."""
import json


def to_json(timing, **kw):
    """the timing as JSON text (tuples become lists); keyword arguments go to json.dumps"""
    kw.setdefault('ensure_ascii', False)
    return json.dumps(timing, **kw)


def _stamp(samples, sample_rate, sep):
    ms = int(samples) * 1000 // int(sample_rate)                       # floored, in integers
    return f'{ms // 3600000:02d}:{ms // 60000 % 60:02d}:{ms // 1000 % 60:02d}{sep}{ms % 1000:03d}'


def cues(timing, max_chars=42, max_gap=0.35):
    """-> [(start, end, text)] in samples.  A word without a span of its own (a pause: start == end) and a word without text never
    open or close a cue and add no text; the gap is measured between the words that are spoken."""
    sr, out, cur = int(timing['sample_rate']), [], None
    for w in timing['words']:
        word = w['word'].strip()
        if not word or w['end'] <= w['start']:
            continue
        if cur is not None and (len(cur[2]) + 1 + len(word) > max_chars or (w['start'] - cur[1]) > max_gap * sr):
            out.append(tuple(cur))
            cur = None
        if cur is None:
            cur = [int(w['start']), int(w['end']), word]
        else:
            cur[1], cur[2] = int(w['end']), cur[2] + ' ' + word
    if cur is not None:
        if timing.get('tokens'):                                       # the closing tokens (the EOS) belong to no word: the last cue stays
            cur[1] = max(cur[1], int(timing['tokens'][-1]['end']))     # until the audio ends
        out.append(tuple(cur))
    return out


def to_srt(timing, max_chars=42, max_gap=0.35):
    sr = timing['sample_rate']
    return ''.join(f'{k}\n{_stamp(s, sr, ",")} --> {_stamp(e, sr, ",")}\n{text}\n\n' for k, (s, e, text) in enumerate(cues(timing, max_chars, max_gap), 1))


def to_vtt(timing, max_chars=42, max_gap=0.35):
    sr = timing['sample_rate']
    return 'WEBVTT\n\n' + ''.join(f'{_stamp(s, sr, ".")} --> {_stamp(e, sr, ".")}\n{text}\n\n' for s, e, text in cues(timing, max_chars, max_gap))
