"""Paragraph -> sentence-sized segments for `tts_long` (host, pure Python; not in the reference, whose callers pass one utterance).

`split_text(s, max_chars)` cuts `s` at punctuation that whitespace (or the end of the text) follows and returns the pieces with the
kind of boundary behind each, so that the caller can choose a pause per kind.  The marks are the same for Arabic script and for
Buckwalter transliteration -- none of them is a Buckwalter letter -- so both renderings of a text split at the same places (the
transliteration is one character for one).  A segment is a substring of `s`, outer whitespace stripped and its closing mark kept:
what a caller passing that sentence to `tts` would have written."""
import re

from text.phonetise import _BW

SENTENCE_MARKS = '.!?؟'          # . ! ? and the Arabic question mark
CLAUSE_MARKS = ';:؛'             # ; : and the Arabic semicolon
COMMA_MARKS = ',،'               # , and the Arabic comma
BOUNDARIES = ('paragraph', 'sentence', 'clause', 'comma', 'forced', 'end')

_BW_LETTERS = frozenset(_BW)


def _has_content(piece):
    """a letter or a digit, in either script (Buckwalter writes some letters with symbols: * $ < > } & ' | ~ ^)"""
    return any(ch.isalnum() or ch in _BW_LETTERS for ch in piece)


_BOUNDARY_MARKS = re.compile('[' + re.escape(SENTENCE_MARKS + CLAUSE_MARKS + COMMA_MARKS) + r']+(?=\s|$)')


def spoken_text(segment):
    """A segment as `tts_long` hands it to the model: the runs of marks that whitespace or the end follows are taken out.  The
    phonetiser turns a free-standing . , ? ! into a token of its own, which the 40-symbol inventory does not hold (tokens_to_ids raises
    KeyError, as the reference does), and drops the other marks; a sentence therefore has to be said without its closing mark.
    Marks inside a token (`3.14`) stay, so everything else reaches the front-end as the caller wrote it."""
    return _BOUNDARY_MARKS.sub('', segment).strip()


def _cuts(s, a, b, marks):
    """The cuts of s[a:b] (stripped) behind one of `marks` that whitespace follows: the index of that whitespace.  Text is left on
    both sides of every cut."""
    return [i + 1 for i in range(a, b - 1) if s[i] in marks and s[i + 1].isspace()]


def _skip_space(s, i):
    while s[i].isspace():
        i += 1
    return i


def _balanced(s, a, b, boundary, max_chars, out):
    """s[a:b] has no sentence or clause cut left: while it is longer than max_chars, halve it at the comma cut that leaves the most
    balanced halves; with no comma cut, at the space nearest the middle ('forced'); with no space, it stays whole."""
    if b - a <= max_chars:
        out.append((a, b, boundary))
        return
    cuts, label = _cuts(s, a, b, COMMA_MARKS), 'comma'
    if not cuts:
        cuts, label = [i for i in range(a + 1, b - 1) if s[i].isspace() and not s[i - 1].isspace()], 'forced'
    if not cuts:
        out.append((a, b, boundary))
        return
    c = min(cuts, key=lambda c: abs((c - a) - (b - _skip_space(s, c))))
    _balanced(s, a, c, label, max_chars, out)
    _balanced(s, _skip_space(s, c), b, boundary, max_chars, out)


def split_text(s, max_chars=200):
    """-> [(segment, boundary), ...], boundary one of 'paragraph' | 'sentence' | 'clause' | 'comma' | 'forced' | 'end' (the last one).
    Always cut: at one or more newlines (paragraph) and behind . ! ? ؟ (sentence).  A piece still longer than max_chars is cut at
    its ; : ؛ (clause); pieces still too long are halved at the , ، (comma) that leaves the most balanced halves, and where
    there is none at the space nearest the middle (forced); a piece with no space stays whole.  A mark is a boundary only when
    whitespace or the end of the text follows it (`3.14` and `a.b` do not split).  Pieces of marks only join the piece before them.
    Empty or whitespace-only text: []."""
    if not isinstance(s, str):
        raise TypeError(f'split_text: expected a string, got {type(s).__name__}')
    max_chars = int(max_chars)
    if max_chars < 1:
        raise ValueError(f'split_text: max_chars = {max_chars}')
    n = len(s)
    a = 0
    while a < n and s[a].isspace():
        a += 1
    end = n
    while end > a and s[end - 1].isspace():
        end -= 1
    if a == end:
        return []
    # paragraph and sentence cuts: every run of whitespace that holds a newline or stands behind a sentence mark
    first, i = [], a
    while i < end:
        if not s[i].isspace():
            i += 1
            continue
        j = _skip_space(s, i)
        if '\n' in s[i:j]:
            first.append((a, i, 'paragraph'))
            a = j
        elif s[i - 1] in SENTENCE_MARKS:
            first.append((a, i, 'sentence'))
            a = j
        i = j
    first.append((a, end, 'end'))
    spans = []
    for a, b, boundary in first:
        if b - a <= max_chars:
            spans.append((a, b, boundary))
            continue
        for c in _cuts(s, a, b, CLAUSE_MARKS):
            _balanced(s, a, c, 'clause', max_chars, spans)
            a = _skip_space(s, c)
        _balanced(s, a, b, boundary, max_chars, spans)
    # pieces of marks only go to the piece before them (a leading one to the piece behind it)
    merged = []
    for a, b, boundary in spans:
        if merged and (not _has_content(s[a:b]) or not _has_content(s[merged[-1][0]:merged[-1][1]])):
            merged[-1] = (merged[-1][0], b, boundary)
        else:
            merged.append((a, b, boundary))
    return [(s[a:b], boundary) for a, b, boundary in merged]
