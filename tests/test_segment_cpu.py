"""CPU: text.split_text (text/segment.py), the paragraph -> segments step in front of `tts_long`."""
import json
import os

import pytest

from conftest import GOLDEN


@pytest.fixture(scope='module')
def lines():
    with open(os.path.join(GOLDEN, 'infer_text_lines.json'), encoding='utf-8') as f:
        return json.load(f)


def _squash(s):
    return ' '.join(s.split())


def test_marks_stay_with_their_segment_and_the_last_boundary_is_end():
    from text import split_text
    got = split_text('qAla lwaladu. hal jA\'a? naEam! vum~a *ahaba')
    assert got == [('qAla lwaladu.', 'sentence'), ("hal jA'a?", 'sentence'), ('naEam!', 'sentence'), ('vum~a *ahaba', 'end')]
    assert split_text('one.') == [('one.', 'end')]
    assert split_text('  one.  \n') == [('one.', 'end')]
    # a run of marks stays together: only the last one has whitespace behind it
    assert split_text('wait... what?! yes') == [('wait...', 'sentence'), ('what?!', 'sentence'), ('yes', 'end')]


def test_marks_inside_a_token_do_not_split():
    from text import split_text
    assert split_text('pi is 3.14 and a.b is a name') == [('pi is 3.14 and a.b is a name', 'end')]
    assert split_text('at 10:30, ok', max_chars=5) == [('at', 'forced'), ('10:30,', 'comma'), ('ok', 'end')]
    assert split_text('v1.2.3 works. really') == [('v1.2.3 works.', 'sentence'), ('really', 'end')]


def test_paragraphs():
    from text import split_text
    assert split_text('first line\nsecond. third\n\n\n fourth') == [('first line', 'paragraph'), ('second.', 'sentence'), ('third', 'paragraph'),
                                                                   ('fourth', 'end')]
    # a sentence mark in front of a newline: the stronger boundary
    assert split_text('one.\r\ntwo') == [('one.', 'paragraph'), ('two', 'end')]


def test_arabic_marks_behave_as_their_latin_twins():
    from text import split_text
    latin = 'aaa bbb? ccc ddd, eee fff; ggg hhh'
    arabic = latin.replace('?', '؟').replace(',', '،').replace(';', '؛')
    for max_chars in (200, 17, 10):
        a, b = split_text(latin, max_chars), split_text(arabic, max_chars)
        assert [k for _, k in a] == [k for _, k in b]
        assert [t for t, _ in a] == [t.replace('؟', '?').replace('،', ',').replace('؛', ';') for t, _ in b]
    assert split_text(arabic, 200) == [('aaa bbb؟', 'sentence'), ('ccc ddd، eee fff؛ ggg hhh', 'end')]
    assert split_text(arabic, 17) == [('aaa bbb؟', 'sentence'), ('ccc ddd، eee fff؛', 'clause'), ('ggg hhh', 'end')]
    assert split_text(arabic, 10) == [('aaa bbb؟', 'sentence'), ('ccc ddd،', 'comma'), ('eee fff؛', 'clause'), ('ggg hhh', 'end')]


def test_buckwalter_and_arabic_renderings_split_at_the_same_places(lines):
    import text
    from text import split_text
    bw = f'{lines[9]}. {lines[14]}، {lines[36]}؛ {lines[19]}\n{lines[1]}, {lines[3]}? {lines[2]}'
    ar = text.buckwalter_to_arabic(bw)
    assert len(ar) == len(bw) and ar != bw
    for max_chars in (200, 80, 40, 12):
        a, b = split_text(bw, max_chars), split_text(ar, max_chars)
        assert [k for _, k in a] == [k for _, k in b]
        assert [t for t, _ in a] == [text.arabic_to_buckwalter(t) for t, _ in b]
        assert [len(t) for t, _ in a] == [len(t) for t, _ in b]


@pytest.mark.parametrize('max_chars', [200, 120, 60, 25, 8, 1])
def test_max_chars_is_honoured_wherever_a_space_exists_and_nothing_is_lost(lines, max_chars):
    from text import split_text
    para = f'{lines[1]}. {lines[16]}، {lines[8]}: {lines[31]}\n\n{lines[50]}, {lines[3]}! {lines[2]}'
    got = split_text(para, max_chars)
    assert got[-1][1] == 'end' and all(k != 'end' for _, k in got[:-1])
    for t, k in got:
        assert t == t.strip() and t and t in para
        assert len(t) <= max_chars or ' ' not in t, (len(t), t)
    assert _squash(' '.join(t for t, _ in got)) == _squash(para)


def test_policy_order_clause_then_balanced_commas_then_forced():
    from text import split_text
    # 41 characters, one clause mark: cut there and nowhere else while the pieces fit
    s = 'aaaa bbbb, cccc dddd; eeee ffff, gggg hhhh'
    assert split_text(s, 100) == [(s, 'end')]
    assert split_text(s, 25) == [('aaaa bbbb, cccc dddd;', 'clause'), ('eeee ffff, gggg hhhh', 'end')]
    # three commas: the middle one leaves the most balanced halves, then each half is halved again only if it is still too long
    c = 'aa bb, cc dd, ee ff, gg hh'
    assert split_text(c, 20) == [('aa bb, cc dd,', 'comma'), ('ee ff, gg hh', 'end')]
    assert split_text(c, 8) == [('aa bb,', 'comma'), ('cc dd,', 'comma'), ('ee ff,', 'comma'), ('gg hh', 'end')]
    # 'forced' appears only where no mark was available
    assert split_text('aaaa bbbb cccc dddd', 10) == [('aaaa bbbb', 'forced'), ('cccc dddd', 'end')]
    got = split_text('aa bb, cccc dddd eeee ffff', 12)
    assert got == [('aa bb,', 'comma'), ('cccc dddd', 'forced'), ('eeee ffff', 'end')]
    for t, k in split_text(c, 8) + split_text(s, 25):
        assert k != 'forced'
    # no space: left whole
    assert split_text('abcdefghijklmnop', 4) == [('abcdefghijklmnop', 'end')]
    assert split_text('abcdefghijklmnop qrs', 4) == [('abcdefghijklmnop', 'forced'), ('qrs', 'end')]


def test_pieces_of_marks_only_join_the_piece_before():
    from text import split_text
    assert split_text('hello . world') == [('hello .', 'sentence'), ('world', 'end')]
    assert split_text('hello. ... world') == [('hello. ...', 'sentence'), ('world', 'end')]
    assert split_text('one.\n--\ntwo') == [('one.\n--', 'paragraph'), ('two', 'end')]
    assert split_text('... hello') == [('... hello', 'end')]
    # Buckwalter letters written with symbols are letters
    assert split_text('a. * b') == [('a.', 'sentence'), ('* b', 'end')]
    assert split_text('a. $ . b') == [('a.', 'sentence'), ('$ .', 'sentence'), ('b', 'end')]


def test_blank_input_and_bad_arguments():
    from text import split_text
    assert split_text('') == [] and split_text(' \n\t  ') == []
    with pytest.raises(TypeError):
        split_text(['a'])
    with pytest.raises(ValueError):
        split_text('a', 0)


def test_no_mark_is_a_buckwalter_letter():
    from text.phonetise import _BW
    from text.segment import CLAUSE_MARKS, COMMA_MARKS, SENTENCE_MARKS
    assert not set(SENTENCE_MARKS + CLAUSE_MARKS + COMMA_MARKS) & set(_BW)
