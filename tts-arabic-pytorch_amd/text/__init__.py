"""Text front-end of the drop-in surface: Arabic script / Buckwalter transliteration ->
phoneme string -> model tokens -> ids.  Function names follow the reference
(text/__init__.py:24-78) because callers import them; the implementation is table-driven.
"""
from text.symbols import symbols, DOUBLING_TOKEN, EOS_TOKEN, SEPARATOR_TOKEN
from text.phonetise import arabic_to_buckwalter, buckwalter_to_arabic, process_utterance, word_groups
from text.segment import split_text, spoken_text        # noqa: F401  (not in the reference: paragraph -> sentences for tts_long)

# phonetiser vowel variants (stress / emphasis / length marks) -> the six vowels the models know.
# Order matters for simplify_phonemes(): long vowels are replaced before their short prefixes.
_VOWEL_FAMILIES = (
    ('aa', 'aa AA'), ('uu', 'uu0 uu1 UU0 UU1'), ('ii', 'ii0 ii1 II0 II1'),
    ('a', 'a A'), ('u', 'u0 u1 U0 U1'), ('i', 'i0 i1 I0 I1'),
)
vowel_map = {variant: base for base, variants in _VOWEL_FAMILIES for variant in variants.split()}
vowels = list(vowel_map)

phon_to_id_ = {sym: idx for idx, sym in enumerate(symbols)}


def tokens_to_ids(phonemes, phon_to_id=None):
    """Token strings -> embedding rows; an unknown token raises KeyError like the reference."""
    lut = phon_to_id if phon_to_id is not None else phon_to_id_
    return [lut[tok] for tok in phonemes]


def ids_to_tokens(ids):
    return [symbols[i] for i in ids]


def _is_geminate(phon):
    return len(phon) == 2 and phon[0] == phon[1] and phon not in vowel_map


def phonemes_to_tokens(phonemes: str, append_space=True):
    """'b aa + dd a' -> ['b','aa','_+_','d','_dbl_','a', ('_+_',) '_eos_']: word separators become a
    token, doubled consonants become consonant + '_dbl_', vowel variants fold onto six vowels."""
    out = []
    for phon in phonemes.replace('sil', '').replace('+', SEPARATOR_TOKEN).split():
        if _is_geminate(phon):
            out.append(vowel_map.get(phon[0], phon[0]))
            out.append(DOUBLING_TOKEN)
        else:
            out.append(vowel_map.get(phon, phon))
    out.extend([SEPARATOR_TOKEN, EOS_TOKEN] if append_space else [EOS_TOKEN])
    return out


def buckwalter_to_phonemes(buckw):
    return process_utterance(buckw)


def arabic_to_phonemes(arabic):
    return buckwalter_to_phonemes(arabic_to_buckwalter(arabic))


def buckwalter_to_tokens(buckw, append_space=True):
    return phonemes_to_tokens(process_utterance(buckw), append_space=append_space)


def arabic_to_tokens(arabic, append_space=True):
    return buckwalter_to_tokens(arabic_to_buckwalter(arabic), append_space=append_space)


# ---- which tokens make which word (not in the reference; what the timestamps of ttsamd.timing are grouped by) ----
def word_ranges(tokens):
    """The half-open token ranges (t0, t1) of the words of a token list: the runs between SEPARATOR_TOKENs up to the first EOS_TOKEN.
    The separators, the EOS and whatever a model wrapper puts behind the last word (the separator of append_space, Tacotron2's inserted
    separator, its EOS run) lie outside every range.  Two separators in a row enclose an EMPTY range (t0 == t1): the pause that `-` or
    `sil` asks for has no tokens.  Range k belongs to line_words(line)[k]."""
    tokens = list(tokens)
    end = tokens.index(EOS_TOKEN) if EOS_TOKEN in tokens else len(tokens)
    while end and tokens[end - 1] == SEPARATOR_TOKEN:
        end -= 1
    ranges, t0 = [], 0
    for i in range(end):
        if tokens[i] == SEPARATOR_TOKEN:
            ranges.append((t0, i))
            t0 = i + 1
    if end:
        ranges.append((t0, end))
    return ranges


def line_words(line, arabic_in=True):
    """The words of a line (after the vowelizer if one is used) as the tokeniser groups them, in the line's own spelling, so that
    len(line_words(line)) == len(word_ranges(tokens of line)) for every line: text.phonetise.word_groups walks process_utterance's own
    steps.  In short: the pieces between single spaces; a free-standing . , ? ! joins the word in front of it (it is pronounced with it,
    not a word of its own); `-`, `sil` and a piece the phonetiser gets nothing from (digits, brackets, an empty piece between two
    spaces) are words with no tokens; and what stands behind the last word that has tokens is dropped, as word_ranges drops the
    separators there.  arabic_in: as arabic_to_tokens (True) or buckwalter_to_tokens (False) reads the line."""
    return tokens_and_words(line, arabic_in)[1]


def tokens_and_words(line, arabic_in=True, append_space=True):
    """(arabic_to_tokens(line, append_space) -- or buckwalter_to_tokens' with arabic_in=False --, line_words(line, arabic_in)) from ONE pass of
    the phonetiser over the line: what a call that wants timestamps tokenises with, so that the words cost no second pass"""
    groups = word_groups(line, to_buckwalter=arabic_in)
    tokens = phonemes_to_tokens(' + '.join(' '.join(phones) for _, phones in groups), append_space=append_space)
    while groups and not groups[-1][1]:
        groups.pop()
    return tokens, [word for word, _ in groups]


def simplify_phonemes(phonemes):
    for variant, base in vowel_map.items():
        phonemes = phonemes.replace(variant, base)
    return phonemes
