"""Text front end of the inference script: the 178-symbol table and ``TextCleaner`` (test.py:19-38; the same table is
in meldataset.py:14-29 and Utils/RelTransformerEnc.py:6-10).  The vocabulary is data that a checkpoint's embedding
rows are indexed by, so it is reproduced exactly (pinned by tests/golden/text_golden.json, generated from the
reference); ``'`` occurs twice in the table and the later index wins, as in the reference's dict construction."""

_pad = "$"
_punctuation = ';:,.!?¡¿—…"«»“” '
_letters = 'ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz'
_letters_ipa = "ɑɐɒæɓʙβɔɕçɗɖðʤəɘɚɛɜɝɞɟʄɡɠɢʛɦɧħɥʜɨɪʝɭɬɫɮʟɱɯɰŋɳɲɴøɵɸθœɶʘɹɺɾɻʀʁɽʂʃʈʧʉʊʋⱱʌɣɤʍχʎʏʑʐʒʔʡʕʢǀǁǂǃˈˌːˑʼʴʰʱʲʷˠˤ˞↓↑→↗↘'̩'ᵻ"
symbols = [_pad] + list(_punctuation) + list(_letters) + list(_letters_ipa)
word_index_dictionary = {s: i for i, s in enumerate(symbols)}


PAUSE_SENTENCE, PAUSE_CLAUSE, PAUSE_WORD = "sentence", "clause", "word"
# the share of the sentence pause a cut of each class gets (ArtSpeech.synthesis_paragraph: pause_ms times this)
PAUSE_SCALE = {PAUSE_SENTENCE: 1.0, PAUSE_CLAUSE: 0.5, PAUSE_WORD: 0.0}
_SENTENCE_END, _CLAUSE_END = ".!?…", ",;:—"


def _cut_after(text, marks):
    """text cut behind every run of `marks` that a space follows; the marks stay with the piece in front, the space is dropped"""
    pieces, start, i = [], 0, 0
    while i < len(text):
        if text[i] in marks:
            j = i + 1
            while j < len(text) and text[j] in marks:
                j += 1
            if j < len(text) and text[j] == " ":
                pieces.append(text[start:j])
                while j < len(text) and text[j] == " ":
                    j += 1
                start = j
            i = j
        else:
            i += 1
    if start < len(text):
        pieces.append(text[start:])
    return [p for p in (q.strip() for q in pieces) if p]


def _pack(parts, max_tokens, sep=" "):
    """neighbours joined again while they fit into max_tokens"""
    out = []
    for p in parts:
        if out and len(out[-1]) + len(sep) + len(p) <= max_tokens:
            out[-1] = out[-1] + sep + p
        else:
            out.append(p)
    return out


def split_sentences(phonemes, max_tokens=None):
    """A paragraph of phonemes -> (pieces, pauses): cut behind ``. ! ? …`` followed by a space; a piece longer than max_tokens characters
    (one token each, TextCleaner) is cut further, first behind ``, ; : —`` and then at spaces (a single word longer than max_tokens stays
    whole).  The punctuation stays with its piece.  pauses[i] is the class of the cut between pieces[i] and pieces[i + 1] (PAUSE_SENTENCE,
    PAUSE_CLAUSE, PAUSE_WORD; PAUSE_SCALE gives each class's share of the sentence pause), so len(pauses) == max(len(pieces) - 1, 0).
    Host only."""
    if max_tokens is not None and max_tokens < 1:
        raise ValueError("split_sentences: max_tokens must be at least 1")
    pieces, pauses = [], []
    for sentence in _cut_after(phonemes.strip(), _SENTENCE_END):
        if max_tokens is None or len(sentence) <= max_tokens:
            parts = [(sentence, PAUSE_SENTENCE)]
        else:
            parts = []
            for clause in _pack(_cut_after(sentence, _CLAUSE_END), max_tokens):
                words = [clause] if len(clause) <= max_tokens else _pack(clause.split(), max_tokens)
                parts += [(w, PAUSE_WORD) for w in words[:-1]] + [(words[-1], PAUSE_CLAUSE)]
            parts[-1] = (parts[-1][0], PAUSE_SENTENCE)
        for text, cls in parts:
            pieces.append(text)
            pauses.append(cls)
    return pieces, pauses[:-1]


class TextCleaner:
    """test.py:30-38: characters -> ids; unknown characters are printed and dropped (meldataset.py's variant raises)."""

    def __init__(self, dummy=None, strict=False):
        self.word_index_dictionary = word_index_dictionary
        self.strict = strict

    def __call__(self, text):
        indexes = []
        for char in text:
            try:
                indexes.append(self.word_index_dictionary[char])
            except KeyError:
                if self.strict:
                    raise
                print(char)
        return indexes
