"""Query and chunk text to BM25 term ids, for a whole batch on the device.

The lexical channel takes term ids; the reference hands text to PostgreSQL (``plainto_tsquery(p_query)`` in
rag2_lexical_search, the text column of ingest.py's child-chunk insert) and the host restatement is
``tokenize`` below (``\\w+`` over ``text.lower()``; re-exported as ``backend.tokenize``), a lookup in ``store.vocab`` and
``GpuIndexClient._query_terms``.  ``TextSearch`` is the part of ``GpuIndex`` that holds a device copy of the
vocabulary (``set_vocabulary`` / ``grow_vocabulary``: an open-addressing hash table beside the keys' bytes)
and turns the texts of a batch into token rows (``text_rows``: thr_text_tokens) or into the int32 [nq, 32]
table ``bm25_search`` / ``retrieve_batch(query_terms=)`` take (``query_terms``: + thr_query_terms).

The analysis is DATA: a ``TextTable`` holds, per BMP code point, the lowered code point, whether the lowered
character is a word character and whether the code point is EXCEPTIONAL -- the per-character model does not
hold for it.  ``TextTable.default()`` is built from Python itself (``chr(cp).lower()``, ``re.fullmatch(r"\\w",
...)``), so the device equals ``backend.tokenize`` by construction and not by a copied Unicode database; the
exceptional code points are derived, never listed: those whose lowering is not one BMP code point, and those
for which the per-character restatement disagrees with the tokenizer in one of ``CONTEXTS``.  A text that
holds an exceptional code point, a code point above U+FFFF or a surrogate is EXCEPTIONAL: the device flags
it, the wrappers here find it on the host beforehand (one regular-expression search per text) and answer it
with the table's host tokenizer, so the answer is always the host's.

The token-level half of the analysis is DATA as well: an ``Analyzer`` puts a stop set and a table of suffix rules
(truncation only, so a stem is the lowered form of a prefix of its token's bytes) on top of a ``TextTable`` and
stands wherever one stands; with it set, the token rows come from thr_text_tokens_analyzed (thr_hip_text.h).

What stays on the host: the UTF-8 encoding (("utf-8", "surrogatepass"), as index_entities), the exceptional
texts, and the strings of unknown tokens (an ingest numbers them: GpuIndexClient.insert_children).

``number_text_rows`` / ``commit_vocabulary`` number the new terms of a batch ON THE DEVICE instead
(thr_vocab_grow: the next id at a token's first sighting, the numbering of that host loop): the rows come back
without a -1, the new keys stay on the device as a ``PendingVocabulary`` until the commit appends them to the key
store and inserts them, and their strings are decoded once per distinct term when the store's vocabulary wants
them.  A batch with an exceptional text, or two new tokens under one hash, takes the host route above.

``query_terms(fuzzy=Fuzzy(...))`` / ``nearest_terms`` add "did you mean" (thr_hip_fuzzy.h): a query token the
vocabulary does not hold is replaced by the vocabulary terms within a small edit distance of it, found by one scan
of the key store on the device (thr_vocab_nearest) and folded into the query table (thr_query_terms_fuzzy).
``nearest_terms_host`` / ``host_query_row_fuzzy`` below are the definition.
"""
from __future__ import annotations

import functools
import re
import unicodedata
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N
from .store import number_tokens  # noqa: F401 (the one host numbering; the store needs it without a device)

_TOKEN = re.compile(r"[\w]+", re.UNICODE)
_WORD = re.compile(r"\w", re.UNICODE)
CONTEXTS = ("a{}a", " {} ", "a{}", "{}a")       # between letters, between spaces, letter-left, letter-right


def tokenize(text: str) -> List[str]:
    """Lower-cased word tokens (the reference leaves tokenisation to PostgreSQL's 'portuguese' text-search configuration,
    which is not reproduced: this is the character half alone; ``Analyzer`` adds a stop list and suffix stemming of the
    project's own).  ``backend.tokenize`` is this object; ``TextTable.default()`` is built from it."""
    return _TOKEN.findall(text.lower())


def fold_accents(c: str) -> str:
    """The shipped example of a character map: accent folding on top of lowering -- NFD of the lowered
    character with the combining marks (Mn) stripped, kept only where that leaves one code point."""
    low = c.lower()
    bare = "".join(ch for ch in unicodedata.normalize("NFD", low) if unicodedata.category(ch) != "Mn")
    return bare if len(bare) == 1 else low


class TextTable:
    """uint32 [65536]: bits 0..15 the lowered code point, THR_TEXT_WORD, THR_TEXT_EXC (thr_hip.h, a9)."""

    def __init__(self, entries: np.ndarray, host: Callable[[str], List[str]]):
        entries = np.ascontiguousarray(entries, dtype=np.uint32)
        if entries.shape != (65536,):
            raise ValueError("a TextTable has one entry per BMP code point")
        self.entries = entries
        self._host = host        # the tokenizer the table restates: the answer for exceptional texts
        low = entries & 0xFFFF
        word = (entries & N.THR_TEXT_WORD) != 0
        # str.translate over a 65536-character string: a word character becomes its lowering, any other a space
        self._map = "".join(chr(int(c)) if w else " " for c, w in zip(low.tolist(), word.tolist()))
        self._exc_re: Optional[re.Pattern] = None

    # ------------------------------------------------------------ the host twin
    def restate(self, text: str) -> List[str]:
        """The per-character model, in plain Python: what the device computes for a text that is not
        exceptional (each character replaced by its entry, maximal runs of word characters)."""
        return text.translate(self._map).split()

    def is_exceptional(self, text: str) -> bool:
        if self._exc_re is None:
            exc = np.flatnonzero(self.entries & N.THR_TEXT_EXC)
            cls = "".join(re.escape(chr(int(c))) for c in exc)
            self._exc_re = re.compile("[" + cls + "\U00010000-\U0010FFFF]")
        return self._exc_re.search(text) is not None

    def exceptional_among(self, texts: Sequence[str]) -> List[int]:
        """The indices of the exceptional texts (one search over the joined batch settles the usual case)."""
        if not self.is_exceptional("\n".join(texts)):
            return []
        return [d for d, t in enumerate(texts) if self.is_exceptional(t)]

    def tokenize(self, text: str) -> List[str]:
        """The host tokenizer of this table (hand it to from_rows / GpuIndexClient): the restatement, and
        for an exceptional text the tokenizer the table was built from."""
        return self._host(text) if self.is_exceptional(text) else self.restate(text)

    # ------------------------------------------------------------ builders
    @staticmethod
    @functools.lru_cache(maxsize=1)
    def default() -> "TextTable":
        """backend.tokenize as a table, built from this Python's own str.lower() and \\w."""
        entries = np.zeros(65536, dtype=np.uint32)
        for cp in range(65536):
            low = chr(cp).lower()
            if len(low) != 1 or ord(low) > 0xFFFF or 0xD800 <= cp <= 0xDFFF:
                entries[cp] = cp | N.THR_TEXT_EXC
                continue
            entries[cp] = ord(low) | (N.THR_TEXT_WORD if _WORD.fullmatch(low) else 0)
        table = TextTable(entries, tokenize)
        # context-dependent lowerings cannot be seen per character: a code point for which the restatement
        # disagrees with the tokenizer in some context is exceptional too
        for cp in range(65536):
            if entries[cp] & N.THR_TEXT_EXC:
                continue
            c = chr(cp)
            if any(table.restate(ctx.format(c)) != tokenize(ctx.format(c)) for ctx in CONTEXTS):
                entries[cp] |= N.THR_TEXT_EXC
        return TextTable(entries, tokenize)

    @staticmethod
    def from_char_map(fn: Callable[[str], str]) -> "TextTable":
        """The analyzer hook: ``fn`` maps one character to one character (``fold_accents``); the tokenizer
        is "map each character, then \\w+".  A code point ``fn`` does not map to one BMP code point is
        exceptional (its texts are answered by that definition on the host)."""
        entries = np.zeros(65536, dtype=np.uint32)
        for cp in range(65536):
            m = fn(chr(cp))
            if len(m) != 1 or ord(m) > 0xFFFF or 0xD800 <= cp <= 0xDFFF:
                entries[cp] = cp | N.THR_TEXT_EXC
                continue
            entries[cp] = ord(m) | (N.THR_TEXT_WORD if _WORD.fullmatch(m) else 0)
        return TextTable(entries, lambda text: _TOKEN.findall("".join(map(fn, text))))


class Analyzer:
    """The token-level analysis on top of a ``TextTable``: a stop list and suffix stemming, as DATA.  This class
    IS the definition (thr_hip_text.h restates it; the device is held to it bit for bit):

        stem(tok):      for each step: among the step's rules (suffix, min_stem) with tok.endswith(suffix) and
                        len(tok) - len(suffix) >= min_stem the one with the longest suffix is taken (none: the step
                        does nothing) and tok = tok[:-len(suffix)]
        tokenize(text): [stem(t) for t in table.tokenize(text) if t not in stop]

    Lengths are code points of the lowered token (after the table's character map); the stop check is made on the
    whole lowered token, before stemming; a rule strips and never replaces, so a stem is the lowered form of a
    prefix of the token's bytes in the text, and everything behind the tokenizer works on a (byte offset, byte
    length) place as before.  It stands wherever a TextTable stands: ``set_vocabulary(terms, table=analyzer)``,
    ``GpuIndexClient(tokenizer=analyzer.tokenize, device_text=True)``, ``from_rows(tokenizer=analyzer.tokenize)``.
    An exceptional text is answered on the host, with the stop list and the stemmer applied on top of the table's
    host tokenizer.  Nothing of it is saved with an index: it is handed to the client that opens the store."""

    def __init__(self, table: Optional[TextTable] = None, stop: Sequence[str] = (), steps: Sequence[Sequence[Tuple[str, int]]] = ()):
        self.table = table if table is not None else TextTable.default()
        self.stop: Tuple[str, ...] = tuple(dict.fromkeys(stop))
        self.steps: Tuple[Tuple[Tuple[str, int], ...], ...] = tuple(tuple((s, int(m)) for s, m in step) for step in steps)
        for w in self.stop:
            self._fixed_point(w, "stop word")
        if len(self.steps) > N.STEM_MAX_STEPS:
            raise ValueError(f"Analyzer: {len(self.steps)} steps, at most THR_STEM_MAX_STEPS ({N.STEM_MAX_STEPS})")
        if sum(map(len, self.steps)) > N.STEM_MAX_RULES:
            raise ValueError(f"Analyzer: {sum(map(len, self.steps))} rules, at most THR_STEM_MAX_RULES ({N.STEM_MAX_RULES})")
        for i, step in enumerate(self.steps):
            seen = set()
            for suffix, min_stem in step:
                if suffix == "":
                    raise ValueError(f"Analyzer: step {i} holds an empty suffix")
                if len(suffix) > N.STEM_MAX_SUFFIX:
                    raise ValueError(f"Analyzer: suffix {suffix!r} of step {i} is longer than THR_STEM_MAX_SUFFIX "
                                     f"({N.STEM_MAX_SUFFIX}) code points")
                self._fixed_point(suffix, f"suffix of step {i}")
                if min_stem < 1:
                    raise ValueError(f"Analyzer: min_stem {min_stem} of suffix {suffix!r} in step {i} is below 1 "
                                     "(a stem is never empty)")
                if suffix in seen:
                    raise ValueError(f"Analyzer: suffix {suffix!r} occurs twice in step {i}")
                seen.add(suffix)
        self._stop = frozenset(self.stop)
        # longest suffix first (two suffixes of one length cannot both end a token): first match = longest match
        self._compiled = tuple(tuple(sorted(step, key=lambda r: -len(r[0]))) for step in self.steps)

    def _fixed_point(self, w: str, what: str) -> None:
        if self.table.is_exceptional(w):
            raise ValueError(f"Analyzer: {what} {w!r} holds an exceptional code point")
        if self.table.tokenize(w) != [w]:
            raise ValueError(f"Analyzer: {what} {w!r} is not a fixed point of the table's tokenizer "
                             f"(it gives {self.table.tokenize(w)!r})")

    # ------------------------------------------------------------ what a TextTable has
    @property
    def entries(self) -> np.ndarray:
        return self.table.entries

    def is_exceptional(self, text: str) -> bool:
        return self.table.is_exceptional(text)

    def exceptional_among(self, texts: Sequence[str]) -> List[int]:
        return self.table.exceptional_among(texts)

    def restate(self, text: str) -> List[str]:
        """The CHARACTER model alone (TextTable.restate): the lowered slice at an unknown stem's place is the stem."""
        return self.table.restate(text)

    @property
    def trivial(self) -> bool:
        """No stop words and no rules: the analyzer is its table."""
        return not self.stop and not any(self.steps)

    # ------------------------------------------------------------ the definition
    def stem(self, tok: str) -> str:
        for step in self._compiled:
            for suffix, min_stem in step:
                if len(tok) - len(suffix) >= min_stem and tok.endswith(suffix):
                    tok = tok[:-len(suffix)]
                    break
        return tok

    def tokenize(self, text: str) -> List[str]:
        """The host tokenizer (from_rows, GpuIndexClient(tokenizer=)): also the answer for an exceptional text."""
        stop = self._stop
        return [self.stem(t) for t in self.table.tokenize(text) if t not in stop]

    # ------------------------------------------------------------ the device tables (thr_hip_text.h)
    def rule_table(self) -> Tuple[List[int], np.ndarray]:
        """-> (step_ptr, rules uint8 [n_rules * THR_STEM_RULE_BYTES]): per step longest suffix first, a record
        { uint16 tail[8] (the suffix from its END), int32 len, int32 min_stem }."""
        step_ptr, recs = [0], []
        for step in self._compiled:
            for suffix, min_stem in step:
                rec = np.zeros(N.STEM_RULE_BYTES, dtype=np.uint8)
                rec[:16].view(np.uint16)[:len(suffix)] = [ord(c) for c in reversed(suffix)]
                rec[16:].view(np.int32)[:] = (len(suffix), min(min_stem, 0x7FFFFFFF))
                recs.append(rec)
            step_ptr.append(len(recs))
        return step_ptr, (np.concatenate(recs) if recs else np.zeros(0, dtype=np.uint8))

    # ------------------------------------------------------------ the shipped example
    @staticmethod
    def portuguese(fold: bool = False) -> "Analyzer":
        """A light Portuguese analysis, THE PROJECT'S OWN: a function-word stop list written for this project
        (articles, prepositions and their contractions, pronouns, conjunctions, the common forms of ser / estar /
        ter / haver) and three truncation steps -- plural; gender, adverb, diminutive and -ão; the common noun
        and verb endings as they stand once the gender vowel is gone.  It is NEITHER the Snowball stemmer NOR the
        PostgreSQL stop file, it claims no equality with the 'portuguese' text-search configuration, and it is
        checked only against the pairs listed in tests/test_text_analyzer_host.py.  ``fold``: over the
        accent-folding table (``fold_accents``), with the list and the suffixes folded the same way."""
        table = _fold_table() if fold else TextTable.default()
        fix = (lambda w: "".join(map(fold_accents, w))) if fold else (lambda w: w)
        steps = [[(fix(s), m) for s, m in step] for step in _PT_STEPS]
        steps = [list(dict(step).items()) for step in steps]          # (folding can make two suffixes one)
        return Analyzer(table, [fix(w) for w in _PT_STOP.split()], steps)


@functools.lru_cache(maxsize=1)
def _fold_table() -> TextTable:
    return TextTable.from_char_map(fold_accents)


_PT_STOP = """
o a os as um uma uns umas
de em por para com sem sob sobre entre até após desde contra perante
do da dos das no na nos nas pelo pela pelos pelas ao aos à às num numa nuns numas dum duma
deste desta destes destas desse dessa desses dessas daquele daquela daqueles daquelas disto disso daquilo
neste nesta nestes nestas nesse nessa nesses nessas naquele naquela naqueles naquelas nisto nisso naquilo àquele àquela
eu tu ele ela nós vós eles elas você vocês me te se lhe lhes vos
meu minha meus minhas teu tua teus tuas seu sua seus suas nosso nossa nossos nossas
este esta estes estas esse essa esses essas aquele aquela aqueles aquelas isto isso aquilo
que quem qual quais cujo cuja onde quando como
e ou mas nem porém contudo todavia porque pois embora enquanto logo portanto também já não mais muito
ser sou és é somos são era eram foi foram seja sejam fosse fossem será serão sendo sido
estar estou está estamos estão estava estavam esteve estiveram esteja estejam estando estado
ter tenho tem têm temos tinha tinham teve tiveram tenha tenham tendo tido terá terão
haver há hei havia haviam houve houveram haja hajam havendo havido
"""
_PT_STEPS = (
    # plural
    (("ões", 2), ("ães", 2), ("ais", 3), ("ns", 3), ("es", 3), ("s", 3)),
    # gender, adverb, diminutive, -ão
    (("mente", 4), ("zinho", 3), ("zinha", 3), ("inho", 3), ("inha", 3), ("ão", 2), ("a", 3), ("o", 3)),
    # noun and verb endings, as they stand behind the two steps above (falado -> falad -> fal)
    (("avam", 3), ("aram", 3), ("eram", 3), ("iram", 3), ("and", 3), ("end", 3), ("ind", 3), ("ar", 3), ("er", 3),
     ("ir", 3), ("ad", 3), ("id", 3), ("av", 3), ("ou", 3), ("eu", 3), ("iu", 3), ("am", 3), ("em", 3), ("ei", 3),
     ("al", 3), ("a", 3), ("e", 3), ("i", 3), ("o", 3)),
)


def is_table_tokenizer(tokenizer):
    """The TextTable (or Analyzer) whose ``.tokenize`` this is, or None.  An Analyzer with no stop words and no
    rules is its table."""
    owner = getattr(tokenizer, "__self__", None)
    func = getattr(tokenizer, "__func__", None)
    if isinstance(owner, TextTable) and func is TextTable.tokenize:
        return owner
    if isinstance(owner, Analyzer) and func is Analyzer.tokenize:
        return owner.table if owner.trivial else owner
    return None


def tokenizer_table(tokenizer, needs: str) -> TextTable:
    """The analysis a tokenizer stands for: ``backend.tokenize`` is ``TextTable.default()``, a table's ``.tokenize``
    that table, an ``Analyzer``'s ``.tokenize`` that analyzer.  Any other is refused by name; ``needs`` begins the
    message (the caller's option)."""
    table = TextTable.default() if tokenizer is tokenize else is_table_tokenizer(tokenizer)
    if table is None:
        name = getattr(tokenizer, "__qualname__", None) or repr(tokenizer)
        raise ValueError(f"{needs} needs backend.tokenize or a TextTable's .tokenize as the tokenizer, "
                         f"not {name}: the device restates a table, not a function")
    return table


def pack_texts(texts: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """The text store of thr_text_tokens -> (bytes uint8 with 16 zero bytes of padding behind the last text,
    ptr int64 [n + 1]); text d is bytes[ptr[d] : ptr[d + 1]]."""
    return pack_encoded([t.encode("utf-8", "surrogatepass") for t in texts])


def pack_encoded(enc: Sequence[bytes]) -> Tuple[np.ndarray, np.ndarray]:
    """``pack_texts`` for texts that are encoded already (a caller that sized its batches by those lengths)."""
    ptr = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        np.cumsum(np.fromiter((len(b) for b in enc), dtype=np.int64, count=len(enc)), out=ptr[1:])
    return np.frombuffer(b"".join(enc) + bytes(16), dtype=np.uint8), ptr


def vocab_capacity(n_terms: int) -> int:
    """Slots of the device table: the smallest power of two that keeps the load at or below 1/2."""
    cap = N.THR_VOCAB_MIN_SLOTS
    while cap < 2 * n_terms:
        cap *= 2
    return cap


def host_query_row(tokens: Sequence[str], ids: Dict[str, int]) -> Tuple[List[int], int, int]:
    """_query_terms' table row from a token list -> (the first THR_BM25_MAX_TERMS distinct known ids in order
    of first appearance, their number clamped at THR_BM25_MAX_TERMS + 1, THR_TEXT_UNKNOWN | THR_TEXT_TOO_MANY)."""
    seen: Dict[int, None] = {}
    flags = 0
    for tok in tokens:
        t = ids.get(tok)
        if t is None:
            flags |= N.THR_TEXT_UNKNOWN
        else:
            seen[t] = None      # (a key that is there keeps its place)
    if len(seen) > N.THR_BM25_MAX_TERMS:
        return list(seen)[:N.THR_BM25_MAX_TERMS], N.THR_BM25_MAX_TERMS + 1, flags | N.THR_TEXT_TOO_MANY
    return list(seen), len(seen), flags


# ---------------------------------------------------------------- typo-tolerant queries: the definition (thr_hip_fuzzy.h)
THR_FUZZY_MAX_LEN = N.FUZZY_MAX_LEN      # code points of a needle; longer tokens are never corrected
THR_FUZZY_MAX_BEST = N.FUZZY_MAX_BEST    # corrections kept per token
THR_TEXT_CORRECTED = N.TEXT_CORRECTED   # flag bit beside THR_TEXT_UNKNOWN / THR_TEXT_TOO_MANY


def levenshtein(a: str, b: str) -> int:
    """Insert / delete / substitute at unit cost, over code points (the two-row dynamic programme)."""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j - 1] + (ca != cb), prev[j] + 1, cur[j - 1] + 1))
        prev = cur
    return prev[-1]


def fuzzy_edits(n: int, max_edits: int) -> int:
    """The edit budget of a needle of n code points: Lucene's AUTO rule, capped."""
    return min(max_edits, 0 if n < 3 else 1 if n < 6 else 2)


def nearest_terms_host(needle: str, terms: Sequence[str], df, max_edits: int, n_best: int) -> List[Tuple[int, int]]:
    """THE DEFINITION of a correction (thr_vocab_nearest is held to it exactly).  needle: the lowered token (with an
    Analyzer: the stem); terms[i] the key of term i; df[i] its document frequency, or df None
    -> [(distance, term id)], best first: distance ascending, then frequency descending, then id ascending."""
    n = len(needle)
    d = fuzzy_edits(n, max_edits)
    if n > THR_FUZZY_MAX_LEN or (d == 0 and max_edits > 0 and n < 3):
        return []
    out = []
    for i, key in enumerate(terms):
        if abs(len(key) - n) > d:
            continue
        if df is not None and df[i] <= 0:       # a term without postings corrects nothing
            continue
        dist = levenshtein(needle, key)
        if dist <= d:
            out.append((dist, -min(int(df[i]), 2 ** 31 - 1) if df is not None else 0, i))
    return [(dist, i) for dist, _, i in sorted(out)[:n_best]]


def host_query_row_fuzzy(tokens: Sequence[str], ids: Dict[str, int], terms: Sequence[str], df, max_edits: int,
                         n_best: int, conjunctive: bool) -> Tuple[List[int], int, int]:
    """``host_query_row`` with an unknown token replaced, at its place, by its nearest terms: the best one alone
    in an AND query (the BM25 AND has no "t or t'" clause), up to n_best in an OR query.  A token with no
    correction keeps THR_TEXT_UNKNOWN; a corrected one sets THR_TEXT_CORRECTED instead."""
    seen: Dict[int, None] = {}
    flags = 0
    for tok in tokens:
        t = ids.get(tok)
        if t is not None:
            seen[t] = None
            continue
        near = nearest_terms_host(tok, terms, df, max_edits, 1 if conjunctive else n_best)
        if near:
            flags |= THR_TEXT_CORRECTED
            for _, i in near:
                seen.setdefault(i)
        else:
            flags |= N.THR_TEXT_UNKNOWN
    if len(seen) > N.THR_BM25_MAX_TERMS:
        return list(seen)[:N.THR_BM25_MAX_TERMS], N.THR_BM25_MAX_TERMS + 1, flags | N.THR_TEXT_TOO_MANY
    return list(seen), len(seen), flags


class Fuzzy:
    """The typo tolerance of a lexical query: an unknown token is replaced by the ``n_best`` (1 .. THR_FUZZY_MAX_BEST)
    vocabulary terms nearest to it, within min(``max_edits`` (1 .. 2), the budget of its length) edits."""

    def __init__(self, max_edits: int = 2, n_best: int = 2):
        if isinstance(max_edits, bool) or not isinstance(max_edits, int) or not 1 <= max_edits <= N.FUZZY_MAX_EDITS:
            raise ValueError(f"Fuzzy: max_edits {max_edits!r} outside 1 .. {N.FUZZY_MAX_EDITS}")
        if isinstance(n_best, bool) or not isinstance(n_best, int) or not 1 <= n_best <= THR_FUZZY_MAX_BEST:
            raise ValueError(f"Fuzzy: n_best {n_best!r} outside 1 .. THR_FUZZY_MAX_BEST ({THR_FUZZY_MAX_BEST})")
        self.max_edits, self.n_best = max_edits, n_best

    def __repr__(self) -> str:
        return f"Fuzzy(max_edits={self.max_edits}, n_best={self.n_best})"

    def __eq__(self, other) -> bool:
        return isinstance(other, Fuzzy) and (self.max_edits, self.n_best) == (other.max_edits, other.n_best)

    def __hash__(self) -> int:
        return hash((self.max_edits, self.n_best))


def check_fuzzy(what: str, fuzzy) -> None:
    if fuzzy is not None and not isinstance(fuzzy, Fuzzy):
        raise ValueError(f"{what}: fuzzy is an index_text.Fuzzy or None, not {type(fuzzy).__name__}")


class TextRows(NamedTuple):
    doc: torch.Tensor            # int32 [T] on the device: the text of each token, ascending
    term: torch.Tensor           # int32 [T] on the device: its term id, -1 for a token outside the vocabulary
    unknown: List[str]           # the distinct unknown tokens (lowered) in order of first appearance
    unknown_which: np.ndarray    # int64 [number of -1 rows]: per -1 row, in row order, its index in ``unknown``


class PendingVocabulary:
    """The new terms of a numbered batch, not yet in the vocabulary (``commit_vocabulary`` puts them there):
    ids ``n_before .. n_before + n_new - 1`` in order of first appearance.  From the device route the keys
    are device memory -- ``key_bytes`` uint8 (lowered UTF-8), ``key_ptr`` int64 [n_new + 1] relative to 0 --
    and ``terms`` decodes their strings on first use from ONE read-back of the blob: one decode per distinct
    new term.  From the host route (a batch with an exceptional text, a hash collision) the strings are
    there and the device halves are None."""

    def __init__(self, n_before: int, n_new: int, n_key_bytes: int = 0, key_bytes: Optional[torch.Tensor] = None,
                 key_ptr: Optional[torch.Tensor] = None, terms: Optional[List[str]] = None):
        self.n_before, self.n_new, self.n_key_bytes = int(n_before), int(n_new), int(n_key_bytes)
        self.key_bytes, self.key_ptr = key_bytes, key_ptr
        self._terms = terms if terms is not None else ([] if n_new == 0 else None)

    @property
    def terms(self) -> List[str]:
        if self._terms is None:
            self._terms = decode_keys(self.key_bytes[:self.n_key_bytes], self.key_ptr[:self.n_new + 1])
        return self._terms


def decode_keys(key_bytes: torch.Tensor, key_ptr: torch.Tensor) -> List[str]:
    """A key store as strings: one read-back of the blob, one decode per key."""
    blob = key_bytes.cpu().numpy().tobytes()
    ptr = key_ptr.cpu().tolist()
    return [blob[a:b].decode("utf-8", "surrogatepass") for a, b in zip(ptr, ptr[1:])]


class NumberedRows(NamedTuple):
    doc: torch.Tensor            # int32 [T] on the device: the text of each token, ascending
    term: torch.Tensor           # int32 [T] on the device: its term id; a new term has its id already, no -1
    n_before: int                # the vocabulary's size the numbering started from
    pending: PendingVocabulary   # the new terms, for commit_vocabulary


class TextSearch:
    text: Optional[dict] = None                 # table, its device copy, the vocabulary's host and device halves
    _ws_text: Optional[torch.Tensor] = None     # thr_text_tokens' workspace, grown on demand and kept
    _ws_qterms: Optional[torch.Tensor] = None
    _ws_grow: Optional[torch.Tensor] = None     # thr_vocab_grow's
    _ws_fuzzy: Optional[torch.Tensor] = None    # thr_vocab_nearest's

    # ------------------------------------------------------------ the vocabulary
    def set_vocabulary(self, terms: Sequence[str], table: Optional[TextTable] = None) -> "TextSearch":
        """The device vocabulary ``query_terms`` / ``text_rows`` look tokens up in (index set-up): terms[i] is
        the string of term id i, as the tokenizer produces it (lowered; with an ``Analyzer``, a stem).  ``table``: the
        analysis, default ``TextTable.default()``; an ``Analyzer``'s stop table and rules are uploaded beside the
        character table and the token rows then come from thr_text_tokens_analyzed.  Derived state: nothing of it is saved with the index.  Duplicates are
        refused; after set_lexical the count must be the lexical index's vocabulary size."""
        terms = list(terms)
        ids = {t: i for i, t in enumerate(terms)}
        if len(ids) != len(terms):
            raise ValueError("set_vocabulary: the terms hold duplicates")
        L = getattr(self, "lex", None)
        if L is not None and max(len(terms), 1) != L["rowptr"].shape[0] - 1:
            raise ValueError(f"set_vocabulary: {len(terms)} terms for the {L['rowptr'].shape[0] - 1} terms of the "
                             "lexical index (set_lexical)")
        table = table or TextTable.default()
        if isinstance(table, Analyzer) and table.trivial:
            table = table.table
        self.text = dict(table=table, table_dev=self._t(table.entries.view(np.int32), torch.int32), ids=ids,
                         term_bytes=torch.zeros(16, dtype=torch.uint8, device=self.device),
                         term_ptr=torch.zeros(1, dtype=torch.int64, device=self.device), n_bytes=0, slots=None,
                         analysis=self._upload_analysis(table) if isinstance(table, Analyzer) else None)
        self._extend_vocabulary(terms)
        return self

    def _upload_analysis(self, analyzer: Analyzer) -> dict:
        """The analyzer's stop set (the vocabulary's layout, built with thr_vocab_insert) and its rule table on the
        device: thr_text_tokens_analyzed's extra operands."""
        step_ptr, rules = analyzer.rule_table()
        A = dict(stop_slots=None, stop_bytes=None, stop_ptr=None, step_ptr=step_ptr,
                 rules=self._t(rules, torch.uint8) if len(rules) else None)
        if analyzer.stop:
            blob, ptr = pack_texts(analyzer.stop)
            A["stop_bytes"], A["stop_ptr"] = self._t(blob, torch.uint8), self._t(ptr, torch.int64)
            A["stop_slots"] = torch.zeros((vocab_capacity(len(analyzer.stop)), 2), dtype=torch.int64, device=self.device)
            N.vocab_insert(A["stop_slots"], A["stop_bytes"], A["stop_ptr"], 0, len(analyzer.stop))
        return A

    def grow_vocabulary(self, new_terms: Sequence[str]) -> "TextSearch":
        """Append terms: they get the next ids (thr_vocab_insert; above 1/2 load the table is reallocated and
        everything inserted again).  A term the vocabulary holds, or one repeated in the call, is refused."""
        if self.text is None:
            raise N.NativeError("grow_vocabulary: the index has no vocabulary (set_vocabulary)")
        new_terms = list(new_terms)
        ids = self._mirror()
        if len(set(new_terms)) != len(new_terms) or any(t in ids for t in new_terms):
            raise ValueError("grow_vocabulary: a term is in the vocabulary already or repeated")
        v0 = len(ids)
        self._extend_vocabulary(new_terms)
        for i, t in enumerate(new_terms):
            ids[t] = v0 + i
        return self

    def _extend_vocabulary(self, terms: Sequence[str]) -> None:
        X = self.text
        v0 = X["term_ptr"].shape[0] - 1
        v1 = v0 + len(terms)
        if terms:
            blob, ptr = pack_texts(terms)
            ptr = X["n_bytes"] + ptr[1:]
            X["term_bytes"] = torch.cat([X["term_bytes"][:X["n_bytes"]], self._t(blob, torch.uint8)])
            X["term_ptr"] = torch.cat([X["term_ptr"], self._t(ptr, torch.int64)])
            X["n_bytes"] = int(ptr[-1])
        self._insert_keys(v0, v1)

    def _insert_keys(self, v0: int, v1: int) -> None:
        """Keys v0 .. v1 - 1 of the key store into the table; above 1/2 load a new table and every key again."""
        X = self.text
        cap = vocab_capacity(v1)
        if X["slots"] is None or X["slots"].shape[0] != cap:
            X["slots"] = torch.zeros((cap, 2), dtype=torch.int64, device=self.device)
            v0 = 0
        if v1 > v0:
            N.vocab_insert(X["slots"], X["term_bytes"], X["term_ptr"], v0, v1 - v0)

    def _mirror(self) -> Dict[str, int]:
        """The host mirror ``text["ids"]``, with the terms of every commit that left its strings on the device
        (``commit_vocabulary(mirror=False)``) decoded and added: called before any host-side lookup."""
        X = self.text
        for pending in X.pop("unmirrored", ()):
            ids = X["ids"]
            for i, t in enumerate(pending.terms):
                ids[t] = pending.n_before + i
        return X["ids"]

    # ------------------------------------------------------------ numbering new terms on the device
    def number_text_rows(self, texts: Sequence[str], hash_mask: Optional[int] = None, packed=None,
                         on_device: bool = True) -> NumberedRows:
        """The token rows of a batch of chunk texts with the new terms NUMBERED on the device ->
        NumberedRows(doc, term, n_before, pending): ``append_rows(lex=(doc, term, None, n_before +
        pending.n_new))`` takes them as they are, ``commit_vocabulary(pending)`` then puts the new keys into
        the vocabulary.  The numbering is ``number_tokens``': the next id at a token's first sighting, in text
        order (thr_text_tokens, then thr_vocab_grow).  Until the commit nothing of the vocabulary changes.
        Two read-backs: the counts, then n_new / n_new_bytes / status.
        ``on_device=False`` numbers on the host: ``text_rows`` (the unknown tokens come back as strings), its
        numbering, one patch of the -1 rows; the pending set then holds the strings.  A batch that holds an
        exceptional text, or whose call comes back with THR_VOCAB_GROW_COLLISION, is answered that way too:
        the same object with the same values.  THR_VOCAB_GROW_OVERFLOW is a second call with the room it
        reported.
        ``hash_mask`` is for tests (thr_hip.h); ``packed``: pack_texts(texts), when the caller has it."""
        if self.text is None:
            raise N.NativeError("number_text_rows: the index has no vocabulary (set_vocabulary)")
        texts = list(texts)
        X = self.text
        n_before = X["term_ptr"].shape[0] - 1
        if not texts:
            empty = torch.empty(0, dtype=torch.int32, device=self.device)
            return NumberedRows(empty, empty.clone(), n_before, PendingVocabulary(n_before, 0))
        if not on_device:
            rows = self.text_rows(texts)
            term = rows.term
            if len(rows.unknown_which):
                term = term.clone()
                term[term < 0] = self._t((n_before + rows.unknown_which).astype(np.int32), torch.int32)
            return NumberedRows(rows.doc, term, n_before,
                                PendingVocabulary(n_before, len(rows.unknown), terms=list(rows.unknown)))
        if X["table"].exceptional_among(texts):
            return self.number_text_rows(texts, on_device=False)
        rows = self._text_tokens(texts, packed)
        n_total, n_unknown = torch.cat([rows["n_total"], rows["n_unknown"]]).tolist()
        assert n_total <= rows["capacity"]
        doc, term = rows["doc"][:n_total], rows["term"][:n_total]
        if n_unknown == 0:
            return NumberedRows(doc, term, n_before, PendingVocabulary(n_before, 0))
        n_bytes = int(rows["ptr"][-1])
        room = min(3 * n_bytes // 2 + 16, 16 * n_unknown)
        mask = (1 << 64) - 1 if hash_mask is None else int(hash_mask)
        need = N.vocab_grow_workspace_bytes(n_unknown)
        patch = term
        while True:
            out = N.vocab_grow(rows["bytes_dev"], rows["ptr_dev"], n_bytes, X["table_dev"], rows, n_unknown, n_before,
                               new_bytes_capacity=room, hash_mask=mask, term=patch,
                               workspace=self._scratch("_ws_grow", max(need, 16)))
            n_new, n_new_bytes, status = torch.cat([out["n_new"].long(), out["n_new_bytes"], out["status"].long()]).tolist()
            if status & N.THR_VOCAB_GROW_COLLISION:
                return self.number_text_rows(texts, on_device=False)
            if not status & N.THR_VOCAB_GROW_OVERFLOW:
                break
            room, patch = n_new_bytes, None     # (the rows are patched already: the ids do not depend on the room)
        return NumberedRows(doc, term, n_before,
                            PendingVocabulary(n_before, n_new, n_new_bytes, out["new_bytes"], out["new_ptr"]))

    def commit_vocabulary(self, pending: PendingVocabulary, mirror: bool = True) -> "TextSearch":
        """Put the new terms of a ``number_text_rows`` call into the vocabulary: the key bytes and pointers
        are appended to the key store ON THE DEVICE (no re-encode, no upload), then thr_vocab_insert (above
        1/2 load the table is reallocated and everything inserted again, as grow_vocabulary does).  A pending
        set that was numbered from another vocabulary size is refused.  ``mirror=False`` leaves the host
        mirror ``text["ids"]`` behind until a host-side lookup needs it (a bulk build: the strings are then
        decoded once from the final key store)."""
        if self.text is None:
            raise N.NativeError("commit_vocabulary: the index has no vocabulary (set_vocabulary)")
        X = self.text
        v0 = X["term_ptr"].shape[0] - 1
        if pending.n_before != v0:
            raise ValueError(f"commit_vocabulary: the terms were numbered from {pending.n_before}, the vocabulary "
                             f"holds {v0} (another commit came in between)")
        if pending.n_new == 0:
            return self
        if pending.key_bytes is None:       # numbered on the host: the strings are encoded and uploaded
            self._extend_vocabulary(pending.terms)
        else:
            nb = X["n_bytes"]
            X["term_bytes"] = torch.cat([X["term_bytes"][:nb], pending.key_bytes[:pending.n_key_bytes],
                                         torch.zeros(16, dtype=torch.uint8, device=self.device)])
            X["term_ptr"] = torch.cat([X["term_ptr"], pending.key_ptr[1:pending.n_new + 1] + nb])
            X["n_bytes"] = nb + pending.n_key_bytes
            self._insert_keys(v0, v0 + pending.n_new)
        X.setdefault("unmirrored", []).append(pending)
        if mirror:
            self._mirror()
        return self

    # ------------------------------------------------------------ texts
    def _text_tokens(self, texts: Sequence[str], packed=None) -> dict:
        X = self.text
        blob, ptr = packed if packed is not None else pack_texts(texts)
        n_bytes = int(ptr[-1])
        cap = N.text_token_capacity(len(texts), n_bytes)
        need = N.text_tokens_workspace_bytes(len(texts), n_bytes, cap)
        bytes_dev, ptr_dev = self._t(blob, torch.uint8), self._t(ptr, torch.int64)
        A = X.get("analysis")
        if A is None:
            rows = N.text_tokens(bytes_dev, ptr_dev, n_bytes, X["table_dev"], X["slots"],
                                 X["term_bytes"], X["term_ptr"], workspace=self._scratch("_ws_text", max(need, 8)))
        else:       # an Analyzer: stop tokens dropped, stems looked up (the workspace is thr_text_tokens')
            rows = N.text_tokens_analyzed(bytes_dev, ptr_dev, n_bytes, X["table_dev"], X["slots"], X["term_bytes"],
                                          X["term_ptr"], workspace=self._scratch("_ws_text", max(need, 8)), **A)
        rows["blob"], rows["ptr"] = blob, ptr
        rows["bytes_dev"], rows["ptr_dev"] = bytes_dev, ptr_dev      # (thr_vocab_grow reads the batch again)
        return rows

    def _term_rowptr(self) -> Optional[torch.Tensor]:
        """The document frequencies of the vocabulary as thr_vocab_nearest takes them: the postings' row pointer
        (a term the lexical index does not hold yet has no postings: the pointer is extended flat), or None for
        an index without a lexical index."""
        L = getattr(self, "lex", None)
        if L is None:
            return None
        rowptr, v = L["rowptr"], self.text["term_ptr"].shape[0] - 1
        if rowptr.shape[0] < v + 1:
            rowptr = torch.cat([rowptr, rowptr[-1:].expand(v + 1 - rowptr.shape[0])])
        return rowptr

    def _nearest(self, bytes_dev, n_bytes: int, unknown_off, unknown_len, n_unknown, fuzzy: Fuzzy, df: bool):
        X = self.text
        cap = min(unknown_off.shape[0], unknown_len.shape[0])
        need = N.vocab_nearest_workspace_bytes(n_bytes, cap, X["term_ptr"].shape[0] - 1, X["n_bytes"], fuzzy.n_best)
        return N.vocab_nearest(bytes_dev, n_bytes, X["table_dev"], unknown_off, unknown_len, n_unknown, X["term_bytes"],
                               X["term_ptr"], X["n_bytes"], term_rowptr=self._term_rowptr() if df else None,
                               max_edits=fuzzy.max_edits, n_best=fuzzy.n_best,
                               workspace=self._scratch("_ws_fuzzy", max(need, 16)))

    def nearest_terms(self, tokens: Sequence[str], fuzzy: Optional[Fuzzy] = None, df: bool = True):
        """"Did you mean": the vocabulary terms nearest to each of the already-lowered token strings -> (ids int32
        [n, n_best], dist int32 [n, n_best]) on the device, best first, padded with -1 (``nearest_terms_host`` is
        the definition; thr_vocab_nearest alone).  ``df``: rank equal distances by the lexical index's document
        frequencies and pass over terms without postings (an index without a lexical index has none to give).  A
        token the table calls exceptional, one of fewer than 3 or more than THR_FUZZY_MAX_LEN code points, gets a
        row of -1; a token that is itself a key finds that key at distance 0."""
        if self.text is None:
            raise N.NativeError("nearest_terms: the index has no vocabulary (set_vocabulary)")
        fuzzy = Fuzzy() if fuzzy is None else fuzzy
        check_fuzzy("nearest_terms", fuzzy)
        tokens = list(tokens)
        if not tokens:
            empty = torch.empty((0, fuzzy.n_best), dtype=torch.int32, device=self.device)
            return empty, empty.clone()
        blob, ptr = pack_texts(tokens)
        n_bytes = int(ptr[-1])
        return self._nearest(self._t(blob, torch.uint8), n_bytes, self._t(ptr[:-1].copy(), torch.int64),
                             self._t(np.diff(ptr).astype(np.int32), torch.int32),
                             self._t(np.asarray([len(tokens)], dtype=np.int32), torch.int32), fuzzy, df)

    def query_terms(self, texts: Sequence[str], conjunctive: bool = False, fuzzy: Optional[Fuzzy] = None):
        """The BM25 term table of a batch of query texts -> (terms int32 [nq, THR_BM25_MAX_TERMS] padded with
        -1, flags int32 [nq]), both on the device: per query GpuIndexClient._query_terms' answer -- the distinct
        known term ids in order of first appearance.  flags: THR_TEXT_EXCEPTIONAL (the row was computed on
        the host through the table's tokenizer and patched in), THR_TEXT_UNKNOWN, THR_TEXT_TOO_MANY.
        ``conjunctive``: a row with an unknown token or more than 32 distinct terms becomes all -1 (no chunk
        can hold every term: _query_terms' None; thr_bm25_topk answers an all -1 row with no rows in both
        forms).  The device path reads nothing back.
        ``fuzzy`` (a ``Fuzzy``; None: exactly the calls above): a token the vocabulary does not hold is replaced,
        at its place, by the vocabulary terms nearest to it (``host_query_row_fuzzy`` is the definition:
        thr_vocab_nearest over the unknown list, with the lexical index's document frequencies when there is
        one, then thr_query_terms_fuzzy) -- the best one alone when ``conjunctive``, up to ``fuzzy.n_best``
        otherwise; such a row carries THR_TEXT_CORRECTED, and THR_TEXT_UNKNOWN only when a token found no
        correction.  The exceptional queries keep their host rows, uncorrected."""
        if self.text is None:
            raise N.NativeError("query_terms: the index has no vocabulary (set_vocabulary)")
        check_fuzzy("query_terms", fuzzy)
        texts = list(texts)
        nq = len(texts)
        if nq == 0:
            return (torch.empty((0, N.THR_BM25_MAX_TERMS), dtype=torch.int32, device=self.device),
                    torch.empty(0, dtype=torch.int32, device=self.device))
        X = self.text
        rows = self._text_tokens(texts)
        if fuzzy is None:
            need = N.query_terms_workspace_bytes(nq)
            terms, _, flags = N.query_terms(rows, workspace=self._scratch("_ws_qterms", max(need, 8)))
        else:
            near, _ = self._nearest(rows["bytes_dev"], int(rows["ptr"][-1]), rows["unknown_off"], rows["unknown_len"],
                                    rows["n_unknown"], fuzzy, True)
            need = N.query_terms_fuzzy_workspace_bytes(nq)
            terms, _, flags = N.query_terms_fuzzy(rows, near, 1 if conjunctive else fuzzy.n_best,
                                                  workspace=self._scratch("_ws_qterms", max(need, 8)))
        redo = X["table"].exceptional_among(texts)
        if redo:
            host = np.full((len(redo), N.THR_BM25_MAX_TERMS), -1, dtype=np.int32)
            hflags = np.zeros(len(redo), dtype=np.int32)
            for i, q in enumerate(redo):
                row, _, f = host_query_row(X["table"].tokenize(texts[q]), self._mirror())
                host[i, :len(row)] = row
                hflags[i] = f | N.THR_TEXT_EXCEPTIONAL
            at = self._t(np.asarray(redo, dtype=np.int64), torch.int64)
            terms[at] = self._t(host, torch.int32)
            flags[at] = self._t(hflags, torch.int32)
        if conjunctive:
            void = (flags & (N.THR_TEXT_UNKNOWN | N.THR_TEXT_TOO_MANY)) != 0
            terms.masked_fill_(void[:, None], -1)
        return terms, flags

    def text_rows(self, texts: Sequence[str]) -> TextRows:
        """The token rows of a batch of chunk texts -> TextRows(doc, term, unknown, unknown_which): what
        ``append_rows(lex=(doc, term, None, n_vocab))`` takes once the -1 entries are numbered.  The
        exceptional texts are tokenised on the host and their rows merged in, in document order.  One host
        read-back (the counts and the unknown tokens' places)."""
        if self.text is None:
            raise N.NativeError("text_rows: the index has no vocabulary (set_vocabulary)")
        texts = list(texts)
        X = self.text
        table, ids = X["table"], self._mirror()
        redo = table.exceptional_among(texts)
        keep = texts
        if redo:
            gone = set(redo)
            kept_idx = [d for d in range(len(texts)) if d not in gone]
            keep = [texts[d] for d in kept_idx]
        unknown_seq: List[Tuple[int, str]] = []      # (text, token) of every unknown token, in row order
        if keep:
            rows = self._text_tokens(keep)
            n_total, n_unknown = int(rows["n_total"].item()), int(rows["n_unknown"].item())
            assert n_total <= rows["capacity"]
            doc, term = rows["doc"][:n_total], rows["term"][:n_total]
            off = rows["unknown_off"][:n_unknown].cpu().numpy()
            ln = rows["unknown_len"][:n_unknown].cpu().numpy()
            of_text = np.searchsorted(rows["ptr"], off, side="right") - 1
            raw = rows["blob"].tobytes()
            for d, o, l in zip(of_text.tolist(), off.tolist(), ln.tolist()):
                piece = raw[o:o + l].decode("utf-8", "surrogatepass")
                unknown_seq.append((kept_idx[d] if redo else d, table.restate(piece)[0]))
            if redo:
                doc = self._t(np.asarray(kept_idx, dtype=np.int32), torch.int32)[doc.long()]
        else:
            doc = torch.empty(0, dtype=torch.int32, device=self.device)
            term = torch.empty(0, dtype=torch.int32, device=self.device)
        if redo:
            hd, ht = [], []
            for d in redo:
                for tok in table.tokenize(texts[d]):
                    t = ids.get(tok, -1)
                    hd.append(d)
                    ht.append(t)
                    if t < 0:
                        unknown_seq.append((d, tok))
            doc = torch.cat([doc, self._t(np.asarray(hd, dtype=np.int32), torch.int32)])
            term = torch.cat([term, self._t(np.asarray(ht, dtype=np.int32), torch.int32)])
            order = torch.sort(doc, stable=True).indices       # a text's rows are all from one side
            doc, term = doc[order].contiguous(), term[order].contiguous()
            unknown_seq.sort(key=lambda e: e[0])                # (stable: a text's tokens keep their order)
        first: Dict[str, int] = {}
        which = np.fromiter((first.setdefault(tok, len(first)) for _, tok in unknown_seq), dtype=np.int64,
                            count=len(unknown_seq))
        return TextRows(doc.contiguous(), term.contiguous(), list(first), which)
