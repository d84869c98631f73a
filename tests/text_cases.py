"""Built cases of the text-to-term-ids path, each named for its property, with the plain restatement the
device is held to (texts -> token lists -> term ids -> the distinct-first-32 table with flags: backend.tokenize,
a dict lookup and _query_terms, nothing else) and a numpy restatement of the vocabulary hash thr_hip.h
documents.  No GPU, no library call: tests/test_text_host.py checks that every case has its property,
tests/test_gpu_text.py runs them."""
import random
from typing import Callable, Dict, List, NamedTuple, Sequence

import numpy as np

from triple_hybrid_rag_amd import _native as N
from triple_hybrid_rag_amd import backend
from triple_hybrid_rag_amd.index_text import TextTable

S = N.THR_TEXT_SLICE_BYTES
MT = N.THR_BM25_MAX_TERMS
FNV_BASIS, FNV_PRIME = np.uint64(0xCBF29CE484222325), np.uint64(0x100000001B3)


def enc(s: str) -> bytes:
    return s.encode("utf-8", "surrogatepass")


# ------------------------------------------------------------------ the documented hash, in numpy
def hash_keys(keys: Sequence[bytes]) -> np.ndarray:
    """64-bit FNV-1a over each key's bytes, 0 replaced by 1 -> uint64 [len(keys)]."""
    out = np.empty(len(keys), dtype=np.uint64)
    by_len: Dict[int, List[int]] = {}
    for i, k in enumerate(keys):
        by_len.setdefault(len(k), []).append(i)
    with np.errstate(over="ignore"):
        for L, idx in by_len.items():
            h = np.full(len(idx), FNV_BASIS, dtype=np.uint64)
            if L:
                m = np.frombuffer(b"".join(keys[i] for i in idx), dtype=np.uint8).reshape(len(idx), L).astype(np.uint64)
                for j in range(L):
                    h = (h ^ m[:, j]) * FNV_PRIME
            h[h == 0] = 1
            out[idx] = h
    return out


def home_slot(h: np.ndarray, capacity: int) -> np.ndarray:
    return ((h ^ (h >> np.uint64(32))) & np.uint64(0xFFFFFFFF)).astype(np.int64) & (capacity - 1)


def build_table(keys: Sequence[bytes], capacity: int, ids: Sequence[int] = None) -> np.ndarray:
    """The open-addressing table as thr_vocab_insert would leave it after inserting the keys one after the
    other -> int64 [capacity, 2] (hash word; term_id in the low half of the second word)."""
    slots = np.zeros((capacity, 2), dtype=np.uint64)
    hs = hash_keys(keys)
    for i, (h, s) in enumerate(zip(hs.tolist(), home_slot(hs, capacity).tolist())):
        while slots[s, 0] != 0:
            s = (s + 1) & (capacity - 1)
        slots[s, 0] = h
        slots[s, 1] = (i if ids is None else ids[i]) & 0xFFFFFFFF
    return slots.view(np.int64)


def table_lookup(slots: np.ndarray, keys: Sequence[bytes], key: bytes) -> int:
    """The documented lookup: probe from the home slot to the first empty one, take a slot whose hash AND
    bytes equal the key's."""
    cap = slots.shape[0]
    u = slots.view(np.uint64)
    h = hash_keys([key])
    s = int(home_slot(h, cap)[0])
    for _ in range(cap):
        if u[s, 0] == 0:
            return -1
        t = int(u[s, 1] & np.uint64(0xFFFFFFFF))
        if u[s, 0] == h[0] and t < len(keys) and keys[t] == key:
            return t
        s = (s + 1) & (cap - 1)
    return -1


def colliding_keys(n: int, capacity: int, slot: int = None, pattern: str = "k%d", limit: int = 4_000_000):
    """n keys of the pattern whose home slot in a table of ``capacity`` is the same (``slot``, or the one of
    the pattern's first key)."""
    found: List[str] = []
    for base in range(0, limit, 200_000):
        ks = [pattern % i for i in range(base, base + 200_000)]
        hs = home_slot(hash_keys([k.encode() for k in ks]), capacity)
        if slot is None:
            slot = int(hs[0])
        found += [ks[i] for i in np.flatnonzero(hs == slot).tolist()]
        if len(found) >= n:
            return found[:n], slot
    raise AssertionError("not enough colliding keys")


# ------------------------------------------------------------------ the plain restatement
def expect_rows(texts: Sequence[str], ids: Dict[str, int], table: TextTable = None):
    """-> (doc int32, term int32, n_tokens int32, flags int32): the table's tokenizer (backend.tokenize for
    the default table) and a dict lookup; -1 for a token outside the vocabulary."""
    tokenizer = backend.tokenize if table is None else table.tokenize
    table = table or TextTable.default()
    doc, term, n_tokens, flags = [], [], [], []
    for d, t in enumerate(texts):
        toks = tokenizer(t)
        doc += [d] * len(toks)
        term += [ids.get(tok, -1) for tok in toks]
        n_tokens.append(len(toks))
        flags.append(1 if table.is_exceptional(t) else 0)
    return (np.asarray(doc, dtype=np.int32), np.asarray(term, dtype=np.int32), np.asarray(n_tokens, dtype=np.int32),
            np.asarray(flags, dtype=np.int32))


def expect_query_table(texts: Sequence[str], ids: Dict[str, int], table: TextTable = None):
    """-> (terms int32 [nq, 32] padded with -1, n_distinct clamped at 33, flags): _query_terms' loop."""
    tokenizer = backend.tokenize if table is None else table.tokenize
    table = table or TextTable.default()
    terms = np.full((len(texts), MT), -1, dtype=np.int32)
    nd = np.zeros(len(texts), dtype=np.int32)
    flags = np.zeros(len(texts), dtype=np.int32)
    for q, text in enumerate(texts):
        seen: List[int] = []
        have = set()
        f = 1 if table.is_exceptional(text) else 0
        for tok in tokenizer(text):
            t = ids.get(tok)
            if t is None:
                f |= N.THR_TEXT_UNKNOWN
            elif t not in have:
                have.add(t)
                seen.append(t)
        if len(seen) > MT:
            f |= N.THR_TEXT_TOO_MANY
        terms[q, :min(len(seen), MT)] = seen[:MT]
        nd[q] = min(len(seen), MT + 1)
        flags[q] = f
    return terms, nd, flags


def vocab_of(texts: Sequence[str], tokenizer=backend.tokenize, drop: Sequence[str] = ()) -> List[str]:
    """The distinct tokens of the texts in order of first appearance, without ``drop``."""
    out: Dict[str, None] = {}
    for t in texts:
        for tok in tokenizer(t):
            if tok not in drop:
                out.setdefault(tok, None)
    return list(out)


class Case(NamedTuple):
    name: str
    texts: List[str]
    vocab: List[str]
    holds: Callable[[], bool]      # the property the case is named for


def _blob(texts):
    return b"".join(enc(t) for t in texts)


def _ptr(texts):
    return np.concatenate([[0], np.cumsum([len(enc(t)) for t in texts])]).tolist()


def _filler(n: int) -> str:
    """n bytes of ASCII words and spaces ending in a space."""
    return ("ab cde f " * (n // 9 + 1))[:n - 1] + " " if n > 0 else ""


def slice_cases() -> List[Case]:
    out = []
    t = _filler(S - 2) + "abcdef" + " z"
    out.append(Case("token_from_S-2_to_S+3", [t], ["abcdef", "ab", "z"], lambda t=t: enc(t).find(b"abcdef") == S - 2))
    for ch, word in (("é", True), ("§", False), ("中", True), ("—", False)):
        L = len(enc(ch))
        for k in range(1, L):
            t = _filler(S - k - 2) + "ab" + ch + "cd" + " q"
            voc = vocab_of([t], drop=("f",))
            out.append(Case(f"{L}-byte_{'word' if word else 'separator'}_lead_at_S-{k}", [t], voc,
                            lambda t=t, ch=ch, k=k, word=word: enc(t)[S - k:S - k + len(enc(ch))] == enc(ch) and
                            (("ab" + ch + "cd") in backend.tokenize(t)) == word))
    for delta in (-1, 0, 1):
        first = _filler(S + delta - 2) + "xy"
        texts = [first, "cd ef"]
        out.append(Case(f"text_boundary_at_S{delta:+d}", texts, ["xy", "cd", "xycd"],
                        lambda texts=texts, delta=delta: _ptr(texts)[1] == S + delta and texts[0][-1].isalpha()))
    long = "a" * (2 * S + 500)
    texts = [" q " + long + " r", long + "b"]
    out.append(Case("one_token_of_2S+500_bytes", texts, [long, "r"], lambda texts=texts: len(backend.tokenize(texts[0])[1]) == 2 * S + 500))
    for total in (S, S + 1, 1):
        t = (_filler(total - 1) + "a") if total > 1 else "a"
        out.append(Case(f"total_length_{total}", [t], ["a", "ab", "cde"], lambda t=t, total=total: len(enc(t)) == total))
    return out


def boundary_cases() -> List[Case]:
    out = [Case("ab_cd_no_separator_two_tokens", ["ab", "cd"], ["ab", "cd", "abcd"], lambda: _blob(["ab", "cd"]) == b"abcd"),
           Case("empty_texts", ["", "a", "", "", "b c", ""], ["a", "c"], lambda: True),
           Case("separators_only", ["  ,. ", "—§", "a"], ["a"],
                lambda: backend.tokenize("  ,. ") == [] and backend.tokenize("—§") == []),
           Case("one_text", ["hello world"], ["world"], lambda: True)]
    r = random.Random(7)
    pieces = ["", "a", "b", " ", ",", "ab", "a b", "é", "éa", "中", "abc", " a ", "b,"]
    tiny = [r.choice(pieces) for _ in range(70_000)]
    out.append(Case("70000_texts_of_0_to_3_bytes", tiny, ["a", "ab", "é", "中", "abc"],
                    lambda: len(tiny) == 70_000 and max(len(enc(t)) for t in tiny) == 3 and len(_blob(tiny)) / S < 40))
    return out


LOWERING = ["ȺB xK ẞa Åb Ωc HELLO World",           # Ⱥ K(Kelvin) ẞ Å(Angstrom) Ω(Ohm), ASCII
            "Привет мир τελος ς "
            "中文 字 ٣٤٥ x² a_b _ ²",
            "éa cafés"]


def lowering_cases() -> List[Case]:
    def differs():
        src = LOWERING[0].split()
        return all(len(enc(a)) != len(enc(b)) for a, b in zip(src[:5], backend.tokenize(LOWERING[0])[:5]))
    return [Case("lowering_changes_the_encoded_length", [LOWERING[0]], vocab_of([LOWERING[0]]), differs),
            Case("scripts_digits_and_underscore", [LOWERING[1]], vocab_of([LOWERING[1]], drop=("字",)),
                 lambda: "ς" in backend.tokenize(LOWERING[1]) and "٣٤٥" in backend.tokenize(LOWERING[1])
                 and "x²" in backend.tokenize(LOWERING[1]) and "_" in backend.tokenize(LOWERING[1])),
            Case("combining_acute_splits_a_token", [LOWERING[2]], ["e", "a", "cafe", "s"],
                 lambda: backend.tokenize(LOWERING[2]) == ["e", "a", "cafe", "s"])]


EXCEPTIONAL = ["İstanbul x", "ΣΑΣ ΟΔΟΣ", "ok \U0001F600 fine", "\U0001D400bc d",
               "bad\ud800surrogate"]


def exceptional_cases() -> List[Case]:
    texts = []
    for t in EXCEPTIONAL:
        texts += ["plain neighbour", t]
    texts.append("last plain text")
    T = TextTable.default()
    return [Case("exceptional_texts_between_plain_neighbours", texts, vocab_of(texts, drop=("fine",)),
                 lambda: [T.is_exceptional(t) for t in texts] == [False, True] * len(EXCEPTIONAL) + [False])]


def query_cases() -> List[Case]:
    voc = [f"w{i}" for i in range(40)]
    r = random.Random(11)
    thousand = " ".join(r.choice(voc[:30] + ["nope"]) for _ in range(1000))
    texts = ["w1 w2 w1 w1 w3 w2",
             " ".join(voc[:32]), " ".join(voc[:33]), " ".join(voc[:33] + voc[:33]),
             "zzz w1 w2", "w1 w2 zzz", "zzz", "zzz yyy",
             "", "  ,, ", thousand, "W5 w5 W5"]
    return [Case("query_table_edges", texts, voc,
                 lambda: len(set(thousand.split())) == 31 and len(thousand.split()) == 1000)]


def all_cases() -> List[Case]:
    return slice_cases() + boundary_cases() + lowering_cases() + exceptional_cases() + query_cases()
