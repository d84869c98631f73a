"""Built cases of thr_vocab_grow (numbering the new terms of a batch on the device), each named for its
property, and the plain-Python restatement of its contract: per unknown occurrence ``table.restate`` of its
bytes, a ``dict.setdefault`` numbering in list order, the key bytes by ``str.encode`` and the masked-hash
collision predicate by ``text_cases.hash_keys``.  No GPU, no library call: tests/test_vocab_grow_host.py
checks that every case has its property and that the restatement is the numbering of lexical_rows /
build_lexical, tests/test_gpu_vocab_grow.py runs them."""
import re
from typing import Callable, Dict, List, NamedTuple, Sequence

import numpy as np

import text_cases as TC
from triple_hybrid_rag_amd import _native as N
from triple_hybrid_rag_amd.index_text import TextTable, pack_texts

S = TC.S
UNIT = S // 4                       # bytes a wave of thr_text_tokens owns
ALL_ONES = (1 << 64) - 1
COLLISION, OVERFLOW = N.THR_VOCAB_GROW_COLLISION, N.THR_VOCAB_GROW_OVERFLOW


def scratch_capacity(unknown_capacity: int) -> int:
    """Slots of the scratch dedupe table: the smallest power of two >= 2 * unknown_capacity, at least 16."""
    cap = 16
    while cap < 2 * unknown_capacity:
        cap *= 2
    return cap


def masked_hashes(keys: Sequence[bytes], hash_mask: int) -> np.ndarray:
    h = TC.hash_keys(keys) & np.uint64(hash_mask)
    h[h == 0] = 1
    return h


# ------------------------------------------------------------------ the host twin of the unknown list
def unknown_list(texts: Sequence[str], ids: Dict[str, int], table: TextTable = None):
    """What thr_text_tokens leaves for thr_vocab_grow, made on the host -> dict(blob bytes, ptr, flags, off,
    len, term): the places of the tokens outside ``ids`` in text order, the per-text flags, and tok_term (-1
    for an unknown token).  The rows of an exceptional text are the per-character model's (they "may hold
    anything")."""
    table = table or TextTable.default()
    blob, ptr = pack_texts(texts)
    off, ln, term, flags = [], [], [], []
    for d, t in enumerate(texts):
        flags.append(1 if table.is_exceptional(t) else 0)
        for m in re.finditer(r"\S+", t.translate(table._map)):
            tid = ids.get(m.group(), -1)
            term.append(tid)
            if tid < 0:
                off.append(int(ptr[d]) + len(TC.enc(t[:m.start()])))
                ln.append(len(TC.enc(t[m.start():m.end()])))
    return dict(blob=blob.tobytes()[:int(ptr[-1])], ptr=np.asarray(ptr), flags=np.asarray(flags, dtype=np.int32),
                off=np.asarray(off, dtype=np.int64), len=np.asarray(ln, dtype=np.int32),
                term=np.asarray(term, dtype=np.int32))


# ------------------------------------------------------------------ the contract, restated
def expect_grow(blob: bytes, ptr, flags, off, ln, n_vocab: int, table: TextTable = None, hash_mask: int = ALL_ONES,
                tok_term=None):
    """thr_vocab_grow over an unknown list -> dict(unknown_term, new_bytes, new_ptr, n_new, n_new_bytes,
    collision, keys[, tok_term]).  Under ``collision`` the device only promises the status bit."""
    table = table or TextTable.default()
    first: Dict[str, int] = {}
    unknown_term = []
    of_text = np.searchsorted(np.asarray(ptr), np.asarray(off), side="right") - 1
    for d, o, l in zip(of_text.tolist(), np.asarray(off).tolist(), np.asarray(ln).tolist()):
        if flags[d] & N.THR_TEXT_EXCEPTIONAL:
            unknown_term.append(-1)
            continue
        tok = table.restate(blob[o:o + l].decode("utf-8", "surrogatepass"))[0]
        unknown_term.append(n_vocab + first.setdefault(tok, len(first)))
    keys = [TC.enc(t) for t in first]
    new_ptr = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
    out = dict(unknown_term=np.asarray(unknown_term, dtype=np.int32), new_bytes=np.frombuffer(b"".join(keys), dtype=np.uint8),
               new_ptr=new_ptr, n_new=len(keys), n_new_bytes=int(new_ptr[-1]), keys=list(first),
               collision=len(set(masked_hashes(keys, hash_mask).tolist())) < len(keys))
    if tok_term is not None:
        patched = np.array(tok_term, dtype=np.int32)
        neg = np.flatnonzero(patched < 0)
        assert len(neg) == len(unknown_term)
        patched[neg] = out["unknown_term"]
        out["tok_term"] = patched
    return out


def expect_numbered(texts: Sequence[str], ids: Dict[str, int], tokenizer: Callable[[str], List[str]] = TC.backend.tokenize):
    """The host loop of GpuIndexClient.insert_children -> (doc int32, term int32, the new terms in id order)."""
    grown: Dict[str, int] = {}
    doc, term = [], []
    for d, t in enumerate(texts):
        for tok in tokenizer(t):
            tid = ids.get(tok)
            if tid is None:
                tid = grown.setdefault(tok, len(ids) + len(grown))
            doc.append(d)
            term.append(tid)
    return np.asarray(doc, dtype=np.int32), np.asarray(term, dtype=np.int32), list(grown)


# ------------------------------------------------------------------ the cases
class Case(NamedTuple):
    name: str
    texts: List[str]
    vocab: List[str]
    holds: Callable[[], bool]      # the property the case is named for
    hash_mask: int = ALL_ONES


def n_unknown_of(case: Case) -> int:
    ids = {t: i for i, t in enumerate(case.vocab)}
    return sum(tok not in ids for t in case.texts for tok in TC.backend.tokenize(t))


def count_cases() -> List[Case]:
    out = []
    for k in (0, 1, 63, 64, 65, 255, 256, 257, 3100):
        distinct = max(1, (2 * k) // 3)
        words = []
        for i in range(k):
            words += [f"n{(i * 7) % distinct}", "known"] if i % 3 else [f"N{(i * 7) % distinct}"]
        words.append("known")
        texts = [" ".join(words[a:a + 50]) for a in range(0, len(words), 50)]
        case = Case(f"n_unknown_{k}", texts, ["known", "other"], lambda: True)
        out.append(case._replace(holds=lambda case=case, k=k: n_unknown_of(case) == k))
    return out


def sightings(case: Case, token: str) -> List[int]:
    """Byte offsets of the unknown occurrences whose lowered form is ``token``."""
    U = unknown_list(case.texts, {t: i for i, t in enumerate(case.vocab)})
    return [int(o) for o, l in zip(U["off"], U["len"]) if U["blob"][o:o + l].decode().lower() == token]


def slice_case() -> Case:
    """One new token just in front of and just behind the edge between slices 2 and 3 (two texts), and again
    in slice 9; other new tokens are sighted before it, so its rank is not 0 and its first sighting is in
    neither of the first two workgroups."""
    known = ["ab", "cde", "f"]
    t0 = "early1 early2 " + TC._filler(3 * S - 14 - 7) + "Edgetok"        # ends exactly at the edge, byte 3 S
    t1 = "edgetok later1 " + TC._filler(6 * S) + "EDGETOK early2 end"
    case = Case("sightings_on_both_sides_of_a_slice_edge_and_far_apart", [t0, t1], known, lambda: True)

    def holds():
        at = sightings(case, "edgetok")
        return len(TC.enc(t0)) == 3 * S and [a // S for a in at] == [2, 3, 9] and \
            [a // UNIT for a in at] == [11, 12, 36] and at[0] + 7 == 3 * S and at[1] == 3 * S
    return case._replace(holds=holds)


SPELLINGS = "Hello HELLO hello ȺB ⱥb xK xk ẞa ßa hello Ⱥb"      # (U+212A: the Kelvin sign)


def spelling_case() -> Case:
    def holds():
        src = SPELLINGS.split()
        low = TC.backend.tokenize(SPELLINGS)
        return len(set(low)) == 4 and all(len(TC.enc(src[i])) != len(TC.enc(low[i])) for i in (3, 5, 7)) and \
            not TextTable.default().is_exceptional(SPELLINGS)
    return Case("spellings_that_lower_to_one_key_of_another_byte_length", [SPELLINGS, "x HELLO ⱥB"], ["x"], holds)


def empty_vocabulary_case() -> Case:
    texts = ["the first text", "The second text, first of its kind", ""]
    return Case("empty_vocabulary", texts, [], lambda: True)


def all_known_case() -> Case:
    texts = ["ab cd AB", "cd", "", "Ab cD ab"]
    return Case("every_token_known", texts, ["ab", "cd"], lambda: n_unknown_of(Case("", texts, ["ab", "cd"], None)) == 0)


def many_distinct_case() -> Case:
    texts = [" ".join(f"t{i}" for i in range(a, a + 1000)) for a in range(0, 70_000, 1000)]
    return Case("70000_distinct_new_tokens", texts, ["t"], lambda: len(set(" ".join(texts).split())) == 70_000)


def repeated_case() -> Case:
    others = [f"o{i}" for i in range(50)]
    spell = ("rep", "Rep", "REP")
    texts = [" ".join([spell[i % 3]] * 500 + [others[i % 50]] + [spell[(i + 1) % 3]] * 500) for i in range(100)]

    def holds():
        toks = [tok for t in texts for tok in TC.backend.tokenize(t)]
        return toks.count("rep") == 100_000 and len(set(toks)) == 51
    return Case("one_new_token_100000_times_among_50_others", texts, ["zz"], holds)


def long_token_case() -> Case:
    long = "a" * (2 * S + 500)
    texts = ["q " + long.upper() + " r", long + " " + long + "b q"]
    return Case("new_token_of_2S+500_bytes", texts, ["r"],
                lambda: len(TC.backend.tokenize(texts[0])[1]) == 2 * S + 500 and TC.backend.tokenize(texts[0])[1] == long)


CHAIN_KEYS, CHAIN_REPEATS = 300, 100


def chain_case() -> Case:
    """300 new keys whose home slot in the scratch table (400 occurrences: 1024 slots) is slot 1000: the chain
    wraps past the table's end."""
    cap = scratch_capacity(CHAIN_KEYS + CHAIN_REPEATS)
    keys, slot = TC.colliding_keys(CHAIN_KEYS, cap, slot=cap - 24)
    words = keys + keys[:CHAIN_REPEATS][::-1]
    texts = [" ".join(words[a:a + 40]) for a in range(0, len(words), 40)]

    def holds():
        h = TC.hash_keys([k.encode() for k in keys])
        return cap == 1024 and (TC.home_slot(h, cap) == slot).all() and slot + CHAIN_KEYS > cap and \
            len(set(h.tolist())) == CHAIN_KEYS and n_unknown_of(Case("", texts, [], None)) == CHAIN_KEYS + CHAIN_REPEATS
    return Case("300_new_keys_of_one_scratch_home_slot_in_a_chain_that_wraps", texts, [], holds)


def masked_case() -> Case:
    words = [f"m{i}" for i in range(40)]
    texts = [" ".join(words[:25]), " ".join(words[15:] + words[:5])]

    def holds():
        keys = [w.encode() for w in words]
        return len(set(masked_hashes(keys, 0x7).tolist())) < 40 and len(set(masked_hashes(keys, ALL_ONES).tolist())) == 40
    return Case("40_distinct_tokens_under_hash_mask_7", texts, [], holds, hash_mask=0x7)


MALFORMED = [b"novo um", b"novo \xe2\x82 dois malo", b"dois Novo tres", b"", b"malo"]


def all_cases() -> List[Case]:
    return count_cases() + [slice_case(), spelling_case(), empty_vocabulary_case(), all_known_case(),
                            many_distinct_case(), repeated_case(), long_token_case(), chain_case(), masked_case()]
