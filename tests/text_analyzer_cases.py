"""Built cases of the token-level analysis (stop list + suffix stemming), each named for its property, with
the plain restatement the device is held to.  ``restated_tokens`` is index_text.Analyzer.tokenize derived
again from the issue's words (longest suffix of a step among those that leave min_stem code points; stop check
on the whole lowered token before stemming); ``first_match_tokens`` is the DEVICE's rule for a hand-built table
(the first rule in table order).  No GPU, no library call: tests/test_text_analyzer_host.py checks the cases'
properties, tests/test_gpu_text_analyzer.py runs them."""
import random
import struct
from typing import Callable, Dict, List, NamedTuple, Sequence, Tuple

import numpy as np

import text_cases as TC
from triple_hybrid_rag_amd.index_text import TextTable

S = TC.S
enc = TC.enc
Steps = Sequence[Sequence[Tuple[str, int]]]


# ------------------------------------------------------------------ the plain restatement
def restated_tokens(table: TextTable, stop, steps: Steps, text: str) -> List[str]:
    out = []
    for tok in table.tokenize(text):
        if tok in stop:
            continue
        for step in steps:
            best = ""
            for suffix, min_stem in step:
                if tok.endswith(suffix) and len(tok) - len(suffix) >= min_stem and len(suffix) > len(best):
                    best = suffix
            tok = tok[:len(tok) - len(best)]
        out.append(tok)
    return out


def first_match_tokens(table: TextTable, stop, steps: Steps, text: str) -> List[str]:
    """The device's semantics for a table as it stands: per step the FIRST rule in table order that matches."""
    out = []
    for tok in table.tokenize(text):
        if tok in stop:
            continue
        for step in steps:
            for suffix, min_stem in step:
                if tok.endswith(suffix) and len(tok) - len(suffix) >= min_stem:
                    tok = tok[:len(tok) - len(suffix)]
                    break
        out.append(tok)
    return out


def rule_table(steps: Steps) -> Tuple[List[int], np.ndarray]:
    """The header's layout written out by hand, IN THE ORDER GIVEN: { uint16 tail[8] (from the suffix's end);
    int32 len; int32 min_stem } -> (step_ptr, uint8 [24 * n])."""
    step_ptr, blob = [0], b""
    for step in steps:
        for suffix, min_stem in step:
            tail = [ord(c) for c in reversed(suffix)] + [0] * (8 - len(suffix))
            blob += struct.pack("<8Hii", *tail, len(suffix), min_stem)
        step_ptr.append(len(blob) // 24)
    return step_ptr, np.frombuffer(blob, dtype=np.uint8).copy()


class Expect(NamedTuple):
    doc: np.ndarray
    term: np.ndarray          # -1 for a stem outside the vocabulary
    n_tokens: np.ndarray
    flags: np.ndarray
    unknown: List[str]        # the unknown stems of the plain texts, in row order
    numbered: np.ndarray      # term with the unknown stems numbered from len(ids) in order of first appearance
    new_terms: List[str]


def expect_rows(texts: Sequence[str], ids: Dict[str, int], tokens: Callable[[str], List[str]], table: TextTable) -> Expect:
    doc, term, n_tokens, flags, unknown, numbered = [], [], [], [], [], []
    grown = dict(ids)
    for d, t in enumerate(texts):
        toks = tokens(t)
        exc = table.is_exceptional(t)
        for tok in toks:
            doc.append(d)
            term.append(ids.get(tok, -1))
            if tok not in ids and not exc:
                unknown.append(tok)
            numbered.append(grown.setdefault(tok, len(grown)))
        n_tokens.append(len(toks))
        flags.append(1 if exc else 0)
    i32 = np.int32
    return Expect(np.asarray(doc, i32), np.asarray(term, i32), np.asarray(n_tokens, i32), np.asarray(flags, i32), unknown,
                  np.asarray(numbered, i32), list(grown)[len(ids):])


def expect_query_table(texts, ids, tokens, table):
    """TC.expect_query_table with the analysed tokens: _query_terms' loop over stems."""
    class _T:
        tokenize = staticmethod(tokens)
        is_exceptional = staticmethod(table.is_exceptional)
    return TC.expect_query_table(texts, ids, _T)


# ------------------------------------------------------------------ cases
class Case(NamedTuple):
    name: str
    stop: Tuple[str, ...]
    steps: Steps
    texts: List[str]
    vocab: List[str]              # of STEMS; what is missing comes back as unknown
    holds: Callable[[], bool]
    table_order: bool = False     # the rule table is handed over as written (not longest first): first match wins

    def tokens(self, table: TextTable) -> Callable[[str], List[str]]:
        fn = first_match_tokens if self.table_order else restated_tokens
        return lambda text: fn(table, set(self.stop), self.steps, text)


def _tok(table, case, text):
    return case.tokens(table)(text)


D = TextTable.default
PLURAL = (("s", 2), ("es", 2), ("ões", 2))


def geometry_cases() -> List[Case]:
    out = []
    c = Case("exactly_len_plus_min_stem_and_one_short", (), [[("ção", 3)]], ["locação abcção abção ção xção"],
             ["loca", "abc"], lambda: True)
    out.append(c._replace(holds=lambda c=c: _tok(D(), c, c.texts[0]) == ["loca", "abc", "abção", "ção", "xção"]))
    c = Case("nested_suffixes_in_one_step", (), [PLURAL], ["locações flores casas es ões bs"], ["locaç", "flor"], lambda: True)
    out.append(c._replace(holds=lambda c=c: _tok(D(), c, c.texts[0]) == ["locaç", "flor", "casa", "es", "õe", "bs"]))
    c = Case("two_step_cascade_exposes_the_next_suffix", (), [[("s", 3)], [("mente", 3)]], ["claramentes claramente mentes"],
             ["clara"], lambda: True)
    out.append(c._replace(holds=lambda c=c: _tok(D(), c, c.texts[0]) == ["clara", "clara", "mente"]
                          and restated_tokens(D(), (), [[("mente", 3)], [("s", 3)]], "claramentes") == ["claramente"]))
    c = Case("first_match_in_table_order_is_not_the_longest", (), [[("s", 2), ("es", 2), ("ões", 2)]], ["flores locações"],
             ["flore"], lambda: True, table_order=True)
    out.append(c._replace(holds=lambda c=c: _tok(D(), c, c.texts[0]) == ["flore", "locaçõe"]
                          and restated_tokens(D(), (), c.steps, c.texts[0]) == ["flor", "locaç"]))
    c = Case("suffix_of_8_code_points", (), [[("abcdefgh", 1), ("çãoçãoçã", 2)]], ["xabcdefgh abcdefgh zzçãoçãoçã zçãoçãoçã"],
             ["x"], lambda: True)
    out.append(c._replace(holds=lambda c=c: _tok(D(), c, c.texts[0]) == ["x", "abcdefgh", "zz", "zçãoçãoçã"]))
    four = [[(ch * 8, 1)] for ch in "abcd"]
    word = "x" + "d" * 8 + "c" * 8 + "b" * 8 + "a" * 8
    c = Case("four_steps_strip_32_code_points", (), four, [word + " " + word[1:] + " y" + word], ["x"], lambda: True)
    out.append(c._replace(holds=lambda c=c: _tok(D(), c, c.texts[0]) == ["x", "d" * 8, "yx"]))
    c = Case("a_token_that_is_entirely_one_suffix", (), [[("mente", 1)]], ["mente amente"], ["mente"], lambda: True)
    out.append(c._replace(holds=lambda c=c: _tok(D(), c, c.texts[0]) == ["mente", "a"]))
    return out


def slice_cases() -> List[Case]:
    out = []
    steps = [[("ções", 2), ("中文", 2)]]
    word = "locações"                       # bytes: l o c a ç(2) õ(2) e s = 10
    for delta in (-1, 0, 1):                # the token's last byte at S - 1 + delta ... (ends at S - 1, S, S + 1)
        t = TC._filler(S + delta - len(enc(word))) + word + " casa"
        out.append(Case(f"token_ends_at_S{delta:+d}", (), steps, [t], ["loca"],
                        lambda t=t, delta=delta: enc(t).find(enc(word)) + len(enc(word)) == S + delta))
    for ch, k in (("ç", 1), ("õ", 1), ("中", 1), ("中", 2), ("文", 1), ("文", 2)):
        w = "locações" if ch in "çõ" else "abc中文"
        at = enc(w).find(enc(ch))
        t = TC._filler(S - k - at) + w + " q"
        out.append(Case(f"suffix_character_{ch}_cut_{k}_bytes_before_S", (), steps, [t], ["loca"],
                        lambda t=t, ch=ch, k=k: enc(t)[S - k:S - k + len(enc(ch))] == enc(ch)))
    long = "a" * (2 * S + 500 - len(enc("ções"))) + "ções"
    out.append(Case("one_token_of_2S+500_bytes_with_a_suffix", (), steps, [" q " + long + " r", long], [long[:-4]],
                    lambda: len(enc(long)) == 2 * S + 500))
    c = Case("text_boundary_behind_a_suffix_and_behind_a_stop_word", ("de", "as"), steps, ["as locações", "de casa de", "locações", "as"],
             ["loca", "casa"], lambda: True)
    out.append(c._replace(holds=lambda c=c: b"".join(map(enc, c.texts)) == enc("as locaçõesde casa delocaçõesas")
                          and [_tok(D(), c, t) for t in c.texts] == [["loca"], ["casa"], ["loca"], []]))
    return out


def lowering_cases() -> List[Case]:
    # the Kelvin sign 3 -> 1 bytes, A with stroke 2 -> 3, capital sharp s 3 -> 2 (holds() checks that no editor folded them)
    K, A, SS = "K", "Ⱥ", "ẞ"
    steps = [[("ções", 2), ("ßk", 2)]]
    t = f"{K}a{A}{SS}ções abc{SS}{K} {K}a x{SS}{K} {K}as"
    c = Case("lowering_changes_length_in_the_prefix_in_the_suffix_and_in_a_stop_word", ("ka",), steps, [t], ["abc"], lambda: True)
    return [c._replace(holds=lambda c=c: _tok(D(), c, t) == ["kaⱥß", "abc", "xßk", "kas"] and "ka" not in t
                       and "K" not in t and [len(enc(a)) - len(enc(a.lower())) for a in (K, A, SS)] == [2, -1, 1])]


def stop_cases() -> List[Case]:
    out = []
    steps = [[("s", 3)], [("er", 3), ("eu", 3)]]
    c = Case("stop_words_first_last_alone_and_around_stems", ("de", "a", "com", "comer", "casas"),
             steps, ["de casa a", "a de", "casa", "de", "casas casa comer comeu com", ""], ["casa", "com"], lambda: True)
    out.append(c._replace(holds=lambda c=c: [_tok(D(), c, t) for t in c.texts] ==
                          [["casa"], [], ["casa"], [], ["casa", "com"], []]))
    r = random.Random(7)
    pieces = ["", "a", "b", " ", ",", "ab", "a b", "é", "éa", "中", "abs", " a ", "b,", "as", "bs"]
    tiny = [r.choice(pieces) for _ in range(70_000)]
    out.append(Case("70000_texts_of_0_to_3_bytes", ("a", "é", "as"), [[("s", 2)]], tiny, ["b", "ab"],
                    lambda: len(tiny) == 70_000 and max(len(enc(t)) for t in tiny) == 3))
    keys, slot = TC.colliding_keys(300, 1024, slot=1000)
    stop = tuple(keys + [f"other{i}" for i in range(100)])
    probe = " ".join(keys[:150] + ["k", keys[0] + "x", "kept"] + keys[150:] + ["other7", "other100"])
    out.append(Case("300_stop_keys_of_one_home_slot_in_a_chain_that_wraps", stop, [], [probe], ["kept", "k"],
                    lambda: slot + 300 > 1024 and (TC.home_slot(TC.hash_keys([k.encode() for k in keys]), 1024) == slot).all()
                    and 2 * len(stop) <= 1024 < 4 * len(stop)))
    return out


def unknown_cases() -> List[Case]:
    steps = [[("s", 3)], [("ando", 3), ("ou", 3), ("ar", 3)]]
    texts = ["falando falou de falar", "", "falas Falando cantar", "de de", "cantou novo"]
    c = Case("two_unknown_tokens_with_one_stem", ("de",), steps, texts, [], lambda: True)
    return [c._replace(holds=lambda c=c: [_tok(D(), c, t) for t in c.texts] ==
                       [["fal", "fal", "fal"], [], ["fala", "fal", "cant"], [], ["cant", "novo"]])]


def all_cases() -> List[Case]:
    return geometry_cases() + slice_cases() + lowering_cases() + stop_cases() + unknown_cases()


# ------------------------------------------------------------------ the shipped example's listed pairs
PT_SAME = """documento documentos|locação locações|casa casas|carro carros|flor flores|mulher mulheres|cliente clientes|
homem homens|animal animais|jornal jornais|alemão alemães|lei leis|mão mãos|vez vezes|contrato contratos|
menino menina|aluno aluna|claro clara|novo nova|bonito bonita|advogado advogada|
clara claramente|lenta lentamente|certa certamente|nova novamente|
ação ações|reunião reuniões|opção opções|informação informações|livro livrinho|casa casinha|
falar falou|falar falando|falar falado|falar falava|falar falaram|falar falamos|falar falei|falar falavam|
comer comeu|comer comendo|comer comido|comer comia|partir partiu|partir partindo|partir partido|partir partiram"""
PT_APART = """casa carro|documento locação|mar mau|rio rua|ler lar|sal sol|par pai|livro lei|contrato contraste|cidade cliente|
porta ponte|banco barco|mesa mês|pagar pegar|falar filar|comer correr|partir portar|ação acordo|flor flauta|homem hora|
animal anel|jornal jogo|reunião região|opção oração|lento lindo|claro caro"""


def pairs(block: str) -> List[Tuple[str, str]]:
    return [tuple(p.split()) for p in block.replace("\n", "").split("|")]


def portuguese_corpus(n: int, seed: int = 5) -> List[str]:
    """n short chunks of Portuguese-like text: content words in several inflections between function words."""
    r = random.Random(seed)
    content = [w for p in pairs(PT_SAME) for w in p] + ["pagamento", "aluguel", "prazo", "multa", "imóvel", "fiador"]
    glue = ["de", "a", "o", "que", "para", "com", "não", "os", "das", "em", "foi", "são"]
    out = []
    for _ in range(n):
        words = []
        for _ in range(r.randint(3, 14)):
            words.append(r.choice(glue) if r.random() < 0.45 else r.choice(content))
        text = " ".join(words)
        out.append(text.capitalize() + r.choice([".", "", "!", " —"]))
    return out
