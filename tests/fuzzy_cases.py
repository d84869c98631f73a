"""Built cases of the typo-tolerant lexical route (include/thr_hip_fuzzy.h; the definition is
index_text.nearest_terms_host / host_query_row_fuzzy).  A case carries its vocabulary, the document frequencies (or
None), the needles AS THEY STAND IN A TEXT (the device lowers them; ``lowered`` is the host's half), the edit budget,
the number of corrections kept, and ``want``: the property it is named for, written out -- per needle the keys
expected, best first -- or a check of its own.  ``holds()`` holds the definition to that property; the GPU tests hold
the device to the definition."""
import random
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence

from triple_hybrid_rag_amd import _native as N
from triple_hybrid_rag_amd import index_text as IT

S = N.FUZZY_SLICE_BYTES


def lowered(text: str) -> str:
    """The needle the device makes of a one-token text (the cases hold no exceptional character)."""
    return text.lower()


@dataclass
class Case:
    name: str
    vocab: List[str]
    df: Optional[List[int]]
    needles: List[str]
    max_edits: int = 2
    n_best: int = 2
    want: Optional[Dict[str, List[str]]] = None        # needle -> the keys expected, best first
    check: Optional[Callable[["Case", list], bool]] = None
    raw_only: bool = False                             # frequencies no lexical index can hold
    _memo: dict = field(default_factory=dict, repr=False)

    def answers(self, with_df: bool = True, nearest=None) -> List[list]:
        """The definition's answer per needle: [(distance, term id)], best first."""
        nearest = nearest or IT.nearest_terms_host
        df = self.df if with_df else None
        key = (with_df, nearest)
        memo = self._memo.setdefault(key, {})
        out = []
        for x in self.needles:
            w = lowered(x)
            if w not in memo:
                memo[w] = nearest(w, self.vocab, df, self.max_edits, self.n_best)
            out.append(memo[w])
        return out

    def keys_found(self, with_df: bool = True, nearest=None) -> Dict[str, List[str]]:
        return {x: [self.vocab[i] for _, i in a] for x, a in zip(self.needles, self.answers(with_df, nearest))}

    def holds(self) -> bool:
        assert len(set(self.vocab)) == len(self.vocab), self.name
        assert self.df is None or len(self.df) == len(self.vocab), self.name
        ok = True
        if self.want is not None:
            ok = self.keys_found() == self.want
        if self.check is not None:
            ok = ok and self.check(self, self.answers())
        return ok

    def rowptr(self):
        import numpy as np
        return None if self.df is None else np.concatenate([[0], np.cumsum(np.asarray(self.df, dtype=np.int64))])


# ------------------------------------------------------------------ wrong variants (a named case must change)
def nearest_wrong(variant: str):
    """The definition with one rule broken: "bytes" (distances over UTF-8 bytes), "df_ascending", "no_length_rule"
    (every needle gets max_edits)."""
    def nearest(needle, terms, df, max_edits, n_best):
        enc = (lambda s: s.encode("utf-8", "surrogatepass").decode("latin-1")) if variant == "bytes" else (lambda s: s)
        a = enc(needle)
        n = len(a)
        d = max_edits if variant == "no_length_rule" else IT.fuzzy_edits(n, max_edits)
        if n > IT.THR_FUZZY_MAX_LEN or (d == 0 and max_edits > 0 and n < 3):
            return []
        out = []
        for i, key in enumerate(terms):
            k = enc(key)
            if abs(len(k) - n) > d or (df is not None and df[i] <= 0):
                continue
            dist = IT.levenshtein(a, k)
            if dist <= d:
                f = min(df[i], 2 ** 31 - 1) if df is not None else 0
                out.append((dist, f if variant == "df_ascending" else -f, i))
        return [(dist, i) for dist, _, i in sorted(out)[:n_best]]
    return nearest


# ------------------------------------------------------------------ edit kinds
def edit_kind_cases() -> List[Case]:
    vocab = ["contrato", "cast", "zebra"]
    one = ["xcontrato", "contxrato", "contratox",      # insert: first, middle, last
           "ontrato", "conrato", "contrat",             # delete
           "xontrato", "contxato", "contratx"]          # substitute
    want = {x: ["contrato"] for x in one}
    want.update({"xcontrto": ["contrato"],              # two edits of different kinds
                 "contrtao": ["contrato"],              # a transposition costs 2: found from 6 code points on
                 "cats": [], "acst": []})               # ... and not below
    return [Case("edit_kinds", vocab, [3, 2, 1], list(want), want=want)]


# ------------------------------------------------------------------ multi-byte characters
def multibyte_cases() -> List[Case]:
    vocab = ["locação", "中文字典", "ação", "naïve", "abcdef", "señores"]
    want = {"locacao": ["locação"],                     # two substitutions, each changes the byte length
            "locaçao": ["locação"],
            "LOCACAO": ["locação"],                     # lowered on the device
            "LOCAÇÃO": ["locação"],                     # ... onto the key itself: distance 0 through the stand-alone entry
            "中文子典": ["中文字典"],                     # three-byte characters in both
            "中文字": ["中文字典"],
            "açao": ["ação"],
            "naive": ["naïve"],                         # two-byte character in the key only
            "abc中ef": ["abcdef"],                      # three-byte character in the needle only
            "senõres": ["señores"]}                     # in both, at different places: two substitutions
    return [Case("multibyte", vocab, [2, 1, 4, 1, 1, 1], list(want), want=want)]


# ------------------------------------------------------------------ thresholds
K32 = "abcdefghijklmnopqrstuvwxyz012345"
CJK32 = "".join(chr(0x4E00 + i) for i in range(32))
assert len(K32) == 32


def threshold_cases() -> List[Case]:
    n32 = K32[:-1] + "_"                                # 32 code points, the last one substituted
    vocab = ["ab", "abc", "abcd", "abcde", "abcdef", "mnopq", "mnopqr", "mnopqrs", "mnopqrstu", "mnopqrstuv",
             "mnopqrstuvw", K32, n32 + "yz", K32 + "6"]
    df = list(range(len(vocab), 0, -1))                 # the earlier key is the more frequent one
    want = {"ax": [],                                   # 2 code points: no edits
            "abx": ["ab", "abc"],                       # 3: one edit (abcd is two away)
            "abxdy": [],                                # 5: one edit; abcde is two away
            "abxdyf": ["abcdef"],                       # 6: two edits
            n32: [K32, n32 + "yz", K32 + "6"],          # 32 code points: corrected; a key of 34 is reached
            n32 + "9": [],                              # 33: never, though n32 + "yz" is two away
            # 8: keys of n - 2 .. n + 2 are met (one edit first), n - 3 and n + 3 never
            "mnopqrst": ["mnopqrs", "mnopqrstu", "mnopqr", "mnopqrstuv"]}
    two = Case("thresholds_two_edits", vocab, df, list(want), n_best=4, want=want)
    one = Case("thresholds_one_edit", vocab, df, list(want), max_edits=1, n_best=4,
               want=dict(want, **{"abxdyf": [], n32: [K32], "mnopqrst": ["mnopqrs", "mnopqrstu"]}))
    return [two, one]


# ------------------------------------------------------------------ order
def order_cases() -> List[Case]:
    three = ["casa", "cama", "cara"]
    big = 2 ** 31 - 1
    return [
        Case("order_higher_df_wins", three, [5, 9, 7], ["caxa"], n_best=3, want={"caxa": ["cama", "cara", "casa"]}),
        Case("order_lower_id_wins", three, [4, 4, 4], ["caxa"], n_best=3, want={"caxa": ["casa", "cama", "cara"]}),
        Case("order_distance_beats_df", ["contrito", "contrato"], [10 ** 6, 1], ["contrata"],
             want={"contrata": ["contrato", "contrito"]}),
        Case("order_df_clamped", three + ["cana"], [big + 6, 2 ** 33, big, big - 1], ["caxa"], n_best=4, raw_only=True,
             want={"caxa": ["casa", "cama", "cara", "cana"]}),
        Case("order_df_zero_skipped", ["casa", "cama"], [0, 3], ["caxa"], want={"caxa": ["cama"]},
             check=lambda c, a: c.keys_found(with_df=False) == {"caxa": ["casa", "cama"]}),
    ]


# ------------------------------------------------------------------ counts
def count_cases() -> List[Case]:
    out = []
    for n_best in (1, 2, 3, 4):
        vocab, want = ["zebra"], {"qqqqq": [], "zebrx": ["zebra"]}
        for k in (1, 2, 3, 4):
            vocab += [f"w{k}{v}zz" for v in "aeio"[:k]]
        many = [f"b{v}ll" for v in "aeiouyz"[:n_best + 3]]
        vocab += many
        df = [1 + (7 * i) % 5 for i in range(len(vocab))]
        c = Case(f"counts_n_best_{n_best}", vocab, df, ["qqqqq", "zebrx", f"w{n_best}xzz", "bxll"], n_best=n_best)

        def check(case, answers, n_best=n_best, many=many):
            found = case.keys_found()
            full = IT.nearest_terms_host("bxll", case.vocab, case.df, 2, 99)
            return (found["qqqqq"] == [] and found["zebrx"] == ["zebra"]
                    and sorted(found[f"w{n_best}xzz"]) == sorted(f"w{n_best}{v}zz" for v in "aeio"[:n_best])
                    and len(full) == n_best + 3 and len(found["bxll"]) == n_best and set(found["bxll"]) <= set(many))
        c.check = check
        out.append(c)
    # 300 keys at distance 1 of one needle: the insertion under contention
    needle, keys = "abcdefgh", []
    for p in range(len(needle) + 1):
        for ch in "abcdefghijklmnopqrstuvwxyz":
            for k in (needle[:p] + ch + needle[p:], needle[:p] + ch + needle[p + 1:] if p < len(needle) else None):
                if k and k != needle and k not in keys:
                    keys.append(k)
    keys = keys[:300]
    df = [1 + (7 * i) % 13 for i in range(300)]

    def crowd(case, answers):
        best = sorted(range(300), key=lambda i: (-case.df[i], i))[:4]
        return [i for _, i in answers[0]] == best and all(d == 1 for d, _ in answers[0])
    out.append(Case("counts_300_at_distance_1", keys, df, [needle], n_best=4, check=crowd))
    return out


# ------------------------------------------------------------------ geometry
def _filler(i: int) -> str:
    return f"{i:07d}"          # digits: never within two edits of a needle of letters


def edge_case(end: int, target: str, needle: str, name: str) -> Case:
    """A vocabulary whose key ``target`` ends at byte ``end`` of the key store (so it crosses, touches or clears the
    edge of a staged slice), with a neighbour right behind it."""
    start = end - len(target.encode())
    k, rest = divmod(start, 7)
    vocab = [_filler(i) for i in range(k - 1)] + ["9" * (7 + rest)] + [target, needle + "zz"]
    assert sum(len(t.encode()) for t in vocab[:-2]) == start
    return Case(name, vocab, None, [needle], want={needle: [target, needle + "zz"]})


def geometry_cases() -> List[Case]:
    out = [edge_case(S - 1, "contrato", "contrata", "edge_ends_at_S_minus_1"),
           edge_case(S, "contrato", "contrata", "edge_ends_at_S"),
           edge_case(S + 1, "contrato", "contrata", "edge_ends_at_S_plus_1"),
           edge_case(S + 3, "locação", "locacao", "edge_crossed_by_a_two_byte_character"),
           # 34 three-byte characters that begin on the last byte of a slice: the whole halo
           edge_case(S - 1 + 102, CJK32 + "乐乑", CJK32, "edge_crossed_by_the_longest_key")]
    out.append(Case("one_key", ["contrato"], [1], ["contrata", "zebra"], want={"contrata": ["contrato"], "zebra": []}))
    out.append(Case("long_key_between", ["contrato", "x" * (2 * S + 500), "contrata"], [1, 1, 1], ["contratx"],
                    want={"contratx": ["contrato", "contrata"]}))
    # 70 000 keys, the answers among the 40 highest ids
    base = "administracao"
    tail = []
    for p in range(len(base)):
        for ch in "xyz":
            k = base[:p] + ch + base[p + 1:]
            if k not in tail:
                tail.append(k)
    tail = tail[:39] + [base + "es"]
    vocab = [_filler(i) for i in range(70000 - 40)] + tail
    df = [1 + i % 3 for i in range(len(vocab))]

    def high(case, answers):
        return all(len(a) == case.n_best and all(i >= 70000 - 40 for _, i in a) for a in answers)
    out.append(Case("70000_keys_answers_last", vocab, df, [base, "administracoa", base + "e"], n_best=4, check=high))
    # 6 000 needles in one call (300 distinct ones: the definition is asked once per distinct needle)
    r = random.Random(11)
    words = ["contrato", "locacao", "documento", "cliente", "assinatura", "pagamento", "imovel", "garantia", "fiador",
             "vistoria", "reajuste", "aluguel", "condominio", "rescisao", "multa", "prazo", "caucao", "seguro",
             "proprietario", "inquilino", "chaves", "entrega", "boleto", "vencimento", "juros", "indice", "clausula",
             "registro", "cartorio", "procuracao", "laudo", "reforma", "benfeitoria", "sublocacao", "renovacao",
             "desocupacao", "notificacao", "cobranca", "atraso", "desconto"]

    def mutate(w):
        p = r.randrange(len(w))
        kind = r.randrange(3)
        ch = r.choice("abcdefghijklmnopqrstuvwxyz")
        return w[:p] + ch + w[p:] if kind == 0 else w[:p] + w[p + 1:] if kind == 1 else w[:p] + ch + w[p + 1:]
    pool = [mutate(mutate(r.choice(words))) for _ in range(300)]
    needles = [r.choice(pool) for _ in range(6000)]
    out.append(Case("6000_needles", words, [1 + (5 * i) % 7 for i in range(len(words))], needles, n_best=3,
                    check=lambda c, a: sum(1 for x in a if x) > 3000))
    return out


def all_cases() -> List[Case]:
    return edit_kind_cases() + multibyte_cases() + threshold_cases() + order_cases() + count_cases() + geometry_cases()


# ------------------------------------------------------------------ the query table
@dataclass
class QueryCase:
    name: str
    vocab: List[str]
    df: List[int]
    texts: List[str]
    max_edits: int = 2
    n_best: int = 2

    def rows(self, conjunctive: bool, tokenize=IT.tokenize):
        ids = {t: i for i, t in enumerate(self.vocab)}
        return [IT.host_query_row_fuzzy(tokenize(t), ids, self.vocab, self.df, self.max_edits, self.n_best, conjunctive)
                for t in self.texts]


def query_cases() -> List[QueryCase]:
    vocab = ["contrato", "contrata", "locação", "casa", "cama", "cara", "documento", "de"]
    df = [5, 2, 3, 5, 9, 7, 1, 4]
    out = [QueryCase("places_and_duplicates", vocab, df, [
        "contrato de locacao",                  # a correction at the token's place
        "documento contratx casa",              # two corrections between known terms, best first
        "contrata contratx",                    # a correction that equals a known term already in the row: no duplicate
        "contratx contrata",                    # ... and the other way round: the correction comes first
        "caxa CAXA caxa",                       # the same unknown token thrice
        "qqqqqq casa",                          # no correction: THR_TEXT_UNKNOWN stays
        "qqqqqq caxa",                          # ... beside a corrected one: both flags
        "casa cama",                            # nothing unknown
        "", "de"])]
    # a row that reaches 32 terms only through corrections, and 33
    many = [f"t{chr(97 + i)}{chr(97 + i)}{chr(97 + i)}kk" for i in range(26)] + [f"u{i}{i}{i}kk" for i in range(8)]
    v2 = many + ["zebra"]
    d2 = [1 + i % 4 for i in range(len(v2))]
    typo = [m[:-1] + "x" for m in many]        # each one edit from its own key alone
    out.append(QueryCase("thirty_two_and_thirty_three", v2, d2, [
        " ".join(typo[:32]), " ".join(typo[:33]), " ".join(many[:16] + typo[16:32]), " ".join(many[:31] + typo[31:33]),
        " ".join(typo[:34]) + " zebra"], n_best=1))
    return out
