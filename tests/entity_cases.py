"""Built cases for the batched entity lookup (thr_entity_match, GpuIndex.find_entities), each named for
the property it has, and the yardstick they are held to.

The yardstick, ``restate``, is the semantics in plain words: per keyword of keywords[:5], in order, the
first max(1, limit // len(keywords)) entities in ascending id whose lower-cased name contains the
lower-cased keyword; those not yet in the list are appended (a duplicate still counts); the list is
cut at 16.  It is ``needle in name`` over the lowered strings and nothing else: no trigram index, no
bytes.  test_entity_match_host.py pins it to GpuIndexClient.find_entities on every case.

A case is (names, keyword lists, limit); ``expected`` computes its answer once per process.
"""
import functools
from dataclasses import dataclass
from typing import Dict, List

import numpy as np

MAX_SEEDS = 16
MAX_KEYWORDS = 5
MAX_NEEDLE = 128
SLICE = 8192        # thr_hip.h THR_ENTITY_SLICE_BYTES (test_entity_match_host.py checks it is)


@dataclass
class Case:
    name: str
    names: List[str]
    queries: List[List[str]]
    limit: int = 20


def first_matches(lowered: List[str], needle: str, per: int) -> List[int]:
    out = []
    for e, nm in enumerate(lowered):
        if needle in nm:
            out.append(e)
            if len(out) == per:
                break
    return out


def restate(lowered: List[str], keywords: List[str], limit: int, first=first_matches) -> List[int]:
    if not keywords or not lowered:
        return []
    per = max(1, limit // len(keywords))
    found: List[int] = []
    for kw in keywords[:MAX_KEYWORDS]:
        for e in first(lowered, kw.lower(), per):
            if e not in found:
                found.append(e)
    return found[:MAX_SEEDS]


def expected_lists(case: Case) -> List[List[int]]:
    """restate() of every query of the case; a (needle, per) pair and a whole query are looked up once."""
    lowered = [nm.lower() for nm in case.names]
    memo: Dict[tuple, List[int]] = {}

    def first(lw, needle, per):
        if (needle, per) not in memo:
            memo[(needle, per)] = first_matches(lw, needle, per)
        return memo[(needle, per)]
    whole: Dict[tuple, List[int]] = {}
    out = []
    for kws in case.queries:
        key = tuple(kws)
        if key not in whole:
            whole[key] = restate(lowered, kws, case.limit, first)
        out.append(whole[key])
    return out


def as_tables(lists: List[List[int]]):
    """-> (seeds int32 [nq, 16] padded with -1, counts int32 [nq])."""
    seeds = np.full((len(lists), MAX_SEEDS), -1, dtype=np.int32)
    for q, row in enumerate(lists):
        seeds[q, :len(row)] = row
    return seeds, np.array([len(r) for r in lists], dtype=np.int32)


def name_offsets(names: List[str]) -> List[int]:
    """Byte offset of every name in the packed store (lowered UTF-8, one separator behind each)."""
    off, at = [], 0
    for nm in names:
        off.append(at)
        at += len(nm.lower().encode("utf-8", "surrogatepass")) + 1
    return off + [at]


# ------------------------------------------------------------------------------------------ boundaries
LONG128 = "w" * 127 + "k"


def boundaries() -> Case:
    fill = "q" * 15                                   # 16 bytes with its separator
    names = ["firstname alpha"] + [fill] * 510        # 511 * 16 = 8176 bytes
    names.append("p" * 15 + "zboundary")              # "zboundary" starts in the LAST byte of slice 0
    names += [fill] * 511
    names.append("r" * 6 + LONG128)                   # 128 bytes starting in the last byte of slice 1
    names += ["", "exactname", "ab", "cd", "", "", "twice twice", fill, "omega lastbyte"]
    off = name_offsets(names)
    assert off[511] + 15 == SLICE - 1 and off[511 + 512] + 6 == 2 * SLICE - 1, "the store is built around the slice size"
    assert off[-1] > 2 * SLICE
    queries = [["zboundary"], ["boundary"], [LONG128], ["w" * 127], ["w" * 128], ["firstname"], ["lastbyte"],
               ["omega lastbyte"], ["exactname"], ["exactnamea"], ["xexactname"], ["bc"], ["ab"], ["cd"], ["abcd"], [""],
               ["twice"], ["e"], ["lastbytex"], ["zboundary", LONG128, "lastbyte", "firstname", ""], ["q" * 15],
               ["q" * 16], ["pz"], ["rw"]]
    return Case("boundaries", names, queries)


# --------------------------------------------------------------------------------------------- lengths
def lengths() -> Case:
    names = ["alpha beta", "m" * 127, "m" * 127 + "n", "gamma", "abcde", "abcd", "abc", "ab", "a", "", "xabcdex"]
    needles = ["", "a", "ab", "abc", "abcd", "abcde", "m" * 127, "m" * 127 + "n", "m" * 128, "m" * 126 + "nn",
               "n", "mn", "mmn", "abcdex", "e", "de", "cde"]
    assert sorted({len(n) for n in needles}) == [0, 1, 2, 3, 4, 5, 6, 127, 128]
    return Case("lengths", names, [[n] for n in needles] + [["a", "ab", "abc"]])


# ------------------------------------------------------------------------------------------------ text
def text() -> Case:
    names = ["São Paulo", "Fundação Getulio", "İstanbul", "istanbul", "AÇÃO", "sao paulo", "Ação Direta",
             "ß-carotene", "STRASSE", "£ sterling", "ISTANBUL", "coração", "Ç", "naïve café"]
    needles = ["SÃO", "ção", "são", "sao", "ã", "Ã", "ão", "İstanbul", "İ", "i̇", "istanbul", "ISTANBUL", "£", "ă", "â",
               "ç", "Ç", "ß", "ss", "é", "ï", "̃", "ăo", "oã", "a£", "ãa", "çã"]
    return Case("text", names, [[n] for n in needles] + [["SÃO", "ção", "İstanbul"], ["ç", "ã", "ß", "é", "i̇"]])


# ------------------------------------------------------------------------------------------- many hits
N_MANY = 70_000
SPREAD16 = [int(i * (N_MANY - 1) / 15) for i in range(16)]            # ids 0 .. 69 999, both ends included
SPREAD17 = [int(3 + i * (N_MANY - 10) / 16) for i in range(17)]


def many_hits() -> Case:
    in16, in17 = set(SPREAD16), set(SPREAD17)
    names = []
    for e in range(N_MANY):
        nm = f"ent{e % 977} node{e}"
        if e >= N_MANY - 40:
            nm += " zzhigh"
        if e in in16:
            nm += " sixteenx"
        if e in in17:
            nm += " seventeeny"
        names.append(nm)
    names[41_234] = "aaaaaaaa ent"                                    # contains "aaa" six times
    assert len(in16) == 16 and len(in17) == 17 and 41_234 not in in16 | in17
    return Case("many_hits", names, [["ent"], ["zzhigh"], ["sixteenx"], ["seventeeny"], ["aaa"], ["aaaaaaaa"],
                                     ["sixteenx", "seventeeny"], ["e"], ["node69999"], ["node6999"], [""],
                                     ["zzhigh", "aaa", "sixteenx"]], limit=100)


# ---------------------------------------------------------------------------------------- needle table
N_TABLE = 1200


def table_names():
    return [f"entity{e}" for e in range(N_TABLE)]


def shared_prefix() -> Case:
    """300 needles with the same first three bytes."""
    return Case("shared_prefix", table_names(), [[f"entity{j}"] for j in range(1, 301)])


def six_thousand_needles() -> Case:
    """6 000 distinct needles in one call, five to a query."""
    needles = [f"entity{j}" for j in range(3000)] + [f"y{j}" for j in range(3000)]
    assert len(set(needles)) == 6000
    return Case("six_thousand_needles", table_names(), [needles[i:i + 5] for i in range(0, 6000, 5)])


def same_needle_2048() -> Case:
    return Case("same_needle_2048", table_names(), [["entity7"]] * 2047 + [["tity11", "entity7"]])


# ----------------------------------------------------------------------------- per / dedup / truncation
def per_names():
    names = []
    for e in range(38):
        tag = "groupa" if e < 10 else "fiveb" if e < 15 else "sixb" if e < 21 else "sevenb" if e < 28 else "rest"
        names.append(f"item{e:02d} common {tag}")
    return names + ["tag6 only", "tag7 only"]


KWS7 = ["common", "item0", "item1", "item2", "item3", "tag6", "tag7"]


def per_limit20() -> Case:
    queries = [KWS7[:k] for k in range(1, 8)]                          # per = 20, 10, 6, 5, 4, 3, 2
    queries += [[], ["common", "item", "item1", "item3"], [],          # "item": its first 5 are all duplicates
                ["groupa", "fiveb"], ["groupa", "sixb"], ["groupa", "sevenb"], [], [],
                ["tag6"], ["TAG7", "Tag6"], ["nothing"], ["nothing", "tag6"]]
    return Case("per_limit20", per_names(), queries, limit=20)


def per_limit3() -> Case:
    return Case("per_limit3", per_names(), [["item1", "item2", "common", "tag6", "tag7"], ["common"],
                                            ["item3", "item3"], KWS7], limit=3)


def per_limit100() -> Case:
    return Case("per_limit100", per_names(), [["common"], ["item1", "common"], ["tag7", "rest", "common"], [""]], limit=100)


def three_queries() -> Case:
    """A batch of three: a full list, a short one and a query without keywords."""
    return Case("three_queries", per_names(), [["common", "tag7"], ["sixb", "item2", "nothing"], []])


def single_query() -> Case:
    return Case("single_query", per_names(), [["item2", "tag6"]])


# -------------------------------------------------------------------------------------- launch geometry
def launch_geometry() -> Case:
    """65 600 queries of cheap needles: more than 2^16 of them, not a multiple of the block size."""
    lists = [["item0"], ["tag6", "tag7"], [], ["groupa"], ["item3", "item1", "item2"], ["only"], ["zz"], ["sixb", "common"]]
    return Case("launch_geometry", per_names(), [lists[q % len(lists)] for q in range(65_600)])


BUILDERS = (boundaries, lengths, text, many_hits, shared_prefix, six_thousand_needles, same_needle_2048,
            per_limit20, per_limit3, per_limit100, single_query, three_queries, launch_geometry)
CASE_NAMES = tuple(b.__name__ for b in BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    c = dict(zip(CASE_NAMES, BUILDERS))[name]()
    assert c.name == name
    return c


@functools.lru_cache(maxsize=None)
def expected(name: str):
    """-> (lists, seeds int32 [nq, 16], counts int32 [nq]) of the case, computed once; not to be changed."""
    lists = expected_lists(case(name))
    seeds, counts = as_tables(lists)
    seeds.setflags(write=False)
    counts.setflags(write=False)
    return lists, seeds, counts
