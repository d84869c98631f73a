"""The batched entity lookup without a GPU: the packer of the name store, the host half of
GpuIndex.find_entities (lowering, de-duplication, ``per``, padding, the over-long keyword), the refusals
of thr_entity_match before any launch, and the yardstick of tests/entity_cases.py pinned to the function
the project already ships, GpuIndexClient.find_entities."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import triple_hybrid_rag_amd as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entity_cases as EC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = T._native


def header_define(name):
    text = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    m = re.search(r"#define\s+" + name + r"\s+(\(?[0-9 <]+\)?)", text)
    assert m, f"{name} is not defined in thr_hip.h"
    return eval(m.group(1))


def declared_args(name):
    text = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in thr_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_constants_equal_the_headers_and_the_entry_points_are_bound():
    for name in ("THR_ENTITY_MAX_NEEDLE", "THR_ENTITY_MAX_KEYWORDS", "THR_ENTITY_MAX_QUERIES", "THR_ENTITY_SLICE_BYTES",
                 "THR_GRAPH_MAX_SEEDS"):
        assert getattr(N, name) == header_define(name), name
    assert (N.THR_ENTITY_MAX_NEEDLE, N.THR_ENTITY_MAX_KEYWORDS) == (128, 5) == (EC.MAX_NEEDLE, EC.MAX_KEYWORDS)
    assert N.THR_ENTITY_SLICE_BYTES == EC.SLICE and N.THR_GRAPH_MAX_SEEDS == EC.MAX_SEEDS
    lib = N.load()
    for name in ("thr_entity_match", "thr_entity_match_workspace_bytes"):
        assert hasattr(lib, name) and name in N.EXPORTED_SYMBOLS
        assert len(N._SIGNATURES[name][1]) == declared_args(name)
    assert lib.thr_abi_version() == N.ABI_VERSION == 9


def test_refusals_of_the_c_entry_need_no_gpu():
    lib = N.load()
    P = C.c_void_p(4096)       # (never dereferenced: every call below is refused before a launch)

    def match(name_bytes=P, name_ptr=P, E=100, needles=P, lens=P, M=3, qn=P, per=P, nq=2, seeds=P, counts=P, ws=P,
              wsb=1 << 30):
        return lib.thr_entity_match(name_bytes, name_ptr, E, needles, lens, M, qn, per, nq, seeds, counts, ws, wsb, None)
    for arg in ("name_bytes", "name_ptr", "needles", "lens", "qn", "per", "seeds", "counts", "ws"):
        assert match(**{arg: None}) == -1, arg
    assert match(E=0) == -1 and match(E=-5) == -1 and match(E=2 ** 31) == -1
    assert match(M=0) == -1 and match(M=11) == -1 and match(M=-1) == -1     # 1 .. 5 * n_queries
    assert match(nq=0) == -1 and match(nq=(1 << 20) + 1, M=1) == -1 and match(nq=-3) == -1
    assert match(name_bytes=C.c_void_p(4100)) == -1                         # 16-byte alignment
    assert match(needles=C.c_void_p(4098)) == -1 and match(ws=C.c_void_p(4100)) == -1   # 4 and 8 bytes
    assert match(wsb=0) == -3 and match(M=10, wsb=64) == -3
    w = lib.thr_entity_match_workspace_bytes
    assert match(wsb=w(100, 3, 2) - 1) == -3
    assert w(0, 3, 2) == 0 == w(100, 0, 2) == w(100, 11, 2) == w(100, 1, 0) == w(100, 1, (1 << 20) + 1)
    # 16 ids and a chain link per needle, a table of at least two slots of 8 bytes per needle, the filter
    assert w(100, 6000, 2048) >= 6000 * (64 + 4 + 16) + 8192
    assert w(100, 6000, 2048) > w(100, 300, 2048) >= w(100, 1, 2048) > 0
    assert w(100, 5 << 20, 1 << 20) > (5 << 20) * 84
    assert w(2_500_000, 300, 2048) == w(100, 300, 2048)                      # (nothing is kept per entity)


def test_pack_entity_names():
    from triple_hybrid_rag_amd.index_entities import pack_entity_names
    names = ["São Paulo", "", "İstanbul", "ab", "lone \ud800 surrogate", "Z"]
    blob, ptr = pack_entity_names(names)
    assert blob.dtype == np.uint8 and ptr.dtype == np.int64 and ptr.shape == (len(names) + 1,) and ptr[0] == 0
    raw = blob.tobytes()
    for e, nm in enumerate(names):
        enc = nm.lower().encode("utf-8", "surrogatepass")
        assert raw[ptr[e]:ptr[e + 1] - 1] == enc and raw[ptr[e + 1] - 1] == 0xFF, (e, nm)
        assert 0xFF not in enc
    assert ptr.tolist() == EC.name_offsets(names)
    assert len("İstanbul".lower().encode()) == len("İstanbul".encode()) + 1     # lowering changed the length
    assert b"\xed\xa0\x80" in raw                                                # the surrogate passed
    assert len(raw) - ptr[-1] >= N.THR_ENTITY_MAX_NEEDLE and set(raw[ptr[-1]:]) == {0xFF}
    blob0, ptr0 = pack_entity_names([])
    assert ptr0.tolist() == [0] and len(blob0) >= N.THR_ENTITY_MAX_NEEDLE and set(blob0.tolist()) == {0xFF}


def test_set_entity_names_checks_the_count_against_the_graph():
    torch = pytest.importorskip("torch")
    idx = T.GpuIndex.__new__(T.GpuIndex)      # (no device: the check comes before anything is uploaded)
    assert idx.entities is None
    idx.graph = dict(ent_rowptr=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="2 names for the 3 entities"):
        idx.set_entity_names(["a", "b"])
    with pytest.raises(N.NativeError, match="no entity names"):
        idx.find_entities([["a"]])
    # ... and the other way round: names first, then a graph of another entity count
    idx.graph, idx.entities = None, dict(n=2)
    with pytest.raises(ValueError, match="3 entities, the index holds 2 entity names"):
        idx.set_graph(np.zeros(4, dtype=np.int64), None, None, None, None)


def test_plan_needles_lowers_deduplicates_and_divides_by_the_full_count():
    from triple_hybrid_rag_amd.index_entities import plan_needles
    lists = [["Acme", "SÃO"], [], ["acme"], ["a", "b", "c", "d", "e", "f", "g"], ["são", "", "ACME"]]
    p = plan_needles(lists, 20)
    needles = [bytes(p.needles[i, :p.needle_len[i]]) for i in range(len(p.needle_len))]
    assert needles == [b"acme", "são".encode(), b"a", b"b", b"c", b"d", b"e", b""]      # first use order, distinct
    assert p.needles.shape == (8, 128) and p.needles.dtype == np.uint8 and p.needle_len.dtype == np.int32
    assert not p.needles[0, 4:].any()
    assert p.query_needles.dtype == np.int32 and p.query_needles.tolist() == [
        [0, 1, -1, -1, -1], [-1] * 5, [0, -1, -1, -1, -1], [2, 3, 4, 5, 6], [1, 7, 0, -1, -1]]
    assert p.query_per.tolist() == [10, 1, 20, 2, 6] and p.long_rows == []     # 20 // 7 = 2: keywords 6 and 7 count
    assert plan_needles([["x"] * 5], 3).query_per.tolist() == [1]
    assert plan_needles([["x"]], 100).query_per.tolist() == [100]
    empty = plan_needles([[], []], 20)
    assert empty.needles.shape == (0, 128) and (empty.query_needles == -1).all()


def test_over_long_keywords_are_refused_or_routed():
    from triple_hybrid_rag_amd.index_entities import plan_needles
    fits, long = "é" * 64, "é" * 64 + "x"                  # 128 and 129 bytes of UTF-8
    p = plan_needles([[fits], ["a", long], ["b"], ["a", "b", "c", "d", "e", long]], 20)
    assert p.long_rows == [1] and p.needle_len.tolist() == [128, 1, 1, 1, 1, 1]          # the sixth keyword is unused
    assert p.query_needles[1].tolist() == [-1] * 5 and p.query_needles[3].tolist() == [2, 1, 3, 4, 5]
    # the wrapper: ValueError naming the limit before anything touches the device ...
    idx = T.GpuIndex.__new__(T.GpuIndex)
    idx.entities = dict(n=3)
    with pytest.raises(ValueError, match="THR_ENTITY_MAX_NEEDLE = 128"):
        idx.find_entities([["a"], [long]])
    # ... unless long_keywords= resolves those queries: their rows are patched in (no other query names a
    # needle here, so nothing is launched and the tensors may live on the host)
    torch = pytest.importorskip("torch")
    idx.device = torch.device("cpu")
    asked = []

    def host(keywords, limit):
        asked.append((list(keywords), limit))
        return list(range(2, 2 + 3 * len(keywords)))
    seeds, counts = idx.find_entities([[long], [], ["b", long, "c", "d", "e", "f"]], limit=7, long_keywords=host)
    assert asked == [([long], 7), (["b", long, "c", "d", "e", "f"], 7)]
    assert seeds.dtype == torch.int32 and counts.tolist() == [3, 0, 16]
    assert seeds.tolist() == [[2, 3, 4] + [-1] * 13, [-1] * 16, list(range(2, 18))]


def client_over(names):
    from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient
    store = CorpusStore.synthetic(4)
    store.entity_names = list(names)

    class Client(GpuIndexClient):
        def __init__(self):
            self.store = store
    return Client()


@pytest.mark.parametrize("name", EC.CASE_NAMES)
def test_the_restatement_equals_the_shipped_host_function(name):
    """On every built case: restate() == GpuIndexClient.find_entities (trigram index and all), query by
    query -- each distinct keyword list once."""
    case = EC.case(name)
    lists, seeds, counts = EC.expected(name)
    client = client_over(case.names)
    seen = {}
    for kws, exp in zip(case.queries, lists):
        key = tuple(kws)
        if key not in seen:
            seen[key] = client.find_entities(list(kws), case.limit)
        assert seen[key] == exp, (name, kws)
    assert seeds.shape == (len(case.queries), 16) and counts.tolist() == [len(r) for r in lists]
    assert all((seeds[q, len(r):] == -1).all() for q, r in enumerate(lists))


def test_the_cases_have_the_properties_they_are_named_for():
    lists = dict(zip(map(tuple, EC.case("boundaries").queries), EC.expected("boundaries")[0]))
    n = len(EC.case("boundaries").names)
    assert lists[("zboundary",)] == [511] and lists[(EC.LONG128,)] == [1023] == lists[("w" * 127,)]
    assert lists[("w" * 128,)] == [] == lists[("bc",)] == lists[("exactnamea",)] == lists[("lastbytex",)]
    assert lists[("firstname",)] == [0] and lists[("lastbyte",)] == [n - 1] and lists[("",)] == list(range(16))
    many = dict(zip(map(tuple, EC.case("many_hits").queries), EC.expected("many_hits")[0]))
    assert many[("ent",)] == list(range(16)) and many[("zzhigh",)] == list(range(EC.N_MANY - 40, EC.N_MANY - 24))
    assert many[("sixteenx",)] == EC.SPREAD16 and many[("seventeeny",)] == EC.SPREAD17[:16] and many[("aaa",)] == [41_234]
    per = EC.expected("per_limit20")[0]
    q = EC.case("per_limit20").queries
    assert per[q.index(["common", "item", "item1", "item3"])] == [0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 30, 31, 32, 33, 34]
    assert [len(per[q.index(["groupa", t])]) for t in ("fiveb", "sixb", "sevenb")] == [15, 16, 16]
    assert per[q.index([])] == [] and per[q.index(["tag6"])] == [38]
    assert 38 not in per[5] and 39 not in per[6]          # keywords 6 and 7 are not used
    assert EC.expected("per_limit3")[0][0] == [10, 20, 0, 38, 39]
    assert len(EC.case("launch_geometry").queries) == 65_600 and len(EC.case("same_needle_2048").queries) == 2048
    distinct = {k for kws in EC.case("six_thousand_needles").queries for k in kws}
    assert len(distinct) == 6000
    assert len({k[0][:3] for k in EC.case("shared_prefix").queries}) == 1 and len(EC.case("shared_prefix").queries) == 300


def test_the_insertion_walk_commutes_under_any_interleaving():
    """A model of en_insert (csrc/entity.hip) run by many inserters whose memory operations are interleaved at
    random: a look at a slot may be stale (any value the slot held since the inserter started, never smaller than
    the current one), old = atomicMin(slot, v), stop at old == v, carry max(old, v).  Whatever the order, the 16
    slots end as the 16 smallest distinct values, ascending, padded with INT32_MAX."""
    import random
    MAX = 2 ** 31 - 1

    def run(values, rng):
        slots = [MAX] * 16
        history = [list(slots)]

        def inserter(e):
            v, born = e, len(history) - 1
            for i in range(16):
                seen = history[rng.randrange(born, len(history))][i]      # possibly stale
                yield
                if seen == v:
                    return
                if seen < v:
                    continue
                old = slots[i]
                slots[i] = min(old, v)
                history.append(list(slots))
                yield
                if old == v:
                    return
                v = max(old, v)
                if v == MAX:
                    return
        live = [inserter(e) for e in values]
        while live:
            g = rng.choice(live)
            try:
                next(g)
            except StopIteration:
                live.remove(g)
        return slots

    for seed in range(400):
        rng = random.Random(seed)
        values = [rng.randrange(0, 40) for _ in range(rng.randrange(1, 60))]
        want = sorted(set(values))[:16]
        assert run(values, rng) == want + [MAX] * (16 - len(want)), (seed, values)
