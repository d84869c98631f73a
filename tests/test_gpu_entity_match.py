"""The batched entity lookup on the device against the plain restatement of its semantics
(tests/entity_cases.py; test_entity_match_host.py pins that restatement to GpuIndexClient.find_entities):
thr_entity_match through the C ABI on every built case, GpuIndex.find_entities feeding graph_search,
and GpuIndexClient.find_entities_batch against the per-query host function -- before and after save /
load, an append and a delete.  Every comparison is integer equality."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import entity_cases as EC  # noqa: E402


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.parametrize("name", EC.CASE_NAMES)
def test_entity_match_equals_the_restatement(T, name):
    """seeds row for row with the -1 padding, counts, and the same arrays from a second call."""
    from triple_hybrid_rag_amd.index_entities import pack_entity_names, plan_needles
    N = T._native
    case = EC.case(name)
    _, seeds, counts = EC.expected(name)
    blob, ptr = pack_entity_names(case.names)
    plan = plan_needles(case.queries, case.limit)
    assert not plan.long_rows
    args = [dev(a) for a in (blob, ptr, plan.needles, plan.needle_len, plan.query_needles, plan.query_per)]
    got = [tuple(t.cpu().numpy() for t in N.entity_match(*args)) for _ in range(2)]
    (s1, c1), (s2, c2) = got
    assert s1.dtype == np.int32 and c1.dtype == np.int32 and s1.shape == seeds.shape
    bad = np.flatnonzero((s1 != seeds).any(axis=1) | (c1 != counts))
    assert bad.size == 0, (f"{name}: {bad.size} queries differ, first q{bad[0]} {case.queries[bad[0]]}: "
                           f"{s1[bad[0]].tolist()} ({c1[bad[0]]}) != {seeds[bad[0]].tolist()} ({counts[bad[0]]})")
    assert np.array_equal(s1, s2) and np.array_equal(c1, c2), f"{name}: two calls differ"


def test_find_entities_feeds_graph_search(T):
    """GpuIndex.find_entities -> graph_search equals graph_search on the seed table made on the host."""
    import graph_cases as GC
    case = GC.build("seeds_sixteen", "whole")
    base, n = case.window
    idx = T.GpuIndex(doc_base=base)
    idx.n_docs = n
    idx.set_graph(*case.g)
    E = case.n_entities
    names = [f"Thing{e:05d} kind{e % 7} Ação" if e % 3 else f"thing{e:05d} other" for e in range(E)]
    with pytest.raises(ValueError, match="names for the"):
        idx.set_entity_names(names[:-1])
    with pytest.raises(T._native.NativeError, match="no entity names"):
        idx.find_entities([["x"]])
    idx.set_entity_names(names)
    lists = [["thing0000"], ["KIND3", "other"], [], ["ação", "thing00012", "kind5"], [""], ["nothing here"],
             ["thing", "kind", "o", "a", "e", "unused"]]
    lowered = [nm.lower() for nm in names]
    exp = [EC.restate(lowered, kws, 20) for kws in lists]
    assert any(len(r) == 16 for r in exp) and any(0 < len(r) < 16 for r in exp)
    seeds, counts = idx.find_entities(lists)
    host_seeds, host_counts = EC.as_tables(exp)
    assert seeds.is_cuda and seeds.dtype == torch.int32 and counts.dtype == torch.int32
    assert np.array_equal(seeds.cpu().numpy(), host_seeds) and np.array_equal(counts.cpu().numpy(), host_counts)
    a = idx.graph_search(seeds, case.k, case.hops)
    b = idx.graph_search(dev(host_seeds), case.k, case.hops)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert int(a[2].sum()) > 0
    long = "x" * 129
    with pytest.raises(ValueError, match="128"):
        idx.find_entities([["thing"], [long]])
    s2, c2 = idx.find_entities([["thing00001"], [long, "kind"], ["KIND3", "other"]], long_keywords=lambda kws, limit: [7, 5])
    assert s2.cpu().numpy()[:, :3].tolist() == [[1, -1, -1], [7, 5, -1], host_seeds[1, :3].tolist()]
    assert c2.tolist() == [1, 2, int(host_counts[1])]


NAMES = ["São Paulo Energia", "Fundação Getulio Vargas", "Acme Corp", "ACME Holdings", "acme labs", "İstanbul Ticaret",
         "Banco do Brasil", "Banco Central", "banco de dados", "xy", "x", "", "União Química", "Companhia Energética",
         "Energia Solar Ltda", "Solar Corp", "Corporação Alfa", "alfa beta", "Beta Test", "gamma"]
KEYWORDS = [["acme"], ["BANCO", "energia"], ["são", "ção", "corp"], [], ["x", "xy", "a"], ["solar", "alfa", "beta", "gamma", "acme", "banco"],
            [""], ["İstanbul"], ["nobody"], ["e"], ["corp", "CORP", "Corp"], ["é" * 70, "acme"]]


def rows_for(n, d, seed, n_ent):
    rng = np.random.default_rng(seed)
    emb = rng.standard_normal((n, d)).astype(np.float32)
    rows = [{"id": f"c{i}", "parent_id": f"p{i // 4}", "document_id": f"d{i // 16}", "text": f"w{i % 13} w{i % 7} banco",
             "page": 1 + i % 5, "modality": "text", "content_hash": f"h{i}", "embedding_1024": emb[i].tolist()}
            for i in range(n)]
    parents = [{"id": f"p{j}", "text": f"parent {j}", "section_heading": f"S{j}"} for j in range((n + 3) // 4)]
    ents = [{"id": f"e{j}", "name": NAMES[j % len(NAMES)] + (f" {j}" if j >= len(NAMES) else "")} for j in range(n_ent)]
    rels = [{"subject_entity_id": f"e{int(a)}", "object_entity_id": f"e{int(b)}"} for a, b in rng.integers(0, n_ent, (120, 2))]
    mens = [{"entity_id": f"e{int(e)}", "child_chunk_id": f"c{int(c)}", "confidence": float(w)}
            for e, c, w in zip(rng.integers(0, n_ent, 900), rng.integers(0, n, 900), rng.uniform(0.2, 1.0, 900))]
    return rows, parents, ents, rels, mens, emb


def test_client_batch_equals_the_per_query_host_function(T, tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    N = T._native
    n, n0, d, n_ent = 260, 240, 256, 60
    rows, parents, ents, rels, mens, emb = rows_for(n, d, 11, n_ent)
    hi = IB.from_rows(rows[:n0], parents, ents, rels, [m for m in mens if int(m["child_chunk_id"][1:]) < n0])
    client = GpuIndexClient(hi.to_gpu(), hi.store)
    assert client.index.entities is None                     # uploaded on first use
    host = [client.find_entities(k) for k in KEYWORDS]
    assert any(len(r) == 16 for r in host) and host[3] == [] and host[-1] == client.find_entities(["é" * 70, "acme"])
    assert client.find_entities_batch(KEYWORDS) == host
    assert client.index.entities["n"] == n_ent
    for limit in (3, 50):
        assert client.find_entities_batch(KEYWORDS, limit) == [client.find_entities(k, limit) for k in KEYWORDS]

    # device=True feeds retrieve_batch: the same fused ids as with the seed table made on the host
    seeds, counts = client.find_entities_batch(KEYWORDS, device=True)
    assert seeds.is_cuda and seeds.shape == (len(KEYWORDS), N.THR_GRAPH_MAX_SEEDS)
    host_seeds, host_counts = EC.as_tables(host)
    assert np.array_equal(seeds.cpu().numpy(), host_seeds) and np.array_equal(counts.cpu().numpy(), host_counts)
    q = dev(emb[:len(KEYWORDS)] + 0.01)
    terms = dev(np.array([[hi.store.vocab["banco"], hi.store.vocab[f"w{i % 7}"]] for i in range(len(KEYWORDS))], dtype=np.int32))
    a = client.index.retrieve_batch(q, terms, seeds, top_k=10)
    b = client.index.retrieve_batch(q, terms, dev(host_seeds), top_k=10)
    assert torch.equal(a.ids, b.ids) and torch.equal(a.counts, b.counts) and torch.equal(a.scores, b.scores)
    assert int(a.channels["graph"][2].sum()) > 0

    # the names are not touched by an append and a delete: the same answers, the same device copy
    names_ptr = client.index.entities["name_bytes"].data_ptr()
    client.insert_children([dict(r, mentions=[(i % n_ent, 0.5)]) for i, r in enumerate(rows[n0:])])
    assert client.index.n_docs == n and client.find_entities_batch(KEYWORDS) == host
    client.delete_children([f"c{i}" for i in range(5, 40, 3)])
    assert client.find_entities_batch(KEYWORDS) == host and client.index.entities["name_bytes"].data_ptr() == names_ptr

    # save -> load: nothing new on disk, the device copy is rebuilt from the store's names
    path = str(tmp_path / "idx")
    IB.save(hi, path, client.index)
    assert not [f for f in os.listdir(path) if "name_bytes" in f or "name_ptr" in f]
    back = IB.load(path)
    c2 = GpuIndexClient(back.to_gpu(), back.store)
    assert c2.index.entities is None
    assert c2.find_entities_batch(KEYWORDS) == host == [c2.find_entities(k) for k in KEYWORDS]
