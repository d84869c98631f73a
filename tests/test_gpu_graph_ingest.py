"""Graph ingest on the GPU: thr_csr_merge against its numpy restatement on every built case, and an
index that took new entities, relations and mentions against a fresh one built from all the rows --
array for array, result for result -- and against the oracle."""
import asyncio
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_ingest_cases as GC  # noqa: E402
from oracle import thr_oracle as O  # noqa: E402

SENTINEL = -7
GRAPH_KEYS = ("ent_rowptr", "ent_col", "men_rowptr", "men_chunk", "men_conf")


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} != {b.shape} {b.dtype}"
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{what} differs"


def same_results(r1, r2, what):
    for j, (a, b) in enumerate(zip(r1, r2)):
        if isinstance(a, torch.Tensor):
            same(a, b, f"{what}[{j}]")
        else:
            assert a == b, f"{what}[{j}]: {a} != {b}"


def assert_rows(res, expected, what):
    S, I, cnt = (t.cpu().numpy() for t in res[:3])
    for q, (es, ei) in enumerate(expected):
        m = len(ei)
        assert cnt[q] == m, f"{what} q{q}: count {cnt[q]} != {m}"
        assert np.array_equal(I[q, :m], ei), f"{what} q{q}: ids differ"
        assert np.array_equal(S[q, :m].view(np.uint64), es.view(np.uint64)), f"{what} q{q}: scores differ (bits)"


def oracle_rows(g, seeds, hops, n, k, base):
    S, I = O.graph_topk(*g, seeds, hops, n, k, base)
    return list(zip(S, I))


def host_graph(idx):
    return tuple(idx.graph[k].cpu().numpy() for k in GRAPH_KEYS)


# --------------------------------------------------------------------------- thr_csr_merge alone
def _merge(N, case, mode, cap=None, check=True):
    """One call on a case; mode 0 carries the payload as float32 bit patterns.  -> the wrapper's tuple
    + the destinations (pre-filled with a sentinel)."""
    two = mode == 0
    total = len(case.ids_a) + len(case.ids_b)
    cap = total + 37 if cap is None else cap
    o_ids = torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda")
    o_pay = torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32) if two else None
    rows_a = len(case.rowptr_a) - 1
    out = N.csr_merge(dev(case.rowptr_a) if rows_a else None, dev(case.ids_a),
                      dev(case.pay_a).view(torch.float32) if two else None, dev(case.rowptr_b), dev(case.ids_b),
                      dev(case.pay_b).view(torch.float32) if two else None, bool(mode), ids_out=o_ids, pay_out=o_pay,
                      check=check)
    return out, o_ids, o_pay


IN_ORDER = [(n, m) for n in GC.CASE_NAMES for m in (1, 0) if m in GC.cases()[n].modes]
OUT_OF_ORDER = [(n, m) for n in GC.CASE_NAMES for m in (1, 0) if m not in GC.cases()[n].modes]


@pytest.mark.parametrize("name,mode", IN_ORDER, ids=[f"{n}-{'union' if m else 'multiset'}" for n, m in IN_ORDER])
def test_csr_merge_equals_the_numpy_restatement(T, name, mode):
    N = T._native
    case = GC.cases()[name]
    exp_rp, exp_ids, exp_pay, exp_nnz, exp_status = GC.expected(case, mode)
    assert exp_status == 0
    (rp, ids, pay, nnz, status), o_ids, o_pay = _merge(N, case, mode)
    assert (nnz, status) == (exp_nnz, 0) and (pay is None) == (mode == 1)
    assert np.array_equal(rp.cpu().numpy(), exp_rp), "rowptr_out"
    got = o_ids.cpu().numpy()
    assert np.array_equal(got[:nnz], exp_ids), "ids_out"
    assert np.all(got[nnz:] == SENTINEL), "written behind nnz_out"
    if mode == 0:
        gp = o_pay.view(torch.int32).cpu().numpy()
        assert np.array_equal(gp[:nnz], exp_pay), "pay_out (bit patterns)"
        assert np.all(gp[nnz:] == SENTINEL)
    # out_capacity exactly nnz_out is accepted
    (rp2, _, _, nnz2, status2), o2, p2 = _merge(N, case, mode, cap=exp_nnz)
    assert (nnz2, status2) == (exp_nnz, 0) and np.array_equal(o2.cpu().numpy(), exp_ids)
    assert np.array_equal(rp2.cpu().numpy(), exp_rp)
    # one short: reported, nothing out of bounds (the destination lies inside a guarded buffer)
    if exp_nnz > 0:
        guard = torch.full((exp_nnz + 63,), SENTINEL, dtype=torch.int32, device="cuda")
        gpay = torch.full((exp_nnz + 63,), SENTINEL, dtype=torch.int32, device="cuda")
        two = mode == 0
        rows_a = len(case.rowptr_a) - 1
        args = (dev(case.rowptr_a) if rows_a else None, dev(case.ids_a),
                dev(case.pay_a).view(torch.float32) if two else None, dev(case.rowptr_b), dev(case.ids_b),
                dev(case.pay_b).view(torch.float32) if two else None, bool(mode))
        short = dict(ids_out=guard[32:32 + exp_nnz - 1], pay_out=gpay[32:32 + exp_nnz - 1].view(torch.float32) if two else None)
        _, _, _, nnz3, status3 = N.csr_merge(*args, check=False, **short)
        assert nnz3 == exp_nnz and status3 == GC.OVERFLOW
        g = guard.cpu().numpy()
        assert np.all(g[:32] == SENTINEL) and np.all(g[32 + exp_nnz - 1:] == SENTINEL)
        assert np.array_equal(g[32:32 + exp_nnz - 1], exp_ids[:-1])
        if two:
            gp = gpay.cpu().numpy()
            assert np.all(gp[:32] == SENTINEL) and np.all(gp[32 + exp_nnz - 1:] == SENTINEL)
        with pytest.raises(T.NativeError, match="out_capacity"):
            N.csr_merge(*args, **short)


@pytest.mark.parametrize("name,mode", OUT_OF_ORDER, ids=[f"{n}-{'union' if m else 'multiset'}" for n, m in OUT_OF_ORDER])
def test_csr_merge_reports_inputs_that_are_out_of_order(T, name, mode):
    N = T._native
    case = GC.cases()[name]
    want = case.status[mode]
    assert want and GC.expected(case, mode)[4] == want
    (_, _, _, _, status), o_ids, _ = _merge(N, case, mode, check=False)
    assert status == want
    total = len(case.ids_a) + len(case.ids_b)
    assert np.all(o_ids.cpu().numpy()[total:] == SENTINEL)           # undefined, but inside its buffers
    with pytest.raises(T.NativeError, match="build_graph's canonical form"):
        _merge(N, case, mode)


def test_csr_merge_reuses_a_workspace_and_allocates_destinations(T):
    N = T._native
    case = GC.cases()["random"]
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    exp = GC.expected(case, 1)
    rp, ids, pay, nnz, status = N.csr_merge(dev(case.rowptr_a), dev(case.ids_a), None, dev(case.rowptr_b),
                                            dev(case.ids_b), None, True, workspace=ws)
    assert pay is None and nnz == exp[3] and np.array_equal(ids[:nnz].cpu().numpy(), exp[1])
    assert ids.shape[0] == len(case.ids_a) + len(case.ids_b)
    # an int32 payload (opaque 4-byte elements), union mode with a payload
    expp = GC.csr_merge_ref(case.rowptr_a, case.ids_a, case.pay_a, case.rowptr_b, case.ids_b, case.pay_b, 1)
    rp, ids, pay, nnz, _ = N.csr_merge(dev(case.rowptr_a), dev(case.ids_a), dev(case.pay_a), dev(case.rowptr_b),
                                       dev(case.ids_b), dev(case.pay_b), True, workspace=ws)
    assert pay.dtype == torch.int32 and np.array_equal(pay[:nnz].cpu().numpy(), expp[2])
    assert np.array_equal(rp.cpu().numpy(), expp[0])


# --------------------------------------------------------------------------- index level
N0, N1, E0, M1, M2, DIM = 300, 380, 40, 12, 9, 256


def _ent(i):
    return int(i[1:])


def _texts(rows):
    for r in rows:
        i = int(r["id"][1:])
        r["text"] = f"chunk w{i % 7} w{i % 3} x{i % 11}"       # (every term is in the first rows: one vocabulary)
    return rows


def _pair(T, base):
    """A client whose index took graph ingest, appends and a delete step by step, and a fresh one
    over all surviving rows.  -> (client, fresh index, fresh store, the surviving mention rows)."""
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    child = _texts(GC.child_rows(0, N1, dim=DIM))
    ents0, rels0, mens0 = GC.graph_rows(21, N0, E0, 150, 500)
    hi = IB.from_rows(child[:N0], entity_rows=ents0, relation_rows=rels0, mention_rows=mens0, doc_base=base)
    client = GpuIndexClient(hi.to_gpu(doc_base=base), hi.store, org_id="org")
    idx, st = client.index, client.store
    idx.set_entity_names(st.entity_names)
    seeds = dev(np.array([[0, 3, -1], [5, -1, -1]], dtype=np.int32))
    idx.graph_search(seeds, 10, 2)                       # (the caches of the old graph exist)

    def relation_arrays(rels):
        pairs = [(st.entity_index(r["subject_entity_id"]), st.entity_index(r["object_entity_id"])) for r in rels]
        pairs = [p for p in pairs if None not in p]
        return np.array([a for a, _ in pairs], dtype=np.int64), np.array([b for _, b in pairs], dtype=np.int64)

    def mention_arrays(mens):
        t = [(st.entity_index(m["entity_id"]), st.row_index(m["child_chunk_id"]), m.get("confidence", 1.0)) for m in mens]
        t = [x for x in t if x[0] is not None and x[1] is not None]
        return (np.array([x[0] for x in t], dtype=np.int64), np.array([x[1] for x in t], dtype=np.int64),
                np.array([x[2] for x in t], dtype=np.float32))

    # 1. entities + relations among old, new and mixed endpoints; present and repeated relations, self-loops
    ents1, rels1, _ = GC.graph_rows(22, N0, M1, 120, 0, ent_base=E0)
    rels1 += rels0[:9] + [dict(r, subject_entity_id=r["object_entity_id"], object_entity_id=r["subject_entity_id"])
                          for r in rels0[9:15]]
    rels1 += [{"subject_entity_id": f"e{E0}", "object_entity_id": f"e{E0 + 1}"}, {"subject_entity_id": "e1",
                                                                                 "object_entity_id": f"e{E0 + 2}"}]
    st.append_entities(ents1)
    assert idx.append_graph(entity_names=[e["name"] for e in ents1], relations=relation_arrays(rels1)) == range(E0, E0 + M1)
    # 2. mentions of old chunks, by old and new entities (one without an explicit confidence array)
    _, _, mens1 = GC.graph_rows(23, N0, E0 + M1, 0, 260)
    e, c, w = mention_arrays(mens1)
    idx.append_mentions(e[:200], c[:200], w[:200])
    plain = [dict(m, confidence=1.0) for m in mens1[200:]]
    idx.append_mentions(e[200:], c[200:])
    mens1 = mens1[:200] + plain
    # 3. new chunks whose mentions name new entities too
    _, _, mens2 = GC.graph_rows(24, N1, E0 + M1, 0, 150, chunk_lo=N0, ent_lo=E0 - 5)
    by_chunk = {}
    for m in mens2:
        by_chunk.setdefault(m["child_chunk_id"], []).append((_ent(m["entity_id"]), m.get("confidence", 1.0)))
    client.insert_children([dict(r, mentions=by_chunk.get(r["id"], [])) for r in child[N0:]])
    # 4. a delete (old and new chunks, mentioned ones among them)
    gone = [f"c{i}" for i in (17, 18, 120, 121, 122, 299, 300, 301, 350, 379)]
    client.delete_children(gone)
    # 5. more entities, relations over everything so far, mentions of the surviving chunks
    ents2, rels2, mens3 = GC.graph_rows(25, N1, M2, 80, 140, ent_base=E0 + M1)
    st.append_entities(ents2)
    assert idx.append_graph(entity_names=[e["name"] for e in ents2]) == range(E0 + M1, E0 + M1 + M2)
    assert idx.append_graph(relations=relation_arrays(rels2)) == range(E0 + M1 + M2, E0 + M1 + M2)
    idx.append_mentions(*mention_arrays(mens3))
    alive = [r for r in child if r["id"] not in set(gone)]
    full = IB.from_rows(alive, entity_rows=ents0 + ents1 + ents2, relation_rows=rels0 + rels1 + rels2,
                        mention_rows=mens0 + mens1 + mens2 + mens3, doc_base=base)
    fresh = full.to_gpu(doc_base=base)
    fresh.set_entity_names(full.store.entity_names)
    return client, fresh, full


@pytest.fixture(scope="module", params=[0, 700], ids=["base0", "interior_shard"])
def pair(T, request):
    return (request.param,) + _pair(T, request.param)


def test_mutated_index_equals_fresh_build_array_for_array(T, pair):
    base, client, fresh, full = pair
    idx = client.index
    assert idx.n_docs == fresh.n_docs == N1 - 10 and idx.doc_base == base
    for k in GRAPH_KEYS:
        same(idx.graph[k], fresh.graph[k], k)
    same(idx.entities["name_bytes"], fresh.entities["name_bytes"], "name_bytes")
    same(idx.entities["name_ptr"], fresh.entities["name_ptr"], "name_ptr")
    assert idx.entities["n"] == fresh.entities["n"] == E0 + M1 + M2 == len(client.store.entity_names)
    assert list(client.store.entity_names) == list(full.store.entity_names)
    assert "transposed" not in idx.graph or idx.graph.get("n_chunks") == idx.n_docs
    for a, b in zip(idx._graph_transposed(), fresh._graph_transposed()):
        same(a, b, "transposed mentions")


def test_graph_search_equals_fresh_index_and_oracle(T, pair):
    base, client, fresh, _ = pair
    idx = client.index
    n_ent = E0 + M1 + M2
    rng = np.random.default_rng(31)
    seeds = rng.integers(0, n_ent, (6, 3)).astype(np.int32)
    seeds[0] = [E0, -1, -1]                    # a new entity alone
    seeds[1] = [E0 + M1 + 1, 2, -1]            # newest + old
    seeds[2, 2] = -1
    g = host_graph(fresh)
    for k, hops in ((1, 0), (50, 2), (128, 8), (50, 0), (1, 2)):
        r1, r2 = idx.graph_search(dev(seeds), k, hops), fresh.graph_search(dev(seeds), k, hops)
        same_results(r1[:3], r2[:3], f"graph_search k={k} hops={hops}")
        assert_rows(r1, oracle_rows(g, seeds, hops, fresh.n_docs, k, base), f"oracle k={k} hops={hops}")
    # one scoped call
    col = (np.arange(idx.n_docs) % 3).astype(np.int32)
    for i in (idx, fresh):
        i.set_attributes({"part": col})
    scopes = [{"part": int(q % 3)} for q in range(len(seeds))]
    r1, r2 = idx.graph_search(dev(seeds), 50, 2, scopes=scopes), fresh.graph_search(dev(seeds), 50, 2, scopes=scopes)
    same_results(r1[:3], r2[:3], "scoped graph_search")
    ids = r1[1].cpu().numpy()
    for q in range(len(seeds)):
        got = ids[q][ids[q] >= 0] - base
        assert len(got) and np.all(col[got] == q % 3)


def test_find_entities_sees_the_new_names(T, pair):
    _, client, fresh, _ = pair
    idx = client.index
    newest = E0 + M1 + M2 - 1
    lists = [[f"entity {newest} "], ["ünit"], ["ACME"], [f"Entity {E0} Ünit"], ["nobody here"], ["zeta"]]
    s1, c1 = idx.find_entities(lists)
    s2, c2 = fresh.find_entities(lists)
    same(s1, s2, "seeds")
    same(c1, c2, "counts")
    rows, cnt = s1.cpu().numpy(), c1.cpu().numpy()
    assert rows[0, :cnt[0]].tolist() == [newest]                          # a name only the last batch brought
    assert cnt[1] == 16 and rows[1, 0] == len(GC.NAMES_OLD)               # old and new names match, ascending
    assert rows[2, :cnt[2]].tolist() == [0, 3] and rows[3, :cnt[3]].tolist() == [E0] and cnt[4] == 0
    # the host path of the client (its trigram index was dropped by the inserts) agrees
    ptr = idx.entities["name_bytes"].data_ptr()
    assert client.find_entities_batch(lists) == [client.find_entities(k) for k in lists]
    assert idx.entities["name_bytes"].data_ptr() == ptr              # (no re-upload: the index held the names)
    # a needle that would only match ACROSS the boundary between the old bytes and the new ones
    # (the last old name's tail + the separator's neighbour) matches nothing: the separator is there
    last_old, first_new = GC.entity_name(E0 - 1), GC.entity_name(E0)
    s3, c3 = idx.find_entities([[last_old[-3:] + first_new[:3]], [last_old[-4:]], [first_new[:8]]])
    c3 = c3.cpu().numpy()
    assert c3[0] == 0 and c3[1] >= 1 and c3[2] >= 1


def test_retrieve_batch_with_the_graph_channel_equals_fresh(T, pair):
    _, client, fresh, full = pair
    idx = client.index
    rng = np.random.default_rng(33)
    nq = 8
    q = rng.standard_normal((nq, DIM)).astype(np.float32)
    vocab = client.store.vocab
    assert vocab == full.store.vocab
    qt = np.array([[vocab[f"w{j % 7}"], vocab[f"x{j % 11}"], -1, -1] for j in range(nq)], dtype=np.int32)
    seeds = rng.integers(0, E0 + M1 + M2, (nq, 3)).astype(np.int32)
    seeds[0] = [E0 + 1, -1, -1]
    r1 = idx.retrieve_batch(dev(q), dev(qt), dev(seeds))
    r2 = fresh.retrieve_batch(dev(q), dev(qt), dev(seeds))
    same_results((r1.ids, r1.scores, r1.counts), (r2.ids, r2.scores, r2.counts), "retrieve_batch")
    same_results(r1.channels["graph"], r2.channels["graph"], "graph channel")
    assert int(r1.channels["graph"][2].sum()) > 0


# --------------------------------------------------------------------------- tiers, workspace, atomicity
def _small_graph_index(T, n_docs, base, ent_rows, rel_rows, men_rows):
    from triple_hybrid_rag_amd import index_build as IB
    cidx = {f"c{i}": base + i for i in range(n_docs)}
    g = IB.build_graph([e["id"] for e in ent_rows], rel_rows, men_rows, cidx)
    idx = T.GpuIndex(doc_base=base)
    idx.n_docs = n_docs
    return idx.set_graph(*g), g


def test_a_grown_graph_reaches_every_tier_and_the_workspace_grows(T):
    """10 entities -> 5132: a new star of 1025 and one of 4097 reached entities, and an entity that
    goes from 2047 to 2049 mentions through append_mentions; graph_search before and after."""
    n, base = 4200, 50
    ents = [{"id": f"e{i}"} for i in range(10)]
    rels = [{"subject_entity_id": f"e{i}", "object_entity_id": f"e{i + 1}"} for i in range(1, 9)]
    mens = [{"entity_id": "e0", "child_chunk_id": f"c{c}", "confidence": 0.5 + (c % 7) / 16} for c in range(2047)]
    mens += [{"entity_id": f"e{i}", "child_chunk_id": f"c{3000 + i}"} for i in range(1, 10)]
    idx, g0 = _small_graph_index(T, n, base, ents, rels, mens)
    seeds0 = np.array([[0, -1], [1, -1], [2, 3], [4, -1], [9, -1]], dtype=np.int32)
    assert_rows(idx.graph_search(dev(seeds0), 50, 8), oracle_rows(g0, seeds0, 8, n, 50, base), "before")
    ws_before = idx._ws_graph.numel()
    assert ws_before == T._native.graph_workspace_bytes(len(seeds0), 10)
    # the stars: centre a with 1024 leaves, centre b with 4096; every leaf mentions one chunk
    a, b = 10, 10 + 1025
    total = b + 4097
    new_ents = [{"id": f"e{i}"} for i in range(10, total)]
    new_rels = [{"subject_entity_id": f"e{a}", "object_entity_id": f"e{a + 1 + j}"} for j in range(1024)] + \
        [{"subject_entity_id": f"e{b + 1 + j}", "object_entity_id": f"e{b}"} for j in range(4096)]
    new_mens = [{"entity_id": f"e{a + 1 + j}", "child_chunk_id": f"c{j}", "confidence": 0.25 + (j % 5) / 8} for j in range(1024)] + \
        [{"entity_id": f"e{b + 1 + j}", "child_chunk_id": f"c{j}", "confidence": 0.125 + (j % 3) / 4} for j in range(4096)] + \
        [{"entity_id": "e0", "child_chunk_id": "c2046", "confidence": 0.75}, {"entity_id": "e0", "child_chunk_id": "c1"}]
    assert idx.append_graph(n_new_entities=total - 10,
                            relations=(np.array([_ent(r["subject_entity_id"]) for r in new_rels]),
                                       np.array([_ent(r["object_entity_id"]) for r in new_rels]))) == range(10, total)
    idx.append_mentions(np.array([_ent(m["entity_id"]) for m in new_mens]),
                        np.array([int(m["child_chunk_id"][1:]) for m in new_mens]),
                        np.array([m.get("confidence", 1.0) for m in new_mens], dtype=np.float32))
    fresh, g1 = _small_graph_index(T, n, base, ents + new_ents, rels + new_rels, mens + new_mens)
    for k, arr in zip(GRAPH_KEYS, g1):
        same(idx.graph[k], fresh.graph[k], k)
    assert int(np.diff(g1[2])[0]) == 2049
    seeds = np.array([[a, -1], [b, -1], [0, -1], [a, b], [b + 7, 0]], dtype=np.int32)
    r1, r2 = idx.graph_search(dev(seeds), 50, 1), fresh.graph_search(dev(seeds), 50, 1)
    same_results(r1[:3], r2[:3], "tiers")
    assert_rows(r1, oracle_rows(g1, seeds, 1, n, 50, base), "tiers vs oracle")
    assert len(seeds) == len(seeds0)                                  # the same batch size: only the entities grew
    need = T._native.graph_workspace_bytes(len(seeds), total)
    assert idx._ws_graph.numel() >= need > ws_before                  # the workspace grew with the entity count


def test_a_refused_call_leaves_the_graph_untouched(T):
    n, base = 64, 5
    ents = [{"id": f"e{i}"} for i in range(12)]
    rels = [{"subject_entity_id": f"e{i}", "object_entity_id": f"e{(i * 5 + 1) % 12}"} for i in range(12)]
    mens = [{"entity_id": f"e{i % 12}", "child_chunk_id": f"c{(i * 7) % n}", "confidence": 0.5} for i in range(40)]
    idx, g = _small_graph_index(T, n, base, ents, rels, mens)
    idx.set_entity_names([f"name {i}" for i in range(12)])
    seeds = np.array([[0, 4], [7, -1]], dtype=np.int32)
    want = oracle_rows(g, seeds, 2, n, 20, base)

    def snapshot():
        return {k: (v.data_ptr(), v.clone()) for k, v in list(idx.graph.items()) + list(idx.entities.items())
                if isinstance(v, torch.Tensor)}

    def unchanged(before):
        now = snapshot()
        assert sorted(now) == sorted(before)
        for k, (ptr, val) in before.items():
            assert now[k][0] == ptr and torch.equal(now[k][1], val), k
        assert_rows(idx.graph_search(dev(seeds), 20, 2), want, "after a refusal")

    before, count = snapshot(), idx._mutations
    with pytest.raises(ValueError, match="relation endpoints"):
        idx.append_graph(entity_names=["x"], relations=(np.array([0, 13]), np.array([12, 1])))
    with pytest.raises(T.NativeError, match="entity_names .* required"):
        idx.append_graph(n_new_entities=1)
    with pytest.raises(ValueError, match="stored chunks"):
        idx.append_mentions(np.array([0]), np.array([n]))
    unchanged(before)
    assert idx._mutations == count
    # a graph that is not in canonical form (set_graph takes any arrays): refused, not merged
    er, ec, mr, mc, mw = (a.copy() for a in g)
    row = max(range(12), key=lambda t: er[t + 1] - er[t])
    lo, hi = int(er[row]), int(er[row + 1])
    assert hi - lo >= 2
    ec[lo:hi] = ec[lo:hi][::-1]
    lo_m = next(t for t in range(12) if mr[t + 1] - mr[t] >= 2 and mc[mr[t]] != mc[mr[t] + 1])
    mc[mr[lo_m]], mc[mr[lo_m] + 1] = mc[mr[lo_m] + 1], mc[mr[lo_m]]
    idx.set_graph(er, ec, mr, mc, mw)
    g_bad = (er, ec, mr, mc, mw)
    want = oracle_rows(g_bad, seeds, 2, n, 20, base)
    before = snapshot()
    with pytest.raises(T.NativeError, match="append_graph: .*build_graph's canonical form"):
        idx.append_graph(entity_names=["x"], relations=(np.array([0]), np.array([12])))
    with pytest.raises(T.NativeError, match="append_mentions: .*build_graph's canonical form"):
        idx.append_mentions(np.array([1]), np.array([2]))
    unchanged(before)
    # entities alone need no merge: they are taken
    assert idx.append_graph(entity_names=["x"]) == range(12, 13) and idx.entities["n"] == 13


# --------------------------------------------------------------------------- drop-in, end to end
def test_dropin_entity_extraction_sequence_then_retrieve_and_save_load(T, tmp_path):
    """Children first, then what the reference's extraction does per document: upsert entities
    (select by canonical name, insert when absent), insert relations, insert mentions."""
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.config import SETTINGS
    from triple_hybrid_rag_amd.rag2.embedder import PrecomputedEmbedder
    from triple_hybrid_rag_amd.rag2.query_planner import QueryPlanner
    from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever
    n0, n, d = 120, 136, 1024
    child = GC.child_rows(0, n, dim=d)
    ents0, rels0, mens0 = GC.graph_rows(41, n0, 20, 40, 120)
    parents = [{"id": f"p{j}", "text": f"parent text {j}", "section_heading": None} for j in range(n // 4)]
    hi = IB.from_rows(child[:n0], parents, entity_rows=ents0, relation_rows=rels0, mention_rows=mens0)
    client = GpuIndexClient(hi.to_gpu(), hi.store, org_id="org")
    client.find_entities_batch([["acme"]])                      # (the names are on the device, as in service)
    client.table("rag_child_chunks").insert([dict(r, mentions=[]) for r in child[n0:]]).execute()

    def upsert(name):
        canonical = name.lower()
        got = client.table("rag_entities").select("id").eq("org_id", "org").eq("canonical_name", canonical).limit(1).execute()
        if got.data:
            return got.data[0]["id"]
        eid = f"uuid-{canonical}"
        client.table("rag_entities").insert({"id": eid, "org_id": "org", "document_id": "d8", "entity_type": "ORG",
                                             "name": name, "canonical_name": canonical, "description": None,
                                             "metadata": {}}).execute()
        return eid

    quasar, nebula, acme = upsert("Quasar Dynamics"), upsert("Nebula Söhne"), upsert("Acme Corp")
    assert acme == "e0" and upsert("Quasar Dynamics") == quasar and len(client.store.entity_names) == 22
    client.table("rag_relations").insert({"id": "r-1", "org_id": "org", "document_id": "d8", "relation_type": "owns",
                                          "subject_entity_id": quasar, "object_entity_id": nebula, "confidence": 0.9,
                                          "source_parent_id": "p32", "metadata": {}}).execute()
    for eid, cid, conf in ((quasar, f"c{n - 1}", 0.9), (nebula, f"c{n - 2}", 0.8), (quasar, "c5", 0.7)):
        client.table("rag_entity_mentions").insert({"id": f"m-{eid}-{cid}", "entity_id": eid, "parent_chunk_id": "p0",
                                                    "child_chunk_id": cid, "document_id": "d8", "mention_text": "x",
                                                    "confidence": conf, "char_start": None, "char_end": None}).execute()
    # equal to a bulk build from all the rows
    new_ents = [{"id": quasar, "name": "Quasar Dynamics", "canonical_name": "quasar dynamics"},
                {"id": nebula, "name": "Nebula Söhne", "canonical_name": "nebula söhne"}]
    new_rels = [{"subject_entity_id": quasar, "object_entity_id": nebula}]
    new_mens = [{"entity_id": quasar, "child_chunk_id": f"c{n - 1}", "confidence": 0.9},
                {"entity_id": nebula, "child_chunk_id": f"c{n - 2}", "confidence": 0.8},
                {"entity_id": quasar, "child_chunk_id": "c5", "confidence": 0.7}]
    full = IB.from_rows(child, parents, entity_rows=ents0 + new_ents, relation_rows=rels0 + new_rels,
                        mention_rows=mens0 + new_mens)
    ref = full.to_gpu()
    ref.set_entity_names(full.store.entity_names)
    for k in GRAPH_KEYS:
        same(client.index.graph[k], ref.graph[k], k)
    same(client.index.entities["name_bytes"], ref.entities["name_bytes"], "name_bytes")
    # a query whose only graph seeds are the new entities: the new chunks come through the graph channel
    assert client.find_entities(["quasar"]) == [20] and client.find_entities_batch([["quasar"], ["söhne"]]) == [[20], [21]]
    saved = dict(SETTINGS.__dict__)
    SETTINGS.rag2_safety_threshold = 0.0
    SETTINGS.rag2_denoise_alpha = 0.0
    SETTINGS.rag2_graph_enabled = True

    def graph_hits(c):
        e = PrecomputedEmbedder(store_dim=d)
        e.register("quasar", np.random.default_rng(9).standard_normal(d).astype(np.float32).tolist())
        r = RAG2Retriever(org_id="org", embedder=e, query_planner=QueryPlanner(graph=True), graph_enabled=True)
        r._supabase = c
        res = asyncio.run(r.retrieve("quasar", top_k=10, skip_rerank=True))
        assert res.success
        return sorted(((x.child_id, x.graph_rank) for x in res.contexts if x.graph_rank is not None), key=lambda t: t[1])
    try:
        hits = graph_hits(client)
        # hop 0: quasar's chunks (0.9, 0.7); hop 1: nebula's (0.8 / 2)
        assert hits[:3] == [(f"c{n - 1}", 1), ("c5", 2), (f"c{n - 2}", 3)]
        # save -> load -> to_gpu: the same arrays, the same answer
        path = str(tmp_path / "idx")
        IB.save(hi, path, client.index)
        back = IB.load(path)
        assert list(back.store.entity_names) == list(client.store.entity_names)
        assert back.store.entity_index(quasar) == 20 and back.store.entity_by_canonical("nebula söhne") == 21
        c2 = GpuIndexClient(back.to_gpu(), back.store, org_id="org")
        for k in GRAPH_KEYS:
            same(c2.index.graph[k], client.index.graph[k], "loaded " + k)
        assert graph_hits(c2) == hits
    finally:
        SETTINGS.__dict__.update(saved)
