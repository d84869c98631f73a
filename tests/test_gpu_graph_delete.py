"""Graph delete on the device: thr_csr_prune against its numpy restatement on every built case,
GpuIndex.delete_graph against a fresh build over the surviving rows (arrays, name store, answers),
sequences with the other mutations, the workspace contract, and the drop-in surface end to end."""
import asyncio
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graph_delete_cases as GD  # noqa: E402
import graph_ingest_cases as GC  # noqa: E402
import workspace_cases as W  # noqa: E402

SENTINEL, GUARD = -7, 32
GRAPH_KEYS = ("ent_rowptr", "ent_col", "men_rowptr", "men_chunk", "men_conf")


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()         # (a copy: the cases' arrays are read-only)
    return t if dtype is None else t.to(dtype)


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} != {b.shape} {b.dtype}"
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{what} differs"


def same_results(r1, r2, what):
    for j, (a, b) in enumerate(zip(r1, r2)):
        same(a, b, f"{what}[{j}]")


# --------------------------------------------------------------------------- thr_csr_prune alone
def _case_args(c, two):
    opt = lambda a: None if a is None else dev(a)
    return dict(rowptr_a=dev(c.rowptr_a), ids_a=dev(c.ids_a), pay_a=dev(c.pay_a).view(torch.float32) if two else None,
                row_remap=opt(c.row_remap), rows_out=None if c.row_remap is None else c.rows_out, id_remap=opt(c.id_remap),
                id_base=c.id_base, rowptr_b=opt(c.rowptr_b), ids_b=opt(c.ids_b))


def _prune(N, c, two, cap, **kw):
    """One call on a case, its destinations of ``cap`` elements inside guarded buffers pre-filled with a sentinel."""
    g_ids = torch.full((cap + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    g_pay = torch.full((cap + 2 * GUARD,), SENTINEL, dtype=torch.int32, device="cuda") if two else None
    out = N.csr_prune(**_case_args(c, two), ids_out=g_ids[GUARD:GUARD + cap],
                      pay_out=g_pay[GUARD:GUARD + cap].view(torch.float32) if two else None, want_keep=True, **kw)
    return out, g_ids.cpu().numpy(), None if g_pay is None else g_pay.cpu().numpy()


CASES = list(GD.cases())


@pytest.mark.parametrize("two", [True, False], ids=["payload", "ids_only"])
@pytest.mark.parametrize("name", CASES)
def test_csr_prune_equals_the_numpy_restatement(T, name, two):
    N = T._native
    c = GD.cases()[name]
    exp = GD.expected(c)
    nnz_a = len(c.ids_a)
    if exp["nnz"] is None:                      # a B row out of order: reported; undefined, but inside its buffers
        (_, _, _, _, status, _), g_ids, g_pay = _prune(N, c, two, nnz_a, check=False)
        assert status == c.status == exp["status"]
        assert np.all(g_ids[:GUARD] == SENTINEL) and np.all(g_ids[GUARD + nnz_a:] == SENTINEL)
        with pytest.raises(T.NativeError, match="strictly ascending"):
            _prune(N, c, two, nnz_a)
        return
    cap = GD.capacity(c) if c.short else exp["nnz"] + 5
    (rp, _, pay, nnz, status, keep), g_ids, g_pay = _prune(N, c, two, cap, check=False)
    assert (nnz, status) == (exp["nnz"], exp["status"]) and (pay is None) == (not two)
    assert rp.dtype == torch.int64 and np.array_equal(rp.cpu().numpy(), exp["rowptr"]), "rowptr_out"
    assert np.array_equal(keep.cpu().numpy(), exp["keep"]), "keep_out"
    wrote = min(nnz, cap)
    assert np.array_equal(g_ids[GUARD:GUARD + wrote], exp["ids"][:wrote]), "ids_out"
    assert np.all(g_ids[:GUARD] == SENTINEL) and np.all(g_ids[GUARD + wrote:] == SENTINEL), "written outside [0, min(nnz, capacity))"
    if two:
        assert np.array_equal(g_pay[GUARD:GUARD + wrote], exp["pay"][:wrote]), "pay_out (bit patterns)"
        assert np.all(g_pay[:GUARD] == SENTINEL) and np.all(g_pay[GUARD + wrote:] == SENTINEL)
    if c.short:
        assert status == GD.OVERFLOW and wrote == cap == nnz - 1
        with pytest.raises(T.NativeError, match="out_capacity"):
            _prune(N, c, two, cap)
    elif nnz > 0:                               # out_capacity exactly nnz_out is accepted
        (rp2, _, _, nnz2, status2, _), g2, _ = _prune(N, c, two, nnz)
        assert (nnz2, status2) == (nnz, 0) and np.array_equal(g2[GUARD:GUARD + nnz], exp["ids"])
        assert np.array_equal(rp2.cpu().numpy(), exp["rowptr"])


def test_csr_prune_reports_a_row_destination_outside_the_result(T):
    N = T._native
    c = GD.cases()["first_last_removed"]
    args = _case_args(c, False)
    bad = np.array(c.row_remap)
    bad[5] = c.rows_out + 3                     # (the row is treated as removed: nothing of it is written)
    args["row_remap"] = dev(bad)
    out = N.csr_prune(**args, check=False)
    assert out[4] == GD.BAD_ROW
    with pytest.raises(T.NativeError, match="rows_out"):
        N.csr_prune(**args)


def test_csr_prune_allocates_destinations_and_reuses_a_workspace(T):
    N = T._native
    c = GD.cases()["random_70000"]
    exp = GD.expected(c)
    ws = torch.full((1 << 20,), 0xFF, dtype=torch.uint8, device="cuda")
    assert N.csr_prune_workspace_bytes(len(c.rowptr_a) - 1, len(c.ids_a)) <= ws.numel()
    rp, ids, pay, nnz, status, keep = N.csr_prune(**_case_args(c, False), workspace=ws)
    assert pay is None and keep is None and status == 0 and nnz == exp["nnz"] and ids.shape[0] == len(c.ids_a)
    assert np.array_equal(ids[:nnz].cpu().numpy(), exp["ids"]) and np.array_equal(rp.cpu().numpy(), exp["rowptr"])
    args = _case_args(c, False)
    args["pay_a"] = dev(c.pay_a)                # an int32 payload (opaque 4-byte elements)
    rp, ids, pay, nnz, _, _ = N.csr_prune(**args, workspace=ws)
    assert pay.dtype == torch.int32 and np.array_equal(pay[:nnz].cpu().numpy(), exp["pay"])


# --------------------------------------------------------------------------- the workspace contract
PRUNE_A = "random_70000"
PRUNE_B = ("slice_edges", "empty_runs", "multiset", "nnz_zero", "ids_outside_with_remap_base_700", "overflow")


def _prune_adapter(b: str) -> W.Adapter:
    """thr_csr_prune under the workspace contract: the 70 000-entry case and a small one on one slab."""
    from triple_hybrid_rag_amd import _native as N

    def need(shape):
        c = GD.cases()[shape]
        return N.csr_prune_workspace_bytes(len(c.rowptr_a) - 1, len(c.ids_a))

    def run(shape, ws):
        c = GD.cases()[shape]
        cap = GD.capacity(c)
        ids_out = torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda")
        pay_out = torch.full((cap,), SENTINEL, dtype=torch.int32, device="cuda")
        args = _case_args(c, False)
        args["pay_a"] = dev(c.pay_a)
        rp, ids, pay, nnz, status, keep = N.csr_prune(**args, ids_out=ids_out, pay_out=pay_out, want_keep=True,
                                                      workspace=ws, check=False)
        n = min(nnz, cap)                        # UNDEFINED["csr"]: cut at nnz_out (and the capacity)
        return dict(rowptr=rp, ids=ids[:n], pay=pay[:n], keep=keep, nnz=np.array([nnz], dtype=np.int64),
                    status=np.array([status], dtype=np.int64))

    def expected(shape):
        c = GD.cases()[shape]
        e = GD.expected(c)
        n = min(e["nnz"], GD.capacity(c))
        return dict(rowptr=e["rowptr"], ids=e["ids"][:n], pay=e["pay"][:n], keep=e["keep"],
                    nnz=np.array([e["nnz"]], dtype=np.int64), status=np.array([e["status"]], dtype=np.int64))
    return W.Adapter(f"csr_prune/{b}", (), {"A": PRUNE_A, "B": b}, need, run, expected)


@pytest.mark.parametrize("b", PRUNE_B)
def test_workspace_contract_of_csr_prune(T, b):
    """B on 0x00, B on 0xFF, A then B, B then A: byte-identical outputs, the restatement's, and every byte of
    the slab outside each call's view unchanged (tests/workspace_cases.py holds the harness)."""
    W.exercise(_prune_adapter(b), "cuda")


# --------------------------------------------------------------------------- index level
N_CHUNKS, N_ENT, DIM = 300, 260, 256


def _texts(rows):
    for r in rows:
        i = int(r["id"][1:])
        r["text"] = f"chunk w{i % 7} w{i % 3} x{i % 11}"
    return rows


_ROWS = {}


def table_rows():
    if not _ROWS:
        ents, rels, mens = GC.graph_rows(61, N_CHUNKS, N_ENT, 700, 1500)
        _ROWS.update(child=_texts(GC.child_rows(0, N_CHUNKS, dim=DIM)), ents=ents, rels=rels, mens=mens)
    return _ROWS["child"], _ROWS["ents"], _ROWS["rels"], _ROWS["mens"]


def build(child, ents, rels, mens, base):
    """A fresh index over these rows: from_rows -> to_gpu -> set_entity_names."""
    from triple_hybrid_rag_amd import index_build as IB
    full = IB.from_rows(child, entity_rows=ents, relation_rows=rels, mention_rows=mens, doc_base=base)
    idx = full.to_gpu(doc_base=base)
    idx.set_entity_names(full.store.entity_names)
    return idx


def assert_same_graph(idx, fresh, what=""):
    for k in GRAPH_KEYS:
        same(idx.graph[k], fresh.graph[k], f"{what} {k}")
    same(idx.entities["name_bytes"], fresh.entities["name_bytes"], f"{what} name_bytes")
    same(idx.entities["name_ptr"], fresh.entities["name_ptr"], f"{what} name_ptr")
    assert idx.entities["n"] == fresh.entities["n"] == idx.graph["men_rowptr"].shape[0] - 1
    for a, b in zip(idx._graph_transposed(), fresh._graph_transposed()):
        same(a, b, f"{what} transposed mentions")


def deletions(seed, ents, rels, mens, child):
    """GD.graph_deletions over rows whose entity ids are no longer e<position> and whose chunks are no longer
    c<local id>: the rows are renamed by position first (a mention of a chunk that is gone names nothing)."""
    pos = {e["id"]: i for i, e in enumerate(ents)}
    row = {r["id"]: i for i, r in enumerate(child)}
    named = lambda r, k: dict(r, **{k: f"e{pos[r[k]]}"})
    rels = [named(named(r, "subject_entity_id"), "object_entity_id") for r in rels
            if r["subject_entity_id"] in pos and r["object_entity_id"] in pos]
    mens = [dict(named(m, "entity_id"), child_chunk_id=f"c{row[m['child_chunk_id']]}") for m in mens
            if m["entity_id"] in pos and m["child_chunk_id"] in row]
    return GD.graph_deletions(seed, len(ents), rels, mens, len(child))


@pytest.mark.parametrize("base", [0, 700], ids=["base0", "interior_shard"])
@pytest.mark.parametrize("kinds", ["entities", "relations", "mentions", "all"])
def test_delete_graph_equals_a_fresh_build_and_answers_like_it(T, kinds, base):
    child, ents, rels, mens = table_rows()
    idx = build(child, ents, rels, mens, base)
    old_seeds = np.array([[0, 3, -1], [5, 17, 40], [N_ENT - 1, -1, -1], [100, 101, 102]], dtype=np.int32)
    idx.graph_search(dev(old_seeds), 10, 2)                       # (the caches of the old graph exist)
    de, dr, dm = GD.graph_deletions(7, N_ENT, rels, mens, N_CHUNKS)
    de = np.concatenate([de, [5, 101]])                           # entities the seeds name
    de, dr, dm = (de if kinds in ("entities", "all") else None, dr if kinds in ("relations", "all") else None,
                  dm if kinds in ("mentions", "all") else None)
    count = idx._mutations
    remap = idx.delete_graph(entities=de, relations=dr, mentions=dm)
    assert idx._mutations == count + 1 and remap.dtype == torch.int32 and remap.shape == (N_ENT,) and remap.is_cuda
    e2, r2, m2 = GD.surviving_rows(ents, rels, mens, () if de is None else de, dr, dm)
    fresh = build(child, e2, r2, m2, base)
    assert_same_graph(idx, fresh, kinds)
    keep = np.ones(N_ENT, dtype=bool)
    if de is not None:
        keep[de] = False
    want = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    assert np.array_equal(remap.cpu().numpy(), want)
    # seeds that touched removed entities, renumbered with the remap the call returned
    seeds = np.where(old_seeds >= 0, want[np.maximum(old_seeds, 0)], -1).astype(np.int32)
    seeds = np.stack([np.concatenate([r[r >= 0], r[r < 0]]) for r in seeds])      # (the seeds that are left, then -1)
    assert (kinds in ("entities", "all")) == bool((seeds[1] == -1).any())
    for k, hops in ((10, 0), (50, 2), (128, 4)):
        same_results(idx.graph_search(dev(seeds), k, hops)[:3], fresh.graph_search(dev(seeds), k, hops)[:3],
                     f"graph_search k={k} hops={hops}")
    lists = [[ents[5]["name"]], ["ünit"], ["acme"], [ents[101]["name"]], ["nobody here"]]
    (s1, c1), (s2, c2) = idx.find_entities(lists), fresh.find_entities(lists)
    same(s1, s2, "find_entities seeds")
    same(c1, c2, "find_entities counts")
    if de is not None:
        full_name = c1.cpu().numpy()[3], s1.cpu().numpy()[3]
        assert all(e2[int(i)]["name"] != ents[101]["name"] for i in full_name[1][:full_name[0]])     # the removed name is gone
    # scoped: the graph channel alone, and once through retrieve_batch with scope_graph
    col = (np.arange(N_CHUNKS) % 3).astype(np.int32)
    for i in (idx, fresh):
        i.set_attributes({"part": col})
    scopes = [{"part": int(q % 3)} for q in range(len(seeds))]
    same_results(idx.graph_search(dev(seeds), 50, 2, scopes=scopes)[:3], fresh.graph_search(dev(seeds), 50, 2, scopes=scopes)[:3],
                 "scoped graph_search")
    if kinds == "all":
        rng = np.random.default_rng(33)
        q = rng.standard_normal((len(seeds), DIM)).astype(np.float32)
        r1 = idx.retrieve_batch(dev(q), None, dev(seeds), scopes=scopes, scope_graph=True)
        r2 = fresh.retrieve_batch(dev(q), None, dev(seeds), scopes=scopes, scope_graph=True)
        same_results((r1.ids, r1.scores, r1.counts), (r2.ids, r2.scores, r2.counts), "retrieve_batch, scope_graph")
        same_results(r1.channels["graph"], r2.channels["graph"], "scoped graph channel")


def test_delete_graph_in_sequence_with_the_other_mutations(T):
    """delete -> append_graph / append_mentions -> delete; delete_rows after delete_graph and the reverse: after
    each step the arrays are a fresh build's over the rows that are left."""
    base = 40
    child, ents, rels, mens = (list(x) for x in table_rows())
    idx = build(child, ents, rels, mens, base)

    def check(what):
        assert_same_graph(idx, build(child, ents, rels, mens, base), what)

    def positions(rows, key):
        pos = {e["id"]: i for i, e in enumerate(ents)}
        return np.array([pos[r[key]] for r in rows], dtype=np.int64)

    de, dr, dm = GD.graph_deletions(8, len(ents), rels, mens, len(child))
    idx.delete_graph(entities=de, relations=dr, mentions=dm)
    ents, rels, mens = GD.surviving_rows(ents, rels, mens, de, dr, dm)
    check("first delete")
    # new entities with relations to old ones, mentions by old and new entities
    new_ents, new_rels, new_mens = GC.graph_rows(62, len(child), 30, 80, 160, ent_base=1000, ent_lo=1000)
    new_rels += [dict(r, subject_entity_id=ents[3]["id"]) for r in new_rels[:20]] + rels[:5]
    new_mens += [dict(m, entity_id=ents[7]["id"]) for m in new_mens[:30]]
    ents = ents + new_ents
    assert idx.append_graph(entity_names=[e["name"] for e in new_ents],
                            relations=(positions(new_rels, "subject_entity_id"), positions(new_rels, "object_entity_id"))) == \
        range(len(ents) - 30, len(ents))
    rels = rels + new_rels
    idx.append_mentions(positions(new_mens, "entity_id"), np.array([int(m["child_chunk_id"][1:]) for m in new_mens]),
                        np.array([m.get("confidence", 1.0) for m in new_mens], dtype=np.float32))
    mens = mens + [dict(m, confidence=m.get("confidence", 1.0)) for m in new_mens]
    check("append after delete")
    de, dr, dm = deletions(9, ents, rels, mens, child)
    de = np.concatenate([de, [len(ents) - 1, len(ents) - 2]])      # new entities among them
    idx.delete_graph(entities=de, relations=dr, mentions=dm)
    ents, rels, mens = GD.surviving_rows(ents, rels, mens, de, dr, dm)
    check("second delete")
    # delete_rows after delete_graph: the mentions of the chunks go by the chunk cascade
    gone = [3, 4, 77, 150, 151, 299]
    idx.delete_rows(np.array(gone))
    child = [r for i, r in enumerate(child) if i not in set(gone)]
    check("delete_rows after delete_graph")
    # ... and the reverse: chunk ids are local ids of the rows that are left
    de, dr, dm = deletions(10, ents, rels, mens, child)
    idx.delete_graph(entities=de[:5], relations=dr, mentions=dm)
    ents, rels, mens = GD.surviving_rows(ents, rels, mens, de[:5], dr, dm, chunk_ids=[r["id"] for r in child])
    check("delete_graph after delete_rows")
    # every mention of one entity and every mention of one chunk, on their own
    idx.delete_graph(mentions=(np.array([2, -1]), np.array([-1, 9])))
    ents, rels, mens = GD.surviving_rows(ents, rels, mens, (), None, (np.array([2, -1]), np.array([-1, 9])),
                                         chunk_ids=[r["id"] for r in child])
    check("wildcards")
    # nothing named: a no-op, the identity remap
    count = idx._mutations
    assert idx.delete_graph().tolist() == list(range(len(ents))) and idx._mutations == count
    assert idx.delete_graph(entities=[], relations=([], []), mentions=([], [])).tolist() == list(range(len(ents)))
    assert idx._mutations == count


def test_a_refused_delete_graph_leaves_every_array_as_it_was(T):
    child, ents, rels, mens = table_rows()
    idx = build(child, ents, rels, mens, 5)

    def snapshot():
        return {k: (v.data_ptr(), v.clone()) for k, v in list(idx.graph.items()) + list(idx.entities.items())
                if isinstance(v, torch.Tensor)}

    before, count = snapshot(), idx._mutations
    with pytest.raises(ValueError, match="entity ids are 0"):
        idx.delete_graph(entities=np.array([3, N_ENT]), relations=(np.array([0]), np.array([1])))
    with pytest.raises(ValueError, match="chunk ids are local doc ids"):
        idx.delete_graph(entities=np.array([3]), mentions=(np.array([0]), np.array([N_CHUNKS])))
    with pytest.raises(T.NativeError, match="every entity would be deleted"):
        idx.delete_graph(entities=torch.arange(N_ENT, device="cuda"))
    with pytest.raises(T.NativeError, match="one length"):
        idx.delete_graph(relations=(np.array([0, 1]), np.array([1])))
    now = snapshot()
    assert sorted(now) == sorted(before) and idx._mutations == count
    for k, (ptr, val) in before.items():
        assert now[k][0] == ptr and torch.equal(now[k][1], val), k
    bare = T.GpuIndex()
    with pytest.raises(T.NativeError, match="no graph channel"):
        bare.delete_graph(entities=[0])


# --------------------------------------------------------------------------- drop-in, end to end
def test_dropin_graph_cascade_table_deletes_and_save_load(T, tmp_path):
    """The extraction sequence of test_gpu_graph_ingest with entities that carry their document_id; then the
    document is deleted with and without graph_cascade, then rows of the three graph tables."""
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.config import SETTINGS
    from triple_hybrid_rag_amd.rag2.embedder import PrecomputedEmbedder
    from triple_hybrid_rag_amd.rag2.query_planner import QueryPlanner
    from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever
    n0, n, d = 120, 136, 1024
    child = GC.child_rows(0, n, dim=d)
    ents0, rels0, mens0 = GC.graph_rows(41, n0, 20, 40, 120)
    ents0 = [dict(e, document_id=f"d{i % 5}") for i, e in enumerate(ents0)]
    parents = [{"id": f"p{j}", "text": f"parent text {j}", "section_heading": None} for j in range(n // 4)]
    new_ents = [{"id": "uuid-quasar", "name": "Quasar Dynamics", "canonical_name": "quasar dynamics", "document_id": "d8"},
                {"id": "uuid-nebula", "name": "Nebula Söhne", "canonical_name": "nebula söhne", "document_id": "d8"}]
    new_rels = [{"id": "r-1", "subject_entity_id": "uuid-quasar", "object_entity_id": "uuid-nebula"}]
    new_mens = [{"entity_id": "uuid-quasar", "child_chunk_id": f"c{n - 1}", "confidence": 0.9},
                {"entity_id": "uuid-nebula", "child_chunk_id": f"c{n - 2}", "confidence": 0.8},
                {"entity_id": "uuid-quasar", "child_chunk_id": "c5", "confidence": 0.7},
                {"entity_id": "uuid-nebula", "child_chunk_id": "c6", "confidence": 0.6}]

    def extracted(**kw):
        hi = IB.from_rows(child[:n0], parents, entity_rows=ents0, relation_rows=rels0, mention_rows=mens0)
        client = GpuIndexClient(hi.to_gpu(), hi.store, org_id="org", **kw)
        client.find_entities_batch([["acme"]])                      # (the names are on the device, as in service)
        client.table("rag_child_chunks").insert([dict(r, mentions=[]) for r in child[n0:]]).execute()
        client.table("rag_entities").insert([dict(e, org_id="org") for e in new_ents]).execute()
        client.table("rag_relations").insert(new_rels).execute()
        client.table("rag_entity_mentions").insert(new_mens).execute()
        assert client.store.entity_documents[-2:] == ["d8", "d8"]
        return hi, client

    def assert_bulk(client, rows, e, r, m, what):
        full = IB.from_rows(rows, parents, entity_rows=e, relation_rows=r, mention_rows=m)
        ref = full.to_gpu()
        ref.set_entity_names(full.store.entity_names)
        for k in GRAPH_KEYS:
            same(client.index.graph[k], ref.graph[k], f"{what}: {k}")
        same(client.index.entities["name_bytes"], ref.entities["name_bytes"], f"{what}: name_bytes")
        same(client.index.entities["name_ptr"], ref.entities["name_ptr"], f"{what}: name_ptr")
        assert list(client.store.entity_names) == list(full.store.entity_names)

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
        alive = [r for r in child if r["document_id"] != "d8"]
        # with the flag: the document takes its entities, their relations and their mentions
        _, cascade = extracted(graph_cascade=True)
        assert cascade.find_entities(["quasar"]) == [20] and graph_hits(cascade)[0] == (f"c{n - 1}", 1)
        assert cascade.table("rag_documents").delete().eq("id", "d8").execute().data == [{"id": "d8"}]
        assert cascade.find_entities(["quasar"]) == [] and cascade.find_entities_batch([["quasar"], ["söhne"]]) == [[], []]
        assert graph_hits(cascade) == []                              # c5 is still there, the way to it is not
        assert_bulk(cascade, alive, ents0, rels0, mens0, "graph_cascade")
        # the default: the entity stays, as before the flag; its mention of c5 still leads there
        hi, client = extracted()
        assert client.table("rag_documents").delete().eq("id", "d8").execute().data == [{"id": "d8"}]
        assert client.find_entities(["quasar"]) == [20]
        assert_bulk(client, alive, ents0 + new_ents, rels0 + new_rels, mens0 + new_mens, "default")
        assert [h[0] for h in graph_hits(client)][:2] == ["c5", "c6"]
        # the three tables, each followed by the comparison with a bulk build
        got = client.table("rag_entity_mentions").delete().eq("entity_id", "uuid-quasar").eq("child_chunk_id", "c5").execute().data
        assert got == [{"entity_id": "uuid-quasar", "child_chunk_id": "c5", "confidence": pytest.approx(0.7)}]
        mens = [m for m in mens0 + new_mens if (m["entity_id"], m["child_chunk_id"]) != ("uuid-quasar", "c5")]
        assert_bulk(client, alive, ents0 + new_ents, rels0 + new_rels, mens, "mention delete")
        assert [h[0] for h in graph_hits(client)][:1] == ["c6"]       # through quasar -> nebula
        got = client.table("rag_relations").delete().eq("subject_entity_id", "uuid-nebula").eq("object_entity_id", "uuid-quasar").execute().data
        assert got == [{"subject_entity_id": "uuid-nebula", "object_entity_id": "uuid-quasar"}]
        assert_bulk(client, alive, ents0 + new_ents, rels0 + new_rels[1:], mens, "relation delete")
        assert graph_hits(client) == []
        got = client.table("rag_entities").delete().in_("id", ["uuid-nebula", "e3"]).execute().data
        assert [r["id"] for r in got] == ["e3", "uuid-nebula"]
        gone = {"uuid-nebula", "e3"}
        e3 = [e for e in ents0 + new_ents if e["id"] not in gone]
        r3 = [r for r in rels0 + new_rels[1:] if r["subject_entity_id"] not in gone and r["object_entity_id"] not in gone]
        m3 = [m for m in mens if m["entity_id"] not in gone]
        assert_bulk(client, alive, e3, r3, m3, "entity delete")
        assert client.find_entities(["quasar"]) == [19] and client.find_entities(["söhne"]) == []
        by_doc = client.table("rag_entities").delete().eq("document_id", "d8").execute().data
        assert [r["id"] for r in by_doc] == ["uuid-quasar"]
        e3, m3 = [e for e in e3 if e["id"] != "uuid-quasar"], [m for m in m3 if m["entity_id"] != "uuid-quasar"]
        assert_bulk(client, alive, e3, r3, m3, "entity delete by document")
        # save -> load -> to_gpu: the same arrays, the same answers
        path = str(tmp_path / "idx")
        IB.save(hi, path, client.index)
        back = IB.load(path)
        assert list(back.store.entity_names) == list(client.store.entity_names)
        assert list(back.store.entity_documents) == list(client.store.entity_documents)
        c2 = GpuIndexClient(back.to_gpu(), back.store, org_id="org", graph_cascade=True)
        for k in GRAPH_KEYS:
            same(c2.index.graph[k], client.index.graph[k], "loaded " + k)
        assert c2.find_entities(["acme"]) == client.find_entities(["acme"]) and graph_hits(c2) == graph_hits(client) == []
        seeds = dev(np.array([[0, 3, -1], [5, -1, -1]], dtype=np.int32))
        same_results(c2.index.graph_search(seeds, 20, 2)[:3], client.index.graph_search(seeds, 20, 2)[:3], "loaded graph_search")
    finally:
        SETTINGS.__dict__.update(saved)
