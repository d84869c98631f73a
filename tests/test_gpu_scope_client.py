"""One GpuIndexClient over several tenants: every RPC and the graph channel rank inside the caller's
org -- the rows, order and scores of the batch API with ``scopes=`` and of the oracle over the org's
rows -- no foreign chunk anywhere, and a second request resolves no scope."""
import asyncio

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import thr_oracle as O  # noqa: E402

ORGS = ("acme", "bolt", "core")          # a wide tenant and two thinner ones
N_ROWS, DIM, N_ENT, N_WORDS = 3000, 256, 200, 400


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def org_of(i):
    return ORGS[(0, 0, 0, 0, 1, 1, 2)[i % 7]]


def corpus():
    rng = np.random.default_rng(77)
    words = [f"w{i}" for i in range(N_WORDS)]
    zipf = 1.0 / np.arange(1, N_WORDS + 1)
    zipf /= zipf.sum()
    emb = rng.standard_normal((N_ROWS, DIM)).astype(np.float32)
    children = []
    for i in range(N_ROWS):
        toks = rng.choice(N_WORDS, size=int(rng.integers(3, 40)), p=zipf)
        children.append({"id": f"c{i}", "parent_id": f"p{i // 4}", "document_id": f"d{i // 50}",
                         "text": " ".join(words[t] for t in toks), "page": 1 + i % 7, "modality": "text",
                         "collection": f"col{i % 3}", "org_id": org_of(i), "content_hash": f"h{i}",
                         "embedding_1024": emb[i].tolist()})
    parents = [{"id": f"p{j}", "text": f"parent text {j}", "section_heading": f"S{j % 9}"} for j in range(N_ROWS // 4)]
    ents = [{"id": f"e{j}", "name": f"entity{j}"} for j in range(N_ENT)]
    rels = [{"subject_entity_id": f"e{int(a)}", "object_entity_id": f"e{int(b)}"}
            for a, b in rng.integers(0, N_ENT, size=(600, 2))]
    mens = [{"entity_id": f"e{int(e)}", "child_chunk_id": f"c{int(c)}", "confidence": float(cf)}
            for e, c, cf in zip(rng.integers(0, N_ENT, 4000), rng.integers(0, N_ROWS, 4000),
                                rng.uniform(0.2, 1.0, 4000).astype(np.float32))]
    return rng, words, zipf, emb, children, parents, ents, rels, mens


def build(T, image=True):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    rng, words, zipf, emb, children, parents, ents, rels, mens = corpus()
    hi = IB.from_rows(children, parents, ents, rels, mens)
    idx = hi.to_gpu()
    kw = {}
    if image:
        image_rows = list(range(0, N_ROWS, 10))
        ximg = np.random.default_rng(5).standard_normal((len(image_rows), DIM)).astype(np.float32)
        kw = dict(image_index=T.GpuIndex().set_dense(ximg, shortlist="exact"), image_rows=image_rows)
    client = GpuIndexClient(idx, hi.store, **kw)
    assert client.multi_tenant and "org" in idx.attribute_names()
    return client, hi, idx, rng, words, zipf


def expected_rows(store, S, I, cnt, key, limit):
    ids, sc = I[0].tolist()[:int(cnt[0])], S[0].tolist()
    out = []
    for g, s in zip(ids[:limit], sc):
        i = g - store.doc_base
        out.append({"child_id": store.child_ids[i], "parent_id": store.parent_ids[i],
                    "document_id": store.document_ids[i], "text": store.texts[i], "page": store.pages[i],
                    "modality": store.modalities[i], key: s})
    return out


def in_org(store, rows, org, key="child_id"):
    return all(store.org_ids[store.row_index(r[key])] == org for r in rows)


def masked_graph(hi, seeds, hops, k, mask):
    s = O.graph_scores(hi.ent_rowptr, hi.ent_col, hi.men_rowptr, hi.men_chunk, hi.men_conf, [int(e) for e in seeds],
                       hops, len(mask))
    return O.topk_desc(np.where(mask, s, -np.inf), k)[1]


def test_every_rpc_ranks_inside_the_callers_org(T, monkeypatch):
    N = T._native
    client, hi, idx, rng, words, zipf = build(T)
    st = hi.store
    x = np.asarray(hi.docs)
    orgs = np.array(st.org_ids)
    colls = np.array(st.collections)
    code = client._org_code
    assert code == {"acme": 0, "bolt": 1, "core": 2}
    q = (x[17] + 0.7 * rng.standard_normal(DIM)).astype(np.float32)
    qimg = rng.standard_normal(DIM).astype(np.float32)
    text = f"{words[3]} {words[11]} {words[40]}"
    tids = np.array([[st.vocab[w] for w in text.split()]], dtype=np.int32)
    seeds = [5, 17, 120]
    seeds_t = dev(np.array([seeds], dtype=np.int32))

    def requests(org):
        p = {"p_org_id": org}
        out = {
            "semantic": client.rpc("rag2_semantic_search", dict(p, p_embedding=q.tolist(), p_limit=20)).execute().data,
            "semantic/col1": client.rpc("rag2_semantic_search", dict(p, p_embedding=q.tolist(), p_limit=20,
                                                                      p_collection="col1")).execute().data,
            "lexical": list(client.rpc("rag2_lexical_search", dict(p, p_query=text, p_limit=15)).execute().data),
            "lexical/col2": list(client.rpc("rag2_lexical_search", dict(p, p_query=text, p_limit=15,
                                                                        p_collection="col2")).execute().data),
            "deferred": list(client.rpc("rag2_lexical_search", dict(p, p_query=text, p_limit=15, _defer=True)).execute().data),
            "hybrid": client.rpc("rag2_hybrid_rrf_search", dict(p, p_query=text, p_embedding=q.tolist(),
                                                                p_limit=10)).execute().data,
            "kb_vector": client.rpc("kb_chunks_vector_search", dict(p, p_embedding=q.tolist(), p_limit=20)).execute().data,
            "kb_fts": client.rpc("kb_chunks_fts_pt", dict(p, p_query=text, p_limit=15)).execute().data,
            "kb_image": client.rpc("kb_chunks_image_search", dict(p, p_image_embedding=qimg.tolist(), p_limit=8)).execute().data,
            "graph": client.graph_chunks(seeds, 50, 2, org_id=org),
        }
        return out

    first = {org: requests(org) for org in ORGS}
    for org in ORGS:
        got, c = first[org], code[org]
        mine = orgs == org
        # --- the batch API over the same index with scopes=, formatted as the single-tenant client's rows
        S, I, cnt, _ = idx.dense_search(dev(q[None]), 20, scopes=[{"org": c}])
        assert got["semantic"] == expected_rows(st, S, I, cnt, "similarity", 20) and len(got["semantic"]) == 20
        S, I, cnt, _ = idx.dense_search(dev(q[None]), 20, scopes=[{"org": c, "collection": client._coll_id["col1"]}])
        assert got["semantic/col1"] == expected_rows(st, S, I, cnt, "similarity", 20)
        S, I, cnt = idx.bm25_search(dev(tids), 15, scopes=[{"org": c}])
        assert got["lexical"] == expected_rows(st, S, I, cnt, "rank", 15) == got["deferred"] and got["lexical"]
        S, I, cnt = idx.bm25_search(dev(tids), 15, scopes=[{"org": c, "collection": client._coll_id["col2"]}])
        assert got["lexical/col2"] == expected_rows(st, S, I, cnt, "rank", 15)
        S, I, cnt = idx.graph_search(seeds_t, 50, 2, scopes=[{"org": c}])
        assert got["graph"] == [st.child_ids[g] for g in I[0].tolist()[:int(cnt[0])]] and got["graph"]
        S, I, cnt, _ = client.image_index.dense_search(dev(qimg[None]), 8, scopes=[{"org": c}])
        assert [r["id"] for r in got["kb_image"]] == [st.child_ids[client.image_rows[j]] for j in I[0].tolist()[:int(cnt[0])]]
        assert [r["similarity"] for r in got["kb_image"]] == [float(np.float32(v)) for v in S[0].tolist()[:int(cnt[0])]]
        assert len(got["kb_image"]) == 8
        # --- the oracle over the org's rows
        s = np.where(mine, O.cosine_scores_f64(x, q), -np.inf)
        ts, ti = O.topk_desc(s, 20)
        assert [r["child_id"] for r in got["semantic"]] == [f"c{j}" for j in ti]
        assert [r["similarity"] for r in got["semantic"]] == list(ts)
        ts, ti = O.topk_desc(np.where(mine & (colls == "col1"), s, -np.inf), 20)
        assert [r["child_id"] for r in got["semantic/col1"]] == [f"c{j}" for j in ti]
        Sl, Il = O.bm25_topk(hi.rowptr, hi.post_doc, hi.post_tf, hi.doclen, hi.idf, hi.avgdl, tids, N_ROWS, 15,
                             doc_coll=mine.astype(np.int32), query_coll=[1])
        assert [r["child_id"] for r in got["lexical"]] == [f"c{j}" for j in Il[0]]
        assert [r["rank"] for r in got["lexical"]] == list(Sl[0])
        assert got["graph"] == [f"c{j}" for j in masked_graph(hi, seeds, 2, 50, mine)]
        # --- the calls built on those
        assert [r["id"] for r in got["kb_vector"]] == [r["child_id"] for r in got["semantic"]]
        assert [r["similarity"] for r in got["kb_vector"]] == [r["similarity"] for r in got["semantic"]]
        assert [r["id"] for r in got["kb_fts"]] == [r["child_id"] for r in got["lexical"]]
        assert [r["rank"] for r in got["kb_fts"]] == [r["rank"] for r in got["lexical"]]
        for legacy, rows in ((got["kb_vector"], got["semantic"]), (got["kb_fts"], got["lexical"])):
            assert [(r["content"], r["source_document"], r["page"]) for r in legacy] == \
                [(r["text"], r["document_id"], r["page"]) for r in rows]
        wide_l = client.rpc("rag2_lexical_search", {"p_org_id": org, "p_query": text, "p_limit": 20}).execute().data
        wide_s = client.rpc("rag2_semantic_search", {"p_org_id": org, "p_embedding": q.tolist(), "p_limit": 20}).execute().data
        lex_ids, sem_ids = ([int(r["child_id"][1:]) for r in rows] for rows in (wide_l, wide_s))
        fused, fused_sc = O.fused_topk_ids(lex_ids, sem_ids, None, 10)
        assert [r["child_id"] for r in got["hybrid"]] == [f"c{j}" for j in fused]
        assert [r["rrf_score"] for r in got["hybrid"]] == [float(np.float32(v)) for v in fused_sc]     # ::REAL
        assert [r["lexical_rank"] for r in got["hybrid"]] == [lex_ids.index(j) + 1 if j in lex_ids else None for j in fused]
        assert [r["semantic_rank"] for r in got["hybrid"]] == [sem_ids.index(j) + 1 if j in sem_ids else None for j in fused]
        assert all(r["text"] == st.texts[int(r["child_id"][1:])] and r["parent_id"] == st.parent_ids[int(r["child_id"][1:])]
                   for r in got["hybrid"])
        # --- no foreign chunk anywhere
        for name, rows in got.items():
            if name == "graph":
                assert all(orgs[st.row_index(cid)] == org for cid in rows), name
            else:
                assert rows and in_org(st, rows, org, "id" if name.startswith("kb_") else "child_id"), name
    # the filter is not vacuous: the unscoped lists hold other tenants' chunks
    _, I, _ = idx.graph_search(seeds_t, 50, 2)
    assert len({orgs[g] for g in I[0].tolist() if g >= 0}) > 1
    # a missing or unknown org: no rows, as WHERE org_id = $1 gives
    for p in ({}, {"p_org_id": None}, {"p_org_id": "nobody"}):
        assert client.rpc("rag2_semantic_search", dict(p, p_embedding=q.tolist(), p_limit=20)).execute().data == []
        assert list(client.rpc("rag2_lexical_search", dict(p, p_query=text, p_limit=15, _defer=True)).execute().data) == []
        assert client.rpc("rag2_hybrid_rrf_search", dict(p, p_query=text, p_embedding=q.tolist())).execute().data == []
        assert client.rpc("kb_chunks_vector_search", dict(p, p_embedding=q.tolist())).execute().data == []
        assert client.rpc("kb_chunks_fts_pt", dict(p, p_query=text)).execute().data == []
        assert client.rpc("kb_chunks_image_search", dict(p, p_image_embedding=qimg.tolist())).execute().data == []
        assert client.graph_chunks(seeds, 50, 2, org_id=p.get("p_org_id")) == []
    # a collection no row carries: no rows
    assert client.rpc("rag2_semantic_search", {"p_org_id": "acme", "p_embedding": q.tolist(),
                                               "p_collection": "nowhere"}).execute().data == []

    # a second request for the same (org, collection) resolves no scope
    def boom(*_a, **_kw):
        raise AssertionError("thr_scope_resolve was called for an (org, collection) seen before")
    monkeypatch.setattr(N, "scope_resolve", boom)
    for org in ORGS:
        assert requests(org) == first[org]
    with pytest.raises(AssertionError, match="seen before"):       # (the patch bites: a new pair does resolve)
        client.rpc("rag2_semantic_search", {"p_org_id": "core", "p_embedding": q.tolist(), "p_collection": "col0"})


def test_the_retriever_over_a_shared_client_stays_in_its_org(T):
    from triple_hybrid_rag_amd.config import SETTINGS
    from triple_hybrid_rag_amd.rag2.embedder import PrecomputedEmbedder
    from triple_hybrid_rag_amd.rag2.query_planner import QueryPlanner
    from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever
    client, hi, idx, rng, words, zipf = build(T, image=False)
    st = hi.store
    x = np.asarray(hi.docs)
    orgs = np.array(st.org_ids)
    graph_lists = []
    inner = client.graph_chunks

    def spy(seeds, top_k, hops=2, **kw):
        out = inner(seeds, top_k, hops, **kw)
        graph_lists.append((kw.get("org_id"), list(seeds), out))
        return out
    client.graph_chunks = spy
    saved = dict(SETTINGS.__dict__)
    SETTINGS.rag2_graph_enabled = True
    SETTINGS.rag2_safety_threshold = 0.0
    SETTINGS.rag2_denoise_alpha = 0.0
    try:
        emb = PrecomputedEmbedder(store_dim=DIM)
        leaked = False
        for qi, org in enumerate(("bolt", "core", "acme", "bolt")):
            kw = [words[int(t)] for t in rng.choice(60, size=3, replace=False)] + [f"entity{int(rng.integers(10, 99))}"]
            text = " ".join(kw)
            raw = np.concatenate([x[100 + qi] * 5.0 + rng.standard_normal(DIM).astype(np.float32),
                                  rng.standard_normal(64).astype(np.float32)])
            emb.register(text, raw.tolist())
            r = RAG2Retriever(org_id=org, embedder=emb, query_planner=QueryPlanner(graph=True), graph_enabled=True)
            r._supabase = client
            res = asyncio.run(r.retrieve(text, top_k=10, skip_rerank=True))
            assert res.success and not res.refused and len(res.contexts) == 10
            assert all(orgs[st.row_index(c.child_id)] == org for c in res.contexts)
            # the graph channel ran, inside the org
            got_org, seeds, chunk_ids = graph_lists[-1]
            assert got_org == org and seeds == client.find_entities(kw, 50) and chunk_ids
            assert all(orgs[st.row_index(cid)] == org for cid in chunk_ids)
            _, Iu, _ = idx.graph_search(dev(np.array([seeds + [-1] * (16 - len(seeds))], dtype=np.int32)), 50, 2)
            leaked |= any(orgs[g] != org for g in Iu[0].tolist() if g >= 0)
            # the oracle pipeline over the org's rows
            mine = orgs == org
            qv = np.asarray(emb.embed_query(text), dtype=np.float32)
            _, Id = O.topk_desc(np.where(mine, O.cosine_scores_f64(x, qv), -np.inf), 100)
            tids = [st.vocab[w] for w in kw if w in st.vocab]
            _, Il = O.bm25_topk(hi.rowptr, hi.post_doc, hi.post_tf, hi.doclen, hi.idf, hi.avgdl, [tids], N_ROWS, 50,
                                doc_coll=mine.astype(np.int32), query_coll=[1])
            Ig = masked_graph(hi, seeds, 2, 50, mine)
            assert chunk_ids == [f"c{j}" for j in Ig]
            ei, es = O.fused_topk_ids(list(Il[0]), list(Id), list(Ig), 10)
            assert [c.child_id for c in res.contexts] == [f"c{i}" for i in ei]
            assert [c.rrf_score for c in res.contexts] == es
        assert leaked       # without the filter some query's graph list would have left its org
        r = RAG2Retriever(org_id="nobody", embedder=emb, query_planner=QueryPlanner(graph=True), graph_enabled=True)
        r._supabase = client
        res = asyncio.run(r.retrieve(text, top_k=10, skip_rerank=True))
        assert res.refused and res.refusal_reason == "No candidates found"
    finally:
        SETTINGS.__dict__.update(saved)


def test_insert_delete_by_org_save_and_load(T, tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    client, hi, idx, rng, words, zipf = build(T, image=False)
    st = hi.store
    vec = rng.standard_normal((8, DIM)).astype(np.float32)
    new = [{"id": f"n{j}", "parent_id": "p0", "document_id": "dnew", "text": f"zebra quagga {words[3]} n{j}", "page": 2,
            "modality": "text", "collection": "col1", "org_id": "aardvark" if j < 5 else "bolt",
            "content_hash": f"hn{j}", "embedding_1024": vec[j].tolist(), "mentions": [(3, 0.9), (7, 0.5)]}
           for j in range(8)]
    table = lambda: client.table("rag_child_chunks")      # noqa: E731
    with pytest.raises(ValueError, match="every row needs its org_id"):
        table().insert([dict(new[0], org_id=None)]).execute()
    assert idx.n_docs == N_ROWS
    assert table().insert(new).execute().data == [{"id": f"n{j}"} for j in range(8)]
    assert idx.n_docs == N_ROWS + 8 and st.org_ids[-8:] == ["aardvark"] * 5 + ["bolt"] * 3
    # (an org that sorts before the others got the next id: ids never move)
    assert client._org_code == {"acme": 0, "bolt": 1, "core": 2, "aardvark": 3}
    assert idx.attribute("org")[-8:].tolist() == [3] * 5 + [1] * 3

    def sem(c, org, j, **kw):
        return c.rpc("rag2_semantic_search", dict({"p_org_id": org, "p_embedding": vec[j].tolist(), "p_limit": 10}, **kw)).execute().data
    assert [r["child_id"] for r in sem(client, "aardvark", 0)] [0] == "n0"
    assert sorted(r["child_id"] for r in sem(client, "aardvark", 0)) == [f"n{j}" for j in range(5)]    # the org's five rows
    assert sem(client, "bolt", 6)[0]["child_id"] == "n6" and sem(client, "bolt", 0)[0]["child_id"] != "n0"
    assert not any(r["child_id"].startswith("n") for r in sem(client, "acme", 0) + sem(client, "core", 6))
    assert sem(client, "aardvark", 0, p_collection="col0") == []
    lex = client.rpc("rag2_lexical_search", {"p_org_id": "aardvark", "p_query": "zebra quagga", "p_limit": 10}).execute().data
    assert sorted(r["child_id"] for r in lex) == [f"n{j}" for j in range(5)]
    assert client.rpc("rag2_lexical_search", {"p_org_id": "core", "p_query": "zebra quagga", "p_limit": 10}).execute().data == []
    assert sorted(client.graph_chunks([3], 50, 0, org_id="aardvark")) == [f"n{j}" for j in range(5)]
    assert not any(c.startswith("n") for c in client.graph_chunks([3], 50, 0, org_id="acme"))
    # reads inside an org
    assert [r["id"] for r in table().select("*").eq("org_id", "bolt").in_("id", ["n0", "n6", "c4", "c0"]).execute().data] == ["n6", "c4"]
    assert table().select("content_hash").eq("org_id", "aardvark").in_("content_hash", ["hn0", "hn6", "h4"]).execute().data == \
        [{"content_hash": "hn0"}]
    # delete by org: that tenant's rows, nobody else's
    gone = table().delete().eq("org_id", "aardvark").execute().data
    assert [r["id"] for r in gone] == [f"n{j}" for j in range(5)] and idx.n_docs == N_ROWS + 3
    assert sem(client, "aardvark", 0) == [] and client.graph_chunks([3], 50, 0, org_id="aardvark") == []
    assert sem(client, "bolt", 6)[0]["child_id"] == "n6"
    assert table().delete().eq("org_id", "core").eq("id", "n6").execute().data == []      # another org's row: untouched
    assert [r["id"] for r in table().delete().eq("org_id", "bolt").in_("id", ["n7", "c0"]).execute().data] == ["n7"]
    assert idx.n_docs == N_ROWS + 2 == len(st.child_ids) == len(st.org_ids)
    # an org without rows is no tenant any more; the others are listed
    assert client.table("organizations").select("id").execute().data == [{"id": o} for o in ("acme", "bolt", "core")]
    assert client.table("rag_documents").select("org_id").eq("org_id", "aardvark").execute().data == []
    # documents and parents of this corpus span orgs (d0 = c0..c49, p0 = c0..c3): a delete inside an org
    # takes that org's chunks only, and what other orgs' chunks still name stays
    mine = [f"c{i}" for i in range(50) if org_of(i) == "core"]
    n_before = idx.n_docs
    assert client.table("rag_documents").delete().eq("org_id", "core").eq("id", "d0").execute().data == []   # (d0 lives on)
    assert idx.n_docs == n_before - len(mine) and all(st.row_index(c) is None for c in mine)
    assert all(st.row_index(f"c{i}") is not None for i in range(50) if org_of(i) != "core")
    assert "p0" in st.parents and "p1" in st.parents            # (c6 was core's; c4, c5, c7 are not)
    ptab = lambda: client.table("rag_parent_chunks")      # noqa: E731
    assert [r["id"] for r in ptab().select("*").eq("org_id", "bolt").in_("id", ["p0", "p1", "p5"]).execute().data] == ["p0", "p1"]    # (p0: the inserted n5, n6; p5: acme and core only)
    assert [r["id"] for r in ptab().select("*").in_("id", ["p0", "p1"]).execute().data] == ["p0", "p1"]
    assert ptab().delete().eq("org_id", "bolt").eq("id", "p1").execute().data == []      # c7 (acme) still names p1
    assert st.row_index("c4") is None and st.row_index("c5") is None and st.row_index("c7") is not None
    gone_p = ptab().delete().eq("org_id", "acme").eq("id", "p1").execute().data
    assert [r["id"] for r in gone_p] == ["p1"] and "p1" not in st.parents and st.row_index("c7") is None
    assert len(st.child_ids) == len(st.org_ids) == idx.n_docs
    # save -> load: the same answers from a fresh client over the loaded directory
    IB.save(hi, str(tmp_path / "ix"), idx)
    back = IB.load(str(tmp_path / "ix"))
    assert list(back.store.org_ids) == st.org_ids
    client2 = GpuIndexClient(back.to_gpu(), back.store)
    assert client2.multi_tenant and client2._org_code == {"acme": 0, "bolt": 1, "core": 2}
    text = f"{words[3]} {words[11]}"
    for org in ORGS + ("aardvark",):
        assert sem(client2, org, 6) == sem(client, org, 6)
        a, b = (c.rpc("rag2_lexical_search", {"p_org_id": org, "p_query": text, "p_limit": 15}).execute().data
                for c in (client, client2))
        assert a == b
        assert client2.graph_chunks([3, 50], 50, 2, org_id=org) == client.graph_chunks([3, 50], 50, 2, org_id=org)
    assert sem(client2, "bolt", 6)[0]["child_id"] == "n6"
