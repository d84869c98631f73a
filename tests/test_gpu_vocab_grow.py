"""Numbering new BM25 terms on the GPU (thr_vocab_grow and the Python surface over it: number_text_rows /
commit_vocabulary, GpuIndexClient(number_on_device=True), from_rows(device="text")), held array for array to
plain Python on the CPU: the restatement of tests/vocab_grow_cases.py, text_rows + the host numbering, the twin
client and from_rows()."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_cases as TC  # noqa: E402
import vocab_grow_cases as VG  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GUARD = 64                      # elements behind every output that must stay as they were
FILL32, FILL8, FILL64 = 0x5A5A5A5A, 0xA5, -0x0123456789ABCDEF


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def ids_of(vocab):
    return {t: i for i, t in enumerate(vocab)}


def index_with(T, vocab, table=None):
    return T.GpuIndex().set_vocabulary(vocab, table)


# ------------------------------------------------------------------ the raw ABI
def raw_grow(T, idx, blobs, hash_mask=VG.ALL_ONES, room=None):
    """thr_text_tokens, then thr_vocab_grow through the library itself into buffers with guard elements behind
    them -> (what the device wrote, the restatement over the same unknown list)."""
    N = T._native
    lib = N.load()
    blobs = [b if isinstance(b, bytes) else TC.enc(b) for b in blobs]
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    raw = b"".join(blobs)
    n_bytes = len(raw)
    X = idx.text
    n_vocab = X["term_ptr"].shape[0] - 1
    bytes_dev, ptr_dev = dev(np.frombuffer(raw + bytes(16), dtype=np.uint8)), dev(ptr)
    rows = N.text_tokens(bytes_dev, ptr_dev, n_bytes, X["table_dev"], X["slots"], X["term_bytes"], X["term_ptr"])
    n_total, n_unknown = int(rows["n_total"].item()), int(rows["n_unknown"].item())
    E = VG.expect_grow(raw, ptr, rows["flags"].cpu().numpy(), rows["unknown_off"][:n_unknown].cpu().numpy(),
                       rows["unknown_len"][:n_unknown].cpu().numpy(), n_vocab, X["table"], hash_mask,
                       tok_term=rows["term"][:n_total].cpu().numpy())
    U = max(n_unknown, 1)
    room = E["n_new_bytes"] if room is None else room
    i32, i64 = torch.int32, torch.int64
    unknown_term = torch.full((U + GUARD,), FILL32, dtype=i32, device="cuda")
    new_bytes = torch.full((room + GUARD,), FILL8, dtype=torch.uint8, device="cuda")
    new_ptr = torch.full((U + 1 + GUARD,), FILL64, dtype=i64, device="cuda")
    tok = torch.cat([rows["term"][:n_total], torch.full((GUARD,), -9, dtype=i32, device="cuda")])
    n_new = torch.full((1 + GUARD,), FILL32, dtype=i32, device="cuda")
    n_new_bytes = torch.full((1 + GUARD,), FILL64, dtype=i64, device="cuda")
    status = torch.full((1 + GUARD,), FILL32, dtype=i32, device="cuda")
    need = int(lib.thr_vocab_grow_workspace_bytes(U))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.thr_vocab_grow(bytes_dev.data_ptr(), ptr_dev.data_ptr(), len(blobs), n_bytes, X["table_dev"].data_ptr(),
                            rows["flags"].data_ptr(), rows["unknown_off"].data_ptr(), rows["unknown_len"].data_ptr(),
                            rows["n_unknown"].data_ptr(), U, n_vocab, hash_mask,
                            tok.data_ptr() if n_total else None, rows["n_total"].data_ptr(), n_total,
                            unknown_term.data_ptr(), new_bytes.data_ptr(), room, new_ptr.data_ptr(), n_new.data_ptr(),
                            n_new_bytes.data_ptr(), status.data_ptr(), ws.data_ptr(), need,
                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = dict(unknown_term=unknown_term.cpu().numpy(), new_bytes=new_bytes.cpu().numpy(), new_ptr=new_ptr.cpu().numpy(),
               tok_term=tok.cpu().numpy(), n_new=n_new.cpu().numpy(), n_new_bytes=n_new_bytes.cpu().numpy(),
               status=status.cpu().numpy(), n_unknown=n_unknown, n_total=n_total, room=room)
    return got, E


def assert_grow(got, E):
    """Array for array; the elements behind every output are as they were."""
    n, room = got["n_unknown"], got["room"]
    overflow = E["n_new_bytes"] > room
    want = (VG.COLLISION if E["collision"] else 0) | (VG.OVERFLOW if overflow else 0)
    assert got["status"][0] == want, ("status", got["status"][0], want)
    assert (got["status"][1:] == FILL32).all() and (got["n_new"][1:] == FILL32).all() and (got["n_new_bytes"][1:] == FILL64).all()
    assert (got["unknown_term"][n:] == FILL32).all(), "unknown_term: written behind n_unknown"
    assert (got["new_bytes"][room:] == FILL8).all(), "new_bytes: written at or behind the capacity"
    assert (got["tok_term"][got["n_total"]:] == -9).all(), "tok_term: written behind n_total"
    if E["collision"]:
        return                      # the status bit is the whole promise
    assert got["n_new"][0] == E["n_new"] and got["n_new_bytes"][0] == E["n_new_bytes"]
    assert np.array_equal(got["unknown_term"][:n], E["unknown_term"]), "unknown_term"
    assert np.array_equal(got["new_ptr"][:E["n_new"] + 1], E["new_ptr"]), "new_ptr"
    assert (got["new_ptr"][E["n_new"] + 1:] == FILL64).all(), "new_ptr: written behind n_new + 1"
    kept = min(room, E["n_new_bytes"])
    assert np.array_equal(got["new_bytes"][:kept], E["new_bytes"][:kept]), "new_bytes"
    assert (got["new_bytes"][kept:] == FILL8).all()
    assert np.array_equal(got["tok_term"][:got["n_total"]], E["tok_term"]), "tok_term"


CASES = VG.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_raw_outputs_equal_the_restatement(T, case):
    assert case.holds()
    idx = index_with(T, case.vocab)
    got, E = raw_grow(T, idx, case.texts, hash_mask=case.hash_mask)
    assert got["n_unknown"] == VG.n_unknown_of(case)
    assert_grow(got, E)
    if case.hash_mask == VG.ALL_ONES:
        # ... and the restatement over the device's list is the host loop over the texts
        doc, term, grown = VG.expect_numbered(case.texts, ids_of(case.vocab))
        assert E["keys"] == grown and np.array_equal(got["tok_term"][:got["n_total"]], term)
        assert (got["tok_term"][:got["n_total"]] >= 0).all()
    else:
        assert E["collision"] and got["status"][0] & VG.COLLISION
        got, E = raw_grow(T, idx, case.texts)                 # the same input under the full hash: clear
        assert not E["collision"] and got["status"][0] == 0
        assert_grow(got, E)


def test_every_token_known_writes_nothing(T):
    case = VG.all_known_case()
    got, E = raw_grow(T, index_with(T, case.vocab), case.texts, room=32)
    assert got["n_unknown"] == 0 and got["status"][0] == 0 and got["n_new"][0] == 0 and got["n_new_bytes"][0] == 0
    assert (got["unknown_term"] == FILL32).all() and (got["new_bytes"] == FILL8).all()
    assert got["new_ptr"][0] == 0 and (got["new_ptr"][1:] == FILL64).all()
    assert np.array_equal(got["tok_term"][:got["n_total"]], E["tok_term"]) and (E["tok_term"] >= 0).all()


def test_malformed_text_is_not_numbered_and_its_neighbours_are_as_if_it_were_not_there(T):
    idx = index_with(T, ["um"])
    got, E = raw_grow(T, idx, VG.MALFORMED)
    assert_grow(got, E)
    assert E["keys"] == ["novo", "dois", "tres", "malo"]         # "dois" and "malo" from their later sightings
    without, E2 = raw_grow(T, idx, [b for i, b in enumerate(VG.MALFORMED) if i != 1])
    assert E2["keys"] == E["keys"] and bytes(got["new_bytes"][:got["room"]]) == bytes(without["new_bytes"][:without["room"]])
    n = got["n_unknown"]
    assert (got["unknown_term"][:n] == -1).sum() == 3 and b"\xe2" not in bytes(got["new_bytes"][:got["room"]])
    assert np.array_equal(got["unknown_term"][:n][got["unknown_term"][:n] >= 0], without["unknown_term"][:without["n_unknown"]])
    bad = got["tok_term"][:got["n_total"]]
    assert (bad == -1).sum() == 3                                 # its rows stay -1


def test_new_bytes_capacity_one_byte_short_reports_the_need_and_writes_nothing_behind_it(T):
    case = VG.spelling_case()
    idx = index_with(T, case.vocab)
    full, E = raw_grow(T, idx, case.texts)
    got, _ = raw_grow(T, idx, case.texts, room=E["n_new_bytes"] - 1)
    assert got["status"][0] == VG.OVERFLOW and got["n_new_bytes"][0] == E["n_new_bytes"] and got["n_new"][0] == E["n_new"]
    assert_grow(got, E)
    assert full["status"][0] == 0 and np.array_equal(full["unknown_term"], got["unknown_term"])


@pytest.mark.parametrize("name", ["n_unknown_3100", "one_new_token_100000_times_among_50_others"])
def test_two_runs_of_one_input_give_the_same_bytes(T, name):
    case = next(c for c in CASES if c.name == name)
    idx = index_with(T, case.vocab)
    a, _ = raw_grow(T, idx, case.texts)
    b, _ = raw_grow(T, idx, case.texts)
    for key in ("unknown_term", "new_bytes", "new_ptr", "tok_term", "n_new", "n_new_bytes", "status"):
        assert a[key].tobytes() == b[key].tobytes(), key


# ------------------------------------------------------------------ number_text_rows + commit_vocabulary
def host_numbered(twin, texts):
    """text_rows + the host numbering (insert_children's) on an index of the same vocabulary."""
    n_before = len(twin.text["ids"])
    R = twin.text_rows(texts)
    term = R.term.cpu().numpy().copy()
    term[term < 0] = n_before + R.unknown_which
    return R.doc.cpu().numpy(), term.astype(np.int32), list(R.unknown)


def key_store(idx):
    X = idx.text
    return X["term_bytes"][:X["n_bytes"]].cpu().numpy().tobytes(), X["term_ptr"].cpu().numpy()


SURFACE = TC.all_cases()


@pytest.mark.parametrize("case", SURFACE, ids=[c.name for c in SURFACE])
def test_number_and_commit_equal_text_rows_and_the_host_numbering(T, case):
    half = case.vocab[::2]
    idx, twin = index_with(T, half), index_with(T, half)
    slots_before, store_before = idx.text["slots"].clone(), key_store(idx)
    R = idx.number_text_rows(case.texts)
    doc, term, unknown = host_numbered(twin, case.texts)
    assert np.array_equal(R.doc.cpu().numpy(), doc) and np.array_equal(R.term.cpu().numpy(), term)
    assert (term >= 0).all() and R.n_before == len(half) and R.pending.n_new == len(unknown)
    assert R.pending.terms == unknown
    exceptional = bool(idx.text["table"].exceptional_among(case.texts))
    assert (R.pending.key_bytes is None) == (exceptional or not unknown)       # the fallback, and only then
    # until the commit the device vocabulary is exactly as before
    assert torch.equal(idx.text["slots"], slots_before) and key_store(idx)[0] == store_before[0]
    assert np.array_equal(key_store(idx)[1], store_before[1]) and idx.text["ids"] == ids_of(half)
    idx.commit_vocabulary(R.pending)
    twin.grow_vocabulary(unknown)
    assert idx.text["ids"] == twin.text["ids"] and list(idx.text["ids"]) == half + unknown
    assert key_store(idx)[0] == key_store(twin)[0] and np.array_equal(key_store(idx)[1], key_store(twin)[1])
    assert idx.text["slots"].shape == twin.text["slots"].shape
    # afterwards the device finds the new terms: query_terms over texts that use them equals the host table
    texts = case.texts[:3000]
    got, flags = idx.query_terms(texts)
    want, _, wflags = TC.expect_query_table(texts, idx.text["ids"])
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(flags.cpu().numpy(), wflags)
    assert not (wflags & T._native.THR_TEXT_UNKNOWN).any()
    with pytest.raises(ValueError, match="numbered from"):
        idx.commit_vocabulary(R.pending) if R.pending.n_new else idx.commit_vocabulary(
            type(R.pending)(R.n_before + 1, 1, terms=["zzzz"]))


def test_collision_fallback_forced_through_the_wrapper_gives_the_same_values(T):
    case = VG.masked_case()
    idx = index_with(T, ["m3", "zz"])
    plain = idx.number_text_rows(case.texts)
    forced = idx.number_text_rows(case.texts, hash_mask=0x7)
    assert plain.pending.key_bytes is not None and forced.pending.key_bytes is None       # the host answered
    assert torch.equal(plain.doc, forced.doc) and torch.equal(plain.term, forced.term)
    assert plain.pending.terms == forced.pending.terms and plain.pending.n_new == forced.pending.n_new == 39
    assert plain.n_before == forced.n_before == 2
    doc, term, grown = VG.expect_numbered(case.texts, ids_of(["m3", "zz"]))
    assert np.array_equal(forced.term.cpu().numpy(), term) and forced.pending.terms == grown
    idx.commit_vocabulary(forced.pending)
    assert list(idx.text["ids"]) == ["m3", "zz"] + grown
    got, flags = idx.query_terms(case.texts)
    want, _, wflags = TC.expect_query_table(case.texts, idx.text["ids"])
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(flags.cpu().numpy(), wflags)


def test_a_key_longer_than_the_first_guess_is_a_second_call_with_the_reported_size(T):
    idx = index_with(T, ["q"])
    long = "Ⱥ" * 40 + "x"                  # one unknown occurrence: 16 bytes of room, 121 lowered bytes
    R = idx.number_text_rows(["q " + long + " q", long.lower()])
    assert R.term.tolist() == [0, 1, 0, 1] and R.pending.terms == [long.lower()]
    assert R.pending.n_key_bytes == len(TC.enc(long.lower())) == 121
    idx.commit_vocabulary(R.pending)
    assert idx.query_terms([long])[0][0, 0].item() == 1
    empty = idx.number_text_rows([])
    assert empty.doc.numel() == 0 and empty.pending.n_new == 0 and empty.n_before == 2


# ------------------------------------------------------------------ twin clients
def _rows(texts, d, seed, first=0, tokens=None):
    rng = np.random.default_rng(seed)
    out = [{"id": f"c{first + i}", "parent_id": "p0", "document_id": "d0", "text": t, "page": 1, "modality": "text",
            "embedding_1024": rng.standard_normal(d).astype(np.float32).tolist(), "org_id": "org"}
           for i, t in enumerate(texts)]
    if tokens is not None:
        for r in out:
            r["tokens"] = rng.standard_normal(tokens).astype(np.float16)
    return out


PARENTS = [{"id": "p0", "text": "parent", "section_heading": "S"}]


def _client(T, rows, tokens=None, **kw):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    hi = IB.from_rows(rows, PARENTS)
    if tokens is not None:
        hi.tokens = np.stack([r["tokens"] for r in rows])
    return GpuIndexClient(hi.to_gpu(), hi.store, org_id="org", device_text=True, **kw), hi


def _same_index(a, b):
    from test_gpu_append import _assert_lex_equal, same
    same(a.docs, b.docs, "docs")
    _assert_lex_equal(a, b)


def _same_vocabulary(a, b, texts):
    assert list(a.store.vocab.items()) == list(b.store.vocab.items())
    assert a.index.text["ids"] == a.store.vocab and b.index.text["ids"] == b.store.vocab
    assert key_store(a.index)[0] == key_store(b.index)[0] and np.array_equal(key_store(a.index)[1], key_store(b.index)[1])
    assert a.index.text["slots"].shape == b.index.text["slots"].shape
    qa, qb = a.query_terms_batch(texts), b.query_terms_batch(texts)
    assert torch.equal(qa, qb)
    want, _, _ = TC.expect_query_table(texts, a.store.vocab)
    assert np.array_equal(qa.cpu().numpy(), want)


def test_twin_clients_over_two_inserts_the_second_crossing_a_reallocation(T):
    d = 1024
    rng = np.random.default_rng(3)
    words = [f"w{i}" for i in range(215)]
    base = _rows([" ".join(words[i:i + 5]) for i in range(0, 215, 5)] +
                 [" ".join(rng.choice(words, 10)) for _ in range(200)], d, 1)
    first = ["novo termo w1 novo", "", "w2 İstanbul primeiro termo", "outro novo W3 primeiro", "  ,, ",
             "İstanbul de novo ΣΟΣ"] + [" ".join(rng.choice(words + ["raro", "Novo", "ȺB"], 8)) for _ in range(40)]
    second = [" ".join(f"fresh{i + j}" for j in range(4)) + " novo i̇stanbul W7" for i in range(0, 60, 3)] + ["ⱥb σος w1"]
    host, _ = _client(T, base)
    devc, _ = _client(T, base, number_on_device=True)
    assert len(host.store.vocab) == 215 and host.index.text["slots"].shape[0] == 512
    for texts, at, slots in ((first, 1000, 512), (second, 2000, 1024)):
        rows = _rows(texts, d, at, at)
        assert host.insert_children(rows) == devc.insert_children(rows)
        _same_index(host.index, devc.index)
        _same_vocabulary(host, devc, texts + ["novo raro w5", "nenhum"])
        assert devc.index.text["slots"].shape[0] == slots, len(devc.store.vocab)
    assert 256 < len(devc.store.vocab) <= 512
    for q in ("novo termo", "İstanbul primeiro", "fresh10 w7", "nenhum"):
        for conj in (False, True):
            host.lexical_and = devc.lexical_and = conj
            a = host.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": q, "p_limit": 10}).data
            b = devc.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": q, "p_limit": 10}).data
            assert list(a) == list(b), (q, conj)
    assert list(devc.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": "fresh10", "p_limit": 5}).data)


def test_a_refused_insert_leaves_everything_untouched_and_the_corrected_one_equals_the_twin(T, tmp_path):
    import asyncio
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.config import SETTINGS
    from triple_hybrid_rag_amd.rag2.embedder import PrecomputedEmbedder
    from triple_hybrid_rag_amd.rag2.query_planner import QueryPlanner
    from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever
    d, tok = 1024, (32, 16)
    rng = np.random.default_rng(5)
    words = [f"w{i}" for i in range(100)]
    base = _rows([" ".join(rng.choice(words, 10)) for _ in range(120)], d, 1, tokens=tok)
    host, _ = _client(T, base, tokens=tok)
    devc, hi = _client(T, base, tokens=tok, number_on_device=True)
    texts = ["um termo novo w1", "outro Termo raro novo", "w2 w3"]
    rows = _rows(texts, d, 7, 500, tokens=tok)
    broken = [dict(r) for r in rows]
    del broken[1]["tokens"]
    X = devc.index.text
    before = (X["term_ptr"].clone(), X["slots"].clone(), key_store(devc.index)[0], list(devc.store.vocab.items()),
              devc.index.n_docs, len(devc.store.child_ids))
    with pytest.raises(ValueError, match="tokens"):
        devc.insert_children(broken)
    X = devc.index.text
    assert torch.equal(X["term_ptr"], before[0]) and torch.equal(X["slots"], before[1]) and key_store(devc.index)[0] == before[2]
    assert list(devc.store.vocab.items()) == before[3] and X["ids"] == devc.store.vocab
    assert (devc.index.n_docs, len(devc.store.child_ids)) == before[4:]
    assert host.insert_children(rows) == devc.insert_children(rows)
    _same_index(host.index, devc.index)
    _same_vocabulary(host, devc, texts)
    assert list(devc.store.vocab)[-5:] == ["um", "termo", "novo", "outro", "raro"]
    # retrieve, then save and load
    saved = dict(SETTINGS.__dict__)
    SETTINGS.rag2_safety_threshold = 0.0
    SETTINGS.rag2_denoise_alpha = 0.0
    try:
        e = PrecomputedEmbedder(store_dim=d)
        e.register("outro termo raro", rows[1]["embedding_1024"])
        r = RAG2Retriever(org_id="org", embedder=e, query_planner=QueryPlanner())
        r._supabase = devc
        res = asyncio.run(r.retrieve("outro termo raro", top_k=5, skip_rerank=True))
        assert res.success and res.contexts[0].child_id == "c501"
    finally:
        SETTINGS.__dict__.update(saved)
    hi.tokens = np.concatenate([hi.tokens, np.stack([r["tokens"] for r in rows])])
    path = str(tmp_path / "idx")
    IB.save(hi, path, devc.index)
    back = IB.load(path)
    assert list(back.store.vocab.items()) == list(devc.store.vocab.items())
    again = GpuIndexClient(back.to_gpu(), back.store, org_id="org", device_text=True, number_on_device=True)
    for k in ("rowptr", "post_doc", "post_tf", "doclen", "idf"):
        assert torch.equal(again.index.lex[k], devc.index.lex[k]), k
    a = devc.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": "outro termo raro", "p_limit": 5}).data
    b = again.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": "outro termo raro", "p_limit": 5}).data
    assert list(a) == list(b) and list(a)[0]["child_id"] == "c501"


# ------------------------------------------------------------------ from_rows(device="text")
def _chunks(texts):
    return [{"id": f"c{i}", "parent_id": "p0", "document_id": "d0", "text": t, "embedding_1024": [float(i % 7), 1.0, 0.0, 2.0]}
            for i, t in enumerate(texts)]


def _corpus():
    rng = np.random.default_rng(17)
    words = [f"w{i}" for i in range(300)] + ["Ação", "RAZÃO", "coração", "Hello", "HELLO", "ȺB", "ⱥb", "x²"]
    texts = [" ".join(rng.choice(words, rng.integers(3, 12))) + f" doc{i}" for i in range(400)]
    texts[57] = ""
    texts[211] = "uma İstanbul no meio w5 nunca_visto"
    texts[212] = "nunca_visto depois"
    return texts


def assert_same_host_index(a, b):
    for name in ("docs", "rowptr", "post_doc", "post_tf", "doclen", "idf"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), name
    assert a.avgdl == b.avgdl
    assert list(a.store.vocab.items()) == list(b.store.vocab.items())
    assert list(a.store.texts) == list(b.store.texts) and list(a.store.child_ids) == list(b.store.child_ids)


@pytest.mark.parametrize("fold", [False, True], ids=["default_table", "fold_accents_table"])
def test_from_rows_device_text_equals_from_rows(T, fold):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.index_text import TextTable, fold_accents
    texts = _corpus()
    kw = {"tokenizer": TextTable.from_char_map(fold_accents).tokenize} if fold else {}
    sizes = np.cumsum([len(TC.enc(t)) for t in texts])
    assert sizes[-1] > 3 * 4096 and sizes[56] < 4096 < sizes[211]                # batches split mid-corpus
    want = IB.from_rows(_chunks(texts), PARENTS, **kw)
    got = IB.from_rows(_chunks(texts), PARENTS, device="text", batch_bytes=4096, **kw)
    assert_same_host_index(got, want)
    assert ("acao" in got.store.vocab) == fold and "nunca_visto" in got.store.vocab
    one = IB.from_rows(_chunks(texts), PARENTS, device="text", **kw)               # one batch: the default size
    assert_same_host_index(one, want)


def test_from_rows_device_text_of_a_corpus_without_tokens_and_a_foreign_tokenizer(T):
    from triple_hybrid_rag_amd import index_build as IB
    texts = ["", "  ,, ", "—§", ""]
    assert_same_host_index(IB.from_rows(_chunks(texts), PARENTS, device="text", batch_bytes=4),
                           IB.from_rows(_chunks(texts), PARENTS))

    def my_tokenizer(text):
        return text.split()
    with pytest.raises(ValueError, match="my_tokenizer"):
        IB.from_rows(_chunks(["a b"]), PARENTS, tokenizer=my_tokenizer, device="text")
