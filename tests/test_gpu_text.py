"""Text to BM25 term ids on the GPU (thr_vocab_insert, thr_text_tokens, thr_query_terms and the Python surface
over them), held array for array to plain Python on the CPU: backend.tokenize, a dict lookup and
_query_terms (tests/text_cases.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

S = TC.S
MT = TC.MT


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def index_with(T, vocab, table=None):
    return T.GpuIndex().set_vocabulary(vocab, table)


def device_rows(idx, texts):
    """The raw outputs of one thr_text_tokens call over the texts, on the host."""
    rows = idx._text_tokens(texts)
    torch.cuda.synchronize()
    n_total, n_unknown = int(rows["n_total"].item()), int(rows["n_unknown"].item())
    assert 0 <= n_total <= rows["capacity"] and 0 <= n_unknown <= n_total
    return dict(doc=rows["doc"][:n_total].cpu().numpy(), term=rows["term"][:n_total].cpu().numpy(),
                n_tokens=rows["n_tokens"].cpu().numpy(), flags=rows["flags"].cpu().numpy(),
                unknown_off=rows["unknown_off"][:n_unknown].cpu().numpy(),
                unknown_len=rows["unknown_len"][:n_unknown].cpu().numpy(), blob=rows["blob"], ptr=rows["ptr"], raw=rows)


def assert_rows(got, texts, ids, table=None):
    """doc, term, n_tokens and flags array for array against the restatement; the rows of a flagged text may
    hold anything, in their place and n_tokens in number."""
    doc, term, n_tokens, flags = TC.expect_rows(texts, ids, table)
    assert np.array_equal(got["flags"], flags), "flags"
    ok = flags == 0
    assert np.array_equal(got["n_tokens"][ok], n_tokens[ok]), "n_tokens"
    assert (got["n_tokens"] >= 0).all() and int(got["n_tokens"].sum()) == got["doc"].shape[0]
    assert np.array_equal(got["doc"], np.repeat(np.arange(len(texts), dtype=np.int32), got["n_tokens"])), "doc"
    if ok.all():
        assert np.array_equal(got["doc"], doc) and np.array_equal(got["term"], term), "rows"
    else:
        assert np.array_equal(got["term"][ok[got["doc"]]], term[ok[doc]]), "term"
    # the unknown tokens of the plain texts: where they are and how long
    tokenizer = TC.backend.tokenize if table is None else table.tokenize
    want = [tok for d, t in enumerate(texts) if ok[d] for tok in tokenizer(t) if tok not in ids]
    of_text = np.searchsorted(got["ptr"], got["unknown_off"], side="right") - 1
    raw = got["blob"].tobytes()
    have = [tokenizer(raw[o:o + l].decode("utf-8", "surrogatepass"))
            for o, l, d in zip(got["unknown_off"].tolist(), got["unknown_len"].tolist(), of_text.tolist()) if ok[d]]
    assert have == [[w] for w in want], "unknown tokens"


def ids_of(vocab):
    return {t: i for i, t in enumerate(vocab)}


ROW_CASES = TC.slice_cases() + TC.boundary_cases() + TC.lowering_cases() + TC.exceptional_cases()


@pytest.mark.parametrize("case", ROW_CASES, ids=[c.name for c in ROW_CASES])
def test_token_rows_equal_the_restatement(T, case):
    assert case.holds()
    idx = index_with(T, case.vocab)
    assert_rows(device_rows(idx, case.texts), case.texts, ids_of(case.vocab))


def test_lowered_token_matches_a_key_of_another_byte_length(T):
    case = TC.lowering_cases()[0]
    idx = index_with(T, case.vocab)
    got = device_rows(idx, case.texts)
    assert (got["term"] >= 0).all() and got["term"].tolist() == list(range(len(case.vocab)))


# ------------------------------------------------------------------ malformed bytes, through the raw ABI
def raw_rows(T, idx, blobs):
    N = T._native
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    blob = np.frombuffer(b"".join(blobs) + bytes(16), dtype=np.uint8)
    X = idx.text
    rows = N.text_tokens(dev(blob), dev(ptr), int(ptr[-1]), X["table_dev"], X["slots"], X["term_bytes"], X["term_ptr"])
    torch.cuda.synchronize()
    n = int(rows["n_total"].item())
    return rows["doc"][:n].cpu().numpy(), rows["term"][:n].cpu().numpy(), rows["n_tokens"].cpu().numpy(), \
        rows["flags"].cpu().numpy()


@pytest.mark.parametrize("bad,last,where", [(b"ab \xe2\x82", True, "truncated lead at the very end of the blob"),
                                             (b"ab \xc3", True, "truncated two-byte lead at the very end of the blob"),
                                             (b"ab \xe2\x82", False, "truncated lead at the end of a text"),
                                             (b"ab \x80 cd", False, "stray continuation byte"),
                                             (b"\xa9ab", False, "a text that begins with a continuation byte"),
                                             (b"ab \xc0\xaf cd", False, "overlong pair"),
                                             (b"ab \xe0\x80\xaf cd", False, "overlong triple"),
                                             (b"ab \xf5\x80\x80\x80", False, "a lead byte UTF-8 never holds"),
                                             (b"x\xe2\x82\xac\xac y", False, "one continuation byte too many")])
def test_malformed_utf8_flags_its_text_and_spares_the_neighbours(T, bad, last, where):
    vocab = ["ab", "cd", "ef"]
    idx = index_with(T, vocab)
    blobs = [b"ab cd", bad] if last else [b"ab cd", bad, b"ef ab"]
    doc, term, n_tokens, flags = raw_rows(T, idx, blobs)
    assert flags.tolist() == [0, 1] + [0] * (len(blobs) - 2), where
    assert np.array_equal(doc, np.repeat(np.arange(len(blobs)), n_tokens))
    assert term[doc == 0].tolist() == [0, 1] and n_tokens[0] == 2
    if len(blobs) == 3:
        assert term[doc == 2].tolist() == [2, 0] and n_tokens[2] == 2


def test_a_character_cut_by_a_text_boundary_flags_both_texts(T):
    idx = index_with(T, ["ab"])
    doc, term, n_tokens, flags = raw_rows(T, idx, [b"ab", b"ab \xe2\x82", b"\xac ab", b"ab"])
    assert flags.tolist() == [0, 1, 1, 0] and n_tokens[0] == n_tokens[3] == 1


def test_surface_answers_exceptional_texts_with_the_host(T):
    case = TC.exceptional_cases()[0]
    ids = ids_of(case.vocab)
    idx = index_with(T, case.vocab)
    terms, flags = idx.query_terms(case.texts)
    e_terms, _, e_flags = TC.expect_query_table(case.texts, ids)
    assert np.array_equal(terms.cpu().numpy(), e_terms) and np.array_equal(flags.cpu().numpy(), e_flags)
    R = idx.text_rows(case.texts)
    doc, term, _, _ = TC.expect_rows(case.texts, ids)
    assert np.array_equal(R.doc.cpu().numpy(), doc) and np.array_equal(R.term.cpu().numpy(), term)
    want = [tok for t in case.texts for tok in TC.backend.tokenize(t) if tok not in ids]
    assert [R.unknown[i] for i in R.unknown_which.tolist()] == want
    assert R.unknown == list(dict.fromkeys(want))


# ------------------------------------------------------------------ the vocabulary table
def lookups(T, idx, tokens):
    got = device_rows(idx, [" ".join(tokens)])
    assert got["n_tokens"].tolist() == [len(tokens)]
    return got["term"].tolist()


def test_300_keys_of_one_home_slot_and_a_chain_that_wraps(T):
    keys, slot = TC.colliding_keys(300, 1024, slot=1000)      # 300 from slot 1000 on: the chain wraps
    others = [f"other{i}" for i in range(200)]
    vocab = keys + others
    idx = index_with(T, vocab)
    assert idx.text["slots"].shape[0] == 1024
    h = TC.hash_keys([k.encode() for k in keys])
    assert (TC.home_slot(h, 1024) == slot).all() and slot + 300 > 1024
    probe = keys + others + ["k", "missing", keys[0] + "x"]
    assert lookups(T, idx, probe) == list(range(500)) + [-1, -1, -1]
    # the documented layout: a table built in numpy by the header's words holds the same keys in the same chain
    u = idx.text["slots"].cpu().numpy()
    mine = TC.build_table([k.encode() for k in vocab], 1024)
    assert sorted(map(tuple, u.tolist())) == sorted(map(tuple, mine.tolist()))
    assert (u[:, 0] != 0).sum() == 500
    for k in (keys[0], keys[299], others[7]):
        assert TC.table_lookup(u, [v.encode() for v in vocab], k.encode()) == vocab.index(k)


def test_keys_that_are_prefixes_of_one_another(T):
    vocab = ["casa", "casas", "cas", "c", "casamento"]
    idx = index_with(T, vocab)
    assert lookups(T, idx, ["casas", "c", "casa", "casam", "cas", "casamento", "ca"]) == [1, 3, 0, -1, 2, 4, -1]


def hand_built(T, keys, slots):
    """An index whose device table is ``slots`` (int64 [capacity, 2]) over the key store of ``keys``."""
    idx = index_with(T, keys)
    idx.text["slots"] = dev(slots)
    return idx


def test_hand_built_table_foreign_id_under_the_tokens_hash_is_passed_over(T):
    keys = ["alpha", "betas", "gamma"]      # (of one length: only the bytes tell them apart)
    cap = 16
    slots = TC.build_table([k.encode() for k in keys], cap).view(np.uint64)
    h = TC.hash_keys([b"alpha"])[0]
    s = int(TC.home_slot(np.array([h]), cap)[0])
    assert slots[s, 0] == h and slots[s, 1] == 0
    # in front of alpha's slot in its chain: alpha's hash with beta's id; alpha itself moves one slot on
    moved = slots.copy()
    chain = s
    while moved[chain, 0] != 0:
        chain = (chain + 1) % cap
    moved[chain] = moved[s]
    moved[s, 1] = 1
    # (whatever lay between s and the free slot keeps its place: the chain stays unbroken)
    idx = hand_built(T, keys, moved.view(np.int64))
    assert lookups(T, idx, ["alpha", "betas", "gamma"]) == [0, 1, 2]
    # and with no true slot behind it the token is unknown, not betas
    moved[chain] = 0
    idx = hand_built(T, keys, moved.view(np.int64))
    assert lookups(T, idx, ["alpha", "gamma"]) == [-1, 2]


def test_hash_zero_is_remapped(T):
    # no key of a reasonable search hashes to 0: the remap through a hand-built table.  A key that hashes to 0
    # is stored under hash word 1; such a slot is occupied -- a chain runs through it -- and 0 alone is empty
    assert TC.hash_keys([b""])[0] == TC.FNV_BASIS
    keys = ["alpha", "beta"]
    cap = 16
    slots = np.zeros((cap, 2), dtype=np.uint64)
    hs = TC.hash_keys([b"alpha"])
    s = int(TC.home_slot(hs, cap)[0])
    slots[s] = (1, 1)                         # in alpha's home slot: hash word 1 (with beta's id)
    slots[(s + 1) % cap] = (hs[0], 0)         # alpha behind it
    idx = hand_built(T, keys, slots.view(np.int64))
    assert lookups(T, idx, ["alpha", "beta"]) == [0, -1]


def test_half_load_before_and_after_a_rebuild(T):
    vocab = [f"t{i}" for i in range(512)]
    idx = index_with(T, vocab)
    assert idx.text["slots"].shape[0] == 1024                 # exactly 1/2
    before = lookups(T, idx, vocab + ["new0"])
    assert before == list(range(512)) + [-1]
    idx.grow_vocabulary(["new0"])
    assert idx.text["slots"].shape[0] == 2048                 # rebuilt
    assert lookups(T, idx, vocab + ["new0"]) == list(range(513))
    idx.grow_vocabulary([f"g{i}" for i in range(511)])        # in place, to exactly 1/2 again
    assert idx.text["slots"].shape[0] == 2048 and len(idx.text["ids"]) == 1024
    assert lookups(T, idx, vocab + ["new0", "g0", "g510", "g511"]) == list(range(513)) + [513, 1023, -1]
    with pytest.raises(ValueError):
        idx.grow_vocabulary(["t3"])
    with pytest.raises(ValueError):
        idx.grow_vocabulary(["u", "u"])
    with pytest.raises(ValueError):
        T.GpuIndex().set_vocabulary(["a", "b", "a"])


# ------------------------------------------------------------------ the query table
def test_query_table_edges_in_both_forms(T):
    case = TC.query_cases()[0]
    assert case.holds()
    ids = ids_of(case.vocab)
    idx = index_with(T, case.vocab)
    rows = idx._text_tokens(case.texts)
    terms, nd, flags = T._native.query_terms(rows)
    e_terms, e_nd, e_flags = TC.expect_query_table(case.texts, ids)
    assert np.array_equal(terms.cpu().numpy(), e_terms)
    assert np.array_equal(nd.cpu().numpy(), e_nd) and np.array_equal(flags.cpu().numpy(), e_flags)
    assert e_nd.tolist()[:4] == [3, 32, 33, 33] and e_flags.tolist()[1:3] == [0, 4]
    # the surface against _query_terms itself, query by query
    from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient
    for conj in (False, True):
        client = GpuIndexClient.__new__(GpuIndexClient)
        client.store = CorpusStore([], [], [], [], [], [], vocab=ids)
        client.index, client.lexical_and = type("Lexical", (), {"lex": {}})(), conj
        got = idx.query_terms(case.texts, conjunctive=conj)[0].cpu().numpy()
        for q, text in enumerate(case.texts):
            want = client._query_terms(text) or []
            assert got[q].tolist() == want + [-1] * (MT - len(want)), (conj, text[:40])


def test_65600_queries_in_one_call(T):
    rng = np.random.default_rng(5)
    vocab = [f"w{i}" for i in range(1000)]
    ids = ids_of(vocab)
    words = np.array(vocab + ["zz", "Yy"])
    texts = [" ".join(words[rng.integers(0, len(words), rng.integers(0, 9))]) for _ in range(65_600)]
    idx = index_with(T, vocab)
    terms, flags = idx.query_terms(texts)
    e_terms, _, e_flags = TC.expect_query_table(texts, ids)
    assert np.array_equal(terms.cpu().numpy(), e_terms) and np.array_equal(flags.cpu().numpy(), e_flags)


def test_bm25_search_of_the_device_table_equals_the_host_made_one(T):
    from triple_hybrid_rag_amd import index_build as IB
    rng = np.random.default_rng(9)
    words = [f"w{i}" for i in range(300)]
    rows = _rows([" ".join(rng.choice(words, 12)) for _ in range(1000)], 1024, 8)
    hi = IB.from_rows(rows, [{"id": "p0", "text": "parent", "section_heading": "S"}])
    idx = hi.to_gpu()
    vocab = sorted(hi.store.vocab, key=hi.store.vocab.get)
    idx.set_vocabulary(vocab)
    texts = [" ".join(rng.choice(words + ["Nope"], rng.integers(1, 7))).upper() for _ in range(64)] + ["", "nope"]
    host, _, _ = TC.expect_query_table(texts, hi.store.vocab)
    for conj in (False, True):
        qt = idx.query_terms(texts, conjunctive=conj)[0]
        want = host.copy()
        if conj:
            want[(TC.expect_query_table(texts, hi.store.vocab)[2] & 6) != 0] = -1
        assert np.array_equal(qt.cpu().numpy(), want)
        S1, I1, c1 = idx.bm25_search(qt, 10, conjunctive=conj)
        S2, I2, c2 = idx.bm25_search(dev(want), 10, conjunctive=conj)
        assert torch.equal(S1.view(torch.int64), S2.view(torch.int64)) and torch.equal(I1, I2) and torch.equal(c1, c2)
        # an all -1 row ranks nothing, in both forms: what lets the AND form void a query in the table
        void = np.flatnonzero((want < 0).all(axis=1))
        assert len(void) >= 2 and (c1.cpu().numpy()[void] == 0).all()


# ------------------------------------------------------------------ ingest through the client
def _twin(T, rows, parents, table=None, **kw):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    tok = {} if table is None else {"tokenizer": table.tokenize}
    hi = IB.from_rows(rows, parents, **tok)
    return GpuIndexClient(hi.to_gpu(), hi.store, org_id="org", **tok, **kw)


def _rows(texts, d, seed, first=0):
    rng = np.random.default_rng(seed)
    return [{"id": f"c{first + i}", "parent_id": "p0", "document_id": "d0", "text": t, "page": 1, "modality": "text",
             "embedding_1024": rng.standard_normal(d).astype(np.float32).tolist(), "org_id": "org"}
            for i, t in enumerate(texts)]


def _same_index(a, b):
    from test_gpu_append import _assert_lex_equal, same
    same(a.docs, b.docs, "docs")
    _assert_lex_equal(a, b)


def test_insert_children_device_text_equals_the_host_route(T):
    d = 1024
    rng = np.random.default_rng(3)
    words = [f"w{i}" for i in range(200)]
    base = _rows([" ".join(rng.choice(words, 10)) for _ in range(300)], d, 1)
    parents = [{"id": "p0", "text": "parent", "section_heading": "S"}]
    batch = ["novo termo w1 novo", "", "w2 İstanbul primeiro termo", "outro novo W3 primeiro",
             "  ,, ", "İstanbul de novo ΣΟΣ"] + [" ".join(rng.choice(words + ["raro", "Novo"], 8)) for _ in range(40)]
    second = ["novo termo primeiro raro w5 ainda", "i̇stanbul σος w1"]
    host, devc = _twin(T, base, parents), _twin(T, base, parents, device_text=True)
    for texts, first in ((batch, 1000), (second, 2000)):
        rows = _rows(texts, d, first, first)
        assert host.insert_children(rows) == devc.insert_children(rows)
        _same_index(host.index, devc.index)
        assert list(host.store.vocab.items()) == list(devc.store.vocab.items())
        assert devc.index.text["ids"] == devc.store.vocab
    for q in ("novo termo", "İstanbul primeiro", "raro w5", "nenhum"):
        for conj in (False, True):
            host.lexical_and = devc.lexical_and = conj
            a = host.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": q, "p_limit": 10}).data
            b = devc.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": q, "p_limit": 10}).data
            assert list(a) == list(b), (q, conj)
    assert list(devc.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": "novo termo", "p_limit": 5}).data)
    # ... and through the retriever
    import asyncio
    from triple_hybrid_rag_amd.config import SETTINGS
    from triple_hybrid_rag_amd.rag2.embedder import PrecomputedEmbedder
    from triple_hybrid_rag_amd.rag2.query_planner import QueryPlanner
    from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever
    host.lexical_and = devc.lexical_and = False
    saved = dict(SETTINGS.__dict__)
    SETTINGS.rag2_safety_threshold = 0.0
    SETTINGS.rag2_denoise_alpha = 0.0
    try:
        found = []
        for c in (host, devc):
            e = PrecomputedEmbedder(store_dim=d)
            e.register("novo termo primeiro", _rows(["x"], d, 2000, 2000)[0]["embedding_1024"])
            r = RAG2Retriever(org_id="org", embedder=e, query_planner=QueryPlanner())
            r._supabase = c
            res = asyncio.run(r.retrieve("novo termo primeiro", top_k=5, skip_rerank=True))
            assert res.success
            found.append([(x.child_id, x.parent_text) for x in res.contexts])
        assert found[0] == found[1] and found[0] and found[0][0][0] == "c2000"
    finally:
        SETTINGS.__dict__.update(saved)


def test_accent_folding_table_end_to_end(T):
    from triple_hybrid_rag_amd.index_text import TextTable, fold_accents
    table = TextTable.from_char_map(fold_accents)
    d = 1024
    base = _rows(["uma frase qualquer", "outra frase"], d, 4)
    parents = [{"id": "p0", "text": "parent", "section_heading": "S"}]
    host, devc = _twin(T, base, parents, table), _twin(T, base, parents, table, device_text=True)
    rows = _rows(["a ACAO do dia", "coração e RAZÃO", "nada aqui"], d, 5, 100)
    host.insert_children(rows)
    devc.insert_children(rows)
    _same_index(host.index, devc.index)
    assert list(host.store.vocab.items()) == list(devc.store.vocab.items()) and "acao" in devc.store.vocab
    qt = devc.query_terms_batch(["ação", "CORACAO razao", "frase"]).cpu().numpy()
    want, _, _ = TC.expect_query_table(["ação", "CORACAO razao", "frase"], devc.store.vocab, table)
    assert np.array_equal(qt, want) and qt[0, 0] == devc.store.vocab["acao"]
    got = devc.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": "ação", "p_limit": 5}).data
    assert [r["child_id"] for r in got] == ["c100"]
