"""Typo-tolerant lexical queries on the GPU (include/thr_hip_fuzzy.h): thr_vocab_nearest and
thr_query_terms_fuzzy, and the Python surface over them, held array for array to the plain restatement
(index_text.nearest_terms_host / host_query_row_fuzzy) on every built case of tests/fuzzy_cases.py.  Integers
throughout: no tolerance anywhere.

In bounds: a needle is read through a walk that ends at its clamped end, a key only from the staged slice inside
[term_ptr[t], term_ptr[t + 1]) -- the raw-ABI test shows it by guard bytes the outputs do not depend on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fuzzy_cases as FC  # noqa: E402
import text_cases as TC  # noqa: E402

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MT = 32
CASES = FC.all_cases()
QUERY_CASES = FC.query_cases()


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def u8(b: bytes):
    return dev(np.frombuffer(b, dtype=np.uint8).copy())


def table_of(rows, n_best):
    """[(distance, id)] per needle -> (ids, dist) int32 [n, n_best] padded with -1."""
    ids = np.full((len(rows), n_best), -1, dtype=np.int32)
    dist = np.full((len(rows), n_best), -1, dtype=np.int32)
    for u, row in enumerate(rows):
        for j, (d, i) in enumerate(row):
            ids[u, j], dist[u, j] = i, d
    return ids, dist


def nearest_of_rows(T, idx, rows, case, rowptr):
    """thr_vocab_nearest over the unknown list of a text_tokens call -> (n_unknown, the needles as the host reads
    them at the list's places, near_term, near_dist) with the arrays prefilled with 7: rows behind n_unknown stay."""
    N, X = T._native, idx.text
    cap = rows["unknown_off"].shape[0]
    near = torch.full((cap, case.n_best), 7, dtype=torch.int32, device="cuda")
    dist = torch.full((cap, case.n_best), 7, dtype=torch.int32, device="cuda")
    N.vocab_nearest(rows["bytes_dev"], int(rows["ptr"][-1]), X["table_dev"], rows["unknown_off"], rows["unknown_len"],
                    rows["n_unknown"], X["term_bytes"], X["term_ptr"], X["n_bytes"],
                    term_rowptr=None if rowptr is None else dev(rowptr), max_edits=case.max_edits, n_best=case.n_best,
                    near_term=near, near_dist=dist)
    torch.cuda.synchronize()
    nu = int(rows["n_unknown"].item())
    off, ln = rows["unknown_off"][:nu].cpu().tolist(), rows["unknown_len"][:nu].cpu().tolist()
    raw = rows["blob"].tobytes()
    needles = [X["table"].restate(raw[o:o + l].decode("utf-8", "surrogatepass"))[0] for o, l in zip(off, ln)]
    return nu, needles, near.cpu().numpy(), dist.cpu().numpy()


def expect(case, needles, with_df):
    from triple_hybrid_rag_amd.index_text import nearest_terms_host
    memo = case._memo.setdefault((with_df, None), {})
    df = case.df if with_df else None
    for w in needles:
        if w not in memo:
            memo[w] = nearest_terms_host(w, case.vocab, df, case.max_edits, case.n_best)
    return table_of([memo[w] for w in needles], case.n_best)


# ------------------------------------------------------------------ thr_vocab_nearest on the built cases
@pytest.mark.parametrize("analyzed", [False, True], ids=["text_tokens", "text_tokens_analyzed"])
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_vocab_nearest_equals_the_definition(T, case, analyzed):
    from triple_hybrid_rag_amd.index_text import Analyzer
    assert case.holds()
    if analyzed:       # the needle is the STEM: every text carries a suffix the analyzer strips, and a stop word
        idx = T.GpuIndex().set_vocabulary(case.vocab, Analyzer(stop=["zzstop"], steps=[[("qzq", 1)]]))
        texts = [x + "QZQ zzstop" for x in case.needles]
    else:
        idx = T.GpuIndex().set_vocabulary(case.vocab)
        texts = list(case.needles)
    rows = idx._text_tokens(texts)
    known = set(case.vocab)
    want_needles = [FC.lowered(x) for x in case.needles if FC.lowered(x) not in known]
    for with_df in (False, True):
        if with_df and case.df is None:
            continue
        nu, needles, near, dist = nearest_of_rows(T, idx, rows, case, case.rowptr() if with_df else None)
        assert needles == want_needles and nu == len(want_needles)
        ids, d = expect(case, needles, with_df)
        assert np.array_equal(near[:nu], ids), (case.name, with_df)
        assert np.array_equal(dist[:nu], d), (case.name, with_df)
        assert (near[nu:] == 7).all() and (dist[nu:] == 7).all(), "rows at or behind n_unknown are not written"


def test_nearest_terms_is_the_stage_alone(T):
    """Already-lowered strings, keys among them (distance 0 wins), with and without frequencies; an exceptional
    token, a four-byte character, an empty and a too long token get a row of -1."""
    from triple_hybrid_rag_amd.index_text import Fuzzy
    for case in CASES:
        if case.name in ("70000_keys_answers_last", "6000_needles"):
            continue
        idx = T.GpuIndex().set_vocabulary(case.vocab)
        needles = [FC.lowered(x) for x in case.needles] + case.vocab[:3]
        fz = Fuzzy(case.max_edits, case.n_best)
        got = idx.nearest_terms(needles, fz, df=False)
        ids, d = expect(case, needles, False)
        assert np.array_equal(got[0].cpu().numpy(), ids) and np.array_equal(got[1].cpu().numpy(), d), case.name
        if case.df is not None:
            idx.lex = dict(rowptr=dev(case.rowptr()))          # (only the row pointer is read)
            got = idx.nearest_terms(needles, fz)
            ids, d = expect(case, needles, True)
            assert np.array_equal(got[0].cpu().numpy(), ids) and np.array_equal(got[1].cpu().numpy(), d), case.name
    idx = T.GpuIndex().set_vocabulary(["istanbul", "contrato", "abc\U0001F600def"])
    got = idx.nearest_terms(["İstanbul", "contrat\U0001F600", "", "c" * 33, "contrato", "istanbvl", "abcXdef"], Fuzzy(2, 1))
    assert got[0].cpu().numpy()[:, 0].tolist() == [-1, -1, -1, -1, 1, 0, -1]
    assert got[1].cpu().numpy()[:, 0].tolist() == [-1, -1, -1, -1, 0, 1, -1]
    assert idx.nearest_terms([])[0].shape == (0, 2)


def test_no_unknown_token_leaves_the_outputs_untouched(T):
    case = FC.order_cases()[0]
    idx = T.GpuIndex().set_vocabulary(case.vocab)
    rows = idx._text_tokens(["casa cama", "", "CARA"])
    nu, needles, near, dist = nearest_of_rows(T, idx, rows, case, case.rowptr())
    assert nu == 0 and (near == 7).all() and (dist == 7).all()


# ------------------------------------------------------------------ inputs only the raw entry can send
def test_raw_inputs_are_answered_as_defined_and_stay_in_bounds(T):
    """Offsets outside the text, a needle with a stray continuation byte, a needle cut inside a character, an invalid
    key, a key with a four-byte character, a key whose pointer runs past the store: each answered as the header
    defines.  The text and the key store are views INTO guard-filled buffers: the same outputs with two fills."""
    N = T._native
    from triple_hybrid_rag_amd.index_text import TextTable
    text = "contrata caxa".encode() + b"contr\x80ta" + "locaçao".encode()
    keys = [b"contrato", b"contr\xffto", b"casa", "contra\U0001F600o".encode(), b"cama", b"cont\xe7", "locação".encode()]
    kptr = np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int64)
    kptr_bad = kptr.copy()
    kptr_bad[-1] += 40                                            # the last key claims bytes behind the store
    n_text, n_keys = len(text), int(kptr[-1])
    loc = n_text - len("locaçao".encode())
    unknown = [(0, 8), (9, 4), (13, 8), (-5, 8), (9, 400), (n_text + 50, 3), (5, -2), (loc, 5), (loc, 8)]
    #           contrata caxa   stray    clamped to "contrata", to "caxa" + the stray bytes + ..., to nothing, to nothing;
    #           "loca" + half a ç; locaçao
    want = [[0], [2, 4], [], [0], [], [], [], [], [6]]
    table = dev(TextTable.default().entries.view(np.int32))
    outs = []
    for fill in (0x00, 0xE7):
        tbuf = torch.full((256 + n_text + 256,), fill, dtype=torch.uint8, device="cuda")
        tbuf[256:256 + n_text] = u8(text)
        kbuf = torch.full((1024 + n_keys + 1024,), fill, dtype=torch.uint8, device="cuda")
        kbuf[1027:1027 + n_keys] = u8(b"".join(keys))      # (not 16-byte aligned)
        for ptr in (kptr, kptr_bad):
            near, dist = N.vocab_nearest(tbuf[256:256 + n_text], n_text, table, dev(np.array([u[0] for u in unknown], dtype=np.int64)),
                                         dev(np.array([u[1] for u in unknown], dtype=np.int32)), dev(np.array([len(unknown)], dtype=np.int32)),
                                         kbuf[1027:1027 + n_keys], dev(ptr), n_keys, max_edits=2, n_best=2)
            torch.cuda.synchronize()
            outs.append((near.cpu().numpy(), dist.cpu().numpy()))
    for near, dist in outs:
        assert [[i for i in row if i >= 0] for row in near.tolist()] == want
        assert np.array_equal(near, outs[0][0]) and np.array_equal(dist, outs[0][1])
    assert outs[0][1].tolist()[:2] == [[1, -1], [1, 1]] and outs[0][1].tolist()[8] == [1, -1]
    # *n_unknown beyond the capacity, and negative: clamped
    for claimed, rows in ((1000, 2), (-3, 0)):
        near = torch.full((2, 2), 7, dtype=torch.int32, device="cuda")
        N.vocab_nearest(u8(text), n_text, table, dev(np.array([0, 9], dtype=np.int64)),
                        dev(np.array([8, 4], dtype=np.int32)), dev(np.array([claimed], dtype=np.int32)),
                        u8(b"".join(keys)), dev(kptr), n_keys, near_term=near)
        assert near.cpu().numpy().tolist() == ([[0, -1], [2, 4]] if rows else [[7, 7], [7, 7]])


# ------------------------------------------------------------------ thr_query_terms_fuzzy
def lexical_index(T, vocab, df):
    """A GpuIndex whose lexical index gives term i the document frequency df[i] (document d holds the terms with
    df > d), with the vocabulary set."""
    n_docs = max(max(df), 1)
    doc = np.concatenate([np.arange(f, dtype=np.int32) for f in df])
    term = np.concatenate([np.full(f, i, dtype=np.int32) for i, f in enumerate(df)])
    idx = T.GpuIndex()
    idx.set_lexical_rows(doc, term, None, len(vocab), n_docs=n_docs)
    assert np.array_equal(np.diff(idx.lex["rowptr"].cpu().numpy()), np.asarray(df))
    return idx.set_vocabulary(vocab)


def host_table(rows, conjunctive):
    N_U, N_M = 2, 4
    terms = np.full((len(rows), MT), -1, dtype=np.int32)
    flags = np.zeros(len(rows), dtype=np.int32)
    for q, (row, _, f) in enumerate(rows):
        flags[q] = f
        if not (conjunctive and f & (N_U | N_M)):
            terms[q, :len(row)] = row
    return terms, flags


@pytest.mark.parametrize("qc", QUERY_CASES, ids=[c.name for c in QUERY_CASES])
def test_query_terms_with_corrections_equals_the_host_rows(T, qc):
    from triple_hybrid_rag_amd.index_text import Fuzzy, host_query_row_fuzzy, tokenize
    N = T._native
    idx = lexical_index(T, qc.vocab, qc.df)
    fz = Fuzzy(qc.max_edits, qc.n_best)
    for conj in (False, True):
        terms, flags = idx.query_terms(qc.texts, conjunctive=conj, fuzzy=fz)
        want_t, want_f = host_table(qc.rows(conj), conj)
        assert np.array_equal(flags.cpu().numpy(), want_f), (qc.name, conj)
        assert np.array_equal(terms.cpu().numpy(), want_t), (qc.name, conj)
    # the entry itself: n_use 1 .. n_best over one list of corrections, n_distinct, and the clamp
    rows = idx._text_tokens(qc.texts)
    near, _ = idx._nearest(rows["bytes_dev"], int(rows["ptr"][-1]), rows["unknown_off"], rows["unknown_len"],
                           rows["n_unknown"], fz, True)
    ids = {t: i for i, t in enumerate(qc.vocab)}
    for n_use in range(1, qc.n_best + 1):
        terms, nd, flags = N.query_terms_fuzzy(rows, near, n_use)
        want = [host_query_row_fuzzy(tokenize(t), ids, qc.vocab, qc.df, qc.max_edits, n_use, False) for t in qc.texts]
        want_t, want_f = host_table(want, False)
        assert np.array_equal(terms.cpu().numpy(), want_t) and np.array_equal(flags.cpu().numpy(), want_f), (qc.name, n_use)
        assert nd.cpu().numpy().tolist() == [w[1] for w in want]


def test_without_a_correction_the_entry_is_thr_query_terms_bit_for_bit(T):
    N = T._native
    cases = TC.slice_cases() + TC.boundary_cases() + TC.lowering_cases() + TC.exceptional_cases()
    for case in cases:
        idx = T.GpuIndex().set_vocabulary(case.vocab)
        rows = idx._text_tokens(case.texts)
        a = N.query_terms(rows)
        for n_best, n_use in ((1, 1), (4, 1), (4, 4)):
            none = torch.full((rows["capacity"], n_best), -1, dtype=torch.int32, device="cuda")
            b = N.query_terms_fuzzy(rows, none, n_use)
            for x, y, what in zip(a, b, ("terms", "n_distinct", "flags")):
                assert torch.equal(x, y), (case.name, what, n_best, n_use)
        # ... and fuzzy=None is today's call: the same tensors
        for conj in (False, True):
            p, q = idx.query_terms(case.texts, conjunctive=conj), idx.query_terms(case.texts, conjunctive=conj, fuzzy=None)
            assert torch.equal(p[0], q[0]) and torch.equal(p[1], q[1])


def test_sixty_five_thousand_six_hundred_one_token_queries(T):
    from triple_hybrid_rag_amd.index_text import Fuzzy
    qc = QUERY_CASES[0]
    idx = lexical_index(T, qc.vocab, qc.df)
    pool = ["contrato", "contratx", "CAXA", "qqqqqq", "locacao", "de", "", "casa", "documentx", "ca"]
    one = FC.QueryCase("pool", qc.vocab, qc.df, pool)
    texts = [pool[(7 * i) % len(pool)] for i in range(65600)]
    pick = np.array([(7 * i) % len(pool) for i in range(65600)])
    for conj in (False, True):
        want_t, want_f = host_table(one.rows(conj), conj)
        terms, flags = idx.query_terms(texts, conjunctive=conj, fuzzy=Fuzzy())
        assert np.array_equal(terms.cpu().numpy(), want_t[pick]) and np.array_equal(flags.cpu().numpy(), want_f[pick])


# ------------------------------------------------------------------ a live index: growth, commits, appends, deletes
def _twin(T, texts):
    """A fresh index over ``texts``: vocabulary in order of first appearance, lexical index, device vocabulary."""
    from triple_hybrid_rag_amd.index_text import tokenize
    vocab, doc, term = {}, [], []
    for d, t in enumerate(texts):
        for tok in tokenize(t):
            doc.append(d)
            term.append(vocab.setdefault(tok, len(vocab)))
    doc, term = np.asarray(doc, dtype=np.int32), np.asarray(term, dtype=np.int32)
    idx = T.GpuIndex()
    idx.set_lexical_rows(doc, term, None, len(vocab), n_docs=len(texts))
    return idx.set_vocabulary(sorted(vocab, key=vocab.get)), vocab


def _same_corrections(a, b, probes, conj_too=True):
    from triple_hybrid_rag_amd.index_text import Fuzzy, tokenize, host_query_row_fuzzy
    fz = Fuzzy(2, 3)
    na, nb = a.nearest_terms(probes, fz), b.nearest_terms(probes, fz)
    assert torch.equal(na[0], nb[0]) and torch.equal(na[1], nb[1])
    for conj in (False, True):
        qa, qb = a.query_terms(probes, conjunctive=conj, fuzzy=fz), b.query_terms(probes, conjunctive=conj, fuzzy=fz)
        assert torch.equal(qa[0], qb[0]) and torch.equal(qa[1], qb[1])
    # ... and the twin is the definition's
    vocab = sorted(b.text["ids"], key=b.text["ids"].get)
    df = np.diff(b.lex["rowptr"].cpu().numpy()).tolist()
    df += [0] * (len(vocab) - len(df))
    want = [host_query_row_fuzzy(tokenize(t), b.text["ids"], vocab, df, 2, 3, False) for t in probes]
    want_t, want_f = host_table(want, False)
    got = b.query_terms(probes, fuzzy=fz)
    assert np.array_equal(got[0].cpu().numpy(), want_t) and np.array_equal(got[1].cpu().numpy(), want_f)
    return na[0].cpu().numpy()


def test_corrections_follow_the_vocabulary_and_the_frequencies_of_a_live_index(T):
    base = ["contrato de locação", "contrato assinado", "casa alugada", "cama e mesa", "cara casa"]
    more = ["contrata novo fiador", "fiador assinado cama", "garantia do contrata"]
    probes = ["contratx", "fiadxr", "garantla", "caxa", "locacao", "mesx assinadx"]
    # grow_vocabulary: the new keys are candidates at once where no frequencies are asked; with them they have no postings yet
    idx, vocab = _twin(T, base)
    idx.grow_vocabulary(["fiador", "garantia"])
    from triple_hybrid_rag_amd.index_text import Fuzzy
    got = idx.nearest_terms(["fiadxr", "garantla"], Fuzzy(2, 1), df=False)[0].cpu().numpy()[:, 0].tolist()
    assert got == [len(vocab), len(vocab) + 1]
    assert idx.nearest_terms(["fiadxr", "garantla"], Fuzzy(2, 1))[0].cpu().numpy()[:, 0].tolist() == [-1, -1]
    fresh = T.GpuIndex().set_vocabulary(sorted(vocab, key=vocab.get) + ["fiador", "garantia"])
    a, b = idx.nearest_terms(probes, df=False), fresh.nearest_terms(probes, df=False)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # number_text_rows + append_rows + commit_vocabulary, both mirror settings, against a twin built fresh
    for mirror in (True, False):
        idx, _ = _twin(T, base)
        R = idx.number_text_rows(more)
        idx.append_rows(None, lex=(R.doc, R.term, None, R.n_before + R.pending.n_new), n_rows=len(more))
        idx.commit_vocabulary(R.pending, mirror=mirror)
        fresh, fv = _twin(T, base + more)
        near = _same_corrections(idx, fresh, probes)
        assert near[0, 0] == fv["contrato"] and near[0, 1] == fv["contrata"] and near[1, 0] == fv["fiador"]
    # delete_rows: frequencies change the order, and a term whose last posting goes stops being a correction
    gone = [5, 7]                                   # both chunks that hold "contrata"; "fiador" keeps one
    idx.delete_rows(np.asarray(gone))
    fresh2, fv2 = _twin(T, [t for d, t in enumerate(base + more) if d not in gone])
    before = fv["contrata"]
    near = idx.nearest_terms(probes, Fuzzy(2, 3))[0].cpu().numpy()
    assert before not in near[0].tolist() and near[0, 0] == fv["contrato"]
    # (the twin numbers its vocabulary afresh: compare through the strings)
    names = sorted(fv, key=fv.get)
    names2 = sorted(fv2, key=fv2.get)
    near2 = fresh2.nearest_terms(probes, Fuzzy(2, 3))[0].cpu().numpy()
    for row, row2 in zip(near.tolist(), near2.tolist()):
        assert [names[i] for i in row if i >= 0] == [names2[i] for i in row2 if i >= 0]


# ------------------------------------------------------------------ through bm25_search and the client
def test_bm25_with_a_misspelt_word(T):
    from oracle import thr_oracle as O
    from triple_hybrid_rag_amd.index_text import Fuzzy
    rng = np.random.default_rng(3)
    words = ["contrato", "locação", "fiador", "garantia", "aluguel", "casa", "cama", "cara", "prazo", "multa"]
    texts = [" ".join(rng.choice(words, rng.integers(2, 7))) for _ in range(400)]
    idx, vocab = _twin(T, texts)
    L = idx.lex
    csr = [L[k].cpu().numpy() for k in ("rowptr", "post_doc", "post_tf", "doclen")]
    idf = L["idf"].cpu().numpy()

    def oracle(row, k=20):
        qt = np.full((1, 4), -1, dtype=np.int32)
        qt[0, :len(row)] = row
        S, I = O.bm25_topk(*csr, idf, L["avgdl"], qt, len(texts), k)
        return S[0], I[0]

    def search(text, conj, fuzzy):
        qt = idx.query_terms([text], conjunctive=conj, fuzzy=fuzzy)[0]
        S, I, cnt = idx.bm25_search(qt, 20, conjunctive=conj)
        c = int(cnt[0])
        return S[0, :c].cpu().numpy(), I[0, :c].cpu().numpy()
    # AND: one misspelt word empties the query; with the correction it is the query of the corrected row
    S, I = search("contrtao fiador", True, None)
    assert len(I) == 0
    S, I = search("contrtao fiador", True, Fuzzy())
    both = sorted(d for d, t in enumerate(texts) if "contrato" in t.split() and "fiador" in t.split())
    Se, Ie = oracle([vocab["contrato"], vocab["fiador"]], k=len(texts))      # the whole OR list: the AND list is its rows with both
    keep = np.isin(Ie, both)
    assert len(both) > 3 and len(I) == min(20, len(both))
    assert np.array_equal(I, Ie[keep][:20]) and np.array_equal(S, Se[keep][:20])
    # OR with two corrections: "caxa" stands for its two most frequent neighbours
    df = np.diff(csr[0])
    near = sorted((w for w in ("casa", "cama", "cara")), key=lambda w: (-df[vocab[w]], vocab[w]))[:2]
    S, I = search("caxa multa", False, Fuzzy(2, 2))
    Se, Ie = oracle([vocab[near[0]], vocab[near[1]], vocab["multa"]])
    assert np.array_equal(I, Ie) and np.array_equal(S, Se)
    S0, I0 = search("caxa multa", False, None)
    Se, Ie = oracle([vocab["multa"]])
    assert np.array_equal(I0, Ie) and np.array_equal(S0, Se)


def test_the_client_routes_lexical_queries_through_the_corrections(T):
    import asyncio
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.config import SETTINGS
    from triple_hybrid_rag_amd.index_text import Fuzzy
    from triple_hybrid_rag_amd.rag2.embedder import PrecomputedEmbedder
    from triple_hybrid_rag_amd.rag2.query_planner import QueryPlanner
    from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever
    rng = np.random.default_rng(8)
    d = 1024
    texts = ["contrato de locação do imóvel", "fiador e garantia", "contrato do fiador", "prazo e multa", "casa alugada"]
    rows = [{"id": f"c{i}", "parent_id": "p0", "document_id": "d0", "text": t, "page": 1, "modality": "text",
             "embedding_1024": rng.standard_normal(d).astype(np.float32).tolist(), "org_id": "org"} for i, t in enumerate(texts)]
    hi = IB.from_rows(rows, [{"id": "p0", "text": "parent", "section_heading": "S"}])

    def client(**kw):
        return GpuIndexClient(hi.to_gpu(), hi.store, org_id="org", device_text=True, **kw)

    def lexical(c, q):
        return [r["child_id"] for r in c.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": q, "p_limit": 10}).data]
    for conj in (True, False):
        plain, fuzzy = client(lexical_and=conj), client(lexical_and=conj, fuzzy=Fuzzy())
        assert lexical(plain, "contrato fiador") == lexical(fuzzy, "contrato fiador") != []
        assert lexical(fuzzy, "contrtao fiadro") == lexical(plain, "contrato fiador")
        assert lexical(plain, "contrtao fiadro") == []
        want = plain.query_terms_batch(["contrato fiador"])
        assert torch.equal(fuzzy.query_terms_batch(["contrtao fiadro"]), want)
    saved = dict(SETTINGS.__dict__)
    SETTINGS.rag2_safety_threshold = 0.0
    SETTINGS.rag2_denoise_alpha = 0.0
    try:
        found = []
        for c, q in ((client(lexical_and=True), "contrato fiador"), (client(lexical_and=True, fuzzy=Fuzzy()), "contrtao fiadro")):
            e = PrecomputedEmbedder(store_dim=d)
            e.register(q, rows[2]["embedding_1024"])
            r = RAG2Retriever(org_id="org", embedder=e, query_planner=QueryPlanner())
            r._supabase = c
            res = asyncio.run(r.retrieve(q, top_k=3, skip_rerank=True))
            assert res.success
            found.append([x.child_id for x in res.contexts])
        assert found[0] == found[1] and found[0][0] == "c2"
    finally:
        SETTINGS.__dict__.update(saved)


# ------------------------------------------------------------------ the workspace contract
def test_same_bits_whatever_the_workspace_held(T):
    N = T._native
    case = [c for c in CASES if c.name == "counts_300_at_distance_1"][0]
    qc = QUERY_CASES[0]
    idx = T.GpuIndex().set_vocabulary(case.vocab)
    X = idx.text
    rows = idx._text_tokens(case.needles + ["abcdefg9", "zzzzzzzz"])
    rowptr = dev(case.rowptr())
    need = N.vocab_nearest_workspace_bytes(int(rows["ptr"][-1]), rows["capacity"], len(case.vocab), X["n_bytes"], 4)
    idq = lexical_index(T, qc.vocab, qc.df)
    qrows = idq._text_tokens(qc.texts)
    qnear = idq.nearest_terms(["x"], df=False)[0].new_full((qrows["capacity"], 2), -1)
    qnear[:3] = torch.tensor([[0, 1], [4, -1], [2, 3]], dtype=torch.int32)
    qneed = N.query_terms_fuzzy_workspace_bytes(len(qc.texts))
    outs, qouts = [], []
    left = torch.empty(max(need, qneed) + 64, dtype=torch.uint8, device="cuda")
    for fill in (0, 0xFF, None, None):              # zeros, ones, then twice over the leftovers of the calls before
        if fill is not None:
            left.fill_(fill)
        near, dist = N.vocab_nearest(rows["bytes_dev"], int(rows["ptr"][-1]), X["table_dev"], rows["unknown_off"],
                                     rows["unknown_len"], rows["n_unknown"], X["term_bytes"], X["term_ptr"], X["n_bytes"],
                                     term_rowptr=rowptr, max_edits=2, n_best=4, workspace=left)
        outs.append((near.clone(), dist.clone()))
        qouts.append(tuple(t.clone() for t in N.query_terms_fuzzy(qrows, qnear, 2, workspace=left)))
    for o in outs[1:]:
        assert torch.equal(o[0], outs[0][0]) and torch.equal(o[1], outs[0][1])
    for o in qouts[1:]:
        assert all(torch.equal(x, y) for x, y in zip(o, qouts[0]))
    nu = int(rows["n_unknown"].item())
    ids, d = expect(case, [FC.lowered(x) for x in case.needles] + ["abcdefg9", "zzzzzzzz"], True)
    assert nu == 3 and np.array_equal(outs[0][0][:nu].cpu().numpy(), ids) and np.array_equal(outs[0][1][:nu].cpu().numpy(), d)
