"""The token-level analysis on the GPU (thr_text_tokens_analyzed and the Python surface over it), held array for
array to the plain restatement of tests/text_analyzer_cases.py: stop tokens give no row, a row's term is its
stem's, an unknown stem is named by its token's first byte and the SOURCE byte length of the kept prefix.

Malformed UTF-8: in bounds is by construction -- every byte is read through a walk that ends at its text's end
(clamped to n_bytes), every key read lies inside the key of a slot whose id is inside the table, every rule
index is below the host-checked step pointer; a rule's len / min_stem are the only values CLAMPED on the device."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_analyzer_cases as AC  # noqa: E402
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


def ids_of(vocab):
    return {t: i for i, t in enumerate(vocab)}


def index_for(T, case, vocab=None):
    """A GpuIndex whose vocabulary is the case's with the case's analysis; a hand-built table replaces the
    compiled one as it stands."""
    from triple_hybrid_rag_amd.index_text import Analyzer, TextTable
    analyzer = Analyzer(TextTable.default(), case.stop, case.steps)
    idx = T.GpuIndex().set_vocabulary(case.vocab if vocab is None else vocab, analyzer)
    if case.table_order:
        step_ptr, rules = AC.rule_table(case.steps)
        idx.text["analysis"].update(step_ptr=step_ptr, rules=dev(rules))
    return idx


def host_copy(rows):
    torch.cuda.synchronize()
    n_total, n_unknown = int(rows["n_total"].item()), int(rows["n_unknown"].item())
    assert 0 <= n_total <= rows["capacity"] and 0 <= n_unknown <= n_total
    return dict(doc=rows["doc"][:n_total].cpu().numpy(), term=rows["term"][:n_total].cpu().numpy(),
                n_tokens=rows["n_tokens"].cpu().numpy(), flags=rows["flags"].cpu().numpy(),
                unknown_off=rows["unknown_off"][:n_unknown].cpu().numpy(),
                unknown_len=rows["unknown_len"][:n_unknown].cpu().numpy(), n_total=n_total, n_unknown=n_unknown)


def expect_places(texts, ids, case, table):
    """(offset, byte length) of every unknown stem of the plain texts, in row order, from the TEXT: the token's
    first byte and the source bytes of as many characters as the stem has."""
    ptr = np.concatenate([[0], np.cumsum([len(TC.enc(t)) for t in texts])])
    tokens = case.tokens(table)
    off, ln = [], []
    for d, t in enumerate(texts):
        if table.is_exceptional(t):
            continue
        for m in re.finditer(r"\S+", t.translate(table._map)):
            stem = tokens(m.group())
            if stem and stem[0] not in ids:
                off.append(int(ptr[d]) + len(TC.enc(t[:m.start()])))
                ln.append(len(TC.enc(t[m.start():m.start() + len(stem[0])])))
    return np.asarray(off, dtype=np.int64), np.asarray(ln, dtype=np.int32)


def assert_rows(got, texts, ids, case, table):
    E = AC.expect_rows(texts, ids, case.tokens(table), table)
    assert np.array_equal(got["flags"], E.flags), "flags"
    assert (E.flags == 0).all()                                    # (the cases here hold plain texts)
    assert np.array_equal(got["n_tokens"], E.n_tokens), "n_tokens"
    assert got["n_total"] == int(E.n_tokens.sum()) and np.array_equal(got["doc"], E.doc), "doc"
    assert np.array_equal(got["term"], E.term), "term"
    off, ln = expect_places(texts, ids, case, table)
    assert got["n_unknown"] == len(E.unknown) == len(off)
    assert np.array_equal(got["unknown_off"], off), "unknown_off"
    assert np.array_equal(got["unknown_len"], ln), "unknown_len: the kept prefix's SOURCE bytes"
    raw = b"".join(map(TC.enc, texts))
    have = [table.restate(raw[o:o + l].decode("utf-8", "surrogatepass")) for o, l in zip(off.tolist(), ln.tolist())]
    assert have == [[w] for w in E.unknown], "the lowered slice at an unknown row's place is the stem"


# ------------------------------------------------------------------ empty analyzer == thr_text_tokens
def test_empty_analyzer_equals_thr_text_tokens_on_every_text_case(T):
    N = T._native
    from triple_hybrid_rag_amd.index_text import pack_texts
    cases = TC.slice_cases() + TC.boundary_cases() + TC.lowering_cases() + TC.exceptional_cases()
    for case in cases:
        idx = T.GpuIndex().set_vocabulary(case.vocab)
        X = idx.text
        blob, ptr = pack_texts(case.texts)
        args = (dev(blob), dev(ptr), int(ptr[-1]), X["table_dev"], X["slots"], X["term_bytes"], X["term_ptr"])
        a = N.text_tokens(*args)
        b = N.text_tokens_analyzed(*args)
        torch.cuda.synchronize()
        n, u = int(a["n_total"].item()), int(a["n_unknown"].item())
        assert (n, u) == (int(b["n_total"].item()), int(b["n_unknown"].item())), case.name
        for k, m in (("doc", n), ("term", n), ("n_tokens", None), ("flags", None), ("unknown_off", u), ("unknown_len", u)):
            assert torch.equal(a[k][:m], b[k][:m]), (case.name, k)


# ------------------------------------------------------------------ the built cases
CASES = AC.all_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_analysed_rows_equal_the_restatement(T, case):
    from triple_hybrid_rag_amd.index_text import TextTable
    assert case.holds()
    idx = index_for(T, case)
    got = host_copy(idx._text_tokens(case.texts))
    assert_rows(got, case.texts, ids_of(case.vocab), case, TextTable.default())


def test_unknown_len_is_the_source_length_where_lowering_changes_it(T):
    """K 3 -> 1, Ⱥ 2 -> 3, ẞ 3 -> 2 bytes: the kept prefix 'KaȺẞ' is 9 source bytes and 7 lowered ones ... and the
    stop word 'ka' is reached only through the Kelvin sign's lowering."""
    from triple_hybrid_rag_amd.index_text import TextTable
    case = AC.lowering_cases()[0]
    idx = index_for(T, case)
    got = host_copy(idx._text_tokens(case.texts))
    text = case.texts[0]
    assert got["n_tokens"].tolist() == [4] and got["term"].tolist() == [-1, 0, -1, -1]
    words = text.split(" ")
    at = np.cumsum([0] + [len(TC.enc(w)) + 1 for w in words]).tolist()
    assert words[0][:4] == "\u212aa\u023a\u1e9e" and words[2] == "\u212aa" and len(words) == 5
    assert got["unknown_off"].tolist() == [at[0], at[3], at[4]]
    assert got["unknown_len"].tolist() == [len(TC.enc(words[0][:4])), len(TC.enc(words[3])), len(TC.enc(words[4]))] == [9, 7, 5]
    assert len(TC.enc(words[0][:4].lower())) == 7
    R = idx.text_rows(case.texts)
    assert R.unknown == ["ka\u2c65\u00df", "x\u00dfk", "kas"] and TextTable.default().restate("\u212aa") == ["ka"]


def test_a_slot_with_the_tokens_hash_and_other_bytes_is_passed_over(T):
    """A hand-built stop table: at foo's home slot an entry with foo's hash that names the key 'bar', behind it
    (first table only) the true entry.  The byte-for-byte verify passes the first over."""
    N = T._native
    from triple_hybrid_rag_amd.index_text import pack_texts
    idx = T.GpuIndex().set_vocabulary(["foo", "bar", "qux"])
    X = idx.text
    keys = [b"bar", b"foo"]
    sb, sp = pack_texts(["bar", "foo"])
    h = TC.hash_keys(keys)
    home = int(TC.home_slot(h[1:], 16)[0])
    assert int(TC.home_slot(h[:1], 16)[0]) not in (home, (home + 1) % 16)
    blob, ptr = pack_texts(["foo bar qux foo", "foo"])
    for with_true_entry, want in ((True, [2]), (False, [0, 2, 0, 0])):
        slots = np.zeros((16, 2), dtype=np.uint64)
        slots[home] = (h[1], 0)                                  # foo's hash, bar's bytes
        if with_true_entry:
            slots[(home + 1) % 16] = (h[1], 1)
        slots[int(TC.home_slot(h[:1], 16)[0])] = (h[0], 0)       # bar itself
        rows = N.text_tokens_analyzed(dev(blob), dev(ptr), int(ptr[-1]), X["table_dev"], X["slots"], X["term_bytes"], X["term_ptr"],
                                      stop_slots=dev(slots.view(np.int64)), stop_bytes=dev(sb), stop_ptr=dev(sp))
        got = host_copy(rows)
        assert got["term"].tolist() == want, with_true_entry
        assert got["n_tokens"].tolist() == ([1, 0] if with_true_entry else [3, 1])


# ------------------------------------------------------------------ unknown stems and numbering
def test_two_unknown_tokens_with_one_stem_get_one_id_and_one_key(T):
    from triple_hybrid_rag_amd.index_text import TextTable
    case = AC.unknown_cases()[0]
    table = TextTable.default()
    E = AC.expect_rows(case.texts, {}, case.tokens(table), table)
    assert E.new_terms == ["fal", "fala", "cant", "novo"] and E.numbered.tolist() == [0, 0, 0, 1, 0, 2, 2, 3]
    on, off = index_for(T, case), index_for(T, case)
    a = on.number_text_rows(case.texts)
    b = off.number_text_rows(case.texts, on_device=False)
    assert a.pending.key_bytes is not None and b.pending.key_bytes is None
    for r in (a, b):
        assert np.array_equal(r.doc.cpu().numpy(), E.doc) and np.array_equal(r.term.cpu().numpy(), E.numbered)
        assert r.pending.terms == E.new_terms and r.pending.n_new == 4 and r.n_before == 0
    on.commit_vocabulary(a.pending)
    off.commit_vocabulary(b.pending)
    assert list(on.text["ids"]) == list(off.text["ids"]) == E.new_terms
    for idx in (on, off):
        again = host_copy(idx._text_tokens(case.texts))
        assert again["n_unknown"] == 0 and np.array_equal(again["term"], E.numbered)
    rows = on.text_rows(case.texts + ["cantando nunca"])
    assert rows.unknown == ["nunca"] and rows.term.tolist()[-2:] == [2, -1]


# ------------------------------------------------------------------ malformed bytes, through the raw ABI
@pytest.mark.parametrize("bad", [b"casas \xe2\x82", b"de \x80 casas", b"\xa9casas de", b"casas\xc0\xaf de", b"casa\xe2\x82s de",
                                 b"de\xf5\x80\x80\x80"], ids=["cut_lead", "stray_continuation", "leading_continuation", "overlong",
                                                              "cut_inside_a_suffix", "impossible_lead"])
def test_malformed_utf8_flags_its_text_and_spares_the_neighbours(T, bad):
    N = T._native
    case = AC.stop_cases()[0]
    idx = index_for(T, case)
    X, A = idx.text, idx.text["analysis"]
    blobs = [b"de casa a", bad, b"comeu casa de"]
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    blob = np.frombuffer(b"".join(blobs) + bytes(16), dtype=np.uint8)
    got = host_copy(N.text_tokens_analyzed(dev(blob), dev(ptr), int(ptr[-1]), X["table_dev"], X["slots"], X["term_bytes"],
                                           X["term_ptr"], **A))
    assert got["flags"].tolist() == [0, 1, 0]
    assert np.array_equal(got["doc"], np.repeat(np.arange(3), got["n_tokens"]))
    assert got["n_tokens"][0] == 1 and got["n_tokens"][2] == 2           # comeu -> com, a stem that equals a stop word
    assert got["term"][got["doc"] == 0].tolist() == [0] and got["term"][got["doc"] == 2].tolist() == [1, 0]


# ------------------------------------------------------------------ workspace
def test_same_bits_whatever_the_workspace_held_and_every_run(T):
    N = T._native
    from triple_hybrid_rag_amd.index_text import pack_texts
    case = AC.stop_cases()[1]                                         # 70 000 tiny texts: several slices, stop words, a rule
    idx = index_for(T, case)
    X, A = idx.text, idx.text["analysis"]
    blob, ptr = pack_texts(case.texts)
    args = (dev(blob), dev(ptr), int(ptr[-1]), X["table_dev"], X["slots"], X["term_bytes"], X["term_ptr"])
    cap = N.text_token_capacity(len(case.texts), int(ptr[-1]))
    need = N.text_tokens_analyzed_workspace_bytes(len(case.texts), int(ptr[-1]), cap)
    outs = []
    for fill in (0x00, 0xFF, 0xFF):
        ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
        rows = N.text_tokens_analyzed(*args, workspace=ws, **A)
        h = host_copy(rows)
        outs.append(h)
    for other in outs[1:]:
        for k in ("doc", "term", "n_tokens", "flags", "unknown_off", "unknown_len"):
            assert outs[0][k].tobytes() == other[k].tobytes(), k
        assert (outs[0]["n_total"], outs[0]["n_unknown"]) == (other["n_total"], other["n_unknown"])


# ------------------------------------------------------------------ queries
def test_query_terms_for_65600_queries_both_forms(T):
    from triple_hybrid_rag_amd.index_text import Analyzer, TextTable
    table = TextTable.default()
    a = Analyzer.portuguese()
    words = [w for p in AC.pairs(AC.PT_SAME) for w in p]
    vocab = list(dict.fromkeys(a.stem(w) for w in words)) + [f"t{i}" for i in range(40)]
    ids = ids_of(vocab)
    r = np.random.default_rng(9)
    glue = ["de", "a", "o", "que", "não", "para"]
    special = ["de a o que", "", "Os documentos das locações", "os documentos nuncavisto", " ".join(f"t{i}" for i in range(33)),
               " ".join(f"t{i}" for i in range(32)) + " de a", "que de QUE", "nuncavisto de"]
    queries = special + [" ".join(r.choice(words + glue + ["nuncavisto"] * 2, r.integers(0, 9))) for _ in range(65_600 - len(special))]
    assert len(queries) == 65_600
    idx = T.GpuIndex().set_vocabulary(vocab, a)
    want, _, wflags = AC.expect_query_table(queries, ids, a.tokenize, table)
    N = T._native
    # all-stop-word queries behave as an empty query: nothing, no UNKNOWN flag, not voided
    assert wflags[0] == wflags[1] == wflags[6] == 0 and (want[[0, 1, 6]] == -1).all()
    assert wflags[3] == wflags[7] == N.THR_TEXT_UNKNOWN and wflags[4] == N.THR_TEXT_TOO_MANY and wflags[5] == 0
    assert want[2, :3].tolist() == [ids["document"], ids["locaç"], -1]
    for conj in (False, True):
        terms, flags = idx.query_terms(queries, conjunctive=conj)
        torch.cuda.synchronize()
        e = want.copy()
        if conj:
            e[(wflags & (N.THR_TEXT_UNKNOWN | N.THR_TEXT_TOO_MANY)) != 0] = -1
        assert np.array_equal(flags.cpu().numpy(), wflags), conj
        assert np.array_equal(terms.cpu().numpy(), e), conj
    assert (idx.query_terms(queries, conjunctive=True)[0][2, :2].cpu().numpy() == want[2, :2]).all()


# ------------------------------------------------------------------ the surface
def _rows(texts, d, seed, first=0):
    rng = np.random.default_rng(seed)
    return [{"id": f"c{first + i}", "parent_id": "p0", "document_id": "d0", "text": t, "page": 1, "modality": "text",
             "embedding_1024": rng.standard_normal(d).astype(np.float32).tolist(), "org_id": "org"} for i, t in enumerate(texts)]


PARENTS = [{"id": "p0", "text": "parent", "section_heading": "S"}]


def test_twin_clients_host_hook_and_device_text_insert_search_delete_insert(T):
    from test_gpu_append import _assert_lex_equal, same
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.index_text import Analyzer
    a = Analyzer.portuguese()
    d = 1024
    corpus = AC.portuguese_corpus(300)
    corpus[7] = "O documento do fiador"                       # the singular only: c7
    base = _rows(corpus, d, 1)
    clients = []
    for kw in ({}, {"device_text": True, "number_on_device": True}):
        hi = IB.from_rows(base, PARENTS, tokenizer=a.tokenize)
        clients.append(GpuIndexClient(hi.to_gpu(), hi.store, org_id="org", tokenizer=a.tokenize, **kw))
    host, devc = clients
    assert devc.index.text["table"] is a and host.index.text is None
    first = _rows(["Novos inquilinos pagaram as multas", "", "de a o", "İstanbul dos inquilinos", "Pagando multa nova"], d, 2, 1000)
    second = _rows(["Os inquilinos devolveram os imóveis", "multas e devoluções"], d, 3, 2000)

    def search(q, conj):
        out = []
        for c in (host, devc):
            c.lexical_and = conj
            out.append([(r["child_id"], r["rank"]) for r in c.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": q, "p_limit": 100}).data])
        assert out[0] == out[1], (q, conj)
        return out[0]

    def same_state():
        assert list(host.store.vocab.items()) == list(devc.store.vocab.items())
        same(host.index.docs, devc.index.docs, "docs")
        _assert_lex_equal(host.index, devc.index)
        assert devc.index.text["ids"] == devc.store.vocab

    assert host.insert_children(first) == devc.insert_children(first)
    same_state()
    assert "inquilin" in devc.store.vocab and "de" not in devc.store.vocab and "multa" not in devc.store.vocab
    for q in ("documentos", "os documentos dos fiadores", "inquilino pagou multa", "de a o", "nuncavisto documentos", "İstanbul"):
        for conj in (False, True):
            search(q, conj)
    # a query in plural form returns the chunk that holds the singular
    assert "c7" in [cid for cid, _ in search("documentos fiadores", True)]
    assert search("de a o que", False) == [] and search("nuncavisto documentos", True) == []
    gone = ["c7", "c1000", "c12"]
    assert host.delete_children(gone) == devc.delete_children(gone)
    same_state()
    assert "c7" not in [cid for cid, _ in search("documentos fiadores", False)]
    assert host.insert_children(second) == devc.insert_children(second)
    same_state()
    assert "c2000" in [cid for cid, _ in search("imóveis devolveram", True)]
    # bm25_search on the device-made term table equals the host-made one
    qs = ["os documentos das locações", "falando de contratos", "que de", "clientes novos pagaram"]
    dev_terms = devc.query_terms_batch(qs)
    host_terms = np.full((len(qs), MT), -1, dtype=np.int32)
    for i, q in enumerate(qs):
        row = host._query_terms(q) or []
        host_terms[i, :len(row)] = row
    assert np.array_equal(dev_terms.cpu().numpy(), host_terms)
    Sa, Ia, _ = devc.index.bm25_search(dev_terms, 10)
    Sb, Ib, _ = host.index.bm25_search(dev(host_terms), 10)
    assert torch.equal(Ia, Ib) and torch.equal(Sa, Sb)


def test_from_rows_device_text_equals_from_rows_with_the_analyzer(T):
    from test_gpu_vocab_grow import assert_same_host_index
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.index_text import Analyzer
    a = Analyzer.portuguese()
    texts = AC.portuguese_corpus(400, seed=8)
    texts[57] = ""
    texts[58] = "de a o que"
    texts[211] = "uma İstanbul no meio dos documentos nunca_vistos"
    texts[212] = "nunca_visto depois"
    chunks = [{"id": f"c{i}", "parent_id": "p0", "document_id": "d0", "text": t, "embedding_1024": [float(i % 7), 1.0, 0.0, 2.0]}
              for i, t in enumerate(texts)]
    want = IB.from_rows(chunks, PARENTS, tokenizer=a.tokenize)
    got = IB.from_rows(chunks, PARENTS, tokenizer=a.tokenize, device="text", batch_bytes=4096)
    assert_same_host_index(got, want)
    assert "document" in got.store.vocab and "de" not in got.store.vocab and got.doclen[58] == 0
    assert_same_host_index(IB.from_rows(chunks, PARENTS, tokenizer=a.tokenize, device="text"), want)
