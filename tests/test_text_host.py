"""No GPU: the analysis table against backend.tokenize (every BMP code point in four contexts, random
strings), the exceptional set derived and not listed, the folding table, the properties of tests/text_cases.py,
the argument checks of thr_vocab_insert / thr_text_tokens / thr_query_terms before any launch (through the
library and in a stand-alone program under ASan + UBSan), and the client's ingest logic with the device calls
stubbed."""
import os
import random
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import text_cases as TC  # noqa: E402
import vocab_grow_cases as VG  # noqa: E402

import triple_hybrid_rag_amd as T  # noqa: E402
from triple_hybrid_rag_amd import backend, index_text as IT  # noqa: E402
from triple_hybrid_rag_amd.index_text import CONTEXTS, TextTable, fold_accents  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = T._native


@pytest.fixture(scope="module")
def table():
    return TextTable.default()


def exceptional_code_points(table):
    return [int(c) for c in np.flatnonzero(table.entries & N.THR_TEXT_EXC)]


# --------------------------------------------------------------------------- the table
def test_restatement_equals_tokenize_for_every_plain_bmp_code_point_in_four_contexts(table):
    exc = set(exceptional_code_points(table))
    assert len(exc) < 2048 + 64                  # the surrogates and a handful
    for cp in range(0x10000):
        if cp in exc:
            continue
        for ctx in CONTEXTS:
            s = ctx.format(chr(cp))
            assert table.restate(s) == backend.tokenize(s), (hex(cp), ctx)


@pytest.mark.parametrize("below", [0x10000, 0x250])
def test_restatement_equals_tokenize_on_random_strings(table, below):
    r = random.Random(below)
    plain = 0
    for _ in range(20_000):
        s = "".join(chr(r.randrange(below)) for _ in range(r.randrange(24)))
        assert table.tokenize(s) == backend.tokenize(s), repr(s)
        if not table.is_exceptional(s):
            plain += 1
            assert table.restate(s) == backend.tokenize(s), repr(s)
    assert plain > 5_000


def test_every_exceptional_code_point_is_one_where_the_model_fails(table):
    """None is listed by hand: each is a surrogate (the device sees its three-byte generalised form), has a
    lowering that is not one BMP code point, or breaks the per-character model in one of the contexts."""
    found = []
    for cp in exceptional_code_points(table):
        low = chr(cp).lower()
        if 0xD800 <= cp <= 0xDFFF:
            continue
        entry = int(table.entries[cp])
        # the model a plain entry would state for it
        plain = np.array(table.entries)
        plain[cp] = (ord(low[0]) if len(low) == 1 and ord(low) < 0x10000 else cp) | \
            (N.THR_TEXT_WORD if re.fullmatch(r"\w", low) else 0)
        model = TextTable(plain, backend.tokenize)
        fails = len(low) != 1 or ord(low) > 0xFFFF or \
            any(model.restate(c.format(chr(cp))) != backend.tokenize(c.format(chr(cp))) for c in CONTEXTS)
        assert fails, hex(cp)
        assert entry & N.THR_TEXT_EXC
        found.append(cp)
    assert 0x130 in found and 0x3A3 in found       # (what this Python gives; the set itself is derived)
    assert all(table.is_exceptional(chr(cp)) for cp in found)
    assert table.is_exceptional("a\U0001F600") and table.is_exceptional("\ud800") and not table.is_exceptional("añ中")
    assert all(int(table.entries[cp]) & N.THR_TEXT_EXC for cp in range(0xD800, 0xE000))
    # the lowerings that change the encoded length are plain entries, not exceptions
    longer = [cp for cp in range(0x10000) if not int(table.entries[cp]) & N.THR_TEXT_EXC and
              len(TC.enc(chr(cp))) != len(TC.enc(chr(int(table.entries[cp]) & 0xFFFF)))]
    assert {0x23A, 0x212A, 0x1E9E, 0x212B, 0x2126} <= set(longer)


def test_from_char_map_folding_table_is_map_each_character_then_words():
    fold = TextTable.from_char_map(fold_accents)

    def twin(text):
        return re.findall(r"\w+", "".join(fold_accents(c) for c in text))
    assert fold.tokenize("A AÇÃO do Coração, ÀS 5h") == ["a", "acao", "do", "coracao", "as", "5h"]
    r = random.Random(3)
    for below in (0x250, 0x10000, 0x20000):
        for _ in range(5_000):
            s = "".join(chr(r.randrange(below)) for _ in range(r.randrange(20)))
            assert fold.tokenize(s) == twin(s), repr(s)
            if not fold.is_exceptional(s):
                assert fold.restate(s) == twin(s), repr(s)
    assert IT.is_table_tokenizer(fold.tokenize) is fold and IT.is_table_tokenizer(backend.tokenize) is None
    assert IT.is_table_tokenizer(fold.restate) is None


# --------------------------------------------------------------------------- the cases and the restatements
def test_every_case_has_the_property_it_is_named_for():
    cases = TC.all_cases()
    assert len({c.name for c in cases}) == len(cases) >= 20
    for c in cases:
        assert c.holds(), c.name
        assert len(set(c.vocab)) == len(c.vocab), c.name
    names = " ".join(c.name for c in cases)
    for word in ("S-2", "lead_at_S-1", "lead_at_S-2", "boundary_at_S+0", "boundary_at_S-1", "boundary_at_S+1", "2S+500",
                 f"total_length_{TC.S}", f"total_length_{TC.S + 1}", "total_length_1", "70000"):
        assert word in names, word


def test_numpy_hash_is_fnv1a_and_the_numpy_table_is_found_by_the_documented_lookup():
    def fnv(b):
        h = 0xCBF29CE484222325
        for x in b:
            h = ((h ^ x) * 0x100000001B3) % (1 << 64)
        return h or 1
    keys = [b"", b"a", b"foobar", "ação".encode(), b"k123456", bytes(range(256))]
    assert TC.hash_keys(keys).tolist() == [fnv(k) for k in keys]
    assert fnv(b"a") == 0xAF63DC4C8601EC8C and fnv(b"foobar") == 0x85944171F73967E8      # the published vectors
    vocab = [f"t{i}".encode() for i in range(500)]
    slots = TC.build_table(vocab, 1024)
    assert [TC.table_lookup(slots, vocab, k) for k in vocab[:50]] == list(range(50))
    assert TC.table_lookup(slots, vocab, b"nope") == -1
    keys, slot = TC.colliding_keys(5, 1024)
    assert (TC.home_slot(TC.hash_keys([k.encode() for k in keys]), 1024) == slot).all()


def test_restatement_of_the_query_table_is_query_terms_loop():
    case = TC.query_cases()[0]
    ids = {t: i for i, t in enumerate(case.vocab)}
    terms, nd, flags = TC.expect_query_table(case.texts, ids)
    client = backend.GpuIndexClient.__new__(backend.GpuIndexClient)
    client.store = backend.CorpusStore([], [], [], [], [], [], vocab=ids)
    client.index = type("Lexical", (), {"lex": {}})()
    for conj in (False, True):
        client.lexical_and = conj
        for q, text in enumerate(case.texts):
            want = client._query_terms(text)
            row = terms[q][terms[q] >= 0].tolist()
            if conj and flags[q] & (N.THR_TEXT_UNKNOWN | N.THR_TEXT_TOO_MANY):
                assert want is None
            else:
                assert (want or []) == row
            assert IT.host_query_row(backend.tokenize(text), ids) == (row, int(nd[q]), int(flags[q]) & 6)


# --------------------------------------------------------------------------- the ABI, before any launch
def test_defines_equal_the_python_constants():
    header = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    for name in ("THR_TEXT_SLICE_BYTES", "THR_TEXT_MAX_TEXTS", "THR_TEXT_MAX_BYTES", "THR_TEXT_WORD", "THR_TEXT_EXC",
                 "THR_TEXT_EXCEPTIONAL", "THR_TEXT_UNKNOWN", "THR_TEXT_TOO_MANY", "THR_VOCAB_MIN_SLOTS", "THR_VOCAB_MAX_SLOTS"):
        m = re.search(r"#define\s+" + name + r"\s+(.+)", header)
        assert m, name
        assert eval(m.group(1).strip().strip("()"), {}) == getattr(N, name), name
    assert N.THR_TEXT_MAX_TEXTS == N.THR_ENTITY_MAX_QUERIES and N.THR_TEXT_MAX_BYTES < 2 ** 31
    assert N.ABI_VERSION == 9
    for sym in ("thr_vocab_table_bytes", "thr_vocab_insert", "thr_text_tokens_workspace_bytes", "thr_text_tokens",
                "thr_query_terms_workspace_bytes", "thr_query_terms"):
        assert sym in N.EXPORTED_SYMBOLS


def test_argument_checks_refuse_before_any_launch():
    lib = N.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    assert lib.thr_error_string(UNSUPPORTED) == b"unsupported shape" and lib.thr_error_string(WORKSPACE) == b"workspace too small"
    # the vocabulary
    assert lib.thr_vocab_table_bytes(1024) == 16384 and lib.thr_vocab_table_bytes(1000) == 0
    assert lib.thr_vocab_insert(None, 1024, 8192, 12288, 0, 1, None) == INVALID
    assert lib.thr_vocab_insert(4096, 1000, 8192, 12288, 0, 1, None) == INVALID          # not a power of two
    assert lib.thr_vocab_insert(4100, 1024, 8192, 12288, 0, 1, None) == INVALID          # misaligned
    assert lib.thr_vocab_insert(4096, 1024, 8192, 12288, 0, 513, None) == INVALID        # above 1/2 load

    def tokens(**kw):
        a = dict(text_bytes=4096, text_ptr=8192, n_texts=3, n_bytes=100, table=12288, slots=16384, capacity=1024,
                 term_bytes=20481, term_ptr=24576, n_vocab=512, token_capacity=52, tok_doc=28672, tok_term=32768,
                 n_tokens=36864, flags=40960, n_total=45056, unknown_off=49152, unknown_len=53248, n_unknown=57344,
                 workspace=61440, workspace_bytes=0)
        a.update(kw)
        return lib.thr_text_tokens(*a.values(), None)
    assert tokens() == WORKSPACE                          # every argument check passed
    for name in ("text_bytes", "text_ptr", "table", "slots", "term_bytes", "term_ptr", "tok_doc", "tok_term", "n_tokens",
                 "flags", "n_total", "unknown_off", "unknown_len", "n_unknown", "workspace"):
        assert tokens(**{name: None}) == INVALID, name
    for name, value in (("text_bytes", 4104), ("slots", 16392), ("text_ptr", 8196), ("term_ptr", 24580),
                        ("unknown_off", 49156), ("table", 12290)):
        assert tokens(**{name: value}) == INVALID, name
    assert tokens(workspace=61444, workspace_bytes=1 << 20) == INVALID
    assert tokens(capacity=1000) == INVALID and tokens(n_vocab=513) == INVALID
    assert tokens(n_texts=0) == UNSUPPORTED and tokens(n_texts=N.THR_TEXT_MAX_TEXTS + 1) == UNSUPPORTED
    assert tokens(n_bytes=N.THR_TEXT_MAX_BYTES + 1) == UNSUPPORTED and tokens(n_bytes=-1) == UNSUPPORTED
    assert tokens(n_texts=N.THR_TEXT_MAX_TEXTS, n_bytes=N.THR_TEXT_MAX_BYTES) == WORKSPACE
    need = lib.thr_text_tokens_workspace_bytes(3, 100, 52)
    assert need == 256 + 256 + 512 + 256 and tokens(workspace_bytes=need - 1) == WORKSPACE
    assert lib.thr_text_tokens_workspace_bytes(N.THR_TEXT_MAX_TEXTS + 1, 100, 52) == 0
    assert lib.thr_text_tokens_workspace_bytes(3, N.THR_TEXT_MAX_BYTES + 1, 52) == 0
    assert lib.thr_text_tokens_workspace_bytes(3, 100, 0) == 0 and lib.thr_text_tokens_workspace_bytes(0, 100, 52) == 0

    def query(**kw):
        a = dict(tok_term=4096, n_tokens=8192, text_flags=12288, n_total=16384, token_capacity=100, n_queries=7,
                 out_terms=20480, n_distinct=24576, out_flags=28672, workspace=32768, workspace_bytes=0)
        a.update(kw)
        return lib.thr_query_terms(*a.values(), None)
    assert query() == WORKSPACE
    for name in ("tok_term", "n_tokens", "text_flags", "n_total", "out_terms", "n_distinct", "out_flags", "workspace"):
        assert query(**{name: None}) == INVALID, name
    assert query(workspace=32770, workspace_bytes=4096) == INVALID
    assert query(n_queries=0) == UNSUPPORTED and query(n_queries=N.THR_TEXT_MAX_TEXTS + 1) == UNSUPPORTED
    assert lib.thr_query_terms_workspace_bytes(0) == 0 and lib.thr_query_terms_workspace_bytes(N.THR_TEXT_MAX_TEXTS + 1) == 0
    assert lib.thr_query_terms_workspace_bytes(7) == 256 and query(workspace_bytes=255) == WORKSPACE


def test_argument_checks_under_sanitizers(tmp_path):
    """The same checks in a stand-alone program (its own main), the host side of csrc/text.hip compiled with
    ASan + UBSan: run as a program on the CPU, never loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the library itself could not have been built")
    exe = str(tmp_path / "text_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "text.hip"),
                    os.path.join(ROOT, "tests", "native", "text_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "text host check: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# --------------------------------------------------------------------------- the client, device calls stubbed
class StubIndex(IT.TextSearch):
    """TextSearch with the two device calls restated on the host: what is tested is the logic around them."""
    torch = pytest.importorskip("torch")
    docs = doc_coll = tokens = graph = None

    def __init__(self, n_vocab):
        self.device = self.torch.device("cpu")
        self.lex = {"rowptr": self.torch.zeros(max(n_vocab, 1) + 1, dtype=self.torch.int64)}
        self.log = []

    def _t(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(dtype)

    def _extend_vocabulary(self, terms):
        self.log.append(("vocabulary", list(terms)))
        # (the key store's pointers stay in step: commit_vocabulary reads the vocabulary's size off them)
        self.text["term_ptr"] = self.torch.zeros(self.text["term_ptr"].shape[0] + len(terms), dtype=self.torch.int64)

    def _text_tokens(self, texts):
        X = self.text
        assert not any(X["table"].is_exceptional(t) for t in texts), "exceptional texts stay on the host"
        blob, ptr = IT.pack_texts(texts)
        doc, term, off, ln = [], [], [], []
        for d, t in enumerate(texts):
            for m in re.finditer(r"\S+", t.translate(X["table"]._map)):
                tid = X["ids"].get(m.group(), -1)
                doc.append(d)
                term.append(tid)
                if tid < 0:
                    off.append(int(ptr[d]) + len(TC.enc(t[:m.start()])))
                    ln.append(len(TC.enc(t[m.start():m.end()])))
        i32, i64 = self.torch.int32, self.torch.int64
        return dict(doc=self.torch.tensor(doc, dtype=i32), term=self.torch.tensor(term, dtype=i32),
                    n_total=self.torch.tensor([len(doc)], dtype=i32), n_unknown=self.torch.tensor([len(off)], dtype=i32),
                    unknown_off=self.torch.tensor(off, dtype=i64), unknown_len=self.torch.tensor(ln, dtype=i32),
                    capacity=max(len(doc), 1), blob=blob, ptr=ptr)

    def append_rows(self, **parts):
        if getattr(self, "refuse", False):
            raise N.NativeError("append_rows: refused")
        self.log.append(("append_rows", parts))


def _client(vocab, **kw):
    store = backend.CorpusStore([], [], [], [], [], [], vocab={t: i for i, t in enumerate(vocab)})
    return backend.GpuIndexClient(StubIndex(len(vocab)), store, org_id="org", **kw)


def _rows(texts, first=0):
    return [{"id": f"c{first + i}", "parent_id": "p", "document_id": "d", "text": t, "org_id": "org"}
            for i, t in enumerate(texts)]


BATCH = ["novo termo w1 novo", "", "w2 İstanbul primeiro termo", "outro Novo W3 primeiro", " ,, ", "İstanbul de novo"]


def test_device_text_numbers_new_terms_as_the_host_loop_and_commits_the_index_first():
    vocab = ["w1", "w2", "w3"]
    client = _client(vocab, device_text=True)
    idx = client.index
    assert idx.log == [("vocabulary", vocab)] and idx.text["ids"] == client.store.vocab
    client.insert_children(_rows(BATCH))
    # the host route's numbering, from its own loop
    want = {t: i for i, t in enumerate(vocab)}
    d_tok, t_tok = [], []
    for i, text in enumerate(BATCH):
        for tok in backend.tokenize(text):
            d_tok.append(i)
            t_tok.append(want.setdefault(tok, len(want)))
    assert list(client.store.vocab.items()) == list(want.items())
    kinds = [k for k, _ in idx.log]
    assert kinds == ["vocabulary", "append_rows", "vocabulary"]            # the rows, then the device vocabulary
    parts = idx.log[1][1]
    doc, term, tf, n_vocab = parts["lex"]
    assert doc.tolist() == d_tok and term.tolist() == t_tok and tf is None and n_vocab == len(want)
    assert idx.log[2][1] == list(want)[3:] and idx.text["ids"] == want
    assert client.store.texts == BATCH


def test_a_refused_append_leaves_store_and_vocabulary_as_they_were():
    client = _client(["w1", "w2", "w3"], device_text=True)
    client.index.refuse = True
    with pytest.raises(N.NativeError):
        client.insert_children(_rows(BATCH))
    assert client.store.vocab == {"w1": 0, "w2": 1, "w3": 2} and client.store.child_ids == []
    assert client.index.text["ids"] == {"w1": 0, "w2": 1, "w3": 2}
    assert [k for k, _ in client.index.log] == ["vocabulary"]


def test_device_text_refuses_a_custom_tokenizer_by_name():
    def my_tokenizer(text):
        return text.split()
    with pytest.raises(ValueError, match="my_tokenizer"):
        _client(["a"], device_text=True, tokenizer=my_tokenizer)
    assert _client(["a"], tokenizer=my_tokenizer).device_text is False          # the host route takes any
    fold = TextTable.from_char_map(fold_accents)
    client = _client(["acao"], device_text=True, tokenizer=fold.tokenize)
    assert client.index.text["table"] is fold
    client.insert_children(_rows(["Ação e reação"]))
    assert list(client.store.vocab) == ["acao", "e", "reacao"]
    with pytest.raises(ValueError, match="device_text"):
        _client(["a"]).query_terms_batch(["a"])
    with pytest.raises(ValueError, match="duplicates"):
        StubIndex(3).set_vocabulary(["a", "b", "a"])
    with pytest.raises(ValueError, match="lexical index"):
        StubIndex(3).set_vocabulary(["a", "b"])


def test_the_host_route_tokenises_each_text_once_and_hands_over_what_the_device_text_twin_does():
    calls = []

    def counting(text):
        calls.append(text)
        return backend.tokenize(text)
    vocab = ["w1", "w2", "w3"]
    host, twin = _client(vocab, tokenizer=counting), _client(vocab, device_text=True)
    assert host.insert_children(_rows(BATCH)) == twin.insert_children(_rows(BATCH))
    assert calls == BATCH                                        # once per row: not again for the store
    assert list(host.store.vocab.items()) == list(twin.store.vocab.items()) and len(host.store.vocab) == 10
    assert host.store.texts == twin.store.texts == BATCH
    assert [k for k, _ in host.index.log] == ["append_rows"] and host.index.text is None
    a, b = host.index.log[0][1]["lex"], twin.index.log[1][1]["lex"]
    assert np.asarray(a[0]).tolist() == b[0].tolist() and np.asarray(a[1]).tolist() == b[1].tolist()
    assert np.asarray(a[0]).dtype == np.asarray(a[1]).dtype == np.int32 and a[2:] == b[2:] == (None, 10)


def test_tokenizer_table_maps_tokenize_and_a_tables_tokenize_and_refuses_the_rest_by_name():
    fold = TextTable.from_char_map(fold_accents)
    assert IT.tokenizer_table(backend.tokenize, "x") is TextTable.default()
    assert IT.tokenizer_table(fold.tokenize, "x") is fold

    def plain_function(text):
        return text.split()
    for prefix in ("device_text=True", "from_rows(device=\"text\")"):
        for fn, name in ((fold.restate, "TextTable.restate"), (plain_function, "plain_function")):
            with pytest.raises(ValueError) as err:
                IT.tokenizer_table(fn, prefix)
            assert str(err.value).startswith(prefix + " needs ") and name in str(err.value)


def test_numbering_on_the_host_does_not_depend_on_hash_mask_or_packed():
    """Over the stub this shows the two arguments inert on the host route; that a forced collision on the
    device falls back to these values is tests/test_gpu_vocab_grow.py's."""
    vocab = ["w1", "w2", "w3"]
    idx = StubIndex(3).set_vocabulary(vocab)
    ids = {t: i for i, t in enumerate(vocab)}
    d_tok, t_tok, grown = VG.expect_numbered(BATCH, ids)
    for kw in ({}, {"hash_mask": 0x7}, {"packed": IT.pack_texts(BATCH)}, {"hash_mask": 0x7, "packed": IT.pack_texts(BATCH)}):
        R = idx.number_text_rows(BATCH, on_device=False, **kw)
        assert R.doc.tolist() == d_tok.tolist() and R.term.tolist() == t_tok.tolist(), kw
        assert R.pending.terms == grown and R.n_before == 3 and R.pending.key_bytes is None, kw
    assert idx.text["ids"] == ids and idx.log == [("vocabulary", vocab)]       # nothing was committed
