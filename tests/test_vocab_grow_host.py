"""No GPU: the restatement of thr_vocab_grow's contract (tests/vocab_grow_cases.py) against the numbering of
lexical_rows (pandas' factorize) and build_lexical, the properties the built cases are named for, the new
names in the header / the exports / the binding, the argument checks before any launch (through the library and
in a stand-alone program under ASan + UBSan), and the client's ingest order with the device calls stubbed."""
import os
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
from triple_hybrid_rag_amd import backend, index_build as IB, index_text as IT  # noqa: E402
from triple_hybrid_rag_amd.index_text import TextTable, fold_accents  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = T._native


def ids_of(vocab):
    return {t: i for i, t in enumerate(vocab)}


# --------------------------------------------------------------------------- the restatement
CORPORA = [(c.name, c.texts) for c in TC.all_cases()] + [(c.name, c.texts) for c in VG.all_cases()]


@pytest.mark.parametrize("name,texts", CORPORA, ids=[n for n, _ in CORPORA])
def test_restatement_is_the_numbering_of_lexical_rows_and_build_lexical(name, texts):
    """From an empty vocabulary every token is unknown: the restatement's ids are pandas' factorize codes and
    its keys build_lexical's vocabulary, in order.  (Exceptional texts are the host's: left out here.)"""
    table = TextTable.default()
    plain = [t for t in texts if not table.is_exceptional(t)]
    U = VG.unknown_list(plain, {})
    E = VG.expect_grow(U["blob"], U["ptr"], U["flags"], U["off"], U["len"], 0, tok_term=U["term"])
    vocab, doc, term = IB.lexical_rows(plain)
    assert E["keys"] == list(vocab) and np.array_equal(E["unknown_term"], term) and np.array_equal(E["tok_term"], term)
    assert not E["collision"] and E["n_new"] == len(vocab)
    assert bytes(E["new_bytes"]) == b"".join(TC.enc(t) for t in vocab) and E["new_ptr"][-1] == E["n_new_bytes"]
    if len(plain) <= 200:
        assert list(IB.build_lexical(plain)[0]) == E["keys"]
    d2, t2, grown = VG.expect_numbered(plain, {})
    assert grown == E["keys"] and np.array_equal(t2, term) and np.array_equal(d2, doc)


def test_restatement_numbers_behind_a_vocabulary_and_skips_flagged_texts():
    texts = ["novo w1 Novo", "İstanbul novo raro", "raro W2 outro novo"]
    ids = ids_of(["w1", "w2"])
    U = VG.unknown_list(texts, ids)
    assert U["flags"].tolist() == [0, 1, 0]
    E = VG.expect_grow(U["blob"], U["ptr"], U["flags"], U["off"], U["len"], 2, tok_term=U["term"])
    assert E["keys"] == ["novo", "raro", "outro"] and E["unknown_term"].tolist()[:2] == [2, 2]
    assert (E["unknown_term"] == -1).sum() >= 3 and E["unknown_term"].tolist()[-3:] == [3, 4, 2]
    assert E["tok_term"].tolist()[:3] == [2, 0, 2] and E["tok_term"].tolist()[-4:] == [3, 1, 4, 2]
    # a folding table: the keys are the folded strings
    fold = TextTable.from_char_map(fold_accents)
    U = VG.unknown_list(["Ação ACAO razão"], {}, fold)
    assert VG.expect_grow(U["blob"], U["ptr"], U["flags"], U["off"], U["len"], 0, fold)["keys"] == ["acao", "razao"]


# --------------------------------------------------------------------------- the cases
def test_every_case_has_the_property_it_is_named_for():
    cases = VG.all_cases()
    assert len({c.name for c in cases}) == len(cases) >= 18
    for c in cases:
        assert c.holds(), c.name
        assert len(set(c.vocab)) == len(c.vocab), c.name
    names = " ".join(c.name for c in cases)
    for word in ("n_unknown_0", "n_unknown_1", "n_unknown_63", "n_unknown_64", "n_unknown_65", "n_unknown_255",
                 "n_unknown_256", "n_unknown_257", "n_unknown_3100", "slice_edge", "byte_length", "empty_vocabulary",
                 "every_token_known", "70000", "100000", "2S+500", "wraps", "hash_mask_7"):
        assert word in names, word
    assert "K" in VG.SPELLINGS and "Ⱥ" in VG.SPELLINGS and "ẞ" in VG.SPELLINGS


def test_sightings_fall_in_the_units_the_slice_case_names():
    case = VG.slice_case()
    at = VG.sightings(case, "edgetok")
    assert [a // VG.S for a in at] == [2, 3, 9] and [a // VG.UNIT for a in at] == [11, 12, 36]
    assert at[0] < 3 * VG.S <= at[1]                      # on either side of the edge, in two texts
    U = VG.unknown_list(case.texts, ids_of(case.vocab))
    E = VG.expect_grow(U["blob"], U["ptr"], U["flags"], U["off"], U["len"], 3)
    assert E["keys"] == ["early1", "early2", "edgetok", "later1", "end"]       # its rank is 2: others came first


def test_masked_hashes_collide_and_full_hashes_do_not():
    case = VG.masked_case()
    U = VG.unknown_list(case.texts, {})
    assert VG.expect_grow(U["blob"], U["ptr"], U["flags"], U["off"], U["len"], 0, hash_mask=0x7)["collision"]
    assert not VG.expect_grow(U["blob"], U["ptr"], U["flags"], U["off"], U["len"], 0)["collision"]
    assert VG.masked_hashes([b"a"], VG.ALL_ONES)[0] == 0xAF63DC4C8601EC8C and VG.masked_hashes([b"a"], 0x3)[0] == 1
    assert VG.masked_hashes([b"a"], 0xF0)[0] == 0x80


def test_the_chain_of_the_scratch_table_wraps():
    case = VG.chain_case()
    assert case.holds()
    n = VG.n_unknown_of(case)
    cap = VG.scratch_capacity(n)
    assert (n, cap) == (400, 1024) and VG.scratch_capacity(1) == 16 and VG.scratch_capacity(8) == 16
    assert VG.scratch_capacity(9) == 32 and VG.scratch_capacity(512) == 1024 and VG.scratch_capacity(513) == 2048
    keys = list(dict.fromkeys(tok for t in case.texts for tok in t.split()))
    slots = TC.build_table([k.encode() for k in keys], cap)
    used = np.flatnonzero(slots[:, 0] != 0)
    assert len(used) == 300 and used.min() == 0 and used.max() == cap - 1      # the chain runs over the end


# --------------------------------------------------------------------------- the ABI, before any launch
def test_header_exports_and_binding_agree_on_the_new_names():
    header = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    for name in ("THR_VOCAB_GROW_COLLISION", "THR_VOCAB_GROW_OVERFLOW"):
        m = re.search(r"#define\s+" + name + r"\s+(.+)", header)
        assert m, name
        assert eval(m.group(1).strip().strip("()"), {}) == getattr(N, name), name
    lib = N.load()
    for sym in ("thr_vocab_grow_workspace_bytes", "thr_vocab_grow"):
        assert sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym) and re.search(rf"\b{sym}\s*\(", header)
    assert N.ABI_VERSION == 9 and lib.thr_abi_version() == 9                    # additions only
    proto = re.search(r"int thr_vocab_grow\((.*?)\);", header, flags=re.S).group(1)
    assert len(proto.split(",")) == len(N._SIGNATURES["thr_vocab_grow"][1]) == 25
    assert all(hasattr(IT.TextSearch, m) for m in ("number_text_rows", "commit_vocabulary"))


def test_argument_checks_refuse_before_any_launch():
    lib = N.load()
    INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
    need = lib.thr_vocab_grow_workspace_bytes
    assert need(52) == 128 * 16 + 3 * 256 + 512 + 65792 and need(0) == 0 and need(N.THR_TEXT_MAX_BYTES + 1) == 0

    def grow(**kw):
        a = dict(text_bytes=4096, text_ptr=8192, n_texts=3, n_bytes=100, table=12288, flags=16384, unknown_off=20480,
                 unknown_len=24576, n_unknown=28672, unknown_capacity=52, n_vocab=512, hash_mask=(1 << 64) - 1,
                 tok_term=32768, n_total=36864, token_capacity=52, unknown_term=40960, new_bytes=45057,
                 new_bytes_capacity=1000, new_ptr=49152, n_new=53248, n_new_bytes=57344, status=61440, workspace=65536,
                 workspace_bytes=0)
        a.update(kw)
        return lib.thr_vocab_grow(*a.values(), None)
    assert grow() == WORKSPACE                            # every argument check passed
    for name in ("text_bytes", "text_ptr", "table", "flags", "unknown_off", "unknown_len", "n_unknown", "unknown_term",
                 "new_bytes", "new_ptr", "n_new", "n_new_bytes", "status", "workspace", "n_total"):
        assert grow(**{name: None}) == INVALID, name
    assert grow(tok_term=None, n_total=None, token_capacity=0) == WORKSPACE      # the patch is optional
    for name, value in (("text_bytes", 4104), ("text_ptr", 8196), ("unknown_off", 20484), ("new_ptr", 49156),
                        ("table", 12290)):
        assert grow(**{name: value}) == INVALID, name
    assert grow(workspace=65544, workspace_bytes=1 << 20) == INVALID
    assert grow(n_texts=0) == UNSUPPORTED and grow(n_texts=N.THR_TEXT_MAX_TEXTS + 1) == UNSUPPORTED
    assert grow(n_bytes=-1) == UNSUPPORTED and grow(n_bytes=N.THR_TEXT_MAX_BYTES + 1) == UNSUPPORTED
    assert grow(unknown_capacity=0) == UNSUPPORTED and grow(unknown_capacity=N.THR_TEXT_MAX_BYTES + 1) == UNSUPPORTED
    assert grow(n_vocab=-1) == INVALID and grow(n_vocab=2 ** 31 - 1 - 51) == INVALID
    assert grow(n_vocab=2 ** 31 - 1 - 52) == WORKSPACE and grow(n_vocab=0) == WORKSPACE
    assert grow(hash_mask=0) == INVALID and grow(hash_mask=7) == WORKSPACE
    assert grow(workspace_bytes=need(52) - 1) == WORKSPACE


def test_argument_checks_under_sanitizers(tmp_path):
    """The same checks in a stand-alone program (its own main), the host side of csrc/vocab_grow.hip compiled
    with ASan + UBSan: run as a program on the CPU, never loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the library itself could not have been built")
    exe = str(tmp_path / "vocab_grow_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "vocab_grow.hip"),
                    os.path.join(ROOT, "tests", "native", "vocab_grow_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "vocab grow host check: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# --------------------------------------------------------------------------- the client, device calls stubbed
class StubIndex(IT.TextSearch):
    """TextSearch with number_text_rows / commit_vocabulary restated on the host (the contract's words: the
    host loop's numbering): what is tested is the order the client calls them in and what it hands over."""
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

    def number_text_rows(self, texts, hash_mask=None, packed=None):
        ids = self.text["ids"]
        doc, term, grown = VG.expect_numbered(texts, ids, self.text["table"].tokenize)
        self.log.append(("number_text_rows", len(texts)))
        return IT.NumberedRows(self.torch.from_numpy(doc), self.torch.from_numpy(term), len(ids),
                               IT.PendingVocabulary(len(ids), len(grown), terms=grown))

    def commit_vocabulary(self, pending, mirror=True):
        assert pending.n_before == len(self.text["ids"])
        self.log.append(("commit_vocabulary", list(pending.terms)))
        for i, t in enumerate(pending.terms):
            self.text["ids"][t] = pending.n_before + i

    def append_rows(self, **parts):
        if getattr(self, "refuse", False):
            raise N.NativeError("append_rows: refused")
        self.log.append(("append_rows", parts))


def _client(vocab, **kw):
    store = backend.CorpusStore([], [], [], [], [], [], vocab=ids_of(vocab))
    return backend.GpuIndexClient(StubIndex(len(vocab)), store, org_id="org", **kw)


def _rows(texts, first=0):
    return [{"id": f"c{first + i}", "parent_id": "p", "document_id": "d", "text": t, "org_id": "org"}
            for i, t in enumerate(texts)]


BATCH = ["novo termo w1 novo", "", "w2 İstanbul primeiro termo", "outro Novo W3 primeiro", " ,, ", "İstanbul de novo"]


NUMBERED = [("the_batch", BATCH, ["w1", "w2", "w3"]), ("the_empty_batch", [], ["w1"]),
            ("every_token_known", ["w1 W2", "", "w2 w1 W1"], ["w1", "w2"]),
            ("every_token_new", ["novo termo Novo", " ,, ", "outro termo novo"], [])]


@pytest.mark.parametrize("name,texts,vocab", NUMBERED, ids=[n for n, _, _ in NUMBERED])
def test_number_tokens_is_the_restatement(name, texts, vocab):
    ids = ids_of(vocab)
    doc, term, new_terms = IT.number_tokens([backend.tokenize(t) for t in texts], ids)
    d_tok, t_tok, grown = VG.expect_numbered(texts, ids_of(vocab))
    assert doc.dtype == term.dtype == np.int32 and doc.shape == term.shape == d_tok.shape
    assert np.array_equal(doc, d_tok) and np.array_equal(term, t_tok) and new_terms == grown
    assert ids == ids_of(vocab)                                   # the vocabulary is only read
    if name == "every_token_known":
        assert new_terms == [] and len(term) == 5
    if name == "every_token_new":
        assert new_terms == ["novo", "termo", "outro"] and term.tolist() == [0, 1, 0, 2, 1, 0]


def test_number_on_device_takes_number_append_commit_store_in_that_order():
    vocab = ["w1", "w2", "w3"]
    client = _client(vocab, device_text=True, number_on_device=True)
    idx = client.index
    client.insert_children(_rows(BATCH))
    d_tok, t_tok, grown = VG.expect_numbered(BATCH, ids_of(vocab))
    assert [k for k, _ in idx.log] == ["vocabulary", "number_text_rows", "append_rows", "commit_vocabulary"]
    doc, term, tf, n_vocab = idx.log[2][1]["lex"]
    assert doc.tolist() == d_tok.tolist() and term.tolist() == t_tok.tolist() and tf is None
    assert n_vocab == len(vocab) + len(grown) and idx.log[3][1] == grown
    assert list(client.store.vocab.items()) == [(t, i) for i, t in enumerate(vocab + grown)]
    assert idx.text["ids"] == client.store.vocab and client.store.texts == BATCH
    # ... and the vocabulary is the host route's
    host = _client(vocab)
    host.insert_children(_rows(BATCH))
    assert list(host.store.vocab.items()) == list(client.store.vocab.items())


def test_a_refused_append_leaves_store_and_vocabulary_as_they_were():
    client = _client(["w1", "w2", "w3"], device_text=True, number_on_device=True)
    client.index.refuse = True
    with pytest.raises(N.NativeError):
        client.insert_children(_rows(BATCH))
    assert client.store.vocab == {"w1": 0, "w2": 1, "w3": 2} and client.store.child_ids == []
    assert client.index.text["ids"] == {"w1": 0, "w2": 1, "w3": 2}
    assert [k for k, _ in client.index.log] == ["vocabulary", "number_text_rows"]


def test_number_on_device_without_device_text_is_refused_by_name():
    with pytest.raises(ValueError, match="number_on_device"):
        _client(["a"], number_on_device=True)
    assert _client(["a"], device_text=True).number_on_device is False           # the default stays off
    assert _client(["a"]).number_on_device is False


def test_pending_vocabulary_and_commit_checks_without_a_device():
    idx = StubIndex(2)
    idx.text = dict(ids={"a": 0, "b": 1}, term_ptr=idx.torch.zeros(3, dtype=idx.torch.int64))
    p = IT.PendingVocabulary(2, 2, terms=["c", "d"])
    assert p.terms == ["c", "d"] and IT.PendingVocabulary(5, 0).terms == []
    with pytest.raises(ValueError, match="numbered from 1"):
        IT.TextSearch.commit_vocabulary(idx, IT.PendingVocabulary(1, 1, terms=["x"]))
    IT.TextSearch.commit_vocabulary(idx, IT.PendingVocabulary(2, 0))
    assert idx.text["ids"] == {"a": 0, "b": 1}


def test_from_rows_device_text_refuses_a_foreign_tokenizer_and_an_unknown_mode_by_name():
    def my_tokenizer(text):
        return text.split()
    rows = [{"id": "c0", "text": "a b"}]
    with pytest.raises(ValueError, match="my_tokenizer"):
        IB.from_rows(rows, tokenizer=my_tokenizer, device="text")
    with pytest.raises(ValueError, match="texts"):
        IB.from_rows(rows, device="texts")
