"""No GPU: typo-tolerant lexical queries (include/thr_hip_fuzzy.h; index_text.nearest_terms_host is the definition).
The new header against its binding table, the edit distance against an independent definition, every built case
against the property it is named for (and a wrong variant against it), Fuzzy's refusals, the fuzzy=None route call
for call, and the argument checks of both entries (through the library and in a stand-alone sanitized program)."""
import functools
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import fuzzy_cases as FC  # noqa: E402
import triple_hybrid_rag_amd as T  # noqa: E402
from test_native_abi import ctype_class, declared_symbols, header_class  # noqa: E402
from triple_hybrid_rag_amd import _native as N  # noqa: E402
from triple_hybrid_rag_amd import index_text as IT  # noqa: E402
from triple_hybrid_rag_amd.index_text import Fuzzy  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thr_hip_fuzzy.h")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3
NAMES = ["thr_query_terms_fuzzy", "thr_query_terms_fuzzy_workspace_bytes", "thr_vocab_nearest",
         "thr_vocab_nearest_workspace_bytes"]


# --------------------------------------------------------------------------- header, binding, constants
def _header_text():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    lines = text.split("\n")
    return "\n".join(ln for ln in lines if not ln.lstrip().startswith("#")), [ln for ln in lines if ln.lstrip().startswith("#")]


def _header_prototypes():
    text, _ = _header_text()
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(thr_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text):
        res, name, params = m.group(1), m.group(2), m.group(3).strip()
        res = " ".join(w for w in res.split() if w != "extern")
        args = []
        for p in params.split(","):
            p = p.strip()
            args.append(header_class(re.sub(r"[A-Za-z_]\w*$", "", p) if re.search(r"[\s\*][A-Za-z_]\w*$", p) else p))
        protos[name] = (header_class(res), args)
    return protos


def test_the_new_header_and_its_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(N._SIGNATURES_FUZZY) == NAMES
    for name, (res, args) in N._SIGNATURES_FUZZY.items():
        want_res, want_args = protos[name]
        assert ctype_class(res) == want_res, name
        got = [ctype_class(a) for a in args]
        assert len(got) == len(want_args), f"{name}: {len(got)} argtypes, the header declares {len(want_args)} parameters"
        for i, (g, w) in enumerate(zip(got, want_args)):
            assert g == w, f"{name}: argument {i}"
    lib = N.load()
    for name in protos:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == N._SIGNATURES_FUZZY[name][1]
    # everything thr_query_terms takes, in its order, around the four correction operands
    base = N._SIGNATURES["thr_query_terms"][1]
    mine = N._SIGNATURES_FUZZY["thr_query_terms_fuzzy"][1]
    assert mine[:6] == base[:6] and mine[10:] == base[6:] and len(mine) == len(base) + 4
    _, defines = _header_text()
    header = {m.group(1): int(m.group(2)) for m in (re.match(r"\s*#\s*define\s+(THR_[A-Z0-9_]+)\s+(\d+)\s*$", ln) for ln in defines) if m}
    assert header == {"THR_FUZZY_MAX_LEN": N.FUZZY_MAX_LEN, "THR_FUZZY_MAX_BEST": N.FUZZY_MAX_BEST,
                      "THR_FUZZY_SLICE_BYTES": N.FUZZY_SLICE_BYTES, "THR_TEXT_CORRECTED": N.TEXT_CORRECTED}
    assert (N.FUZZY_MAX_LEN, N.FUZZY_MAX_BEST, N.TEXT_CORRECTED, N.FUZZY_MAX_EDITS) == (32, 4, 8, 2)
    assert (IT.THR_FUZZY_MAX_LEN, IT.THR_FUZZY_MAX_BEST, IT.THR_TEXT_CORRECTED) == (32, 4, 8)
    assert N.TEXT_CORRECTED & (N.THR_TEXT_EXCEPTIONAL | N.THR_TEXT_UNKNOWN | N.THR_TEXT_TOO_MANY) == 0
    assert '#include "thr_hip.h"' in open(HEADER).read()
    assert "thr_hip_fuzzy.h" in [os.path.basename(h) for h in T._build._headers()]
    assert os.path.join(T._build.CSRC, "fuzzy.hip") in T._build.sources()
    # additive: thr_hip.h keeps its prototypes and the ABI version
    assert len(declared_symbols()) == len(N.EXPORTED_SYMBOLS) == 65 and N.ABI_VERSION == 9
    others = (set(N.EXPORTED_SYMBOLS) | set(N._SIGNATURES_GRAPH) | set(N._SIGNATURES_TEXT) | set(N._SIGNATURES_RERANK)
              | set(N._SIGNATURES_PARENT) | set(N._SIGNATURES_DIVERSIFY))
    assert not set(N._SIGNATURES_FUZZY) & others
    assert "fuzzy" not in open(os.path.join(ROOT, "include", "thr_hip.h")).read().lower()
    assert T.Fuzzy is Fuzzy


def test_design_md_holds_a_row_for_every_area_of_the_new_workspaces():
    """Every area the two entries carve out of their workspace is in DESIGN.md's Workspace contract table, which says
    who writes it first."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = design.index("## Workspace contract")
    table = design[at:design.index("\n## ", at + 5)]
    source = open(os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "fuzzy.hip")).read()
    areas = re.findall(r"(?:plan\.|\*\s*)(\w+)\s*=\s*A\.take", source)
    assert sorted(areas) == ["best_slots", "length_start", "needle_cps", "needle_len", "needle_rank", "row_of", "sorted_cps",
                             "sorted_len", "sorted_of", "unknown_of"]
    assert source.count("A.take") == len(areas) + 2                  # (+ the size query of thr_query_terms_fuzzy)
    for name in areas:
        assert re.search(rf"\|\s*`{name}`", table), f"DESIGN.md, Workspace contract: no row for `{name}`"


# --------------------------------------------------------------------------- the edit distance
def _recursive(a: str, b: str) -> int:
    """Levenshtein's recurrence as it is written down, memoised: independent of the two-row programme."""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (a[i - 1] != b[j - 1]))
    return d(len(a), len(b))


def test_levenshtein_against_the_recurrence_and_written_out_pairs():
    r = random.Random(5)
    for _ in range(4000):
        a = "".join(r.choice("abcd") for _ in range(r.randint(0, 9)))
        b = "".join(r.choice("abcd") for _ in range(r.randint(0, 9)))
        assert IT.levenshtein(a, b) == _recursive(a, b) == IT.levenshtein(b, a), (a, b)
    for a, b, want in (("", "", 0), ("", "abc", 3), ("abc", "", 3), ("kitten", "sitting", 3), ("flaw", "lawn", 2),
                       ("contrtao", "contrato", 2), ("locacao", "locação", 2), ("saturday", "sunday", 3),
                       ("abc", "abc", 0), ("abc", "acb", 2), ("中文", "中文字", 1), ("ação", "acao", 2), ("a", "b", 1),
                       ("intention", "execution", 5), ("gumbo", "gambol", 2)):
        assert IT.levenshtein(a, b) == want, (a, b)
    assert [IT.fuzzy_edits(n, 2) for n in (0, 2, 3, 5, 6, 32, 40)] == [0, 0, 1, 1, 2, 2, 2]
    assert [IT.fuzzy_edits(n, 1) for n in (2, 3, 5, 6, 32)] == [0, 1, 1, 1, 1]


# --------------------------------------------------------------------------- the cases
CASES = FC.all_cases()


def test_each_case_has_the_property_it_is_named_for():
    assert len({c.name for c in CASES}) == len(CASES) >= 20
    for c in CASES:
        assert c.holds(), c.name
        for x, a in zip(c.needles, c.answers()):
            assert len(a) <= c.n_best and a == sorted(a, key=lambda e: (e[0], -min(c.df[e[1]], 2 ** 31 - 1) if c.df else 0, e[1]))
    S = FC.S
    assert S == N.FUZZY_SLICE_BYTES
    ends = {}
    for c in CASES:
        if c.name.startswith("edge_"):
            at = sum(len(t.encode()) for t in c.vocab[:-1])
            ends[c.name] = at
    assert [ends[n] for n in ("edge_ends_at_S_minus_1", "edge_ends_at_S", "edge_ends_at_S_plus_1")] == [S - 1, S, S + 1]
    assert ends["edge_crossed_by_the_longest_key"] - 102 == S - 1


def test_a_wrong_variant_changes_a_named_case():
    by = {c.name: c for c in CASES}
    m = by["multibyte"]
    wrong = m.keys_found(nearest=FC.nearest_wrong("bytes"))
    assert wrong["locacao"] == [] and m.want["locacao"] == ["locação"]           # four byte edits, two code points
    o = by["order_higher_df_wins"]
    assert o.keys_found(nearest=FC.nearest_wrong("df_ascending"))["caxa"] == ["casa", "cara", "cama"] != o.want["caxa"]
    t = by["thresholds_two_edits"]
    wrong = t.keys_found(nearest=FC.nearest_wrong("no_length_rule"))
    assert wrong["abxdy"] == ["abcd", "abcde"] and t.want["abxdy"] == []
    assert wrong["ax"] == ["ab", "abc"] and t.want["ax"] == []                    # (two code points: no edits at all)
    # the variants are the definition where the rule does not bite
    e = by["edit_kinds"]
    assert e.keys_found(nearest=FC.nearest_wrong("bytes")) == e.want
    assert e.keys_found(nearest=FC.nearest_wrong("df_ascending")) == e.want


def test_the_query_rows_of_the_cases():
    places, many = FC.query_cases()
    U, M, C = N.THR_TEXT_UNKNOWN, N.THR_TEXT_TOO_MANY, N.TEXT_CORRECTED
    v = {t: i for i, t in enumerate(places.vocab)}
    OR = dict(zip(places.texts, places.rows(False)))
    AND = dict(zip(places.texts, places.rows(True)))
    assert OR["contrato de locacao"] == ([v["contrato"], v["de"], v["locação"]], 3, C)
    assert OR["documento contratx casa"] == ([v["documento"], v["contrato"], v["contrata"], v["casa"]], 4, C)
    assert AND["documento contratx casa"] == ([v["documento"], v["contrato"], v["casa"]], 3, C)      # the best one alone
    assert OR["contrata contratx"] == ([v["contrata"], v["contrato"]], 2, C)                          # no duplicate
    assert OR["contratx contrata"] == ([v["contrato"], v["contrata"]], 2, C)
    assert OR["caxa CAXA caxa"] == ([v["cama"], v["cara"]], 2, C) and AND["caxa CAXA caxa"] == ([v["cama"]], 1, C)
    assert OR["qqqqqq casa"] == ([v["casa"]], 1, U) and OR["qqqqqq caxa"][2] == U | C
    assert OR["casa cama"] == ([v["casa"], v["cama"]], 2, 0) and OR[""] == ([], 0, 0)
    for conj in (False, True):
        rows = many.rows(conj)
        assert [r[1] for r in rows] == [32, 33, 32, 33, 33]
        assert [r[2] for r in rows] == [C, C | M, C, C | M, C | M]
        assert rows[0][0] == list(range(32)) == rows[1][0] == rows[4][0]
    # with nothing to correct it is host_query_row
    ids = {t: i for i, t in enumerate(places.vocab)}
    for text in ("casa cama de", "qq casa", ""):
        toks = IT.tokenize(text)
        assert IT.host_query_row_fuzzy(toks, ids, places.vocab, places.df, 2, 2, False) == IT.host_query_row(toks, ids)


# --------------------------------------------------------------------------- refusals by name
def test_fuzzy_refuses_by_name():
    assert (Fuzzy().max_edits, Fuzzy().n_best) == (2, 2) and Fuzzy(1, 4) == Fuzzy(max_edits=1, n_best=4)
    assert repr(Fuzzy(1, 3)) == "Fuzzy(max_edits=1, n_best=3)"
    for bad in (0, 3, -1, 1.0, True, None, "2"):
        with pytest.raises(ValueError, match="Fuzzy: max_edits .* outside 1 .. 2"):
            Fuzzy(max_edits=bad)
    for bad in (0, 5, 2.0, False, None):
        with pytest.raises(ValueError, match=r"Fuzzy: n_best .* outside 1 .. THR_FUZZY_MAX_BEST \(4\)"):
            Fuzzy(n_best=bad)
    idx = object.__new__(T.GpuIndex)
    for call in (lambda: idx.query_terms(["a"], fuzzy=Fuzzy()), lambda: idx.nearest_terms(["abc"])):
        with pytest.raises(N.NativeError, match="the index has no vocabulary"):
            call()
    idx.text = {}
    with pytest.raises(ValueError, match="query_terms: fuzzy is an index_text.Fuzzy or None, not int"):
        idx.query_terms(["a"], fuzzy=2)
    with pytest.raises(ValueError, match="nearest_terms: fuzzy is an index_text.Fuzzy or None, not dict"):
        idx.nearest_terms(["abc"], fuzzy={})
    with pytest.raises(N.NativeError, match="max_edits 3 outside 1 .. 2"):
        N.fuzzy_check("x", 3, 2)
    with pytest.raises(N.NativeError, match=r"n_best 5 outside 1 .. THR_FUZZY_MAX_BEST \(4\)"):
        N.fuzzy_check("x", 2, 5)


def test_the_clients_refuse_by_name():
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    from triple_hybrid_rag_amd.sharded_client import ShardedIndexClient
    with pytest.raises(ValueError, match="fuzzy= needs device_text=True"):
        GpuIndexClient(None, None, fuzzy=Fuzzy())
    with pytest.raises(ValueError, match="GpuIndexClient: fuzzy is an index_text.Fuzzy or None, not bool"):
        GpuIndexClient(None, None, device_text=True, fuzzy=True)
    with pytest.raises(N.NativeError, match="fuzzy= is not supported through a sharded index client: .* per shard"):
        ShardedIndexClient(None, None, fuzzy=Fuzzy())
    sh = object.__new__(ShardedIndex)
    with pytest.raises(N.NativeError, match=r"fuzzy= is not supported through ShardedIndex.query_terms"):
        sh.query_terms(["a"], fuzzy=Fuzzy())
    with pytest.raises(N.NativeError, match=r"fuzzy= is not supported through ShardedIndex.nearest_terms"):
        sh.nearest_terms(["abc"])


# --------------------------------------------------------------------------- fuzzy=None is the parent's route
class StubLibrary:
    """Stands in for the loaded library: records the entry points called, answers 0 (a size query: 64)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("thr_"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append(name)
            return 64 if name.endswith("_workspace_bytes") else 0
        return entry


def _host_index(monkeypatch, vocab):
    torch = pytest.importorskip("torch")
    lib = StubLibrary()
    monkeypatch.setattr(N, "load", lambda build_if_missing=True: lib)
    monkeypatch.setattr(N, "_dev", lambda t, dtype, name, ndim=None: 0 if t is None else t.data_ptr())   # (host tensors)
    monkeypatch.setattr(N, "_stream", lambda: 0)
    idx = object.__new__(T.GpuIndex)
    idx.__dict__.update(device=torch.device("cpu"), lex=None)
    idx.set_vocabulary(vocab)
    return idx, lib


# what the parent commit's query_terms enqueues: the workspace sizes are asked by the wrapper and by the binding
PARENT_CALLS = ["thr_text_tokens_workspace_bytes", "thr_text_tokens_workspace_bytes", "thr_text_tokens",
                "thr_query_terms_workspace_bytes", "thr_query_terms_workspace_bytes", "thr_query_terms"]
FUZZY_CALLS = ["thr_text_tokens_workspace_bytes", "thr_text_tokens_workspace_bytes", "thr_text_tokens",
               "thr_vocab_nearest_workspace_bytes", "thr_vocab_nearest_workspace_bytes", "thr_vocab_nearest",
               "thr_query_terms_fuzzy_workspace_bytes", "thr_query_terms_fuzzy_workspace_bytes", "thr_query_terms_fuzzy"]


def test_without_fuzzy_query_terms_and_the_client_make_exactly_the_parents_native_calls(monkeypatch):
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.store import CorpusStore
    vocab = ["contrato", "casa"]
    idx, lib = _host_index(monkeypatch, vocab)
    assert lib.calls == ["thr_vocab_insert"]
    for conj in (False, True):
        lib.calls.clear()
        idx.query_terms(["contrato casa", "contrtao"], conjunctive=conj)
        assert lib.calls == PARENT_CALLS
        lib.calls.clear()
        idx.query_terms(["contrato casa", "contrtao"], conjunctive=conj, fuzzy=None)
        assert lib.calls == PARENT_CALLS
        lib.calls.clear()
        idx.query_terms(["contrato casa", "contrtao"], conjunctive=conj, fuzzy=Fuzzy())
        assert lib.calls == FUZZY_CALLS
    for fuzzy, want in ((None, PARENT_CALLS), (Fuzzy(1, 1), FUZZY_CALLS)):
        client = GpuIndexClient.__new__(GpuIndexClient)
        client.store = CorpusStore([], [], [], [], [], [], vocab={t: i for i, t in enumerate(vocab)})
        client.index, client.lexical_and, client.device_text, client.fuzzy = idx, True, True, fuzzy
        client.tokenizer = IT.tokenize
        lib.calls.clear()
        client.query_terms_batch(["contrtao casa"])
        assert lib.calls == want
    lib.calls.clear()
    idx.nearest_terms(["contrtao"])
    assert lib.calls == FUZZY_CALLS[3:6]
    lib.calls.clear()
    assert idx.nearest_terms([])[0].shape == (0, 2) and lib.calls == []


# --------------------------------------------------------------------------- the entries' argument checks
def test_argument_checks_refuse_before_any_launch():
    lib = N.load()
    p = 4096
    ok = dict(text_bytes=p + 1, n_bytes=100, table=2 * p, unknown_off=3 * p, unknown_len=4 * p, n_unknown=5 * p,
              unknown_capacity=50, term_bytes=6 * p + 1, term_ptr=7 * p, n_vocab=512, n_term_bytes=4000, term_rowptr=8 * p,
              max_edits=2, n_best=4, near_term=9 * p, near_dist=10 * p, workspace=11 * p, workspace_bytes=0, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.thr_vocab_nearest(*[a[k] for k in ok])
    assert call() == WORKSPACE and call(term_rowptr=None) == WORKSPACE and call(n_vocab=0) == WORKSPACE
    assert call(n_bytes=-1) == UNSUPPORTED and call(n_bytes=N.THR_TEXT_MAX_BYTES + 1) == UNSUPPORTED
    assert call(unknown_capacity=0) == UNSUPPORTED and call(unknown_capacity=N.THR_TEXT_MAX_BYTES + 1) == UNSUPPORTED
    assert call(n_vocab=1 << 31) == UNSUPPORTED and call(n_term_bytes=(1 << 43) + 1) == UNSUPPORTED
    for name in ("text_bytes", "table", "unknown_off", "unknown_len", "n_unknown", "term_bytes", "term_ptr", "near_term",
                 "near_dist", "workspace"):
        assert call(**{name: None}) == INVALID, name
    assert call(n_vocab=-1) == INVALID and call(n_term_bytes=-1) == INVALID
    assert [call(max_edits=m) for m in (0, 1, 2, 3)] == [INVALID, WORKSPACE, WORKSPACE, INVALID]
    assert [call(n_best=b) for b in (0, 1, 4, 5)] == [INVALID, WORKSPACE, WORKSPACE, INVALID]
    for name, off in (("unknown_off", 4), ("term_ptr", 4), ("term_rowptr", 4), ("table", 2), ("unknown_len", 2), ("n_unknown", 2),
                      ("near_term", 2), ("near_dist", 2)):
        assert call(**{name: ok[name] + off}) == INVALID, name
    assert call(workspace=11 * p + 8, workspace_bytes=1 << 20) == INVALID
    need = lib.thr_vocab_nearest_workspace_bytes(100, 50, 512, 4000, 4)
    assert need == N.vocab_nearest_workspace_bytes(100, 50, 512, 4000, 4) > 0 and call(workspace_bytes=need - 1) == WORKSPACE
    assert lib.thr_vocab_nearest_workspace_bytes(100, 0, 512, 4000, 4) == 0 == lib.thr_vocab_nearest_workspace_bytes(100, 50, 512, 4000, 5)

    qok = dict(tok_term=p, n_tokens=2 * p, text_flags=3 * p, n_total=4 * p, token_capacity=52, n_queries=3, near_term=5 * p,
               near_capacity=52, n_best=3, n_use=2, out_terms=6 * p, n_distinct=7 * p, out_flags=8 * p, workspace=9 * p,
               workspace_bytes=0, stream=None)

    def qcall(**kw):
        a = dict(qok, **kw)
        return lib.thr_query_terms_fuzzy(*[a[k] for k in qok])
    assert qcall() == WORKSPACE
    assert qcall(n_queries=0) == UNSUPPORTED and qcall(n_queries=N.THR_TEXT_MAX_TEXTS + 1) == UNSUPPORTED
    assert qcall(token_capacity=0) == UNSUPPORTED
    for name in ("tok_term", "n_tokens", "text_flags", "n_total", "near_term", "out_terms", "n_distinct", "out_flags", "workspace"):
        assert qcall(**{name: None}) == INVALID, name
    assert qcall(near_capacity=0) == INVALID and qcall(n_best=0) == INVALID and qcall(n_best=5, n_use=1) == INVALID
    assert [qcall(n_use=u) for u in (0, 1, 3, 4)] == [INVALID, WORKSPACE, WORKSPACE, INVALID]
    assert qcall(workspace=9 * p + 2, workspace_bytes=1 << 20) == INVALID
    need = lib.thr_query_terms_fuzzy_workspace_bytes(3)
    assert need == N.query_terms_fuzzy_workspace_bytes(3) > 0 and qcall(workspace_bytes=need - 1) == WORKSPACE
    assert lib.thr_query_terms_fuzzy_workspace_bytes(0) == 0


def test_argument_checks_under_sanitizers(tmp_path):
    """The same checks in a stand-alone program (its own main), the host side of csrc/fuzzy.hip compiled with
    ASan + UBSan: run as a program on the CPU, never loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the library itself could not have been built")
    exe = str(tmp_path / "fuzzy_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "fuzzy.hip"),
                    os.path.join(ROOT, "tests", "native", "fuzzy_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "fuzzy host check: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def test_the_binding_refuses_shapes_before_any_pointer_is_taken(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(N, "_dev", lambda t, dtype, name, ndim=None: 0 if t is None else t.data_ptr())   # (host tensors)
    args = dict(text_bytes=torch.zeros(32, dtype=torch.uint8), n_bytes=16, table=torch.zeros(65536, dtype=torch.int32),
                unknown_off=torch.zeros(4, dtype=torch.int64), unknown_len=torch.zeros(4, dtype=torch.int32),
                n_unknown=torch.zeros(1, dtype=torch.int32), term_bytes=torch.zeros(32, dtype=torch.uint8),
                term_ptr=torch.zeros(3, dtype=torch.int64), n_term_bytes=10)
    with pytest.raises(N.NativeError, match="vocab_nearest: max_edits 0 outside"):
        N.vocab_nearest(**args, max_edits=0)
    with pytest.raises(N.NativeError, match="40 text bytes, the array holds 32"):
        N.vocab_nearest(**dict(args, n_bytes=40))
    with pytest.raises(N.NativeError, match="33 key bytes, the array holds 32"):
        N.vocab_nearest(**dict(args, n_term_bytes=33))
    with pytest.raises(N.NativeError, match="term_rowptr holds 2 entries for 2 terms"):
        N.vocab_nearest(**args, term_rowptr=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(N.NativeError, match=r"near_term is int32 \[4, 2\]"):
        N.vocab_nearest(**args, near_term=torch.zeros((4, 3), dtype=torch.int32))
    rows = dict(n_tokens=torch.zeros(2, dtype=torch.int32), term=torch.zeros(4, dtype=torch.int32))
    with pytest.raises(N.NativeError, match=r"n_use 3 outside 1 .. n_best \(2\)"):
        N.query_terms_fuzzy(rows, torch.zeros((4, 2), dtype=torch.int32), 3)
