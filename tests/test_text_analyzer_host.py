"""No GPU: the token-level analysis (index_text.Analyzer: a stop list and suffix stemming).  The new header
against its binding table, the definition's refusals by name, the compiled rule table byte for byte, longest
match and step order, the empty analyzer against its table, exceptional texts, the shipped Portuguese example
against its written-out pairs, from_rows on the host route, and thr_text_tokens_analyzed's argument checks
(through the library and in a stand-alone sanitized program)."""
import os
import random
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import text_analyzer_cases as AC  # noqa: E402
import text_cases as TC  # noqa: E402
import triple_hybrid_rag_amd as T  # noqa: E402
from test_native_abi import ctype_class, declared_symbols, header_class  # noqa: E402
from triple_hybrid_rag_amd import _native as N  # noqa: E402
from triple_hybrid_rag_amd import backend  # noqa: E402
from triple_hybrid_rag_amd import index_build as IB  # noqa: E402
from triple_hybrid_rag_amd import index_text as IT  # noqa: E402
from triple_hybrid_rag_amd.index_text import Analyzer, TextTable, fold_accents  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thr_hip_text.h")
INVALID, UNSUPPORTED, WORKSPACE = -1, -2, -3


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
    assert sorted(protos) == sorted(N._SIGNATURES_TEXT) == ["thr_text_tokens_analyzed", "thr_text_tokens_analyzed_workspace_bytes"]
    for name, (res, args) in N._SIGNATURES_TEXT.items():
        want_res, want_args = protos[name]
        assert ctype_class(res) == want_res, name
        got = [ctype_class(a) for a in args]
        assert len(got) == len(want_args), f"{name}: {len(got)} argtypes, the header declares {len(want_args)} parameters"
        for i, (g, w) in enumerate(zip(got, want_args)):
            assert g == w, f"{name}: argument {i}"
    lib = N.load()
    for name in protos:
        assert hasattr(lib, name)
    # everything thr_text_tokens takes, in its order, around the eight analysis operands
    base = N._SIGNATURES["thr_text_tokens"][1]
    mine = N._SIGNATURES_TEXT["thr_text_tokens_analyzed"][1]
    assert mine[:10] == base[:10] and mine[18:] == base[10:] and len(mine) == len(base) + 8
    _, defines = _header_text()
    header = {m.group(1): int(m.group(2)) for m in (re.match(r"\s*#\s*define\s+(THR_[A-Z0-9_]+)\s+(\d+)\s*$", ln) for ln in defines) if m}
    assert header == {"THR_STEM_MAX_SUFFIX": N.STEM_MAX_SUFFIX, "THR_STEM_MAX_STEPS": N.STEM_MAX_STEPS,
                      "THR_STEM_MAX_RULES": N.STEM_MAX_RULES, "THR_STEM_RULE_BYTES": N.STEM_RULE_BYTES}
    assert (N.STEM_MAX_SUFFIX, N.STEM_MAX_STEPS, N.STEM_MAX_RULES, N.STEM_RULE_BYTES) == (8, 4, 1024, 24)
    assert '#include "thr_hip.h"' in open(HEADER).read()
    # additive: thr_hip.h keeps its prototypes and the ABI version
    assert len(declared_symbols()) == len(N.EXPORTED_SYMBOLS) == 65 and N.ABI_VERSION == 9
    assert not set(N._SIGNATURES_TEXT) & (set(N.EXPORTED_SYMBOLS) | set(N._SIGNATURES_GRAPH))
    assert "analyzed" not in open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    import inspect
    assert "workspace" in inspect.signature(N.text_tokens_analyzed).parameters
    assert T.Analyzer is Analyzer


# --------------------------------------------------------------------------- the definition's refusals
def test_construction_refuses_by_name():
    ok = Analyzer(stop=["de"], steps=[[("s", 1)]])
    assert ok.tokenize("casas de campo") == ["casa", "campo"]
    for stop, what in ((["De"], "not a fixed point"), (["a b"], "not a fixed point"), ([""], "not a fixed point"),
                       (["İstanbul"], "exceptional"), (["\U0001F600"], "exceptional")):
        with pytest.raises(ValueError, match="stop word.*" + what):
            Analyzer(stop=stop)
    with pytest.raises(ValueError, match="suffix of step 0.*not a fixed point"):
        Analyzer(steps=[[("S", 1)]])
    with pytest.raises(ValueError, match="suffix of step 1.*exceptional"):
        Analyzer(steps=[[("s", 1)], [("İ", 1)]])
    with pytest.raises(ValueError, match="empty suffix"):
        Analyzer(steps=[[("", 1)]])
    with pytest.raises(ValueError, match="THR_STEM_MAX_SUFFIX"):
        Analyzer(steps=[[("abcdefghi", 1)]])
    Analyzer(steps=[[("abcdefgh", 1)]])
    with pytest.raises(ValueError, match="min_stem 0.*below 1"):
        Analyzer(steps=[[("s", 0)]])
    with pytest.raises(ValueError, match="'s' occurs twice in step 0"):
        Analyzer(steps=[[("s", 1), ("es", 1), ("s", 2)]])
    Analyzer(steps=[[("s", 1)], [("s", 2)]])                         # (the same suffix in two steps is fine)
    with pytest.raises(ValueError, match="5 steps.*THR_STEM_MAX_STEPS"):
        Analyzer(steps=[[("s", 1)]] * 5)
    many = [(f"{i:04d}", 1) for i in range(1025)]
    with pytest.raises(ValueError, match="1025 rules.*THR_STEM_MAX_RULES"):
        Analyzer(steps=[many[:600], many[600:]])
    Analyzer(steps=[many[:600], many[600:1024]])
    # a folded table: an accented suffix is no fixed point of it
    fold = TextTable.from_char_map(fold_accents)
    with pytest.raises(ValueError, match="'ção'.*not a fixed point"):
        Analyzer(fold, steps=[[("ção", 1)]])
    assert Analyzer(fold, steps=[[("cao", 2)]]).tokenize("Locação") == ["loca"]


def test_compiled_rule_table_byte_for_byte():
    a = Analyzer(steps=[[("s", 3), ("ões", 2), ("es", 4)], [], [("中文", 1)]])
    step_ptr, rules = a.rule_table()
    want = b"".join([
        struct.pack("<8Hii", ord("s"), ord("e"), 0xF5, 0, 0, 0, 0, 0, 3, 2),          # longest first: ões
        struct.pack("<8Hii", ord("s"), ord("e"), 0, 0, 0, 0, 0, 0, 2, 4),
        struct.pack("<8Hii", ord("s"), 0, 0, 0, 0, 0, 0, 0, 1, 3),
        struct.pack("<8Hii", 0x6587, 0x4E2D, 0, 0, 0, 0, 0, 0, 2, 1)])
    assert step_ptr == [0, 3, 3, 4] and rules.dtype == np.uint8 and rules.tobytes() == want
    assert len(want) == 4 * N.STEM_RULE_BYTES
    # the cases' own writer, in the order given, is the same layout
    p2, r2 = AC.rule_table([[("ões", 2), ("es", 4), ("s", 3)], [], [("中文", 1)]])
    assert p2 == step_ptr and r2.tobytes() == want
    assert Analyzer().rule_table()[0] == [0] and Analyzer().rule_table()[1].size == 0


def test_longest_match_and_step_order_change_named_cases():
    a = Analyzer(steps=[AC.PLURAL])
    assert [a.stem(w) for w in ("locações", "flores", "casas")] == ["locaç", "flor", "casa"]
    shortest = AC.first_match_tokens(TextTable.default(), (), [sorted(AC.PLURAL, key=lambda r: len(r[0]))], "locações flores")
    assert shortest == ["locaçõe", "flore"]                          # the wrong variant: shortest match
    two = Analyzer(steps=[[("s", 3)], [("mente", 3)]])
    swapped = Analyzer(steps=[[("mente", 3)], [("s", 3)]])
    assert two.stem("claramentes") == "clara" and swapped.stem("claramentes") == "claramente"
    assert two.stem("mentes") == "mente" and two.stem("as") == "as"                 # min_stem holds
    # the stop check is on the whole lowered token BEFORE stemming: a stem that equals a stop word stays
    s = Analyzer(stop=["com", "comer"], steps=[[("eu", 3), ("er", 3)]])
    assert s.tokenize("Comer comeu COM correr") == ["com", "corr"]


def test_the_restatement_of_the_cases_equals_the_analyzer():
    cases = AC.all_cases()
    assert len({c.name for c in cases}) == len(cases) >= 20
    table = TextTable.default()
    for c in cases:
        assert c.holds(), c.name
        if c.table_order:
            continue
        a = Analyzer(table, c.stop, c.steps)
        for t in c.texts[:200]:
            assert a.tokenize(t) == c.tokens(table)(t), c.name


def test_empty_analyzer_is_its_table_on_random_strings():
    a, table = Analyzer(), TextTable.default()
    assert a.trivial and IT.tokenizer_table(a.tokenize, "x") is table
    r = random.Random(3)
    alphabet = "abcXYZ çÃõÉ ,.-_09 中文 ẞKȺ İΣς\U0001F600\n"
    for _ in range(5000):
        t = "".join(r.choice(alphabet) for _ in range(r.randint(0, 24)))
        assert a.tokenize(t) == table.tokenize(t) and a.is_exceptional(t) == table.is_exceptional(t)
    assert a.entries is table.entries and a.exceptional_among(["a", "İ", "b"]) == [1]


def test_exceptional_texts_are_answered_with_stop_words_and_stems_applied():
    a = Analyzer(stop=["de", "σας"], steps=[[("s", 3), ("ς", 2)]])
    for text, want in (("İstanbul de casas", backend.tokenize("İstanbul") + ["casa"]), ("ΟΔΟΣ de ΣΑΣ casas", ["οδο", "casa"]),
                       ("casas \U0001F600 de x\U0001D400bs", ["casa", "x\U0001D400b"])):
        assert a.is_exceptional(text)
        assert a.tokenize(text) == want, text
        assert a.tokenize(text) == AC.restated_tokens(TextTable.default(), {"de", "σας"}, a.steps, text)


def test_tokenizer_table_takes_an_analyzers_tokenize_and_refuses_the_rest_with_todays_message():
    a = Analyzer.portuguese()
    assert IT.tokenizer_table(a.tokenize, "x") is a

    def foreign(text):
        return text.split()
    for fn, name in ((foreign, "foreign"), (a.stem, "Analyzer.stem"), (a.restate, "Analyzer.restate")):
        with pytest.raises(ValueError) as err:
            IT.tokenizer_table(fn, "device_text=True")
        assert str(err.value).startswith("device_text=True needs backend.tokenize or a TextTable's .tokenize") and name in str(err.value)


# --------------------------------------------------------------------------- the shipped example
def test_portuguese_conflates_and_keeps_apart_its_written_out_pairs_and_drops_its_stop_words():
    a = Analyzer.portuguese()
    same, apart = AC.pairs(AC.PT_SAME), AC.pairs(AC.PT_APART)
    assert len(set(same)) >= 40 and len(set(apart)) >= 20
    for x, y in same:
        assert a.stem(x) == a.stem(y), (x, y, a.stem(x), a.stem(y))
        assert a.tokenize(x.upper()) == a.tokenize(y) == [a.stem(x)]
    for x, y in apart:
        assert a.stem(x) != a.stem(y), (x, y, a.stem(x))
    assert a.stem("documentos") == "document" and a.stem("locações") == a.stem("locação") == "locaç"
    assert len(a.stop) > 150 and all(a.tokenize(w) == [] and a.tokenize(w.upper() + ".") == [] for w in a.stop)
    for w in ("de", "a", "o", "que", "não", "pelos", "àquela", "está", "têm", "houve"):
        assert w in a.stop
    assert a.tokenize("Os documentos da locação não foram assinados pelos clientes.") == ["document", "locaç", "assin", "client"]
    assert 2 <= len(a.steps) <= 3 and "Snowball" in Analyzer.portuguese.__doc__ and "own" in Analyzer.portuguese.__doc__.lower()
    f = Analyzer.portuguese(fold=True)
    assert f.tokenize("As LOCAÇÕES da locacao") == ["locac", "locac"] and f.tokenize("NÃO nao") == []


# --------------------------------------------------------------------------- the host route
def test_from_rows_with_the_analyzers_tokenizer_builds_the_expected_postings():
    a = Analyzer.portuguese()
    texts = ["Os documentos da locação", "O documento foi assinado", "Locações de casas", "A casa do cliente",
             "de a o que", "", "Clientes falaram do contrato", "Falar não é assinar", "Contratos e documentos", "casinha nova"]
    hi = IB.from_rows([{"id": f"c{i}", "parent_id": "p", "document_id": "d", "text": t} for i, t in enumerate(texts)],
                      tokenizer=a.tokenize)
    vocab = hi.store.vocab
    assert list(vocab) == ["document", "locaç", "assin", "cas", "client", "fal", "contrat", "nov"]

    def postings(stem):
        t = vocab[stem]
        return hi.post_doc[hi.rowptr[t]:hi.rowptr[t + 1]].tolist()
    assert postings("document") == [0, 1, 8] and postings("locaç") == [0, 2] and postings("cas") == [2, 3, 9]
    assert postings("fal") == [6, 7] and postings("assin") == [1, 7]
    assert hi.doclen.tolist() == [2, 2, 2, 2, 0, 0, 3, 2, 2, 2]            # stop words do not count
    client = backend.GpuIndexClient(None, hi.store, tokenizer=a.tokenize)
    assert client._query_terms("os documentos das locações") == [vocab["document"], vocab["locaç"]]


# --------------------------------------------------------------------------- the entry's argument checks
def test_argument_checks_refuse_before_any_launch():
    import ctypes as C
    lib = N.load()
    p = 4096
    steps = (C.c_int32 * 3)(0, 3, 10)
    ok = dict(text_bytes=p, text_ptr=2 * p, n_texts=3, n_bytes=100, table=3 * p, slots=4 * p, capacity=1024, term_bytes=5 * p + 1,
              term_ptr=6 * p, n_vocab=512, stop_slots=16 * p, stop_capacity=64, stop_bytes=17 * p + 1, stop_ptr=18 * p, n_stop=20,
              h_step_ptr=C.cast(steps, C.c_void_p), n_steps=2, rules=19 * p, token_capacity=52, tok_doc=7 * p, tok_term=8 * p,
              n_tokens=9 * p, flags=10 * p, n_total=11 * p, unknown_off=12 * p, unknown_len=13 * p, n_unknown=14 * p,
              workspace=15 * p, workspace_bytes=0, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.thr_text_tokens_analyzed(*[a[k] for k in ok])

    def host(*v):
        return C.cast((C.c_int32 * len(v))(*v), C.c_void_p)
    assert call() == WORKSPACE
    assert call(n_texts=0) == UNSUPPORTED and call(n_bytes=-1) == UNSUPPORTED and call(token_capacity=0) == UNSUPPORTED
    for name in ("text_bytes", "text_ptr", "table", "slots", "term_bytes", "term_ptr", "tok_doc", "tok_term", "n_tokens", "flags",
                 "n_total", "unknown_off", "unknown_len", "n_unknown", "workspace", "stop_slots", "stop_bytes", "stop_ptr",
                 "h_step_ptr", "rules"):
        assert call(**{name: None}) == INVALID, name
    assert call(n_steps=-1) == INVALID and call(n_steps=5) == INVALID
    assert call(n_steps=0, h_step_ptr=None, rules=None) == WORKSPACE
    for bad in (host(1, 3, 10), host(0, 5, 4), host(0, 3, 1025), host(0, -1, 4)):
        assert call(h_step_ptr=bad) == INVALID
    assert call(h_step_ptr=host(0, 0, 1000, 1000, 1024), n_steps=4) == WORKSPACE
    assert call(h_step_ptr=host(0, 0, 0), rules=None) == WORKSPACE
    assert call(rules=19 * p + 4) == INVALID
    none = dict(stop_capacity=0, stop_slots=None, stop_bytes=None, stop_ptr=None, n_stop=0)
    assert call(**none) == WORKSPACE
    assert call(stop_capacity=0) == INVALID and call(**dict(none, n_stop=1)) == INVALID
    assert call(stop_capacity=60) == INVALID and call(stop_capacity=8, n_stop=2) == INVALID
    assert call(n_stop=33) == INVALID and call(n_stop=-1) == INVALID and call(n_stop=32) == WORKSPACE
    assert call(stop_slots=16 * p + 8) == INVALID and call(stop_ptr=18 * p + 4) == INVALID
    need = lib.thr_text_tokens_analyzed_workspace_bytes(3, 100, 52)
    assert need == lib.thr_text_tokens_workspace_bytes(3, 100, 52) == N.text_tokens_analyzed_workspace_bytes(3, 100, 52)
    assert call(workspace_bytes=need - 1) == WORKSPACE and lib.thr_text_tokens_analyzed_workspace_bytes(0, 100, 52) == 0


def test_argument_checks_under_sanitizers(tmp_path):
    """The same checks in a stand-alone program (its own main), the host side of csrc/text.hip compiled with
    ASan + UBSan: run as a program on the CPU, never loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the library itself could not have been built")
    exe = str(tmp_path / "text_analyzer_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "text.hip"),
                    os.path.join(ROOT, "tests", "native", "text_analyzer_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "text analyzer host check: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def test_the_binding_refuses_shapes_before_any_pointer_is_taken(monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(N, "_dev", lambda t, dtype, name, ndim=None: 0 if t is None else t.data_ptr())   # (host tensors)
    z = torch.zeros(4, dtype=torch.int64)
    base = (torch.zeros(32, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64), 4, torch.zeros(65536, dtype=torch.int32),
            torch.zeros((16, 2), dtype=torch.int64), torch.zeros(16, dtype=torch.uint8), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(N.NativeError, match="slots, bytes and pointers, or none"):
        N.text_tokens_analyzed(*base, stop_slots=torch.zeros((16, 2), dtype=torch.int64))
    with pytest.raises(N.NativeError, match="0 .. 4 steps"):
        N.text_tokens_analyzed(*base, step_ptr=[0, 0, 0, 0, 0, 0])
    with pytest.raises(N.NativeError, match="ascends from 0"):
        N.text_tokens_analyzed(*base, step_ptr=[0, 2, 1], rules=torch.zeros(48, dtype=torch.uint8))
    with pytest.raises(N.NativeError, match="2 rules of 24 bytes, the array holds 47"):
        N.text_tokens_analyzed(*base, step_ptr=[0, 2], rules=torch.zeros(47, dtype=torch.uint8))
    assert z.numel() == 4
