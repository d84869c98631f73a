"""CPU-side checks of the C-ABI library: it builds, loads and exports every symbol
include/thr_hip.h declares (no compute calls without a GPU)."""
import os
import re

import pytest

import triple_hybrid_rag_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(thr_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    T._build.build_native()
    lib = T._native.load()
    names = declared_symbols()
    assert len(names) >= 15
    for name in names:
        assert hasattr(lib, name), f"{name} declared in thr_hip.h but not exported"
    assert sorted(T._native.EXPORTED_SYMBOLS) == names
    assert lib.thr_abi_version() == T._native.ABI_VERSION == 9
    assert lib.thr_error_string(-3) == b"workspace too small"


def test_host_side_argument_checks_do_not_need_a_gpu():
    lib = T._native.load()
    # null pointers / bad sizes are rejected before any launch
    assert lib.thr_dense_topk(None, None, None, 10, 768, 0, None, 1, 10, 128, None, None, None, None,
                              None, None, None, 0, None) == -1
    # bm25: a vocabulary size is part of the call (term ids >= V are ignored, not dereferenced)
    assert lib.thr_bm25_topk(None, None, None, None, None, None, None, None, None, None, None, 0, 1.0, 1.2, 0.75,
                             10, 5, 0, None, 1, 4, 10, 0, None, None, None, None, None, None, 0, None) == -1
    # dense-term rows: one window of zero padding behind the shard's docs, 16-byte aligned
    assert lib.thr_bm25_dense_stride(1000) == 1008 + 65536 and lib.thr_bm25_dense_stride(0) == 0
    assert lib.thr_bm25_dense_rows(None, None, None, None, None, 1, 10, 5, None, None, None) == -1
    # the work decomposition's item list, slice edges and per-slice lists: grows with nq, terms, k
    assert lib.thr_bm25_workspace_bytes(2048, 4, 50) > (2048 + 8192) * 50 * 16
    assert lib.thr_bm25_workspace_bytes(2048, 32, 50) > lib.thr_bm25_workspace_bytes(2048, 4, 50)
    assert lib.thr_bm25_workspace_bytes(0, 4, 50) == 0
    assert lib.thr_bm25_block_count(129) == 2 and lib.thr_bm25_block_count(0) == 0
    assert lib.thr_graph_workspace_bytes(2, 1000) == 2 * 8192 * 8 + 64 * 1024
    assert lib.thr_dense_workspace_bytes(1_000_000, 768, 1024, 128) > 2 ** 20
    assert lib.thr_maxsim(None, 1, 32, None, 1, 128, 128, None, 1, None, 0, None) == -1
    assert lib.thr_rrf_fuse(None, 0, None, 0, None, 0, 1, 0.7, 0.8, 1.0, 60, 10, None, None, None,
                            None, None) == -1


def test_bm25_batch_limit_and_workspace_growth_are_host_arithmetic():
    """One thr_bm25_topk call takes at most THR_BM25_MAX_QUERIES queries: a larger batch is
    refused on the host, before any pointer is looked at and before anything is launched (the
    library without the limit answered these null pointers with THR_ERR_INVALID).  Below it the
    item list has one wave slot per query on top of the tuned 16384 -- what lets the plan
    kernel's fit loop end for every batch -- and the workspace grows as the header documents."""
    import pytest
    N = T._native
    lib = N.load()
    limit = N.THR_BM25_MAX_QUERIES
    header = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    assert re.search(r"#define\s+THR_BM25_MAX_QUERIES\s+\(1 << 20\)", header) and limit == 1 << 20

    def call(nq):
        return lib.thr_bm25_topk(None, None, None, None, None, None, None, None, None, None, None, 0, 1.0, 1.2,
                                 0.75, 10, 5, 0, None, nq, 4, 10, 0, None, None, None, None, None, None, 0, None)
    assert call(limit + 1) == -2 and call(2 ** 31 - 1) == -2       # THR_ERR_UNSUPPORTED
    assert call(limit) == -1 and call(20000) == -1                  # (null pointers: THR_ERR_INVALID)
    assert lib.thr_error_string(-2) == b"unsupported shape"
    assert lib.thr_bm25_workspace_bytes(limit + 1, 4, 10) == 0
    assert lib.thr_bm25_workspace_bytes(limit, 32, 128) > 0
    with pytest.raises(N.NativeError, match=str(limit)):
        N.bm25_check_batch(limit + 1)
    N.bm25_check_batch(limit)
    # monotonic in n_queries across the waves' tuned 16384 slots, and linear with the documented
    # slope: 48 + 4 mt bytes per query, three item slots of 368 + 8 mt + 16 k bytes per query
    # (each of the 20 arrays is rounded up to 256 bytes)
    for mt, k in ((4, 10), (8, 50), (32, 128)):
        sizes = [lib.thr_bm25_workspace_bytes(nq, mt, k) for nq in (1, 2048, 16383, 16384, 16385, 20000, 65537, limit)]
        assert all(a < b for a, b in zip(sizes, sizes[1:]))
        per_query = 48 + 4 * mt + 3 * (368 + 8 * mt + 16 * k)
        for lo, hi in ((2048, 16384), (16384, 16385), (16384, 40000), (40000, limit)):
            grow = lib.thr_bm25_workspace_bytes(hi, mt, k) - lib.thr_bm25_workspace_bytes(lo, mt, k)
            assert abs(grow - (hi - lo) * per_query) <= 20 * 256, (mt, k, lo, hi, grow)
        # ... of which the waves' slot per query is this change's
        assert lib.thr_bm25_workspace_bytes(2048, mt, k) >= (3 * 2048 + 32768) * (368 + 8 * mt + 16 * k)


def test_host_side_planning_functions():
    """Sizes and the query-tile choice are pure host arithmetic (no launch)."""
    N = T._native
    N.load()
    # f16 copy scan: 32 queries per wave (their B operands live in registers), 8 waves per block;
    # at dim 1024 4 waves (one per SIMD) of 48 queries -- 384 B-operand registers each
    assert N.dense_f16_query_tile(768, True, 1024) == 256
    assert N.dense_f16_query_tile(512, True, 1536) == 256
    assert N.dense_f16_query_tile(1024, True, 1536) == 192
    assert N.dense_f16_query_tile(768, False, 1536) == 64     # in-flight rounding: transpose tiles
    assert N.dense_f16_query_tile(1024, False, 1536) == 32
    assert N.dense_f16_query_tile(640, True, 64) == 0         # no f16 kernel at that dim
    # the copy scan's candidate-segment offsets are 32 bits: 131072 bytes per query, whole tiles
    assert N.dense_f16_max_queries(768, True) == 32512 and N.dense_f16_max_queries(1024, True) == 32640
    assert N.dense_f16_max_queries(768, True) * 131072 < 2 ** 32
    assert N.dense_f16_max_queries(768, False) == 2 ** 31 - 1
    lib = N.load()
    assert lib.thr_dense_f16_copy_bytes(33, 768) == 64 * 768 * 2   # rows padded to tiles of 32
    assert lib.thr_dense_rescue_workspace_bytes(1024, 100) == 1024 * 64 * 100 * 16
    assert lib.thr_dense_f16_workspace_bytes(1_000_000, 768, 1536, 192) >= \
        lib.thr_dense_f16_workspace_bytes(1_000_000, 768, 1024, 192)
    # the threshold sample grows with the corpus (n * 64 / 4096 rows, one float per query and
    # row): a capped sample would let tens of thousands of rows per query through on a 10M-row
    # shard and overflow every candidate list
    grow = lib.thr_dense_f16_workspace_bytes(10_000_000, 768, 1536, 192) - \
        lib.thr_dense_f16_workspace_bytes(1_000_000, 768, 1536, 192)
    assert abs(grow - 1536 * (10_000_000 - 1_000_000) * 64 // 4096 * 4) < 64 * 1536 * 4 + 4096


def test_no_cpu_fallback_in_the_product_package():
    """The product path must not import the oracle or fall back to CPU math."""
    pkg = os.path.join(ROOT, "triple-hybrid-rag_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


# ----------------------------------------------------------- the binding against the header
def header_text():
    """include/thr_hip.h without comments and preprocessor lines (#define lines are kept apart)."""
    text = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    lines = text.split("\n")
    defines = [ln for ln in lines if ln.lstrip().startswith("#")]
    return "\n".join(ln for ln in lines if not ln.lstrip().startswith("#")), defines


def ctype_class(ct):
    """What the comparison knows of a ctypes type: a pointer, or (float?, bytes, signed?) of a scalar
    -- by size and signedness, not by name (c_size_t IS c_uint64 here, c_int64 is c_long)."""
    import ctypes as C
    if ct is None:
        return "void"
    if issubclass(ct, C._Pointer) or ct._type_ in "Pz":
        return "pointer"
    return (ct._type_ in "fdg", C.sizeof(ct), ct._type_ not in "fdg" and ct(-1).value < 0)


def header_class(ctype: str):
    """The class of one C type of the header (the issue's table: pointers and thr_stream_t are
    pointers; int, int64_t, uint64_t, size_t and double by their size and signedness)."""
    import ctypes as C
    words = [w for w in re.sub(r"\*", " * ", ctype).split() if w != "const"]
    if "*" in words or words == ["thr_stream_t"]:
        return "pointer"
    scalar = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
              "double": C.c_double}
    assert len(words) == 1 and words[0] in scalar, f"thr_hip.h uses a type this test does not know: {ctype!r}"
    return ctype_class(scalar[words[0]])


def header_prototypes():
    """{name: (result class, [parameter classes])} of every thr_* function thr_hip.h declares."""
    text, _ = header_text()
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(thr_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text):
        res, name, params = m.group(1), m.group(2), m.group(3).strip()
        res = " ".join(w for w in res.split() if w != "extern")
        args = []
        if params != "void":
            for p in params.split(","):
                p = p.strip()
                ctype = re.sub(r"[A-Za-z_]\w*$", "", p) if re.search(r"[\s\*][A-Za-z_]\w*$", p) else p   # drop the name
                args.append(header_class(ctype))
        protos[name] = (header_class(res), args)
    return protos


def test_signatures_agree_with_the_header():
    """Every entry of _SIGNATURES has the header's result type and, argument by argument, the
    header's parameter classes: an argtypes list that gains or loses one entry (every later argument
    of that call shifts by one) fails here, on the CPU.  (Tried by hand once: with one _vp taken
    from thr_dense_rescue's list and with one added to thr_rrf_fuse's, this test fails naming the
    symbol.)"""
    N = T._native
    protos = header_prototypes()
    assert sorted(protos) == declared_symbols() == sorted(N._SIGNATURES) and len(protos) == 65
    for name, (res, args) in N._SIGNATURES.items():
        want_res, want_args = protos[name]
        assert ctype_class(res) == want_res, f"{name}: result type differs from thr_hip.h"
        got = [ctype_class(a) for a in args]
        assert len(got) == len(want_args), f"{name}: {len(got)} argtypes, thr_hip.h declares {len(want_args)} parameters"
        for i, (g, w) in enumerate(zip(got, want_args)):
            assert g == w, f"{name}: argument {i} is {args[i].__name__}, thr_hip.h wants {w}"


# THR_* names of _native that thr_hip.h does not #define, each with its reason (none today)
NOT_IN_HEADER = {}


def test_constants_agree_with_the_header():
    N = T._native
    _, defines = header_text()
    header = {}
    for ln in defines:
        m = re.match(r"\s*#\s*define\s+(THR_[A-Z0-9_]+)\s+(\S.*)$", ln)
        if m:
            expr = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]*\b", r"\1", m.group(2).strip())
            assert re.fullmatch(r"[0-9a-fA-FxX<>()|+*\s-]+", expr), f"{m.group(1)}: cannot evaluate {m.group(2)!r}"
            header[m.group(1)] = eval(expr, {"__builtins__": {}})
    assert header["THR_ABI_VERSION"] == N.ABI_VERSION
    assert header["THR_BM25_MAX_QUERIES"] == 1 << 20 and header["THR_TEXT_MAX_BYTES"] == 0x7FFFFFFF and \
        header["THR_FLAG_CERTIFIED"] == 1                       # the three forms are evaluated
    mine = {k: v for k, v in vars(N).items() if k.startswith("THR_") and isinstance(v, int)}
    assert len(mine) >= 30
    for name, value in mine.items():
        if name in NOT_IN_HEADER:
            assert name not in header, f"{name} is in thr_hip.h now: drop it from NOT_IN_HEADER"
            continue
        assert name in header, f"_native.{name} is not a #define of thr_hip.h (list it in NOT_IN_HEADER with the reason, or remove it)"
        assert value == header[name], f"_native.{name} = {value}, thr_hip.h says {header[name]}"


# ----------------------------------------------------------- twins and accessors, library stubbed
class RecordingLibrary:
    """Stands in for libthr_hip.so: every thr_* attribute is a function that records its call."""

    def __init__(self, result=0):
        self.calls, self.result = [], result

    def __getattr__(self, name):
        if not name.startswith("thr_"):
            raise AttributeError(name)
        return lambda *args: (self.calls.append((name, args)), self.result)[1]


def test_rrf_twins_reach_their_own_entry_with_the_same_arguments(monkeypatch):
    """rrf_fuse and rrf_fuse_standalone share one body: each still calls its own entry point with
    the argument tuple it passed when it had a body of its own -- three (pointer, width) pairs, nq,
    the three weights, its own scalar (rrf_k / the two_channels flag), top_k, the four outputs
    (a null ranks pointer unless asked for) and the stream."""
    torch = pytest.importorskip("torch")
    N = T._native
    lib = RecordingLibrary()
    monkeypatch.setattr(N, "load", lambda build_if_missing=True: lib)
    monkeypatch.setattr(N, "_dev", lambda t, dtype, name, ndim=None: 0 if t is None else t.data_ptr())   # (host tensors)
    monkeypatch.setattr(N, "_stream", lambda: 77)
    lex = torch.zeros((3, 5), dtype=torch.int64)
    sem = torch.zeros((3, 7), dtype=torch.int64)

    def outputs(a, ranks):
        assert all(isinstance(p, int) and p for p in a[12:14] + a[15:16]) and (a[14] != 0) == ranks and a[16] == 77
    head = (lex.data_ptr(), 5, sem.data_ptr(), 7, 0, 0, 3)
    ids, sc, rk, cnt = N.rrf_fuse(lex, sem, None, 4, rrf_k=61)
    (name, a), = lib.calls
    assert name == "thr_rrf_fuse" and a[:12] == head + (0.7, 0.8, 1.0, 61, 4) and len(a) == 17
    outputs(a, False)
    assert rk is None and (ids.shape, sc.shape, cnt.shape) == ((3, 4), (3, 4), (3,))
    assert a[12:16] == (ids.data_ptr(), sc.data_ptr(), 0, cnt.data_ptr())
    lib.calls.clear()
    ids, sc, rk, cnt = N.rrf_fuse_standalone(lex, sem, None, 6, w_lex=0.5, two_channels=True)
    (name, a), = lib.calls
    assert name == "thr_rrf_fuse_standalone" and a[:12] == head + (0.5, 0.8, 1.0, 1, 6) and len(a) == 17
    outputs(a, True)
    assert a[12:16] == (ids.data_ptr(), sc.data_ptr(), rk.data_ptr(), cnt.data_ptr()) and rk.shape == (3, 6, 3)
    lib.calls.clear()
    N.rrf_fuse_standalone(None, sem, None, 2, want_ranks=False)
    (name, a), = lib.calls
    assert name == "thr_rrf_fuse_standalone" and a[:12] == (0, 0, sem.data_ptr(), 7, 0, 0, 3, 0.7, 0.8, 1.0, 0, 2)
    outputs(a, False)
    lib.calls.clear()
    N.rrf_fuse(lex, None, None, 3, want_ranks=True)
    (name, a), = lib.calls
    assert name == "thr_rrf_fuse" and a[:12] == (lex.data_ptr(), 5, 0, 0, 0, 0, 3, 0.7, 0.8, 1.0, 60, 3)
    outputs(a, True)
    for fuse, what in ((N.rrf_fuse, "rrf_fuse:"), (N.rrf_fuse_standalone, "rrf_fuse_standalone:")):
        with pytest.raises(N.NativeError, match=what + ".*512"):
            fuse(lex, sem, None, 513)
    lib.result = -1                                              # a failing call is reported under its own name
    monkeypatch.setattr(lib, "thr_error_string", lambda rc: b"invalid argument", raising=False)
    with pytest.raises(N.NativeError, match="thr_rrf_fuse_standalone failed"):
        N.rrf_fuse_standalone(lex, sem, None, 2)


def test_workspace_size_accessors_forward_their_arguments(monkeypatch):
    N = T._native
    lib = RecordingLibrary(result=4096)
    monkeypatch.setattr(N, "load", lambda build_if_missing=True: lib)
    for accessor, args in ((N.entity_match_workspace_bytes, (1000, 7, 3)), (N.text_tokens_workspace_bytes, (5, 300, 152)),
                           (N.query_terms_workspace_bytes, (9,)), (N.vocab_grow_workspace_bytes, (31,)),
                           (N.bm25_workspace_bytes, (2048, 4, 50))):
        lib.calls.clear()
        got = accessor(*args)
        assert type(got) is int and got == 4096
        assert lib.calls == [("thr_" + accessor.__name__, args)]
    # ... and no file of the package reaches around them: thr_* entry points are called in _native alone
    pkg = os.path.join(ROOT, "triple-hybrid-rag_amd")
    for f in sorted(os.listdir(pkg)):
        if f.endswith(".py") and f != "_native.py":
            assert not re.search(r"\.thr_[a-z0-9_]+\(", open(os.path.join(pkg, f)).read()), f


# ----------------------------------------------------------- every entry with a workspace takes the caller's
def workspace_takers():
    """The thr_* entry points whose prototype in thr_hip.h has ``void *workspace, size_t workspace_bytes``."""
    text, _ = header_text()
    out = []
    for m in re.finditer(r"\b(thr_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text):
        params = " ".join(m.group(2).split())
        if re.search(r"void \*\s*workspace, size_t workspace_bytes", params):
            out.append(m.group(1))
    return sorted(out)


def test_every_binding_of_an_entry_with_a_workspace_has_a_workspace_parameter():
    """thr_hip.h gives 22 entry points a workspace; the binding of each (same name without thr_) takes
    ``workspace``: none allocates behind the caller's back without a way to hand one in."""
    import inspect
    N = T._native
    takers = workspace_takers()
    assert len(takers) == 22 and "thr_dense_topk_exact" in takers and "thr_csr_compact" in takers
    for entry in takers:
        fn = getattr(N, entry[4:], None)
        assert fn is not None, f"_native has no binding named {entry[4:]}"
        assert "workspace" in inspect.signature(fn).parameters, f"_native.{entry[4:]} takes no workspace"


class SizedLibrary(RecordingLibrary):
    """RecordingLibrary whose size functions answer 4096 bytes."""

    def __getattr__(self, name):
        if name.endswith("_workspace_bytes"):
            return lambda *args: 4096
        return super().__getattr__(name)


def test_the_six_bindings_that_allocated_inside_hand_the_callers_workspace_through(monkeypatch):
    """dense_topk_exact, dense_topk_rows, scope_resolve, scope_resolve_clauses, lexical_build and csr_compact:
    with ``workspace`` of at least the size function's bytes the library gets that pointer and its byte count
    (the last two arguments in front of the stream, as the header orders them); a smaller one or None is
    replaced by a fresh allocation of the size -- the behaviour before, and _workspace's rule for every call."""
    torch = pytest.importorskip("torch")
    np = pytest.importorskip("numpy")
    N = T._native
    lib = SizedLibrary()
    monkeypatch.setattr(N, "load", lambda build_if_missing=True: lib)
    monkeypatch.setattr(N, "_dev", lambda t, dtype, name, ndim=None: 0 if t is None else t.data_ptr())   # (host tensors)
    monkeypatch.setattr(N, "_stream", lambda: 77)
    f32, f64, i32, i64 = torch.float32, torch.float64, torch.int32, torch.int64
    docs, dn, q = torch.zeros((6, 8), dtype=f32), torch.ones(6, dtype=f64), torch.zeros((2, 8), dtype=f32)
    cols = [torch.zeros(6, dtype=i32)]
    calls = {
        "thr_dense_topk_exact": lambda ws: N.dense_topk_exact(docs, dn, q, 3, workspace=ws),
        "thr_dense_topk_rows": lambda ws: N.dense_topk_rows(docs, dn, q, 3, torch.zeros(2, dtype=i64), torch.zeros(4, dtype=i32),
                                                            torch.zeros(2, dtype=i32), workspace=ws),
        "thr_scope_resolve": lambda ws: N.scope_resolve(cols, torch.zeros((2, 1), dtype=i32), workspace=ws),
        "thr_scope_resolve_clauses": lambda ws: N.scope_resolve_clauses(cols, np.zeros((2, 1, 4), dtype=np.int32), workspace=ws),
        "thr_lexical_build": lambda ws: N.lexical_build(torch.zeros(5, dtype=i32), torch.zeros(5, dtype=i32), None, 6, 4,
                                                        workspace=ws),
        "thr_csr_compact": lambda ws: N.csr_compact(torch.zeros(3, dtype=i64), torch.zeros(5, dtype=i32), None,
                                                    torch.zeros(4, dtype=i32), workspace=ws),
    }
    assert sorted(calls) == sorted(set(calls) & set(workspace_takers()))
    for entry, call in calls.items():
        for ws, mine in ((torch.empty(4096 + 512, dtype=torch.uint8), True), (torch.empty(1024, dtype=torch.int32), True),
                         (torch.empty(4095, dtype=torch.uint8), False), (None, False)):
            lib.calls.clear()
            call(ws)
            (name, a), = [c for c in lib.calls if not c[0].endswith("_workspace_bytes")]
            assert name == entry and a[-1] == 77
            if mine:
                assert a[-3:-1] == (ws.data_ptr(), ws.numel() * ws.element_size()), f"{entry}: the caller's workspace did not arrive"
            else:
                assert a[-2] == 4096 and a[-3] != 0 and (ws is None or a[-3] != ws.data_ptr()), \
                    f"{entry}: a workspace that is too small (or none) is replaced by one of the size function's bytes"
