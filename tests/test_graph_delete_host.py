"""No GPU: graph delete.  The new header against its binding table, thr_csr_prune's refusals (through the
library and in a stand-alone sanitized program), the numpy restatement pinned to index_build.build_graph,
the built cases' properties, delete_graph's refusals, the store's entity columns and the table surface."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import graph_delete_cases as GD  # noqa: E402
import graph_ingest_cases as GC  # noqa: E402
import triple_hybrid_rag_amd as T  # noqa: E402
from test_native_abi import ctype_class, declared_symbols, header_class  # noqa: E402
from triple_hybrid_rag_amd import _native as N  # noqa: E402
from triple_hybrid_rag_amd import index_build as IB  # noqa: E402
from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient  # noqa: E402
from triple_hybrid_rag_amd.index import GpuIndex  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thr_hip_graph.h")
INVALID, WORKSPACE = -1, -3


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
        if params != "void":
            for p in params.split(","):
                p = p.strip()
                args.append(header_class(re.sub(r"[A-Za-z_]\w*$", "", p) if re.search(r"[\s\*][A-Za-z_]\w*$", p) else p))
        protos[name] = (header_class(res), args)
    return protos


def test_the_new_header_and_the_second_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(N._SIGNATURES_GRAPH) == ["thr_csr_prune", "thr_csr_prune_slice", "thr_csr_prune_workspace_bytes"]
    for name, (res, args) in N._SIGNATURES_GRAPH.items():
        want_res, want_args = protos[name]
        assert ctype_class(res) == want_res, name
        got = [ctype_class(a) for a in args]
        assert len(got) == len(want_args), f"{name}: {len(got)} argtypes, the header declares {len(want_args)} parameters"
        for i, (g, w) in enumerate(zip(got, want_args)):
            assert g == w, f"{name}: argument {i}"
    lib = N.load()
    for name in protos:
        assert hasattr(lib, name)
    # the constants: bound under names that do not start with THR_, equal to the header's #defines
    _, defines = _header_text()
    header = {m.group(1): int(m.group(2)) for m in (re.match(r"\s*#\s*define\s+(THR_[A-Z0-9_]+)\s+(\d+)\s*$", ln) for ln in defines) if m}
    assert header == {"THR_CSR_PRUNE_SLICE": N.CSR_PRUNE_SLICE, "THR_CSR_PRUNE_UNSORTED_B": N.CSR_PRUNE_UNSORTED_B,
                      "THR_CSR_PRUNE_OVERFLOW": N.CSR_PRUNE_OVERFLOW, "THR_CSR_PRUNE_BAD_ROW": N.CSR_PRUNE_BAD_ROW}
    assert lib.thr_csr_prune_slice() == N.CSR_PRUNE_SLICE == GD.S
    assert (GD.UNSORTED_B, GD.OVERFLOW, GD.BAD_ROW) == (N.CSR_PRUNE_UNSORTED_B, N.CSR_PRUNE_OVERFLOW, N.CSR_PRUNE_BAD_ROW)
    assert '#include "thr_hip.h"' in open(HEADER).read()


def test_thr_hip_h_and_the_exported_symbols_are_unchanged_in_count():
    assert len(declared_symbols()) == len(N.EXPORTED_SYMBOLS) == 65 and N.ABI_VERSION == 9
    assert not set(N._SIGNATURES_GRAPH) & set(N.EXPORTED_SYMBOLS)
    assert "csr_prune" not in open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    import inspect
    assert "workspace" in inspect.signature(N.csr_prune).parameters and callable(N.csr_prune_workspace_bytes)


def test_csr_prune_checks_its_arguments_on_the_host():
    lib = N.load()
    p = 4096
    ok = dict(rowptr_a=p, rows_a=6, nnz_a=8, ids_a=2 * p, pay_a=3 * p, row_remap=4 * p, rows_out=4, id_remap=5 * p, n_ids=6,
              id_base=0, rowptr_b=6 * p, nnz_b=3, ids_b=7 * p, rowptr_out=8 * p, ids_out=9 * p, pay_out=10 * p, cap=8,
              keep=11 * p, nnz_out=12 * p, status=13 * p, ws=14 * p, ws_bytes=0, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.thr_csr_prune(*[a[k] for k in ok])
    assert call() == WORKSPACE                                     # everything else passed
    for name in ("rowptr_out", "nnz_out", "status", "rowptr_a", "ids_a", "ids_out", "id_remap", "ids_b", "rowptr_b"):
        assert call(**{name: None}) == INVALID, name                # null pointers with non-zero sizes
    assert call(rowptr_b=None, nnz_b=0) == INVALID                  # B given without rowptr_b
    for name in ("rows_a", "nnz_a", "nnz_b", "n_ids", "id_base", "rows_out", "cap"):
        assert call(**{name: -1}) == INVALID, name                  # negative sizes
    assert call(rows_out=7) == INVALID and call(row_remap=None) == INVALID
    assert call(row_remap=None, rows_out=6) == WORKSPACE
    assert call(pay_a=None) == INVALID and call(pay_out=None) == INVALID      # a payload on one side only
    assert call(pay_a=None, pay_out=None) == WORKSPACE
    assert call(id_remap=None, n_ids=0) == WORKSPACE and call(rowptr_b=None, ids_b=None, nnz_b=0) == WORKSPACE
    assert call(keep=None) == WORKSPACE
    for dst, src in (("rowptr_out", "rowptr_a"), ("rowptr_out", "rowptr_b"), ("ids_out", "ids_a"), ("ids_out", "ids_b"),
                     ("ids_out", "row_remap"), ("ids_out", "id_remap"), ("pay_out", "pay_a"), ("pay_out", "ids_out"),
                     ("keep", "ids_a"), ("keep", "ids_out")):
        assert call(**{dst: ok[src]}) == INVALID, (dst, src)        # a destination that is one of the sources
    assert call(rows_a=0, rows_out=0) == INVALID                    # entries without rows
    assert call(rows_a=0, rows_out=0, nnz_a=0, nnz_b=0, rowptr_a=None, ids_a=None) == WORKSPACE    # an empty A is valid
    assert call(ws_bytes=1 << 20, ws=None) == INVALID
    need = lib.thr_csr_prune_workspace_bytes(6, 8)
    assert need == 4 * 256 and call(ws_bytes=need - 1) == WORKSPACE
    assert lib.thr_csr_prune_workspace_bytes(0, 0) == 256 and lib.thr_csr_prune_workspace_bytes(10, GD.S + 1) == 256 + 4352 + 256 + 256
    assert lib.thr_csr_prune_workspace_bytes(-1, 0) == 0 and lib.thr_csr_prune_workspace_bytes(1, -1) == 0
    assert N.csr_prune_workspace_bytes(6, 8) == need


def test_host_checks_are_clean_under_address_and_ub_sanitizer(tmp_path):
    """The entry's argument checks and its workspace-size function, compiled together with a stand-alone
    program (its own main) with the host side under ASan + UBSan, run on the CPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "csr_prune_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "csr_prune.hip"),
                    os.path.join(ROOT, "tests", "native", "csr_prune_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "csr_prune host check: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


def test_native_wrapper_refuses_shapes_before_any_pointer_is_taken():
    import torch
    rp, ids = torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    remap = torch.zeros(2, dtype=torch.int32)
    E = T.NativeError
    with pytest.raises(E, match="row_remap needs rows_out"):
        N.csr_prune(rp, ids, row_remap=remap)
    with pytest.raises(E, match="one entry per row"):
        N.csr_prune(rp, ids, row_remap=torch.zeros(3, dtype=torch.int32), rows_out=2)
    with pytest.raises(E, match="rows_out differs"):
        N.csr_prune(rp, ids, rows_out=1)
    with pytest.raises(E, match="rows_out is 3"):
        N.csr_prune(rp, ids, row_remap=remap, rows_out=3)
    with pytest.raises(E, match="4-byte"):
        N.csr_prune(rp, ids, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(E, match="pay_out without a payload"):
        N.csr_prune(rp, ids, pay_out=torch.zeros(2))
    with pytest.raises(E, match="row pointers and ids, or neither"):
        N.csr_prune(rp, ids, ids_b=ids)
    with pytest.raises(E, match="one entry per row of A and one more"):
        N.csr_prune(rp, ids, rowptr_b=torch.zeros(2, dtype=torch.int64), ids_b=ids)
    with pytest.raises(E, match="CUDA"):
        N.csr_prune(rp, ids)
    assert N.csr_prune_status_message(0) is None and "strictly ascending" in N.csr_prune_status_message(1)
    assert "out_capacity" in N.csr_prune_status_message(2) and "rows_out" in N.csr_prune_status_message(4)


# --------------------------------------------------------------------------- the restatement and the cases
def _rows(seed, n_chunks=60, n_ent=30):
    ents, rels, mens = GC.graph_rows(seed, n_chunks, n_ent, 90, 200)
    return ents, rels, mens, {f"c{i}": 1000 + i for i in range(n_chunks)}


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
@pytest.mark.parametrize("kinds", ["entities", "relations", "mentions", "all"])
def test_the_restatement_of_a_delete_is_the_fresh_build_over_the_surviving_rows(seed, kinds):
    """build_graph(surviving rows) == csr_prune_ref applied as delete_graph applies thr_csr_prune, array for
    array, for random rows and random deletions of every kind: the restatement may stand as the reference."""
    ents, rels, mens, cidx = _rows(seed)
    de, dr, dm = GD.graph_deletions(seed + 50, len(ents), rels, mens, 60)
    de, dr, dm = (de if kinds in ("entities", "all") else None, dr if kinds in ("relations", "all") else None,
                  dm if kinds in ("mentions", "all") else None)
    graph = IB.build_graph([e["id"] for e in ents], rels, mens, cidx)
    got, remap = GD.delete_graph_ref(graph, 60, 1000, de, dr, dm)
    e2, r2, m2 = GD.surviving_rows(ents, rels, mens, () if de is None else de, dr, dm)
    fresh = IB.build_graph([e["id"] for e in e2], r2, m2, cidx)
    assert (len(r2) < len(rels)) == (kinds != "mentions") and (len(m2) < len(mens)) == (kinds != "relations")
    for name, a, b in zip(("ent_rowptr", "ent_col", "men_rowptr", "men_chunk", "men_conf"), got, fresh):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, kinds, seed)
    keep = np.ones(len(ents), dtype=bool)
    if de is not None:
        keep[de] = False
    assert np.array_equal(remap[keep], np.arange(len(e2))) and (remap[~keep] == -1).all()


def test_the_restatement_is_sensitive_to_its_rules():
    C = GD.cases()
    c = C["multiset"]
    e = GD.expected(c)
    lo, hi = c.span("multi")
    assert list(c.ids_a[lo:hi]).count(7) == 5 and e["keep"][lo:hi].tolist() == [0, 1, 0, 1, 0, 1, 0, 1, 0, 1]
    assert e["pay"][:5].tolist() == [2, 4, 6, 8, 10]                          # each kept copy carries its own payload
    c = C["b_under_removed"]
    assert GD.expected(c)["status"] == 0 and GD.expected(c)["nnz"] == 5       # the unsorted B row lies under a removed row
    flat = GD.csr_prune_ref(c.rowptr_a, c.ids_a, c.pay_a, None, 4, None, 0, c.rowptr_b, c.ids_b)
    assert flat["status"] == GD.UNSORTED_B                                    # ... with every row alive it counts
    c = C["b_absent"]
    assert GD.expected(c)["nnz"] == len(c.ids_a) - 1                          # only (between, 30) names an entry


def test_every_case_has_the_property_it_is_named_for():
    C, S = GD.cases(), GD.S
    c = C["slice_edges"]
    assert [c.span(n)[1] - c.span(n)[0] for n in ("s_minus_1", "s", "s_plus_1")] == [S - 1, S, S + 1]
    for n in ("s_minus_1", "s", "s_plus_1", "straddles"):
        lo, hi = c.span(n)
        assert lo // S != (hi - 1) // S, n                                    # the row straddles a slice edge
    assert c.span("s")[1] == 2 * S + 4 and c.row_remap[c.rows["removed"]] == -1
    c = C["star"]
    assert c.span("star")[1] - c.span("star")[0] == 3 * S + 5
    c = C["empty_runs"]
    lens = np.diff(c.rowptr_a)
    assert (lens[:1000] == 0).all() and (lens[-1000:] == 0).all() and (lens[1002:2002] == 0).all() and len(lens) == 3003
    assert (c.row_remap == -1).sum() == 4 and c.rows_out == 2999
    c = C["first_last_removed"]
    assert c.row_remap[0] == -1 and c.row_remap[-1] == -1 and (c.row_remap[1:-1] >= 0).all()
    c = C["slice_emptied"]
    keep = GD.expected(c)["keep"]
    assert len(keep) > 2 * S and not keep[S:2 * S].any() and keep[:S].all() and keep[2 * S:].all()
    c = C["nothing_dropped"]
    e = GD.expected(c)
    assert len(c.ids_b) > 0 and e["keep"].all() and np.array_equal(e["ids"], c.ids_a) and np.array_equal(e["rowptr"], c.rowptr_a)
    c = C["b_absent"]
    assert not np.isin(c.row(c.rows["below"]), c.ids_b[c.rowptr_b[0]:c.rowptr_b[1]]).any() and len(c.row(c.rows["empty_a"])) == 0
    c = C["b_under_removed"]
    t = c.rows["removed_unsorted_b"]
    assert c.row_remap[t] == -1 and np.any(np.diff(c.ids_b[c.rowptr_b[t]:c.rowptr_b[t + 1]]) <= 0)
    for base in (0, 700):
        w, wo = C[f"ids_outside_with_remap_base_{base}"], C[f"ids_outside_without_remap_base_{base}"]
        assert w.id_base == wo.id_base == base and wo.id_remap is None and np.array_equal(w.ids_a, wo.ids_a)
        i = w.ids_a.astype(np.int64) - base
        assert ((i < 0) | (i >= len(w.id_remap))).sum() >= 4
        outside = (i < 0) | (i >= len(w.id_remap))
        assert not GD.expected(w)["keep"][outside].any() and GD.expected(wo)["keep"][outside].all()
        assert np.array_equal(GD.expected(wo)["ids"], wo.ids_a[GD.expected(wo)["keep"] == 1])      # passed through
    c = C["overflow"]
    assert c.short == 1 and GD.capacity(c) == GD.expected(c)["nnz"] - 1 and GD.expected(c)["status"] == GD.OVERFLOW
    assert C["unsorted_b"].status == GD.expected(C["unsorted_b"])["status"] == GD.UNSORTED_B
    assert C["repeated_b"].status == GD.expected(C["repeated_b"])["status"] == GD.UNSORTED_B
    assert len(C["nnz_zero"].ids_a) == 0 and len(C["nnz_zero"].rowptr_a) == 4 and C["nnz_zero"].rows_out == 2
    assert len(C["rows_zero"].rowptr_a) == 1 and C["rows_zero"].rows_out == 0
    assert C["no_remaps"].row_remap is None and C["no_remaps"].id_remap is None
    c = C["random_70000"]
    e = GD.expected(c)
    assert 65_000 <= len(c.ids_a) <= 80_000 and (c.row_remap == -1).sum() > 100 and np.array_equal(c.row_remap, c.id_remap)
    by_row = e["keep"][c.row_remap[GD.row_of_positions(c.rowptr_a)] >= 0]
    assert 0 < (by_row == 0).sum() and len(c.ids_b) > 1000                    # all three kinds remove something
    for c in C.values():
        if c.status == 0:
            assert GD.expected(c)["status"] == (GD.OVERFLOW if c.short else 0), c.name


# --------------------------------------------------------------------------- delete_graph's refusals
class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def _bare_index(**attrs):
    idx = object.__new__(GpuIndex)
    base = dict(docs=None, dim=0, n_docs=100, lex=None, doc_coll=None, tokens=None, graph=None, entities=None,
                _lex_global=False)
    base.update(attrs)
    idx.__dict__.update(base)
    return idx


def test_delete_graph_refuses_before_any_device_work():
    E = T.NativeError
    with pytest.raises(E, match="delete_graph: this index has no graph channel"):
        _bare_index().delete_graph(entities=[0])
    idx = _bare_index(graph={"men_rowptr": _Shape(11), "ent_rowptr": _Shape(11)})
    for bad in ([10], [-1], [3, 11]):
        with pytest.raises(ValueError, match=r"entity ids are 0 \.\. 9"):
            idx.delete_graph(entities=np.array(bad))
    with pytest.raises(ValueError, match=r"relation endpoints are entity ids, 0 \.\. 9"):
        idx.delete_graph(relations=(np.array([0]), np.array([10])))
    with pytest.raises(ValueError, match=r"relation endpoints"):
        idx.delete_graph(relations=(np.array([-1]), np.array([1])))
    with pytest.raises(ValueError, match=r"chunk ids are local doc ids, 0 \.\. 99"):
        idx.delete_graph(mentions=(np.array([0]), np.array([100])))
    with pytest.raises(ValueError, match=r"entity ids are 0 \.\. 9"):
        idx.delete_graph(mentions=(np.array([-2]), np.array([5])))
    with pytest.raises(ValueError, match="names nothing"):
        idx.delete_graph(mentions=(np.array([-1]), np.array([-1])))
    for part in ("relations", "mentions"):
        with pytest.raises(E, match="one length"):
            idx.delete_graph(**{part: (np.array([1, 2]), np.array([1]))})
        with pytest.raises(E, match="pair of id arrays"):
            idx.delete_graph(**{part: (np.array([1]),)})
    with pytest.raises(E, match="integer"):
        idx.delete_graph(entities=np.array([0.5]))
    with pytest.raises(E, match="every entity would be deleted: build a new index"):
        idx.delete_graph(entities=np.array(list(range(10)) + [3, 3]))
    with pytest.raises(E, match="unusable"):
        _bare_index(graph=idx.graph, _unusable="this index is unusable: test").delete_graph(entities=[0])


def test_sharded_classes_refuse_graph_deletes():
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    from triple_hybrid_rag_amd.sharded_client import ShardedIndexClient
    for call in (ShardedIndex.delete_graph, ShardedIndexClient._delete_entities_where,
                 ShardedIndexClient._delete_relations_where, ShardedIndexClient._delete_mentions_where):
        with pytest.raises(T.NativeError, match="not supported"):
            call(object(), [])
    with pytest.raises(T.NativeError, match="graph_cascade is not supported"):
        ShardedIndexClient(object(), _store(), graph_cascade=True)


@pytest.mark.parametrize("names,gone", [
    (["Acme Corp", "zeta", "Beta"], [1]), (["São Paulo", "İstanbul Büyükşehir", "Ünİ", ""], [0, 3]),
    (["", "", "x"], [0]), (["x" * 128, "é" * 64, "k"], [2]), (["a", "b"], [])])
def test_name_store_without_the_removed_names_equals_packing_the_survivors(names, gone):
    """What delete_graph does on the device, in numpy: the kept names' bytes (each with its 0xFF) in order,
    the padding moved to the new end -- byte for byte pack_entity_names(surviving names)."""
    from triple_hybrid_rag_amd.index_entities import pack_entity_names
    blob, ptr = pack_entity_names(names)
    keep = np.ones(len(names), dtype=bool)
    keep[gone] = False
    used = len(blob) - N.THR_ENTITY_MAX_NEEDLE
    lens = np.diff(ptr)
    got = np.concatenate([blob[:used][np.repeat(keep, lens)], blob[used:]])
    want, want_ptr = pack_entity_names([n for n, k in zip(names, keep) if k])
    assert np.array_equal(got, want) and np.array_equal(np.concatenate([[0], np.cumsum(lens[keep])]), want_ptr)


# --------------------------------------------------------------------------- the store
def _store(n=6, entities=("Acme Corp", "Zeta", "Beta"), **kw):
    return CorpusStore(child_ids=[f"c{i}" for i in range(n)], parent_ids=[f"p{i // 2}" for i in range(n)],
                       document_ids=[f"d{i // 3}" for i in range(n)], texts=[f"alpha t{i}" for i in range(n)], pages=[1] * n,
                       modalities=["text"] * n, entity_names=list(entities), **kw)


def test_store_delete_entities_and_the_document_column(tmp_path):
    st = _store(entity_ids=["e0", "e1", "e2"], entity_canonical=["acme", None, "beta"])
    assert st.entity_documents is None
    st.append_entities([{"id": "e3", "name": "Gamma"}])
    assert st.entity_documents is None                                    # None until a row carries one
    st.append_entities([{"id": "e4", "name": "Delta", "document_id": "d1"}, {"id": "e5", "name": "Eps"}])
    assert st.entity_documents == [None, None, None, None, "d1", None]
    assert st.entity_index("e4") == 4 and st.entity_by_canonical("beta") == 2
    gone = st.delete_entities([4, 1, 1])
    assert gone == [{"id": "e1", "name": "Zeta", "canonical_name": "Zeta"}, {"id": "e4", "name": "Delta", "canonical_name": "Delta"}]
    assert st.entity_names == ["Acme Corp", "Beta", "Gamma", "Eps"] and st.entity_ids == ["e0", "e2", "e3", "e5"]
    assert st.entity_canonical == ["acme", "beta", None, None] and st.entity_documents == [None] * 4
    assert st.entity_index("e1") is None and st.entity_index("e2") == 1 and st.entity_by_canonical("beta") == 1
    assert st.delete_entities([]) == []
    with pytest.raises(ValueError, match="out of range"):
        st.delete_entities([4])
    plain = _store()                                                       # no id column: the integer ids stay those entities'
    plain.delete_entities([0])
    assert plain.entity_ids == [1, 2] and plain.entity_index(1) == 0 and plain.entity_index(0) is None
    # from_rows reads the column, save / load carry it, an older directory loads with None
    ents, rels, mens = GC.graph_rows(3, 8, 4, 8, 8)
    ents[1]["document_id"], ents[3]["document_id"] = "d0", "d7"
    hi = IB.from_rows(GC.child_rows(0, 8), entity_rows=ents, relation_rows=rels, mention_rows=mens)
    assert hi.store.entity_documents == [None, "d0", None, "d7"]
    IB.save(hi, str(tmp_path / "with"))
    back = IB.load(str(tmp_path / "with")).store
    assert list(back.entity_documents) == [None, "d0", None, "d7"]
    back.delete_entities([1])
    assert list(back.entity_documents) == [None, None, "d7"]
    assert IB.from_rows(GC.child_rows(0, 8), entity_rows=GC.graph_rows(3, 8, 4, 8, 8)[0]).store.entity_documents is None
    IB.save(IB.HostIndex(docs=np.zeros((6, 4), dtype=np.float32), store=_store()), str(tmp_path / "old"))
    assert not (tmp_path / "old" / "store_entity_documents_blob.npy").exists()
    assert IB.load(str(tmp_path / "old")).store.entity_documents is None


# --------------------------------------------------------------------------- the table surface
class _StubIndex:
    """What the graph deletes need of an index: the channels, host graph rows, delete_rows and delete_graph."""

    def __init__(self, n_docs, n_ent, relations, mentions):
        self.docs, self.dim, self.n_docs = None, 0, n_docs
        self.lex = self.doc_coll = self.tokens = self.entities = None
        self.graph = {"men_rowptr": _Shape(n_ent + 1)}
        self.n_ent, self.relations, self.mentions = n_ent, relations, mentions       # {e: [ids]}, {e: [(chunk, conf)]}
        self.calls, self.store, self._attrs, self.refuse = [], None, {}, False

    def attribute_names(self):
        return sorted(self._attrs)

    def set_attributes(self, columns):
        self._attrs.update(columns)

    def graph_rows_host(self, which, entities=None):
        es = range(self.n_ent) if entities is None else entities
        rows = [self.relations.get(e, []) if which == "relations" else [c for c, _ in self.mentions.get(e, [])] for e in es]
        rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
        ids = np.array([x for r in rows for x in r], dtype=np.int64)
        conf = None if which == "relations" else np.array([w for e in es for _, w in self.mentions.get(e, [])], dtype=np.float32)
        return rp, ids, conf

    def delete_rows(self, ids):
        self.calls.append(("rows", np.asarray(ids).tolist(), len(self.store.child_ids)))
        self.n_docs -= len(ids)

    def delete_graph(self, entities=None, relations=None, mentions=None):
        if self.refuse:
            raise T.NativeError("delete_graph: refused")
        as_lists = lambda p: None if p is None else tuple(np.asarray(a).tolist() for a in p)
        self.calls.append(("graph", None if entities is None else np.asarray(entities).tolist(), as_lists(relations),
                           as_lists(mentions), len(self.store.entity_names)))       # (the store's size AT the call)


def _graph_client(tenants=False, **kw):
    st = _store(entities=("Acme Corp", "Zeta", "Beta", "Quasar"), entity_ids=["e0", "e1", "e2", "e3"],
                entity_canonical=["acme", None, "beta", "quasar"], entity_documents=["d0", "d1", None, "d1"],
                org_ids=["acme"] * 3 + ["bolt"] * 3 if tenants else None)
    idx = _StubIndex(6, 4, {0: [1, 2], 1: [0, 3], 2: [0], 3: [1]},
                     {0: [(0, 0.5), (4, 1.0)], 1: [(1, 0.25), (1, 0.75), (5, 1.0)], 3: [(2, 1.0), (3, 0.125)]})
    idx.store = st
    return GpuIndexClient(idx, st, org_id=None if tenants else "org", **kw), idx, st


def test_entity_table_delete_over_a_stub_index():
    client, idx, st = _graph_client()
    ent = lambda: client.table("rag_entities").delete()
    client._tri = ("stale",)
    assert ent().in_("id", ["nobody"]).execute().data == [] and idx.calls == [] and client._tri == ("stale",)
    got = ent().eq("org_id", "org").in_("id", ["e3", "e1", "zz"]).execute().data
    assert got == [{"id": "e1", "name": "Zeta", "canonical_name": "Zeta"}, {"id": "e3", "name": "Quasar", "canonical_name": "quasar"}]
    assert idx.calls == [("graph", [1, 3], None, None, 4)] and client._tri is None       # the index changed before the store
    assert st.entity_ids == ["e0", "e2"] and st.entity_documents == ["d0", None]
    assert ent().eq("canonical_name", "beta").execute().data[0]["id"] == "e2" and st.entity_ids == ["e0"]
    client, idx, st = _graph_client()
    assert [r["id"] for r in ent().eq("document_id", "d1").execute().data] == ["e1", "e3"]
    assert [r["id"] for r in ent().in_("document_id", ["d0", "d9"]).eq("id", "e0").execute().data] == ["e0"]
    assert ent().eq("document_id", "d0").execute().data == []                               # gone already
    with pytest.raises(ValueError, match="addressed by id / canonical_name / document_id, not 'name'"):
        ent().eq("name", "x").execute()
    with pytest.raises(ValueError, match="DELETE requires a WHERE clause"):
        ent().execute()
    assert ent().eq("org_id", "other").eq("id", "e2").execute().data == [] and st.entity_ids == ["e2"]
    # a refused index call leaves the store as it was
    idx.refuse = True
    with pytest.raises(T.NativeError, match="refused"):
        ent().eq("id", "e2").execute()
    assert st.entity_ids == ["e2"]
    # without the column, document_id is not served
    bare = GpuIndexClient(_StubIndex(6, 3, {}, {}), _store(), org_id="org")
    with pytest.raises(ValueError, match="addressed by id / canonical_name, not 'document_id'"):
        bare.table("rag_entities").delete().eq("document_id", "d0").execute()
    many, idx, _ = _graph_client(tenants=True)
    with pytest.raises(ValueError, match="DELETE requires a WHERE clause"):
        many.table("rag_entities").delete().eq("org_id", "acme").execute()                 # org_id narrows nothing: no filter


def test_relation_table_delete_over_a_stub_index():
    client, idx, st = _graph_client()
    rel = lambda: client.table("rag_relations").delete()
    for one in ("subject_entity_id", "object_entity_id"):
        with pytest.raises(ValueError, match="undirected edges .* cannot tell subject from object"):
            rel().eq(one, "e0").execute()
    with pytest.raises(ValueError, match="addressed by subject_entity_id / object_entity_id, not 'id'"):
        rel().eq("id", "r0").execute()
    client._tri = ("stale",)
    assert rel().eq("subject_entity_id", "e0").eq("object_entity_id", "e3").execute().data == []      # no such edge
    assert rel().eq("subject_entity_id", "e0").eq("object_entity_id", "e0").execute().data == []      # a self pair
    assert rel().eq("subject_entity_id", "zz").eq("object_entity_id", "e0").execute().data == []
    assert idx.calls == [] and client._tri == ("stale",)
    got = rel().in_("subject_entity_id", ["e1", "e0"]).in_("object_entity_id", ["e0", "e2", "e3", "nobody"]).execute().data
    assert got == [{"subject_entity_id": "e0", "object_entity_id": "e2"}, {"subject_entity_id": "e1", "object_entity_id": "e0"},
                   {"subject_entity_id": "e1", "object_entity_id": "e3"}]
    assert idx.calls == [("graph", None, ([0, 1, 1], [2, 0, 3]), None, 4)] and client._tri is None


def test_mention_table_delete_over_a_stub_index():
    client, idx, st = _graph_client()
    men = lambda c=client: c.table("rag_entity_mentions").delete()
    with pytest.raises(ValueError, match="DELETE requires a WHERE clause"):
        men().execute()
    with pytest.raises(ValueError, match="addressed by entity_id / child_chunk_id, not 'id'"):
        men().eq("id", "m0").execute()
    assert men().eq("entity_id", "e2").execute().data == [] and men().eq("entity_id", "zz").execute().data == []
    assert idx.calls == []
    got = men().eq("entity_id", "e1").execute().data
    assert got == [{"entity_id": "e1", "child_chunk_id": "c1", "confidence": 0.25},
                   {"entity_id": "e1", "child_chunk_id": "c1", "confidence": 0.75},
                   {"entity_id": "e1", "child_chunk_id": "c5", "confidence": 1.0}]
    assert idx.calls[-1] == ("graph", None, None, ([1], [-1]), 4)
    got = men().in_("child_chunk_id", ["c4", "c2", "c9"]).execute().data
    assert [(r["entity_id"], r["child_chunk_id"]) for r in got] == [("e0", "c4"), ("e3", "c2")]
    assert idx.calls[-1] == ("graph", None, None, ([-1, -1], [2, 4]), 4)
    got = men().eq("entity_id", "e3").eq("child_chunk_id", "c3").execute().data
    assert got == [{"entity_id": "e3", "child_chunk_id": "c3", "confidence": 0.125}]
    assert idx.calls[-1] == ("graph", None, None, ([3], [3]), 4)
    # multi-tenant: a mention's tenant is its chunk's (c0 .. c2 acme, c3 .. c5 bolt)
    many, idx, _ = _graph_client(tenants=True)
    got = men(many).eq("org_id", "bolt").in_("entity_id", ["e0", "e1", "e3"]).execute().data
    assert [(r["entity_id"], r["child_chunk_id"]) for r in got] == [("e0", "c4"), ("e1", "c5"), ("e3", "c3")]
    assert idx.calls[-1] == ("graph", None, None, ([0, 1, 3], [4, 5, 3]), 4)
    assert men(many).eq("org_id", "nobody").eq("entity_id", "e0").execute().data == []


def test_graph_cascade_flag_over_a_stub_index():
    with pytest.raises(ValueError, match="graph_cascade=True needs the store's entity_documents column"):
        GpuIndexClient(_StubIndex(6, 3, {}, {}), _store(), org_id="org", graph_cascade=True)
    # the default: the chunks go, the entities stay, as before the flag
    client, idx, st = _graph_client()
    assert client.graph_cascade is False
    assert client.table("rag_documents").delete().eq("id", "d1").execute().data == [{"id": "d1"}]
    assert idx.calls == [("rows", [3, 4, 5], 6)] and st.entity_ids == ["e0", "e1", "e2", "e3"]
    # with the flag: after the chunk cascade, one delete_graph call, the index before the store
    client, idx, st = _graph_client(graph_cascade=True)
    client._tri = ("stale",)
    assert client.table("rag_documents").delete().eq("id", "d1").execute().data == [{"id": "d1"}]
    assert idx.calls == [("rows", [3, 4, 5], 6), ("graph", [1, 3], None, None, 4)] and client._tri is None
    assert st.entity_ids == ["e0", "e2"] and st.child_ids == ["c0", "c1", "c2"]
    assert client.table("rag_documents").delete().eq("id", "d9").execute().data == [] and len(idx.calls) == 2
    # every entity would go: refused before the chunks are touched
    st2 = _store(entities=("A", "B"), entity_ids=["e0", "e1"], entity_documents=["d0", "d0"])
    idx2 = _StubIndex(6, 2, {}, {})
    idx2.store = st2
    c2 = GpuIndexClient(idx2, st2, org_id="org", graph_cascade=True)
    with pytest.raises(T.NativeError, match="every entity of the index would be deleted"):
        c2.table("rag_documents").delete().eq("id", "d0").execute()
    assert idx2.calls == [] and len(st2.child_ids) == 6
    # multi-tenant: a document other orgs' chunks still name stays, and so do its entities
    many, idx, st = _graph_client(tenants=True, graph_cascade=True)
    st.document_ids[2] = "d1"                                                # (d1: c2 of acme, c3 .. c5 of bolt)
    many.table("rag_documents").delete().eq("org_id", "bolt").eq("id", "d1").execute()
    assert [c[0] for c in idx.calls] == ["rows"] and st.entity_ids == ["e0", "e1", "e2", "e3"]
    many.table("rag_documents").delete().eq("org_id", "acme").eq("id", "d1").execute()
    assert idx.calls[-1][:2] == ("graph", [1, 3])
