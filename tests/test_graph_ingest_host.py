"""Graph ingest, the parts that need no GPU: the new C entry's symbols and host-side argument checks
(also under AddressSanitizer + UBSan, in a stand-alone program), ``csr_merge_ref`` pinned to the
project's own fresh build, the built cases' properties, the refusals of ``append_graph`` /
``append_mentions`` (validation runs before any device work), the name store's concatenation rule
and the three graph tables over a store and a stub index."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import graph_ingest_cases as GC
import triple_hybrid_rag_amd as T
from triple_hybrid_rag_amd import index_build as IB
from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient
from triple_hybrid_rag_amd.index import GpuIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = T._native


# --------------------------------------------------------------------------- the C entry
def test_csr_merge_is_declared_exported_and_bound():
    lib = N.load()
    header = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    for name in ("thr_csr_merge", "thr_csr_merge_workspace_bytes", "thr_csr_merge_slice"):
        assert name in N.EXPORTED_SYMBOLS and hasattr(lib, name) and re.search(rf"\b{name}\s*\(", header)
    assert lib.thr_abi_version() == N.ABI_VERSION == 9              # additive: no version bump
    m = re.search(r"#define\s+THR_CSR_MERGE_SLICE\s+(\d+)", header)
    assert m and int(m.group(1)) == lib.thr_csr_merge_slice() == N.THR_CSR_MERGE_SLICE == GC.S
    for name, bit in (("UNSORTED_A", GC.UNSORTED_A), ("UNSORTED_B", GC.UNSORTED_B), ("OVERFLOW", GC.OVERFLOW)):
        assert re.search(rf"#define\s+THR_CSR_MERGE_{name}\s+{bit}\b", header)
        assert getattr(N, "THR_CSR_MERGE_" + name) == bit


def test_csr_merge_checks_its_arguments_on_the_host():
    lib = N.load()
    INVALID, WORKSPACE = -1, -3
    p = 4096          # (non-null, aligned pointer values: every call below is refused before any launch)
    ok = dict(rowptr_a=p, rows_a=4, nnz_a=8, ids_a=2 * p, pay_a=3 * p, rowptr_b=4 * p, rows_b=6, nnz_b=3, ids_b=5 * p,
              pay_b=6 * p, drop=0, rowptr_out=7 * p, ids_out=8 * p, pay_out=9 * p, cap=11, nnz_out=10 * p,
              status=11 * p, ws=12 * p, ws_bytes=0, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.thr_csr_merge(*[a[k] for k in ok])
    assert call() == WORKSPACE                                    # everything else passed
    for name in ("rowptr_b", "rowptr_out", "nnz_out", "status", "rowptr_a", "ids_a", "ids_b", "ids_out"):
        assert call(**{name: None}) == INVALID, name               # null pointers with non-zero sizes
    assert call(rows_b=3) == INVALID                               # rows_b < rows_a
    assert call(rows_a=-1) == INVALID and call(nnz_a=-1) == INVALID and call(nnz_b=-2) == INVALID
    assert call(cap=-1) == INVALID and call(drop=2) == INVALID and call(drop=-1) == INVALID
    for one_side in ("pay_a", "pay_b", "pay_out"):                 # a payload on one side only
        assert call(**{one_side: None}) == INVALID
    assert call(pay_a=None, pay_b=None, pay_out=None) == WORKSPACE
    assert call(rows_a=0, rowptr_a=None) == INVALID                # entries without rows
    assert call(rows_a=0, rowptr_a=None, nnz_a=0, ids_a=None, pay_a=None) == WORKSPACE   # an empty A
    assert call(rowptr_out=ok["rowptr_a"]) == INVALID and call(ids_out=ok["ids_b"]) == INVALID   # out of place only
    assert call(ws_bytes=1 << 20, ws=None) == INVALID
    need = lib.thr_csr_merge_workspace_bytes(6, 8, 3)
    assert need == 4 * 256 and call(ws_bytes=need - 1) == WORKSPACE
    assert lib.thr_csr_merge_workspace_bytes(10, 0, 0) == 256
    # one word per position of B, 12 bytes per slice of B: A's size does not enter
    assert lib.thr_csr_merge_workspace_bytes(10, 1 << 30, GC.S + 1) == 256 + 4352 + 256 + 256
    assert lib.thr_csr_merge_workspace_bytes(-1, 0, 0) == 0 and lib.thr_csr_merge_workspace_bytes(1, 0, -1) == 0


def test_host_checks_are_clean_under_address_and_ub_sanitizer(tmp_path):
    """The entry's argument checks and its workspace-size function, compiled together with a
    stand-alone program (its own main) with the host side under ASan + UBSan, run on the CPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "csr_merge_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "csr_merge.hip"),
                    os.path.join(ROOT, "tests", "native", "csr_merge_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "csr_merge host check: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# --------------------------------------------------------------------------- csr_merge_ref and the cases
def _graph_steps(seed, n_chunks=60, e0=25, m=9):
    """Old rows and a batch: (entity ids, old relations, old mentions, new relations, new mentions)."""
    ents0, rels0, mens0 = GC.graph_rows(seed, n_chunks, e0, 60, 120)
    ents1, rels1, mens1 = GC.graph_rows(seed + 100, n_chunks, m, 50, 90, ent_base=e0)
    rels1 += rels0[:7] + [dict(r, subject_entity_id=r["object_entity_id"], object_entity_id=r["subject_entity_id"])
                          for r in rels0[7:12]]          # edges the index already holds, both orientations
    mens1 += mens0[:5]                                   # mentions it already holds: kept again
    rels1.append({"subject_entity_id": "e1", "object_entity_id": "nobody"})     # unknown ids: skipped
    mens1.append({"entity_id": "e1", "child_chunk_id": "nothing"})
    return [e["id"] for e in ents0], [e["id"] for e in ents1], rels0, mens0, rels1, mens1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_merge_ref_of_a_canonical_batch_is_the_fresh_build(seed):
    """build_graph(old rows + new rows) == csr_merge_ref(build_graph(old rows), the batch as
    append_graph / append_mentions canonicalise it), array for array."""
    ids0, ids1, rels0, mens0, rels1, mens1 = _graph_steps(seed)
    cidx = {f"c{i}": 1000 + i for i in range(60)}
    fresh = IB.build_graph(ids0 + ids1, rels0 + rels1, mens0 + mens1, cidx)
    er, ec, mr, mc, mw = IB.build_graph(ids0, rels0, mens0, cidx)
    eidx = {e: i for i, e in enumerate(ids0 + ids1)}
    n = len(eidx)
    pairs = [(eidx.get(r["subject_entity_id"]), eidx.get(r["object_entity_id"])) for r in rels1]
    pairs = [(a, b) for a, b in pairs if a is not None and b is not None]
    rp_b, dst_b = GC.canonical_relations([a for a, _ in pairs], [b for _, b in pairs], n)
    got_er, got_ec, _, nnz, status = GC.csr_merge_ref(er, ec, None, rp_b, dst_b, None, 1)
    assert status == 0 and nnz == len(fresh[1]) < len(ec) + len(dst_b)            # (some were present)
    assert np.array_equal(got_er, fresh[0]) and np.array_equal(got_ec, fresh[1]) and got_ec.dtype == fresh[1].dtype
    men = [(eidx.get(m["entity_id"]), cidx.get(m["child_chunk_id"]), float(m.get("confidence", 1.0))) for m in mens1]
    men = [t for t in men if t[0] is not None and t[1] is not None]
    mr_a = np.concatenate([mr, np.full(len(ids1), mr[-1])])                        # (append_graph grew the rows)
    rp_m, mc_b, mw_b = GC.canonical_mentions([t[0] for t in men], [t[1] for t in men], [t[2] for t in men], n)
    got = GC.csr_merge_ref(mr_a, mc, mw.view(np.int32), rp_m, mc_b, mw_b.view(np.int32), 0)
    assert got[4] == 0 and np.array_equal(got[0], fresh[2]) and np.array_equal(got[1], fresh[3])
    assert np.array_equal(got[2], fresh[4].view(np.int32))
    # the rules matter: each wrong variant changes this very result
    assert not np.array_equal(GC.csr_merge_ref(er, ec, None, rp_b, dst_b, None, 1, "keep_in_union")[1], fresh[1])
    wrong = GC.csr_merge_ref(mr_a, mc, mw.view(np.int32), rp_m, mc_b, mw_b.view(np.int32), 0, "drop_in_multiset")
    assert wrong[3] < len(fresh[3])
    wrong = GC.csr_merge_ref(mr_a, mc, mw.view(np.int32), rp_m, mc_b, mw_b.view(np.int32), 0, "b_first")
    assert np.array_equal(wrong[1], fresh[3]) and not np.array_equal(wrong[2], fresh[4].view(np.int32))


def test_merge_ref_is_sensitive_to_its_rules_on_named_cases():
    C = GC.cases()
    runs, shapes = C["runs"], C["shapes"]
    right = GC.expected(runs, 0)
    b_first = GC.csr_merge_ref(runs.rowptr_a, runs.ids_a, runs.pay_a, runs.rowptr_b, runs.ids_b, runs.pay_b, 0, "b_first")
    assert np.array_equal(b_first[1], right[1]) and not np.array_equal(b_first[2], right[2])    # ties: A first
    t = runs.rows["run_across"]
    row = right[2][right[0][t]:right[0][t + 1]]
    assert row.tolist()[:4] == sorted(row.tolist()[:4], key=lambda v: (v < 0, abs(v)))        # A's (+), then B's (-)
    assert (row[:2] > 0).all() and (row[2:4] < 0).all()
    dropped = GC.csr_merge_ref(runs.rowptr_a, runs.ids_a, runs.pay_a, runs.rowptr_b, runs.ids_b, runs.pay_b, 0,
                               "drop_in_multiset")
    assert dropped[3] < right[3] == len(runs.ids_a) + len(runs.ids_b)
    union = GC.expected(shapes, 1)
    kept = GC.csr_merge_ref(shapes.rowptr_a, shapes.ids_a, None, shapes.rowptr_b, shapes.ids_b, None, 1, "keep_in_union")
    assert kept[3] > union[3] and kept[3] == len(shapes.ids_a) + len(shapes.ids_b)


def test_every_case_has_the_property_it_is_named_for():
    C, S = GC.cases(), GC.S
    assert sorted(C) == sorted(GC.CASE_NAMES)
    sh = C["shapes"]
    rows_a = len(sh.rowptr_a) - 1
    r = sh.rows
    assert len(sh.row("a", r["both_empty"])) == len(sh.row("b", r["both_empty"])) == 0
    assert len(sh.row("a", r["only_a"])) and not len(sh.row("b", r["only_a"]))
    assert not len(sh.row("a", r["only_b"])) and len(sh.row("b", r["only_b"]))
    assert r["b_only_row"] >= rows_a and len(sh.row("b", r["b_only_row"])) and r["b_only_last"] == len(sh.rowptr_b) - 2
    assert sh.row("b", r["b_below"]).max() < sh.row("a", r["b_below"]).min()
    assert sh.row("b", r["b_above"]).min() > sh.row("a", r["b_above"]).max()
    both = np.sort(np.concatenate([sh.row("a", r["interleaved"]), sh.row("b", r["interleaved"])]))
    assert np.array_equal(both, np.arange(10)) and sh.row("a", r["interleaved"])[0] == 0
    assert np.isin(sh.row("b", r["b_present"]), sh.row("a", r["b_present"])).all()
    a, b = sh.row("a", r["ends_equal"]), sh.row("b", r["ends_equal"])
    assert a[0] == b[0] and a[-1] == b[-1] and not np.isin(b[1:-1], a).any()
    a, b = sh.row("a", r["id_extremes"]), sh.row("b", r["id_extremes"])
    assert a[0] == b[0] == 0 and a[-1] == b[-1] == 2 ** 31 - 2
    # everything of B present: the union changes nothing
    ap = C["all_present"]
    out = GC.expected(ap, 1)
    assert len(ap.ids_b) > 100 and np.array_equal(out[0], ap.rowptr_a) and np.array_equal(out[1], ap.ids_a)
    assert np.array_equal(ap.row("a", ap.rows["whole_row"]), ap.row("b", ap.rows["whole_row"]))
    # lengths against S, on each side and in the output of each mode; rows start, end and span slice edges
    se = C["slice_edges"]
    union, multi = GC.expected(se, 1), GC.expected(se, 0)
    for L in (S - 1, S, S + 1, 2 * S + 1):
        assert len(se.row("a", se.rows[f"a_{L}"])) == L and len(se.row("b", se.rows[f"b_{L}"])) == L
        t = se.rows[f"out_union_{L}"]
        assert union[0][t + 1] - union[0][t] == L
        t = se.rows[f"out_multiset_{L}"]
        assert multi[0][t + 1] - multi[0][t] == L
    for rp in (se.rowptr_a, se.rowptr_b, union[0], multi[0]):
        lens = np.diff(rp)
        spans = (rp[:-1] // S) != ((rp[1:] - 1) // S)
        assert (spans & (lens > 0)).sum() >= 4                     # rows that cross a slice edge
        assert ((rp[1:] - rp[:-1]) > 2 * S).any()                  # one that holds a whole slice
    st = C["star"]
    a, b = st.row("a", st.rows["star"]), st.row("b", st.rows["star"])
    assert len(a) == 4097 and len(b) == 1025 and int(np.isin(b, a).sum()) == 512
    assert len(C["nnz_b_zero"].ids_b) == 0 and len(C["nnz_b_zero"].ids_a) > 0
    assert len(C["nnz_a_zero"].ids_a) == 0 and len(C["nnz_a_zero"].ids_b) > 0
    assert len(C["rows_a_zero"].rowptr_a) == 1 and len(C["rows_a_zero"].ids_b) > 0
    ru = C["runs"]
    assert ru.modes == (0,) and GC.csr_merge_ref(ru.rowptr_a, ru.ids_a, None, ru.rowptr_b, ru.ids_b, None, 1)[4] == 3
    for name, side in (("run_in_a", "a"), ("run_in_b", "b")):
        assert (np.diff(ru.row(side, ru.rows[name])) == 0).any()
    assert np.isin(ru.row("b", ru.rows["run_across"]), ru.row("a", ru.rows["run_across"])).all()
    assert len(set(ru.pay_a.tolist()) | set(ru.pay_b.tolist())) == len(ru.pay_a) + len(ru.pay_b)    # order is visible
    fb = C["float_bits"]
    f = np.concatenate([fb.pay_a, fb.pay_b]).view(np.float32)
    assert np.isnan(f).sum() == 2 and (np.signbit(f) & (f == 0)).sum() == 2
    # the precondition cases: which side, in which mode
    for name in GC.CASE_NAMES:
        c = C[name]
        for mode in (0, 1):
            status = GC.csr_merge_ref(c.rowptr_a, c.ids_a, None, c.rowptr_b, c.ids_b, None, mode)[4]
            assert status == c.status.get(mode, 0), (name, mode)
            assert (status == 0) == (mode in c.modes), (name, mode)
    assert C["duplicate_in_a"].status == {1: 1} and C["duplicate_in_b"].status == {1: 2}
    assert C["descending_in_a"].status == {0: 1, 1: 1} and C["descending_in_b"].status == {0: 2, 1: 2}
    assert C["descending_across_rows"].status == {}


# --------------------------------------------------------------------------- the wrapper's refusals
class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def _bare_index(**attrs):
    """A GpuIndex without a device: only what the validation reads."""
    idx = object.__new__(GpuIndex)
    base = dict(docs=None, dim=0, n_docs=100, lex=None, doc_coll=None, tokens=None, graph=None, entities=None,
                _lex_global=False)
    base.update(attrs)
    idx.__dict__.update(base)
    return idx


def test_append_graph_and_append_mentions_refuse_before_any_device_work():
    E = T.NativeError
    none = _bare_index()
    with pytest.raises(E, match="append_graph: this index has no graph channel"):
        none.append_graph(n_new_entities=1)
    with pytest.raises(E, match="append_mentions: this index has no graph channel"):
        none.append_mentions([0], [0])
    graph = {"men_rowptr": _Shape(11), "ent_rowptr": _Shape(11)}
    named = _bare_index(graph=graph, entities={"n": 10})
    plain = _bare_index(graph=graph)
    with pytest.raises(E, match="entity_names for the 2 new entities are required"):
        named.append_graph(n_new_entities=2)
    with pytest.raises(E, match="holds no names for its 10 entities"):
        plain.append_graph(entity_names=["x"])
    with pytest.raises(E, match="n_new_entities differs"):
        named.append_graph(entity_names=["x"], n_new_entities=2)
    with pytest.raises(E, match="one length"):
        named.append_graph(relations=(np.array([1, 2]), np.array([1])))
    with pytest.raises(E, match=r"relations is \(subject, object\)"):
        named.append_graph(relations=(np.array([1]),))
    with pytest.raises(E, match="integer"):
        named.append_graph(relations=(np.array([1.0]), np.array([2.0])))
    for s, o, m in (([10], [0], 0), ([0], [-1], 0), ([0], [12], 2)):
        with pytest.raises(ValueError, match=r"relation endpoints are entity ids, 0 \.\. "):
            named.append_graph(entity_names=["n"] * m, relations=(np.array(s), np.array(o)))
    # nothing to add: a no-op, an empty range, no device touched
    assert named.append_graph() == range(10, 10) and plain.append_graph(n_new_entities=0) == range(10, 10)
    assert named.append_graph(entity_names=[], relations=(np.zeros(0, np.int64), [])) == range(10, 10)
    with pytest.raises(E, match="one length"):
        named.append_mentions(np.array([1, 2]), np.array([1]))
    with pytest.raises(E, match="one length"):
        named.append_mentions(np.array([1]), np.array([1]), np.array([1.0, 2.0]))
    with pytest.raises(ValueError, match=r"existing entities, 0 \.\. 9"):
        named.append_mentions(np.array([10]), np.array([0]))
    with pytest.raises(ValueError, match=r"stored chunks, 0 \.\. 99"):
        named.append_mentions(np.array([9]), np.array([100]))
    with pytest.raises(E, match="integer"):
        named.append_mentions(np.array([0.5]), np.array([1]))
    assert named.append_mentions([], []) is None
    unusable = _bare_index(graph=graph, _unusable="this index is unusable: test")
    with pytest.raises(E, match="unusable"):
        unusable.append_graph(n_new_entities=1)
    with pytest.raises(E, match="unusable"):
        unusable.append_mentions([0], [0])


def test_sharded_classes_refuse_graph_ingest():
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    from triple_hybrid_rag_amd.sharded_client import ShardedIndexClient
    for call in (ShardedIndex.append_graph, ShardedIndex.append_mentions, ShardedIndexClient.insert_entities,
                 ShardedIndexClient.insert_relations, ShardedIndexClient.insert_mentions):
        with pytest.raises(T.NativeError, match="not supported"):
            call(object(), [])


def test_native_wrapper_refuses_shapes_before_any_pointer_is_taken():
    import torch
    rp = torch.zeros(3, dtype=torch.int64)
    ids = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(T.NativeError, match="rows only grow"):
        N.csr_merge(torch.zeros(5, dtype=torch.int64), ids, None, rp, ids, None, True)
    with pytest.raises(T.NativeError, match="both sides or on neither"):
        N.csr_merge(rp, ids, ids.view(torch.float32), rp, ids, None, False)
    with pytest.raises(T.NativeError, match="one per id"):
        N.csr_merge(rp, ids, torch.zeros(3), rp, ids, torch.zeros(2), False)
    with pytest.raises(T.NativeError, match="4-byte"):
        N.csr_merge(rp, ids, torch.zeros(2, dtype=torch.float64), rp, ids, torch.zeros(2, dtype=torch.float64), False)
    with pytest.raises(T.NativeError, match="CUDA"):
        N.csr_merge(rp, ids, None, rp, ids, None, True)
    assert "build_graph" in N.csr_merge_status_message(1) and "A" in N.csr_merge_status_message(1)
    assert "out_capacity" in N.csr_merge_status_message(4) and N.csr_merge_status_message(0) is None


# --------------------------------------------------------------------------- the name store
@pytest.mark.parametrize("old,new", [
    ([], ["Acme"]), (["Acme"], []), (["Acme Corp", "zeta"], ["Beta", "ACME robotics"]),
    (["São Paulo", "İstanbul Büyükşehir"], ["Ünİ", "AÇÃO", ""]), (["", ""], ["", "x"]),
    (["x" * 128, "é" * 64], ["y" * 128, "İ" * 60, "k"])])
def test_name_store_concatenation_equals_packing_all_names(old, new):
    """What append_graph does on the device: the old bytes up to name_ptr[E], then the new names'
    packing -- equal, byte for byte, to pack_entity_names(old + new)."""
    from triple_hybrid_rag_amd.index_entities import pack_entity_names
    blob0, ptr0 = pack_entity_names(old)
    blob1, ptr1 = pack_entity_names(new)
    used = len(blob0) - N.THR_ENTITY_MAX_NEEDLE
    assert used == ptr0[-1]
    blob, ptr = pack_entity_names(old + new)
    assert np.array_equal(np.concatenate([blob0[:used], blob1]), blob)
    assert np.array_equal(np.concatenate([ptr0, ptr1[1:] + used]), ptr)
    assert (blob[ptr[-1]:] == 0xFF).all() and len(blob) - ptr[-1] == N.THR_ENTITY_MAX_NEEDLE


# --------------------------------------------------------------------------- the table surface
class _StubIndex:
    """What the graph tables need of an index: the channels, append_graph and append_mentions."""

    def __init__(self, n_docs, n_ent, names=True):
        self.docs, self.dim, self.n_docs = None, 0, n_docs
        self.lex = self.doc_coll = self.tokens = None
        self.graph = {"men_rowptr": _Shape(n_ent + 1)}
        self.entities = {"n": n_ent} if names else None
        self.n_ent = n_ent
        self.calls = []

    def append_graph(self, entity_names=None, n_new_entities=None, relations=None):
        m = len(entity_names) if entity_names is not None else int(n_new_entities or 0)
        self.calls.append(("graph", entity_names, n_new_entities, relations))
        self.n_ent += m
        if self.entities is not None:
            self.entities = {"n": self.n_ent}
        return range(self.n_ent - m, self.n_ent)

    def append_mentions(self, entity, chunk, conf=None):
        self.calls.append(("mentions", entity, chunk, conf))


def _store(n=6, entities=("Acme Corp", "Zeta"), **kw):
    return CorpusStore(child_ids=[f"c{i}" for i in range(n)], parent_ids=[f"p{i // 2}" for i in range(n)],
                       document_ids=["d0"] * n, texts=[f"alpha t{i}" for i in range(n)], pages=[1] * n,
                       modalities=["text"] * n, entity_names=list(entities), **kw)


def test_graph_tables_over_a_store():
    st = _store(entity_ids=["e0", "e1"], entity_canonical=["acme", None])
    idx = _StubIndex(6, 2)
    client = GpuIndexClient(idx, st, org_id="org")
    ent = lambda: client.table("rag_entities")
    # the upsert lookup (entity_extraction.py:459-470); a store row without a canonical name: its name
    found = ent().select("id").eq("org_id", "org").eq("canonical_name", "acme").limit(1).execute().data
    assert found == [{"id": "e0", "name": "Acme Corp", "canonical_name": "acme"}]
    assert ent().select("id").eq("org_id", "org").eq("canonical_name", "Zeta").limit(1).execute().data[0]["id"] == "e1"
    assert ent().select("id").eq("org_id", "org").eq("canonical_name", "nobody").limit(1).execute().data == []
    assert ent().select("id").eq("org_id", "other").eq("canonical_name", "acme").limit(1).execute().data == []
    assert [r["id"] for r in ent().select("*").in_("id", ["e1", "zz", "e0"]).execute().data] == ["e1", "e0"]
    with pytest.raises(ValueError, match="canonical_name"):
        ent().select("*").eq("name", "x").execute()
    client._tri = ("stale",)
    row = {"id": "e2", "org_id": "org", "document_id": "d0", "entity_type": "ORG", "name": "Beta GmbH",
           "canonical_name": "beta", "description": None, "metadata": {}}
    assert ent().insert(row).execute().data == [{"id": "e2"}]
    assert idx.calls[-1] == ("graph", ["Beta GmbH"], None, None) and client._tri is None
    assert st.entity_names == ["Acme Corp", "Zeta", "Beta GmbH"] and st.entity_index("e2") == 2
    assert ent().select("id").eq("canonical_name", "beta").limit(1).execute().data[0]["id"] == "e2"
    # the index holds the names already: find_entities_batch's re-upload condition stays false
    assert idx.entities["n"] == len(st.entity_names)
    for bad in (row, dict(row, id="e0")):
        with pytest.raises(ValueError, match="duplicate key value violates unique constraint on rag_entities"):
            ent().insert(bad).execute()
    with pytest.raises(ValueError, match="duplicate"):
        ent().insert([dict(row, id="e7"), dict(row, id="e7")]).execute()
    with pytest.raises(ValueError, match="org_id"):
        ent().insert(dict(row, id="e8", org_id="other")).execute()
    assert len(idx.calls) == 1 and len(st.entity_names) == 3                          # nothing changed
    # relations: unknown entities are skipped, as build_graph skips them
    client._tri = ("stale",)
    rels = [{"id": "r0", "org_id": "org", "subject_entity_id": "e2", "object_entity_id": "e0", "relation_type": "x",
             "confidence": 0.9}, {"id": "r1", "subject_entity_id": "e2", "object_entity_id": "nobody"},
            {"id": "r2", "subject_entity_id": "e1", "object_entity_id": "e1"}]
    assert client.table("rag_relations").insert(rels).execute().data == [{"id": "r0"}, {"id": "r1"}, {"id": "r2"}]
    kind, names, m, (s, o) = idx.calls[-1]
    assert kind == "graph" and names is None and s.tolist() == [2, 1] and o.tolist() == [0, 1] and client._tri is None
    n_calls = len(idx.calls)
    client.table("rag_relations").insert({"id": "r3", "subject_entity_id": "x", "object_entity_id": "y"}).execute()
    assert len(idx.calls) == n_calls                                                   # all skipped: no call
    # mentions: unknown entity / chunk skipped, confidence defaults to 1.0, no org_id on the rows
    client._tri = ("stale",)
    mens = [{"id": "m0", "entity_id": "e2", "parent_chunk_id": "p1", "child_chunk_id": "c3", "document_id": "d0",
             "mention_text": "Beta", "confidence": 0.25, "char_start": None, "char_end": None},
            {"id": "m1", "entity_id": "e0", "child_chunk_id": "c5"}, {"id": "m2", "entity_id": "e9", "child_chunk_id": "c1"},
            {"id": "m3", "entity_id": "e1", "child_chunk_id": "c99"}, {"id": "m4", "entity_id": "e1", "child_chunk_id": "c0",
                                                                        "confidence": None}]
    assert len(client.table("rag_entity_mentions").insert(mens).execute().data) == 5
    kind, e, c, w = idx.calls[-1]
    assert kind == "mentions" and e.tolist() == [2, 0, 1] and c.tolist() == [3, 5, 0] and w.tolist() == [0.25, 1.0, 1.0]
    assert w.dtype == np.float32 and client._tri is None
    with pytest.raises(ValueError, match="org_id"):
        client.table("rag_entity_mentions").insert(dict(mens[0], org_id="other")).execute()


def test_store_defaults_without_id_columns_and_the_late_name_upload(tmp_path):
    st = _store()                                  # an older saved index, synth: no id columns
    assert st.entity_ids is None and st.entity_index(1) == 1 and st.entity_index(2) is None
    assert st.entity_index("1") is None and st.entity_index(True) is None
    assert st.entity_row(0) == {"id": 0, "name": "Acme Corp", "canonical_name": "Acme Corp"}
    assert st.entity_by_canonical("Zeta") == 1
    idx = _StubIndex(6, 2, names=False)            # the names were never uploaded (find_entities_batch does it)
    client = GpuIndexClient(idx, st, org_id="org")
    client.table("rag_entities").insert({"id": "u-1", "name": "New", "canonical_name": "new"}).execute()
    assert idx.calls[-1] == ("graph", None, 1, None)           # rows only: the upload takes all names later
    assert st.entity_ids == [0, 1, "u-1"] and st.entity_canonical == [None, None, "new"]
    assert st.entity_index(1) == 1 and st.entity_index("u-1") == 2 and st.entity_by_canonical("Acme Corp") == 0
    client.table("rag_relations").insert({"subject_entity_id": 0, "object_entity_id": "u-1"}).execute()
    assert [a.tolist() for a in idx.calls[-1][3]] == [[0], [2]]
    # save -> load: the grown names and the id columns come back; a directory without them loads as before
    hi = IB.HostIndex(docs=np.zeros((6, 4), dtype=np.float32), store=st)
    IB.save(hi, str(tmp_path / "grown"))
    back = IB.load(str(tmp_path / "grown")).store
    assert list(back.entity_names) == ["Acme Corp", "Zeta", "New"] and list(back.entity_canonical) == [None, None, "new"]
    assert back.entity_index("u-1") == 2 and back.entity_index(1) == 1 and back.entity_index("0") == 0
    back.append_entities([{"id": "u-2", "name": "Later"}])
    assert back.entity_index("u-2") == 3 and back.entity_row(3)["canonical_name"] == "Later"
    IB.save(IB.HostIndex(docs=np.zeros((6, 4), dtype=np.float32), store=_store()), str(tmp_path / "old"))
    assert not (tmp_path / "old" / "store_entity_ids_blob.npy").exists()
    old = IB.load(str(tmp_path / "old")).store
    assert old.entity_ids is None and old.entity_canonical is None and old.entity_index(0) == 0
    # from_rows fills the columns from the entity rows
    ents, rels, mens = GC.graph_rows(3, 8, 4, 8, 8)
    fr = IB.from_rows(GC.child_rows(0, 8), entity_rows=ents, relation_rows=rels, mention_rows=mens).store
    assert fr.entity_ids == ["e0", "e1", "e2", "e3"] and fr.entity_canonical[1] == "são paulo"
    assert fr.entity_by_canonical("são paulo") == 1
