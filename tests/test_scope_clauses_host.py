"""Scope clauses without a GPU: the two new entry points are declared, exported and bound; they refuse
bad arguments on the host before any launch; the clause language's canonical forms, refusals, encoding
and grouping; and an equality-only batch still plans exactly as it did, without a clause call."""
import ctypes as C
import itertools
import os
import re
import sys

import numpy as np
import pytest

import triple_hybrid_rag_amd as T
from triple_hybrid_rag_amd import index_scope as IS

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scope_clause_cases as SC  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
In, Between, Not = T.In, T.Between, T.Not
MAX = 2 ** 31 - 1
cc = IS.canonical_clause


def host_index(n=6):
    torch = pytest.importorskip("torch")
    idx = T.GpuIndex.__new__(T.GpuIndex)      # (no device: only the host half of the scope layer)
    idx.device, idx.n_docs, idx.doc_coll, idx._attrs = torch.device("cpu"), n, None, {}
    idx.set_collections(np.arange(n, dtype=np.int32) % 2)
    return idx.set_attributes({"org": (np.arange(n, dtype=np.int32) // 2), "document": np.arange(n, dtype=np.int32)})


def test_new_entry_points_are_declared_exported_and_bound():
    N = T._native
    lib = N.load()
    text = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    assert re.search(r"#define\s+THR_SCOPE_MAX_SET_VALUES\s+\(1 << 22\)", text) and N.THR_SCOPE_MAX_SET_VALUES == 1 << 22
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("thr_scope_resolve_clauses", "thr_scope_resolve_clauses_workspace_bytes"):
        m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", bare, flags=re.S)
        assert m, f"{name} is not declared in thr_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N.EXPORTED_SYMBOLS
        assert len(N._SIGNATURES[name][1]) == len([a for a in m.group(1).split(",") if a.strip()])
    assert lib.thr_abi_version() == N.ABI_VERSION == 9
    assert (T.In, T.Between, T.Not, T.SCOPE_MAX_GENERAL) == (IS.In, IS.Between, IS.Not, 256)


def test_host_side_argument_checks_of_the_clause_calls():
    lib = T._native.load()
    one = (C.c_void_p * 1)(8)    # (never dereferenced: every call below is refused before a launch)
    P8 = C.c_void_p(8)

    def resolve(cols=one, C_=1, n=100, tab=P8, P=2, sv=P8, nsv=4, rowptr=P8, rows=P8, cap=100, labels=P8, overlap=P8,
                ws=P8, wsb=1 << 30):
        return lib.thr_scope_resolve_clauses(cols, C_, n, tab, P, sv, nsv, rowptr, rows, cap, labels, overlap, ws, wsb, None)
    assert resolve(C_=0) == -1 and resolve(C_=9) == -1
    assert resolve(P=0) == -1 and resolve(P=4097) == -1
    assert resolve(n=0) == -1 and resolve(n=2 ** 31) == -1 and resolve(cap=-1) == -1
    assert resolve(nsv=-1) == -1 and resolve(nsv=(1 << 22) + 1) == -1
    assert resolve(sv=None) == -1 and resolve(sv=P8, nsv=0) == -1                # set_values NULL iff n_set_values == 0
    assert resolve(rows=None) == -1 and resolve(rows=P8, cap=0) == -1             # rows and cap: both or neither
    assert resolve(labels=None) == -1 and resolve(overlap=None) == -1             # labels and overlap: both or neither
    assert resolve(cols=None) == -1 and resolve(tab=None) == -1 and resolve(rowptr=None) == -1 and resolve(ws=None) == -1
    assert resolve(cols=(C.c_void_p * 1)(None)) == -1
    assert resolve(wsb=0) == -3 and resolve(sv=None, nsv=0, wsb=0) == -3 and resolve(nsv=1 << 22, wsb=0) == -3
    w = lib.thr_scope_resolve_clauses_workspace_bytes
    assert w(1_000_000, 64) >= 64 * (1_000_000 // 512) * 12
    assert w(0, 4) == 0 == w(10, 0) == w(10, 4097) == w(2 ** 31, 4) == w(-1, 4)


def test_the_wrapper_validates_the_table_before_the_upload():
    torch = pytest.importorskip("torch")
    N = T._native
    col = torch.zeros(10, dtype=torch.int32)
    tab = np.zeros((2, 1, 4), dtype=np.int32)

    def refused(match, table, sv=None, cols=(col,)):
        with pytest.raises(N.NativeError, match=match):
            N.scope_resolve_clauses(list(cols), table, sv)
    refused("attribute columns", tab, cols=())
    refused("same length", np.zeros((2, 2, 4), np.int32), cols=(col, col[:5]))
    refused(r"clauses must be \[P, 1, 4\]", np.zeros((2, 2, 4), np.int32))
    refused("predicates per call", np.zeros((5000, 1, 4), np.int32))
    refused("host numpy", torch.zeros((2, 1, 4), dtype=torch.int32))

    def one(kind, a, b):
        t = tab.copy()
        t[1, 0] = (kind, a, b, 0)
        return t
    sv = np.array([1, 4, 9, 9, 12, 3], dtype=np.int32)
    refused("unknown clause kind 8", one(8, 0, 0))
    refused("unknown clause kind 5", one(5, 0, 0))
    refused("unknown clause kind -1", one(-1, 0, 0))
    refused("0 <= a <= b", one(2, 5, 4))
    refused("0 <= a <= b", one(6, -1, 4))
    refused("offset / length", one(3, 4, 3), sv)          # reaches past the end
    refused("offset / length", one(7, -1, 2), sv)
    refused("offset / length", one(3, 2, 0), sv)          # an empty set is kind 1
    refused("offset / length", one(3, 0, 1), None)        # no set values at all
    refused("ascending and distinct", one(3, 1, 3), sv)   # 4 9 9
    refused("ascending and distinct", one(3, 4, 2), sv)   # 12 3
    refused("set values are >= 0", one(3, 0, 2), np.array([-1, 2], np.int32))
    good, gsv = N.scope_check_clauses(one(7, 0, 3), sv, 1)
    assert good.dtype == np.int32 and good.flags.c_contiguous and gsv.tolist() == sv.tolist()
    N.scope_check_clauses(one(3, 4, 1), sv, 1)            # windows are checked one by one: 12 alone is a set


def test_canonical_forms():
    assert cc(5) == cc([5]) == cc(In([5, 5])) == cc(Between(5, 5)) == cc(range(5, 6)) == cc(np.array([5, -3])) == ("eq", 5)
    assert cc(np.int32(5)) == ("eq", 5)
    assert cc(None) == cc(-1) == cc(-7) == cc([]) == cc(In(())) == cc([-1, -2]) == cc(Between(4, 3)) == cc(range(3, 3)) == ("none",)
    assert cc(Between(-9, -1)) == ("none",) and cc(Between(None, -1)) == ("none",)
    assert cc({9, 2, 2, -1, 5}) == cc((5, 9, 2)) == cc(frozenset([2, 5, 9])) == cc(In(np.array([9, 5, 2, 2]))) == ("set", (2, 5, 9), False)
    torch = pytest.importorskip("torch")
    assert cc(torch.tensor([9, 5, 2])) == ("set", (2, 5, 9), False)
    assert cc(Between(3, 8)) == cc(range(3, 9)) == ("range", 3, 8, False)
    assert cc(Between(None, 8)) == cc(Between(-5, 8)) == ("range", 0, 8, False)
    assert cc(Between(3, None)) == cc(Between(3, 2 ** 40)) == ("range", 3, MAX, False)
    assert cc(Between()) == cc(Not(In([]))) == cc(Not([-1])) == ("range", 0, MAX, False)
    assert cc(Not(5)) == cc(Not([5])) == cc(Not(Between(5, 5))) == ("range", 5, 5, True)
    assert cc(Not([2, 9, 5])) == ("set", (2, 5, 9), True) and cc(Not(range(3, 9))) == ("range", 3, 8, True)


def test_every_refusal_carries_its_message():
    idx = host_index()
    for bad, match in ((range(0, 10, 2), "step 1, got step 2"), (range(9, 0, -1), "step 1"), (True, "integer"),
                       ([1, True], "integer"), (3.0, "integer"), ("3", "integer"), ([1.5], "integer"),
                       (np.array([1.0, 2.0]), "1-d integer array"), (np.zeros((2, 2), np.int32), "1-d integer array"),
                       (np.array([True, False]), "1-d integer array"), (Between(1.5, 3), "integer"),
                       (Between(True, 3), "integer"), (Not(None), "Not"), (Not(Not(3)), "Not"), (In(5), "In"),
                       (Not(True), "integer")):
        with pytest.raises(ValueError, match=match):
            cc(bad)
        with pytest.raises(ValueError, match=match):
            idx.scope_plan([{"org": bad}], 1)
    with pytest.raises(ValueError, match="unknown attribute 'tenant'"):
        idx.scope_plan([{"tenant": [1, 2]}], 1)
    with pytest.raises(ValueError, match="one per query"):
        idx.scope_plan([{"org": [1, 2]}], 2)
    with pytest.raises(ValueError, match="at most 256 distinct scopes"):
        idx.scope_plan([{"document": [i, i + 1]} for i in range(257)], 257)
    with pytest.raises(ValueError, match="table"):            # the table form stays equality-only: [nq, C] ints
        idx.scope_plan(np.zeros((2, 3, 4), dtype=np.int32), 2)


class Recorder:
    """Stands in for _native's resolve calls: records them and answers with empty lists."""

    def __init__(self, monkeypatch, n):
        torch = pytest.importorskip("torch")
        self.calls, self.n = [], n

        def answer(P, want_labels):
            return (torch.zeros(P + 1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32),
                    torch.full((n,), -2, dtype=torch.int32) if want_labels else None, None)

        def eq(cols, preds, cap=None, want_labels=True, rows_out=None):
            self.calls.append(("eq", preds.cpu().numpy().copy()))
            return answer(preds.shape[0], want_labels)

        def clauses(cols, tab, sv=None, cap=None, want_labels=True):
            self.calls.append(("clauses", np.array(tab), np.array(sv)))
            return answer(len(tab), want_labels)
        monkeypatch.setattr(T._native, "scope_resolve", eq)
        monkeypatch.setattr(T._native, "scope_resolve_clauses", clauses)


def test_an_equality_only_batch_plans_as_it_always_did_and_makes_no_clause_call(monkeypatch):
    idx = host_index(8)
    rec = Recorder(monkeypatch, 8)
    plain = [None, {"org": 2}, {"collection": 1, "org": 0}, {"org": None}, {}, {"org": 2}, {"document": 7, "org": -4},
             {"collection": 1}]
    # the parent's plan, restated: the table, its distinct rows in np.unique's order, disjoint_groups
    _, tab = idx._scope_table(plain, len(plain))
    scoped = np.any(tab != -1, axis=1)
    preds, inv = np.unique(tab[scoped], axis=0, return_inverse=True)
    qscope = np.full(len(plain), -1, dtype=np.int32)
    qscope[scoped] = inv.reshape(-1)
    groups = IS.disjoint_groups(preds)
    # ... from the plain batch, and from the same predicates written as one-member sets and ranges
    dressed = [None, {"org": [2]}, {"collection": In([1, 1]), "org": Between(0, 0)}, {"org": In([])}, {}, {"org": range(2, 3)},
               {"document": np.array([7]), "org": [-4]}, {"collection": (1,)}]
    for scopes in (plain, dressed):
        rec.calls.clear()
        plan = idx.scope_plan(scopes, len(scopes))
        assert np.array_equal(plan.preds, preds) and plan.preds.dtype == np.int32
        assert np.array_equal(plan.qscope, qscope)
        assert len(plan.groups) == len(groups) and all(np.array_equal(a, b) for a, b in zip(plan.groups, groups))
        assert plan.clauses is None and plan.set_values is None
        assert rec.calls and all(c[0] == "eq" for c in rec.calls)
        assert np.array_equal(rec.calls[0][1], preds)
    # one general clause anywhere in the batch: the clause entry, and no equality call
    rec.calls.clear()
    plan = idx.scope_plan(plain + [{"org": [1, 3]}], len(plain) + 1)
    assert rec.calls and all(c[0] == "clauses" for c in rec.calls)
    assert plan.clauses is not None and plan.clauses.shape == (6, 3, 4) and plan.set_values.tolist() == [1, 3]
    assert plan.qscope.tolist() == [-1, 0, 1, 2, -1, 0, 3, 4, 5]           # distinct scopes in order of first appearance
    assert plan.preds.tolist() == [[-1, 2, -1], [1, 0, -1], [-1, -2, -1], [-1, -2, 7], [1, -1, -1], [-1, IS.GENERAL, -1]]


def test_duplicates_collapse_and_the_encoding_round_trips(monkeypatch):
    idx = host_index(8)
    rec = Recorder(monkeypatch, 8)
    scopes = [{"org": [3, 1]}, {"org": In((1, 3, 3))}, {"org": np.array([3, 1, -1])}, {"org": Not(Between(1, 2))},
              {"org": Not(range(1, 3))}, {"document": Between(2, None), "org": 1}, {"org": [1], "document": range(2, MAX + 1)},
              {"org": Not(In([]))}, {"org": Between(0, None)}, {"collection": Not([0, 5, 9]), "document": Not(4)}]
    plan = idx.scope_plan(scopes, len(scopes))
    assert plan.qscope.tolist() == [0, 0, 0, 1, 1, 2, 2, 3, 3, 4]
    keys = [(None, ("set", (1, 3), False), None), (None, ("range", 1, 2, True), None), (None, ("eq", 1), ("range", 2, MAX, False)),
            (None, ("range", 0, MAX, False), None), (("set", (0, 5, 9), True), None, ("range", 4, 4, True))]
    assert IS.decode_clauses(plan.clauses, plan.set_values) == keys
    tab, sv = IS.encode_clauses(keys, 3)
    assert np.array_equal(tab, plan.clauses) and np.array_equal(sv, plan.set_values) and sv.tolist() == [1, 3, 0, 5, 9]
    assert tab[0, 1].tolist() == [3, 0, 2, 0] and tab[1, 1].tolist() == [6, 1, 2, 0] and tab[2, 1].tolist() == [2, 1, 1, 0]
    assert tab[4, 0].tolist() == [7, 2, 3, 0] and tab[0, 0].tolist() == [0, 0, 0, 0]
    T._native.scope_check_clauses(tab, sv, 3)                  # what the plan encodes passes the wrapper's validation
    assert IS.decode_clauses(*IS.encode_clauses([(("none",), None)], 2)) == [(("none",), None)]
    # the first call resolved every distinct scope at once
    assert rec.calls[0][0] == "clauses" and np.array_equal(rec.calls[0][1], tab)


def random_clause(rng):
    kind = int(rng.integers(0, 8))
    v = lambda: int(rng.integers(0, 8))                       # noqa: E731
    if kind == 0:
        return v()
    if kind == 1:
        return None
    if kind == 2:
        return sorted(rng.choice(8, int(rng.integers(0, 5)), replace=False).tolist())
    if kind == 3:
        a, b = sorted((v(), v()))
        return Between(a, b)
    if kind == 4:
        return Between(v(), None) if rng.random() < 0.5 else Between(None, v())
    if kind == 5:
        return Not(sorted(rng.choice(8, int(rng.integers(0, 5)), replace=False).tolist()))
    if kind == 6:
        a, b = sorted((v(), v()))
        return Not(Between(a, b))
    return Not(v())


def test_grouping_is_sound_over_every_value_tuple_of_a_small_domain():
    """No two predicates of one group accept the same value tuple: every tuple of {-1, 0 .. 7}^2 against a
    few hundred seeded predicate sets that mix every clause kind, acceptance restated in plain numpy."""
    dom = np.array(list(itertools.product(range(-1, 8), repeat=2)), dtype=np.int64)
    cols = {"x": dom[:, 0], "y": dom[:, 1]}
    rng = np.random.default_rng(11)
    pairs = merged = 0
    for _ in range(300):
        scopes = []
        for _ in range(int(rng.integers(2, 9))):
            sc = {}
            for name in ("x", "y"):
                if rng.random() < 0.7:
                    sc[name] = random_clause(rng)
            scopes.append(sc)
        keys = list(dict.fromkeys(tuple(cc(sc[nm]) if nm in sc else None for nm in ("x", "y")) for sc in scopes))
        masks = {}
        for sc in scopes:
            masks.setdefault(tuple(cc(sc[nm]) if nm in sc else None for nm in ("x", "y")), SC.scope_mask(sc, cols, T))
        groups = IS.clause_groups(keys)
        assert sorted(np.concatenate(groups).tolist()) == list(range(len(keys)))
        for g in groups:
            for i, j in itertools.combinations(g.tolist(), 2):
                pairs += 1
                assert not (masks[keys[i]] & masks[keys[j]]).any(), (keys[i], keys[j])
        merged += sum(len(g) > 1 for g in groups)
        for i, j in itertools.combinations(range(len(keys)), 2):      # the pairwise test alone, both ways round
            d = IS.scopes_disjoint(keys[i], keys[j])
            assert d == IS.scopes_disjoint(keys[j], keys[i])
            assert not d or not (masks[keys[i]] & masks[keys[j]]).any(), (keys[i], keys[j])
    assert pairs > 300 and merged > 100        # (the grouping is not vacuous: predicates do share groups)
    # what must be recognised as disjoint: one pass for these
    one = [(cc([1, 2]),), (cc([3, 4]),), (cc(Between(5, 9)),), (cc(Not(Between(0, 9))),), (cc(0),)]
    assert len(IS.clause_groups(one)) == 1
    assert len(IS.clause_groups([(cc(Not([1, 2, 3])),), (cc([1, 3]),), (cc(Between(2, 2)),)])) == 1
    assert len(IS.clause_groups([(cc(Not([1, 2, 4])),), (cc(Between(1, 2)),), (cc(Between(3, 4)),)])) == 2
    assert len(IS.clause_groups([(cc(Between(0, 10)),), (cc(Between(5, 15)),)])) == 2
    assert len(IS.clause_groups([(cc(Not(1)),), (cc(Not(2)),)])) == 2
    assert len(IS.clause_groups([(cc([1, 2]), None), (None, cc([1, 2]))])) == 2
