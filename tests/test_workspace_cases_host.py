"""The workspace harness (tests/workspace_cases.py) on the CPU: every thr_*_workspace_bytes export of
include/thr_hip.h has an adapter, and the harness catches both ways an entry point can break the contract
-- shown on two fake entries written in torch over CPU tensors, not by breaking a kernel."""
import os
import re
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_cases as W  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "thr_hip.h")).read()


def test_every_size_function_of_the_header_has_an_adapter():
    """A new entry point with a workspace cannot stay outside the contract test: its size function is
    declared in thr_hip.h, and every such function sizes the workspace of some adapter or is listed,
    with its reason, in SIZES_WITHOUT_ADAPTER."""
    text = re.sub(r"/\*.*?\*/", " ", header(), flags=re.S)
    declared = sorted(set(re.findall(r"\bsize_t\s+(thr_\w+_workspace_bytes)\s*\(", text)))
    assert len(declared) >= 16 and "thr_bm25_workspace_bytes" in declared
    covered = {s for a in W.registry() for s in a.sizes}
    assert covered <= set(declared), f"adapters name size functions the header does not declare: {sorted(covered - set(declared))}"
    for name in declared:
        assert (name in covered) != (name in W.SIZES_WITHOUT_ADAPTER), \
            f"{name}: give it an adapter in workspace_cases.py (or list it in SIZES_WITHOUT_ADAPTER with the reason, not both)"
    # the entry points that take a workspace: each is run by an adapter of its size function or is one of the
    # header's exceptions (it reads what a call before it left)
    takers = set(re.findall(r"\bint\s+(thr_\w+)\s*\([^;]*?void\s*\*\s*workspace\b", text, flags=re.S))
    assert len(takers) >= 20
    source = open(os.path.join(ROOT, "tests", "workspace_cases.py")).read()
    binding = open(os.path.join(ROOT, "triple-hybrid-rag_amd", "_native.py")).read()
    for entry in sorted(takers):
        if entry in W.EXCEPTIONS:
            continue
        # the binding function that calls the entry (def ... load().<entry>( or getattr(load(), entry)) is used by the cases
        short = entry[4:]
        assert re.search(rf"\bN\.{short}\(", source) or (short.startswith("graph_topk") and "N.graph_topk" in source), \
            f"{entry} takes a workspace and no adapter of workspace_cases.py calls _native.{short}"
        assert f"def {short}(" in binding
    for entry, why in W.EXCEPTIONS.items():
        assert entry in takers and why


def words(text):
    """Letters, digits and underscores alone: line breaks and comment stars of the header do not matter."""
    return " ".join(re.sub(r"[^A-Za-z0-9_]+", " ", text).split())


def test_the_header_states_the_contract_and_its_exceptions():
    text = words(header())
    for said in ("The workspace's contents on entry are never read", "Nothing outside [workspace, workspace + thr_*_workspace_bytes(...)) is written",
                 "thr_dense_finish_f16 reads what thr_dense_shortlist_f16 left", "read the previous call's tau"):
        assert words(said) in text, said


def test_design_md_holds_a_row_for_every_carve_area():
    """The audit table of DESIGN.md names every area the carve functions take (Arena::take targets and the
    graph's two areas), so an area added to a carve shows up here until the table says who writes it."""
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    at = design.index("## Workspace contract")
    table = design[at:design.index("\n## ", at + 5)] if "\n## " in design[at + 5:] else design[at:]
    areas = {"dense": ["tau", "qerr", "cnt", "tcnt", "cand", "tlist", "sample", "qfrag", "sel_rows", "sel_meta"],
             "bm25": ["ctl", "theta", "q_tot", "q_dub", "q_nt", "q_S", "q_SA", "q_pmask", "q_item0", "q_long", "q_terms", "items",
                      "sweep_items", "ipos", "wrec", "wterm", "slice_s", "slice_id", "slice_cnt", "stamps"],
             "rows": ["cnt", "qptr", "tptr", "cursor", "scope_q", "slab_s", "slab_id"],
             "graph": ["con_val", "dist"], "entity": ["filter", "slots", "rec", "best"],
             "text": ["unit_off", "unit_unknown", "tok_off", "tok_len", "row_of"],
             "grow": ["slots", "slot_of", "low_len", "rank", "byte_at", "unit_neg"],
             "csr": ["total", "loc", "slice_count", "slice_base"], "build": ["keys", "vals", "skeys", "svals", "ukeys", "sums", "count", "tmp"],
             "scope": ["ws_count", "ws_base"]}
    for family, names in areas.items():
        for name in names:
            assert re.search(rf"\|\s*`{re.escape(name)}`", table), f"DESIGN.md, Workspace contract: no row for `{name}` ({family})"
    # ... and every Arena::take of the carve functions is one of them
    csrc = os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc")
    known = {n for names in areas.values() for n in names}
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".hpp")):
            for target in re.findall(r"(?:L\.off_|\*|\b[A-Z]\.|p\.)(\w+)\s*=\s*A\.take", open(os.path.join(csrc, f)).read()):
                assert target in known, f"{f}: the carve takes `{target}`: add its row to DESIGN.md's Workspace contract and to this list"


# ------------------------------------------------------------------------------------------ the harness bites
def fake(name, run):
    shapes = {"A": 4096, "B": 1024}
    return W.Adapter(name, (), shapes, need=lambda shape: shape, run=run,
                     expected=lambda shape: {"sum": np.array([shape * (shape // 4 - 1) // 8], dtype=np.int64)})


def honest(shape, ws):
    """Writes every word it reads: the sum of 0 .. shape / 4 - 1, staged in the workspace."""
    w = ws.view(torch.int32)
    w.copy_(torch.arange(shape // 4, dtype=torch.int32))
    return {"sum": w.sum(dtype=torch.int64).reshape(1)}


def reads_a_word_it_never_wrote(shape, ws):
    w = ws.view(torch.int32)
    w[1:].copy_(torch.arange(1, shape // 4, dtype=torch.int32))       # (word 0 is "zero anyway")
    return {"sum": w.sum(dtype=torch.int64).reshape(1)}


def writes_one_byte_past_its_size(shape, ws):
    out = honest(shape, ws)
    torch.as_strided(ws, (shape + 1,), (1,))[shape] = 7
    return out


def test_an_honest_entry_passes():
    W.exercise(fake("honest", honest), "cpu")


def test_a_word_read_before_it_is_written_is_caught_by_zero_against_ones():
    with pytest.raises(AssertionError, match="zeroed workspace and on one of 0xFF"):
        W.exercise(fake("stale", reads_a_word_it_never_wrote), "cpu")
    # on a zeroed workspace alone it is the reference's answer: a fresh allocation that happens to be zero hides it
    slab = W.Slab(4096, "cpu")
    W.assert_expected(fake("stale", reads_a_word_it_never_wrote), "B", W.run_once(fake("stale", reads_a_word_it_never_wrote), slab, "B", W.ZERO))


def test_a_byte_written_past_the_size_is_caught_by_unchanged_outside():
    with pytest.raises(AssertionError, match=r"byte 1024 relative to the workspace \(behind it, 1024 bytes long\) was written"):
        W.exercise(fake("past", writes_one_byte_past_its_size), "cpu")
    # shape A fills the room: there the byte lands in the guard
    slab = W.Slab(4096, "cpu")
    with pytest.raises(AssertionError, match="byte 4096 relative to the workspace"):
        W.run_once(fake("past", writes_one_byte_past_its_size), slab, "A", W.ONES)


def test_the_slab_hands_out_an_aligned_exact_view_between_two_guards():
    for need in (1, 255, 256, 4097):
        slab = W.Slab(need, "cpu")
        v = slab.view(need)
        assert v.numel() == need and v.data_ptr() % W.ALIGN == 0 and v.is_contiguous()
        lo = v.data_ptr() - slab.buf.data_ptr()
        assert lo >= W.GUARD and slab.buf.numel() - (lo + need) >= W.GUARD
        with pytest.raises(AssertionError):
            slab.view(need + 1)
    slab = W.Slab(512, "cpu")
    slab.fill(0xFF)
    v = slab.view(256)
    with slab.unchanged_outside(v):
        v.fill_(3)                                  # inside: allowed
    with pytest.raises(AssertionError, match="in front of it"):
        with slab.unchanged_outside(v):
            slab.buf[slab.start - 1] = 0


def test_the_exemptions_are_the_headers_words():
    """Every undefined region the adapters cut is called so by a line of thr_hip.h."""
    text = words(header())
    for key, said in W.UNDEFINED.items():
        assert words(said) in text, f"UNDEFINED[{key!r}]: thr_hip.h does not say {said!r}"
