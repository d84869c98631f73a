"""rrf_fuse_kernel with exactly ONE channel given: a duplicate-free list with a weight >= 0 is written
straight from the list (rank = position, no sighting / rank / sort loops).  Ids, scores, per-channel
ranks and counts must be what the general path gives -- which the same list takes as soon as a second
channel is present, even an empty one -- and what the reference arithmetic gives in Python floats,
for the RAG2 flavour and both standalone flavours, in every channel slot."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import thr_oracle as O  # noqa: E402

NQ, WIDTH, TOP_K = 40, 100, 130     # top_k above the 128 threads of a block: the padding loop's second trip


@pytest.fixture(scope="module")
def N():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T._native


def lists(seed):
    """[NQ, WIDTH] ids, -1 padded: empty, full and partly filled lists; every fourth one holds duplicates
    (those take the general path), the others none."""
    rng = np.random.default_rng(seed)
    out = np.full((NQ, WIDTH), -1, dtype=np.int64)
    for q in range(NQ):
        n = (0, WIDTH, 1)[q] if q < 3 else int(rng.integers(1, WIDTH + 1))
        out[q, :n] = rng.integers(0, 60, n) if q % 4 == 3 else rng.choice(100000, n, replace=False)
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fuse(N, mode, chans, w):
    """mode 0: thr_rrf_fuse; 1: thr_rrf_fuse_standalone; 2: ... with two_channels -> numpy (ids, scores, ranks, counts)."""
    if mode == 0:
        out = N.rrf_fuse(chans[0], chans[1], chans[2], TOP_K, w[0], w[1], w[2], 60, want_ranks=True)
    else:
        out = N.rrf_fuse_standalone(chans[0], chans[1], chans[2], TOP_K, w[0], w[1], w[2],
                                    two_channels=mode == 2, want_ranks=True)
    return [o.cpu().numpy() for o in out]


@pytest.mark.parametrize("weight", [0.8, 0.0, -0.5])
@pytest.mark.parametrize("mode,slot", [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 0), (2, 1)])
def test_single_channel_equals_the_general_path(N, mode, slot, weight):
    L = lists(7 * mode + slot)
    w = [0.7, 0.9, 1.1]
    w[slot] = weight                     # (a negative weight reverses the order: general path)
    empty = dev(np.full((NQ, 1), -1, dtype=np.int64))
    alone = [None, None, None]
    alone[slot] = dev(L)
    both = list(alone)
    both[(slot + 1) % (2 if mode == 2 else 3)] = empty     # a second channel without a single id
    ids, sc, rk, cnt = fuse(N, mode, alone, w)
    gi, gs, gr, gc = fuse(N, mode, both, w)
    assert np.array_equal(cnt, gc) and np.array_equal(ids, gi) and np.array_equal(rk, gr)
    assert np.array_equal(sc.view(np.int64), gs.view(np.int64)), "scores differ (bits)"
    # the reference arithmetic, for the lists without duplicates
    for q in range(NQ):
        if q % 4 == 3:
            continue
        n = int((L[q] >= 0).sum())
        assert cnt[q] == n
        order = range(n) if weight >= 0 else range(n - 1, -1, -1)   # stable descending sort
        if weight == 0.0:
            order = range(n)
        exp_ids = [int(L[q, i]) for i in order]
        if mode == 0:
            exp_sc = [0.0 + weight / float(60 + i + 1) for i in order]
        else:
            exp_sc = [0.0 + weight * (1.0 / float(60 + i + 1)) for i in order]
        assert list(ids[q, :n]) == exp_ids and list(sc[q, :n]) == exp_sc
        assert list(rk[q, :n, slot]) == [i + 1 for i in order]
        assert not rk[q, :, [c for c in range(3) if c != slot]].any()
        assert np.all(ids[q, n:] == -1) and np.all(sc[q, n:] == -np.inf) and not rk[q, n:].any()


def test_single_channel_equals_the_oracle_with_duplicates(N):
    """The RAG2 flavour against the CPU oracle, duplicate lists included."""
    L = lists(99)
    w = {"lexical": 0.7, "semantic": 0.8, "graph": 1.0}
    ids, sc, _, cnt = fuse(N, 0, [None, dev(L), None], [0.7, 0.8, 1.0])
    for q in range(NQ):
        n = int((L[q] >= 0).sum())
        ei, es = O.fused_topk_ids(None, [int(x) for x in L[q, :n]], None, TOP_K, w)
        assert list(ids[q, :cnt[q]]) == ei and list(sc[q, :cnt[q]]) == es
