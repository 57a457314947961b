"""Link ranking without a device: the exported symbols, the argument checks of the rank entries
(refused before a device is looked for), the host-built query sets (pgcn_debug_rank_filter) against
a Python set model, and the metric helpers on hand-written counts.

The pattern of the filter test: 40 nodes, directed, with self loops, one edge listed twice, node
39 without slots (and never a column), pairs in all three splits, a positive pair listed twice, a
positive pair that is also an edge, and a query whose anchor has no neighbour on either side.
"""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("pgcn_rank_queries_create", "pgcn_rank_queries_destroy", "pgcn_link_rank_tile",
           "pgcn_link_rank_scores", "pgcn_link_rank", "pgcn_debug_rank_filter",
           "pgcn_gcn_link_ranks")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exported(pgcn):
    for s in SYMBOLS:
        assert s in pgcn.EXPORTED and hasattr(pgcn.lib, s), s
    for k in ("rank_sweep", "rank_filter"):
        assert k in pgcn.KERNEL_PATHS and pgcn.path_counts()[k] >= 0
    tq, tc = pgcn.link_rank_tile()
    assert tq >= 1 and tc >= 1
    for name in ("RankQueries", "rank_filter", "rank_from_counts", "mrr", "hits_at"):
        assert hasattr(pgcn, name)
    assert hasattr(pgcn.GCN, "link_ranks")


def _fake(n_bytes=64):
    """A 16-byte aligned host buffer standing in for a device pointer no check dereferences."""
    raw = np.zeros(n_bytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw, ctypes.c_void_p(raw.ctypes.data + off)


def test_rank_scores_argument_checks(pgcn):
    keep, p = _fake()
    _, mis = _fake()
    mis = ctypes.c_void_p(mis.value + 4)
    f = pgcn.lib.pgcn_link_rank_scores
    ok = (pgcn.PGCN_OK, pgcn.PGCN_E_NODEVICE)
    # a well-formed call gets past the checks (to the device, or to the lack of one) ...
    assert f(p, p, 0, p, 8, 5, p, None) in ok
    # ... and every malformed one is refused before that
    for d in (0, -1, 129):
        assert f(p, p, 1, p, 132, d, p, None) == pgcn.PGCN_E_INVALID
    for ld, d in ((4, 5), (6, 5), (7, 7), (0, 1)):
        assert f(p, p, 1, p, ld, d, p, None) == pgcn.PGCN_E_INVALID
    assert f(p, p, 1, None, 8, 5, p, None) == pgcn.PGCN_E_INVALID
    assert f(None, p, 1, p, 8, 5, p, None) == pgcn.PGCN_E_INVALID
    assert f(p, None, 1, p, 8, 5, p, None) == pgcn.PGCN_E_INVALID
    assert f(p, p, 1, p, 8, 5, None, None) == pgcn.PGCN_E_INVALID
    assert f(p, p, -1, p, 8, 5, p, None) == pgcn.PGCN_E_INVALID
    assert f(p, p, 1, mis, 8, 5, p, None) == pgcn.PGCN_E_INVALID
    del keep


def test_link_rank_argument_checks(pgcn):
    keep, p = _fake()
    f = pgcn.lib.pgcn_link_rank
    assert f(None, p, 8, 5, p, p, None) == pgcn.PGCN_E_INVALID
    assert f(None, p, 8, 0, p, p, None) == pgcn.PGCN_E_INVALID
    assert f(None, p, 6, 5, p, p, None) == pgcn.PGCN_E_INVALID
    assert f(None, None, 8, 5, p, p, None) == pgcn.PGCN_E_INVALID
    assert pgcn.lib.pgcn_gcn_link_ranks(None, 3, 0, 1, None, None) == pgcn.PGCN_E_INVALID
    del keep


def _create(pgcn, n, anchor, target, ptr=None, idx=None):
    a, t = np.asarray(anchor, np.int32), np.asarray(target, np.int32)
    fp = None if ptr is None else np.asarray(ptr, np.int64)
    fi = None if idx is None else np.asarray(idx, np.int32)
    h = ctypes.c_void_p()
    st = pgcn.lib.pgcn_rank_queries_create(n, a.size, _p(a), _p(t),
                                           _p(fp) if fp is not None else None,
                                           _p(fi) if fi is not None else None, ctypes.byref(h))
    if st == pgcn.PGCN_OK:
        pgcn.lib.pgcn_rank_queries_destroy(h)
    return st


def test_rank_queries_validation(pgcn):
    ok = (pgcn.PGCN_OK, pgcn.PGCN_E_NODEVICE)
    bad = pgcn.PGCN_E_INVALID
    assert _create(pgcn, 10, [1, 2], [3, 4]) in ok
    assert _create(pgcn, 10, [1, 2], [3, 4], [0, 2, 2], [0, 9]) in ok
    assert _create(pgcn, 10, [1, 10], [3, 4]) == bad            # anchor out of range
    assert _create(pgcn, 10, [1, 2], [-1, 4]) == bad            # target out of range
    assert _create(pgcn, 10, [1, 2], [3, 4], [0, 2, 3], [5, 2, 0]) == bad   # unsorted
    assert _create(pgcn, 10, [1, 2], [3, 4], [0, 2, 3], [5, 5, 0]) == bad   # duplicated
    assert _create(pgcn, 10, [1, 2], [3, 4], [0, 2, 3], [5, 10, 0]) == bad  # out of range
    assert _create(pgcn, 10, [1, 2], [3, 4], [0, 2, 3], [-1, 5, 0]) == bad
    assert _create(pgcn, 10, [1, 2], [3, 4], [0, 2, 3], [2, 3, 0]) == bad   # holds its target
    assert _create(pgcn, 10, [1, 2], [3, 4], [0, 2, 3], [2, 5, 4]) == bad
    assert _create(pgcn, 10, [1, 2], [3, 4], [0, 2, 1], [2, 5]) == bad      # ptr descends
    assert _create(pgcn, 10, [1, 2], [3, 4], [1, 2, 2], [2, 5]) == bad      # ptr[0] != 0
    h = ctypes.c_void_p()
    a = np.zeros(1, np.int32)
    assert pgcn.lib.pgcn_rank_queries_create(10, 2 ** 31, _p(a), _p(a), None, None,
                                             ctypes.byref(h)) == bad
    assert pgcn.lib.pgcn_rank_queries_create(10, 1, None, _p(a), None, None,
                                             ctypes.byref(h)) == bad
    assert pgcn.lib.pgcn_rank_queries_create(10, 1, _p(a), _p(a), None, None, None) == bad


N = 40


def pattern():
    """(indptr, indices, src, dst, label, split) of the 40-node case."""
    rng = np.random.default_rng(3)
    rows = [[] for _ in range(N)]
    for i in range(N - 2):               # nodes 38, 39 have no slots
        rows[i] = sorted(rng.choice(N - 2, rng.integers(1, 6), replace=False).tolist())
        rows[i] = [j for j in rows[i] if j != 37]   # node 37 is never a column ...
    rows[37] = []                        # ... and has no slots: no neighbour on either side
    for i in (0, 5, 11):
        rows[i] = sorted(set(rows[i]) | {i})        # self loops
    rows[2] = sorted(rows[2] + [rows[2][0]])        # a duplicated edge
    rows[4] = sorted(set(rows[4]) | {9})
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    indices = np.array([j for r in rows for j in r], np.int32)
    E = 90
    src = rng.integers(0, N, E).astype(np.int32)
    dst = rng.integers(0, N, E).astype(np.int32)
    label = (rng.random(E) < 0.6).astype(np.int32)
    label[rng.choice(E, 5, replace=False)] = -1
    split = (1 + np.arange(E) % 3).astype(np.int32)
    split[rng.choice(E, 6, replace=False)] = 0
    src[6], dst[6], label[6], split[6] = 3, 17, 1, 1
    src[7], dst[7], label[7], split[7] = 3, 17, 1, 2        # the same positive pair again
    src[8], dst[8], label[8], split[8] = 4, 9, 1, 3         # a positive pair that is an edge
    src[9], dst[9], label[9], split[9] = 37, 20, 1, 3       # an anchor (side 0) with no neighbour
    src[10], dst[10], label[10], split[10] = 21, 37, 1, 3   # ... and as side 1's anchor
    src[11], dst[11], label[11], split[11] = 5, 5, 1, 3     # the target is the anchor
    return indptr, indices, src, dst, label, split


def model(indptr, indices, src, dst, label, split, s, side, filtered):
    anc, oth = (src, dst) if side == 0 else (dst, src)
    rows = np.repeat(np.arange(N), np.diff(indptr))
    out = []
    for e in range(src.size):
        if label[e] != 1 or split[e] != s:
            continue
        a, t = int(anc[e]), int(oth[e])
        f = set()
        if filtered:
            f.add(a)
            f |= set(indices[rows == a].tolist()) if side == 0 else \
                set(rows[indices == a].tolist())
            f |= {int(oth[p]) for p in range(src.size) if label[p] == 1 and anc[p] == a}
            f.discard(t)
        out.append((a, t, sorted(f)))
    return out


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("side", ["dst", "src"])
def test_rank_filter_matches_set_model(pgcn, side, filtered):
    indptr, indices, src, dst, label, split = pattern()
    assert 39 not in indices and indptr[39] == indptr[40]
    seen_empty_neighbourhood = False
    for s in (1, 2, 3):
        a, t, ptr, idx = pgcn.rank_filter(N, indptr, indices, src, dst, label, split, s, side,
                                          filtered)
        want = model(indptr, indices, src, dst, label, split, s, 0 if side == "dst" else 1,
                     filtered)
        assert a.size == t.size == len(want) > 0 and ptr.shape == (a.size + 1,) and ptr[0] == 0
        assert ptr[-1] == idx.size
        for q, (wa, wt, wf) in enumerate(want):
            assert (a[q], t[q]) == (wa, wt)
            got = idx[ptr[q]:ptr[q + 1]].tolist()
            assert got == wf, (s, q)
            if filtered:
                assert wt not in got and (wa in got or wa == wt)
                seen_empty_neighbourhood |= wa == 37
        if not filtered:
            assert idx.size == 0 and not ptr.any()
    if filtered:
        assert seen_empty_neighbourhood


def test_rank_filter_refusals(pgcn):
    indptr, indices, src, dst, label, split = pattern()
    with pytest.raises(pgcn.PgcnError):
        pgcn.rank_filter(N, indptr, indices, src, dst, label, split, 0)
    with pytest.raises(pgcn.PgcnError):
        pgcn.rank_filter(N, indptr, indices, src, dst, label, split, 4)
    bad = indices.copy()
    bad[3] = N
    with pytest.raises(pgcn.PgcnError):
        pgcn.rank_filter(N, indptr, bad, src, dst, label, split, 3)
    bad = src.copy()
    bad[0] = -1
    with pytest.raises(pgcn.PgcnError):
        pgcn.rank_filter(N, indptr, indices, bad, dst, label, split, 3)


def test_metrics_on_hand_counts(pgcn):
    g, e = np.array([0, 3, 9, 99]), np.array([0, 2, 1, 0])
    assert pgcn.rank_from_counts(g, e, "optimistic").tolist() == [1, 4, 10, 100]
    assert pgcn.rank_from_counts(g, e, "pessimistic").tolist() == [1, 6, 11, 100]
    assert pgcn.rank_from_counts(g, e).tolist() == [1, 5, 10.5, 100]
    with pytest.raises(ValueError):
        pgcn.rank_from_counts(g, e, "best")
    r = pgcn.rank_from_counts(g, e)
    assert pgcn.mrr(r) == pytest.approx((1 + 1 / 5 + 1 / 10.5 + 1 / 100) / 4, rel=1e-15)
    assert pgcn.hits_at(r, 1) == 0.25 and pgcn.hits_at(r, 5) == 0.5
    assert pgcn.hits_at(r, 10) == 0.5 and pgcn.hits_at(r, 11) == 0.75
    assert pgcn.hits_at(r, 100) == 1.0
    assert np.isnan(pgcn.mrr([])) and np.isnan(pgcn.hits_at([], 10))
