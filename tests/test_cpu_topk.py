"""Link top-K without a device: the exported symbols and Python entry points, the argument checks
of pgcn_link_topk and pgcn_topk_queries_create (refused before a device is looked for), the
host-built exclude lists (pgcn_debug_topk_filter) against a Python set model on the ranking filter
test's 40-node pattern and against rank_filter's lists, and the split function."""
import ctypes

import numpy as np
import pytest

import topk_ref
from topk_ref import N

SYMBOLS = ("pgcn_topk_queries_create", "pgcn_topk_queries_destroy", "pgcn_topk_queries_workspace",
           "pgcn_link_topk_tile", "pgcn_link_topk_splits", "pgcn_link_topk",
           "pgcn_debug_topk_filter", "pgcn_gcn_top_links")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_symbols_exported(pgcn):
    for s in SYMBOLS:
        assert s in pgcn.EXPORTED and hasattr(pgcn.lib, s), s
    for k in ("topk_sweep", "topk_merge"):
        assert k in pgcn.KERNEL_PATHS and pgcn.path_counts()[k] >= 0
    for name in ("TopKQueries", "topk_filter", "link_topk_splits", "link_topk_tile"):
        assert hasattr(pgcn, name)
    assert hasattr(pgcn.GCN, "top_links")
    tq, tc, kmax = pgcn.link_topk_tile()
    assert tq >= 1 and tc >= 1 and kmax == 128
    assert (tq, tc) == pgcn.link_rank_tile()
    assert pgcn.link_topk_chunk() == 16384


def _fake(n_bytes=64):
    """A 16-byte aligned host buffer standing in for a device pointer no check dereferences."""
    raw = np.zeros(n_bytes + 16, np.uint8)
    off = (-raw.ctypes.data) % 16
    return raw, ctypes.c_void_p(raw.ctypes.data + off)


def test_link_topk_argument_checks(pgcn):
    keep, p = _fake()
    f = pgcn.lib.pgcn_link_topk
    bad = pgcn.PGCN_E_INVALID
    # (no handle can exist without a device: every call below is refused, whatever else it holds)
    assert f(None, p, 8, 5, p, p, None) == bad
    for d in (0, -1, 129):
        assert f(None, p, 132, d, p, p, None) == bad
    for ld, d in ((4, 5), (6, 5), (7, 7), (0, 1)):
        assert f(None, p, ld, d, p, p, None) == bad
    assert f(None, None, 8, 5, p, p, None) == bad
    assert f(None, ctypes.c_void_p(p.value + 4), 8, 5, p, p, None) == bad
    assert f(None, p, 8, 5, None, None, None) == bad
    assert pgcn.lib.pgcn_gcn_top_links(None, None, 0, 10, 0, 1, None, None) == bad
    assert pgcn.lib.pgcn_topk_queries_workspace(None) == bad
    del keep


def _create(pgcn, n, anchor, ptr=None, idx=None, k=10):
    a = np.asarray(anchor, np.int32)
    xp = None if ptr is None else np.asarray(ptr, np.int64)
    xi = None if idx is None else np.asarray(idx, np.int32)
    h = ctypes.c_void_p()
    st = pgcn.lib.pgcn_topk_queries_create(n, a.size, _p(a), _p(xp) if xp is not None else None,
                                           _p(xi) if xi is not None else None, k, ctypes.byref(h))
    if st == pgcn.PGCN_OK:
        pgcn.lib.pgcn_topk_queries_destroy(h)
    return st


def test_topk_queries_validation(pgcn):
    ok = (pgcn.PGCN_OK, pgcn.PGCN_E_NODEVICE)
    bad = pgcn.PGCN_E_INVALID
    assert _create(pgcn, 10, [1, 2]) in ok
    assert _create(pgcn, 10, [1, 2], [0, 2, 2], [0, 9]) in ok
    assert _create(pgcn, 10, [1, 2], [0, 2, 3], [1, 9, 2]) in ok        # a list may hold the anchor
    for k in (1, 128):
        assert _create(pgcn, 10, [1, 2], k=k) in ok
    for k in (0, 129, -1):
        assert _create(pgcn, 10, [1, 2], k=k) == bad
    assert _create(pgcn, 10, [1, 10]) == bad                            # anchor out of range
    assert _create(pgcn, 10, [-1, 2]) == bad
    assert _create(pgcn, 10, [1, 2], [0, 2, 3], [5, 2, 0]) == bad       # descending
    assert _create(pgcn, 10, [1, 2], [0, 2, 3], [5, 5, 0]) == bad       # duplicated
    assert _create(pgcn, 10, [1, 2], [0, 2, 3], [5, 10, 0]) == bad      # out of range
    assert _create(pgcn, 10, [1, 2], [0, 2, 3], [-1, 5, 0]) == bad
    assert _create(pgcn, 10, [1, 2], [0, 2, 1], [2, 5]) == bad          # ptr descends
    assert _create(pgcn, 10, [1, 2], [1, 2, 2], [2, 5]) == bad          # ptr[0] != 0
    h = ctypes.c_void_p()
    a = np.zeros(1, np.int32)
    f = pgcn.lib.pgcn_topk_queries_create
    assert f(10, 2 ** 31, _p(a), None, None, 10, ctypes.byref(h)) == bad
    assert f(10, 1, None, None, None, 10, ctypes.byref(h)) == bad
    assert f(10, 1, _p(a), None, None, 10, None) == bad
    assert f(0, 1, _p(a), None, None, 10, ctypes.byref(h)) == bad


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("side", ["dst", "src"])
def test_topk_filter_matches_set_model(pgcn, side, filtered):
    indptr, indices, src, dst, label, split = topk_ref.pattern()
    nodes = np.r_[np.arange(N), [3, 3, 37, 39]].astype(np.int32)       # every node, duplicates
    ptr, idx = pgcn.topk_filter(N, indptr, indices, src, dst, label, split, nodes, side, filtered)
    want = topk_ref.exclude_model(N, indptr, indices, src, dst, label, nodes,
                                  0 if side == "dst" else 1, filtered)
    assert ptr.shape == (nodes.size + 1,) and ptr[0] == 0 and ptr[-1] == idx.size
    for q, w in enumerate(want):
        got = idx[ptr[q]:ptr[q + 1]].tolist()
        assert got == w, q
        if filtered:
            assert int(nodes[q]) in got
    if filtered:
        assert idx[ptr[39]:ptr[40]].tolist() == [39]       # the isolated node: itself alone
        assert any(len(w) > 3 for w in want)
    else:
        assert idx.size == 0 and not ptr.any()


@pytest.mark.parametrize("side", ["dst", "src"])
def test_topk_filter_is_rank_filter_plus_target(pgcn, side):
    indptr, indices, src, dst, label, split = topk_ref.pattern()
    a, t, rptr, ridx = pgcn.rank_filter(N, indptr, indices, src, dst, label, split, 3, side, True)
    assert a.size > 0
    ptr, idx = pgcn.topk_filter(N, indptr, indices, src, dst, label, split, a, side, True)
    for q in range(a.size):
        mine = idx[ptr[q]:ptr[q + 1]].tolist()
        assert mine == sorted(set(ridx[rptr[q]:rptr[q + 1]].tolist()) | {int(t[q])}), q


def test_topk_filter_refusals(pgcn):
    indptr, indices, src, dst, label, split = topk_ref.pattern()
    for nodes in ([N], [-1]):
        with pytest.raises(pgcn.PgcnError):
            pgcn.topk_filter(N, indptr, indices, src, dst, label, split, nodes)
    bad = indices.copy()
    bad[3] = N
    with pytest.raises(pgcn.PgcnError):
        pgcn.topk_filter(N, indptr, bad, src, dst, label, split, [1])
    bad = src.copy()
    bad[0] = -1
    with pytest.raises(pgcn.PgcnError):
        pgcn.topk_filter(N, indptr, indices, bad, dst, label, split, [1])
    ptr, idx = pgcn.topk_filter(N, indptr, indices, src, dst, label, split, [])
    assert ptr.tolist() == [0] and idx.size == 0


def test_splits(pgcn):
    tq, tc, _ = pgcn.link_topk_tile()
    for Q in (0, 1, tq, tq + 1, 8192, 2 ** 31 - 1):
        for n in (1, tc, 4096, 232965):
            assert pgcn.link_topk_splits(Q, n) >= 1
    # one query block takes two splits at a small shape: the two-split path is testable
    assert min(n for n in range(1, 4097) if pgcn.link_topk_splits(tq, n) >= 2) <= 4096
    # a function of (Q, n) only: the same answer twice
    assert pgcn.link_topk_splits(8192, 232965) == pgcn.link_topk_splits(8192, 232965) >= 2
