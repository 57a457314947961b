"""The neighbourhood link heuristics' host surface (no GPU): the names, and every argument error
answered with PGCN_E_INVALID before a device is looked for.  The index uploads when it is created,
so pgcn_cn_index_weights -- and the refusal of a query set over another node count -- are checked
in tests/test_gpu_heur.py."""
import ctypes

import numpy as np
import pytest

NAMES = ("pgcn_cn_index_create", "pgcn_cn_index_destroy", "pgcn_cn_index_workspace",
         "pgcn_cn_index_weights", "pgcn_link_heur_score", "pgcn_link_heur_rank",
         "pgcn_cn_index_score_pairs", "pgcn_cn_index_link_ranks")


def test_names(pgcn):
    for s in NAMES:
        assert s in pgcn.EXPORTED and hasattr(pgcn.lib, s), s
    for name in ("CnIndex", "heuristic_link_ranks", "heuristic_pair_scores"):
        assert hasattr(pgcn, name)
    assert pgcn.HEUR_KINDS["cn"] == 1 and pgcn.HEUR_KINDS["aa"] == 2 and pgcn.HEUR_KINDS["ra"] == 3


@pytest.mark.parametrize("n, indptr, indices", [
    (0, [0], []),                   # n_nodes < 1
    (3, None, [0]),                 # null indptr
    (3, [0, 2, 1, 3], [0, 1, 2]),   # indptr descends
    (3, [1, 1, 2, 3], [0, 1, 2]),   # indptr does not start at 0
    (3, [0, 1, 2, 3], None),        # null indices with entries
    (3, [0, 1, 2, 3], [0, 3, 1]),   # index out of range
    (3, [0, 1, 2, 3], [0, -1, 1]),
])
def test_create_validates_on_the_host(pgcn, n, indptr, indices):
    ip = None if indptr is None else np.asarray(indptr, np.int32)
    ix = None if indices is None else np.asarray(indices, np.int32)
    h = ctypes.c_void_p()
    p = [None if a is None else a.ctypes.data_as(ctypes.c_void_p) for a in (ip, ix)]
    assert pgcn.lib.pgcn_cn_index_create(n, *p, ctypes.byref(h)) == pgcn.PGCN_E_INVALID
    assert not h.value


def test_null_arguments_are_invalid(pgcn):
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    ip = np.zeros(2, np.int32)
    assert lib.pgcn_cn_index_create(1, ip.ctypes.data_as(ctypes.c_void_p), None, None) == INV
    assert lib.pgcn_cn_index_workspace(None) == INV
    assert lib.pgcn_cn_index_weights(None, 1, ip.ctypes.data_as(ctypes.c_void_p)) == INV
    # a null index only (the other argument errors need a real one: tests/test_gpu_heur.py)
    assert lib.pgcn_link_heur_score(None, 1, None, None, 0, None, None, None) == INV
    assert lib.pgcn_link_heur_rank(None, 1, None, None, None, None) == INV
    assert lib.pgcn_cn_index_score_pairs(None, 1, None, None, 0, None) == INV
    assert lib.pgcn_cn_index_link_ranks(None, 1, None, None, 0, None, None, None, None, 3, 0, 1,
                                        None, None) == INV
    assert lib.pgcn_cn_index_destroy(None) == pgcn.PGCN_OK
