"""Link top-K under the MLP decoder without a GPU: exports, the split function, argument checks."""
import ctypes
import inspect

import numpy as np


def test_exports_and_signature(pgcn):
    for name in ("pgcn_topk_queries_create_mlp", "pgcn_link_topk_mlp_tile",
                 "pgcn_link_topk_mlp_splits", "pgcn_link_topk_mlp", "pgcn_gcn_top_links_decoder"):
        assert name in pgcn.EXPORTED and hasattr(pgcn.lib, name)
    assert "decoder" in inspect.signature(pgcn.GCN.top_links).parameters
    assert {"topk_mlp_sweep", "topk_mlp_merge"} <= set(pgcn.KERNEL_PATHS)
    assert pgcn.link_topk_mlp_tile() == (*pgcn.link_rank_mlp_tile(), 128)


def test_splits_hold_a_chunk_each(pgcn):
    TQ, TC, _ = pgcn.link_topk_mlp_tile()
    for Q in (0, 1, TQ, TQ + 1, 8192, 16384, 10 ** 6):
        for n in (1, TC, 8 * TC, 8 * TC + 1, 17 * TC + 3, 232965):
            s, chunks = pgcn.link_topk_mlp_splits(Q, n), -(-n // TC)
            per = -(-chunks // s)
            assert s >= 1 and (s - 1) * per < chunks  # the last range starts below the end
    assert [pgcn.link_topk_mlp_splits(TQ, 8 * TC + j) for j in (0, 1)] == [1, 2]
    assert pgcn.link_topk_mlp_splits(16384, 232965) == 4


def test_invalid_arguments_before_the_device(pgcn):
    bad, h = pgcn.PGCN_E_INVALID, ctypes.c_void_p()
    a = np.array([0, 5], np.int32).ctypes.data_as(ctypes.c_void_p)
    create = pgcn.lib.pgcn_topk_queries_create_mlp
    assert create(4, 2, a, None, None, 3, ctypes.byref(h)) == bad       # anchor 5 >= 4 nodes
    for k, anchors in ((0, a), (129, a), (3, None)):
        assert create(9, 2, anchors, None, None, k, ctypes.byref(h)) == bad
    assert create(9, 2, a, None, None, 3, None) == bad
    assert pgcn.lib.pgcn_link_topk_mlp(None, None, 8, 8, None, 8, 8, None, None, None) == bad
    assert pgcn.lib.pgcn_gcn_top_links_decoder(None, a, 2, 3, 0, 1, None, None) == bad
