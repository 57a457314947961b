"""The builders of tests/sparse_cases.py give what the sparse-kernel tests say they run on (no
GPU): the stated row and column lengths, the mean column length that selects the 1024-thread
weight-gradient kernels, exactly sized bitmaps, and a transposed index (pgcn_csr_transpose) equal
to numpy's stable argsort transpose."""
import numpy as np
import pytest

import sparse_cases as sc

LADDERS = {"col": sc.column_ladder, "row": sc.row_ladder}


def _check_csr(L):
    ip, ix = L["indptr"], L["indices"]
    assert ip.dtype == np.int32 and ix.dtype == np.int32 and L["values"].dtype == np.float32
    assert ip[0] == 0 and len(ip) == L["m"] + 1 and ip[-1] == len(ix) == len(L["values"])
    assert (np.diff(ip) >= 0).all() and ix.min() >= 0 and ix.max() < L["F"]
    for i in range(L["m"]):  # a row's columns ascending, none twice
        assert (np.diff(ix[ip[i]:ip[i + 1]]) > 0).all(), i
    assert np.isfinite(L["values"]).all() and (L["values"] != 0).all()


def test_column_ladder_lengths():
    L = sc.column_ladder()
    _check_csr(L)
    assert (L["m"], L["F"]) == (2200, 18)
    got = np.bincount(L["indices"], minlength=L["F"])
    np.testing.assert_array_equal(got, L["col_len"])
    assert sorted(got) == sorted(sc.COL_LENGTHS) == list(sc.COL_LENGTHS)
    assert list(got) != sorted(got), "the ladder is shuffled over the feature ids"
    # every chunk edge of both forms: CH, CH +- 1, 2 CH +- 1 (CH 256 and 1024), the 16-entry
    # add batches' edges, an empty column and a single entry
    for ch in (256, 1024):
        assert {ch - 1, ch, ch + 1, 2 * ch - 1, 2 * ch, 2 * ch + 1} <= set(got)
    assert {0, 1, 15, 16, 17, L["m"]} <= set(got)
    # the launcher's rule: nnz > 512 nf -> the 1024-thread kernels; nnz = 0 -> the 256-thread ones
    nnz = int(L["indptr"][-1])
    assert nnz == 13769 and nnz > 512 * L["F"] and not 0 > 512 * L["F"]
    assert got.max() > 4 * 256  # the tree kernel's more-than-4-CH trips, 256-thread form
    assert np.diff(L["indptr"]).max() <= L["F"]


def test_row_ladder_lengths():
    L = sc.row_ladder()
    _check_csr(L)
    assert (L["m"], L["F"]) == (41, 70)
    got = np.diff(L["indptr"])
    np.testing.assert_array_equal(got, L["row_len"])
    assert got[0] == 0 and got[-1] == 0
    assert sorted(got[1:-1]) == sorted(sc.ROW_LENGTHS * sc.ROW_REPEATS)
    assert list(got[1:-1]) != sorted(got[1:-1])
    # m p is never a multiple of the forward's 256 threads at the tested widths
    for p in (1, 7, 16, 41, 128):
        assert (L["m"] * p) % 256 != 0


def test_ladders_are_seeded():
    for build in LADDERS.values():
        a, b = build(), build()
        for k in ("indptr", "indices", "values"):
            np.testing.assert_array_equal(a[k], b[k])
            assert not a[k].flags.writeable


@pytest.mark.parametrize("base", sc.MASK_BASES)
def test_bitmap_is_exactly_sized(base):
    nnz = 1000
    m = sc.bitmap(nnz, base)
    assert m.dtype == np.uint64 and len(m) == (base + nnz + 63) // 64
    np.testing.assert_array_equal(m, sc.bitmap(nnz, base))
    keep = sc.keep_bits(m, base, nnz)
    assert 0.4 < keep.mean() < 0.6
    for i in (0, 1, 63 - base % 64, 64 - base % 64, nnz - 1):  # across a word's edge
        assert keep[i] == bool((int(m[(base + i) >> 6]) >> ((base + i) & 63)) & 1)
    v = np.arange(1, nnz + 1, dtype=np.float32)
    d = sc.dropped(v, m, base)
    assert d.dtype == np.float32
    np.testing.assert_array_equal(d, np.where(keep, 2 * v, 0).astype(np.float32))
    assert sc.dropped(v, None, base) is v


@pytest.mark.parametrize("name", sorted(LADDERS))
def test_csr_transpose_matches_stable_argsort(pgcn, name):
    L = LADDERS[name]()
    cp, cr, cpos = pgcn.csr_transpose(L["indptr"], L["indices"], L["F"])
    rp, rr, rpos = sc.transpose_ref(L["indptr"], L["indices"], L["F"])
    np.testing.assert_array_equal(cp, rp)
    np.testing.assert_array_equal(cr, rr)
    np.testing.assert_array_equal(cpos, rpos)
    for f in range(L["F"]):  # a column's entries in row order, pointing at its own values
        assert (np.diff(cr[cp[f]:cp[f + 1]]) > 0).all()
        assert (L["indices"][cpos[cp[f]:cp[f + 1]]] == f).all()


def test_engine_order_is_a_stable_descending_sort():
    L = sc.column_ladder()
    cp, _, _ = sc.transpose_ref(L["indptr"], L["indices"], L["F"])
    order = sc.engine_order(cp)
    assert sorted(order) == list(range(L["F"]))
    lens = np.diff(cp)[order]
    assert (np.diff(lens) <= 0).all()
    ties = np.array([3, 5, 5, 0, 5, 3])
    np.testing.assert_array_equal(sc.engine_order(np.concatenate([[0], np.cumsum(ties)])),
                                  [1, 2, 4, 0, 5, 3])


def test_new_path_names_are_known(pgcn):
    """the six sparse launch counters exist and start from a reset at zero"""
    names = ("spmm_csr", "spmm_csr_dual", "spmm_csc_256", "spmm_csc_1024", "spmm_tree_256",
             "spmm_tree_1024")
    for k in names:
        assert k in pgcn.KERNEL_PATHS
        assert pgcn.lib.pgcn_debug_path_count(k.encode(), 0) >= 0
    assert pgcn.lib.pgcn_debug_path_count(b"spmm_csc_512", 0) == pgcn.PGCN_E_INVALID
    for name in ("pgcn_debug_spmm_csr", "pgcn_debug_spmm_csc_bwd", "pgcn_debug_dropout_mask",
                 "pgcn_debug_dropout_mask2", "pgcn_debug_dropout_apply"):
        assert hasattr(pgcn.lib, name) and name in pgcn.EXPORTED
