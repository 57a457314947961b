"""Input builders of the sparse-feature SpMM tests (tests/test_gpu_sparse_kernels.py), checked
on the CPU by tests/test_cpu_sparse_cases.py.  Not a test file.

Two seeded CSR matrices whose row / column lengths sit on the edges of the kernels' loops:

  column_ladder()  2200 x 18: one feature per length of COL_LENGTHS (0, 1, the 16-entry add
                   batches' edges, the 256- and 1024-entry chunks' edges and their doubles, a full
                   column), each on a seeded random sorted subset of the rows, the feature ids
                   shuffled.  765 entries per feature on average: handing the true nnz to the
                   weight-gradient launcher selects its 1024-thread kernels (nnz > 512 nf), nnz = 0
                   the 256-thread ones, so one matrix puts chunk edges in both.
  row_ladder()     41 x 70: rows of ROW_LENGTHS (the forward's unrolled-by-8 loop and its clamped
                   tail of 7) three times over in shuffled order, between an empty first and an
                   empty last row.

and the dropout bitmaps over their values: exactly the words that bits [0, mask_base + nnz) need.
"""
import numpy as np

COL_ROWS = 2200
COL_LENGTHS = (0, 1, 15, 16, 17, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049,
               2200)
ROW_COLS = 70
ROW_LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 23, 24, 25, 64)
ROW_REPEATS = 3
MASK_BASES = (0, 37, 63, 64 * 3 + 61)
SCALE = 2.0


def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


def _csr(rows, cols, m, rng):
    """CSR of the (row, col) pairs, a row's columns ascending; seeded normal values"""
    o = np.lexsort((cols, rows))
    rows, cols = rows[o], cols[o]
    indptr = np.zeros(m + 1, np.int64)
    np.add.at(indptr, rows + 1, 1)
    values = rng.standard_normal(len(cols)).astype(np.float32)
    return np.cumsum(indptr).astype(np.int32), cols.astype(np.int32), values


def column_ladder():
    """dict(m, F, indptr, indices, values, col_len): col_len[f] = entries of feature f"""
    rng = np.random.default_rng(2200)
    F = len(COL_LENGTHS)
    col_len = np.array(COL_LENGTHS)[rng.permutation(F)]  # the ladder not in index order
    rows = np.concatenate([np.sort(rng.choice(COL_ROWS, n, replace=False)) for n in col_len])
    cols = np.repeat(np.arange(F), col_len)
    indptr, indices, values = _csr(rows, cols, COL_ROWS, rng)
    return _frozen(m=COL_ROWS, F=F, indptr=indptr, indices=indices, values=values,
                   col_len=col_len)


def row_ladder():
    """dict(m, F, indptr, indices, values, row_len): row_len[i] = nonzeros of row i"""
    rng = np.random.default_rng(41)
    body = np.tile(np.array(ROW_LENGTHS), ROW_REPEATS)[rng.permutation(
        len(ROW_LENGTHS) * ROW_REPEATS)]
    row_len = np.concatenate([[0], body, [0]])
    m = len(row_len)
    cols = np.concatenate([np.sort(rng.choice(ROW_COLS, n, replace=False)) for n in row_len])
    rows = np.repeat(np.arange(m), row_len)
    indptr, indices, values = _csr(rows, cols, m, rng)
    return _frozen(m=m, F=ROW_COLS, indptr=indptr, indices=indices, values=values,
                   row_len=row_len)


def bitmap(nnz, base, seed=0):
    """random keep bits for values [0, nnz) at bits base + position: exactly the words needed"""
    rng = np.random.default_rng([nnz, base, seed])
    return rng.integers(0, 2**64, (base + nnz + 63) // 64, dtype=np.uint64)


def keep_bits(mask, base, nnz):
    """bits [base, base + nnz) of the bitmap as a bool array"""
    bits = np.unpackbits(mask.view(np.uint8), bitorder="little")
    assert len(bits) >= base + nnz
    return bits[base:base + nnz].astype(bool)


def dropped(values, mask, base, scale=SCALE):
    """a * (bit ? scale : 0) in fp32, as the kernels form it (mask None: the values)"""
    if mask is None:
        return values
    keep = keep_bits(mask, base, len(values))
    return values * np.where(keep, np.float32(scale), np.float32(0.0)).astype(np.float32)


def transpose_ref(indptr, indices, n_cols):
    """(csc_ptr, csc_row, csc_pos) by a stable argsort of the column ids: a column's entries in
    row order, csc_pos their positions in the CSR arrays"""
    pos = np.argsort(indices, kind="stable").astype(np.int32)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)).astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(indices, minlength=n_cols))])
    return ptr.astype(np.int32), rows[pos], pos


def engine_order(csc_ptr):
    """the features by descending column length, ties in index order (the engine's
    weight-gradient launch order: a stable sort)"""
    return np.argsort(-np.diff(csc_ptr), kind="stable").astype(np.int32)
