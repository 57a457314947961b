"""Every form of the sparse first layer's kernels (csrc/k_sparse.hip) the engine runs, through
pgcn_debug_spmm_csr / pgcn_debug_spmm_csc_bwd, which hand over what pgcn_spmm_csr /
pgcn_spmm_csc_bwd fix: the padded row stride (ldc, ldg > p), mask_base, the true nnz (the
1024-thread kernels), the launch order and the tree kernel.

  spmm_csr        k_spmm_csr<false>       c = drop(X) b: 8 nonzeros per trip, a clamped tail of 7
  spmm_csr_dual   k_spmm_csr<true>        c = X b beside c2 = drop(X) b
  spmm_csc_256    k_spmm_csc_bwd<256>     bgrad = drop(X)^T cgrad, a column's chain in 256-entry
  spmm_csc_1024   k_spmm_csc_bwd<1024>      / 1024-entry chunks (nnz > 512 nf), software-pipelined;
                                            ldg % 4 == 0: float4 gradient loads, else scalar ones
  spmm_tree_256 / spmm_tree_1024  k_spmm_csc_tree<CH>   the same sums as a fixed tree (csc_tree)

Inputs: tests/sparse_cases.py (checked in test_cpu_sparse_cases.py).  Every case: fixed seeds;
outputs NaN-filled with two guard rows above and below that must stay NaN; the outputs' and the
gradient's padding columns NaN (the former must stay so, the latter must reach no result);
bitmaps of exactly the words bits [0, mask_base + nnz) need; the launch counter of the expected
form asserted, every other sparse counter zero; a second call repeats the first one's bits.

Reference of the chain kernels and the forward: the C oracle's or_spmm_fwd / or_spmm_bwd (the
sequential CPU loops) on the tight arrays with the values dropped beforehand as
a * (bit ? scale : 0) in fp32; equal bit for bit.  The tree kernels: float64, within
1e-5 (|drop(X)|^T |G|) + 1e-30 per element (helpers.product_ref: fp32 reordering only).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers
import sparse_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 2
SCALE = sc.SCALE
SPMM_PATHS = ("spmm_csr", "spmm_csr_dual", "spmm_csc_256", "spmm_csc_1024", "spmm_tree_256",
              "spmm_tree_1024")
MASKS = (None,) + sc.MASK_BASES  # None: no dropout
BUILDERS = {"col": sc.column_ladder, "row": sc.row_ladder}

# (p, ldc) of the forward: m p is never a multiple of the 256-thread block (m = 41)
FWD_WIDTHS = ((1, 4), (7, 7), (7, 8), (16, 16), (41, 44), (41, 48), (128, 128))
# (p, ldg) of the weight gradient: ldg 1, 7, 41 take the scalar-load branch, the others the
# float4 one -- (7, 8) and (41, 44) with padding inside the last 16-column group, (20, 20) with
# a last group of one float4, (128, 128) eight groups
CSC_WIDTHS = ((1, 1), (7, 7), (7, 8), (16, 16), (20, 20), (41, 41), (41, 44), (128, 128))


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (np.array: a writable copy)


# ------------------------------------------------------------------------------ shared inputs
@functools.lru_cache(maxsize=None)
def ladder(name):
    """The ladder, its transposed index and their device copies (read-only, shared)"""
    L = dict(BUILDERS[name]())
    cp, cr, cpos = helpers.pgcn().csr_transpose(L["indptr"], L["indices"], L["F"])
    L.update(cp=cp, cr=cr, cpos=cpos, nnz=int(L["indptr"][-1]))
    L["dev"] = {k: dev(L[k]) for k in ("indptr", "indices", "values", "cp", "cr", "cpos")}
    return L


@functools.lru_cache(maxsize=None)
def operands(name, p):
    """(b [F][p], cgrad [m][p]): seeded per ladder and width"""
    L = ladder(name)
    rng = np.random.default_rng([L["m"], L["F"], p])
    W = rng.standard_normal((L["F"], p)).astype(np.float32)
    G = rng.standard_normal((L["m"], p)).astype(np.float32)
    W.setflags(write=False)
    G.setflags(write=False)
    return W, G


@functools.lru_cache(maxsize=None)
def bitmap(name, base):
    if base is None:
        return None
    m = sc.bitmap(ladder(name)["nnz"], base)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def oracle_ref(name, kind, p, base):
    """or_spmm_fwd ("fwd": [m][p]) / or_spmm_bwd ("bwd": [F][p]) on the pre-dropped values"""
    L = ladder(name)
    lib = helpers.oracle()
    W, G = operands(name, p)
    xd = np.ascontiguousarray(sc.dropped(L["values"], bitmap(name, base), base or 0))
    assert xd.dtype == np.float32
    if kind == "fwd":
        out = np.full((L["m"], p), np.nan, np.float32)
        lib.or_spmm_fwd(L["m"], helpers.ptr(L["indptr"]), helpers.ptr(L["indices"]),
                        helpers.ptr(xd), helpers.ptr(W), helpers.ptr(out), p)
    else:
        out = np.full((L["F"], p), np.nan, np.float32)
        lib.or_spmm_bwd(L["m"], L["F"], helpers.ptr(L["indptr"]), helpers.ptr(L["indices"]),
                        helpers.ptr(xd), helpers.ptr(out), helpers.ptr(G), p)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def float64_ref(name, p, base):
    """(drop(X)^T G, |drop(X)|^T |G|) in float64"""
    L = ladder(name)
    _, G = operands(name, p)
    xd = sc.dropped(L["values"], bitmap(name, base), base or 0)
    X = np.zeros((L["m"], L["F"]))
    rows = np.repeat(np.arange(L["m"]), np.diff(L["indptr"]))
    X[rows, L["indices"]] = xd
    return helpers.product_ref(X.T, G)


# ------------------------------------------------------------------------------ the calls
def guarded_out(rows, ld):
    return torch.full((rows + 2 * GUARD, ld), float("nan"), device=DEV)


def body_ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * GUARD * t.shape[1])


def counts(pgcn):
    c = pgcn.path_counts()
    return {k: c[k] for k in SPMM_PATHS}, c["launches"]


def only(path, n=1):
    return {k: (n if k == path else 0) for k in SPMM_PATHS}


def call_fwd(pgcn, name, p, ldc, base, dual=False, m=None, masked=True):
    """One pgcn_debug_spmm_csr call into fresh outputs: (status, c, c2 or None, sparse
    counters, launches).  base None: no mask; masked False: the mask withheld (dual: refused)"""
    L = ladder(name)
    d = L["dev"]
    W, _ = operands(name, p)
    dW = dev(W)
    dm = dev(bitmap(name, base).view(np.int64)) if base is not None and masked else None
    C = guarded_out(L["m"], ldc)
    C2 = guarded_out(L["m"], ldc) if dual else None
    pgcn.reset_path_counts()
    st = pgcn.lib.pgcn_debug_spmm_csr(L["m"] if m is None else m, p, ldc, vp(d["indptr"]),
                                      vp(d["indices"]), vp(d["values"]), vp(dm), base or 0,
                                      SCALE, vp(dW), body_ptr(C), body_ptr(C2), stream())
    torch.cuda.synchronize()
    return (st, C, C2) + counts(pgcn)


def call_bwd(pgcn, name, p, ldg, base, big, order=None, tree=False, nf=None):
    """One pgcn_debug_spmm_csc_bwd call into a fresh output: (status, bgrad, sparse counters,
    launches).  big: the true nnz handed over (the 1024-thread kernels on the column ladder)"""
    L = ladder(name)
    d = L["dev"]
    _, G = operands(name, p)
    Gp = np.full((L["m"], ldg), np.nan, np.float32)  # the gradient's padding columns: NaN
    Gp[:, :p] = G
    dG = dev(Gp)
    assert dG.data_ptr() % 16 == 0
    dm = dev(bitmap(name, base).view(np.int64)) if base is not None else None
    do = dev(order) if order is not None else None
    B = guarded_out(L["F"], p)
    pgcn.reset_path_counts()
    st = pgcn.lib.pgcn_debug_spmm_csc_bwd(L["F"] if nf is None else nf, p, ldg, vp(d["cp"]),
                                          vp(d["cr"]), vp(d["cpos"]), vp(d["values"]), vp(dm),
                                          base or 0, SCALE, vp(dG), body_ptr(B),
                                          L["nnz"] if big else 0, vp(do), int(tree), stream())
    torch.cuda.synchronize()
    return (st, B) + counts(pgcn)


def split(t, p):
    """(the [:, :p] block of the body, its padding columns, the guard rows) on the host"""
    o = t.cpu().numpy()
    body = o[GUARD:len(o) - GUARD]
    return body[:, :p], body[:, p:], np.concatenate([o[:GUARD], o[len(o) - GUARD:]])


def assert_exact(t, p, ref, what):
    got, pad, guard = split(t, p)
    np.testing.assert_array_equal(got, ref, err_msg=str(what))
    assert np.isnan(pad).all(), (what, "padding columns written")
    assert np.isnan(guard).all(), (what, "guard rows written")


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def bwd_path(big, tree):
    return ("spmm_tree_" if tree else "spmm_csc_") + ("1024" if big else "256")


def mask_id(base):
    return "nomask" if base is None else f"base{base}"


# ------------------------------------------------------------------------------ CSR forward
@pytest.mark.parametrize("p,ldc", FWD_WIDTHS, ids=[f"p{p}-ldc{l}" for p, l in FWD_WIDTHS])
def test_csr_forward_row_ladder(pgcn, p, ldc):
    """Rows of 0, 1, 2, 7, 8, 9, 15..17, 23..25 and 64 nonzeros, an empty first and last row:
    the bits of or_spmm_fwd at every mask_base and without a mask"""
    assert ladder("row")["m"] == 41
    for base in MASKS:
        what = ("row", p, ldc, mask_id(base))
        st, C, _, paths, launches = call_fwd(pgcn, "row", p, ldc, base)
        assert st == pgcn.PGCN_OK and paths == only("spmm_csr") and launches == 1, what
        assert_exact(C, p, oracle_ref("row", "fwd", p, base), what)
        empty = np.nonzero(ladder("row")["row_len"] == 0)[0]
        assert {0, 40} <= set(empty)
        assert (split(C, p)[0][empty] == 0).all(), what
        st2, C_again, _, _, _ = call_fwd(pgcn, "row", p, ldc, base)
        assert st2 == pgcn.PGCN_OK and same_bits(C, C_again), what


@pytest.mark.parametrize("p,ldc", ((16, 16), (41, 44)))
def test_csr_forward_column_ladder(pgcn, p, ldc):
    """2200 rows (several hundred workgroups) of up to 18 nonzeros"""
    for base in (None, 37, 64 * 3 + 61):
        what = ("col", p, ldc, mask_id(base))
        st, C, _, paths, _ = call_fwd(pgcn, "col", p, ldc, base)
        assert st == pgcn.PGCN_OK and paths == only("spmm_csr"), what
        assert_exact(C, p, oracle_ref("col", "fwd", p, base), what)


@pytest.mark.parametrize("name", ("row", "col"))
@pytest.mark.parametrize("p,ldc", ((7, 8), (16, 16), (41, 44)))
def test_csr_dual(pgcn, name, p, ldc):
    """k_spmm_csr<true>: c has the unmasked single call's bits and c2 the masked one's"""
    _, plain, _, _, _ = call_fwd(pgcn, name, p, ldc, None)
    for base in sc.MASK_BASES:
        what = (name, p, ldc, mask_id(base))
        st, C, C2, paths, launches = call_fwd(pgcn, name, p, ldc, base, dual=True)
        assert st == pgcn.PGCN_OK and paths == only("spmm_csr_dual") and launches == 1, what
        _, masked, _, _, _ = call_fwd(pgcn, name, p, ldc, base)
        assert same_bits(C, plain), what
        assert same_bits(C2, masked), what
        assert_exact(C, p, oracle_ref(name, "fwd", p, None), what)
        assert_exact(C2, p, oracle_ref(name, "fwd", p, base), what)
        st, C_again, C2_again, _, _ = call_fwd(pgcn, name, p, ldc, base, dual=True)
        assert st == pgcn.PGCN_OK and same_bits(C, C_again) and same_bits(C2, C2_again), what


def test_csr_dual_needs_the_mask(pgcn):
    """The dual launcher's check: without the mask PGCN_E_INVALID, nothing launched or written
    (a null second output is, by the entry point's contract, the single forward)."""
    for name, p, ldc in (("row", 16, 16), ("col", 41, 44)):
        for base in (0, 37):
            st, C, C2, paths, launches = call_fwd(pgcn, name, p, ldc, base, dual=True,
                                                  masked=False)
            assert st == pgcn.PGCN_E_INVALID, (name, p, base)
            assert paths == only(None) and launches == 0
            assert torch.isnan(C).all() and torch.isnan(C2).all()
        st, C, C2, paths, _ = call_fwd(pgcn, name, p, ldc, 37, dual=False)
        assert st == pgcn.PGCN_OK and C2 is None and paths == only("spmm_csr")


# ------------------------------------------------------------------------------ CSC, the chain
@pytest.mark.parametrize("big", (False, True), ids=("256", "1024"))
@pytest.mark.parametrize("p,ldg", CSC_WIDTHS, ids=[f"p{p}-ldg{l}" for p, l in CSC_WIDTHS])
def test_csc_chain_column_ladder(pgcn, p, ldg, big):
    """Columns of 0, 1, 15..17, 255..257, 511..513, 1023..1025, 2047..2049 and 2200 entries in
    both chunk sizes: the bits of or_spmm_bwd at every mask_base and without a mask; an empty
    column gives an exact zero row"""
    L = ladder("col")
    assert (L["nnz"] > 512 * L["F"]) and set(sc.COL_LENGTHS) == set(L["col_len"])
    for base in MASKS:
        what = ("col", p, ldg, "1024" if big else "256", mask_id(base))
        st, B, paths, launches = call_bwd(pgcn, "col", p, ldg, base, big)
        assert st == pgcn.PGCN_OK and paths == only(bwd_path(big, False)) and launches == 1, what
        assert_exact(B, p, oracle_ref("col", "bwd", p, base), what)
        empty = np.nonzero(L["col_len"] == 0)[0]
        assert len(empty) == 1 and (split(B, p)[0][empty] == 0).all(), what
        st2, B_again, _, _ = call_bwd(pgcn, "col", p, ldg, base, big)
        assert st2 == pgcn.PGCN_OK and same_bits(B, B_again), what


@pytest.mark.parametrize("p,ldg", ((16, 16), (41, 44), (7, 7)))
def test_csc_chain_short_columns(pgcn, p, ldg):
    """The row ladder transposed: 70 columns of 9 entries on average, the 256-thread form by
    its true nnz"""
    L = ladder("row")
    assert L["nnz"] <= 512 * L["F"]
    for base in (None, 63):
        st, B, paths, _ = call_bwd(pgcn, "row", p, ldg, base, True)
        assert st == pgcn.PGCN_OK and paths == only("spmm_csc_256")
        assert_exact(B, p, oracle_ref("row", "bwd", p, base), ("row", p, ldg, mask_id(base)))


# ------------------------------------------------------------------------------ the launch order
@pytest.mark.parametrize("tree", (False, True), ids=("chain", "tree"))
@pytest.mark.parametrize("big", (False, True), ids=("256", "1024"))
def test_csc_order_changes_no_bit(pgcn, big, tree):
    """order = none, the engine's (descending column length, stable) and a seeded permutation:
    which workgroup takes which feature changes nothing"""
    L = ladder("col")
    engine = sc.engine_order(L["cp"])
    assert list(np.diff(L["cp"])[engine]) == sorted(sc.COL_LENGTHS, reverse=True)
    shuffled = np.random.default_rng(18).permutation(L["F"]).astype(np.int32)
    assert list(shuffled) != list(engine) and list(shuffled) != list(range(L["F"]))
    for p, ldg, base in ((41, 44, 37), (16, 16, None), (7, 7, 64 * 3 + 61)):
        outs = []
        for order in (None, engine, shuffled):
            st, B, paths, _ = call_bwd(pgcn, "col", p, ldg, base, big, order=order, tree=tree)
            assert st == pgcn.PGCN_OK and paths == only(bwd_path(big, tree))
            outs.append(B)
        assert same_bits(outs[0], outs[1]) and same_bits(outs[0], outs[2]), (p, ldg, base)
        if not tree:
            assert_exact(outs[2], p, oracle_ref("col", "bwd", p, base), (p, ldg, base))


# ------------------------------------------------------------------------------ CSC, the tree
@pytest.mark.parametrize("big", (False, True), ids=("256", "1024"))
@pytest.mark.parametrize("p,ldg", ((7, 7), (16, 16), (41, 44), (128, 128)))
def test_csc_tree_column_ladder(pgcn, p, ldg, big):
    """k_spmm_csc_tree on the ladder (spans of 0, 1, 2 .. 1024 threads, more than 4 CH entries
    in the 256-thread form): float64 within the reordering bound, the same bits again, and the
    chain kernel's bits on the columns of no and of one entry"""
    L = ladder("col")
    for base in (None, 37, 64 * 3 + 61):
        what = ("tree", p, ldg, "1024" if big else "256", mask_id(base))
        st, B, paths, launches = call_bwd(pgcn, "col", p, ldg, base, big, tree=True)
        assert st == pgcn.PGCN_OK and paths == only(bwd_path(big, True)) and launches == 1, what
        got, pad, guard = split(B, p)
        ref, bound = float64_ref("col", p, base)
        err = np.abs(got - ref)
        print(f"{what}: max err / bound {(err / (bound + 1e-30)).max():.3g}")
        assert (err <= 1e-5 * bound + 1e-30).all(), (what, (err / (bound + 1e-30)).max())
        assert np.isnan(pad).all() and np.isnan(guard).all(), what
        st2, B_again, _, _ = call_bwd(pgcn, "col", p, ldg, base, big, tree=True)
        assert st2 == pgcn.PGCN_OK and same_bits(B, B_again), what
        _, chain, _, _ = call_bwd(pgcn, "col", p, ldg, base, big)
        short = np.nonzero(L["col_len"] <= 1)[0]
        assert len(short) == 2
        np.testing.assert_array_equal(got[short].view(np.int32),
                                      split(chain, p)[0][short].view(np.int32), err_msg=str(what))


# ------------------------------------------------------------------------------ nothing to do
def test_no_rows_and_no_features(pgcn):
    """m = 0 and nf = 0: status 0, nothing launched, the NaN-filled outputs untouched"""
    for dual in (False, True):
        st, C, C2, paths, launches = call_fwd(pgcn, "row", 16, 16, 37, dual=dual, m=0)
        assert st == pgcn.PGCN_OK and paths == only(None) and launches == 0
        assert torch.isnan(C).all() and (C2 is None or torch.isnan(C2).all())
    for big in (False, True):
        for tree in (False, True):
            st, B, paths, launches = call_bwd(pgcn, "col", 16, 16, 37, big, tree=tree, nf=0)
            assert st == pgcn.PGCN_OK and paths == only(None) and launches == 0
            assert torch.isnan(B).all()


# ------------------------------------------------------------------------------ the engine
@pytest.mark.parametrize("tree", (0, 1), ids=("chain", "csc_tree"))
def test_engine_routing_cora(pgcn, loaded, tree):
    """What SparseMatmul launches on cora at the default knobs (train_ahead, sparse_dual):
    the first training forward is the single masked product; every eval(2) after a training
    epoch is the dual product, whose second output the next training forward swaps in without
    a launch; an eval that finds that output still waiting (eval(3) after eval(2)) is the single
    unmasked product.  One weight-gradient launch per epoch: 34 entries per feature, so the
    256-thread form -- the chain, or the tree under csc_tree."""
    ds = loaded["cora"]
    assert len(ds.feat_indices) <= 512 * ds.input_dim
    with helpers.knobs(pgcn, csc_tree=tree):
        g = pgcn.GCN(pgcn.make_params(ds), ds)
    bwd = "spmm_tree_256" if tree else "spmm_csc_256"
    want = dict.fromkeys(SPMM_PATHS, 0)
    pgcn.reset_path_counts()

    def step(call, **more):
        call()
        g.sync()
        for k, v in more.items():
            want[k] += v
        got = pgcn.path_counts()
        assert {k: got[k] for k in SPMM_PATHS} == want, (call, more)

    try:
        step(g.train_epoch, spmm_csr=1, **{bwd: 1})
        step(lambda: g.eval(2), spmm_csr_dual=1)
        step(g.train_epoch, **{bwd: 1})  # the forward: the dual product's second output
        step(lambda: g.eval(2), spmm_csr_dual=1)
        step(lambda: g.eval(3), spmm_csr=1)
        step(g.train_epoch, **{bwd: 1})
    finally:
        g.close()
    assert want == dict(only(None), spmm_csr=2, spmm_csr_dual=2, **{bwd: 3})
