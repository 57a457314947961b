"""Every kernel form the dense products dispatch to (csrc/k_gemm.hip, k_gemm_wide.hip), through
the C ABI, against float64.

pgcn_gemm (NN: C = drop(A) B) and pgcn_gemm_tn (TN: C = drop(A)^T G) pick a kernel family by
shape, and inside the family a template instantiation by a plan:

  gemm_nn    k_gemm_nn<NT>                 N <= 32 off the X-stream kernels      NT = ceil(N / 16)
  gemm_tn    k_gemm_tn<NJ, KCW, WK>        N <= 32, or G rows not 16-B aligned   tn_plan
  gemm_nn_w  k_gemm_nn_w<NT, TRANS_B, MK>  N in 33..128                          NT 3 | 4 | 8
             k_gemm_nn_wp<NT, TRANS_B, NCH>  ... no mask and K <= 128            NCH = ceil(K / 64)
  gemm_tn_w  k_gemm_tn_w<NH, WK, MK>       N in 33..128, G rows 16-B aligned     NH = 1 | 2
  xs_nn / xs_tn (and their _ring forms at K in 577..640)   N <= 16, K <= 640, no mask

(MK: 0 no dropout, 1 the flat bitmap, 2 the nibble layout, which only pgcn_debug_gemm_nib /
pgcn_debug_gemm_tn_nib can hand over.)  N > 128 runs in 128-column slabs, each on its own
family.  The plans are restated below (nn_forms, tn_forms); every case asserts the families it
launched through pgcn_debug_path_count, and test_every_listed_form_is_reached asserts that the
cases together reach every instantiation the four launchers list.

Every case: A's row padding is NaN, the operands' row padding too; the bitmap has exactly the
words its bits need; the output is NaN-filled with two guard rows above and below that must stay
NaN; seeds are fixed per shape; the TN workspace is NaN-filled.  Reference: float64 drop(A) B,
bound |got - ref| <= 1e-5 |drop(A)| |B| + 1e-30 per element (the bound of test_gemm_nn /
test_gemm_tn: fp32 reordering only).  A second call must repeat the first one's bits.
"""
import collections
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import helpers

DEV = "cuda"
GUARD = 2
SCALE = 2.0
GEMM_PATHS = ("gemm_nn", "gemm_tn", "gemm_nn_w", "gemm_tn_w", "xs_nn", "xs_tn", "xs_nn_ring",
              "xs_tn_ring")

Case = collections.namedtuple(
    "Case", "kind M N K mask base trans_b lda ldb ldc ldg mask_ld g_off",
    defaults=(None, 0, 0, None, None, None, None, None, 0))
# kind "nn" | "tn"; mask None | "flat" | "nib"; base: mask_base; lda / ldb / ldc / ldg /
# mask_ld: None = the tight ones (up4(K); N, or K when transposed; NN up4(N), TN N; N; K);
# g_off: floats G is offset by from a 16-byte aligned address


def up4(x):
    return (x + 3) // 4 * 4


def cdiv(a, b):
    return -(-a // b)


def strides(c):
    lda = up4(c.K) if c.lda is None else c.lda
    ldb = (c.K if c.trans_b else c.N) if c.ldb is None else c.ldb
    ldc = (up4(c.N) if c.kind == "nn" else c.N) if c.ldc is None else c.ldc
    ldg = c.N if c.ldg is None else c.ldg
    mask_ld = c.K if c.mask_ld is None else c.mask_ld
    return lda, ldb, ldc, ldg, mask_ld


# ------------------------------------------------------------------------------ the plans
def xs_ok(N, K):  # xstream_ok
    return 1 <= N <= 16 and 1 <= K <= 640


def xs_ring(K, lda):  # xstream_ring_ok at the default knobs
    return 576 < K <= 640 and lda == up4(K)


def col_slabs(N, ldc):
    """(columns, nst) of the launches: 128-column slabs above 128 (launch_gemm_nn / _tn)"""
    if N <= 128:
        return [(N, ldc)]
    return [(min(128, N - j0), ldc - j0 if j0 + 128 >= N else 128) for j0 in range(0, N, 128)]


def tn_plan(N, K):
    """k_gemm_tn<NJ, KCW, WK> of tn_plan: WK waves along K take KCW 64-wide chunks each; one and
    two waves along K (up to three chunks) keep one chunk per wave, more k-groups instead"""
    nj, nkc = cdiv(N, 16), cdiv(K, 64)
    wk = 4 if nkc >= 4 else (2 if nkc >= 2 else 1)
    kcw = min(3, cdiv(nkc, wk)) if wk == 4 and nj <= 4 else 1
    return nj, kcw, wk


def tn_slabs(M, wk):
    """row slabs of tn_plan (two row steps in flight per wave)"""
    q = 4 * (4 // wk) * 2
    slab = max(64, cdiv(cdiv(M, 1024), q) * q)
    return max(1, cdiv(M, slab))


def nn_forms(c):
    """[(family, form)] of the launches of an NN case"""
    lda, _, ldc, _, _ = strides(c)
    out = []
    for n, nst in col_slabs(c.N, ldc) if c.M > 0 else []:
        if not c.mask and xs_ok(n, c.K) and nst == ldc:
            out.append(("xs_nn_ring" if xs_ring(c.K, lda) else "xs_nn", ("xs_nn", cdiv(c.K, 64))))
        elif 33 <= n <= 128:
            nt = cdiv(n, 16)
            t = 3 if nt <= 3 else (4 if nt == 4 else 8)
            if not c.mask and c.K <= 128:
                out.append(("gemm_nn_w", ("nn_wp", t, c.trans_b, cdiv(c.K, 64))))
            else:
                mk = 0 if not c.mask else (2 if c.mask == "nib" and c.K <= 1024 else 1)
                out.append(("gemm_nn_w", ("nn_w", t, c.trans_b, mk)))
        else:
            out.append(("gemm_nn", ("nn", cdiv(n, 16))))
    return out


def tn_forms(c):
    """[(family, form)] of the launches of a TN case"""
    lda, _, ldc, ldg, _ = strides(c)
    out = []
    for n, nst in col_slabs(c.N, ldc) if c.M > 0 else []:
        if not c.mask and xs_ok(n, c.K) and nst == ldc:
            out.append(("xs_tn_ring" if xs_ring(c.K, lda) else "xs_tn", ("xs_tn", cdiv(c.K, 64))))
        elif 33 <= n <= 128 and ldg % 4 == 0 and c.g_off % 4 == 0:
            mk = 0 if not c.mask else (2 if c.mask == "nib" and c.K <= 1024 else 1)
            out.append(("gemm_tn_w", ("tn_w", 1 if n <= 64 else 2, 2 if c.K > 64 else 1, mk)))
        else:
            out.append(("gemm_tn", ("tn",) + tn_plan(n, c.K)))
    return out


def forms(c):
    return nn_forms(c) if c.kind == "nn" else tn_forms(c)


# what the launchers list (gemm_nn_slab, gemm_tn_slab, launch_gemm_nn_wide, launch_gemm_tn_wide)
LISTED = set(
    [("nn", nt) for nt in (1, 2)] +
    [("tn", nj, kcw, wk) for nj in (1, 2, 3, 4) for kcw, wk in
     ((1, 1), (1, 2), (1, 4), (2, 4), (3, 4))] +
    [("tn", nj, 1, wk) for nj in (5, 6, 7, 8) for wk in (1, 2, 4)] +
    [("nn_w", t, d, mk) for t in (3, 4, 8) for d in (0, 1) for mk in (0, 1, 2)] +
    [("nn_wp", t, d, nch) for t in (3, 4, 8) for d in (0, 1) for nch in (1, 2)] +
    [("tn_w", nh, wk, mk) for nh in (1, 2) for wk in (1, 2) for mk in (0, 1, 2)])


def case_id(c):
    lda, ldb, ldc, ldg, mask_ld = strides(c)
    s = f"{c.kind}-M{c.M}-N{c.N}-K{c.K}"
    if c.mask:
        s += f"-{c.mask}{c.base}"
    if c.trans_b:
        s += "-Bt"
    loose = [f"{k}{v}" for k, v in (("lda", c.lda), ("ldb", c.ldb), ("ldc", c.ldc),
                                     ("ldg", c.ldg), ("mld", c.mask_ld)) if v is not None]
    if c.g_off:
        loose.append(f"goff{c.g_off}")
    s += "".join("-" + x for x in loose)
    fs = sorted({"".join(str(x) + "." for x in f)[:-1] for _, f in forms(c)})
    return s + "-" + "+".join(fs) if fs else s + "-none"


# ------------------------------------------------------------------------------ the cases
MASKS3 = [(None, 0), ("flat", 0), ("flat", 61)]  # base 61: a 4-bit read straddles a word

# Generic TN k_gemm_tn<NJ, KCW, WK>.  N = 16 NJ - 3 gives NJ; K gives the chunk count and with it
# (KCW, WK) for NJ <= 4 (KCW = 1 for NJ >= 5):
#   K    40     100    160    192    200    300    512    602
#   nkc  1      2      3      3      4      5      8      10
#        (1,1)  (1,2)  (1,2)  (1,2)  (1,4)  (2,4)  (2,4)  (3,4)     three chunks: two k-groups
TN_KS = (40, 100, 160, 192, 200, 300, 512, 602)
TN_GENERIC = []
for _nj, _k in itertools.product(range(1, 9), TN_KS):
    _n = 16 * _nj - 3
    for _mask, _base in MASKS3:
        if _nj >= 3:  # the wide kernel refused: G rows off the 16-byte grid, either way
            TN_GENERIC.append(Case("tn", 70, _n, _k, _mask, _base, ldg=up4(_n) + 1))
            TN_GENERIC.append(Case("tn", 70, _n, _k, _mask, _base, ldg=up4(_n), g_off=1))
        elif _nj == 2 or _mask:  # N = 13 without a mask is the X-stream kernels'
            TN_GENERIC.append(Case("tn", 70, _n, _k, _mask, _base))
TN_GENERIC += [Case("tn", 70, 17, _k, _m, _b) for _k in (160, 192) for _m, _b in MASKS3]
TN_GENERIC += [
    Case("tn", 70, 29, 1433, "flat", 61),          # (2,3,4): 23 chunks, two k-groups of 12
    Case("tn", 70, 77, 1433, None, ldg=81),        # (5,1,4): six k-groups
]
# 16 row slabs of 64: one ordered pass; 17 and 18: two passes (groups of 16 slabs, then the groups)
for _m in (1024, 1025, 1100):
    TN_GENERIC += [Case("tn", _m, 29, 100, "flat", 61),      # (2,1,2)
                   Case("tn", _m, 77, 300, None, ldg=81)]    # (5,1,4), two k-groups
# no rows: C comes back all zero (no kernel of the family runs, the reduce writes zeros)
TN_GENERIC += [Case("tn", 0, 29, 100), Case("tn", 0, 13, 100), Case("tn", 0, 77, 100)]

# Wide TN k_gemm_tn_w<NH, WK, MK>: N 33..64 -> NH 1, 65..128 -> NH 2; K 40 -> WK 1, 100 -> WK 2
# (one k-group), 300 -> WK 2 (three k-groups); M 200: 4 slabs, 1100: 18 (two reduce passes)
TN_WIDE = [Case("tn", _m, _n, _k, _mask, 61 if _mask else 0, ldg=up4(_n))
           for _m in (200, 1100) for _n in (33, 40, 64, 65, 128) for _k in (40, 100, 300)
           for _mask in (None, "flat", "nib")]

# Wide NN: N 33, 48 -> NT 3; 49, 64 -> NT 4; 65, 80, 128 -> NT 8.
#   no mask, K 40 / 100, 128      k_gemm_nn_wp NCH 1 / 2 (B stays in LDS)
#   no mask, K 129, 300           k_gemm_nn_w MK 0
#   flat mask, K 40, 300          MK 1
#   nibbles, K 40, 300            MK 2
# M 1, 127, 128, 129: the 128-row tile's edges; 300: three tiles
NN_WIDE = [Case("nn", _m, _n, _k, _mask, 61 if _mask else 0, _d)
           for _m in (1, 127, 128, 129, 300) for _n in (33, 48, 49, 64, 65, 80, 128)
           for _d in (0, 1)
           for _k, _mask in ((40, None), (100, None), (128, None), (129, None), (300, None),
                             (40, "flat"), (300, "flat"), (40, "nib"), (300, "nib"))]
# 516 row tiles over the persistent kernel's 512 workgroups: the walk's second trip
NN_WIDE.append(Case("nn", 66000, 40, 16))

# Generic NN k_gemm_nn<NT>: N <= 16 with a mask, or past the X-stream kernels' K (NT 1);
# N 17..32 (NT 2).  M 1, 63, 64, 65: the 64-row block's edges; 300: five blocks
NN_GENERIC = [Case("nn", _m, _n, _k, _mask, _base, _d)
              for _m in (1, 63, 64, 65, 300) for _d in (0, 1)
              for _n, _k, _mask, _base in (
                  (1, 40, "flat", 0), (13, 100, "flat", 61), (16, 40, "flat", 61),
                  (16, 100, "flat", 0), (16, 700, None, 0), (17, 40, None, 0),
                  (17, 100, "flat", 61), (32, 100, None, 0), (32, 40, "flat", 61))]
NN_GENERIC.append(Case("nn", 0, 29, 100))  # no rows: nothing launched, nothing written

# Above 128 columns: 128-column slabs, the last one 1, 16, 32, 33 or 1 columns wide and
# writing C's padding columns too (nst != ldc: the general or the wide kernel, never X-stream)
SLABS = [Case(_kind, 300, _n, 72, _mask, 61 if _mask else 0, ldc=_ldc(_n))
         for _kind in ("nn", "tn") for _n in (129, 144, 160, 161, 257)
         for _mask in (None, "flat")
         for _ldc in (up4, (lambda n: up4(n) + 8))]
SLABS += [Case("nn", 300, 161, 72, None, 0, 1), Case("nn", 300, 257, 72, "flat", 61, 1)]

# Every stride loose at once and all different, one shape per family
def _loose(kind, M, N, K, mask=None, base=0, trans_b=0):
    return Case(kind, M, N, K, mask, base, trans_b, lda=up4(K) + 8,
                ldb=(K if trans_b else N) + 4, ldc=(up4(N) + 8) if kind == "nn" else N + 4,
                ldg=up4(N) + 12, mask_ld=K + 5)


LOOSE = [_loose("nn", 150, 29, 100, "flat", 61, _d) for _d in (0, 1)]           # gemm_nn
LOOSE += [_loose("nn", 150, 13, 100, None, 0, _d) for _d in (0, 1)]             # xs_nn
LOOSE += [_loose("nn", 150, 77, _k, _mask, 61 if _mask else 0, _d)              # gemm_nn_w
          for _d in (0, 1) for _k, _mask in ((100, None), (300, None), (100, "flat"),
                                             (100, "nib"))]
LOOSE += [_loose("nn", 150, 161, 100, "flat", 61, _d) for _d in (0, 1)]         # slabs
LOOSE += [_loose("tn", 150, 29, 100, "flat", 61)]                               # gemm_tn
LOOSE += [_loose("tn", 150, 13, 100)]                                           # xs_tn
LOOSE += [_loose("tn", 150, 77, 100, _mask, 61 if _mask else 0)                 # gemm_tn_w
          for _mask in (None, "flat", "nib")]
LOOSE += [_loose("tn", 150, 161, 100, "flat", 61)]                              # slabs

# Boundaries of every plan at M = 70: the chunk counts' edges (64 k), the persistent kernel's
# (128), the X-stream kernels' (576 / 640), the nibble layout's (1024), and the first Ks
SWEEP_KS = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 511, 512, 513,
            576, 577, 640, 641, 1023, 1024, 1025)
SWEEP_NS = (16, 17, 32, 33, 64, 65, 128)
SWEEP = {(_kind, _n, _mask): [Case(_kind, 70, _n, _k, _mask, 61 if _mask else 0,
                                   ldg=up4(_n) if _kind == "tn" else None)
                              for _k in SWEEP_KS]
         for _kind in ("nn", "tn") for _n in SWEEP_NS for _mask in (None, "flat")}

# at K > 1024 the wide kernels ignore the nibbles (the flat bitmap's kernel runs)
NIB_IGNORED = [Case("nn", 150, 77, 1030, "nib", 61), Case("tn", 150, 77, 1030, "nib", 61,
                                                          ldg=80)]

ALL_CASES = (TN_GENERIC + TN_WIDE + NN_WIDE + NN_GENERIC + SLABS + LOOSE + NIB_IGNORED +
             [c for cs in SWEEP.values() for c in cs])


# ------------------------------------------------------------------------------ the runner
def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def padded(x, ld):
    """x's rows at stride ld, the padding NaN"""
    out = np.full((x.shape[0], ld), np.nan, np.float32)
    out[:, :x.shape[1]] = x
    return out


@functools.lru_cache(maxsize=4)
def problem(M, N, K, base, mask_ld):
    """Host operands and the float64 references of one shape (shared by the cases on it; the
    arrays are read-only)."""
    rng = np.random.default_rng([M, N, K, base, mask_ld])
    A = rng.standard_normal((M, K)).astype(np.float32)
    B = rng.standard_normal((K, N)).astype(np.float32)
    G = rng.standard_normal((M, N)).astype(np.float32)
    bits = base + (M - 1) * mask_ld + K if M else base + 1
    mask = rng.integers(0, 2**64, cdiv(bits, 64), dtype=np.uint64)  # exactly the words needed
    keep = helpers.mask_window(mask, base, M, K, mask_ld)
    refs = {}
    for drop in (False, True):
        Ae = helpers.dropped64(A, K, keep if drop else None, SCALE)
        refs["nn", drop] = helpers.product_ref(Ae, B)
        refs["tn", drop] = helpers.product_ref(Ae.T, G)
    for a in (A, B, G, mask, keep) + tuple(x for r in refs.values() for x in r):
        a.setflags(write=False)
    return dict(A=A, B=B, G=G, mask=mask, refs=refs)


def call(pgcn, c, dev, nib_entry):
    """One call of the case into a fresh NaN-filled output with guard rows; returns (status, the
    whole output buffer)."""
    lda, ldb, ldc, ldg, mask_ld = strides(c)
    rows = c.M if c.kind == "nn" else c.K
    C = torch.full((rows + 2 * GUARD, ldc), float("nan"), device=DEV)
    Cp = ctypes.c_void_p(C.data_ptr() + 4 * GUARD * ldc)
    m = vp(dev["mask"]) if c.mask else None
    lib = pgcn.lib
    if c.kind == "nn":
        args = (c.M, c.N, c.K, vp(dev["A"]), lda, vp(dev["B"]), ldb, c.trans_b, Cp, ldc, m,
                c.base, mask_ld, SCALE)
        if nib_entry:
            st = lib.pgcn_debug_gemm_nib(*args, vp(dev["nib"]), stream())
        else:
            st = lib.pgcn_gemm(*args, stream())
    else:
        dev["ws"].fill_(float("nan"))
        args = (c.M, c.N, c.K, vp(dev["A"]), lda, vp(dev["G"]), ldg, Cp, ldc, m, c.base,
                mask_ld, SCALE)
        if nib_entry:
            st = lib.pgcn_debug_gemm_tn_nib(*args, vp(dev["nib"]), vp(dev["ws"]), stream())
        else:
            st = lib.pgcn_gemm_tn(*args, vp(dev["ws"]), stream())
    torch.cuda.synchronize()
    return st, C


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def operands(pgcn, c):
    """(the shape's host problem, the case's device operands at its strides)"""
    lda, ldb, ldc, ldg, mask_ld = strides(c)
    P = problem(c.M, c.N, c.K, c.base, mask_ld)
    rows1 = max(c.M, 1)  # no rows: the pointers must still be valid
    A = np.full((rows1, lda), np.nan, np.float32)
    A[:c.M, :c.K] = P["A"]
    dev = {"A": torch.from_numpy(A).to(DEV),
           "mask": torch.from_numpy(P["mask"].view(np.int64).copy()).to(DEV)}
    if c.kind == "nn":
        B = np.ascontiguousarray(P["B"].T) if c.trans_b else P["B"]
        dev["B"] = torch.from_numpy(padded(B, ldb)).to(DEV)
    else:
        G = np.full((rows1, ldg), np.nan, np.float32)
        G[:c.M, :c.N] = P["G"]
        flat = torch.full((rows1 * ldg + 4,), float("nan"), device=DEV)
        flat[c.g_off:c.g_off + rows1 * ldg] = torch.from_numpy(G.reshape(-1)).to(DEV)
        dev["G"] = flat[c.g_off:]
        assert dev["G"].data_ptr() % 16 == 4 * c.g_off
        dev["ws"] = torch.empty(pgcn.lib.pgcn_gemm_tn_workspace(c.M, c.N, c.K) // 4 + 16,
                                device=DEV)
    if c.mask == "nib":
        if c.K <= 1024:
            nib = helpers.nibble_mask_ref(P["mask"], c.base, c.M, c.K, mask_ld)
        else:  # ignored: nibbles that would drop everything
            nib = np.zeros((c.M, 16), np.uint64)
        dev["nib"] = torch.from_numpy(nib.view(np.int64)).to(DEV)
    return P, dev


def run_case(pgcn, c):
    """Runs the case, asserts the status, the families launched, the reference bound, the
    padding columns and the guard rows, that a second call repeats the bits and (nibble cases)
    that the flat bitmap's call gives the same bits.  Returns the output buffer."""
    P, dev = operands(pgcn, c)
    pgcn.reset_path_counts()
    st, C = call(pgcn, c, dev, c.mask == "nib")
    paths = pgcn.path_counts()
    assert st == pgcn.PGCN_OK, (case_id(c), st)
    want = collections.Counter(fam for fam, _ in forms(c))
    assert {k: paths[k] for k in GEMM_PATHS} == {k: want[k] for k in GEMM_PATHS}, case_id(c)
    ref, bound = P["refs"][c.kind, bool(c.mask)]
    o = C.cpu().numpy()
    body = o[GUARD:len(o) - GUARD]
    err = np.abs(body[:, :c.N] - ref)
    print(f"{case_id(c)}: max err / bound {(err / (bound + 1e-30)).max(initial=0.0):.3g}")
    assert (err <= 1e-5 * bound + 1e-30).all(), (case_id(c), (err / (bound + 1e-30)).max())
    if c.kind == "nn":  # C's own padding columns are zero (test_gemm_nn pins the same)
        np.testing.assert_array_equal(body[:, c.N:up4(c.N)], 0.0)
    rest = body[:, up4(c.N) if c.kind == "nn" else c.N:]
    # further columns: the 16-column tiles write zeros as far as they reach, the NaN fill stays
    assert (np.isnan(rest) | (rest == 0.0)).all(), case_id(c)
    assert np.isnan(o[:GUARD]).all() and np.isnan(o[len(o) - GUARD:]).all(), case_id(c)
    st2, C2 = call(pgcn, c, dev, c.mask == "nib")
    assert st2 == pgcn.PGCN_OK and same_bits(C, C2), case_id(c)
    if c.mask == "nib":
        # the same kernel template and MFMA order; only where the four keep bits are read differs
        st3, C3 = call(pgcn, c, dev, False)
        assert st3 == pgcn.PGCN_OK and same_bits(C, C3), case_id(c)
    return C


def params(cases):
    return [pytest.param(c, id=case_id(c)) for c in cases]


# ------------------------------------------------------------------------------ CPU: the table
def test_every_listed_form_is_reached():
    """The parametrised shapes reach, by the plans restated above, every instantiation the
    launchers list (and the plans give nothing the launchers do not list)."""
    reached = {f for c in ALL_CASES for _, f in forms(c) if f[0] not in ("xs_nn", "xs_tn")}
    assert reached - LISTED == set(), sorted(reached - LISTED)
    assert LISTED - reached == set(), sorted(LISTED - reached)
    assert len(LISTED) == 2 + 32 + 18 + 12 + 12
    fams = {fam for c in ALL_CASES for fam, _ in forms(c)}
    assert fams == set(GEMM_PATHS)


def test_tn_plan_lists_every_shape():
    """tn_plan over N 1..128, K 1..1999 gives listed forms only (three chunks once did not)."""
    listed = {f[1:] for f in LISTED if f[0] == "tn"}
    bad = [(n, k) for n in range(1, 129) for k in range(1, 2000, 7)
           if tn_plan(n, k) not in listed]
    bad += [(n, k) for n in (1, 17, 32, 64) for k in range(1, 2000) if tn_plan(n, k) not in listed]
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------ GPU
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("c", params(TN_GENERIC))
def test_tn_generic(pgcn, c):
    C = run_case(pgcn, c)
    if c.M == 0:
        assert (C[GUARD:GUARD + c.K] == 0).all()


@gpu
@pytest.mark.parametrize("c", params(TN_WIDE))
def test_tn_wide(pgcn, c):
    run_case(pgcn, c)


@gpu
@pytest.mark.parametrize("c", params(NN_WIDE))
def test_nn_wide(pgcn, c):
    run_case(pgcn, c)


@gpu
@pytest.mark.parametrize("c", params(NN_GENERIC))
def test_nn_generic(pgcn, c):
    run_case(pgcn, c)


@gpu
@pytest.mark.parametrize("c", params(SLABS))
def test_column_slabs(pgcn, c):
    run_case(pgcn, c)


@gpu
@pytest.mark.parametrize("c", params(LOOSE))
def test_loose_strides(pgcn, c):
    run_case(pgcn, c)


@gpu
@pytest.mark.parametrize("c", params(NIB_IGNORED))
def test_nibbles_ignored_past_1024(pgcn, c):
    run_case(pgcn, c)


@gpu
@pytest.mark.parametrize("kind,N,mask", sorted(SWEEP, key=str),
                         ids=[f"{k}-N{n}-{m}" for k, n, m in sorted(SWEEP, key=str)])
def test_boundary_sweep(pgcn, kind, N, mask):
    """Every K at a plan's edge returns PGCN_OK and meets the bound."""
    for c in SWEEP[kind, N, mask]:
        run_case(pgcn, c)


def test_tn_workspace_three_chunks(pgcn):
    """pgcn_gemm_tn_workspace does not depend on how the chunks are dealt to waves: slabs plus
    first-pass groups of [K][16 NJ] partials, at three chunks as elsewhere."""
    for N, K, M in itertools.product((17, 24, 32), (100, 129, 160, 192, 200), (70, 1100, 70000)):
        nj, _, wk = tn_plan(N, K)
        n_slabs = tn_slabs(M, wk)
        want = (n_slabs + cdiv(n_slabs, 16)) * K * 16 * nj * 4
        assert pgcn.lib.pgcn_gemm_tn_workspace(M, N, K) == want, (M, N, K)
