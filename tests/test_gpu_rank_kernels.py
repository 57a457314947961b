"""The ranking kernels through the kernel ABI -- pgcn_link_rank_scores and pgcn_link_rank on a
pgcn_rank_queries handle -- against float64 numpy.  TQ, TC = pgcn_link_rank_tile().

The rank score is the k-ordered fp32 fmaf chain; the sweep computes it on the f32 MFMA, the
thresholds and the filter correction with fmaf loops, and all three must agree bit for bit:
  exact:       H on a grid where every partial sum is exact in fp32 (integers in [-8, 8] over 8;
               {-1, 0, 1} at d = 3, which forces many ties): any summation order gives the same
               bits, so the counts must equal the float64 model's, unfiltered and with filter lists.
  definition:  random normal H; pgcn_link_rank_scores against a numpy emulation of the chain, bit
               for bit, and the counts numpy derives from those device scores against
               pgcn_link_rank's, exactly: the MFMA sweep is the fused chain.
  float64:     the same data; with u = 2^-24 a candidate is decided when |s64(a, v) - s64(a, t)| >
               (d + 1) u (sum_c |H_a H_v| + sum_c |H_a H_t|) -- twice the chain's worst-case error,
               gamma_d < (d + 1) u for d <= 128 -- and the kernel must classify every decided
               candidate as float64 does: G_dec <= greater <= G_dec + U_e and equal <= U_e with
               U_e the query's undecided candidates.  Condition on the reference alone: at most
               0.1 % of all (query, candidate) pairs undecided.
  all filtered: F_e = every node but the target leaves both counts exactly 0 -- the bitwise
               agreement of the sweep and the correction pass.
Shapes: n in {TC - 1, TC, TC + 1, 2 TC + 5} and 9 TC + 7 (the first n with two candidate splits at
one query block), Q in {1, TQ - 1, TQ, TQ + 3}, widths 1, 3, 4, 17, 64, 127, 128, ld_h = d rounded
up to 4 plus 4 with NaN in the padding, sentinels behind the outputs.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WIDTHS = (1, 3, 4, 17, 64, 127, 128)
SENTINEL = 0xDEADBEEF


def _ld(d):
    return (d + 3) // 4 * 4 + 4


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _sync():
    import torch
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def tile(pgcn):
    return pgcn.link_rank_tile()


def padded(x):
    """[n][ld]: x in the d columns, NaN in the padding."""
    n, d = x.shape
    out = np.full((n, _ld(d)), np.nan, np.float32)
    out[:, :d] = x
    return out


def grid_input(n, d, seed):
    rng = np.random.default_rng(seed)
    if d == 3:
        return rng.integers(-1, 2, (n, d)).astype(np.float32)
    return (rng.integers(-8, 9, (n, d)) / 8.0).astype(np.float32)


def normal_input(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def queries(n, Q, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, Q).astype(np.int32), rng.integers(0, n, Q).astype(np.int32)


def random_filters(n, target, seed):
    """Per query a sorted list without its target: query 0 empty, query 1 every other node."""
    rng = np.random.default_rng(seed)
    lists = []
    for e, t in enumerate(target):
        if e == 0:
            f = np.zeros(0, np.int64)
        elif e == 1:
            f = np.arange(n)
        else:
            f = np.flatnonzero(rng.random(n) < rng.choice([0.02, 0.3, 0.9]))
        lists.append(f[f != t].astype(np.int32))
    ptr = np.r_[0, np.cumsum([f.size for f in lists])].astype(np.int64)
    return ptr, np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)


def mask_of(n, target, ptr=None, idx=None):
    m = np.ones((target.size, n), bool)
    m[np.arange(target.size), target] = False
    if ptr is not None:
        for e in range(target.size):
            m[e, idx[ptr[e]:ptr[e + 1]]] = False
    return m


def counts_from(S, target, mask):
    thr = S[np.arange(target.size), target][:, None]
    return ((S > thr) & mask).sum(1), ((S == thr) & mask).sum(1)


def rank(pgcn, n, anchor, target, Hd, d, ptr=None, idx=None, calls=1):
    """(greater, equal) of pgcn_link_rank, the last of `calls` calls; sentinels checked."""
    Q = anchor.size
    q = pgcn.RankQueries(n, anchor, target, ptr, idx)
    out = []
    for _ in range(calls):
        g = _dev(np.full(Q + 8, SENTINEL, np.uint32).view(np.int32))
        e = _dev(np.full(Q + 8, SENTINEL, np.uint32).view(np.int32))
        st = pgcn.lib.pgcn_link_rank(q.handle, _p(Hd), Hd.shape[1], d, _p(g), _p(e), None)
        assert st == pgcn.PGCN_OK
        _sync()
        g, e = g.cpu().numpy().view(np.uint32), e.cpu().numpy().view(np.uint32)
        assert (g[Q:] == SENTINEL).all() and (e[Q:] == SENTINEL).all()
        out.append((g[:Q].astype(np.int64), e[:Q].astype(np.int64)))
    q.close()
    for o in out[1:]:
        assert (o[0] == out[0][0]).all() and (o[1] == out[0][1]).all(), "two calls differ"
    return out[-1]


def device_scores(pgcn, Hd, d, src, dst):
    m = src.size
    s = _dev(np.full(m + 8, 7.25, np.float32))
    sd, dd = _dev(src.astype(np.int32)), _dev(dst.astype(np.int32))
    assert pgcn.lib.pgcn_link_rank_scores(_p(sd), _p(dd), m, _p(Hd), Hd.shape[1], d, _p(s),
                                          None) == pgcn.PGCN_OK
    _sync()
    s = s.cpu().numpy()
    assert (s[m:] == 7.25).all()
    return s[:m]


def all_pairs_scores(pgcn, Hd, d, anchor, n):
    src = np.repeat(anchor, n)
    dst = np.tile(np.arange(n, dtype=np.int32), anchor.size)
    return device_scores(pgcn, Hd, d, src, dst).reshape(anchor.size, n)


def shapes(tile):
    TQ, TC = tile
    return [(n, Q) for n in (TC - 1, TC, TC + 1, 2 * TC + 5) for Q in (1, TQ - 1, TQ, TQ + 3)]


@pytest.mark.parametrize("d", WIDTHS)
def test_exact_grid(pgcn, tile, d):
    for k, (n, Q) in enumerate(shapes(tile) + [(9 * tile[1] + 7, 5)]):
        x = grid_input(n, d, 100 + k)
        Hd = _dev(padded(x))
        anchor, target = queries(n, Q, 200 + k)
        S = x[anchor].astype(np.float64) @ x.astype(np.float64).T
        g, e = rank(pgcn, n, anchor, target, Hd, d)
        wg, we = counts_from(S, target, mask_of(n, target))
        assert (g == wg).all() and (e == we).all(), (n, Q, d)
        if d == 3:
            assert we.sum() > Q  # the ties are there
        ptr, idx = random_filters(n, target, 300 + k)
        g, e = rank(pgcn, n, anchor, target, Hd, d, ptr, idx)
        wg, we = counts_from(S, target, mask_of(n, target, ptr, idx))
        assert (g == wg).all() and (e == we).all(), (n, Q, d, "filtered")
        if Q > 1:
            assert g[1] == 0 and e[1] == 0


def chain_emulation(a, b):
    """The fp32 fmaf chain over the columns of a, b [m][d] in float64 arithmetic: a product of two
    floats is exact in float64, so one step rounds twice (to 53 bits, then to 24).  Returns the
    scores and the pairs where a step's float64 sum was inexact (two-sum's error term) and sat on a
    float32 rounding boundary: the only place double rounding can differ from a fused step."""
    s = np.zeros(a.shape[0], np.float32)
    hazard = np.zeros(a.shape[0], bool)
    for c in range(a.shape[1]):
        p, s64 = a[:, c].astype(np.float64) * b[:, c].astype(np.float64), s.astype(np.float64)
        x = p + s64
        bb = x - p
        err = (p - (x - bb)) + (s64 - bb)
        midpoint = (x.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
        hazard |= midpoint & (err != 0.0)
        s = x.astype(np.float32)
    return s, hazard


@pytest.mark.parametrize("d", WIDTHS)
def test_definition(pgcn, tile, d):
    TQ, TC = tile
    n, Q = 2 * TC + 5, TQ + 3
    x = normal_input(n, d, 40 + d)
    Hd = _dev(padded(x))
    anchor, target = queries(n, Q, 50 + d)
    S = all_pairs_scores(pgcn, Hd, d, anchor, n)
    want, hazard = chain_emulation(np.repeat(x[anchor], n, axis=0), np.tile(x, (Q, 1)))
    same = S.ravel().view(np.uint32) == want.view(np.uint32)
    assert hazard.mean() < 1e-6 and (same | hazard).all(), "scores are not the fmaf chain"
    g, e = rank(pgcn, n, anchor, target, Hd, d)
    wg, we = counts_from(S, target, mask_of(n, target))
    assert (g == wg).all() and (e == we).all()
    ptr, idx = random_filters(n, target, 60 + d)
    g, e = rank(pgcn, n, anchor, target, Hd, d, ptr, idx)
    wg, we = counts_from(S, target, mask_of(n, target, ptr, idx))
    assert (g == wg).all() and (e == we).all()


@pytest.mark.parametrize("d", WIDTHS)
def test_against_float64(pgcn, d):
    n, Q = 333, 130
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    anchor = rng.integers(0, n, Q).astype(np.int32)
    target = rng.integers(0, n, Q).astype(np.int32)
    a64, x64 = x[anchor].astype(np.float64), x.astype(np.float64)
    S = a64 @ x64.T
    A = np.abs(a64) @ np.abs(x64).T
    rows = np.arange(Q)
    thr, athr = S[rows, target][:, None], A[rows, target][:, None]
    mask = mask_of(n, target)
    decided = np.abs(S - thr) > (d + 1) * U * (A + athr)
    und = (~decided & mask).sum(1)
    print(f"d {d}: undecided share {und.sum() / (Q * n):.3g}")
    assert und.sum() <= 1e-3 * Q * n, "the reference leaves too many candidates undecided"
    g_dec = ((S > thr) & decided & mask).sum(1)
    g, e = rank(pgcn, n, anchor, target, _dev(padded(x)), d)
    assert (g >= g_dec).all() and (g <= g_dec + und).all() and (e <= und).all()


@pytest.mark.parametrize("d", (1, 4, 17, 128))
def test_every_node_filtered(pgcn, tile, d):
    TQ, TC = tile
    n, Q = 2 * TC + 5, TQ + 3
    x = normal_input(n, d, 70 + d)
    anchor, target = queries(n, Q, 80 + d)
    lists = [np.delete(np.arange(n, dtype=np.int32), t) for t in target]
    ptr = (np.arange(Q + 1, dtype=np.int64) * (n - 1))
    g, e = rank(pgcn, n, anchor, target, _dev(padded(x)), d, ptr, np.concatenate(lists))
    assert not g.any() and not e.any()


def test_target_is_anchor_and_duplicates(pgcn, tile):
    TQ, TC = tile
    n, d = TC + 1, 17
    x = normal_input(n, d, 90)
    anchor = np.array([3, 3, 7, 7, 3, n - 1], np.int32)
    target = np.array([3, 5, 7, 7, 3, n - 1], np.int32)
    Hd = _dev(padded(x))
    g, e = rank(pgcn, n, anchor, target, Hd, d)
    S = all_pairs_scores(pgcn, Hd, d, anchor, n)
    wg, we = counts_from(S, target, mask_of(n, target))
    assert (g == wg).all() and (e == we).all()
    assert (g[0], e[0]) == (g[4], e[4]) and (g[2], e[2]) == (g[3], e[3])


def test_determinism_and_launches(pgcn, tile):
    TQ, TC = tile
    n, Q, d = 9 * TC + 7, TQ + 3, 64
    x = normal_input(n, d, 95)
    anchor, target = queries(n, Q, 96)
    Hd = _dev(padded(x))
    ptr, idx = random_filters(n, target, 97)
    pgcn.reset_path_counts()
    rank(pgcn, n, anchor, target, Hd, d, calls=2)
    c = pgcn.path_counts(reset=True)
    assert c["rank_sweep"] == 2 and c["rank_filter"] == 0 and c["launches"] == 4
    rank(pgcn, n, anchor, target, Hd, d, ptr, idx, calls=2)
    c = pgcn.path_counts(reset=True)
    assert c["rank_sweep"] == 2 and c["rank_filter"] == 2 and c["launches"] == 6
    # no queries: nothing is launched
    q = pgcn.RankQueries(n, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert pgcn.lib.pgcn_link_rank(q.handle, _p(Hd), Hd.shape[1], d, None, None,
                                   None) == pgcn.PGCN_OK
    q.close()
    assert pgcn.path_counts(reset=True)["launches"] == 0


def test_argument_rules_on_device(pgcn):
    n, d = 10, 5
    Hd = _dev(padded(normal_input(n, d, 1)))
    q = pgcn.RankQueries(n, [1], [2])
    out = _dev(np.zeros(4, np.int32))
    bad = pgcn.PGCN_E_INVALID
    f = pgcn.lib.pgcn_link_rank
    assert f(q.handle, _p(Hd), Hd.shape[1], 0, _p(out), _p(out), None) == bad
    assert f(q.handle, _p(Hd), Hd.shape[1], 129, _p(out), _p(out), None) == bad
    assert f(q.handle, _p(Hd), 4, d, _p(out), _p(out), None) == bad
    assert f(q.handle, _p(Hd), 10, d, _p(out), _p(out), None) == bad
    assert f(q.handle, None, Hd.shape[1], d, _p(out), _p(out), None) == bad
    assert f(q.handle, _p(Hd), Hd.shape[1], d, None, _p(out), None) == bad
    assert f(q.handle, ctypes.c_void_p(Hd.data_ptr() + 4), Hd.shape[1], d, _p(out), _p(out),
             None) == bad
    q.close()
