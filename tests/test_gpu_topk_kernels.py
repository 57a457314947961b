"""The top-K retrieval kernels through the kernel ABI -- pgcn_link_topk on a pgcn_topk_queries
handle -- against the numpy model of tests/topk_ref.py.  TQ, TC, KMAX = pgcn_link_topk_tile().

The score is the rank score (the k-ordered fp32 fmaf chain, computed on the f32 MFMA) and the order
"higher score, then lower index" is total, so the answer is unique and every comparison is ==:
  exact grid:  H on a grid where every partial sum is exact in fp32 (integers in [-8, 8] over 8;
               {-1, 0, 1} at d = 3, which forces heavy ties): idx and score equal the float64
               model's, without lists and with them (query 0 empty, query 1 every node -- all
               padding --, the rest at densities 0.02 / 0.3 / 0.9).
  all ties:    H all ones: the k smallest non-excluded indices, across the split boundary.
  monotone:    d = 1, scores ascending in v (H[v] = v, anchor 1: every candidate passes the
               threshold, a prune in nearly every tile) and descending (H[v] = 1 - v, anchor 0, whose
               own row is +1; H[v] = -v with anchor 1, read literally, ascends again and is run too).
  definition:  random normal H; numpy's top-K over the device scores of pgcn_link_rank_scores for
               every (a, v) equals the kernel's idx exactly and its scores by value, and those
               scores are the chain emulation's bit for bit, up to the sign of a zero.
  float64:     B(a, v) = (d + 1) 2^-24 sum_c |H_a H_v| bounds the chain's error (gamma_d < (d + 1) u
               for d <= 128): every returned score is within B(a, v) of the float64 dot, and every
               candidate w not returned has s64(a, w) <= s64(a, v_last) + B(a, w) + B(a, v_last).
               No case is left out.
Shapes: n in {TC - 1, TC, TC + 1, 2 TC + 5} and n2 = the smallest j TC + 7 with two candidate splits
at one query block, Q in {1, TQ - 1, TQ, TQ + 3}, k in {1, 2, 10, 63, 64, 65, 128}, widths 1, 3, 4,
17, 64, 127, 128 -- a covering selection; ld_h = d rounded up to 4 plus 4 with NaN in the padding,
sentinels behind both outputs.
"""
import ctypes

import numpy as np
import pytest

import topk_ref

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
WIDTHS = (1, 3, 4, 17, 64, 127, 128)
SENT_I, SENT_S = -77, 7.25


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
    return pgcn.link_topk_tile()


def n_two_splits(pgcn, tile):
    TQ, TC, _ = tile
    n2 = next(j * TC + 7 for j in range(1, 65) if pgcn.link_topk_splits(TQ, j * TC + 7) >= 2)
    assert n2 <= 4096 + 7
    return n2


def resolve(pgcn, tile, n, Q):
    TQ, TC, _ = tile
    ns = {"TC-1": TC - 1, "TC": TC, "TC+1": TC + 1, "2TC+5": 2 * TC + 5}
    qs = {"1": 1, "TQ-1": TQ - 1, "TQ": TQ, "TQ+3": TQ + 3}
    return (n_two_splits(pgcn, tile) if n == "n2" else ns[n]), qs[Q]


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


def random_lists(n, Q, seed):
    """Per query a sorted exclude list: query 0 empty, query 1 every node."""
    rng = np.random.default_rng(seed)
    lists = []
    for e in range(Q):
        if e == 0:
            f = np.zeros(0, np.int64)
        elif e == 1:
            f = np.arange(n)
        else:
            f = np.flatnonzero(rng.random(n) < rng.choice([0.02, 0.3, 0.9]))
        lists.append(f.astype(np.int32))
    ptr = np.r_[0, np.cumsum([f.size for f in lists])].astype(np.int64)
    return ptr, np.concatenate(lists).astype(np.int32)


def topk(pgcn, n, anchor, Hd, d, k, ptr=None, idx=None, calls=1):
    """(idx [Q][k], score [Q][k]) of pgcn_link_topk, the last of `calls` calls on one handle;
    sentinels behind both outputs checked, the calls' bits compared."""
    Q = anchor.size
    q = pgcn.TopKQueries(n, anchor, ptr, idx, k=k)
    assert q.workspace >= Q * k * 8
    out = []
    for _ in range(calls):
        di = _dev(np.full(Q * k + 8, SENT_I, np.int32))
        ds = _dev(np.full(Q * k + 8, SENT_S, np.float32))
        st = pgcn.lib.pgcn_link_topk(q.handle, _p(Hd), Hd.shape[1], d, _p(di), _p(ds), None)
        assert st == pgcn.PGCN_OK
        _sync()
        hi, hs = di.cpu().numpy(), ds.cpu().numpy()
        assert (hi[Q * k:] == SENT_I).all() and (hs[Q * k:] == SENT_S).all()
        out.append((hi[:Q * k].reshape(Q, k), hs[:Q * k].reshape(Q, k)))
    q.close()
    for o in out[1:]:
        assert (o[0] == out[0][0]).all(), "two calls differ"
        assert (o[1].view(np.uint32) == out[0][1].view(np.uint32)).all(), "two calls differ"
    return out[-1]


def check(got, want, what):
    gi, gs = got
    wi, ws = want
    assert (gi == wi).all(), (what, np.argwhere(gi != wi)[:5].tolist())
    assert (gs.astype(np.float64) == ws.astype(np.float64)).all(), what


CASES = [("TC-1", "1", 1, 1), ("TC", "TQ-1", 2, 3), ("TC+1", "TQ", 10, 4),
         ("2TC+5", "TQ+3", 63, 17), ("TC-1", "TQ+3", 64, 64), ("2TC+5", "1", 65, 127),
         ("TC+1", "TQ-1", 128, 128), ("2TC+5", "TQ", 128, 4), ("n2", "TQ+3", 1, 3),
         ("n2", "TQ+3", 10, 64), ("n2", "TQ+3", 128, 128), ("n2", "TQ+3", 65, 17),
         ("n2", "TQ+3", 64, 1), ("n2", "TQ", 2, 127)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_exact_grid(pgcn, tile, case):
    n_key, q_key, k, d = CASES[case]
    n, Q = resolve(pgcn, tile, n_key, q_key)
    x = grid_input(n, d, 100 + case)
    Hd = _dev(padded(x))
    anchor = np.random.default_rng(200 + case).integers(0, n, Q).astype(np.int32)
    S = x[anchor].astype(np.float64) @ x.astype(np.float64).T
    check(topk(pgcn, n, anchor, Hd, d, k), topk_ref.topk_model(S, k), (CASES[case], "plain"))
    if d == 3:  # the ties are there: the k-th and the (k + 1)-th candidate share a score
        full = topk_ref.topk_model(S, min(k + 1, n))[1]
        assert k + 1 > n or (full[:, k - 1] == full[:, k]).any()
    ptr, idx = random_lists(n, Q, 300 + case)
    got = topk(pgcn, n, anchor, Hd, d, k, ptr, idx)
    check(got, topk_ref.topk_model(S, k, ptr, idx), (CASES[case], "lists"))
    assert got[0][0, 0] >= 0
    if Q > 1:
        assert (got[0][1] == -1).all() and np.isneginf(got[1][1]).all()


@pytest.mark.parametrize("k", (1, 10, 128))
def test_all_ties(pgcn, tile, k):
    TQ, TC, _ = tile
    n, Q, d = n_two_splits(pgcn, tile), TQ + 3, 4
    x = np.ones((n, d), np.float32)
    Hd = _dev(padded(x))
    anchor = np.random.default_rng(k).integers(0, n, Q).astype(np.int32)
    gi, gs = topk(pgcn, n, anchor, Hd, d, k)
    assert (gi == np.arange(k)[None, :]).all() and (gs == d).all()
    ptr, idx = random_lists(n, Q, 400 + k)
    got = topk(pgcn, n, anchor, Hd, d, k, ptr, idx)
    want = topk_ref.topk_model(np.full((Q, n), float(d)), k, ptr, idx)
    check(got, want, "all ties with lists")
    tiles = -(-n // TC)
    boundary = -(-tiles // pgcn.link_topk_splits(Q, n)) * TC    # the second split's first candidate
    if k == 128:  # the dense lists push the k smallest survivors across the split boundary
        rows = (got[0] >= boundary).any(1) & (got[0][:, 0] < boundary) & (got[0][:, 0] >= 0)
        assert rows.any()


@pytest.mark.parametrize("k", (1, 65, 128))
@pytest.mark.parametrize("form", ("ascending", "descending", "negated"))
def test_monotone_scores(pgcn, tile, form, k):
    TQ, _, _ = tile
    n = n_two_splits(pgcn, tile)
    v = np.arange(n, dtype=np.float32)
    h, a = {"ascending": (v, 1), "descending": (1 - v, 0), "negated": (-v, 1)}[form]
    x = h[:, None].astype(np.float32)
    anchor = np.full(TQ + 3, a, np.int32)
    S = x[anchor].astype(np.float64) @ x.astype(np.float64).T
    want = topk_ref.topk_model(S, k)
    assert want[0][0, 0] == (0 if form == "descending" else n - 1)
    check(topk(pgcn, n, anchor, _dev(padded(x)), 1, k), want, form)
    ptr, idx = random_lists(n, anchor.size, 500 + k)
    check(topk(pgcn, n, anchor, _dev(padded(x)), 1, k, ptr, idx),
          topk_ref.topk_model(S, k, ptr, idx), form + " with lists")


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


@pytest.mark.parametrize("d", WIDTHS)
def test_definition(pgcn, tile, d):
    TQ, TC, _ = tile
    n, Q = n_two_splits(pgcn, tile), TQ + 3
    k = 10 if d % 2 else 128
    x = normal_input(n, d, 40 + d)
    Hd = _dev(padded(x))
    anchor = np.random.default_rng(50 + d).integers(0, n, Q).astype(np.int32)
    S = all_pairs_scores(pgcn, Hd, d, anchor, n)
    want, hazard = topk_ref.chain_emulation(np.repeat(x[anchor], n, axis=0), np.tile(x, (Q, 1)))
    same = (S.ravel().view(np.uint32) == want.view(np.uint32)) | \
        ((S.ravel() == 0.0) & (want == 0.0))
    assert hazard.mean() < 1e-6 and (same | hazard).all(), "scores are not the fmaf chain"
    check(topk(pgcn, n, anchor, Hd, d, k), topk_ref.topk_model(S, k), "definition")
    ptr, idx = random_lists(n, Q, 60 + d)
    check(topk(pgcn, n, anchor, Hd, d, k, ptr, idx), topk_ref.topk_model(S, k, ptr, idx),
          "definition with lists")


@pytest.mark.parametrize("d", WIDTHS)
def test_against_float64(pgcn, d):
    n, Q, k = 333, 130, 10
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, d)).astype(np.float32)
    anchor = rng.integers(0, n, Q).astype(np.int32)
    ptr, idx = random_lists(n, Q, 6)
    a64, x64 = x[anchor].astype(np.float64), x.astype(np.float64)
    S = a64 @ x64.T
    B = (d + 1) * U * (np.abs(a64) @ np.abs(x64).T)
    rows = np.arange(Q)[:, None]
    for lists in (None, (ptr, idx)):
        gi, gs = topk(pgcn, n, anchor, _dev(padded(x)), d, k, *(lists or ()))
        cand = np.ones((Q, n), bool)
        if lists:
            for e in range(Q):
                cand[e, idx[ptr[e]:ptr[e + 1]]] = False
        found = gi >= 0
        assert (found.sum(1) == np.minimum(k, cand.sum(1))).all()
        safe = np.where(found, gi, 0)
        assert (cand[rows, safe] | ~found).all(), "an excluded node was returned"
        err = np.abs(gs.astype(np.float64) - S[rows, safe])
        assert (err <= B[rows, safe])[found].all()
        for e in range(Q):
            if not found[e].all():
                continue  # fewer candidates than k: every one of them is in the row
            last = gi[e, k - 1]
            rest = cand[e].copy()
            rest[gi[e]] = False
            assert (S[e, rest] <= S[e, last] + B[e, rest] + B[e, last]).all(), (d, e)


def test_fewer_candidates_than_k(pgcn, tile):
    TQ, TC, _ = tile
    d = 17
    for n, k in ((TC - 1, TC - 1), (TC + 1, TC + 1), (TC - 1, 128), (5, 10)):
        x = normal_input(n, d, 90 + n)
        Hd = _dev(padded(x))
        anchor = np.array([0, n - 1, 2, 2, 3], np.int32)
        S = all_pairs_scores(pgcn, Hd, d, anchor, n)
        gi, gs = got = topk(pgcn, n, anchor, Hd, d, k)
        check(got, topk_ref.topk_model(S, k), (n, k))
        assert (np.sort(gi[:, :min(n, k)], 1) == np.arange(n)[None, :k]).all() or k < n
        assert (gi[:, n:] == -1).all() and np.isneginf(gs[:, n:]).all()
        assert (gi[2] == gi[3]).all()
        # lists: one holds its anchor alone, one all but two nodes, one the anchor and more
        lists = [np.array([0]), np.arange(n)[:-2], np.zeros(0, int), np.array([1, 2, 4]),
                 np.arange(3, n)]
        ptr = np.r_[0, np.cumsum([f.size for f in lists])].astype(np.int64)
        idx = np.concatenate(lists).astype(np.int32)
        gi, gs = got = topk(pgcn, n, anchor, Hd, d, k, ptr, idx)
        check(got, topk_ref.topk_model(S, k, ptr, idx), (n, k, "lists"))
        assert 0 not in gi[0] and set(gi[1][gi[1] >= 0]) == {n - 2, n - 1}
        assert 2 not in gi[3] and set(gi[4][gi[4] >= 0]) == {0, 1, 2}


def test_zero_sign(pgcn, tile):
    TQ, TC, _ = tile
    n = n_two_splits(pgcn, tile)
    x = np.zeros((n, 2), np.float32)
    x[0] = (1.0, -1.0)                      # the anchor
    x[1::3] = (1.0, 1.0)                    # 1 - 1
    x[2::3] = (-0.0, 0.0)                   # a negative zero product
    x[3::3] = (0.0, 0.0)
    x[7] = (-1.0, 1.0)                      # one candidate below zero, one above
    x[n - 2] = (2.0, 1.0)
    anchor = np.zeros(3, np.int32)
    S = x[anchor].astype(np.float64) @ x.astype(np.float64).T
    lists = [np.zeros(0, int), np.array([0]), np.array([0, n - 2, 1, 2, 3][:5])]
    lists = [np.sort(f) for f in lists]
    ptr = np.r_[0, np.cumsum([f.size for f in lists])].astype(np.int64)
    idx = np.concatenate(lists).astype(np.int32)
    for k in (1, 10, 128):
        gi, gs = got = topk(pgcn, n, anchor, _dev(padded(x)), 2, k, ptr, idx)
        check(got, topk_ref.topk_model(S, k, ptr, idx), ("zero sign", k))
        if k >= 10:
            # after the two positive scores the zeros of either sign tie: ascending index
            assert gi[1, 0] == n - 2 and (gs[1, 1:] == 0.0).all()
            assert (np.diff(gi[1, 1:]) > 0).all() and 7 not in gi[1]
            assert gi[1, 1:4].tolist() == [1, 2, 3]


def test_determinism_and_launches(pgcn, tile):
    TQ, TC, _ = tile
    n, Q, d = n_two_splits(pgcn, tile), TQ + 3, 64
    x = normal_input(n, d, 95)
    anchor = np.random.default_rng(96).integers(0, n, Q).astype(np.int32)
    Hd = _dev(padded(x))
    ptr, idx = random_lists(n, Q, 97)
    for k, lists in ((10, ()), (128, (ptr, idx))):
        pgcn.reset_path_counts()
        topk(pgcn, n, anchor, Hd, d, k, *lists, calls=3)
        c = pgcn.path_counts(reset=True)
        # the header: exactly two launches per call, whatever (Q, n, k) and the data
        assert c["topk_sweep"] == 3 and c["topk_merge"] == 3 and c["launches"] == 6
        assert c["rank_sweep"] == 0 and c["rank_filter"] == 0
    # the rank call on the same data launches what it launched before
    target = np.random.default_rng(98).integers(0, n, Q).astype(np.int32)
    g, e = _dev(np.zeros(Q, np.int32)), _dev(np.zeros(Q, np.int32))
    q = pgcn.RankQueries(n, anchor, target)
    for _ in range(2):
        assert pgcn.lib.pgcn_link_rank(q.handle, _p(Hd), Hd.shape[1], d, _p(g), _p(e),
                                       None) == pgcn.PGCN_OK
    _sync()
    q.close()
    c = pgcn.path_counts(reset=True)
    assert c["rank_sweep"] == 2 and c["rank_filter"] == 0 and c["launches"] == 4
    assert c["topk_sweep"] == 0 and c["topk_merge"] == 0
    keep = np.delete(np.arange(n), target[0])
    fp = np.r_[0, np.full(Q, keep.size)].astype(np.int64)
    q = pgcn.RankQueries(n, anchor, np.full(Q, target[0], np.int32), fp, keep.astype(np.int32))
    assert pgcn.lib.pgcn_link_rank(q.handle, _p(Hd), Hd.shape[1], d, _p(g), _p(e),
                                   None) == pgcn.PGCN_OK
    _sync()
    q.close()
    c = pgcn.path_counts(reset=True)
    assert c["rank_sweep"] == 1 and c["rank_filter"] == 1 and c["launches"] == 3


def test_argument_rules_on_device(pgcn):
    n, d = 10, 5
    Hd = _dev(padded(normal_input(n, d, 1)))
    q = pgcn.TopKQueries(n, [1], k=3)
    oi, os_ = _dev(np.zeros(4, np.int32)), _dev(np.zeros(4, np.float32))
    bad = pgcn.PGCN_E_INVALID
    f = pgcn.lib.pgcn_link_topk
    assert f(q.handle, _p(Hd), Hd.shape[1], 0, _p(oi), _p(os_), None) == bad
    assert f(q.handle, _p(Hd), Hd.shape[1], 129, _p(oi), _p(os_), None) == bad
    assert f(q.handle, _p(Hd), 4, d, _p(oi), _p(os_), None) == bad
    assert f(q.handle, _p(Hd), 10, d, _p(oi), _p(os_), None) == bad
    assert f(q.handle, None, Hd.shape[1], d, _p(oi), _p(os_), None) == bad
    assert f(q.handle, _p(Hd), Hd.shape[1], d, None, _p(os_), None) == bad
    assert f(q.handle, _p(Hd), Hd.shape[1], d, _p(oi), None, None) == bad
    assert f(q.handle, ctypes.c_void_p(Hd.data_ptr() + 4), Hd.shape[1], d, _p(oi), _p(os_),
             None) == bad
    q.close()
    # no queries: nothing is launched and the outputs stay as they are
    q = pgcn.TopKQueries(n, np.zeros(0, np.int32), k=3)
    oi, os_ = _dev(np.full(8, SENT_I, np.int32)), _dev(np.full(8, SENT_S, np.float32))
    pgcn.reset_path_counts()
    assert f(q.handle, _p(Hd), Hd.shape[1], d, _p(oi), _p(os_), None) == pgcn.PGCN_OK
    assert f(q.handle, _p(Hd), Hd.shape[1], d, None, None, None) == pgcn.PGCN_OK
    _sync()
    assert pgcn.path_counts(reset=True)["launches"] == 0
    assert (oi.cpu().numpy() == SENT_I).all() and (os_.cpu().numpy() == SENT_S).all()
    assert q.workspace == 0
    q.close()
