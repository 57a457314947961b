"""pgcn_link_rank_mlp through the kernel ABI: the 1-vs-all ranking counts under the Hadamard-MLP
decoder against the device's own pair forward.

The claim is bitwise agreement, so nothing here has a tolerance: the reference scores are
Links.mlp_fwd on all Q x n explicit (anchor, v) pairs (its agreement with float64 is pinned by
tests/test_gpu_link_mlp_kernels.py), numpy counts `>` and `==` against the score of the pair
(a_e, t_e) over v != t_e outside the query's list, and RankQueries.rank_mlp must return exactly
those counts.  H and P are random normal, their row padding NaN, a sentinel behind each output.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SENTINEL = 0x5EED5EED
SHAPES = ((1, 1), (3, 128), (17, 33), (33, 32), (64, 65), (128, 128))  # every ND / UT class
# candidates in units of the chunk TC; 8 TC + 1 is the first n with two candidate splits (a split
# holds at least 8 chunks)
NODES = {"TC-1": lambda c: c - 1, "TC": lambda c: c, "TC+1": lambda c: c + 1,
         "2TC+5": lambda c: 2 * c + 5, "8TC+1": lambda c: 8 * c + 1}
QUERIES = {"1": lambda q: 1, "TQ-1": lambda q: q - 1, "TQ": lambda q: q, "TQ+3": lambda q: q + 3}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def _padded(x, extra=4):
    out = np.full((x.shape[0], (x.shape[1] + 3) // 4 * 4 + extra), np.nan, np.float32)
    out[:, :x.shape[1]] = x
    return out


def _tensors(rng, n, d, h, b1=None):
    P = np.zeros((d + 3, h), np.float32)
    P[:d + 2] = rng.standard_normal((d + 2, h))
    P[d + 2, 0] = rng.standard_normal()
    if b1 is not None:
        P[d] = b1
    return _padded(rng.standard_normal((n, d)).astype(np.float32)), _padded(P)


def run(pgcn, n, Q, d, h, seed, b1=None, lists=None):
    """rank_mlp's (greater, equal), checked against the counts of mlp_fwd's Q x n scores"""
    rng = np.random.default_rng(seed)
    H, P = _tensors(rng, n, d, h, b1)
    anchor, target = (rng.integers(0, n, Q).astype(np.int32) for _ in range(2))
    Hd, Pd = _dev(H), _dev(P)
    every = pgcn.Links(n, np.repeat(anchor, n), np.tile(np.arange(n, dtype=np.int32), Q), None)
    out = _dev(np.zeros((Q * n, 4), np.float32))
    every.mlp_fwd(Hd, H.shape[1], d, Pd, P.shape[1], h, out, 4)
    _sync()
    S = out.cpu().numpy()[:, 0].reshape(Q, n)
    every.close()
    assert np.isfinite(S).all()
    mask = np.ones((Q, n), bool)
    mask[np.arange(Q), target] = False
    ptr = idx = None
    if lists is not None:
        rows = [np.setdiff1d(lists(rng, e), [target[e]]).astype(np.int32) for e in range(Q)]
        ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])]).astype(np.int64)
        idx = np.concatenate(rows) if ptr[-1] else np.zeros(0, np.int32)
        for e, r in enumerate(rows):
            mask[e, r] = False
    thr = S[np.arange(Q), target][:, None]
    want = ((S > thr) & mask).sum(1), ((S == thr) & mask).sum(1)
    rq = pgcn.RankQueries(n, anchor, target, ptr, idx)
    got = []
    for _ in range(2):
        counts = _dev(np.full((2, Q + 1), SENTINEL, np.int32))
        rq.rank_mlp(Hd, H.shape[1], d, Pd, P.shape[1], h, counts[0], counts[1])
        _sync()
        got.append(counts.cpu().numpy().view(np.uint32))
        assert (got[-1][:, Q] == SENTINEL).all()
    rq.close()
    np.testing.assert_array_equal(got[0], got[1])  # integer sums: identical bits over two calls
    np.testing.assert_array_equal(got[0][0, :Q], want[0])
    np.testing.assert_array_equal(got[0][1, :Q], want[1])
    return got[0][0, :Q], got[0][1, :Q]


@pytest.mark.parametrize("d,h", SHAPES)
def test_every_shape_class(pgcn, d, h):
    TQ, TC = pgcn.link_rank_mlp_tile()
    greater, _ = run(pgcn, 2 * TC + 5, TQ + 3, d, h, seed=d * 1000 + h)
    assert greater.max() > 0  # the counts are not trivially zero


@pytest.mark.parametrize("nq", list(QUERIES))
@pytest.mark.parametrize("nn", list(NODES))
def test_every_tile_edge(pgcn, nn, nq):
    TQ, TC = pgcn.link_rank_mlp_tile()
    run(pgcn, NODES[nn](TC), QUERIES[nq](TQ), 17, 33, seed=7)


@pytest.mark.parametrize("h", [1, 4])
def test_all_units_dead_every_score_ties(pgcn, h):
    TQ, TC = pgcn.link_rank_mlp_tile()
    n, Q = 2 * TC + 5, TQ + 3
    greater, equal = run(pgcn, n, Q, 5, h, seed=3, b1=np.full(h, -100.0, np.float32))
    assert (greater == 0).all() and (equal == n - 1).all()  # every score is exactly b2


def test_half_the_units_dead(pgcn):
    TQ, TC = pgcn.link_rank_mlp_tile()
    b1 = np.where(np.arange(33) % 2 == 0, -100.0, 0.25).astype(np.float32)
    run(pgcn, 2 * TC + 5, TQ + 3, 17, 33, seed=4, b1=b1)


def test_filtered_random_lists(pgcn):
    TQ, TC = pgcn.link_rank_mlp_tile()
    n = 8 * TC + 1

    def lists(rng, e):  # empty lists first, last and in between; some longer than a pair tile
        size = 0 if e in (0, TQ + 2) or e % 5 == 1 else int(rng.integers(1, 2 * TC))
        return rng.choice(n, size, replace=False)
    run(pgcn, n, TQ + 3, 33, 32, seed=5, lists=lists)


def test_filtered_every_node_but_the_target(pgcn):
    """The sweep counts every candidate and the correction takes every one out again: both counts
    are exactly zero only if the two agree on every (query, candidate) score."""
    TQ, TC = pgcn.link_rank_mlp_tile()
    n = 2 * TC + 5
    greater, equal = run(pgcn, n, TQ + 3, 64, 65, seed=6, lists=lambda rng, e: np.arange(n))
    assert (greater == 0).all() and (equal == 0).all()


def test_invalid_arguments_launch_nothing(pgcn):
    rng = np.random.default_rng(8)
    n, Q, d, h = 70, 5, 17, 33
    H, P = _tensors(rng, n, d, h)
    Hd, Pd, out = _dev(H), _dev(P), _dev(np.zeros((2, Q), np.int32))
    rq = pgcn.RankQueries(n, np.arange(Q, dtype=np.int32), np.arange(Q, dtype=np.int32) + 1)
    ld_h, ld_p = H.shape[1], P.shape[1]
    good = dict(H=Hd, ld_h=ld_h, d=d, P=Pd, ld_p=ld_p, h=h, greater=out[0], equal=out[1])
    bad = [dict(d=0), dict(d=129), dict(h=0), dict(h=129), dict(ld_h=ld_h + 1), dict(ld_h=16),
           dict(ld_p=ld_p + 2), dict(ld_p=32), dict(H=Hd.data_ptr() + 4), dict(P=Pd.data_ptr() + 8),
           dict(H=None), dict(P=None), dict(greater=None), dict(equal=None)]
    _sync()
    pgcn.reset_path_counts()
    for kw in bad:
        with pytest.raises(pgcn.PgcnError) as e:
            rq.rank_mlp(**{**good, **kw})
        assert e.value.status == pgcn.PGCN_E_INVALID, kw
    assert not any(pgcn.path_counts().values())
    rq.rank_mlp(**good)
    _sync()
    c = pgcn.path_counts()
    assert c["rank_mlp_sweep"] == 1 and c["rank_mlp_filter"] == 0 and c["link_mlp_fwd"] == 1
    rq.close()
