"""pgcn_link_topk_mlp through the kernel ABI: 1-vs-all top-K retrieval under the Hadamard-MLP
decoder against the device's own pair forward.  TQ, TC, KMAX = pgcn_link_topk_mlp_tile().

The claim is exact: numpy's stable top-K (tests/topk_ref.py) of S = Links.mlp_fwd on all Q x n
explicit (anchor, v) pairs must equal idx exactly and score by value, -1 / -inf from min(k,
candidates) on.  The only tolerance is test_against_float64's, the pair forward's own bound.  H and
P: random normal, NaN row padding; sentinels behind idx and score; two calls per handle, equal bits.
Exclude lists (test_gpu_topk_kernels.random_lists): query 0 empty, query 1 every node, the rest at
densities 0.02 / 0.3 / 0.9.
"""
import numpy as np
import pytest

import link_mlp_ref
import topk_ref
from test_gpu_rank_mlp_kernels import _dev, _padded
from test_gpu_topk_kernels import random_lists

pytestmark = pytest.mark.gpu

EPS, SENT_I, SENT_S = 2.0 ** -24, -77, 7.25
SHAPES = ((1, 1), (3, 128), (17, 33), (33, 32), (64, 65), (128, 128))  # every ND / UT class
# (shape, n, Q, k), a covering selection: every n (n2: the first with two splits), Q and k (both
# E; k > candidates at TC - 1) of the issue's lists, every shape class at two splits
CASES = [(0, "TC-1", "1", 1), (1, "TC", "TQ-1", 10), (2, "TC+1", "TQ", 64),
         (3, "2TC+5", "TQ+3", 65), (4, "n2", "TQ+3", 128), (5, "n2", "TQ", 10),
         (2, "TC-1", "TQ+3", 128), (0, "n2", "TQ-1", 65), (1, "n2", "1", 64), (3, "n2", "TQ+3", 1),
         (5, "2TC+5", "TQ+3", 128), (2, "n2", "TQ", 10)]


def sizes(pgcn, nn, nq):
    TQ, TC, _ = pgcn.link_topk_mlp_tile()
    n2 = next(n for n in range(1, 64 * TC) if pgcn.link_topk_mlp_splits(TQ, n) >= 2)
    n = {"TC-1": TC - 1, "TC": TC, "TC+1": TC + 1, "2TC+5": 2 * TC + 5, "n2": n2}[nn]
    return n, {"1": 1, "TQ-1": TQ - 1, "TQ": TQ, "TQ+3": TQ + 3}[nq]


class Problem:
    """H [n][d], P and Q anchors on the device, and S [Q][n]: mlp_fwd's score of every pair;
    topk: (idx [Q][k], score [Q][k]) of two calls on one handle, sentinels and equal bits checked"""

    def __init__(self, pgcn, n, Q, d, h, seed, x=None, P=None, anchor=None):
        rng = np.random.default_rng(seed)
        self.pgcn, self.n, self.Q, self.d, self.h = pgcn, n, Q, d, h
        self.x = rng.standard_normal((n, d)).astype(np.float32) if x is None else x
        if P is None:
            P = np.zeros((d + 3, h), np.float32)
            P[:d + 2] = rng.standard_normal((d + 2, h))
            P[d + 2, 0] = rng.standard_normal()
        self.P = P
        self.anchor = rng.integers(0, n, Q).astype(np.int32) if anchor is None else anchor
        self.Hd, self.Pd = _dev(_padded(self.x)), _dev(_padded(P))
        self.every = (np.repeat(self.anchor, n), np.tile(np.arange(n, dtype=np.int32), Q))
        links = pgcn.Links(n, *self.every, None)
        out = _dev(np.zeros((Q * n, 4), np.float32))
        links.mlp_fwd(self.Hd, self.Hd.shape[1], d, self.Pd, self.Pd.shape[1], h, out, 4)
        self.S = out.cpu().numpy()[:, 0].reshape(Q, n)
        links.close()
        assert np.isfinite(self.S).all()

    def topk(self, k, ptr=None, idx=None):
        Q = self.Q
        q = self.pgcn.TopKQueries(self.n, self.anchor, ptr, idx, k=k, decoder=True)
        lists = 2 * self.pgcn.link_topk_mlp_splits(Q, self.n)
        assert q.workspace == Q * lists * (128 if k <= 64 else 256) * 8
        out = []
        for _ in range(2):
            di = _dev(np.full(Q * k + 8, SENT_I, np.int32))
            ds = _dev(np.full(Q * k + 8, SENT_S, np.float32))
            q.topk_mlp(self.Hd, self.Hd.shape[1], self.d, self.Pd, self.Pd.shape[1], self.h, di, ds)
            hi, hs = di.cpu().numpy(), ds.cpu().numpy()
            assert (hi[Q * k:] == SENT_I).all() and (hs[Q * k:] == SENT_S).all()
            out.append((hi[:Q * k].reshape(Q, k), hs[:Q * k].reshape(Q, k)))
        q.close()
        assert (out[0][0] == out[1][0]).all()
        assert (out[0][1].view(np.uint32) == out[1][1].view(np.uint32)).all()
        return out[0]

    def check(self, k, ptr=None, idx=None):
        gi, gs = self.topk(k, ptr, idx)
        wi, ws = topk_ref.topk_model(self.S, k, ptr, idx)
        assert (gi == wi).all(), np.argwhere(gi != wi)[:5].tolist()
        assert (gs == ws).all()
        return gi, gs


@pytest.mark.parametrize("shape,nn,nq,k", CASES)
def test_definition(pgcn, shape, nn, nq, k):
    (n, Q), (d, h) = sizes(pgcn, nn, nq), SHAPES[shape]
    p = Problem(pgcn, n, Q, d, h, seed=1000 * d + h + k)
    gi, gs = p.check(k)
    assert (gi[:, :min(k, n)] >= 0).all() and (gi[:, n:] == -1).all()
    gi, gs = p.check(k, *random_lists(n, Q, seed=k))
    assert Q == 1 or ((gi[1] == -1).all() and np.isneginf(gs[1]).all())


@pytest.mark.parametrize("k", (1, 65, 128))
@pytest.mark.parametrize("form", ("ties", "ascending", "descending"))
def test_ties_and_forced_prunes(pgcn, form, k):
    """At the two-split n.  ties: every unit dead, every score exactly b2 -- the k smallest indices
    not excluded, across the 32-candidate block, the chunk and the split boundary.  Otherwise
    d = h = 1 and score = relu(H[a] H[v]): ascending in v every candidate passes tau and a prune
    is due every few chunks; descending, nothing passes after the first prune."""
    n, Q = sizes(pgcn, "n2", "TQ+3")
    if form == "ties":
        P = np.random.default_rng(k).standard_normal((8, 4)).astype(np.float32)
        P[5], P[7, 1:] = -1e4, 0.0
        p = Problem(pgcn, n, Q, 5, 4, seed=k, P=P)
        want, first = np.full(n, P[7, 0]), 0
    else:
        v = np.arange(1, n + 1, dtype=np.float32)
        want, first = (v, n - 1) if form == "ascending" else (n + 1 - v, 0)
        P = np.array([[1.0], [0.0], [1.0], [0.0]], np.float32)
        anchor = np.full(Q, n - 1 - first, np.int32)   # the row that holds 1
        p = Problem(pgcn, n, Q, 1, 1, seed=0, x=want[:, None], P=P, anchor=anchor)
    assert (p.S == want).all() and p.check(k)[0][0, 0] == first
    gi, _ = p.check(k, *random_lists(n, Q, seed=40 + k))
    if form == "ties" and k == 128:  # the dense lists push the survivors across the split boundary
        TC = pgcn.link_topk_mlp_tile()[1]
        boundary = -(-(-(-n // TC)) // pgcn.link_topk_mlp_splits(Q, n)) * TC
        assert ((gi >= boundary).any(1) & (gi[:, 0] >= 0) & (gi[:, 0] < boundary)).any()


@pytest.mark.parametrize("d,h", SHAPES)
def test_against_float64(pgcn, d, h):
    """Every returned score within the pair forward's bound of the float64 score; every candidate w
    not returned has s64(w) <= s64(v_last) + bound(w) + bound(v_last).  No case is left out."""
    n, Q, k = 333, 67, 10
    p = Problem(pgcn, n, Q, d, h, seed=5)
    s64, A, B, _ = link_mlp_ref.forward(*p.every, p.x, p.P, d, h)
    bound = ((h + 2) * EPS * A + (d + 3) * EPS * B + EPS * abs(float(p.P[d + 2, 0]))).reshape(Q, n)
    s64, rows = s64.reshape(Q, n), np.arange(Q)[:, None]
    ptr, idx = random_lists(n, Q, seed=6)
    for lists in ((), (ptr, idx)):
        gi, gs = p.topk(k, *lists)
        cand = np.ones((Q, n), bool)
        for e in range(Q if lists else 0):
            cand[e, idx[ptr[e]:ptr[e + 1]]] = False
        found = gi >= 0
        safe = np.where(found, gi, 0)
        assert (found.sum(1) == np.minimum(k, cand.sum(1))).all()
        assert (cand[rows, safe] | ~found).all(), "an excluded node was returned"
        assert (np.abs(gs - s64[rows, safe]) <= bound[rows, safe])[found].all()
        for e in np.flatnonzero(found.all(1)):  # (fewer candidates than k: all are returned)
            rest, last = cand[e].copy(), gi[e, k - 1]
            rest[gi[e]] = False
            assert (s64[e, rest] <= s64[e, last] + bound[e, rest] + bound[e, last]).all(), (d, h, e)


def test_launches_and_refusals(pgcn):
    n, Q, d, h, k = 70, 5, 17, 33, 3
    p = Problem(pgcn, n, Q, d, h, seed=8)
    ld_h, ld_p, bad = p.Hd.shape[1], p.Pd.shape[1], pgcn.PGCN_E_INVALID
    di, ds = _dev(np.full(Q * k, SENT_I, np.int32)), _dev(np.full(Q * k, SENT_S, np.float32))
    good = dict(H=p.Hd, ld_h=ld_h, d=d, P=p.Pd, ld_p=ld_p, h=h, idx=di, score=ds)
    mlp, dot = pgcn.TopKQueries(n, p.anchor, k=k, decoder=True), pgcn.TopKQueries(n, p.anchor, k=k)
    none = pgcn.TopKQueries(n, np.zeros(0, np.int32), k=k, decoder=True)
    pgcn.reset_path_counts()
    for kw in (dict(q=dot), dict(d=0), dict(d=129), dict(h=0), dict(h=129), dict(H=None),
               dict(idx=None)):
        with pytest.raises(pgcn.PgcnError) as e:
            kw.pop("q", mlp).topk_mlp(**{**good, **kw})
        assert e.value.status == bad, kw
    assert pgcn.lib.pgcn_link_topk(mlp.handle, p.Hd.data_ptr(), ld_h, d, di.data_ptr(),
                                   ds.data_ptr(), None) == bad
    for bad_k in (0, 129):
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.TopKQueries(n, p.anchor, k=bad_k, decoder=True)
        assert e.value.status == bad
    none.topk_mlp(**good)  # Q = 0 launches nothing
    assert not any(pgcn.path_counts().values()) and none.workspace == 0
    assert (di.cpu().numpy() == SENT_I).all() and (ds.cpu().numpy() == SENT_S).all()
    mlp.topk_mlp(**good)
    assert (di.cpu().numpy() != SENT_I).all()
    c = pgcn.path_counts(reset=True)
    assert c["topk_mlp_sweep"] == 1 and c["topk_mlp_merge"] == 1 and c["launches"] == 2
    [q.close() for q in (mlp, dot, none)]
