"""The numpy model of link top-K (include/pgcn.h, "1-vs-all top-K retrieval") and what its tests
share: the selection by np.lexsort, the fmaf chain's emulation, the 40-node filter pattern and its
set model.  Imports nothing from the test modules."""
import numpy as np

N = 40


def topk_model(S, k, ptr=None, idx=None):
    """(idx int32 [Q][k], score [Q][k] in S's dtype) of the score matrix S [Q][n]: per row the
    candidates not in its exclude list idx[ptr[e]:ptr[e + 1]], ordered by descending score, then
    ascending index (float comparison: -0.0 == +0.0); -1 / -inf from the candidate count on."""
    Q, n = S.shape
    out_i = np.full((Q, k), -1, np.int32)
    out_s = np.full((Q, k), -np.inf, S.dtype)
    v = np.arange(n)
    for e in range(Q):
        keep = np.ones(n, bool)
        if ptr is not None:
            keep[idx[ptr[e]:ptr[e + 1]]] = False
        cand, s = v[keep], S[e][keep]
        order = np.lexsort((cand, -s))[:k]
        out_i[e, :order.size] = cand[order]
        out_s[e, :order.size] = s[order]
    return out_i, out_s


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


def pattern():
    """(indptr, indices, src, dst, label, split) of the ranking filter test's 40-node case:
    directed, with self loops, one edge listed twice, node 39 without slots (and never a column),
    node 37 without a neighbour on either side, pairs in all three splits, a positive pair listed
    twice, a positive pair that is also an edge."""
    rng = np.random.default_rng(3)
    rows = [[] for _ in range(N)]
    for i in range(N - 2):               # nodes 38, 39 have no slots
        rows[i] = sorted(rng.choice(N - 2, rng.integers(1, 6), replace=False).tolist())
        rows[i] = [j for j in rows[i] if j != 37]   # node 37 is never a column ...
    rows[37] = []                        # ... and has no slots: no neighbour on either side
    for i in (0, 5, 11):
        rows[i] = sorted(set(rows[i]) | {i})        # self loops
    rows[2] = sorted(rows[2] + [rows[2][0]])        # a duplicated edge
    rows[4] = sorted(set(rows[4]) | {9})
    indptr = np.r_[0, np.cumsum([len(r) for r in rows])].astype(np.int32)
    indices = np.array([j for r in rows for j in r], np.int32)
    E = 90
    src = rng.integers(0, N, E).astype(np.int32)
    dst = rng.integers(0, N, E).astype(np.int32)
    label = (rng.random(E) < 0.6).astype(np.int32)
    label[rng.choice(E, 5, replace=False)] = -1
    split = (1 + np.arange(E) % 3).astype(np.int32)
    split[rng.choice(E, 6, replace=False)] = 0
    src[6], dst[6], label[6], split[6] = 3, 17, 1, 1
    src[7], dst[7], label[7], split[7] = 3, 17, 1, 2        # the same positive pair again
    src[8], dst[8], label[8], split[8] = 4, 9, 1, 3         # a positive pair that is an edge
    src[9], dst[9], label[9], split[9] = 37, 20, 1, 3       # an anchor (side 0) with no neighbour
    src[10], dst[10], label[10], split[10] = 21, 37, 1, 3   # ... and as side 1's anchor
    src[11], dst[11], label[11], split[11] = 5, 5, 1, 3     # the target is the anchor
    return indptr, indices, src, dst, label, split


def exclude_model(n, indptr, indices, src, dst, label, nodes, side, filtered):
    """Per node of `nodes` the sorted exclude list as a Python set builds it (side 0 / 1)."""
    anc, oth = (src, dst) if side == 0 else (dst, src)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    out = []
    for a in nodes:
        a = int(a)
        f = set()
        if filtered:
            f.add(a)
            f |= set(indices[rows == a].tolist()) if side == 0 else \
                set(rows[indices == a].tolist())
            f |= {int(oth[p]) for p in range(src.size) if label[p] == 1 and anc[p] == a}
        out.append(sorted(f))
    return out
