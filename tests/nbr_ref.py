"""numpy restatement of the neighbour-sampling kernels (include/pgcn.h, pgcn_nbr_sample_draw):
the generator word for word in uint64, the transposed index as a stable argsort, the float64
aggregation formulas on a given sampled pattern, and the seeded test graph."""
import numpy as np

GAMMA = np.uint64(0x9E3779B97F4A7C15)


def mix(z):
    z = np.asarray(z, np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def draw(indptr, indices, K, seed, rnd):
    """(cnt [n], slot [n][K], nbr [n][K]) of pgcn_nbr_sample_draw(seed, rnd)."""
    n = len(indptr) - 1
    with np.errstate(over="ignore"):
        k = mix(np.uint64(seed) + GAMMA * np.uint64(rnd + 1))
        key = mix(k + GAMMA * np.arange(1, n + 1, dtype=np.uint64))
        h = mix(key[:, None] + GAMMA * np.arange(1, K + 1, dtype=np.uint64)[None, :]) >> np.uint64(32)
    slot = np.full((n, K), -1, np.int32)
    for i in range(n):
        b, L = int(indptr[i]), int(indptr[i + 1] - indptr[i])
        if L <= K:
            picks = list(range(L))
        else:
            picks = []
            for t in range(K):
                m = L - K + t
                r = (int(h[i, t]) * (m + 1)) >> 32
                picks.append(m if r in picks else r)
        slot[i, :len(picks)] = b + np.sort(np.array(picks, np.int64))
    cnt = (slot >= 0).sum(1).astype(np.int32)
    nbr = np.where(slot >= 0, np.asarray(indices)[np.maximum(slot, 0)], -1).astype(np.int32)
    return cnt, slot, nbr


def transposed(slot, nbr, n):
    """(t_ptr [n + 1], t_row, t_slot) of the kept entries: a stable sort by neighbour."""
    rows = np.repeat(np.arange(n), slot.shape[1]).reshape(slot.shape)
    real = slot >= 0
    order = np.argsort(nbr[real], kind="stable")
    t_ptr = np.zeros(n + 1, np.int64)
    t_ptr[1:] = np.cumsum(np.bincount(nbr[real], minlength=n))
    return t_ptr, rows[real][order], slot[real][order]


def forward(mode, cnt, slot, nbr, Q, R=None):
    """float64 (out, bound scale, arg): mean = R + sum / cnt, max = R + max with the lowest winning
    slot; scale = (1 / cnt) sum|Q| + |R| (the mean's bound)."""
    real = (slot >= 0)[:, :, None]
    X = Q.astype(np.float64)[np.maximum(nbr, 0)]
    c = np.maximum(cnt, 1)[:, None]
    add = 0.0 if R is None else R.astype(np.float64)
    if mode == 1:
        return (add + np.where(real, X, 0).sum(1) / c,
                np.where(real, np.abs(X), 0).sum(1) / c + np.abs(add), None)
    X = np.where(real, X, -np.inf)
    win = X.argmax(1)  # (the first maximum: slots ascend along the row)
    arg = np.where(cnt[:, None] > 0, np.take_along_axis(slot, win, 1), -1)
    top = np.take_along_axis(X, win[:, None, :], 1)[:, 0, :]  # (its value: -0.0 == +0.0 is a tie)
    top = np.where(cnt[:, None] > 0, top, 0.0).astype(np.float32)
    out = top if R is None else np.where(cnt[:, None] > 0, R + top, R)
    return out.astype(np.float32), None, arg.astype(np.int32)


def backward(mode, cnt, slot, nbr, G, arg=None):
    """float64 (din, sum of |terms|) over the transposed sampled pattern."""
    n, d = G.shape
    i, p = np.nonzero(slot >= 0)
    if mode == 1:
        terms = G.astype(np.float64)[i] / cnt[i][:, None]
    else:
        terms = np.where(arg[i] == slot[i, p][:, None], G.astype(np.float64)[i], 0.0)
    din, mag = np.zeros((n, d)), np.zeros((n, d))
    np.add.at(din, nbr[i, p], terms)
    np.add.at(mag, nbr[i, p], np.abs(terms))
    return din, mag


HUB_ROWS = 1200


def graph(K, seed=5):
    """2,000 rows: rows 0..6 have 0, 1, K - 1, K, K + 1, 2 K and 3,000 slots; rows 7 .. 7 + 1,199
    have K + 1 slots of which one is node 0 (the hub column); the rest 0 .. 2 K + 2 slots.  Apart
    from the hub slots no row names node 0, and none names node n - 1."""
    rng = np.random.default_rng(seed)
    n = 2000
    lens = np.concatenate([[0, 1, K - 1, K, K + 1, 2 * K, 3000], np.full(HUB_ROWS, K + 1),
                           rng.integers(0, 2 * K + 3, n - 7 - HUB_ROWS)]).astype(np.int64)
    rows = [rng.integers(1, n - 1, L) for L in lens]
    for i in range(7, 7 + HUB_ROWS):
        rows[i][rng.integers(0, K + 1)] = 0
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum(lens)
    return indptr, np.concatenate(rows).astype(np.int32)
