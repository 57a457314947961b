"""Float64 numpy reference of the GraphSAGE aggregators over a CSR pattern and of an engine built
on them (tests/test_cpu_sage.py checks the backward formulas against central differences).

Slot s = (i, j) is global position s of `indices`; len_i is the CSR row length as given (self
loops and duplicated edges count as the pattern has them).

    mean:  Z_i = R_i + (1 / len_i) * sum over row i's slots of Q_j
    max:   Z_i[c] = R_i[c] + max over row i's slots of Q_j[c]   (arg_i[c]: the lowest such slot)

A row without a slot gives Z_i = R_i (or 0 without R) and arg_i = -1.
"""
import numpy as np


def rows_of(indptr):
    return np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))


def mean_forward(indptr, indices, Q, R=None):
    Q = np.asarray(Q, np.float64)
    n = len(indptr) - 1
    lens = np.diff(indptr).astype(np.float64)
    Z = np.zeros((n, Q.shape[1]))
    np.add.at(Z, rows_of(indptr), Q[indices])
    Z[lens > 0] /= lens[lens > 0, None]
    return Z if R is None else Z + np.asarray(R, np.float64)


def mean_backward(indptr, indices, G):
    """dQ_j = sum over the slots (i, j) into column j of G_i / len_i."""
    G = np.asarray(G, np.float64)
    rows = rows_of(indptr)
    lens = np.diff(indptr).astype(np.float64)
    dQ = np.zeros_like(G)
    np.add.at(dQ, indices, G[rows] / lens[rows, None])
    return dQ


def max_forward(indptr, indices, Q, R=None):
    """(Z, arg) in Q's dtype arithmetic: the first (lowest-slot) argmax of every row and column;
    Z = R + max is one add in that dtype."""
    Q = np.asarray(Q)
    n, d = len(indptr) - 1, Q.shape[1]
    Z = np.zeros((n, d), Q.dtype)
    arg = np.full((n, d), -1, np.int64)
    for i in range(n):
        b, e = int(indptr[i]), int(indptr[i + 1])
        if e > b:
            cand = Q[indices[b:e]]
            a = cand.argmax(axis=0)  # the first occurrence: the lowest slot
            arg[i] = b + a
            Z[i] = cand[a, np.arange(d)]
    if R is not None:
        R = np.asarray(R, Q.dtype)
        has = np.diff(indptr) > 0
        Z[has] = R[has] + Z[has]
        Z[~has] = R[~has]
    return Z, arg


def max_backward(indptr, indices, G, arg):
    """dQ_j[c] = sum over the slots s = (i, j) into j with arg[i][c] == s of G_i[c]."""
    G = np.asarray(G, np.float64)
    dQ = np.zeros_like(G)
    i, c = np.nonzero(arg >= 0)
    np.add.at(dQ, (indices[arg[i, c]], c), G[i, c])
    return dQ


def max_backward_terms(indptr, indices, G, arg):
    """Per element of dQ: the number of non-zero terms and the sum of their magnitudes."""
    G = np.asarray(G, np.float64)
    cnt = np.zeros(G.shape, np.int64)
    mag = np.zeros_like(G)
    i, c = np.nonzero((arg >= 0) & (G != 0.0))
    np.add.at(cnt, (indices[arg[i, c]], c), 1)
    np.add.at(mag, (indices[arg[i, c]], c), np.abs(G[i, c]))
    return cnt, mag


def max_margin(indptr, indices, Q):
    """Per element (i, c): the gap between the largest and the second largest DISTINCT-slot
    candidate value of the row (inf for rows of fewer than two slots; 0 on an exact tie)."""
    Q = np.asarray(Q, np.float64)
    n, d = len(indptr) - 1, Q.shape[1]
    gap = np.full((n, d), np.inf)
    for i in range(n):
        b, e = int(indptr[i]), int(indptr[i + 1])
        if e - b >= 2:
            top = np.sort(Q[indices[b:e]], axis=0)[-2:]
            gap[i] = top[1] - top[0]
    return gap


# --------------------------------------------------------------------------- the engine model
AGGREGATORS = ("mean", "max")


def _gat_ref():
    import gat_ref  # (scipy: only the engine model needs it)
    return gat_ref


def glorot_weights(pgcn, seed, dims, root_weight):
    """The engine's initial layer weights without a device: Glorot-uniform with fan-out 2 d_l
    under root_weight, drawn in layer order from the xorshift stream of `seed`; (weights, draws)."""
    g = _gat_ref()
    rng = g.Xorshift(pgcn.rng_seed(seed))
    out, draws = [], 0
    for a, b in zip(dims, dims[1:]):
        wc = 2 * b if root_weight else b
        limit = np.sqrt(np.float32(6.0) / np.float32(a + wc))
        r = rng.draws(a * wc).astype(np.float32) / np.float32(g.RAND_MAX)
        out.append((((r.astype(np.float64) - 0.5) * np.float64(limit)) * 2.0).astype(np.float32))
        draws += a * wc
    return out, draws


class NumpySageGCN:
    """The L-layer GraphSAGE model in float64: per layer P = drop(A) W_l, R / Q its halves (root
    weight) or Q = P, Z = R + aggr(Q); hidden layers [LayerNorm] -> ReLU -> [+ A on a residual
    layer]; the loss is softmax cross-entropy or (label_bits given) sigmoid BCE.  weights: the
    engine's W_l; rng: a gat_ref.Xorshift standing behind the engine's initial draws (one training
    forward consumes the input dropout's nnz_X draws, then each hidden dropout's N * h_l), or None
    for no dropout.  After a forward, self.gap[l] holds the max aggregator's margins
    (max_margin) and self.qmax[l] the largest |Q| of the layer."""

    def __init__(self, ds, hidden, weights, dropouts, rng=None, aggregator="mean",
                 root_weight=False, residual=False, layer_norm=False, label_bits=None,
                 indptr=None, indices=None):
        g = _gat_ref()
        assert aggregator in AGGREGATORS
        self.agg, self.root = aggregator, bool(root_weight)
        self.ip = np.asarray(ds.graph_indptr if indptr is None else indptr, np.int64)
        self.idx = np.asarray(ds.graph_indices if indices is None else indices, np.int64)
        self.X = g._features(ds)
        self.n = ds.num_nodes
        self.dims = [ds.input_dim] + list(hidden) + [ds.output_dim]
        self.L = L = len(self.dims) - 1
        k = 2 if self.root else 1
        self.W = [np.asarray(w, np.float64).reshape(self.dims[l], k * self.dims[l + 1])
                  for l, w in enumerate(weights)]
        self.ln = layer_norm
        self.gamma = [np.ones(h) for h in hidden] if layer_norm else []
        self.beta = [np.zeros(h) for h in hidden] if layer_norm else []
        self.params = self.W + [t for l in range(len(self.gamma))
                                for t in (self.gamma[l], self.beta[l])]
        self.m = [np.zeros_like(w) for w in self.params]
        self.v = [np.zeros_like(w) for w in self.params]
        self.t = 0
        self.p, self.rng = list(dropouts), rng
        self.label, self.split = np.asarray(ds.label), np.asarray(ds.split)
        self.bits = None if label_bits is None else np.asarray(label_bits, np.float64)
        self.res = [residual and 1 <= l <= L - 2 and self.dims[l + 1] == self.dims[l]
                    for l in range(L)]

    def _mask(self, shape, p, training):
        if not training or self.rng is None:
            return None
        n = int(np.prod(shape))
        return self.rng.keep(n, p).reshape(shape) * (1.0 / (1.0 - np.float64(np.float32(p))))

    def forward(self, split, training=False):
        g = _gat_ref()
        L = self.L
        self.masks, self.A, self.Y, self.arg, self.gap, self.qmax = [], [], [], [], [], []
        self.xhat, self.rstd = [], []
        h = None
        for l in range(L):
            if l == 0:
                k = self._mask((self.X.nnz,), self.p[0], training)
                a_in = self.X
                if k is not None:
                    a_in = self.X.copy()
                    a_in.data = a_in.data * k
            else:
                k = self._mask(h.shape, self.p[l], training)
                a_in = h if k is None else h * k
            self.masks.append(k)
            self.A.append(a_in)
            P = np.asarray(a_in @ self.W[l])
            d = self.dims[l + 1]
            R, Q = (P[:, :d], P[:, d:]) if self.root else (None, P)
            if self.agg == "mean":
                Z = mean_forward(self.ip, self.idx, Q, R)
                self.arg.append(None)
                self.gap.append(None)
            else:
                Z, arg = max_forward(self.ip, self.idx, Q, R)
                self.arg.append(arg)
                self.gap.append(max_margin(self.ip, self.idx, Q))
            self.qmax.append(float(np.abs(Q).max()))
            if l == L - 1:
                break
            y = Z
            if self.ln:
                mean = y.mean(axis=1, keepdims=True)
                rstd = 1.0 / np.sqrt(((y - mean) ** 2).mean(axis=1, keepdims=True) + g.LN_EPS)
                xhat = (y - mean) * rstd
                self.xhat.append(xhat)
                self.rstd.append(rstd)
                y = self.gamma[l] * xhat + self.beta[l]
            hn = np.maximum(y, 0.0)
            if self.res[l]:
                hn = hn + self.A[l]
            self.Y.append(y)
            h = hn
        logits = Z
        rows = np.nonzero((self.split == split) & (self.label >= 0))[0]
        self.rows, self.logits = rows, logits
        l2 = g.WD * float((self.W[0] ** 2).sum()) / 2.0
        if self.bits is not None:
            x, y = logits[rows], self.bits[rows]
            self.count = x.size
            loss = float((np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).sum())
            self.acc = 1.0 - float(((x > 0) != (y > 0)).sum()) / self.count
            return loss / self.count + l2
        zr = logits[rows] - logits[rows].max(axis=1, keepdims=True)
        lse = np.log(np.exp(zr).sum(axis=1))
        t = self.label[rows]
        self.shifted, self.lse = zr, lse
        self.acc = float((zr.argmax(axis=1) == t).mean())
        return float((lse - zr[np.arange(len(rows)), t]).mean()) + l2

    def backward(self):
        L, rows = self.L, self.rows
        g = np.zeros_like(self.logits)
        if self.bits is not None:
            x, y = self.logits[rows], self.bits[rows]
            g[rows] = (1.0 / (1.0 + np.exp(-x)) - y) / self.count
        else:
            p = np.exp(self.shifted - self.lse[:, None])
            p[np.arange(len(rows)), self.label[rows]] -= 1.0
            g[rows] = p / len(rows)
        self.dW, self.dvar1 = [None] * L, [None] * L
        self.dgamma, self.dbeta = [None] * (L - 1), [None] * (L - 1)
        for l in range(L - 1, -1, -1):
            skip = None
            if l < L - 1:  # g = dLoss/dH_l: back through [residual], ReLU, [LayerNorm]
                skip = g if self.res[l] else None
                g = g * (self.Y[l] > 0)
                if self.ln:
                    xhat = self.xhat[l]
                    self.dgamma[l] = (g * xhat).sum(axis=0)
                    self.dbeta[l] = g.sum(axis=0)
                    gh = g * self.gamma[l]
                    g = self.rstd[l] * (gh - gh.mean(axis=1, keepdims=True) -
                                        xhat * (gh * xhat).mean(axis=1, keepdims=True))
            if self.agg == "mean":
                dQ = mean_backward(self.ip, self.idx, g)
            else:
                dQ = max_backward(self.ip, self.idx, g, self.arg[l])
            dP = np.concatenate([g, dQ], axis=1) if self.root else dQ
            self.dvar1[l] = dP
            self.dW[l] = np.asarray(self.A[l].T @ dP)
            if l == 0:
                break
            g = dP @ self.W[l].T  # dLoss/d drop(H_{l-1})
            if skip is not None:
                g = g + skip
            if self.masks[l] is not None:
                g = g * self.masks[l]

    def norm_grad(self):
        return np.concatenate([x for l in range(self.L - 1)
                               for x in (self.dgamma[l], self.dbeta[l])])

    def step(self):
        g = _gat_ref()
        self.t += 1
        ss = g.LR * np.sqrt(1.0 - g.B2 ** self.t) / (1.0 - g.B1 ** self.t)
        grads = self.dW + [t for l in range(len(self.gamma))
                           for t in (self.dgamma[l], self.dbeta[l])]
        for k in range(len(self.params)):
            grad = grads[k] + (g.WD * self.params[k] if k == 0 else 0.0)
            self.m[k] = g.B1 * self.m[k] + (1.0 - g.B1) * grad
            self.v[k] = g.B2 * self.v[k] + (1.0 - g.B2) * grad * grad
            self.params[k] -= ss * self.m[k] / (np.sqrt(self.v[k]) + g.EPS)  # in place

    def train_logits(self):
        out = self.logits.copy()
        if self.bits is None:
            out[self.rows] = self.shifted
        return out

    def near_tied(self, rel):
        """Per layer of the last forward (max only): the mask of elements whose top two candidates
        lie within rel * max|Q| of each other without being an exact tie."""
        return [None if gp is None else (gp > 0) & (gp < rel * q)
                for gp, q in zip(self.gap, self.qmax)]
