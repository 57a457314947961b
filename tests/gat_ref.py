"""The float64 numpy reference of the graph attention layers (pgcn_params.attention), shared by
tests/test_cpu_gat.py (which checks it against central differences), test_gpu_gat_kernels.py
and test_gpu_gat.py.  Not a test file.

One layer, single head, additive attention over the CSR slots s = (i, j) of the pattern as it is
(self loops and duplicated slots count as they stand):
    u_i = P_i . a_dst, v_j = P_j . a_src, x_s = u_i + v_j, e_s = x_s > 0 ? x_s : slope x_s
    alpha_s = exp(e_s - max_row) / sum_row exp(e - max_row),  Z_i = sum_row alpha_s P_j
    c_i = G_i . Z_i,  dx_s = alpha_s (G_i . P_j - c_i) (x_s > 0 ? 1 : slope)
    du_i = sum over row i of dx, dv_j = sum over the slots into column j of dx
    dP_j = sum into column j of alpha_s G_i + du_j a_dst + dv_j a_src
    da_dst = sum du_i P_i,  da_src = sum dv_j P_j
The model (NumpyGatGCN) follows tests/test_gpu_layernorm.py's reference: scipy CSR algebra,
hpdga's Adam, weight decay on W0 only, started from the engine's initial tensors; the dropout
masks are hpdga's (one xorshift128+ draw per element, tests/helpers.py's oracle restates them).
"""
import numpy as np

SLOPE = 0.2
LR, WD, B1, B2, EPS = 0.01, 5e-4, 0.9, 0.999, 1e-8
LN_EPS = 1e-5
RAND_MAX = 0x7fffffff


def gat_forward(indptr, indices, P, a_dst, a_src, slope=SLOPE, dtype=np.float64):
    """dict of u, v, x, alpha (per slot), Z, rows (the slot's row).  dtype float32 runs the same
    statements in float32 (the tolerance rule's measure of the format's own error)."""
    import scipy.sparse as sps
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    P = np.asarray(P, dtype)
    a_dst, a_src = np.asarray(a_dst, dtype), np.asarray(a_src, dtype)
    n = len(indptr) - 1
    rows = np.repeat(np.arange(n), np.diff(indptr))
    u, v = P @ a_dst, P @ a_src
    x = u[rows] + v[indices]
    e = np.where(x > 0, x, dtype(slope) * x)
    m = np.full(n, -np.inf, dtype)
    np.maximum.at(m, rows, e)
    w = np.exp(e - m[rows])
    s = np.bincount(rows, weights=w, minlength=n).astype(dtype)
    alpha = (w / s[rows]).astype(dtype)
    Z = np.asarray(sps.csr_matrix((alpha, indices, indptr), shape=(n, n)) @ P, dtype)
    return dict(u=u, v=v, x=x, alpha=alpha, Z=Z, rows=rows)


def gat_backward(fwd, indptr, indices, P, a_dst, a_src, G, slope=SLOPE):
    """dict of dP, da_dst, da_src, du, dv, dx for G = dLoss/dZ (float64)."""
    import scipy.sparse as sps
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    a_dst, a_src = np.asarray(a_dst, np.float64), np.asarray(a_src, np.float64)
    n = len(indptr) - 1
    rows, alpha, x = fwd["rows"], fwd["alpha"], fwd["x"]
    c = (G * fwd["Z"]).sum(axis=1)
    t = (G[rows] * P[indices]).sum(axis=1)
    dx = alpha * (t - c[rows]) * np.where(x > 0, 1.0, slope)
    du = np.bincount(rows, weights=dx, minlength=n)
    dv = np.bincount(indices, weights=dx, minlength=n)
    A = sps.csr_matrix((alpha, indices, indptr), shape=(n, n))
    dP = np.asarray(A.T @ G) + np.outer(du, a_dst) + np.outer(dv, a_src)
    return dict(dP=dP, da_dst=du @ P, da_src=dv @ P, du=du, dv=dv, dx=dx)


# --------------------------------------------------------------------------- dropout masks
class Xorshift:
    """hpdga's xorshift128+ (rand.cpp:17-28) from a two-word state."""

    def __init__(self, state):
        self.s0, self.s1 = int(state[0]), int(state[1])

    def draws(self, n):
        out = np.empty(n, np.int64)
        s0, s1, M = self.s0, self.s1, (1 << 64) - 1
        for i in range(n):
            t, u = s0, s1
            s0 = u
            t ^= (t << 23) & M
            t ^= t >> 17
            t ^= u ^ (u >> 26)
            s1 = t
            out[i] = ((t + u) & M) & RAND_MAX
        self.s0, self.s1 = s0, s1
        return out

    def keep(self, n, p):
        """hpdga module.cpp:208-219: keep iff RAND() >= int(p * RAND_MAX), the product in float."""
        thr = int(np.float32(p) * np.float32(RAND_MAX))
        return self.draws(n) >= thr


# --------------------------------------------------------------------------- the model
def _features(ds):
    import scipy.sparse as sps
    return sps.csr_matrix((np.asarray(ds.feat_values, np.float64), np.asarray(ds.feat_indices),
                           np.asarray(ds.feat_indptr)), shape=(ds.num_nodes, ds.input_dim))


class NumpyGatGCN:
    """The L-layer attention model in float64: per layer P = drop(A) W_l, Z = attention(P), hidden
    layers [LayerNorm] -> ReLU -> [+ A on a residual layer]; the loss is softmax cross-entropy, or
    (label_bits given) the per-class sigmoid with binary cross-entropy.
    weights: the engine's W_l; attn: its attention tensor (per layer a_dst then a_src); rng: an
    Xorshift standing behind the engine's initial draws, or None for no dropout."""

    def __init__(self, ds, hidden, weights, attn, dropouts, rng=None, residual=False,
                 layer_norm=False, label_bits=None, indptr=None, indices=None):
        self.ip = np.asarray(ds.graph_indptr if indptr is None else indptr, np.int64)
        self.idx = np.asarray(ds.graph_indices if indices is None else indices, np.int64)
        self.X = _features(ds)
        self.n = ds.num_nodes
        self.dims = [ds.input_dim] + list(hidden) + [ds.output_dim]
        self.L = L = len(self.dims) - 1
        self.W = [np.asarray(w, np.float64).reshape(self.dims[l], self.dims[l + 1])
                  for l, w in enumerate(weights)]
        attn = np.asarray(attn, np.float64)
        self.a, at = [], 0
        for l in range(L):
            d = self.dims[l + 1]
            self.a.append(attn[at:at + 2 * d].copy())  # a_dst then a_src
            at += 2 * d
        assert at == len(attn)
        self.ln = layer_norm
        self.gamma = [np.ones(h) for h in hidden] if layer_norm else []
        self.beta = [np.zeros(h) for h in hidden] if layer_norm else []
        # Adam's tensors in the engine's order: W, [gamma_l, beta_l ...], attention
        self.params = self.W + [t for l in range(len(self.gamma))
                                for t in (self.gamma[l], self.beta[l])] + self.a
        self.m = [np.zeros_like(w) for w in self.params]
        self.v = [np.zeros_like(w) for w in self.params]
        self.t = 0
        self.p, self.rng = list(dropouts), rng
        self.label, self.split = np.asarray(ds.label), np.asarray(ds.split)
        self.bits = None if label_bits is None else np.asarray(label_bits, np.float64)
        self.res = [residual and 1 <= l <= L - 2 and self.dims[l + 1] == self.dims[l]
                    for l in range(L)]

    def _mask(self, shape, p, training):
        """The dropout factor of one module: hpdga draws even at p = 0 (everything kept)."""
        if not training or self.rng is None:
            return None
        n = int(np.prod(shape))
        return self.rng.keep(n, p).reshape(shape) * (1.0 / (1.0 - np.float64(np.float32(p))))

    def forward(self, split, training=False):
        L = self.L
        self.masks, self.A, self.Pm, self.att, self.Y, self.H = [], [], [], [], [], []
        self.xhat, self.rstd = [], []
        h = None
        for l in range(L):
            if l == 0:
                k = self._mask((self.X.nnz,), self.p[0], training)
                if k is None:
                    a_in = self.X
                else:
                    a_in = self.X.copy()
                    a_in.data = a_in.data * k
            else:
                k = self._mask(h.shape, self.p[l], training)
                a_in = h if k is None else h * k
            self.masks.append(k)
            self.A.append(a_in)
            P = np.asarray(a_in @ self.W[l])
            d = self.dims[l + 1]
            f = gat_forward(self.ip, self.idx, P, self.a[l][:d], self.a[l][d:])
            self.Pm.append(P)
            self.att.append(f)
            if l == L - 1:
                break
            y = f["Z"]
            if self.ln:
                mean = y.mean(axis=1, keepdims=True)
                rstd = 1.0 / np.sqrt(((y - mean) ** 2).mean(axis=1, keepdims=True) + LN_EPS)
                xhat = (y - mean) * rstd
                self.xhat.append(xhat)
                self.rstd.append(rstd)
                y = self.gamma[l] * xhat + self.beta[l]
            hn = np.maximum(y, 0.0)
            if self.res[l]:
                hn = hn + self.A[l]
            self.Y.append(y)
            self.H.append(hn)
            h = hn
        logits = self.att[L - 1]["Z"]
        rows = np.nonzero((self.split == split) & (self.label >= 0))[0]
        self.rows, self.logits = rows, logits
        l2 = WD * float((self.W[0] ** 2).sum()) / 2.0
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
        self.dW, self.da, self.dvar1 = [None] * L, [None] * L, [None] * L
        self.dgamma, self.dbeta = [None] * (L - 1), [None] * (L - 1)
        for l in range(L - 1, -1, -1):
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
            else:
                skip = None
            d = self.dims[l + 1]
            b = gat_backward(self.att[l], self.ip, self.idx, self.Pm[l], self.a[l][:d],
                             self.a[l][d:], g)
            self.dvar1[l] = b["dP"]
            self.da[l] = np.concatenate([b["da_dst"], b["da_src"]])
            self.dW[l] = np.asarray(self.A[l].T @ b["dP"])
            if l == 0:
                break
            g = b["dP"] @ self.W[l].T  # dLoss/d drop(H_{l-1})
            if skip is not None:
                g = g + skip
            if self.masks[l] is not None:
                g = g * self.masks[l]

    def attn_grad(self):
        return np.concatenate(self.da)

    def norm_grad(self):
        return np.concatenate([x for l in range(self.L - 1)
                               for x in (self.dgamma[l], self.dbeta[l])])

    def step(self):
        self.t += 1
        ss = LR * np.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t)
        grads = self.dW + [t for l in range(len(self.gamma))
                           for t in (self.dgamma[l], self.dbeta[l])] + self.da
        for k in range(len(self.params)):
            grad = grads[k] + (WD * self.params[k] if k == 0 else 0.0)
            self.m[k] = B1 * self.m[k] + (1.0 - B1) * grad
            self.v[k] = B2 * self.v[k] + (1.0 - B2) * grad * grad
            self.params[k] -= ss * self.m[k] / (np.sqrt(self.v[k]) + EPS)  # in place

    def train_logits(self):
        """The engine's output variable after a training forward: the single-label loss shifts the
        labelled rows by their maximum in place; the multi-label loss leaves them."""
        out = self.logits.copy()
        if self.bits is None:
            out[self.rows] = self.shifted
        return out
