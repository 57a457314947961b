"""The float64 numpy reference of multi-head graph attention with dropout on the attention
weights (pgcn_params.attention_heads / attention_dropout, the pgcn_gat_*_mh kernel entries),
shared by tests/test_cpu_gat_heads.py (which checks it against central differences and against
tests/gat_ref.py), test_gpu_gat_heads_kernels.py and test_gpu_gat_heads.py.  Not a test file.

One layer, K heads concatenated inside the width d: head h owns columns [h dh, (h + 1) dh),
dh = d / K.  With rows(s) = i, cols(s) = j, per head h:
    u_i^h = P_i[h] . a_dst[h],  v_j^h = P_j[h] . a_src[h],  x_s^h = u_i^h + v_j^h
    e = x > 0 ? x : slope x;  alpha_s^h = row softmax of e over the slots of row i
    m'_s^h = keep_s^h scale  (a mask given; else 1)
    Z_i[h] = sum_row alpha_s^h m'_s^h P_j[h]
    c_i^h = G_i[h] . Z_i[h];  t_s^h = G_i[h] . P_j[h]
    dx_s^h = alpha_s^h (m'_s^h t_s^h - c_i^h) (x_s^h > 0 ? 1 : slope)
    du_i^h = sum_row dx^h;  dv_j^h = sum over the slots into column j of dx^h
    dP_j[h] = sum into column j of alpha_s^h m'_s^h G_i[h] + du_j^h a_dst[h] + dv_j^h a_src[h]
    da_dst[h] = sum_i du_i^h P_i[h];  da_src[h] = sum_j dv_j^h P_j[h]
Mask element s K + h belongs to slot s (CSR order) and head h.
"""
import numpy as np

import gat_ref
from gat_ref import SLOPE


def gat_forward_mh(indptr, indices, P, a_dst, a_src, heads, keep=None, scale=1.0, slope=SLOPE):
    """dict of u, v [n][K], x, alpha [nnz][K] (alpha before dropout), mfac [nnz][K] (the factor
    m'), Z [n][d], rows.  keep: [nnz][K] (or flat) booleans, None for no dropout."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    P = np.asarray(P, np.float64)
    a_dst, a_src = np.asarray(a_dst, np.float64), np.asarray(a_src, np.float64)
    n, d = P.shape
    K = int(heads)
    assert d % K == 0
    dh = d // K
    nnz = len(indices)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    Ph = P.reshape(n, K, dh)
    u = (Ph * a_dst.reshape(1, K, dh)).sum(axis=2)
    v = (Ph * a_src.reshape(1, K, dh)).sum(axis=2)
    x = u[rows] + v[indices]
    e = np.where(x > 0, x, slope * x)
    m = np.full((n, K), -np.inf)
    np.maximum.at(m, rows, e)
    w = np.exp(e - m[rows])
    s = np.zeros((n, K))
    np.add.at(s, rows, w)
    alpha = w / s[rows]
    if keep is None:
        mfac = np.ones((nnz, K))
    else:
        mfac = np.asarray(keep, bool).reshape(nnz, K) * np.float64(scale)
    Z = np.zeros((n, K, dh))
    np.add.at(Z, rows, (alpha * mfac)[:, :, None] * Ph[indices])
    return dict(u=u, v=v, x=x, alpha=alpha, mfac=mfac, Z=Z.reshape(n, d), rows=rows, heads=K)


def gat_backward_mh(fwd, indptr, indices, P, a_dst, a_src, G, slope=SLOPE):
    """dict of dP [n][d], da_dst, da_src [d], du, dv [n][K], dx [nnz][K] for G = dLoss/dZ."""
    indices = np.asarray(indices, np.int64)
    P, G = np.asarray(P, np.float64), np.asarray(G, np.float64)
    a_dst, a_src = np.asarray(a_dst, np.float64), np.asarray(a_src, np.float64)
    n, d = P.shape
    K = fwd["heads"]
    dh = d // K
    rows, alpha, x, mfac = fwd["rows"], fwd["alpha"], fwd["x"], fwd["mfac"]
    Ph, Gh, Zh = P.reshape(n, K, dh), G.reshape(n, K, dh), fwd["Z"].reshape(n, K, dh)
    c = (Gh * Zh).sum(axis=2)
    t = (Gh[rows] * Ph[indices]).sum(axis=2)
    dx = alpha * (mfac * t - c[rows]) * np.where(x > 0, 1.0, slope)
    du, dv = np.zeros((n, K)), np.zeros((n, K))
    np.add.at(du, rows, dx)
    np.add.at(dv, indices, dx)
    dP = np.zeros((n, K, dh))
    np.add.at(dP, indices, (alpha * mfac)[:, :, None] * Gh[rows])
    dP += du[:, :, None] * a_dst.reshape(1, K, dh) + dv[:, :, None] * a_src.reshape(1, K, dh)
    da_dst = (du[:, :, None] * Ph).sum(axis=0).reshape(d)
    da_src = (dv[:, :, None] * Ph).sum(axis=0).reshape(d)
    return dict(dP=dP.reshape(n, d), da_dst=da_dst, da_src=da_src, du=du, dv=dv, dx=dx)


class NumpyGatGCN(gat_ref.NumpyGatGCN):
    """gat_ref.NumpyGatGCN with `heads` heads on every hidden layer (the output layer keeps one)
    and dropout `attn_p` on every layer's attention weights.  A training forward consumes one
    block of the xorshift stream: the input dropout's nnz_X draws and each hidden dropout's
    N * h_l (as the base class draws them), then -- attn_p > 0 only -- each attention layer's
    nnz * K_l draws, layer by layer, element s * K_l + h for slot s and head h."""

    def __init__(self, *args, heads=1, attn_p=0.0, **kw):
        super().__init__(*args, **kw)
        self.heads, self.attn_p = int(heads), float(attn_p)

    def layer_heads(self, l):
        return 1 if l == self.L - 1 else self.heads

    def _draw_block(self, training):
        """Every mask of this forward in stream order: (dropout factors per layer, attention keep
        masks per layer)."""
        L, nnz = self.L, len(self.idx)
        drop = [self._mask((self.X.nnz,), self.p[0], training)]
        for l in range(1, L):
            drop.append(self._mask((self.n, self.dims[l]), self.p[l], training))
        keep = [None] * L
        if training and self.rng is not None and self.attn_p > 0:
            keep = [self.rng.keep(nnz * self.layer_heads(l), self.attn_p)
                    .reshape(nnz, self.layer_heads(l)) for l in range(L)]
        return drop, keep

    def forward(self, split, training=False):
        L = self.L
        self.masks, self.A, self.Pm, self.att, self.Y, self.H = [], [], [], [], [], []
        self.xhat, self.rstd = [], []
        drop, keep = self._draw_block(training)
        self.keep = keep
        scale = 1.0 / (1.0 - np.float64(np.float32(self.attn_p)))
        h = None
        for l in range(L):
            k = drop[l]
            if l == 0:
                if k is None:
                    a_in = self.X
                else:
                    a_in = self.X.copy()
                    a_in.data = a_in.data * k
            else:
                a_in = h if k is None else h * k
            self.masks.append(k)
            self.A.append(a_in)
            P = np.asarray(a_in @ self.W[l])
            d = self.dims[l + 1]
            f = gat_forward_mh(self.ip, self.idx, P, self.a[l][:d], self.a[l][d:],
                               self.layer_heads(l), keep=keep[l], scale=scale)
            self.Pm.append(P)
            self.att.append(f)
            if l == L - 1:
                break
            y = f["Z"]
            if self.ln:
                mean = y.mean(axis=1, keepdims=True)
                rstd = 1.0 / np.sqrt(((y - mean) ** 2).mean(axis=1, keepdims=True) + gat_ref.LN_EPS)
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
        return self._loss(split)

    def _loss(self, split):
        """The base class's loss on the last layer's Z (its forward's tail, restated)."""
        logits = self.att[self.L - 1]["Z"]
        rows = np.nonzero((self.split == split) & (self.label >= 0))[0]
        self.rows, self.logits = rows, logits
        l2 = gat_ref.WD * float((self.W[0] ** 2).sum()) / 2.0
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
        """The base class's backward with gat_backward_mh in gat_backward's place."""
        saved = gat_ref.gat_backward
        gat_ref.gat_backward = lambda fwd, ip, idx, P, ad, as_, G: gat_backward_mh(
            fwd, ip, idx, P, ad, as_, G)
        try:
            super().backward()
        finally:
            gat_ref.gat_backward = saved


def pack_bits(keep, base=0, fill=True):
    """keep (flat booleans) as the kernels' bit array: bit base + e of uint64 words (bit b = word
    b // 64, bit b % 64); the bits below base and the tail of the last word are `fill`."""
    keep = np.asarray(keep, bool).ravel()
    total = base + len(keep)
    bits = np.full((total + 63) // 64 * 64 + 64, fill, bool)
    bits[base:total] = keep
    return np.packbits(bits, bitorder="little").view(np.uint64).copy()
