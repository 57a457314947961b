"""Float64 numpy reference of the pair-score kernels (pgcn_link_score_fwd / _bwd) and of an engine
with a link-prediction head (pgcn_params.link_decoder), shared by tests/test_cpu_link.py (which
checks the backward formula against central differences), test_gpu_link_kernels.py and
test_gpu_link.py.  Not a test file.

    forward:   score_e = sum_c H[src_e][c] * H[dst_e][c]
    backward:  dH_i = sum over the selected pairs e of g_e * (1[src_e == i] H[dst_e] +
                                                             1[dst_e == i] H[src_e])

A pair is selected iff select is None or select[e] >= 0; a self pair (i, i) contributes 2 g_e H_i,
a duplicated pair as often as it is listed.
"""
import numpy as np


def score_forward(src, dst, H):
    H = np.asarray(H, np.float64)
    return (H[np.asarray(src)] * H[np.asarray(dst)]).sum(axis=1)


def _selected(n_pairs, select):
    return np.ones(n_pairs, bool) if select is None else np.asarray(select) >= 0


def score_backward(src, dst, H, g, select=None):
    """dH [n][d] (float64) for g [E] = dLoss/dscore; g of an unselected pair is not read."""
    H = np.asarray(H, np.float64)
    src, dst = np.asarray(src), np.asarray(dst)
    on = _selected(len(src), select)
    gs = np.where(on, np.asarray(g, np.float64), 0.0)[on]
    dH = np.zeros_like(H)
    np.add.at(dH, src[on], gs[:, None] * H[dst[on]])
    np.add.at(dH, dst[on], gs[:, None] * H[src[on]])
    return dH


def score_backward_magnitude(src, dst, H, g, select=None):
    """(sum |g_e H_o[c]| [n][d], entries m_i [n]) over every node's incidence entries: the terms of
    the kernel tests' error bound."""
    H = np.abs(np.asarray(H, np.float64))
    src, dst = np.asarray(src), np.asarray(dst)
    on = _selected(len(src), select)
    gs = np.abs(np.where(on, np.asarray(g, np.float64), 0.0))[on]
    mag = np.zeros_like(H)
    np.add.at(mag, src[on], gs[:, None] * H[dst[on]])
    np.add.at(mag, dst[on], gs[:, None] * H[src[on]])
    m = np.bincount(src[on], minlength=H.shape[0]) + np.bincount(dst[on], minlength=H.shape[0])
    return mag, m


def incidence(n, src, dst, select=None):
    """(ptr, pair, other): every node's entries in ascending pair order, the src role of a pair
    before its dst role -- the index pgcn_links_create builds, stated the slow way."""
    lists = [[] for _ in range(n)]
    on = _selected(len(src), select)
    for e, (s, t) in enumerate(zip(src, dst)):
        if on[e]:
            lists[int(s)].append((e, int(t)))
            lists[int(t)].append((e, int(s)))
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    flat = [x for lst in lists for x in lst]
    pair = np.array([x[0] for x in flat], np.int64).reshape(-1)
    other = np.array([x[1] for x in flat], np.int64).reshape(-1)
    return ptr, pair, other


def auc(scores, labels):
    """The ROC area by its definition: P(s_pos > s_neg) + P(s_pos == s_neg) / 2 over all
    positive / negative pairs of labelled entries."""
    s, y = np.asarray(scores, np.float64), np.asarray(labels)
    p, n = s[y == 1], s[y == 0]
    gt = (p[:, None] > n[None, :]).sum()
    eq = (p[:, None] == n[None, :]).sum()
    return float((gt + 0.5 * eq) / (len(p) * len(n)))


# --------------------------------------------------------------------------- the engine model
def ahat_forward(indptr, indices, Q, R=None):
    """Z_i = sum over row i's slots (i, j) of Q_j / sqrt(len_i len_j): the plain engine's Â on the
    pattern as loaded, in float64 (sage_ref.mean_forward's signature)."""
    import sage_ref
    Q = np.asarray(Q, np.float64)
    rows = sage_ref.rows_of(indptr)
    lens = np.diff(indptr).astype(np.float64)
    Z = np.zeros((len(indptr) - 1, Q.shape[1]))
    np.add.at(Z, rows, Q[indices] / np.sqrt(lens[rows] * lens[indices])[:, None])
    return Z if R is None else Z + np.asarray(R, np.float64)


def ahat_backward(indptr, indices, G):
    """dQ_j = sum over the slots (i, j) into column j of G_i / sqrt(len_i len_j)."""
    import sage_ref
    G = np.asarray(G, np.float64)
    rows = sage_ref.rows_of(indptr)
    lens = np.diff(indptr).astype(np.float64)
    dQ = np.zeros_like(G)
    np.add.at(dQ, indices, G[rows] / np.sqrt(lens[rows] * lens[indices])[:, None])
    return dQ


def glorot_attention(pgcn, seed, dims, draws):
    """The engine's initial attention tensor without a device: per layer a_dst[d_l] then
    a_src[d_l], each Glorot-uniform with limit sqrt(6 / (d_l + 1)), drawn from the xorshift stream
    of `seed` right behind the `draws` draws of the layer weights (tests/test_gpu_gat.py checks
    this statement against the engine bit for bit)."""
    import gat_ref
    rng = gat_ref.Xorshift(pgcn.rng_jump(pgcn.rng_seed(seed), draws))
    out = []
    for d in dims[1:]:
        limit = np.sqrt(np.float32(6.0) / np.float32(d + 1))
        for _ in range(2):
            r = rng.draws(d).astype(np.float32) / np.float32(gat_ref.RAND_MAX)
            out.append((((r.astype(np.float64) - 0.5) * np.float64(limit)) * 2.0)
                       .astype(np.float32))
    return np.concatenate(out)


class AhatLayers:
    """sage_ref.NumpySageGCN's mean model with Â in the mean's place (mixed in before it, built
    with aggregator="mean" and no root weight): the plain GCN engine in float64.  The swap is the
    one gat_heads_ref.NumpyGatGCN.backward makes; every call checks that the base class did go
    through the swapped-in functions, once per layer, so a base class that stops looking them up
    fails here instead of quietly computing the mean."""

    def _swapped(self, call):
        import sage_ref
        used = [0]

        def counted(f):
            def g(*args):
                used[0] += 1
                return f(*args)
            return g
        saved = sage_ref.mean_forward, sage_ref.mean_backward
        sage_ref.mean_forward, sage_ref.mean_backward = counted(ahat_forward), \
            counted(ahat_backward)
        try:
            out = call()
        finally:
            sage_ref.mean_forward, sage_ref.mean_backward = saved
        assert used[0] == self.L, "the base class did not aggregate through the swapped functions"
        return out

    def forward(self, split, training=False):
        return self._swapped(lambda: super(AhatLayers, self).forward(split, training))

    def backward(self):
        return self._swapped(lambda: super(AhatLayers, self).backward())


class LinkHead:
    """A link-prediction head on the node models of sage_ref.py / gat_heads_ref.py, by
    subclassing, built the way readout_ref.GraphHead is: the base runs its layers (its node-level
    loss is discarded), the head scores the pairs on the output layer's embedding and computes the
    mean sigmoid BCE over the split's labelled pairs; backward() hands the base class the
    gradient with respect to the embedding through its multi-label first step, g[rows] =
    (sigmoid(x) - y) / count: with every row, count = 1 and y = sigmoid(x) - Gnode that step gives
    Gnode itself (to float64 rounding), and everything behind it is the base class's own code."""

    def set_links(self, src, dst, label, split):
        self.psrc, self.pdst = np.asarray(src, np.int64), np.asarray(dst, np.int64)
        self.plabel, self.psplit = np.asarray(label, np.int64), np.asarray(split, np.int64)
        return self

    def forward(self, split, training=False):
        import gat_ref
        super().forward(split, training)
        self.embed = self.logits
        s = score_forward(self.psrc, self.pdst, self.embed)
        self.scores = s
        pairs = np.nonzero((self.psplit == split) & (self.plabel >= 0))[0]
        self.pairs = pairs
        x, y = s[pairs], (self.plabel[pairs] == 1).astype(np.float64)
        self.acc = float(((x > 0) == (y > 0)).mean())
        l2 = gat_ref.WD * float((self.W[0] ** 2).sum()) / 2.0
        return float((np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).mean()) + l2

    def score_grad(self):
        """dLoss/dscore [E] of the last forward: (sigmoid - y) / count on the split's labelled
        pairs, zero elsewhere."""
        g = np.zeros_like(self.scores)
        x = self.scores[self.pairs]
        y = (self.plabel[self.pairs] == 1).astype(np.float64)
        g[self.pairs] = (1.0 / (1.0 + np.exp(-x)) - y) / len(self.pairs)
        return g

    def backward(self):
        gnode = score_backward(self.psrc, self.pdst, self.embed, self.score_grad())
        self.node_grad = gnode
        x = self.embed
        keep = (self.bits, self.rows, getattr(self, "count", None))
        self.bits = 1.0 / (1.0 + np.exp(-x)) - gnode
        self.rows = np.arange(x.shape[0])
        self.count = 1
        try:
            super().backward()
        finally:
            self.bits, self.rows, self.count = keep

    def near_zero(self, split, rel=1e-5):
        """The split's labelled pairs whose score lies within rel * max|score| of zero: the only
        ones whose verdict a last-bits difference can flip."""
        on = (self.psplit == split) & (self.plabel >= 0)
        return int((on & (np.abs(self.scores) < rel * np.abs(self.scores).max())).sum())


def sage_model(*args, **kw):
    import sage_ref

    class SageLinkModel(LinkHead, sage_ref.NumpySageGCN):
        pass
    return SageLinkModel(*args, **kw)


def gcn_model(*args, **kw):
    import sage_ref

    class GcnLinkModel(LinkHead, AhatLayers, sage_ref.NumpySageGCN):
        pass
    return GcnLinkModel(*args, aggregator="mean", root_weight=False, **kw)


def gat_model(*args, **kw):
    import gat_heads_ref

    class GatLinkModel(LinkHead, gat_heads_ref.NumpyGatGCN):
        pass
    return GatLinkModel(*args, **kw)
