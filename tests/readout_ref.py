"""Float64 numpy reference of the graph-level readouts (pgcn_readout_fwd / _bwd) and of an engine
with a graph-level head (pgcn_params.readout), shared by tests/test_cpu_readout.py (which checks
the backward formulas against central differences), test_gpu_readout_kernels.py and
test_gpu_readout.py.  Not a test file.

Graph g owns the rows [graph_ptr[g], graph_ptr[g + 1]) of a node variable; len_g is that length.

    sum:   out_g = sum of in_i over the range
    mean:  out_g = (1 / len_g) * that sum
    max:   out_g[c] = max over the range of in_i[c]   (arg_g[c]: the lowest such row)

An empty range gives a zero row and arg_g = -1.  Backward, with G = dLoss/dout:

    sum:   din_i = G_graph(i)
    mean:  din_i = G_graph(i) / len
    max:   din_i[c] = G_graph(i)[c] where arg[graph(i)][c] == i, else 0
"""
import numpy as np

MODES = ("sum", "mean", "max")
MODE_ID = {"sum": 1, "mean": 2, "max": 3}


def node_graph(graph_ptr):
    """The range of every row: [n]."""
    graph_ptr = np.asarray(graph_ptr, np.int64)
    return np.repeat(np.arange(len(graph_ptr) - 1), np.diff(graph_ptr))


def readout_forward(graph_ptr, X, mode):
    """(out [G][d], arg [G][d]) in X's dtype arithmetic (sum and mean: pass float64 for the
    reference; the max rounds nothing, so float32 in gives the exact float32 result).  arg is the
    first (lowest-row) argmax of every range and column, -1 for sum, mean and empty ranges."""
    X = np.asarray(X)
    graph_ptr = np.asarray(graph_ptr, np.int64)
    G, d = len(graph_ptr) - 1, X.shape[1]
    out = np.zeros((G, d), X.dtype)
    arg = np.full((G, d), -1, np.int64)
    for g in range(G):
        b, e = int(graph_ptr[g]), int(graph_ptr[g + 1])
        if e <= b:
            continue
        if mode == "max":
            a = X[b:e].argmax(axis=0)  # the first occurrence: the lowest row (-0.0 == +0.0)
            arg[g] = b + a
            out[g] = X[b + a, np.arange(d)]
        else:
            out[g] = X[b:e].sum(axis=0)
            if mode == "mean":
                out[g] = out[g] / (e - b)
    return out, arg


def readout_backward(graph_ptr, Gout, mode, arg=None):
    """din [n][d] (float64) for Gout = dLoss/dout."""
    Gout = np.asarray(Gout, np.float64)
    graph_ptr = np.asarray(graph_ptr, np.int64)
    ng = node_graph(graph_ptr)
    din = Gout[ng]
    if mode == "mean":
        din = din / np.diff(graph_ptr)[ng][:, None]
    elif mode == "max":
        rows = np.arange(len(ng))[:, None]
        din = np.where(np.asarray(arg)[ng] == rows, din, 0.0)
    return din


def max_margin(graph_ptr, X):
    """Per element (g, c): the gap between the largest and the second largest row value of the
    range (inf for ranges of fewer than two rows; 0 on an exact tie)."""
    X = np.asarray(X, np.float64)
    graph_ptr = np.asarray(graph_ptr, np.int64)
    G = len(graph_ptr) - 1
    gap = np.full((G, X.shape[1]), np.inf)
    for g in range(G):
        b, e = int(graph_ptr[g]), int(graph_ptr[g + 1])
        if e - b >= 2:
            top = np.sort(X[b:e], axis=0)[-2:]
            gap[g] = top[1] - top[0]
    return gap


# --------------------------------------------------------------------------- the engine model
class GraphHead:
    """A graph-level head on the node models of gat_ref.py / sage_ref.py, by subclassing: the
    model's layers run unchanged on the batch, the readout pools the output layer's node logits
    and the softmax cross-entropy runs over the graphs of the split.

    The base classes compute their loss inside forward() and start backward() from the loss
    gradient they derive themselves.  forward() here lets the base run (its node-level loss is
    discarded), then computes the pooled loss from self.logits.  backward() hands the base class
    the gradient with respect to the node logits through its multi-label first step, g[rows] =
    (sigmoid(x) - y) / count: with every row, count = 1 and y = sigmoid(x) - Gnode that step gives
    Gnode itself (to float64 rounding), and everything behind it is the base class's own code."""

    def set_graphs(self, graph_ptr, graph_label, graph_split, mode):
        assert mode in MODES
        self.gp = np.asarray(graph_ptr, np.int64)
        self.glabel = np.asarray(graph_label, np.int64)
        self.gsplit = np.asarray(graph_split, np.int64)
        self.mode = mode
        return self

    def forward(self, split, training=False):
        import gat_ref
        super().forward(split, training)
        self.node_logits = self.logits
        pooled, arg = readout_forward(self.gp, self.node_logits, self.mode)
        self.pooled, self.parg = pooled, arg
        self.pool_gap = max_margin(self.gp, self.node_logits) if self.mode == "max" else None
        graphs = np.nonzero((self.gsplit == split) & (self.glabel >= 0))[0]
        self.graphs = graphs
        zr = pooled[graphs] - pooled[graphs].max(axis=1, keepdims=True)
        lse = np.log(np.exp(zr).sum(axis=1))
        t = self.glabel[graphs]
        self.gshifted, self.glse = zr, lse
        self.acc = float((zr.argmax(axis=1) == t).mean())
        l2 = gat_ref.WD * float((self.W[0] ** 2).sum()) / 2.0
        return float((lse - zr[np.arange(len(graphs)), t]).mean()) + l2

    def pooled_grad(self):
        """dLoss/dpooled [G][C] of the last forward: (softmax - 1[t]) / count on the split's
        labelled graphs, zero elsewhere."""
        g = np.zeros_like(self.pooled)
        p = np.exp(self.gshifted - self.glse[:, None])
        p[np.arange(len(self.graphs)), self.glabel[self.graphs]] -= 1.0
        g[self.graphs] = p / len(self.graphs)
        return g

    def backward(self):
        gnode = readout_backward(self.gp, self.pooled_grad(), self.mode, self.parg)
        self.node_grad = gnode
        x = self.node_logits
        keep = (self.bits, self.rows, getattr(self, "count", None))
        self.bits = 1.0 / (1.0 + np.exp(-x)) - gnode
        self.rows = np.arange(x.shape[0])
        self.count = 1
        try:
            super().backward()
        finally:
            self.bits, self.rows, self.count = keep

    def predict(self):
        """argmax of the pooled logits of the last forward (the lowest index of equal values)."""
        return self.pooled.argmax(axis=1)

    def pool_near_tied(self, rel):
        """max only: the (graph, class) elements whose top two rows lie within rel * max|logit| of
        each other without being an exact tie."""
        return (self.pool_gap > 0) & (self.pool_gap < rel * np.abs(self.node_logits).max())


def sage_model(*args, **kw):
    import sage_ref

    class SageGraphModel(GraphHead, sage_ref.NumpySageGCN):
        pass
    return SageGraphModel(*args, **kw)


def gat_model(*args, **kw):
    import gat_ref

    class GatGraphModel(GraphHead, gat_ref.NumpyGatGCN):
        pass
    return GatGraphModel(*args, **kw)
