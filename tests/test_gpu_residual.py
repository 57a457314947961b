"""Residual connections of the L-layer model (pgcn_params.residual; the reference's
ResidualConnection, include/module.cuh:149-161, with a real backward), fused into GraphSum's
final write (gs_epilogue.hpp).

A residual layer is a middle layer 1 <= l <= L-2 as wide as the layer before it:
    Z_l = Â (A_{l-1} W_l),  H_l = relu(Z_l) + A_{l-1}          (A: the layer's input as it read it)
    dZ_l = G * [Z_l > 0],   dA_{l-1} = (Â dZ_l) W_l^T + G       (G = dLoss/dH_l)
The numeric reference is a float64 numpy restatement of that model in this file (the oracle has
no residual model): dense algebra on scipy CSR matrices, the mean cross entropy over the split,
wd * sum(W0^2) / 2 in the loss and wd * W0 in W0's Adam gradient, hpdga's Adam (conventions of
oracle/pgcn_oracle.c).  It starts from the engine's initial weights.
"""
import ctypes

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

LR, WD, B1, B2, EPS = 0.01, 5e-4, 0.9, 0.999, 1e-8


def _var1(l):
    return 1 + 3 * l


def _w(l):
    return 2 + 3 * l


def _var2(l):
    return 3 + 3 * l


def _ahat(ds):
    """Â in float64: hpdga's coefficient 1 / sqrt(deg_i * deg_j) per stored slot."""
    import scipy.sparse as sps
    ip = np.asarray(ds.graph_indptr, np.int64)
    idx = np.asarray(ds.graph_indices, np.int64)
    deg = np.diff(ip).astype(np.float64)
    rows = np.repeat(np.arange(len(deg)), np.diff(ip))
    vals = 1.0 / np.sqrt(deg[rows] * deg[idx])
    n = ds.num_nodes
    return sps.csr_matrix((vals, idx, ip), shape=(n, n))


def _features(ds):
    import scipy.sparse as sps
    return sps.csr_matrix((np.asarray(ds.feat_values, np.float64), np.asarray(ds.feat_indices),
                           np.asarray(ds.feat_indptr)), shape=(ds.num_nodes, ds.input_dim))


class NumpyResidualGCN:
    """The residual model without dropout, float64.  reassociated: the engine's output layer
    runs as (Â H) W, so its var1 is Â H (else H W); the logits are the same product."""

    def __init__(self, ds, hidden, weights, reassociated):
        self.A, self.X = _ahat(ds), _features(ds)
        self.dims = [ds.input_dim] + list(hidden) + [ds.output_dim]
        self.L = len(self.dims) - 1
        self.W = [np.asarray(w, np.float64).reshape(self.dims[l], self.dims[l + 1])
                  for l, w in enumerate(weights)]
        self.m = [np.zeros_like(w) for w in self.W]
        self.v = [np.zeros_like(w) for w in self.W]
        self.t = 0
        self.label, self.split = np.asarray(ds.label), np.asarray(ds.split)
        self.re = reassociated
        self.res = [1 <= l <= self.L - 2 and self.dims[l + 1] == self.dims[l]
                    for l in range(self.L)]

    def forward(self, split):
        A, L = self.A, self.L
        self.Z, self.H = [], []
        h = None
        for l in range(L - 1):
            z = A @ ((self.X @ self.W[0]) if l == 0 else (h @ self.W[l]))
            hn = np.maximum(z, 0.0)
            if self.res[l]:
                hn = hn + h
            self.Z.append(z)
            self.H.append(hn)
            h = hn
        if self.re:
            self.last_var1 = A @ h
            logits = self.last_var1 @ self.W[L - 1]
        else:
            self.last_var1 = h @ self.W[L - 1]
            logits = A @ self.last_var1
        rows = np.nonzero((self.split == split) & (self.label >= 0))[0]
        zr = logits[rows] - logits[rows].max(axis=1, keepdims=True)
        lse = np.log(np.exp(zr).sum(axis=1))
        t = self.label[rows]
        loss = float((lse - zr[np.arange(len(rows)), t]).mean())
        self.rows, self.shifted, self.lse, self.logits = rows, zr, lse, logits
        return loss + WD * float((self.W[0] ** 2).sum()) / 2.0

    def backward(self):
        A, L = self.A, self.L
        rows = self.rows
        d_out = np.zeros_like(self.logits)
        p = np.exp(self.shifted - self.lse[:, None])
        p[np.arange(len(rows)), self.label[rows]] -= 1.0
        d_out[rows] = p / len(rows)
        self.dW = [None] * L
        self.dvar1 = [None] * L
        h_last = self.H[L - 2]
        if self.re:
            self.dW[L - 1] = self.last_var1.T @ d_out
            self.dvar1[L - 1] = d_out @ self.W[L - 1].T
            g = A @ self.dvar1[L - 1]
        else:
            self.dvar1[L - 1] = A @ d_out
            self.dW[L - 1] = h_last.T @ self.dvar1[L - 1]
            g = self.dvar1[L - 1] @ self.W[L - 1].T
        for l in range(L - 2, -1, -1):
            dz = g * (self.Z[l] > 0)
            self.dvar1[l] = A @ dz
            if l == 0:
                self.dW[0] = np.asarray(self.X.T @ self.dvar1[0])
                break
            self.dW[l] = self.H[l - 1].T @ self.dvar1[l]
            g = self.dvar1[l] @ self.W[l].T + (g if self.res[l] else 0.0)

    def step(self):
        self.t += 1
        ss = LR * np.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t)
        for l in range(self.L):
            grad = self.dW[l] + (WD * self.W[l] if l == 0 else 0.0)
            self.m[l] = B1 * self.m[l] + (1.0 - B1) * grad
            self.v[l] = B2 * self.v[l] + (1.0 - B2) * grad * grad
            self.W[l] = self.W[l] - ss * self.m[l] / (np.sqrt(self.v[l]) + EPS)

    def train_logits(self):
        """The output variable after a training forward: labelled rows max-shifted in place."""
        out = self.logits.copy()
        out[self.rows] = self.shifted
        return out


@pytest.mark.parametrize("name,hidden", [("cora", (16, 16, 16)), ("citeseer", (128, 128, 128))])
def test_numeric_parity_no_dropout(loaded, pgcn, name, hidden):
    """Logits, every var2, every weight gradient and every var1.grad after one train_epoch, then
    train and val loss over 5 epochs, against the float64 numpy model.  cora: the plain gather
    kernels at d = 16, the output layer reassociated (its prestaged input is the post-add
    value); citeseer: the wide 16-column passes (col0 != 0)."""
    ds = loaded[name]
    L = len(hidden) + 1
    p = pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.0,) * L, residual=True)
    g = pgcn.GCN(p, ds)
    assert g.query("residual_layers") == 2
    w0 = [g.get_var(_w(l)) for l in range(L)]
    ref = NumpyResidualGCN(ds, hidden, w0, g.query("reassociated") == 1)
    tl = g.train_epoch()[0]
    want_tl = ref.forward(1)
    ref.backward()
    n, c = ds.num_nodes, ds.output_dim
    print(f"{name}: train loss {tl:.9g} numpy {want_tl:.9g}")
    np.testing.assert_allclose(g.get_var(_var2(L - 1)).reshape(n, c), ref.train_logits(),
                               rtol=1e-4, atol=1e-6, err_msg="logits")
    for l in range(L - 1):
        np.testing.assert_allclose(g.get_var(_var2(l)).reshape(n, -1), ref.H[l], rtol=1e-4,
                                   atol=1e-6, err_msg=f"var2 of layer {l}")
    for l in range(L):
        np.testing.assert_allclose(g.get_var(_w(l), 1).reshape(ref.dW[l].shape), ref.dW[l],
                                   rtol=1e-4, atol=1e-7, err_msg=f"W{l} grad")
        np.testing.assert_allclose(g.get_var(_var1(l), 1).reshape(n, -1), ref.dvar1[l], rtol=1e-4,
                                   atol=1e-7, err_msg=f"var1.grad of layer {l}")
    for e in range(5):
        if e:
            tl = g.train_epoch()[0]
            want_tl = ref.forward(1)
            ref.backward()
        ref.step()
        vl, want_vl = g.eval(2)[0], ref.forward(2)
        print(f"{name} epoch {e + 1}: train {tl:.9g} / {want_tl:.9g}  val {vl:.9g} / {want_vl:.9g}")
        assert abs(tl - want_tl) <= 1e-4 * abs(want_tl), (e, tl, want_tl)
        assert abs(vl - want_vl) <= 1e-4 * abs(want_vl), (e, vl, want_vl)
    g.close()


def test_semantics_under_dropout(loaded, pgcn):
    """Dropped prev, add before the next dropout, without knowing the masks: with A = var2 of
    layer l-1 as stored after the epoch (dropped in place by layer l's Dropout) and W_l as the
    forward used it (read before the epoch: Adam has stepped it since), every element of var2_l
    is 0 or S / (1 - p) for S = relu(Â A W_l) + A, and the share of zeros where S != 0 is p."""
    ds, hidden, pd = loaded["cora"], (16, 16, 16), 0.5
    p = pgcn.make_params(ds, hidden_dims=hidden, dropouts=(pd,) * 4, residual=True)
    g = pgcn.GCN(p, ds)
    w = [g.get_var(_w(l)).astype(np.float64).reshape(16, 16) for l in (1, 2)]
    g.train_epoch()
    A = _ahat(ds)
    n = ds.num_nodes
    for l in (1, 2):
        a = g.get_var(_var2(l - 1)).astype(np.float64).reshape(n, 16)
        s = np.maximum(A @ (a @ w[l - 1]), 0.0) + a
        got = g.get_var(_var2(l)).astype(np.float64).reshape(n, 16)
        kept = s / (1.0 - pd)
        ok = (got == 0.0) | (np.abs(got - kept) <= 1e-4 * np.abs(kept) + 1e-6)
        assert ok.all(), (l, int((~ok).sum()))
        live = np.abs(s) > 1e-6
        share = float((got[live] == 0.0).mean())
        print(f"layer {l}: zero share {share:.4f} of {int(live.sum())}")
        assert abs(share - pd) <= 0.03, (l, share)
    g.close()


FUSE_CASES = {
    "cora": (None, (16, 16, 16)),
    "lds_deep": ((70000, 32, 41, 600000, 23), (128, 128, 128)),   # LDS ring, the wide combine
    "lds_d16": ((120000, 64, 41, 1500000, 21), (16, 16)),         # LDS ring, prestaged table
}


def _res_run(pgcn, ds, hidden, fuse, epochs=4, **kn):
    L = len(hidden) + 1
    with helpers.knobs(pgcn, fuse_epilogue=fuse, **kn):
        g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * L,
                                      residual=True), ds)
        lines = [g.train_epoch() + g.eval(2) for _ in range(epochs)]
        g.train_epoch()
        out = dict(lines=np.array(lines, np.float32), layers=g.query("residual_layers"),
                   fused=g.query("fused_residuals"),
                   vars=[g.get_var(i) for l in range(L - 1) for i in (_var1(l), _var2(l))],
                   grads=[g.get_var(i, 1) for l in range(L - 1) for i in (_var1(l), _var2(l))],
                   wgrads=[g.get_var(_w(l), 1) for l in range(L)])
        g.close()
    return out


@pytest.mark.parametrize("case", sorted(FUSE_CASES))
def test_fused_residual_bit_identical(loaded, pgcn, case):
    """The add inside the GraphSum's final write (fuse_epilogue 15) against the separate
    launches (0) and the partial settings 13 / 11 / 7: epoch lines over 4 epochs, the hidden
    variables and every gradient, bit for bit."""
    syn, hidden = FUSE_CASES[case]
    ds = loaded["cora"] if syn is None else pgcn.Dataset.synthetic(*syn)
    on = _res_run(pgcn, ds, hidden, 15)
    want_layers = len(hidden) - 1
    assert on["layers"] == want_layers and on["fused"] == want_layers
    for fuse in (0, 13, 11, 7):
        other = _res_run(pgcn, ds, hidden, fuse)
        assert other["layers"] == want_layers
        if fuse == 0:
            assert other["fused"] == 0
        np.testing.assert_array_equal(on["lines"], other["lines"], err_msg=f"fuse {fuse}")
        for k in ("vars", "grads", "wgrads"):
            for i, (a, b) in enumerate(zip(on[k], other[k])):
                np.testing.assert_array_equal(a, b, err_msg=f"fuse {fuse} {k}[{i}]")


@pytest.mark.parametrize("sparse_dual", [1, 0])
def test_epoch_graph_residual_cora(loaded, pgcn, sparse_dual):
    """Three epoch_async calls with epoch_graph 1 equal the eager ones bit for bit (sparse_dual
    0: the setting with which a sparse-feature engine does capture its epoch)."""
    ds, hidden = loaded["cora"], (16, 16, 16)
    runs = []
    for on in (0, 1):
        with helpers.knobs(pgcn, epoch_graph=on, sparse_dual=sparse_dual):
            g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * 4,
                                          residual=True), ds)
            for _ in range(3):
                g.epoch_async()
            runs.append((g.results(3), [g.get_var(_w(l)) for l in range(4)],
                         g.query("fused_residuals")))
            g.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(a, b)
    assert runs[0][2] == runs[1][2] == 2


def _lines(g, n):
    return np.array([g.train_epoch() + g.eval(2) for _ in range(n)], np.float32)


def test_which_layers(loaded, pgcn, tmp_path):
    ds = loaded["cora"]
    hidden = (16, 32, 32, 8)
    runs = []
    for res in (True, False):
        g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * 5, residual=res),
                     ds)
        assert g.query("residual_layers") == (1 if res else 0)
        runs.append(_lines(g, 3))
        g.close()
    assert not np.array_equal(runs[0], runs[1])
    # L = 2: no middle layer, the plain engine bit for bit
    out = []
    for res in (True, False):
        g = pgcn.GCN(pgcn.make_params(ds, residual=res), ds)
        assert g.query("residual_layers") == 0 and g.query("fused_residuals") == 0
        lines = _lines(g, 4)
        path = str(tmp_path / f"l2_{int(res)}.pgcnck")
        g.save(path)
        out.append((lines, g.get_var(2), g.get_var(5), open(path, "rb").read()))
        g.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    np.testing.assert_array_equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3]
    assert pgcn.checkpoint_flags(str(tmp_path / "l2_1.pgcnck")) == 0


EDGE_CASES = {"cora": (None, (16, 16, 16), 1e-5),
              "lds_deep": ((70000, 32, 41, 600000, 23), (128, 128, 128), helpers.DEEP_TIE_TOL)}


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_edge_cut_matches_one_gpu(loaded, pgcn, case):
    """Loopback ranks at world 2 and the world-1 dist engine against the one-GPU residual
    engine (validated against numpy above) at tests/test_gpu_multirank.py's tolerances: losses
    1e-4 relative, accuracies within the reference run's near-tied rows."""
    syn, hidden, tie_tol = EDGE_CASES[case]
    ds = loaded["cora"] if syn is None else pgcn.Dataset.synthetic(*syn)
    L, epochs = len(hidden) + 1, 3
    p = pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * L, residual=True)
    cnt = helpers.split_counts(ds)
    c = ds.output_dim
    one = pgcn.GCN(p, ds)
    assert one.query("residual_layers") == 2
    want, ties = [], []
    for _ in range(epochs):
        tr = one.train_epoch()
        t1 = helpers.near_ties(one.get_var(_var2(L - 1)), ds.label, ds.split, 1, c, tie_tol)
        ev = one.eval(2)
        t2 = helpers.near_ties(one.get_var(_var2(L - 1)), ds.label, ds.split, 2, c, tie_tol)
        want.append(tr + ev)
        ties.append({1: t1, 2: t2})
    one.close()

    group = pgcn.LoopbackGroup(2)

    def rank_fn(r):
        g = pgcn.GCN(p, ds, device=0, rank=r, loopback=group)
        out = (g.query("residual_layers"), [g.train_epoch() + g.eval(2) for _ in range(epochs)],
               g.query("fused_residuals"))
        g.close()
        return out
    res = pgcn.run_ranks(2, rank_fn)
    np.testing.assert_array_equal(np.asarray(res[0][1]), np.asarray(res[1][1]))
    assert res[0][0] == 2 and res[1][0] == 2
    cut = pgcn.GCN(p, ds, device=0, rank=0, world=1, unique_id=pgcn.comm_unique_id())
    assert cut.query("residual_layers") == 2
    dist = [cut.train_epoch() + cut.eval(2) for _ in range(epochs)]
    cut.close()
    for what, lines in (("loopback 2", res[0][1]), ("dist world 1", dist)):
        for e in range(epochs):
            print(what, e + 1, lines[e], want[e])
            helpers.assert_line_close(lines[e], want[e], cnt, what=f"{what} epoch {e + 1}",
                                      ties=ties[e])


def test_engine_services(loaded, pgcn, tmp_path):
    """save -> 3 epochs -> load -> 3 epochs reproduces the lines; predict between epochs leaves
    training as it was; a residual file is refused by a plain engine and the other way round
    (PGCN_E_INVALID, the engine untouched); a weights-only load crosses the mismatch."""
    ds, hidden = loaded["cora"], (16, 16, 16)

    def make(res):
        return pgcn.GCN(pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * 4,
                                         residual=res), ds)
    paths = {}
    for res in (True, False):
        g = make(res)
        _lines(g, 2)
        paths[res] = str(tmp_path / f"r{int(res)}.pgcnck")
        g.save(paths[res])
        assert pgcn.checkpoint_flags(paths[res]) == (1 if res else 0)
        if res:
            a = _lines(g, 3)
            g.load(paths[res])
            np.testing.assert_array_equal(a, _lines(g, 3))
        g.close()
    # predict between epochs
    g1, g2 = make(True), make(True)
    for _ in range(3):
        np.testing.assert_array_equal(_lines(g1, 1), _lines(g2, 1))
        cls, conf = g1.predict()
        assert cls.shape == (ds.num_nodes,) and np.isfinite(conf).all()
    np.testing.assert_array_equal(g1.get_var(_w(2)), g2.get_var(_w(2)))
    g1.close()
    g2.close()
    # refusals, both directions
    for res in (True, False):
        g, twin = make(res), make(res)
        np.testing.assert_array_equal(_lines(g, 1), _lines(twin, 1))
        with pytest.raises(pgcn.PgcnError) as e:
            g.load(paths[not res])
        assert e.value.status == pgcn.PGCN_E_INVALID
        np.testing.assert_array_equal(_lines(g, 1), _lines(twin, 1))
        g.load(paths[not res], weights_only=True)
        info = pgcn.checkpoint_info(paths[not res])
        assert info["n_layers"] == 4 and g.query("adam_steps") == 0
        other = make(not res)
        other.load(paths[not res])
        for l in range(4):
            np.testing.assert_array_equal(g.get_var(_w(l)), other.get_var(_w(l)))
        assert np.isfinite(_lines(g, 1)).all()
        for x in (g, twin, other):
            x.close()


@pytest.mark.parametrize("n", [1, 3, 4, 4097])
@pytest.mark.parametrize("offset", [0, 1])
def test_kernel_abi(pgcn, n, offset):
    """pgcn_residual_fwd / pgcn_residual_bwd: one fp32 add per element, exactly numpy's, for
    sizes around the float4 body and a pointer off the 16-byte grid."""
    import torch
    rng = np.random.default_rng(n + offset)
    for fn in (pgcn.lib.pgcn_residual_fwd, pgcn.lib.pgcn_residual_bwd):
        y = rng.standard_normal(n + 8).astype(np.float32)
        x = rng.standard_normal(n + 8).astype(np.float32)
        dy, dx = torch.from_numpy(y).cuda(), torch.from_numpy(x).cuda()
        torch.cuda.synchronize()
        st = fn(ctypes.c_void_p(dy.data_ptr() + 4 * offset),
                ctypes.c_void_p(dx.data_ptr() + 4 * offset), n, None)
        assert st == pgcn.PGCN_OK
        torch.cuda.synchronize()
        want = y.copy()
        want[offset:offset + n] = y[offset:offset + n] + x[offset:offset + n]
        np.testing.assert_array_equal(dy.cpu().numpy(), want)  # nothing outside [offset, +n)
        np.testing.assert_array_equal(dx.cpu().numpy(), x)
