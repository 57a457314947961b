"""The multi-label engine (pgcn_params.multilabel): sigmoid + binary cross-entropy behind the
output layer, the label bit matrix, Hamming accuracy, thresholded prediction, per-class counts
and F1, checkpoints, and the refusals.

With the labelled rows of the split (label >= 0), logits x, targets y and count = rows * C:
    loss = sum [ max(x, 0) - x y + log1p(exp(-|x|)) ] / count + wd * sum W0^2 / 2
    grad = (sigmoid(x) - y) / count;   acc = 1 - #{(x > 0) != y} / count
The numeric reference is a float64 numpy restatement in this file (the oracle has no such model)
with the conventions of tests/test_gpu_layernorm.py: dense algebra on scipy CSR matrices, no
dropout, hpdga's Adam with weight decay on W0 only, started from the engine's initial weights.
"""
import ctypes

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

LR, WD, B1, B2, EPS = 0.01, 5e-4, 0.9, 0.999, 1e-8
LN_EPS = 1e-5


def _w(l):
    return 2 + 3 * l


def _var2(l):
    return 3 + 3 * l


def _ahat(ds):
    import scipy.sparse as sps
    ip = np.asarray(ds.graph_indptr, np.int64)
    idx = np.asarray(ds.graph_indices, np.int64)
    deg = np.diff(ip).astype(np.float64)
    rows = np.repeat(np.arange(len(deg)), np.diff(ip))
    vals = 1.0 / np.sqrt(deg[rows] * deg[idx])
    return sps.csr_matrix((vals, idx, ip), shape=(ds.num_nodes, ds.num_nodes))


def _features(ds):
    import scipy.sparse as sps
    return sps.csr_matrix((np.asarray(ds.feat_values, np.float64), np.asarray(ds.feat_indices),
                           np.asarray(ds.feat_indptr)), shape=(ds.num_nodes, ds.input_dim))


class NumpyMultilabelGCN:
    """float64, no dropout; optional residual layers and LayerNorm (forward only for those)."""

    def __init__(self, ds, Y, hidden, weights, residual=False, layer_norm=False):
        self.A, self.X = _ahat(ds), _features(ds)
        self.Y = np.asarray(Y, np.float64)
        self.C = self.Y.shape[1]
        self.dims = [ds.input_dim] + list(hidden) + [self.C]
        self.L = len(self.dims) - 1
        self.W = [np.asarray(w, np.float64).reshape(self.dims[l], self.dims[l + 1])
                  for l, w in enumerate(weights)]
        self.m = [np.zeros_like(w) for w in self.W]
        self.v = [np.zeros_like(w) for w in self.W]
        self.t = 0
        self.label, self.split = np.asarray(ds.label), np.asarray(ds.split)
        self.ln = layer_norm
        self.res = [residual and 1 <= l <= self.L - 2 and self.dims[l + 1] == self.dims[l]
                    for l in range(self.L)]

    def forward(self, split):
        """(loss, Hamming accuracy) of the split."""
        A, L = self.A, self.L
        self.Z, self.H = [], []
        h = None
        for l in range(L - 1):
            z = A @ (np.asarray(self.X @ self.W[0]) if l == 0 else (h @ self.W[l]))
            if self.ln:  # gamma = 1, beta = 0 (the start values)
                mean = z.mean(axis=1, keepdims=True)
                z = (z - mean) / np.sqrt(((z - mean) ** 2).mean(axis=1, keepdims=True) + LN_EPS)
            hn = np.maximum(z, 0.0)
            if self.res[l]:
                hn = hn + h
            self.Z.append(z)
            self.H.append(hn)
            h = hn
        x = A @ (h @ self.W[L - 1])
        rows = np.nonzero((self.split == split) & (self.label >= 0))[0]
        xr, yr = x[rows], self.Y[rows]
        e = np.exp(-np.abs(xr))
        count = len(rows) * self.C
        loss = float((np.maximum(xr, 0.0) - xr * yr + np.log1p(e)).sum()) / count
        wrong = int(((xr > 0) != (yr > 0.5)).sum())
        self.rows, self.logits, self.count = rows, x, count
        self.sig = np.where(xr >= 0, 1.0, e) / (1.0 + e)
        return loss + WD * float((self.W[0] ** 2).sum()) / 2.0, (count - wrong) / count

    def backward(self):
        assert not self.ln
        A, L = self.A, self.L
        d_out = np.zeros_like(self.logits)
        d_out[self.rows] = (self.sig - self.Y[self.rows]) / self.count
        self.dW = [None] * L
        dvar1 = A @ d_out
        self.dW[L - 1] = self.H[L - 2].T @ dvar1
        g = dvar1 @ self.W[L - 1].T
        for l in range(L - 2, -1, -1):
            dvar1 = A @ (g * (self.Z[l] > 0))
            if l == 0:
                self.dW[0] = np.asarray(self.X.T @ dvar1)
                break
            self.dW[l] = self.H[l - 1].T @ dvar1
            g = dvar1 @ self.W[l].T + (g if self.res[l] else 0.0)

    def step(self):
        self.t += 1
        ss = LR * np.sqrt(1.0 - B2 ** self.t) / (1.0 - B1 ** self.t)
        for k in range(self.L):
            grad = self.dW[k] + (WD * self.W[k] if k == 0 else 0.0)
            self.m[k] = B1 * self.m[k] + (1.0 - B1) * grad
            self.v[k] = B2 * self.v[k] + (1.0 - B2) * grad * grad
            self.W[k] -= ss * self.m[k] / (np.sqrt(self.v[k]) + EPS)

    def closest(self):
        """(min |pre-activation|, min |labelled logit|) of the last forward, each relative to
        the largest of its tensor: a value that near zero could flip a ReLU mask or a
        thresholded class between fp32 and float64 (an fp32 sum of k <= 100 products is
        typically within sqrt(k) 2^-24 = 6e-7 of its terms' scale, itself below the largest).
        Exact zeros do not count: they come from all-zero ReLU rows, zero in fp32 as well."""
        def rel(a, scale):
            a = np.abs(a[a != 0])
            return float(a.min() / scale) if a.size else 1.0
        return (min(rel(z, np.abs(z).max()) for z in self.Z),
                rel(self.logits[self.rows], np.abs(self.logits).max()))


def _label_matrix(n, c, seed):
    return np.random.default_rng(seed).random((n, c)) < 0.3


@pytest.fixture(scope="module")
def data(pgcn):
    """name -> (dataset, Y): synthetic n = 300, F = 24 with C = 5 and C = 41, and cora's graph
    and features with a seeded 7-class matrix (a second load: the session's cora stays as is)."""
    out = {}
    for c in (5, 41):
        ds = pgcn.Dataset.synthetic(300, 24, c, 900, 17 + c)
        Y = _label_matrix(300, c, 100 + c)
        ds.set_multilabel(Y)
        out[f"syn{c}"] = (ds, Y)
    return out


@pytest.fixture(scope="module")
def cora_ml(pgcn, datasets):
    root, names = datasets
    ds = pgcn.Dataset.load(root, names["cora"])
    Y = _label_matrix(ds.num_nodes, 7, 7)
    ds.set_multilabel(Y)
    assert ds.output_dim == 7
    return ds, Y


def _get(name, data, cora_ml):
    return cora_ml if name == "cora" else data[name]


def _params(pgcn, ds, hidden=(16,), drop=0.0, **kw):
    L = len(hidden) + 1
    return pgcn.make_params(ds, hidden_dims=hidden, dropouts=(drop,) * L, multilabel=True, **kw)


def _tie_free(pgcn, ds, Y, hidden=(16,), **kw):
    """The first seed in 1..16 whose float64 first training forward keeps every hidden
    pre-activation and every labelled logit at least 2e-6 of its tensor's largest value from
    zero (three times closest()'s fp32 error) -- a condition on the reference alone."""
    L = len(hidden) + 1
    for seed in range(1, 17):
        g = pgcn.GCN(_params(pgcn, ds, hidden, seed=seed, **kw), ds)
        ref = NumpyMultilabelGCN(ds, Y, hidden, [g.get_var(_w(l)) for l in range(L)], **kw)
        ref.forward(1)
        z, x = ref.closest()
        print(f"seed {seed}: min |Z| / max {z:.3g} min |logit| / max {x:.3g}")
        if z >= 2e-6 and x >= 2e-6:
            return g, ref
        g.close()
    raise AssertionError("no seed in 1..16 without a value within 2e-6 (relative) of zero")


@pytest.mark.parametrize("name", ["syn5", "syn41", "cora"])
def test_forward_gradients_and_five_epochs(pgcn, data, cora_ml, name):
    """First train_epoch: loss at 1e-4 relative, Hamming accuracy exact, every weight gradient
    within 1e-4 of its tensor's largest entry; then five epochs of train and validation loss
    follow the float64 model with hpdga's Adam at 1e-4 relative.  get_var of the logits
    variable holds raw logits (nothing shifted)."""
    ds, Y = _get(name, data, cora_ml)
    g, ref = _tie_free(pgcn, ds, Y)
    assert g.query("multilabel") == 1
    tl, ta = g.train_epoch()
    want_tl, want_ta = ref.forward(1)
    ref.backward()
    print(f"{name}: train loss {tl:.9g} / {want_tl:.9g} acc {ta:.9g} / {want_ta:.9g}")
    assert abs(tl - want_tl) <= 1e-4 * abs(want_tl)
    assert ta == np.float32(np.float32(round(want_ta * ref.count)) / np.float32(ref.count))
    np.testing.assert_allclose(g.get_var(_var2(1)).reshape(ds.num_nodes, -1), ref.logits,
                               rtol=1e-4, atol=1e-6, err_msg="raw logits")
    for l in range(2):
        got = g.get_var(_w(l), 1).reshape(ref.dW[l].shape)
        err = np.abs(got - ref.dW[l]).max() / np.abs(ref.dW[l]).max()
        print(f"W{l} grad: error {err:.3g} of the largest entry")
        assert err <= 1e-4, (l, err)
    for e in range(5):
        if e:
            tl, want_tl = g.train_epoch()[0], ref.forward(1)[0]
            ref.backward()
        ref.step()
        vl, want_vl = g.eval(2)[0], ref.forward(2)[0]
        print(f"epoch {e + 1}: train {tl:.9g} / {want_tl:.9g}  val {vl:.9g} / {want_vl:.9g}")
        assert abs(tl - want_tl) <= 1e-4 * abs(want_tl), (e, tl, want_tl)
        assert abs(vl - want_vl) <= 1e-4 * abs(want_vl), (e, vl, want_vl)
    g.close()


def _lines(g, n):
    return np.array([g.train_epoch() + g.eval(2) for _ in range(n)], np.float32)


def test_training_lowers_validation_loss(pgcn, data):
    ds, _ = data["syn41"]
    g = pgcn.GCN(_params(pgcn, ds, drop=0.5), ds)
    lines = _lines(g, 30)
    g.close()
    print("val loss", lines[0, 2], "->", lines[-1, 2])
    assert np.isfinite(lines).all() and lines[-1, 2] < lines[0, 2]
    assert ((lines[:, 1] >= 0) & (lines[:, 1] <= 1)).all()


def test_epoch_graph_bit_identical(pgcn, data):
    ds, _ = data["syn41"]
    runs = []
    for on in (0, 1):
        with helpers.knobs(pgcn, epoch_graph=on):
            g = pgcn.GCN(_params(pgcn, ds, drop=0.5), ds)
            for _ in range(3):
                g.epoch_async()
            runs.append((g.results(3), [g.get_var(_w(l)) for l in range(2)]))
            g.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert np.isfinite(runs[0][0]).all()
    for a, b in zip(*(r[1] for r in runs)):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["syn41", "cora"])
def test_loopback_matches_one_gpu(pgcn, data, cora_ml, name, world):
    """Edge-cut ranks: losses within 1e-4 relative of the one-GPU engine's, accuracies equal;
    every rank reports the same lines; the ranks' counts add up to the one-GPU engine's."""
    ds, Y = _get(name, data, cora_ml)
    p = _params(pgcn, ds, drop=0.5)
    one = pgcn.GCN(p, ds)
    want = _lines(one, 3)
    want_counts = one.multilabel_counts(2)
    want_pred = one.predict_multilabel()
    one.close()
    group = pgcn.LoopbackGroup(world)

    def rank_fn(r):
        g = pgcn.GCN(p, ds, device=0, rank=r, loopback=group)
        assert g.query("multilabel") == 1 and g.query("world") == world
        out = (_lines(g, 3), g.multilabel_counts(2), g.predict_multilabel(), g.node_range())
        g.close()
        return out
    res = pgcn.run_ranks(world, rank_fn)
    for r in res:
        np.testing.assert_array_equal(r[0], res[0][0])
    got = res[0][0]
    print(name, world, got, want)
    for k in (0, 2):
        assert (np.abs(got[:, k] - want[:, k]) <= 1e-4 * np.abs(want[:, k])).all(), (k, got, want)
    for k in (1, 3):
        np.testing.assert_array_equal(got[:, k], want[:, k])
    np.testing.assert_array_equal(sum(r[1] for r in res), want_counts)
    pred = np.concatenate([r[2] for r in res])
    assert pred.shape == want_pred.shape and res[-1][3][1] == ds.num_nodes
    assert (pred != want_pred).sum() <= 2  # (a logit within rounding of zero may flip)


@pytest.mark.parametrize("opts", [dict(residual=True), dict(layer_norm=True),
                                  dict(residual=True, layer_norm=True)],
                         ids=["residual", "layer_norm", "both"])
def test_model_options(pgcn, data, opts):
    """(8, 8, 8) engines with residual layers and / or LayerNorm: the first forward loss matches
    float64 at dropout 0, and they train (finite lines, the weights move)."""
    ds, Y = data["syn41"]
    hidden = (8, 8, 8)
    g, ref = _tie_free(pgcn, ds, Y, hidden, **opts)
    assert g.query("residual_layers") == (2 if opts.get("residual") else 0)
    assert g.query("norm_layers") == (3 if opts.get("layer_norm") else 0)
    w0 = g.get_var(_w(3)).copy()
    tl, ta = g.train_epoch()
    want_tl, want_ta = ref.forward(1)
    print(opts, tl, want_tl, ta, want_ta)
    assert abs(tl - want_tl) <= 1e-4 * abs(want_tl)
    lines = _lines(g, 3)
    assert np.isfinite(lines).all() and (g.get_var(_w(3)) != w0).any()
    g.close()


def test_predict_counts_and_f1(pgcn, data, cora_ml):
    """predict_multilabel equals thresholding the logits variable after an eval; its probs are
    the sigmoid of them; multilabel_counts equals numpy's tp / fp / fn; f1_scores within 1e-12;
    training after a predict is bit-identical to training without it."""
    for ds, Y in (data["syn41"], cora_ml):
        n, c = ds.num_nodes, ds.output_dim
        p = _params(pgcn, ds, drop=0.5)
        g1, g2 = pgcn.GCN(p, ds), pgcn.GCN(p, ds)
        for _ in range(3):
            np.testing.assert_array_equal(_lines(g1, 1), _lines(g2, 1))
            pred, probs = g1.predict_multilabel(probs=True)
            x = g1.get_var(_var2(1)).reshape(n, c)
            np.testing.assert_array_equal(pred, x > 0)
            assert pred.dtype == bool and pred.shape == (n, c)
            np.testing.assert_allclose(probs, 1.0 / (1.0 + np.exp(-x.astype(np.float64))),
                                       atol=2.0 ** -22, rtol=0)
            g1.eval(2)
            x = g1.get_var(_var2(1)).reshape(n, c)  # (the same logits: eval-mode forwards)
            np.testing.assert_array_equal(pred, x > 0)
            g2.eval(2)
            for split in (1, 2, 3):
                counts = g1.multilabel_counts(split)
                rows = (np.asarray(ds.split) == split) & (np.asarray(ds.label) >= 0)
                P, T = pred[rows], Y[rows]
                want = np.stack([(P & T).sum(0), (P & ~T).sum(0), (~P & T).sum(0)])
                np.testing.assert_array_equal(counts, want)
                assert counts.dtype == np.int64
                tp, fp, fn = want.astype(np.float64)
                den = 2 * tp + fp + fn
                micro = 2 * tp.sum() / den.sum() if den.sum() else 0.0
                macro = np.where(den > 0, 2 * tp / np.maximum(den, 1), 0.0).mean()
                got = pgcn.f1_scores(counts)
                assert abs(got[0] - micro) <= 1e-12 and abs(got[1] - macro) <= 1e-12
        for l in range(2):
            np.testing.assert_array_equal(g1.get_var(_w(l)), g2.get_var(_w(l)))
        with pytest.raises(pgcn.PgcnError) as e:
            g1.confusion(2)
        assert e.value.status == pgcn.PGCN_E_INVALID
        with pytest.raises(pgcn.PgcnError) as e:
            g1.predict()
        assert e.value.status == pgcn.PGCN_E_INVALID
        g1.close()
        g2.close()


def test_checkpoints(pgcn, data, tmp_path):
    """save -> 3 epochs -> load -> 3 epochs reproduces lines and weights bit for bit; the file
    carries CKPT_MULTILABEL; a flags-0 load of a single-label file of the same dims is refused
    with the engine untouched (and the other way round); weights-only loads cross."""
    ds, Y = data["syn41"]
    single = pgcn.Dataset.synthetic(300, 24, 41, 900, 17 + 41)  # the same graph, one class each
    hidden = (8, 8)
    ps = pgcn.make_params(single, hidden_dims=hidden, dropouts=(0.5,) * 3)
    pm = _params(pgcn, ds, hidden, drop=0.5)
    multi, plain = str(tmp_path / "multi.pgcnck"), str(tmp_path / "plain.pgcnck")
    g = pgcn.GCN(pm, ds)
    _lines(g, 2)
    g.save(multi)
    assert pgcn.checkpoint_flags(multi) == pgcn.CKPT_MULTILABEL
    assert pgcn.checkpoint_info(multi)["version"] == 1
    a = _lines(g, 3)
    wa = [g.get_var(_w(l)) for l in range(3)]
    g.load(multi)
    np.testing.assert_array_equal(a, _lines(g, 3))
    for l in range(3):
        np.testing.assert_array_equal(wa[l], g.get_var(_w(l)))
    fresh = pgcn.GCN(pm, ds)
    fresh.load(multi)
    np.testing.assert_array_equal(a, _lines(fresh, 3))
    fresh.close()
    s = pgcn.GCN(ps, single)
    _lines(s, 2)
    s.save(plain)
    assert pgcn.checkpoint_flags(plain) == 0
    # refusals in both directions, the engines untouched
    for eng, other_file, twin_p, twin_ds in ((g, plain, pm, ds), (s, multi, ps, single)):
        twin = pgcn.GCN(twin_p, twin_ds)
        twin.load(multi if eng is g else plain)
        if eng is g:
            _lines(twin, 3)  # g stands three epochs behind its reload of `multi`
        with pytest.raises(pgcn.PgcnError) as e:
            eng.load(other_file)
        assert e.value.status == pgcn.PGCN_E_INVALID
        np.testing.assert_array_equal(_lines(eng, 2), _lines(twin, 2))
        twin.close()
    # weights-only loads cross the bit
    g.load(plain, weights_only=True)
    assert g.query("adam_steps") == 0
    s2 = pgcn.GCN(ps, single)
    s2.load(plain)
    for l in range(3):
        np.testing.assert_array_equal(g.get_var(_w(l)), s2.get_var(_w(l)))
    assert np.isfinite(_lines(g, 1)).all()
    s.load(multi, weights_only=True)
    assert np.isfinite(_lines(s, 1)).all()
    # a LayerNorm multi-label engine: version 3 (version 2's layout with both bits), resumable
    gl = pgcn.GCN(_params(pgcn, ds, hidden, drop=0.5, layer_norm=True), ds)
    _lines(gl, 1)
    both = str(tmp_path / "both.pgcnck")
    gl.save(both)
    assert pgcn.checkpoint_flags(both) == pgcn.CKPT_MULTILABEL | pgcn.CKPT_LAYERNORM
    assert pgcn.checkpoint_info(both)["version"] == 3
    b = _lines(gl, 2)
    gl.load(both)
    np.testing.assert_array_equal(b, _lines(gl, 2))
    for x in (g, s, s2, gl):
        x.close()


def test_refusals(pgcn, data):
    """Engine build refuses multilabel without bits, with a word count that does not match
    output_dim, and with more than 128 classes; single-label engines refuse the multi-label
    services."""
    ds, Y = data["syn5"]
    INV = pgcn.PGCN_E_INVALID
    plain = pgcn.Dataset.synthetic(300, 24, 5, 900, 22)
    with pytest.raises(pgcn.PgcnError) as e:
        pgcn.GCN(_params(pgcn, plain), plain)  # no label_bits
    assert e.value.status == INV
    # a view with the wrong word count / output_dim that does not match the bits
    h = ctypes.c_void_p()
    p = _params(pgcn, ds)
    view = pgcn.PgcnData.from_buffer_copy(ds.view)
    view.label_words = 2
    assert pgcn.lib.pgcn_gcn_create(ctypes.byref(p), ctypes.byref(view), 0,
                                    ctypes.byref(h)) == INV
    p.output_dim = 41  # needs 2 words, the data has 1
    assert pgcn.lib.pgcn_gcn_create(ctypes.byref(p), ctypes.byref(ds.view), 0,
                                    ctypes.byref(h)) == INV
    p.output_dim = 129
    view.label_words = 5
    assert pgcn.lib.pgcn_gcn_create(ctypes.byref(p), ctypes.byref(view), 0,
                                    ctypes.byref(h)) == INV
    assert not h.value
    # single-label engines refuse the multi-label services
    s = pgcn.GCN(pgcn.make_params(plain, dropouts=(0.0, 0.0)), plain)
    assert s.query("multilabel") == 0
    with pytest.raises(pgcn.PgcnError) as e:
        s.predict_multilabel()
    assert e.value.status == INV
    with pytest.raises(pgcn.PgcnError) as e:
        s.multilabel_counts(2)
    assert e.value.status == INV
    s.close()


def test_refuses_more_than_2_pow_24_elements(pgcn):
    """labelled rows of a split * C > 2^24 is refused at build, before anything is uploaded:
    about 145,000 training rows x 128 classes = 18.5 M (an edgeless graph with two features per
    node: the refusal is by argument, nothing of this size is built)."""
    n, c = 220000, 128
    ds = pgcn.Dataset.synthetic(n, 2, 2, 0, 3)
    ds.set_multilabel(np.zeros((n, c), bool))
    cnt = helpers.split_counts(ds)
    assert max(cnt.values()) * c > 2 ** 24 >= min(cnt.values()) * c, cnt
    with pytest.raises(pgcn.PgcnError) as e:
        pgcn.GCN(_params(pgcn, ds), ds)
    assert e.value.status == pgcn.PGCN_E_INVALID
