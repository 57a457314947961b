"""The engine with GraphSAGE layers (pgcn_params.aggregator / root_weight) against the float64
numpy model of tests/sage_ref.py (NumpySageGCN), started from the engine's initial weights, and
the engine's services on such an engine: checkpoints, predict, epoch graphs, refusals, queries.

Tolerances are tests/test_gpu_gat.py's: rtol 1e-4 throughout, with atol 1e-6 on the logits and
1e-7 on gradients.  Hidden tensors take atol 1e-6 of the tensor's largest entry (see
check_epoch).  Losses are within 1e-4 relative, the project's parity bar.  Accuracies are within
the reference's near-tied rows.

Seeds.  A ReLU argument or a max margin that the float64 run has within 2e-6 of its tensor's
largest value (three times an fp32 sum's error at these widths) could fall on the other side in
fp32 and move whole gradient rows; the tests take the first seed in 0..15 whose float64 run has
none -- a condition on the reference alone, computed on the host from the seed (the engine's
initial weights must then equal the host's Glorot draws bit for bit).  Beyond that, elements of
a max layer whose top two candidates lie within 1e-5 max|Q| of each other without being an exact
tie are left out of that layer's element-wise comparison; their share stays below 1 %
(tests/test_cpu_sage.py checks the same seeds on the CPU).
"""
import numpy as np
import pytest

import gat_ref
import helpers
import sage_ref
from test_gpu_gat import PatternDataset

pytestmark = pytest.mark.gpu

AGG = {"mean": 1, "max": 2}
FLIP, NEAR, CAP = 2e-6, 1e-5, 0.01


def _var1(l):
    return 1 + 3 * l


def _w(l):
    return 2 + 3 * l


def _var2(l):
    return 3 + 3 * l


def _params(pgcn, ds, agg, root, hidden=(16,), dropouts=None, **kw):
    L = len(hidden) + 1
    return pgcn.make_params(ds, hidden_dims=hidden, dropouts=dropouts or (0.5,) * L,
                            aggregator=agg, root_weight=root, **kw)


def _lines(g, n):
    return np.array([g.train_epoch() + g.eval(2) for _ in range(n)], np.float32)


def reference_epoch(pgcn, ds, hidden, dropouts, seed, agg, root, label_bits=None, **kw):
    """One train_epoch + eval(2) of the reference from the host's Glorot draws of `seed`: the
    tensors the engine is compared with, and how close a ReLU argument or a max margin came to
    flipping.  No device."""
    dims = [ds.input_dim] + list(hidden) + [ds.output_dim]
    w0, draws = sage_ref.glorot_weights(pgcn, seed, dims, root)
    rng = gat_ref.Xorshift(pgcn.rng_jump(pgcn.rng_seed(seed), draws))
    ref = sage_ref.NumpySageGCN(ds, hidden, w0, dropouts, rng, aggregator=agg, root_weight=root,
                                residual=kw.get("residual", False),
                                layer_norm=kw.get("layer_norm", False), label_bits=label_bits,
                                indptr=ds.graph_indptr, indices=ds.graph_indices)
    L, c = ref.L, ds.output_dim

    def closest():
        def rel(a):
            nz = np.abs(a[a != 0])
            return float(nz.min() / np.abs(a).max()) if nz.size else 1.0
        out = [rel(y) for y in ref.Y]
        out += [float(gp[gp > 0].min() / q) for gp, q in zip(ref.gap, ref.qmax) if gp is not None]
        if ref.bits is not None:
            out.append(rel(ref.logits[ref.rows]))
        return min(out)
    tl = ref.forward(1, training=True)
    ta, close = ref.acc, closest()
    near = ref.near_tied(NEAR)
    ref.backward()
    ep = dict(w0=w0, logits=ref.train_logits(), var2=[ref.A[l + 1].copy() for l in range(L - 1)],
              dW=[w.copy() for w in ref.dW], dnorm=ref.norm_grad() if ref.ln else None, near=near,
              share=[0.0 if m is None else float(m.mean()) for m in near])
    t1 = helpers.near_ties(ref.logits, ds.label, ds.split, 1, c) if ref.bits is None else 0
    ref.step()
    vl = ref.forward(2)
    t2 = helpers.near_ties(ref.logits, ds.label, ds.split, 2, c) if ref.bits is None else 0
    ep.update(line=(tl, ta, vl, ref.acc), ties={1: t1, 2: t2}, close=min(close, closest()))
    return ep


def flip_free(pgcn, ds, hidden, dropouts, agg, root, **kw):
    for seed in range(16):
        ep = reference_epoch(pgcn, ds, hidden, dropouts, seed, agg, root, **kw)
        print(f"seed {seed}: closest argument {ep['close']:.3g}, near-tied share {ep['share']}")
        if ep["close"] >= FLIP and max(ep["share"]) < CAP:
            return seed, ep
    raise AssertionError("no seed in 0..15 keeps every ReLU argument and max margin off a flip")


def check_epoch(pgcn, ds, hidden, dropouts, agg, root, cnt=None, label_bits=None, **kw):
    seed, ep = flip_free(pgcn, ds, hidden, dropouts, agg, root, label_bits=label_bits, **kw)
    L, n = len(hidden) + 1, ds.num_nodes
    g = pgcn.GCN(_params(pgcn, ds, agg, root, hidden, dropouts, seed=seed,
                         multilabel=label_bits is not None, **kw), ds)
    assert g.query("aggregator") == AGG[agg] and g.query("root_weight") == int(root)
    for l in range(L):  # Glorot with fan-out 2 d_l, one draw per element, in layer order
        np.testing.assert_array_equal(g.get_var(_w(l)), ep["w0"][l], err_msg=f"W{l}")
    tr = g.train_epoch()

    def masked(got, want, l):
        m = ep["near"][l]
        if m is None:
            return got, want
        assert m.mean() < CAP
        return np.where(m, 0.0, got), np.where(m, 0.0, want)
    got, want = masked(g.get_var(_var2(L - 1)).reshape(n, -1), ep["logits"], L - 1)
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6, err_msg="logits")
    for l in range(L - 1):
        # (var2 l after its tail: the next layer's input before its Dropout ... as the engine keeps
        # it after the Dropout ran in place.  Its atol is tests/test_gpu_gat_kernels.py's form, 1e-6
        # of the tensor's largest entry: behind a LayerNorm and a residual add an entry's rounding
        # error follows its row's scale, not its own size -- an entry of 4.6e-4 beside entries of
        # 7.4 was off by 1.5e-6 = 2e-7 of the scale, which an absolute 1e-6 does not allow for)
        got, want = masked(g.get_var(_var2(l)).reshape(n, -1), ep["var2"][l], l)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6 * max(1.0, np.abs(want).max()),
                                   err_msg=f"var2 {l}")
    for l in range(L):
        np.testing.assert_allclose(g.get_var(_w(l), 1).reshape(ep["dW"][l].shape), ep["dW"][l],
                                   rtol=1e-4, atol=1e-7, err_msg=f"W{l} grad")
    if ep["dnorm"] is not None:
        np.testing.assert_allclose(g.get_var(3 * L + 1, 1), ep["dnorm"], rtol=1e-4, atol=1e-7,
                                   err_msg="gamma / beta grad")
    ev = g.eval(2)
    print(f"engine {tr + ev} reference {ep['line']}")
    helpers.assert_line_close(tr + ev, ep["line"], cnt or helpers.split_counts(ds), what=agg,
                              ties=ep["ties"])
    return g


@pytest.mark.parametrize("root", [False, True])
@pytest.mark.parametrize("agg", ["mean", "max"])
def test_numeric_parity_cora(loaded, pgcn, agg, root):
    """2 layers, hidden 16, the default dropouts: the initial weights, then after one training
    epoch the logits, var2, every weight gradient and the loss / accuracy line with eval(2)."""
    ds = loaded["cora"]
    g = check_epoch(pgcn, ds, (16,), (0.5, 0.5), agg, root)
    assert g.num_vars() == 7
    n = ds.num_nodes
    assert g.get_var(_var1(0)).size == n * (32 if root else 16)
    assert g.get_var(_var1(1)).size == n * ds.output_dim * (2 if root else 1)
    for key in ("reassociated", "eval_ax_us", "attention_layers"):
        assert g.query(key) == 0, key
    if agg == "max":
        assert g.query("graphsum_lds") == 0
    g.close()


@pytest.mark.parametrize("agg", ["mean", "max"])
def test_numeric_parity_residual_layernorm(loaded, pgcn, agg):
    """3 layers 16 / 16 with the root weight, residual and LayerNorm on (the shape of
    tests/test_gpu_gat.py's case): the residual layer's aggregation backward reads the ReLU-masked
    gradient the LayerNorm backward transformed.  (At width 8 the float64 run of this model has
    rows of zero and near-zero variance in its second LayerNorm -- rstd up to 1 / sqrt(eps) = 316
    against a median of 1.2 -- which multiply any fp32 rounding by that factor: no element-wise
    bound at 1e-4 holds there for any aggregation, so the narrow case below runs without it.)"""
    ds = loaded["cora"]
    g = check_epoch(pgcn, ds, (16, 16), (0.5, 0.5, 0.5), agg, True, residual=True,
                    layer_norm=True)
    assert g.query("residual_layers") == 1 and g.query("norm_layers") == 2
    g.close()


@pytest.mark.parametrize("agg", ["mean", "max"])
def test_numeric_parity_three_narrow_layers(loaded, pgcn, agg):
    """3 layers 8 / 8 with the root weight and the residual connection: GL 2 in the max kernels,
    var1 [n][16]."""
    ds = loaded["cora"]
    g = check_epoch(pgcn, ds, (8, 8), (0.5, 0.5, 0.5), agg, True, residual=True)
    assert g.query("residual_layers") == 1 and g.num_vars() == 10
    g.close()


@pytest.fixture(scope="module")
def small(pgcn):
    """A synthetic n = 300, F = 24 graph with a seeded 5-class label matrix."""
    ds = pgcn.Dataset.synthetic(300, 24, 5, 900, 22)
    Y = np.random.default_rng(105).random((300, 5)) < 0.3
    return ds, Y


@pytest.mark.parametrize("agg", ["mean", "max"])
def test_multilabel(small, pgcn, agg):
    _, Y = small
    ds = pgcn.Dataset.synthetic(300, 24, 5, 900, 22)
    ds.set_multilabel(Y)
    cnt = {s: k * 5 for s, k in helpers.split_counts(ds).items()}
    g = check_epoch(pgcn, ds, (16,), (0.5, 0.5), agg, True, cnt=cnt, label_bits=Y)
    assert g.query("multilabel") == 1
    g.close()


def directed_cora(pgcn, base):
    """cora with some reverse edges removed: of every pair i < j, the slot (j, i) goes when
    (i + j) % 3 == 1; the self loops and every forward slot stay.  (The rule is one for which the
    float64 model has a flip-free seed in 0..15 for both aggregators: a property of the reference.)"""
    rows = np.repeat(np.arange(base.num_nodes), np.diff(base.graph_indptr))
    cols = np.asarray(base.graph_indices)
    keep = ~((cols < rows) & ((rows + cols) % 3 == 1))
    indptr = np.zeros(base.num_nodes + 1, np.int64)
    np.add.at(indptr, rows[keep] + 1, 1)
    assert 0.05 * len(keep) < (~keep).sum() < 0.3 * len(keep)
    return PatternDataset(pgcn, base, np.cumsum(indptr), cols[keep])


@pytest.mark.parametrize("agg", ["mean", "max"])
def test_directed_pattern(loaded, pgcn, agg):
    """cora with some reverse edges removed: the backward walks the transposed pattern, it does
    not rely on A = A^T (logits and gradients against the float64 model, as above)."""
    ds = directed_cora(pgcn, loaded["cora"])
    g = check_epoch(pgcn, ds, (16,), (0.5, 0.5), agg, True)
    assert g.query("graph_symmetric") == 0
    g.close()


@pytest.mark.parametrize("agg,root", [("mean", False), ("max", True)])
def test_checkpoints(loaded, pgcn, tmp_path, agg, root):
    """Save at epoch 3 and resume on a fresh engine to epoch 6: bit-identical to 6 straight
    epochs; the file is version 6 with flags bit 4 and the block; a flags-0 load across another
    aggregator or root weight (a plain engine included) is PGCN_E_INVALID with the engine
    untouched; a weights-only load crosses the aggregator exactly when the shapes agree."""
    ds, hidden, L = loaded["cora"], (16,), 2

    def make(a, r, **kw):
        return pgcn.GCN(_params(pgcn, ds, a, r, hidden, **kw), ds)
    straight = make(agg, root)
    want = _lines(straight, 6)
    a = make(agg, root)
    np.testing.assert_array_equal(_lines(a, 3), want[:3])
    path = str(tmp_path / "sage.pgcnck")
    a.save(path)
    info = pgcn.checkpoint_info(path)
    n_w = (ds.input_dim * 16 + 16 * ds.output_dim) * (2 if root else 1)
    assert info["version"] == 6 and info["weights"] == n_w
    assert pgcn.checkpoint_flags(path) == 16
    assert pgcn.checkpoint_sage(path) == (AGG[agg], int(root))
    b = make(agg, root)
    b.load(path)
    np.testing.assert_array_equal(_lines(b, 3), want[3:])
    np.testing.assert_array_equal(b.results(6), want)
    for l in range(L):
        np.testing.assert_array_equal(b.get_var(_w(l)), straight.get_var(_w(l)))
    other_agg = "max" if agg == "mean" else "mean"
    for oa, orr in ((other_agg, root), (agg, not root), (None, False)):
        o = make(oa, orr)
        twin = make(oa, orr)
        with pytest.raises(pgcn.PgcnError) as e:
            o.load(path)
        assert e.value.status == pgcn.PGCN_E_INVALID
        if orr == root:  # the same shapes: weights only crosses the aggregator
            o.load(path, weights_only=True)
            assert o.query("adam_steps") == 0
            for l in range(L):
                np.testing.assert_array_equal(o.get_var(_w(l)), a.get_var(_w(l)))
            assert np.isfinite(_lines(o, 1)).all()
        else:
            with pytest.raises(pgcn.PgcnError) as e:
                o.load(path, weights_only=True)
            assert e.value.status == pgcn.PGCN_E_INVALID
            np.testing.assert_array_equal(_lines(o, 1), _lines(twin, 1))
        o.close()
        twin.close()
    # a plain engine's version-1 file: (0, 0), refused by a flags-0 load into the SAGE engine
    p = make(None, False)
    _lines(p, 1)
    ppath = str(tmp_path / "plain.pgcnck")
    p.save(ppath)
    assert pgcn.checkpoint_info(ppath)["version"] == 1 and pgcn.checkpoint_sage(ppath) == (0, 0)
    with pytest.raises(pgcn.PgcnError) as e:
        a.load(ppath)
    assert e.value.status == pgcn.PGCN_E_INVALID
    # with LayerNorm: flags 2 | 16, the norm tensor behind the layer weights
    nrm = make(agg, root, layer_norm=True)
    _lines(nrm, 1)
    npath = str(tmp_path / "sage_norm.pgcnck")
    nrm.save(npath)
    assert pgcn.checkpoint_flags(npath) == 18 and pgcn.checkpoint_info(npath)["version"] == 6
    assert pgcn.checkpoint_info(npath)["weights"] == n_w + 2 * 16
    for x in (straight, a, b, p, nrm):
        x.close()


@pytest.mark.parametrize("agg,root", [("mean", True), ("max", True), ("max", False)])
def test_predict_and_epoch_graph(loaded, pgcn, agg, root):
    """predict between two epochs leaves training bit-identical; epoch_graph on equals off bit
    for bit."""
    ds, hidden, L = loaded["cora"], (16,), 2
    g1, g2 = (pgcn.GCN(_params(pgcn, ds, agg, root, hidden), ds) for _ in range(2))
    for _ in range(2):
        np.testing.assert_array_equal(_lines(g1, 1), _lines(g2, 1))
        cls, conf = g1.predict()
        assert cls.shape == (ds.num_nodes,) and np.isfinite(conf).all()
        assert g1.confusion(2).sum() == helpers.split_counts(ds)[2]
    for l in range(L):
        np.testing.assert_array_equal(g1.get_var(_w(l)), g2.get_var(_w(l)))
    w = g1.get_var(_w(1))
    assert w.size == 16 * ds.output_dim * (2 if root else 1)
    g1.set_var(_w(1), w * np.float32(0.5))
    with pytest.raises(pgcn.PgcnError):
        g1.set_var(_w(1), w[:-1])
    g1.close()
    g2.close()
    runs = []
    for on in (0, 1):
        with helpers.knobs(pgcn, epoch_graph=on, sparse_dual=0):
            g = pgcn.GCN(_params(pgcn, ds, agg, root, hidden), ds)
            for _ in range(3):
                g.epoch_async()
            runs.append((g.results(3), [g.get_var(_w(l)) for l in range(L)]))
            g.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert np.isfinite(runs[0][0]).all()
    for x, y in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(x, y)


def test_refusals(loaded, pgcn):
    """PGCN_E_INVALID at engine build: an aggregator outside 0..2, a root weight without an
    aggregator, an aggregator with attention, a hidden width or an output_dim above 128, and the
    edge-cut creators."""
    ds = loaded["cora"]
    many = pgcn.Dataset.synthetic(300, 24, 130, 900, 22)  # output_dim 130
    p = _params(pgcn, ds, "max", True)
    group = pgcn.LoopbackGroup(1)

    def raw(**kw):
        q = pgcn.make_params(ds)
        for k, v in kw.items():
            setattr(q, k, v)
        return lambda: pgcn.GCN(q, ds)
    makers = {
        "aggregator 3": raw(aggregator=3),
        "aggregator -1": raw(aggregator=-1),
        "root alone": raw(root_weight=1),
        "root 2": raw(aggregator=1, root_weight=2),
        "attention": raw(aggregator=2, attention=1),
        "wide": lambda: pgcn.GCN(_params(pgcn, ds, "mean", False, (132,)), ds),
        "classes": lambda: pgcn.GCN(_params(pgcn, many, "max", True), many),
        "dist": lambda: pgcn.GCN(p, ds, rank=0, world=1, unique_id=b"\0" * 128),
        "peer": lambda: pgcn.GCN(p, ds, rank=0, world=1, allgather=lambda data: [data]),
        "loopback": lambda: pgcn.GCN(p, ds, rank=0, loopback=group),
        "solo": lambda: pgcn.GCN(p, ds, rank=0, world=2, solo=True),
    }
    for name, make in makers.items():
        with pytest.raises(pgcn.PgcnError) as e:
            make()
        assert e.value.status == pgcn.PGCN_E_INVALID, name
    g = pgcn.GCN(_params(pgcn, ds, "max", True, (128,)), ds)
    assert np.isfinite(_lines(g, 1)).all()
    g.close()


def test_off_is_off(loaded, pgcn):
    """aggregator 0, root_weight 0 written out is the default engine bit for bit -- the epoch
    results, the weights and the launches per epoch -- also after a SAGE engine ran in the same
    process."""
    ds = loaded["cora"]
    s = pgcn.GCN(_params(pgcn, ds, "max", True), ds)
    _lines(s, 1)
    s.close()
    out = []
    for explicit in (False, True):
        p = pgcn.make_params(ds)
        if explicit:
            p.aggregator, p.root_weight = 0, 0
        g = pgcn.GCN(p, ds)
        assert g.query("aggregator") == 0 and g.query("root_weight") == 0 and g.num_vars() == 7
        _lines(g, 1)
        g.sync()
        pgcn.reset_path_counts()
        lines = _lines(g, 4)
        out.append((lines, pgcn.path_counts()["launches"], [g.get_var(_w(l)) for l in range(2)]))
        g.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]
    for x, y in zip(out[0][2], out[1][2]):
        np.testing.assert_array_equal(x, y)
