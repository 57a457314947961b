"""The engine with graph attention layers (pgcn_params.attention) against the float64 numpy
model of tests/gat_ref.py (NumpyGatGCN: scipy CSR algebra, hpdga's Adam and dropout draws,
weight decay on W0 only), started from the engine's initial tensors read with get_var; and the
engine's services on such an engine: checkpoints, set_var, predict, epoch graphs, refusals.

Tolerances are tests/test_gpu_layernorm.py's: rtol 1e-4, atol 1e-6 on values, 1e-7 on gradients;
losses within 1e-4 relative; accuracies within the reference's near-tied rows.
"""
import ctypes

import numpy as np
import pytest

import gat_ref
import helpers

pytestmark = pytest.mark.gpu


def _var1(l):
    return 1 + 3 * l


def _w(l):
    return 2 + 3 * l


def _var2(l):
    return 3 + 3 * l


def _params(pgcn, ds, hidden=(16,), dropouts=None, **kw):
    L = len(hidden) + 1
    return pgcn.make_params(ds, hidden_dims=hidden, dropouts=dropouts or (0.5,) * L,
                            attention=True, **kw)


def _lines(g, n):
    return np.array([g.train_epoch() + g.eval(2) for _ in range(n)], np.float32)


def _pair(pgcn, ds, hidden, dropouts, seed, label_bits=None, **kw):
    """An attention engine and the reference started from its initial tensors; the reference's
    dropout stream stands behind the engine's initial draws (weights, then the attention
    vectors)."""
    L = len(hidden) + 1
    g = pgcn.GCN(_params(pgcn, ds, hidden, dropouts, seed=seed,
                         multilabel=label_bits is not None, **kw), ds)
    w0 = [g.get_var(_w(l)) for l in range(L)]
    attn0 = g.get_var(g.num_vars() - 1)
    draws = sum(w.size for w in w0) + attn0.size
    rng = gat_ref.Xorshift(pgcn.rng_jump(pgcn.rng_seed(seed), draws))
    ref = gat_ref.NumpyGatGCN(ds, hidden, w0, attn0, dropouts, rng,
                              residual=kw.get("residual", False),
                              layer_norm=kw.get("layer_norm", False), label_bits=label_bits,
                              indptr=ds.graph_indptr, indices=ds.graph_indices)
    return g, ref


def _closest(ref):
    """min |value| relative to its tensor's largest over every hidden pre-activation (a ReLU mask)
    and every slot score (the LeakyReLU's branch) of the last forward; exact zeros do not count
    (all-zero rows are zero in fp32 as well).  tests/test_gpu_multilabel.py's measure."""
    def rel(a):
        nz = np.abs(a[a != 0])
        return float(nz.min() / np.abs(a).max()) if nz.size else 1.0
    out = [rel(y) for y in ref.Y] + [rel(f["x"]) for f in ref.att]
    if ref.bits is not None:  # ... and every labelled logit (a thresholded class)
        out.append(rel(ref.logits[ref.rows]))
    return min(out)


def _reference_epochs(ref, epochs, ds):
    """The reference's train_epoch + eval(2) `epochs` times: per epoch the training tensors the
    engine is compared with, the line, the near-tied rows, and how close any ReLU / LeakyReLU
    argument came to zero."""
    out = []
    L, c = ref.L, ds.output_dim
    for _ in range(epochs):
        tl = ref.forward(1, training=True)
        ta = ref.acc
        close = _closest(ref)
        ref.backward()
        ep = dict(logits=ref.train_logits(), var2=[ref.A[l + 1].copy() for l in range(L - 1)],
                  dW=[w.copy() for w in ref.dW], dattn=ref.attn_grad(),
                  dnorm=ref.norm_grad() if ref.ln else None,
                  dvar1=[x.copy() for x in ref.dvar1])
        t1 = helpers.near_ties(ref.logits, ds.label, ds.split, 1, c) if ref.bits is None else 0
        ref.step()
        vl = ref.forward(2)
        t2 = helpers.near_ties(ref.logits, ds.label, ds.split, 2, c) if ref.bits is None else 0
        ep.update(line=(tl, ta, vl, ref.acc), ties={1: t1, 2: t2}, close=min(close, _closest(ref)))
        out.append(ep)
    return out


def _tie_free(pgcn, ds, hidden, dropouts, epochs, **kw):
    """The first seed in 0..7 for which no ReLU, LeakyReLU or class-threshold argument of the
    float64 run comes within 2e-6 of its tensor's largest value of zero in any of the epochs
    (three times an fp32 sum's error at these widths) -- a condition on the reference alone."""
    for seed in range(8):
        g, ref = _pair(pgcn, ds, hidden, dropouts, seed, **kw)
        want = _reference_epochs(ref, epochs, ds)
        close = min(e["close"] for e in want)
        print(f"seed {seed}: closest argument {close:.3g}")
        if close >= 2e-6:
            return g, ref, want, seed
        g.close()
    raise AssertionError("no seed in 0..7 keeps every ReLU / LeakyReLU argument off zero")


def _check_epochs(g, ref, want, ds, cnt):
    """The tensors after the first train_epoch, the lines of every epoch -- the structure of
    tests/test_gpu_layernorm.py's parity test.  From the second epoch on the weights have gone
    through Adam, whose first steps are lr * g / (|g| + eps / sqrt(1 - beta2)): a gradient
    element near 3e-7 turns an fp32 rounding error of 1e-8 into 1e-4 of a weight, so tensors
    behind a step have no element-wise bound at 1e-6; the losses do (1e-4 relative)."""
    L = ref.L
    n = ds.num_nodes
    attn_idx = g.num_vars() - 1
    for e, ep in enumerate(want):
        tr = g.train_epoch()
        if e > 0:
            ev = g.eval(2)
            print(f"epoch {e + 1}: engine {tr + ev} reference {ep['line']}")
            helpers.assert_line_close(tr + ev, ep["line"], cnt, what=f"epoch {e + 1}",
                                      ties=ep["ties"])
            continue
        np.testing.assert_allclose(g.get_var(_var2(L - 1)).reshape(n, -1), ep["logits"],
                                   rtol=1e-4, atol=1e-6, err_msg=f"epoch {e + 1} logits")
        for l in range(L - 1):
            np.testing.assert_allclose(g.get_var(_var2(l)).reshape(n, -1), ep["var2"][l],
                                       rtol=1e-4, atol=1e-6, err_msg=f"epoch {e + 1} var2 {l}")
        for l in range(L):
            np.testing.assert_allclose(g.get_var(_w(l), 1).reshape(ep["dW"][l].shape),
                                       ep["dW"][l], rtol=1e-4, atol=1e-7,
                                       err_msg=f"epoch {e + 1} W{l} grad")
            np.testing.assert_allclose(g.get_var(_var1(l), 1).reshape(n, -1), ep["dvar1"][l],
                                       rtol=1e-4, atol=1e-7, err_msg=f"epoch {e + 1} var1.grad {l}")
        np.testing.assert_allclose(g.get_var(attn_idx, 1), ep["dattn"], rtol=1e-4, atol=1e-7,
                                   err_msg=f"epoch {e + 1} attn grad")
        if ep["dnorm"] is not None:
            np.testing.assert_allclose(g.get_var(3 * L + 1, 1), ep["dnorm"], rtol=1e-4, atol=1e-7,
                                       err_msg=f"epoch {e + 1} gamma / beta grad")
        ev = g.eval(2)
        print(f"epoch {e + 1}: engine {tr + ev} reference {ep['line']}")
        helpers.assert_line_close(tr + ev, ep["line"], cnt, what=f"epoch {e + 1}",
                                  ties=ep["ties"])


def test_initial_attention_tensor(loaded, pgcn):
    """attn is Glorot-uniform per vector (limit sqrt(6 / (d + 1))), drawn from the engine's
    xorshift stream right after the last layer weight, in tensor order -- bit for bit; the layer
    weights equal the plain engine's."""
    ds, hidden = loaded["cora"], (16, 8)
    L = 3
    g = pgcn.GCN(_params(pgcn, ds, hidden), ds)
    plain = pgcn.GCN(pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * L), ds)
    assert g.num_vars() == 3 * L + 2 and plain.num_vars() == 3 * L + 1
    n_w = 0
    for l in range(L):
        np.testing.assert_array_equal(g.get_var(_w(l)), plain.get_var(_w(l)))
        n_w += g.get_var(_w(l)).size
    attn = g.get_var(3 * L + 1)
    rng = gat_ref.Xorshift(pgcn.rng_jump(pgcn.rng_seed(0), n_w))
    want = []
    for d in (16, 8, ds.output_dim):
        limit = np.sqrt(np.float32(6.0) / np.float32(d + 1))
        for _ in range(2):
            r = rng.draws(d).astype(np.float32) / np.float32(gat_ref.RAND_MAX)
            want.append((((r.astype(np.float64) - 0.5) * np.float64(limit)) * 2.0)
                        .astype(np.float32))
    np.testing.assert_array_equal(attn, np.concatenate(want))
    g.close()
    plain.close()


def test_numeric_parity_cora(loaded, pgcn):
    """2 layers, hidden 16, the default dropouts, 3 training epochs each followed by eval(2):
    logits, every var2, every weight gradient, every var1.grad and the attn gradient after the
    first, the loss / accuracy lines of all three."""
    ds = loaded["cora"]
    g, ref, want, seed = _tie_free(pgcn, ds, (16,), (0.5, 0.5), 3)
    assert g.query("attention_layers") == 2 and g.num_vars() == 8
    _check_epochs(g, ref, want, ds, helpers.split_counts(ds))
    g.close()


def test_numeric_parity_residual_layernorm(loaded, pgcn):
    """3 layers, hidden 16 / 16, residual and LayerNorm on: one epoch.  The residual layer's
    attention backward reads the ReLU-masked gradient (dev_grad_z) the LayerNorm backward
    transformed."""
    ds = loaded["cora"]
    g, ref, want, seed = _tie_free(pgcn, ds, (16, 16), (0.5, 0.5, 0.5), 1, residual=True,
                                   layer_norm=True)
    assert g.query("attention_layers") == 3 and g.num_vars() == 3 * 3 + 3
    assert g.query("residual_layers") == 1 and g.query("norm_layers") == 2
    _check_epochs(g, ref, want, ds, helpers.split_counts(ds))
    g.close()


@pytest.fixture(scope="module")
def small(pgcn):
    """A synthetic n = 300, F = 24 graph with a seeded 5-class label matrix."""
    ds = pgcn.Dataset.synthetic(300, 24, 5, 900, 22)
    Y = np.random.default_rng(105).random((300, 5)) < 0.3
    return ds, Y


def test_multilabel(small, pgcn):
    """One epoch on a small multi-label dataset: the loss and the Hamming accuracy of the
    training and the validation pass against the reference (the same thresholded entries: no
    labelled logit of the reference is near zero), and the gradients."""
    _, Y = small
    ds = pgcn.Dataset.synthetic(300, 24, 5, 900, 22)
    ds.set_multilabel(Y)
    g, ref, want, seed = _tie_free(pgcn, ds, (16,), (0.5, 0.5), 1, label_bits=Y)
    assert g.query("multilabel") == 1 and g.query("attention_layers") == 2
    cnt = {s: k * 5 for s, k in helpers.split_counts(ds).items()}
    _check_epochs(g, ref, want, ds, cnt)
    bits, probs = g.predict_multilabel(probs=True)
    assert np.isfinite(probs).all()
    g.close()


class PatternDataset:
    """`ds` with another adjacency pattern (host arrays kept alive here)."""

    def __init__(self, pgcn, ds, indptr, indices):
        self.base = ds
        self.graph_indptr = np.ascontiguousarray(indptr, np.int32)
        self.graph_indices = np.ascontiguousarray(indices, np.int32)
        for k in ("num_nodes", "input_dim", "output_dim", "feat_indptr", "feat_indices",
                  "feat_values", "label", "split", "label_bits", "label_words"):
            setattr(self, k, getattr(ds, k))
        self.view = pgcn.PgcnData()
        for name, _ in pgcn.PgcnData._fields_:
            setattr(self.view, name, getattr(ds.view, name))
        ip = ctypes.POINTER(ctypes.c_int)
        self.view.graph_indptr = self.graph_indptr.ctypes.data_as(ip)
        self.view.graph_indices = self.graph_indices.ctypes.data_as(ip)


def test_directed_pattern(small, pgcn):
    """The small synthetic graph with half of each undirected pair removed (the slots below the
    diagonal): one epoch matches the reference -- the case the GCN path cannot train correctly
    (its backward needs a symmetric pattern)."""
    base, _ = small
    rows = np.repeat(np.arange(base.num_nodes), np.diff(base.graph_indptr))
    keep = base.graph_indices >= rows
    indptr = np.zeros(base.num_nodes + 1, np.int64)
    np.add.at(indptr, rows[keep] + 1, 1)
    indptr = np.cumsum(indptr)
    ds = PatternDataset(pgcn, base, indptr, base.graph_indices[keep])
    assert 0 < keep.sum() < len(keep)
    g, ref, want, seed = _tie_free(pgcn, ds, (16,), (0.5, 0.5), 1)
    assert g.query("graph_symmetric") == 0 and g.query("attention_layers") == 2
    _check_epochs(g, ref, want, ds, helpers.split_counts(ds))
    g.close()


def test_engine_facts(loaded, pgcn):
    """An attention engine has no reassociated output layer, no Â X precompute, no LDS GraphSum,
    runs no GraphSum kernel over an epoch, and calls the attention forward twice per layer and
    epoch (training + eval) and its backward once."""
    ds, hidden = loaded["cora"], (16, 16)
    L = 3
    g = pgcn.GCN(_params(pgcn, ds, hidden), ds)
    assert g.query("attention_layers") == L
    for key in ("reassociated", "eval_ax_us", "graphsum_lds"):
        assert g.query(key) == 0, key
    g.sync()
    pgcn.reset_path_counts()
    line = g.train_epoch() + g.eval(2)
    c = pgcn.path_counts()
    assert np.isfinite(line).all()
    assert c["gs_ring"] == 0 and c["gs_gather"] == 0 and c["out_xent"] == 0
    assert c["gat_fwd"] == 2 * L and c["gat_bwd"] == L
    g.close()
    plain = pgcn.GCN(pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * L), ds)
    assert plain.query("attention_layers") == 0
    plain.close()


def test_checkpoints(loaded, pgcn, tmp_path):
    """Save at epoch 3 and resume on a fresh engine to epoch 6: bit-identical to 6 straight
    epochs; the file is version 4 with flags bit 3; a flags-0 load of an attention file into a
    plain engine, and the reverse, is PGCN_E_INVALID (the engine untouched); weights-only loads
    cross in both directions."""
    ds, hidden = loaded["cora"], (16,)
    L = 2

    def make(attention, **kw):
        return pgcn.GCN(pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * L,
                                         attention=attention, **kw), ds)
    straight = make(True)
    want = _lines(straight, 6)
    a = make(True)
    np.testing.assert_array_equal(_lines(a, 3), want[:3])
    path = str(tmp_path / "attn.pgcnck")
    a.save(path)
    info = pgcn.checkpoint_info(path)
    n_w = ds.input_dim * 16 + 16 * ds.output_dim
    assert info["version"] == 4 and info["weights"] == n_w + 2 * (16 + ds.output_dim)
    assert pgcn.checkpoint_flags(path) == pgcn.CKPT_ATTENTION == 8
    b = make(True)
    b.load(path)
    np.testing.assert_array_equal(_lines(b, 3), want[3:])
    np.testing.assert_array_equal(b.results(6), want)
    for i in (_w(0), _w(1), 3 * L + 1):
        np.testing.assert_array_equal(b.get_var(i), straight.get_var(i))
    # with LayerNorm the file carries the norm tensor, then attn: flags 2 | 8
    n = make(True, layer_norm=True)
    _lines(n, 1)
    npath = str(tmp_path / "attn_norm.pgcnck")
    n.save(npath)
    assert pgcn.checkpoint_flags(npath) == 10 and pgcn.checkpoint_info(npath)["version"] == 4
    assert pgcn.checkpoint_info(npath)["weights"] == n_w + 2 * 16 + 2 * (16 + ds.output_dim)
    # a plain engine's file
    p = make(False)
    _lines(p, 2)
    ppath = str(tmp_path / "plain.pgcnck")
    p.save(ppath)
    assert pgcn.checkpoint_info(ppath)["version"] == 1 and pgcn.checkpoint_flags(ppath) == 0
    for eng, twin, other in ((a, make(True), ppath), (p, make(False), path)):
        twin.load(ppath if eng is p else path)
        with pytest.raises(pgcn.PgcnError) as e:
            eng.load(other)
        assert e.value.status == pgcn.PGCN_E_INVALID
        np.testing.assert_array_equal(_lines(eng, 1), _lines(twin, 1))
        twin.close()
    # weights only: a plain file leaves attn alone, a plain engine ignores the file's attn
    attn_before = a.get_var(3 * L + 1)
    a.load(ppath, weights_only=True)
    assert a.query("adam_steps") == 0
    fresh = make(False)
    fresh.load(ppath)
    for l in range(L):
        np.testing.assert_array_equal(a.get_var(_w(l)), fresh.get_var(_w(l)))
    np.testing.assert_array_equal(a.get_var(3 * L + 1), attn_before)
    p.load(path, weights_only=True)
    assert p.num_vars() == 3 * L + 1
    saved = make(True)
    saved.load(path)
    for l in range(L):
        np.testing.assert_array_equal(p.get_var(_w(l)), saved.get_var(_w(l)))
    # ... and an attention + LayerNorm file into an attention engine: attn from behind the norm
    a.load(npath, weights_only=True)
    np.testing.assert_array_equal(a.get_var(3 * L + 1), n.get_var(3 * L + 2))
    assert np.isfinite(_lines(a, 1)).all() and np.isfinite(_lines(p, 1)).all()
    for x in (straight, a, b, n, p, fresh, saved):
        x.close()


def test_set_var_predict_and_epoch_graph(loaded, pgcn):
    """set_var on attn changes the next logits; predict between two epochs leaves training
    bit-identical; epoch_graph on equals off bit for bit."""
    ds, hidden = loaded["cora"], (16,)
    L = 2
    attn_idx = 3 * L + 1
    g1, g2 = (pgcn.GCN(_params(pgcn, ds, hidden), ds) for _ in range(2))
    for _ in range(2):
        np.testing.assert_array_equal(_lines(g1, 1), _lines(g2, 1))
        cls, conf = g1.predict()
        assert cls.shape == (ds.num_nodes,) and np.isfinite(conf).all()
        assert g1.confusion(2).sum() == helpers.split_counts(ds)[2]
    np.testing.assert_array_equal(g1.get_var(attn_idx), g2.get_var(attn_idx))
    g1.eval(2)
    before = g1.get_var(_var2(L - 1))
    attn = g1.get_var(attn_idx)
    new = (attn + np.linspace(-1.0, 1.0, attn.size).astype(np.float32))
    g1.set_var(attn_idx, new)
    np.testing.assert_array_equal(g1.get_var(attn_idx), new)
    with pytest.raises(pgcn.PgcnError):
        g1.set_var(attn_idx, new[:-1])
    g1.eval(2)
    after = g1.get_var(_var2(L - 1))
    assert np.isfinite(after).all() and np.abs(after - before).max() > 1e-4
    g1.close()
    g2.close()
    runs = []
    for on in (0, 1):
        with helpers.knobs(pgcn, epoch_graph=on, sparse_dual=0):
            g = pgcn.GCN(_params(pgcn, ds, hidden), ds)
            for _ in range(3):
                g.epoch_async()
            runs.append((g.results(3), [g.get_var(_w(l)) for l in range(L)] +
                         [g.get_var(attn_idx)]))
            g.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert np.isfinite(runs[0][0]).all()
    for x, y in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(x, y)


def test_refusals(loaded, pgcn):
    """All four edge-cut creators and a hidden width of 132 are PGCN_E_INVALID."""
    ds = loaded["cora"]
    p = _params(pgcn, ds)
    group = pgcn.LoopbackGroup(1)
    makers = {
        "dist": lambda: pgcn.GCN(p, ds, rank=0, world=1, unique_id=b"\0" * 128),
        "peer": lambda: pgcn.GCN(p, ds, rank=0, world=1, allgather=lambda data: [data]),
        "loopback": lambda: pgcn.GCN(p, ds, rank=0, loopback=group),
        "solo": lambda: pgcn.GCN(p, ds, rank=0, world=2, solo=True),
        "wide": lambda: pgcn.GCN(_params(pgcn, ds, (132,)), ds),
    }
    for name, make in makers.items():
        with pytest.raises(pgcn.PgcnError) as e:
            make()
        assert e.value.status == pgcn.PGCN_E_INVALID, name
    g = pgcn.GCN(_params(pgcn, ds, (128,)), ds)
    assert g.num_vars() == 8 and np.isfinite(_lines(g, 1)).all()
    g.close()


def test_off_is_off(loaded, pgcn):
    """A plain engine built after an attention engine in the same process reproduces the golden
    cora lines as tests/test_gpu_engine.py's test_epoch_lines asks (losses within 1e-4,
    accuracies within the oracle's near-tied rows), with num_vars unchanged."""
    ds = loaded["cora"]
    a = pgcn.GCN(_params(pgcn, ds), ds)
    _lines(a, 1)
    a.close()
    g = pgcn.GCN(pgcn.make_params(ds), ds)
    assert g.num_vars() == 7 and g.query("attention_layers") == 0
    epochs = 10
    ours = _lines(g, epochs)
    g.close()
    gold = helpers.golden("cora")["epoch_lines"].reshape(-1, 4)[:epochs]
    ref = helpers.OracleGCN(helpers.ds_dict(ds))
    cnt = helpers.split_counts(ds)
    for e in range(epochs):
        _, ties = ref.epoch_with_ties(ds.label, ds.split, ds.output_dim, tol=1e-4)
        helpers.assert_line_close(ours[e], gold[e], cnt, what=f"epoch {e + 1}", ties=ties)
