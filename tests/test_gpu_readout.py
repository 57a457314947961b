"""The engine with a graph-level head (pgcn_params.readout) against the float64 numpy models of
tests/readout_ref.py (the node models of sage_ref.py / gat_heads_ref.py with a GraphHead), and
the engine's services on such an engine: predict, confusion, checkpoints, refusals, the loader.

The data: a Dataset.synthetic graph of 24 contiguous ranges of 5..40 rows (F = 12, C = 3, hidden
8), eight graphs per split, one of the training graphs unlabelled.  The adjacency is the synthetic
graph's own: the readout looks at row ranges only, the pattern need not be block-diagonal.

Tolerances are tests/test_gpu_sage.py's: rtol 1e-4 throughout, atol 1e-6 on the logits and 1e-7
on gradients, losses within 1e-4 relative, accuracies within the reference's near-tied graphs.
The weights after three epochs take rtol 1e-4 and atol 3e-6: Adam normalises the gradient, so each
step moves a weight by about LR = 0.01 whatever the gradient's size, the 1e-4 parity on such a
step is 1e-6 absolute, and there are three steps.

Seeds, as in test_gpu_sage.py: the first seed in 0..15 whose float64 run keeps every ReLU argument
and every max margin (the readout's, and a max aggregator's) 2e-6 of its tensor's largest value
away from a flip, over all three epochs -- a condition on the reference alone, computed on the
host (tests/test_cpu_readout.py checks the same seeds without a device; the attention case alone
takes the initial tensors from the engine, whose attention vectors have no host restatement
here, and searches its seed in the GPU test).  Under the max readout
the (graph, class) elements whose top two rows lie within 1e-5 max|logit| of each other without
being an exact tie are left out of the node-logit gradient's comparison (the rows of that graph
in that column); their share must stay below 2 %, or the test fails.
"""
import numpy as np
import pytest

import gat_ref
import helpers
import readout_ref as rr
import sage_ref

pytestmark = pytest.mark.gpu

FLIP, NEAR, CAP = 2e-6, 1e-5, 0.02
HIDDEN = (8,)
EPOCHS = 3
W_ATOL = 3e-6


def _w(l):
    return 2 + 3 * l


def _var2(l):
    return 3 + 3 * l


def graph_arrays():
    """(graph_ptr, labels, splits) of the 24 ranges."""
    rng = np.random.default_rng(7)
    lens = rng.integers(5, 41, 24)
    gp = np.zeros(25, np.int32)
    gp[1:] = np.cumsum(lens)
    labels = rng.integers(0, 3, 24).astype(np.int32)
    splits = (1 + np.arange(24) % 3).astype(np.int32)
    labels[3] = -1  # an unlabelled training graph
    assert splits[3] == 1
    return gp, labels, splits


def make_dataset(pgcn):
    gp, labels, splits = graph_arrays()
    n = int(gp[-1])
    ds = pgcn.Dataset.synthetic(n, 12, 3, 3 * n, 31)
    ds.set_graphs(gp, labels, splits, 3)
    return ds


def graph_counts(ds):
    lab, sp = np.asarray(ds.graph_label), np.asarray(ds.graph_split)
    return {s: int(((sp == s) & (lab >= 0)).sum()) for s in (1, 2, 3)}


# configurations: (name, engine keywords, hidden)
SAGE_MEAN = dict(aggregator="mean")
COMPOSED_SAGE = dict(aggregator="max", root_weight=True, layer_norm=True, residual=True)
COMPOSED_GAT = dict(attention=True, attention_heads=2)


def build_model(pgcn, ds, mode, hidden, dropout, seed, kw, init=None):
    """The float64 model of one configuration from the host's Glorot draws of `seed` (SAGE
    families), or from the engine's initial tensors `init` = (weights, attention tensor)."""
    dims = [ds.input_dim] + list(hidden) + [ds.output_dim]
    L = len(hidden) + 1
    p = (0.5,) * L if dropout else (0.0,) * L
    if kw.get("attention"):
        import gat_heads_ref
        w0, attn = init
        draws = sum(w.size for w in w0) + attn.size
    else:
        w0, draws = sage_ref.glorot_weights(pgcn, seed, dims, kw.get("root_weight", False))
    rng = gat_ref.Xorshift(pgcn.rng_jump(pgcn.rng_seed(seed), draws)) if dropout else None
    common = dict(residual=kw.get("residual", False), layer_norm=kw.get("layer_norm", False),
                  indptr=ds.graph_indptr, indices=ds.graph_indices)
    if kw.get("attention"):
        class Model(rr.GraphHead, gat_heads_ref.NumpyGatGCN):
            pass
        m = Model(ds, hidden, w0, attn, p, rng, heads=kw.get("attention_heads", 1), **common)
    else:
        m = rr.sage_model(ds, hidden, w0, p, rng, aggregator=kw["aggregator"],
                          root_weight=kw.get("root_weight", False), **common)
    return m.set_graphs(ds.graph_ptr, ds.graph_label, ds.graph_split, mode), w0, p


def reference_run(pgcn, ds, mode, hidden, dropout, seed, kw, init=None):
    """EPOCHS x (train_epoch + eval(2)) and a final eval(3) of the reference: what the engine is
    compared with, and how close a ReLU argument or a max margin came to a flip.  No device."""
    ref, w0, p = build_model(pgcn, ds, mode, hidden, dropout, seed, kw, init)
    c = ds.output_dim
    close = [1.0]

    def note():
        for y in ref.Y:
            nz = np.abs(y[y != 0])
            if nz.size:
                close.append(float(nz.min() / np.abs(y).max()))
        for gp_, q in zip(getattr(ref, "gap", []), getattr(ref, "qmax", [])):
            if gp_ is not None and (gp_ > 0).any():
                close.append(float(gp_[gp_ > 0].min() / q))
        if mode == "max":
            gap = ref.pool_gap[np.isfinite(ref.pool_gap) & (ref.pool_gap > 0)]
            close.append(float(gap.min() / np.abs(ref.node_logits).max()))

    def ties(sp):
        return helpers.near_ties(ref.pooled, ds.graph_label, ds.graph_split, sp, c)
    ep = dict(w0=w0, p=p, lines=[], ties=[])
    for e in range(EPOCHS):
        tl = ref.forward(1, training=True)
        ta, t1 = ref.acc, ties(1)
        note()
        if e == 0:
            ep["node_logits"] = ref.node_logits.copy()
            ep["near"] = ref.pool_near_tied(NEAR) if mode == "max" else None
        ref.backward()
        if e == 0:
            ep["node_grad"] = ref.node_grad.copy()
            ep["dW"] = [w.copy() for w in ref.dW]
        ref.step()
        vl = ref.forward(2)
        note()
        ep["lines"].append((tl, ta, vl, ref.acc))
        ep["ties"].append({1: t1, 2: ties(2)})
    ep["W"] = [w.copy() for w in ref.W]
    tsl = ref.forward(3)
    ep["test"] = (tsl, ref.acc, ties(3))
    ep["pooled"] = ref.pooled.copy()
    ep["close"] = min(close)
    ep["share"] = 0.0 if ep["near"] is None else float(ep["near"].mean())
    return ep


def flip_free(pgcn, ds, mode, hidden, dropout, kw, init_of=None):
    for seed in range(16):
        ep = reference_run(pgcn, ds, mode, hidden, dropout, seed, kw,
                           init_of(seed) if init_of else None)
        print(f"seed {seed}: closest argument {ep['close']:.3g}, near-tied share {ep['share']:.3g}")
        if ep["close"] >= FLIP and ep["share"] < CAP:
            return seed, ep
    raise AssertionError("no seed in 0..15 keeps every ReLU argument and max margin off a flip")


def _params(pgcn, ds, mode, hidden, p, seed=0, **kw):
    return pgcn.make_params(ds, hidden_dims=hidden, dropouts=p, readout=mode, seed=seed, **kw)


def check_run(pgcn, ds, mode, hidden, dropout, kw):
    L, n, c = len(hidden) + 1, ds.num_nodes, ds.output_dim
    p = (0.5,) * L if dropout else (0.0,) * L
    init_of = None
    if kw.get("attention"):  # the attention tensor's draws: from the engine itself
        def init_of(seed):
            e = pgcn.GCN(_params(pgcn, ds, mode, hidden, p, seed, **kw), ds)
            out = [e.get_var(_w(l)) for l in range(L)], e.get_var(e.num_vars() - 1)
            e.close()
            return out
    seed, ep = flip_free(pgcn, ds, mode, hidden, dropout, kw, init_of)
    g = pgcn.GCN(_params(pgcn, ds, mode, hidden, p, seed, **kw), ds)
    assert g.query("readout") == rr.MODE_ID[mode] and g.query("num_graphs") == ds.num_graphs
    assert g.query("reassociated") == 0
    for l in range(L):
        np.testing.assert_array_equal(g.get_var(_w(l)).ravel(), np.ravel(ep["w0"][l]),
                                      err_msg=f"W{l}")
    cnt = graph_counts(ds)
    for e in range(EPOCHS):
        tr = g.train_epoch()
        if e == 0:
            got = g.get_var(_var2(L - 1)).reshape(n, c)
            np.testing.assert_allclose(got, ep["node_logits"], rtol=1e-4, atol=1e-6,
                                       err_msg="node logits")
            got, want = g.get_var(_var2(L - 1), 1).reshape(n, c), ep["node_grad"]
            if ep["near"] is not None:
                assert ep["near"].mean() < CAP
                m = ep["near"][rr.node_graph(ds.graph_ptr)]
                got, want = np.where(m, 0.0, got), np.where(m, 0.0, want)
            np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-7, err_msg="node-logit grad")
            for l in range(L):
                np.testing.assert_allclose(g.get_var(_w(l), 1).reshape(ep["dW"][l].shape),
                                           ep["dW"][l], rtol=1e-4, atol=1e-7,
                                           err_msg=f"W{l} grad")
        ev = g.eval(2)
        print(f"epoch {e}: engine {tr + ev} reference {ep['lines'][e]}")
        helpers.assert_line_close(tr + ev, ep["lines"][e], cnt, what=f"{mode} epoch {e}",
                                  ties=ep["ties"][e])
    for l in range(L):
        np.testing.assert_allclose(g.get_var(_w(l)).reshape(ep["W"][l].shape), ep["W"][l],
                                   rtol=1e-4, atol=W_ATOL, err_msg=f"W{l} after {EPOCHS} epochs")
    tl, ta = g.eval(3)
    wl, wa, wt = ep["test"]
    print(f"eval(3): engine {(tl, ta)} reference {(wl, wa)}")
    assert abs(tl - wl) <= 1e-4 * abs(wl)
    assert abs(ta - wa) * cnt[3] <= wt + 1e-3
    return g, ep


@pytest.fixture(scope="module")
def data(pgcn):
    return make_dataset(pgcn)


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("mode", rr.MODES)
def test_numeric_parity(data, pgcn, mode, dropout):
    """Per mode, without dropout and with it: the node logits, their gradient and every weight
    gradient of the first epoch, three epoch lines, the weights after them, and eval(3)."""
    g, ep = check_run(pgcn, data, mode, HIDDEN, dropout, SAGE_MEAN)
    # predict: G rows, the model's argmax (graphs with a top-two margin below 1e-5 aside)
    cls, conf, probs = g.predict(probs=True)
    G = data.num_graphs
    assert cls.shape == (G,) and conf.shape == (G,) and probs.shape == (G, data.output_dim)
    top = np.sort(ep["pooled"], axis=1)
    clear = top[:, -1] - top[:, -2] > 1e-5 * np.abs(ep["pooled"]).max()
    assert clear.sum() >= G - 1
    np.testing.assert_array_equal(cls[clear], ep["pooled"].argmax(axis=1)[clear])
    np.testing.assert_allclose(probs.sum(axis=1), 1.0, rtol=1e-5)
    cnt = graph_counts(data)
    for s in (1, 2, 3):
        assert g.confusion(s).sum() == cnt[s]
    assert cnt[1] == 7 and cnt[2] == 8
    assert g.node_range() == (0, data.num_nodes)
    g.close()


def test_composes_with_attention_heads(data, pgcn):
    g, _ = check_run(pgcn, data, "mean", HIDDEN, True, COMPOSED_GAT)
    assert g.query("attention_layers") == 2 and g.query("attention_heads") == 2
    g.close()


def test_composes_with_max_aggregator_layernorm_residual(data, pgcn):
    """3 layers 8 / 8: the middle layer is residual-eligible."""
    g, _ = check_run(pgcn, data, "mean", (8, 8), True, COMPOSED_SAGE)
    assert g.query("residual_layers") == 1 and g.query("norm_layers") == 2
    assert g.query("aggregator") == 2 and g.query("root_weight") == 1
    g.close()


def _lines(g, k):
    return np.array([g.train_epoch() + g.eval(2) for _ in range(k)], np.float32)


@pytest.mark.parametrize("mode,kw", [("max", {}), ("mean", SAGE_MEAN)])
def test_checkpoints(data, pgcn, tmp_path, mode, kw):
    """save -> new engine -> load -> the continued epochs equal an uninterrupted run bit for bit;
    the file is version 7 with flag bit 5 and the {readout, num_graphs} block; a load into an
    engine without a readout or with another mode is refused; a plain engine's file keeps its
    version."""
    ds, p = data, (0.5, 0.5)

    def make(m, **k):
        return pgcn.GCN(_params(pgcn, ds, m, HIDDEN, p, **k), ds)
    straight = make(mode, **kw)
    want = _lines(straight, 6)
    a = make(mode, **kw)
    np.testing.assert_array_equal(_lines(a, 3), want[:3])
    path = str(tmp_path / "readout.pgcnck")
    a.save(path)
    assert pgcn.checkpoint_info(path)["version"] == 7
    flags = pgcn.checkpoint_flags(path)
    assert flags & 32 and pgcn.CKPT_READOUT == 32
    assert bool(flags & pgcn.CKPT_SAGE) == bool(kw)
    assert pgcn.checkpoint_readout(path) == (rr.MODE_ID[mode], ds.num_graphs)
    assert pgcn.checkpoint_sage(path) == ((1, 0) if kw else (0, 0))
    b = make(mode, **kw)
    b.load(path)
    np.testing.assert_array_equal(_lines(b, 3), want[3:])
    np.testing.assert_array_equal(b.results(6), want)
    for l in range(2):
        np.testing.assert_array_equal(b.get_var(_w(l)), straight.get_var(_w(l)))
    other = "sum" if mode != "sum" else "mean"
    for m in (None, other):
        o, twin = make(m, **kw), make(m, **kw)
        for weights_only in (False, True):
            with pytest.raises(pgcn.PgcnError) as e:
                o.load(path, weights_only=weights_only)
            assert e.value.status == pgcn.PGCN_E_INVALID
        np.testing.assert_array_equal(_lines(o, 1), _lines(twin, 1))  # (untouched)
        o.close()
        twin.close()
    plain = make(None)
    _lines(plain, 1)
    ppath = str(tmp_path / "plain.pgcnck")
    plain.save(ppath)
    assert pgcn.checkpoint_info(ppath)["version"] == 1 and pgcn.checkpoint_flags(ppath) == 0
    assert pgcn.checkpoint_readout(ppath) == (0, 0)
    with pytest.raises(pgcn.PgcnError) as e:
        a.load(ppath)
    assert e.value.status == pgcn.PGCN_E_INVALID
    for x in (straight, a, b, plain):
        x.close()


def test_epoch_graph_and_predict_leave_training_alone(data, pgcn):
    """Plain GCN layers under a readout: predict between epochs changes nothing, and captured
    epochs equal eager ones bit for bit."""
    ds, p = data, (0.5, 0.5)
    g1, g2 = (pgcn.GCN(_params(pgcn, ds, "sum", HIDDEN, p), ds) for _ in range(2))
    for _ in range(2):
        np.testing.assert_array_equal(_lines(g1, 1), _lines(g2, 1))
        assert g1.predict()[0].shape == (ds.num_graphs,)
    g1.close()
    g2.close()
    runs = []
    for on in (0, 1):
        with helpers.knobs(pgcn, epoch_graph=on):
            g = pgcn.GCN(_params(pgcn, ds, "max", HIDDEN, p), ds)
            for _ in range(3):
                g.epoch_async()
            runs.append((g.results(3), [g.get_var(_w(l)) for l in range(2)]))
            g.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert np.isfinite(runs[0][0]).all()
    for x, y in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(x, y)


def test_refusals(data, pgcn):
    """PGCN_E_INVALID at engine build: a readout with multilabel, without graphs attached, with a
    mode outside 0..3, and on a loopback rank."""
    ds = data
    n = ds.num_nodes
    bare = pgcn.Dataset.synthetic(n, 12, 3, 3 * n, 31)
    multi = make_dataset(pgcn)
    multi.set_multilabel(np.random.default_rng(1).random((n, 3)) < 0.4)
    group = pgcn.LoopbackGroup(1)

    def raw(d, **kw):
        q = pgcn.make_params(d, hidden_dims=HIDDEN)
        for k, v in kw.items():
            setattr(q, k, v)
        return lambda: pgcn.GCN(q, d)
    p = _params(pgcn, ds, "mean", HIDDEN, (0.5, 0.5))
    makers = {
        "multilabel": raw(multi, readout=2, multilabel=1),
        "no graphs": raw(bare, readout=1),
        "mode 4": raw(ds, readout=4),
        "mode -1": raw(ds, readout=-1),
        "loopback": lambda: pgcn.GCN(p, ds, rank=0, loopback=group),
        "dist": lambda: pgcn.GCN(p, ds, rank=0, world=1, unique_id=b"\0" * 128),
    }
    for name, make in makers.items():
        with pytest.raises(pgcn.PgcnError) as e:
            make()
        assert e.value.status == pgcn.PGCN_E_INVALID, name
    with pytest.raises(ValueError):
        pgcn.make_params(multi, readout="mean", multilabel=True)


def test_text_loader_equals_set_graphs(pgcn, tmp_path):
    """A block-diagonal batch written as .graph / .svmlight / .split / .graphs text and loaded
    through Dataset.load + load_graphs trains to the same losses as the same data attached with
    set_graphs (plain GCN layers, mean readout)."""
    rng = np.random.default_rng(3)
    lens = rng.integers(5, 13, 9)
    gp = np.zeros(10, np.int32)
    gp[1:] = np.cumsum(lens)
    n = int(gp[-1])
    labels = rng.integers(0, 3, 9)
    labels[:3] = (0, 1, 2)
    labels[5] = -1
    splits = 1 + np.arange(9) % 3
    nbr = [set() for _ in range(n)]
    for g in range(9):
        b, e = int(gp[g]), int(gp[g + 1])
        for _ in range(2 * (e - b)):
            i, j = rng.integers(b, e, 2)
            if i != j:
                nbr[i].add(int(j))
                nbr[j].add(int(i))
    data = tmp_path / "data"
    data.mkdir()
    with open(data / "mol.graph", "w") as f:
        f.write("".join(" ".join(map(str, sorted(s))) + "\n" for s in nbr))
    with open(data / "mol.svmlight", "w") as f:
        for i in range(n):
            f.write(f"{i % 3} " + " ".join(f"{k}:{rng.standard_normal():.5f}" for k in range(6)) +
                    "\n")
    with open(data / "mol.split", "w") as f:
        f.write("".join(f"{1 + i % 3}\n" for i in range(n)))
    with open(data / "mol.graphs", "w") as f:
        f.write("".join(f"{k} {l} {s}\n" for k, l, s in zip(lens, labels, splits)))
    a = pgcn.Dataset.load(str(tmp_path), "mol")
    a.load_graphs(str(data / "mol.graphs"))
    b = pgcn.Dataset.load(str(tmp_path), "mol")
    b.set_graphs(gp, labels, splits)
    assert a.num_graphs == b.num_graphs == 9 and a.output_dim == b.output_dim == 3
    for k in ("graph_ptr", "graph_label", "graph_split"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)
    np.testing.assert_array_equal(a.graph_ptr, gp)
    lines = []
    for ds in (a, b):
        g = pgcn.GCN(_params(pgcn, ds, "mean", HIDDEN, (0.5, 0.5)), ds)
        lines.append(_lines(g, 3))
        g.close()
    np.testing.assert_array_equal(lines[0], lines[1])
    assert np.isfinite(lines[0]).all()
