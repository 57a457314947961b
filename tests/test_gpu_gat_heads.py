"""The attention engine with several heads and attention dropout (pgcn_params.attention_heads /
attention_dropout) against the float64 numpy model of tests/gat_heads_ref.py (NumpyGatGCN:
tests/gat_ref.py's model with heads and the attention masks drawn at their stream positions),
started from the engine's initial tensors; and the engine's services on such an engine:
checkpoints (version 5), set_var, predict, epoch graphs, the stats keys, the refusals.

Tolerances are tests/test_gpu_gat.py's: rtol 1e-4, atol 1e-6 on values, 1e-7 on gradients;
losses within 1e-4 relative; accuracies within the reference's near-tied rows.
"""
import os
import subprocess

import numpy as np
import pytest

import gat_heads_ref as ref_mh
import gat_ref
import helpers
from test_gpu_gat import (PatternDataset, _check_epochs, _closest, _lines, _var2, _w,
                          small)  # noqa: F401  (small: a fixture)

pytestmark = pytest.mark.gpu


def _params(pgcn, ds, hidden=(16,), dropouts=None, heads=1, p=0.0, attention=True, **kw):
    L = len(hidden) + 1
    return pgcn.make_params(ds, hidden_dims=hidden, dropouts=dropouts or (0.5,) * L,
                            attention=attention, attention_heads=heads, attention_dropout=p, **kw)


def _pair(pgcn, ds, hidden, dropouts, seed, heads, p, label_bits=None, **kw):
    """An engine and the reference started from its initial tensors; the reference's stream
    stands behind the engine's initial draws (weights, then the attention vectors)."""
    L = len(hidden) + 1
    g = pgcn.GCN(_params(pgcn, ds, hidden, dropouts, heads, p, seed=seed,
                         multilabel=label_bits is not None, **kw), ds)
    w0 = [g.get_var(_w(l)) for l in range(L)]
    attn0 = g.get_var(g.num_vars() - 1)
    draws = sum(w.size for w in w0) + attn0.size
    rng = gat_ref.Xorshift(pgcn.rng_jump(pgcn.rng_seed(seed), draws))
    ref = ref_mh.NumpyGatGCN(ds, hidden, w0, attn0, dropouts, rng,
                             residual=kw.get("residual", False),
                             layer_norm=kw.get("layer_norm", False), label_bits=label_bits,
                             indptr=ds.graph_indptr, indices=ds.graph_indices, heads=heads,
                             attn_p=p)
    return g, ref


def _reference_epochs(ref, epochs, ds):
    """tests/test_gpu_gat.py's _reference_epochs (the reference's train_epoch + eval(2), the
    tensors of each training pass, the line, the near-tied rows), with how close any ReLU /
    LeakyReLU / class-threshold argument of the TRAINING forward came to zero kept apart."""
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
        ep.update(line=(tl, ta, vl, ref.acc), ties={1: t1, 2: t2}, close_train=close)
        out.append(ep)
    return out


def _tie_free(pgcn, ds, hidden, dropouts, epochs, heads, p, seeds=range(8), bound=2e-6, **kw):
    """The first of `seeds` for which no ReLU, LeakyReLU or class-threshold argument of the
    float64 run's first training forward comes within `bound` of its tensor's largest value of
    zero -- a condition on the reference alone; 2e-6 is tests/test_gpu_gat.py's bound (three
    times an fp32 sum's error at these widths).  It is asked of the first training pass, whose
    tensors and gradients are compared element by element (a LeakyReLU branch taken the other
    way changes a slot's dx by a factor of 5); the later epochs are compared by their loss lines
    at 1e-4, which one slot's branch does not reach."""
    for seed in seeds:
        g, ref = _pair(pgcn, ds, hidden, dropouts, seed, heads, p, **kw)
        want = _reference_epochs(ref, 1, ds)
        close = want[0]["close_train"]
        print(f"seed {seed}: closest argument {close:.3g}")
        if close >= bound:
            return g, ref, want + _reference_epochs(ref, epochs - 1, ds), seed
        g.close()
    raise AssertionError("no seed keeps every ReLU / LeakyReLU argument off zero")


# The published shape on cora has 13,566 x 8 + 13,566 scores and 2,708 x 64 ReLU arguments in
# one forward, 8.5 times the single-head model's: of the seeds 0..47 none keeps all of them 2e-6
# of the largest away from zero (the best, 36, reaches 1.6e-6).  Its bound is 1e-6: a score is a
# 9-term fp32 sum (a head's 8 products and the add), whose worst-case error is 9 * 2^-24 =
# 5.4e-7 of the terms' absolute sum, and 1e-6 is about twice that; the first seed from 32 on
# that meets it is 35.
WIDE = dict(seeds=range(32, 48), bound=1e-6)


@pytest.mark.parametrize("hidden,heads,p,kw", [
    ((16,), 4, 0.0, {}),
    ((64,), 8, 0.6, WIDE),  # the published model's shape
    ((16, 16), 2, 0.3, dict(residual=True, layer_norm=True)),
], ids=["h16_k4", "h64_k8_p06", "h16x2_k2_res_ln_p03"])
def test_numeric_parity_cora(loaded, pgcn, hidden, heads, p, kw):
    """3 training epochs each followed by eval(2): logits, every var2, every weight gradient,
    every var1.grad, the attention gradient (and the LayerNorm gradients) after the first, the
    loss / accuracy lines of all three."""
    ds = loaded["cora"]
    L = len(hidden) + 1
    g, ref, want, seed = _tie_free(pgcn, ds, hidden, (0.5,) * L, 3, heads, p, **kw)
    assert g.query("attention_layers") == L and g.query("attention_heads") == heads
    assert g.query("attention_dropout_layers") == (L if p > 0 else 0)
    _check_epochs(g, ref, want, ds, helpers.split_counts(ds))
    g.close()


def test_multilabel(small, pgcn):
    """The small multi-label dataset, 2 heads, attention dropout 0.3: three epochs."""
    _, Y = small
    ds = pgcn.Dataset.synthetic(300, 24, 5, 900, 22)
    ds.set_multilabel(Y)
    g, ref, want, seed = _tie_free(pgcn, ds, (16,), (0.5, 0.5), 3, 2, 0.3, label_bits=Y)
    assert g.query("multilabel") == 1 and g.query("attention_heads") == 2
    cnt = {s: k * 5 for s, k in helpers.split_counts(ds).items()}
    _check_epochs(g, ref, want, ds, cnt)
    g.close()


def test_directed_pattern(small, pgcn):
    """The small synthetic graph with the slots below the diagonal removed, 4 heads, attention
    dropout 0.6: three epochs (the transposed index is not the CSR; the mask is per CSR slot)."""
    base, _ = small
    rows = np.repeat(np.arange(base.num_nodes), np.diff(base.graph_indptr))
    keep = base.graph_indices >= rows
    indptr = np.zeros(base.num_nodes + 1, np.int64)
    np.add.at(indptr, rows[keep] + 1, 1)
    indptr = np.cumsum(indptr)
    ds = PatternDataset(pgcn, base, indptr, base.graph_indices[keep])
    g, ref, want, seed = _tie_free(pgcn, ds, (16,), (0.5, 0.5), 3, 4, 0.6)
    assert g.query("graph_symmetric") == 0
    _check_epochs(g, ref, want, ds, helpers.split_counts(ds))
    g.close()


def test_off_is_off(loaded, pgcn):
    """attention = 1, heads = 1, p = 0 (and heads = 0, which counts as 1) gives the losses and
    the get_var bits of an engine built without the new members set, and launches the
    single-head kernels; a non-attention engine is untouched by the members' defaults."""
    ds = loaded["cora"]
    base = pgcn.make_params(ds, attention=True)
    assert base.attention_heads == 1 and base.attention_dropout == 0.0
    runs = []
    for heads in (None, 1, 0):
        p = pgcn.make_params(ds, attention=True) if heads is None else _params(pgcn, ds, heads=heads)
        g = pgcn.GCN(p, ds)
        g.sync()
        pgcn.reset_path_counts()
        lines = _lines(g, 3)
        assert pgcn.path_counts()["gat_heads"] == 0
        assert g.query("attention_heads") == 1 and g.query("attention_dropout_layers") == 0
        runs.append((lines, [g.get_var(i) for i in range(1, g.num_vars())],
                     g.get_var(_w(0), 1)))
        g.close()
    for lines, vars_, grad in runs[1:]:
        np.testing.assert_array_equal(lines, runs[0][0])
        for x, y in zip(vars_, runs[0][1]):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(grad, runs[0][2])
    plain = pgcn.GCN(pgcn.make_params(ds), ds)
    assert plain.query("attention_heads") == 1 and plain.query("attention_dropout_layers") == 0
    gold = helpers.golden("cora")["epoch_lines"].reshape(-1, 4)[:2]
    ours = _lines(plain, 2)
    np.testing.assert_allclose(ours[:, [0, 2]], gold[:, [0, 2]], rtol=1e-4)
    plain.close()


def test_existing_masks_keep_their_offsets(loaded, pgcn):
    """Epoch 1 of an engine with attention dropout: the dropped input features are the p = 0
    engine's bit for bit (the input mask), and the hidden layer's dropped entries are the ones
    the stream gives right behind the input mask's draws (the hidden mask) -- the attention
    masks stand behind both."""
    ds, seed = loaded["cora"], 3
    a = pgcn.GCN(_params(pgcn, ds, (16,), heads=4, p=0.6, seed=seed), ds)
    b = pgcn.GCN(_params(pgcn, ds, (16,), heads=4, p=0.0, seed=seed), ds)
    a.train_epoch()
    b.train_epoch()
    xa, xb = a.get_var(0), b.get_var(0)
    assert (xa == 0).sum() > 0.3 * xa.size
    np.testing.assert_array_equal(xa, xb)
    draws = sum(a.get_var(_w(l)).size for l in range(2)) + a.get_var(a.num_vars() - 1).size
    rng = gat_ref.Xorshift(pgcn.rng_jump(pgcn.rng_seed(seed), draws))
    rng.draws(len(ds.feat_values))
    keep = rng.keep(ds.num_nodes * 16, 0.5).reshape(ds.num_nodes, 16)
    for g in (a, b):
        h = g.get_var(_var2(0)).reshape(ds.num_nodes, 16)
        assert (h[~keep] == 0).all() and (h[keep] != 0).mean() > 0.2
    a.close()
    b.close()


def test_checkpoints(loaded, pgcn, tmp_path):
    """K = 4, p = 0.6: save at epoch 2, resume in a fresh engine, epochs 3-4 bit-equal to an
    uninterrupted run; the file is version 5 with flags bit 3 and the extension
    checkpoint_attention reads; a flags-0 load refuses a file whose heads or dropout differ
    (a version-4 file into such an engine and the reverse included, the engine untouched); a
    weights-only load crosses it."""
    ds, hidden = loaded["cora"], (16,)

    def make(heads=4, p=0.6, **kw):
        return pgcn.GCN(_params(pgcn, ds, hidden, heads=heads, p=p, **kw), ds)
    straight = make()
    want = _lines(straight, 4)
    a = make()
    np.testing.assert_array_equal(_lines(a, 2), want[:2])
    path = str(tmp_path / "heads.pgcnck")
    a.save(path)
    info = pgcn.checkpoint_info(path)
    n_w = ds.input_dim * 16 + 16 * ds.output_dim + 2 * (16 + ds.output_dim)
    assert info["version"] == 5 and info["weights"] == n_w and info["epochs"] == 2
    assert pgcn.checkpoint_flags(path) == pgcn.CKPT_ATTENTION
    heads, p = pgcn.checkpoint_attention(path)
    assert heads == 4 and p == np.float32(0.6)
    b = make()
    b.load(path)
    np.testing.assert_array_equal(_lines(b, 2), want[2:])
    np.testing.assert_array_equal(b.results(4), want)
    for i in (_w(0), _w(1), b.num_vars() - 1):
        np.testing.assert_array_equal(b.get_var(i), straight.get_var(i))
    # a single-head file without attention dropout stays version 4
    one = make(1, 0.0)
    _lines(one, 1)
    v4 = str(tmp_path / "one.pgcnck")
    one.save(v4)
    assert pgcn.checkpoint_info(v4)["version"] == 4 and pgcn.checkpoint_attention(v4) == (1, 0.0)
    # heads only, dropout only: version 5 both
    for eng_kw, name in (((2, 0.0), "k2"), ((1, 0.25), "p25")):
        e = make(*eng_kw)
        _lines(e, 1)
        f = str(tmp_path / f"{name}.pgcnck")
        e.save(f)
        assert pgcn.checkpoint_info(f)["version"] == 5
        assert pgcn.checkpoint_attention(f) == (eng_kw[0], float(np.float32(eng_kw[1])))
        e.close()
    k2 = str(tmp_path / "k2.pgcnck")
    # refusals, the engine untouched: it goes on as a twin that never tried
    for eng, twin, own, others in ((a, make(), path, (v4, k2, str(tmp_path / "p25.pgcnck"))),
                                   (one, make(1, 0.0), v4, (path, k2))):
        twin.load(own)
        eng.load(own)
        for other in others:
            with pytest.raises(pgcn.PgcnError) as e:
                eng.load(other)
            assert e.value.status == pgcn.PGCN_E_INVALID, other
        np.testing.assert_array_equal(_lines(eng, 1), _lines(twin, 1))
        twin.close()
    # weights only crosses heads and dropout in both directions
    one.load(path, weights_only=True)
    a.load(v4, weights_only=True)
    saved, saved1 = make(), make(1, 0.0)
    saved.load(path)
    saved1.load(v4)
    for i in (_w(0), _w(1), a.num_vars() - 1):
        np.testing.assert_array_equal(one.get_var(i), saved.get_var(i))
        np.testing.assert_array_equal(a.get_var(i), saved1.get_var(i))
    assert one.query("adam_steps") == 0 and a.query("adam_steps") == 0
    assert np.isfinite(_lines(one, 1)).all() and np.isfinite(_lines(a, 1)).all()
    for x in (straight, a, b, one, saved, saved1):
        x.close()


def test_set_var_predict_and_epoch_graph(loaded, pgcn):
    """K = 4, p = 0.6: predict between two epochs leaves training bit-identical (an eval forward
    draws nothing); set_var on attn changes the next logits; epoch_graph on equals off bit for
    bit."""
    ds, hidden = loaded["cora"], (16,)
    L = 2
    attn_idx = 3 * L + 1
    g1, g2 = (pgcn.GCN(_params(pgcn, ds, hidden, heads=4, p=0.6), ds) for _ in range(2))
    for _ in range(2):
        np.testing.assert_array_equal(_lines(g1, 1), _lines(g2, 1))
        cls, conf = g1.predict()
        assert cls.shape == (ds.num_nodes,) and np.isfinite(conf).all()
    np.testing.assert_array_equal(g1.get_var(attn_idx), g2.get_var(attn_idx))
    g1.eval(2)
    before = g1.get_var(_var2(L - 1))
    g1.eval(2)
    np.testing.assert_array_equal(g1.get_var(_var2(L - 1)), before)  # eval uses no mask
    attn = g1.get_var(attn_idx)
    g1.set_var(attn_idx, attn + np.linspace(-1.0, 1.0, attn.size).astype(np.float32))
    g1.eval(2)
    after = g1.get_var(_var2(L - 1))
    assert np.isfinite(after).all() and np.abs(after - before).max() > 1e-4
    g1.close()
    g2.close()
    runs = []
    for on in (0, 1):
        with helpers.knobs(pgcn, epoch_graph=on, sparse_dual=0):
            g = pgcn.GCN(_params(pgcn, ds, hidden, heads=4, p=0.6), ds)
            for _ in range(3):
                g.epoch_async()
            runs.append((g.results(3), [g.get_var(_w(l)) for l in range(L)] +
                         [g.get_var(attn_idx)]))
            g.close()
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert np.isfinite(runs[0][0]).all()
    for x, y in zip(runs[0][1], runs[1][1]):
        np.testing.assert_array_equal(x, y)


def test_kernel_calls(loaded, pgcn):
    """Per epoch (training + eval) every layer calls the attention forward twice and its backward
    once; the hidden layers' calls count as "gat_heads", the single-head output layer's do not."""
    ds, hidden = loaded["cora"], (16, 16)
    L = 3
    g = pgcn.GCN(_params(pgcn, ds, hidden, heads=2, p=0.5), ds)
    g.sync()
    pgcn.reset_path_counts()
    line = g.train_epoch() + g.eval(2)
    c = pgcn.path_counts()
    assert np.isfinite(line).all()
    assert c["gat_fwd"] == 2 * L and c["gat_bwd"] == L and c["gat_heads"] == 3 * (L - 1)
    g.close()


def test_refusals(loaded, pgcn):
    """PGCN_E_INVALID at engine build: heads outside [1, 32], heads not dividing a hidden width,
    a head width of 2 (or 12), p outside [0, 1), heads or dropout without attention, and the
    edge-cut creators."""
    ds = loaded["cora"]
    bad = {
        "heads -1": _params(pgcn, ds, heads=-1),
        "heads 33": _params(pgcn, ds, (128,), heads=33),
        "heads 3 of 16": _params(pgcn, ds, heads=3),
        "dh 2": _params(pgcn, ds, heads=8),
        "dh 12": _params(pgcn, ds, (24,), heads=2),
        "second width": _params(pgcn, ds, (16, 24), heads=4),
        "p 1": _params(pgcn, ds, p=1.0),
        "p -0.1": _params(pgcn, ds, p=-0.1),
        "heads without attention": _params(pgcn, ds, heads=2, attention=False),
        "dropout without attention": _params(pgcn, ds, p=0.5, attention=False),
    }
    for name, p in bad.items():
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.GCN(p, ds)
        assert e.value.status == pgcn.PGCN_E_INVALID, name
    p = _params(pgcn, ds, heads=4, p=0.6)
    group = pgcn.LoopbackGroup(1)
    makers = {
        "dist": lambda: pgcn.GCN(p, ds, rank=0, world=1, unique_id=b"\0" * 128),
        "peer": lambda: pgcn.GCN(p, ds, rank=0, world=1, allgather=lambda data: [data]),
        "loopback": lambda: pgcn.GCN(p, ds, rank=0, loopback=group),
        "solo": lambda: pgcn.GCN(p, ds, rank=0, world=2, solo=True),
    }
    for name, make in makers.items():
        with pytest.raises(pgcn.PgcnError) as e:
            make()
        assert e.value.status == pgcn.PGCN_E_INVALID, name
    g = pgcn.GCN(_params(pgcn, ds, (128,), heads=32, p=0.9), ds)
    assert np.isfinite(_lines(g, 1)).all()
    g.close()


def test_cli(pgcn, datasets, tmp_path):
    """gcn-par takes heads= and attn_dropout= from the command line and from the parameter file:
    the checkpoint it saves is a version-5 file with those values; heads that do not divide the
    hidden width, or heads without attention, end the run with an error."""
    root, names = datasets
    exe = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "gcn-par")
    ck, ck2 = str(tmp_path / "ck"), str(tmp_path / "ck2")

    def run(*args):
        return subprocess.run([exe, names["cora"], f"root={root}", *args], capture_output=True,
                              text=True, timeout=300)
    r = run("attention=1", "heads=4", "attn_dropout=0.6", "epochs=2", f"save={ck}")
    assert r.returncode == 0, r.stderr[-2000:]
    assert pgcn.checkpoint_info(ck)["version"] == 5
    assert pgcn.checkpoint_attention(ck) == (4, float(np.float32(0.6)))
    pfile = tmp_path / "params.txt"
    pfile.write_text("attention = 1\nheads = 2\nattn_dropout = 0.25\nepochs = 1\n")
    r = run(f"file={pfile}", f"save={ck2}")
    assert r.returncode == 0, r.stderr[-2000:]
    assert pgcn.checkpoint_attention(ck2) == (2, 0.25)
    r = run("attention=1", "heads=3", "epochs=1")
    assert r.returncode != 0 and "GCN creation failed" in r.stderr
    r = run("heads=2", "epochs=1")  # heads without attention
    assert r.returncode != 0
