"""BatchNorm of the hidden layers (pgcn_params.batch_norm) in the engine: parity with the float64
model of tests/batchnorm_ref.py, the fused tail, off-is-off, refusals, checkpoints and one run per
composition.  The kernels themselves: tests/test_gpu_batchnorm_kernels.py.
"""
import numpy as np
import pytest

import batchnorm_ref as ref
import helpers
from test_gpu_layernorm import _lines, _norm, _var2, _w

pytestmark = pytest.mark.gpu

SYN = (600, 48, 7, 2400, 5)  # nodes, features, classes, undirected edges, seed
SEED = 5  # (the float64 model is tie-free under it at both widths: asserted below)


@pytest.fixture(scope="module")
def ds(pgcn):
    return pgcn.Dataset.synthetic(*SYN)


@pytest.mark.parametrize("width", [16, 20])
@pytest.mark.parametrize("residual", [False, True])
def test_numeric_parity(ds, pgcn, width, residual):
    """3 layers, hidden (width, width), dropout 0, against float64 at the LayerNorm engine test's
    tolerances: logits, hidden activations, weight and scale / shift gradients after one
    train_epoch, then train and val loss over 3 epochs at 1e-4 relative.  The float64 run has no
    hidden |Y| < 1e-5 (asserted): no ReLU argument sits where fp32 could flip its mask."""
    hidden, L = (width, width), 3
    p = pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.0,) * L, residual=residual,
                         batch_norm=True, seed=SEED)
    g = pgcn.GCN(p, ds)
    assert g.query("batch_norm_layers") == L - 1 and g.query("norm_layers") == 0
    assert g.num_vars() == 3 * L + 2 and g.query("residual_layers") == (1 if residual else 0)
    m = ref.Model(ds, hidden, [g.get_var(_w(l)) for l in range(L)], g.query("reassociated") == 1,
                  residual)
    tl, want_tl = g.train_epoch()[0], m.forward(1)
    closest = min(float(np.abs(y).min()) for y in m.Y)
    print(f"width {width} residual {residual}: min |Y| {closest:.3g}")
    assert closest >= 1e-5
    m.backward()
    n = ds.num_nodes
    np.testing.assert_allclose(g.get_var(_var2(L - 1)).reshape(n, -1), m.train_logits(),
                               rtol=1e-4, atol=1e-6, err_msg="logits")
    for l in range(L - 1):
        np.testing.assert_allclose(g.get_var(_var2(l)).reshape(n, -1), m.H[l], rtol=1e-4,
                                   atol=1e-6, err_msg=f"var2 of layer {l}")
    for l in range(L):
        np.testing.assert_allclose(g.get_var(_w(l), 1).reshape(m.dW[l].shape), m.dW[l],
                                   rtol=1e-4, atol=1e-7, err_msg=f"W{l} grad")
    np.testing.assert_allclose(g.get_var(_norm(L), 1), m.norm_grad(), rtol=1e-4, atol=1e-7,
                               err_msg="gamma / beta grad")
    for e in range(3):
        if e:
            tl, want_tl = g.train_epoch()[0], m.forward(1)
            m.backward()
        m.step()
        vl, want_vl = g.eval(2)[0], m.forward(2)
        print(f"epoch {e + 1}: train {tl:.9g} / {want_tl:.9g}  val {vl:.9g} / {want_vl:.9g}")
        assert abs(tl - want_tl) <= 1e-4 * abs(want_tl), (e, tl, want_tl)
        assert abs(vl - want_vl) <= 1e-4 * abs(want_vl), (e, vl, want_vl)
    g.close()


def _run(pgcn, ds, epochs=2, fuse=None, hidden=(16, 16, 16), **kw):
    """(epoch lines, scale / shift tensor, fused_norm_tails) of a dropout-0.5 BatchNorm engine."""
    L = len(hidden) + 1
    kw.setdefault("batch_norm", True)
    with helpers.knobs(pgcn, **({} if fuse is None else dict(fuse_epilogue=fuse))):
        g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * L, **kw), ds)
        lines = _lines(g, epochs)
        out = (lines, g.get_var(_norm(L)), g.query("fused_norm_tails"),
               [g.get_var(_w(l)) for l in range(L)])
        g.close()
    return out


def test_fused_tail_bit_identical(ds, pgcn):
    """fuse_epilogue 15 (the ReLU, the add and the Dropout inside the apply launch) against 0
    (modules of their own): epoch lines, weights and the scale / shift tensor over two epochs with
    dropout 0.5 and residual, bit for bit; every hidden layer's tail is fused."""
    on, off = (_run(pgcn, ds, fuse=f, residual=True) for f in (15, 0))
    assert on[2] == 3 and off[2] == 0 and np.isfinite(on[0]).all()
    np.testing.assert_array_equal(on[0], off[0])
    for a, b in zip([on[1]] + on[3], [off[1]] + off[3]):
        np.testing.assert_array_equal(a, b)


def test_off_is_off(ds, pgcn, tmp_path):
    """batch_norm = 0 equals an engine whose params never mention it: lines, weights and
    checkpoint bytes (version 1, flags 0); with it the weights start as the plain engine's."""
    blobs = []
    for i, kw in enumerate((dict(), dict(batch_norm=False))):
        L = 4
        g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=(16, 16, 16), dropouts=(0.5,) * L, **kw), ds)
        assert g.query("batch_norm_layers") == 0 and g.num_vars() == 3 * L + 1
        w0 = [g.get_var(_w(l)) for l in range(L)]
        lines, path = _lines(g, 2), str(tmp_path / f"off{i}.pgcnck")
        g.save(path)
        assert pgcn.checkpoint_info(path)["version"] == 1 and pgcn.checkpoint_flags(path) == 0
        assert not pgcn.checkpoint_batch_norm(path)
        blobs.append((lines, w0, open(path, "rb").read()))
        g.close()
    np.testing.assert_array_equal(blobs[0][0], blobs[1][0])
    assert blobs[0][2] == blobs[1][2]
    g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=(16, 16, 16), dropouts=(0.5,) * 4,
                                  batch_norm=True), ds)
    for a, b in zip(blobs[0][1], [g.get_var(_w(l)) for l in range(4)]):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(g.get_var(_norm(4)),
                                  np.tile(np.repeat(np.float32([1.0, 0.0]), 16), 3))
    g.close()


def test_refusals(ds, pgcn):
    """batch_norm with layer_norm, and batch_norm on more than one rank: PGCN_E_INVALID."""
    p = pgcn.make_params(ds, batch_norm=True)
    group = pgcn.LoopbackGroup(2)
    makers = {
        "layer_norm": lambda: pgcn.GCN(pgcn.make_params(ds, batch_norm=True, layer_norm=True), ds),
        "loopback": lambda: pgcn.GCN(p, ds, rank=0, loopback=group),
        "solo": lambda: pgcn.GCN(p, ds, rank=0, world=2, solo=True),
    }
    for name, make in makers.items():
        with pytest.raises(pgcn.PgcnError) as e:
            make()
        assert e.value.status == pgcn.PGCN_E_INVALID, name


def test_checkpoint_resume(ds, pgcn, tmp_path):
    """Save at epoch 2, resume to 4: bit for bit the straight run.  The file is a BatchNorm
    engine's (version 11, bit 7 and not bit 1); a LayerNorm engine's full load refuses it, its
    weights-only load takes it."""
    hidden, L = (16, 16), 3

    def make(**kw):
        return pgcn.GCN(pgcn.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * L, **kw), ds)
    path = str(tmp_path / "bn.pgcnck")
    g = make(batch_norm=True)
    first = _lines(g, 2)
    g.save(path)
    rest, end = _lines(g, 2), g.get_var(_norm(L))
    g.close()
    assert pgcn.checkpoint_batch_norm(path) and pgcn.checkpoint_info(path)["version"] == 11
    assert pgcn.checkpoint_flags(path) == pgcn.CKPT_BATCHNORM
    g = make(batch_norm=True)
    g.load(path)
    np.testing.assert_array_equal(_lines(g, 2), rest)
    np.testing.assert_array_equal(g.get_var(_norm(L)), end)
    assert np.isfinite(first).all()
    g.close()
    for kw in (dict(layer_norm=True), dict()):
        g = make(**kw)
        with pytest.raises(pgcn.PgcnError) as e:
            g.load(path)
        assert e.value.status == pgcn.PGCN_E_INVALID
        g.load(path, weights_only=True)
        g.close()


COMPOSITIONS = {"attention": dict(attention=True, attention_heads=2),
                "max": dict(aggregator="max"),
                "readout": dict(readout="mean"),
                "link": dict(link_decoder="dot")}


@pytest.mark.parametrize("case", sorted(COMPOSITIONS))
def test_composition(pgcn, case):
    """batch_norm with attention (2 heads), the max aggregator, a mean readout and the dot link
    decoder: two epochs run with finite losses, every hidden layer normalised and its tail fused,
    and a second identical run gives the same bits (no float64 model here: the existing *_ref
    files each carry a model of their own that a BatchNorm cannot be slipped into cheaply)."""
    d = pgcn.Dataset.synthetic(*SYN)
    rng = np.random.default_rng(11)
    n = d.num_nodes
    if case == "readout":
        gp = np.arange(0, n + 1, 20)
        d.set_graphs(gp, rng.integers(0, 3, len(gp) - 1), rng.integers(1, 4, len(gp) - 1), 3)
    if case == "link":
        e = 400
        d.set_links(rng.integers(0, n, e), rng.integers(0, n, e), rng.integers(0, 2, e),
                    rng.integers(1, 4, e), 16)
    runs = [_run(pgcn, d, hidden=(16, 16), **COMPOSITIONS[case]) for _ in range(2)]
    assert np.isfinite(runs[0][0]).all() and runs[0][2] == 2
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][3], runs[1][3]):
        np.testing.assert_array_equal(a, b)
