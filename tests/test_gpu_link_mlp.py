"""The engine with the Hadamard-MLP link decoder (pgcn_params.link_hidden = 8) on
tests/test_gpu_link.py's data set: 500 nodes, embedding width 8, hidden (8,), 1,200 pairs.

The decoder is checked against tests/link_mlp_ref.py applied to the engine's own embedding and
decoder tensor (get_var), within the kernel test's per-pair bound (u = 2^-24; derivation in
tests/test_gpu_link_mlp_kernels.py):
    |err_e| <= (h + 2) u sum_u |w2_u hid_u| + (d + 3) u sum_u |w2_u| (|b1_u| + sum_i |z_i W1_iu|)
               + u |b2|,
and the first training loss against the float64 BCE of those scores (plus the engine's L2 term of
the first layer's weight) within the project's 1e-4 relative parity.
"""
import numpy as np
import pytest

import link_mlp_ref as mr
from test_gpu_link import EMBED, HIDDEN, _var2, _w, make_dataset

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
H = 8
WD = 5e-4


@pytest.fixture(scope="module")
def data(pgcn):
    return make_dataset(pgcn)


def make(pgcn, ds, p=(0.5, 0.5), hidden=H):
    return pgcn.GCN(pgcn.make_params(ds, hidden_dims=HIDDEN, dropouts=p, link_decoder="dot",
                                     link_hidden=hidden), ds)


def lines(g, k):
    return np.array([g.train_epoch() + g.eval(2) for _ in range(k)], np.float32)


def test_decoder_first_loss_and_training(data, pgcn):
    ds = data
    g = make(pgcn, ds, p=(0.0, 0.0))
    dot = pgcn.GCN(pgcn.make_params(ds, hidden_dims=HIDDEN, dropouts=(0.0, 0.0),
                                    link_decoder="dot"), ds)
    nv = g.num_vars()
    assert g.query("link_hidden") == H and dot.query("link_hidden") == 0
    assert nv == dot.num_vars() + 1
    for l in range(2):  # a seed's encoder weights are the dot engine's
        np.testing.assert_array_equal(g.get_var(_w(l)), dot.get_var(_w(l)))
    P0 = g.get_var(nv - 2).reshape(EMBED + 3, H)
    assert (P0[EMBED] == 0).all() and (P0[EMBED + 2] == 0).all() and np.abs(P0[:EMBED]).max() > 0
    assert np.abs(P0[:EMBED]).max() <= np.sqrt(6.0 / (EMBED + H))
    assert 0 < np.abs(P0[EMBED + 1]).max() <= np.sqrt(6.0 / (H + 1))

    # 1. the scores are the float64 decoder of the engine's embedding and tensor
    scores = g.predict_links()
    emb = g.get_var(_var2(1)).reshape(ds.num_nodes, EMBED)
    src, dst = np.asarray(ds.pair_src), np.asarray(ds.pair_dst)
    ref, A, B, _ = mr.forward(src, dst, emb, P0, EMBED, H)
    bound = (H + 2) * EPS * A + (EMBED + 3) * EPS * B + EPS * abs(float(P0[EMBED + 2, 0]))
    err = np.abs(scores.astype(np.float64) - ref)
    assert (err <= bound).all(), float((err - bound).max())
    np.testing.assert_array_equal(g.score_pairs(src[:100], dst[:100]), scores[:100])
    tp, fp, fn = g.link_counts(3)
    lab, sp = np.asarray(ds.pair_label), np.asarray(ds.pair_split)
    test = (sp == 3) & (lab >= 0)
    assert tp + fn == int((lab[test] == 1).sum())

    # 2. the first loss (no dropout: the training forward is the forward above)
    train = (sp == 1) & (lab >= 0)
    x, y = ref[train], (lab[train] == 1).astype(np.float64)
    W0 = g.get_var(_w(0)).astype(np.float64)
    want = float((np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x)))).mean()) + \
        WD * float((W0 ** 2).sum()) / 2.0
    first = g.train_epoch()[0]
    assert abs(first - want) <= 1e-4 * abs(want), (first, want)

    # 3. training moves the decoder and lowers the loss
    for _ in range(28):
        g.train_epoch()
    last = g.train_epoch()[0]
    P30 = g.get_var(nv - 2).reshape(EMBED + 3, H)
    assert last < first and np.abs(P30 - P0).max() > 1e-3 and np.isfinite(P30).all()
    assert (P30[EMBED + 2, 1:] == 0).all()
    g.close()
    dot.close()


def test_save_load_and_warm_start(data, pgcn, tmp_path):
    ds = data
    straight = make(pgcn, ds)
    want = lines(straight, 20)
    a = make(pgcn, ds)
    np.testing.assert_array_equal(lines(a, 10), want[:10])
    path = str(tmp_path / "mlp.pgcnck")
    a.save(path)
    assert pgcn.checkpoint_info(path)["version"] == 9
    assert pgcn.checkpoint_link_hidden(path) == H
    assert pgcn.checkpoint_links(path) == (1, ds.num_pairs)
    b = make(pgcn, ds)
    b.load(path)
    np.testing.assert_array_equal(lines(b, 10), want[10:])
    nv = b.num_vars()
    np.testing.assert_array_equal(b.get_var(nv - 2), straight.get_var(nv - 2))
    # a version-8 (dot) checkpoint of equal dims: refused on resume, a warm start weights only
    dot = pgcn.GCN(pgcn.make_params(ds, hidden_dims=HIDDEN, dropouts=(0.5, 0.5),
                                    link_decoder="dot"), ds)
    dot.train_epoch()
    v8 = str(tmp_path / "dot.pgcnck")
    dot.save(v8)
    assert pgcn.checkpoint_info(v8)["version"] == 8 and pgcn.checkpoint_link_hidden(v8) == 0
    c = make(pgcn, ds)
    P0 = c.get_var(nv - 2)
    for eng, file in ((c, v8), (dot, path), (make(pgcn, ds, hidden=4), path)):
        with pytest.raises(pgcn.PgcnError) as e:
            eng.load(file)
        assert e.value.status == pgcn.PGCN_E_INVALID
    c.load(v8, weights_only=True)
    for l in range(2):
        np.testing.assert_array_equal(c.get_var(_w(l)), dot.get_var(_w(l)))
    np.testing.assert_array_equal(c.get_var(nv - 2), P0)  # the decoder tensor keeps its init
    assert np.isfinite(lines(c, 1)).all()
    for x in (straight, a, b, c, dot):
        x.close()


def test_refusals(data, pgcn):
    ds = data
    g = make(pgcn, ds)
    for call in (lambda: g.link_ranks(3), lambda: g.top_links([0, 1], k=5)):
        with pytest.raises(pgcn.PgcnError) as e:
            call()
        assert e.value.status == pgcn.PGCN_E_INVALID
    g.close()
    for kw in (dict(link_decoder=1, link_hidden=-1), dict(link_decoder=1, link_hidden=129),
               dict(link_decoder=0, link_hidden=8)):
        q = pgcn.make_params(ds, hidden_dims=HIDDEN)
        for k, v in kw.items():
            setattr(q, k, v)
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.GCN(q, ds)
        assert e.value.status == pgcn.PGCN_E_INVALID, kw
