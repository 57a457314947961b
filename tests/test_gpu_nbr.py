"""pgcn_params.fanout on the engine: SAGE layers that train on sampled neighbours and evaluate on
the whole neighbourhood, on a synthetic n = 300 graph whose longest row fits fanout 64.

Parity (a) is the project's stated tolerance, 1e-4 relative: per loss value, and per logit
relative to the largest logit magnitude (a logit near zero has no relative scale of its own)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HIDDEN, DROP = (16,), (0.5, 0.5)
W, LOGITS = (2, 5), 6  # the two layers' weight variables; the output layer's var2


@pytest.fixture(scope="module")
def ds(pgcn):
    d = pgcn.Dataset.synthetic(300, 24, 5, 900, 22)
    assert 3 < np.diff(d.graph_indptr).max() <= 64
    return d


def make(pgcn, ds, agg, fanout, seed=0):
    return pgcn.GCN(pgcn.make_params(ds, hidden_dims=HIDDEN, dropouts=DROP, aggregator=agg,
                                     root_weight=True, seed=seed, fanout=fanout), ds)


def lines(g, n):
    return np.array([g.train_epoch() + g.eval(2) for _ in range(n)], np.float32)


@pytest.mark.parametrize("agg", ["mean", "max"])
def test_fanout_covering_every_row_is_the_full_engine(pgcn, ds, agg):
    full, samp = make(pgcn, ds, agg, 0), make(pgcn, ds, agg, 64)
    a, b = lines(full, 3), lines(samp, 3)
    np.testing.assert_allclose(b[:, [0, 2]], a[:, [0, 2]], rtol=1e-4, atol=0)
    za, zb = full.get_var(LOGITS), samp.get_var(LOGITS)
    assert np.abs(zb - za).max() <= 1e-4 * np.abs(za).max()
    full.close(), samp.close()


@pytest.mark.parametrize("agg", ["mean", "max"])
def test_eval_runs_the_full_neighbourhood(pgcn, ds, agg):
    full, samp = make(pgcn, ds, agg, 0), make(pgcn, ds, agg, 3)
    lines(samp, 1)
    for w in W:
        full.set_var(w, samp.get_var(w))
    for split in (2, 3):
        assert full.eval(split) == samp.eval(split)
    np.testing.assert_array_equal(full.get_var(LOGITS).view(np.uint32),
                                  samp.get_var(LOGITS).view(np.uint32))
    full.close(), samp.close()


@pytest.mark.parametrize("agg", ["mean", "max"])
def test_resume_redraws_the_straight_run(pgcn, ds, tmp_path, agg):
    straight, a, b, plain = (make(pgcn, ds, agg, f) for f in (3, 3, 3, 0))
    want = lines(straight, 4)
    np.testing.assert_array_equal(lines(a, 2), want[:2])
    lines(plain, 2)
    path, ppath = str(tmp_path / "nbr.pgcnck"), str(tmp_path / "full.pgcnck")
    a.save(path)
    plain.save(ppath)
    assert os.path.getsize(path) == os.path.getsize(ppath)
    assert pgcn.checkpoint_info(path)["version"] == pgcn.checkpoint_info(ppath)["version"]
    b.load(path)
    np.testing.assert_array_equal(lines(b, 2), want[2:])
    for w in W:
        np.testing.assert_array_equal(b.get_var(w), straight.get_var(w))
    [g.close() for g in (straight, a, b, plain)]


@pytest.mark.parametrize("agg", ["mean", "max"])
def test_seeds_and_paths(pgcn, ds, agg):
    a, b, c = (make(pgcn, ds, agg, 3, seed=s) for s in (4, 4, 5))
    full = make(pgcn, ds, agg, 0, seed=4)
    pgcn.reset_path_counts()
    la = lines(a, 2)
    hits = pgcn.path_counts(reset=True)
    assert hits["nbr_draw"] == 4 and hits["nbr_fwd"] == 4 and 2 <= hits["nbr_bwd"] <= 4
    np.testing.assert_array_equal(lines(b, 2), la)
    assert (lines(c, 2)[:, 0] != la[:, 0]).all()
    assert (lines(full, 2)[:, 0] != la[:, 0]).any()  # (the sample changes the training loss)
    assert pgcn.path_counts()["nbr_draw"] == 8  # (b and c drew; the fanout-0 engine did not)
    [g.close() for g in (a, b, c, full)]

