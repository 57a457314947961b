"""The engine with per-epoch negative sampling (pgcn_params.neg_ratio) on the small link data set
of tests/test_gpu_link.py (its fixture, copied): the drawn pairs against tests/neg_ref.py, the loss
against a float64 BCE over the engine's own embedding, resume, warm start and refusals."""
import numpy as np
import pytest

import neg_ref

pytestmark = pytest.mark.gpu

HIDDEN, EMBED, R = (8,), 8, 2
N, F, EDGES, DS_SEED = 500, 12, 1500, 31
SEED = 3


def pair_arrays(pgcn, ds):
    """(src, dst, label, split) of the 1,200 pairs."""
    rng = np.random.default_rng(17)
    rows = np.repeat(np.arange(ds.num_nodes), np.diff(ds.graph_indptr))
    cols = np.asarray(ds.graph_indices)
    up = np.nonzero(rows < cols)[0]
    pick = rng.choice(up, 600, replace=False)
    ps, pd = rows[pick].astype(np.int32), cols[pick].astype(np.int32)
    ns, nd = pgcn.sample_negative_pairs(ds, ps, 1, 5)
    order = rng.permutation(1200)
    src = np.concatenate([ps, ns])[order].astype(np.int32)
    dst = np.concatenate([pd, nd])[order].astype(np.int32)
    label = np.concatenate([np.ones(600), np.zeros(600)])[order].astype(np.int32)
    split = (1 + np.arange(1200) % 3).astype(np.int32)
    label[0] = -1          # an unlabelled training pair
    dst[3] = src[3]        # a self pair
    src[9], dst[9], label[9] = src[6], dst[6], label[6]  # one pair listed twice
    return src, dst, label, split


@pytest.fixture(scope="module")
def ds(pgcn):
    d = pgcn.Dataset.synthetic(N, F, 3, EDGES, DS_SEED)
    d.set_links(*pair_arrays(pgcn, d), EMBED)
    return d


def engine(pgcn, ds, **kw):
    kw.setdefault("seed", SEED)
    return pgcn.GCN(pgcn.make_params(ds, hidden_dims=HIDDEN, link_decoder="dot", **kw), ds)


def epochs(g, n):
    return [g.train_epoch() + g.eval(2) for _ in range(n)]


def exclusion(ds):
    """Per node: itself, its adjacency row, the dst of its label-1 pairs of any split."""
    src, dst, lab = (np.asarray(a) for a in (ds.pair_src, ds.pair_dst, ds.pair_label))
    ptr, idx = np.asarray(ds.graph_indptr), np.asarray(ds.graph_indices)
    rows = [sorted({s} | set(idx[ptr[s]:ptr[s + 1]].tolist()) |
                   set(dst[(src == s) & (lab == 1)].tolist())) for s in range(N)]
    xp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return xp, np.concatenate(rows).astype(np.int32), rows


def test_off_is_the_engine_without_the_field(pgcn, ds):
    a, b = engine(pgcn, ds, neg_ratio=0), engine(pgcn, ds)
    assert a.query("neg_pairs") == 0 and epochs(a, 3) == epochs(b, 3)
    a.close()
    b.close()


def test_drawn_pairs_and_loss(pgcn, ds):
    """Epochs 0 and 1: the scores of the drawn rows are the dot products over neg_ref's pairs of
    that round, and the training loss is the float64 BCE over the training pairs and those."""
    src, dst, lab, sp = (np.asarray(a) for a in (ds.pair_src, ds.pair_dst, ds.pair_label,
                                                  ds.pair_split))
    xp, xi, rows = exclusion(ds)
    anchors = np.repeat(src[(sp == 1) & (lab == 1)], R)
    E, train = len(src), (sp == 1) & (lab >= 0)
    g = engine(pgcn, ds, neg_ratio=R, dropouts=(0.0, 0.0), weight_decay=0.0)
    assert g.query("neg_pairs") == len(anchors) and g.query("num_pairs") == E
    drawn = []
    for rnd in range(2):
        loss = g.train_epoch()[0]
        nd = neg_ref.draw(anchors, N, xp, xi, SEED, rnd)
        assert all(d not in rows[s] for s, d in zip(anchors, nd))  # no edge, positive or self pair
        H = g.get_var(g.num_vars() - 2).astype(np.float64).reshape(N, -1)[:, :EMBED]
        x = np.concatenate([(H[src] * H[dst]).sum(1)[train], (H[anchors] * H[nd]).sum(1)])
        y = np.concatenate([lab[train], np.zeros(len(nd))])
        got = g.get_var(g.num_vars() - 1).reshape(E + len(nd), -1)[E:, 0]
        np.testing.assert_allclose(got, x[train.sum():], rtol=1e-4, atol=1e-6)
        want = np.mean(np.maximum(x, 0) - x * y + np.log1p(np.exp(-np.abs(x))))
        assert abs(loss - want) <= 1e-4 * want
        g.eval(2)
        drawn.append(nd)
    assert (drawn[0] != drawn[1]).any()
    g.close()


@pytest.mark.parametrize("hidden", [0, 8])
def test_resume_is_bit_exact(pgcn, ds, hidden, tmp_path):
    path = str(tmp_path / "neg.pgcnck")
    kw = dict(neg_ratio=R, link_hidden=hidden)
    straight, first = engine(pgcn, ds, **kw), engine(pgcn, ds, **kw)
    want = epochs(straight, 10)
    assert epochs(first, 5) == want[:5]
    first.save(path)
    assert pgcn.checkpoint_neg_ratio(path) == R and pgcn.checkpoint_info(path)["version"] == 10
    assert pgcn.checkpoint_link_hidden(path) == hidden
    second = engine(pgcn, ds, **kw)
    second.load(path)
    assert epochs(second, 5) == want[5:]
    for v in range(straight.num_vars()):
        assert straight.get_var(v).tobytes() == second.get_var(v).tobytes()
    for g in (straight, first, second):
        g.close()


def test_warm_start_and_ratio_mismatch(pgcn, ds, tmp_path):
    fixed, neg = engine(pgcn, ds), engine(pgcn, ds, neg_ratio=R)
    epochs(fixed, 2)
    old, new = str(tmp_path / "v8.pgcnck"), str(tmp_path / "v10.pgcnck")
    fixed.save(old)
    assert pgcn.checkpoint_info(old)["version"] == 8 and pgcn.checkpoint_neg_ratio(old) == 0
    neg.load(old, weights_only=True)
    assert neg.get_var(2).tobytes() == fixed.get_var(2).tobytes()
    epochs(neg, 1)
    neg.save(new)
    other = engine(pgcn, ds, neg_ratio=1)
    for g, path in ((neg, old), (other, new), (fixed, new)):
        with pytest.raises(pgcn.PgcnError) as e:
            g.load(path)
        assert e.value.status == pgcn.PGCN_E_INVALID
    for g in (fixed, neg, other):
        g.close()


def test_training_does_not_raise_the_validation_loss(pgcn, ds):
    g = engine(pgcn, ds, neg_ratio=R)
    lines = epochs(g, 30)
    assert lines[-1][2] <= lines[0][2]
    g.close()
