"""Per-node prediction: the pgcn_predict_rows / pgcn_confusion kernels against numpy, the
engine's predict() / confusion() against the reference's own logits (tests/golden), and the
guarantee that predicting changes nothing in a training run.

Device memory comes from torch (plumbing only); every compute call goes through libpgcn.so.
"""
import ctypes

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

FLT_MIN = float(np.finfo(np.float32).tiny)
# the project's logits tolerance: rows whose two largest reference logits are closer than this
# (relative to max(1, max|z|)) may be classed either way
BAND = 1e-4


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def softmax64(z):
    z = np.asarray(z, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def _logits(n, c, rng):
    """N(0, 3^2) rows; the last rows (where n allows) are the three special kinds: all-equal
    values, an exact tie of the maximum at two indices, one entry 1e30 above the rest."""
    z = (rng.standard_normal((n, c)) * 3).astype(np.float32)
    want = np.full(n, -1, np.int64)  # forced class of a special row
    if n >= 4:
        z[n - 1, :] = np.float32(rng.standard_normal() * 3)
        want[n - 1] = 0
        if c >= 2:
            a, b = sorted(rng.choice(c, 2, replace=False))
            z[n - 2, a] = z[n - 2, b] = np.float32(z[n - 2].max() + 1.5)
            want[n - 2] = a
        j = int(rng.integers(c))
        z[n - 3, j] += np.float32(1e30)
        want[n - 3] = j
    return z, want


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 7, 41, 48, 49, 113, 128])
def test_predict_rows_matches_float64_softmax(pgcn, c):
    """Classes exact (lowest index of the maximum); probabilities within rtol (c + 3) 2^-24 and
    atol FLT_MIN of the float64 softmax (device expf at 1 ulp, the c - 1 adds of the sum, one
    division); NaN in every padding column; logits unchanged; each output alone."""
    R = pgcn.PREDICT_ROWS
    rng = np.random.default_rng(1000 + c)
    cp = (c + 3) // 4 * 4
    rtol = (c + 3) * 2.0 ** -24
    for n in (1, R - 1, R, R + 1, 3 * R + 5):
        z, forced = _logits(n, c, rng)
        p64 = softmax64(z)
        arg = z.argmax(axis=1)  # numpy: the first maximum
        assert (arg[forced >= 0] == forced[forced >= 0]).all()
        for ld in (cp, cp + 8):
            host = np.full((n, ld), np.nan, np.float32)
            host[:, :c] = z
            dz = torch.from_numpy(host).to("cuda")
            cls = torch.full((n,), -7, dtype=torch.int32, device="cuda")
            conf = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
            ldp = cp + 4
            pr = torch.full((n, ldp), -2.0, dtype=torch.float32, device="cuda")
            st = pgcn.lib.pgcn_predict_rows(vp(dz), ld, n, c, vp(cls), vp(conf), vp(pr), ldp,
                                            stream())
            assert st == 0
            torch.cuda.synchronize()
            what = f"c {c} n {n} ld {ld}"
            got_cls, got_conf, got_pr = cls.cpu().numpy(), conf.cpu().numpy(), pr.cpu().numpy()
            np.testing.assert_array_equal(got_cls, arg, err_msg=what)
            p = got_pr[:, :c]
            assert np.isfinite(p).all(), what
            err = np.abs(p.astype(np.float64) - p64)
            worst = float((np.maximum(err - FLT_MIN, 0) / np.maximum(p64, 1e-300)).max())
            print(f"{what}: worst relative error {worst / 2.0 ** -24:.2f} x 2^-24 "
                  f"(bound {c + 3})")
            assert (err <= rtol * p64 + FLT_MIN).all(), what
            np.testing.assert_array_equal(got_conf, p[np.arange(n), arg], err_msg=what)
            assert (got_pr[:, c:cp] == 0).all() and (got_pr[:, cp:] == -2.0).all(), what
            if n >= 4:  # 1e30 above the rest: exactly one and zeros; all-equal: 1 / c
                j = forced[n - 3]
                assert p[n - 3, j] == 1.0 and np.delete(p[n - 3], j).max(initial=0.0) == 0.0
                assert abs(float(p[n - 1, 0]) - 1.0 / c) <= rtol / c
            # logits untouched (padding NaN included)
            np.testing.assert_array_equal(dz.cpu().numpy().view(np.uint32), host.view(np.uint32))
            # each output alone, the others NULL: the same bits
            for keep in range(3):
                c2 = torch.full_like(cls, -7) if keep == 0 else None
                f2 = torch.full_like(conf, -1.0) if keep == 1 else None
                p2 = torch.full_like(pr, -2.0) if keep == 2 else None
                assert pgcn.lib.pgcn_predict_rows(vp(dz), ld, n, c, vp(c2), vp(f2), vp(p2), ldp,
                                                  stream()) == 0
                torch.cuda.synchronize()
                for mine, full in ((c2, cls), (f2, conf), (p2, pr)):
                    if mine is not None:
                        assert torch.equal(mine, full), (what, keep)


def _confusion(pgcn, cls, truth, c, counts=None):
    n = len(cls)
    dc = torch.from_numpy(np.ascontiguousarray(cls, np.int32)).to("cuda")
    dt = torch.from_numpy(np.ascontiguousarray(truth, np.int32)).to("cuda")
    if counts is None:  # garbage: the call zeroes it
        counts = torch.full((c * c,), 12345, dtype=torch.int32, device="cuda")
    assert pgcn.lib.pgcn_confusion(vp(dc), vp(dt), n, c, vp(counts), stream()) == 0
    torch.cuda.synchronize()
    return counts, counts.cpu().numpy().view(np.uint32).reshape(c, c).astype(np.int64)


def _confusion_ref(cls, truth, c):
    ref = np.zeros((c, c), np.int64)
    keep = np.asarray(truth) >= 0
    np.add.at(ref, (np.asarray(truth)[keep], np.asarray(cls)[keep]), 1)
    return ref


@pytest.mark.parametrize("case", ["n1", "c1", "c128", "unlabelled", "one_cell", "random"])
def test_confusion_matches_add_at(pgcn, case):
    rng = np.random.default_rng(7)
    if case == "n1":
        c, cls, truth = 5, np.array([3]), np.array([1])
    elif case == "c1":
        c, cls, truth = 1, np.zeros(300, np.int32), rng.integers(-1, 1, 300)
    elif case == "c128":
        c = 128
        cls, truth = rng.integers(0, c, 30000), rng.integers(-1, c, 30000)
    elif case == "unlabelled":
        c, cls, truth = 7, rng.integers(0, 7, 5000), np.full(5000, -1)
    elif case == "one_cell":
        c, cls, truth = 41, np.full(100000, 17), np.full(100000, 40)
    else:
        c, n = 41, 50000
        cls = rng.integers(0, c, n)
        truth = np.where(rng.random(n) < 0.4, rng.integers(0, c, n), -1)
    buf, got = _confusion(pgcn, cls, truth, c)
    ref = _confusion_ref(cls, truth, c)
    np.testing.assert_array_equal(got, ref)
    if case == "unlabelled":
        assert got.sum() == 0
    if case == "one_cell":
        assert got[40, 17] == 100000 and got.sum() == 100000
    if case == "random":  # a second call on the same buffer does not accumulate
        _, again = _confusion(pgcn, cls, truth, c, counts=buf)
        np.testing.assert_array_equal(again, ref)


# --------------------------------------------------------------------------- engine
def _set_golden_weights(g, gold):
    g.set_var(2, gold["final_W1"])
    g.set_var(g.num_vars() - 2, gold["final_W2"])


def _band(z):
    """Rows whose two largest logits are within BAND * max(1, max|z|)."""
    top2 = np.sort(z, axis=1)[:, -2:]
    scale = np.maximum(1.0, np.abs(z).max(axis=1))
    return (top2[:, 1] - top2[:, 0]) <= BAND * scale


def _golden_logits(gold, ds):
    return np.asarray(gold["final_test_logits"], np.float64).reshape(ds.num_nodes, ds.output_dim)


@pytest.mark.parametrize("split_rows", [0, 1])
@pytest.mark.parametrize("name", ["cora", "citeseer"])
def test_engine_predict_matches_reference_logits(pgcn, loaded, name, split_rows):
    """A fresh engine given the reference's trained weights predicts what the reference's own
    final logits say (tests/golden): classes equal outside the near-tie band, probabilities
    within 2e-4 max(1, max|z|) of their float64 softmax, eval(3) at the project's 1e-4, and the
    confusion matrix equal to the one built on the host from predict() and the labels.  With
    split_rows on predict still covers every row."""
    ds, gold = loaded[name], helpers.golden(name)
    z = _golden_logits(gold, ds)
    band = _band(z)
    assert band.sum() < 0.005 * ds.num_nodes  # (0 rows on cora and on citeseer)
    with helpers.knobs(pgcn, split_rows=split_rows):
        g = pgcn.GCN(pgcn.make_params(ds), ds)
        _set_golden_weights(g, gold)
        cls, conf, probs = g.predict(probs=True)
        te = g.eval(3)
        cm = g.confusion(3)
        cls2, conf2 = g.predict()
        g.close()
    assert cls.shape == (ds.num_nodes,) and probs.shape == (ds.num_nodes, ds.output_dim)
    np.testing.assert_array_equal(cls[~band], z.argmax(axis=1)[~band])
    atol = 2 * BAND * max(1.0, float(np.abs(z).max()))
    assert np.abs(probs.astype(np.float64) - softmax64(z)).max() <= atol
    np.testing.assert_array_equal(conf, probs[np.arange(ds.num_nodes), cls])
    np.testing.assert_array_equal(cls2, cls)
    np.testing.assert_array_equal(conf2, conf)
    want = gold["test_scalars"]
    assert abs(te[0] - want[0]) <= 1e-4 * abs(want[0])
    assert abs(te[1] - want[1]) <= 1e-4 * abs(want[1])
    lab, sp = np.asarray(ds.label), np.asarray(ds.split)
    truth = np.where((sp == 3) & (lab >= 0), lab, -1)
    np.testing.assert_array_equal(cm, _confusion_ref(cls, truth, ds.output_dim))
    assert np.float32(np.trace(cm)) / np.float32(cm.sum()) == np.float32(te[1])


@pytest.fixture(scope="module")
def lds_ds(pgcn):
    # dense X, the LDS ring GraphSum and eval_ax
    return pgcn.Dataset.synthetic(80000, 40, 8, 2000000, 11)


def _weights(g):
    return [g.get_var(i) for i in (2, g.num_vars() - 2)]


@pytest.mark.parametrize("which", ["cora", "lds", "lds_graph"])
def test_predict_changes_nothing(pgcn, loaded, lds_ds, which):
    """3 epochs, predict, confusion(2), 3 epochs equals 6 epochs bit for bit: results, weights,
    epoch and step counts (lds_graph: the epochs replay a captured graph around the eager
    predict pass)."""
    ds = loaded["cora"] if which == "cora" else lds_ds
    with helpers.knobs(pgcn, epoch_graph=1 if which == "lds_graph" else 0):
        _predict_changes_nothing(pgcn, ds, which)


def _predict_changes_nothing(pgcn, ds, which):
    a = pgcn.GCN(pgcn.make_params(ds), ds)
    for _ in range(3):
        a.epoch_async()
    a.predict(probs=True)
    a.confusion(2)
    for _ in range(3):
        a.epoch_async()
    ra, wa = a.results(6), _weights(a)
    qa = (a.query("epochs"), a.query("adam_steps"), a.query("graphsum_lds"))
    a.close()
    b = pgcn.GCN(pgcn.make_params(ds), ds)
    for _ in range(6):
        b.epoch_async()
    rb, wb = b.results(6), _weights(b)
    qb = (b.query("epochs"), b.query("adam_steps"), b.query("graphsum_lds"))
    b.close()
    assert qa == qb and qa[:2] == (6, 6)
    if which != "cora":
        assert qa[2] == 1
    assert ra.shape == (6, 4)
    np.testing.assert_array_equal(ra.view(np.uint32), rb.view(np.uint32))
    for x, y in zip(wa, wb):
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_loopback_predict_matches_one_gpu(pgcn, loaded):
    """W = 2 in-process ranks on cora: the ranks' predictions, concatenated by node_range, equal
    the one-GPU engine's outside the near-tie band; the summed confusion matrices equal the
    one-GPU matrix up to the rows in the band."""
    ds, gold = loaded["cora"], helpers.golden("cora")
    g = pgcn.GCN(pgcn.make_params(ds), ds)
    _set_golden_weights(g, gold)
    one_cls, _ = g.predict()
    one_cm = g.confusion(3)
    g.close()
    group = pgcn.LoopbackGroup(2)

    def rank_fn(r):
        e = pgcn.GCN(pgcn.make_params(ds), ds, device=0, rank=r, loopback=group)
        _set_golden_weights(e, gold)
        cls, conf = e.predict()
        cm = e.confusion(3)
        rng = e.node_range()
        e.close()
        return rng, cls, conf, cm
    res = pgcn.run_ranks(2, rank_fn)
    assert res[0][0][0] == 0 and res[0][0][1] == res[1][0][0] and res[1][0][1] == ds.num_nodes
    cls = np.concatenate([r[1] for r in res])
    band = _band(_golden_logits(gold, ds))
    np.testing.assert_array_equal(cls[~band], one_cls[~band])
    cm = res[0][3] + res[1][3]
    assert cm.sum() == one_cm.sum()
    assert np.abs(cm - one_cm).sum() <= 2 * int(band.sum())
