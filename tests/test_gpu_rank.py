"""GCN.link_ranks on a link engine over cora: pairs built the way tests/test_gpu_link.py builds
them (positives drawn from the adjacency, as many sampled negatives, dealt to the splits 1 / 2 / 3
in turn, one unlabelled pair, one self pair, one pair listed twice), three training epochs, then
the test split's ranking counts against numpy.

The comparison is exact: the counts are derived in numpy from the rank scores of every (query,
candidate) pair, computed by pgcn_link_rank_scores (the fmaf chain itself) over the output
embedding read back with get_var, with the query sets of rank_filter.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EMBED = 8
OUT_VAR = 6  # the output embedding of the 2-layer engine (test_gpu_link._var2(1))


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def pair_arrays(pgcn, ds, pos=600):
    rng = np.random.default_rng(17)
    rows = np.repeat(np.arange(ds.num_nodes), np.diff(ds.graph_indptr))
    cols = np.asarray(ds.graph_indices)
    up = np.nonzero(rows < cols)[0]
    pick = rng.choice(up, pos, replace=False)
    ps, pd = rows[pick].astype(np.int32), cols[pick].astype(np.int32)
    ns, nd = pgcn.sample_negative_pairs(ds, ps, 1, 5)
    order = rng.permutation(2 * pos)
    src = np.concatenate([ps, ns])[order].astype(np.int32)
    dst = np.concatenate([pd, nd])[order].astype(np.int32)
    label = np.concatenate([np.ones(pos), np.zeros(pos)])[order].astype(np.int32)
    split = (1 + np.arange(2 * pos) % 3).astype(np.int32)
    label[0] = -1
    dst[3] = src[3]
    src[9], dst[9], label[9] = src[6], dst[6], label[6]
    return src, dst, label, split


@pytest.fixture(scope="module")
def data(pgcn, datasets):
    root, names = datasets
    ds = pgcn.Dataset.load(root, names["cora"])
    ds.set_links(*pair_arrays(pgcn, ds), EMBED)
    return ds


def _engine(pgcn, ds, **kw):
    return pgcn.GCN(pgcn.make_params(ds, hidden_dims=(16,), link_decoder="dot", **kw), ds)


@pytest.fixture(scope="module")
def trained(pgcn, data):
    """The engine after three epochs, and -- computed once -- every (test anchor, node) rank
    score of its eval-mode embedding per side: side -> (anchor, target, S [Q][n])."""
    import torch
    g = _engine(pgcn, data)
    for _ in range(3):
        g.train_epoch()
    n = data.num_nodes
    g.link_ranks(3, "dst", False)  # leaves the eval-mode embedding in the variable
    H = g.get_var(OUT_VAR).reshape(n, EMBED)
    Hd = _dev(H.astype(np.float32))
    scores = {}
    for side in ("dst", "src"):
        a, t, _, _ = pgcn.rank_filter(n, data.graph_indptr, data.graph_indices, data.pair_src,
                                      data.pair_dst, data.pair_label, data.pair_split, 3, side,
                                      False)
        src, dst = _dev(np.repeat(a, n)), _dev(np.tile(np.arange(n, dtype=np.int32), a.size))
        out = _dev(np.zeros(a.size * n, np.float32))
        assert pgcn.lib.pgcn_link_rank_scores(_p(src), _p(dst), a.size * n, _p(Hd), EMBED, EMBED,
                                              _p(out), None) == pgcn.PGCN_OK
        torch.cuda.synchronize()
        scores[side] = (a, t, out.cpu().numpy().reshape(a.size, n))
    yield g, scores
    g.close()


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("side", ["dst", "src"])
def test_link_ranks_equal_numpy_counts(pgcn, data, trained, side, filtered):
    g, scores = trained
    n = data.num_nodes
    a, t, S = scores[side]
    a2, t2, ptr, idx = pgcn.rank_filter(n, data.graph_indptr, data.graph_indices, data.pair_src,
                                        data.pair_dst, data.pair_label, data.pair_split, 3, side,
                                        filtered)
    np.testing.assert_array_equal(a, a2)
    np.testing.assert_array_equal(t, t2)
    lab, sp = np.asarray(data.pair_label), np.asarray(data.pair_split)
    want = (lab == 1) & (sp == 3)
    first, second = (data.pair_src, data.pair_dst) if side == "dst" else \
        (data.pair_dst, data.pair_src)
    np.testing.assert_array_equal(a, np.asarray(first)[want])
    np.testing.assert_array_equal(t, np.asarray(second)[want])
    mask = np.ones((a.size, n), bool)
    mask[np.arange(a.size), t] = False
    for e in range(a.size):
        mask[e, idx[ptr[e]:ptr[e + 1]]] = False
    thr = S[np.arange(a.size), t][:, None]
    greater, equal = g.link_ranks(3, side, filtered)
    assert greater.dtype == np.int64 and greater.shape == equal.shape == (a.size,)
    np.testing.assert_array_equal(greater, ((S > thr) & mask).sum(1))
    np.testing.assert_array_equal(equal, ((S == thr) & mask).sum(1))
    if filtered:
        assert idx.size > a.size  # the anchors and their neighbours are in the lists
        g0, _ = g.link_ranks(3, side, False)
        assert (greater <= g0).all() and (greater < g0).any()
    ranks = pgcn.rank_from_counts(greater, equal)
    assert 0.0 < pgcn.mrr(ranks) <= 1.0 and 0.0 <= pgcn.hits_at(ranks, 10) <= 1.0
    assert pgcn.lib.pgcn_gcn_link_ranks(g._h, 3, 0 if side == "dst" else 1, int(filtered), None,
                                        None) == a.size


def test_training_continues_bit_identically(pgcn, data):
    g1, g2 = (_engine(pgcn, data) for _ in range(2))
    for _ in range(2):
        assert g1.train_epoch() == g2.train_epoch()
        for side in ("dst", "src"):
            g1.link_ranks(3, side, True)
        g1.link_ranks(2, "dst", False)
    assert g1.train_epoch() + g1.eval(2) == g2.train_epoch() + g2.eval(2)
    for v in range(g1.num_vars()):
        np.testing.assert_array_equal(g1.get_var(v), g2.get_var(v))
    g1.close()
    g2.close()


def test_cli_rank_line_and_file(pgcn, datasets, tmp_path):
    """gcn-par NAME link=dot rank=FILE: the line after the run holds the filtered MRR and Hits@K of
    the test split for both sides, the file `src dst greater equal` per test positive pair -- the
    link_ranks() of an engine loaded from the run's checkpoint."""
    import os
    import subprocess

    import helpers
    root, names = datasets
    base = pgcn.Dataset.load(root, names["cora"])
    src, dst, lab, sp = pair_arrays(pgcn, base, 300)
    links = os.path.join(root, "data", names["cora"] + ".links")
    with open(links, "w") as f:
        for e in range(src.size):
            f.write(f"{src[e]} {dst[e]} {lab[e]} {sp[e]}\n")
    exe = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "gcn-par")
    ck, out = str(tmp_path / "ck"), str(tmp_path / "ranks.txt")
    r = subprocess.run([exe, names["cora"], f"root={root}", "link=dot", "embed=8", "epochs=3",
                        f"save={ck}", f"rank={out}"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("rank ")]
    assert len(line) == 1
    tok = line[0].split()[1:]
    assert [t.split("=")[0] for t in tok] == ["side", "queries", "mrr", "hits@10", "hits@50",
                                              "hits@100"] * 2
    base.load_links(links, 8)
    g = pgcn.GCN(pgcn.make_params(base, link_decoder="dot"), base)
    g.load(ck)
    for k, side in enumerate(("dst", "src")):
        greater, equal = g.link_ranks(3, side, True)
        ranks = pgcn.rank_from_counts(greater, equal)
        got = dict(t.split("=") for t in tok[6 * k:6 * k + 6])
        assert got["side"] == side and int(got["queries"]) == greater.size
        want = [pgcn.mrr(ranks)] + [pgcn.hits_at(ranks, at) for at in (10, 50, 100)]
        have = [float(got[key]) for key in ("mrr", "hits@10", "hits@50", "hits@100")]
        np.testing.assert_allclose(have, want, atol=1e-6)
        if side == "dst":
            rows = np.array([ln.split() for ln in open(out).read().splitlines()], np.int64)
            sel = (lab == 1) & (sp == 3)
            np.testing.assert_array_equal(rows[:, 0], src[sel])
            np.testing.assert_array_equal(rows[:, 1], dst[sel])
            np.testing.assert_array_equal(rows[:, 2], greater)
            np.testing.assert_array_equal(rows[:, 3], equal)
    g.close()


def test_refusals(pgcn, data, datasets):
    root, names = datasets
    bare = pgcn.Dataset.load(root, names["cora"])
    node = pgcn.GCN(pgcn.make_params(bare), bare)
    with pytest.raises(pgcn.PgcnError) as err:
        node.link_ranks(3)
    assert err.value.status == pgcn.PGCN_E_INVALID
    node.close()
    g = _engine(pgcn, data)
    for args in ((0, "dst", True), (4, "dst", True)):
        with pytest.raises(pgcn.PgcnError) as err:
            g.link_ranks(*args)
        assert err.value.status == pgcn.PGCN_E_INVALID
    with pytest.raises(ValueError):
        g.link_ranks(3, "both")
    one = np.zeros(4096, np.int64)
    assert pgcn.lib.pgcn_gcn_link_ranks(g._h, 3, 0, 1, one.ctypes.data_as(ctypes.c_void_p),
                                        None) == pgcn.PGCN_E_INVALID
    assert pgcn.lib.pgcn_gcn_link_ranks(g._h, 3, 2, 1, None, None) == pgcn.PGCN_E_INVALID
    g.close()
