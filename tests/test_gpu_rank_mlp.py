"""GCN.link_ranks(decoder=True): ranking by the Hadamard-MLP decoder's score on the engine of
tests/test_gpu_link_mlp.py (500 nodes, embedding width 8, link_hidden = 8) after three epochs.

The comparison is exact: numpy derives the counts from g.score_pairs of every test anchor against
all nodes -- the pair forward the sweep has to reproduce bit for bit -- with pgcn.rank_filter's
query sets and lists.
"""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_link import HIDDEN, make_dataset
from test_gpu_rank import pair_arrays

pytestmark = pytest.mark.gpu

H = 8


def _filter(pgcn, ds, side, filtered):
    return pgcn.rank_filter(ds.num_nodes, ds.graph_indptr, ds.graph_indices, ds.pair_src,
                            ds.pair_dst, ds.pair_label, ds.pair_split, 3, side, filtered)


@pytest.fixture(scope="module")
def trained(pgcn):
    """(data set, engine, side -> S [Q][n], the decoder's score of every (test anchor, node))"""
    ds = make_dataset(pgcn)
    g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=HIDDEN, link_decoder="dot", link_hidden=H), ds)
    for _ in range(3):
        g.train_epoch()
    n, scores = ds.num_nodes, {}
    for side in ("dst", "src"):
        a = _filter(pgcn, ds, side, False)[0]
        every = np.tile(np.arange(n, dtype=np.int32), a.size)
        scores[side] = g.score_pairs(np.repeat(a, n), every).reshape(a.size, n)
    yield ds, g, scores
    g.close()


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("side", ["dst", "src"])
def test_decoder_ranks_equal_numpy_counts(pgcn, trained, side, filtered):
    ds, g, scores = trained
    S, n = scores[side], ds.num_nodes
    a, t, ptr, idx = _filter(pgcn, ds, side, filtered)
    mask = np.ones((a.size, n), bool)
    mask[np.arange(a.size), t] = False
    for e in range(a.size):
        mask[e, idx[ptr[e]:ptr[e + 1]]] = False
    thr = S[np.arange(a.size), t][:, None]
    greater, equal = g.link_ranks(3, side, filtered, decoder=True)
    assert greater.dtype == np.int64 and a.size > 100 and (not filtered or idx.size > a.size)
    np.testing.assert_array_equal(greater, ((S > thr) & mask).sum(1))
    np.testing.assert_array_equal(equal, ((S == thr) & mask).sum(1))


def test_dot_engine_has_no_decoder(pgcn, trained):
    ds = trained[0]
    dot = pgcn.GCN(pgcn.make_params(ds, hidden_dims=HIDDEN, link_decoder="dot"), ds)
    with pytest.raises(pgcn.PgcnError) as e:
        dot.link_ranks(3, decoder=True)
    assert e.value.status == pgcn.PGCN_E_INVALID
    dot.close()


def test_cli_rank_line_under_the_decoder(pgcn, datasets, tmp_path):
    """gcn-par NAME link=dot link_hidden=8 rank=1 prints link_ranks(decoder=True)'s metrics."""
    import helpers
    root, names = datasets
    base = pgcn.Dataset.load(root, names["cora"])
    src, dst, lab, sp = pair_arrays(pgcn, base, 300)
    links = os.path.join(root, "data", names["cora"] + ".links")
    with open(links, "w") as f:
        for e in range(src.size):
            f.write(f"{src[e]} {dst[e]} {lab[e]} {sp[e]}\n")
    exe = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "gcn-par")
    ck = str(tmp_path / "ck")
    r = subprocess.run([exe, names["cora"], f"root={root}", "link=dot", "embed=8", f"link_hidden={H}",
                        "epochs=3", f"save={ck}", "rank=1"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("rank ")]
    assert len(line) == 1
    tok = line[0].split()[1:]
    base.load_links(links, 8)
    g = pgcn.GCN(pgcn.make_params(base, link_decoder="dot", link_hidden=H), base)
    g.load(ck)
    for k, side in enumerate(("dst", "src")):
        ranks = pgcn.rank_from_counts(*g.link_ranks(3, side, True, decoder=True))
        got = dict(t.split("=") for t in tok[6 * k:6 * k + 6])
        assert got["side"] == side and int(got["queries"]) == ranks.size
        want = [pgcn.mrr(ranks)] + [pgcn.hits_at(ranks, at) for at in (10, 50, 100)]
        have = [float(got[key]) for key in ("mrr", "hits@10", "hits@50", "hits@100")]
        np.testing.assert_allclose(have, want, atol=1e-6)
    g.close()
