"""GCN.top_links(decoder=True) on tests/test_gpu_rank_mlp.py's engine (500 nodes, embedding width
8, link_hidden = 8, three epochs), exactly: numpy's top-K (tests/topk_ref.py) over g.score_pairs of
every anchor against all nodes -- the pair forward itself -- minus pgcn.topk_filter's lists."""
import os
import subprocess

import numpy as np
import pytest

import topk_ref
from test_gpu_link import HIDDEN, make_dataset
from test_gpu_rank import pair_arrays
from test_gpu_rank_mlp import H

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trained(pgcn):
    """(data set, engine, nodes, S [m][n]: the decoder's score of every (node, candidate))"""
    ds = make_dataset(pgcn)
    g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=HIDDEN, link_decoder="dot", link_hidden=H), ds)
    for _ in range(3):
        g.train_epoch()
    n = ds.num_nodes
    nodes = np.r_[np.arange(0, n, 13), 0, n - 1].astype(np.int32)   # one node twice
    S = g.score_pairs(np.repeat(nodes, n), np.tile(np.arange(n, dtype=np.int32), nodes.size))
    yield ds, g, nodes, S.reshape(nodes.size, n)
    g.close()


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("side", ["dst", "src"])
def test_decoder_top_links_equal_numpy_topk(pgcn, trained, side, filtered, k):
    ds, g, nodes, S = trained
    ptr, idx = pgcn.topk_filter(ds.num_nodes, ds.graph_indptr, ds.graph_indices, ds.pair_src,
                                ds.pair_dst, ds.pair_label, ds.pair_split, nodes, side, filtered)
    pgcn.reset_path_counts()
    gi, gs = g.top_links(nodes, k, side, filtered, decoder=True)
    c = pgcn.path_counts(reset=True)
    assert c["topk_mlp_sweep"] == 1 and c["topk_mlp_merge"] == 1 and c["topk_sweep"] == 0
    assert gi.dtype == np.int32 and gs.dtype == np.float32 and gi.shape == (nodes.size, k)
    wi, ws = topk_ref.topk_model(S, k, ptr if filtered else None, idx)
    np.testing.assert_array_equal(gi, wi)
    assert (gs == ws).all()
    assert not filtered or (idx.size > nodes.size and not (gi == nodes[:, None]).any())


def test_cli_recommend_file_under_the_decoder(pgcn, datasets, tmp_path):
    """gcn-par NAME link=dot link_hidden=8 recommend=FILE topk=5: top_links(decoder=True)'s rows;
    decoder=True on a dot engine is PGCN_E_INVALID."""
    import helpers
    root, names = datasets
    base = pgcn.Dataset.load(root, names["cora"])
    src, dst, lab, sp = pair_arrays(pgcn, base, 300)
    links = os.path.join(root, "data", names["cora"] + ".links")
    np.savetxt(links, np.c_[src, dst, lab, sp], fmt="%d")
    exe = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "gcn-par")
    ck, out = str(tmp_path / "ck"), str(tmp_path / "rec.txt")
    r = subprocess.run([exe, names["cora"], f"root={root}", "link=dot", "embed=8", f"link_hidden={H}",
                        "epochs=3", f"save={ck}", f"recommend={out}", "topk=5"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    base.load_links(links, 8)
    dot = pgcn.GCN(pgcn.make_params(base, link_decoder="dot"), base)
    with pytest.raises(pgcn.PgcnError) as e:
        dot.top_links([0], 3, decoder=True)
    assert e.value.status == pgcn.PGCN_E_INVALID
    dot.close()
    g = pgcn.GCN(pgcn.make_params(base, link_decoder="dot", link_hidden=H), base)
    g.load(ck)
    gi, gs = g.top_links(np.arange(base.num_nodes), 5, "dst", True, decoder=True)
    g.close()
    lines = open(out).read().splitlines()
    assert len(lines) == base.num_nodes
    for i, ln in enumerate(lines):
        tok, keep = ln.split(), gi[i] >= 0
        assert int(tok[0]) == i and [int(x) for x in tok[1::2]] == gi[i][keep].tolist()
        np.testing.assert_allclose([float(x) for x in tok[2::2]], gs[i][keep], atol=1e-6)
