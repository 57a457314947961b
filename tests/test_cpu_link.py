"""Link prediction without a device: the reference formulas of tests/link_ref.py, the incidence
index pgcn_links_create builds (through the host-only pgcn_debug_links_incidence), the .links
loader, the host helpers link_auc and sample_negative_pairs, the struct layouts, version-8
checkpoints, and the seed search of tests/test_gpu_link.py."""
import ctypes
import struct

import numpy as np
import pytest

import link_ref as lr
from test_cpu_readout import _v7
from test_cpu_residual import fnv1a


def test_reference_backward_against_central_differences():
    """The analytic dH of sum(g * score) over the selected pairs against central differences in
    float64: a self pair, a duplicated pair, an unselected pair, a node without pairs."""
    rng = np.random.default_rng(4)
    n, d = 7, 5
    src = np.array([0, 1, 2, 2, 3, 3, 5, 0])
    dst = np.array([1, 2, 2, 4, 1, 1, 0, 1])
    sel = np.array([0, 0, 0, 3, 0, 0, -1, 1])
    H, g = rng.standard_normal((n, d)), rng.standard_normal(len(src))
    an = lr.score_backward(src, dst, H, g, sel)
    assert (an[6] == 0).all() and (an[5] == 0).all()  # no pair; only an unselected one
    planted = np.where(sel < 0, np.nan, g)  # g of an unselected pair is never read
    np.testing.assert_allclose(lr.score_backward(src, dst, H, planted, sel), an)
    on = sel >= 0
    h = 1e-6
    num = np.zeros((n, d))
    for i in range(n):
        for c in range(d):
            hi, lo = H.copy(), H.copy()
            hi[i, c] += h
            lo[i, c] -= h
            num[i, c] = ((g * lr.score_forward(src, dst, hi))[on].sum() -
                         (g * lr.score_forward(src, dst, lo))[on].sum()) / (2 * h)
    assert np.abs(num - an).max() <= 1e-6 * np.abs(an).max()
    mag, m = lr.score_backward_magnitude(src, dst, H, g, sel)
    assert m.tolist() == [2, 5, 4, 2, 1, 0, 0] and (mag >= np.abs(an) - 1e-12).all()


def test_incidence_order(pgcn):
    """Ascending pair order per node, the src role before the dst role: a self pair gives two
    consecutive entries, a duplicated pair counts twice, select < 0 is left out."""
    src = np.array([2, 0, 1, 1, 0, 3, 0], np.int32)
    dst = np.array([0, 0, 0, 0, 2, 0, 1], np.int32)
    sel = np.array([5, 0, 0, 7, 0, -1, 0], np.int32)
    ptr, pair, other = pgcn.links_incidence(5, src, dst, sel)
    assert ptr.tolist() == [0, 7, 10, 12, 12, 12]
    assert pair[:7].tolist() == [0, 1, 1, 2, 3, 4, 6]   # node 0: the self pair 1 twice in a row
    assert other[:7].tolist() == [2, 0, 0, 1, 1, 2, 1]
    assert pair[7:10].tolist() == [2, 3, 6] and other[7:10].tolist() == [0, 0, 0]
    assert pair[10:].tolist() == [0, 4] and other[10:].tolist() == [0, 0]
    for s in (sel, None):
        got = pgcn.links_incidence(5, src, dst, s)
        want = lr.incidence(5, src, dst, s)
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)
    assert pgcn.links_incidence(5, src, dst)[0][-1] == 14
    rng = np.random.default_rng(2)
    s, t = rng.integers(0, 40, 3000).astype(np.int32), rng.integers(0, 40, 3000).astype(np.int32)
    k = rng.integers(-1, 2, 3000).astype(np.int32)
    for a, b in zip(pgcn.links_incidence(40, s, t, k), lr.incidence(40, s, t, k)):
        np.testing.assert_array_equal(a, b)
    for bad in ((np.array([5], np.int32), np.array([0], np.int32)),
                (np.array([0], np.int32), np.array([-1], np.int32))):
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.links_incidence(5, *bad)
        assert e.value.status == pgcn.PGCN_E_INVALID
    empty = pgcn.links_incidence(3, np.zeros(0, np.int32), np.zeros(0, np.int32))
    assert empty[0].tolist() == [0, 0, 0, 0] and empty[1].size == 0


def test_kernel_entries_without_device(pgcn):
    """The symbols exist; bad d, ld and null pointers are PGCN_E_INVALID before the device is
    looked for (this machine may have none)."""
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    for name in ("pgcn_links_create", "pgcn_links_destroy", "pgcn_link_segment_slots",
                 "pgcn_links_slots", "pgcn_link_score_fwd", "pgcn_link_score_bwd",
                 "pgcn_debug_links_incidence", "pgcn_gcn_predict_links", "pgcn_gcn_link_counts",
                 "pgcn_gcn_score_pairs", "pgcn_dataset_set_links", "pgcn_dataset_load_links",
                 "pgcn_checkpoint_links"):
        assert hasattr(lib, name) and name in pgcn.EXPORTED
    assert lib.pgcn_link_segment_slots() == 512
    assert "link_fwd" in pgcn.KERNEL_PATHS and "link_bwd" in pgcn.path_counts()
    raw = np.zeros(64 + 4, np.float32)
    a = raw[(-raw.ctypes.data % 16) // 4:][:64]
    vp = a.ctypes.data_as(ctypes.c_void_p)
    assert lib.pgcn_link_score_fwd(None, vp, 4, 4, vp, 4, None) == INV
    assert lib.pgcn_link_score_bwd(None, vp, 4, 4, vp, 4, vp, 4, None) == INV
    assert lib.pgcn_links_slots(None) == INV
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.Links(3, [0], [1])
        assert e.value.status == pgcn.PGCN_E_NODEVICE
    with pytest.raises(pgcn.PgcnError) as e:
        pgcn.Links(3, [0], [3])
    assert e.value.status == INV


def test_links_loader(pgcn, tmp_path):
    ds = pgcn.Dataset.synthetic(20, 4, 3, 40, 1)
    assert ds.num_pairs == 0 and ds.pair_src is None

    def put(text):
        p = tmp_path / "t.links"
        p.write_text(text)
        return str(p)
    ds.load_links(put("0 1 1 1\n\n2 3 0 2\n19 0 -1 3\n5 5 1 0\n"), 16)
    assert ds.num_pairs == 4 and ds.output_dim == 16
    assert ds.pair_src.tolist() == [0, 2, 19, 5] and ds.pair_dst.tolist() == [1, 3, 0, 5]
    assert ds.pair_label.tolist() == [1, 0, -1, 1] and ds.pair_split.tolist() == [1, 2, 3, 0]
    bad = {"three integers": "0 1 1\n", "five": "0 1 1 1 1\n", "a word": "0 1 x 1\n",
           "a real": "0 1 0.5 1\n", "endpoint n": "0 20 1 1\n", "endpoint -1": "-1 2 1 1\n",
           "label 2": "0 1 2 1\n", "label -2": "0 1 -2 1\n", "split 4": "0 1 1 4\n",
           "split -1": "0 1 1 -1\n", "empty": "\n"}
    for name, text in bad.items():
        with pytest.raises(pgcn.PgcnError) as e:
            ds.load_links(put("1 2 0 1\n" + text if name != "empty" else text), 16)
        assert e.value.status == pgcn.PGCN_E_IO, name
    with pytest.raises(pgcn.PgcnError) as e:
        ds.load_links(str(tmp_path / "missing.links"), 16)
    assert e.value.status == pgcn.PGCN_E_IO
    for dim in (0, 129):
        with pytest.raises(pgcn.PgcnError) as e:
            ds.load_links(put("0 1 1 1\n"), dim)
        assert e.value.status == pgcn.PGCN_E_INVALID
    assert ds.num_pairs == 4 and ds.output_dim == 16  # (a failed load changes nothing)
    ds.set_links([1, 2], [3, 4], [1, 0], [1, 2], 8)
    assert ds.num_pairs == 2 and ds.output_dim == 8 and ds.pair_dst.tolist() == [3, 4]
    # the binary cache carries the node-level arrays only
    path = str(tmp_path / "syn.pgcnbin")
    ds.save(path)
    assert pgcn.Dataset.load_binary(path).num_pairs == 0


def test_link_auc(pgcn):
    pg = pgcn
    assert pg.link_auc([0.1, 0.4, 0.35, 0.8], [0, 0, 1, 1]) == 0.75
    assert pg.link_auc([1, 2, 3, 4], [0, 0, 1, 1]) == 1.0
    assert pg.link_auc([4, 3, 2, 1], [0, 0, 1, 1]) == 0.0
    assert pg.link_auc([1, 1, 1, 1], [0, 1, 0, 1]) == 0.5          # all tied
    assert pg.link_auc([1, 1, 1, 2, 0], [0, 1, 1, 1, -1]) == pytest.approx(2 / 3)  # ties, a skip
    assert pg.link_auc([0.5, 0.5, 0.2, 0.9], [1, 0, 0, 1]) == pytest.approx(3.5 / 4)
    assert np.isnan(pg.link_auc([1, 2], [1, 1])) and np.isnan(pg.link_auc([1, 2], [-1, 0]))
    rng = np.random.default_rng(6)
    s = rng.integers(0, 12, 300).astype(np.float64)  # many ties
    y = rng.integers(-1, 2, 300)
    assert pg.link_auc(s, y) == pytest.approx(lr.auc(s[y >= 0], y[y >= 0]), abs=1e-12)


def test_sample_negative_pairs(pgcn):
    ds = pgcn.Dataset.synthetic(60, 4, 3, 500, 3)  # dense enough that rejections happen
    src = np.arange(60).repeat(2)
    s, d = pgcn.sample_negative_pairs(ds, src, ratio=3, seed=9)
    assert s.dtype == d.dtype == np.int32 and s.shape == d.shape == (360,)
    np.testing.assert_array_equal(s, src.repeat(3))
    assert (s != d).all() and d.min() >= 0 and d.max() < 60
    rows = np.repeat(np.arange(60), np.diff(ds.graph_indptr))
    adj = set(zip(rows.tolist(), ds.graph_indices.tolist()))
    assert adj and not any((a, b) in adj or (b, a) in adj for a, b in zip(s.tolist(), d.tolist()))
    s2, d2 = pgcn.sample_negative_pairs(ds, src, ratio=3, seed=9)
    np.testing.assert_array_equal(d, d2)
    assert (pgcn.sample_negative_pairs(ds, src, ratio=3, seed=10)[1] != d).any()
    assert len(np.unique(d)) > 30  # (spread over the nodes)
    with pytest.raises(ValueError):
        pgcn.sample_negative_pairs(ds, [60])


def test_params_layout_and_default(pgcn):
    """link_decoder in the Python struct where the header has it; residual stays the last member;
    the sizes agree; pgcn_params_default writes 0 over a poisoned struct; the pair members of
    pgcn_data sit behind label / split."""
    P = pgcn.PgcnParams
    names = [f[0] for f in P._fields_]
    i = names.index("link_decoder")
    assert names[i - 1] == "n_layers" and names[i + 1] == "hidden_dims" and names[-1] == "residual"
    assert P.n_layers.offset + 4 == P.link_decoder.offset == P.hidden_dims.offset - 4
    assert ctypes.sizeof(P) == pgcn.lib.pgcn_params_sizeof()
    p = P()
    ctypes.memset(ctypes.byref(p), 0x5A, ctypes.sizeof(p))
    pgcn.lib.pgcn_params_default(ctypes.byref(p))
    assert p.link_decoder == 0 and p.readout == 0 and p.n_layers == 2
    D = [f[0] for f in pgcn.PgcnData._fields_]
    k = D.index("num_pairs")
    assert D[k - 1] == "split" and D[k:k + 5] == ["num_pairs", "pair_src", "pair_dst",
                                                  "pair_label", "pair_split"]

    class Ds:  # make_params reads the three sizes only
        num_nodes, input_dim, output_dim = 10, 5, 8
    assert pgcn.make_params(Ds).link_decoder == 0
    assert pgcn.make_params(Ds, link_decoder="dot", aggregator="max").link_decoder == 1
    for bad in (dict(link_decoder="mlp"), dict(link_decoder="dot", multilabel=True),
                dict(link_decoder="dot", readout="sum")):
        with pytest.raises(ValueError):
            pgcn.make_params(Ds, **bad)


def _v8(decoder=1, pairs=1200, flags=64, zero=0, version=8, readout=0, graphs=0, **kw):
    """A version-8 file by hand: test_cpu_readout's version-7 bytes with the fourth block."""
    blob, n_w = _v7(readout=readout, graphs=graphs, flags=flags, version=version, **kw)
    head, ext, payload = blob[:208], blob[216:216 + 48], blob[216 + 48:]
    ext += struct.pack("<IIQ", decoder, zero, pairs)
    return head + struct.pack("<Q", fnv1a(head + ext + payload)) + ext + payload, n_w


def test_checkpoint_links(pgcn, tmp_path):
    """Older files read as (0, 0); version 8 = flag bit 6 and four 16-byte blocks under the
    checksum; a bad block, a wrong bit or garbage is no valid file."""
    def put(name, blob):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(blob)
        return path
    assert pgcn.CKPT_LINKS == 64
    v7 = put("v7.pgcnck", _v7()[0])
    assert pgcn.checkpoint_links(v7) == (0, 0) and pgcn.checkpoint_readout(v7) == (2, 24)
    for kw, want in ((dict(), (1, 1200)), (dict(pairs=1, flags=64 | 1 | 2), (1, 1)),
                     (dict(flags=64 | 8, heads=2, p=0.5, dims=(5, 8, 8, 3)), (1, 1200)),
                     (dict(flags=64 | 16 | 2, agg=2, root=1, pairs=2 ** 31 - 1), (1, 2 ** 31 - 1))):
        blob, n_w = _v8(**kw)
        path = put("v8.pgcnck", blob)
        assert pgcn.checkpoint_links(path) == want, kw
        info = pgcn.checkpoint_info(path)
        assert info["version"] == 8 and info["weights"] == n_w
        assert pgcn.checkpoint_flags(path) == kw.get("flags", 64)
        assert pgcn.checkpoint_readout(path) == (0, 0)
        assert pgcn.checkpoint_attention(path) == (kw.get("heads", 1), kw.get("p", 0.0))
        assert pgcn.checkpoint_sage(path) == (kw.get("agg", 0), kw.get("root", 0))
    bad = {
        "decoder 0": _v8(decoder=0)[0], "decoder 2": _v8(decoder=2)[0],
        "no pairs": _v8(pairs=0)[0], "pairs 2^31": _v8(pairs=2 ** 31)[0],
        "middle word": _v8(zero=1)[0], "no bit 6": _v8(flags=0)[0],
        "readout bit": _v8(flags=64 | 32)[0], "multilabel bit": _v8(flags=64 | 4)[0],
        "a readout block": _v8(readout=2, graphs=3)[0], "bit 6 in version 7": _v8(version=7)[0],
        "bit 6 in version 1": _v8(version=1)[0], "truncated": _v8()[0][:-4],
        "the fourth block missing": _v7(readout=0, graphs=0, flags=64, version=8)[0],
        "garbage": np.random.default_rng(1).bytes(600), "empty": b"",
    }
    for name, blob in bad.items():
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.checkpoint_links(put("bad.pgcnck", blob))
        assert e.value.status == pgcn.PGCN_E_IO, name


def test_multi_rank_creators_refuse_before_the_device(pgcn):
    """The edge-cut creators refuse a link engine while the parameters are read, device or not."""
    import test_gpu_link as T
    ds = T.make_dataset(pgcn)
    p = pgcn.make_params(ds, hidden_dims=(8,), link_decoder="dot")
    with pytest.raises(pgcn.PgcnError) as e:
        pgcn.GCN(p, ds, rank=0, world=1, unique_id=b"\0" * 128)
    assert e.value.status == pgcn.PGCN_E_INVALID


@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("family,hidden", [("PLAIN", (8,)), ("SAGE_MEAN", (8,)),
                                           ("COMPOSED_SAGE", (8, 8)), ("COMPOSED_GAT", (8,))])
def test_seeds_of_the_gpu_parity_tests(pgcn, family, hidden, dropout):
    """With the reference model alone: a seed in 0..15 keeps every ReLU argument and max margin
    2e-6 away from a flip over the three epochs, and the model learns something."""
    import test_gpu_link as T
    ds = T.make_dataset(pgcn)
    assert ds.num_pairs == 1200 and ds.num_nodes == 500 and ds.output_dim == 8
    assert (family, hidden) in T.HOST_CASES
    seed, ep = T.flip_free(pgcn, ds, hidden, dropout, getattr(T, family))
    assert ep["close"] >= T.FLIP
    assert np.isfinite(np.array(ep["lines"])).all()
    assert np.abs(ep["node_grad"]).max() > 0 and np.abs(ep["scores"]).max() > 0
