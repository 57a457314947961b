"""Graph classification's host-only side (no GPU): the `readout` member of pgcn_params in step
between the C struct and the Python glue, make_params, the .graphs loader and set_graphs, the
argument checks of pgcn_readout_fwd / _bwd without a device, pgcn_checkpoint_readout on older
files and on a version-7 file written by hand, the float64 reference of tests/readout_ref.py
against central differences, and the seeds tests/test_gpu_readout.py relies on.
"""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import helpers
import readout_ref as rr
from test_cpu_layernorm import make_checkpoint
from test_cpu_residual import fnv1a


def test_params_layout_and_default(pgcn):
    """readout sits between epochs and early_stopping, in the Python struct and in the header's
    text; residual stays the last member; the sizes agree; pgcn_params_default writes 0 over a
    poisoned struct."""
    P = pgcn.PgcnParams
    names = [f[0] for f in P._fields_]
    i = names.index("readout")
    assert names[i - 1] == "epochs" and names[i + 1] == "early_stopping"
    assert names[-1] == "residual"
    assert P.epochs.offset + 4 == P.readout.offset
    assert P.readout.offset + 4 == P.early_stopping.offset
    assert ctypes.sizeof(P) == pgcn.lib.pgcn_params_sizeof()
    text = open(os.path.join(helpers.REPO, "include", "pgcn.h")).read()
    body = text[text.index("typedef struct {\n  int num_nodes"):text.index("} pgcn_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m for decl in re.findall(r"(?:unsigned )?(?:int|float) ([^;]+);", body)
               for m in re.sub(r"\[[^\]]*\]", "", decl).replace(" ", "").split(",")]
    assert members == names
    p = P()
    ctypes.memset(ctypes.byref(p), 0x5A, ctypes.sizeof(p))
    pgcn.lib.pgcn_params_default(ctypes.byref(p))
    assert p.readout == 0 and p.epochs == 100 and p.early_stopping == 0 and p.residual == 0
    # pgcn_data: the graph members behind label_words, in the header's order
    D = [f[0] for f in pgcn.PgcnData._fields_]
    assert D[-6:] == ["label_bits", "label_words", "num_graphs", "graph_ptr", "graph_label",
                      "graph_split"]
    dbody = text[text.index("typedef struct {\n  int num_nodes;"):text.index("} pgcn_data;")]
    dbody = re.sub(r"/\*.*?\*/", "", dbody, flags=re.S)
    dmembers = [m.replace("*", "") for decl in
                re.findall(r"(?:const )?(?:int|float|uint32_t) ([^;]+);", dbody)
                for m in decl.replace(" ", "").split(",")]
    assert dmembers == D


def test_make_params(pgcn):
    class Ds:  # make_params reads the three sizes only
        num_nodes, input_dim, output_dim = 10, 5, 3
    assert pgcn.make_params(Ds).readout == 0
    for name, k in (("sum", 1), ("mean", 2), ("max", 3), (None, 0)):
        assert pgcn.make_params(Ds, readout=name).readout == k
    p = pgcn.make_params(Ds, hidden_dims=(8, 8), dropouts=(0.5,) * 3, readout="mean",
                         attention=True, attention_heads=2, residual=True, layer_norm=True)
    assert p.readout == 2 and p.attention == 1 and p.attention_heads == 2 and p.residual == 1
    p = pgcn.make_params(Ds, readout="max", aggregator="max", root_weight=True)
    assert p.readout == 3 and p.aggregator == 2 and p.root_weight == 1
    for bad in (dict(readout="avg"), dict(readout=1), dict(readout="mean", multilabel=True)):
        with pytest.raises(ValueError):
            pgcn.make_params(Ds, **bad)


def _tiny(tmp_path, n=7):
    """A 7-node data set as text under tmp_path/data."""
    data = tmp_path / "data"
    data.mkdir(exist_ok=True)
    with open(data / "t.graph", "w") as f:
        f.write("".join(f"{(i + 1) % n}\n" for i in range(n)))
    with open(data / "t.svmlight", "w") as f:
        f.write("".join(f"{i % 2} 0:1.5 1:{i}\n" for i in range(n)))
    with open(data / "t.split", "w") as f:
        f.write("".join(f"{1 + i % 3}\n" for i in range(n)))
    return data


def test_graphs_loader_and_set_graphs(pgcn, tmp_path):
    data = _tiny(tmp_path)

    def load():
        return pgcn.Dataset.load(str(tmp_path), "t")

    def write(text):
        path = str(data / "t.graphs")
        with open(path, "w") as f:
            f.write(text)
        return path
    ds = load()
    assert ds.num_graphs == 0 and ds.graph_ptr is None and ds.graph_label is None
    assert ds.view.num_graphs == 0 and not ds.view.graph_ptr and ds.output_dim == 2
    ds.load_graphs(write("3 0 1\n0 2 2\n4 -1 3\n"))
    assert ds.num_graphs == 3 and ds.output_dim == 3  # (max label + 1, as load_labels)
    assert ds.graph_ptr.tolist() == [0, 3, 3, 7]
    assert ds.graph_label.tolist() == [0, 2, -1] and ds.graph_split.tolist() == [1, 2, 3]
    assert ds.num_nodes == 7 and ds.label.tolist() == [i % 2 for i in range(7)]  # (untouched)
    ds.load_graphs(write("3 0 1\n4 1 0\n"), num_classes=5)
    assert ds.num_graphs == 2 and ds.output_dim == 5 and ds.graph_split.tolist() == [1, 0]
    bad = {
        "rows short": "3 0 1\n3 1 2\n", "rows long": "3 0 1\n5 1 2\n", "split 4": "3 0 1\n4 1 4\n",
        "split -1": "3 0 1\n4 1 -1\n", "label -2": "3 -2 1\n4 1 2\n", "two fields": "3 0\n4 1 2\n",
        "four fields": "3 0 1 9\n4 1 2\n", "not a number": "3 x 1\n4 1 2\n",
        "negative rows": "-1 0 1\n8 1 2\n", "empty": "",
    }
    for name, text in bad.items():
        with pytest.raises(pgcn.PgcnError) as e:
            load().load_graphs(write(text))
        assert e.value.status == pgcn.PGCN_E_IO, name
    with pytest.raises(pgcn.PgcnError) as e:  # label >= classes
        load().load_graphs(write("3 0 1\n4 2 2\n"), num_classes=2)
    assert e.value.status == pgcn.PGCN_E_IO
    with pytest.raises(pgcn.PgcnError) as e:
        load().load_graphs(str(data / "missing.graphs"))
    assert e.value.status == pgcn.PGCN_E_IO
    # set_graphs: the same arrays, copied
    b = load()
    gp = np.array([0, 3, 3, 7])
    b.set_graphs(gp, [0, 2, -1], [1, 2, 3])
    gp[:] = 0
    assert b.graph_ptr.tolist() == [0, 3, 3, 7] and b.output_dim == 3 and b.num_graphs == 3
    b.set_graphs([0, 7], [1], [2], num_classes=4)
    assert b.num_graphs == 1 and b.output_dim == 4
    for args in (([0, 3, 6], [0, 1], [1, 2]), ([1, 3, 7], [0, 1], [1, 2]),
                 ([0, 4, 3, 7], [0, 1, 1], [1, 2, 3]), ([0, 3, 7], [0, 1], [1, 4]),
                 ([0, 3, 7], [0, -2], [1, 2]), ([0, 3, 7], [0, 3], [1, 2], 3)):
        with pytest.raises(pgcn.PgcnError) as e:
            load().set_graphs(*args)
        assert e.value.status == pgcn.PGCN_E_INVALID, args
    with pytest.raises(ValueError):
        load().set_graphs([0, 3, 7], [0], [1, 2])


def test_entries_argument_checks(pgcn):
    """The symbols exist; bad d, ld, mode and null pointers are PGCN_E_INVALID before the device
    is looked for (this machine may have none)."""
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    for name in ("pgcn_readout_fwd", "pgcn_readout_bwd", "pgcn_readout_chunk_rows",
                 "pgcn_readout_workspace", "pgcn_dataset_set_graphs", "pgcn_dataset_load_graphs",
                 "pgcn_checkpoint_readout"):
        assert hasattr(lib, name) and name in pgcn.EXPORTED
    T = lib.pgcn_readout_chunk_rows()
    assert T >= 64 and lib.pgcn_readout_workspace(3 * T + 5) >= 4 * 128 * 8
    raw = np.zeros(4 * 132 + 4, np.float32)
    a = raw[(-raw.ctypes.data % 16) // 4:][:4 * 132]  # rows on the 16-byte grid
    vp = a.ctypes.data_as(ctypes.c_void_p)
    off = ctypes.c_void_p(a.ctypes.data + 4)
    import torch
    have = torch.cuda.is_available()  # (with a device a valid call would launch on host memory)

    def fwd(d=4, mode=1, ld_in=4, ld_out=4, ld_arg=4, inp=vp, gp=vp, out=vp, arg=vp, G=2, n=4,
            max_len=4, ws=vp):
        return lib.pgcn_readout_fwd(inp, ld_in, gp, G, n, d, mode, max_len, out, ld_out, arg,
                                    ld_arg, ws, None)
    assert fwd(d=0) == INV and fwd(d=-1) == INV
    assert fwd(d=129, ld_in=132, ld_out=132, ld_arg=132) == INV
    assert fwd(mode=0) == INV and fwd(mode=4) == INV and fwd(mode=-1) == INV
    for k in ("ld_in", "ld_out", "ld_arg"):
        assert fwd(**{k: 6}) == INV and fwd(**{k: 0}) == INV and fwd(d=5, **{k: 4}) == INV, k
    for k in ("inp", "out", "gp"):
        assert fwd(**{k: None}) == INV, k
    for k in ("inp", "out", "arg"):
        assert fwd(**{k: off}) == INV, k
    assert fwd(G=-1) == INV and fwd(n=-1) == INV and fwd(max_len=-1) == INV
    assert fwd(n=2 * T, max_len=T + 1, ws=None) == INV  # long ranges need the workspace
    assert fwd(n=2 * T, max_len=T + 1, ws=off) == INV

    def bwd(d=4, mode=3, ld_g=4, ld_arg=4, ld_din=4, G_out=vp, gp=vp, ng=vp, arg=vp, din=vp):
        return lib.pgcn_readout_bwd(G_out, ld_g, gp, ng, arg, ld_arg, 2, 4, d, mode, din, ld_din,
                                    None)
    assert bwd(d=0) == INV and bwd(d=129, ld_g=132, ld_arg=132, ld_din=132) == INV
    assert bwd(mode=0) == INV and bwd(mode=4) == INV
    for k in ("ld_g", "ld_arg", "ld_din"):
        assert bwd(**{k: 6}) == INV and bwd(**{k: 0}) == INV and bwd(d=5, **{k: 4}) == INV, k
    for k in ("G_out", "gp", "ng", "arg", "din"):
        assert bwd(**{k: None}) == INV, k
    for k in ("G_out", "arg", "din"):
        assert bwd(**{k: off}) == INV, k
    if not have:
        assert fwd() == pgcn.PGCN_E_NODEVICE and bwd() == pgcn.PGCN_E_NODEVICE
        assert bwd(mode=1, arg=None) == pgcn.PGCN_E_NODEVICE  # (arg: the max only)


def _v7(readout=2, graphs=24, flags=32, heads=1, p=0.0, agg=0, root=0, zero=0, version=7,
        dims=(5, 4, 4, 3)):
    """A version-7 file by hand: make_checkpoint's header, the three blocks, plain layer weights."""
    n_w = sum(a * b for a, b in zip(dims, dims[1:])) * (2 if root == 1 else 1)
    if flags & 2:
        n_w += 2 * sum(dims[1:-1])
    if flags & 8:
        n_w += 2 * sum(dims[1:])
    rng = np.random.default_rng(3)
    payload = b"".join(rng.standard_normal(k).astype("<f4").tobytes() for k in (8, n_w, n_w, n_w))
    proto, _ = make_checkpoint(1, 0, False, dims=dims, rows=2)
    head = bytearray(proto[:208])
    struct.pack_into("<I", head, 8, version)
    struct.pack_into("<I", head, 164, flags)
    struct.pack_into("<q", head, 200, n_w)
    head = bytes(head)
    ext = struct.pack("<IfQ", heads, p, 0) + struct.pack("<IIQ", agg, root, 0) + \
        struct.pack("<IIQ", readout, graphs, zero)
    return head + struct.pack("<Q", fnv1a(head + ext + payload)) + ext + payload, n_w


def test_checkpoint_readout(pgcn, tmp_path):
    """Older files read as (0, 0); version 7 = flags bit 5 and three 16-byte blocks under the
    checksum; a bad block, a missing bit or bit 5 in an older version is no valid file."""
    def put(name, blob):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(blob)
        return path
    v1, _ = make_checkpoint(1, 0, False)
    v2, _ = make_checkpoint(2, 2, True)
    for name, blob in (("v1.pgcnck", v1), ("v2.pgcnck", v2)):
        assert pgcn.checkpoint_readout(put(name, blob)) == (0, 0)
    from test_cpu_sage import _sage_file
    assert pgcn.checkpoint_readout(put("v6.pgcnck", _sage_file()[0])) == (0, 0)
    assert pgcn.CKPT_READOUT == 32
    for kw, want in ((dict(), (2, 24)), (dict(readout=3, graphs=1, flags=32 | 1 | 2), (3, 1)),
                     (dict(readout=1, flags=32 | 8, heads=1), (1, 24)),
                     (dict(readout=1, flags=32 | 8, heads=2, p=0.5, dims=(5, 8, 8, 3)), (1, 24)),
                     (dict(readout=2, flags=32 | 16 | 2, agg=2, root=1), (2, 24))):
        blob, n_w = _v7(**kw)
        path = put("v7.pgcnck", blob)
        assert pgcn.checkpoint_readout(path) == want, kw
        info = pgcn.checkpoint_info(path)
        assert info["version"] == 7 and info["weights"] == n_w
        assert pgcn.checkpoint_flags(path) == kw.get("flags", 32)
        assert pgcn.checkpoint_attention(path) == (kw.get("heads", 1), kw.get("p", 0.0))
        assert pgcn.checkpoint_sage(path) == (kw.get("agg", 0), kw.get("root", 0))
    bad = {
        "mode 0": _v7(readout=0)[0], "mode 4": _v7(readout=4)[0], "no graphs": _v7(graphs=0)[0],
        "last word": _v7(zero=1)[0], "no bit 5": _v7(flags=0)[0],
        "multilabel bit": _v7(flags=32 | 4)[0], "bit 5 in version 1": _v7(version=1)[0],
        "heads without attention": _v7(heads=2, dims=(5, 8, 8, 3))[0],
        "head width 2": _v7(flags=32 | 8, heads=2)[0], "aggregator without bit 4": _v7(agg=1)[0],
        "bit 4 without aggregator": _v7(flags=32 | 16)[0], "truncated": _v7()[0][:-4],
    }
    for name, blob in bad.items():
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.checkpoint_readout(put("bad.pgcnck", blob))
        assert e.value.status == pgcn.PGCN_E_IO, name


@pytest.mark.parametrize("mode", rr.MODES)
def test_reference_backward_against_central_differences(mode):
    """The analytic din of sum(G * out) against central differences in float64, on inputs whose
    per-column values are pairwise distinct (no argmax sits on a tie): relative difference below
    1e-6.  Ranges of 0, 1 and more rows."""
    rng = np.random.default_rng(12)
    gp = np.array([0, 0, 1, 6, 6, 14])
    n, d = 14, 4
    X = rng.permuted(np.linspace(-2.0, 2.0, n * d).reshape(n, d), axis=0)
    G = rng.standard_normal((len(gp) - 1, d))
    out, arg = rr.readout_forward(gp, X, mode)
    assert (out[[0, 3]] == 0).all() and (arg[[0, 3]] == -1).all()
    if mode == "max":
        assert (arg[1] == 0).all() and ((arg[2] >= 1) & (arg[2] < 6)).all()
        assert np.isinf(rr.max_margin(gp, X)[[0, 1, 3]]).all()
    an = rr.readout_backward(gp, G, mode, arg)
    assert an.shape == (n, d)
    h = 1e-6
    num = np.zeros((n, d))
    for i in range(n):
        for c in range(d):
            hi, lo = X.copy(), X.copy()
            hi[i, c] += h
            lo[i, c] -= h
            num[i, c] = ((G * rr.readout_forward(gp, hi, mode)[0]).sum() -
                         (G * rr.readout_forward(gp, lo, mode)[0]).sum()) / (2 * h)
    assert np.abs(num - an).max() <= 1e-6 * np.abs(an).max()


def test_reference_max_takes_the_lowest_row():
    gp = np.array([0, 3, 3, 5])
    X = np.array([[3.0, -0.0], [3.0, 0.0], [1.0, -5.0], [2.0, 0.0], [2.0, -0.0]], np.float32)
    out, arg = rr.readout_forward(gp, X, "max")
    assert arg.tolist() == [[0, 0], [-1, -1], [3, 3]]
    assert np.signbit(out[0, 1]) and not np.signbit(out[2, 1])
    gap = rr.max_margin(gp, X)
    assert gap[0, 0] == 0.0 and np.isinf(gap[1]).all()
    assert rr.node_graph(gp).tolist() == [0, 0, 0, 2, 2]


CASES = [(mode, (8,), dropout, "SAGE_MEAN") for mode in rr.MODES for dropout in (False, True)] + \
        [("mean", (8, 8), True, "COMPOSED_SAGE")]


@pytest.mark.parametrize("mode,hidden,dropout,family", CASES)
def test_seeds_of_the_gpu_parity_tests(pgcn, mode, hidden, dropout, family):
    """With the reference model alone: a seed in 0..15 keeps every ReLU argument and max margin
    2e-6 away from a flip over the three epochs, and the (graph, class) elements
    test_gpu_readout.py leaves out of the max readout's gradient comparison stay below 2 %."""
    import test_gpu_readout as T
    ds = T.make_dataset(pgcn)
    assert ds.num_graphs == 24 and 200 <= ds.num_nodes <= 960
    lens = np.diff(ds.graph_ptr)
    assert lens.min() >= 5 and lens.max() <= 40
    seed, ep = T.flip_free(pgcn, ds, mode, hidden, dropout, getattr(T, family))
    assert ep["close"] >= T.FLIP and ep["share"] < T.CAP
    assert np.isfinite(np.array(ep["lines"])).all()
