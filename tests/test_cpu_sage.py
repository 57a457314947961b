"""GraphSAGE's host-only side (no GPU): the `aggregator` / `root_weight` members of pgcn_params
in step between the C struct and the Python glue, the argument checks of pgcn_agg_max_fwd / _bwd
and pgcn_graph_create_mean without a device, make_params' refusals, the version-6 checkpoint
header, the float64 reference of tests/sage_ref.py against central differences, and the seeds
tests/test_gpu_sage.py relies on (its near-tie exclusions stay below 1 % of a layer).
"""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import helpers
import sage_ref
from test_cpu_layernorm import make_checkpoint
from test_cpu_residual import fnv1a


def test_params_layout_and_default(pgcn):
    """aggregator and root_weight sit between dropouts and epochs, in the Python struct and in the
    header's text; residual stays the last member; the sizes agree; pgcn_params_default writes 0
    over a poisoned struct."""
    P = pgcn.PgcnParams
    names = [f[0] for f in P._fields_]
    i = names.index("aggregator")
    assert names[i - 1] == "dropouts" and names[i + 1] == "root_weight" and names[i + 2] == "epochs"
    assert names[-1] == "residual"
    assert P.dropouts.offset + 4 * pgcn.MAX_LAYERS == P.aggregator.offset
    assert P.aggregator.offset + 4 == P.root_weight.offset
    assert P.root_weight.offset + 4 == P.epochs.offset
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
    assert p.aggregator == 0 and p.root_weight == 0 and p.epochs == 100 and p.residual == 0


def test_make_params(pgcn):
    class Ds:  # make_params reads the three sizes only
        num_nodes, input_dim, output_dim = 10, 5, 3
    p = pgcn.make_params(Ds)
    assert p.aggregator == 0 and p.root_weight == 0
    p = pgcn.make_params(Ds, aggregator="mean")
    assert p.aggregator == 1 and p.root_weight == 0
    p = pgcn.make_params(Ds, hidden_dims=(4, 4), dropouts=(0.5,) * 3, aggregator="max",
                         root_weight=True, residual=True)
    assert p.aggregator == 2 and p.root_weight == 1 and p.residual == 1 and p.attention == 0
    for bad in (dict(aggregator="sum"), dict(aggregator=1), dict(root_weight=True),
                dict(aggregator="max", attention=True)):
        with pytest.raises(ValueError):
            pgcn.make_params(Ds, **bad)


def test_entries_argument_checks(pgcn):
    """The symbols exist; bad d, bad ld and null pointers are PGCN_E_INVALID before the device is
    looked for (this machine may have none)."""
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    for name in ("pgcn_agg_max_fwd", "pgcn_agg_max_bwd", "pgcn_graph_create_mean",
                 "pgcn_checkpoint_sage"):
        assert hasattr(lib, name) and name in pgcn.EXPORTED
    raw = np.zeros(4 * 132 + 4, np.float32)
    a = raw[(-raw.ctypes.data % 16) // 4:][:4 * 132]  # rows on the 16-byte grid
    vp = a.ctypes.data_as(ctypes.c_void_p)
    off = ctypes.c_void_p(a.ctypes.data + 4)

    # (a graph handle needs a device: without one every call ends at the null handle at the latest)
    def fwd(d=4, ld_in=4, ld_add=4, ld_out=4, ld_arg=4, inp=vp, add=vp, out=vp, arg=vp):
        return lib.pgcn_agg_max_fwd(None, inp, ld_in, d, add, ld_add, out, ld_out, arg, ld_arg, None)
    assert fwd() == INV and fwd(d=0) == INV and fwd(d=-1) == INV
    assert fwd(d=129, ld_in=132, ld_add=132, ld_out=132, ld_arg=132) == INV
    for k in ("ld_in", "ld_add", "ld_out", "ld_arg"):
        assert fwd(**{k: 6}) == INV and fwd(**{k: 0}) == INV and fwd(d=5, **{k: 4}) == INV, k
    for k in ("inp", "out"):
        assert fwd(**{k: None}) == INV and fwd(**{k: off}) == INV, k
    assert fwd(add=off) == INV and fwd(arg=off) == INV

    def bwd(d=4, ld_g=4, ld_arg=4, ld_din=4, G=vp, arg=vp, din=vp):
        return lib.pgcn_agg_max_bwd(None, G, ld_g, arg, ld_arg, d, din, ld_din, None)
    assert bwd() == INV and bwd(d=0) == INV and bwd(d=129, ld_g=132, ld_arg=132, ld_din=132) == INV
    for k in ("ld_g", "ld_arg", "ld_din"):
        assert bwd(**{k: 6}) == INV and bwd(**{k: 0}) == INV and bwd(d=5, **{k: 4}) == INV, k
    for k in ("G", "arg", "din"):
        assert bwd(**{k: None}) == INV and bwd(**{k: off}) == INV, k

    ip = np.array([0, 2, 3, 3], np.int32)
    idx = np.array([1, 2, 0], np.int32)

    def mean(n=3, ip=ip, idx=idx, tr=0, out=True):
        h = ctypes.c_void_p()
        return lib.pgcn_graph_create_mean(n, ip.ctypes.data_as(ctypes.c_void_p) if ip is not None
                                          else None,
                                          idx.ctypes.data_as(ctypes.c_void_p) if idx is not None
                                          else None, tr, ctypes.byref(h) if out else None)
    assert mean(n=0) == INV and mean(n=-3) == INV and mean(tr=2) == INV and mean(tr=-1) == INV
    assert mean(ip=None) == INV and mean(idx=None) == INV and mean(out=False) == INV
    assert mean(idx=np.array([1, 3, 0], np.int32)) == INV
    assert mean(idx=np.array([1, -1, 0], np.int32)) == INV
    assert mean(ip=np.array([0, 2, 1, 3], np.int32)) == INV
    assert mean(ip=np.array([1, 2, 3, 3], np.int32)) == INV
    import torch
    if torch.cuda.is_available():
        return  # with a device the launches are covered by tests/test_gpu_sage_kernels.py
    assert mean() == pgcn.PGCN_E_NODEVICE


def _sage_file(flags=16, agg=2, root=1, zero=0, with_norm=False, version=6,
               dims=(5, 4, 4, 3), rows=2):
    """A version-6 file by hand: make_checkpoint's header fields, the block behind the header,
    every layer weight [d_in][(1 + root) d_l]."""
    L = len(dims) - 1
    n_w = sum(a * b for a, b in zip(dims, dims[1:])) * (2 if root == 1 else 1)
    if with_norm:
        n_w += 2 * sum(dims[1:-1])
    rng = np.random.default_rng(3)
    payload = b"".join(rng.standard_normal(k).astype("<f4").tobytes()
                       for k in (rows * 4, n_w, n_w, n_w))
    proto, _ = make_checkpoint(1, 0, False, dims=dims, rows=rows)
    head = bytearray(proto[:208])
    struct.pack_into("<I", head, 8, version)
    struct.pack_into("<I", head, 164, flags)
    struct.pack_into("<q", head, 200, n_w)
    head = bytes(head)
    assert struct.unpack_from("<I", head, 12)[0] == L
    ext = struct.pack("<IIQ", agg, root, zero) if version == 6 else b""
    return head + struct.pack("<Q", fnv1a(head + ext + payload)) + ext + payload, n_w


def test_version6_checkpoint(pgcn, tmp_path):
    """Version 6 = flags bit 4 and the 16-byte block {aggregator, root_weight, 0} under the
    checksum; pgcn_checkpoint_sage / _info / _flags read it; versions 1-5 read as (0, 0); a bad
    block, a missing bit, the attention bit or a weight count for the other root weight is no
    valid file."""
    def put(name, blob):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(blob)
        return path
    for agg, root, norm in ((1, 0, False), (2, 1, False), (2, 1, True), (1, 1, True)):
        blob, n_w = _sage_file(flags=16 | (2 if norm else 0), agg=agg, root=root, with_norm=norm)
        path = put(f"v6_{agg}{root}{int(norm)}.pgcnck", blob)
        assert pgcn.checkpoint_sage(path) == (agg, root)
        info = pgcn.checkpoint_info(path)
        assert info["version"] == 6 and info["weights"] == n_w and info["n_layers"] == 3
        assert pgcn.checkpoint_flags(path) == 16 | (2 if norm else 0)
        assert pgcn.checkpoint_attention(path) == (1, 0.0)
    assert pgcn.CKPT_SAGE == 16
    v1, _ = make_checkpoint(1, 0, False)
    v2, _ = make_checkpoint(2, 2, True)
    for name, blob in (("v1.pgcnck", v1), ("v2.pgcnck", v2)):
        assert pgcn.checkpoint_sage(put(name, blob)) == (0, 0)
    # versions 4 and 5 (an attention engine's; 5 keeps its own 16 bytes where version 6 has its
    # block): 0, 0, and what they read as before is unchanged
    from test_cpu_gat_heads import _v5
    n_attn = 5 * 8 + 8 * 8 + 8 * 3 + 2 * (8 + 8 + 3)
    for name, kw, want in (("v5.pgcnck", dict(heads=2, p=0.5), (2, 0.5)),
                           ("v5f.pgcnck", dict(heads=1, p=0.25, flags=9), (1, 0.25)),
                           ("v4.pgcnck", dict(version=4, heads=1, p=0.0, ext=False), (1, 0.0))):
        path = put(name, _v5(**kw))
        assert pgcn.checkpoint_sage(path) == (0, 0), name
        assert pgcn.checkpoint_attention(path) == want, name
        info = pgcn.checkpoint_info(path)
        assert info["version"] == kw.get("version", 5) and info["weights"] == n_attn, name
        assert pgcn.checkpoint_flags(path) == kw.get("flags", 8), name
    bad = {
        "aggregator 0": _sage_file(agg=0)[0], "aggregator 3": _sage_file(agg=3)[0],
        "root 2": _sage_file(root=2)[0], "last word": _sage_file(zero=1)[0],
        "no bit 4": _sage_file(flags=0)[0], "attention bit": _sage_file(flags=16 | 8)[0],
        "bit 4 in version 1": _sage_file(version=1, root=0)[0],
        "wide": _sage_file(dims=(5, 132, 4, 3))[0],
    }
    blob, _ = _sage_file(agg=2, root=1)
    other = bytearray(blob)  # the block says root 0 over a root-1 payload (checksum redone)
    struct.pack_into("<I", other, 216 + 4, 0)
    struct.pack_into("<Q", other, 208, fnv1a(bytes(other[:208]) + bytes(other[216:])))
    bad["count"] = bytes(other)
    bad["truncated"] = blob[:-4]
    for name, b in bad.items():
        path = put("bad.pgcnck", b)
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.checkpoint_sage(path)
        assert e.value.status == pgcn.PGCN_E_IO, name


def _graph(rng, n):
    rows = [rng.integers(0, n, rng.integers(0, 6)) for _ in range(n)]
    rows[1] = np.array([2, 2, 0])  # a duplicated edge
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int64)


@pytest.mark.parametrize("agg", ["mean", "max"])
def test_reference_backward_against_central_differences(agg):
    """The analytic dQ and dR of sum(G * Z) against central differences in float64, on inputs
    whose per-column values are pairwise distinct (no argmax sits on a tie): relative difference
    below 1e-6."""
    rng = np.random.default_rng(11)
    n, d = 14, 5
    indptr, indices = _graph(rng, n)
    assert (np.diff(indptr) == 0).any() and (np.bincount(indices, minlength=n) == 0).any()
    Q = rng.permuted(np.linspace(-2.0, 2.0, n * d).reshape(n, d), axis=0)
    R, G = rng.standard_normal((n, d)), rng.standard_normal((n, d))
    assert all(len(np.unique(Q[:, c])) == n for c in range(d))

    def value(Q, R):
        Z = sage_ref.mean_forward(indptr, indices, Q, R) if agg == "mean" else \
            sage_ref.max_forward(indptr, indices, Q, R)[0]
        return float((G * Z).sum())
    if agg == "mean":
        dQ = sage_ref.mean_backward(indptr, indices, G)
    else:
        _, arg = sage_ref.max_forward(indptr, indices, Q, R)
        assert (arg[np.diff(indptr) == 0] == -1).all()
        dQ = sage_ref.max_backward(indptr, indices, G, arg)
        cnt, mag = sage_ref.max_backward_terms(indptr, indices, G, arg)
        assert cnt.sum() == (arg >= 0).sum() and np.all(np.abs(dQ) <= mag + 1e-15)
        assert np.isinf(sage_ref.max_margin(indptr, indices, Q)[np.diff(indptr) < 2]).all()
    h = 1e-6
    for name, an, which in (("dQ", dQ, 0), ("dR", G, 1)):
        num = np.zeros((n, d))
        for i in range(n):
            for c in range(d):
                args = [[Q.copy(), R.copy()] for _ in range(2)]
                args[0][which][i, c] += h
                args[1][which][i, c] -= h
                num[i, c] = (value(*args[0]) - value(*args[1])) / (2 * h)
        assert np.abs(num - an).max() <= 1e-6 * np.abs(an).max(), name


def test_max_forward_takes_the_lowest_slot():
    indptr = np.array([0, 3, 3, 5])
    indices = np.array([1, 2, 2, 0, 1])
    Q = np.array([[1.0, -0.0], [3.0, 0.0], [3.0, -0.0]], np.float32)
    Z, arg = sage_ref.max_forward(indptr, indices, Q)
    assert arg.tolist() == [[0, 0], [-1, -1], [4, 3]]
    assert Z[0, 0] == 3.0 and not np.signbit(Z[0, 1]) and np.signbit(Z[2, 1])
    gap = sage_ref.max_margin(indptr, indices, Q)
    assert gap[0, 0] == 0.0 and np.isinf(gap[1]).all() and gap[2, 0] == 2.0


CASES = [("cora", (16,), agg, root, {}) for agg in ("mean", "max") for root in (False, True)] + \
        [("cora", (16, 16), agg, True, dict(residual=True, layer_norm=True))
         for agg in ("mean", "max")] + \
        [("cora", (8, 8), agg, True, dict(residual=True)) for agg in ("mean", "max")] + \
        [("cora-directed", (16,), agg, True, {}) for agg in ("mean", "max")]


@pytest.mark.parametrize("name,hidden,agg,root,kw", CASES)
def test_seeds_of_the_gpu_parity_tests(loaded, pgcn, name, hidden, agg, root, kw):
    """With the reference model alone: a seed in 0..15 keeps every ReLU argument and max margin
    2e-6 away from a flip, and the elements test_gpu_sage.py leaves out of a max layer's
    comparison (top two within 1e-5 max|Q|, not an exact tie) stay below 1 % per layer."""
    import test_gpu_sage as T
    ds = T.directed_cora(pgcn, loaded["cora"]) if name == "cora-directed" else loaded[name]
    seed, ep = T.flip_free(pgcn, ds, hidden, (0.5,) * (len(hidden) + 1), agg, root, **kw)
    assert ep["close"] >= T.FLIP and max(ep["share"]) < T.CAP
    assert np.isfinite(ep["line"]).all()
