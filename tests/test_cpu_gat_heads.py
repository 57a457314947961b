"""Multi-head graph attention's host-only side (no GPU): the attention_heads /
attention_dropout members of pgcn_params in step between the C struct and the Python glue, the
pgcn_gat_*_mh entries' argument checks without a device, the version-5 checkpoint header, and
the float64 reference of tests/gat_heads_ref.py itself -- against central differences under a
fixed mask, and against tests/gat_ref.py at one head -- the yardstick the GPU tests rely on.
"""
import ctypes
import os
import re
import struct

import numpy as np
import pytest

import gat_heads_ref as ref_mh
import gat_ref
import helpers
from test_cpu_gat import small_directed_graph
from test_cpu_layernorm import make_checkpoint
from test_cpu_residual import HEADER, fnv1a


def test_params_layout_and_default(pgcn):
    """attention_heads (int) and attention_dropout (float) sit between early_stopping and
    learning_rate in the Python struct and in the header's text; the sizes agree;
    pgcn_params_default writes 1 and 0 over a poisoned struct."""
    P = pgcn.PgcnParams
    names = [f[0] for f in P._fields_]
    i = names.index("attention_heads")
    assert names[i - 1] == "early_stopping" and names[i + 1] == "attention_dropout"
    assert names[i + 2] == "learning_rate"
    assert dict(P._fields_)["attention_heads"] is ctypes.c_int
    assert dict(P._fields_)["attention_dropout"] is ctypes.c_float
    assert P.early_stopping.offset + 4 == P.attention_heads.offset
    assert P.attention_heads.offset + 4 == P.attention_dropout.offset
    assert P.attention_dropout.offset + 4 == P.learning_rate.offset
    assert ctypes.sizeof(P) == pgcn.lib.pgcn_params_sizeof()
    text = open(os.path.join(helpers.REPO, "include", "pgcn.h")).read()
    body = text[text.index("typedef struct {\n  int num_nodes"):text.index("} pgcn_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = re.findall(r"((?:unsigned )?(?:int|float)) ([^;]+);", body)
    members = [m for _, decl in decls
               for m in re.sub(r"\[[^\]]*\]", "", decl).replace(" ", "").split(",")]
    assert members == names
    types = {m: t for t, decl in decls
             for m in re.sub(r"\[[^\]]*\]", "", decl).replace(" ", "").split(",")}
    assert types["attention_heads"] == "int" and types["attention_dropout"] == "float"
    p = P()
    ctypes.memset(ctypes.byref(p), 0x5A, ctypes.sizeof(p))
    pgcn.lib.pgcn_params_default(ctypes.byref(p))
    assert p.attention_heads == 1 and p.attention_dropout == 0.0 and p.attention == 0
    assert p.early_stopping == 0 and p.learning_rate == np.float32(0.01)


def test_make_params(pgcn):
    class Ds:  # make_params reads the three sizes only
        num_nodes, input_dim, output_dim = 10, 5, 3
    p = pgcn.make_params(Ds)
    assert p.attention_heads == 1 and p.attention_dropout == 0.0 and p.attention == 0
    p = pgcn.make_params(Ds, hidden_dims=(64,), attention=True, attention_heads=8,
                         attention_dropout=0.6)
    assert p.attention == 1 and p.attention_heads == 8
    assert p.attention_dropout == np.float32(0.6) and p.learning_rate == np.float32(0.01)


def _v5(heads=2, p=0.5, zero=0, version=5, flags=8, dims=(5, 8, 8, 3), ext=True, hashed=True):
    """A checkpoint file in Python: the 208 header bytes, the checksum, [the 16-byte extension
    {u32 heads; f32 dropout; u64 zero}], the payload (with the attention tensor counted last);
    the checksum runs over the header bytes, the extension (hashed) and the payload."""
    L = len(dims) - 1
    n_w = sum(a * b for a, b in zip(dims, dims[1:])) + (2 * sum(dims[1:]) if flags & 8 else 0)
    rng = np.random.default_rng(4)
    payload = b"".join(rng.standard_normal(k).astype("<f4").tobytes()
                       for k in (2 * 4, n_w, n_w, n_w))
    head = struct.pack(HEADER, b"PGCNCK01", version, L, 10, *(list(dims) + [0] * (18 - len(dims))),
                       *([0.5] * L + [0.0] * (16 - L)), 7, flags, 2, 2, 2, 2, n_w)
    assert len(head) == 208
    e = struct.pack("<IfQ", heads, p, zero) if ext else b""
    return head + struct.pack("<Q", fnv1a(head + (e if hashed else b"") + payload)) + e + payload


def test_version5_checkpoint(pgcn, tmp_path):
    """Version 5 = the version-4 header and flags with the extension before the payload, under
    the checksum; checkpoint_attention reads it and gives (1, 0) for versions 1-4, which stay
    as they were."""
    def write(name, **kw):
        path = tmp_path / name
        path.write_bytes(_v5(**kw))
        return str(path)
    n_w = 5 * 8 + 8 * 8 + 8 * 3 + 2 * (8 + 8 + 3)
    for name, kw, want in (("k2", dict(heads=2, p=0.5), (2, 0.5)),
                           ("k1p", dict(heads=1, p=0.25), (1, 0.25)),
                           ("k2p0", dict(heads=2, p=0.0), (2, 0.0)),
                           ("k2f", dict(heads=2, p=0.5, flags=9), (2, 0.5))):
        path = write(name, **kw)
        info = pgcn.checkpoint_info(path)
        assert info["version"] == 5 and info["n_layers"] == 3 and info["weights"] == n_w
        assert pgcn.checkpoint_flags(path) == kw.get("flags", 8)
        assert pgcn.checkpoint_attention(path) == want
    bad = dict(
        defaults=dict(heads=1, p=0.0),              # that engine writes version 4
        heads0=dict(heads=0, p=0.5), heads33=dict(heads=33, p=0.5),
        heads3=dict(heads=3, p=0.5),                # does not divide the hidden width 8
        dh2=dict(heads=4, p=0.5),                   # head width 2
        p1=dict(heads=2, p=1.0), pneg=dict(heads=2, p=-0.5), pnan=dict(heads=2, p=float("nan")),
        reserved=dict(zero=1),
        unhashed=dict(hashed=False),                # the extension is under the checksum
        no_ext=dict(ext=False),                     # version 5 without it: 16 bytes short
        no_bit3=dict(flags=0), unknown_bit=dict(flags=24),
        v4_with_ext=dict(version=4),                # versions 1-4 carry none
        v6=dict(version=6))
    for name, kw in bad.items():
        path = write("bad_" + name, **kw)
        for fn in (pgcn.checkpoint_info, pgcn.checkpoint_flags, pgcn.checkpoint_attention):
            with pytest.raises(pgcn.PgcnError) as e:
                fn(path)
            assert e.value.status == pgcn.PGCN_E_IO, name
    # versions 1-4: read as before, (1, 0)
    v4 = write("v4", version=4, ext=False)
    assert pgcn.checkpoint_info(v4)["version"] == 4 and pgcn.checkpoint_attention(v4) == (1, 0.0)
    v1 = tmp_path / "v1"
    v1.write_bytes(make_checkpoint(1, 0, False)[0])
    v2 = tmp_path / "v2"
    v2.write_bytes(make_checkpoint(2, 2, True)[0])
    for path, version in ((v1, 1), (v2, 2)):
        assert pgcn.checkpoint_info(str(path))["version"] == version
        assert pgcn.checkpoint_attention(str(path)) == (1, 0.0)
    with pytest.raises(pgcn.PgcnError) as e:
        pgcn.checkpoint_attention(str(tmp_path / "missing"))
    assert e.value.status == pgcn.PGCN_E_IO


def test_model_with_one_head_and_no_attention_dropout_is_gat_ref(pgcn):
    """tests/gat_heads_ref.NumpyGatGCN at heads = 1, attn_p = 0 is tests/gat_ref.NumpyGatGCN
    (the same draws, the same numbers); with attention dropout the Dropout modules' masks of an
    epoch stay where they were and the epoch's block grows by nnz * K_l draws per layer."""
    ds = pgcn.Dataset.synthetic(60, 12, 4, 200, 5)
    hidden, dropouts = (8, 8), (0.5, 0.5, 0.5)
    dims = [ds.input_dim, 8, 8, ds.output_dim]
    rng = np.random.default_rng(6)
    w = [rng.standard_normal((a, b)) * 0.3 for a, b in zip(dims, dims[1:])]
    attn = rng.standard_normal(2 * sum(dims[1:])) * 0.3
    seed = [12345, 67890]

    def run(cls, epochs, **kw):
        m = cls(ds, hidden, [x.copy() for x in w], attn.copy(), dropouts, gat_ref.Xorshift(seed),
                **kw)
        out = []
        for _ in range(epochs):
            loss = m.forward(1, training=True)
            masks = [None if k is None else k.copy() for k in m.masks]
            keeps = [None if k is None else k.shape for k in getattr(m, "keep", [])]
            m.backward()
            m.step()
            out.append((loss, m.forward(2), masks, [x.copy() for x in m.dW], m.attn_grad(),
                        keeps))
        return m, out
    _, base = run(gat_ref.NumpyGatGCN, 2)
    _, same = run(ref_mh.NumpyGatGCN, 2, heads=1, attn_p=0.0)
    for a, b in zip(base, same):
        np.testing.assert_allclose(b[:2], a[:2], rtol=1e-12)
        for x, y in zip(a[3], b[3]):
            np.testing.assert_allclose(y, x, rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(b[4], a[4], rtol=1e-12, atol=1e-15)
    m, dropped = run(ref_mh.NumpyGatGCN, 2, heads=2, attn_p=0.5)
    for k, k0 in zip(dropped[0][2], base[0][2]):  # epoch 1: the same Dropout masks
        np.testing.assert_array_equal(k, k0)
    nnz = len(ds.graph_indices)
    assert dropped[0][5] == [(nnz, 2), (nnz, 2), (nnz, 1)] and same[0][5] == [None] * 3
    # epoch 2's input mask: behind epoch 1's block of nnz_X + 2 * 60 * 8 + nnz * (2 + 2 + 1) draws
    probe = gat_ref.Xorshift(seed)
    probe.draws(len(ds.feat_values) + 2 * 60 * 8 + 5 * nnz)
    want = probe.keep(len(ds.feat_values), 0.5) * 2.0
    np.testing.assert_array_equal(dropped[1][2][0], want)
    assert abs(dropped[0][0] - base[0][0]) > 1e-9  # the attention masks did change the model


def test_gat_mh_entries_argument_checks(pgcn):
    """The symbols exist; the head rules (heads < 1 or > 32, a head width of 2 / 12 / 24, heads
    not dividing d), bad d, bad ld, null pointers and a mask without alpha are PGCN_E_INVALID
    before the device is looked for (this machine may have none)."""
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    for name in ("pgcn_gat_scores_mh", "pgcn_gat_fwd_mh", "pgcn_gat_bwd_workspace_mh",
                 "pgcn_gat_bwd_mh"):
        assert hasattr(lib, name) and name in pgcn.EXPORTED
    assert "gat_heads" in pgcn.KERNEL_PATHS and pgcn.path_counts()["gat_heads"] == 0
    raw = np.zeros(4 * 132 + 4, np.float32)
    a = raw[(-raw.ctypes.data % 16) // 4:][:4 * 132]  # rows on the 16-byte grid
    vp = a.ctypes.data_as(ctypes.c_void_p)
    BAD_HEADS = ((8, 0), (8, -1), (8, 4), (24, 2), (48, 2), (16, 3), (128, 64), (6, 2), (2, 2))

    def scores(ld=128, n=4, d=8, K=2, P=vp, ad=vp, as_=vp, u=vp, v=vp):
        return lib.pgcn_gat_scores_mh(P, ld, n, d, K, ad, as_, u, v, None)
    for d, K in BAD_HEADS:
        assert scores(d=d, K=K) == INV, (d, K)
    assert scores(d=0, K=1) == INV and scores(d=129, ld=132, K=1) == INV
    assert scores(ld=6) == INV and scores(ld=4) == INV and scores(n=-1) == INV
    for null in ("P", "ad", "as_", "u", "v"):
        assert scores(**{null: None}) == INV, null
    assert scores(n=0, P=None) == pgcn.PGCN_OK  # nothing to do: no device needed

    def fwd(g=None, ld=128, d=8, K=2, mask=None, alpha=vp):
        return lib.pgcn_gat_fwd_mh(g, vp, ld, vp, vp, 0.2, vp, ld, d, K, mask, 0, 1.0, alpha, None)
    assert fwd() == INV  # no graph
    for d, K in BAD_HEADS:
        assert fwd(d=d, K=K) == INV
    assert fwd(mask=vp, alpha=None) == INV and fwd(K=1, mask=vp, alpha=None) == INV

    def bwd(g=None, ld=128, d=8, K=2):
        return lib.pgcn_gat_bwd_mh(g, vp, ld, vp, vp, 0.2, vp, vp, ld, vp, ld, vp, vp, vp, ld, d,
                                   K, None, 0, 1.0, vp, vp, None)
    assert bwd() == INV
    for d, K in BAD_HEADS:
        assert bwd(d=d, K=K) == INV
    assert lib.pgcn_gat_bwd_workspace_mh(None, 16, 4) == 0
    import torch
    if torch.cuda.is_available():
        return  # with a device the launches are covered by tests/test_gpu_gat_heads_kernels.py
    # every width the rules admit passes the checks and reaches the search for a device
    for d, K in ((8, 2), (16, 4), (128, 32), (64, 8), (128, 8), (128, 2), (128, 1), (12, 3),
                 (3, 1)):
        assert scores(d=d, K=K) == pgcn.PGCN_E_NODEVICE, (d, K)


def _fixture(d, K, seed):
    indptr, indices = small_directed_graph()
    n, nnz = 12, len(indices)
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((n, d))
    a_dst, a_src = rng.standard_normal(d), rng.standard_normal(d)
    G = rng.standard_normal((n, d))
    keep = rng.random((nnz, K)) >= 0.4
    return indptr, indices, P, a_dst, a_src, G, keep


def test_reference_gradients_against_central_differences():
    """The analytic dP, da_dst, da_src of gat_backward_mh against central differences of
    sum(G * Z) in float64 under a fixed mask (scale 1 / 0.6), on the directed graph with a
    duplicated slot, an empty row and a column without an incoming slot, at d = 8, K = 2 and
    d = 16, K = 4: relative difference (largest absolute difference over the largest analytic
    value of the tensor) below 1e-6."""
    for d, K, seed in ((8, 2, 21), (16, 4, 22)):
        indptr, indices, P, a_dst, a_src, G, keep = _fixture(d, K, seed)
        n, scale = 12, 1.0 / 0.6
        assert 0 < keep.sum() < keep.size
        fwd = ref_mh.gat_forward_mh(indptr, indices, P, a_dst, a_src, K, keep=keep, scale=scale)
        assert np.abs(fwd["x"]).min() > 1e-3  # no slot near the LeakyReLU's kink
        np.testing.assert_array_equal(fwd["Z"][5], np.zeros(d))
        for h in range(K):
            sums = np.bincount(fwd["rows"], weights=fwd["alpha"][:, h], minlength=n)
            np.testing.assert_allclose(np.delete(sums, 5), 1.0, rtol=1e-12)
        got = ref_mh.gat_backward_mh(fwd, indptr, indices, P, a_dst, a_src, G)

        def loss(P_, ad, as_):
            f = ref_mh.gat_forward_mh(indptr, indices, P_, ad, as_, K, keep=keep, scale=scale)
            return float((G * f["Z"]).sum())

        def numeric(which):
            base = [P.copy(), a_dst.copy(), a_src.copy()]
            out = np.zeros_like(base[which])
            h = 1e-6
            for i in np.ndindex(out.shape):
                hi = [b.copy() for b in base]
                lo = [b.copy() for b in base]
                hi[which][i] += h
                lo[which][i] -= h
                out[i] = (loss(*hi) - loss(*lo)) / (2 * h)
            return out
        for which, key in ((0, "dP"), (1, "da_dst"), (2, "da_src")):
            want = numeric(which)
            rel = np.abs(got[key] - want).max() / np.abs(got[key]).max()
            print(f"d {d} K {K} {key}: relative difference {rel:.3g}")
            assert rel < 1e-6, (d, K, key)
        # a column without an incoming slot: dP_j[h] = du_j^h a_dst[h] exactly
        np.testing.assert_array_equal(got["dv"][11], 0.0)
        np.testing.assert_allclose(got["dP"][11], np.repeat(got["du"][11], d // K) * a_dst,
                                   rtol=1e-15)


def test_heads_are_independent_single_head_layers():
    """Head h of the K-head reference is gat_ref's single-head layer on the column slice."""
    d, K = 16, 4
    indptr, indices, P, a_dst, a_src, G, _ = _fixture(d, K, 23)
    fwd = ref_mh.gat_forward_mh(indptr, indices, P, a_dst, a_src, K)
    bwd = ref_mh.gat_backward_mh(fwd, indptr, indices, P, a_dst, a_src, G)
    for h in range(K):
        c = slice(h * 4, h * 4 + 4)
        f1 = gat_ref.gat_forward(indptr, indices, P[:, c], a_dst[c], a_src[c])
        b1 = gat_ref.gat_backward(f1, indptr, indices, P[:, c], a_dst[c], a_src[c], G[:, c])
        np.testing.assert_allclose(fwd["Z"][:, c], f1["Z"], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(fwd["alpha"][:, h], f1["alpha"], rtol=1e-12)
        np.testing.assert_allclose(bwd["dP"][:, c], b1["dP"], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(bwd["da_dst"][c], b1["da_dst"], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(bwd["da_src"][c], b1["da_src"], rtol=1e-12, atol=1e-15)


def test_one_head_without_mask_is_gat_ref():
    """K = 1 without a mask: gat_ref.gat_forward / gat_backward."""
    indptr, indices, P, a_dst, a_src, G, _ = _fixture(5, 1, 24)
    f1 = gat_ref.gat_forward(indptr, indices, P, a_dst, a_src)
    b1 = gat_ref.gat_backward(f1, indptr, indices, P, a_dst, a_src, G)
    fwd = ref_mh.gat_forward_mh(indptr, indices, P, a_dst, a_src, 1)
    bwd = ref_mh.gat_backward_mh(fwd, indptr, indices, P, a_dst, a_src, G)
    for k in ("u", "v", "x", "alpha"):
        np.testing.assert_allclose(fwd[k][:, 0], f1[k], rtol=1e-13, atol=1e-15, err_msg=k)
    np.testing.assert_allclose(fwd["Z"], f1["Z"], rtol=1e-13, atol=1e-15)
    for k in ("dP", "da_dst", "da_src"):
        np.testing.assert_allclose(bwd[k], b1[k], rtol=1e-12, atol=1e-15, err_msg=k)
    for k in ("du", "dv", "dx"):
        np.testing.assert_allclose(bwd[k][..., 0], b1[k], rtol=1e-12, atol=1e-15, err_msg=k)


def test_pack_bits():
    keep = np.array([1, 0, 1, 1, 0] * 30, bool)
    w = ref_mh.pack_bits(keep, base=61, fill=False)
    for e, k in enumerate(keep):
        b = 61 + e
        assert bool((int(w[b >> 6]) >> (b & 63)) & 1) == bool(k)
    assert int(w[0]) & ((1 << 61) - 1) == 0
