"""Graph attention's host-only side (no GPU): the `attention` member of pgcn_params in step
between the C struct and the Python glue, the pgcn_gat_* entries' argument checks without a
device, the version-4 checkpoint header, and the float64 reference of tests/gat_ref.py itself
against central differences -- the yardstick the GPU tests rely on.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import gat_ref
import helpers
from test_cpu_layernorm import make_checkpoint


def test_params_layout_and_default(pgcn):
    """`attention` sits between eps and reassociate_last in the Python struct and in the header's
    text; the sizes agree; pgcn_params_default writes 0 over a poisoned struct."""
    P = pgcn.PgcnParams
    names = [f[0] for f in P._fields_]
    i = names.index("attention")
    assert names[i - 1] == "eps" and names[i + 1] == "reassociate_last"
    assert names[-5:] == ["reassociate_last", "multilabel", "seed", "layer_norm", "residual"]
    assert P.eps.offset + ctypes.sizeof(ctypes.c_float) == P.attention.offset
    assert P.attention.offset + ctypes.sizeof(ctypes.c_int) == P.reassociate_last.offset
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
    assert p.attention == 0 and p.reassociate_last == 1 and p.layer_norm == 0 and p.residual == 0


def test_make_params_sets_attention(pgcn):
    class Ds:  # make_params reads the three sizes only
        num_nodes, input_dim, output_dim = 10, 5, 3
    assert pgcn.make_params(Ds).attention == 0
    p = pgcn.make_params(Ds, hidden_dims=(4, 4), dropouts=(0.5,) * 3, attention=True)
    assert p.attention == 1 and p.layer_norm == 0 and p.residual == 0 and p.multilabel == 0
    p = pgcn.make_params(Ds, layer_norm=True, multilabel=True)
    assert p.attention == 0 and p.layer_norm == 1 and p.multilabel == 1


def test_gat_entries_argument_checks(pgcn):
    """The symbols exist; bad d, bad ld and null pointers are PGCN_E_INVALID before the device
    is looked for (this machine may have none)."""
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    for name in ("pgcn_gat_scores", "pgcn_gat_fwd", "pgcn_gat_bwd_workspace", "pgcn_gat_bwd"):
        assert hasattr(lib, name) and name in pgcn.EXPORTED
    raw = np.zeros(4 * 132 + 4, np.float32)
    a = raw[(-raw.ctypes.data % 16) // 4:][:4 * 132]  # rows on the 16-byte grid
    vp = a.ctypes.data_as(ctypes.c_void_p)

    def scores(ld=4, n=4, d=4, P=vp, ad=vp, as_=vp, u=vp, v=vp):
        return lib.pgcn_gat_scores(P, ld, n, d, ad, as_, u, v, None)
    assert scores(d=0) == INV and scores(d=129, ld=132) == INV and scores(d=-1) == INV
    assert scores(ld=6, d=4) == INV and scores(ld=4, d=5) == INV and scores(ld=0) == INV
    assert scores(n=-1) == INV
    for null in ("P", "ad", "as_", "u", "v"):
        assert scores(**{null: None}) == INV, null
    assert scores(n=0) == pgcn.PGCN_OK and scores(n=0, P=None) == pgcn.PGCN_OK

    def fwd(g=None, ld_p=4, ld_z=4, d=4, P=vp, u=vp, v=vp, Z=vp):
        return lib.pgcn_gat_fwd(g, P, ld_p, u, v, 0.2, Z, ld_z, d, None, None)
    # (a graph handle needs a device: without one every call ends at the null handle at the latest)
    assert fwd() == INV and fwd(d=0) == INV and fwd(d=129, ld_p=132, ld_z=132) == INV
    assert fwd(ld_p=6) == INV and fwd(ld_z=2) == INV and fwd(P=None) == INV and fwd(Z=None) == INV

    def bwd(g=None, ld=4, ld_dp=4, d=4, dP=vp, da=vp, ws=vp):
        return lib.pgcn_gat_bwd(g, vp, ld, vp, vp, 0.2, vp, vp, ld, vp, ld, vp, vp, dP, ld_dp, d,
                                da, ws, None)
    assert bwd() == INV and bwd(d=0) == INV and bwd(d=129, ld=132, ld_dp=132) == INV
    assert bwd(ld=6) == INV and bwd(ld_dp=7) == INV
    assert bwd(dP=None) == INV and bwd(da=None) == INV and bwd(ws=None) == INV
    assert lib.pgcn_gat_bwd_workspace(None, 16) == 0
    import torch
    if torch.cuda.is_available():
        return  # with a device the launches are covered by tests/test_gpu_gat_kernels.py
    assert scores() == pgcn.PGCN_E_NODEVICE


def test_version4_checkpoint(pgcn, tmp_path):
    """Version 4 = flags bit 3, the attention tensor (2 * (hidden dims + output dim) floats)
    counted last in n_weights, bits 0-3 known; in versions 1-3 bit 3 stays unknown."""
    def write(name, version, flags, n_extra, with_norm):
        blob, n_w = _checkpoint(version, flags, n_extra, with_norm)
        path = tmp_path / name
        path.write_bytes(blob)
        return str(path), n_w
    assert pgcn.CKPT_ATTENTION == 8
    n_attn, base = 2 * (4 + 4 + 3), 5 * 4 + 4 * 4 + 4 * 3
    for flags in (8, 9, 10, 12, 15):
        path, n_w = write(f"v4_{flags}", 4, flags, n_attn, bool(flags & 2))
        info = pgcn.checkpoint_info(path)
        assert info["version"] == 4 and info["n_layers"] == 3
        assert info["weights"] == n_w == base + n_attn + (16 if flags & 2 else 0)
        assert pgcn.checkpoint_flags(path) == flags
    bad = [write("v4_nobit", 4, 2, 0, True)[0],       # version 4 is the attention file
           write("v4_short", 4, 8, 0, False)[0],      # n_weights lacks the attention tensor
           write("v4_unknown", 4, 24, n_attn, False)[0],
           write("v1_bit3", 1, 8, n_attn, False)[0],  # bit 3 stays unknown in versions 1-3
           write("v1_bit3_s", 1, 8, 0, False)[0],
           write("v2_bit3", 2, 10, n_attn, True)[0],
           write("v3_bit3", 3, 14, n_attn, True)[0],
           write("v5", 5, 8, n_attn, False)[0]]
    for path in bad:
        for fn in (pgcn.checkpoint_info, pgcn.checkpoint_flags):
            with pytest.raises(pgcn.PgcnError) as e:
                fn(path)
            assert e.value.status == pgcn.PGCN_E_IO, path


def _checkpoint(version, flags, n_extra, with_norm):
    """test_cpu_layernorm.make_checkpoint's file with n_extra more floats per payload tensor."""
    import struct

    from test_cpu_residual import HEADER, fnv1a
    blob, n_w = make_checkpoint(version, flags, with_norm)
    head = bytearray(blob[:208])
    rows = struct.unpack_from("<q", head, 192)[0]
    assert struct.unpack_from("<q", head, 200)[0] == n_w and struct.calcsize(HEADER) == 208
    struct.pack_into("<q", head, 200, n_w + n_extra)
    rng = np.random.default_rng(5)
    payload = b"".join(rng.standard_normal(k).astype("<f4").tobytes()
                       for k in (rows * 4, n_w + n_extra, n_w + n_extra, n_w + n_extra))
    head = bytes(head)
    return head + struct.pack("<Q", fnv1a(head + payload)) + payload, n_w + n_extra


# --------------------------------------------------------------------------- the reference
def small_directed_graph():
    """12 nodes, directed: self loops on most rows, row 5 empty, the edge 2 -> 7 twice, column
    11 without an incoming slot."""
    adj = {0: [0, 3, 4], 1: [1, 0], 2: [2, 7, 7, 9], 3: [3, 1, 8, 10, 6], 4: [4, 2], 5: [],
           6: [6, 5, 0, 1], 7: [7, 3], 8: [2, 4, 9], 9: [9, 8, 1], 10: [10, 0, 6, 5, 3],
           11: [4, 8]}
    indptr = np.zeros(13, np.int32)
    indices = []
    for i in range(12):
        indices += adj[i]
        indptr[i + 1] = len(indices)
    return indptr, np.asarray(indices, np.int32)


def test_reference_gradients_against_central_differences():
    """The analytic dP, da_dst, da_src of gat_ref.gat_backward against central differences of
    sum(G * Z) in float64: relative difference (largest absolute difference over the largest
    analytic value of the tensor) below 1e-6."""
    indptr, indices = small_directed_graph()
    n, d = 12, 3
    assert indptr[6] == indptr[5] and 11 not in indices
    rng = np.random.default_rng(11)
    P = rng.standard_normal((n, d))
    a_dst, a_src = rng.standard_normal(d), rng.standard_normal(d)
    G = rng.standard_normal((n, d))
    fwd = gat_ref.gat_forward(indptr, indices, P, a_dst, a_src)
    assert np.abs(fwd["x"]).min() > 1e-3  # no slot near the LeakyReLU's kink
    np.testing.assert_array_equal(fwd["Z"][5], np.zeros(d))
    sums = np.bincount(fwd["rows"], weights=fwd["alpha"], minlength=n)
    np.testing.assert_allclose(np.delete(sums, 5), 1.0, rtol=1e-12)
    got = gat_ref.gat_backward(fwd, indptr, indices, P, a_dst, a_src, G)

    def loss(P_, ad, as_):
        return float((G * gat_ref.gat_forward(indptr, indices, P_, ad, as_)["Z"]).sum())

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
        print(f"{key}: relative difference {rel:.3g}")
        assert rel < 1e-6, key
    # a column without an incoming slot: dP_j = du_j a_dst exactly
    np.testing.assert_array_equal(got["dv"][11], 0.0)
    np.testing.assert_allclose(got["dP"][11], got["du"][11] * a_dst, rtol=1e-15)


def test_reference_float32_mode_is_close():
    """The float32 run of the same statements (the tolerance rule's measure) stays within 1e-5
    of float64 on this graph."""
    indptr, indices = small_directed_graph()
    rng = np.random.default_rng(12)
    P = rng.standard_normal((12, 3)).astype(np.float32)
    a_dst, a_src = (rng.standard_normal(3).astype(np.float32) for _ in range(2))
    f64 = gat_ref.gat_forward(indptr, indices, P, a_dst, a_src)
    f32 = gat_ref.gat_forward(indptr, indices, P, a_dst, a_src, dtype=np.float32)
    assert f32["Z"].dtype == np.float32
    np.testing.assert_allclose(f32["Z"], f64["Z"], rtol=1e-5, atol=1e-6)


def test_xorshift_matches_the_oracle():
    """gat_ref.Xorshift (the reference's dropout draws) against the C oracle's or_rng_next."""
    lib = helpers.oracle()
    s = (ctypes.c_uint64 * 2)(0x1234567, 0x89abcdef)
    mine = gat_ref.Xorshift([s[0], s[1]]).draws(200)
    want = [lib.or_rng_next(s) for _ in range(200)]
    np.testing.assert_array_equal(mine, np.asarray(want, np.int64))
