"""LayerNorm's host-only side (no GPU): the `layer_norm` member of pgcn_params in step between
the C struct and the Python glue, the version-2 checkpoint (flags bit 1, the scale / shift
tensor counted in n_weights) read by pgcn_checkpoint_info / pgcn_checkpoint_flags from files
written here in INTEGRATION.md's layout, and the kernel entries' answer without a device.
"""
import ctypes
import struct

import numpy as np
import pytest

from test_cpu_residual import HEADER, fnv1a


def make_checkpoint(version, flags, with_norm, dims=(5, 4, 4, 3), num_nodes=10, seed=7,
                    dropouts=(0.5, 0.25, 0.25), rows=2):
    """The layout of test_cpu_residual.make_checkpoint with the version word and, with_norm, the
    scale / shift tensor (2 * sum of the hidden dims floats) counted behind the layer weights."""
    L = len(dims) - 1
    n_w = sum(a * b for a, b in zip(dims, dims[1:]))
    if with_norm:
        n_w += 2 * sum(dims[1:-1])
    rng = np.random.default_rng(3)
    payload = b"".join(rng.standard_normal(k).astype("<f4").tobytes()
                       for k in (rows * 4, n_w, n_w, n_w))
    head = struct.pack(HEADER, b"PGCNCK01", version, L, num_nodes,
                       *(list(dims) + [0] * (18 - len(dims))),
                       *(list(dropouts) + [0.0] * (16 - len(dropouts))), seed, flags, 2, 2, 2,
                       rows, n_w)
    assert len(head) == 208
    return head + struct.pack("<Q", fnv1a(head + payload)) + payload, n_w


def test_params_layout_and_default(pgcn):
    p = pgcn.PgcnParams()
    p.layer_norm = 77
    pgcn.lib.pgcn_params_default(ctypes.byref(p))
    assert p.layer_norm == 0 and p.residual == 0
    assert ctypes.sizeof(pgcn.PgcnParams) == pgcn.lib.pgcn_params_sizeof()
    names = [f[0] for f in pgcn.PgcnParams._fields_]
    assert names[-2:] == ["layer_norm", "residual"]
    assert pgcn.PgcnParams.layer_norm.offset + ctypes.sizeof(ctypes.c_int) == \
        pgcn.PgcnParams.residual.offset
    assert pgcn.PgcnParams.seed.offset + ctypes.sizeof(ctypes.c_uint) == \
        pgcn.PgcnParams.layer_norm.offset


def test_make_params_sets_layer_norm(pgcn):
    class Ds:  # make_params reads the three sizes only
        num_nodes, input_dim, output_dim = 10, 5, 3
    assert pgcn.make_params(Ds).layer_norm == 0
    p = pgcn.make_params(Ds, hidden_dims=(4, 4), dropouts=(0.5,) * 3, layer_norm=True)
    assert p.layer_norm == 1 and p.residual == 0 and p.n_layers == 3
    p = pgcn.make_params(Ds, hidden_dims=(4, 4), dropouts=(0.5,) * 3, residual=True)
    assert p.layer_norm == 0 and p.residual == 1


def test_version2_checkpoint(pgcn, tmp_path):
    def write(name, *args):
        blob, n_w = make_checkpoint(*args)
        path = tmp_path / name
        path.write_bytes(blob)
        return str(path), n_w
    assert pgcn.CKPT_LAYERNORM == 2
    for flags in (2, 3):  # LayerNorm, LayerNorm + residual
        path, n_w = write(f"v2_{flags}", 2, flags, True)
        info = pgcn.checkpoint_info(path)
        assert info["version"] == 2 and info["n_layers"] == 3
        assert info["weights"] == n_w == 5 * 4 + 4 * 4 + 4 * 3 + 2 * (4 + 4)
        assert pgcn.checkpoint_flags(path) == flags
    plain, n_w = write("v1", 1, 1, False)
    assert pgcn.checkpoint_info(plain)["version"] == 1
    assert pgcn.checkpoint_info(plain)["weights"] == n_w == 48
    bad = [write("v2_short", 2, 2, False)[0],     # n_weights lacks the norm tensor
           write("v2_nobit", 2, 0, False)[0],     # version 2 is the LayerNorm file
           write("v2_nobit_n", 2, 1, True)[0],
           write("v2_unknown", 2, 6, True)[0],    # bit 2 is unknown
           write("v1_bit1", 1, 2, False)[0],      # bit 1 stays unknown in a version-1 file
           write("v1_bit1_n", 1, 2, True)[0],
           write("v1_long", 1, 0, True)[0],
           write("v3", 3, 2, True)[0]]
    for path in bad:
        for fn in (pgcn.checkpoint_info, pgcn.checkpoint_flags):
            with pytest.raises(pgcn.PgcnError) as e:
                fn(path)
            assert e.value.status == pgcn.PGCN_E_IO, path


def test_layernorm_kernel_entries_without_device(pgcn):
    """No CPU fallback: without a HIP device the kernel ABI entries answer with a status; bad
    arguments are refused before the device is looked for."""
    raw = np.zeros(64 + 4, np.float32)
    a = raw[(-raw.ctypes.data % 16) // 4:][:64]  # rows on the 16-byte grid
    vp = a.ctypes.data_as(ctypes.c_void_p)
    lib = pgcn.lib
    assert lib.pgcn_layernorm_fwd(vp, 4, vp, 4, 4, 1025, vp, vp, 1e-5, None, 0, None, None) == \
        pgcn.PGCN_E_INVALID
    assert lib.pgcn_layernorm_fwd(vp, 6, vp, 8, 4, 4, vp, vp, 1e-5, None, 0, None, None) == \
        pgcn.PGCN_E_INVALID
    assert lib.pgcn_layernorm_bwd(vp, 4, vp, 4, vp, vp, 4, 4, None, 4, vp, vp, vp, None) == \
        pgcn.PGCN_E_INVALID
    assert lib.pgcn_layernorm_bwd_workspace(4097, 128) > 0
    assert lib.pgcn_layernorm_bwd_workspace(4, 1025) == 0
    import torch
    if torch.cuda.is_available():
        return  # with a device they are covered by tests/test_gpu_layernorm.py
    assert a.ctypes.data % 16 == 0
    assert lib.pgcn_layernorm_fwd(vp, 4, vp, 4, 4, 4, vp, vp, 1e-5, None, 0, None, None) == \
        pgcn.PGCN_E_NODEVICE
    assert lib.pgcn_layernorm_bwd(vp, 4, vp, 4, vp, vp, 4, 4, vp, 4, vp, vp, vp, None) == \
        pgcn.PGCN_E_NODEVICE
    assert lib.pgcn_debug_layernorm_fwd_tail(vp, 4, vp, 4, 4, 4, vp, vp, 1e-5, None, 0, None, vp,
                                             4, None, 0, None, 0, 1.0, None) == \
        pgcn.PGCN_E_NODEVICE
