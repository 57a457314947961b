"""The residual model's host-only side (no GPU): the `residual` member of pgcn_params in step
between the C struct and the Python glue, and the checkpoint header's flags word (bit 0:
residual; unknown bits refused) read by pgcn_checkpoint_info / pgcn_checkpoint_flags from files
written here in INTEGRATION.md's layout.
"""
import ctypes
import struct

import numpy as np
import pytest

HEADER = "<8sIIq18i16fIIqqqqq"  # ... then the u64 checksum: 216 bytes in all


def fnv1a(data, h=14695981039346656037):
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def make_checkpoint(flags, dims=(5, 4, 4, 3), num_nodes=10, seed=7, dropouts=(0.5, 0.25, 0.25),
                    adam_steps=2, draw_epochs=2, epochs=2, rows=2):
    """INTEGRATION.md's layout with the given flags word: header (FNV-1a over its first 208
    bytes and the payload), then results, weights, m, v as float32."""
    L = len(dims) - 1
    n_w = sum(a * b for a, b in zip(dims, dims[1:]))
    rng = np.random.default_rng(3)
    payload = b"".join(rng.standard_normal(k).astype("<f4").tobytes()
                       for k in (rows * 4, n_w, n_w, n_w))
    head = struct.pack(HEADER, b"PGCNCK01", 1, L, num_nodes,
                       *(list(dims) + [0] * (18 - len(dims))),
                       *(list(dropouts) + [0.0] * (16 - len(dropouts))), seed, flags, adam_steps,
                       draw_epochs, epochs, rows, n_w)
    assert len(head) == 208
    return head + struct.pack("<Q", fnv1a(head + payload)) + payload


def test_params_default_and_layout(pgcn):
    p = pgcn.PgcnParams()
    p.residual = 77
    pgcn.lib.pgcn_params_default(ctypes.byref(p))
    assert p.residual == 0 and p.n_layers == 2 and p.reassociate_last == 1
    assert ctypes.sizeof(pgcn.PgcnParams) == pgcn.lib.pgcn_params_sizeof()
    # the last member: nothing of the C struct lies behind it
    assert pgcn.PgcnParams.residual.offset + ctypes.sizeof(ctypes.c_int) == \
        ctypes.sizeof(pgcn.PgcnParams)
    assert pgcn.PgcnParams._fields_[-1][0] == "residual"


def test_make_params_sets_residual(pgcn):
    class Ds:  # make_params reads the three sizes only
        num_nodes, input_dim, output_dim = 10, 5, 3
    assert pgcn.make_params(Ds).residual == 0
    p = pgcn.make_params(Ds, hidden_dims=(4, 4), dropouts=(0.5,) * 3, residual=True)
    assert p.residual == 1 and p.n_layers == 3


def test_checkpoint_flags_word(pgcn, tmp_path):
    plain, res, unknown, both = (tmp_path / n for n in ("plain", "res", "unknown", "both"))
    plain.write_bytes(make_checkpoint(0))
    res.write_bytes(make_checkpoint(1))
    unknown.write_bytes(make_checkpoint(2))
    both.write_bytes(make_checkpoint(3))
    assert pgcn.checkpoint_flags(str(plain)) == 0
    assert pgcn.checkpoint_info(str(res))["n_layers"] == 3  # OK: a known flag
    assert pgcn.checkpoint_flags(str(res)) == 1 == pgcn.CKPT_RESIDUAL
    for bad in (unknown, both):
        for fn in (pgcn.checkpoint_info, pgcn.checkpoint_flags):
            with pytest.raises(pgcn.PgcnError) as e:
                fn(str(bad))
            assert e.value.status == pgcn.PGCN_E_IO
    with pytest.raises(pgcn.PgcnError) as e:
        pgcn.checkpoint_flags(str(tmp_path / "missing"))
    assert e.value.status == pgcn.PGCN_E_IO
    assert pgcn.lib.pgcn_checkpoint_flags(None) == pgcn.PGCN_E_INVALID


def test_residual_kernel_entries_without_device(pgcn):
    """No CPU fallback: without a HIP device the two kernel ABI entries answer with a status."""
    import torch
    if torch.cuda.is_available():
        return  # with a device they are covered by tests/test_gpu_residual.py
    a = np.zeros(4, np.float32)
    vp = a.ctypes.data_as(ctypes.c_void_p)
    assert pgcn.lib.pgcn_residual_fwd(vp, vp, 4, None) == pgcn.PGCN_E_NODEVICE
    assert pgcn.lib.pgcn_residual_bwd(vp, vp, 4, None) == pgcn.PGCN_E_NODEVICE
