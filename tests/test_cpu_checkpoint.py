"""The checkpoint file's host-only side (no GPU): the documented format, written here from
Python, is what the library's parser accepts; damaged files are refused with PGCN_E_IO; the new
entry points answer with a status, not a crash, without an engine or a device.
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


def make_checkpoint(dims=(5, 4, 3), num_nodes=10, seed=7, dropouts=(0.5, 0.25), adam_steps=2,
                    draw_epochs=2, epochs=2, rows=2, version=1):
    """INTEGRATION.md's layout: header, then results, weights, m, v as float32."""
    L = len(dims) - 1
    n_w = sum(a * b for a, b in zip(dims, dims[1:]))
    rng = np.random.default_rng(3)
    payload = b"".join(rng.standard_normal(k).astype("<f4").tobytes()
                       for k in (rows * 4, n_w, n_w, n_w))
    head = struct.pack(HEADER, b"PGCNCK01", version, L, num_nodes,
                       *(list(dims) + [0] * (18 - len(dims))),
                       *(list(dropouts) + [0.0] * (16 - len(dropouts))), seed, 0, adam_steps,
                       draw_epochs, epochs, rows, n_w)
    assert len(head) == 208
    return head + struct.pack("<Q", fnv1a(head + payload)) + payload


def test_python_written_checkpoint_is_accepted(pgcn, tmp_path):
    path = tmp_path / "ok.pgcnck"
    path.write_bytes(make_checkpoint())
    info = pgcn.checkpoint_info(str(path))
    assert info == dict(version=1, n_layers=2, num_nodes=10, input_dim=5, output_dim=3,
                        adam_steps=2, epochs=2, weights=5 * 4 + 4 * 3)


def test_damaged_checkpoints_are_refused(pgcn, tmp_path):
    good = make_checkpoint()
    flipped = bytearray(good)
    flipped[-9] ^= 1  # a payload byte
    header_flip = bytearray(good)
    header_flip[20] ^= 1  # num_nodes: covered by the checksum too
    wrong_count = make_checkpoint(rows=3)  # more results rows than epochs
    cases = {"truncated": good[:-1], "trailing": good + b"\0", "flipped": bytes(flipped),
             "header": bytes(header_flip), "magic": b"PGCNCK02" + good[8:],
             "version": make_checkpoint(version=2), "rows": wrong_count,
             "short": good[:100], "empty": b""}
    for name, data in cases.items():
        path = tmp_path / name
        path.write_bytes(data)
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.checkpoint_info(str(path))
        assert e.value.status == pgcn.PGCN_E_IO, name
    with pytest.raises(pgcn.PgcnError) as e:
        pgcn.checkpoint_info(str(tmp_path / "missing"))
    assert e.value.status == pgcn.PGCN_E_IO


def test_new_entry_points_without_engine_or_device(pgcn, tmp_path):
    """A null engine is PGCN_E_INVALID; the kernel entries without a HIP device are
    PGCN_E_NODEVICE (no CPU fallback)."""
    lib = pgcn.lib
    w = np.zeros(4, np.float32)
    path = str(tmp_path / "x").encode()
    assert lib.pgcn_gcn_set_var(None, 2, 0, w.ctypes.data_as(ctypes.c_void_p), 4) == \
        pgcn.PGCN_E_INVALID
    assert lib.pgcn_gcn_save(None, path) == pgcn.PGCN_E_INVALID
    assert lib.pgcn_gcn_load(None, path, 0) == pgcn.PGCN_E_INVALID
    assert lib.pgcn_gcn_predict(None, None, None, None) == pgcn.PGCN_E_INVALID
    assert lib.pgcn_gcn_confusion(None, 3, None) == pgcn.PGCN_E_INVALID
    assert lib.pgcn_checkpoint_info(None, None) == pgcn.PGCN_E_INVALID
    import torch
    if torch.cuda.is_available():
        return  # with a device the kernel entries are covered by tests/test_gpu_predict.py
    assert lib.pgcn_predict_rows(None, 4, 1, 3, None, None, None, 4, None) == \
        pgcn.PGCN_E_NODEVICE
    assert lib.pgcn_confusion(None, None, 1, 3, None, None) == pgcn.PGCN_E_NODEVICE
