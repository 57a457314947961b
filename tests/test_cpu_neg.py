"""Host-only parts of per-epoch negative sampling (no device): make_params' validation of
neg_ratio, the struct layout, and pgcn_checkpoint_neg_ratio on hand-written headers."""
import ctypes
import struct

import pytest


class _Ds:
    num_nodes, input_dim, output_dim = 10, 4, 8


def test_make_params_validation(pgcn):
    p = pgcn.make_params(_Ds, link_decoder="dot", neg_ratio=3)
    assert (p.link_decoder, p.neg_ratio) == (1, 3)
    assert pgcn.make_params(_Ds, link_decoder="dot").neg_ratio == 0
    for kw in (dict(neg_ratio=1), dict(link_decoder="dot", neg_ratio=-1),
               dict(link_decoder="dot", neg_ratio=65), dict(link_decoder="dot", neg_ratio=1.5)):
        with pytest.raises(ValueError):
            pgcn.make_params(_Ds, **kw)


def test_struct_layout(pgcn):
    P = pgcn.PgcnParams
    assert ctypes.sizeof(P) == pgcn.lib.pgcn_params_sizeof()
    assert P.link_hidden.offset + 4 == P.neg_ratio.offset == P.dropouts.offset - 4
    p = P()
    pgcn.lib.pgcn_params_default(ctypes.byref(p))
    assert p.neg_ratio == 0
    assert "pgcn_checkpoint_neg_ratio" in pgcn.EXPORTED


def _v10(ratio, hidden=0, block=None):
    """test_cpu_link_mlp's version-8 / -9 bytes as version 10: the fifth block behind the four."""
    from test_cpu_link_mlp import _v9
    from test_cpu_residual import fnv1a
    blob = _v9(hidden, version=10)
    head, ext, payload = blob[:208], blob[216:280], blob[280:]
    ext += struct.pack("<IIQ", ratio, 0, 0) if block is None else block
    return head + struct.pack("<Q", fnv1a(head + ext + payload)) + ext + payload


def test_checkpoint_neg_ratio(pgcn, tmp_path):
    from test_cpu_link_mlp import _v9

    def put(blob):
        path = tmp_path / "f.pgcnck"
        path.write_bytes(blob)
        return str(path)
    for ratio, hidden in ((1, 0), (2, 8), (64, 128)):
        path = put(_v10(ratio, hidden))
        assert pgcn.checkpoint_neg_ratio(path) == ratio
        assert pgcn.checkpoint_link_hidden(path) == hidden
        assert pgcn.checkpoint_links(path) == (1, 1200)
        assert pgcn.checkpoint_info(path)["version"] == 10
    assert pgcn.checkpoint_neg_ratio(put(_v9(8))) == 0
    assert pgcn.checkpoint_neg_ratio(put(_v9(0, version=8))) == 0
    bad = {"ratio 0": _v10(0), "ratio 65": _v10(65), "no block": _v9(0, version=10),
           "a spare word set": _v10(2, block=struct.pack("<IIQ", 2, 1, 0)),
           "truncated": _v10(2)[:-4]}
    for name, blob in bad.items():
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.checkpoint_neg_ratio(put(blob))
        assert e.value.status == pgcn.PGCN_E_IO, name
