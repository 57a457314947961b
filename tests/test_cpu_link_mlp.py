"""Host-only parts of the Hadamard-MLP link decoder (no device): the kernel ABI's host entries,
make_params' validation of link_hidden, and pgcn_checkpoint_link_hidden on hand-written headers."""
import ctypes
import struct

import numpy as np
import pytest


def test_tile_and_exports(pgcn):
    t = ctypes.c_int()
    pgcn.lib.pgcn_link_mlp_tile(ctypes.byref(t))
    assert t.value == 64
    pgcn.lib.pgcn_link_mlp_tile(None)
    for name in ("pgcn_link_mlp_tile", "pgcn_link_mlp_workspace", "pgcn_link_mlp_fwd",
                 "pgcn_link_mlp_bwd", "pgcn_checkpoint_link_hidden"):
        assert name in pgcn.EXPORTED and hasattr(pgcn.lib, name)
    assert {"link_mlp_fwd", "link_mlp_bwd"} <= set(pgcn.KERNEL_PATHS)
    assert ctypes.sizeof(pgcn.PgcnParams) == pgcn.lib.pgcn_params_sizeof()


def test_null_arguments_are_invalid(pgcn):
    lib = pgcn.lib
    assert lib.pgcn_link_mlp_workspace(None, 8, 8) == -1
    assert lib.pgcn_link_mlp_fwd(None, None, 8, 8, None, 8, 8, None, 4, None) == -1
    assert lib.pgcn_link_mlp_bwd(None, None, 8, 8, None, 8, 8, None, 4, None, 8, None, 8, None, 0,
                                 None) == -1


class _Ds:
    num_nodes, input_dim, output_dim = 10, 4, 8


def test_make_params_validation(pgcn):
    p = pgcn.make_params(_Ds, link_decoder="dot", link_hidden=64)
    assert (p.link_decoder, p.link_hidden) == (1, 64)
    assert pgcn.make_params(_Ds, link_decoder="dot").link_hidden == 0
    assert pgcn.make_params(_Ds).link_hidden == 0
    for kw in (dict(link_hidden=8), dict(link_decoder="dot", link_hidden=-1),
               dict(link_decoder="dot", link_hidden=129), dict(link_decoder="dot", link_hidden=2.5)):
        with pytest.raises(ValueError):
            pgcn.make_params(_Ds, **kw)


def _v9(hidden, extra=None, version=9, dims=(5, 4, 4, 3)):
    """test_cpu_link's version-8 bytes with `hidden` in the link block's spare word and `extra`
    more weights (default: the decoder tensor's) in each of the three payload arrays."""
    from test_cpu_link import _v8
    from test_cpu_residual import fnv1a
    blob, n_w = _v8(zero=hidden, version=version, dims=dims)
    if extra is None:
        extra = (dims[-1] + 3) * ((hidden + 3) // 4 * 4) if hidden else 0
    head, ext = bytearray(blob[:208]), blob[216:216 + 64]
    struct.pack_into("<q", head, 200, n_w + extra)
    payload = np.arange(8 + 3 * (n_w + extra)).astype("<f4").tobytes()
    head = bytes(head)
    return head + struct.pack("<Q", fnv1a(head + ext + payload)) + ext + payload


def test_checkpoint_link_hidden(pgcn, tmp_path):
    """Version 9 = version 8 with link_hidden in the block's spare word and the decoder tensor in
    the payload; versions up to 8 read as 0 and keep requiring 0 there."""
    def put(blob):
        path = tmp_path / "f.pgcnck"
        path.write_bytes(blob)
        return str(path)
    for h in (1, 5, 64, 128):
        path = put(_v9(h))
        assert pgcn.checkpoint_link_hidden(path) == h
        assert pgcn.checkpoint_links(path) == (1, 1200)
        assert pgcn.checkpoint_info(path)["version"] == 9
    assert pgcn.checkpoint_link_hidden(put(_v9(0, version=8))) == 0
    bad = {"hidden 0 in version 9": _v9(0), "hidden 129": _v9(129),
           "hidden in version 8": _v9(8, version=8), "no decoder tensor": _v9(8, extra=0),
           "a short decoder tensor": _v9(5, extra=(3 + 3) * 5), "truncated": _v9(8)[:-4]}
    for name, blob in bad.items():
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.checkpoint_link_hidden(put(blob))
        assert e.value.status == pgcn.PGCN_E_IO, name
