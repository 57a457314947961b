"""Neighbour sampling's host-only side (no GPU): the `fanout` member of pgcn_params, the new
entries' argument checks before the device is looked for, and the creation-time refusal."""
import ctypes

import numpy as np
import pytest


def test_params_layout(pgcn):
    P = pgcn.PgcnParams
    names = [f[0] for f in P._fields_]
    i = names.index("fanout")
    assert names[i - 1] == "batch_norm" and names[i + 1] == "link_hidden"
    assert P.batch_norm.offset + 4 == P.fanout.offset and P.fanout.offset + 4 == P.link_hidden.offset
    assert ctypes.sizeof(P) == pgcn.lib.pgcn_params_sizeof()
    p = P(fanout=9)
    pgcn.lib.pgcn_params_default(ctypes.byref(p))
    assert p.fanout == 0


def test_entries_argument_checks(pgcn):
    """Bad fanout, d, ld, mode and null handles are PGCN_E_INVALID before the device is looked for
    (a graph handle needs a device: without one every call ends at the null handle at the latest)."""
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    for name in ("pgcn_nbr_sample_create", "pgcn_nbr_sample_destroy", "pgcn_nbr_sample_draw",
                 "pgcn_nbr_sample_copy", "pgcn_nbr_agg_fwd", "pgcn_nbr_agg_bwd"):
        assert hasattr(lib, name) and name in pgcn.EXPORTED
    h = ctypes.c_void_p()
    for fanout in (0, 65, -1, 5):
        assert lib.pgcn_nbr_sample_create(None, fanout, ctypes.byref(h)) == INV and not h.value
    assert lib.pgcn_nbr_sample_draw(None, 1, 0, None) == INV
    assert lib.pgcn_nbr_sample_copy(None, None, None, None, None, None, None) == INV
    raw = np.zeros(4 * 132 + 4, np.float32)
    a = raw[(-raw.ctypes.data % 16) // 4:][:4 * 132]  # rows on the 16-byte grid
    vp = a.ctypes.data_as(ctypes.c_void_p)

    def fwd(mode=1, d=4, ld=4):
        return lib.pgcn_nbr_agg_fwd(None, mode, vp, ld, d, vp, ld, vp, ld, vp, ld, None)

    def bwd(mode=2, d=4, ld=4):
        return lib.pgcn_nbr_agg_bwd(None, mode, vp, ld, vp, ld, d, vp, ld, None)
    for f in (fwd, bwd):
        assert f() == INV and f(d=0) == INV and f(d=129, ld=132) == INV
        assert f(ld=6) == INV and f(d=5, ld=4) == INV and f(mode=0) == INV and f(mode=3) == INV


def test_fanout_needs_an_aggregator(pgcn):
    """Refused at creation, while the parameters are read, device or not; the edge-cut creators
    refuse a fanout engine as they refuse SAGE."""
    ds = pgcn.Dataset.synthetic(40, 6, 3, 80, 3)
    for kw, dist in ((dict(fanout=5), {}), (dict(fanout=65, aggregator="mean"), {}),
                     (dict(fanout=5, aggregator="mean"), dict(rank=0, world=1, unique_id=b"\0" * 128))):
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.GCN(pgcn.make_params(ds, hidden_dims=(8,), **kw), ds, **dist)
        assert e.value.status == pgcn.PGCN_E_INVALID
