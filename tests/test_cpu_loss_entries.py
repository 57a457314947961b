"""Host-side (no GPU) tests of the loss kernel family's debug entry points (include/pgcn.h):
every argument is checked before anything touches the device, so a bad call is PGCN_E_INVALID
and an empty one (n = 0) PGCN_OK on a host without one.

The pointers passed here are never dereferenced: every call is refused, or returns, first."""
import ctypes

P = 0x1000  # a non-null "device pointer" (never read: the calls below launch nothing)


def final(pgcn, **kw):
    f = pgcn.PgcnXentFinal()
    f.out2, f.ticket, f.part4, f.ring_cap = P, P, P, 1
    for k, v in kw.items():
        setattr(f, k, v)
    return f


def xent(pgcn, logits=P, ld=8, grad=P, truth=P, n=5, c=7, count=3, training=1, partials=P,
         write_back=1, fin=None):
    return pgcn.lib.pgcn_debug_xent_fwd(logits, ld, grad, truth, n, c, count, training, partials,
                                        write_back, ctypes.byref(fin) if fin else None, None)


def fused(pgcn, H=P, ldh=16, kh=16, W=P, ldw=8, logits=P, ld=8, grad=P, truth=P, n=5, c=7,
          count=3, training=1, partials=P, dH=None, lddh=16, dWp=None, table=None, scale=None,
          pos=None, rows=0, fin=None):
    return pgcn.lib.pgcn_debug_out_xent(H, ldh, kh, W, ldw, logits, ld, grad, truth, n, c, count,
                                        training, partials, dH, lddh, dWp, table, scale, pos,
                                        rows, ctypes.byref(fin) if fin else None, None)


def test_xent_fwd_entry_validates(pgcn):
    bad = pgcn.PGCN_E_INVALID
    for kw in (dict(logits=None), dict(truth=None), dict(partials=None), dict(grad=None),
               dict(ld=6), dict(ld=128, c=100), dict(c=0), dict(c=9), dict(n=-1),
               dict(fin=final(pgcn, ticket=None)), dict(fin=final(pgcn, part4=None)),
               dict(fin=final(pgcn, out2=None)), dict(fin=final(pgcn, group=3)),
               dict(fin=final(pgcn, group=3, gticket=P)), dict(fin=final(pgcn, group=-1)),
               dict(fin=final(pgcn, n_w=10)), dict(fin=final(pgcn, ctr=P, ring_cap=0))):
        assert xent(pgcn, **kw) == bad, kw
    assert xent(pgcn, n=0) == pgcn.PGCN_OK
    assert xent(pgcn, n=0, logits=None, grad=None, truth=None, partials=None) == pgcn.PGCN_OK
    assert xent(pgcn, n=0, fin=final(pgcn, group=3, gticket=P, gpart4=P)) == pgcn.PGCN_OK
    assert xent(pgcn, n=0, ld=124, c=124, training=0, grad=None) == pgcn.PGCN_OK


def test_out_xent_entry_validates(pgcn):
    bad = pgcn.PGCN_E_INVALID
    for kw in (dict(H=None), dict(W=None), dict(logits=None), dict(truth=None),
               dict(partials=None), dict(grad=None), dict(kh=0), dict(kh=17, ldh=20),
               dict(ldh=12), dict(ld=120, c=118, ldw=118), dict(ld=6), dict(c=0), dict(c=9),
               dict(ldw=6), dict(n=-1), dict(dH=P, lddh=12),
               dict(dWp=P, ld=52, c=50, ldw=50),
               dict(dH=P, table=P, scale=P, kh=8, lddh=8),
               dict(dH=P, table=P, scale=None), dict(table=P, scale=P),
               dict(dH=P, table=P, scale=P, rows=-1),
               dict(fin=final(pgcn, ticket=None)), dict(fin=final(pgcn, group=2)),
               dict(fin=final(pgcn, group=2, gpart4=P))):
        assert fused(pgcn, **kw) == bad, kw
    assert fused(pgcn, n=0) == pgcn.PGCN_OK
    assert fused(pgcn, n=0, H=None, W=None, logits=None, grad=None, truth=None,
                 partials=None) == pgcn.PGCN_OK
    assert fused(pgcn, n=0, dH=P, dWp=P, table=P, scale=P, rows=0,
                 fin=final(pgcn, group=2, gticket=P, gpart4=P)) == pgcn.PGCN_OK
    assert fused(pgcn, n=0, ld=116, c=116, ldw=116, kh=1, ldh=1) == pgcn.PGCN_OK


def test_reduction_entries_validate(pgcn):
    lib, bad, ok = pgcn.lib, pgcn.PGCN_E_INVALID, pgcn.PGCN_OK
    for fn in (lib.pgcn_debug_tn_reduce_blocks, lib.pgcn_debug_tn_reduce_one_pass):
        assert fn(None, 4, 16, 7, 48, P, 8, None) == bad
        assert fn(P, 4, 16, 7, 48, None, 8, None) == bad
        assert fn(P, 4, 0, 7, 48, P, 8, None) == bad
        assert fn(P, 4, 16, 0, 48, P, 8, None) == bad
        assert fn(P, 4, 16, 9, 48, P, 8, None) == bad   # N > ldc
        assert fn(P, 4, 16, 7, 4, P, 8, None) == bad    # ldc > ldp
        assert fn(P, -1, 16, 7, 48, P, 8, None) == bad
        assert fn(P, 0, 16, 7, 48, P, 8, None) == ok
        assert fn(None, 0, 16, 7, 48, None, 8, None) == ok
    ws = lib.pgcn_debug_tn_reduce_blocks_workspace
    # the partials and, after them, one group sum per spg of them (spg = 16 up to 256 blocks)
    assert ws(16, 16, 48) == (16 + 1) * 16 * 48 * 4
    assert ws(256, 5, 48) == (256 + 16) * 5 * 48 * 4
    assert ws(257, 5, 48) == (257 + 9) * 5 * 48 * 4    # spg = 32
    assert ws(-1, 5, 48) == 0 and ws(4, 0, 48) == 0
    fin = lib.pgcn_debug_finalize_ring
    assert fin(None, 4, 10, None, 0, 0.0, P, None, 1, None, None) == bad
    assert fin(P, 4, 10, None, 0, 0.0, None, None, 1, None, None) == bad
    assert fin(P, 4, 10, None, 5, 0.0, P, None, 1, None, None) == bad   # n_l2 without w
    assert fin(P, 4, 10, None, 0, 0.0, P, P, 0, None, None) == bad      # ring_cap < 1
    assert fin(P, -1, 10, None, 0, 0.0, P, None, 1, None, None) == bad
    assert fin(P, 0, 10, None, 0, 0.0, P, None, 1, None, None) == ok
    assert fin(None, 0, 10, None, 0, 0.0, None, None, 1, None, None) == ok
    assert lib.pgcn_debug_ring_slice_rows() > 0 and lib.pgcn_debug_ring_slice_rows() % 64 == 0
