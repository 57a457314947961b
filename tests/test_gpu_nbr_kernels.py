"""The neighbour-sampling kernels through the kernel ABI -- pgcn_nbr_sample_draw, pgcn_nbr_agg_fwd
/ _bwd -- against the numpy restatement of tests/nbr_ref.py on its 2,000-row graph (rows of 0, 1,
K - 1, K, K + 1, 2 K and 3,000 slots; 1,200 rows of K + 1 slots that all hold node 0).

Bounds.  The draw, the index, the max and its arg are exact.  A mean element is within (cnt + 2)
2^-24 ((1 / cnt) sum|in| + |add|) of float64: cnt - 1 adds, the reciprocal, the scale, the add.  A
backward element over a list of `len` entries is within (len + 2) 2^-24 sum|terms|, terms = G_i /
cnt_i (mean) or the routed G_i[c] (max): one or two roundings per term and len - 1 adds, in any
order of a merge."""
import ctypes

import numpy as np
import pytest

import nbr_ref

pytestmark = pytest.mark.gpu

EPS, SEED, FILL = 2.0 ** -24, 1234567, -3.0


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def sampled(pgcn):
    """K -> (NbrSample, indptr, indices), created at first use and shared by the module."""
    made, handles = {}, []

    def get(K):
        if K not in made:
            indptr, indices = nbr_ref.graph(K)
            h = ctypes.c_void_p()
            pgcn.check(pgcn.lib.pgcn_graph_create(len(indptr) - 1, indptr.ctypes.data_as(ctypes.c_void_p),
                                                  indices.ctypes.data_as(ctypes.c_void_p),
                                                  ctypes.byref(h)), "graph_create")
            handles.append(h)
            made[K] = (pgcn.NbrSample(h, len(indptr) - 1, K), indptr, indices)
        return made[K]
    yield get
    for s, _, _ in made.values():
        s.close()
    for h in handles:
        pgcn.lib.pgcn_graph_destroy(h)


@pytest.mark.parametrize("K", [1, 2, 5, 25, 64])
def test_draw_and_index(pgcn, sampled, K):
    """cnt, slots, neighbours and the transposed index equal the restatement element for element
    over two rounds; kept slots are distinct, ascending and inside their row; the same (seed,
    round) repeats the bits and another round differs; node 0's list exceeds one segment."""
    s, indptr, indices = sampled(K)
    n, seg = len(indptr) - 1, pgcn.lib.pgcn_link_segment_slots()
    assert set([0, 1, K - 1, K, K + 1, 2 * K, 3000]) <= set(np.diff(indptr)[:7].tolist())
    got = {}
    for rnd in (0, 7, 0):
        s.draw(SEED, rnd)
        cnt, slot, nbr, t_ptr, t_row, t_slot = s.copy()
        rc, rs, rn = nbr_ref.draw(indptr, indices, K, SEED, rnd)
        np.testing.assert_array_equal(cnt, rc)
        np.testing.assert_array_equal(slot, rs)
        np.testing.assert_array_equal(nbr, rn)
        kept = slot >= 0
        assert (kept == (np.arange(K)[None, :] < cnt[:, None])).all()
        assert (np.diff(slot, axis=1)[kept[:, 1:]] > 0).all()
        assert ((slot >= indptr[:-1, None]) & (slot < indptr[1:, None]))[kept].all()
        (rp, rr, rsl), total = nbr_ref.transposed(rs, rn, n), int(cnt.sum())
        np.testing.assert_array_equal(t_ptr, rp)
        np.testing.assert_array_equal(t_row[:total], rr)
        np.testing.assert_array_equal(t_slot[:total], rsl)
        assert (t_row[total:] == -1).all() and (t_slot[total:] == -1).all()
        if K >= 2:
            assert rp[1] - rp[0] > seg  # (a condition on the input: the hub is a segmented list)
        if rnd in got:
            np.testing.assert_array_equal(got[rnd], slot)
        got[rnd] = slot
    assert (got[0] != got[7]).any()


@pytest.mark.parametrize("with_add", [False, True])
@pytest.mark.parametrize("d", [1, 4, 20, 128])
@pytest.mark.parametrize("mode", [1, 2])
def test_forward_backward(pgcn, sampled, mode, d, with_add):
    s, indptr, _ = sampled(25)
    n, ld, up4 = len(indptr) - 1, (d + 3) // 4 * 4 + 8, (d + 3) // 4 * 4
    s.draw(SEED, 3)
    cnt, slot, nbr, t_ptr, _, _ = s.copy()
    assert t_ptr[1] - t_ptr[0] > pgcn.lib.pgcn_link_segment_slots() and (cnt == 0).any()
    rng = np.random.default_rng(10 * d + mode)
    body = lambda: rng.standard_normal((n, d)).astype(np.float32)  # noqa: E731
    Qb, Rb, Gb = body(), body(), body()
    if mode == 2:
        Qb = np.round(Qb * 2) / 2  # (many ties: the lowest slot must win)

    def padded(b):
        a = np.full((n, ld), np.nan, np.float32)
        a[:, :d] = b
        return _dev(a)
    Q, R, G = padded(Qb), (padded(Rb) if with_add else None), padded(Gb)

    def fwd():
        out, arg = _dev(np.full((n, ld), FILL, np.float32)), _dev(np.full((n, ld), -77, np.int32))
        assert s.agg_fwd(mode, Q, ld, d, R, ld if with_add else 0, out, ld, arg, ld) == pgcn.PGCN_OK
        return out.cpu().numpy(), arg.cpu().numpy(), arg
    out, arg, dev_arg = fwd()
    want, scale, want_arg = nbr_ref.forward(mode, cnt, slot, nbr, Qb, Rb if with_add else None)
    if mode == 1:
        err = np.abs(out[:, :d] - want)
        assert (err <= (cnt[:, None] + 2) * EPS * scale).all(), err.max()
        assert (arg == -77).all()
    else:
        np.testing.assert_array_equal(out[:, :d].view(np.uint32), want.view(np.uint32))
        np.testing.assert_array_equal(arg[:, :d], want_arg)
        assert (arg[:, d:up4] == -1).all() and (arg[:, up4:] == -77).all()
    assert (out[:, d:up4].view(np.uint32) == 0).all() and (out[:, up4:] == FILL).all()
    np.testing.assert_array_equal(fwd()[0].view(np.uint32), out.view(np.uint32))

    def bwd():
        din = _dev(np.full((n, ld), FILL, np.float32))
        assert s.agg_bwd(mode, G, ld, dev_arg if mode == 2 else None, ld, d, din, ld) == pgcn.PGCN_OK
        return din.cpu().numpy()
    din = bwd()
    want, mag = nbr_ref.backward(mode, cnt, slot, nbr, Gb, want_arg)
    err = np.abs(din[:, :d] - want)
    assert (err <= (np.diff(t_ptr)[:, None] + 2) * EPS * mag).all(), err.max()
    assert (din[np.diff(t_ptr) == 0, :up4].view(np.uint32) == 0).all() and t_ptr[-1] == t_ptr[-2]
    assert (din[:, d:up4].view(np.uint32) == 0).all() and (din[:, up4:] == FILL).all()
    np.testing.assert_array_equal(bwd().view(np.uint32), din.view(np.uint32))
