"""The GraphSAGE aggregator kernels through the kernel ABI -- pgcn_agg_max_fwd / _bwd, and
pgcn_graph_create_mean through pgcn_graphsum -- against the numpy formulas of tests/sage_ref.py.

Graphs (both directed: the transposed index is not the CSR):
  five: 5 nodes; row 0 = [1, 2, 2] (a duplicated edge), row 2 empty, column 4 without an
        incoming slot.
  hub:  300 nodes; rows 0..3 have 4,100 / 511 / 512 / 513 slots (nine row segments, and the
        three lengths around one segment), row 4 is empty; columns 4..7 carry 511 / 512 / 513 /
        4,100 incoming slots (duplicated edges from rows 8..57, the column segments); rows 5..7
        have 63 / 64 / 65 slots; column 299 has no incoming slot.

Bounds.  The forward is exact: a maximum rounds nothing and out = add + max is one fp32 add, so
out and arg equal numpy's float32 result and first argmax bit for bit.  A backward element that
sums k non-zero terms is within k 2^-24 sum|terms| of float64 (the fp32 sequential-sum bound,
which holds for any order of a merge); k <= 1 is exact.  A mean element over len slots is within
(len + 2) 2^-24 sum|terms|: one rounding per product, len - 1 adds, the scale.
"""
import ctypes

import numpy as np
import pytest

import sage_ref

pytestmark = pytest.mark.gpu

GUARD = 7.25
EPS = 2.0 ** -24


def _up4(d):
    return (d + 3) // 4 * 4


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _sync():
    import torch
    torch.cuda.synchronize()


def five_graph():
    rows = [[1, 2, 2], [0, 1], [], [0, 3, 1], [1]]
    indptr = np.zeros(6, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.array([j for r in rows for j in r], np.int32)


HUB_ROWS = {0: 4100, 1: 511, 2: 512, 3: 513, 5: 63, 6: 64, 7: 65}
HUB_COLS = {4: 511, 5: 512, 6: 513, 7: 4100}


def hub_graph():
    rng = np.random.default_rng(77)
    n = 300
    rows = [None] * n
    for i, k in HUB_ROWS.items():
        rows[i] = rng.integers(100, 299, k)
    rows[4] = np.zeros(0, np.int64)
    feeders = np.arange(8, 58)
    for i in range(8, n):
        rows[i] = rng.integers(100, 299, rng.integers(1, 13))
    for c, k in HUB_COLS.items():  # k slots into column c, dealt over the 50 feeder rows
        for i, part in zip(feeders, np.array_split(np.full(k, c), len(feeders))):
            rows[i] = np.concatenate([rows[i], part])
    for i in feeders:
        rows[i] = rng.permutation(rows[i])
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    return indptr, np.concatenate(rows).astype(np.int32)


GRAPHS = {"five": five_graph, "hub": hub_graph}


@pytest.fixture(scope="module")
def graphs(pgcn):
    """name -> (handle, indptr, indices); the handles are shared by every test of the module."""
    out, handles = {}, []
    for name, make in GRAPHS.items():
        indptr, indices = make()
        h = ctypes.c_void_p()
        pgcn.check(pgcn.lib.pgcn_graph_create(len(indptr) - 1, indptr.ctypes.data_as(ctypes.c_void_p),
                                              indices.ctypes.data_as(ctypes.c_void_p),
                                              ctypes.byref(h)), "graph_create")
        out[name] = (h, indptr, indices)
        handles.append(h)
    yield out
    for h in handles:
        pgcn.lib.pgcn_graph_destroy(h)


def test_graph_shapes(graphs):
    _, indptr, indices = graphs["five"]
    assert list(np.diff(indptr)) == [3, 2, 0, 3, 1]
    assert list(indices[:3]) == [1, 2, 2] and 4 not in indices
    _, indptr, indices = graphs["hub"]
    n = 300
    lens = np.diff(indptr)
    for i, k in HUB_ROWS.items():
        assert lens[i] == k
    assert lens[4] == 0
    incoming = np.bincount(indices, minlength=n)
    for c, k in HUB_COLS.items():
        assert incoming[c] == k
    assert incoming[299] == 0
    import scipy.sparse as sps
    a = sps.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    assert (a != a.T).nnz > 0


# every GL boundary (4, 8, 16, 32, 64 columns) from both sides, each with a tight stride and
# one with 8 columns of padding
WIDTHS = [(d, _up4(d) + pad) for d in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 127, 128)
          for pad in (0, 8)]


def _padded(n, d, ld, body, fill=np.nan, dtype=np.float32):
    a = np.full((n, ld), fill, dtype)
    a[:, :d] = body
    return a


def _guarded(n, ld, fill, dtype=np.float32):
    a = np.full((n + 2, ld), fill, dtype)
    a[0] = a[-1] = GUARD
    return a


def run_fwd(pgcn, graph, Q, d, ld, add=None, want_arg=True, stream=None):
    """The forward on guarded outputs: (out, arg) host copies with the guard rows."""
    h, indptr, _ = graph
    n = len(indptr) - 1
    dQ, dadd = _dev(Q), (_dev(add) if add is not None else None)
    dout = _dev(_guarded(n, ld, -3.0))
    darg = _dev(_guarded(n, ld, -77, np.int32)) if want_arg else None
    _sync()
    st = pgcn.lib.pgcn_agg_max_fwd(h, _p(dQ), ld, d, _p(dadd), ld if add is not None else 0,
                                   _p(dout, 4 * ld), ld, _p(darg, 4 * ld) if want_arg else None,
                                   ld if want_arg else 0, stream)
    assert st == pgcn.PGCN_OK
    _sync()
    return dout.cpu().numpy(), (darg.cpu().numpy() if want_arg else None)


def check_fwd(got, Zref, aref, d, ld):
    out, arg = got
    Z = out[1:-1]
    np.testing.assert_array_equal(Z[:, :d].view(np.uint32), Zref.view(np.uint32), err_msg="out")
    assert (Z[:, d:_up4(d)].view(np.uint32) == 0).all() and (Z[:, _up4(d):] == -3.0).all()
    assert (out[0] == GUARD).all() and (out[-1] == GUARD).all()
    if arg is not None:
        A = arg[1:-1]
        np.testing.assert_array_equal(A[:, :d], aref, err_msg="arg")
        assert (A[:, d:_up4(d)] == -1).all() and (A[:, _up4(d):] == -77).all()
        assert (arg[0] == int(GUARD)).all() and (arg[-1] == int(GUARD)).all()


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld", WIDTHS)
def test_forward(pgcn, graphs, name, d, ld):
    """out and arg equal numpy's float32 add + max and first argmax bit for bit, with and without
    `add`; NaN in the padding of in / add reaches nothing; [d, round_up4(d)) is 0 / -1, the
    columns beyond and the guard rows are untouched; the empty row gives add (or 0) and -1; a
    call without arg and a second call give the same bits."""
    h, indptr, indices = graphs[name]
    n = len(indptr) - 1
    rng = np.random.default_rng(100 * d + n)
    Qb = rng.standard_normal((n, d)).astype(np.float32)
    Rb = rng.standard_normal((n, d)).astype(np.float32)
    Q, R = _padded(n, d, ld, Qb), _padded(n, d, ld, Rb)
    Zref, aref = sage_ref.max_forward(indptr, indices, Qb, Rb)
    got = run_fwd(pgcn, graphs[name], Q, d, ld, add=R)
    check_fwd(got, Zref, aref, d, ld)
    empty = np.diff(indptr) == 0
    assert empty.any() and (aref[empty] == -1).all()
    np.testing.assert_array_equal(got[0][1:-1][empty, :d], Rb[empty])
    Zmax, _ = sage_ref.max_forward(indptr, indices, Qb)
    bare = run_fwd(pgcn, graphs[name], Q, d, ld)
    check_fwd(bare, Zmax, aref, d, ld)
    assert (bare[0][1:-1][empty, :d] == 0.0).all()
    noarg = run_fwd(pgcn, graphs[name], Q, d, ld, add=R, want_arg=False)
    np.testing.assert_array_equal(noarg[0].view(np.uint32), got[0].view(np.uint32))
    again = run_fwd(pgcn, graphs[name], Q, d, ld, add=R)
    np.testing.assert_array_equal(again[0].view(np.uint32), got[0].view(np.uint32))
    np.testing.assert_array_equal(again[1], got[1])


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld", [(1, 4), (5, 8), (16, 16), (33, 36), (128, 128)])
def test_forward_ties_take_the_lowest_slot(pgcn, graphs, name, d, ld):
    """Small-integer inputs: most maxima are shared by many slots (and, on the hub row, by several
    lane groups and segments); arg is numpy's first argmax everywhere."""
    h, indptr, indices = graphs[name]
    n = len(indptr) - 1
    rng = np.random.default_rng(7 * d + n)
    Qb = rng.integers(-2, 3, (n, d)).astype(np.float32)
    Zref, aref = sage_ref.max_forward(indptr, indices, Qb)
    lens = np.diff(indptr)
    cand = [Qb[indices[indptr[i]:indptr[i + 1]]] for i in range(n) if lens[i] > 1]
    assert sum(int(((c == c.max(axis=0)).sum(axis=0) > 1).sum()) for c in cand) > 0
    check_fwd(run_fwd(pgcn, graphs[name], _padded(n, d, ld, Qb), d, ld), Zref, aref, d, ld)


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld", [(3, 4), (16, 16), (65, 76)])
def test_forward_signed_zeros_tie(pgcn, graphs, name, d, ld):
    """Every input is -0.0 or +0.0: they compare equal, so the lowest slot wins and `out` carries
    that slot's sign bit; some row has -0.0 ahead of +0.0."""
    h, indptr, indices = graphs[name]
    n = len(indptr) - 1
    rng = np.random.default_rng(3 * d + n)
    Qb = np.where(rng.integers(0, 2, (n, d)) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    lens = np.diff(indptr)
    first = Qb[indices[indptr[:-1][lens > 1]]]
    second = Qb[indices[indptr[:-1][lens > 1] + 1]]
    assert (np.signbit(first) & ~np.signbit(second)).any()
    rows = np.arange(n)[lens > 0]
    Zref = np.zeros((n, d), np.float32)
    Zref[rows] = Qb[indices[indptr[rows]]]
    aref = np.full((n, d), -1, np.int64)
    aref[rows] = indptr[rows][:, None]
    check_fwd(run_fwd(pgcn, graphs[name], _padded(n, d, ld, Qb), d, ld), Zref, aref, d, ld)


def run_bwd(pgcn, graph, G, arg, d, ld, stream=None):
    h, indptr, _ = graph
    n = len(indptr) - 1
    dG, da = _dev(G), _dev(arg)
    ddin = _dev(_guarded(n, ld, -3.0))
    _sync()
    assert pgcn.lib.pgcn_agg_max_bwd(h, _p(dG), ld, _p(da), ld, d, _p(ddin, 4 * ld), ld,
                                     stream) == pgcn.PGCN_OK
    _sync()
    return ddin.cpu().numpy()


def check_bwd(got, indptr, indices, Gb, aref, d):
    din = got[1:-1]
    ref = sage_ref.max_backward(indptr, indices, Gb, aref)
    cnt, mag = sage_ref.max_backward_terms(indptr, indices, Gb, aref)
    err = np.abs(din[:, :d].astype(np.float64) - ref)
    bound = cnt * EPS * mag
    worst = float((err / np.maximum(bound, 1e-300))[cnt > 1].max()) if (cnt > 1).any() else 0.0
    print(f"dQ: up to {int(cnt.max())} terms, worst error {worst:.3g} of the bound")
    assert (err <= bound).all()
    one = cnt <= 1
    np.testing.assert_array_equal(din[:, :d][one].astype(np.float64), ref[one])
    assert (din[:, d:_up4(d)].view(np.uint32) == 0).all() and (din[:, _up4(d):] == -3.0).all()
    assert (got[0] == GUARD).all() and (got[-1] == GUARD).all()
    return cnt


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld", WIDTHS)
def test_backward(pgcn, graphs, name, d, ld):
    """dQ against float64 within k 2^-24 sum|terms| (k <= 1: exact), for the forward's own arg and
    for an arg that names a random slot of its row (many winners in the hub columns); NaN in G's
    padding and slot ids in arg's padding reach nothing; the column without an incoming slot is a
    zero row; two calls give the same bits."""
    h, indptr, indices = graphs[name]
    n = len(indptr) - 1
    rng = np.random.default_rng(9 * d + n)
    Qb = rng.standard_normal((n, d)).astype(np.float32)
    Gb = (rng.standard_normal((n, d)) * 0.5).astype(np.float32)
    G = _padded(n, d, ld, Gb)
    _, a_fwd = sage_ref.max_forward(indptr, indices, Qb)
    lens = np.diff(indptr)
    a_rand = np.where(lens[:, None] > 0,
                      indptr[:-1, None] + rng.integers(0, 1 << 30, (n, d)) % np.maximum(lens, 1)[:, None],
                      -1)
    most = 0
    for aref in (a_fwd, a_rand):
        # (arg's padding names slot 0 and, on the hub graph, a slot into a hub column)
        arg = _padded(n, d, ld, aref, fill=0, dtype=np.int32)
        arg[:, d:] = int(np.flatnonzero(indices == indices.max())[0]) if name == "five" else \
            int(np.flatnonzero(indices == 7)[0])
        got = run_bwd(pgcn, graphs[name], G, arg, d, ld)
        cnt = check_bwd(got, indptr, indices, Gb, aref, d)
        most = max(most, int(cnt.max()))
        none_in = np.bincount(indices, minlength=n) == 0
        assert none_in.any() and (got[1:-1][none_in, :_up4(d)].view(np.uint32) == 0).all()
        again = run_bwd(pgcn, graphs[name], G, arg, d, ld)
        np.testing.assert_array_equal(again.view(np.uint32), got.view(np.uint32))
    assert most >= 2


def _mean_graph(pgcn, indptr, indices, transpose):
    h = ctypes.c_void_p()
    pgcn.check(pgcn.lib.pgcn_graph_create_mean(len(indptr) - 1,
                                               indptr.ctypes.data_as(ctypes.c_void_p),
                                               indices.ctypes.data_as(ctypes.c_void_p), transpose,
                                               ctypes.byref(h)), "graph_create_mean")
    return h


@pytest.fixture(scope="module")
def mean_graphs(pgcn, graphs):
    out = {(name, t): _mean_graph(pgcn, g[1], g[2], t) for name, g in graphs.items() for t in (0, 1)}
    yield out
    for h in out.values():
        pgcn.lib.pgcn_graph_destroy(h)


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld", [(1, 4), (3, 4), (4, 4), (16, 16), (17, 20), (33, 44), (64, 64),
                                  (128, 128)])
def test_mean_graphs(pgcn, graphs, mean_graphs, name, d, ld):
    """pgcn_graphsum on pgcn_graph_create_mean's two graphs is the mean forward (transpose 0) and
    backward (transpose 1): every element within (len + 2) 2^-24 sum|terms| of float64, len the
    slots summed into it; rows / columns without a slot give zero; two calls give the same bits."""
    _, indptr, indices = graphs[name]
    n = len(indptr) - 1
    rng = np.random.default_rng(5 * d + n)
    Xb = rng.standard_normal((n, d)).astype(np.float32)
    X = _padded(n, d, ld, Xb, fill=0.0)
    rows = sage_ref.rows_of(indptr)
    lens = np.diff(indptr).astype(np.float64)
    inv = np.zeros(n)
    inv[lens > 0] = 1.0 / lens[lens > 0]
    for t in (0, 1):
        if t == 0:
            ref = sage_ref.mean_forward(indptr, indices, Xb)
            mag = np.zeros((n, d))
            np.add.at(mag, rows, np.abs(Xb[indices].astype(np.float64)) * inv[rows, None])
            k = lens
        else:
            ref = sage_ref.mean_backward(indptr, indices, Xb)
            mag = np.zeros((n, d))
            np.add.at(mag, indices, np.abs(Xb[rows].astype(np.float64)) * inv[rows, None])
            k = np.bincount(indices, minlength=n).astype(np.float64)
        outs = []
        for _ in range(2):
            dX, dout = _dev(X), _dev(_guarded(n, ld, -3.0))
            _sync()
            assert pgcn.lib.pgcn_graphsum(mean_graphs[(name, t)], _p(dX), ld, _p(dout, 4 * ld), ld,
                                          d, None) == pgcn.PGCN_OK
            _sync()
            outs.append(dout.cpu().numpy())
        got = outs[0][1:-1, :d].astype(np.float64)
        err = np.abs(got - ref)
        bound = (k[:, None] + 2) * EPS * mag
        worst = float((err / np.maximum(bound, 1e-300))[mag > 0].max())
        print(f"mean transpose={t}: worst error {worst:.3g} of the bound")
        assert (err <= bound).all()
        assert (k == 0).any() and (got[k == 0] == 0.0).all()
        assert (outs[0][0] == GUARD).all() and (outs[0][-1] == GUARD).all()
        np.testing.assert_array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def test_argument_refusals_with_a_graph(pgcn, graphs):
    """With a real graph handle: bad d, bad strides, null and misaligned pointers are
    PGCN_E_INVALID."""
    h, indptr, _ = graphs["five"]
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    t = _dev(np.zeros((8, 132), np.float32))
    a = _dev(np.zeros((8, 132), np.int32))

    def fwd(d=4, ld_in=4, ld_add=4, ld_out=4, ld_arg=4, inp=_p(t), add=_p(t), out=_p(t), arg=_p(a)):
        return lib.pgcn_agg_max_fwd(h, inp, ld_in, d, add, ld_add, out, ld_out, arg, ld_arg, None)
    wide = dict(ld_in=8, ld_add=8, ld_out=8, ld_arg=8)
    assert fwd(d=5, **wide) == pgcn.PGCN_OK
    assert fwd(d=0) == INV and fwd(d=129, ld_in=132, ld_add=132, ld_out=132, ld_arg=132) == INV
    for k in wide:
        assert fwd(d=5, **{**wide, k: 4}) == INV and fwd(**{k: 6}) == INV, k
    assert fwd(inp=None) == INV and fwd(out=None) == INV
    assert fwd(inp=_p(t, 4)) == INV and fwd(out=_p(t, 8)) == INV and fwd(add=_p(t, 4)) == INV
    assert fwd(arg=_p(a, 4)) == INV
    assert fwd(add=None, ld_add=0, arg=None, ld_arg=0) == pgcn.PGCN_OK

    def bwd(d=4, ld_g=4, ld_arg=4, ld_din=4, G=_p(t), arg=_p(a), din=_p(t)):
        return lib.pgcn_agg_max_bwd(h, G, ld_g, arg, ld_arg, d, din, ld_din, None)
    wide = dict(ld_g=8, ld_arg=8, ld_din=8)
    assert bwd(d=5, **wide) == pgcn.PGCN_OK
    assert bwd(d=0) == INV and bwd(d=129, ld_g=132, ld_arg=132, ld_din=132) == INV
    for k in wide:
        assert bwd(d=5, **{**wide, k: 4}) == INV and bwd(**{k: 6}) == INV, k
    assert bwd(G=None) == INV and bwd(arg=None) == INV and bwd(din=None) == INV
    assert bwd(G=_p(t, 4)) == INV and bwd(arg=_p(a, 4)) == INV and bwd(din=_p(t, 4)) == INV
    _sync()

    def mean(n=5, ip=indptr, idx=graphs["five"][2], tr=0):
        out = ctypes.c_void_p()
        return lib.pgcn_graph_create_mean(n, ip.ctypes.data_as(ctypes.c_void_p),
                                          idx.ctypes.data_as(ctypes.c_void_p), tr, ctypes.byref(out))
    assert mean(n=0) == INV and mean(tr=2) == INV
    assert mean(idx=np.full(9, 5, np.int32)) == INV
    assert mean(ip=np.array([0, 3, 2, 5, 8, 9], np.int32)) == INV


def test_captured_graph_replays_the_calls(pgcn, graphs):
    """After the graph's first call the forward and the backward allocate nothing: captured into
    one device graph on a side stream and replayed on fresh inputs, they give the eager bits."""
    import torch
    name, d, ld = "hub", 17, 20
    h, indptr, indices = graphs[name]
    n = len(indptr) - 1
    rng = np.random.default_rng(5)
    mk = lambda: _padded(n, d, ld, rng.standard_normal((n, d)).astype(np.float32))  # noqa: E731
    Q0, R0, G0, Q1, R1, G1 = mk(), mk(), mk(), mk(), mk(), mk()
    eager = []
    for Q, R, G in ((Q0, R0, G0), (Q1, R1, G1)):
        out, arg = run_fwd(pgcn, graphs[name], Q, d, ld, add=R)
        eager.append((out[1:-1], arg[1:-1], run_bwd(pgcn, graphs[name], G, arg[1:-1], d, ld)[1:-1]))
    dQ, dR, dG = _dev(Q0), _dev(R0), _dev(G0)
    dout, darg = _dev(np.zeros((n, ld), np.float32)), _dev(np.zeros((n, ld), np.int32))
    ddin = _dev(np.zeros((n, ld), np.float32))
    side = torch.cuda.Stream()
    cg = torch.cuda.CUDAGraph()
    _sync()
    with torch.cuda.graph(cg, stream=side):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert pgcn.lib.pgcn_agg_max_fwd(h, _p(dQ), ld, d, _p(dR), ld, _p(dout), ld, _p(darg), ld,
                                         st) == pgcn.PGCN_OK
        assert pgcn.lib.pgcn_agg_max_bwd(h, _p(dG), ld, _p(darg), ld, d, _p(ddin), ld,
                                         st) == pgcn.PGCN_OK
    for k, (Q, R, G) in enumerate(((Q0, R0, G0), (Q1, R1, G1))):
        dQ.copy_(torch.from_numpy(Q))
        dR.copy_(torch.from_numpy(R))
        dG.copy_(torch.from_numpy(G))
        cg.replay()
        _sync()
        out, arg, din = eager[k]
        np.testing.assert_array_equal(dout.cpu().numpy()[:, :_up4(d)].view(np.uint32),
                                      out[:, :_up4(d)].view(np.uint32))
        np.testing.assert_array_equal(darg.cpu().numpy()[:, :_up4(d)], arg[:, :_up4(d)])
        np.testing.assert_array_equal(ddin.cpu().numpy()[:, :_up4(d)].view(np.uint32),
                                      din[:, :_up4(d)].view(np.uint32))
