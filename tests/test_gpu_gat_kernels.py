"""The graph attention kernels through the kernel ABI (pgcn_gat_scores / _fwd / _bwd) against
the float64 reference of tests/gat_ref.py (checked itself in tests/test_cpu_gat.py).

Graph: n = 300, directed (the transposed index is not the CSR).  Row 0 has 4,100 slots cycling
over 7 columns: duplicates, nine 512-slot row segments, and those 7 columns carry more than
512 incoming slots each (column segments); row 1 is empty, row 2 has one slot, rows 3, 4, 5 have
63, 64, 65 slots (the wave's width), the others 1-12 random slots; column 299 has no incoming
slot.  Also n = 1 with one self loop.
"""
import ctypes

import numpy as np
import pytest

import gat_ref

pytestmark = pytest.mark.gpu

GUARD = 7.25
SLOPE = 0.2


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


def hub_graph():
    rng = np.random.default_rng(2024)
    n = 300
    rows = [None] * n
    rows[0] = np.arange(4100) % 7
    rows[1] = np.zeros(0, np.int64)
    rows[2] = np.array([5])
    for i, k in ((3, 63), (4, 64), (5, 65)):
        rows[i] = rng.integers(0, 299, k)
    for i in range(6, n):
        rows[i] = rng.integers(0, 299, rng.integers(1, 13))
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate(rows).astype(np.int32)
    return indptr, indices


GRAPHS = {"hub": hub_graph,
          "one": lambda: (np.array([0, 1], np.int32), np.array([0], np.int32))}


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


def test_graph_shape(graphs):
    _, indptr, indices = graphs["hub"]
    n = 300
    lens = np.diff(indptr)
    assert lens[0] == 4100 and lens[1] == 0 and lens[2] == 1 and list(lens[3:6]) == [63, 64, 65]
    assert lens[6:].min() >= 1 and lens[6:].max() <= 12
    incoming = np.bincount(indices, minlength=n)
    assert incoming[299] == 0 and incoming[:7].min() > 512
    import scipy.sparse as sps
    a = sps.csr_matrix((np.ones(len(indices)), indices, indptr), shape=(n, n))
    assert (a != a.T).nnz > 0


def _inputs(n, d, ld, seed, scale=1.0):
    """P [n][ld] with NaN padding, a_dst / a_src [d]."""
    rng = np.random.default_rng(seed)
    P = np.full((n, ld), np.nan, np.float32)
    P[:, :d] = rng.standard_normal((n, d))
    a_dst = (scale * rng.standard_normal(d) / np.sqrt(d)).astype(np.float32)
    a_src = (scale * rng.standard_normal(d) / np.sqrt(d)).astype(np.float32)
    return P, a_dst, a_src


def _guarded(n, ld, fill):
    a = np.full((n + 2, ld), fill, np.float32)
    a[0] = a[-1] = GUARD
    return a


def run_forward(pgcn, graph, P, a_dst, a_src, d, ld, training=True):
    """scores + forward on guarded outputs; host copies with the guard rows."""
    h, indptr, _ = graph
    n, nnz = len(indptr) - 1, int(indptr[-1])
    lib = pgcn.lib
    dP, dad, das = _dev(P), _dev(a_dst), _dev(a_src)
    du, dv = _dev(np.full(n + 2, GUARD, np.float32)), _dev(np.full(n + 2, GUARD, np.float32))
    dZ = _dev(_guarded(n, ld, -3.0))
    dal = _dev(np.full(nnz + 2, GUARD, np.float32)) if training else None
    _sync()
    assert lib.pgcn_gat_scores(_p(dP), ld, n, d, _p(dad), _p(das), _p(du, 4), _p(dv, 4),
                               None) == pgcn.PGCN_OK
    assert lib.pgcn_gat_fwd(h, _p(dP), ld, _p(du, 4), _p(dv, 4), SLOPE, _p(dZ, 4 * ld), ld, d,
                            _p(dal, 4) if training else None, None) == pgcn.PGCN_OK
    _sync()
    out = dict(u=du.cpu().numpy(), v=dv.cpu().numpy(), Z=dZ.cpu().numpy())
    if training:
        out["alpha"] = dal.cpu().numpy()
    return out


def _close(got, want, what, scale=1.0):
    """rtol 1e-4, atol 1e-6 max|ref| (x scale): the project's parity bound."""
    big = float(np.abs(want).max()) if want.size else 0.0
    tol = 1e-6 * scale * big + 1e-4 * np.abs(want)
    worst = float((np.abs(got - want) / np.maximum(tol, 1e-300)).max()) if want.size else 0.0
    print(f"{what}: worst error {worst:.3g} of the tolerance")
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-6 * scale * big, err_msg=what)


WIDTHS = [(1, 4), (3, 4), (4, 4), (16, 16), (20, 20), (64, 64), (128, 128), (6, 12)]


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld", WIDTHS)
def test_forward(pgcn, graphs, name, d, ld):
    """Z, alpha, u, v against float64; every non-empty row's alpha sums to 1 within 1e-5; the
    empty row of Z exactly 0; guard rows untouched; columns [d, round_up4(d)) zero, further
    padding left alone; an eval call (alpha NULL) and a second call give the same bits."""
    h, indptr, indices = graphs[name]
    n = len(indptr) - 1
    P, a_dst, a_src = _inputs(n, d, ld, 100 * d + n)
    got = run_forward(pgcn, graphs[name], P, a_dst, a_src, d, ld)
    ref = gat_ref.gat_forward(indptr, indices, P[:, :d], a_dst, a_src)
    Z = got["Z"][1:-1]
    _close(got["u"][1:-1], ref["u"], "u")
    _close(got["v"][1:-1], ref["v"], "v")
    _close(Z[:, :d], ref["Z"], "Z")
    _close(got["alpha"][1:-1], ref["alpha"], "alpha")
    sums = np.bincount(ref["rows"], weights=got["alpha"][1:-1].astype(np.float64), minlength=n)
    lens = np.diff(indptr)
    np.testing.assert_allclose(sums[lens > 0], 1.0, atol=1e-5, rtol=0)
    assert (Z[lens == 0, :_up4(d)] == 0.0).all()
    assert (Z[:, d:_up4(d)] == 0.0).all() and (Z[:, _up4(d):] == -3.0).all()
    for k in ("u", "v", "alpha"):
        assert got[k][0] == GUARD and got[k][-1] == GUARD, k
    assert (got["Z"][0] == GUARD).all() and (got["Z"][-1] == GUARD).all()
    ev = run_forward(pgcn, graphs[name], P, a_dst, a_src, d, ld, training=False)
    np.testing.assert_array_equal(ev["Z"].view(np.uint32), got["Z"].view(np.uint32))
    again = run_forward(pgcn, graphs[name], P, a_dst, a_src, d, ld)
    for k in ("u", "v", "Z", "alpha"):
        np.testing.assert_array_equal(again[k].view(np.uint32), got[k].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("d,ld", [(3, 4), (16, 16), (128, 128)])
def test_forward_wide_scores(pgcn, graphs, d, ld):
    """Scores spanning +-80 (a_* scaled so that the largest |u_i + v_j| is 80): every output
    finite and within the same bound (the row maximum is subtracted before the exp)."""
    h, indptr, indices = graphs["hub"]
    n = len(indptr) - 1
    P, a_dst, a_src = _inputs(n, d, ld, 7 * d)
    x = gat_ref.gat_forward(indptr, indices, P[:, :d], a_dst, a_src)["x"]
    k = np.float32(80.0 / np.abs(x).max())
    a_dst, a_src = a_dst * k, a_src * k
    ref = gat_ref.gat_forward(indptr, indices, P[:, :d], a_dst, a_src)
    assert ref["x"].max() > 60 and ref["x"].min() < -60
    got = run_forward(pgcn, graphs["hub"], P, a_dst, a_src, d, ld)
    assert np.isfinite(got["Z"][1:-1, :d]).all() and np.isfinite(got["alpha"][1:-1]).all()
    _close(got["Z"][1:-1, :d], ref["Z"], "Z")
    _close(got["alpha"][1:-1], ref["alpha"], "alpha")


@pytest.mark.parametrize("d,ld", [(4, 4), (16, 16), (20, 20)])
def test_forward_zero_attention_is_the_row_mean(pgcn, graphs, d, ld):
    """a_dst = a_src = 0: alpha = 1 / len within 1e-6 and Z the row mean of the gathered P_j."""
    h, indptr, indices = graphs["hub"]
    n = len(indptr) - 1
    P, _, _ = _inputs(n, d, ld, 3 * d)
    zero = np.zeros(d, np.float32)
    got = run_forward(pgcn, graphs["hub"], P, zero, zero, d, ld)
    lens = np.diff(indptr).astype(np.float64)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    np.testing.assert_allclose(got["alpha"][1:-1], 1.0 / lens[rows], atol=1e-6, rtol=0)
    mean = np.zeros((n, d))
    np.add.at(mean, rows, P[indices, :d].astype(np.float64))
    mean[lens > 0] /= lens[lens > 0, None]
    _close(got["Z"][1:-1, :d], mean, "Z")


def run_backward(pgcn, graph, P, a_dst, a_src, G, d, ld):
    """forward (training) then backward on guarded outputs."""
    h, indptr, _ = graph
    n, nnz = len(indptr) - 1, int(indptr[-1])
    lib = pgcn.lib
    dP, dad, das, dG = _dev(P), _dev(a_dst), _dev(a_src), _dev(G)
    du, dv = _dev(np.zeros(n, np.float32)), _dev(np.zeros(n, np.float32))
    dZ, dal = _dev(np.full((n, ld), np.nan, np.float32)), _dev(np.zeros(max(nnz, 1), np.float32))
    ddP = _dev(_guarded(n, ld, -3.0))
    dda = _dev(np.full(2 * d + 2, GUARD, np.float32))
    ws_bytes = lib.pgcn_gat_bwd_workspace(h, d)
    assert ws_bytes > 0
    dws = _dev(np.zeros(ws_bytes // 4 + 4, np.float32))
    _sync()
    assert lib.pgcn_gat_scores(_p(dP), ld, n, d, _p(dad), _p(das), _p(du), _p(dv),
                               None) == pgcn.PGCN_OK
    assert lib.pgcn_gat_fwd(h, _p(dP), ld, _p(du), _p(dv), SLOPE, _p(dZ), ld, d, _p(dal),
                            None) == pgcn.PGCN_OK
    _sync()
    Z = dZ.cpu().numpy()
    Z[:, _up4(d):] = np.nan  # the padding of the backward's inputs is never read into the result
    dZ = _dev(Z)
    _sync()
    assert lib.pgcn_gat_bwd(h, _p(dP), ld, _p(du), _p(dv), SLOPE, _p(dal), _p(dZ), ld, _p(dG), ld,
                            _p(dad), _p(das), _p(ddP, 4 * ld), ld, d, _p(dda, 4), _p(dws),
                            None) == pgcn.PGCN_OK
    _sync()
    return dict(dP=ddP.cpu().numpy(), da=dda.cpu().numpy())


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld", WIDTHS)
def test_backward(pgcn, graphs, name, d, ld):
    """dP (atol 1e-6 max|ref|) and da (atol 1e-6 sqrt(n) max|ref|) against float64, rtol 1e-4;
    dP of the column without an incoming slot is du_j a_dst as the reference has it; padding
    columns of dP zero, further padding and the guards untouched; two calls give the same bits."""
    h, indptr, indices = graphs[name]
    n = len(indptr) - 1
    P, a_dst, a_src = _inputs(n, d, ld, 100 * d + n)
    rng = np.random.default_rng(9 * d + n)
    G = np.full((n, ld), np.nan, np.float32)
    G[:, :d] = rng.standard_normal((n, d)) * 0.5
    fwd = gat_ref.gat_forward(indptr, indices, P[:, :d], a_dst, a_src)
    assert np.abs(fwd["x"]).min() > 1e-6  # no slot at the LeakyReLU's kink
    ref = gat_ref.gat_backward(fwd, indptr, indices, P[:, :d], a_dst, a_src, G[:, :d])
    got = run_backward(pgcn, graphs[name], P, a_dst, a_src, G, d, ld)
    dP = got["dP"][1:-1]
    _close(dP[:, :d], ref["dP"], "dP")
    _close(got["da"][1:1 + d], ref["da_dst"], "da_dst", scale=np.sqrt(n))
    _close(got["da"][1 + d:1 + 2 * d], ref["da_src"], "da_src", scale=np.sqrt(n))
    if name == "hub":
        assert ref["dv"][299] == 0.0
        np.testing.assert_allclose(ref["dP"][299], ref["du"][299] * a_dst.astype(np.float64),
                                   rtol=1e-12)
    assert (dP[:, d:_up4(d)] == 0.0).all() and (dP[:, _up4(d):] == -3.0).all()
    assert (got["dP"][0] == GUARD).all() and (got["dP"][-1] == GUARD).all()
    assert got["da"][0] == GUARD and got["da"][-1] == GUARD
    again = run_backward(pgcn, graphs[name], P, a_dst, a_src, G, d, ld)
    for k in ("dP", "da"):
        np.testing.assert_array_equal(again[k].view(np.uint32), got[k].view(np.uint32), err_msg=k)


def test_counters_and_empty_call(pgcn, graphs):
    """"gat_fwd" / "gat_bwd" advance once per call; an n == 0 call is PGCN_OK and launches
    nothing."""
    h, indptr, indices = graphs["one"]
    P, a_dst, a_src = _inputs(1, 4, 4, 1)
    G = np.ones((1, 4), np.float32)
    pgcn.reset_path_counts()
    run_backward(pgcn, graphs["one"], P, a_dst, a_src, G, 4, 4)
    c = pgcn.path_counts()
    assert c["gat_fwd"] == 1 and c["gat_bwd"] == 1 and c["launches"] >= 5
    t = _dev(np.zeros(16, np.float32))
    before = pgcn.path_counts()["launches"]
    assert pgcn.lib.pgcn_gat_scores(_p(t), 4, 0, 4, _p(t), _p(t), _p(t), _p(t),
                                    None) == pgcn.PGCN_OK
    after = pgcn.path_counts()
    assert after["launches"] == before and after["gat_fwd"] == 1
    _sync()
