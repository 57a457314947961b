"""The multi-head graph attention kernels through the kernel ABI (pgcn_gat_scores_mh / _fwd_mh /
_bwd_mh) against the float64 reference of tests/gat_heads_ref.py (checked itself in
tests/test_cpu_gat_heads.py), on the graphs of tests/test_gpu_gat_kernels.py: the 300-node hub
graph (a 4,100-slot row, segmented columns, an empty row, a one-slot row, rows of 63 / 64 / 65
slots, a column without an incoming slot) and n = 1.  The bounds are that file's _close: rtol
1e-4, atol 1e-6 max|ref| (da: x sqrt(n), as there).  There is one kernel family: the single-head
entries are these kernels at heads = 1 with a null mask, so the tests that compare the two pin
the two sets of ABI entries to each other.
"""
import ctypes

import numpy as np
import pytest

import gat_heads_ref as ref_mh
from test_gpu_gat_kernels import (GRAPHS, GUARD, SLOPE, _close, _dev, _guarded, _inputs, _p, _sync,
                                  _up4, graphs)  # noqa: F401  (graphs: the module's fixture)

pytestmark = pytest.mark.gpu

# (d, ld, K): dh = 4 (one lane per head) at three group widths, dh = 8, 16, 64, one head over
# the full width, and a NaN-padded stride
CASES = [(8, 8, 2), (16, 16, 4), (128, 128, 32), (64, 64, 8), (128, 128, 8), (128, 128, 2),
         (128, 128, 1), (8, 12, 2)]


def _grad(n, d, ld, seed):
    rng = np.random.default_rng(seed)
    G = np.full((n, ld), np.nan, np.float32)
    G[:, :d] = rng.standard_normal((n, d)) * 0.5
    return G


def run_mh(pgcn, graph, P, a_dst, a_src, d, ld, K, G=None, bits=None, base=0, scale=1.0,
           training=True, old=False):
    """scores + forward (+ backward when G is given) on guarded outputs, through the _mh entries
    (old: the single-head entries pgcn_gat_scores / _fwd / _bwd, which reach the same kernels at
    heads = 1 without a mask); host copies with the guards."""
    h, indptr, _ = graph
    n, nnz = len(indptr) - 1, int(indptr[-1])
    lib = pgcn.lib
    dP, dad, das = _dev(P), _dev(a_dst), _dev(a_src)
    du = _dev(np.full(n * K + 2, GUARD, np.float32))
    dv = _dev(np.full(n * K + 2, GUARD, np.float32))
    dZ = _dev(_guarded(n, ld, -3.0))
    dal = _dev(np.full(nnz * K + 2, GUARD, np.float32)) if training else None
    dbits = _dev(bits.view(np.int64)) if bits is not None else None
    _sync()
    if old:
        assert K == 1 and bits is None
        assert lib.pgcn_gat_scores(_p(dP), ld, n, d, _p(dad), _p(das), _p(du, 4), _p(dv, 4),
                                   None) == pgcn.PGCN_OK
        assert lib.pgcn_gat_fwd(h, _p(dP), ld, _p(du, 4), _p(dv, 4), SLOPE, _p(dZ, 4 * ld), ld, d,
                                _p(dal, 4) if training else None, None) == pgcn.PGCN_OK
    else:
        assert lib.pgcn_gat_scores_mh(_p(dP), ld, n, d, K, _p(dad), _p(das), _p(du, 4), _p(dv, 4),
                                      None) == pgcn.PGCN_OK
        assert lib.pgcn_gat_fwd_mh(h, _p(dP), ld, _p(du, 4), _p(dv, 4), SLOPE, _p(dZ, 4 * ld), ld,
                                   d, K, _p(dbits), base, scale,
                                   _p(dal, 4) if training else None, None) == pgcn.PGCN_OK
    _sync()
    out = dict(u=du.cpu().numpy(), v=dv.cpu().numpy(), Z=dZ.cpu().numpy())
    if training:
        out["alpha"] = dal.cpu().numpy()
    if G is None:
        return out
    Z = out["Z"][1:-1].copy()
    Z[:, _up4(d):] = np.nan  # the padding of the backward's inputs is never read into the result
    dZin, dG = _dev(Z), _dev(G)
    ddP = _dev(_guarded(n, ld, -3.0))
    dda = _dev(np.full(2 * d + 2, GUARD, np.float32))
    ws_bytes = lib.pgcn_gat_bwd_workspace(h, d) if old else lib.pgcn_gat_bwd_workspace_mh(h, d, K)
    assert ws_bytes > 0
    dws = _dev(np.zeros(ws_bytes // 4 + 4, np.float32))
    _sync()
    if old:
        assert lib.pgcn_gat_bwd(h, _p(dP), ld, _p(du, 4), _p(dv, 4), SLOPE, _p(dal, 4), _p(dZin),
                                ld, _p(dG), ld, _p(dad), _p(das), _p(ddP, 4 * ld), ld, d,
                                _p(dda, 4), _p(dws), None) == pgcn.PGCN_OK
    else:
        assert lib.pgcn_gat_bwd_mh(h, _p(dP), ld, _p(du, 4), _p(dv, 4), SLOPE, _p(dal, 4),
                                   _p(dZin), ld, _p(dG), ld, _p(dad), _p(das), _p(ddP, 4 * ld),
                                   ld, d, K, _p(dbits), base, scale, _p(dda, 4), _p(dws),
                                   None) == pgcn.PGCN_OK
    _sync()
    out.update(dP=ddP.cpu().numpy(), da=dda.cpu().numpy())
    return out


def _same_bits(a, b, keys):
    for k in keys:
        np.testing.assert_array_equal(a[k].view(np.uint32), b[k].view(np.uint32), err_msg=k)


def _check_forward(got, ref, indptr, d, K, with_sums=True):
    n = len(indptr) - 1
    Z = got["Z"][1:-1]
    _close(got["u"][1:-1].reshape(n, K), ref["u"], "u")
    _close(got["v"][1:-1].reshape(n, K), ref["v"], "v")
    _close(Z[:, :d], ref["Z"], "Z")
    alpha = got["alpha"][1:-1].reshape(-1, K)
    _close(alpha, ref["alpha"], "alpha")
    lens = np.diff(indptr)
    if with_sums:
        for h in range(K):
            sums = np.bincount(ref["rows"], weights=alpha[:, h].astype(np.float64), minlength=n)
            np.testing.assert_allclose(sums[lens > 0], 1.0, atol=1e-5, rtol=0)
    assert (Z[lens == 0, :_up4(d)] == 0.0).all()
    assert (Z[:, d:_up4(d)] == 0.0).all() and (Z[:, _up4(d):] == -3.0).all()
    for k in ("u", "v", "alpha"):
        assert got[k][0] == GUARD and got[k][-1] == GUARD, k
    assert (got["Z"][0] == GUARD).all() and (got["Z"][-1] == GUARD).all()


def _check_backward(got, ref, n, d):
    dP = got["dP"][1:-1]
    _close(dP[:, :d], ref["dP"], "dP")
    _close(got["da"][1:1 + d], ref["da_dst"], "da_dst", scale=np.sqrt(n))
    _close(got["da"][1 + d:1 + 2 * d], ref["da_src"], "da_src", scale=np.sqrt(n))
    assert (dP[:, d:_up4(d)] == 0.0).all() and (dP[:, _up4(d):] == -3.0).all()
    assert (got["dP"][0] == GUARD).all() and (got["dP"][-1] == GUARD).all()
    assert got["da"][0] == GUARD and got["da"][-1] == GUARD


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld,K", CASES)
def test_forward_backward(pgcn, graphs, name, d, ld, K):
    """Z, alpha, u, v, dP, da against float64; every head's alpha sums to 1 per non-empty row
    within 1e-5; the empty row of Z exactly 0; guards untouched; columns [d, round_up4(d)) zero,
    further padding left alone; an eval forward and a second call give the same bits."""
    h, indptr, indices = graphs[name]
    n = len(indptr) - 1
    P, a_dst, a_src = _inputs(n, d, ld, 100 * d + n + K)
    a_dst, a_src = a_dst * np.float32(np.sqrt(K)), a_src * np.float32(np.sqrt(K))
    G = _grad(n, d, ld, 9 * d + n + K)
    fwd = ref_mh.gat_forward_mh(indptr, indices, P[:, :d], a_dst, a_src, K)
    assert np.abs(fwd["x"]).min() > 1e-6  # no slot at the LeakyReLU's kink
    bwd = ref_mh.gat_backward_mh(fwd, indptr, indices, P[:, :d], a_dst, a_src, G[:, :d])
    got = run_mh(pgcn, graphs[name], P, a_dst, a_src, d, ld, K, G=G)
    _check_forward(got, fwd, indptr, d, K)
    _check_backward(got, bwd, n, d)
    ev = run_mh(pgcn, graphs[name], P, a_dst, a_src, d, ld, K, training=False)
    _same_bits(ev, got, ("Z",))
    again = run_mh(pgcn, graphs[name], P, a_dst, a_src, d, ld, K, G=G)
    _same_bits(again, got, ("u", "v", "Z", "alpha", "dP", "da"))


@pytest.mark.parametrize("d,ld,K", [(8, 8, 2), (64, 64, 8), (128, 128, 32)])
def test_heads_of_different_scale(pgcn, graphs, d, ld, K):
    """Head 0's scores span +-80, the other heads' stay within a few units of 0: a maximum or
    an exponent sum shared across heads would wipe out the small heads' weights (exp(-70)
    against the wide head's maximum) or flatten the wide one's."""
    h, indptr, indices = graphs["hub"]
    n, dh = len(indptr) - 1, d // K
    P, a_dst, a_src = _inputs(n, d, ld, 7 * d + K + 1)
    x = ref_mh.gat_forward_mh(indptr, indices, P[:, :d], a_dst, a_src, K)["x"]
    k = np.full(d, np.sqrt(K), np.float32)
    k[:dh] = np.float32(80.0 / np.abs(x[:, 0]).max())
    a_dst, a_src = a_dst * k, a_src * k
    G = _grad(n, d, ld, 5 * d + K)
    fwd = ref_mh.gat_forward_mh(indptr, indices, P[:, :d], a_dst, a_src, K)
    assert fwd["x"][:, 0].max() > 50 and fwd["x"][:, 0].min() < -60
    assert np.abs(fwd["x"][:, 1:]).max() < 10
    assert np.abs(fwd["x"]).min() > 1e-6  # no slot at the LeakyReLU's kink
    bwd = ref_mh.gat_backward_mh(fwd, indptr, indices, P[:, :d], a_dst, a_src, G[:, :d])
    got = run_mh(pgcn, graphs["hub"], P, a_dst, a_src, d, ld, K, G=G)
    assert np.isfinite(got["Z"][1:-1, :d]).all() and np.isfinite(got["alpha"][1:-1]).all()
    _check_forward(got, fwd, indptr, d, K)
    _check_backward(got, bwd, n, d)


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld", [(3, 4), (8, 8), (16, 16), (20, 20), (64, 64), (128, 128)])
def test_one_head_without_mask_is_the_single_head_entry(pgcn, graphs, name, d, ld):
    """heads = 1 with a null mask through the _mh entries: the bits of pgcn_gat_scores / _fwd /
    _bwd, forward and backward, at one width inside every lane-group size (the single-head
    entries are the same kernels behind their own argument checks)."""
    h, indptr, indices = graphs[name]
    n = len(indptr) - 1
    P, a_dst, a_src = _inputs(n, d, ld, 31 * d + n)
    G = _grad(n, d, ld, 17 * d + n)
    old = run_mh(pgcn, graphs[name], P, a_dst, a_src, d, ld, 1, G=G, old=True)
    new = run_mh(pgcn, graphs[name], P, a_dst, a_src, d, ld, 1, G=G)
    _same_bits(new, old, ("u", "v", "Z", "alpha", "dP", "da"))


MASKED = [(8, 8, 2, 0), (64, 64, 8, 77), (128, 128, 32, 64), (128, 128, 2, 1), (16, 16, 1, 5),
          (3, 4, 1, 0)]


@pytest.mark.parametrize("d,ld,K,base", MASKED)
def test_mask_against_float64(pgcn, graphs, d, ld, K, base):
    """Random keep bits at p = 0.6 (scale 2.5), read from bit drop_base on (the bits below it
    are the complement of a kept slot, so an ignored base shows): Z, dP, da against float64;
    alpha is the weight before dropout (it still sums to 1)."""
    h, indptr, indices = graphs["hub"]
    n, nnz = len(indptr) - 1, int(indptr[-1])
    P, a_dst, a_src = _inputs(n, d, ld, 13 * d + K)
    G = _grad(n, d, ld, 3 * d + K)
    keep = np.random.default_rng(d + K).random((nnz, K)) >= 0.6
    scale = float(np.float32(1.0 / (1.0 - 0.6)))
    bits = ref_mh.pack_bits(keep, base=base, fill=False)
    fwd = ref_mh.gat_forward_mh(indptr, indices, P[:, :d], a_dst, a_src, K, keep=keep, scale=scale)
    assert np.abs(fwd["x"]).min() > 1e-6  # no slot at the LeakyReLU's kink
    bwd = ref_mh.gat_backward_mh(fwd, indptr, indices, P[:, :d], a_dst, a_src, G[:, :d])
    got = run_mh(pgcn, graphs["hub"], P, a_dst, a_src, d, ld, K, G=G, bits=bits, base=base,
                 scale=scale)
    _check_forward(got, fwd, indptr, d, K)
    _check_backward(got, bwd, n, d)
    again = run_mh(pgcn, graphs["hub"], P, a_dst, a_src, d, ld, K, G=G, bits=bits, base=base,
                   scale=scale)
    _same_bits(again, got, ("Z", "alpha", "dP", "da"))


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("d,ld,K", [(8, 8, 2), (64, 64, 8), (128, 128, 32), (16, 16, 1),
                                    (3, 4, 1), (128, 128, 1)])
def test_all_ones_mask_is_the_null_mask(pgcn, graphs, name, d, ld, K):
    """An all-ones mask with scale 1 gives the null mask's bits; at one head the null-mask call
    goes through the single-head entries (the same kernels at heads = 1 behind their own
    argument checks)."""
    h, indptr, indices = graphs[name]
    n, nnz = len(indptr) - 1, int(indptr[-1])
    P, a_dst, a_src = _inputs(n, d, ld, 11 * d + K + n)
    G = _grad(n, d, ld, 19 * d + K + n)
    bits = ref_mh.pack_bits(np.ones(nnz * K, bool), base=3, fill=False)
    plain = run_mh(pgcn, graphs[name], P, a_dst, a_src, d, ld, K, G=G, old=K == 1)
    ones = run_mh(pgcn, graphs[name], P, a_dst, a_src, d, ld, K, G=G, bits=bits, base=3, scale=1.0)
    _same_bits(ones, plain, ("u", "v", "Z", "alpha", "dP", "da"))


@pytest.mark.parametrize("d,ld,K", [(8, 8, 2), (64, 64, 8)])
def test_one_slot_row_dropped_in_head_0(pgcn, graphs, d, ld, K):
    """Row 2 has one slot; dropped in head 0 only, head 0's columns of Z_2 are exact zeros and
    the other heads' the undropped bits."""
    h, indptr, indices = graphs["hub"]
    n, nnz, dh = len(indptr) - 1, int(indptr[-1]), d // K
    assert indptr[3] - indptr[2] == 1
    P, a_dst, a_src = _inputs(n, d, ld, 23 * d + K)
    keep = np.ones((nnz, K), bool)
    keep[indptr[2], 0] = False
    bits = ref_mh.pack_bits(keep, fill=False)
    plain = run_mh(pgcn, graphs["hub"], P, a_dst, a_src, d, ld, K)
    got = run_mh(pgcn, graphs["hub"], P, a_dst, a_src, d, ld, K, bits=bits, scale=1.0)
    row, want = got["Z"][1:-1][2], plain["Z"][1:-1][2]
    assert (row[:dh] == 0.0).all() and np.abs(want[:dh]).min() > 0
    np.testing.assert_array_equal(row[dh:].view(np.uint32), want[dh:].view(np.uint32))
    others = np.delete(np.arange(n), 2)
    np.testing.assert_array_equal(got["Z"][1:-1][others].view(np.uint32),
                                  plain["Z"][1:-1][others].view(np.uint32))
    np.testing.assert_array_equal(got["alpha"].view(np.uint32), plain["alpha"].view(np.uint32))


def test_launch_counts(pgcn, graphs):
    """Eight heads launch as many kernels as one head on the hub graph, forward and backward;
    "gat_heads" counts the calls with heads > 1."""
    h, indptr, indices = graphs["hub"]
    n, d = len(indptr) - 1, 64
    P, a_dst, a_src = _inputs(n, d, d, 5)
    G = _grad(n, d, d, 6)
    counts = {}
    for K in (1, 8):
        pgcn.reset_path_counts()
        run_mh(pgcn, graphs["hub"], P, a_dst, a_src, d, d, K, G=G)
        counts[K] = pgcn.path_counts()
    # scores; forward + its long rows' merge; rows, columns + their merge, da + its reduction
    assert counts[8]["launches"] == counts[1]["launches"] == 8, counts
    for K in (1, 8):
        assert counts[K]["gat_fwd"] == 1 and counts[K]["gat_bwd"] == 1
    assert counts[1]["gat_heads"] == 0 and counts[8]["gat_heads"] == 2


def test_refusals(pgcn, graphs):
    """The head rules with a real graph: PGCN_E_INVALID and nothing launched."""
    h, indptr, indices = graphs["one"]
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    t, z, al = (_dev(np.zeros(4 * 132, np.float32)) for _ in range(3))
    bits = _dev(np.full(8, -1, np.int64))
    _sync()
    before = pgcn.path_counts()["launches"]

    def fwd(d, K, mask=None, alpha=al, ld=128):
        return lib.pgcn_gat_fwd_mh(h, _p(t), ld, _p(t), _p(t), SLOPE, _p(z), ld, d, K, _p(mask), 0,
                                   1.0, _p(alpha), None)

    def bwd(d, K, ld=128):
        return lib.pgcn_gat_bwd_mh(h, _p(t), ld, _p(t), _p(t), SLOPE, _p(t), _p(t), ld, _p(t), ld,
                                   _p(t), _p(t), _p(t), ld, d, K, None, 0, 1.0, _p(t), _p(t), None)

    def scores(d, K, ld=128):
        return lib.pgcn_gat_scores_mh(_p(t), ld, 1, d, K, _p(t), _p(t), _p(t), _p(t), None)

    for d, K in ((8, 0), (8, -1), (8, 4), (24, 2), (48, 2), (16, 3), (128, 64), (6, 2)):
        assert fwd(d, K) == INV and bwd(d, K) == INV and scores(d, K) == INV, (d, K)
        assert lib.pgcn_gat_bwd_workspace_mh(h, d, K) == 0
    assert fwd(8, 2, mask=bits, alpha=None) == INV
    assert fwd(8, 1, mask=bits, alpha=None) == INV
    assert pgcn.path_counts()["launches"] == before
    assert fwd(8, 2, mask=bits) == pgcn.PGCN_OK and fwd(8, 2, alpha=None) == pgcn.PGCN_OK
    assert lib.pgcn_gat_bwd_workspace_mh(h, 8, 2) > 0
    _sync()
