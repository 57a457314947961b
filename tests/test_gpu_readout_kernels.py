"""The readout kernels through the kernel ABI -- pgcn_readout_fwd / _bwd -- against the numpy
formulas of tests/readout_ref.py.  T = pgcn_readout_chunk_rows() is the length above which a range
is cut into pieces.

Calls:
  edges:  the range lengths 0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 T + 5 in one call, an empty
          range first and last (the long ranges start at row offsets that are no multiple of T, so
          first and last pieces are partial and a row block holds pieces of two long ranges).
  tiny:   1,000 ranges of 1..3 rows.
  one:    G = 1 over 2 T + 77 rows.
  short:  every range <= T (one launch).

Bounds.  Sum and mean against float64, per element: |err| <= len 2^-24 sum|x| for any summation
order (each of the len - 1 adds rounds by at most 2^-24 of a partial sum no larger than sum|x|),
plus 2 2^-24 |ref| for the mean's reciprocal and product.  Nothing is measured.  The max rounds
nothing: values and arg equal numpy's float32 maximum and first argmax bit for bit.  The backward
copies, scales by one float32 factor or selects: bit-exact against the same float32 statements.
"""
import ctypes

import numpy as np
import pytest

import readout_ref as rr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SENTINEL = 7.25
WIDTHS = (1, 3, 4, 16, 17, 64, 128)


def _up4(d):
    return (d + 3) // 4 * 4


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _sync():
    import torch
    torch.cuda.synchronize()


def _ptr_of(lens):
    gp = np.zeros(len(lens) + 1, np.int32)
    gp[1:] = np.cumsum(lens)
    return gp


def calls(T):
    rng = np.random.default_rng(5)
    return {
        "edges": _ptr_of([0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5, 0]),
        "tiny": _ptr_of(rng.integers(1, 4, 1000)),
        "one": _ptr_of([2 * T + 77]),
        "short": _ptr_of([T, 0, 5, T - 1, 40, 1, T]),
    }


@pytest.fixture(scope="module")
def T(pgcn):
    return int(pgcn.lib.pgcn_readout_chunk_rows())


def _input(n, d, ld, seed):
    """[n][ld]: N(0, 1) in the d columns, NaN in the padding."""
    rng = np.random.default_rng(seed)
    x = np.full((n, ld), np.nan, np.float32)
    x[:, :d] = rng.standard_normal((n, d)).astype(np.float32)
    return x


def run_fwd(pgcn, gp, x, d, mode, want_arg=True, max_len=None):
    """(out, arg) host copies [G][ld] with the sentinel behind round_up4(d)."""
    G, n, ld = len(gp) - 1, x.shape[0], x.shape[1]
    lens = np.diff(gp)
    max_len = int(lens.max()) if max_len is None else max_len
    out = _dev(np.full((G, ld), SENTINEL, np.float32))
    arg = _dev(np.full((G, ld), 77, np.int32)) if want_arg else None
    import torch
    ws = torch.empty(max(int(pgcn.lib.pgcn_readout_workspace(n)), 16), dtype=torch.uint8,
                     device="cuda")
    dx, dgp = _dev(x), _dev(gp)
    pgcn.check(pgcn.lib.pgcn_readout_fwd(_p(dx), ld, _p(dgp), G, n, d, rr.MODE_ID[mode], max_len,
                                         _p(out), ld, _p(arg), ld, _p(ws), None), "readout_fwd")
    _sync()
    return out.cpu().numpy(), (arg.cpu().numpy() if want_arg else None)


def check_padding(a, d, fill, sentinel):
    """Columns [d, round_up4(d)) hold `fill`, those behind them the untouched sentinel."""
    u = _up4(d)
    assert (a[:, d:u] == fill).all()
    assert (a[:, u:] == sentinel).all()


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", ["edges", "tiny", "one"])
def test_forward(pgcn, T, name, d):
    gp = calls(T)[name]
    n, ld = int(gp[-1]), _up4(d) + 8
    x = _input(n, d, ld, 100 + d)
    lens = np.diff(gp).astype(np.float64)
    x64 = x[:, :d].astype(np.float64)
    mag, _ = rr.readout_forward(gp, np.abs(x64), "sum")
    for mode in ("sum", "mean"):
        out, arg = run_fwd(pgcn, gp, x, d, mode)
        ref, _ = rr.readout_forward(gp, x64, mode)
        bound = lens[:, None] * EPS * mag
        if mode == "mean":
            bound = bound / np.maximum(lens, 1)[:, None] + 2 * EPS * np.abs(ref)
        err = np.abs(out[:, :d].astype(np.float64) - ref)
        assert (err <= bound).all(), (mode, float((err - bound).max()))
        assert (out[lens == 0][:, :d] == 0).all()
        check_padding(out, d, 0.0, SENTINEL)
        assert (arg[:, :_up4(d)] == -1).all()
        check_padding(arg, d, -1, 77)
    out, arg = run_fwd(pgcn, gp, x, d, "max")
    ref, rarg = rr.readout_forward(gp, x[:, :d], "max")
    assert out[:, :d].tobytes() == ref.tobytes()
    assert (arg[:, :d] == rarg).all()
    check_padding(out, d, 0.0, SENTINEL)
    check_padding(arg, d, -1, 77)


@pytest.mark.parametrize("d", (3, 64))
def test_max_ties(pgcn, T, d):
    """Planted exact ties inside a lane's rows, across lanes, across waves and across pieces, and
    a -0.0 / +0.0 tie: the lowest row wins."""
    gp = calls(T)["edges"]
    n, ld = int(gp[-1]), _up4(d)
    x = _input(n, d, ld, 9)
    x[:, :d] = -np.abs(x[:, :d]) - 1.0  # every planted value is the maximum
    for g in range(len(gp) - 1):
        b, e = int(gp[g]), int(gp[g + 1])
        if e - b >= 2:
            for k, (r0, r1) in enumerate([(b + (e - b) // 2, e - 1), (b, e - 1), (b, b + 1)]):
                c = k % d
                x[r0, c] = x[r1, c] = 5.0 if k else 0.0
                if not k:
                    x[r0, c], x[r1, c] = -0.0, 0.0
    out, arg = run_fwd(pgcn, gp, x, d, "max")
    ref, rarg = rr.readout_forward(gp, x[:, :d], "max")
    assert (out[:, :d] == ref).all()
    assert (arg[:, :d] == rarg).all()
    long_g = len(gp) - 3  # the 3 T + 5 range: its tie spans pieces
    assert arg[long_g, 1 % d] == gp[long_g]


@pytest.mark.parametrize("name", ["edges", "tiny"])
def test_forward_without_arg_and_loose_max_len(pgcn, T, name):
    """arg NULL (an inference call), and max_len = n as an upper bound: the same bits."""
    gp = calls(T)[name]
    n, d = int(gp[-1]), 17
    x = _input(n, d, _up4(d), 3)
    for mode in rr.MODES:
        a, _ = run_fwd(pgcn, gp, x, d, mode)
        b, none = run_fwd(pgcn, gp, x, d, mode, want_arg=False, max_len=n)
        assert none is None
        if name == "tiny":  # (edges: max_len = n also exceeds T, the same kernels)
            assert a.tobytes() == b.tobytes()
        assert a[:, :d].tobytes() == b[:, :d].tobytes()


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", ["edges", "tiny", "one"])
def test_backward(pgcn, T, name, d):
    gp = calls(T)[name]
    G, n, ld = len(gp) - 1, int(gp[-1]), _up4(d) + 4
    x = _input(n, d, ld, 200 + d)
    g = _input(G, d, ld, 300 + d)
    ng = rr.node_graph(gp).astype(np.int32)
    lens = np.diff(gp)
    _, rarg = rr.readout_forward(gp, x[:, :d], "max")
    arg = np.full((G, ld), 12345, np.int32)
    arg[:, :d] = rarg
    dg, dgp, dng, darg = _dev(g), _dev(gp), _dev(ng), _dev(arg)
    for mode in rr.MODES:
        din = _dev(np.full((n, ld), np.nan, np.float32))
        pgcn.check(pgcn.lib.pgcn_readout_bwd(_p(dg), ld, _p(dgp), _p(dng),
                                             _p(darg) if mode == "max" else None, ld, G, n, d,
                                             rr.MODE_ID[mode], _p(din), ld, None), "readout_bwd")
        _sync()
        got = din.cpu().numpy()
        want = g[ng][:, :d]
        if mode == "mean":
            want = want * (np.float32(1) / lens[ng].astype(np.float32))[:, None]
        elif mode == "max":
            want = np.where(rarg[ng] == np.arange(n)[:, None], want, np.float32(0))
        assert got.shape[0] == n  # (rows of empty ranges do not exist)
        assert got[:, :d].tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), mode
        u = _up4(d)
        assert (got[:, d:u] == 0).all() and np.isnan(got[:, u:]).all()


def test_two_calls_same_bits(pgcn, T):
    gp = calls(T)["edges"]
    n, d = int(gp[-1]), 64
    x = _input(n, d, d, 1)
    for mode in rr.MODES:
        a, aa = run_fwd(pgcn, gp, x, d, mode)
        b, ba = run_fwd(pgcn, gp, x, d, mode)
        assert a.tobytes() == b.tobytes() and aa.tobytes() == ba.tobytes()


def test_short_ranges_take_one_launch(pgcn, T):
    gp = calls(T)["short"]
    assert np.diff(gp).max() <= T < gp[-1]
    n, d = int(gp[-1]), 16
    x = _input(n, d, d, 2)
    for mode in rr.MODES:
        pgcn.reset_path_counts()
        out, _ = run_fwd(pgcn, gp, x, d, mode)
        assert pgcn.path_counts()["launches"] == 1
        ref, _ = rr.readout_forward(gp, x.astype(np.float64), mode)
        assert np.allclose(out, ref, rtol=0, atol=T * EPS * np.abs(x).sum(axis=0).max())
    pgcn.reset_path_counts()
    run_fwd(pgcn, calls(T)["edges"], _input(int(calls(T)["edges"][-1]), d, d, 2), d, "sum")
    assert pgcn.path_counts()["launches"] == 3
