"""The BatchNorm kernels through the kernel ABI (pgcn_batchnorm_fwd / _bwd, include/pgcn.h)
against the float64 restatements of tests/batchnorm_ref.py.

Shapes: a width per lane-group class plus ragged ones; per width n = 1, 2, R - 1, R, R + 1,
3 R + 5 and 16 R + 1 (17 tiles: the merge's second level), R = pgcn_batchnorm_tile_rows(d); one
forward case of 4,097 tiles (more than the merge's 64 slots squared).  ld > d with NaN in the padding.
"""
import numpy as np
import pytest

import batchnorm_ref as ref
from test_gpu_layernorm import _dev, _host, _p, _sync, _up4

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 16, 20, 64, 100, 128, 256, 260, 1024)


def _tile_rows(d):
    """The launcher's tile height (k_batchnorm.hip), checked against the library in _fwd."""
    d4 = (d + 3) // 4
    lanes = 4 if d4 <= 4 else 16 if d4 <= 16 else 32 if d4 <= 32 else 64
    return 256 // lanes * 16 // (1 if d4 <= 64 else 2 if d4 <= 128 else 4)


SHAPES = [(d, n) for d in WIDTHS for R in [_tile_rows(d)]
          for n in (1, 2, R - 1, R, R + 1, 3 * R + 5, 16 * R + 1)]
MANY_TILES = (17, 4097 * _tile_rows(17))


def _inputs(n, d, ld):
    """Column c ~ N(100 (c % 3), 1): the case an uncentred variance fails.  NaN padding."""
    rng = np.random.default_rng(1000 * d + n)
    x = np.full((n, ld), np.nan, np.float32)
    x[:, :d] = rng.standard_normal((n, d)) + 100.0 * (np.arange(d) % 3)
    gamma = (1.0 + 0.5 * rng.standard_normal(d)).astype(np.float32)
    return x, gamma, rng.standard_normal(d).astype(np.float32)


def _fwd(pgcn, x, gamma, beta, n, d, ld, training=True, in_place=False, tail=None):
    lib = pgcn.lib
    dx = _dev(x)
    dy = dx if in_place else _dev(np.full((n, ld), 7.25, np.float32))
    dxh = _dev(np.full((n, ld), 7.25, np.float32)) if training else None
    dst = _dev(np.full(2 * _up4(d), 7.25, np.float32))
    ws = lib.pgcn_batchnorm_fwd_workspace(n, d)
    assert lib.pgcn_batchnorm_tile_rows(d) == _tile_rows(d)
    assert ws == -(-n // _tile_rows(d)) * (4 + 2 * _up4(d)) * 4
    dws, dg, db = _dev(np.zeros(ws // 4, np.float32)), _dev(gamma), _dev(beta)
    args = [_p(dx), ld, _p(dy), ld, n, d, _p(dg), _p(db), ref.BN_EPS, _p(dxh), ld, _p(dst),
            _p(dws)]
    _sync()
    if tail is None:
        st = lib.pgcn_batchnorm_fwd(*args, None)
    else:
        st = lib.pgcn_debug_batchnorm_fwd_tail(*args, _p(tail["relu"]), ld, _p(tail["res"]), ld,
                                               _p(tail["mask"]), tail["base"], tail["scale"], None)
    assert st == pgcn.PGCN_OK
    _sync()
    return dict(y=_host(dy), xhat=_host(dxh) if training else None,
                stats=_host(dst).reshape(2, -1))


@pytest.mark.parametrize("d,n", SHAPES + [MANY_TILES])
def test_forward(pgcn, d, n):
    """y, xhat and stats against float64.  rstd: rtol 1e-4, LayerNorm's.  y / xhat: LayerNorm's
    rtol 1e-4 and atol 1e-5 PLUS, per column, 2 * 2^-23 |mean_c| rstd_c (times |gamma_c| for y):
    a float32 mean near 200 is only known to an ulp, 1.5e-5, so xhat = (x - mean) rstd inherits up
    to that times rstd whatever the summation -- LayerNorm's rows have means below 4.  A float32
    numpy restatement of the pivoted tile passes and the merge, on these inputs, is off float64 on
    xhat by 6.6e-6 at d 16, n 16,385 (0.63 of LayerNorm's tolerance, 0.11 of the one used here),
    by 1.0e-5 at d 256, n 1,025 (0.96 / 0.17) and by 1.2e-3 at d 256, n 2, where rstd reaches 188
    (12.8 / 0.16): not inside LayerNorm's bound, well inside this one.  The mean itself: 2 ulp.  n = 1: xhat = 0, y = beta, rstd = 1 / sqrtf(eps).  Padding columns of the
    outputs are zero; an eval call (no xhat), an in-place call and a second call give the same
    bits."""
    ld = _up4(d) + 4
    x, gamma, beta = _inputs(n, d, ld)
    got = _fwd(pgcn, x, gamma, beta, n, d, ld)
    want_y, want_xhat, want_mean, want_rstd = ref.fwd(x[:, :d], gamma, beta)
    mean, rstd = got["stats"][0, :d], got["stats"][1, :d]
    np.testing.assert_allclose(mean, want_mean, rtol=2.4e-7, atol=1e-6)
    np.testing.assert_allclose(rstd, want_rstd, rtol=1e-4)
    atol = 1e-5 + 2.0 ** -22 * np.abs(want_mean) * want_rstd
    for name, a, want, tol in (("xhat", got["xhat"], want_xhat, atol),
                               ("y", got["y"], want_y, atol * np.maximum(np.abs(gamma), 1.0))):
        err = np.abs(a[:, :d] - want) / (tol + 1e-4 * np.abs(want))
        print(f"d {d} n {n}: worst {name} error {err.max():.3g} of the tolerance")
        assert err.max() <= 1.0, name
        assert (a[:, d:_up4(d)] == 0.0).all() and (a[:, _up4(d):] == 7.25).all(), name
    if n == 1:
        np.testing.assert_array_equal(got["xhat"][0, :d], np.zeros(d, np.float32))
        np.testing.assert_array_equal(got["y"][0, :d], beta)
        np.testing.assert_allclose(rstd, np.float32(1.0) / np.sqrt(np.float32(1e-5)), rtol=2.4e-7)
    for kw in (dict(), dict(training=False), dict(in_place=True)) if (d, n) != MANY_TILES else ():
        again = _fwd(pgcn, x, gamma, beta, n, d, ld, **kw)
        w = _up4(d)
        np.testing.assert_array_equal(again["y"][:, :w].view(np.uint32),
                                      got["y"][:, :w].view(np.uint32), err_msg=str(kw))
        np.testing.assert_array_equal(again["stats"], got["stats"], err_msg=str(kw))
        if again["xhat"] is not None:
            np.testing.assert_array_equal(again["xhat"], got["xhat"], err_msg=str(kw))


def _bwd(pgcn, dy, xhat, stats, gamma, n, d, ld, in_place=False):
    lib = pgcn.lib
    ddy, dxh, dst, dg = _dev(dy), _dev(xhat), _dev(stats), _dev(gamma)
    ddx = ddy if in_place else _dev(np.full((n, ld), 7.25, np.float32))
    dgb = _dev(np.full((2, d + 2), 7.25, np.float32))
    ws = lib.pgcn_batchnorm_bwd_workspace(n, d)
    assert ws > 0
    dws = _dev(np.zeros(ws // 4, np.float32))
    _sync()
    st = lib.pgcn_batchnorm_bwd(_p(ddy), ld, _p(dxh), ld, _p(dst), _p(dg), n, d, _p(ddx), ld,
                                _p(dgb, 4), _p(dgb, 4 * (d + 3)), _p(dws), None)
    assert st == pgcn.PGCN_OK
    _sync()
    return dict(dx=_host(ddx), gb=_host(dgb))


@pytest.mark.parametrize("d,n", SHAPES)
def test_backward(pgcn, d, n):
    """dx (rtol 1e-4, atol 1e-6 max|dy|) and dgamma / dbeta (rtol 1e-4, atol 1e-6 sqrt(n) max|dy|)
    against float64 from the same inputs; in place on dy and a second call give the same bits;
    padding columns of dx zero, the words around dgamma / dbeta untouched.  xhat ~ N(0, 1) and
    rstd in [0.5, 2] are drawn, not taken from a forward: at n = 2 a forward's rstd reaches the
    hundreds, and no float32 evaluation holds 1e-6 max|dy| on a difference scaled by that."""
    ld = _up4(d) + 4
    rng = np.random.default_rng(7 * d + n)
    dy, xhat = (np.full((n, ld), np.nan, np.float32) for _ in range(2))
    dy[:, :d] = rng.standard_normal((n, d)) * 0.5
    xhat[:, :d] = rng.standard_normal((n, d))
    stats = np.zeros((2, _up4(d)), np.float32)
    stats[1, :d] = rng.uniform(0.5, 2.0, d)
    gamma = (1.0 + 0.5 * rng.standard_normal(d)).astype(np.float32)
    got = _bwd(pgcn, dy, xhat, stats, gamma, n, d, ld)
    want_dx, want_dg, want_db = ref.bwd(dy[:, :d], xhat[:, :d], stats[1, :d], gamma)
    big = float(np.abs(dy[:, :d]).max())
    np.testing.assert_allclose(got["dx"][:, :d], want_dx, rtol=1e-4, atol=1e-6 * big)
    for row, want in ((0, want_dg), (1, want_db)):
        np.testing.assert_allclose(got["gb"][row, 1:-1], want, rtol=1e-4,
                                   atol=1e-6 * np.sqrt(n) * big)
    assert (got["dx"][:, d:_up4(d)] == 0.0).all() and (got["dx"][:, _up4(d):] == 7.25).all()
    assert (got["gb"][:, 0] == 7.25).all() and (got["gb"][:, -1] == 7.25).all()
    for in_place in (False, True):
        again = _bwd(pgcn, dy, xhat, stats, gamma, n, d, ld, in_place=in_place)
        w = _up4(d)
        np.testing.assert_array_equal(again["dx"][:, :w].view(np.uint32),
                                      got["dx"][:, :w].view(np.uint32))
        np.testing.assert_array_equal(again["gb"], got["gb"])


@pytest.mark.parametrize("d,n", [(16, 1029), (20, 300), (128, 133), (256, 67), (516, 40)])
def test_fused_tail(pgcn, d, n):
    """pgcn_debug_batchnorm_fwd_tail against pgcn_batchnorm_fwd -> pgcn_relu_fwd ->
    pgcn_residual_fwd -> pgcn_dropout_apply, bit for bit (output, ReLU mask bytes, xhat); base 61:
    a row's first 4-bit dropout group straddles two mask words."""
    lib, base = pgcn.lib, 61
    x, gamma, beta = _inputs(n, d, d)
    rng = np.random.default_rng(d + n)
    res = rng.standard_normal((n, d)).astype(np.float32)
    words = rng.integers(0, 2 ** 63, size=(base + n * d) // 64 + 3, dtype=np.uint64)
    bits = np.unpackbits(words.view(np.uint8), bitorder="little")
    shifted = np.packbits(np.concatenate([bits[base:], np.zeros(64 + base, np.uint8)]),
                          bitorder="little").view(np.uint64)
    scale = np.float32(2.0)
    dm = _dev(np.full((n, d), 9, np.uint8))
    tail = dict(relu=dm, res=_dev(res), mask=_dev(words), base=base, scale=scale)
    got = _fwd(pgcn, x, gamma, beta, n, d, d, tail=tail)
    plain = _fwd(pgcn, x, gamma, beta, n, d, d)
    dy, dm2, dsh = _dev(plain["y"]), _dev(np.full((n, d), 9, np.uint8)), _dev(shifted.copy())
    _sync()
    assert lib.pgcn_relu_fwd(_p(dy), n * d, _p(dm2), 1, None) == pgcn.PGCN_OK
    assert lib.pgcn_residual_fwd(_p(dy), _p(tail["res"]), n * d, None) == pgcn.PGCN_OK
    assert lib.pgcn_dropout_apply(_p(dy), n * d, _p(dsh), scale, None) == pgcn.PGCN_OK
    _sync()
    np.testing.assert_array_equal(got["y"].view(np.uint32), _host(dy).view(np.uint32))
    np.testing.assert_array_equal(_host(dm), _host(dm2))
    np.testing.assert_array_equal(got["xhat"], plain["xhat"])


def test_argument_checks(pgcn):
    """Bad ld, d > 1024, a NULL required pointer or rows off the 16-byte grid: PGCN_E_INVALID
    with nothing launched (the outputs keep their fill); n == 0 is OK."""
    n, d, ld = 5, 8, 8
    x, gamma, beta = _inputs(n, d, ld)
    dx, dg, db = _dev(x), _dev(gamma), _dev(beta)
    dy, dxh = (_dev(np.full((n, ld), 7.25, np.float32)) for _ in range(2))
    dst, dws = _dev(np.full(2 * ld, 7.25, np.float32)), _dev(np.zeros(1 << 12, np.float32))
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    _sync()

    def fwd(ld_x=ld, ld_y=ld, n_=n, d_=d, y=dy, st=dst, ws=dws, ld_xh=ld, off=0):
        return lib.pgcn_batchnorm_fwd(_p(dx, off), ld_x, _p(y), ld_y, n_, d_, _p(dg), _p(db),
                                      ref.BN_EPS, _p(dxh), ld_xh, _p(st), _p(ws), None)
    assert fwd(ld_x=6) == INV and fwd(ld_y=4) == INV and fwd(ld_y=10) == INV and fwd(d_=0) == INV
    assert fwd(d_=1025, ld_x=1028, ld_y=1028, ld_xh=1028) == INV and fwd(n_=-1) == INV
    assert fwd(y=None) == INV and fwd(st=None) == INV and fwd(ws=None) == INV
    assert fwd(ld_xh=4) == INV and fwd(off=4, n_=n - 1) == INV
    assert fwd(n_=0) == pgcn.PGCN_OK and fwd(n_=0, y=None) == pgcn.PGCN_OK

    def bwd(ld_dy=ld, n_=n, d_=d, out=dy, dgam=dxh, ws=dws):
        return lib.pgcn_batchnorm_bwd(_p(dx), ld_dy, _p(dx), ld, _p(dst), _p(dg), n_, d_, _p(out),
                                      ld, _p(dgam), _p(dst), _p(ws), None)
    assert bwd(ld_dy=6) == INV and bwd(d_=1025) == INV and bwd(out=None) == INV
    assert bwd(dgam=None) == INV and bwd(ws=None) == INV and bwd(n_=0) == pgcn.PGCN_OK
    x12, dm = _dev(np.zeros((n, 12), np.float32)), _dev(np.zeros((n, 12), np.uint8))
    assert lib.pgcn_debug_batchnorm_fwd_tail(  # the tail needs ld_y == d
        _p(x12), 12, _p(x12), 12, n, d, _p(dg), _p(db), ref.BN_EPS, None, 0, _p(dst), _p(dws),
        _p(dm), 12, None, 0, None, 0, 1.0, None) == INV
    _sync()
    for t in (dy, dxh, dst):
        assert (_host(t) == 7.25).all()
    assert lib.pgcn_batchnorm_fwd_workspace(0, 16) == 0 == lib.pgcn_batchnorm_bwd_workspace(0, 16)
