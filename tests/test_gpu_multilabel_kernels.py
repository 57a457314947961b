"""The multi-label kernels through the kernel ABI (k_multilabel.hip): pgcn_bce_fwd,
pgcn_predict_multilabel_rows and pgcn_multilabel_counts.

For the labelled rows (truth >= 0), logits x and target bits y, columns < c:
    loss  = sum [ max(x, 0) - x y + log1p(exp(-|x|)) ]      per block of R rows
    wrong = #{(x > 0) != y}                                   per block of R rows
    grad  = (sigmoid(x) - y) / count, zero on unlabelled rows and in columns [c, ld)
The reference is a float64 numpy restatement in this file on the same float32 logits, with the
conventions of tests/test_gpu_layernorm.py: guard rows around every output buffer, NaN in the
padding columns of the inputs.

Gradient bound: 2^-21 / count absolute.  Derived: sigmoid - y = +-(1 or e) / (1 + e) with e =
exp(-|x|) from the device exp (1 ulp) and three roundings of half an ulp each (1 + e, the
quotient, the division by count) on values <= 1: 5 * 2^-24 / count; the bound leaves 1.6x.
Largest error seen on the MI355X over every case below: 2.44 * 2^-24 / count.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 7.25
GUARD_BITS = 0xA5A5A5A5


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _p(t, byte_offset=0):
    return ctypes.c_void_p(t.data_ptr() + byte_offset) if t is not None else None


def _host(t, dtype=None):
    a = t.cpu().numpy()
    return a.view(dtype) if dtype is not None else a


def _sync():
    import torch
    torch.cuda.synchronize()


def _up4(c):
    return (c + 3) // 4 * 4


@pytest.fixture(scope="module")
def R(pgcn):
    """PGCN_XENT_ROWS, from pgcn_xent_blocks: the largest n that one block covers."""
    r = 1
    while pgcn.lib.pgcn_xent_blocks(r + 1) == 1:
        r += 1
    assert pgcn.lib.pgcn_xent_blocks(r) == 1 and pgcn.lib.pgcn_xent_blocks(3 * r + 5) == 4
    return r


def _logits(n, c, ld, seed):
    """Standard normal x 3 with entries at exactly 0, +-100 and +-1e4; NaN in [c, ld)."""
    rng = np.random.default_rng(seed)
    x = np.full((n, ld), np.nan, np.float32)
    v = (3.0 * rng.standard_normal((n, c))).astype(np.float32)
    special = np.array([0.0, -0.0, 100.0, -100.0, 1e4, -1e4], np.float32)
    k = max(1, n * c // 8)
    v.reshape(-1)[rng.choice(n * c, k, replace=False)] = special[rng.integers(0, 6, k)]
    if n * c >= 6:
        v.reshape(-1)[rng.choice(n * c, 6, replace=False)] = special
    # the first and the last row keep one plain entry: a labelled set made of +-100 / +-1e4
    # entries alone can have a loss of 1e-44, which no float32 holds to 1e-4 relative
    v[0, 0], v[-1, 0] = keep = (3.0 * rng.standard_normal(2)).astype(np.float32)
    assert abs(keep[0]) < 20 and abs(keep[1]) < 20
    x[:, :c] = v
    return x


def _truth(n, rows, rng):
    if rows == "all":
        t = rng.integers(0, 5, n)
    elif rows == "third":  # every third row unlabelled
        t = np.where(np.arange(n) % 3 == 2, -1, rng.integers(0, 5, n))
    else:  # only the last row labelled
        t = np.full(n, -1)
        t[-1] = 0
    return t.astype(np.int32)


def _targets(n, c, kind, rng):
    if kind == "zeros":
        return np.zeros((n, c), bool)
    if kind == "ones":
        return np.ones((n, c), bool)
    return rng.random((n, c)) < 0.4


def _reference(x, Y, truth, c, count, R):
    """float64: (per-block loss sums, per-block wrong counts, grad [n][c])."""
    x64 = x[:, :c].astype(np.float64)
    y = Y.astype(np.float64)
    lab = (truth >= 0)[:, None]
    e = np.exp(-np.abs(x64))
    loss = (np.maximum(x64, 0.0) - x64 * y + np.log1p(e)) * lab
    sig = np.where(x64 >= 0, 1.0, e) / (1.0 + e)
    grad = (sig - y) / count * lab
    wrong = ((x[:, :c] > 0) != Y) & lab
    nb = (len(x) + R - 1) // R
    pad = nb * R - len(x)
    lb = np.pad(loss.sum(axis=1), (0, pad)).reshape(nb, R).sum(axis=1)
    wb = np.pad(wrong.sum(axis=1), (0, pad)).reshape(nb, R).sum(axis=1)
    return lb, wb, grad


class _Bce:
    """Device buffers of one problem, every output between guards."""

    def __init__(self, pgcn, x, Y, truth, c, ld):
        self.pgcn, self.n, self.c, self.ld = pgcn, len(x), c, ld
        self.words = (c + 31) // 32
        self.nb = pgcn.lib.pgcn_xent_blocks(self.n)
        self.x = _dev(x)
        self.bits = _dev(pgcn.pack_label_bits(Y))
        self.truth = _dev(truth)

    def run(self, count, training=True, grad=True):
        n, ld, nb = self.n, self.ld, self.nb
        g = _dev(np.full((n + 2, ld), GUARD, np.float32))
        part = _dev(np.full(2 * nb + 2, GUARD, np.float32))
        _sync()
        st = self.pgcn.lib.pgcn_bce_fwd(_p(self.x), ld, _p(g, 4 * ld) if grad else None,
                                        _p(self.truth), _p(self.bits), self.words, n, self.c,
                                        count, 1 if training else 0, _p(part, 4), None)
        assert st == self.pgcn.PGCN_OK
        _sync()
        return _host(g), _host(part)


CLASSES = (1, 3, 31, 32, 33, 41, 64, 65, 128)
worst_grad = {}


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("c", CLASSES)
def test_bce_forward(pgcn, R, c, pad):
    """Every n in {1, R - 1, R, R + 1, 3 R + 5} x label pattern x target pattern at this (c, ld),
    with count = labelled rows * c and count = 7."""
    ld = _up4(c) + pad
    worst = 0.0
    for n in (1, R - 1, R, R + 1, 3 * R + 5):
        assert n * c < 2 ** 24
        for ri, rows in enumerate(("all", "third", "last")):
            for ti, kind in enumerate(("zeros", "ones", "random")):
                seed = ((c * 8 + pad) * 1000 + n) * 16 + ri * 4 + ti
                rng = np.random.default_rng(seed)
                x = _logits(n, c, ld, seed + 1)
                truth, Y = _truth(n, rows, rng), _targets(n, c, kind, rng)
                lab = truth >= 0
                prob = _Bce(pgcn, x, Y, truth, c, ld)
                what = f"c {c} ld {ld} n {n} rows {rows} targets {kind}"
                first = None
                for count in (int(lab.sum()) * c, 7):
                    lb, wb, grad = _reference(x, Y, truth, c, count, R)
                    g, part = prob.run(count)
                    # wrong: exact per block; loss: finite, its sum within 1e-4 relative
                    np.testing.assert_array_equal(part[2:-1:2], wb.astype(np.float32), what)
                    got_l = part[1:-1:2].astype(np.float64)
                    assert np.isfinite(got_l).all(), what
                    assert abs(got_l.sum() - lb.sum()) <= 1e-4 * abs(lb.sum()), \
                        (what, got_l.sum(), lb.sum())
                    # gradient: 2^-21 / count absolute; zero in the padding and unlabelled rows
                    err = np.abs(g[1:-1, :c].astype(np.float64) - grad).max() * count
                    worst = max(worst, err)
                    assert err <= 2.0 ** -21, (what, count, err)
                    assert (g[1:-1, c:] == 0.0).all(), what
                    assert (g[1:-1][~lab] == 0.0).all(), what
                    # guards untouched, logits bit-unchanged
                    assert (g[0] == GUARD).all() and (g[-1] == GUARD).all(), what
                    assert part[0] == GUARD and part[-1] == GUARD, what
                    np.testing.assert_array_equal(_host(prob.x, np.uint32), x.view(np.uint32))
                    if first is None:
                        first = (g, part)
                        g2, part2 = prob.run(count)  # two calls: identical bits
                        np.testing.assert_array_equal(g2.view(np.uint32), g.view(np.uint32))
                        np.testing.assert_array_equal(part2.view(np.uint32), part.view(np.uint32))
                # eval: the same partials, no grad written (given or NULL)
                count = int(lab.sum()) * c
                g, part = prob.run(count, training=False)
                assert (g == GUARD).all(), what
                np.testing.assert_array_equal(part.view(np.uint32), first[1].view(np.uint32))
                g, part = prob.run(count, training=False, grad=False)
                np.testing.assert_array_equal(part.view(np.uint32), first[1].view(np.uint32))
    worst_grad[(c, pad)] = worst
    print(f"c {c} ld {ld}: largest gradient error {worst * 2.0 ** 24:.3f} x 2^-24 / count "
          f"(bound 8, derived 5)")


def test_bce_argument_checks(pgcn):
    """Each bad argument: PGCN_E_INVALID and nothing written; n == 0: PGCN_OK, nothing written."""
    n, c, ld = 5, 6, 8
    x = _dev(_logits(n, c, ld, 1))
    g = _dev(np.full((n, ld), GUARD, np.float32))
    part = _dev(np.full(4, GUARD, np.float32))
    truth = _dev(np.zeros(n, np.int32))
    bits = _dev(np.zeros((n, 1), np.uint32))
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    _sync()

    def call(ld_=ld, words=1, n_=n, c_=c, count=30):
        return lib.pgcn_bce_fwd(_p(x), ld_, _p(g), _p(truth), _p(bits), words, n_, c_, count, 1,
                                _p(part), None)
    assert call(c_=0) == INV and call(c_=129, ld_=132, words=5) == INV
    assert call(ld_=4) == INV and call(ld_=6) == INV and call(ld_=10) == INV
    assert call(words=0) == INV and call(words=2) == INV
    assert call(count=0) == INV and call(count=-1) == INV
    assert call(n_=0) == pgcn.PGCN_OK
    _sync()
    assert (_host(g) == GUARD).all() and (_host(part) == GUARD).all()


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("c", CLASSES)
def test_predict_rows(pgcn, R, c, pad):
    """bits == (x > 0) exactly, bits >= c zero; probs within 2^-22 of the float64 sigmoid, zero
    in [c, round_up4(c)), further padding and the guard rows left alone; logits unchanged."""
    ld, words = _up4(c) + pad, (c + 31) // 32
    ldp = _up4(c) + 8 - pad
    for n in (1, R - 1, R, R + 1, 3 * R + 5):
        x = _logits(n, c, ld, 77 * c + n + pad)
        dx = _dev(x)
        db = _dev(np.full((n + 2, words), GUARD_BITS, np.uint32))
        dp = _dev(np.full((n + 2, ldp), GUARD, np.float32))
        _sync()
        for probs in (True, False):
            st = pgcn.lib.pgcn_predict_multilabel_rows(
                _p(dx), ld, n, c, _p(db, 4 * words), words, _p(dp, 4 * ldp) if probs else None,
                ldp, None)
            assert st == pgcn.PGCN_OK
            _sync()
            bits = _host(db, np.uint32)
            assert (bits[0] == GUARD_BITS).all() and (bits[-1] == GUARD_BITS).all()
            np.testing.assert_array_equal(bits[1:-1], pgcn.pack_label_bits(x[:, :c] > 0))
        pr = _host(dp)
        x64 = x[:, :c].astype(np.float64)
        e = np.exp(-np.abs(x64))
        want = np.where(x64 >= 0, 1.0, e) / (1.0 + e)
        err = np.abs(pr[1:-1, :c].astype(np.float64) - want).max()
        assert err <= 2.0 ** -22, (c, ld, n, err)
        assert (pr[1:-1, c:_up4(c)] == 0.0).all()
        assert (pr[1:-1, _up4(c):] == GUARD).all()
        assert (pr[0] == GUARD).all() and (pr[-1] == GUARD).all()
        np.testing.assert_array_equal(_host(dx, np.uint32), x.view(np.uint32))


@pytest.mark.parametrize("c", CLASSES)
def test_counts(pgcn, R, c):
    """tp, fp, fn per class equal numpy's, rows with truth < 0 skipped; the call zeroes counts."""
    words = (c + 31) // 32
    for n in (1, R + 1, 3 * R + 5, 4099):
        rng = np.random.default_rng(5 * c + n)
        P, Y = rng.random((n, c)) < 0.5, rng.random((n, c)) < 0.3
        truth = np.where(rng.random(n) < 0.25, -1, 0).astype(np.int32)
        truth[0] = 0
        lab = (truth >= 0)[:, None]
        want = np.stack([(P & Y & lab).sum(0), (P & ~Y & lab).sum(0), (~P & Y & lab).sum(0)])
        dc = _dev(np.full((3 * c + 2,), GUARD_BITS, np.uint32))
        dpb, dyb, dt = _dev(pgcn.pack_label_bits(P)), _dev(pgcn.pack_label_bits(Y)), _dev(truth)
        _sync()
        for _ in range(2):  # the second call starts from the first one's counts: zeroed again
            st = pgcn.lib.pgcn_multilabel_counts(_p(dpb), _p(dyb), _p(dt), n, c, words,
                                                 _p(dc, 4), None)
            assert st == pgcn.PGCN_OK
            _sync()
            got = _host(dc, np.uint32)
            assert got[0] == GUARD_BITS and got[-1] == GUARD_BITS
            np.testing.assert_array_equal(got[1:-1].reshape(3, c), want.astype(np.uint32))
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    assert lib.pgcn_multilabel_counts(_p(dpb), _p(dyb), _p(dt), n, c, words + 1, _p(dc, 4),
                                      None) == INV
    assert lib.pgcn_multilabel_counts(_p(dpb), _p(dyb), _p(dt), n, 0, words, _p(dc, 4),
                                      None) == INV
    assert lib.pgcn_multilabel_counts(_p(dpb), _p(dyb), _p(dt), n, c, words, None, None) == INV
    assert lib.pgcn_multilabel_counts(None, None, None, 0, c, words, _p(dc, 4), None) == \
        pgcn.PGCN_OK
    _sync()
    assert (_host(dc, np.uint32)[1:-1] == 0).all()  # n == 0: zeroed, nothing counted


def test_predict_argument_checks(pgcn):
    n, c, ld = 5, 6, 8
    x = _dev(_logits(n, c, ld, 2))
    b = _dev(np.full((n, 1), GUARD_BITS, np.uint32))
    pr = _dev(np.full((n, ld), GUARD, np.float32))
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    _sync()

    def call(ld_=ld, n_=n, c_=c, words=1, bits=b, ldp=ld):
        return lib.pgcn_predict_multilabel_rows(_p(x), ld_, n_, c_, _p(bits), words, _p(pr), ldp,
                                                None)
    assert call(c_=0) == INV and call(c_=129, ld_=132, words=5) == INV
    assert call(ld_=4) == INV and call(ld_=6) == INV and call(words=2) == INV
    assert call(ldp=4) == INV and call(ldp=6) == INV and call(bits=None) == INV
    assert call(n_=0) == pgcn.PGCN_OK
    _sync()
    assert (_host(b, np.uint32) == GUARD_BITS).all() and (_host(pr) == GUARD).all()
