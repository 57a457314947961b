"""Kernel-level tests of the loss family (k_elementwise.hip: xent_tile plain and fused with the
output layer, its fused finish, k_reduce_scalars) and of the block reductions of the output
layer's weight-grad partials (k_gemm.hip), through the debug entries of include/pgcn.h.

References: numpy float32 where the kernel's arithmetic is exact or IEEE (the max shift, the
wrong count, the table's products, the reductions' documented order), the library's own
separate kernels where kernels.hpp claims the same bits (pgcn_gemm + pgcn_xent_fwd), float64
everywhere else.  Every output buffer and a guard past it is filled with a NaN pattern, every
ld padding of an input with NaN; nothing outside an entry's contract may change and no padding
may reach a result.

Bounds.  Products: 1e-5 * sum|terms| + 1e-30 (test_gemm_nn / test_gemm_tn).  Scalars: 1e-5 *
sum|terms|, the terms being the rows' losses (and wd w^2 / 2); every test first checks on the
CPU that a float32 emulation in the worst order (one sequential sum) stays inside it for its
own inputs (a block's loss: inside a quarter of it).  Grad: |g - ref| <= 1e-5 |ref| + GRAD_A /
count, see GRAD_A.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64                       # floats past every output buffer
FILL = np.uint32(0x7FC5A5A5)     # a quiet NaN with a payload: the fill of outputs and padding
XR = 64                          # rows per loss block (pgcn_xent_blocks)
SCALE = 1.0                      # the random logits' standard deviation

# The grad's absolute term.  prob - 1 at the true class cancels: prob carries the exp's and the
# sum's rounding (a few 2^-24 relative of prob <= 1) and the difference is then exact, so the
# error is absolute, ~1e-7, whatever is left of prob - 1.  LossRef.grad_emu restates the
# kernel's formula in numpy float32 (shift, exp, the (s0 + s1) + (s2 + s3) quad sum, IEEE
# divide, subtract, divide); over every case of test_xent_ladder, test_known_answer_rows and
# test_fused_output_layer (its logits taken as float32(H W)) the largest |emulation - float64|
# * count at a true-class entry is 9.98e-8 (fused, c = 3, kh = 8, n = 1000; the plain ladder's
# is 9.80e-8 at c = 5, n = 1000, ld = 12, all rows labelled).  GRAD_A is four times that: the
# device exp may differ from numpy's by an ulp.  Every case re-checks that its own emulation
# stays within GRAD_A / 2 (not / 4: the fused cases' logits come from the device GEMM, whose
# last bits the recorded figure did not see).
GRAD_A = 4 * 9.98e-8

# SCALE: with a standard deviation of 2 two blocks of the ladder that hold one labelled row
# whose true class wins by ~5 (loss 0.0034 and 0.0057: the float32 sum 1 + e^-5 alone is half an
# ulp of 1 off) left the block-loss bound in the CPU emulation (1.22 and 0.93 of it).  At 1 the
# emulation's worst block is at 0.07 of the bound (c = 2, n = 65, loss 0.073).


def vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def down(t):
    return t.cpu().numpy()


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(u32(a), u32(b))


def filled(*shape):
    return np.full(shape, FILL, np.uint32).view(np.float32)


def out_buf(nfloats):
    """A device output of nfloats plus the guard, all FILL."""
    return up(filled(nfloats + GUARD))


def untouched(a):
    return bool((u32(a) == FILL).all())


def r4(x):
    return (x + 3) // 4 * 4


def blocks(n):
    return (n + XR - 1) // XR


# ------------------------------------------------------------------------------------------
# inputs and references of the loss
# ------------------------------------------------------------------------------------------
LABELS = ("random", "all", "none", "one")


def make_truth(rng, n, c, pattern):
    if pattern == "random":
        t = np.where(rng.random(n) < 0.4, rng.integers(0, c, n), -1)
    elif pattern == "all":
        t = rng.integers(0, c, n)
    elif pattern == "none":
        t = np.full(n, -1)
    else:  # one labelled row: the last row of the last block
        t = np.full(n, -1)
        t[n - 1] = rng.integers(0, c)
    return t.astype(np.int32)


def special_rows(x, truth, c, rows, rng, force_label):
    """Rows with a known exact answer written over x[rows[k], :c] (kinds in order: equal, tie,
    ulp, big (true class), big (another class), huge); force_label: they get a label even where
    the pattern left them without one.  Returns {row: kind}."""
    kinds = {}
    for kind, i in zip(("equal", "tie", "ulp", "big_true", "big_other", "huge"), rows):
        if c < 2 and kind in ("tie", "ulp", "big_other"):
            continue
        t = int(truth[i])
        if t < 0:
            if not force_label:
                continue
            t = int(rng.integers(0, c))
            truth[i] = t
        j = (t + 1 + int(rng.integers(0, max(1, c - 1)))) % c if c > 1 else 0  # j != t
        if kind == "equal":
            x[i, :c] = np.float32(0.37)
        elif kind == "tie":      # the true class tied with the maximum: not wrong
            m = np.float32(x[i, :c].max() + 1.0)
            x[i, t] = m
            x[i, j] = m
        elif kind == "ulp":      # another class one ulp above the true one: wrong
            m = np.float32(x[i, :c].max() + 1.0)
            x[i, j] = m
            x[i, t] = np.nextafter(m, np.float32(-np.inf))
        elif kind == "big_true":  # one class 110 above the rest: their exps underflow to 0
            x[i, :c] = np.float32(-1.5)
            x[i, t] = np.float32(108.5)
        elif kind == "big_other":
            x[i, :c] = np.float32(-1.5)
            x[i, j] = np.float32(108.5)
        else:                    # magnitude 1e4, small differences: the max shift keeps it finite
            x[i, :c] = (1e4 + 0.5 * rng.standard_normal(c)).astype(np.float32)
        kinds[int(i)] = kind
    return kinds


def make_logits(rng, n, c, ld):
    x = filled(n, ld)            # columns [c, ld) stay NaN
    x[:, :c] = (SCALE * rng.standard_normal((n, c))).astype(np.float32)
    return x


def quad_sum(e, c):
    """The kernel's exp sum of each row in float32: lane q of the row's quad adds classes q,
    q + 4, ... in order, then (s0 + s1) + (s2 + s3)."""
    s = np.zeros((e.shape[0], 4), np.float32)
    for j in range(c):
        s[:, j & 3] = s[:, j & 3] + e[:, j]
    return (s[:, 0] + s[:, 1]) + (s[:, 2] + s[:, 3])


class LossRef:
    """Everything the loss kernel computes from logits x [n][>= c] (float32) and truth, on the
    CPU: the float32 shift and wrong flags (exact), the rows' loss and grad in float64 from the
    float32 shifted logits, and a float32 emulation of the kernel's own formulas."""

    def __init__(self, x, truth, c, count):
        n = x.shape[0]
        self.lab = np.flatnonzero(truth >= 0)
        xl = x[self.lab, :c]
        tl = truth[self.lab]
        idx = np.arange(len(tl))
        self.shifted = xl - xl.max(axis=1, keepdims=True)           # float32, as the kernel
        lt = self.shifted[idx, tl]
        self.wrong = np.zeros(n)
        self.wrong[self.lab] = (self.shifted > lt[:, None]).any(axis=1)
        s64 = self.shifted.astype(np.float64)
        e64 = np.exp(s64)
        se64 = e64.sum(axis=1)
        self.loss = np.zeros(n)                                    # float64 row losses
        self.loss[self.lab] = np.log(se64) - s64[idx, tl]
        onehot = np.zeros_like(e64)
        onehot[idx, tl] = 1.0
        self.grad = np.zeros((n, c))
        self.true_mask = np.zeros((n, c), bool)
        self.true_mask[self.lab, tl] = True
        if count > 0:
            self.grad[self.lab] = (e64 / se64[:, None] - onehot) / count
        # float32 emulation: exp, the quad sum, IEEE divide, subtract, divide; log and subtract
        with np.errstate(under="ignore"):
            e32 = np.exp(self.shifted)
        se32 = quad_sum(e32, c)
        prob = e32 / se32[:, None]
        prob[idx, tl] = prob[idx, tl] - np.float32(1.0)
        self.grad_emu = np.zeros((n, c), np.float32)
        if count > 0:
            self.grad_emu[self.lab] = prob / np.float32(count)
        self.loss_emu = np.zeros(n, np.float32)
        self.loss_emu[self.lab] = np.log(se32) - lt

    def grad_a_seen(self, count):
        """largest |emulation - float64| * count at a true-class entry (GRAD_A's measurement)"""
        d = np.abs(self.grad_emu.astype(np.float64) - self.grad)[self.true_mask]
        return float(d.max() * count) if d.size else 0.0

    def block_sums(self, n):
        """per block: float64 loss sum, exact wrong count, and the float32 emulation's loss
        summed sequentially (the worst order of up to 64 terms)"""
        nb = blocks(n)
        ls, ws, es = np.zeros(nb), np.zeros(nb), np.zeros(nb, np.float32)
        for b in range(nb):
            sl = slice(b * XR, min(n, (b + 1) * XR))
            ls[b] = self.loss[sl].sum()
            ws[b] = self.wrong[sl].sum()
            acc = np.float32(0.0)
            for v in self.loss_emu[sl]:
                acc = np.float32(acc + v)
            es[b] = acc
        return ls, ws, es


def check_loss_outputs(ref, truth, n, c, ld, count, training, logits0, logits, grad, partials,
                       what):
    """The contract of one loss launch (plain or fused) against LossRef: logits0 / logits are
    the buffer before / after [n][ld], grad [n][ld] or None, partials [2 blocks]."""
    lab = ref.lab
    unl = np.flatnonzero(truth < 0)
    # shifted logits of labelled rows bit for bit, everything else as it was
    assert same_bits(logits[lab, :c], ref.shifted), (what, "shift")
    assert same_bits(logits[lab, c:], logits0[lab, c:]), (what, "logits padding")
    assert same_bits(logits[unl], logits0[unl]), (what, "unlabelled rows")
    ls, ws, es = ref.block_sums(n)
    got_l, got_w = partials[0::2], partials[1::2]
    assert np.array_equal(got_w, ws), (what, "wrong", got_w, ws)
    bound = 1e-5 * ls
    assert (np.abs(es.astype(np.float64) - ls) <= bound / 4).all(), \
        (what, "inputs outside the bound")
    assert (np.abs(got_l.astype(np.float64) - ls) <= bound).all(), \
        (what, "block loss", got_l, ls)
    if not training:
        return
    assert ref.grad_a_seen(count) <= GRAD_A / 2, (what, "GRAD_A", ref.grad_a_seen(count))
    assert (u32(grad[:, c:]) == 0).all(), (what, "grad padding")
    assert (u32(grad[unl]) == 0).all(), (what, "grad of unlabelled rows")
    err = np.abs(grad[:, :c].astype(np.float64) - ref.grad)
    tol = 1e-5 * np.abs(ref.grad) + GRAD_A / max(count, 1)
    assert (err <= tol).all(), (what, "grad", float((err - tol).max()))


def check_known_rows(kinds, x, truth, c, count, training, logits, grad, what):
    """The exact answers of special_rows' rows that show in the row's own outputs."""
    cnt = np.float32(count)
    for i, kind in kinds.items():
        t = int(truth[i])
        g = grad[i, :c] if training else None
        if kind == "equal":
            assert (u32(logits[i, :c]) == 0).all(), (what, i, kind)
            if training:  # se = c exactly: the IEEE quotients 1 / c and (1 / c - 1), by count
                p = np.float32(1.0) / np.float32(c)
                want = np.full(c, p / cnt, np.float32)
                want[t] = (p - np.float32(1.0)) / cnt
                assert same_bits(g, want), (what, i, kind, g, want)
        elif kind in ("big_true", "big_other") and training:
            want = np.zeros(c, np.float32)   # the other probabilities are exactly +0.0
            if kind == "big_true":           # 1 / 1 - 1 = +0.0, by count: +0.0
                pass
            else:
                want[t] = np.float32(-1.0) / cnt
                want[int(np.argmax(x[i, :c]))] = np.float32(1.0) / cnt
            assert same_bits(g, want), (what, i, kind, g, want)
        elif kind == "huge":
            assert np.isfinite(logits[i, :c]).all() and (logits[i, :c] <= 0).all(), (what, i)
            if training:
                assert np.isfinite(g).all(), (what, i, kind)
        if c == 1 and training:
            assert (u32(g) == 0).all(), (what, i, "c = 1")


def run_xent(pg, x, truth, c, count, training, write_back, fin=None):
    """pgcn_debug_xent_fwd over a copy of x; returns (logits, grad, partials) with guards."""
    n, ld = x.shape
    dl = up(np.concatenate([x.ravel(), filled(GUARD)]))
    dg = out_buf(n * ld)
    dp = out_buf(2 * blocks(n))
    dt = up(truth)
    pg.check(pg.lib.pgcn_debug_xent_fwd(vp(dl), ld, vp(dg), vp(dt), n, c, count, training,
                                        vp(dp), write_back, ctypes.byref(fin) if fin else None,
                                        stream()), "debug_xent_fwd")
    torch.cuda.synchronize()
    return down(dl), down(dg), down(dp)


# ------------------------------------------------------------------------------------------
# a. the loss over given logits
# ------------------------------------------------------------------------------------------
C_LADDER = (1, 2, 3, 4, 5, 7, 8, 41, 47, 48, 49, 50, 63, 64, 65, 113, 121, 124)
N_LADDER = (1, 15, 16, 17, 63, 64, 65, 129, 1000)


def xent_cases(c):
    """Two cases per n for this c, walking the 32 (ld, training, write_back, labels)
    combinations so that the 324 cases of the ladder cover each of them about ten times."""
    ci = C_LADDER.index(c)
    for ni, n in enumerate(N_LADDER):
        for rep in range(2):
            k = ((ci * len(N_LADDER) + ni) * 5 + 17 * rep) % 32
            ld = r4(c) + (4 if (k & 1) and r4(c) + 4 <= 124 else 0)
            yield n, ld, 1 - ((k >> 1) & 1), 1 - ((k >> 2) & 1), LABELS[k >> 3]


@pytest.mark.parametrize("c", C_LADDER)
def test_xent_ladder(pgcn, c):
    for n, ld, training, write_back, pattern in xent_cases(c):
        what = dict(c=c, n=n, ld=ld, training=training, write_back=write_back, labels=pattern)
        rng = np.random.default_rng([c, n, ld, training, write_back, LABELS.index(pattern)])
        x = make_logits(rng, n, c, ld)
        truth = make_truth(rng, n, c, pattern)
        rows = [r for r in (3, 7, 9, 12, 14, n - 2) if 0 <= r < n - 1] if n >= 16 else []
        kinds = special_rows(x, truth, c, rows, rng, force_label=pattern == "random")
        count = int((truth >= 0).sum())
        ref = LossRef(x, truth, c, count)
        runs = [run_xent(pgcn, x, truth, c, count, training, write_back) for _ in range(2)]
        for a, b in zip(*runs):
            assert same_bits(a, b), (what, "run to run")
        lg, gr, pt = runs[0]
        assert untouched(lg[n * ld:]) and untouched(gr[n * ld:]) and \
            untouched(pt[2 * blocks(n):]), (what, "guards")
        lg, gr, pt = lg[:n * ld].reshape(n, ld), gr[:n * ld].reshape(n, ld), pt[:2 * blocks(n)]
        if not training:
            assert untouched(gr), (what, "grad written in eval")
        if not write_back:
            assert same_bits(lg, x), (what, "write_back = 0 wrote the logits")
            lg = x.copy()        # the rest of the contract, over the shift the kernel kept in LDS
            lg[ref.lab, :c] = ref.shifted
        check_loss_outputs(ref, truth, n, c, ld, count, training, x, lg, gr, pt, what)
        check_known_rows(kinds, x, truth, c, count, training, lg, gr, what)


# ------------------------------------------------------------------------------------------
# b. rows with a known exact answer, one per block: the block's partials are the row's own
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (1, 2, 3, 7, 41, 48, 49, 64, 124))
def test_known_answer_rows(pgcn, c):
    n, ld = 6 * XR, r4(c)
    rng = np.random.default_rng([77, c])
    x = make_logits(rng, n, c, ld)
    truth = np.full(n, -1, np.int32)
    rows = [XR * b + (17 * b + 5) % XR for b in range(6)]   # another wave and quad each
    kinds = special_rows(x, truth, c, rows, rng, force_label=True)
    count = int((truth >= 0).sum())
    ref = LossRef(x, truth, c, count)
    lg, gr, pt = run_xent(pgcn, x, truth, c, count, 1, 1)
    lg, gr, pt = lg[:n * ld].reshape(n, ld), gr[:n * ld].reshape(n, ld), pt[:12]
    what = dict(c=c)
    check_loss_outputs(ref, truth, n, c, ld, count, 1, x, lg, gr, pt, what)
    check_known_rows(kinds, x, truth, c, count, 1, lg, gr, what)
    for i, kind in kinds.items():
        loss, wrong = pt[2 * (i // XR)], pt[2 * (i // XR) + 1]
        if kind != "huge":   # (its random label: whatever check_loss_outputs counted)
            assert wrong == (1.0 if kind in ("ulp", "big_other") else 0.0), (c, kind, wrong)
        if c == 1 or kind == "big_true":
            assert u32(np.float32(loss)) == 0, (c, kind, loss)      # log(1) - 0
        elif kind == "big_other":
            assert loss == np.float32(110.0), (c, kind, loss)       # log(1) - (-110)
        elif kind == "equal":
            assert abs(float(loss) - np.log(c)) <= 1e-5 * np.log(c), (c, kind, loss)


# ------------------------------------------------------------------------------------------
# c. the output layer fused into the loss
# ------------------------------------------------------------------------------------------
def run_fused(pg, H, kh, W, c, ld, truth, count, training, lddh=0, with_dwp=False, table=None,
              fin=None):
    """pgcn_debug_out_xent; H [n][ldh], W [kh][ldw] host arrays (padding NaN).  Returns a dict
    of host arrays with their guards: logits, grad, partials, dH, dWp."""
    n, ldh = H.shape
    ldw = W.shape[1]
    nb = blocks(n)
    dHin = up(np.concatenate([H.ravel(), filled(GUARD)]))   # NaN past the inputs too
    dW, dt = up(np.concatenate([W.ravel(), filled(GUARD)])), up(truth)
    dl, dg, dp = out_buf(n * ld), out_buf(n * ld), out_buf(2 * nb)
    ddh = out_buf(n * lddh) if lddh else None
    ws = pg.lib.pgcn_debug_tn_reduce_blocks_workspace(nb, kh, 48) // 4
    ddw = out_buf(ws) if with_dwp else None
    tb = table or {}
    pg.check(pg.lib.pgcn_debug_out_xent(
        vp(dHin), ldh, kh, vp(dW), ldw, vp(dl), ld, vp(dg), vp(dt), n, c, count, training,
        vp(dp), vp(ddh), lddh, vp(ddw), vp(tb.get("table")), vp(tb.get("scale")),
        vp(tb.get("pos")), tb.get("rows", 0), ctypes.byref(fin) if fin else None, stream()),
        "debug_out_xent")
    torch.cuda.synchronize()
    return dict(logits=down(dl), grad=down(dg), partials=down(dp),
                dH=down(ddh) if lddh else None, dWp_dev=ddw,
                dWp=down(ddw) if with_dwp else None)


def fused_inputs(rng, n, c, kh, ldh, ldw):
    H = filled(n, ldh)
    H[:, :kh] = rng.standard_normal((n, kh)).astype(np.float32)
    W = filled(kh, ldw)
    # (0.25: the logits' standard deviation is SCALE at kh = 16, the range GRAD_A was taken at)
    W[:, :c] = (0.25 * rng.standard_normal((kh, c))).astype(np.float32)
    truth = make_truth(rng, n, c, "random")
    if (truth >= 0).sum() == 0:
        truth[n - 1] = rng.integers(0, c)
    return H, W, truth, int((truth >= 0).sum())


def separate_reference(pg, H, kh, W, c, ld, truth, count, training):
    """pgcn_gemm then pgcn_xent_fwd: what kernels.hpp says the fused kernel reproduces bit for
    bit.  (Aligned copies of H and W: the GEMM needs lda % 4 == 0.)"""
    n = H.shape[0]
    H2 = np.zeros((n, r4(kh)), np.float32)
    H2[:, :kh] = H[:, :kh]
    W2 = np.zeros((kh, r4(c)), np.float32)
    W2[:, :c] = W[:, :c]
    dH2, dW2, dt = up(H2), up(W2), up(truth)
    dl, dg, dp = out_buf(n * ld), out_buf(n * ld), out_buf(2 * blocks(n))
    pg.check(pg.lib.pgcn_gemm(n, c, kh, vp(dH2), r4(kh), vp(dW2), r4(c), 0, vp(dl), ld, None, 0,
                              0, 1.0, stream()), "gemm")
    torch.cuda.synchronize()
    raw = down(dl)[:n * ld].reshape(n, ld)
    pg.check(pg.lib.pgcn_xent_fwd(vp(dl), ld, vp(dg), vp(dt), n, c, count, training, vp(dp),
                                  stream()), "xent_fwd")
    torch.cuda.synchronize()
    return raw, down(dl), down(dg), down(dp), dW2


def fused_case(pg, c, ld, kh, n, ldh, ldw, lddh, training, with_dwp, seed):
    """One fused launch against the separate kernels (bits) and float64; returns the list of
    failed checks (empty: the case passes)."""
    rng = np.random.default_rng(seed)
    H, W, truth, count = fused_inputs(rng, n, c, kh, ldh, ldw)
    nb = blocks(n)
    bad = []

    def expect(ok, name):
        if not ok:
            bad.append(name)

    r = run_fused(pg, H, kh, W, c, ld, truth, count, training, lddh, with_dwp)
    r2 = run_fused(pg, H, kh, W, c, ld, truth, count, training, lddh, with_dwp)
    for k in ("logits", "grad", "partials", "dH", "dWp"):
        if r[k] is not None:
            expect(same_bits(r[k], r2[k]), "run to run " + k)
    expect(untouched(r["logits"][n * ld:]) and untouched(r["grad"][n * ld:]) and
           untouched(r["partials"][2 * nb:]), "guards")
    lg = r["logits"][:n * ld].reshape(n, ld)
    gr = r["grad"][:n * ld].reshape(n, ld)
    pt = r["partials"][:2 * nb]
    # float64: the raw logits H W within the product bound; shifted rows: the shift's own
    # rounding (2^-24 of the difference) and the max's error (at most the row's largest bound)
    H64, W64 = H[:, :kh].astype(np.float64), W[:, :c].astype(np.float64)
    z = H64 @ W64
    zb = 1e-5 * (np.abs(H64) @ np.abs(W64)) + 1e-30
    lab = truth >= 0
    expect((np.abs(lg[~lab, :c] - z[~lab]) <= zb[~lab]).all(), "raw logits vs float64")
    zs = z[lab] - z[lab].max(axis=1, keepdims=True)
    expect((np.abs(lg[lab, :c] - zs) <= zb[lab] + zb[lab].max(axis=1, keepdims=True) +
            1e-6 * np.abs(zs)).all(), "shifted logits vs float64")
    expect((u32(lg[:, c:]) == 0).all(), "logits padding not zero")
    # the separate kernels, bit for bit
    raw, sl, sg, sp, dW2 = separate_reference(pg, H, kh, W, c, ld, truth, count, training)
    expect(same_bits(lg, sl[:n * ld].reshape(n, ld)), "logits bits vs gemm + xent")
    expect(same_bits(pt, sp[:2 * nb]), "partials bits vs gemm + xent")
    # the loss's own contract (float64, exact shift and wrong count) from the unshifted logits
    # the separate GEMM wrote
    try:
        check_loss_outputs(LossRef(raw, truth, c, count), truth, n, c, ld, count, training, raw,
                           lg, gr, pt, "loss contract")
    except AssertionError as e:
        bad.append(str(e)[:300])
    if training:
        expect(same_bits(gr, sg[:n * ld].reshape(n, ld)), "grad bits vs gemm + xent")
    else:
        expect(untouched(r["grad"]), "grad written in eval")
        if lddh:
            expect(untouched(r["dH"]), "dH written in eval")
        if with_dwp:
            expect(untouched(r["dWp"]), "dWp written in eval")
        return bad
    g64 = gr.astype(np.float64)
    if lddh:
        dh = r["dH"]
        expect(untouched(dh[n * lddh:]), "dH rows >= n")
        dh = dh[:n * lddh].reshape(n, lddh)
        expect((u32(dh[:, kh:min(16, lddh)]) == 0).all(), "dH columns [kh, 16) not zero")
        expect(untouched(dh[:, 16:]), "dH columns >= 16")
        ref = g64[:, :c] @ W64.T
        rb = 1e-5 * (np.abs(g64[:, :c]) @ np.abs(W64).T) + 1e-30
        expect((np.abs(dh[:, :kh] - ref) <= rb).all(), "dH vs float64")
        # Matmul backward's product from the grad this launch wrote
        dgr = up(gr)
        dref = out_buf(n * r4(kh))
        pg.check(pg.lib.pgcn_gemm(n, kh, c, vp(dgr), ld, vp(dW2), r4(c), 1, vp(dref), r4(kh),
                                  None, 0, 0, 1.0, stream()), "gemm_t")
        torch.cuda.synchronize()
        sref = down(dref)[:n * r4(kh)].reshape(n, r4(kh))
        expect(same_bits(dh[:, :kh], sref[:, :kh]), "dH bits vs gemm")
    if with_dwp:
        dwp = r["dWp"]
        expect(untouched(dwp[nb * kh * 48:]), "dWp past the partials")
        part = dwp[:nb * kh * 48].reshape(nb, kh, 48)
        expect((u32(part[:, :, c:]) == 0).all(), "dWp columns [c, 48) not zero")
        ldc = r4(c)
        dC = out_buf(kh * ldc)
        pg.check(pg.lib.pgcn_debug_tn_reduce_blocks(vp(r["dWp_dev"]), nb, kh, c, 48, vp(dC), ldc,
                                                    stream()), "tn_reduce_blocks")
        torch.cuda.synchronize()
        C = down(dC)
        expect(untouched(C[kh * ldc:]), "W.grad guard")
        C = C[:kh * ldc].reshape(kh, ldc)
        expect((u32(C[:, c:]) == 0).all(), "W.grad padding not zero")
        wref = H64.T @ g64[:, :c]
        wb = 1e-5 * (np.abs(H64).T @ np.abs(g64[:, :c])) + 1e-30
        expect((np.abs(C[:, :c] - wref) <= wb).all(), "W.grad vs float64")
    return bad


def ldh_of(kh, k):
    """the ldh ladder: round_up4(kh), a wider multiple of 4, and kh itself when odd (no
    alignment: the scalar load path)"""
    opts = [r4(kh), r4(kh) + 8] + ([kh] if kh % 2 else [])
    return opts[k % len(opts)]


FUSED_C = (1, 3, 6, 7, 8, 16, 17, 32, 33, 41, 48, 49, 64, 100, 113, 116)
FUSED_KH = (1, 2, 3, 4, 5, 7, 8, 12, 13, 15)
# (c, ld, kh): the ladders at ld = round_up4(c) -- among them the four specialised triples (41,
# 44, 16), (7, 8, 16), (6, 8, 16), (3, 4, 16) -- and near misses of each on the generic path
FUSED_SHAPES = [(c, r4(c), 16) for c in FUSED_C] + \
    [(c, r4(c), kh) for kh in FUSED_KH for c in (3, 7, 41, 60)] + \
    [(41, 48, 16), (7, 12, 16), (6, 12, 16), (3, 8, 16), (6, 8, 15), (6, 8, 5), (116, 116, 3)]
FUSED_N = (1, 17, 64, 65, 1000)


@pytest.mark.parametrize("c,ld,kh", FUSED_SHAPES)
def test_fused_output_layer(pgcn, c, ld, kh):
    si = FUSED_SHAPES.index((c, ld, kh))
    fails = []
    for ni, n in enumerate(FUSED_N):
        # the thinning: each ladder walks on its own function of (shape, n), so that over the
        # shapes every n meets training and eval launches, and every ldh every lddh and ldw
        k = si * len(FUSED_N) + ni
        ldh = ldh_of(kh, k)
        ldw = c + 3 * ((k // 2) & 1)
        lddh = (16, r4(kh), 20)[(k // 3) % 3]
        training = 0 if (si + ni) % 5 == 3 else 1
        with_dwp = ld <= 48 and (k % 2 == 0 or n in (17, 1000))
        bad = fused_case(pgcn, c, ld, kh, n, ldh, ldw, lddh, training, with_dwp,
                         seed=[c, ld, kh, n])
        if bad:
            fails.append((dict(n=n, ldh=ldh, ldw=ldw, lddh=lddh, training=training,
                               dwp=with_dwp), bad))
        # without dH: the loss alone (dWp still allowed)
        if n == 65:
            bad = fused_case(pgcn, c, ld, kh, n, ldh, ldw, 0, 1, ld <= 48, seed=[c, ld, kh, n])
            if bad:
                fails.append((dict(n=n, ldh=ldh, ldw=ldw, lddh=0), bad))
    assert not fails, fails


@pytest.mark.parametrize("c,ld", [(7, 8), (41, 44), (10, 12), (60, 60)])
@pytest.mark.parametrize("mode", ["rows_n", "rows_700", "pos"])
def test_fused_table(pgcn, c, ld, mode):
    """The prescaled ring table of dH (kh = 16): three slices of RING_SR rows."""
    SR = pgcn.lib.pgcn_debug_ring_slice_rows()
    n, kh, slots = 1100, 16, 3 * SR
    assert 2 * SR < n <= slots
    rng = np.random.default_rng([c, ld, len(mode)])
    H, W, truth, count = fused_inputs(rng, n, c, kh, 16, c)
    scale = rng.uniform(0.05, 1.0, slots).astype(np.float32)
    if mode == "pos":  # a random injection into the slots, a tenth of the rows without one
        pos = rng.permutation(slots)[:n].astype(np.int32)
        pos[rng.random(n) < 0.1] = -1
        rows = 0
    else:
        rows = n if mode == "rows_n" else 700
        pos = np.where(np.arange(n) < rows, np.arange(n), -1).astype(np.int32)
    dtab = out_buf(slots * 16)
    tb = dict(table=dtab, scale=up(scale), pos=up(pos) if mode == "pos" else None, rows=rows)
    r = run_fused(pgcn, H, kh, W, c, ld, truth, count, 1, 16, False, tb)
    plain = run_fused(pgcn, H, kh, W, c, ld, truth, count, 1, 16, False)
    for k in ("logits", "grad", "partials", "dH"):
        assert same_bits(r[k], plain[k]), k
    dh = r["dH"][:n * 16].reshape(n, 16)
    want = filled(slots * 4, 4)                       # float4s
    for i in np.flatnonzero(pos >= 0):
        p = int(pos[i])
        for v in range(4):
            want[(p // SR) * 4 * SR + v * SR + p % SR] = scale[p] * dh[i, 4 * v:4 * v + 4]
    got = down(dtab)
    assert untouched(got[slots * 16:])
    got = got[:slots * 16].reshape(slots * 4, 4)
    assert same_bits(got, want), np.flatnonzero((u32(got) != u32(want)).any(axis=1))[:10]
    # eval: the table is not written
    dtab2 = out_buf(slots * 16)
    tb["table"] = dtab2
    run_fused(pgcn, H, kh, W, c, ld, truth, count, 0, 16, False, tb)
    assert untouched(down(dtab2))


# ------------------------------------------------------------------------------------------
# d. the fused finish
# ------------------------------------------------------------------------------------------
class Finish:
    """A pgcn_xent_final over fresh device buffers for `nb` blocks."""

    def __init__(self, pg, nb, group, w, wd, ctr, sums=True):
        ng = (nb + group - 1) // group if group else 0
        self.out2 = out_buf(12)
        self.sums = out_buf(2) if sums else None
        self.ticket = torch.zeros(16, dtype=torch.int32, device=DEV)
        self.part4 = out_buf(4 * nb)
        self.gticket = torch.zeros(16 * ng + 16, dtype=torch.int32, device=DEV) if group else None
        self.gpart4 = out_buf(4 * ng) if group else None
        self.w = up(w) if w is not None else None
        self.ctr = up(np.array(ctr, np.int32)) if ctr is not None else None
        f = pg.PgcnXentFinal()
        f.w = self.w.data_ptr() if w is not None else None
        f.n_w = len(w) if w is not None else 0
        f.wd = wd
        f.out2 = self.out2.data_ptr()
        f.ctr = self.ctr.data_ptr() if ctr is not None else None
        f.ring_cap = 3 if ctr is not None else 1
        f.sums = self.sums.data_ptr() if sums else None
        f.ticket = self.ticket.data_ptr()
        f.part4 = self.part4.data_ptr()
        f.group = group
        f.gticket = self.gticket.data_ptr() if group else None
        f.gpart4 = self.gpart4.data_ptr() if group else None
        self.c = f
        self.ng, self.nb = ng, nb

    def read(self):
        torch.cuda.synchronize()
        return dict(out2=down(self.out2), sums=down(self.sums) if self.sums is not None else None,
                    ticket=down(self.ticket),
                    gticket=down(self.gticket) if self.gticket is not None else None,
                    part4=down(self.part4))


@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("group", [0, 1, 3, 8, 64])
@pytest.mark.parametrize("kernel", ["xent", "fused"])
def test_fused_finish(pgcn, kernel, group, ring):
    n, c, ld, kh, wd = 453, 7, 8, 16, 5e-4
    nb = blocks(n)
    assert nb == 8
    rng = np.random.default_rng([453, group, ring])
    H, W, truth, count = fused_inputs(rng, n, c, kh, 16, c)
    x = make_logits(rng, n, c, ld)
    epoch = 7
    slot = 4 * (epoch % 3) if ring else 0

    def launch(fin):
        if kernel == "xent":
            lg, gr, pt = run_xent(pgcn, x, truth, c, count, 1, 1, fin)
            return dict(logits=lg, grad=gr, partials=pt)
        r = run_fused(pgcn, H, kh, W, c, ld, truth, count, 1, 16, True, None, fin)
        return {k: r[k] for k in ("logits", "grad", "partials", "dH", "dWp")}

    base = launch(None)
    pt = base["partials"][:2 * nb]
    shifted = base["logits"][:n * ld].reshape(n, ld)
    ref = LossRef(shifted, truth, c, count)          # the shift of shifted rows is the identity
    loss64, wrong = ref.loss.sum(), int(ref.wrong.sum())
    assert wrong == pt[1::2].sum()
    # the bound holds for the worst order of these inputs (one sequential float32 sum)
    assert abs(float(seq_sum32(ref.loss_emu[ref.lab])) - loss64) <= 1e-5 * loss64
    for w in (rng.standard_normal(1000).astype(np.float32), None):
        if w is not None:
            q64 = float((w.astype(np.float64) ** 2).sum())
            assert abs(float(seq_sum32(w * w)) - q64) <= 1e-5 * q64
        f = Finish(pgcn, nb, group, w, wd, [5, epoch] if ring else None, sums=w is not None)
        l2 = wd * float((w.astype(np.float64) ** 2).sum()) / 2 if w is not None else 0.0
        what = dict(kernel=kernel, group=group, ring=ring, w=w is not None)
        first = None
        for rep in range(2):                          # the second launch: nothing re-zeroed
            out = launch(f.c)
            for k, v in out.items():
                assert same_bits(v, base[k]), (what, rep, k)
            got = f.read()
            assert not got["ticket"].any(), (what, rep, "ticket")
            assert group == 0 or not got["gticket"].any(), (what, rep, "group tickets")
            o2 = got["out2"]
            keep = np.ones(o2.size, bool)
            keep[slot:slot + 2] = False
            assert untouched(o2[keep]), (what, rep, "out2 outside its slot")
            o = o2[slot:slot + 2]
            assert u32(o[1]) == u32(np.float32(count - wrong) / np.float32(count)), (what, o)
            want = loss64 / count + l2
            assert abs(float(o[0]) - want) <= 1e-5 * want, (what, o, want)
            if got["sums"] is not None:
                assert untouched(got["sums"][2:]), what
                assert got["sums"][1] == wrong, (what, got["sums"])
                assert abs(float(got["sums"][0]) - loss64) <= 1e-5 * loss64, (what, got["sums"])
            # pgcn_finalize from the same partials (the engine test's 1e-6)
            out4 = out_buf(4)
            dpt = up(pt)
            pgcn.check(pgcn.lib.pgcn_finalize(vp(dpt), nb, count, vp(f.w), f.c.n_w, wd, vp(out4),
                                              stream()), "finalize")
            torch.cuda.synchronize()
            o4 = down(out4)
            assert abs(float(o[0]) - float(o4[0])) <= 1e-6 * abs(float(o4[0])), (what, o, o4)
            assert u32(o[1]) == u32(o4[1]), (what, o, o4)
            if got["sums"] is not None:
                assert abs(float(got["sums"][0]) - float(o4[2])) <= 1e-6 * float(o4[2]), what
            if first is None:
                first = got
            else:
                for k in ("out2", "sums", "part4"):
                    assert got[k] is None or same_bits(got[k], first[k]), \
                        (what, "second launch", k)


# ------------------------------------------------------------------------------------------
# e. pgcn_finalize and the block reductions on synthetic partials
# ------------------------------------------------------------------------------------------
def seq_sum32(a):
    """one sequential float32 sum (the worst order)"""
    return np.add.accumulate(a.astype(np.float32), dtype=np.float32)[-1]


FIN_L2 = (1, 1023, 1025, 32768, 32769, 100003)


@pytest.mark.parametrize("n_blocks", [1, 2, 1023, 1024, 1025, 8192, 8193, 20000])
def test_finalize(pgcn, n_blocks):
    for li, n_l2 in enumerate(FIN_L2):
        wd = 5e-4 if (li + n_blocks) % 2 else 0.0
        rng = np.random.default_rng([n_blocks, n_l2])
        # One sequential float32 sum of 20,000 random losses or 100,003 random squares leaves
        # the bound (a random walk of half ulps of the running sum: ~0.7 of it at 100,003), so
        # the inputs' range is cut down to where the check below holds: losses on a 2^-8 grid
        # in [0.5, 1.5], weights on a 1/4 grid in [-2, 2].  What these sizes are here for is the
        # loops' second trips: an element dropped or counted twice moves a sum by far more.
        part = np.empty((n_blocks, 2), np.float32)
        part[:, 0] = rng.integers(128, 385, n_blocks) / 256.0
        part[:, 1] = rng.integers(0, 4, n_blocks)
        w = (rng.integers(-8, 9, n_l2) / 4.0).astype(np.float32)
        w[0] = 0.75  # sum w^2 > 0
        wrong = int(part[:, 1].sum())
        assert wrong < 2 ** 24
        count = wrong + 1000
        l64 = float(part[:, 0].astype(np.float64).sum())
        q64 = float((w.astype(np.float64) ** 2).sum())
        want = l64 / count + wd * q64 / 2
        # the bound holds for the worst order of these inputs
        assert abs(float(seq_sum32(part[:, 0])) - l64) <= 1e-5 * l64
        assert abs(float(seq_sum32(w * w)) - q64) <= 1e-5 * q64
        dpart, dw, out4 = up(part), up(w), out_buf(4)
        pgcn.check(pgcn.lib.pgcn_finalize(vp(dpart), n_blocks, count, vp(dw), n_l2, wd, vp(out4),
                                          stream()), "finalize")
        torch.cuda.synchronize()
        o = down(out4)
        what = dict(n_blocks=n_blocks, n_l2=n_l2, wd=wd, out=o[:4])
        assert untouched(o[4:]), what
        assert o[3] == wrong, what
        assert abs(float(o[2]) - l64) <= 1e-5 * l64, what
        assert abs(float(o[0]) - want) <= 1e-5 * want, what
        # on these grids every float32 sum is exact in any order (< 2^23 grid steps), so the
        # sums and the kernel's own composition of them (IEEE float32, no contraction) are too:
        # one element dropped or counted twice shows whatever the seed
        assert float(o[2]) == l64 and float(np.float32(q64)) == q64, what
        exact = np.float32(l64) / np.float32(count) + \
            np.float32(wd) * np.float32(q64) / np.float32(2.0)
        assert u32(o[0]) == u32(np.float32(exact)), (what, exact)
        assert u32(o[1]) == u32(np.float32(count - wrong) / np.float32(count)), what
        # the results-ring slot: only slot 4 * (epoch % ring_cap) changes, with the same bits
        ring, sums = out_buf(12), out_buf(2)
        ctr = up(np.array([9, 5], np.int32))
        pgcn.check(pgcn.lib.pgcn_debug_finalize_ring(vp(dpart), n_blocks, count, vp(dw), n_l2, wd,
                                                     vp(ring), vp(ctr), 3, vp(sums), stream()),
                   "finalize_ring")
        torch.cuda.synchronize()
        rg, sm = down(ring), down(sums)
        assert same_bits(rg[8:10], o[0:2]) and same_bits(sm[:2], o[2:4]), (what, rg, sm)
        assert untouched(rg[:8]) and untouched(rg[10:]) and untouched(sm[2:]), (what, rg, sm)


def spg_of(n_blocks):
    spg = 16
    while spg * spg < n_blocks:
        spg += 16
    return spg


def ordered_sum32(parts):
    """float32 sum over axis 0, in order, from 0.0f"""
    s = np.zeros(parts.shape[1:], np.float32)
    for p in parts:
        s = s + p
    return s


@pytest.mark.parametrize("K,N,ldp,ldc", [(16, 7, 48, 8), (5, 41, 48, 44), (1, 3, 48, 4)])
@pytest.mark.parametrize("n_blocks", [1, 2, 16, 17, 256, 257, 300])
def test_tn_reduce_blocks(pgcn, n_blocks, K, N, ldp, ldc):
    rng = np.random.default_rng([n_blocks, K, N])
    part = filled(n_blocks, K, ldp)                   # columns [N, ldp) NaN: never in a result
    part[:, :, :N] = rng.standard_normal((n_blocks, K, N)).astype(np.float32)
    p = part[:, :, :N]
    ref64 = p.astype(np.float64).sum(axis=0)
    bound = 1e-5 * np.abs(p.astype(np.float64)).sum(axis=0)
    spg = spg_of(n_blocks)
    if n_blocks <= spg:
        two = ordered_sum32(p)
    else:
        two = ordered_sum32(np.stack([ordered_sum32(p[g:g + spg])
                                      for g in range(0, n_blocks, spg)]))
    one = ordered_sum32(p)
    ws = pgcn.lib.pgcn_debug_tn_reduce_blocks_workspace(n_blocks, K, ldp)
    assert ws >= part.nbytes and ws % 4 == 0
    for name, want in (("blocks", two), ("one_pass", one)):
        dpart = up(np.concatenate([part.ravel(), filled(ws // 4 - part.size + GUARD)]))
        dC = out_buf(K * ldc)
        fn = pgcn.lib.pgcn_debug_tn_reduce_blocks if name == "blocks" else \
            pgcn.lib.pgcn_debug_tn_reduce_one_pass
        pgcn.check(fn(vp(dpart), n_blocks, K, N, ldp, vp(dC), ldc, stream()), name)
        torch.cuda.synchronize()
        C, pa = down(dC), down(dpart)
        what = (name, n_blocks, K, N)
        assert untouched(C[K * ldc:]), what
        C = C[:K * ldc].reshape(K, ldc)
        assert (u32(C[:, N:]) == 0).all(), what
        assert same_bits(C[:, :N], want), (what, C[:, :N], want)
        assert (np.abs(C[:, :N] - ref64) <= bound).all(), what
        assert same_bits(pa[:part.size], part.ravel()), what      # the partials are inputs
        assert untouched(pa[ws // 4:]), what                      # nothing past the workspace
        if name == "one_pass":
            assert untouched(pa[part.size:]), what                # no workspace used
