"""The dropout mask draw (csrc/mask_draw.hpp, k_dropout_mask) and k_dropout_apply as the engine
launches them, through pgcn_debug_dropout_mask / _mask2 / _apply: one state per 128 draws
(per = 2), element windows [elem0, elem_end), a capped grid, two segments in one launch, and
keep bits read from base + i.  (test_dropout_masks_bit_exact in test_gpu_kernels.py runs per = 1,
one segment, elem0 = 0, p = 0.5 on 100 k elements.)

Reference: the sequential stream of the C oracle (or_rng_seed / or_rng_next), element e of a
segment keeping its value when draw (offset + e - elem0) >= int(float32(p) * float32(0x7fffffff)).
Chunk states come from pgcn.rng_jump on the host: state k of a segment sits at draw
offset + 64 per k.  Every launch is checked three ways: the mask words equal the reference bits
up to elem_end and are zero from there on (the words are pre-filled with a pattern), a sentinel
word after n_chunks and a sentinel state after the last state are untouched, and the stored
states equal the old ones jumped by the period on the host -- so a second launch gives the next
epoch's bits, which is checked too.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers

pytestmark = pytest.mark.gpu

DEV = "cuda"
OFFSET = 1000     # stream position of a segment's first element
PERIOD = 17001    # draws per epoch (odd: the next epoch's chunks start inside a word)
ELEM0 = 64 * 5    # a window that does not start at element 0
MAX_DRAWS = OFFSET + PERIOD + 64 * 600
FILL = np.uint64(0xA5A5A5A5A5A5A5A5)
SENTINEL = np.uint64(0x0123456789ABCDEF)


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev64(a):
    return torch.from_numpy(np.array(a, np.uint64).view(np.int64)).to(DEV)


def host64(t):
    return t.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def draws():
    """the first MAX_DRAWS draws of the sequential stream"""
    lib = helpers.oracle()
    s = np.zeros(2, np.uint64)
    sp = helpers.ptr(s)
    lib.or_rng_seed(sp)
    out = np.array([lib.or_rng_next(sp) for _ in range(MAX_DRAWS)], np.int64)
    out.setflags(write=False)
    return out


def threshold(p):
    return int(np.float32(p) * np.float32(0x7FFFFFFF))


def reference_words(offset, n_chunks, n_valid, p):
    """n_chunks mask words: bit j of word c keeps element 64 c + j < n_valid, zero beyond"""
    bits = np.zeros(64 * n_chunks, np.uint8)
    k = min(max(n_valid, 0), 64 * n_chunks)
    assert offset + k <= MAX_DRAWS
    bits[:k] = draws()[offset:offset + k] >= threshold(p)
    return np.packbits(bits, bitorder="little").view(np.uint64)


@functools.lru_cache(maxsize=None)
def jump_table():
    return dev64(helpers.pgcn().rng_jump_table(PERIOD))


class Seg:
    """One variable's draw: its chunk states on the device (a sentinel state after them), its
    mask words (pre-filled, a sentinel word after them), and the host's copy of the states"""

    def __init__(self, per, n_chunks, n_valid, p, offset=OFFSET, elem0=ELEM0):
        pg = helpers.pgcn()
        self.per, self.n_chunks, self.n_valid, self.p = per, n_chunks, n_valid, p
        self.offset, self.elem0, self.epoch = offset, elem0, 0
        n_states = (n_chunks + per - 1) // per
        st = pg.rng_jump(pg.rng_seed(), offset)
        states = []
        for _ in range(n_states):
            states.append(st)
            st = pg.rng_jump(st, 64 * per)
        self.host_states = np.array(states, np.uint64).reshape(n_states, 2)
        self.states = dev64(np.concatenate([self.host_states,
                                            np.full((1, 2), SENTINEL)]).reshape(-1))
        self.mask = None
        self.refill()

    def refill(self):
        self.mask = dev64(np.concatenate([np.full(self.n_chunks, FILL), [SENTINEL]]))

    def args(self):
        """(states, n_chunks, elem0, elem_end, p, mask): null pointers when there is no chunk"""
        if self.n_chunks == 0:
            return (None, 0, self.elem0, self.elem0 + self.n_valid, self.p, None)
        return (vp(self.states), self.n_chunks, self.elem0, self.elem0 + self.n_valid, self.p,
                vp(self.mask))

    def check(self, what=""):
        """after a launch (synchronised): this epoch's words, the sentinels, the advanced states"""
        pg = helpers.pgcn()
        words = host64(self.mask)
        assert words[-1] == SENTINEL, (what, "word past n_chunks written")
        want = reference_words(self.offset + self.epoch * PERIOD, self.n_chunks, self.n_valid,
                               self.p)
        np.testing.assert_array_equal(words[:-1], want, err_msg=f"{what} epoch {self.epoch}")
        st = host64(self.states).reshape(-1, 2)
        assert (st[-1] == SENTINEL).all(), (what, "state past the last one written")
        self.host_states = np.array([pg.rng_jump(s, PERIOD) for s in self.host_states],
                                    np.uint64).reshape(-1, 2)
        np.testing.assert_array_equal(st[:-1], self.host_states, err_msg=f"{what} states")
        self.epoch += 1
        return words[:-1].copy(), st[:-1].copy()

    def untouched(self):
        words, st = host64(self.mask), host64(self.states).reshape(-1, 2)
        assert (words[:-1] == FILL).all() and words[-1] == SENTINEL
        np.testing.assert_array_equal(st[:-1], self.host_states)


def launch(pgcn, seg, max_blocks=0):
    pgcn.reset_path_counts()
    st = pgcn.lib.pgcn_debug_dropout_mask(*seg.args(), vp(jump_table()), seg.per, max_blocks,
                                          stream())
    torch.cuda.synchronize()
    assert st == pgcn.PGCN_OK
    return pgcn.path_counts()["launches"]


def launch2(pgcn, a, b):
    pgcn.reset_path_counts()
    st = pgcn.lib.pgcn_debug_dropout_mask2(*a.args(), a.per, *b.args(), b.per, vp(jump_table()),
                                           stream())
    torch.cuda.synchronize()
    assert st == pgcn.PGCN_OK
    return pgcn.path_counts()["launches"]


def two_epochs(pgcn, seg, what, max_blocks=0):
    out = []
    for _ in range(2):
        seg.refill()
        assert launch(pgcn, seg, max_blocks) == 1, what
        out.append(seg.check(what))
    return out


# ------------------------------------------------------------------------------ one segment
@pytest.mark.parametrize("n_chunks", (1, 2, 3, 64, 257))
@pytest.mark.parametrize("per", (1, 2))
def test_draw_chunk_counts(pgcn, per, n_chunks):
    """Odd chunk counts under per = 2: the last state emits one word only.  The window ends
    inside the last chunk; two epochs."""
    seg = Seg(per, n_chunks, 64 * n_chunks - 13, 0.5)
    assert len(seg.host_states) == (n_chunks + per - 1) // per
    (w1, _), (w2, _) = two_epochs(pgcn, seg, (per, n_chunks))
    assert int(w1[-1]) >> 51 == 0 and (n_chunks < 2 or (w1 != w2).any())


@pytest.mark.parametrize("n_chunks", (3, 64))
@pytest.mark.parametrize("per", (1, 2))
def test_draw_window_ends(pgcn, per, n_chunks):
    """elem_end at the end of the last chunk, at its first element (the word is zero), before
    it (the word before is trimmed too), before the last state's first element, one element
    long, and empty"""
    full = 64 * n_chunks
    for n_valid in (full, full - 64, full - 64 - 5, full - 128 - 5, 1, 0):
        seg = Seg(per, n_chunks, n_valid, 0.5)
        (w1, _), _ = two_epochs(pgcn, seg, (per, n_chunks, n_valid))
        if n_valid <= full - 64:
            assert w1[-1] == 0
        if n_valid == 0:
            assert (w1 == 0).all()
        if n_valid == full:  # (the reference is not all zeros by accident)
            assert 0.4 < np.unpackbits(w1.view(np.uint8)).mean() < 0.6


@pytest.mark.parametrize("p", (0.0, 0.1, 0.5, 0.9))
def test_draw_thresholds(pgcn, p):
    for per in (1, 2):
        seg = Seg(per, 63, 64 * 63 - 13, p)
        (w1, _), _ = two_epochs(pgcn, seg, (per, p))
        kept = np.unpackbits(w1.view(np.uint8), bitorder="little")[:seg.n_valid].mean()
        assert abs(kept - (1 - p)) < 0.03, (p, kept)
        if p == 0.0:
            assert kept == 1.0


@pytest.mark.parametrize("n_chunks", (257, 600))
@pytest.mark.parametrize("per", (1, 2))
def test_draw_small_grid(pgcn, per, n_chunks):
    """max_blocks = 1: 256 threads take the states in pairs (t, t + 256), 257 states leave
    one unpaired, 600 give a second trip without a partner; the same words and states as the
    default grid"""
    outs = []
    for max_blocks in (0, 1):
        seg = Seg(per, n_chunks, 64 * n_chunks - 13, 0.5)
        outs.append(two_epochs(pgcn, seg, (per, n_chunks, max_blocks), max_blocks))
    for (wa, sa), (wb, sb) in zip(*outs):
        np.testing.assert_array_equal(wa, wb)
        np.testing.assert_array_equal(sa, sb)


# ------------------------------------------------------------------------------ two segments
def _pair():
    a = Seg(2, 65, 64 * 65 - 13, 0.5)
    b = Seg(1, 3, 150, 0.1, offset=9000, elem0=64 * 11)
    return a, b


def test_draw_two_segments(pgcn):
    """Two variables in one launch, their per, p, sizes and windows different; either order"""
    for swap in (False, True):
        a, b = _pair()
        for _ in range(2):
            a.refill()
            b.refill()
            assert launch2(pgcn, *((b, a) if swap else (a, b))) == 1
            wa, _ = a.check(("pair a", swap))
            wb, _ = b.check(("pair b", swap))
        # ... and each alone gives the same words
        a1, b1 = _pair()
        launch(pgcn, a1)
        launch(pgcn, b1)
        a1.check()
        b1.check()
        launch(pgcn, a1)
        launch(pgcn, b1)
        np.testing.assert_array_equal(a1.check()[0], wa)
        np.testing.assert_array_equal(b1.check()[0], wb)


def test_draw_two_segments_one_empty(pgcn):
    """Each segment empty in turn (no chunks, null pointers): the other is drawn as alone"""
    for first_empty in (False, True):
        for which in (0, 1):
            seg = _pair()[which]
            none = Seg(2 - which, 0, 0, 0.5)
            for _ in range(2):
                seg.refill()
                assert launch2(pgcn, *((none, seg) if first_empty else (seg, none))) == 1
                seg.check((which, first_empty))
    none = Seg(1, 0, 0, 0.5)
    assert launch2(pgcn, none, Seg(2, 0, 0, 0.1)) == 0
    assert launch(pgcn, none) == 0


def test_draw_refuses_other_per(pgcn):
    seg = Seg(1, 3, 100, 0.5)
    for per in (0, 3):
        st = pgcn.lib.pgcn_debug_dropout_mask(*seg.args(), vp(jump_table()), per, 0, stream())
        torch.cuda.synchronize()
        assert st == pgcn.PGCN_E_INVALID
        seg.untouched()


# ------------------------------------------------------------------------------ the apply
def test_dropout_apply_based(pgcn):
    """x[i] *= bit(base + i) ? scale : 0 with the four keep bits of a float4 read across a
    word's edge (base % 64 > 60) and the tail of n % 4 elements; the bitmap has exactly the words
    bits [0, base + n) need; nothing past n is written"""
    guard = 8
    for base in (0, 1, 61, 62, 63, 64 + 61):
        for n in (1000, 1001, 1002, 1003):
            rng = np.random.default_rng([base, n])
            x = rng.standard_normal(n + guard).astype(np.float32)
            x[n:] = np.nan
            words = rng.integers(0, 2**64, (base + n + 63) // 64, dtype=np.uint64)
            keep = helpers.mask_bits(words, base + n)[base:]
            want = x.copy()
            want[:n] = x[:n] * np.where(keep, np.float32(2.0), np.float32(0.0))
            dx, dw = torch.from_numpy(x.copy()).to(DEV), dev64(words)
            assert dx.data_ptr() % 16 == 0
            pgcn.reset_path_counts()
            st = pgcn.lib.pgcn_debug_dropout_apply(vp(dx), n, vp(dw), base, 2.0, stream())
            torch.cuda.synchronize()
            assert st == pgcn.PGCN_OK and pgcn.path_counts()["launches"] == 1
            np.testing.assert_array_equal(dx.cpu().numpy().view(np.int32), want.view(np.int32),
                                          err_msg=f"base {base} n {n}")
    # nothing to do: no launch, nothing read
    assert pgcn.lib.pgcn_debug_dropout_apply(None, 0, None, 5, 2.0, stream()) == pgcn.PGCN_OK
