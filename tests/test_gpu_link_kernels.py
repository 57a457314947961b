"""The pair-score kernels through the kernel ABI -- pgcn_link_score_fwd / _bwd on a pgcn_links
handle -- against the float64 formulas of tests/link_ref.py.  T = pgcn_link_segment_slots() is the
incidence length above which a node's list is cut into segments.

Pair lists:
  edges:  ten hub nodes whose incidence lists (over the selected pairs) have the lengths 0, 1, 2,
          63, 64, 65, T - 1, T, T + 1 and 3 T + 5, their partners cycling through 2,000 leaf nodes
          with the hub alternately src and dst; three self pairs on the T + 1 hub, one leaf pair
          listed three times, every seventh pair with select = -1, one node without any pair.
  tiny:   1,000 random pairs on 50 nodes (no list above T).
  one:    E = 1.

Bounds, from the arithmetic alone (nothing is measured; u = 2^-24):
  forward, per pair: d products and d - 1 adds in any order, gamma_d < (d + 1) u for d <= 128:
      |err| <= (d + 1) u sum_c |H_src[c] H_dst[c]|.
  backward, per element: m_i products and at most m_i - 1 rounding adds on any term's path (a
  rounding add joins two non-empty sets of terms):
      |err| <= (m_i + 1) u sum |G_e H_o[c]| over node i's m_i entries.
"""
import ctypes

import numpy as np
import pytest

import link_ref as lr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SENTINEL = 7.25
WIDTHS = (1, 3, 4, 16, 17, 64, 128)
HUBS, LEAVES = 10, 2000
PGCN_E_INVALID = -1


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


def hub_lengths(T):
    return [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5]


def edges_case(T):
    """(n, src, dst, select) of the `edges` list."""
    src, dst, sel = [], [], []

    def add(s, t):
        on = len(src) % 7 != 6
        src.append(s)
        dst.append(t)
        sel.append(0 if on else -1)
        return on

    leaf = 0
    for hub, want in enumerate(hub_lengths(T)):
        have = selfs = k = 0
        while want == T + 1 and selfs < 3:
            if add(hub, hub):
                have, selfs = have + 2, selfs + 1
        while have < want:
            other = HUBS + leaf % LEAVES
            leaf += 1
            have += add(hub, other) if k % 2 == 0 else add(other, hub)
            k += 1
    for _ in range(3):
        add(HUBS + 5, HUBS + 17)
    n = HUBS + LEAVES + 1  # the last node has no pair at all
    return n, np.array(src, np.int32), np.array(dst, np.int32), np.array(sel, np.int32)


def cases(T):
    rng = np.random.default_rng(11)
    return {
        "edges": edges_case(T),
        "tiny": (50, rng.integers(0, 50, 1000).astype(np.int32),
                 rng.integers(0, 50, 1000).astype(np.int32), None),
        "one": (3, np.array([0], np.int32), np.array([2], np.int32), None),
    }


@pytest.fixture(scope="module")
def T(pgcn):
    return int(pgcn.lib.pgcn_link_segment_slots())


@pytest.fixture(scope="module")
def lists(pgcn, T):
    """name -> (n, src, dst, select, Links handle), built once."""
    out = {}
    for name, (n, src, dst, sel) in cases(T).items():
        out[name] = (n, src, dst, sel, pgcn.Links(n, src, dst, sel))
    yield out
    for v in out.values():
        v[4].close()


def _input(n, d, ld, seed):
    """[n][ld]: N(0, 1) in the d columns, NaN in the padding."""
    rng = np.random.default_rng(seed)
    x = np.full((n, ld), np.nan, np.float32)
    x[:, :d] = rng.standard_normal((n, d)).astype(np.float32)
    return x


def check_padding(a, d, fill, sentinel):
    """Columns [d, round_up4(d)) hold `fill`, those behind them the untouched sentinel."""
    u = _up4(d)
    assert (a[:, d:u] == fill).all()
    assert (a[:, u:] == sentinel).all()


def run_fwd(pgcn, links, H, d, E, ld_s=12):
    dH, out = _dev(H), _dev(np.full((E, ld_s), SENTINEL, np.float32))
    pgcn.check(pgcn.lib.pgcn_link_score_fwd(links.handle, _p(dH), H.shape[1], d, _p(out), ld_s,
                                            None), "link_score_fwd")
    _sync()
    return out.cpu().numpy()


def run_bwd(pgcn, links, H, d, G, n):
    ld = H.shape[1]
    dH, dG = _dev(H), _dev(G)
    out = _dev(np.full((n, ld), SENTINEL, np.float32))
    pgcn.check(pgcn.lib.pgcn_link_score_bwd(links.handle, _p(dH), ld, d, _p(dG), G.shape[1],
                                            _p(out), ld, None), "link_score_bwd")
    _sync()
    return out.cpu().numpy()


def _grad(E, sel, seed, ld_g=8):
    """G [E][ld_g]: N(0, 1) in column 0, NaN behind it and on the pairs left out of the index."""
    rng = np.random.default_rng(seed)
    G = np.full((E, ld_g), np.nan, np.float32)
    G[:, 0] = rng.standard_normal(E).astype(np.float32)
    if sel is not None:
        G[sel < 0, 0] = np.nan
    return G


def test_edges_case_is_what_it_says(pgcn, T, lists):
    n, src, dst, sel, links = lists["edges"]
    ptr, pair, other = pgcn.links_incidence(n, src, dst, sel)
    assert list(np.diff(ptr)[:HUBS]) == hub_lengths(T)
    assert np.diff(ptr)[-1] == 0 and n >= 2000 and len(src) >= 3300
    assert ((src == dst) & (sel >= 0)).sum() == 3 and (sel < 0).sum() >= len(src) // 7
    assert ((src == HUBS + 5) & (dst == HUBS + 17)).sum() == 3
    assert links.slots() == 2 * int((sel >= 0).sum()) == ptr[-1]
    assert lists["tiny"][4].slots() == 2000 and lists["one"][4].slots() == 2


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", ["edges", "tiny", "one"])
def test_forward(pgcn, lists, name, d):
    n, src, dst, sel, links = lists[name]
    H = _input(n, d, _up4(d) + 8, 100 + d)
    out = run_fwd(pgcn, links, H, d, len(src))
    H64 = H[:, :d].astype(np.float64)
    ref = lr.score_forward(src, dst, H64)
    bound = (d + 1) * EPS * lr.score_forward(src, dst, np.abs(H64))
    err = np.abs(out[:, 0].astype(np.float64) - ref)
    assert (err <= bound).all(), float((err - bound).max())
    check_padding(out, 1, 0.0, SENTINEL)  # {s, 0, 0, 0}, nothing behind


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("name", ["edges", "tiny", "one"])
def test_backward(pgcn, lists, name, d):
    n, src, dst, sel, links = lists[name]
    H = _input(n, d, _up4(d) + 8, 200 + d)
    G = _grad(len(src), sel, 300 + d)
    got = run_bwd(pgcn, links, H, d, G, n)
    H64 = H[:, :d].astype(np.float64)
    ref = lr.score_backward(src, dst, H64, G[:, 0], sel)
    mag, m = lr.score_backward_magnitude(src, dst, H64, G[:, 0], sel)
    bound = (m[:, None] + 1) * EPS * mag
    err = np.abs(got[:, :d].astype(np.float64) - ref)
    assert np.isfinite(got[:, :d]).all()
    assert (err <= bound).all(), float((err - bound).max())
    assert (got[m == 0][:, :d] == 0).all() and ((m == 0).any() or name == "tiny")
    check_padding(got, d, 0.0, SENTINEL)


def test_two_calls_same_bits(pgcn, lists):
    n, src, dst, sel, links = lists["edges"]
    for d in (17, 64):
        H = _input(n, d, _up4(d), 1)
        G = _grad(len(src), sel, 2)
        assert run_fwd(pgcn, links, H, d, len(src)).tobytes() == \
            run_fwd(pgcn, links, H, d, len(src)).tobytes()
        assert run_bwd(pgcn, links, H, d, G, n).tobytes() == \
            run_bwd(pgcn, links, H, d, G, n).tobytes()


def test_launch_counts(pgcn, lists):
    d = 16
    for name, bwd_launches in (("tiny", 1), ("edges", 2)):
        n, src, dst, sel, links = lists[name]
        H = _input(n, d, d, 3)
        G = _grad(len(src), sel, 4)
        pgcn.reset_path_counts()
        run_fwd(pgcn, links, H, d, len(src))
        c = pgcn.path_counts()
        assert c["launches"] == 1 and c["link_fwd"] == 1 and c["link_bwd"] == 0
        pgcn.reset_path_counts()
        run_bwd(pgcn, links, H, d, G, n)
        c = pgcn.path_counts()
        assert c["launches"] == bwd_launches and c["link_bwd"] == 1 and c["link_fwd"] == 0


def test_no_pairs_launch_nothing(pgcn):
    links = pgcn.Links(5, np.zeros(0, np.int32), np.zeros(0, np.int32))
    H = _dev(_input(5, 4, 4, 5))
    out = _dev(np.full((5, 4), SENTINEL, np.float32))
    pgcn.reset_path_counts()
    pgcn.check(pgcn.lib.pgcn_link_score_fwd(links.handle, _p(H), 4, 4, _p(out), 4, None))
    pgcn.check(pgcn.lib.pgcn_link_score_bwd(links.handle, _p(H), 4, 4, _p(out), 4, _p(out), 4,
                                            None))
    _sync()
    assert pgcn.path_counts()["launches"] == 0 and (out.cpu().numpy() == SENTINEL).all()
    links.close()


def test_invalid_arguments_write_nothing(pgcn, lists):
    n, src, dst, sel, links = lists["tiny"]
    E, ld = len(src), 8
    H = _dev(_input(n, 8, ld, 6))
    G = _dev(_grad(E, sel, 7, 4))
    scores = _dev(np.full((E, 4), SENTINEL, np.float32))
    dH = _dev(np.full((n, ld), SENTINEL, np.float32))
    lib = pgcn.lib
    h = links.handle
    bad = [
        lib.pgcn_link_score_fwd(h, _p(H), ld, 0, _p(scores), 4, None),
        lib.pgcn_link_score_fwd(h, _p(H), 132, 129, _p(scores), 4, None),
        lib.pgcn_link_score_fwd(h, _p(H), 6, 5, _p(scores), 4, None),
        lib.pgcn_link_score_fwd(h, _p(H), ld, 8, _p(scores), 6, None),
        lib.pgcn_link_score_fwd(h, None, ld, 8, _p(scores), 4, None),
        lib.pgcn_link_score_fwd(None, _p(H), ld, 8, _p(scores), 4, None),
        lib.pgcn_link_score_bwd(h, _p(H), ld, 0, _p(G), 4, _p(dH), ld, None),
        lib.pgcn_link_score_bwd(h, _p(H), 132, 129, _p(G), 4, _p(dH), 132, None),
        lib.pgcn_link_score_bwd(h, _p(H), ld, 8, _p(G), 6, _p(dH), ld, None),
        lib.pgcn_link_score_bwd(h, _p(H), ld, 8, _p(G), 4, _p(dH), 6, None),
        lib.pgcn_link_score_bwd(h, None, ld, 8, _p(G), 4, _p(dH), ld, None),
        lib.pgcn_link_score_bwd(h, _p(H), ld, 8, None, 4, _p(dH), ld, None),
    ]
    _sync()
    assert bad == [PGCN_E_INVALID] * len(bad)
    assert (scores.cpu().numpy() == SENTINEL).all() and (dH.cpu().numpy() == SENTINEL).all()
    with pytest.raises(pgcn.PgcnError) as e:
        pgcn.Links(n, np.array([0, n], np.int32), np.array([1, 2], np.int32))
    assert e.value.status == PGCN_E_INVALID
    with pytest.raises(pgcn.PgcnError):
        pgcn.Links(n, np.array([0, 1], np.int32), np.array([1, -1], np.int32))
