"""The Hadamard-MLP decoder's kernels through the kernel ABI -- pgcn_link_mlp_fwd / _bwd on a
pgcn_links handle -- against the float64 formulas of tests/link_mlp_ref.py.

Bounds, from the arithmetic alone (nothing is measured; u = 2^-24):
  forward, per pair.  pre_u carries one rounding of z_i, one of each product, at most d adds of the
  k-ordered chain and the add of b1: |d pre_u| <= (d + 3) u (|b1_u| + sum_i |z_i W1_iu|).  ReLU is
  1-Lipschitz (a sign flip near zero stays inside), so the hidden layer's error enters the score
  times |w2_u|.  The outer sum has one product per unit, at most h - 1 rounding adds that join
  non-empty sets of terms (the padded units add exact zeros) and the add of b2:
      |err_e| <= (h + 2) u sum_u |w2_u hid_u| + (d + 3) u sum_u |w2_u| (|b1_u| + sum_i |z_i W1_iu|)
                 + u |b2|.
  backward.  H, W1 and b1 are multiples of 1/8 in [-2, 2]: every z_i W1_iu is a multiple of 2^-9
  below 8 and a pre below 2^11, so pre is exact in fp32 (asserted here on the CPU) and the ReLU
  mask is the reference's.  A term of dW1 / db1 / dw2 / db2 then carries at most three roundings
  of its factors and product and at most E rounding adds over the pairs (lane, wave, workgroup
  and reduce stages each join non-empty sets): (E + h + 3) u sum |terms| covers them.  A term of
  dH carries dz's chain over the h units (h + 1 roundings), its product with H and at most m_i
  adds over node i's m_i entries: (m_i + h + 3) u sum |terms|.
"""
import ctypes

import numpy as np
import pytest

import link_mlp_ref as mr

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
SENTINEL = 7.25
SHAPES = ((1, 1), (3, 5), (4, 32), (17, 33), (64, 64), (128, 128))
NODES = 50
COUNTS = {"1": lambda t: 1, "tile-1": lambda t: t - 1, "tile": lambda t: t, "tile+1": lambda t: t + 1,
          "5tile+3": lambda t: 5 * t + 3}
PGCN_E_INVALID = -1


def _up4(d):
    return (d + 3) // 4 * 4


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def tile(pgcn):
    t = ctypes.c_int()
    pgcn.lib.pgcn_link_mlp_tile(ctypes.byref(t))
    return t.value


@pytest.fixture(scope="module")
def lists(pgcn, tile):
    """name -> (n, src, dst, select, Links): prefixes of one random list on 50 nodes that opens with
    a self pair and a pair listed twice; `tiny`, 1,000 random pairs; `hub`, node 0 with 3 T + 5
    incidence entries (alternately src and dst), every seventh pair unselected, a last node without
    pairs."""
    rng = np.random.default_rng(5)
    E = 5 * tile + 3
    src, dst = (rng.integers(0, NODES, E).astype(np.int32) for _ in range(2))
    src[:3], dst[:3] = (3, 7, 7), (3, 9, 9)
    out = {}
    for cnt in (f(tile) for f in COUNTS.values()):
        out[cnt] = (NODES, src[:cnt], dst[:cnt], None)
    out["tiny"] = (NODES, rng.integers(0, NODES, 1000).astype(np.int32),
                   rng.integers(0, NODES, 1000).astype(np.int32), None)
    T = int(pgcn.lib.pgcn_link_segment_slots())
    hs, hd, sel = [], [], []
    while len(sel) - sel.count(-1) < 3 * T + 5:
        k = len(hs)
        other = 1 + k % 40
        hs.append(0 if k % 2 == 0 else other)
        hd.append(other if k % 2 == 0 else 0)
        sel.append(-1 if k % 7 == 6 else 0)
    out["hub"] = (42, np.array(hs, np.int32), np.array(hd, np.int32), np.array(sel, np.int32))
    out = {k: v + (pgcn.Links(v[0], v[1], v[2], v[3]),) for k, v in out.items()}
    ptr, _, _ = pgcn.links_incidence(*out["hub"][:4])
    assert ptr[1] - ptr[0] == 3 * T + 5 and ptr[-1] == ptr[-2]
    yield out
    for v in out.values():
        v[4].close()


def _padded(x, ld, fill=np.nan):
    out = np.full((x.shape[0], ld), fill, np.float32)
    out[:, :x.shape[1]] = x
    return out


def run_fwd(links, H, d, P, h, E, ld_s=8):
    out = _dev(np.full((E + 1, ld_s), SENTINEL, np.float32))
    links.mlp_fwd(_dev(H), H.shape[1], d, _dev(P), P.shape[1], h, out, ld_s)
    _sync()
    return out.cpu().numpy()


def run_bwd(links, H, d, P, h, G, n):
    import torch
    ld, ld_dp = H.shape[1], _up4(h) + 4
    dH = _dev(np.full((n, ld), SENTINEL, np.float32))
    dP = _dev(np.full((d + 3, ld_dp), SENTINEL, np.float32))
    nbytes = links.mlp_workspace(d, h)
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
    links.mlp_bwd(_dev(H), ld, d, _dev(P), P.shape[1], h, _dev(G), G.shape[1], dH, ld, dP, ld_dp,
                  ws, nbytes)
    _sync()
    return dH.cpu().numpy(), dP.cpu().numpy()


@pytest.mark.parametrize("d,h", SHAPES)
@pytest.mark.parametrize("count", COUNTS)
def test_forward(lists, tile, count, d, h):
    n, src, dst, _, links = lists[COUNTS[count](tile)]
    rng = np.random.default_rng(100 * d + h)
    H = _padded(rng.standard_normal((n, d)).astype(np.float32), _up4(d) + 4)
    P = mr.pack(rng.standard_normal((d, h)), rng.standard_normal(h), rng.standard_normal(h),
                rng.standard_normal(), _up4(h) + 4, fill=np.nan)
    out = run_fwd(links, H, d, P, h, len(src))
    ref, A, B, _ = mr.forward(src, dst, H, P, d, h)
    bound = (h + 2) * EPS * A + (d + 3) * EPS * B + EPS * abs(float(P[d + 2, 0]))
    err = np.abs(out[:-1, 0].astype(np.float64) - ref)
    assert (err <= bound).all(), float((err - bound).max())
    assert (out[:-1, 1:4] == 0).all() and (out[:-1, 4:] == SENTINEL).all()
    assert (out[-1] == SENTINEL).all()


def _exact_inputs(n, d, h, E, sel, seed):
    """H, P, G of the backward tests: H, W1, b1 multiples of 1/8 in [-2, 2]; w2, b2, G normal, G
    zero on the unselected pairs."""
    rng = np.random.default_rng(seed)
    eighths = lambda *shape: (rng.integers(-16, 17, shape) / 8.0).astype(np.float32)
    H = _padded(eighths(n, d), _up4(d) + 4)
    P = mr.pack(eighths(d, h), eighths(h), rng.standard_normal(h), rng.standard_normal(),
                _up4(h) + 4, fill=np.nan)
    G = _padded(rng.standard_normal((E, 1)).astype(np.float32), 4)
    if sel is not None:
        G[sel < 0, 0] = 0.0
    return H, P, G


@pytest.mark.parametrize("d,h", SHAPES)
@pytest.mark.parametrize("name", ["tiny", "hub"])
def test_backward(lists, name, d, h):
    n, src, dst, sel, links = lists[name]
    E = len(src)
    H, P, G = _exact_inputs(n, d, h, E, sel, 1000 * d + h)
    pre64 = mr.forward(src, dst, H, P, d, h)[3]
    pre32 = (H[src, :d] * H[dst, :d]) @ P[:d, :h] + P[d, :h]
    assert pre32.dtype == np.float32 and (pre32.astype(np.float64) == pre64).all()
    dH, dP = run_bwd(links, H, d, P, h, G, n)
    rH, rP, mH, mP, m = mr.backward(src, dst, H, P, G[:, 0], d, h, sel)
    errP = np.abs(dP[:, :h].astype(np.float64) - rP)
    assert (errP <= (E + h + 3) * EPS * mP).all(), float((errP - (E + h + 3) * EPS * mP).max())
    errH = np.abs(dH[:, :d].astype(np.float64) - rH)
    boundH = (m[:, None] + h + 3) * EPS * mH
    assert (errH <= boundH).all(), float((errH - boundH).max())
    assert (dH[m == 0, :d] == 0).all() and ((m == 0).any() or name == "tiny")
    assert (dH[:, d:_up4(d)] == 0).all() and (dH[:, _up4(d):] == SENTINEL).all()
    assert (dP[:, h:] == 0).all() and (dP[d + 2, 1:] == 0).all()


def test_two_calls_same_bits(lists):
    n, src, dst, sel, links = lists["hub"]
    d, h = 17, 33
    H, P, G = _exact_inputs(n, d, h, len(src), sel, 9)
    assert run_fwd(links, H, d, P, h, len(src)).tobytes() == \
        run_fwd(links, H, d, P, h, len(src)).tobytes()
    a, b = run_bwd(links, H, d, P, h, G, n), run_bwd(links, H, d, P, h, G, n)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_invalid_arguments_launch_nothing(pgcn, lists):
    n, src, dst, _, links = lists["tiny"]
    E, d, h = len(src), 8, 8
    H, P, G = (_dev(np.zeros(s, np.float32)) for s in ((n, 132), (132, 132), (E, 4)))
    sc, dH, dP = (_dev(np.full(s, SENTINEL, np.float32)) for s in ((E, 4), (n, 132), (132, 132)))
    nbytes = max(links.mlp_workspace(8, 8), links.mlp_workspace(128, 128))
    ws = _dev(np.zeros(nbytes // 4, np.float32))
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lib, hd = pgcn.lib, links.handle

    def fwd(ld_h=8, d=d, ld_p=8, h=h, ld_s=4):
        return lib.pgcn_link_mlp_fwd(hd, p(H), ld_h, d, p(P), ld_p, h, p(sc), ld_s, None)

    def bwd(ld_h=8, d=d, ld_p=8, h=h, ld_g=4, ld_dh=8, ld_dp=8, nb=nbytes):
        return lib.pgcn_link_mlp_bwd(hd, p(H), ld_h, d, p(P), ld_p, h, p(G), ld_g, p(dH), ld_dh,
                                     p(dP), ld_dp, p(ws), nb, None)

    pgcn.reset_path_counts()
    bad = [fwd(d=0), fwd(d=129, ld_h=132), fwd(h=0), fwd(h=129, ld_p=132), fwd(ld_h=6),
           fwd(ld_p=10), fwd(ld_s=6), fwd(ld_h=4),
           bwd(d=0), bwd(d=129, ld_h=132, ld_dh=132), bwd(h=0), bwd(h=129, ld_p=132, ld_dp=132),
           bwd(ld_h=6), bwd(ld_p=10), bwd(ld_g=6), bwd(ld_dh=6), bwd(ld_dp=10), bwd(ld_dp=4),
           bwd(nb=links.mlp_workspace(8, 8) - 4)]
    _sync()
    assert bad == [PGCN_E_INVALID] * len(bad)
    c = pgcn.path_counts()
    assert c["launches"] == 0 and c["link_mlp_fwd"] == 0 and c["link_mlp_bwd"] == 0
    assert all((t.cpu().numpy() == SENTINEL).all() for t in (sc, dH, dP))
    assert fwd() == 0 and bwd() == 0
    _sync()
    c = pgcn.path_counts()
    assert c["link_mlp_fwd"] == 1 and c["link_mlp_bwd"] == 1 and c["launches"] == 4
