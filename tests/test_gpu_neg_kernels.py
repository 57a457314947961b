"""k_neg.hip through the kernel ABI: the negative draw (pgcn_neg_sample) against the numpy
transcription in tests/neg_ref.py, and the device incidence build (pgcn_links_create_dynamic,
_set_dst_range, _rebuild) against the host index of pgcn_debug_links_incidence.  Everything is
integer work, or float bits against the host-built handle: every comparison is exact."""
import ctypes

import numpy as np
import pytest

import neg_ref

pytestmark = pytest.mark.gpu

PGCN_E_INVALID = -1
SEED = 0x123456789ABCDEF


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def excl_rows(n, kind):
    """(ptr, idx): per node its own id only, all nodes but one, or a random set with itself."""
    rng = np.random.default_rng(n)
    rows = []
    for s in range(n):
        if kind == "self":
            row = [s]
        elif kind == "one_free":  # [0 .. n - 2]; the last node, which that row lacks: [1 .. n - 1]
            row = range(n - 1) if s < n - 1 else range(1, n)
        else:
            row = set(rng.choice(n, rng.integers(0, n - 1), replace=False).tolist()) - {s}
            row = sorted(row | {s})
        rows.append(np.array(row, np.int32))
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return ptr, np.concatenate(rows)


@pytest.mark.parametrize("m", [1, 255, 256, 257])
@pytest.mark.parametrize("kind", ["self", "one_free", "random"])
@pytest.mark.parametrize("n", [2, 65, 1000])
def test_draw(pgcn, n, kind, m):
    ptr, idx = excl_rows(n, kind)
    sampler = pgcn.NegSampler(n, ptr, idx)
    src = np.random.default_rng(m).integers(0, n, m).astype(np.int32)
    got = []
    for seed, rnd in ((SEED, 0), (SEED, 1), (7, 0)):
        out = _dev(np.full(m + 1, -5, np.int32))
        sampler.sample(_dev(src), m, seed, rnd, out)
        out = out.cpu().numpy()
        assert out[m] == -5
        assert (out[:m] == neg_ref.draw(src, n, ptr, idx, seed, rnd)).all()
        for e in range(m):
            assert out[e] not in idx[ptr[src[e]]:ptr[src[e] + 1]]
        got.append(out[:m])
    # another seed or round must change the draws -- asserted only where chance cannot make them
    # agree: 999 free nodes per anchor and at least 255 draws
    if kind == "self" and n == 1000 and m >= 255:
        assert (got[0] != got[1]).any() and (got[0] != got[2]).any()
    sampler.close()


def test_full_row_is_refused(pgcn):
    for n, ptr, idx in ((1, [0, 1], [0]), (3, [0, 1, 4, 5], [0, 0, 1, 2, 2])):
        with pytest.raises(pgcn.PgcnError) as e:
            pgcn.NegSampler(n, ptr, idx)
        assert e.value.status == PGCN_E_INVALID


def same_index(pgcn, links, n, src, dst, sel):
    want = links.incidence()
    for a, b in zip(want, pgcn.links_incidence(n, src, dst, sel)):
        assert a.tobytes() == b.tobytes()
    return want


@pytest.fixture(scope="module")
def tile(pgcn):
    return pgcn.links_sort_tile()


# pair counts as (tiles, offset), in entries-per-tile units: two entries a pair, so the half tiles
# put the ENTRY count on a tile edge and the whole ones the pair count
@pytest.mark.parametrize("pairs", [(0, 1), (1, -1), (1, 0), (1, 1), (5, 3), (0.5, 0), (0.5, 1)])
@pytest.mark.parametrize("n", [1, 256, 257, 65537])
def test_rebuild(pgcn, tile, n, pairs):
    E = int(pairs[0] * tile) + pairs[1]
    rng = np.random.default_rng(E + n)
    src, dst = (rng.integers(0, n, E).astype(np.int32) for _ in range(2))
    dst[1::11] = src[1::11]                      # self pairs
    src[2::13], dst[2::13] = src[0], dst[0]      # duplicates of pair 0
    sel = np.where(np.arange(E) % 5 == 3, -1, 0).astype(np.int32) if E > 1 else None
    links = pgcn.Links(n, src, dst, sel, dynamic=True)
    assert links.slots() == 2 * (E if sel is None else int((sel >= 0).sum()))
    same_index(pgcn, links, n, src, dst, sel)
    first, count = E // 3, E - E // 3 - E // 4
    dst[first:first + count] = rng.integers(0, n, count)
    links.set_dst_range(first, _dev(dst[first:first + count]), count)
    links.rebuild()
    one = same_index(pgcn, links, n, src, dst, sel)
    links.rebuild()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, links.incidence()))
    links.close()


def run_bwd(pgcn, links, H, d, G, n):
    out = _dev(np.full((n, d), 7.25, np.float32))
    pgcn.check(pgcn.lib.pgcn_link_score_bwd(links.handle, _p(H), d, d, _p(G), 4, _p(out), d, None))
    return out.cpu().numpy()


def run_mlp_bwd(links, H, d, P, h, G, n):
    """dH and dP of pgcn_link_mlp_bwd, as bytes."""
    nbytes = links.mlp_workspace(d, h)
    ws = _dev(np.zeros(nbytes // 4, np.float32))
    dH, dP = _dev(np.full((n, d), 7.25, np.float32)), _dev(np.full((d + 3, h), 7.25, np.float32))
    links.mlp_bwd(H, d, d, P, h, h, G, 4, dH, d, dP, h, ws, nbytes)
    return dH.cpu().numpy().tobytes() + dP.cpu().numpy().tobytes()


@pytest.mark.parametrize("hub", [0, 5])
@pytest.mark.parametrize("length", [(1, -1), (1, 0), (1, 1), (3, 5)])  # (segments, offset)
def test_hub_segments(pgcn, tile, length, hub):
    """A node at the segment edges, as node 0 (whose records the padding reuses) and elsewhere:
    the index, and the backward's bits against a host-built handle, which read the segment
    records; then most of the hub's pairs move to a second node and the rebuild must follow."""
    T = int(pgcn.lib.pgcn_link_segment_slots())
    n, want = 900, length[0] * T + length[1]
    rng = np.random.default_rng(want + hub)
    leaf = 10 + np.arange(want, dtype=np.int32) % (n - 10)
    src = np.where(np.arange(want) % 2 == 0, hub, leaf).astype(np.int32)
    dst = np.where(np.arange(want) % 2 == 0, leaf, hub).astype(np.int32)
    src = np.concatenate([src, rng.integers(6, n, 300).astype(np.int32)])
    dst = np.concatenate([dst, rng.integers(6, n, 300).astype(np.int32)])
    E = len(src)
    links = pgcn.Links(n, src, dst, dynamic=True)
    G = _dev(rng.standard_normal((E, 4)).astype(np.float32))
    for step in range(2):
        ptr = same_index(pgcn, links, n, src, dst, None)[0]
        assert ptr[hub + 1] - ptr[hub] == (want if step == 0 else (want + 1) // 2)
        fixed = pgcn.Links(n, src, dst)
        for d in (16, 64):
            H = _dev(rng.standard_normal((n, d)).astype(np.float32))
            assert run_bwd(pgcn, links, H, d, G, n).tobytes() == \
                run_bwd(pgcn, fixed, H, d, G, n).tobytes()
        P = _dev(rng.standard_normal((d + 3, 8)).astype(np.float32))  # the MLP decoder, h = 8
        assert run_mlp_bwd(links, H, d, P, 8, G, n) == run_mlp_bwd(fixed, H, d, P, 8, G, n)
        fixed.close()
        dst[1:want:2] = 7  # the pairs that ended at the hub now end at node 7
        links.set_dst_range(0, _dev(dst[:want]), want)
        links.rebuild()
    links.close()


def test_invalid_arguments_launch_nothing(pgcn, tile):
    src, dst = np.array([0, 1, 2], np.int32), np.array([1, 2, 0], np.int32)
    fixed, dyn = pgcn.Links(3, src, dst), pgcn.Links(3, src, dst, dynamic=True)
    new, lib = _dev(dst), pgcn.lib
    pgcn.reset_path_counts()
    bad = [
        lib.pgcn_links_rebuild(fixed.handle, None),
        lib.pgcn_links_set_dst_range(fixed.handle, 0, 3, _p(new), None),
        lib.pgcn_links_rebuild(None, None),
        lib.pgcn_links_set_dst_range(dyn.handle, 1, 3, _p(new), None),
        lib.pgcn_links_set_dst_range(dyn.handle, -1, 1, _p(new), None),
        lib.pgcn_links_set_dst_range(dyn.handle, 0, 1, None, None),
        lib.pgcn_neg_sample(None, _p(new), 3, 1, 0, _p(new), None),
    ]
    assert bad == [PGCN_E_INVALID] * len(bad) and pgcn.path_counts()["launches"] == 0
    same_index(pgcn, dyn, 3, src, dst, None)
    same_index(pgcn, fixed, 3, src, dst, None)
    with pytest.raises(pgcn.PgcnError):
        pgcn.Links(3, np.array([0, 3], np.int32), np.array([1, 2], np.int32), dynamic=True)
    fixed.close()
    dyn.close()
