"""GraphSum at kernel level where the random-graph tests do not reach: every width body, row
lengths on every schedule boundary, empty rows, rectangular (edge-cut rank) graphs, the blocked
layout at widths other than 16, unequal leading dimensions and stray writes.

Reference: scipy's float64 CSR product of the graph's values (helpers.csr_reference); bound: the
same product of absolute values; accepted: err <= 1e-5 * bound + 1e-30 per element (the
project's GraphSum rule, fp32 reordering only).  Every case also checks: padding columns
dim .. 4 vec exactly 0, three calls giving the same bits (arrival counters back at zero, partial
buffers reused), the kernel family taken (pgcn_debug_path_count), and 64 guard rows before and
after the output left alone.

The builders' own properties (boundaries present, slot counts against kSmallNnz, table sizes
against kL2Budget, the ring thresholds of the rank graphs) are host-only tests: not marked gpu.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest
import torch

import helpers

gpu = pytest.mark.gpu

DEV = "cuda"
TOL = 1e-5
GUARD = 64           # guard rows before and after the output
SENTINEL = 12345.5   # their value
CALLS = 3

# float4 per row with a kernel body of their own (graphsum_vec_supported, launch_graphsum)
VECS = tuple(range(1, 13)) + (16, 32)
# literal copy of graphsum_group_lanes (k_graphsum.hip): lanes per work item
GROUP_LANES = {1: 16, 2: 16, 3: 64, 4: 16, 5: 64, 6: 64, 7: 64, 8: 32, 9: 64, 10: 64, 11: 64,
               12: 64, 16: 64, 32: 64}
ITEM_ITERS = (2, 4, 8, 16, 32)   # "gs_item_iters"
K_SMALL_NNZ = 1 << 20            # DevGraph::kSmallNnz
L2_BUDGET = 4.0e6                # DevGraph::kL2Budget
LDS_MIN_ROWS = 32768             # DevGraph::kLdsMinRows
LDS_MIN_COLS = (1 << 20) // 64   # DevGraph::kLdsMinBytes / 64: the ring needs cols above it

LADDER_N = 6400
LADDER_DIMS = tuple(range(1, 49)) + (61, 64, 125, 128)


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# --------------------------------------------------------------------------- the ladder
def ladder_boundaries():
    """vec -> the row lengths at which DevGraph::schedule or a kernel loop changes form:
    chunk = NB * it (NB = G / vec neighbours per group iteration; also the 4x unrolled loop's
    stride at it = 4 and 8 * chunk of gs_split 2), and for power-of-two vec the workgroup
    items' wide_max = 256 / vec * 8 and their 4 * NS unrolling (NS = 256 / vec)."""
    out = {}
    for vec in VECS:
        nb = GROUP_LANES[vec] // vec
        b = [nb * it for it in ITEM_ITERS]
        if vec & (vec - 1) == 0:
            b += [256 // vec * 8, 4 * 256 // vec]
        out[vec] = b
    return out


def ladder_lengths():
    lens = set(range(261)) | {5000}
    for bs in ladder_boundaries().values():
        for b in bs:
            for k in (1, 2, 3):
                lens.update((k * b - 1, k * b, k * b + 1))
    return sorted(lens)


@functools.lru_cache(maxsize=None)
def ladder(tiles=1):
    """Square graph of LADDER_N nodes: row i has exactly L[i] random neighbours (duplicates
    allowed), the ladder `tiles` times over, every later row empty; random values in [-1, 1];
    a 128-wide input and its float64 reference, shared by every test and read-only."""
    lens = np.tile(np.array(ladder_lengths(), np.int64), tiles)
    assert len(lens) <= LADDER_N
    indptr = np.full(LADDER_N + 1, lens.sum(), np.int64)
    indptr[0] = 0
    indptr[1:len(lens) + 1] = np.cumsum(lens)
    indptr = indptr.astype(np.int32)
    rng = np.random.default_rng(1000 + tiles)
    nnz = int(indptr[-1])
    indices = rng.integers(0, LADDER_N, nnz).astype(np.int32)
    vals = rng.uniform(-1, 1, nnz).astype(np.float32)
    x = rng.standard_normal((LADDER_N, 128)).astype(np.float32)
    ref, bound = helpers.csr_reference(indptr, indices, vals, x)
    frozen(indptr, indices, vals, x, ref, bound)
    return dict(n=LADDER_N, indptr=indptr, indices=indices, vals=vals, x=x, ref=ref, bound=bound)


def test_ladder_has_every_boundary():
    """Host only: the ladder holds b - 1, b and b + 1 of every derived boundary (and of 2 b and
    3 b), has the sizes the schedule thresholds assume, and its 9-fold tiling is past
    kSmallNnz."""
    lens = ladder_lengths()
    have = set(lens)
    for vec, bs in ladder_boundaries().items():
        assert len(bs) == (7 if vec & (vec - 1) == 0 else 5)
        for b in bs:
            for k in (1, 2, 3):
                assert {k * b - 1, k * b, k * b + 1} <= have, (vec, b, k)
    assert set(range(261)) <= have and 5000 in have
    assert (len(lens), sum(lens), max(lens)) == (337, 133802, 6145)
    lad = ladder()
    assert np.array_equal(np.diff(lad["indptr"])[:len(lens)], lens)
    assert (np.diff(lad["indptr"])[len(lens):] == 0).all()
    assert lad["indptr"][-1] == 133802 <= K_SMALL_NNZ       # the small-graph schedules
    assert 9 * len(lens) <= LADDER_N and 9 * 133802 > K_SMALL_NNZ  # the tiled one: past them


# --------------------------------------------------------------------------- running a case
@contextlib.contextmanager
def values_graph(pgcn, gr):
    """pgcn_graph_create_values of a builder's dict (square; any values: the gather kernels)."""
    g = ctypes.c_void_p()
    pgcn.check(pgcn.lib.pgcn_graph_create_values(gr["n"], helpers.ptr(gr["indptr"]),
                                                 helpers.ptr(gr["indices"]), helpers.ptr(gr["vals"]),
                                                 ctypes.byref(g)), "graph_create_values")
    try:
        yield g
    finally:
        pgcn.lib.pgcn_graph_destroy(g)


def gs_calls(pgcn, g, x, n_rows, dim, wide_in=0, wide_out=0):
    """CALLS calls of pgcn_graphsum on x[:, :dim] (host, one row per graph column).  The input
    has ld 4 vec + wide_in, its columns past 4 vec NaN; every output is a view of n_rows rows in
    the middle of an allocation of ld 4 vec + wide_out, prefilled with NaN between GUARD rows of
    SENTINEL.  Returns the whole allocations (host) and the path counts of the calls."""
    ld = (dim + 3) // 4 * 4
    ld_in, ld_out = ld + wide_in, ld + wide_out
    hx = np.zeros((x.shape[0], ld_in), np.float32)
    hx[:, :dim] = x[:, :dim]
    hx[:, ld:] = np.nan
    xin = torch.from_numpy(hx).to(DEV)
    bigs = []
    pgcn.reset_path_counts()
    for _ in range(CALLS):
        big = torch.full((n_rows + 2 * GUARD, ld_out), SENTINEL, device=DEV)
        out = big[GUARD:GUARD + n_rows]
        out.fill_(float("nan"))
        pgcn.check(pgcn.lib.pgcn_graphsum(g, vp(xin), ld_in, vp(out), ld_out, dim, stream()),
                   "graphsum")
        bigs.append(big)
    torch.cuda.synchronize()
    paths = pgcn.path_counts()
    return [b.cpu().numpy() for b in bigs], paths


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_case(bigs, paths, ref, bound, dim, family, what):
    """The assertions every case shares; returns the output rows [n_rows, 4 vec] of the first
    call and prints the largest err / bound."""
    ld = (dim + 3) // 4 * 4
    first = bigs[0]
    for k, o in enumerate(bigs[1:]):
        assert same_bits(o, first), f"{what}: call {k + 2} differs from call 1"
    assert (first[:GUARD] == SENTINEL).all() and (first[-GUARD:] == SENTINEL).all(), \
        f"{what}: rows next to the output were written"
    body = first[GUARD:-GUARD]
    assert ref.shape[0] == body.shape[0]
    assert np.isnan(body[:, ld:]).all(), f"{what}: output columns past 4 vec were written"
    assert (body[:, dim:ld] == 0.0).all(), f"{what}: padding columns are not 0"
    err = np.abs(body[:, :dim].astype(np.float64) - ref[:, :dim])
    bnd = bound[:, :dim]
    ratio = float(np.nan_to_num(err / (bnd + 1e-30), nan=np.inf).max())
    print(f"{what}: max err/bound {ratio:.3g}")
    assert (err <= TOL * bnd + 1e-30).all(), f"{what}: max err/bound {ratio:.3g}"
    other = "gs_ring" if family == "gs_gather" else "gs_gather"
    assert paths[family] >= CALLS and paths[other] == 0, (what, paths)
    return body[:, :ld]


# --------------------------------------------------------------------------- 1. the ladder
@gpu
@pytest.mark.parametrize("dim", LADDER_DIMS)
def test_ladder_default(pgcn, dim):
    """Every width body at several paddings on the ladder, default knobs (gs_split 3: item
    length by shape, workgroup items at power-of-two widths, in-kernel arrivals: one launch)."""
    lad = ladder()
    with values_graph(pgcn, lad) as g:
        bigs, paths = gs_calls(pgcn, g, lad["x"], lad["n"], dim)
    check_case(bigs, paths, lad["ref"], lad["bound"], dim, "gs_gather", f"ladder dim {dim}")
    assert paths["launches"] == CALLS, paths


KNOB_CASES = (dict(gs_split=0),                     # the combine launch
              dict(gs_split=2),                     # long rows as one item
              dict(gs_split=1, gs_item_iters=2),    # most rows split, most arrivals
              dict(gs_split=1, gs_item_iters=32))


@gpu
@pytest.mark.parametrize("vec", VECS)
def test_ladder_knobs(pgcn, vec):
    """One dim per body under the other split modes; gs_split 1 gives gs_split 0's bits at the
    same item length (32 iterations: gs_split 0 never shortens its items) without its combine
    launches.  (gs_split 2 / 3 and shorter items sum in another order: reference only.)"""
    lad, dim = ladder(), 4 * vec - 3
    res = []
    for kw in KNOB_CASES:
        with helpers.knobs(pgcn, **kw), values_graph(pgcn, lad) as g:
            bigs, paths = gs_calls(pgcn, g, lad["x"], lad["n"], dim)
        check_case(bigs, paths, lad["ref"], lad["bound"], dim, "gs_gather",
                   f"ladder vec {vec} {kw}")
        res.append((bigs[0], paths["launches"]))
    assert same_bits(res[3][0], res[0][0]), "gs_split 1 at 32 iterations != gs_split 0"
    assert res[0][1] == 2 * CALLS and res[3][1] == CALLS, (res[0][1], res[3][1])


@gpu
@pytest.mark.parametrize("vec", VECS)
def test_ladder_large(pgcn, vec):
    """The ladder 9 times over (1.2 M slots, past kSmallNnz): the non-small unblocked schedule,
    items of NB * 32 slots and a combine launch."""
    lad, dim = ladder(9), 4 * vec - 3
    assert lad["indptr"][-1] > K_SMALL_NNZ
    with values_graph(pgcn, lad) as g:
        bigs, paths = gs_calls(pgcn, g, lad["x"], lad["n"], dim)
    check_case(bigs, paths, lad["ref"], lad["bound"], dim, "gs_gather", f"large ladder vec {vec}")
    assert paths["launches"] == 2 * CALLS, paths


@gpu
@pytest.mark.parametrize("dim", [52, 72, 100])
def test_ladder_multipass(pgcn, dim):
    """Widths without a body of their own on the plain path: 16-column passes, the last one
    overlapping (DevGraph::graphsum: c = min(c0, ld - 16)); each pass as a d = 16 call of its
    own gives the same bits."""
    lad, n = ladder(), LADDER_N
    assert (dim + 3) // 4 not in VECS and dim % 4 == 0
    n_pass = (dim + 15) // 16
    with values_graph(pgcn, lad) as g:
        bigs, paths = gs_calls(pgcn, g, lad["x"], n, dim)
        xin = torch.from_numpy(np.ascontiguousarray(lad["x"][:, :dim])).to(DEV)
        ones = {}
        for c0 in range(0, dim, 16):
            c = min(c0, dim - 16)
            one = torch.full((n, 16), float("nan"), device=DEV)
            pgcn.check(pgcn.lib.pgcn_graphsum(g, vp(xin[:, c:]), dim, vp(one), 16, 16, stream()),
                       "graphsum pass")
            ones[c] = one
        torch.cuda.synchronize()
    body = check_case(bigs, paths, lad["ref"], lad["bound"], dim, "gs_gather",
                      f"ladder multi-pass dim {dim}")
    assert paths["gs_gather"] == n_pass * CALLS, paths
    for c, one in ones.items():
        assert same_bits(one.cpu().numpy(), np.ascontiguousarray(body[:, c:c + 16])), c


# --------------------------------------------------------------------------- 2. leading dims
@functools.lru_cache(maxsize=None)
def small_ring_graph():
    """The smallest square graph that takes the LDS ring (rows >= kLdsMinRows, table > 1 MB):
    n = 32768, average degree 8, a few hubs; the parser's coefficients (pgcn_graph_create)."""
    n = 32768
    indptr, indices = helpers.random_graph(n, 8, seed=77, hubs=4, hub_deg=1500)
    deg = np.diff(indptr).astype(np.float64)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    vals = 1.0 / np.sqrt(deg[rows] * deg[indices])
    x = np.random.default_rng(78).standard_normal((n, 44)).astype(np.float32)
    ref, bound = helpers.csr_reference(indptr, indices, vals, x)
    frozen(indptr, indices, x, ref, bound)
    return dict(n=n, indptr=indptr, indices=indices, x=x, ref=ref, bound=bound)


def test_small_ring_graph_takes_the_ring():
    """Host only: DevGraph::uses_lds' shape conditions."""
    gr = small_ring_graph()
    assert gr["n"] >= LDS_MIN_ROWS and gr["n"] > LDS_MIN_COLS
    assert (np.diff(gr["indptr"]) >= 1).all()  # self loops: no empty row, finite coefficients


LD_CASES = [(0, 8), (8, 0)]  # (ld_in, ld_out) - 4 vec


@gpu
@pytest.mark.parametrize("wide_in,wide_out", LD_CASES)
@pytest.mark.parametrize("vec", VECS)
def test_leading_dims_gather(pgcn, vec, wide_in, wide_out):
    """ld_in != ld_out on the gather kernels: NaN input columns past 4 vec reach no output, the
    wider output keeps its NaN prefill past 4 vec, the rows around the output stay untouched."""
    lad, dim = ladder(), 4 * vec - 3
    with values_graph(pgcn, lad) as g:
        bigs, paths = gs_calls(pgcn, g, lad["x"], lad["n"], dim, wide_in, wide_out)
    check_case(bigs, paths, lad["ref"], lad["bound"], dim, "gs_gather",
               f"ld vec {vec} in +{wide_in} out +{wide_out}")


@gpu
@pytest.mark.parametrize("wide_in,wide_out", LD_CASES)
@pytest.mark.parametrize("dim", [16, 41])
def test_leading_dims_ring(pgcn, dim, wide_in, wide_out):
    """The same on the LDS ring.  pass_col in DevGraph::graphsum: pass p of ceil(dim / 16) reads
    and writes the 16 columns from min(16 p, min(ld_in, ld_out) - 16).  The narrower of the two
    leading dims is 4 vec here, so the passes' union is columns 0 .. 4 vec of both buffers (dim
    41, ld 44: passes at 0, 16 and 28, the last overlapping the second): nothing past 4 vec may
    be read or written -- what check_case asserts."""
    gr = small_ring_graph()
    ldm = (dim + 3) // 4 * 4
    cols = set()
    for p in range((dim + 15) // 16):
        c = min(16 * p, ldm - 16)
        cols.update(range(c, c + 16))
    assert cols == set(range(ldm))
    g = ctypes.c_void_p()
    pgcn.check(pgcn.lib.pgcn_graph_create(gr["n"], helpers.ptr(gr["indptr"]),
                                          helpers.ptr(gr["indices"]), ctypes.byref(g)), "create")
    try:
        bigs, paths = gs_calls(pgcn, g, gr["x"], gr["n"], dim, wide_in, wide_out)
    finally:
        pgcn.lib.pgcn_graph_destroy(g)
    check_case(bigs, paths, gr["ref"], gr["bound"], dim, "gs_ring",
               f"ld ring dim {dim} in +{wide_in} out +{wide_out}")


# --------------------------------------------------------------------------- 3. blocked layout
# (dim, n, gs16_gather): the smallest power-of-two n whose table n * vec * 16 B exceeds kL2Budget
BLOCKED_CASES = [(3, 262144, 0), (7, 131072, 0), (13, 65536, 1), (13, 65536, 2), (15, 65536, 1),
                 (15, 65536, 2), (29, 32768, 0), (32, 32768, 0)]


@functools.lru_cache(maxsize=2)
def blocked_graph(n):
    """Random symmetric graph, average degree 6, a few hubs of 3000, then every 5th row emptied;
    random values (no ring); a 32-wide input and its reference."""
    indptr, indices = helpers.random_graph(n, 6, seed=n, hubs=5, hub_deg=3000, empty_rows=5)
    rng = np.random.default_rng(n + 1)
    vals = rng.uniform(-1, 1, len(indices)).astype(np.float32)
    x = rng.standard_normal((n, 32)).astype(np.float32)
    ref, bound = helpers.csr_reference(indptr, indices, vals, x)
    frozen(indptr, indices, vals, x, ref, bound)
    return dict(n=n, indptr=indptr, indices=indices, vals=vals, x=x, ref=ref, bound=bound)


def test_blocked_sizes_are_past_the_switch():
    """Host only: DevGraph::column_blocks returns 8 when G < 64 and n_cols * vec * 16 >
    kL2Budget; each case's n is the smallest power of two there, and the builder empties rows."""
    for dim, n, _ in BLOCKED_CASES:
        vec = (dim + 3) // 4
        assert GROUP_LANES[vec] < 64
        assert n * vec * 16.0 > L2_BUDGET >= (n // 2) * vec * 16.0, (dim, n)
    indptr, _ = helpers.random_graph(1000, 6, seed=1, hubs=2, hub_deg=100, empty_rows=5)
    deg = np.diff(indptr)
    assert (deg[4::5] == 0).all() and (np.delete(deg, np.arange(4, 1000, 5)) >= 1).all()


@gpu
@pytest.mark.parametrize("dim,n,gather16", BLOCKED_CASES)
def test_blocked_layout_widths(pgcn, dim, n, gather16):
    """nbc = 8 with 4-padded segments through k_graphsum<1, 16>, <2, 16>, <8, 32>, and at dim
    13 / 15 (padding columns inside the last float4) through k_graphsum16 (gs16_gather 1) and
    the interleaved k_graphsum<4, 16> (2); empty rows are comb entries of count 0."""
    gr = blocked_graph(n)
    with helpers.knobs(pgcn, gs16_gather=gather16), values_graph(pgcn, gr) as g:
        bigs, paths = gs_calls(pgcn, g, gr["x"], n, dim)
    body = check_case(bigs, paths, gr["ref"], gr["bound"], dim, "gs_gather",
                      f"blocked dim {dim} n {n} gs16_gather {gather16}")
    assert paths["launches"] == 2 * CALLS, paths  # the blocked layout always combines
    assert (body[4::5] == 0.0).all()


# --------------------------------------------------------------------------- 4. rank graphs
@functools.lru_cache(maxsize=4)
def varied_graph(n, deg_hi, deg_lo):
    """Symmetric random graph (self loop first) whose expected degree is deg_hi on the first
    quarter of the nodes and deg_lo on the rest, so that nnz-balanced node ranges hold unequal
    node counts; an input of 128 columns and the whole graph's float64 GraphSum."""
    rng = np.random.default_rng(n)
    w = np.where(np.arange(n) < n // 4, deg_hi - 1.0, deg_lo - 1.0)
    m = int(w.sum() / 2)
    u = rng.choice(n, m, p=w / w.sum())
    v = rng.choice(n, m, p=w / w.sum())
    keep = u != v
    u, v = u[keep], v[keep]
    src = np.concatenate([u, v, np.arange(n)])
    dst = np.concatenate([v, u, np.arange(n)])
    order = np.lexsort((dst, src != dst, src))
    src, dst = src[order], dst[order]
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, src + 1, 1)
    indptr = np.cumsum(indptr).astype(np.int32)
    indices = dst.astype(np.int32)
    deg = np.diff(indptr).astype(np.float64)
    vals = 1.0 / np.sqrt(deg[src] * deg[indices])
    x = rng.standard_normal((n, 128)).astype(np.float32)
    ref, bound = helpers.csr_reference(indptr, indices, vals, x)
    frozen(indptr, indices, x, ref, bound)
    return dict(n=n, indptr=indptr, indices=indices, x=x, ref=ref, bound=bound)


def rank_chunk(pgcn, gr, world, rank, chunks, chunk):
    """Rank `rank`'s GraphSum graph of reduce-scatter chunk `chunk`, cut out of
    pgcn_partition_subgraph's padded layout (world * maxrows rows) by make_partition's rule:
    maxrows rounded up to a multiple of chunks, h = maxrows / chunks rows per owner and chunk,
    chunk row q h + j = owner q's local row chunk h + j (padding past the owner's nodes).
    Returns (indptr, indices, vals, node): node[r] = the global node of row r, -1 = padding."""
    bounds, maxrows = pgcn.partition_bounds(gr["indptr"], world)
    sp, si, sv = pgcn.partition_subgraph(gr["indptr"], gr["indices"], world, rank)
    h = (maxrows + chunks - 1) // chunks
    q, j = np.divmod(np.arange(world * h), h)
    local = chunk * h + j
    real = local < np.diff(bounds)[q]
    src = np.where(real, q * maxrows + local, 0)
    lens = np.where(real, sp[src + 1] - sp[src], 0).astype(np.int64)
    ip = np.concatenate([[0], np.cumsum(lens)])
    idx = np.repeat(sp[src] - ip[:-1], lens) + np.arange(ip[-1])
    node = np.where(real, bounds[q] + local, -1)
    return ip.astype(np.int32), si[idx], sv[idx], node, bounds


# gather path: degrees about 20 / 4.  Ring path: every rank that is run needs more than
# kLdsMinBytes / 64 = 16384 columns, i.e. rank 0 more than 16384 of 36000 (140000 / 8 = 17500)
# nodes, which bounds the first quarter's degree by 1.36x (1.09x) the rest's: 5 / 4 and 4.2 / 4
RANK_GATHER = dict(n=6000, hi=20, lo=4, world=3)
RANK_RING = dict(n=36000, hi=5, lo=4, world=2)
RANK_RING_TALL = dict(n=140000, hi=4.2, lo=4, world=8)


def test_rank_graph_shapes(pgcn):
    """Host only: the rank graphs' rows and cols against the thresholds their cases assume, real
    padded rows in each, and rank_chunk's cut of the padded layout keeping every slot."""
    for spec, ranks, ring in ((RANK_GATHER, (0, 1, 2), False), (RANK_RING, (0, 1), True),
                              (RANK_RING_TALL, (0, 7), True)):
        gr = varied_graph(spec["n"], spec["hi"], spec["lo"])
        bounds, maxrows = pgcn.partition_bounds(gr["indptr"], spec["world"])
        counts = np.diff(bounds)
        assert counts.min() < maxrows, "no padded rows"
        rows = spec["world"] * maxrows
        for r in ranks:
            cols = int(counts[r])
            if ring:  # DevGraph::uses_lds
                assert rows >= LDS_MIN_ROWS and cols > LDS_MIN_COLS, (spec, r, rows, cols)
            else:
                assert rows < LDS_MIN_ROWS
        if spec is RANK_RING:        # lds_blocks: square-ish, short of the tall rule (4 blocks)
            assert all(0.9 * c <= rows < 6 * c for c in counts)
        if spec is RANK_RING_TALL:   # lds_blocks: rows >= 6 cols -> 2 blocks
            assert all(rows >= 6 * counts[r] for r in ranks)
    gr = varied_graph(RANK_GATHER["n"], RANK_GATHER["hi"], RANK_GATHER["lo"])
    for rank in range(3):
        total = 0
        for chunk in range(2):
            ip, ix, vals, node, bounds = rank_chunk(pgcn, gr, 3, rank, 2, chunk)
            total += len(ix)
            assert len(ix) == ip[-1] and (np.diff(ip)[node < 0] == 0).all()
            assert ix.size == 0 or ix.max() < bounds[rank + 1] - bounds[rank]
        _, si, _ = pgcn.partition_subgraph(gr["indptr"], gr["indices"], 3, rank)
        assert total == len(si)


def run_rank_graphs(pgcn, spec, chunks, ranks, dim, family, what):
    """Every (rank, chunk) graph of pgcn_debug_rank_graph against its float64 reference; returns
    the outputs summed over the given ranks in float64, by global node."""
    gr = varied_graph(spec["n"], spec["hi"], spec["lo"])
    n, world = spec["n"], spec["world"]
    total = np.zeros((n, dim))
    for rank in ranks:
        for chunk in range(chunks):
            ip, ix, vals, node, bounds = rank_chunk(pgcn, gr, world, rank, chunks, chunk)
            lo, hi = int(bounds[rank]), int(bounds[rank + 1])
            xr = gr["x"][lo:hi]
            ref, bound = helpers.csr_reference(ip, ix, vals, xr[:, :dim], n_cols=hi - lo)
            g, rows, cols = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
            pgcn.check(pgcn.lib.pgcn_debug_rank_graph(
                n, helpers.ptr(gr["indptr"]), helpers.ptr(gr["indices"]), world, rank, chunks,
                chunk, ctypes.byref(g), ctypes.byref(rows), ctypes.byref(cols)), "rank_graph")
            try:
                assert (rows.value, cols.value) == (len(ip) - 1, hi - lo)
                assert pgcn.lib.pgcn_graph_nnz(g) == len(ix)
                bigs, paths = gs_calls(pgcn, g, xr, rows.value, dim)
            finally:
                pgcn.lib.pgcn_graph_destroy(g)
            body = check_case(bigs, paths, ref, bound, dim, family,
                              f"{what} rank {rank} chunk {chunk}/{chunks}")
            pad = node < 0
            assert pad.any() or chunks > 1
            assert same_bits(body[pad], np.zeros_like(body[pad])), "padded rows are not +0"
            np.add.at(total, node[~pad], body[~pad][:, :dim].astype(np.float64))
    return gr, total


def check_recomposed(gr, total, dim, what):
    """The ranks' outputs summed by node against the whole graph's float64 GraphSum: each
    rank's error is within 1e-5 of its own bound and the ranks' bounds add up to the whole
    graph's, so the same rule holds for the sum."""
    err = np.abs(total - gr["ref"][:, :dim])
    bnd = gr["bound"][:, :dim]
    print(f"{what}: recomposed max err/bound {(err / (bnd + 1e-30)).max():.3g}")
    assert (err <= TOL * bnd + 1e-30).all(), (what, (err / (bnd + 1e-30)).max())


@gpu
@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("dim", [7, 16])
def test_rank_graphs_gather(pgcn, dim, chunks):
    """Edge-cut rank graphs below the ring's size (n = 6000 at 3 ranks): rectangular, padded
    empty tail rows of scale 0, every rank and chunk; recomposed over the ranks they give the
    whole graph's GraphSum (the GPU counterpart of test_partition_subgraphs_recompose_graphsum)."""
    what = f"rank gather dim {dim} chunks {chunks}"
    gr, total = run_rank_graphs(pgcn, RANK_GATHER, chunks, range(3), dim, "gs_gather", what)
    check_recomposed(gr, total, dim, what)


@gpu
@pytest.mark.parametrize("dim,blocks", [(16, 0), (41, 0), (128, 0), (16, 8), (16, 32)])
def test_rank_graphs_ring(pgcn, dim, blocks):
    """Rank graphs on the LDS ring (38 k padded rows x 17 - 19 k columns at 2 ranks): the shape
    rule's 4 column blocks, and 8 and 32 through lds_blocks; padded rows exactly 0; both ranks
    recomposed."""
    what = f"rank ring dim {dim} lds_blocks {blocks}"
    with helpers.knobs(pgcn, lds_blocks=blocks):
        gr, total = run_rank_graphs(pgcn, RANK_RING, 1, range(2), dim, "gs_ring", what)
    check_recomposed(gr, total, dim, what)


@gpu
def test_rank_graphs_ring_tall(pgcn):
    """Ranks 0 and 7 of 8 at n = 140000: rows >= 6 x cols, lds_blocks' 2-block rule."""
    run_rank_graphs(pgcn, RANK_RING_TALL, 1, (0, 7), 16, "gs_ring", "rank ring tall dim 16")


# --------------------------------------------------------------------------- knob scope
def _scoped_calls(pgcn, kw, create, dims, x, n_rows, calls_inside):
    """A graph created inside knobs(**kw); its first GraphSum of every width in `dims` made
    inside the block too, or only after it has closed."""
    with contextlib.ExitStack() as st:
        with helpers.knobs(pgcn, **kw):
            g = st.enter_context(create())
            if calls_inside:
                return [gs_calls(pgcn, g, x, n_rows, dim) for dim in dims]
        return [gs_calls(pgcn, g, x, n_rows, dim) for dim in dims]


@contextlib.contextmanager
def rank_graph(pgcn, gr, world, rank):
    g, rows, cols = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
    pgcn.check(pgcn.lib.pgcn_debug_rank_graph(
        gr["n"], helpers.ptr(gr["indptr"]), helpers.ptr(gr["indices"]), world, rank, 1, 0,
        ctypes.byref(g), ctypes.byref(rows), ctypes.byref(cols)), "rank_graph")
    try:
        yield g
    finally:
        pgcn.lib.pgcn_graph_destroy(g)


@gpu
def test_graph_keeps_the_knobs_it_was_created_with(pgcn):
    """A graph builds the schedule of a width at its first GraphSum of that width, with the
    knobs it was created under, whatever they are by then: created inside knobs(gs_split=0,
    gs_item_iters=32) and first called after the block (dim 16 and dim 5), the ladder gives the
    bits and the launches (the combine's) of the same calls made inside the block; and so does
    a ring graph (RANK_RING's rank 0) created under lds_blocks=2."""
    lad = ladder()
    kw = dict(gs_split=0, gs_item_iters=32)
    make = functools.partial(values_graph, pgcn, lad)
    inside = _scoped_calls(pgcn, kw, make, (16, 5), lad["x"], lad["n"], True)
    after = _scoped_calls(pgcn, kw, make, (16, 5), lad["x"], lad["n"], False)
    for (bi, pi), (ba, pa), dim in zip(inside, after, (16, 5)):
        assert pi["launches"] == 2 * CALLS and pi["gs_gather"] >= CALLS, (dim, pi)
        assert pa == pi, (dim, pa, pi)
        for x, y in zip(bi, ba):
            assert same_bits(x, y), f"ladder dim {dim}: first call after the block differs"
    gr = varied_graph(RANK_RING["n"], RANK_RING["hi"], RANK_RING["lo"])
    bounds, maxrows = pgcn.partition_bounds(gr["indptr"], RANK_RING["world"])
    xr, rows = gr["x"][:int(bounds[1])], RANK_RING["world"] * maxrows
    make = functools.partial(rank_graph, pgcn, gr, RANK_RING["world"], 0)
    (bi, pi), = _scoped_calls(pgcn, dict(lds_blocks=2), make, (16,), xr, rows, True)
    (ba, pa), = _scoped_calls(pgcn, dict(lds_blocks=2), make, (16,), xr, rows, False)
    assert pi["gs_ring"] >= CALLS and pi["gs_gather"] == 0, pi
    assert pa == pi, (pa, pi)
    for x, y in zip(bi, ba):
        assert same_bits(x, y), "ring, lds_blocks 2: first call after the block differs"
