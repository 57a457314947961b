"""The neighbourhood link heuristics (CN / AA / RA) on the device against Python integers.

One synthetic graph of 300 nodes per pattern whose raw CSR has shuffled rows, duplicates and self
loops; an isolated node, a degree-1 leaf, two hub rows above 256 cleaned entries (longer than a
lane group's share and than the LDS-staged head's threshold) and rows of exactly 8, 9, 16, 17, 32,
33, 64 and 65 entries (every group size and one more).
The patterns: symmetric and directed with 7 random edges a node (mean cleaned rows of 18 and 9
entries: lane groups of 16 and 8), and two denser directed ones with 90 and 280 (means of 89 and
271: groups of 32 and 64), so every instantiation of the pair kernel runs.  The cleaned rows
are recomputed in numpy from the raw CSR; sums of index.weights(kind) over set intersections are
Python integers, so every comparison of fixed-point sums and of counts is exact.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

N, HUBS, EXACT, LEAF, ISO = 300, (0, 1), dict(zip(range(2, 10), (8, 9, 16, 17, 32, 33, 64, 65))), 298, 299
KINDS = ("cn", "aa", "ra")


def raw_graph(symmetric, extra):
    rng = np.random.default_rng(5)
    rows = [set() for _ in range(N)]
    pool = np.arange(10, LEAF)

    def add(u, v):
        rows[u].add(int(v))
        if symmetric:
            rows[int(v)].add(u)
    for hub, deg in zip(HUBS, (270, 260)):
        for v in rng.choice(pool, deg, replace=False):
            add(hub, v)
    for u in pool:
        for v in rng.choice(pool[pool != u], extra, replace=False):
            add(int(u), v)
    for u, deg in EXACT.items():
        for v in rng.permutation(pool):
            if len(rows[u]) < deg:
                add(u, v)
    add(LEAF, HUBS[0])
    indptr, indices = [0], []
    for i, r in enumerate(rows):
        r = sorted(r)
        indices += list(rng.permutation(r + r[:2] + [i]))  # duplicates and the self loop, shuffled
        indptr.append(len(indices))
    return np.asarray(indptr, np.int32), np.asarray(indices, np.int32)


PATTERNS = {"symmetric": (True, 7, 16), "directed": (False, 7, 8), "dense": (False, 90, 32),
            "full": (False, 280, 64)}  # name: symmetric, random edges a node, the lane group


@pytest.fixture(scope="module", params=list(PATTERNS))
def graph(pgcn, request):
    """(index, cleaned rows as sets, degrees) -- the rows recomputed from the raw CSR."""
    symmetric, extra, group = PATTERNS[request.param]
    indptr, indices = raw_graph(symmetric, extra)
    clean = [set(np.unique(indices[indptr[i]:indptr[i + 1]]).tolist()) - {i} for i in range(N)]
    deg = np.array([len(c) for c in clean])
    assert all(deg[u] == d for u, d in EXACT.items()) and deg[list(HUBS)].min() >= 256
    assert deg[ISO] == 0 and deg[LEAF] == 1 and not any(ISO in c for c in clean)
    mean = deg.sum() // N  # the launcher's rule: groups of 8 / 16 / 32 / 64 up to 16 / 64 / 256
    assert group == (8 if mean <= 16 else 16 if mean <= 64 else 32 if mean <= 256 else 64)
    index = pgcn.CnIndex(N, indptr, indices)
    yield index, clean, deg
    index.close()


def test_weights_and_workspace(pgcn, graph):
    index, _, deg = graph
    assert (index.weights("cn") == 1).all()
    aa, ra = index.weights("aa").astype(np.float64), index.weights("ra").astype(np.float64)
    assert (aa[deg < 2] == 0).all() and (ra[deg < 1] == 0).all()
    big = deg >= 2
    assert np.abs(aa[big] * 2.0 ** -32 - 1.0 / np.log(deg[big])).max() <= 2.0 ** -32
    assert np.abs(ra[deg >= 1] * 2.0 ** -32 - 1.0 / deg[deg >= 1]).max() <= 2.0 ** -32
    assert index.workspace == 512 * N * 12


def test_argument_errors(pgcn, graph):
    """Every PGCN_E_INVALID case that needs a real index; nothing is launched."""
    import torch
    lib, INV, h = pgcn.lib, pgcn.PGCN_E_INVALID, graph[0].handle
    dev = torch.zeros(8, dtype=torch.int64, device="cuda")
    d = ctypes.c_void_p(dev.data_ptr())
    host = np.zeros(N, np.uint64)
    p = host.ctypes.data_as(ctypes.c_void_p)
    qs, other = pgcn.RankQueries(N, [0], [1]), pgcn.RankQueries(N + 1, [0], [1])
    for kind in (0, 4, -1):
        assert lib.pgcn_link_heur_score(h, kind, d, d, 1, d, d, None) == INV
        assert lib.pgcn_link_heur_rank(h, kind, qs.handle, d, d, None) == INV
        assert lib.pgcn_cn_index_weights(h, kind, p) == INV
        assert lib.pgcn_cn_index_score_pairs(h, kind, p, p, 1, p) == INV
        assert lib.pgcn_cn_index_link_ranks(h, kind, p, p, 0, None, None, None, None, 3, 0, 1,
                                            None, None) == INV
    for m in (2 ** 31, -1):
        assert lib.pgcn_link_heur_score(h, 1, d, d, m, d, d, None) == INV
        assert lib.pgcn_cn_index_score_pairs(h, 1, p, p, m, p) == INV
    assert lib.pgcn_link_heur_score(h, 1, d, d, 1, None, None, None) == INV  # no output
    assert lib.pgcn_link_heur_score(h, 1, None, d, 1, d, d, None) == INV
    assert lib.pgcn_link_heur_score(h, 1, d, None, 1, d, d, None) == INV
    assert lib.pgcn_cn_index_weights(h, 1, None) == INV
    assert lib.pgcn_link_heur_rank(h, 1, None, d, d, None) == INV
    assert lib.pgcn_link_heur_rank(h, 1, qs.handle, None, d, None) == INV
    assert lib.pgcn_link_heur_rank(h, 1, other.handle, d, d, None) == INV  # another node count
    assert lib.pgcn_link_heur_score(h, 1, None, None, 0, d, None, None) == pgcn.PGCN_OK  # m == 0
    assert not dev.cpu().any()


@pytest.mark.parametrize("kind", KINDS)
def test_pair_scores_are_exact(pgcn, graph, kind):
    index, clean, deg = graph
    rng = np.random.default_rng(11)
    special = [(s, s) for s in (0, 5, LEAF, ISO)] + [(0, 1), (1, 0), (0, LEAF), (LEAF, 0),
                                                      (LEAF, ISO), (LEAF, 10), (ISO, 5), (5, ISO)]
    special += [(u, v) for u in range(10) for v in range(10)]
    pairs = np.array(special + rng.integers(0, N, (1900, 2)).tolist(), np.int32)
    src, dst = pairs[:, 0].copy(), pairs[:, 1].copy()
    w = [int(x) for x in index.weights(kind)]
    common = [clean[s] & clean[d] for s, d in pairs]
    want = np.array([sum(w[z] for z in c) for c in common], np.uint64)
    assert any(len(c) == 0 for c in common[4:]) and len(common[4]) >= 128  # empty; hub-hub
    fx = index.score(src, dst, kind, raw=True)
    np.testing.assert_array_equal(fx, want)
    score = index.score(src, dst, kind)
    assert score.dtype == np.float32
    as_float = want.astype(np.float64) * (1.0 if kind == "cn" else 2.0 ** -32)
    np.testing.assert_array_equal(score, as_float.astype(np.float32))
    # independently: the float64 heuristic itself
    term = {"cn": lambda z: 1.0, "aa": lambda z: 1.0 / np.log(deg[z]) if deg[z] >= 2 else 0.0,
            "ra": lambda z: 1.0 / deg[z] if deg[z] >= 1 else 0.0}[kind]
    ref = np.array([sum(term(z) for z in sorted(c)) for c in common])
    size = np.array([len(c) for c in common])
    assert (np.abs(score.astype(np.float64) - ref) <= size * 2.0 ** -33 + 2.0 ** -23 * ref).all()
    if kind == "cn":
        np.testing.assert_array_equal(fx, size.astype(np.uint64))


@pytest.mark.parametrize("kind", KINDS)
def test_rank_counts_equal_the_pair_kernel(pgcn, graph, kind):
    index = graph[0]
    rng = np.random.default_rng(23)
    Q = 64
    anchor = np.r_[[0, 1, LEAF, ISO, 10, 5], rng.integers(0, N, Q - 6)].astype(np.int32)
    target = np.r_[[1, 7, 0, 3, ISO, 9], rng.integers(0, N, Q - 6)].astype(np.int32)
    lists = [np.setdiff1d(rng.choice(N, rng.integers(0, 21), replace=False), [t])
             for t in target]
    lists[0] = np.setdiff1d(np.r_[lists[0], anchor[0]], [target[0]])  # holds the anchor
    lists[1] = lists[1][:0]
    ptr = np.r_[0, np.cumsum([x.size for x in lists])].astype(np.int64)
    S = index.score(np.repeat(anchor, N), np.tile(np.arange(N, dtype=np.int32), Q), kind,
                    raw=True).reshape(Q, N)
    T = S[np.arange(Q), target][:, None]
    assert T[4, 0] == 0 and (T > 0).any()
    for filtered in (True, False):
        mask = np.ones((Q, N), bool)
        mask[np.arange(Q), target] = False
        if filtered:
            for e in range(Q):
                mask[e, lists[e]] = False
        qs = pgcn.RankQueries(N, anchor, target, ptr if filtered else None,
                              np.concatenate(lists).astype(np.int32) if filtered else None)
        for _ in range(2):  # the second call finds the accumulator rows zeroed
            greater, equal = index.rank(qs, kind)
            np.testing.assert_array_equal(greater, ((S > T) & mask).sum(1))
            np.testing.assert_array_equal(equal, ((S == T) & mask).sum(1))
        qs.close()


def test_python_layer_and_cli(pgcn, tmp_path):
    root = str(tmp_path)
    name = helpers.materialize_dataset("cora", root)
    ds = pgcn.Dataset.load(root, name)
    n, rng = ds.num_nodes, np.random.default_rng(3)
    rows, cols = np.repeat(np.arange(n), np.diff(ds.graph_indptr)), np.asarray(ds.graph_indices)
    pick = rng.choice(np.nonzero(rows < cols)[0], 60, replace=False)
    src = np.r_[rows[pick], rng.integers(0, n, 60)].astype(np.int32)
    dst = np.r_[cols[pick], rng.integers(0, n, 60)].astype(np.int32)
    label = np.r_[np.ones(60), np.zeros(60)].astype(np.int32)
    split = (1 + np.arange(120) % 3).astype(np.int32)
    with open(os.path.join(root, "data", name + ".links"), "w") as f:
        for e in range(120):
            f.write(f"{src[e]} {dst[e]} {label[e]} {split[e]}\n")
    ds.set_links(src, dst, label, split, 8)
    index = pgcn.CnIndex(n, ds.graph_indptr, ds.graph_indices)
    mrr = {}
    for side in ("dst", "src"):
        a, t, ptr, idx = pgcn.rank_filter(n, ds.graph_indptr, ds.graph_indices, src, dst, label,
                                          split, 3, side, True)
        qs = pgcn.RankQueries(n, a, t, ptr, idx)
        greater, equal = pgcn.heuristic_link_ranks(ds, 3, "aa", side)
        want = index.rank(qs, "aa")
        np.testing.assert_array_equal(greater, want[0])
        np.testing.assert_array_equal(equal, want[1])
        assert greater.size == a.size == 20
        mrr[side] = pgcn.mrr(pgcn.rank_from_counts(greater, equal))
    sel = split == 3
    auc = pgcn.link_auc(pgcn.heuristic_pair_scores(ds, "aa")[sel], label[sel])
    assert 0.0 <= auc <= 1.0

    exe = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "gcn-par")
    r = subprocess.run([exe, name, f"root={root}", "heuristic=aa"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    (first,) = [ln for ln in r.stdout.splitlines() if ln.startswith("heuristic ")]
    head = dict(t.split("=") for t in first.split()[1:])
    assert head["kind"] == "aa" and int(head["pairs"]) == 120
    assert abs(float(head["auc"]) - auc) <= 1e-6
    (second,) = [ln for ln in r.stdout.splitlines() if ln.startswith("rank ")]
    tok = second.split()
    for k, side in enumerate(("dst", "src")):
        got = dict(t.split("=") for t in tok[1 + 6 * k:7 + 6 * k])
        assert got["side"] == side and int(got["queries"]) == 20
        assert abs(float(got["mrr"]) - mrr[side]) <= 1e-6
    os.remove(os.path.join(root, "data", name + ".links"))
    r = subprocess.run([exe, name, f"root={root}", "heuristic=aa"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and ".links" in r.stderr
