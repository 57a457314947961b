"""Device time of the neighbourhood-heuristic kernels (DESIGN.md §3 "Link heuristics") through the
kernel ABI.

    python3 tools/heur_bench.py [--nodes 232965] [--edges 57307946] [--pairs 1000000]
                                [--queries 2048] [--width 64] [--reps 10] [--warmup 2]

On the reddit-shaped synthetic graph (bench.py's generator and sizes) the script times, per kind,
pgcn_link_heur_score on --pairs random pairs and pgcn_link_heur_rank on --queries random
(anchor, target) queries without filter lists, and beside them pgcn_link_rank -- the dot-product
sweep over a random normal embedding of --width columns -- on the same queries.  The heuristic
sweep's work is the anchors' 2-hop neighbourhood sizes, which the output carries (`two_hop_mean`,
the mean number of accumulator adds per query), not a flop count: there is no peak to hold it to.
HIP events around each call on the null stream: `warmup` calls, then `reps` timed ones, the calls
taken in turn; the median, minimum and maximum in microseconds.
Prints one JSON line.  Needs a HIP device; there is no CPU fallback."""
import argparse
import ctypes
import json
import sys
import time

import numpy as np

from rank_bench import load_pkg, timed


def note(msg, t0=[time.time()]):
    print(f"[heur_bench {time.time() - t0[0]:6.1f}s] {msg}", file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--edges", type=int, default=57307946)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("heur_bench needs a HIP device")
    lib, n, Q, m, d = pg.lib, args.nodes, args.queries, args.pairs, args.width
    rng = np.random.default_rng(1)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    ds = pg.Dataset.synthetic(n, 2, 41, args.edges, seed=1)
    note(f"graph: {int(ds.graph_indptr[-1])} stored entries")
    index = pg.CnIndex(n, ds.graph_indptr, ds.graph_indices)
    note(f"index: workspace {index.workspace} bytes")
    anchor = rng.integers(0, n, Q).astype(np.int32)
    target = rng.integers(0, n, Q).astype(np.int32)
    queries = pg.RankQueries(n, anchor, target)
    # the sweep's work: per query the sum over the anchor's neighbours of their degrees (the
    # stored pattern is symmetric, self loops and duplicates aside)
    deg = np.diff(ds.graph_indptr).astype(np.int64)
    two_hop = [int(deg[ds.graph_indices[ds.graph_indptr[a]:ds.graph_indptr[a + 1]]].sum())
               for a in anchor]
    src = torch.from_numpy(rng.integers(0, n, m).astype(np.int32)).cuda()
    dst = torch.from_numpy(rng.integers(0, n, m).astype(np.int32)).cuda()
    scores = torch.zeros(m, device="cuda", dtype=torch.float32)
    greater = torch.zeros(Q, device="cuda", dtype=torch.int32)
    equal = torch.zeros(Q, device="cuda", dtype=torch.int32)
    H = torch.randn(n, d, device="cuda", dtype=torch.float32,
                    generator=torch.Generator(device="cuda").manual_seed(1))

    def pairs(kind):
        return lambda: pg.check(lib.pgcn_link_heur_score(index.handle, kind, p(src), p(dst), m, None,
                                                         p(scores), None), "link_heur_score")

    def sweep(kind):
        return lambda: pg.check(lib.pgcn_link_heur_rank(index.handle, kind, queries.handle,
                                                        p(greater), p(equal), None), "link_heur_rank")
    calls = {"dot_rank": lambda: pg.check(lib.pgcn_link_rank(queries.handle, p(H), d, d, p(greater),
                                                             p(equal), None), "link_rank")}
    for name, kind in (("cn", 1), ("aa", 2), ("ra", 3)):
        calls[name + "_pairs"] = pairs(kind)
        calls[name + "_rank"] = sweep(kind)
    note("timing")
    out = {"nodes": n, "stored_entries": int(ds.graph_indptr[-1]), "pairs": m, "queries": Q,
           "dot_width": d, "reps": args.reps, "workspace_bytes": index.workspace,
           "two_hop_mean": round(float(np.mean(two_hop)), 1), "two_hop_max": int(max(two_hop))}
    out.update(timed(torch, calls, args.reps, args.warmup))
    for name in ("cn", "aa", "ra"):
        out[name + "_pairs"]["Mpairs_per_s"] = round(m / out[name + "_pairs"]["us_median"], 1)
        out[name + "_rank"]["Gadds_per_s"] = round(
            float(np.sum(two_hop)) / out[name + "_rank"]["us_median"] / 1e3, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
