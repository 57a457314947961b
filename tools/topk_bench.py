"""Device time of the top-K retrieval kernels (DESIGN.md §3 "Link top-K") through the kernel ABI.

    python3 tools/topk_bench.py [--nodes 232965] [--queries 8192] [--widths 16,64,128]
                                [--ks 10,100] [--reps 30] [--warmup 5] [--row 492]

Over a random normal embedding H [nodes][d] and --queries random anchors the script times
pgcn_link_topk at every k of --ks, without lists and with exclude lists of --row random entries
each (the reddit-shaped average row length), and its YARDSTICK, pgcn_link_rank without lists on the
same anchors: the same operands, flops and staging with a counting epilogue.  Per (d, k) it reports
top-K / rank: the ratio of the medians, and the median, minimum and maximum of the per-repetition
ratios.  One adversarial line without a bar: d = 4 with every score ascending in v (H[v] = (v / n,
0, 0, 0), anchors >= 1), so every candidate passes the threshold and prunes are at their most
frequent.
HIP events around each call on the null stream: `warmup` calls, then `reps` timed ones, the calls
taken in turn; the median, minimum and maximum in microseconds.
Prints one JSON line.  Needs a HIP device; there is no CPU fallback."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(torch, calls, reps, warmup):
    """name -> the `reps` times in microseconds, the calls taken in turn."""
    null = torch.cuda.default_stream()
    times = {k: [] for k in calls}
    with torch.cuda.stream(null):
        for _ in range(warmup):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        for _ in range(reps):
            for k, f in calls.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(null)
                f()
                e1.record(null)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
    return times


def stats(t):
    return {"us_median": round(statistics.median(t), 1), "us_min": round(min(t), 1),
            "us_max": round(max(t), 1)}


def ratio(t, base):
    r = [a / b for a, b in zip(t, base)]
    return {"of_medians": round(statistics.median(t) / statistics.median(base), 3),
            "median": round(statistics.median(r), 3), "min": round(min(r), 3),
            "max": round(max(r), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--widths", default="16,64,128")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--row", type=int, default=492)
    args = ap.parse_args()
    widths = [int(w) for w in args.widths.split(",")]
    ks = [int(k) for k in args.ks.split(",")]
    if any(w % 4 or not 4 <= w <= 128 for w in widths):
        raise SystemExit("--widths: multiples of 4 in [4, 128]")
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench needs a HIP device")
    lib, n, Q = pg.lib, args.nodes, args.queries
    rng = np.random.default_rng(1)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    anchors = rng.integers(1, n, Q).astype(np.int32)
    targets = rng.integers(0, n, Q).astype(np.int32)
    # `row` distinct entries per query, ascending
    xidx = (np.sort(rng.integers(0, n - args.row, (Q, args.row)), axis=1) +
            np.arange(args.row)).astype(np.int32)
    xptr = (np.arange(Q + 1, dtype=np.int64) * args.row)
    rankq = pg.RankQueries(n, anchors, targets)
    sets = {}
    for k in ks:
        sets[f"topk{k}"] = pg.TopKQueries(n, anchors, k=k)
        sets[f"topk{k}_lists"] = pg.TopKQueries(n, anchors, xptr, xidx.ravel(), k=k)
    kmax = max(ks)
    greater = torch.zeros(Q, device="cuda", dtype=torch.int32)
    equal = torch.zeros(Q, device="cuda", dtype=torch.int32)
    idx = torch.zeros(Q * kmax, device="cuda", dtype=torch.int32)
    score = torch.zeros(Q * kmax, device="cuda", dtype=torch.float32)
    out = {"nodes": n, "queries": Q, "reps": args.reps, "tile": list(pg.link_topk_tile()),
           "splits": pg.link_topk_splits(Q, n), "exclude_row": args.row,
           "workspace_bytes": {name: q.workspace for name, q in sets.items()}}
    gen = torch.Generator(device="cuda").manual_seed(1)

    def run(H, d, names):
        def topk(q):
            return lambda: pg.check(lib.pgcn_link_topk(q.handle, p(H), d, d, p(idx), p(score),
                                                       None), "link_topk")
        calls = {"rank": lambda: pg.check(lib.pgcn_link_rank(rankq.handle, p(H), d, d, p(greater),
                                                             p(equal), None), "link_rank")}
        for name in names:
            calls[name] = topk(sets[name])
        t = timed(torch, calls, args.reps, args.warmup)
        res = {name: stats(v) for name, v in t.items()}
        for name in names:
            res[name]["over_rank"] = ratio(t[name], t["rank"])
        return res

    for d in widths:
        H = torch.randn(n, d, device="cuda", generator=gen, dtype=torch.float32)
        out[f"d{d}"] = run(H, d, list(sets))
    # the adversarial line: every candidate passes, a prune in nearly every tile
    H = torch.zeros(n, 4, device="cuda", dtype=torch.float32)
    H[:, 0] = torch.arange(n, device="cuda", dtype=torch.float32) / n
    out["d4_ascending"] = run(H, 4, [f"topk{k}" for k in ks])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
