"""Device time of top-K retrieval under the MLP decoder (DESIGN.md §3 "Link top-K under the
decoder") through the kernel ABI.

    python3 tools/topk_mlp_bench.py [--nodes 232965] [--queries 8192]
                                    [--shapes 16x16,64x64,128x128] [--ks 10,100] [--reps 30]
                                    [--warmup 5] [--row 492]

Over a random normal embedding H [nodes][d], a random normal decoder tensor P [d + 3][h] and
--queries random anchors the script times pgcn_link_topk_mlp at every k of --ks, without lists and
with exclude lists of --row random entries each (the reddit-shaped average row length), and its
YARDSTICK, pgcn_link_rank_mlp without lists on the same anchors and inputs: the same operands,
flops, staging and per-query MFMA code with a counting epilogue (its thresholds' pair forward and
the counts' zeroing are in its time; the top-K call's merge is in its).  Per (shape, k) it reports
top-K / rank: the ratio of the medians, and the median, minimum and maximum of the per-repetition
ratios; and the top-K call's whole-call TF/s of 2 Q n d h flops.
HIP events around each call on the null stream: `warmup` calls, then `reps` timed ones, the calls
taken in turn; the median, minimum and maximum in microseconds.
Prints one JSON line.  Needs a HIP device; there is no CPU fallback."""
import argparse
import json

import numpy as np

from topk_bench import load_pkg, ratio, stats, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--shapes", default="16x16,64x64,128x128")
    ap.add_argument("--ks", default="10,100")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--row", type=int, default=492)
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    ks = [int(k) for k in args.ks.split(",")]
    if any(d % 4 or h % 4 or not (4 <= d <= 128 and 4 <= h <= 128) for d, h in shapes):
        raise SystemExit("--shapes: DxH, multiples of 4 in [4, 128]")
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("topk_mlp_bench needs a HIP device")
    n, Q = args.nodes, args.queries
    rng = np.random.default_rng(1)
    anchors = rng.integers(0, n, Q).astype(np.int32)
    targets = rng.integers(0, n, Q).astype(np.int32)
    # `row` distinct entries per query, ascending
    xidx = (np.sort(rng.integers(0, n - args.row, (Q, args.row)), axis=1) +
            np.arange(args.row)).astype(np.int32)
    xptr = np.arange(Q + 1, dtype=np.int64) * args.row
    rankq = pg.RankQueries(n, anchors, targets)
    sets = {}
    for k in ks:
        sets[f"topk{k}"] = pg.TopKQueries(n, anchors, k=k, decoder=True)
        sets[f"topk{k}_lists"] = pg.TopKQueries(n, anchors, xptr, xidx.ravel(), k=k, decoder=True)
    greater = torch.zeros(Q, device="cuda", dtype=torch.int32)
    equal = torch.zeros(Q, device="cuda", dtype=torch.int32)
    idx = torch.zeros(Q * max(ks), device="cuda", dtype=torch.int32)
    score = torch.zeros(Q * max(ks), device="cuda", dtype=torch.float32)
    out = {"nodes": n, "queries": Q, "reps": args.reps, "tile": list(pg.link_topk_mlp_tile()),
           "splits": pg.link_topk_mlp_splits(Q, n), "exclude_row": args.row,
           "workspace_bytes": {name: q.workspace for name, q in sets.items()}}
    gen = torch.Generator(device="cuda").manual_seed(1)
    for d, h in shapes:
        H = torch.randn(n, d, device="cuda", generator=gen, dtype=torch.float32)
        P = torch.zeros(d + 3, h, device="cuda", dtype=torch.float32)
        P[:d + 2] = torch.randn(d + 2, h, device="cuda", generator=gen, dtype=torch.float32)

        def topk(q, H=H, P=P, d=d, h=h):
            return lambda: q.topk_mlp(H, d, d, P, h, h, idx, score)
        calls = {"rank_mlp": lambda: rankq.rank_mlp(H, d, d, P, h, h, greater, equal)}
        calls.update({name: topk(q) for name, q in sets.items()})
        t = timed(torch, calls, args.reps, args.warmup)
        res = {name: stats(v) for name, v in t.items()}
        for name in sets:
            res[name]["over_rank"] = ratio(t[name], t["rank_mlp"])
            res[name]["whole_call_TFps"] = round(
                2.0 * Q * n * d * h / res[name]["us_median"] / 1e6, 1)
        out[f"d{d}h{h}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
