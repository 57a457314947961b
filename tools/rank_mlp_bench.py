"""Device time of the ranking sweep under the MLP decoder (DESIGN.md §3 "Link ranking under the
decoder") through the kernel ABI.

    python3 tools/rank_mlp_bench.py [--nodes 232965] [--queries 8192]
                                    [--shapes 16x16,64x64,128x128] [--reps 30] [--warmup 5]
                                    [--pairs 10000000]

Over a random normal embedding H [nodes][d], a random normal decoder tensor P [d + 3][h] and
--queries random (anchor, target) queries without filter lists the script times pgcn_link_rank_mlp
and its YARDSTICK, pgcn_link_mlp_fwd on the explicit pairs (anchor, v), v = 0 .. nodes - 1, of as
many whole queries as fit in --pairs pairs: the same flops per pair, but two rows gathered per pair
and no candidate row reused across queries.  The two are compared per scored pair (the rank call
scores queries x nodes of them, its thresholds included in its time).
HIP events around each call on the null stream: `warmup` calls, then `reps` timed ones, the calls
taken in turn; the median, minimum and maximum in microseconds, ns per pair, and the rank call's
TF/s of 2 Q n d h flops against the 157.3 TF fp32 matrix peak.
Prints one JSON line.  Needs a HIP device; there is no CPU fallback."""
import argparse
import json

import numpy as np

from rank_bench import PEAK_TF, load_pkg, timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--shapes", default="16x16,64x64,128x128")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=10_000_000)
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    if any(d % 4 or h % 4 or not (4 <= d <= 128 and 4 <= h <= 128) for d, h in shapes):
        raise SystemExit("--shapes: DxH, multiples of 4 in [4, 128]")
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rank_mlp_bench needs a HIP device")
    n, Q = args.nodes, args.queries
    rng = np.random.default_rng(1)
    anchor = rng.integers(0, n, Q).astype(np.int32)
    target = rng.integers(0, n, Q).astype(np.int32)
    queries = pg.RankQueries(n, anchor, target)
    whole = max(1, min(Q, args.pairs // n))  # the yardstick's queries
    pairs = pg.Links(n, np.repeat(anchor[:whole], n),
                     np.tile(np.arange(n, dtype=np.int32), whole), np.full(whole * n, -1, np.int32))
    gen = torch.Generator(device="cuda").manual_seed(1)
    greater = torch.zeros(Q, device="cuda", dtype=torch.int32)
    equal = torch.zeros(Q, device="cuda", dtype=torch.int32)
    scores = torch.empty(whole * n, 4, device="cuda", dtype=torch.float32)
    out = {"nodes": n, "queries": Q, "reps": args.reps, "tile": list(pg.link_rank_mlp_tile()),
           "yardstick_pairs": whole * n}
    for d, h in shapes:
        H = torch.randn(n, d, device="cuda", generator=gen, dtype=torch.float32)
        P = torch.zeros(d + 3, h, device="cuda", dtype=torch.float32)
        P[:d + 2] = torch.randn(d + 2, h, device="cuda", generator=gen, dtype=torch.float32)
        calls = {
            "rank_mlp": lambda: queries.rank_mlp(H, d, d, P, h, h, greater, equal),
            "yardstick": lambda: pairs.mlp_fwd(H, d, d, P, h, h, scores, 4),
        }
        res = timed(torch, calls, args.reps, args.warmup)
        res["rank_mlp"]["ns_per_pair"] = round(res["rank_mlp"]["us_median"] * 1e3 / (Q * n), 5)
        res["yardstick"]["ns_per_pair"] = round(res["yardstick"]["us_median"] * 1e3 / (whole * n), 5)
        res["rank_over_yardstick_per_pair"] = round(
            res["rank_mlp"]["ns_per_pair"] / res["yardstick"]["ns_per_pair"], 3)
        tf = 2.0 * Q * n * d * h / res["rank_mlp"]["us_median"] / 1e6
        res["rank_mlp"]["TFps"] = round(tf, 1)
        res["rank_mlp"]["of_peak"] = round(tf / PEAK_TF, 3)
        res["yardstick"]["TFps"] = round(2.0 * whole * n * d * h / res["yardstick"]["us_median"] / 1e6, 1)
        out[f"d{d}h{h}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
