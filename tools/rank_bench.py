"""Device time of the ranking kernels (DESIGN.md §3 "Link ranking") through the kernel ABI.

    python3 tools/rank_bench.py [--nodes 232965] [--queries 8192] [--widths 16,64,128]
                                [--reps 30] [--warmup 5] [--big 100000] [--row 492]

Over a random normal embedding H [nodes][d] and --queries random (anchor, target) queries the script
times pgcn_link_rank without filter lists and its YARDSTICK, pgcn_gemm(M = queries, N = nodes,
K = d, trans_b = 1) on a dense copy of the gathered anchor rows (made untimed): the same flops over
the same operands, plus a queries x nodes matrix written that the rank call never forms.  Then,
without a yardstick, --big queries (0: skipped) unfiltered, as TF/s of 2 Q n d flops against the
157.3 TF fp32 peak, and the same --queries queries with filter lists of --row random entries each
(the reddit-shaped average row length), whose extra time is the filter correction's share.
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
PEAK_TF = 157.3


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def timed(torch, calls, reps, warmup):
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
    return {k: {"us_median": round(statistics.median(t), 1), "us_min": round(min(t), 1),
                "us_max": round(max(t), 1)} for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--queries", type=int, default=8192)
    ap.add_argument("--widths", default="16,64,128")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--big", type=int, default=100000)
    ap.add_argument("--row", type=int, default=492)
    args = ap.parse_args()
    widths = [int(w) for w in args.widths.split(",")]
    if any(w % 4 or not 4 <= w <= 128 for w in widths):
        raise SystemExit("--widths: multiples of 4 in [4, 128]")
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rank_bench needs a HIP device")
    lib, n, Q = pg.lib, args.nodes, args.queries
    rng = np.random.default_rng(1)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def query_set(count, row=0):
        a = rng.integers(0, n, count).astype(np.int32)
        t = rng.integers(0, n, count).astype(np.int32)
        if not row:
            return a, pg.RankQueries(n, a, t)
        # `row` distinct entries per query, ascending, none the target
        idx = np.sort(rng.integers(0, n - row, (count, row)), axis=1) + np.arange(row)
        idx[idx == t[:, None]] = -1
        lists = [r[r >= 0].astype(np.int32) for r in idx]
        ptr = np.r_[0, np.cumsum([len(r) for r in lists])].astype(np.int64)
        return a, pg.RankQueries(n, a, t, ptr, np.concatenate(lists))

    gen = torch.Generator(device="cuda").manual_seed(1)
    anchors, plain = query_set(Q)
    _, listed = query_set(Q, args.row)
    big = query_set(args.big)[1] if args.big else None
    nq = max(Q, args.big)
    greater = torch.zeros(nq, device="cuda", dtype=torch.int32)
    equal = torch.zeros(nq, device="cuda", dtype=torch.int32)
    C = torch.empty(Q, n, device="cuda", dtype=torch.float32)
    out = {"nodes": n, "queries": Q, "reps": args.reps, "tile": list(pg.link_rank_tile()),
           "filter_row": args.row}
    for d in widths:
        H = torch.randn(n, d, device="cuda", generator=gen, dtype=torch.float32)
        A = H[torch.from_numpy(anchors.astype(np.int64)).cuda()].contiguous()

        def rank(q):
            return lambda: pg.check(lib.pgcn_link_rank(q.handle, p(H), d, d, p(greater), p(equal),
                                                       None), "link_rank")
        calls = {
            "rank": rank(plain),
            "yardstick": lambda: pg.check(lib.pgcn_gemm(Q, n, d, p(A), d, p(H), d, 1, p(C), n,
                                                        None, 0, 0, 1.0, None), "gemm"),
            "rank_filtered": rank(listed),
        }
        if big is not None:
            calls["rank_big"] = rank(big)
        res = timed(torch, calls, args.reps, args.warmup)
        flops = 2.0 * Q * n * d
        res["rank"]["TFps"] = round(flops / res["rank"]["us_median"] / 1e6, 1)
        res["yardstick"]["TFps"] = round(flops / res["yardstick"]["us_median"] / 1e6, 1)
        res["rank_over_yardstick"] = round(res["rank"]["us_median"] /
                                           res["yardstick"]["us_median"], 3)
        res["filter_share"] = round(1.0 - res["rank"]["us_median"] /
                                    res["rank_filtered"]["us_median"], 3)
        if big is not None:
            tf = 2.0 * args.big * n * d / res["rank_big"]["us_median"] / 1e6
            res["rank_big"]["TFps"] = round(tf, 1)
            res["rank_big"]["of_peak"] = round(tf / PEAK_TF, 3)
        out[f"d{d}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
