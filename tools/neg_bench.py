"""Device time of per-epoch negative sampling (DESIGN.md §3 "Negative sampling") through the
kernel ABI: the draw (pgcn_neg_sample) and the incidence rebuild (pgcn_links_rebuild).

    python3 tools/neg_bench.py [--lists uniform,chunglu] [--reps 30] [--warmup 5]
                               [--nodes 232965] [--pairs 1000000] [--host-reps 3]

--pairs positive pairs over --nodes nodes (reddit's count), seeded, with the anchors (src) uniform
or drawn with probability proportional to (rank + 1)^-0.6 (Chung-Lu; dst likewise).  The graph is
the positives themselves; a node's exclusion row is itself and the dst of its positives.  The pair
list of the rebuildable handle is the positives followed by as many drawn pairs (ratio 1), all
selected: 4 x --pairs incidence entries.  Timed, with HIP events on the null stream, `warmup`
calls then `reps` timed ones, the calls taken in turn (median, minimum, maximum in microseconds):
    draw       pgcn_neg_sample of --pairs anchors, the round changing every call
    rebuild    pgcn_links_set_dst_range of the drawn half + pgcn_links_rebuild, every launch of it
    stages     the same rebuild with an event behind every stage (pgcn_debug_links_rebuild_times):
               per radix pass the histogram, the scan and the scatter, then the index launches and
               the segment records; the median of `reps` runs per stage
    bwd64      the YARDSTICK on the device: one pgcn_link_score_bwd at d = 64 on the same handle,
               the work a rebuild sits beside each epoch
and the YARDSTICK on the host, the route without these kernels: sample_negative_pairs +
pgcn_links_create on the new arrays, wall clock of --host-reps runs (host work, so no events).
Prints one JSON line.  Needs a HIP device; there is no CPU fallback."""
import argparse
import ctypes
import json
import statistics
import time
import types

import numpy as np

from link_bench import load_pkg, pair_list


def exclusion(n, src, dst):
    """(ptr int64 [n + 1], idx): per node the ascending union of itself and its positives' dst."""
    key = np.unique(np.concatenate([src.astype(np.int64) * n + dst,
                                    np.arange(n, dtype=np.int64) * (n + 1)]))
    rows = key // n
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return ptr, (key % n).astype(np.int32)


def stats(t):
    return {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2),
            "us_max": round(max(t), 2)}


def bench_list(pg, torch, n, src, dst, args):
    lib, P = pg.lib, len(src)
    ptr, idx = exclusion(n, src, dst)
    sampler = pg.NegSampler(n, ptr, idx)
    all_src = np.concatenate([src, src])
    links = pg.Links(n, all_src, np.concatenate([dst, dst]), dynamic=True)
    d_src = torch.from_numpy(src).cuda()
    d_new = torch.zeros(P, device="cuda", dtype=torch.int32)
    gen = torch.Generator(device="cuda").manual_seed(1)
    H = torch.randn(n, 64, device="cuda", generator=gen, dtype=torch.float32)
    G = torch.randn(2 * P, 4, device="cuda", generator=gen, dtype=torch.float32)
    dH = torch.zeros(n, 64, device="cuda", dtype=torch.float32)
    rnd = [0]

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def draw():
        rnd[0] += 1
        sampler.sample(d_src, P, 1, rnd[0], d_new)

    def rebuild():
        links.set_dst_range(P, d_new, P)
        links.rebuild()

    def bwd64():
        pg.check(lib.pgcn_link_score_bwd(links.handle, p(H), 64, 64, p(G), 4, p(dH), 64, None),
                 "link_score_bwd")
    calls = {"draw": draw, "rebuild": rebuild, "bwd64": bwd64}
    null = torch.cuda.default_stream()
    launches = {}
    with torch.cuda.stream(null):
        for k, f in calls.items():
            pg.reset_path_counts()
            f()
            launches[k] = pg.path_counts()["launches"]
        for _ in range(args.warmup):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.reps):
            for k, f in calls.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(null)
                f()
                e1.record(null)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
    stage_us = np.array([links.rebuild_times() for _ in range(args.reps)])
    # what was timed is the index of the arrays the device holds
    new = np.concatenate([dst, d_new.cpu().numpy()])
    assert all((a == b).all() for a, b in zip(links.incidence(),
                                              pg.links_incidence(n, all_src, new)))
    lens = np.diff(links.incidence()[0])
    res = {"nodes": n, "positives": P, "entries": int(lens.sum()), "longest": int(lens.max()),
           "long_nodes": int((lens > lib.pgcn_link_segment_slots()).sum()),
           "passes": (max(n - 1, 1).bit_length() + 7) // 8}
    for k, t in times.items():
        res[k] = dict(stats(t), launches=launches[k])
    names = [f"pass{p}_{k}" for p in range(res["passes"]) for k in ("hist", "scan", "scatter")]
    names += ["index", "segments"]
    res["stages"] = {k: stats([float(x) for x in stage_us[:, i]])
                     for i, k in enumerate(names[:stage_us.shape[1]])}
    ds = types.SimpleNamespace(num_nodes=n, graph_indptr=(ptr - np.arange(n + 1)).astype(np.int64),
                               graph_indices=idx[idx != np.repeat(np.arange(n), np.diff(ptr))])
    host = []
    for r in range(args.host_reps):
        t0 = time.perf_counter()
        _, neg = pg.sample_negative_pairs(ds, src, 1, r)
        pg.Links(n, all_src, np.concatenate([dst, neg])).close()
        host.append((time.perf_counter() - t0) * 1e6)
    res["host_route"] = stats(host)
    both = [a + b for a, b in zip(times["draw"], times["rebuild"])]
    res["host_over_device"] = {"median": round(statistics.median(host) / statistics.median(both), 1),
                               "min": round(min(host) / max(both), 1),
                               "max": round(max(host) / min(both), 1)}
    res["rebuild_over_bwd64"] = {
        "median": round(res["rebuild"]["us_median"] / res["bwd64"]["us_median"], 3),
        "min": round(res["rebuild"]["us_min"] / res["bwd64"]["us_max"], 3),
        "max": round(res["rebuild"]["us_max"] / res["bwd64"]["us_min"], 3)}
    links.close()
    sampler.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", default="uniform,chunglu")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--pairs", type=int, default=1000000)
    ap.add_argument("--host-reps", type=int, default=3)
    args = ap.parse_args()
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("neg_bench needs a HIP device")
    out = {"reps": args.reps, "sort_tile": pg.links_sort_tile()}
    for name in args.lists.split(","):
        src, dst = pair_list(name, args.nodes, args.pairs)
        out[name] = bench_list(pg, torch, args.nodes, src, dst, args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
