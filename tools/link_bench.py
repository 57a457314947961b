"""Device time of the pair-score kernels (DESIGN.md §3 "Link prediction") through the kernel ABI.

    python3 tools/link_bench.py [--lists uniform,chunglu] [--widths 16,64] [--reps 30]
                                [--warmup 5] [--nodes 232965] [--pairs 1000000]

Two pair lists over --nodes nodes (reddit's count), --pairs pairs each, seeded:
    uniform   both endpoints uniform: every incidence list is short, the backward is one launch
    chunglu   both endpoints drawn with probability proportional to (rank + 1)^-0.6 (a Chung-Lu
              graph with power-law expected degrees): the first nodes' lists exceed
              pgcn_link_segment_slots() and go through the segment pass, two launches
Per list and width the script times pgcn_link_score_fwd, pgcn_link_score_bwd and the YARDSTICK of
the backward: pgcn_graphsum on a graph made with pgcn_graph_create_values from the same incidence
index (row i = node i's entries, columns = the other endpoints) with the coefficients G[e][0] baked
into its values, which takes the per-edge gather kernels -- the same rows moved, the same sums.
HIP events around each call on the null stream: `warmup` calls, then `reps` timed ones, the calls
taken in turn; the median, minimum and maximum in microseconds.  Beside them the bytes each call
must move and the rate that implies:
    forward    2 E rows of 4 d bytes gathered + 8 E index bytes + 16 E score bytes written
    backward   S = 2 E entries: S rows of 4 d bytes gathered + 8 S (pair, other) + 4 S (G[e]) +
               4 (n + 1) ptr + n rows of 4 d bytes written
    yardstick  the same without the 4 S pair indices (its values array stands for G)
(gathered rows are counted per entry: what the caches serve twice is not subtracted).
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


def pair_list(kind, n, E, seed=1):
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        return (rng.integers(0, n, E).astype(np.int32), rng.integers(0, n, E).astype(np.int32))
    w = (np.arange(n) + 1.0) ** -0.6
    cdf = np.cumsum(w / w.sum())

    def draw():
        return np.minimum(np.searchsorted(cdf, rng.random(E)), n - 1).astype(np.int32)
    return draw(), draw()


def byte_model(n, E, d):
    S, row = 2 * E, 4 * d
    bwd = S * row + 8 * S + 4 * S + 4 * (n + 1) + n * row
    return {"fwd": 2 * E * row + 8 * E + 16 * E, "bwd": bwd, "yardstick": bwd - 4 * S}


def bench_list(pg, torch, n, src, dst, widths, reps, warmup):
    lib = pg.lib
    E = len(src)
    links = pg.Links(n, src, dst)
    ptr, pair, other = pg.links_incidence(n, src, dst)
    gen = torch.Generator(device="cuda").manual_seed(1)
    G = torch.zeros(E, 4, device="cuda", dtype=torch.float32)
    G[:, 0] = torch.randn(E, device="cuda", generator=gen, dtype=torch.float32)
    vals = np.ascontiguousarray(G[:, 0].cpu().numpy()[pair], np.float32)
    yard = ctypes.c_void_p()
    pg.check(lib.pgcn_graph_create_values(n, pg._ptr(ptr), pg._ptr(other), pg._ptr(vals),
                                          ctypes.byref(yard)), "graph_create_values")
    scores = torch.zeros(E, 4, device="cuda", dtype=torch.float32)
    lens = np.diff(ptr)
    res = {"nodes": n, "pairs": E, "entries": int(ptr[-1]), "longest": int(lens.max()),
           "long_nodes": int((lens > lib.pgcn_link_segment_slots()).sum())}

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    null = torch.cuda.default_stream()
    for d in widths:
        H = torch.randn(n, d, device="cuda", generator=gen, dtype=torch.float32)
        dH = torch.zeros(n, d, device="cuda", dtype=torch.float32)
        dY = torch.zeros(n, d, device="cuda", dtype=torch.float32)
        calls = {
            "fwd": lambda: pg.check(lib.pgcn_link_score_fwd(links.handle, p(H), d, d, p(scores), 4,
                                                            None), "link_score_fwd"),
            "bwd": lambda: pg.check(lib.pgcn_link_score_bwd(links.handle, p(H), d, d, p(G), 4,
                                                            p(dH), d, None), "link_score_bwd"),
            "yardstick": lambda: pg.check(lib.pgcn_graphsum(yard, p(H), d, p(dY), d, d, None),
                                          "graphsum"),
        }
        launches = {}
        with torch.cuda.stream(null):
            for k, f in calls.items():
                pg.reset_path_counts()
                f()
                launches[k] = pg.path_counts()["launches"]
            for _ in range(warmup):
                for f in calls.values():
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in calls}
            for _ in range(reps):
                for k, f in calls.items():
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record(null)
                    f()
                    e1.record(null)
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3)
        # the two backwards compute the same sums in another order
        scale = float(dY.abs().max())
        assert bool(torch.isfinite(dH).all()) and float((dH - dY).abs().max()) <= 1e-4 * scale
        model = byte_model(n, E, d)
        out = {}
        for k, t in times.items():
            med = statistics.median(t)
            out[k] = {"us_median": round(med, 2), "us_min": round(min(t), 2),
                      "us_max": round(max(t), 2), "launches": launches[k],
                      "model_bytes": model[k], "model_GBps": round(model[k] / med / 1e3, 1)}
        out["bwd_over_yardstick"] = round(out["bwd"]["us_median"] /
                                          out["yardstick"]["us_median"], 3)
        res[f"d{d}"] = out
    lib.pgcn_graph_destroy(yard)
    links.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", default="uniform,chunglu")
    ap.add_argument("--widths", default="16,64")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--pairs", type=int, default=1000000)
    args = ap.parse_args()
    widths = [int(w) for w in args.widths.split(",")]
    if any(w % 4 or not 4 <= w <= 128 for w in widths):
        raise SystemExit("--widths: multiples of 4 in [4, 128]")
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("link_bench needs a HIP device")
    out = {"reps": args.reps, "segment_slots": int(pg.lib.pgcn_link_segment_slots())}
    for name in args.lists.split(","):
        src, dst = pair_list(name, args.nodes, args.pairs)
        out[name] = bench_list(pg, torch, args.nodes, src, dst, widths, args.reps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
