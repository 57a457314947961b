"""Device time of GraphSAGE neighbour sampling, beside the full-neighbourhood mean it replaces in
training (DESIGN.md §3 "Neighbour sampling"): at d = 128 and d = 16 (bench.py's hidden width),
fanout 10 and 25.

    python3 tools/nbr_bench.py [--reps 20] [--warmup 3] [--widths 128,16] [--fanouts 10,25]
                               [--nodes N --edges E]

On bench.py's reddit shape (Dataset.synthetic: 232,965 nodes, 57,307,946 undirected edges, seed 1)
the script times, through the kernel ABI with HIP events around each call on the null stream,
    draw       pgcn_nbr_sample_draw: the draw and the transposed index behind it (a new round
               every call)
    nbr_fwd    pgcn_nbr_agg_fwd, mean, with the root term added
    nbr_bwd    pgcn_nbr_agg_bwd, mean
    full_fwd   pgcn_graphsum on pgcn_graph_create_mean's forward graph (what the engine runs)
    full_bwd   pgcn_graphsum on its transposed graph
`warmup` calls, then `reps` timed ones, taken in turn; the median, minimum and maximum in
microseconds, and ratio = (draw + nbr_fwd + nbr_bwd) / (full_fwd + full_bwd) of the medians: one
layer's aggregation cost per training epoch, sampled over full.  Prints one JSON line.  Needs a
HIP device; there is no CPU fallback."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NODES, N_CLASS, EDGES = 232965, 41, 57307946  # bench.py's reddit-114M graph


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def time_calls(torch, calls, reps, warmup):
    null = torch.cuda.default_stream()
    times = {k: [] for k in calls}
    with torch.cuda.stream(null):
        for _ in range(warmup):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        for _ in range(reps):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(null)
                f()
                e1.record(null)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
    return {k: {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2),
                "us_max": round(max(t), 2)} for k, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--widths", default="128,16")
    ap.add_argument("--fanouts", default="10,25")
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--nodes", type=int, default=N_NODES)
    args = ap.parse_args()
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nbr_bench needs a HIP device")
    lib = pg.lib
    # (the graph alone is used: a narrow feature matrix keeps the set-up short)
    ds = pg.Dataset.synthetic(args.nodes, 16, N_CLASS, args.edges, seed=1)
    n, nnz = ds.num_nodes, int(ds.graph_indptr[-1])
    ip = ds.graph_indptr.ctypes.data_as(ctypes.c_void_p)
    idx = ds.graph_indices.ctypes.data_as(ctypes.c_void_p)
    h, mf, mb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    pg.check(lib.pgcn_graph_create(n, ip, idx, ctypes.byref(h)), "graph_create")
    pg.check(lib.pgcn_graph_create_mean(n, ip, idx, 0, ctypes.byref(mf)), "graph_create_mean")
    pg.check(lib.pgcn_graph_create_mean(n, ip, idx, 1, ctypes.byref(mb)), "graph_create_mean")
    gen = torch.Generator(device="cuda").manual_seed(1)
    out = {"nodes": n, "slots": nnz, "reps": args.reps}
    for D in (int(w) for w in args.widths.split(",")):
        Q, R, G = (torch.randn(n, D, device="cuda", generator=gen) for _ in range(3))
        Z, dQ = torch.zeros_like(Q), torch.zeros_like(Q)

        def p(t):
            return ctypes.c_void_p(t.data_ptr())

        def gs(graph, src, dst):
            return lambda: pg.check(lib.pgcn_graphsum(graph, p(src), D, p(dst), D, D, None),
                                    "graphsum")
        res = time_calls(torch, {"full_fwd": gs(mf, Q, Z), "full_bwd": gs(mb, G, dQ)}, args.reps,
                         args.warmup + 1)  # (the first call builds the graph's schedule)
        full = res["full_fwd"]["us_median"] + res["full_bwd"]["us_median"]
        for K in (int(k) for k in args.fanouts.split(",")):
            s = pg.NbrSample(h, n, K)
            rounds = iter(range(1 << 30))
            calls = {
                "draw": lambda: s.draw(1, next(rounds)),
                "nbr_fwd": lambda: pg.check(s.agg_fwd(1, Q, D, D, R, D, Z, D), "nbr_agg_fwd"),
                "nbr_bwd": lambda: pg.check(s.agg_bwd(1, G, D, None, 0, D, dQ, D), "nbr_agg_bwd"),
            }
            r = time_calls(torch, calls, args.reps, args.warmup)
            r["kept_slots"] = int(torch.from_numpy(s.copy()[3])[-1])
            r["ratio"] = round(sum(r[k]["us_median"] for k in calls) / full, 4)
            res[f"fanout_{K}"] = r
            s.close()
        assert bool(torch.isfinite(Z).all()) and bool(torch.isfinite(dQ).all())
        out[f"d_{D}"] = res
    for g in (h, mf, mb):
        lib.pgcn_graph_destroy(g)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
