"""Device time of the GraphSAGE aggregators, beside the plain GraphSum on the same graph
(DESIGN.md §3 "SAGE layers"): at d = 16 by default, --width for others.

    python3 tools/sage_bench.py [--graphs cora,reddit] [--reps 30] [--warmup 5] [--root DIR]
                                [--width D]

Per graph -- cora (from tests/golden, or data/cora.* under --root) and bench.py's reddit shape
(Dataset.synthetic: 232,965 nodes, 57,307,946 undirected edges, seed 1) -- the script times
pgcn_agg_max_fwd (training: arg written, with the root term added), pgcn_agg_max_bwd,
pgcn_graphsum on pgcn_graph_create_mean's two graphs and pgcn_graphsum on pgcn_graph_create's
through the kernel ABI, with HIP events around each call on the null stream: `warmup` calls, then
`reps` timed ones, the five taken in turn; the median, minimum and maximum in microseconds.
Beside them the bytes each call has to move and the rate that implies:
    max forward   indptr + idx (4 per slot) + the neighbour rows gathered (4 d per slot) + add
                  read, out and arg written (8 d per row ... 12 d with add)
    max backward  the transposed index (ptr; row, pos: 8 per slot) + arg and G rows gathered
                  (8 d per slot) + din written
    graphsum      DevGraph::algorithmic_bytes: indptr + 8 nnz + 4 N d read + 4 N d written
(gathered rows are counted once per slot: what the L2 serves is not subtracted).  "lds": whether
the graph's d = 16 GraphSum takes the LDS ring schedule (the launches counted as "gs_ring").
Prints one JSON line.  Needs a HIP device; there is no CPU fallback."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NODES, N_CLASS, EDGES = 232965, 41, 57307946  # bench.py's reddit-114M graph


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def byte_model(n, nnz, d):
    row = 4 * d
    gs = 4 * (n + 1) + 8 * nnz + 2 * n * row
    return {"max_fwd": 4 * (n + 1) + nnz * (4 + row) + 3 * n * row,
            "max_bwd": 4 * (n + 1) + nnz * (8 + 2 * row) + n * row,
            "mean_fwd": gs, "mean_bwd": gs, "graphsum": gs}


def bench_graph(pg, torch, ds, reps, warmup, D=16):
    lib = pg.lib
    n, nnz = ds.num_nodes, int(ds.graph_indptr[-1])
    ip = ds.graph_indptr.ctypes.data_as(ctypes.c_void_p)
    idx = ds.graph_indices.ctypes.data_as(ctypes.c_void_p)
    h, mf, mb = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    pg.check(lib.pgcn_graph_create(n, ip, idx, ctypes.byref(h)), "graph_create")
    pg.check(lib.pgcn_graph_create_mean(n, ip, idx, 0, ctypes.byref(mf)), "graph_create_mean")
    pg.check(lib.pgcn_graph_create_mean(n, ip, idx, 1, ctypes.byref(mb)), "graph_create_mean")
    gen = torch.Generator(device="cuda").manual_seed(1)

    def randn(*shape):
        return torch.randn(*shape, device="cuda", generator=gen, dtype=torch.float32)
    Q, R, G = randn(n, D), randn(n, D), randn(n, D)
    out, din = torch.zeros_like(Q), torch.zeros_like(Q)
    arg = torch.zeros(n, D, device="cuda", dtype=torch.int32)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def gs(graph, src, dst):
        return lambda: pg.check(lib.pgcn_graphsum(graph, p(src), D, p(dst), D, D, None), "graphsum")
    calls = {
        "max_fwd": lambda: pg.check(lib.pgcn_agg_max_fwd(h, p(Q), D, D, p(R), D, p(out), D, p(arg),
                                                         D, None), "agg_max_fwd"),
        "max_bwd": lambda: pg.check(lib.pgcn_agg_max_bwd(h, p(G), D, p(arg), D, D, p(din), D,
                                                         None), "agg_max_bwd"),
        "mean_fwd": gs(mf, Q, out), "mean_bwd": gs(mb, G, din), "graphsum": gs(h, Q, out),
    }
    null = torch.cuda.default_stream()
    lds = {}
    with torch.cuda.stream(null):
        for k, f in calls.items():  # (the first call builds the graph's schedule / index)
            f()
            torch.cuda.synchronize()
            pg.reset_path_counts()
            f()
            lds[k] = pg.path_counts()["gs_ring"] > 0
        for _ in range(warmup):
            for f in calls.values():
                f()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(reps):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(null)
                f()
                e1.record(null)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(din).all())
    model = byte_model(n, nnz, D)
    lens = ds.graph_indptr[1:] - ds.graph_indptr[:-1]
    res = {"nodes": n, "slots": nnz, "longest_row": int(max(lens))}
    for k, t in times.items():
        med = statistics.median(t)
        res[k] = {"us_median": round(med, 2), "us_min": round(min(t), 2),
                  "us_max": round(max(t), 2), "model_bytes": model[k],
                  "model_GBps": round(model[k] / med / 1e3, 1)}
        if k in ("mean_fwd", "mean_bwd", "graphsum"):
            res[k]["lds"] = bool(lds[k])
    for g in (h, mf, mb):
        lib.pgcn_graph_destroy(g)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="cora,reddit")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default="")
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--nodes", type=int, default=N_NODES)
    ap.add_argument("--width", type=int, default=16)
    args = ap.parse_args()
    if args.width % 4 or not 4 <= args.width <= 128:
        raise SystemExit("--width: a multiple of 4 in [4, 128]")
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("sage_bench needs a HIP device")
    out = {"d": args.width, "reps": args.reps}
    for name in args.graphs.split(","):
        if name == "cora":
            if args.root:
                ds = pg.Dataset.load(args.root, "cora")
            else:
                sys.path.insert(0, os.path.join(REPO, "tests"))
                import helpers
                with tempfile.TemporaryDirectory() as root:
                    ds = pg.Dataset.load(root, helpers.materialize_dataset("cora", root))
        else:
            # (the graph alone is used: a narrow feature matrix keeps the set-up short)
            ds = pg.Dataset.synthetic(args.nodes, 16, N_CLASS, args.edges, seed=1)
        out[name] = bench_graph(pg, torch, ds, args.reps, args.warmup, args.width)
        del ds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
