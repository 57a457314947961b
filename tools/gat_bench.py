"""Device time of the graph attention kernels, beside the GraphSum on the same graph (DESIGN.md
§3 "Attention layers"): at d = 16 with one head by default, --width / --heads for others.

    python3 tools/gat_bench.py [--graphs cora,reddit] [--reps 30] [--warmup 5] [--root DIR]
                               [--heads K] [--width D]

Per graph -- cora (from tests/golden, or data/cora.* under --root) and bench.py's reddit shape
(Dataset.synthetic: 232,965 nodes, 57,307,946 undirected edges, seed 1) -- the script times
pgcn_gat_scores_mh + pgcn_gat_fwd_mh (training: alpha written, no mask), pgcn_gat_bwd_mh and
pgcn_graphsum through the kernel ABI (at one head these are the kernels behind pgcn_gat_scores /
_fwd / _bwd) with HIP events around each call on the null stream: `warmup` calls, then `reps`
timed ones, the three taken in turn; the median, minimum and maximum in microseconds.  Beside
them the bytes each call has to move and the rate that implies:
    forward   indptr + idx + u, v (K per node and K per slot's column) + P rows gathered
              (nnz x d) + Z + alpha (nnz x K) written
    backward  row pass: idx + alpha + v (nnz x K each) + P rows gathered + G, Z rows + dx
              (nnz x K) written; column pass: the transposed index (ptr, row, pos) + alpha + dx
              (read twice: dv and du) + G rows gathered + dP written; du, dv (n x K each)
    graphsum  DevGraph::algorithmic_bytes: indptr + 8 nnz + 4 N d read + 4 N d written
(gathered rows are counted once per slot: what the L2 serves is not subtracted).  Prints one
JSON line.  Needs a HIP device; there is no CPU fallback."""
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
SLOPE = 0.2


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def byte_model(n, nnz, d, K=1):
    row, per = 4 * d, 4 * K  # a row of P / G / Z; a slot's or a node's per-head scalars
    fwd = 4 * (n + 1) + 4 * nnz + per * n + per * nnz + nnz * row + n * row + per * nnz
    bwd_rows = 4 * (n + 1) + 4 * nnz + per * nnz + per * nnz + nnz * row + 2 * n * row + per * nnz
    bwd_cols = (4 * (n + 1) + 8 * nnz + per * nnz + per * nnz + nnz * row + n * row + 2 * per * n +
                per * nnz)
    gs = 4 * (n + 1) + 8 * nnz + 2 * n * row
    return {"gat_fwd": fwd, "gat_bwd": bwd_rows + bwd_cols + 2 * n * row, "graphsum": gs}


def bench_graph(pg, torch, ds, reps, warmup, D=16, K=1):
    lib = pg.lib
    n, nnz = ds.num_nodes, int(ds.graph_indptr[-1])
    h = ctypes.c_void_p()
    pg.check(lib.pgcn_graph_create(n, ds.graph_indptr.ctypes.data_as(ctypes.c_void_p),
                                   ds.graph_indices.ctypes.data_as(ctypes.c_void_p),
                                   ctypes.byref(h)), "graph_create")
    gen = torch.Generator(device="cuda").manual_seed(1)

    def randn(*shape):
        return torch.randn(*shape, device="cuda", generator=gen, dtype=torch.float32)
    P, G = randn(n, D), randn(n, D)
    a_dst, a_src = randn(D) * 0.25, randn(D) * 0.25
    u, v = torch.zeros(n * K, device="cuda"), torch.zeros(n * K, device="cuda")
    Z, dP, out = torch.zeros_like(P), torch.zeros_like(P), torch.zeros_like(P)
    alpha = torch.zeros(max(nnz, 1) * K, device="cuda")
    da = torch.zeros(2 * D, device="cuda")
    # (builds the transposed index)
    ws_bytes = lib.pgcn_gat_bwd_workspace_mh(h, D, K)
    assert ws_bytes > 0
    ws = torch.zeros(ws_bytes // 4 + 4, device="cuda")

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def fwd():
        pg.check(lib.pgcn_gat_scores_mh(p(P), D, n, D, K, p(a_dst), p(a_src), p(u), p(v), None),
                 "scores_mh")
        pg.check(lib.pgcn_gat_fwd_mh(h, p(P), D, p(u), p(v), SLOPE, p(Z), D, D, K, None, 0, 1.0,
                                     p(alpha), None), "fwd_mh")

    def bwd():
        pg.check(lib.pgcn_gat_bwd_mh(h, p(P), D, p(u), p(v), SLOPE, p(alpha), p(Z), D, p(G), D,
                                     p(a_dst), p(a_src), p(dP), D, D, K, None, 0, 1.0, p(da),
                                     p(ws), None), "bwd_mh")

    def gs():
        pg.check(lib.pgcn_graphsum(h, p(P), D, p(out), D, D, None), "graphsum")
    calls = {"gat_fwd": fwd, "gat_bwd": bwd, "graphsum": gs}
    null = torch.cuda.default_stream()
    with torch.cuda.stream(null):
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
    assert bool(torch.isfinite(Z).all()) and bool(torch.isfinite(dP).all())
    model = byte_model(n, nnz, D, K)
    res = {"nodes": n, "slots": nnz, "longest_row": int(max(ds.graph_indptr[1:] -
                                                           ds.graph_indptr[:-1]))}
    for k, t in times.items():
        med = statistics.median(t)
        res[k] = {"us_median": round(med, 2), "us_min": round(min(t), 2),
                  "us_max": round(max(t), 2), "model_bytes": model[k],
                  "model_GBps": round(model[k] / med / 1e3, 1)}
    lib.pgcn_graph_destroy(h)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="cora,reddit")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--root", default="")
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--nodes", type=int, default=N_NODES)
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--width", type=int, default=16)
    args = ap.parse_args()
    if args.width % 4 or not 4 <= args.width <= 128 or args.heads < 1:
        raise SystemExit("--width: a multiple of 4 in [4, 128]; --heads >= 1")
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gat_bench needs a HIP device")
    out = {"d": args.width, "heads": args.heads, "reps": args.reps}
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
        out[name] = bench_graph(pg, torch, ds, args.reps, args.warmup, args.width, args.heads)
        del ds
    print(json.dumps(out))


if __name__ == "__main__":
    main()
