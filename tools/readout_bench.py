"""Device time of the readout kernels (DESIGN.md §3 "Readout") through the kernel ABI.

    python3 tools/readout_bench.py [--shapes molecules,long] [--reps 30] [--warmup 5] [--width 64]
                                   [--graphs 40000] [--rows 1000000]

Two shapes:
    molecules  --graphs ranges of 10..40 rows (seeded), the batch a molecule data set makes: one
               launch, a wave per range
    long       one range of --rows rows: the pieces pass and the combine pass behind the (then
               empty) per-range launch, three launches
Per shape and mode (sum, mean, max with arg written) the script times pgcn_readout_fwd and
pgcn_readout_bwd with HIP events around each call on the null stream: `warmup` calls, then `reps`
timed ones, the calls taken in turn; the median, minimum and maximum in microseconds.  Beside them
the bytes each call must move and the rate that implies:
    forward   n d floats read + graph_ptr + G d floats written (max: + G d ints)
    backward  n d floats written + node_graph read (4 n) + G d floats read once (max: + G d ints;
              mean: + graph_ptr)
(the G rows a backward gathers per node are counted once: what the L2 serves is not added).
Prints one JSON line.  Needs a HIP device; there is no CPU fallback."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"sum": 1, "mean": 2, "max": 3}


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def byte_model(n, G, d, mode):
    row = 4 * d
    extra = G * row if mode == "max" else 0
    return {"fwd": n * row + 4 * (G + 1) + G * row + extra,
            "bwd": n * row + 4 * n + G * row + extra + (4 * (G + 1) if mode == "mean" else 0)}


def bench_shape(pg, torch, gp, D, reps, warmup):
    lib = pg.lib
    G, n = len(gp) - 1, int(gp[-1])
    lens = np.diff(gp)
    max_len = int(lens.max())
    gen = torch.Generator(device="cuda").manual_seed(1)
    X = torch.randn(n, D, device="cuda", generator=gen, dtype=torch.float32)
    Gout = torch.randn(G, D, device="cuda", generator=gen, dtype=torch.float32)
    out = torch.zeros(G, D, device="cuda", dtype=torch.float32)
    din = torch.zeros(n, D, device="cuda", dtype=torch.float32)
    arg = torch.zeros(G, D, device="cuda", dtype=torch.int32)
    dgp = torch.from_numpy(np.ascontiguousarray(gp, np.int32)).cuda()
    dng = torch.from_numpy(np.repeat(np.arange(G, dtype=np.int32), lens)).cuda()
    ws = torch.empty(max(int(lib.pgcn_readout_workspace(n)), 16), dtype=torch.uint8, device="cuda")

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    calls = {}
    for name, m in MODES.items():
        calls[name, "fwd"] = lambda m=m: pg.check(lib.pgcn_readout_fwd(
            p(X), D, p(dgp), G, n, D, m, max_len, p(out), D, p(arg), D, p(ws), None), "readout_fwd")
        calls[name, "bwd"] = lambda m=m: pg.check(lib.pgcn_readout_bwd(
            p(Gout), D, p(dgp), p(dng), p(arg), D, G, n, D, m, p(din), D, None), "readout_bwd")
    null = torch.cuda.default_stream()
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
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(null)
                f()
                e1.record(null)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(din).all())
    res = {"rows": n, "ranges": G, "longest": max_len}
    for (name, which), t in times.items():
        med = statistics.median(t)
        nbytes = byte_model(n, G, D, name)[which]
        res[f"{name}_{which}"] = {"us_median": round(med, 2), "us_min": round(min(t), 2),
                                  "us_max": round(max(t), 2), "launches": launches[name, which],
                                  "model_bytes": nbytes, "model_GBps": round(nbytes / med / 1e3, 1)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="molecules,long")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--graphs", type=int, default=40000)
    ap.add_argument("--rows", type=int, default=1000000)
    args = ap.parse_args()
    if args.width % 4 or not 4 <= args.width <= 128:
        raise SystemExit("--width: a multiple of 4 in [4, 128]")
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("readout_bench needs a HIP device")
    out = {"d": args.width, "reps": args.reps, "chunk_rows": int(pg.lib.pgcn_readout_chunk_rows())}
    for name in args.shapes.split(","):
        if name == "molecules":
            lens = np.random.default_rng(1).integers(10, 41, args.graphs)
        else:
            lens = np.array([args.rows])
        gp = np.zeros(len(lens) + 1, np.int64)
        gp[1:] = np.cumsum(lens)
        out[name] = bench_shape(pg, torch, gp, args.width, args.reps, args.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
