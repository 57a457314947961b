"""Epoch time of the L-layer model with and without LayerNorm, and of the ReLU / Dropout tail
fused into the LayerNorm kernel against the separate launches (DESIGN.md "LayerNorm").

    python3 tools/layernorm_bench.py [--hidden 128,128,128] [--configs plain,norm,unfused]
                                     [--epochs 10] [--rounds 5] [--warmup 5] [--edges N]
                                     [--residual 1]

One process, one data set (bench.py's reddit shape: 232,965 nodes, 602 dense features, 41
classes, seed 1), one engine per configuration, all resident together:
    plain    layer_norm 0
    norm     layer_norm 1 (ReLU, residual add and Dropout inside the LayerNorm's final write)
    unfused  layer_norm 1 built with fuse_epilogue 0 (every element-wise module a launch)
    plain0   layer_norm 0 built with fuse_epilogue 0 (what "unfused" is to be compared with)
A window is `epochs` calls of epoch_async (train_epoch + eval(2), no host sync) followed by a
sync, timed by the host clock around it; the configurations alternate window by window over
`rounds` rounds after `warmup` epochs each.  Prints one JSON line: per configuration the median,
minimum and maximum window time per epoch in ms, and the algorithmic bytes of one LayerNorm
forward / backward launch at the first hidden width (kernel times come from a kernel trace of
this script, in a run of its own).  PGCN_LIB=<another build's libpgcn.so> runs the same script
on that build (only "plain" and "plain0" exist before the option did)."""
import argparse
import importlib.util
import json
import os
import statistics
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NODES, N_FEAT, N_CLASS, EDGES = 232965, 602, 41, 57307946  # bench.py's reddit-114M

CONFIGS = {"plain": (0, 15), "norm": (1, 15), "unfused": (1, 0), "plain0": (0, 0)}


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel_bytes(n, d, dropout=True):
    """Bytes one launch has to move at N x d fp32: forward = read Z, write H, write xhat, the
    ReLU mask bytes and the dropout bits of the fused tail (+ rstd); backward = read dY, read
    xhat, write dZ (+ rstd; the column partials are a few hundred KB)."""
    pass4 = 4 * n * d
    fwd = 3 * pass4 + n * d + (n * d // 8 if dropout else 0) + 4 * n
    return {"fwd_train": fwd, "fwd_eval": 2 * pass4, "bwd": 3 * pass4 + 4 * n}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", default="128,128,128")
    ap.add_argument("--configs", default="plain,norm,unfused")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--nodes", type=int, default=N_NODES)
    ap.add_argument("--residual", type=int, default=0)
    args = ap.parse_args()
    pg = load_pkg()
    hidden = tuple(int(h) for h in args.hidden.split(","))
    names = args.configs.split(",")
    ds = pg.Dataset.synthetic(args.nodes, N_FEAT, N_CLASS, args.edges, seed=1)
    engines = {}
    for name in names:
        norm, fuse = CONFIGS[name]
        pg.lib.pgcn_debug_set(b"fuse_epilogue", fuse)  # read at engine build
        p = pg.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * (len(hidden) + 1))
        if norm:
            p.layer_norm = 1
        if args.residual:
            p.residual = 1
        g = pg.GCN(p, ds)
        for _ in range(args.warmup):
            g.epoch_async()
        g.sync()
        engines[name] = g
    pg.lib.pgcn_debug_set(b"fuse_epilogue", 15)
    times = {name: [] for name in names}
    for _ in range(args.rounds):
        for name in names:
            g = engines[name]
            t0 = time.perf_counter()
            for _ in range(args.epochs):
                g.epoch_async()
            g.sync()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.epochs)
    out = {"hidden": list(hidden), "nodes": args.nodes, "edges": args.edges,
           "epochs_per_window": args.epochs, "rounds": args.rounds, "residual": args.residual,
           "lib": os.environ.get("PGCN_LIB", "this tree"),
           "kernel_bytes": kernel_bytes(args.nodes, hidden[0])}
    for name in names:
        g, t = engines[name], times[name]
        info = {}
        for key in ("norm_layers", "fused_norm_tails", "fused_tails"):
            try:
                info[key] = g.query(key)
            except pg.PgcnError:
                pass  # a build from before the key
        out[name] = dict(ms_per_epoch_median=round(statistics.median(t), 4),
                         ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                         last_line=[float(x) for x in g.results(1)[0]], **info)
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
