"""Epoch time of the L-layer model with and without residual connections, and of the fused
residual add against the separate launches it replaces (DESIGN.md "Residual layers").

    python3 tools/residual_bench.py [--hidden 128,128,128] [--configs plain,residual,unfused]
                                    [--epochs 10] [--rounds 5] [--warmup 5] [--edges N]

One process, one data set (bench.py's reddit shape: 232,965 nodes, 602 dense features, 41
classes, seed 1), one engine per configuration, all resident together:
    plain     residual 0
    residual  residual 1 (the add inside the GraphSum's final write)
    unfused   residual 1 built with fuse_epilogue 0 (ReLU, add and Dropout as launches)
    plain0    residual 0 built with fuse_epilogue 0 (what "unfused" is to be compared with)
A window is `epochs` calls of epoch_async (train_epoch + eval(2), no host sync) followed by a
sync, timed by the host clock around it; the configurations alternate window by window over
`rounds` rounds after `warmup` epochs each.  Prints one JSON line: per configuration the median,
minimum and maximum window time per epoch in ms.  PGCN_LIB=<another build's libpgcn.so> runs
the same script on that build (only "plain" exists before this option did)."""
import argparse
import importlib.util
import json
import os
import statistics
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NODES, N_FEAT, N_CLASS, EDGES = 232965, 602, 41, 57307946  # bench.py's reddit-114M

CONFIGS = {"plain": (0, 15), "residual": (1, 15), "unfused": (1, 0), "plain0": (0, 0)}


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", default="128,128,128")
    ap.add_argument("--configs", default="plain,residual,unfused")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--edges", type=int, default=EDGES)
    ap.add_argument("--nodes", type=int, default=N_NODES)
    args = ap.parse_args()
    pg = load_pkg()
    hidden = tuple(int(h) for h in args.hidden.split(","))
    names = args.configs.split(",")
    ds = pg.Dataset.synthetic(args.nodes, N_FEAT, N_CLASS, args.edges, seed=1)
    engines = {}
    for name in names:
        residual, fuse = CONFIGS[name]
        pg.lib.pgcn_debug_set(b"fuse_epilogue", fuse)  # read at engine build
        p = pg.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * (len(hidden) + 1))
        if residual:
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
           "epochs_per_window": args.epochs, "rounds": args.rounds,
           "lib": os.environ.get("PGCN_LIB", "this tree")}
    for name in names:
        g, t = engines[name], times[name]
        info = {}
        for key in ("residual_layers", "fused_residuals", "fused_tails"):
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
