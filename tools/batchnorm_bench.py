"""BatchNorm's cost (DESIGN.md "BatchNorm"): the epoch with and without batch_norm, and the three
kernel ABI calls on their own at the flagship row count.

    python3 tools/batchnorm_bench.py [--hidden 128,128,128] [--configs plain,norm,unfused]
                                     [--epochs 10] [--rounds 5] [--warmup 5] [--edges N]
    python3 tools/batchnorm_bench.py --kernels [--widths 16,128] [--iters 200]

Epoch mode is tools/layernorm_bench.py's, with batch_norm in layer_norm's place: one process, one
data set (bench.py's reddit shape), one engine per configuration, all resident together,
    plain    batch_norm 0
    norm     batch_norm 1 (ReLU, residual add and Dropout inside the apply launch)
    unfused  batch_norm 1 built with fuse_epilogue 0
    plain0   batch_norm 0 built with fuse_epilogue 0
windows of `epochs` epoch_async calls ending in a sync, the configurations alternating window by
window.
--kernels: pgcn_batchnorm_fwd (training and eval) and pgcn_batchnorm_bwd at N = 232,965 per width,
`iters` calls each between two device events after a warm-up, with the bytes each call has to
move; a kernel trace of this mode gives the per-kernel times.  Prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import time

from layernorm_bench import EDGES, N_CLASS, N_FEAT, N_NODES, load_pkg

CONFIGS = {"plain": (0, 15), "norm": (1, 15), "unfused": (1, 0), "plain0": (0, 0)}


def kernel_bytes(n, d):
    """Bytes a call has to move at N x d fp32: the statistics read Z; the apply reads Z and writes
    H (+ xhat in training); the backward reads dY and xhat twice (sums, then dZ) and writes dZ.
    The tile records, partials and column vectors are a few hundred KB."""
    pass4 = 4 * n * d
    return {"stats": pass4, "fwd_train": 4 * pass4, "fwd_eval": 3 * pass4, "bwd": 5 * pass4}


def kernels(pg, widths, iters):
    import torch
    n, out = N_NODES, {}
    for d in widths:
        x = torch.randn(n, d, device="cuda") + 100.0
        y, xhat, dy = torch.empty_like(x), torch.empty_like(x), torch.randn_like(x)
        gamma, beta = torch.ones(d, device="cuda"), torch.zeros(d, device="cuda")
        stats, dgb = torch.zeros(2 * d, device="cuda"), torch.zeros(2 * d, device="cuda")
        ws = torch.zeros(max(pg.lib.pgcn_batchnorm_fwd_workspace(n, d),
                             pg.lib.pgcn_batchnorm_bwd_workspace(n, d)) // 4, device="cuda")
        p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + 4 * off)  # noqa: E731
        s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        calls = {
            "fwd_train": lambda: pg.lib.pgcn_batchnorm_fwd(
                p(x), d, p(y), d, n, d, p(gamma), p(beta), 1e-5, p(xhat), d, p(stats), p(ws), s),
            "fwd_eval": lambda: pg.lib.pgcn_batchnorm_fwd(
                p(x), d, p(y), d, n, d, p(gamma), p(beta), 1e-5, None, d, p(stats), p(ws), s),
            "bwd": lambda: pg.lib.pgcn_batchnorm_bwd(
                p(dy), d, p(xhat), d, p(stats), p(gamma), n, d, p(y), d, p(dgb), p(dgb, d),
                p(ws), s),
        }
        res = {}
        for name, call in calls.items():
            for _ in range(10):
                assert call() == pg.PGCN_OK
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                call()
            b.record()
            torch.cuda.synchronize()
            us = a.elapsed_time(b) * 1e3 / iters
            nbytes = kernel_bytes(n, d)[name]
            res[name] = dict(us_per_call=round(us, 2), bytes=nbytes,
                             tb_per_s=round(nbytes / us / 1e6, 3))
        out[str(d)] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--widths", default="16,128")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--hidden", default="128,128,128")
    ap.add_argument("--configs", default="plain,norm,unfused")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--edges", type=int, default=EDGES)
    args = ap.parse_args()
    pg = load_pkg()
    if args.kernels:
        print(json.dumps({"nodes": N_NODES, "iters": args.iters,
                          "calls": kernels(pg, [int(w) for w in args.widths.split(",")],
                                           args.iters)}))
        return
    hidden = tuple(int(h) for h in args.hidden.split(","))
    names = args.configs.split(",")
    ds = pg.Dataset.synthetic(N_NODES, N_FEAT, N_CLASS, args.edges, seed=1)
    engines = {}
    for name in names:
        norm, fuse = CONFIGS[name]
        pg.lib.pgcn_debug_set(b"fuse_epilogue", fuse)  # read at engine build
        p = pg.make_params(ds, hidden_dims=hidden, dropouts=(0.5,) * (len(hidden) + 1))
        if norm:
            p.batch_norm = 1
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
    out = {"hidden": list(hidden), "nodes": N_NODES, "edges": args.edges,
           "epochs_per_window": args.epochs, "rounds": args.rounds,
           "lib": os.environ.get("PGCN_LIB", "this tree")}
    for name in names:
        g, t = engines[name], times[name]
        out[name] = dict(ms_per_epoch_median=round(statistics.median(t), 4),
                         ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                         last_line=[float(v) for v in g.results(1)[0]])
        g.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
