"""The multi-label loss kernel's time and the multi-label epoch's (DESIGN.md "Multi-label loss").

    python3 tools/multilabel_bench.py kernel [--nodes 232965] [--classes 41] [--reps 200]
    python3 tools/multilabel_bench.py epoch  [--hidden 16] [--configs multi,single0,single]
                                             [--epochs 10] [--rounds 5] [--warmup 5] [--edges N]

kernel: pgcn_bce_fwd on N x c logits (ld = c rounded up to 4, standard normal x 3, every row
  labelled, a seeded label matrix), training and eval, `reps` launches each between two HIP
  events after 20 warm-up launches, five such windows; prints the median time per launch, the
  algorithmic bytes (read N c floats and N words of labels + N truth ints; training: write N ld
  floats) and the rate as a fraction of 6.29 TB/s, the rate a float4 copy reaches on this GPU.
epoch: bench.py's reddit shape (232,965 nodes, 602 dense features, 41 classes, seed 1), one
  engine per configuration, all resident together:
    multi    multilabel 1 with a seeded 41-class label matrix (density 0.3)
    single0  the single-label engine built with fuse_output 0 (the output Matmul on its own, as
             the multi-label engine runs it)
    single   the single-label engine as it is by default
  A window is `epochs` calls of epoch_async followed by a sync, timed by the host clock; the
  configurations alternate window by window over `rounds` rounds after `warmup` epochs each.
Prints one JSON line.  PGCN_LIB=<another build's libpgcn.so> is not supported here: the
parameter struct changed with the option (run the other tree's own tools instead)."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_NODES, N_FEAT, N_CLASS, EDGES = 232965, 602, 41, 57307946  # bench.py's reddit-114M
COPY_RATE = 6.29e12  # bytes / s of a float4 copy on the MI355X (8 TB/s spec)


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernel_bytes(n, c, ld, words):
    read = 4 * n * c + 4 * n * words + 4 * n
    return {"train": read + 4 * n * ld, "eval": read}


def bench_kernel(pg, args):
    import numpy as np
    import torch
    n, c = args.nodes, args.classes
    ld, words = (c + 3) // 4 * 4, (c + 31) // 32
    rng = np.random.default_rng(1)
    x = np.zeros((n, ld), np.float32)
    x[:, :c] = 3.0 * rng.standard_normal((n, c))
    bits = pg.pack_label_bits(rng.random((n, c)) < 0.3).view(np.int32)
    dx, db = torch.from_numpy(x).cuda(), torch.from_numpy(bits).cuda()
    dt = torch.zeros(n, dtype=torch.int32, device="cuda")
    dg = torch.empty((n, ld), dtype=torch.float32, device="cuda")
    dp = torch.empty(2 * pg.lib.pgcn_xent_blocks(n) + 2, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream()
    sp = ctypes.c_void_p(stream.cuda_stream)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())

    def launch(training):
        st = pg.lib.pgcn_bce_fwd(p(dx), ld, p(dg), p(dt), p(db), words, n, c, n * c,
                                 1 if training else 0, p(dp), sp)
        assert st == 0, st
    out = {"nodes": n, "classes": c, "ld": ld, "reps": args.reps,
           "bytes": kernel_bytes(n, c, ld, words)}
    for name, training in (("train", True), ("eval", False)):
        for _ in range(20):
            launch(training)
        torch.cuda.synchronize()
        windows = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(args.reps):
                launch(training)
            e1.record(stream)
            torch.cuda.synchronize()
            windows.append(e0.elapsed_time(e1) * 1e3 / args.reps)  # us per launch
        us = statistics.median(windows)
        rate = out["bytes"][name] / (us * 1e-6)
        out[name] = dict(us_median=round(us, 3), us_min=round(min(windows), 3),
                         us_max=round(max(windows), 3), tb_per_s=round(rate / 1e12, 3),
                         of_copy_rate=round(rate / COPY_RATE, 3))
    print(json.dumps(out))


CONFIGS = {"multi": (1, 2), "single0": (0, 0), "single": (0, 2)}  # (multilabel, fuse_output)


def bench_epoch(pg, args):
    import numpy as np
    hidden = tuple(int(h) for h in args.hidden.split(","))
    names = args.configs.split(",")
    drops = (0.5,) * (len(hidden) + 1)
    single = pg.Dataset.synthetic(args.nodes, N_FEAT, N_CLASS, args.edges, seed=1)
    multi = None
    if "multi" in names:
        multi = pg.Dataset.synthetic(args.nodes, N_FEAT, N_CLASS, args.edges, seed=1)
        multi.set_multilabel(np.random.default_rng(1).random((args.nodes, N_CLASS)) < 0.3)
    engines = {}
    for name in names:
        ml, fuse = CONFIGS[name]
        pg.lib.pgcn_debug_set(b"fuse_output", fuse)  # read at engine build
        ds = multi if ml else single
        g = pg.GCN(pg.make_params(ds, hidden_dims=hidden, dropouts=drops, multilabel=bool(ml)), ds)
        for _ in range(args.warmup):
            g.epoch_async()
        g.sync()
        engines[name] = g
    pg.lib.pgcn_debug_set(b"fuse_output", 2)
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
           "epochs_per_window": args.epochs, "rounds": args.rounds}
    for name in names:
        g, t = engines[name], times[name]
        out[name] = dict(ms_per_epoch_median=round(statistics.median(t), 4),
                         ms_min=round(min(t), 4), ms_max=round(max(t), 4),
                         multilabel=g.query("multilabel"),
                         last_line=[float(x) for x in g.results(1)[0]])
        g.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "epoch"))
    ap.add_argument("--nodes", type=int, default=N_NODES)
    ap.add_argument("--classes", type=int, default=N_CLASS)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--hidden", default="16")
    ap.add_argument("--configs", default="multi,single0,single")
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--edges", type=int, default=EDGES)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("multilabel_bench needs a HIP device: nothing is measured without one")
    pg = load_pkg()
    (bench_kernel if args.what == "kernel" else bench_epoch)(pg, args)


if __name__ == "__main__":
    main()
