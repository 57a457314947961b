"""Device time of the Hadamard-MLP decoder's kernels (DESIGN.md §3 "Link MLP decoder") through the
kernel ABI.

    python3 tools/link_mlp_bench.py [--shapes 16x16,64x64,128x128] [--reps 30] [--warmup 5]
                                    [--nodes 232965] [--pairs 1000000]

One seeded uniform pair list over --nodes nodes (reddit's count).  Per (d, h) the script times
pgcn_link_mlp_fwd, pgcn_link_mlp_bwd and two YARDSTICKS made of the project's other kernels, never
of the code under test:
    gather   pgcn_link_score_fwd on the same pairs: the two row gathers alone
    gemm     pgcn_gemm(M = E, N = h, K = d) on a dense z made untimed: the same flops of the first
             layer, plus the [E][h] array the fused kernel never writes
The expectation: fwd <= gather + gemm (that sum already omits the z write and the ReLU / w2 pass),
bwd <= 3 (gather + gemm) (it runs three products).  HIP events around each call on the null stream:
`warmup` calls, then `reps` timed ones, the calls taken in turn; the median, minimum and maximum in
microseconds, the two ratios, and the share of the fp32 MFMA peak (157.3 TFLOP/s: 256 CUs x 256
flop per clock x 2.4 GHz) that 2 E d h flops (forward; three times that backward) amount to.
Prints one JSON line.  Needs a HIP device; there is no CPU fallback."""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_FP32_MFMA = 157.3e12


def load_pkg():
    import torch  # noqa: F401  (first: one HIP runtime per process)
    spec = importlib.util.spec_from_file_location(
        "pgcn_amd", os.path.join(REPO, "parallel-gcn_amd", "__init__.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def bench_shape(pg, torch, links, n, E, d, h, reps, warmup):
    lib = pg.lib
    gen = torch.Generator(device="cuda").manual_seed(d * 1000 + h)

    def randn(*shape):
        return torch.randn(*shape, device="cuda", generator=gen, dtype=torch.float32)

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    ld_p = (h + 3) // 4 * 4
    H, P, z = randn(n, d), randn(d + 3, ld_p), randn(E, d)
    G = torch.zeros(E, 4, device="cuda")
    G[:, 0] = randn(E)
    scores, yard = torch.zeros(E, 4, device="cuda"), torch.zeros(E, 4, device="cuda")
    hid = torch.zeros(E, ld_p, device="cuda")
    dH, dP = torch.zeros(n, d, device="cuda"), torch.zeros(d + 3, ld_p, device="cuda")
    nbytes = links.mlp_workspace(d, h)
    ws = torch.zeros(nbytes // 4, device="cuda")
    calls = {
        "fwd": lambda: links.mlp_fwd(H, d, d, P, ld_p, h, scores, 4),
        "bwd": lambda: links.mlp_bwd(H, d, d, P, ld_p, h, G, 4, dH, d, dP, ld_p, ws, nbytes),
        "gather": lambda: pg.check(lib.pgcn_link_score_fwd(links.handle, p(H), d, d, p(yard), 4,
                                                           None), "link_score_fwd"),
        "gemm": lambda: pg.check(lib.pgcn_gemm(E, h, d, p(z), d, p(P), ld_p, 0, p(hid), ld_p, None,
                                               0, 0, 1.0, None), "gemm"),
    }
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
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record(null)
                f()
                e1.record(null)
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
    assert bool(torch.isfinite(scores).all()) and bool(torch.isfinite(dH).all())
    out = {"workspace_MB": round(nbytes / 1e6, 1)}
    for k, t in times.items():
        out[k] = {"us_median": round(statistics.median(t), 2), "us_min": round(min(t), 2),
                  "us_max": round(max(t), 2), "launches": launches[k]}
    yardsum = out["gather"]["us_median"] + out["gemm"]["us_median"]
    flops = 2.0 * E * d * h
    out["fwd_over_yardsticks"] = round(out["fwd"]["us_median"] / yardsum, 3)
    out["bwd_over_3_yardsticks"] = round(out["bwd"]["us_median"] / (3 * yardsum), 3)
    out["fwd_mfma_peak_share"] = round(flops / (out["fwd"]["us_median"] * 1e-6) / PEAK_FP32_MFMA, 4)
    out["bwd_mfma_peak_share"] = round(3 * flops / (out["bwd"]["us_median"] * 1e-6) /
                                       PEAK_FP32_MFMA, 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x16,64x64,128x128")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--nodes", type=int, default=232965)
    ap.add_argument("--pairs", type=int, default=1000000)
    args = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")]
    if any(d % 4 or not 4 <= d <= 128 or not 1 <= h <= 128 for d, h in shapes):
        raise SystemExit("--shapes: DxH with D a multiple of 4 in [4, 128], H in [1, 128]")
    pg = load_pkg()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("link_mlp_bench needs a HIP device")
    rng = np.random.default_rng(1)
    n, E = args.nodes, args.pairs
    src, dst = (rng.integers(0, n, E).astype(np.int32) for _ in range(2))
    links = pg.Links(n, src, dst)
    out = {"reps": args.reps, "nodes": n, "pairs": E}
    for d, h in shapes:
        out[f"d{d}h{h}"] = bench_shape(pg, torch, links, n, E, d, h, args.reps, args.warmup)
    links.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
