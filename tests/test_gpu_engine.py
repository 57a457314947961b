"""GPU parity of the whole training epoch (the hot path) against the reference's outputs.

Tolerances (north star: "within 1e-4 relative on loss/logits, integer indexing bit-exact"):
  * loss values: |ours - ref| <= 1e-4 * |ref| per epoch line, all 100 epochs;
  * accuracies: a count difference of at most 2 labelled rows per split (near-ties of logits
    may flip a row when fp32 summation orders differ; the large-graph tests count the oracle's
    near-tied rows instead, tests/test_gpu_parity_large.py);
  * integer/bit work bit-exact: dropout masks (compared through the dropped input and the
    hidden activations' zero pattern), the parsed CSR, labels/splits;
  * tensors after epoch 1: rtol 1e-4 / atol 1e-6 (SpMM over sparse X is bit-exact).
"""
import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

DATASETS = ["cora", "citeseer", "pubmed_synth"]
VAR_NAMES = ["input", "l1_var1", "W1", "l1_var2", "l2_var1", "W2", "output"]


def _counts(ds):
    lab, sp = np.asarray(ds.label), np.asarray(ds.split)
    return {s: int(((sp == s) & (lab >= 0)).sum()) for s in (1, 2, 3)}


def _run_all(loaded, pgcn, reassoc_small=0):
    """The engine with reassociate_last requested, output layer over every row.  With
    reassoc_small 0 (hidden 16 above the class count of cora (7), citeseer (6) and pubmed (3))
    the output layer keeps the reference's module order Â (H W2), so every intermediate is
    comparable tensor by tensor; with reassoc_small 1 (the default: graphs under 65,536 nodes
    run the output layer as (Â H) W2, its Matmul inside the loss kernel) the epoch lines,
    eval logits and weights are compared (test_epoch_lines, test_final_weights); the
    reassociated order is also covered by test_reassociated_* below and by
    tests/test_gpu_parity_large.py."""
    out = {}
    for name in DATASETS:
        ds = loaded[name]
        with helpers.knobs(pgcn, reassoc_small=reassoc_small):
            g = pgcn.GCN(pgcn.make_params(ds), ds)
        assert g.query("reassociated") == reassoc_small
        e1 = {}
        lines = []
        for e in range(100):
            tl, ta = g.train_epoch()
            if e == 0:
                e1["vars"] = [g.get_var(i) for i in range(7)]
                e1["grads"] = [g.get_var(i, 1) for i in range(7)]
            vl, va = g.eval(2)
            if e == 0:
                e1["eval_logits"] = g.get_var(6)
            lines.append([tl, ta, vl, va])
        test = g.eval(3)
        out[name] = dict(lines=np.array(lines, np.float32), e1=e1, test=test,
                         counts=_counts(ds), w1=g.get_var(2), w2=g.get_var(5))
        g.close()
    return out


@pytest.fixture(scope="module")
def engine_runs(loaded, pgcn):
    return _run_all(loaded, pgcn, reassoc_small=0)


@pytest.fixture(scope="module")
def engine_runs_small(loaded, pgcn):
    return _run_all(loaded, pgcn, reassoc_small=1)


@pytest.fixture(params=["reference_order", "reassociated"])
def any_runs(request):
    return request.getfixturevalue("engine_runs" if request.param == "reference_order"
                                   else "engine_runs_small")


@pytest.fixture(scope="module")
def oracle_ties(loaded):
    """Per dataset, the oracle's near-tied rows (within 1e-4 of a tie, the north star's logit
    tolerance: after 100 Adam epochs the logits carry that much drift) of every pass of the
    100 epochs and of eval(3): the accuracy tolerance of test_epoch_lines (the oracle is
    bit-exact with the reference build, tests/test_oracle_pinned.py)."""
    out = {}
    for name in DATASETS:
        ds = loaded[name]
        ref = helpers.OracleGCN(helpers.ds_dict(ds))
        ties = [ref.epoch_with_ties(ds.label, ds.split, ds.output_dim, tol=1e-4)[1]
                for _ in range(100)]
        out[name] = (ties, ref.eval_with_ties(3, ds.label, ds.split, ds.output_dim, tol=1e-4)[1])
    return out


@pytest.mark.parametrize("name", DATASETS)
def test_epoch_lines(any_runs, oracle_ties, name):
    runs = any_runs
    gold = helpers.golden(name)["epoch_lines"].reshape(-1, 4)
    ours = runs[name]["lines"]
    cnt = runs[name]["counts"]
    for col in (0, 2):  # losses
        rel = np.abs(ours[:, col] - gold[:, col]) / np.abs(gold[:, col])
        assert rel.max() <= 1e-4, f"{name} loss col {col}: max rel {rel.max():.3g}"
    ties, test_ties = oracle_ties[name]
    for col, split in ((1, 1), (3, 2)):  # accuracies: only near-tied rows may differ
        dcount = np.abs(ours[:, col] - gold[:, col]) * cnt[split]
        allowed = np.array([t[split] for t in ties], np.float64)
        bad = np.nonzero(dcount > allowed + 1e-3)[0]
        assert len(bad) == 0, (f"{name} acc col {col}: epochs {bad + 1} differ by "
                               f"{dcount[bad]} rows, near-ties {allowed[bad]}")
    tl, ta = runs[name]["test"]
    gt = helpers.golden(name)["test_scalars"]
    assert abs(tl - gt[0]) <= 1e-4 * abs(gt[0])
    assert abs(ta - gt[1]) * cnt[3] <= test_ties + 1e-3


@pytest.mark.parametrize("split_rows", [0, 1])
def test_reassociated_output_layer_cora(loaded, pgcn, split_rows):
    """hidden 4 < 7 classes: the output layer runs as (Â H) W2 (cora's pattern is symmetric),
    with the output-layer row restriction on or off, against the oracle's reference order
    Â (H W2) at 1e-4; full logits after eval match the oracle's when the restriction is off,
    and get_var refuses them when it is on (their other rows are stale)."""
    ds = loaded["cora"]
    with helpers.knobs(pgcn, split_rows=split_rows):
        g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=(4,)), ds)
        assert g.query("graph_symmetric") == 1 and g.query("reassociated") == 1
        ref = helpers.OracleGCN(helpers.ds_dict(ds), hidden_dims=(4,))
        cnt = _counts(ds)
        for e in range(30):
            ours = g.train_epoch() + g.eval(2)
            want = ref.train_epoch() + ref.eval(2)
            helpers.assert_line_close(ours, want, cnt, what=f"epoch {e}")
        if split_rows:
            with pytest.raises(pgcn.PgcnError):
                g.get_var(6)
        else:
            np.testing.assert_allclose(g.get_var(6), ref.var(6), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(g.get_var(5), ref.var(5), rtol=1e-3, atol=1e-6)
        g.close()


def test_reassociation_off_for_directed_pattern(loaded, pgcn):
    """A non-symmetric pattern (one edge redirected, row lengths kept): (Â H) W2 would give the
    W2 gradient H^T Â^T dOut instead of the reference's H^T Â dOut (hpdga module.cpp:98-111),
    so the engine keeps the reference order; its lines match the oracle on the same arrays."""
    ds = pgcn.Dataset.synthetic(3000, 24, 9, 6000, 17)
    ip = ds.graph_indptr
    row = int(np.argmax(np.diff(ip)))  # a row with several neighbours
    ds.graph_indices[ip[row] + 1] = (ds.graph_indices[ip[row] + 1] + 7) % ds.num_nodes
    g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=(4,)), ds)
    assert g.query("graph_symmetric") == 0 and g.query("reassociated") == 0
    ref = helpers.OracleGCN(helpers.ds_dict(ds), hidden_dims=(4,))
    cnt = _counts(ds)
    for e in range(10):
        helpers.assert_line_close(g.train_epoch() + g.eval(2), ref.train_epoch() + ref.eval(2),
                                  cnt, what=f"epoch {e}")
    g.close()


@pytest.mark.parametrize("name", ["cora", "citeseer"])
def test_epoch1_tensors(engine_runs, name):
    gold = helpers.golden(name)
    e1 = engine_runs[name]["e1"]
    # dropped input: dropout masks are bit-exact and X is scaled exactly
    np.testing.assert_array_equal(e1["vars"][0], gold["e1_input"])
    # sparse-X SpMM walks the CSR in order with separate mul/add: bit-exact
    np.testing.assert_array_equal(e1["vars"][1], gold["e1_l1_var1"])
    for i, n in enumerate(VAR_NAMES):
        if i == 0:
            continue
        if n in ("W1", "W2"):
            np.testing.assert_allclose(e1["grads"][i], gold[f"e1_{n}_grad"], rtol=1e-4, atol=1e-7,
                                       err_msg=n + " grad")
            np.testing.assert_allclose(e1["vars"][i], gold[f"e1_{n}_after_step"], rtol=1e-4,
                                       atol=1e-7, err_msg=n)
            continue
        np.testing.assert_allclose(e1["vars"][i], gold[f"e1_{n}"], rtol=1e-4, atol=1e-6, err_msg=n)
        np.testing.assert_allclose(e1["grads"][i], gold[f"e1_{n}_grad"], rtol=1e-4, atol=1e-7,
                                   err_msg=n + " grad")
    # hidden dropout mask: zero pattern of the dropped ReLU output matches exactly
    ours_zero = e1["vars"][3] == 0
    gold_zero = gold["e1_l1_var2"] == 0
    assert (ours_zero != gold_zero).sum() <= 2  # a value exactly at 0 may flip ReLU
    np.testing.assert_allclose(e1["eval_logits"], gold["e1_eval_logits"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("name", ["cora", "citeseer"])
def test_epoch1_tensors_reassociated(engine_runs_small, name):
    """The default small-graph engine (output layer as (Â H) W2): the tensors its module
    order shares with the reference's -- the dropped input and the first layer bit-exact, the
    hidden activations, both weights and their gradients, the output logits and eval's
    logits at 1e-4 (variable 4 is Â H here, not H W2)."""
    gold = helpers.golden(name)
    e1 = engine_runs_small[name]["e1"]
    np.testing.assert_array_equal(e1["vars"][0], gold["e1_input"])
    np.testing.assert_array_equal(e1["vars"][1], gold["e1_l1_var1"])
    for i, n in enumerate(VAR_NAMES):
        if n in ("W1", "W2"):
            np.testing.assert_allclose(e1["grads"][i], gold[f"e1_{n}_grad"], rtol=1e-4, atol=1e-7,
                                       err_msg=n + " grad")
            np.testing.assert_allclose(e1["vars"][i], gold[f"e1_{n}_after_step"], rtol=1e-4,
                                       atol=1e-7, err_msg=n)
        elif n in ("l1_var2", "output"):
            np.testing.assert_allclose(e1["vars"][i], gold[f"e1_{n}"], rtol=1e-4, atol=1e-6,
                                       err_msg=n)
    np.testing.assert_allclose(e1["eval_logits"], gold["e1_eval_logits"], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("name", DATASETS)
def test_final_weights(any_runs, name):
    """Weights after 100 Adam epochs against the reference build's.  Adam's update is
    m/(sqrt(v)+eps): a gradient entry near zero flips the sign of its few-ulp steps, so single
    entries may drift by a few step sizes (lr = 0.01); the bulk must stay near fp32 noise
    (pubmed_synth measured: median 1.1e-4 of max|W|, 97.2 % of entries within 1e-3; its 500
    TF-IDF features make many W1 rows see near-zero gradients)."""
    gold = helpers.golden(name)
    for ours, ref in ((any_runs[name]["w1"], gold["final_W1"]),
                      (any_runs[name]["w2"], gold["final_W2"])):
        scale = np.abs(ref).max()
        err = np.abs(ours - ref)
        assert err.max() <= 5e-3 * scale, err.max() / scale
        assert np.median(err) <= 2.5e-4 * scale, np.median(err) / scale
        assert np.mean(err <= 1e-3 * scale) >= 0.95, np.mean(err <= 1e-3 * scale)


@pytest.mark.parametrize("name", ["cora", "pubmed_synth"])
def test_edge_cut_engine_world1(loaded, pgcn, name):
    """The multi-GPU engine (partitioned graph, RCCL reduce-scatter / all-reduce) with a
    one-rank communicator: the same epoch lines as the reference."""
    ds = loaded[name]
    g = pgcn.GCN(pgcn.make_params(ds), ds, device=0, rank=0, world=1,
                 unique_id=pgcn.comm_unique_id())
    assert g.node_range() == (0, ds.num_nodes)
    gold = helpers.golden(name)["epoch_lines"].reshape(-1, 4)
    for e in range(20):
        tl, ta = g.train_epoch()
        vl, va = g.eval(2)
        for ours, ref in ((tl, gold[e, 0]), (vl, gold[e, 2])):
            assert abs(ours - ref) <= 1e-4 * abs(ref), (e, ours, ref)
    g.close()


def test_edge_cut_world1_hidden80_matches_single(loaded, pgcn):
    """Edge-cut engine at world 1 with a hidden width the plain GraphSum has no fused-tail
    kernel for (80 = 20 float4s): its ReLU / Dropout run as modules, as on the one-GPU
    engine (the tail was handed to a combine that cannot take it)."""
    ds = loaded["cora"]
    p = pgcn.make_params(ds, hidden_dims=(80,), dropouts=(0.5, 0.5))
    single = pgcn.GCN(p, ds, device=0)
    cut = pgcn.GCN(p, ds, device=0, rank=0, world=1, unique_id=pgcn.comm_unique_id())
    for e in range(3):
        a = single.train_epoch() + single.eval(2)
        b = cut.train_epoch() + cut.eval(2)
        for k in (0, 2):
            assert abs(a[k] - b[k]) <= 1e-4 * abs(a[k]), (e, k, a, b)
    single.close()
    cut.close()


def test_edge_cut_world1_large_matches_single(pgcn):
    """Edge-cut engine at world 1 on a graph whose feature table takes the LDS GraphSum path:
    the chunked partial sums + reduce-scatters (two row chunks, comm stream) give the same
    losses as the single-GPU engine."""
    ds = pgcn.Dataset.synthetic(150000, 64, 8, 6000000, 3)
    p = pgcn.make_params(ds)
    single = pgcn.GCN(p, ds, device=0)
    cut = pgcn.GCN(p, ds, device=0, rank=0, world=1, unique_id=pgcn.comm_unique_id())
    for e in range(4):
        a = single.train_epoch() + single.eval(2)
        b = cut.train_epoch() + cut.eval(2)
        for k in (0, 2):
            assert abs(a[k] - b[k]) <= 1e-4 * abs(a[k]), (e, k, a, b)
    single.close()
    cut.close()


@pytest.mark.parametrize("name", ["cora", "synthetic"])
def test_edge_cut_split_rows_matches_all_rows(loaded, pgcn, name):
    """Edge-cut engine: the output layer's forward over the split's rows of every reduce-
    scatter chunk gives the same losses, accuracies and weights as summing all rows."""
    ds = loaded["cora"] if name == "cora" else pgcn.Dataset.synthetic(150000, 32, 8, 5000000, 6)
    p = pgcn.make_params(ds)
    runs = []
    for on in (1, 0):
        with helpers.knobs(pgcn, split_rows=on):
            g = pgcn.GCN(p, ds, device=0, rank=0, world=1, unique_id=pgcn.comm_unique_id())
            lines = [g.train_epoch() + g.eval(2) for _ in range(4)]
            for _ in range(2):
                g.epoch_async()
            lines += [tuple(r) for r in g.results(2)]
            lines.append(g.eval(3) + (0.0, 0.0))
            runs.append((np.array(lines, np.float64), g.get_var(2)))
            g.close()
    (a, wa), (b, wb) = runs
    np.testing.assert_allclose(a[:, [0, 2]], b[:, [0, 2]], rtol=1e-5)
    np.testing.assert_allclose(a[:, [1, 3]], b[:, [1, 3]], atol=2e-3)
    np.testing.assert_allclose(wa, wb, rtol=1e-4, atol=1e-6)


def test_deep_model_matches_oracle(loaded, pgcn):
    """4-layer, hidden 128 (the deep configuration of SURVEY.md §8a): the engine's L-layer
    stack against the oracle's L-layer restatement of the same module order."""
    ds = loaded["citeseer"]
    dims, drops = (128, 128, 128), (0.5, 0.5, 0.5, 0.5)
    g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=dims, dropouts=drops), ds)
    ref = helpers.OracleGCN(helpers.ds_dict(ds), hidden_dims=dims, dropouts=drops)
    for e in range(10):
        ours = g.train_epoch() + g.eval(2)
        want = ref.train_epoch() + ref.eval(2)
        for k in (0, 2):
            assert abs(ours[k] - want[k]) <= 1e-4 * abs(want[k]), (e, k, ours, want)
    g.close()


def test_async_epochs_match_sync(loaded, pgcn):
    """epoch_async (the bench loop: no host sync per epoch) produces the same lines."""
    ds = loaded["cora"]
    g = pgcn.GCN(pgcn.make_params(ds), ds)
    for _ in range(10):
        g.epoch_async()
    g.sync()
    res = g.results(10)
    gold = helpers.golden("cora")["epoch_lines"].reshape(-1, 4)
    np.testing.assert_allclose(res[:, 0], gold[:10, 0], rtol=1e-4)
    np.testing.assert_allclose(res[:, 2], gold[:10, 2], rtol=1e-4)
    g.close()


def test_train_ahead_bit_identical(pgcn):
    """Train-ahead (eval's first-layer pass also computes the next training forward's
    drop(X) W1, one stream over dense X) changes nothing: the same bits as separate passes,
    including an eval repeated before the next training epoch and an epoch without eval."""
    ds = pgcn.Dataset.synthetic(20000, 96, 8, 300000, 5)  # dense N(0,1) features
    p = pgcn.make_params(ds)
    runs = []
    pgcn.lib.pgcn_debug_set(b"eval_ax", 0)  # eval streams X (else it reads Â X instead)
    for ahead in (1, 0):
        pgcn.lib.pgcn_debug_set(b"train_ahead", ahead)
        g = pgcn.GCN(p, ds, device=0)
        lines = []
        for e in range(6):
            lines.append(g.train_epoch())
            if e != 3:  # epoch 3: no eval, so no product ahead
                lines.append(g.eval(2))
            if e == 1:
                lines.append(g.eval(3))  # a second eval: the product ahead is kept
        for _ in range(3):
            g.epoch_async()
        lines.append(tuple(g.results(3).ravel()))
        lines.append(tuple(g.get_var(2).ravel()))  # W1
        runs.append(lines)
        g.close()
    pgcn.lib.pgcn_debug_set(b"train_ahead", 1)
    pgcn.lib.pgcn_debug_set(b"eval_ax", 1)
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            np.testing.assert_array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32))


def test_split_rows_restriction_matches_all_rows(pgcn):
    """Output-layer row restriction (the last GraphSum's forward sums only the current split's
    labelled rows) on a graph that takes the LDS GraphSum path: the same losses, accuracies and
    weights as summing every row (fp32 summation order of a row may differ: rtol 1e-5)."""
    ds = pgcn.Dataset.synthetic(80000, 32, 8, 2000000, 7)
    p = pgcn.make_params(ds)
    runs = []
    for on in (1, 0):
        with helpers.knobs(pgcn, split_rows=on):
            g = pgcn.GCN(p, ds, device=0)
            lines = [g.train_epoch() + g.eval(2) for _ in range(4)]
            lines.append(g.eval(3))
            runs.append((np.array(lines[:-1], np.float64), lines[-1], g.get_var(2),
                         g.get_var(5)))
            g.close()
    (a, ta, w1a, w2a), (b, tb, w1b, w2b) = runs
    np.testing.assert_allclose(a[:, [0, 2]], b[:, [0, 2]], rtol=1e-5)
    np.testing.assert_allclose(a[:, [1, 3]], b[:, [1, 3]], atol=2e-4)  # a row may flip on a tie
    np.testing.assert_allclose(ta, tb, rtol=1e-5, atol=2e-4)
    np.testing.assert_allclose(w1a, w1b, rtol=1e-4, atol=1e-6)
    np.testing.assert_allclose(w2a, w2b, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("hidden", [16, 64])
def test_eval_ax_matches_graphsum_of_xw(pgcn, hidden):
    """eval's first layer from Â X computed once at build ((Â X) W1 instead of Â (X W1): the same
    product, another fp32 rounding order) gives the same eval losses and accuracies, and leaves
    training untouched (bit-identical training lines), on a graph that takes the LDS path
    (hidden 16: X-stream kernel; hidden 64: MFMA GEMM for (Â X) W1)."""
    ds = pgcn.Dataset.synthetic(80000, 40, 8, 2000000, 9)  # dense features, F = 40
    p = pgcn.make_params(ds, hidden_dims=(hidden,))
    runs = []
    for on in (1, 0):
        pgcn.lib.pgcn_debug_set(b"eval_ax", on)
        g = pgcn.GCN(p, ds, device=0)
        runs.append(np.array([g.train_epoch() + g.eval(2) for _ in range(4)], np.float64))
        g.close()
    pgcn.lib.pgcn_debug_set(b"eval_ax", 1)
    a, b = runs
    np.testing.assert_array_equal(a[0, :2], b[0, :2])  # epoch 1's training pass: same bits
    np.testing.assert_allclose(a[:, [0, 2]], b[:, [0, 2]], rtol=1e-5)
    np.testing.assert_allclose(a[:, [1, 3]], b[:, [1, 3]], atol=2e-4)


def _graph_vs_eager(pgcn, ds, schedule, n_res=8):
    runs = []
    for on in (0, 1):
        pgcn.lib.pgcn_debug_set(b"epoch_graph", on)
        g = pgcn.GCN(pgcn.make_params(ds), ds, device=0)
        lines = []
        for step in schedule:
            if step == "train":
                lines.append(g.train_epoch())
            elif step == "eval3":
                lines.append(g.eval(3))
            else:
                for _ in range(step):
                    g.epoch_async()
                lines.append(tuple(g.results(min(step, n_res)).ravel()))
        lines.append(tuple(g.get_var(2).ravel()))  # W1
        lines.append(tuple(g.get_var(5 if g.num_vars() == 7 else g.num_vars() - 2).ravel()))
        runs.append(lines)
        g.close()
    pgcn.lib.pgcn_debug_set(b"epoch_graph", 0)  # the engine default
    for a, b in zip(*runs):
        np.testing.assert_array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32))


def test_epoch_graph_bit_identical_cora(loaded, pgcn):
    """The per-epoch hipGraph replay (epoch_async) gives the same bits as eager epochs, with
    eager train_epoch/eval calls in between (device counters re-synced), over 4,200 epochs
    (the Adam step-size table block of 4,096 steps and the 1,024-slot results ring wrap)."""
    _graph_vs_eager(pgcn, loaded["cora"], [3, "train", "eval3", 5, "train", 4200, 2])


def test_epoch_graph_bit_identical_dense_lds(pgcn):
    """The same on a dense-feature graph that takes the LDS GraphSum, eval_ax and the compact
    output layer (the reddit configuration), and with eval_ax off, where train-ahead swaps
    buffers on the host and the engine stays eager (same bits either way)."""
    ds = pgcn.Dataset.synthetic(80000, 40, 8, 2000000, 11)
    _graph_vs_eager(pgcn, ds, [2, "train", 6, "eval3", 3])
    pgcn.lib.pgcn_debug_set(b"eval_ax", 0)
    try:
        _graph_vs_eager(pgcn, ds, [2, "train", 4])
    finally:
        pgcn.lib.pgcn_debug_set(b"eval_ax", 1)


# PART2 parameter files of the reference (parameters/parameters_<ds>.txt): hidden widths the
# kernels have no instantiation for (72: 16-column GraphSum passes; 200 > 128: 128-column
# GEMM slabs), zero input dropout, seeds, NO_FEATURE (binary features)
PART2 = {
    "cora": dict(hidden=(72,), dropouts=(0.4, 0.2), wd=5e-5, seed=1382895624, binary=False),
    "citeseer": dict(hidden=(200,), dropouts=(0.6, 0.6), wd=5e-4, seed=311288059, binary=False),
    "pubmed_synth": dict(hidden=(8,), dropouts=(0.0, 0.2), wd=5e-3, seed=2108234352,
                         binary=True),
}


@pytest.mark.parametrize("name", sorted(PART2))
def test_part2_configs_match_oracle(datasets, pgcn, name):
    """PART2 configurations against the oracle run with the same parameters and seed: loss
    lines within the north-star 1e-4, accuracies within the usual row tolerance."""
    cfg = PART2[name]
    root, names = datasets
    ds = pgcn.Dataset.load(root, names[name])
    if cfg["binary"]:
        ds.binarize()
    p = pgcn.make_params(ds, hidden_dims=cfg["hidden"], dropouts=cfg["dropouts"],
                         weight_decay=cfg["wd"], seed=cfg["seed"])
    g = pgcn.GCN(p, ds)
    ref = helpers.OracleGCN(helpers.ds_dict(ds), hidden_dims=cfg["hidden"],
                            dropouts=cfg["dropouts"], wd=cfg["wd"], seed=cfg["seed"])
    cnt = _counts(ds)
    for e in range(15):
        helpers.assert_line_close(g.train_epoch() + g.eval(2), ref.train_epoch() + ref.eval(2),
                                  cnt, what=f"epoch {e + 1}")
    g.close()


def test_three_chunk_weight_grad_matches_oracle(loaded, pgcn):
    """hidden_dims (160, 32): the second layer's weight gradient is a TN product of 32 output
    columns over K = 160, three 64-wide chunks on the general TN kernel (tn_plan once paired
    three chunks with a form the launcher does not list, and train_epoch failed with "gemm_tn:
    no kernel for N=32 K=160").  Two epochs against the oracle."""
    ds = loaded["cora"]
    dims, drops = (160, 32), (0.5, 0.5, 0.5)
    g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=dims, dropouts=drops), ds)
    ref = helpers.OracleGCN(helpers.ds_dict(ds), hidden_dims=dims, dropouts=drops)
    cnt = _counts(ds)
    for e in range(2):
        helpers.assert_line_close(g.train_epoch() + g.eval(2), ref.train_epoch() + ref.eval(2),
                                  cnt, what=f"epoch {e + 1}")
    g.close()


def _fused_run(pgcn, ds, fuse, epochs, reassoc_small=1, **make):
    with helpers.knobs(pgcn, fuse_epilogue=fuse, reassoc_small=reassoc_small):
        g = pgcn.GCN(pgcn.make_params(ds, **make), ds)
        lines = [g.train_epoch() + g.eval(2) for _ in range(epochs)]
        g.train_epoch()  # tensors of a training pass: relu/dropout forward and backward
    out = dict(lines=np.array(lines, np.float32), tails=g.query("fused_tails"),
               vars=[g.get_var(i) for i in (2, 3, 5)], grads=[g.get_var(i, 1) for i in (1, 3)])
    g.close()
    return out


@pytest.mark.parametrize("case", ["cora", "cora_h4", "lds_dense", "lds_deep"])
def test_fused_epilogue_bit_identical(loaded, pgcn, case):
    """ReLU + hidden Dropout in the first GraphSum's final write, and the Dropout + ReLU
    backward in the output GraphSum's backward (reassociated order, cora_h4 / lds_dense) give
    the same bits as the separate kernels: epoch lines, weights, the hidden activations and
    their gradients (gs_epilogue.hpp; plain gather kernels on cora, LDS ring + combine on the
    dense graph, where the epilogue also writes the next GraphSum's prescaled input table and
    that GraphSum skips its prescale: compared without that bit too; and the first layer's
    X-stream product applying the eval ReLU / writing the ring tables, compared without it; and
    on cora's module order the Dropout + ReLU backward in the output Matmul's input-grad
    product (k_xstream_nn epilogue), compared without it: fuse_epilogue 15 = all, 0 = none,
    13 = no prestaged tables, 11 = no X-stream epilogue, 7 = no Matmul tails; "cora" keeps
    the reference module order with reassoc_small 0, cora_h4 is reassociated either way)."""
    if case == "lds_dense":
        ds, make, tails = pgcn.Dataset.synthetic(120000, 64, 41, 1500000, 21), {}, 2
    elif case == "lds_deep":  # 128-wide rows: the tails ride the wide (all-pass) combine
        ds = pgcn.Dataset.synthetic(70000, 32, 41, 600000, 23)
        make, tails = dict(hidden_dims=(128, 128, 128), dropouts=(0.5,) * 4), 3
    else:
        ds = loaded["cora"]
        make, tails = ({"hidden_dims": (4,)}, 2) if case == "cora_h4" else ({"reassoc_small": 0}, 2)
    on = _fused_run(pgcn, ds, 15, 4, **make)
    off = _fused_run(pgcn, ds, 0, 4, **make)
    no_stage = _fused_run(pgcn, ds, 13, 4, **make)
    no_xs = _fused_run(pgcn, ds, 11, 4, **make)
    no_mm = _fused_run(pgcn, ds, 7, 4, **make)
    assert on["tails"] == tails and off["tails"] == 0
    assert no_mm["tails"] == (1 if case == "cora" else tails)
    for other in (off, no_stage, no_xs, no_mm):
        np.testing.assert_array_equal(on["lines"], other["lines"])
        for a, b in zip(on["vars"] + on["grads"], other["vars"] + other["grads"]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("case", ["lds_dense", "cora", "lds_deep"])
def test_fold_and_dense_co_draw_bit_identical(loaded, pgcn, case):
    """r06 launch cuts give the bits of the launches they replace: the weight gradients' last
    ordered reduction pass inside the Adam launch (tn_fold 1 vs 0: the X-stream TN's and the
    fused loss kernel's W.grad partials; eager and through the epoch hipGraph), on dense X the
    hidden dropout's mask drawn in the input dropout's launch (co_draw 2 vs 1), and the next
    epoch's masks drawn by the Adam launch (mask_adam 1 vs 0): epoch lines, the dropped input,
    weights, activations and gradients; the launch counter shows the cuts."""
    if case == "lds_dense":
        ds, make = pgcn.Dataset.synthetic(120000, 64, 41, 1500000, 21), {}
    elif case == "lds_deep":
        ds = pgcn.Dataset.synthetic(70000, 32, 41, 600000, 23)
        make = dict(hidden_dims=(128, 128, 128), dropouts=(0.5,) * 4)
    else:
        ds, make = loaded["cora"], {}
    runs = {}
    for name, kn in (("base", dict(tn_fold=0, co_draw=1, mask_adam=0)),
                     ("cut", dict(tn_fold=1, co_draw=2, mask_adam=1)),
                     ("graph", dict(tn_fold=1, co_draw=2, epoch_graph=1))):
        with helpers.knobs(pgcn, **kn):
            g = pgcn.GCN(pgcn.make_params(ds, **make), ds)
            g.train_epoch()
            g.eval(2)
            pgcn.reset_path_counts()
            for _ in range(4):
                g.epoch_async()
            lines = g.results(4)
            n = pgcn.path_counts()["launches"]
            g.train_epoch()
            runs[name] = dict(lines=np.array(lines, np.float32), launches=n,
                              vars=[g.get_var(i) for i in (0, 2, 3, 5)],
                              grads=[g.get_var(i, 1) for i in (1, 3)] + [g.get_var(2, 1)])
            g.close()
    a = runs["base"]
    for b in (runs["cut"], runs["graph"]):
        np.testing.assert_array_equal(a["lines"], b["lines"])
        for x, y in zip(a["vars"] + a["grads"], b["vars"] + b["grads"]):
            np.testing.assert_array_equal(x, y)
    # (cora: its one-pass W2.grad reduce; its masks were co-drawn already)
    assert runs["cut"]["launches"] <= a["launches"] - 4, (a["launches"], runs["cut"]["launches"])


def test_mask_xstream_bit_identical(rw_ds, pgcn):
    """mask_xstream 1 (off by default: measured slower): the next training forward's masks
    drawn by two extra waves of
    eval's (A X) W1 X-stream pass (reddit's feature width: the ring NN kernel) instead of by
    the Adam launch (mask_adam) or the forward itself: the same stream positions, so the same
    bits -- epoch lines, the dropped input, weights, activations and gradients -- over eager
    epochs, epoch_async runs and a training epoch with no eval before the next."""
    runs = {}
    for name, kn in (("adam", dict(mask_xstream=0, mask_adam=1)),
                     ("forward", dict(mask_xstream=0, mask_adam=0)),
                     ("xstream", dict(mask_xstream=1))):
        with helpers.knobs(pgcn, **kn):
            g = pgcn.GCN(pgcn.make_params(rw_ds), rw_ds)
            lines = [g.train_epoch() + g.eval(2)]
            for _ in range(3):
                g.epoch_async()
            lines += [tuple(x) for x in g.results(3)]
            lines.append(g.train_epoch() + g.train_epoch() + g.eval(2))
            runs[name] = dict(lines=lines, vars=[g.get_var(i) for i in (0, 2, 3, 5)],
                              grads=[g.get_var(i, 1) for i in (1, 3)] + [g.get_var(2, 1)])
            g.close()
    a = runs["forward"]
    for b in (runs["adam"], runs["xstream"]):
        assert a["lines"] == b["lines"]
        for x, y in zip(a["vars"] + a["grads"], b["vars"] + b["grads"]):
            np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("case", ["cora", "lds_dense"])
def test_mask_states_per_128_draws_bit_identical(loaded, pgcn, case):
    """mask_per 2 (one xorshift state per 128 draws, jumped by the epoch's period once) draws
    the masks of mask_per 1 (a state per 64 draws): epoch lines, the dropped input and every
    weight and gradient bit for bit over 4 epochs (an odd chunk count included: cora's input
    mask has 49,216 nonzeros / 64 = 769 chunks)."""
    ds = (pgcn.Dataset.synthetic(120000, 64, 41, 1500000, 21) if case == "lds_dense"
          else loaded["cora"])
    runs = []
    for per in (1, 2):
        with helpers.knobs(pgcn, mask_per=per):
            g = pgcn.GCN(pgcn.make_params(ds), ds)
            lines = [g.train_epoch() + g.eval(2) for _ in range(3)]
            g.train_epoch()
            runs.append(dict(lines=np.array(lines, np.float32),
                             t=[g.get_var(i) for i in (0, 2, 3, 5)] + [g.get_var(i, 1) for i in (1, 3)]))
            g.close()
    np.testing.assert_array_equal(runs[0]["lines"], runs[1]["lines"])
    for x, y in zip(runs[0]["t"], runs[1]["t"]):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("name", ["cora", "citeseer", "pubmed_synth"])  # 256 / 1024 threads
def test_csc_tree_matches_sequential_chain(loaded, pgcn, name):
    """csc_tree 1 (off by default: measured slower): sparse X's W1.grad as a fixed tree over
    each feature's entries (k_spmm_csc_tree) against hpdga's sequential scatter order
    (csc_tree 0, the default, k_spmm_csc_bwd,
    bit-exact with the reference): W1.grad within the reordering bound after an epoch, the
    epoch lines within 1e-5 over 5 epochs, and the tree repeats its own bits."""
    ds = loaded[name]
    runs = []
    for tree in (0, 1, 1):
        with helpers.knobs(pgcn, csc_tree=tree):
            g = pgcn.GCN(pgcn.make_params(ds), ds)
            g.train_epoch()
            gw1 = g.get_var(2, 1)
            lines = [g.train_epoch() + g.eval(2) for _ in range(5)]
            runs.append(dict(g=gw1, lines=np.array(lines, np.float64), w1=g.get_var(2)))
            g.close()
    seq, tree, again = runs
    scale = np.abs(seq["g"]).max()
    assert np.abs(tree["g"] - seq["g"]).max() <= 1e-5 * scale, np.abs(tree["g"] - seq["g"]).max()
    np.testing.assert_allclose(tree["lines"][:, [0, 2]], seq["lines"][:, [0, 2]], rtol=1e-5)
    np.testing.assert_array_equal(tree["g"], again["g"])
    np.testing.assert_array_equal(tree["w1"], again["w1"])


@pytest.mark.parametrize("case", ["cora", "pubmed_like", "two_level"])
def test_fuse_finish_matches_reduce_launch(loaded, pgcn, case):
    """fuse_finish 1 / 2: the loss kernel's last block sums the pass's (loss, wrong, W1^2)
    partials and writes the results ring slot (one launch fewer per pass; two_level: > 512
    blocks, each group of 64 summed by its last block first) -- the same losses and
    accuracies as the separate k_reduce_scalars launch up to the summation order (1e-6
    relative; the accuracies exactly), the same gradients and weights bit for bit (the scalars
    feed nothing else); eager and through the epoch hipGraph; one launch fewer per pass."""
    fused = 1
    if case == "pubmed_like":  # 310 loss blocks: still fused (up to 512)
        ds = pgcn.Dataset.synthetic(19717, 64, 3, 50000, 21)
    elif case == "two_level":  # 1,000 loss blocks: group tickets of 64, then the top ticket
        ds, fused = pgcn.Dataset.synthetic(64000, 64, 41, 400000, 23), 2
    else:
        ds = loaded["cora"]
    runs = {}
    for name, kn in (("launch", dict(fuse_finish=0)), ("fused", dict(fuse_finish=fused)),
                     ("graph", dict(fuse_finish=fused, epoch_graph=1))):
        with helpers.knobs(pgcn, **kn):
            g = pgcn.GCN(pgcn.make_params(ds), ds)
            sync_lines = [g.train_epoch() + g.eval(2) for _ in range(2)]
            pgcn.reset_path_counts()
            for _ in range(4):
                g.epoch_async()
            lines = np.array(sync_lines + [tuple(x) for x in g.results(4)], np.float64)
            n = pgcn.path_counts()["launches"]
            runs[name] = dict(lines=lines, launches=n, w=[g.get_var(2), g.get_var(4)])
            g.close()
    a = runs["launch"]
    for b in (runs["fused"], runs["graph"]):
        np.testing.assert_allclose(b["lines"][:, [0, 2]], a["lines"][:, [0, 2]], rtol=1e-6)
        np.testing.assert_array_equal(b["lines"][:, [1, 3]], a["lines"][:, [1, 3]])
        for x, y in zip(a["w"], b["w"]):
            np.testing.assert_array_equal(x, y)
    assert runs["fused"]["launches"] == a["launches"] - 8, (a["launches"], runs["fused"]["launches"])


def test_co_draw_and_split_rows_bit_identical(loaded, pgcn):
    """cora's small-graph launch cuts give the same bits as the launches they replace: the
    hidden dropout's mask drawn in the input dropout's launch (co_draw 1 vs 0), the hub rows'
    slots summed by the last item of the row in the GraphSum launch (gs_split 1 vs 0 at one
    item length), the output layer's column-subset backward gathering through original column
    ids instead of compacting its input (gs_orig_cols 1 vs 0), and eval's sparse product also
    computing the next training forward's, its masks drawn ahead (sparse_dual 1 vs 0); the cut
    launches show in the launch counter."""
    ds = loaded["cora"]
    runs = {}
    for name, kn in (("base", dict(co_draw=0, gs_split=0, gs_item_iters=32, gs_orig_cols=0,
                                   sparse_dual=0)),
                     ("cut", dict(co_draw=1, gs_split=1, gs_item_iters=32, gs_orig_cols=1,
                                  sparse_dual=1))):
        with helpers.knobs(pgcn, **kn):
            g = pgcn.GCN(pgcn.make_params(ds), ds)
            g.train_epoch()
            pgcn.reset_path_counts()
            lines = [g.train_epoch() + g.eval(2) for _ in range(4)]
            n = pgcn.path_counts()["launches"]
            g.train_epoch()
            runs[name] = dict(lines=np.array(lines, np.float32), launches=n,
                              vars=[g.get_var(i) for i in (2, 3, 5)],
                              grads=[g.get_var(i, 1) for i in (1, 3)])
            g.close()
    a, b = runs["base"], runs["cut"]
    np.testing.assert_array_equal(a["lines"], b["lines"])
    for x, y in zip(a["vars"] + a["grads"], b["vars"] + b["grads"]):
        np.testing.assert_array_equal(x, y)
    # per epoch: one mask launch, cora's d = 16 GraphSum combines (3 calls), one row gather
    assert b["launches"] <= a["launches"] - 5 * 4, (a["launches"], b["launches"])


@pytest.mark.parametrize("case", ["cora_h4", "lds_dense"])
def test_fused_output_layer_bit_identical(loaded, pgcn, case):
    """The output layer's Matmul forward computed inside the loss kernel (launch_out_xent: an
    fmaf chain in k_gemm_nn's MFMA order, then the same cross-entropy tile) gives the bits of
    the separate Matmul + CrossEntropyLoss: epoch lines, weights, activations and gradients
    (reassociated output layer: cora with hidden 4 < 7 classes; the LDS-path graph, 41
    classes)."""
    if case == "lds_dense":
        ds, make = pgcn.Dataset.synthetic(120000, 64, 41, 1500000, 21), {}
    else:
        ds, make = loaded["cora"], {"hidden_dims": (4,)}
    runs = {}
    for fo in (1, 0):  # 1: the logits and the input grad fused (no weight-grad partials)
        with helpers.knobs(pgcn, fuse_output=fo):
            g = pgcn.GCN(pgcn.make_params(ds, **make), ds)
            lines = np.array([g.train_epoch() + g.eval(2) for _ in range(3)], np.float32)
            g.train_epoch()
            runs[fo] = (lines, [g.get_var(i) for i in (2, 3, 5)] + [g.get_var(i, 1) for i in (1, 3)])
            g.close()
    np.testing.assert_array_equal(runs[1][0], runs[0][0])
    for a, b in zip(runs[1][1], runs[0][1]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("case", ["lds_dense", "cora_h4"])
def test_fused_output_weight_grad_close(loaded, pgcn, case):
    """The loss kernel's per-block partials of W2.grad, reduced in block order
    (fuse_output 2 / 3): the same sums as k_gemm_tn's in another grouping -- W2.grad of the
    first step within 2e-6 relative of the k_gemm_tn one, and the epoch lines after it within
    float rounding (LDS-path graph, 41 classes, hidden 16; cora at hidden 4, 7 classes: a
    grad tile narrower than the waves' partials, which the launch then sizes the LDS for)."""
    if case == "lds_dense":
        ds, make = pgcn.Dataset.synthetic(120000, 64, 41, 1500000, 21), {}
    else:
        ds, make = loaded["cora"], {"hidden_dims": (4,)}
    runs = {}
    for wg in (3, 1):  # 3: the partials on any graph size (2, the default, from 65,536 rows)
        with helpers.knobs(pgcn, fuse_output=wg):
            g = pgcn.GCN(pgcn.make_params(ds, **make), ds)
            first = g.train_epoch()
            w2g = g.get_var(5, 1).copy()
            lines = [first] + [g.train_epoch() + g.eval(2) for _ in range(3)]
            runs[wg] = (np.array(lines[0]), np.array(lines[1:], np.float64), w2g)
            g.close()
    np.testing.assert_array_equal(runs[3][0], runs[1][0])  # the first forward: same bits
    scale = np.abs(runs[1][2]).max()
    assert np.abs(runs[3][2] - runs[1][2]).max() <= 2e-6 * scale
    # the losses after it agree to float rounding (accuracies may flip a near-tied row)
    np.testing.assert_allclose(runs[3][1][:, [0, 2]], runs[1][1][:, [0, 2]], rtol=2e-5)


@pytest.mark.parametrize("name", ["cora", "citeseer", "pubmed_synth"])
def test_deferred_output_wgrad_small_graph(loaded, pgcn, name):
    """defer_wgrad 1 (default; small graphs of <= 128 loss blocks -- pubmed_synth's 309 keep
    the k_xstream_tn path: the same lines, launches and bits; output layer reassociated): the fused loss
    kernel's per-block W2.grad partials go to the deferred-reduction pool and the Adam launch
    sums them in block order -- no k_xstream_tn launch.  W2.grad within 2e-6 relative of the
    k_xstream_tn one (defer_wgrad 0: another grouping of the same sums), the epoch lines within
    float rounding, one launch fewer per epoch; tn_fold 0 reduces the same partials in one
    ordered pass of its own: the same bits as the Adam launch's sum."""
    ds = loaded[name]
    runs = {}
    for tag, kn in (("tn", dict(defer_wgrad=0)), ("defer", dict(defer_wgrad=1)),
                    ("pass", dict(defer_wgrad=1, tn_fold=0))):
        with helpers.knobs(pgcn, **kn):
            g = pgcn.GCN(pgcn.make_params(ds), ds)
            assert g.query("reassociated") == 1
            g.train_epoch()
            w2g = g.get_var(5, 1).copy()
            lines = [g.train_epoch() + g.eval(2) for _ in range(3)]
            pgcn.reset_path_counts()
            for _ in range(4):
                g.epoch_async()
            g.results(4)
            n = pgcn.path_counts()["launches"]
            runs[tag] = dict(g=w2g, lines=np.array(lines, np.float64), launches=n,
                             w=g.get_var(5).copy())
            g.close()
    a, b, c = runs["tn"], runs["defer"], runs["pass"]
    scale = np.abs(a["g"]).max()
    assert np.abs(b["g"] - a["g"]).max() <= 2e-6 * scale
    np.testing.assert_allclose(b["lines"][:, [0, 2]], a["lines"][:, [0, 2]], rtol=2e-5)
    np.testing.assert_array_equal(b["g"], c["g"])
    np.testing.assert_array_equal(b["w"], c["w"])
    if name == "pubmed_synth":
        np.testing.assert_array_equal(b["g"], a["g"])
        assert b["launches"] == a["launches"]
    else:
        assert b["launches"] == a["launches"] - 4, (a["launches"], b["launches"])


def test_early_stopping_matches_reference(datasets, pgcn):
    """GCN::run's early stopping (hpdga gcn.cpp:238-250, src/gcn.cu:377-395): after epoch e >=
    k, stop when val_loss(e) > the mean of the last k val losses (the current one included,
    summed in float in epoch order).  The reference's cora parameter file (k = 10, 1000 epochs,
    hidden 72, seed) stops at the epoch the oracle's loss history gives (136); every
    comparison up to it clears its threshold by >= 3e-4 relative, far above the engine's
    loss error, so the stop epoch is a parity property."""
    cfg, k = PART2["cora"], 10
    root, names = datasets
    ds = pgcn.Dataset.load(root, names["cora"])
    ref = helpers.OracleGCN(helpers.ds_dict(ds), hidden_dims=cfg["hidden"],
                            dropouts=cfg["dropouts"], wd=cfg["wd"], seed=cfg["seed"])
    hist, stop, margin = [], None, 1.0
    for epoch in range(1, 1001):
        ref.train_epoch()
        vl = np.float32(ref.eval(2)[0])
        hist.append(vl)
        if epoch >= k:
            recent = np.float32(0.0)
            for i in range(epoch - k, epoch):
                recent = np.float32(recent + hist[i])
            thr = np.float32(recent / np.float32(k))
            margin = min(margin, abs(float(vl) - float(thr)) / float(vl))
            if vl > thr:
                stop = epoch
                break
    assert stop is not None and margin >= 3e-4, (stop, margin)
    p = pgcn.make_params(ds, hidden_dims=cfg["hidden"], dropouts=cfg["dropouts"],
                         weight_decay=cfg["wd"], seed=cfg["seed"], epochs=1000, early_stopping=k)
    g = pgcn.GCN(p, ds)
    g.run(verbose=False)
    assert g.query("epochs") == stop
    g.close()


def _cpp_api(datasets, mode, epochs):
    import os
    import subprocess
    root, names = datasets
    exe = os.path.join(os.path.dirname(helpers.__file__), "..", "parallel-gcn_amd", "bin",
                       "test_module_api")
    return subprocess.run([exe, mode, root, names["cora"], str(epochs)], capture_output=True,
                          text=True, timeout=300)


@pytest.mark.parametrize("mode", ["modules", "streams", "gcn"])
def test_cpp_module_api_matches_reference(datasets, pgcn, mode):
    """The reference-shaped C++ API (include/pgcn.hpp) from a C++ program
    (tests/cpp/test_module_api.cpp): "modules" assembles the 2-layer GCN from Variable,
    Dropout, SparseMatmul, GraphSum, ReLU, Matmul, CrossEntropyLoss and Adam objects exactly
    as hpdga-spring23's GCN constructor does and runs its train_epoch / eval(2); "streams"
    wires the same modules to the CUDA reference's streams and events (training forward,
    backward, Matmul weight gradient + Adam on a second backward stream, eval on its own
    stream; src/gcn.cu:5-11, src/module.cu, src/optim.cu:57-95), which the API honours; "gcn"
    runs pgcn::api::GCN.  All 100 cora epoch lines against the reference's golden lines
    (losses 1e-4 relative, accuracies within 2 rows)."""
    root, names = datasets
    out = _cpp_api(datasets, mode, 100)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = np.array([[float(x) for x in ln.split()[1:]] for ln in out.stdout.splitlines()
                      if ln.startswith("epoch=")], np.float64)
    assert lines.shape == (100, 4)
    gold = helpers.golden("cora")["epoch_lines"].reshape(-1, 4)
    cnt = helpers.split_counts(pgcn.Dataset.load(root, names["cora"]))
    for e in range(100):
        helpers.assert_line_close(lines[e], gold[e], cnt, what=f"{mode} epoch {e + 1}")


def test_cpp_two_graphsums_on_one_index(datasets):
    """Two GraphSums on one DevSparseIndex with different values (Â and 2 Â) each keep their
    own device graph (the first one's graph is not freed when the second is built): the second
    output is twice the first (include/pgcn.hpp DevSparseIndex::graph)."""
    out = _cpp_api(datasets, "twographs", 0)
    assert out.returncode == 0 and "twographs ok" in out.stdout, out.stdout + out.stderr[-2000:]


@pytest.mark.parametrize("case", ["cora", "lds_dense"])
def test_matmul_side_stream_bit_identical(loaded, pgcn, case):
    """Matmul weight gradients on the side stream (mm_side, joined before the optimizer) give
    the same bits as the in-order launches: epoch lines and weights after 4 epochs (cora: the
    reference module order, W2.grad beside Dropout/ReLU/GraphSum backward; the dense LDS
    graph: the reassociated output layer, W2.grad beside both backward GraphSums; both with
    k_gemm_tn for W2.grad, as the loss kernel's partials (fuse_output 2) are off beside
    mm_side)."""
    ds = loaded["cora"] if case == "cora" else pgcn.Dataset.synthetic(120000, 64, 41, 1500000, 21)
    runs = []
    for side in (2, 0):  # 2: on whatever the graph size
        with helpers.knobs(pgcn, mm_side=side, fuse_output=1):
            g = pgcn.GCN(pgcn.make_params(ds), ds)
            lines = np.array([g.train_epoch() + g.eval(2) for _ in range(4)], np.float32)
            runs.append((lines, g.get_var(2), g.get_var(5)))
            g.close()
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)
