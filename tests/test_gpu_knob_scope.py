"""An engine follows the knobs it was built with (csrc/knobs.hpp): pgcn_debug_set changes
nothing in an engine that exists, whichever way the values move and however many engines are
alive.  Every comparison is bit for bit: epoch lines, every variable and its gradient, and the
kernel-path counts (launches included).  (The graph-scope half is in
test_gpu_graphsum_edges.py.)"""
import functools

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

# every knob an existing engine used to re-read at a later call, away from its default
OFF = dict(fuse_epilogue=0, fuse_output=0, tn_fold=0, mask_adam=0, fuse_finish=0, split_cols=0,
           sparse_dual=0, co_draw=0, train_ahead=0, eval_ax=0, csc_tree=1)
# dense X: the smallest kind of graph on which a default engine precomputes Â X (eval_ax)
DENSE = dict(n=3001, f=24, c=8, edges=30000, seed=13)
CASES = ("cora", "dense")


@functools.lru_cache(maxsize=None)
def _dense(pgcn):
    return pgcn.Dataset.synthetic(DENSE["n"], DENSE["f"], DENSE["c"], DENSE["edges"],
                                  DENSE["seed"])


def _data(pgcn, loaded, case):
    """(dataset, OFF for it): the dense case adds split_rows, whose restricted graphs the engine
    builds at the first switch to each split."""
    if case == "cora":
        return loaded["cora"], OFF
    return _dense(pgcn), dict(OFF, split_rows=1)


def _build(pgcn, ds):
    g = pgcn.GCN(pgcn.make_params(ds), ds, device=0)
    assert g.num_vars() == 7  # X, X W1, Â., relu / dropout, ..., W2 at 5, the logits last
    return g


def _steps(pgcn, g):
    """The run, one generator step per engine call: 3 x (train_epoch + eval(2)), eval(3), one
    more train_epoch; yields None, and at the end the lines and what eval(3) left refused."""
    lines = []
    for _ in range(3):
        lines.append(g.train_epoch())
        yield
        lines.append(g.eval(2))
        yield
    lines.append(g.eval(3))
    try:
        g.get_var(g.num_vars() - 1)
        refused = False
    except pgcn.PgcnError:  # the split_rows restriction left the other rows' logits stale
        refused = True
    yield
    lines.append(g.train_epoch())
    yield dict(lines=np.array(lines, np.float32), refused=refused)


def _tensors(pgcn, g):
    out = {}
    for i in range(g.num_vars()):
        for which in (0, 1):
            try:
                out[i, which] = g.get_var(i, which)
            except pgcn.PgcnError:
                out[i, which] = None
    for i in (2, 5):  # W1, W2 and their gradients were read
        assert out[i, 0] is not None and out[i, 0].any() and out[i, 1] is not None, i
    assert out[2, 1].any() or out[5, 1].any()
    return out


def _run(pgcn, g):
    """One engine's whole run and everything it leaves; closes the engine."""
    pgcn.reset_path_counts()
    for res in _steps(pgcn, g):
        pass
    g.sync()
    res["paths"] = pgcn.path_counts()
    res["tensors"] = _tensors(pgcn, g)
    res["knob"] = {k: g.query("knob." + k) for k in ("fuse_output", "split_rows", "tn_fold")}
    g.close()
    return res


def _assert_same(a, b, what, paths=True):
    np.testing.assert_array_equal(a["lines"], b["lines"], err_msg=what)
    assert a["refused"] == b["refused"], what
    assert a["tensors"].keys() == b["tensors"].keys()
    for key, x in a["tensors"].items():
        y = b["tensors"][key]
        assert (x is None) == (y is None), (what, key)
        if x is not None:
            np.testing.assert_array_equal(x, y, err_msg=f"{what}: variable {key}")
    if paths:
        assert a["paths"] == b["paths"], what
    assert a["knob"] == b["knob"], what


_SOLO = {}


def solo(pgcn, loaded, case, off):
    """The reference runs, computed once and shared: an engine built and run with the knobs as
    they stand (off: both inside knobs(**OFF))."""
    if (case, off) not in _SOLO:
        ds, kw = _data(pgcn, loaded, case)
        with helpers.knobs(pgcn, **(kw if off else {})):
            _SOLO[case, off] = _run(pgcn, _build(pgcn, ds))
    return _SOLO[case, off]


@pytest.mark.parametrize("case", CASES)
def test_engine_keeps_its_knobs_after_the_block(pgcn, loaded, case):
    """Built inside knobs(**OFF), run after the block has closed: the same as built and run
    inside it.  Dense: eval(3) switches to a split whose restricted graph the engine first builds
    outside the block, and still leaves the logits refused."""
    ds, kw = _data(pgcn, loaded, case)
    inside = solo(pgcn, loaded, case, True)
    with helpers.knobs(pgcn, **kw):
        g = _build(pgcn, ds)
    after = _run(pgcn, g)
    assert after["knob"]["fuse_output"] == 0 and inside["knob"]["fuse_output"] == 0
    assert inside["knob"]["split_rows"] == (1 if case == "dense" else 0)
    _assert_same(after, inside, f"{case}: built inside, run outside")
    if case == "dense":
        assert after["refused"] and inside["refused"]
    # ... and OFF is another engine than the default one, by its launches
    assert inside["paths"] != solo(pgcn, loaded, case, False)["paths"]


@pytest.mark.parametrize("case", CASES)
def test_default_engine_ignores_knobs_set_later(pgcn, loaded, case):
    """The converse: a default-built engine run inside knobs(**OFF) equals one run outside."""
    ds, kw = _data(pgcn, loaded, case)
    g = _build(pgcn, ds)
    if case == "dense":
        assert g.query("eval_ax_us") > 0
    with helpers.knobs(pgcn, **kw):
        inside = _run(pgcn, g)
    assert inside["knob"] == dict(fuse_output=2, split_rows=0, tn_fold=1)
    assert not inside["refused"]
    _assert_same(inside, solo(pgcn, loaded, case, False), f"{case}: default engine, OFF set later")


@pytest.mark.parametrize("case", CASES)
def test_two_engines_alive_keep_their_own_knobs(pgcn, loaded, case):
    """One default and one OFF engine alive at once, their calls alternated: each equals its solo
    run, and the process-wide path counts are the two solo runs' added up."""
    ds, kw = _data(pgcn, loaded, case)
    a = _build(pgcn, ds)
    with helpers.knobs(pgcn, **kw):
        b = _build(pgcn, ds)
    pgcn.reset_path_counts()
    for ra, rb in zip(_steps(pgcn, a), _steps(pgcn, b)):
        pass
    a.sync()
    b.sync()
    paths = pgcn.path_counts()
    for g, r in ((a, ra), (b, rb)):
        r["tensors"] = _tensors(pgcn, g)
        r["knob"] = {k: g.query("knob." + k) for k in ("fuse_output", "split_rows", "tn_fold")}
        g.close()
    sa, sb = solo(pgcn, loaded, case, False), solo(pgcn, loaded, case, True)
    _assert_same(ra, sa, f"{case}: default engine beside an OFF one", paths=False)
    _assert_same(rb, sb, f"{case}: OFF engine beside a default one", paths=False)
    assert paths == {k: sa["paths"][k] + sb["paths"][k] for k in paths}
