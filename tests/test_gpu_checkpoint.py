"""Checkpoint / resume of the engine: a resumed run continues bit for bit (masks, Adam steps,
results rows), on one GPU and as edge-cut ranks; weights-only loads; refusals that leave the
engine untouched; the gcn-par save= / load= / predict= options.
"""
import os
import subprocess

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _weight_ids(g):
    return [2 + 3 * l for l in range((g.num_vars() - 1) // 3)]


def _state(g, n):
    return dict(results=g.results(n), weights=[g.get_var(i) for i in _weight_ids(g)],
                steps=g.query("adam_steps"), epochs=g.query("epochs"))


def _assert_same(a, b, what):
    assert a["steps"] == b["steps"] and a["epochs"] == b["epochs"], what
    assert a["results"].shape == b["results"].shape, what
    np.testing.assert_array_equal(_bits(a["results"]), _bits(b["results"]), err_msg=what)
    assert len(a["weights"]) == len(b["weights"])
    for x, y in zip(a["weights"], b["weights"]):
        np.testing.assert_array_equal(_bits(x), _bits(y), err_msg=what)


def _epochs(g, n, drive):
    for _ in range(n):
        if drive == "async":
            g.epoch_async()
        else:
            g.train_epoch()
            g.eval(2)


@pytest.fixture(scope="module")
def graphs(pgcn, loaded):
    return {"cora": loaded["cora"],
            "swap": pgcn.Dataset.synthetic(20000, 96, 8, 300000, 5),
            "lds": pgcn.Dataset.synthetic(80000, 40, 8, 2000000, 11)}


CONFIGS = {
    # sparse X: sparse_dual, co_draw, mask_adam
    "cora": ("cora", {}, {}),
    # dense X without eval_ax: the train_ahead buffer swaps
    "swap": ("swap", {}, {"eval_ax": 0}),
    # dense X, the LDS ring GraphSum and eval_ax at defaults
    "lds": ("lds", {}, {}),
    "cora4": ("cora", dict(hidden_dims=(16, 16, 16), dropouts=(0.5, 0.5, 0.5, 0.5)), {}),
    "cora_graph": ("cora", {}, {"epoch_graph": 1}),
    # a configuration whose epochs really replay the captured graph (dense X with eval_ax):
    # the load must re-sync the graph's device counters and step table
    "lds_graph": ("lds", {}, {"epoch_graph": 1}),
}


@pytest.mark.parametrize("drive", ["async", "pairs"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_resume_is_bit_exact(pgcn, graphs, tmp_path, config, drive):
    """U runs 6 epochs; S runs 3, saves, runs 2 more, loads (a rollback on a trained engine
    holding masks and products computed ahead) and runs 3; F is fresh, loads and runs 3.
    results(6), every weight and the step count of S and F equal U's exactly."""
    name, pkw, knobs = CONFIGS[config]
    ds = graphs[name]
    ck = str(tmp_path / "ck.pgcnck")
    with helpers.knobs(pgcn, **knobs):
        u = pgcn.GCN(pgcn.make_params(ds, **pkw), ds)
        _epochs(u, 6, drive)
        want = _state(u, 6)
        u.close()
        s = pgcn.GCN(pgcn.make_params(ds, **pkw), ds)
        _epochs(s, 3, drive)
        if drive == "pairs":
            s.eval(3)  # a stray pass before the save
        s.save(ck)
        assert not os.path.exists(ck + ".tmp")
        _epochs(s, 2, drive)
        s.load(ck)
        assert s.query("epochs") == 3 and s.query("adam_steps") == 3
        _epochs(s, 3, drive)
        _assert_same(_state(s, 6), want, f"{config} {drive}: rolled back")
        s.close()
        f = pgcn.GCN(pgcn.make_params(ds, **pkw), ds)
        f.load(ck)
        np.testing.assert_array_equal(_bits(f.results(6)), _bits(want["results"][:3]))
        _epochs(f, 3, drive)
        _assert_same(_state(f, 6), want, f"{config} {drive}: fresh")
        f.close()
    info = pgcn.checkpoint_info(ck)
    assert info["epochs"] == 3 and info["adam_steps"] == 3 and info["num_nodes"] == ds.num_nodes


def test_edge_cut_resume_and_cross_world(pgcn, loaded, tmp_path):
    """Loopback W = 2 on cora: the rolled-back engine equals the uninterrupted one on both
    ranks, the ranks' checkpoint files are byte-identical, and a one-GPU checkpoint loaded
    into the two ranks continues within rtol 1e-4 of the one-GPU resumed run."""
    ds = loaded["cora"]
    one_ck = str(tmp_path / "one.pgcnck")
    g = pgcn.GCN(pgcn.make_params(ds), ds)
    _epochs(g, 3, "pairs")
    g.save(one_ck)
    g.load(one_ck)
    one_next = [g.train_epoch() + g.eval(2) for _ in range(2)]
    g.close()

    def world(fn):
        group = pgcn.LoopbackGroup(2)

        def rank_fn(r):
            e = pgcn.GCN(pgcn.make_params(ds), ds, device=0, rank=r, loopback=group)
            out = fn(e, r)
            e.close()
            return out
        return pgcn.run_ranks(2, rank_fn)

    def uninterrupted(e, r):
        _epochs(e, 6, "pairs")
        return _state(e, 6)

    def rolled_back(e, r):
        _epochs(e, 3, "pairs")
        e.save(str(tmp_path / f"rank{r}.pgcnck"))
        _epochs(e, 2, "pairs")
        e.load(str(tmp_path / f"rank{r}.pgcnck"))
        _epochs(e, 3, "pairs")
        return _state(e, 6)

    def from_one_gpu(e, r):
        e.load(one_ck)
        assert e.query("epochs") == 3 and e.query("adam_steps") == 3
        return [e.train_epoch() + e.eval(2) for _ in range(2)]

    want, got = world(uninterrupted), world(rolled_back)
    for r in range(2):
        _assert_same(got[r], want[r], f"rank {r}")
    a = open(tmp_path / "rank0.pgcnck", "rb").read()
    assert a == open(tmp_path / "rank1.pgcnck", "rb").read() and len(a) > 216
    lines = world(from_one_gpu)
    assert lines[0] == lines[1]
    np.testing.assert_allclose(np.asarray(lines[0]), np.asarray(one_next), rtol=1e-4)


@pytest.mark.parametrize("dropouts", [(0.0, 0.0), (0.5, 0.5)])
def test_weights_only_load(pgcn, loaded, tmp_path, dropouts):
    """After a weights-only load the weights are the file's, the optimizer is fresh and the
    epoch count stays.  The next training loss is a function of the weights and the masks.
    Without dropout it is compared (1e-4) with a fresh engine given the same weights by
    set_var; with dropout the load keeps the dropout position, which a fresh engine is not at,
    so there the comparison is with an engine at the same position (the same two epochs, then
    the weights by set_var): bit-equal, and the fresh engine's loss is printed only."""
    ds = loaded["cora"]
    ck = str(tmp_path / "ck.pgcnck")
    a = pgcn.GCN(pgcn.make_params(ds, dropouts=dropouts), ds)
    _epochs(a, 4, "async")
    a.save(ck)
    file_w = [a.get_var(i) for i in _weight_ids(a)]
    a.close()
    b = pgcn.GCN(pgcn.make_params(ds, dropouts=dropouts), ds)
    _epochs(b, 2, "async")
    b.load(ck, weights_only=True)
    for i, w in zip(_weight_ids(b), file_w):
        np.testing.assert_array_equal(_bits(b.get_var(i)), _bits(w))
    assert b.query("adam_steps") == 0 and b.query("epochs") == 2
    loss_b = b.train_epoch()[0]
    assert b.query("adam_steps") == 1
    b.close()

    def with_set_var(epochs_before):
        c = pgcn.GCN(pgcn.make_params(ds, dropouts=dropouts), ds)
        _epochs(c, epochs_before, "async")
        for i, w in zip(_weight_ids(c), file_w):
            c.set_var(i, w)
        loss = c.train_epoch()[0]
        c.close()
        return loss
    fresh = with_set_var(0)
    print(f"dropouts {dropouts}: loss after the load {loss_b}, fresh engine {fresh}")
    if dropouts == (0.0, 0.0):
        assert abs(loss_b - fresh) <= 1e-4 * abs(fresh), (loss_b, fresh)
    else:
        assert loss_b == with_set_var(2)


def test_resume_after_weights_only_load(pgcn, loaded, tmp_path):
    """A weights-only load resets the Adam step count but not the dropout position; a
    checkpoint saved after it records both, so a resume from it is still bit-exact."""
    ds = loaded["cora"]
    ck, ck2 = str(tmp_path / "ck.pgcnck"), str(tmp_path / "ck2.pgcnck")
    a = pgcn.GCN(pgcn.make_params(ds), ds)
    _epochs(a, 2, "async")
    a.save(ck)
    _epochs(a, 1, "async")
    a.load(ck, weights_only=True)
    _epochs(a, 1, "async")
    assert a.query("adam_steps") == 1 and a.query("epochs") == 4
    a.save(ck2)
    _epochs(a, 2, "async")
    want = _state(a, 6)
    a.close()
    f = pgcn.GCN(pgcn.make_params(ds), ds)
    f.load(ck2)
    _epochs(f, 2, "async")
    _assert_same(_state(f, 6), want, "resumed after a weights-only load")
    f.close()


def test_refusals_leave_the_engine_untouched(pgcn, loaded, tmp_path):
    """Every refused load or set_var returns its status, and the epoch after it is the one the
    uninterrupted engine runs."""
    ds = loaded["cora"]
    u = pgcn.GCN(pgcn.make_params(ds), ds)
    _epochs(u, 3, "async")
    good = str(tmp_path / "good.pgcnck")
    u.save(good)
    raw = open(good, "rb").read()

    def variant(name, data):
        path = str(tmp_path / name)
        with open(path, "wb") as f:
            f.write(data)
        return path
    flipped = bytearray(raw)
    flipped[len(raw) // 2] ^= 0x10
    bad_io = [variant("truncated", raw[:-1]), variant("flipped", bytes(flipped)),
              variant("magic", b"PGCNCK99" + raw[8:]), str(tmp_path / "missing")]
    wide = pgcn.GCN(pgcn.make_params(ds, hidden_dims=(32,)), ds)
    wide_ck = str(tmp_path / "wide.pgcnck")
    wide.save(wide_ck)
    wide.close()
    seeded = pgcn.GCN(pgcn.make_params(ds, seed=1234), ds)
    seeded_ck = str(tmp_path / "seeded.pgcnck")
    seeded.save(seeded_ck)
    seeded.close()

    refusals = [(lambda e, p=p: e.load(p), pgcn.PGCN_E_IO) for p in bad_io]
    refusals += [(lambda e: e.load(wide_ck), pgcn.PGCN_E_INVALID),
                 (lambda e: e.load(wide_ck, weights_only=True), pgcn.PGCN_E_INVALID),
                 (lambda e: e.load(seeded_ck), pgcn.PGCN_E_INVALID),
                 (lambda e: e.set_var(1, np.zeros(ds.num_nodes * 16, np.float32)),
                  pgcn.PGCN_E_INVALID),
                 (lambda e: e.set_var(2, np.zeros(ds.input_dim * 16, np.float32), which=1),
                  pgcn.PGCN_E_INVALID),
                 (lambda e: e.set_var(2, np.zeros(5, np.float32)), pgcn.PGCN_E_INVALID)]
    u.epoch_async()
    want = _state(u, 4)
    u.close()
    e = pgcn.GCN(pgcn.make_params(ds), ds)
    _epochs(e, 3, "async")
    for call, status in refusals:
        with pytest.raises(pgcn.PgcnError) as err:
            call(e)
        assert err.value.status == status
    e.epoch_async()
    _assert_same(_state(e, 4), want, "after the refusals")
    e.close()
    # (another seed is fine for a weights-only load: only dims and num_nodes identify it)
    e = pgcn.GCN(pgcn.make_params(ds), ds)
    e.load(seeded_ck, weights_only=True)
    e.close()


def _epoch_lines(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("epoch=")]
    return [" ".join(t for t in ln.split() if not t.startswith("time=")) for ln in lines]


def test_cli_save_load_predict(pgcn, datasets, loaded, tmp_path):
    """gcn-par: epochs=3 save=ck, then load=ck up to epoch 6, prints the lines of epochs 4-6 of
    an uninterrupted epochs=6 run (apart from time=); predict= writes one line per node, the
    classes of the Python predict() of an engine loaded from the checkpoint of that state."""
    root, names = datasets
    exe = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "gcn-par")
    ck, ck2, out = (str(tmp_path / n) for n in ("ck", "ck2", "pred.txt"))

    def run(*args):
        r = subprocess.run([exe, names["cora"], f"root={root}", *args], capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return _epoch_lines(r.stdout)
    whole = run("epochs=6")
    first = run("epochs=3", f"save={ck}")
    rest = run("epochs=6", f"load={ck}", f"save={ck2}", f"predict={out}")
    assert len(whole) == 6 and first == whole[:3]
    assert rest == whole[3:] and rest[0].startswith("epoch=4 ")
    rows = [ln.split() for ln in open(out).read().splitlines()]
    ds = loaded["cora"]
    assert len(rows) == ds.num_nodes == 2708
    assert [int(r[0]) for r in rows] == list(range(ds.num_nodes))
    g = pgcn.GCN(pgcn.make_params(ds), ds)
    g.load(ck2)
    cls, conf = g.predict()
    g.close()
    np.testing.assert_array_equal(np.array([int(r[1]) for r in rows]), cls)
    np.testing.assert_allclose(np.array([float(r[2]) for r in rows]), conf, atol=1e-6)
