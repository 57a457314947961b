"""include/pgcn.hpp's BCEWithLogitsLoss from a C++ program (tests/cpp/test_multilabel_api.cpp):
a 2-layer cora model assembled from api modules ending in the multi-label loss, against the
engine's multi-label model on the same data and seed; and gcn-par's multilabel=1."""
import os
import subprocess

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

BIN = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin")


@pytest.fixture(scope="module")
def cora_labels(tmp_path_factory, pgcn):
    """A root of its own with cora's three files and a seeded 7-class data/cora.labels."""
    root = str(tmp_path_factory.mktemp("multilabel"))
    name = helpers.materialize_dataset("cora", root)
    ds = pgcn.Dataset.load(root, name)
    Y = np.random.default_rng(7).random((ds.num_nodes, 7)) < 0.3
    Y[0, 6] = True  # the largest id is present: the file alone gives the class count
    path = os.path.join(root, "data", name + ".labels")
    with open(path, "w") as f:
        for row in Y:
            f.write(" ".join(str(j) for j in np.nonzero(row)[0]) + "\n")
    ds.load_labels(path)
    assert ds.output_dim == 7
    np.testing.assert_array_equal(pgcn.unpack_label_bits(ds.label_bits, 7), Y)
    return root, name, ds, Y


def test_cpp_bce_modules_match_engine(cora_labels, pgcn):
    """The hand-assembled model's first-epoch loss equals the engine's (the reference's module
    order, dropout 0.5: the same mask stream positions) within 1e-6 relative; three epochs stay
    within 1e-4, the Hamming accuracies within 2 elements."""
    root, name, ds, _ = cora_labels
    out = subprocess.run([os.path.join(BIN, "test_multilabel_api"), root, name, "3"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = np.array([[float(x) for x in ln.split()[1:]] for ln in out.stdout.splitlines()
                      if ln.startswith("epoch=")], np.float64)
    assert lines.shape == (3, 4)
    g = pgcn.GCN(pgcn.make_params(ds, multilabel=True, reassociate_last=False), ds)
    cnt = {s: n * 7 for s, n in helpers.split_counts(ds).items()}
    for e in range(3):
        want = g.train_epoch() + g.eval(2)
        print(e + 1, lines[e], want)
        if e == 0:
            assert abs(lines[0][0] - want[0]) <= 1e-6 * abs(want[0]), (lines[0], want)
        helpers.assert_line_close(lines[e], want, cnt, what=f"epoch {e + 1}")
    g.close()


def test_cli_multilabel(cora_labels, pgcn, tmp_path):
    """gcn-par NAME multilabel=1 (command line, or the parameter file) reads data/NAME.labels,
    prints the usual epoch lines, saves a checkpoint with the flag bit, and predict= writes
    `node id id ...` -- the engine's thresholded prediction after the same epochs."""
    root, name, ds, _ = cora_labels
    exe = os.path.join(BIN, "gcn-par")
    params = tmp_path / "params.txt"
    params.write_text("multilabel = 1\n")
    outs = {}
    for how, extra in (("arg", ["multilabel=1"]), ("file", [f"file={params}"])):
        ck, pred = str(tmp_path / f"{how}.pgcnck"), str(tmp_path / f"{how}.pred")
        r = subprocess.run([exe, name, f"root={root}", "epochs=3", f"save={ck}",
                            f"predict={pred}"] + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        assert pgcn.checkpoint_flags(ck) == pgcn.CKPT_MULTILABEL
        epochs = [helpers.parse_line(ln) for ln in r.stdout.splitlines()
                  if ln.startswith("epoch=")]
        for e in epochs:
            del e["time"]
        assert len(epochs) == 3 and "test_loss=" in r.stdout
        outs[how] = (epochs, open(pred).read())
    assert outs["arg"] == outs["file"]
    g = pgcn.GCN(pgcn.make_params(ds, multilabel=True), ds)
    for e in range(3):
        want = g.train_epoch() + g.eval(2)
        got = outs["arg"][0][e]
        ours = (got["train_loss"], got["train_acc"], got["val_loss"], got["val_acc"])
        np.testing.assert_allclose(ours, want, atol=1e-5)  # (%.5f)
    g.eval(3)
    want_pred = g.predict_multilabel()
    g.close()
    rows = outs["arg"][1].splitlines()
    assert len(rows) == ds.num_nodes
    got_pred = np.zeros_like(want_pred)
    for i, ln in enumerate(rows):
        tok = [int(t) for t in ln.split()]
        assert tok[0] == i
        got_pred[i, tok[1:]] = True
    np.testing.assert_array_equal(got_pred, want_pred)
    # without the labels file the run fails
    os.rename(os.path.join(root, "data", name + ".labels"), os.path.join(root, "data", "x"))
    try:
        r = subprocess.run([exe, name, f"root={root}", "epochs=1", "multilabel=1"],
                           capture_output=True, text=True, timeout=120)
        assert r.returncode != 0 and "labels" in r.stderr
    finally:
        os.rename(os.path.join(root, "data", "x"), os.path.join(root, "data", name + ".labels"))
