"""include/pgcn.hpp's ResidualConnection from a C++ program (tests/cpp/test_residual_api.cpp):
a 4-layer (16,16,16) cora model assembled from api modules with two ResidualConnections,
every module's backward called in reverse order, against the engine's residual model."""
import os
import subprocess

import numpy as np
import pytest

import helpers

pytestmark = pytest.mark.gpu

EXE = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "test_residual_api")


def test_cpp_residual_modules_match_engine(datasets, pgcn):
    """10 epoch lines of the hand-assembled model (the reference's module order, output layer
    as Â (H W)) against pgcn.GCN(residual=1) in the same order: losses at 1e-4, accuracies within
    2 rows.  The dropout masks are the same stream positions, so the runs see the same masks."""
    root, names = datasets
    out = subprocess.run([EXE, root, names["cora"], "10"], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = np.array([[float(x) for x in ln.split()[1:]] for ln in out.stdout.splitlines()
                      if ln.startswith("epoch=")], np.float64)
    assert lines.shape == (10, 4)
    ds = pgcn.Dataset.load(root, names["cora"])
    g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=(16, 16, 16), dropouts=(0.5,) * 4,
                                  residual=True, reassociate_last=False), ds)
    assert g.query("residual_layers") == 2
    cnt = helpers.split_counts(ds)
    for e in range(10):
        want = g.train_epoch() + g.eval(2)
        print(e + 1, lines[e], want)
        helpers.assert_line_close(lines[e], want, cnt, what=f"epoch {e + 1}")
    g.close()


def test_cpp_residual_size_mismatch_throws(datasets):
    root, names = datasets
    out = subprocess.run([EXE, "mismatch", root, names["cora"]], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0 and "mismatch ok" in out.stdout, out.stdout + out.stderr[-2000:]


def test_cli_residual_key(datasets, pgcn, tmp_path):
    """gcn-par takes residual=1 from the parameter file (beside n_layers) and from the command
    line, which wins: the saved checkpoint carries the flag, and its weights are the engine's."""
    root, names = datasets
    exe = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "gcn-par")
    params = tmp_path / "params.txt"
    params.write_text("n_layers = 4\nhidden_dims = 16,16,16\ndropouts = 0.5,0.5,0.5,0.5\n"
                      "residual = 1\n")
    ck = {}
    for name, extra in (("file", []), ("off", ["residual=0"])):
        ck[name] = str(tmp_path / f"{name}.pgcnck")
        r = subprocess.run([exe, names["cora"], f"root={root}", f"file={params}", "epochs=3",
                            f"save={ck[name]}"] + extra, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
    assert pgcn.checkpoint_flags(ck["file"]) == pgcn.CKPT_RESIDUAL
    assert pgcn.checkpoint_flags(ck["off"]) == 0
    ds = pgcn.Dataset.load(root, names["cora"])
    for name, res in (("file", True), ("off", False)):
        g = pgcn.GCN(pgcn.make_params(ds, hidden_dims=(16, 16, 16), dropouts=(0.5,) * 4,
                                      residual=res), ds)
        for _ in range(3):
            g.train_epoch()
            g.eval(2)
        twin = pgcn.GCN(pgcn.make_params(ds, hidden_dims=(16, 16, 16), dropouts=(0.5,) * 4,
                                         residual=res), ds)
        twin.load(ck[name])
        for l in range(4):
            np.testing.assert_array_equal(g.get_var(2 + 3 * l), twin.get_var(2 + 3 * l))
        g.close()
        twin.close()
