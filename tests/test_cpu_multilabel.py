"""Multi-label classification (pgcn_params.multilabel), the parts that need no device: the
parameter struct's layout, the labels sidecar file, the dataset view, the checkpoint header's
flag bit and the argument checks of the three kernel entries."""
import ctypes
import re
import struct

import numpy as np
import pytest

import helpers
from test_cpu_residual import make_checkpoint


def _field_names(pgcn):
    return [f[0] for f in pgcn.PgcnParams._fields_]


def test_params_layout(pgcn):
    """multilabel sits right after reassociate_last and right before seed -- in the Python
    struct and in the C header -- defaults to 0, and the two layouts have the same size."""
    names = _field_names(pgcn)
    at = names.index("multilabel")
    assert names[at - 1] == "reassociate_last" and names[at + 1] == "seed"
    assert names[-3:] == ["seed", "layer_norm", "residual"]
    assert ctypes.sizeof(pgcn.PgcnParams) == pgcn.lib.pgcn_params_sizeof()
    text = open(helpers.REPO + "/include/pgcn.h").read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    body = text[text.index("typedef struct {\n  int num_nodes, input_dim"):text.index("} pgcn_params;")]
    members = re.findall(r"(\w+)(?:\[\w+\])?\s*[;,]", body)
    i = members.index("multilabel")
    assert members[i - 1] == "reassociate_last" and members[i + 1] == "seed"
    p = pgcn.PgcnParams()
    for f in names:  # poison: the default must write every member
        if f not in ("hidden_dims", "dropouts"):
            setattr(p, f, 77)
    pgcn.lib.pgcn_params_default(ctypes.byref(p))
    assert p.multilabel == 0 and p.seed == 0 and p.reassociate_last == 1
    assert p.layer_norm == 0 and p.residual == 0


def test_make_params_keyword(pgcn):
    ds = pgcn.Dataset.synthetic(40, 6, 3, 60, 1)
    assert pgcn.make_params(ds).multilabel == 0
    p = pgcn.make_params(ds, multilabel=True, seed=5, residual=True)
    assert p.multilabel == 1 and p.seed == 5 and p.residual == 1 and p.layer_norm == 0


def _write_labels(path, Y):
    with open(path, "w") as f:
        for row in Y:
            f.write(" ".join(str(j) for j in np.nonzero(row)[0]) + "\n")


def test_labels_file_round_trip(pgcn, tmp_path):
    """Written from a seeded matrix (one node with no class: an empty line) and read back:
    the bit matrix, output_dim from the largest id or as given, every node labelled."""
    n, c = 50, 37
    rng = np.random.default_rng(3)
    Y = rng.random((n, c)) < 0.2
    Y[7] = False
    Y[:, c - 1] = False
    Y[11, c - 2] = True  # the largest id present: c - 2
    path = str(tmp_path / "a.labels")
    _write_labels(path, Y)
    assert open(path).read().split("\n")[7] == ""
    ds = pgcn.Dataset.synthetic(n, 6, 3, 80, 2)
    assert ds.label_bits is None and ds.label_words == 0 and not ds.view.label_bits
    ds.load_labels(path)
    assert ds.output_dim == c - 1 and ds.label_words == 2
    np.testing.assert_array_equal(pgcn.unpack_label_bits(ds.label_bits, c - 1), Y[:, :c - 1])
    assert (np.asarray(ds.label) >= 0).all()
    ds.load_labels(path, num_classes=c)
    assert ds.output_dim == c and ds.label_bits.shape == (n, 2)
    np.testing.assert_array_equal(pgcn.unpack_label_bits(ds.label_bits, c), Y)
    ds.load_labels(path, num_classes=128)
    assert ds.output_dim == 128 and ds.label_bits.shape == (n, 4)
    assert not ds.label_bits[:, 2:].any()


def test_labels_file_errors(pgcn, tmp_path):
    n = 6
    ds = pgcn.Dataset.synthetic(n, 4, 3, 8, 1)
    good = ["0 1", "", "2", "1 2", "0", "3"]

    def status(lines, num_classes=0, name="x.labels"):
        path = tmp_path / name
        path.write_text("".join(ln + "\n" for ln in lines))
        return pgcn.lib.pgcn_dataset_load_labels(ds._h, str(path).encode(), num_classes)
    assert status(good) == pgcn.PGCN_OK
    IO = pgcn.PGCN_E_IO
    assert pgcn.lib.pgcn_dataset_load_labels(ds._h, str(tmp_path / "missing").encode(), 0) == IO
    assert status(good[:-1]) == IO and status(good + ["1"]) == IO  # line count
    assert status(good[:2] + ["x"] + good[3:]) == IO               # not a number
    assert status(good[:2] + ["1,2"] + good[3:]) == IO
    assert status(good[:2] + ["-1"] + good[3:]) == IO
    assert status(good[:2] + ["1.5"] + good[3:]) == IO
    assert status(good, num_classes=3) == IO                       # id 3 outside [0, 3)
    assert status(good, num_classes=4) == pgcn.PGCN_OK
    assert status(good[:2] + ["128"] + good[3:]) == IO             # outside [0, 128)
    assert status(good[:2] + ["127"] + good[3:]) == pgcn.PGCN_OK
    assert status(good, num_classes=129) == pgcn.PGCN_E_INVALID
    assert status(good, num_classes=-1) == pgcn.PGCN_E_INVALID
    with pytest.raises(pgcn.PgcnError) as e:
        ds.load_labels(str(tmp_path / "missing"))
    assert e.value.status == IO


def test_dataset_view_and_save_refusal(pgcn, tmp_path):
    """set_multilabel fills the view's two trailing members and output_dim; labelled nodes stay
    labelled; pgcn_dataset_save refuses such a dataset (the cache format has no bit matrix)."""
    n, c = 30, 41
    ds = pgcn.Dataset.synthetic(n, 5, 4, 40, 9)
    before = np.asarray(ds.label).copy()
    ds.save(str(tmp_path / "single.pgcnbin"))
    Y = np.random.default_rng(1).random((n, c)) < 0.3
    ds.set_multilabel(Y)
    assert ds.output_dim == c and ds.view.label_words == 2 and bool(ds.view.label_bits)
    np.testing.assert_array_equal(ds.label_bits, pgcn.pack_label_bits(Y))
    np.testing.assert_array_equal(pgcn.unpack_label_bits(ds.label_bits, c), Y)
    assert not (ds.label_bits[:, 1] >> np.uint32(c - 32)).any()  # bits >= c are zero
    np.testing.assert_array_equal((np.asarray(ds.label) >= 0), before >= 0)
    with pytest.raises(pgcn.PgcnError) as e:
        ds.save(str(tmp_path / "multi.pgcnbin"))
    assert e.value.status == pgcn.PGCN_E_INVALID
    lib, INV = pgcn.lib, pgcn.PGCN_E_INVALID
    bits = pgcn.pack_label_bits(Y)
    vp = bits.ctypes.data_as(ctypes.c_void_p)
    assert lib.pgcn_dataset_set_multilabel(ds._h, vp, 1, c) == INV   # wrong words
    assert lib.pgcn_dataset_set_multilabel(ds._h, vp, 2, 129) == INV
    assert lib.pgcn_dataset_set_multilabel(ds._h, vp, 2, 0) == INV
    assert lib.pgcn_dataset_set_multilabel(ds._h, None, 2, c) == INV
    assert lib.pgcn_dataset_set_multilabel(ds._h, vp, 2, c - 9) == INV  # bits >= c set
    with pytest.raises(ValueError):
        ds.set_multilabel(Y[:-1])


def test_f1_scores(pgcn):
    counts = np.array([[5, 0, 2, 0], [1, 0, 3, 4], [2, 0, 0, 1]])
    micro, macro = pgcn.f1_scores(counts)
    assert micro == pytest.approx(2 * 7 / (2 * 7 + 8 + 3), abs=1e-15)
    per = [10 / 13, 0.0, 4 / 7, 0.0]
    assert macro == pytest.approx(sum(per) / 4, abs=1e-15)
    assert pgcn.f1_scores(np.zeros((3, 5))) == (0.0, 0.0)


def test_checkpoint_flag_bit(pgcn, tmp_path):
    """Bit 2 (value 4, CKPT_MULTILABEL) of a hand-written version-1 header is known, alone or
    with the residual bit; bit 3 (value 8) still is not."""
    assert pgcn.CKPT_MULTILABEL == 4
    for flags in (4, 5):
        path = tmp_path / f"f{flags}"
        path.write_bytes(make_checkpoint(flags))
        assert pgcn.checkpoint_flags(str(path)) == flags
        assert pgcn.checkpoint_info(str(path))["version"] == 1
    for flags in (8, 12):
        path = tmp_path / f"f{flags}"
        path.write_bytes(make_checkpoint(flags))
        for fn in (pgcn.checkpoint_info, pgcn.checkpoint_flags):
            with pytest.raises(pgcn.PgcnError) as e:
                fn(str(path))
            assert e.value.status == pgcn.PGCN_E_IO


def test_kernel_entry_checks_without_device(pgcn):
    """Bad arguments are refused before the device is looked for: c outside [1, 128], ld < c or
    not a multiple of 4, words != ceil(c / 32), count < 1; n == 0 is OK and launches nothing."""
    a = np.zeros(64, np.float32)
    vp = a.ctypes.data_as(ctypes.c_void_p)
    lib, INV, OK = pgcn.lib, pgcn.PGCN_E_INVALID, pgcn.PGCN_OK

    def bce(ld=8, words=1, n=2, c=5, count=10):
        return lib.pgcn_bce_fwd(vp, ld, vp, vp, vp, words, n, c, count, 1, vp, None)
    assert bce(c=0) == INV and bce(c=129, ld=132, words=5) == INV
    assert bce(ld=4) == INV and bce(ld=6) == INV and bce(ld=10) == INV
    assert bce(words=2) == INV and bce(c=33, ld=36, words=1) == INV and bce(words=0) == INV
    assert bce(count=0) == INV and bce(count=-3) == INV and bce(n=-1) == INV
    assert bce(n=0) == OK

    def pred(ld=8, n=2, c=5, words=1, probs=vp, ld_probs=8):
        return lib.pgcn_predict_multilabel_rows(vp, ld, n, c, vp, words, probs, ld_probs, None)
    assert pred(c=0) == INV and pred(c=129, ld=132, words=5) == INV
    assert pred(ld=4) == INV and pred(ld=6) == INV and pred(words=2) == INV
    assert pred(ld_probs=4) == INV and pred(ld_probs=6) == INV and pred(n=-1) == INV
    assert pred(n=0) == OK and pred(n=0, probs=None, ld_probs=0) == OK

    def cnt(n=2, c=5, words=1):
        return lib.pgcn_multilabel_counts(vp, vp, vp, n, c, words, vp, None)
    assert cnt(c=0) == INV and cnt(c=129, words=5) == INV and cnt(words=2) == INV
    assert cnt(c=64, words=1) == INV and cnt(n=-1) == INV
    import torch
    if torch.cuda.is_available():
        return  # with a device the launches are covered by tests/test_gpu_multilabel_kernels.py
    ND = pgcn.PGCN_E_NODEVICE
    assert bce() == ND and pred() == ND and cnt() == ND
