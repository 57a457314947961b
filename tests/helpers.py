"""Test helpers: load the engine package, the C oracle, the reference build, the fixtures.

The oracle (oracle/liboracle.so, oracle/_ref/libhpdga_ref.so) is test infrastructure: it is
loaded here, by __graft_entry__.smoke() and by bench.py's cpu_baseline leg only.
"""
import contextlib
import ctypes
import gzip
import importlib.util
import os
import shutil
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")
ORACLE_SO = os.path.join(REPO, "oracle", "liboracle.so")
REF_SO = os.path.join(REPO, "oracle", "_ref", "libhpdga_ref.so")

_pkg = None


def pgcn():
    """The engine's Python glue (parallel-gcn_amd/__init__.py); raises if not built."""
    global _pkg
    if _pkg is None:
        path = os.path.join(REPO, "parallel-gcn_amd", "__init__.py")
        spec = importlib.util.spec_from_file_location("pgcn_amd", path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules["pgcn_amd"] = mod
        spec.loader.exec_module(mod)
        _pkg = mod
    return _pkg


# --------------------------------------------------------------------------- oracle
class OrParams(ctypes.Structure):
    _fields_ = [("num_nodes", ctypes.c_int), ("input_dim", ctypes.c_int),
                ("output_dim", ctypes.c_int), ("n_layers", ctypes.c_int),
                ("hidden_dims", ctypes.c_int * 16), ("dropouts", ctypes.c_float * 16),
                ("lr", ctypes.c_float), ("weight_decay", ctypes.c_float),
                ("beta1", ctypes.c_float), ("beta2", ctypes.c_float), ("eps", ctypes.c_float),
                ("seed", ctypes.c_uint)]


_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        if not os.path.exists(ORACLE_SO):
            import subprocess
            subprocess.run(["make", "-C", os.path.join(REPO, "oracle")], check=True,
                           stdout=subprocess.DEVNULL)
        lib = ctypes.CDLL(ORACLE_SO)
        vp, ip, fp = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        lib.or_gcn_create.restype = vp
        lib.or_gcn_create.argtypes = [ctypes.POINTER(OrParams)] + [vp] * 7
        lib.or_gcn_get_var.restype = ctypes.c_long
        lib.or_gcn_get_var.argtypes = [vp, ip, ip, vp]
        lib.or_gcn_train_epoch.argtypes = [vp, vp]
        lib.or_gcn_eval.argtypes = [vp, ip, vp]
        lib.or_gcn_free.argtypes = [vp]
        lib.or_gcn_rng_state.argtypes = [vp, vp]
        lib.or_gcn_num_vars.argtypes = [vp]
        lib.or_rng_next.restype = ctypes.c_uint32
        lib.or_rng_next.argtypes = [vp]
        lib.or_graph_coef.restype = fp
        lib.or_xent_fwd.restype = fp
        lib.or_accuracy.restype = fp
        lib.or_l2_penalty.restype = fp
        lib.or_adam_step_size.restype = fp
        lib.or_adam_step_size.argtypes = [fp, fp, fp, ip]
        _oracle = lib
    return _oracle


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class OracleGCN:
    """The C restatement of hpdga's GCN (L layers; L = 2 is exactly the reference)."""

    def __init__(self, ds, hidden_dims=(16,), dropouts=(0.5, 0.5), lr=0.01, wd=5e-4, seed=0):
        lib = oracle()
        p = OrParams()
        p.num_nodes, p.input_dim, p.output_dim = ds["n"], ds["f"], ds["c"]
        p.n_layers = len(hidden_dims) + 1
        for i, h in enumerate(hidden_dims):
            p.hidden_dims[i] = h
        for i, d in enumerate(dropouts):
            p.dropouts[i] = d
        p.lr, p.weight_decay, p.beta1, p.beta2, p.eps = lr, wd, 0.9, 0.999, 1e-8
        p.seed = seed
        self._keep = [np.ascontiguousarray(ds[k]) for k in
                      ("graph_indptr", "graph_indices", "feat_indptr", "feat_indices",
                       "feat_values", "label", "split")]
        self.h = lib.or_gcn_create(ctypes.byref(p), *[ptr(a) for a in self._keep])
        self.lib = lib

    def train_epoch(self):
        out = np.zeros(2, np.float32)
        self.lib.or_gcn_train_epoch(self.h, ptr(out))
        return float(out[0]), float(out[1])

    def eval(self, split):
        out = np.zeros(2, np.float32)
        self.lib.or_gcn_eval(self.h, split, ptr(out))
        return float(out[0]), float(out[1])

    def logits(self):
        """The output variable (the logits of the last forward, max-shifted on labelled rows)."""
        return self.var(self.lib.or_gcn_num_vars(self.h) - 1)

    def epoch_with_ties(self, label, split, c, tol=1e-5):
        """train_epoch() + eval(2), and the near-tied rows of each pass's logits (near_ties):
        the accuracy tolerance of assert_line_close."""
        tr = self.train_epoch()
        t1 = near_ties(self.logits(), label, split, 1, c, tol)
        ev = self.eval(2)
        t2 = near_ties(self.logits(), label, split, 2, c, tol)
        return tr + ev, {1: t1, 2: t2}

    def eval_with_ties(self, split_id, label, split, c, tol=1e-5):
        """eval(split_id) and the near-tied rows of its logits."""
        r = self.eval(split_id)
        return r, near_ties(self.logits(), label, split, split_id, c, tol)

    def var(self, idx, which=0):
        n = self.lib.or_gcn_get_var(self.h, idx, which, None)
        out = np.zeros(max(n, 0), np.float32)
        if n > 0:
            self.lib.or_gcn_get_var(self.h, idx, which, ptr(out))
        return out

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.or_gcn_free(self.h)
            self.h = None


def oracle_run(ds, epochs, **kw):
    """The oracle's epochs x (train_epoch + eval(2)), then eval(3), with the near-tied rows of
    every pass (the accuracy tolerance), the logits after eval(3) and the weights."""
    ref = OracleGCN(ds_dict(ds), **kw)
    c = ds.output_dim
    runs = [ref.epoch_with_ties(ds.label, ds.split, c) for _ in range(epochs)]
    test, tt = ref.eval_with_ties(3, ds.label, ds.split, c)
    n = ref.lib.or_gcn_num_vars(ref.h)
    return dict(lines=[r[0] for r in runs], ties=[r[1] for r in runs], test=test,
                test_ties={1: tt, 2: tt}, logits=ref.logits(), w1=ref.var(2), w2=ref.var(n - 2))


# reddit's feature width and class count (the X-stream ring kernels), ~3.1 M adjacency slots
RW_GRAPH = dict(n=100000, f=602, c=41, edges=1500000, seed=41)


def ds_dict(ds):
    """pgcn Dataset -> plain dict of arrays for the oracle."""
    return {"n": ds.num_nodes, "f": ds.input_dim, "c": ds.output_dim,
            "graph_indptr": ds.graph_indptr, "graph_indices": ds.graph_indices,
            "feat_indptr": ds.feat_indptr, "feat_indices": ds.feat_indices,
            "feat_values": ds.feat_values, "label": ds.label, "split": ds.split}


# --------------------------------------------------------------------------- reference
_ref = None


def ref_lib():
    """oracle/_ref/libhpdga_ref.so: the reference's own sequential sources (None if absent)."""
    global _ref
    if _ref is None and os.path.exists(REF_SO):
        lib = ctypes.CDLL(REF_SO)
        vp, ip, fp, ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong
        lib.ref_create.restype = vp
        lib.ref_create.argtypes = [ip, ip, ip, ip, fp, fp, fp, ip, vp, vp, ll, vp, vp, vp, ll, vp, vp]
        lib.ref_train_epoch.argtypes = [vp, vp]
        lib.ref_eval.argtypes = [vp, ip, vp]
        lib.ref_get_var.restype = ll
        lib.ref_get_var.argtypes = [vp, ip, ip, vp]
        lib.ref_free.argtypes = [vp]
        _ref = lib
    return _ref


# --------------------------------------------------------------------------- fixtures
def golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def golden_lines(name):
    return open(os.path.join(GOLDEN, f"{name}_epoch_lines.txt")).read().splitlines()


def materialize_dataset(name, dest):
    """Write data/<ds>.{graph,split,svmlight} under dest from the committed fixtures.
    name: cora | citeseer | pubmed_synth (pubmed graph/split + seeded synthetic features)."""
    data = os.path.join(dest, "data")
    os.makedirs(data, exist_ok=True)
    src = os.path.join(GOLDEN, "data")
    if name == "pubmed_synth":
        for ext in ("graph", "split"):
            with gzip.open(os.path.join(src, f"pubmed.{ext}.gz")) as fi, \
                    open(os.path.join(data, f"pubmed.{ext}"), "wb") as fo:
                shutil.copyfileobj(fi, fo)
        sys.path.insert(0, GOLDEN)
        import make_golden
        make_golden.pubmed_synth_svmlight(os.path.join(data, "pubmed.svmlight"))
        return "pubmed"
    for ext in ("graph", "split", "svmlight"):
        with gzip.open(os.path.join(src, f"{name}.{ext}.gz")) as fi, \
                open(os.path.join(data, f"{name}.{ext}"), "wb") as fo:
            shutil.copyfileobj(fi, fo)
    return name


def parse_line(line):
    out = {}
    for tok in line.split():
        k, v = tok.split("=")
        out[k] = float(v)
    return out


# --------------------------------------------------------------------------- graph builders
def random_graph(n, avg_deg, seed, hubs=0, hub_deg=0, empty_rows=0):
    """Symmetric random graph in the hpdga CSR form (self loop first, duplicates allowed).
    empty_rows = k > 0: every k-th row (i % k == k - 1) loses all its slots, its self loop
    included (the pattern is then no longer symmetric: for pgcn_graph_create_values)."""
    rng = np.random.default_rng(seed)
    m = n * avg_deg // 2
    u = rng.integers(0, n, m)
    v = rng.integers(0, n, m)
    if hubs:
        hu = rng.integers(0, n, hubs)
        extra_u = np.repeat(hu, hub_deg)
        extra_v = rng.integers(0, n, hubs * hub_deg)
        u, v = np.concatenate([u, extra_u]), np.concatenate([v, extra_v])
    keep = u != v
    u, v = u[keep], v[keep]
    src = np.concatenate([u, v, np.arange(n)])
    dst = np.concatenate([v, u, np.arange(n)])
    if empty_rows:
        keep = src % empty_rows != empty_rows - 1
        src, dst = src[keep], dst[keep]
    order = np.lexsort((dst, src != dst, src))  # self loop first within a row
    src, dst = src[order], dst[order]
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, src + 1, 1)
    indptr = np.cumsum(indptr).astype(np.int32)
    return indptr, dst.astype(np.int32)


def csr_reference(indptr, indices, vals, x, n_cols=None):
    """(A x, |A| |x|) in float64 through scipy's CSR product (duplicates add up): GraphSum's
    reference and the scale of its fp32 reordering error, per output element."""
    import scipy.sparse as sps
    shape = (len(indptr) - 1, x.shape[0] if n_cols is None else n_cols)
    v64 = np.asarray(vals, np.float64)
    x64 = np.asarray(x, np.float64)
    a = sps.csr_matrix((v64, indices, indptr), shape=shape)
    b = sps.csr_matrix((np.abs(v64), indices, indptr), shape=shape)
    return a @ x64, b @ np.abs(x64)


# --------------------------------------------------------------------------- GEMM references
def mask_bits(mask_words, n):
    """the first n bits of a bitmap of uint64 words (bit i = word i / 64, bit i % 64)"""
    b = np.unpackbits(mask_words.view(np.uint8), bitorder="little")
    return b[:n].astype(bool)


def mask_window(mask, base, M, K, mask_ld=None):
    """bits base + m * mask_ld + k (mask_ld = K when not given) of a flat bitmap as an (M, K)
    bool array"""
    ld = K if mask_ld is None else mask_ld
    if M == 0:
        return np.zeros((0, K), bool)
    bits = mask_bits(mask, base + (M - 1) * ld + K)[base:]
    bits = np.concatenate([bits, np.zeros(M * ld - len(bits), bool)])
    return bits.reshape(M, ld)[:, :K]


def nibble_mask_ref(mask, base, M, K, mask_ld=None):
    """maskT[m][j] nibble c = keep bits of (m, 64c + 4j .. +3), zero past K (numpy)"""
    bits = np.zeros((M, 1024), np.uint64)
    bits[:, :K] = mask_window(mask, base, M, K, mask_ld)
    nib = bits.reshape(M, 16, 16, 4)  # [m][c][j][t]: k = 64c + 4j + t
    vals = (nib << np.arange(4, dtype=np.uint64)).sum(-1)  # [m][c][j]
    out = np.zeros((M, 16), np.uint64)
    for c in range(16):
        out |= vals[:, c, :] << np.uint64(4 * c)
    return out


def dropped64(A, K, keep=None, scale=1.0):
    """drop(A)[:, :K] in float64: kept entries (keep, an (M, K) bool array; None: all) times
    scale, the others zero"""
    Ae = A[:, :K].astype(np.float64)
    return Ae if keep is None else Ae * np.where(keep, scale, 0.0)


def product_ref(Ae, B):
    """(Ae B, |Ae| |B|) in float64: a product's reference and, per output element, the sum of
    its terms' magnitudes -- the scale of an fp32 sum's reordering error (the GEMM tests bound
    |got - ref| by 1e-5 of it)"""
    B64 = B.astype(np.float64)
    return Ae @ B64, np.abs(Ae) @ np.abs(B64)


# --------------------------------------------------------------------------- engine knobs
# pgcn_debug_set defaults of the engine (include/pgcn.h; parallel-gcn_amd/csrc/knobs.hpp, whose
# table test_cpu_host.py compares with this one through pgcn_debug_knob)
ENGINE_DEFAULTS = {"train_ahead": 1, "split_rows": 0, "split_cols": 1, "eval_ax": 1,
                   "epoch_graph": 0, "fuse_epilogue": 15, "fuse_output": 2, "mm_side": 0,
                   "xstream_ring": 1, "lds_min_kb": -1, "lds_blocks": 0,
                   "parse_threads": 0, "gs_split": 3, "gs_item_iters": 0, "co_draw": 2,
                   "gs_orig_cols": 1, "sparse_dual": 1, "eval_tail": 0, "gs16_gather": 0,
                   "peer_uncached": 0, "ring_pair": 0, "tn_fold": 1,
                   "fuse_finish": 1, "mask_per": 0,
                   "ring_window": 0, "csc_tree": 0, "mask_adam": 1,
                   "reassoc_small": 1, "defer_wgrad": 1,
                   "mask_xstream": 0}


@contextlib.contextmanager
def knobs(pg, **kw):
    """Sets engine knobs for the engines built inside the block, restores the defaults."""
    try:
        for k, v in kw.items():
            assert pg.lib.pgcn_debug_set(k.encode(), int(v)) == 0, k
        yield
    finally:
        for k in kw:
            pg.lib.pgcn_debug_set(k.encode(), ENGINE_DEFAULTS.get(k, 0))


def split_counts(ds):
    lab, sp = np.asarray(ds.label), np.asarray(ds.split)
    return {s: int(((sp == s) & (lab >= 0)).sum()) for s in (1, 2, 3)}


def near_ties(logits, label, split, sp, c, tol=1e-5):
    """Labelled rows of split `sp` whose true-class logit is within tol (relative to the row's
    largest |logit|, at least tol absolute) of the largest other logit in the oracle's logits:
    the only rows whose correct/wrong verdict a last-bits difference of the logits can flip."""
    z = np.asarray(logits, np.float64).reshape(-1, c)
    lab, spl = np.asarray(label), np.asarray(split)
    rows = np.nonzero((spl[:len(z)] == sp) & (lab[:len(z)] >= 0))[0]
    if len(rows) == 0:
        return 0
    zr, lr = z[rows], lab[rows]
    idx = np.arange(len(rows))
    zl = zr[idx, lr].copy()
    zr[idx, lr] = -np.inf
    gap = np.abs(zl - zr.max(axis=1))
    zr[idx, lr] = zl
    return int((gap <= tol * np.maximum(1.0, np.abs(zr).max(axis=1))).sum())


# The near-tie band of the 4-layer hidden-128 models: their logits go through 4 GraphSums and 4
# contractions, whose fp32 summation order (ring schedule, column blocks, ranks) moves them by
# a few 1e-6 relative; the band is the north star's 1e-4 on the logits (r04: one validation row
# of 14,321 flipped at world 8 with 2-layer-sized 1e-5 band, the losses agreeing to 5e-6)
DEEP_TIE_TOL = 1e-4


def assert_line_close(ours, want, counts, rtol=1e-4, what="", ties=None):
    """One epoch line (train_loss, train_acc, val_loss, val_acc) against the oracle's: losses
    within rtol (the north star's 1e-4); accuracies within `ties[split]` rows (the oracle's
    near-tied rows of that pass, near_ties) when given, else within 2 rows."""
    for k in (0, 2):
        assert abs(ours[k] - want[k]) <= rtol * abs(want[k]), (what, k, ours, want)
    for k, sp in ((1, 1), (3, 2)):
        allowed = 2 if ties is None else ties[sp]
        assert abs(ours[k] - want[k]) * counts[sp] <= allowed + 1e-3, \
            (what, k, ours, want, f"allowed {allowed} rows")
