"""Host-side (no GPU) tests: the C ABI library, the kept hpdga loader, the RNG jump-ahead that
drives the device dropout masks, the edge-cut partition plan and the synthetic generator.

All run on CPU: libpgcn.so is loaded but no device call is made."""
import ctypes
import hashlib
import json
import os
import re

import numpy as np
import pytest

import helpers

HEADER = os.path.join(helpers.REPO, "include", "pgcn.h")


def header_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pgcn_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_header_symbol(pgcn):
    decl = header_functions()
    assert len(decl) >= 40
    raw = ctypes.CDLL(pgcn.LIB_PATH)
    missing = [s for s in decl if not hasattr(raw, s)]
    assert not missing, f"declared in include/pgcn.h but not exported: {missing}"
    assert sorted(pgcn.EXPORTED) == decl, "python glue and header disagree"


def test_status_strings(pgcn):
    for st in (pgcn.PGCN_OK, pgcn.PGCN_E_INVALID, pgcn.PGCN_E_NOMEM, pgcn.PGCN_E_IO,
               pgcn.PGCN_E_COMM, pgcn.PGCN_E_NODEVICE):
        assert pgcn.lib.pgcn_status_string(st)
    assert pgcn.lib.pgcn_version() > 0


def test_create_without_device_fails_loudly(pgcn, loaded):
    """No CPU fallback: creating an engine on a host without a HIP device must raise."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    ds = loaded["cora"]
    with pytest.raises(pgcn.PgcnError):
        pgcn.GCN(pgcn.make_params(ds), ds)
    # the peer-mapped engine: NODEVICE before its host all-gather is ever called
    calls = []

    def ag(data):
        calls.append(data)
        return [data, data]
    with pytest.raises(pgcn.PgcnError) as e:
        pgcn.GCN(pgcn.make_params(ds), ds, rank=0, world=2, allgather=ag)
    assert e.value.status == pgcn.PGCN_E_NODEVICE and not calls


def test_peer_allgather_callback(pgcn):
    """pgcn_allgather_fn over a Python all-gather (what bench.py hands the peer engine): the
    ranks' byte strings land in rank order; a failing or short all-gather reports -1."""
    import ctypes
    fn = pgcn.peer_allgather_fn(lambda d: [d, bytes(reversed(d)), d])
    mine = ctypes.create_string_buffer(b"abcd", 4)
    out = ctypes.create_string_buffer(12)
    assert fn(ctypes.cast(mine, ctypes.c_void_p), 4, ctypes.cast(out, ctypes.c_void_p), None) == 0
    assert out.raw == b"abcddcbaabcd"
    bad = pgcn.peer_allgather_fn(lambda d: [d, d[:2]])
    assert bad(ctypes.cast(mine, ctypes.c_void_p), 4, ctypes.cast(out, ctypes.c_void_p), None) == -1

    def boom(d):
        raise RuntimeError("channel down")
    assert pgcn.peer_allgather_fn(boom)(ctypes.cast(mine, ctypes.c_void_p), 4,
                                        ctypes.cast(out, ctypes.c_void_p), None) == -1


@pytest.mark.parametrize("name", ["cora", "citeseer", "pubmed_synth"])
def test_loader_matches_manifest(loaded, name):
    """The kept hpdga Parser (src/parser.cpp:6-140) yields exactly the arrays the reference
    build parsed (sha256 of the little-endian arrays, tests/golden/manifest.json)."""
    man = json.load(open(os.path.join(helpers.GOLDEN, "manifest.json")))["datasets"][name]["parsed"]
    ds = loaded[name]
    for key, want in man.items():
        a = np.ascontiguousarray(getattr(ds, key))
        assert a.size == want["count"], key
        assert hashlib.sha256(a.tobytes()).hexdigest() == want["sha256"], key


@pytest.mark.parametrize("name,pieces", [("cora", 3), ("citeseer", 7), ("pubmed_synth", 16)])
def test_parallel_parse_matches_manifest(pgcn, tmp_path, name, pieces):
    """The text parse split into line-aligned pieces parsed on several host threads
    (f2: hpdga parser.cpp:18-116 semantics, pieces concatenated in file order) gives the
    manifest's arrays bit for bit (citeseer's empty svmlight lines and explicit self loops
    included), whatever the piece count."""
    man = json.load(open(os.path.join(helpers.GOLDEN, "manifest.json")))["datasets"][name]["parsed"]
    root = str(tmp_path)
    stem = helpers.materialize_dataset(name, root)
    with helpers.knobs(pgcn, parse_threads=pieces):
        ds = pgcn.Dataset.load(root, stem)
    for key, want in man.items():
        a = np.ascontiguousarray(getattr(ds, key))
        assert a.size == want["count"], key
        assert hashlib.sha256(a.tobytes()).hexdigest() == want["sha256"], key


def test_parallel_parse_ragged_text(pgcn, tmp_path):
    """Pieces cut through a ragged file: empty graph lines (a row holding only its self loop),
    empty and label-only svmlight lines, duplicate neighbours, an unterminated last line (dropped,
    hpdga parser.cpp:23-27), more pieces than some files have lines."""
    rng = np.random.default_rng(11)
    n = 3001
    data = tmp_path / "data"
    data.mkdir()
    with open(data / "rag.graph", "w") as f:
        for i in range(n):
            k = 0 if i % 5 == 0 else int(rng.integers(1, 30))
            f.write(" ".join(str(int(x)) for x in rng.integers(0, n, k)) + "\n")
        f.write("7 8 9")  # unterminated: not a node
    with open(data / "rag.svmlight", "w") as f:
        for i in range(n):
            if i % 11 == 3:
                f.write("\n")
            elif i % 13 == 4:
                f.write(f"{i % 5}\n")
            else:
                ks = sorted(set(int(x) for x in rng.integers(0, 300, int(rng.integers(1, 9)))))
                f.write(f"{i % 5} " + " ".join(f"{k}:{rng.standard_normal():.6g}" for k in ks) +
                        "\n")
    with open(data / "rag.split", "w") as f:
        f.write("".join(f"{1 + i % 3}\n" for i in range(n)))
    with helpers.knobs(pgcn, parse_threads=1):
        one = pgcn.Dataset.load(str(tmp_path), "rag")
    assert one.num_nodes == n
    for pieces in (2, 9, 64):
        with helpers.knobs(pgcn, parse_threads=pieces):
            many = pgcn.Dataset.load(str(tmp_path), "rag")
        _same_dataset(one, many)


def test_loader_missing_dataset_raises(pgcn, tmp_path):
    with pytest.raises(pgcn.PgcnError):
        pgcn.Dataset.load(str(tmp_path), "nonexistent")


DS_ARRAYS = ("graph_indptr", "graph_indices", "feat_indptr", "feat_indices", "feat_values",
             "label", "split")


def _same_dataset(a, b):
    assert (a.num_nodes, a.input_dim, a.output_dim) == (b.num_nodes, b.input_dim, b.output_dim)
    for k in DS_ARRAYS:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


@pytest.mark.parametrize("name", ["cora", "citeseer"])
def test_binary_cache_roundtrip(pgcn, name, tmp_path):
    """the binary cache gives the parser's arrays bit for bit; a miss parses
    and writes it, a hit reads it, a touched text file or a corrupted cache falls back to
    the parser (same arrays every time)."""
    import shutil
    root = str(tmp_path)
    dname = helpers.materialize_dataset(name, root)
    text = pgcn.Dataset.load(root, dname)
    d1, hit1 = pgcn.Dataset.load_cached(root, dname)
    cache = os.path.join(root, "data", dname + ".pgcnbin")
    assert not hit1 and os.path.exists(cache)
    d2, hit2 = pgcn.Dataset.load_cached(root, dname)
    assert hit2
    _same_dataset(text, d1)
    _same_dataset(text, d2)
    # a text file changed after the cache was written: stamps differ -> parse again
    gpath = os.path.join(root, "data", dname + ".graph")
    st = os.stat(gpath)
    os.utime(gpath, ns=(st.st_atime_ns, st.st_mtime_ns + 1_000_000_000))
    d3, hit3 = pgcn.Dataset.load_cached(root, dname)
    assert not hit3
    _same_dataset(text, d3)
    # corrupted payload (checksum) and truncated file: rejected, the parser runs
    blob = bytearray(open(cache, "rb").read())
    blob[-5] ^= 0xFF
    open(cache, "wb").write(bytes(blob))
    with pytest.raises(pgcn.PgcnError):
        pgcn.Dataset.load_binary(cache)
    d4, hit4 = pgcn.Dataset.load_cached(root, dname)
    assert not hit4
    _same_dataset(text, d4)
    open(cache, "wb").write(bytes(blob[: len(blob) // 2]))
    with pytest.raises(pgcn.PgcnError):
        pgcn.Dataset.load_binary(cache)
    # save/load_binary of any dataset (a synthetic one too)
    syn = pgcn.Dataset.synthetic(500, 12, 4, 3000, seed=3)
    path = os.path.join(root, "syn.pgcnbin")
    syn.save(path)
    _same_dataset(syn, pgcn.Dataset.load_binary(path))
    shutil.rmtree(os.path.join(root, "data"))
    with pytest.raises(pgcn.PgcnError):
        pgcn.Dataset.load_cached(root, dname)


@pytest.mark.parametrize("k", [0, 1, 2, 63, 64, 1000, 123457])
def test_rng_jump_matches_sequential_draws(pgcn, k):
    """GF(2) jump-ahead (csrc/rng.cpp) == k sequential xorshift128+ draws of the oracle
    (hpdga src/rand.cpp:5-24)."""
    orc = helpers.oracle()
    s = (ctypes.c_uint64 * 2)()
    orc.or_rng_seed(s)
    seed = pgcn.rng_seed()
    assert [int(seed[0]), int(seed[1])] == [s[0], s[1]]
    for _ in range(k):
        orc.or_rng_next(s)
    got = pgcn.rng_jump(seed, k)
    assert [int(got[0]), int(got[1])] == [s[0], s[1]]


def test_rng_jump_table_composes(pgcn):
    """The 16 x 256 byte tables of M^period reproduce rng_jump(state, period) on random states."""
    period = 98765
    t = pgcn.rng_jump_table(period).reshape(16, 256, 2)
    rs = np.random.default_rng(5)
    for _ in range(8):
        st = rs.integers(1, 2**63, size=2, dtype=np.uint64)
        want = pgcn.rng_jump(st, period)
        acc = np.zeros(2, np.uint64)
        bits = int(st[0]) | (int(st[1]) << 64)
        for byte in range(16):
            acc ^= t[byte, (bits >> (8 * byte)) & 0xFF]
        assert [int(acc[0]), int(acc[1])] == [int(want[0]), int(want[1])]


def _coef_matrix(ds):
    """Â as a scipy CSR with the hpdga coefficients (from the oracle's coefficient function)."""
    import scipy.sparse as sp
    ip, ix = ds.graph_indptr, ds.graph_indices
    deg = np.diff(ip).astype(np.int64)
    rows = np.repeat(np.arange(ds.num_nodes), deg)
    vals = np.array([helpers.oracle().or_graph_coef(ip.ctypes.data_as(ctypes.c_void_p),
                                                    int(r), int(c))
                     for r, c in zip(rows[:64], ix[:64])], np.float32)
    dd = (deg[rows] * deg[ix]).astype(np.float32)
    full = (1.0 / np.sqrt(dd).astype(np.float64)).astype(np.float32)
    np.testing.assert_array_equal(full[:64], vals)  # same rounding as the oracle's scalar path
    return sp.csr_matrix((full, ix, ip), shape=(ds.num_nodes, ds.num_nodes))


@pytest.mark.parametrize("world", [1, 2, 3, 8])
def test_partition_bounds_balanced(pgcn, loaded, world):
    ds = loaded["pubmed_synth"]
    ip = ds.graph_indptr
    b, maxrows = pgcn.partition_bounds(ip, world)
    assert b[0] == 0 and b[-1] == ds.num_nodes and np.all(np.diff(b) > 0)
    assert maxrows == np.diff(b).max()
    nnz = np.diff(ip[b])
    # contiguous cuts can miss the ideal by at most one row's worth of slots
    assert nnz.max() <= ip[-1] / world + np.diff(ip).max() + 1


@pytest.mark.parametrize("world", [2, 3])
def test_partition_subgraphs_recompose_graphsum(pgcn, loaded, world):
    """sum over ranks of (rank's column block of Â) x H[rank rows] == Â H, in the padded row
    layout the reduce-scatter consumes."""
    ds = loaded["cora"]
    A = _coef_matrix(ds)
    b, maxrows = pgcn.partition_bounds(ds.graph_indptr, world)
    H = np.random.default_rng(0).standard_normal((ds.num_nodes, 7)).astype(np.float32)
    acc = np.zeros((world * maxrows, 7), np.float64)
    total = 0
    for r in range(world):
        sp_, si, sv = pgcn.partition_subgraph(ds.graph_indptr, ds.graph_indices, world, r)
        total += len(si)
        lo, hi = b[r], b[r + 1]
        assert si.size == 0 or (si.min() >= 0 and si.max() < hi - lo)
        import scipy.sparse as sps
        blk = sps.csr_matrix((sv, si, sp_), shape=(world * maxrows, hi - lo))
        acc += blk @ H[lo:hi].astype(np.float64)
    assert total == ds.graph_indptr[-1]
    want = A.astype(np.float64) @ H.astype(np.float64)
    for r in range(world):
        lo, hi = b[r], b[r + 1]
        np.testing.assert_allclose(acc[r * maxrows:r * maxrows + hi - lo], want[lo:hi],
                                   rtol=1e-5, atol=1e-6)
        assert np.all(acc[r * maxrows + hi - lo:(r + 1) * maxrows] == 0)


def test_csr_transpose(pgcn, loaded):
    ds = loaded["citeseer"]
    cp, cr, cpos = pgcn.csr_transpose(ds.feat_indptr, ds.feat_indices, ds.input_dim)
    import scipy.sparse as sps
    m = sps.csr_matrix((np.arange(1, len(ds.feat_indices) + 1), ds.feat_indices, ds.feat_indptr),
                       shape=(ds.num_nodes, ds.input_dim)).tocsc()
    np.testing.assert_array_equal(cp, m.indptr)
    np.testing.assert_array_equal(cr, m.indices)
    np.testing.assert_array_equal(cpos + 1, m.data)  # row-major slot of each CSC entry


def test_synthetic_generator_properties(pgcn):
    """Seeded reddit-shaped generator: symmetric, sorted rows with a self loop, deterministic,
    labels in range, split counts proportional to reddit's 153431/23831/55703."""
    n, f, c, e = 3000, 12, 5, 40000
    a = pgcn.Dataset.synthetic(n, f, c, e, seed=7)
    b = pgcn.Dataset.synthetic(n, f, c, e, seed=7)
    for key in ("graph_indptr", "graph_indices", "feat_values", "label", "split"):
        np.testing.assert_array_equal(getattr(a, key), getattr(b, key))
    ip, ix = a.graph_indptr, a.graph_indices
    assert ip[-1] == 2 * e + n
    import scipy.sparse as sps
    m = sps.csr_matrix((np.ones(len(ix)), ix, ip), shape=(n, n))
    assert (m != m.T).nnz == 0
    assert np.all(m.diagonal() == 1)
    for i in range(0, n, 97):  # self loop first, then neighbours ascending (hpdga row order)
        row = ix[ip[i]:ip[i + 1]]
        assert row[0] == i and np.all(np.diff(row[1:]) >= 0)
    assert a.label.min() >= 0 and a.label.max() < c
    cnt = np.bincount(a.split, minlength=4)[1:4] / n
    np.testing.assert_allclose(cnt, np.array([153431, 23831, 55703]) / 232965, atol=0.02)
    assert np.array_equal(a.feat_indptr, np.arange(n + 1) * f)
    other = pgcn.Dataset.synthetic(n, f, c, e, seed=8)
    assert not np.array_equal(other.graph_indices[:1000], ix[:1000])


def _lds_check(pgcn, ip, ix, n, window):
    err, nb = ctypes.c_double(), ctypes.c_longlong()
    pgcn.check(pgcn.lib.pgcn_debug_lds_check(n, n, helpers.ptr(ip), helpers.ptr(ix), window,
                                             ctypes.byref(err), ctypes.byref(nb)), "lds_check")
    return err.value, nb.value


def test_graph_create_values_rejects_bad_csr(pgcn):
    """pgcn_graph_create_values validates the CSR before touching a device: a column id out
    of range, a decreasing indptr or a null values pointer is PGCN_E_INVALID (host only)."""
    lib = pgcn.lib
    ip = np.array([0, 2, 3], np.int32)
    vals = np.ones(3, np.float32)
    g = ctypes.c_void_p()
    for ix in (np.array([0, 2, 1], np.int32), np.array([0, -1, 1], np.int32)):
        assert lib.pgcn_graph_create_values(2, helpers.ptr(ip), helpers.ptr(ix),
                                            helpers.ptr(vals), ctypes.byref(g)) \
            == pgcn.PGCN_E_INVALID
    ix = np.array([0, 1, 1], np.int32)
    bad = np.array([0, 3, 2], np.int32)
    assert lib.pgcn_graph_create_values(2, helpers.ptr(bad), helpers.ptr(ix), helpers.ptr(vals),
                                        ctypes.byref(g)) == pgcn.PGCN_E_INVALID
    assert lib.pgcn_graph_create_values(2, helpers.ptr(ip), helpers.ptr(ix), None,
                                        ctypes.byref(g)) == pgcn.PGCN_E_INVALID


RING = 5  # pgcn_debug_lds_check's schedule kind: the ring schedule, the only LDS schedule


@pytest.mark.parametrize("pair,window", [(0, 3), (1, 3), (0, 2)])
def test_lds_schedule_walk_sums_every_edge(pgcn, pair, window):
    """The d = 16 LDS ring schedule (host/ring.cpp), walked on the CPU exactly as
    k_graphsum_ring consumes it (per-wave entry streams, per-visit step counts over 3 resident
    slices, ring-buffer plane offsets, spread hub rows, zero rows; pair 1: rowsets in lockstep
    pairs, their blocks alternating), reproduces every row's CSR sum, with fewer than 4 step
    slots per edge on this sparse power-law graph (3.67; 2.03 on reddit-114M, whose rows have
    8x the edges per slice; pairs 4.49 and 2.29); any other schedule kind is refused."""
    ds = pgcn.Dataset.synthetic(70000, 8, 4, 2000000, 1)
    ip = np.ascontiguousarray(ds.graph_indptr)
    ix = np.ascontiguousarray(ds.graph_indices)
    with helpers.knobs(pgcn, ring_pair=pair, ring_window=window):
        err, nb = _lds_check(pgcn, ip, ix, ds.num_nodes, RING)
    assert err < 1e-12
    bound = 4.6 if pair else (4.0 if window == 3 else 5.4)
    assert nb * 64 < bound * len(ix), nb * 64 / len(ix)
    e, n = ctypes.c_double(), ctypes.c_longlong()
    assert pgcn.lib.pgcn_debug_lds_check(ds.num_nodes, ds.num_nodes, helpers.ptr(ip),
                                         helpers.ptr(ix), 1, ctypes.byref(e),
                                         ctypes.byref(n)) == pgcn.PGCN_E_INVALID


def test_lds_schedule_ragged_graph(pgcn):
    """Isolated rows, a hub adjacent to everything, duplicate edges: the ring schedule stays
    exact."""
    rng = np.random.default_rng(5)
    n = 5000
    rows = [[] for _ in range(n)]
    for i in range(n):
        if i % 7 == 0:  # every 7th row empty
            continue
        k = int(rng.integers(1, 40))
        rows[i] = sorted(rng.integers(0, n, k).tolist())  # duplicates kept
    rows[1] = list(range(n))  # hub
    ip = np.zeros(n + 1, np.int32)
    ip[1:] = np.cumsum([len(r) for r in rows])
    ix = np.ascontiguousarray(np.concatenate([np.array(r, np.int32) for r in rows if r]))
    err, _ = _lds_check(pgcn, ip, ix, n, RING)
    assert err < 1e-12


@pytest.mark.parametrize("seed", [0, 1, 2, 1382895624, 311288059, 2108234352, 19990304])
def test_rng_seed_glibc_matches_srand(pgcn, seed):
    """PART2 `seed`: the xorshift state is the first two rand() values after srand(seed)
    (hpdga rand.cpp:6-14 with the seed applied); seed 0/1 = the unseeded default.  Checked
    against the C library itself, and the engine against the oracle."""
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(ctypes.c_uint(seed))
    want = [libc.rand(), libc.rand()]
    libc.srand(ctypes.c_uint(1))
    got = pgcn.rng_seed(seed) if seed else pgcn.rng_seed()
    assert [int(got[0]), int(got[1])] == want
    orc = helpers.oracle()
    s = np.zeros(2, np.uint64)
    orc.or_rng_seed_glibc(ctypes.c_uint(seed), helpers.ptr(s))
    assert [int(s[0]), int(s[1])] == want


def test_dataset_binarize(pgcn, tmp_path):
    """PART2 NO_FEATURE (src/parser.cpp:100-104): values 1.0, ids and dims unchanged."""
    root = str(tmp_path)
    ds = pgcn.Dataset.load(root, helpers.materialize_dataset("cora", root))
    ids, f = ds.feat_indices.copy(), ds.input_dim
    ds.binarize()
    assert (ds.feat_values == 1.0).all()
    np.testing.assert_array_equal(ds.feat_indices, ids)
    assert ds.input_dim == f


def test_gcn_par_cli_loader_paths(tmp_path):
    """gcn-par (the reference's entry point, src/main.cpp:9-61): a missing dataset is reported
    like the reference; cache=1 writes the binary cache while loading, and the run then stops
    at engine creation on a host without a HIP device (no CPU fallback)."""
    import subprocess
    import torch
    exe = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "gcn-par")
    root = str(tmp_path)
    r = subprocess.run([exe, "nonexistent", f"root={root}"], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "Cannot read input: nonexistent" in r.stderr
    if torch.cuda.is_available():
        pytest.skip("a device is present: gcn-par would train")
    name = helpers.materialize_dataset("cora", root)
    params = os.path.join(root, "params.txt")
    with open(params, "w") as f:
        f.write("n_layers = 2\nhidden_dims = 72\ndropouts = 0.4,0.2\nseed = 1382895624\n")
    r = subprocess.run([exe, name, f"root={root}", f"file={params}", "cache=1", "no_feature=1"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "GCN creation failed" in r.stderr
    assert os.path.exists(os.path.join(root, "data", name + ".pgcnbin"))


def test_cpp_api_header_and_driver_without_device(datasets):
    """include/pgcn.hpp (the reference-shaped C++ API) is self-contained C++17, and the C++
    test driver built against it loads the dataset through api::Parser, then fails loudly
    (the engine has no CPU fallback) when no HIP device is present."""
    import subprocess
    import torch
    hdr = os.path.join(helpers.REPO, "include", "pgcn.hpp")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__",
                        "-I/opt/rocm/include", "-x", "c++", hdr], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    if torch.cuda.is_available():
        pytest.skip("a device is present")
    root, names = datasets
    exe = os.path.join(helpers.REPO, "parallel-gcn_amd", "bin", "test_module_api")
    r = subprocess.run([exe, "modules", root, names["cora"], "1"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "no HIP device" in r.stderr, (r.returncode, r.stderr[-500:])


LLVM_BIN = "/opt/rocm/lib/llvm/bin"


def _kernel_objects():
    """The built gfx950 kernel objects (skips when the build or the llvm tools are absent: a
    CPU-only or sanitizer build checks nothing here)."""
    import glob
    objs = sorted(glob.glob(os.path.join(helpers.REPO, "parallel-gcn_amd", "build", "k_*.o")))
    if not objs:
        pytest.skip("libpgcn.so kernel objects not built")
    for tool in ("llvm-objdump", "llvm-readelf"):
        if not os.access(os.path.join(LLVM_BIN, tool), os.X_OK):
            pytest.skip(f"{tool} not available")
    return objs


def _device_code(obj, tmp_path):
    """The gfx950 code object inside a host object (llvm-objdump --offloading)."""
    import glob
    import shutil
    import subprocess
    local = tmp_path / os.path.basename(obj)
    shutil.copy(obj, local)
    subprocess.run([f"{LLVM_BIN}/llvm-objdump", "--offloading", str(local)], check=True,
                   capture_output=True, cwd=tmp_path)
    dev = glob.glob(str(local) + ".*gfx950")
    assert dev, obj
    return dev[0]


def test_no_kernel_spills_to_scratch(tmp_path):
    """Every HIP kernel of libpgcn.so runs without scratch (private segment 0): a spill is a
    silent slowdown (r03: the X-stream TN kernel lost 40 % to 348 B of spills after an
    unrelated edit).  Reads the gfx950 code objects' metadata of the built objects."""
    import re
    import subprocess
    objs = _kernel_objects()
    seen = 0
    for o in objs:
        dev = _device_code(o, tmp_path)
        notes = subprocess.run([f"{LLVM_BIN}/llvm-readelf", "--notes", dev], check=True,
                               capture_output=True, text=True).stdout
        names = re.findall(r"^\s+\.name:\s+(\S+)", notes, re.M)
        scratch = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", notes)]
        assert len(names) == len(scratch) and names, o
        bad = [(n, b) for n, b in zip(names, scratch) if b]
        assert not bad, bad
        seen += len(names)
    assert seen >= 20


def test_ring_kernel_lds_reads_wait_before_use(tmp_path):
    """k_graphsum_ring issues its LDS reads from inline asm (lds_dma.hpp ds_rd128 / ds_rd64_into):
    hipcc believes their results ready at once, so correctness rests on no instruction reading
    or moving a destination register before the s_waitcnt lgkmcnt(N) that retires the read
    (the asm lgkm_wait).  Walks the gfx950 disassembly in order, keeping the lgkm queue: until
    a wait retires a read, no instruction may name its destination registers (a compiler
    upgrade that inserted a v_mov there would otherwise show up only as wrong sums)."""
    import re
    import subprocess
    obj = [o for o in _kernel_objects() if o.endswith("k_graphsum_ring.o")]
    assert obj, "k_graphsum_ring.o not built"
    dev = _device_code(obj[0], tmp_path)
    asm = subprocess.run([f"{LLVM_BIN}/llvm-objdump", "-d", "--no-show-raw-insn", dev],
                         check=True, capture_output=True, text=True).stdout.splitlines()
    starts = [i for i, l in enumerate(asm) if re.match(r"^[0-9a-f]+ <_ZN4pgcn15k_graphsum_ring", l)]
    assert len(starts) >= 1, "k_graphsum_ring<16> not in the code object"

    def regs(ops):
        out = set()
        for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", ops):
            if m.group(3) is not None:
                out.add(int(m.group(3)))
            else:
                out.update(range(int(m.group(1)), int(m.group(2)) + 1))
        return out
    # every LDS / scalar-memory operation takes a place in the lgkm queue (LDS operations
    # complete in issue order); s_waitcnt lgkmcnt(N) retires all but the newest N, so a read's
    # destination is free once N is below the number of operations issued after it
    lgkm_ops = ("ds_", "s_load", "s_buffer_load", "s_sendmsg")
    for start in starts:
        queue, bad, reads = [], [], 0
        for line in asm[start + 1:]:
            if re.match(r"^[0-9a-f]+ <", line):
                break
            t = line.strip()
            if not t or t.startswith(";"):
                continue
            op, _, ops = t.partition(" ")
            ops = ops.split("//")[0]
            if op == "s_waitcnt":
                m = re.search(r"lgkmcnt\((\d+)\)", ops)
                if m:
                    n = int(m.group(1))
                    queue = queue[len(queue) - n:] if n else []
                continue
            pending = set().union(*queue) if queue else set()
            if op in ("ds_read_b128", "ds_read_b64"):
                if pending & regs(ops.split(",", 1)[1] if "," in ops else ""):
                    bad.append(t)
                queue.append(regs(ops.split(",")[0]))
                reads += 1
            elif op.startswith(lgkm_ops):
                if pending & regs(ops):
                    bad.append(t)
                queue.append(set())
            elif pending & regs(ops):
                bad.append(t)
        assert reads >= 16, reads
        assert not bad, bad[:10]


def test_debug_set_refuses_out_of_range_values(pgcn):
    """pgcn_debug_set range-checks every key (pgcn.h): an out-of-range value returns
    PGCN_E_INVALID and leaves the knob unchanged (host only, no device)."""
    lib = pgcn.lib
    for key, bad in (("train_ahead", 2), ("split_rows", -1), ("split_cols", 5), ("eval_ax", 2),
                     ("epoch_graph", 3), ("fuse_epilogue", 16), ("fuse_output", 4),
                     ("mm_side", 3), ("xstream_ring", 2), ("eval_tail", 2), ("gs16_gather", 3),
                     ("peer_uncached", 2), ("ring_pair", 2), ("tn_fold", 2), ("fuse_finish", 3), ("mask_per", 3), ("ring_window", 1), ("csc_tree", 2), ("mask_adam", 2), ("reassoc_small", 2), ("defer_wgrad", 2), ("mask_xstream", 2),
                     ("lds_blocks", 3), ("parse_threads", -2),
                     ("gs_split", 4), ("gs_item_iters", 5), ("co_draw", 3), ("gs_orig_cols", 2), ("sparse_dual", 2)):
        assert lib.pgcn_debug_set(key.encode(), bad) < 0, key
    assert lib.pgcn_debug_set(b"no_such_knob", 0) < 0
    # diagnostic arms removed in r05: refused like any unknown key
    for key in ("gemm_variant", "plain_blocks", "lds_slots", "mask_nib", "rs_chunks",
                "wide_prescale"):
        assert lib.pgcn_debug_set(key.encode(), 0) < 0, key
    for key, val in helpers.ENGINE_DEFAULTS.items():
        assert lib.pgcn_debug_set(key.encode(), val) == 0, key


def test_knob_table_matches_engine_defaults(pgcn):
    """The library's knob table, enumerated through pgcn_debug_knob, has exactly the keys and
    defaults of helpers.ENGINE_DEFAULTS; past its end the call returns PGCN_E_INVALID."""
    import ctypes
    table, i = {}, 0
    while True:
        name, default = ctypes.c_char_p(), ctypes.c_int()
        st = pgcn.lib.pgcn_debug_knob(i, ctypes.byref(name), ctypes.byref(default))
        if st != 0:
            break
        assert name.value.decode() not in table, name.value
        table[name.value.decode()] = default.value
        i += 1
    assert st == -1 and pgcn.lib.pgcn_debug_knob(-1, None, None) == -1
    assert pgcn.lib.pgcn_debug_knob(0, None, None) == 0
    assert table == helpers.ENGINE_DEFAULTS
