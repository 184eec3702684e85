"""Elastic_PC on base-field streams (include/hobbit_elastic_real.h): the real row code at any length, the streaming commit through half chunk
tensors, the two opening passes and the refusals, against the calls of hobbit_hip.h on the same chunks widened to (x, 0) by hobbit_widen_real.
All arithmetic is exact and canonical, so every comparison is byte for byte.

Commit shapes.  Option 1 (RS x RS, trs = B / 2^11, 4096-point rows): B = 2^13 (trs = 4: an 8-point column transform, the smallest shape where the
row negation of the RS x RS identity can go wrong), 2^14, 2^16, 2^18.  Option 2 (RS x expander, trs = B / 2^14, 32768-point rows): B = 2^16
(trs = 4, the identity code), 2^18 (trs = 16), 2^20 (trs = 64).  N / B = 4 and 8, every chunk different, both settings of gcc_arg_order.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
libc = ctypes.CDLL(None)
c_vp, c_sz, c_int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
P = (1 << 61) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")
EINVAL, ESTATE = "rc=-2", "rc=-5"


@pytest.fixture(scope="module")
def mod():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def hb(mod):
    h = mod.Hobbit(0)
    yield h
    h.close()


def reals(n, seed):
    x = np.random.default_rng(seed).integers(0, P, n, dtype=np.uint64)
    x[:3] = (0, 1, P - 1)
    return x


def widen_dev(hb, d_real, n):
    d = hb.alloc(16 * n)
    hb._chk(hb.lib.hobbit_widen_real(hb.ctx, c_vp(d_real.ptr), c_vp(d.ptr), c_sz(n)))
    return d


# ---- the row code at any length ---------------------------------------------------------------------
def row_inputs(kind, rows, h):
    if kind == "uniform":
        return np.random.default_rng(11 + rows + h).integers(0, P, (rows, h), dtype=np.uint64)
    if kind == "all p-1":
        return np.full((rows, h), P - 1, np.uint64)
    if kind == "below 2^33":
        return np.random.default_rng(33 + rows + h).integers(0, 1 << 33, (rows, h), dtype=np.uint64)
    x = np.zeros((rows, h), np.uint64)                         # unit vectors at positions 0, 1, h - 1
    for r in range(rows):
        x[r, (0, 1, h - 1)[r % 3]] = 1
    return x


@pytest.mark.parametrize("kind", ["uniform", "all p-1", "unit vectors", "below 2^33"])
@pytest.mark.parametrize("rows", [1, 3, 64])
@pytest.mark.parametrize("logL", [3, 5, 11, 12, 13, 15, 16])
def test_real_row_code_is_the_transform_of_the_widened_row(hb, logL, rows, kind):
    L = 1 << logL; h = L // 2
    x = row_inputs(kind, rows, h)
    padded = np.zeros((rows, L, 2), np.uint64); padded[:, :h, 0] = x
    want = hb.fft_any(padded)[:, :h + 1]
    got = hb.fft_real_rows_any(x, logL)
    assert np.array_equal(got, want)
    if kind == "unit vectors":
        assert (got[0] == np.array([1, 0], np.uint64)).all()   # delta at 0: the all-ones row


# ---- the streaming commit ---------------------------------------------------------------------------
def shape(opt, B):
    return (0, B >> 11) if opt == 1 else (1, B >> 14)


def prepare_graphs(hb, opt, B):
    lin, trs = shape(opt, B)
    if lin:
        hb.rng_reset(); hb.graph_draw(trs)


def stream_commit(hb, B, opt, order, chunks, real):
    """hobbit_elastic_begin(_real), one push per chunk (host arrays of B uint64; the full form gets them widened on the device), finish.
    Returns (all 8B - 1 tree hashes, the handle's device bytes)."""
    lin, trs = shape(opt, B)
    e = c_vp()
    begin = hb.lib.hobbit_elastic_begin_real if real else hb.lib.hobbit_elastic_begin
    hb._chk(begin(hb.ctx, B, trs, lin, order, ctypes.byref(e)))
    try:
        held = hb.lib.hobbit_elastic_device_bytes(e)
        for x in chunks:
            d = hb.to_device(x)
            if real:
                hb._chk(hb.lib.hobbit_elastic_push_real(hb.ctx, e, d.ptr))
            else:
                w = widen_dev(hb, d, B)
                hb._chk(hb.lib.hobbit_elastic_push(hb.ctx, e, w.ptr))
            hb.sync()
        lv = hb.alloc(32 * 8 * B)
        hb._chk(hb.lib.hobbit_elastic_finish(hb.ctx, e, lv.ptr))
        return hb.to_host(lv, (8 * B - 1, 32), np.uint8), held
    finally:
        hb.lib.hobbit_elastic_free(e)


COMMIT_SHAPES = [(1, 13), (1, 14), (1, 16), (1, 18), (2, 16), (2, 18), (2, 20)]


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("opt,logB", COMMIT_SHAPES, ids=["opt%d-B2e%d" % s for s in COMMIT_SHAPES])
def test_real_commit_equals_the_commit_of_the_widened_stream(hb, opt, logB, groups, order):
    B = 1 << logB
    prepare_graphs(hb, opt, B)
    chunks = [reals(B, 100 * logB + i) for i in range(4 * groups)]
    want, full_bytes = stream_commit(hb, B, opt, order, chunks, False)
    got, real_bytes = stream_commit(hb, B, opt, order, chunks, True)
    assert np.array_equal(got, want)
    lin, trs = shape(opt, B); cols = 2 * B // trs; rows2 = 2 * trs
    print("device bytes: full %d, real %d" % (full_bytes, real_bytes))
    assert full_bytes >= 4 * 4 * B * 16 + 4 * B * 32
    assert real_bytes <= 4 * (cols // 2 + 1) * rows2 * 16 + 4 * B * 32 + 5 * 4096      # (five buffers, each rounded to a page at most)
    assert real_bytes < full_bytes


@pytest.mark.parametrize("opt,logB", [(1, 14), (2, 18)])
@pytest.mark.parametrize("kind", ["zero chunk in a group", "all p-1"])
def test_real_commit_edge_streams(hb, opt, logB, kind):
    B = 1 << logB
    prepare_graphs(hb, opt, B)
    if kind == "all p-1":
        chunks = [np.full(B, P - 1, np.uint64)] * 4
    else:
        chunks = [reals(B, 7 + i) for i in range(8)]
        chunks[1] = np.zeros(B, np.uint64); chunks[6] = np.zeros(B, np.uint64)
    want, _ = stream_commit(hb, B, opt, 1, chunks, False)
    got, _ = stream_commit(hb, B, opt, 1, chunks, True)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("opt", [1, 2])
def test_real_commit_of_the_default_stream_reproduces_the_fixture_root(hb, opt):
    """tests/golden/elastic.npz: the real reference's root of test_Elastic_PC's commit at (2^18, B = 2^14) on read_stream_PC's default stream"""
    g = np.load(os.path.join(GOLD, "elastic.npz"), allow_pickle=False)
    B = 1 << 14
    assert np.array_equal(hb.read_stream_PC_real(4096), hb.read_stream_PC(4096)[:, 0]) and not hb.read_stream_PC(4096)[:, 1].any()
    hb.rng_reset()
    lv = hb.elastic_commit_real(1 << 18, B, opt)
    assert np.array_equal(lv[-1], g["el_%d_root" % opt])


# ---- refusals -----------------------------------------------------------------------------------------
def test_refusals(hb, mod):
    B, trs = 1 << 18, 16
    hb.rng_reset(); hb.graph_draw(trs)
    d_real = hb.to_device(reals(B, 4)); d_wide = widen_dev(hb, d_real, B)
    for begin, wrong in ((hb.lib.hobbit_elastic_begin_real, lambda e: hb.lib.hobbit_elastic_push(hb.ctx, e, d_wide.ptr)),
                         (hb.lib.hobbit_elastic_begin, lambda e: hb.lib.hobbit_elastic_push_real(hb.ctx, e, d_real.ptr))):
        e = c_vp()
        hb._chk(begin(hb.ctx, B, trs, 1, 1, ctypes.byref(e)))
        with pytest.raises(mod.HobbitError, match=ESTATE):
            hb._chk(wrong(e))
        hb.lib.hobbit_elastic_free(e)
    # the two opening passes: one form per pass
    N = 4 * B; x = splitmix_field(20, 1)
    for first, second in ((hb.lib.hobbit_elastic_open_aggregate_push, hb.lib.hobbit_elastic_open_aggregate_push_real),
                          (hb.lib.hobbit_elastic_open_aggregate_push_real, hb.lib.hobbit_elastic_open_aggregate_push)):
        e = c_vp()
        hb._chk(hb.lib.hobbit_elastic_open_begin_lin(hb.ctx, N, B, trs, x.ctypes.data_as(c_vp), 64, ctypes.byref(e)))
        hb._chk(first(hb.ctx, e, (d_wide if first is hb.lib.hobbit_elastic_open_aggregate_push else d_real).ptr))
        with pytest.raises(mod.HobbitError, match=ESTATE + ".*mixed"):
            hb._chk(second(hb.ctx, e, (d_wide if second is hb.lib.hobbit_elastic_open_aggregate_push else d_real).ptr))
        hb.lib.hobbit_elastic_open_free(e)
    # RS x expander needs base-field weights: the same graphs drawn on the host, one weight changed
    hb.rng_reset(); hb.expander_init_store(trs)
    w = hb._graph_levels[(0, 1)][4].copy()
    w[7, 1] = 1
    hb.rng_reset(); hb.expander_init_store(trs, weights={(0, 1): w})
    e = c_vp()
    with pytest.raises(mod.HobbitError, match=EINVAL + ".*img != 0"):
        hb._chk(hb.lib.hobbit_elastic_begin_real(hb.ctx, B, trs, 1, 1, ctypes.byref(e)))
    assert not e.value
    hb._chk(hb.lib.hobbit_elastic_begin_real(hb.ctx, B >> 3, B >> 14, 0, 1, ctypes.byref(e)))      # RS x RS does not look at the graphs
    hb.lib.hobbit_elastic_free(e)
    # the context is still usable, and base-field graphs are accepted again
    chunks = [reals(B, 50 + i) for i in range(4)]
    hb.rng_reset(); hb.graph_draw(trs)
    want, _ = stream_commit(hb, B, 2, 1, chunks, False)
    got, _ = stream_commit(hb, B, 2, 1, chunks, True)
    assert np.array_equal(got, want)


# ---- the opening --------------------------------------------------------------------------------------
def same(a, b, where=""):
    assert set(a) == set(b), where
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k], where + k + "/")
        elif a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, where + k
        else:
            assert np.array_equal(a[k], b[k]), where + k


def test_real_opening_option_1_is_the_opening_of_the_widened_stream(hb):
    """(2^18, B = 2^14, 700 queries), srandom(99): queries, replies, paths, roots, round polynomials and final values"""
    N, B = 1 << 18, 1 << 14
    x = splitmix_field(18, 7)
    d_real = hb.to_device(reals(B, 18)); d_wide = widen_dev(hb, d_real, B)
    _, dlv = hb.elastic_commit_real(N, B, 1, chunk=d_real, keep_levels=True)
    libc.srandom(99); want = hb.elastic_open(N, B, x, 700, commit_levels=dlv, chunk=d_wide)
    libc.srandom(99); got = hb.elastic_open_real(N, B, x, 700, commit_levels=dlv, chunk=d_real)
    assert got["checks"].tolist() == [1, 1] and int(got["reply_len"][0]) == N // B
    assert (got["cols"] > 2048).sum() > 100 and (got["cols"] <= 2048).sum() > 100
    same(got, want)


def test_real_opening_option_2_is_the_opening_of_the_widened_stream(hb):
    """(2^20, B = 2^16, 5900 queries), srandom(77), every chunk different; the stale-parity picks included"""
    N, B = 1 << 20, 1 << 16
    x = splitmix_field(20, 7)
    hb.rng_reset()
    real = [hb.to_device(reals(B, 20 + i)) for i in range(N // B)]
    wide = [widen_dev(hb, d, B) for d in real]
    _, dlv = hb.elastic_commit_real(N, B, 2, chunks=lambda i: real[i], keep_levels=True)
    libc.srandom(77); want = hb.elastic_open2(N, B, x, 5900, commit_levels=dlv, chunks=lambda i: wide[i])
    libc.srandom(77); got = hb.elastic_open2_real(N, B, x, 5900, commit_levels=dlv, chunks=lambda i: real[i])
    assert got["checks"].tolist() == [1] and int(got["reply_len"][0]) == N // B
    assert (got["cols"] > B // 4).sum() > 1000 and (got["cols"] <= B // 4).sum() > 1000          # (cols = 2^15: both halves are queried)
    same(got, want)


# ---- the driver ---------------------------------------------------------------------------------------
def _test_pc(args, timeout):
    exe = os.path.join(PKG, "host", "test_pc")
    return subprocess.run(["timeout", "-k", "10", str(timeout), exe] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT)


@pytest.mark.parametrize("logN,logB,opt", [(18, 14, 1), (20, 16, 2)])
def test_driver_prints_the_same_root_and_proof_size(logN, logB, opt):
    """host/test_pc elastic_real <logN> <logB> <opt> and host/test_pc elastic <logN> <logB> <opt>, each a fresh child process: the same root, the
    same proof size, and every other line that carries no time the same"""
    def lines(p):
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        out = p.stdout.splitlines()
        root = [l for l in out if l.startswith("root ")]
        ps = [l.split(",")[0] for l in out if l.startswith("PC : ps = ")]
        assert len(root) == 1 and len(ps) == 1
        timeless = [l for l in out if "time" not in l and not l.startswith("PC : ps = ")]
        return root[0], ps[0], timeless
    a = lines(_test_pc(("elastic_real", logN, logB, opt), 120))
    b = lines(_test_pc(("elastic", logN, logB, opt), 120))
    assert a == b
