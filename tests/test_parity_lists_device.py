"""The parity matrix' access lists built on the device (include/hobbit_parity_lists.h): hobbit_parity_commit_device and hobbit_parity_shape.

The independent statements of the lists are the ones tests/test_parity_matrix.py already pins: the host builder hobbit_parity_commit (the
restatement of generate_access_idx, src/sumcheck.cpp:2622-2669, that the reference's fixture pins), tests/parity_model.py, and
tests/golden/parity_matrix.npz.  Every comparison here is bit for bit; graphs come from the oracle on the fresh-process libc stream, through
that file's helpers.
"""
import ctypes
import os
import re
import time

import numpy as np
import pytest

import test_parity_matrix as tpm
from test_parity_matrix import check_commit, graphs, libc, model, next_draws, same_opening, start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P61 = (1 << 61) - 1
LISTS = ("idx1", "idx2", "cnt1", "cnt2", "weight", "acc1", "acc2")
GRAPH_BUDGET_S = 10.0                 # the 2^20 case is skipped when the oracle needs longer than this for the graphs


def _mod():
    from __graft_entry__ import load_package
    return load_package()


# ---- the header and its symbols (CPU) -------------------------------------------------------------------------------------------------------------
ASYNC = {"hobbit_parity_commit_device"}
HOST_ONLY = {"hobbit_parity_shape"}


def declared():
    src = open(os.path.join(ROOT, "include", "hobbit_parity_lists.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(hobbit_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound():
    from __graft_entry__ import build_hip
    build_hip()
    mod = _mod()
    lib = mod.load_library()
    decl = declared()
    assert len(decl) == 2 and sorted(mod.PARITY_LISTS_SYMBOLS) == decl
    for s in decl:
        assert hasattr(lib, s), "missing export " + s
        assert getattr(lib, s).argtypes is not None, "no prototype bound for " + s
    for other in (mod.ABI_SYMBOLS, mod.PARITY_SYMBOLS, mod.WHIR_SYMBOLS, mod.BRAKINGBASE_SYMBOLS):
        assert not set(decl) & set(other)
    for meth in ("commit_parity_matrix_device", "parity_shape"):
        assert callable(getattr(mod.Hobbit, meth))


def test_every_export_is_classified():
    """asynchronous (the stream test below) or host only"""
    names = set(declared())
    assert ASYNC | HOST_ONLY == names and not ASYNC & HOST_ONLY


# ---- the device ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hb():
    h = _mod().Hobbit(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(tpm.GOLD, allow_pickle=False))


def same_commit(dev, host, levels=True):
    """all seven lists over their full length (padding included), the dimensions, the root and the tree"""
    assert (dev.n, dev.m, dev.P) == (host.n, host.m, host.P)
    a, b = dev.lists(), host.lists()
    for k in LISTS:
        bad = np.nonzero(a[k].reshape(a[k].shape[0], -1) != b[k].reshape(b[k].shape[0], -1))[0]
        assert not len(bad), "%s: first differing entry %d of %d (m = %d)" % (k, bad[0], a[k].shape[0], dev.m)
    assert np.array_equal(dev.root(), host.root()), "root"
    if levels:
        assert np.array_equal(dev.levels(), host.levels()), "levels"
    return a


def both(hb, n):
    return hb.commit_parity_matrix_device(n), hb.commit_parity_matrix(n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 64, 128, 1024, 4096, 8192])
def test_against_the_host_builder_the_model_and_the_fixture(hb, oracle, gold, n):
    """every depth of the recursion: one level at 16, two at 64 and 128, up to the long-code graphs of 8192"""
    C = model(oracle, n, opened=False)["C"]
    start(oracle, n); hb.upload_graphs(n, graphs(oracle, n))
    want = next_draws(5)
    libc.srandom(5)
    dev = hb.commit_parity_matrix_device(n)
    assert [libc.random() for _ in range(4)] == want, "the commit drew from libc"
    host = hb.commit_parity_matrix(n)
    same_commit(dev, host)
    check_commit(dev, C)
    if n in tpm.NS:
        assert np.array_equal(dev.root(), gold["cp_root_%d" % n])
    dev.free(); host.free()


def structured(levels, how):
    """the oracle's levels with L, R and degree kept (so m, P and the layout check stay) and the edges replaced"""
    out = {}
    for key, g in levels.items():
        L, R, d = g["L"], g["R"], g["degree"]
        e = np.arange(L * d, dtype=np.int64)
        nbr, w = g["nbr"], g["w"]
        if how == "one_bucket":
            nbr = np.zeros(L * d, np.int64)                       # one bucket holds the whole level
        elif how == "runs":
            nbr = (e // d) % R                                    # every edge of input i to cell i % R: runs of `degree` duplicates
        elif how == "even_up":
            nbr = e % R
        elif how == "even_down":
            nbr = R - 1 - e % R
        elif how == "general_weights":
            w = np.zeros((L * d, 2), np.uint64)
            k = e % 3
            w[:, 0] = np.where(k == 0, P61 - 1, np.where(k == 1, (1 << 32) + e, 7 * e + 1)).astype(np.uint64)
            w[:, 1] = np.where(k == 0, 0, np.where(k == 1, 5 + e, (1 << 40) + e)).astype(np.uint64)
        out[key] = dict(L=L, R=R, degree=d, nbr=np.ascontiguousarray(nbr, np.int64), w=w)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["one_bucket", "runs", "even_up", "even_down", "general_weights"])
@pytest.mark.parametrize("n", [1024, 4096])
def test_structured_graphs(hb, oracle, n, how):
    start(oracle, n)
    lv = structured(graphs(oracle, n), how)
    hb.upload_graphs(n, lv)
    dev, host = both(hb, n)
    ls = same_commit(dev, host, levels=False)
    if how == "one_bucket":                                       # the first level's n * degree edges all count up in one cell
        E = lv[(0, 0)]["L"] * lv[(0, 0)]["degree"]
        assert np.array_equal(ls["cnt1"][:E], np.arange(1, E + 1, dtype=np.uint32))
    if how == "general_weights":
        assert (ls["weight"][:, 1] != 0).any() and (ls["weight"][:, 0] >> np.uint64(32)).any()
    dev.free(); host.free()


def accs(pc):
    a1 = np.zeros((2 * pc.n, 2), np.uint64); a2 = np.zeros((2 * pc.n, 2), np.uint64)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pc.hb._chk(pc.hb.lib.hobbit_parity_lists(pc.hb.ctx, pc.h, None, None, None, None, None, hp(a1), hp(a2)))
    return a1, a2


@pytest.mark.gpu
def test_size_2e17(hb, oracle):
    n = 1 << 17
    start(oracle, n); hb.upload_graphs(n, graphs(oracle, n))
    dev, host = both(hb, n)
    same_commit(dev, host, levels=False)
    dev.free(); host.free()


@pytest.mark.gpu
def test_size_2e20(hb, oracle):
    """(m, P), the access counts and the root: the root binds every list entry (the lists are 1.2 GB)"""
    n = 1 << 20
    t0 = time.perf_counter()
    start(oracle, n); lv = graphs(oracle, n)
    if time.perf_counter() - t0 > GRAPH_BUDGET_S:
        pytest.skip("the oracle took %.1f s for the graphs of 2^20" % (time.perf_counter() - t0))
    hb.upload_graphs(n, lv)
    del lv
    dev, host = both(hb, n)
    assert (dev.m, dev.P) == (host.m, host.P) == hb.parity_shape(n)
    for a, b, k in zip(accs(dev), accs(host), ("acc1", "acc2")):
        assert np.array_equal(a, b), k
    assert np.array_equal(dev.root(), host.root())
    dev.free(); host.free()
    hb.upload_graphs(16, graphs_of(oracle, 16))                  # let go of the 2^20 code's device tables


def graphs_of(oracle, n):
    start(oracle, n)
    return graphs(oracle, n)


@pytest.mark.gpu
def test_reproducible_cached_and_following_the_graphs(hb, oracle):
    n = 4096
    mod = _mod()
    hb.upload_graphs(n, graphs_of(oracle, n))
    a = hb.commit_parity_matrix_device(n); b = hb.commit_parity_matrix_device(n)          # the second uses the cached forward form
    la = same_commit(b, a)
    a.free(); b.free()
    oracle.rng_reset(); oracle.generate_randomness(3); oracle.expander_init_store(n)      # other graphs of the same n
    hb.upload_graphs(n, graphs(oracle, n))
    dev, host = both(hb, n)
    lb = same_commit(dev, host)
    assert not np.array_equal(la["idx1"], lb["idx1"]) and not np.array_equal(la["cnt1"], lb["cnt1"])
    dev.free(); host.free()
    hb._chk(hb.lib.hobbit_graph_reset(hb.ctx))
    with pytest.raises(mod.HobbitError, match="rc=-5"):
        hb.commit_parity_matrix_device(n)


@pytest.mark.gpu
def test_refusals_and_shape(hb, oracle):
    mod = _mod()
    hb.upload_graphs(128, graphs_of(oracle, 128))
    want = next_draws(5)
    libc.srandom(5)
    with pytest.raises(mod.HobbitError, match="rc=-2"):
        hb.commit_parity_matrix_device(100)
    with pytest.raises(mod.HobbitError, match="rc=-5"):
        hb.commit_parity_matrix_device(256)              # graphs finalized for another n
    with pytest.raises(mod.HobbitError, match="rc=-2"):
        hb.parity_shape(100)
    with pytest.raises(mod.HobbitError, match="rc=-5"):
        hb.parity_shape(256)
    assert [libc.random() for _ in range(4)] == want, "a refused call drew from libc"
    for n in (16, 128, 8192):
        hb.upload_graphs(n, graphs_of(oracle, n))
        libc.srandom(5)
        shape = hb.parity_shape(n)
        assert [libc.random() for _ in range(4)] == want
        pc = hb.commit_parity_matrix(n)
        assert shape == (pc.m, pc.P)
        pc.free()


@pytest.mark.gpu
def test_device_commit_queued_behind_a_backlog_then_opened(hb, oracle):
    """tests/test_parity_matrix.py::test_commit_queued_behind_a_backlog_then_opened for the device builder, with its backlog: commit on a
    caller's (torch) stream behind the backlog, the opening right behind it with no synchronisation in between"""
    import torch
    n = 128
    r1, r2 = start(oracle, n); levels = graphs(oracle, n)
    hb.upload_graphs(n, levels)
    pc = hb.commit_parity_matrix_device(n); hb.sync()
    libc.srandom(77); want = hb.open_parity_matrix(pc, r1, r2); root = pc.root(); pc.free()
    stream = torch.cuda.Stream()
    hs = _mod().Hobbit(0, stream=stream.cuda_stream)
    try:
        hs.upload_graphs(n, levels)
        w = hs.commit_parity_matrix_device(n); libc.srandom(3); hs.open_parity_matrix(w, r1, r2); w.free()      # the shapes once: caches and workspaces exist now
        t = [torch.empty((tpm.BACKLOG_N, 2), dtype=torch.int64, device="cuda") for _ in range(3)]
        for i in range(2):
            hs._chk(hs.lib.hobbit_fill_splitmix(hs.ctx, t[i].data_ptr(), tpm.BACKLOG_N, 77 + i))
        hs.sync()
        for _ in range(tpm.BACKLOG_REPS):
            hs._chk(hs.lib.hobbit_f_binop(hs.ctx, 2, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), tpm.BACKLOG_N))
        pc2 = hs.commit_parity_matrix_device(n)
        busy = not stream.query()
        libc.srandom(77); got = hs.open_parity_matrix(pc2, r1, r2)
        assert np.array_equal(pc2.root(), root)
        same_opening(got, want)
        assert busy, "the commit returned to an idle stream: it waited, or the backlog is too short"
        pc2.free()
    finally:
        hs.close()


@pytest.mark.gpu
def test_opening_of_a_device_built_commitment(hb, oracle):
    n = 1024
    want = model(oracle, n)
    r1, r2 = start(oracle, n); hb.upload_graphs(n, graphs(oracle, n))
    pc = hb.commit_parity_matrix_device(n)
    got = hb.open_parity_matrix(pc, r1, r2)
    assert got["checks"].tolist() == [1, 1]
    same_opening(got, want["open"])
    pc.free()
