"""Every handle of the C ABI gives back what it took: hobbit_mem_live() -- the library's own count of live device and pinned allocations
-- reads the same before a context is created and after it is destroyed, whatever was created, freed (finished or not) and parked in between.

Every case makes its own context (in_fresh_context) and does all its work inside a function, so that no Python wrapper of a device buffer is
alive when the context goes.  The results that have a cheap reference are compared on the way (roots against the oracle); the shapes are the
smallest the handles' own test files use.  No case provokes an error on the device: the error returns are tests/mem_owner_check.cpp's."""
import ctypes
import gc

import numpy as np
import pytest

from adversarial import graphs_from
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
V, S, I32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
libc = ctypes.CDLL(None)


def _mod():
    from __graft_entry__ import load_package
    return load_package()


def live():
    a, b = S(), S()
    _mod().load_library().hobbit_mem_live(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def in_fresh_context(body, stream=None):
    """body(hb) on a context of its own; the live count after hobbit_ctx_destroy is the one from before hobbit_ctx_create"""
    gc.collect()
    before = live()
    hb = _mod().Hobbit(0, stream=stream)
    try:
        body(hb)
        gc.collect()
    finally:
        hb.close()
    assert live() == before, "allocations (count, bytes) before the context and after its destruction"


def oracle_graphs(hb, oracle, n):
    oracle.rng_reset(); oracle.expander_init_store(n)
    hb.upload_graphs(n, graphs_from(oracle, n))


# ---- Our_PC commit: the parked tensor / levels pair ------------------------------------------------------------------------------------------
_WANT = {}


def commit_root(oracle, N, K, trs):
    """the oracle's root of commit_standard(splitmix(N), K, trs, linear_time), once per shape; leaves the oracle's graphs for n = trs"""
    oracle.rng_reset(); oracle.expander_init_store(trs)
    if (N, K) not in _WANT:
        _WANT[(N, K)] = oracle.commit_standard(splitmix_field(N, 41), K, trs, 1)[0][-1].copy()
    return _WANT[(N, K)]


def test_commit_parks_adopts_and_releases(oracle):
    trs = 16
    (N1, K1), (N2, K2) = (1 << 20, 32), (1 << 19, 16)                  # the smoke shape; then the same leaf count with half the tensor
    want1, want2 = commit_root(oracle, N1, K1, trs), commit_root(oracle, N2, K2, trs)
    tensor_bytes = lambda N: 4 * N * 16                                 # K chunks x (2 N / K / trs) columns x 2 trs rows of 16 bytes

    def body(hb):
        hb.upload_graphs(trs, graphs_from(oracle, trs))
        d = hb.to_device(splitmix_field(N1, 41))                        # the polynomial of both shapes: the second takes its first half
        c = hb.commit_standard((d, N1), K1, trs, 1)
        assert np.array_equal(c.root(), want1)
        c.free()
        parked = live()                                                 # the pair is parked, the commit's scratch and tables exist
        c = hb.commit_standard((d, N1), K1, trs, 1)                     # the same shape adopts the pair: nothing new
        got = live()
        assert got[0] <= parked[0] and got[1] <= parked[1], (parked, got)
        assert np.array_equal(c.root(), want1)
        c.free()
        assert live() == parked
        c = hb.commit_standard((d, N2), K2, trs, 1)                     # another tensor size: the parked pair goes before the new one comes
        got = live()
        assert got[0] <= parked[0] and got[1] <= parked[1] - (tensor_bytes(N1) - tensor_bytes(N2)), (parked, got)
        assert np.array_equal(c.root(), commit_root(oracle, N2, K2, trs)) and np.array_equal(c.root(), want2)
        c.free()
    in_fresh_context(body)


def test_open_with_its_helper_contexts(oracle):
    """open_standard creates the helper contexts of the concurrent inner proofs; they go with their owner"""
    N, K, trs = 1 << 20, 32, 16
    want = commit_root(oracle, N, K, trs)

    def body(hb):
        hb.upload_graphs(trs, graphs_from(oracle, trs))
        poly = splitmix_field(N, 41)
        c = hb.commit_standard(poly, K, trs, 1)
        assert np.array_equal(c.root(), want)
        libc.srandom(5)
        g = hb.open_standard(poly, c, splitmix_field(20, 42), 5900, want_paths=False)
        assert g["checks"].tolist() == [1, 1, 1]
        c.free()
    in_fresh_context(body)


# ---- parity matrix: the five parked buffers, keyed by (P, n) -------------------------------------------------------------------------------------
def test_parity_parks_adopts_and_releases():
    def body(hb):
        hb.rng_reset(); hb.expander_init_store(16)
        a = hb.commit_parity_matrix_device(16); root = a.root(); a.free()
        parked = live()
        b = hb.commit_parity_matrix_device(16)                          # adopts the five buffers
        got = live()
        assert got[0] <= parked[0] and got[1] <= parked[1], (parked, got)
        assert np.array_equal(b.root(), root)
        h = hb.commit_parity_matrix(16)                                 # the host-built path, with its pinned copies; the set is taken: allocates
        assert np.array_equal(h.root(), root)
        h.free(); b.free()
        hb.rng_reset(); hb.expander_init_store(32)
        c = hb.commit_parity_matrix_device(32)                          # another (P, n): the parked set goes first
        h = hb.commit_parity_matrix(32)
        assert np.array_equal(c.root(), h.root())
        c.free(); h.free()
    in_fresh_context(body)


# ---- every other handle: twice to the end, once freed mid-stream ------------------------------------------------------------------------------
def test_elastic_commit_and_opens():
    def body(hb):
        lib, N, B = hb.lib, 1 << 18, 1 << 14
        d = hb.fill_splitmix(B, 7)
        roots = [hb.elastic_commit(N, B, 1, chunk=d, levels="device")[0] for _ in range(2)]
        assert np.array_equal(roots[0], roots[1])
        e = V()
        hb._chk(lib.hobbit_elastic_begin(hb.ctx, S(B), I32(B >> 11), I32(0), I32(1), ctypes.byref(e)))
        hb._chk(lib.hobbit_elastic_push(hb.ctx, e, V(d.ptr)))
        lib.hobbit_elastic_free(e)                                      # one push queued, no finish
        x = splitmix_field(18, 8)
        res = []
        for _ in range(2):
            libc.srandom(901); res.append(hb.elastic_open(N, B, x, 700, chunk=d, shockwave=False))
        assert res[0]["checks"].tolist() == [1, 1] and np.array_equal(res[0]["cf_root"], res[1]["cf_root"]) and np.array_equal(res[0]["reply"], res[1]["reply"])
        hb._chk(lib.hobbit_elastic_open_begin(hb.ctx, S(N), S(B), I32(B >> 11), x.ctypes.data_as(V), I32(700), ctypes.byref(e)))
        hb._chk(lib.hobbit_elastic_open_aggregate_push(hb.ctx, e, V(d.ptr)))
        lib.hobbit_elastic_open_free(e)
        # option 2 (RS x expander): trs = B >> 14 = 4, five more buffers
        N2, B2 = 1 << 20, 1 << 16
        d2 = hb.fill_splitmix(B2, 9); x2 = splitmix_field(20, 10)
        hb.rng_reset(); hb.expander_init_store(B2 >> 14)
        res = []
        for _ in range(2):
            libc.srandom(902); res.append(hb.elastic_open2(N2, B2, x2, 5900, chunks=lambda i: d2))
        assert res[0]["checks"].tolist() == [1] and np.array_equal(res[0]["cc_root"], res[1]["cc_root"]) and np.array_equal(res[0]["reply"], res[1]["reply"])
        hb._chk(lib.hobbit_elastic_open_begin_lin(hb.ctx, S(N2), S(B2), I32(B2 >> 14), x2.ctypes.data_as(V), I32(5900), ctypes.byref(e)))
        hb._chk(lib.hobbit_elastic_open_aggregate_push(hb.ctx, e, V(d2.ptr)))
        lib.hobbit_elastic_open_free(e)
    in_fresh_context(body)


def test_brakedown_and_its_streaming_form(oracle):
    def body(hb):
        lib = hb.lib
        N = 1 << 16; B = hb.brakedown_shape(N)[0]
        oracle_graphs(hb, oracle, B)
        d = hb.fill_splitmix(N, 11)
        roots = []
        for _ in range(2):
            c = hb.brakedown_commit((d, N)); roots.append(c.root()); c.free()
        assert np.array_equal(roots[0], roots[1])
        h = V()
        hb._chk(lib.hobbit_brakedown_commit(hb.ctx, V(d.ptr), S(N), I32(1), ctypes.byref(h)))
        lib.hobbit_brakedown_free(h)                                    # freed while its kernels are queued
        Bs, k = 1 << 13, 8
        oracle_graphs(hb, oracle, Bs)
        x = splitmix_field(3, 12); r0 = splitmix_field(1, 13)[0]; Iq = np.arange(0, 2 * Bs, 97, dtype=np.uint64)
        lv = [hb.brakedown_stream_commit([d] * k, Bs, levels="device") for _ in range(2)]
        assert np.array_equal(hb.to_host(lv[0], (4 * Bs - 1, 32), np.uint8), hb.to_host(lv[1], (4 * Bs - 1, 32), np.uint8))
        o = [hb.brakedown_stream_open([d] * k, [d] * k, Bs, k, x, r0, Iq, levels=lv[0]) for _ in range(2)]
        assert np.array_equal(o[0]["reply"], o[1]["reply"]) and np.array_equal(o[0]["aggr_beta"], o[1]["aggr_beta"])
        hb._chk(lib.hobbit_brakedown_stream_begin(hb.ctx, S(Bs), I32(1), ctypes.byref(h)))
        assert lib.hobbit_brakedown_stream_device_bytes(h) == 192 * Bs
        hb._chk(lib.hobbit_brakedown_stream_push(hb.ctx, h, V(d.ptr)))
        lib.hobbit_brakedown_stream_free(h)
        beta = np.ascontiguousarray(o[0]["beta"]); rv = np.ascontiguousarray(o[0]["r_v"])
        hb._chk(lib.hobbit_brakedown_stream_open_begin(hb.ctx, S(Bs), S(k), beta.ctypes.data_as(V), rv.ctypes.data_as(V), Iq.ctypes.data_as(V), S(len(Iq)), ctypes.byref(h)))
        assert lib.hobbit_brakedown_stream_open_device_bytes(h) == (8 * Bs + 2 * Bs + 2 * k + len(Iq) * k) * 16 + len(Iq) * 4
        hb._chk(lib.hobbit_brakedown_stream_open_aggregate_push(hb.ctx, h, V(d.ptr)))
        lib.hobbit_brakedown_stream_open_free(h)
    in_fresh_context(body)


def test_orion_and_brakingbase(oracle):
    import brakingbase_model as bm
    import orion_model as om

    def body(hb):
        poly, x = om.begin(oracle, 14)
        hb.upload_graphs(om.shape(1 << 14)[0], om.graphs(oracle, om.shape(1 << 14)[0]))
        d = hb.to_device(poly)
        roots = []
        for _ in range(2):
            c = hb.orion_commit((d, 1 << 14)); roots.append(c.root())
            libc.srandom(3); assert c.open(x, want_paths=False)["checks"].tolist() == [1, 1]
            c.free()
        assert np.array_equal(roots[0], roots[1])
        hb.orion_commit((d, 1 << 14), sync=False).free()               # freed while its kernels are queued
        logn, K = 9, 4
        poly = bm.start(oracle, 1 << logn, K); x = oracle.generate_randomness(logn)
        hb.upload_graphs((1 << logn) // K, bm.graphs(oracle, (1 << logn) // K))
        d = hb.to_device(poly)
        roots = []
        for _ in range(2):
            c = hb.brakingbase_commit((d, 1 << logn), K); roots.append(c.root())
            libc.srandom(3); assert c.open(x)["checks"].tolist() == [1, 1]
            c.free()
        assert np.array_equal(roots[0], roots[1])
        hb.brakingbase_commit((d, 1 << logn), K, sync=False).free()
    in_fresh_context(body)


# ---- the finalized code's device tables ------------------------------------------------------------------------------------------------------------
def test_graph_finalize_twice_then_reset(oracle):
    def body(hb):
        def cycle():
            base = live()
            for n in (4096, 1000):                                      # the deep code with its fat and narrow forms, then a plain one over it
                oracle_graphs(hb, oracle, n)
                assert live()[0] > base[0]
                a = hb.encode_monolithic(splitmix_field(n, 3))
                assert np.array_equal(a, oracle.encode_monolithic(splitmix_field(n, 3))[0][:a.shape[0]])
            hb._chk(hb.lib.hobbit_graph_reset(hb.ctx))
            return live()
        before = live()
        first = cycle()                                                 # leaves what the pool parks (two buffers per encode) and the workspaces hold
        assert first[0] <= before[0] + 4 + 5, (before, first)
        assert cycle() == first                                         # ... and nothing else: every device table of both codes went with the reset
    in_fresh_context(body)


# ---- contexts side by side, and on a caller's stream --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first_out", [0, 1])
def test_two_contexts_either_order(first_out):
    gc.collect()
    before = live()
    hbs = [_mod().Hobbit(0), _mod().Hobbit(0)]
    for i, hb in enumerate(hbs):
        assert hb.fft_any(splitmix_field(1 << 13, i)).shape == (1 << 13, 2)
    gc.collect()
    hbs[first_out].close()
    assert live()[0] > before[0]                                        # the other context still holds its own
    assert hbs[1 - first_out].fft_any(splitmix_field(1 << 13, 5)).shape == (1 << 13, 2)
    gc.collect()
    hbs[1 - first_out].close()
    assert live() == before


def test_context_on_a_callers_stream():
    import torch
    s = torch.cuda.Stream()
    in_fresh_context(lambda hb: hb.fft_any(splitmix_field(4096, 7)), stream=s.cuda_stream)
    with torch.cuda.stream(s):
        t = torch.arange(1 << 10, device="cuda") * 2
        s.synchronize()
    assert int(t.sum()) == (1 << 10) * ((1 << 10) - 1)
