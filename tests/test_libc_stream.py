"""The libc random stream drawn on the device (include/hobbit_libcgen.h): raw draws, generate_randomness, one expander level, the whole
expander_init_store, and the C++ mirror's two functions on either side of their switch-over sizes.

The yardstick is libc itself (srandom / rand / random through ctypes) and the host functions that existed before (hobbit_generate_randomness,
Hobbit._draw, Hobbit.expander_init_store), never the code under test.  hobbit_libc_window / hobbit_libc_advance, which place the controls, are
pinned against real calls on the CPU (tests/test_libc_stream_cpu.py).  Every comparison is exact.
"""
import ctypes
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")
libc = ctypes.CDLL(None)
libc.random.restype = ctypes.c_long
libc.initstate.restype = ctypes.c_void_p
libc.initstate.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t]
libc.setstate.restype = ctypes.c_void_p
libc.setstate.argtypes = [ctypes.c_void_p]
V = ctypes.c_void_p
ESTATE = -5
SEED = 5
FIRSTS = [0, 1, 5, 10 ** 6 + 1]
BIG = 2 ** 20 + 3


def _mod():
    from __graft_entry__ import load_package
    return load_package()


def draws(n):
    rnd = libc.rand
    return np.array([rnd() for _ in range(n)], np.uint32)


@pytest.fixture(scope="module")
def hb():
    h = _mod().Hobbit(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def control():
    """the first FIRSTS[-1] + BIG real draws after srandom(SEED), drawn once and shared"""
    libc.srandom(SEED)
    c = draws(FIRSTS[-1] + BIG)
    c.setflags(write=False)
    return c


def seed_window(hb, seed=SEED):
    libc.srandom(seed)
    return hb.libc_window()


def dev_draws(hb, w, first, n):
    return hb.to_host(hb.libc_draws_dev(w, first, n), (n,), np.uint32)


# ---- raw draws ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("first", FIRSTS)
@pytest.mark.parametrize("n", [1, 31, 32, 63, 64, 65, 1000, BIG])
def test_draws_dev_against_libc(hb, control, n, first):
    w = seed_window(hb)
    got = dev_draws(hb, w, first, n)
    assert np.array_equal(got, control[first:first + n])
    assert np.array_equal(draws(4), control[:4]), "hobbit_libc_draws_dev moved the process generator"


@pytest.mark.gpu
def test_draws_dev_at_the_kernel_s_own_sizes(hb, control):
    """one draw short of, exactly at and one past the run of one lane and the span of one workgroup (hobbit_libc_draws_shape), and two spans"""
    run, span = hb.libc_draws_shape()
    assert 0 < run < span and span % run == 0 and 2 * span + 1 <= BIG
    w = seed_window(hb)
    for n in (run - 1, run, run + 1, span - 1, span, span + 1, 2 * span - 1, 2 * span, 2 * span + 1):
        for first in FIRSTS:
            got = dev_draws(hb, w, first, n)
            assert np.array_equal(got, control[first:first + n]), (n, first)


@pytest.mark.gpu
def test_draws_dev_first_above_2_32(hb):
    """a first draw index past 2^32; the control is hobbit_libc_advance (pinned on the CPU against real calls) followed by real draws"""
    first, n = 2 ** 32 + 12345, 40000
    w = seed_window(hb)
    got = dev_draws(hb, w, first, n)
    libc.srandom(SEED)
    hb.libc_advance(first)
    assert np.array_equal(got, draws(n))


# ---- generate_randomness --------------------------------------------------------------------------------------------------------------------------------
def host_and_dev_randomness(hb, seed, lengths):
    """the host's and the device's polynomials of consecutive calls from one seed, and the 8 draws that follow on either side"""
    libc.srandom(seed)
    want = [hb.generate_randomness(n) for n in lengths]
    want_tail = draws(8)
    libc.srandom(seed)
    bufs = [hb.generate_randomness_dev(n) for n in lengths]
    got_tail = draws(8)                                  # before anything waits for the stream: the generator has moved at the call's return
    got = [hb.to_host(b, (n, 2), np.uint64) for b, n in zip(bufs, lengths)]
    return want, want_tail, got, got_tail


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 99, 100, 101, 199, 200, 201, 2 ** 16 + 37, 2 ** 22])
def test_generate_randomness_dev_against_host(hb, n):
    want, want_tail, got, got_tail = host_and_dev_randomness(hb, 7, [n])
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got_tail, want_tail)


@pytest.mark.gpu
@pytest.mark.parametrize("n1,whole_groups", [(300, True), (250, False)])
def test_generate_randomness_dev_back_to_back(hb, n1, whole_groups):
    """two calls equal the host's two calls; they equal ONE host call of the summed length only when the first length is a multiple of 100"""
    n2 = 150
    want, want_tail, got, got_tail = host_and_dev_randomness(hb, 8, [n1, n2])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and np.array_equal(got_tail, want_tail)
    libc.srandom(8)
    one = hb.generate_randomness(n1 + n2)
    assert np.array_equal(np.concatenate(got), one) == whole_groups


# ---- one level ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("L,R,degree", [(14, 2, 9), (2, 8, 12), (4096, 864, 9), (5000, 1055, 9)])
def test_graph_level_dev_against_host_loop(hb, L, R, degree):
    first = 3
    w = seed_window(hb, 13)
    draws(first)
    nbr, wt = hb._draw(L, R, degree)
    dn, dw = hb.libc_graph_level_dev(w, first, L, R, degree)
    got_nbr = hb.to_host(dn, (L * degree,), np.int64); got_w = hb.to_host(dw, (L * degree, 2), np.uint64)
    assert got_nbr.min() >= 0 and got_nbr.max() < R
    assert np.array_equal(got_nbr, nbr) and np.array_equal(got_w, wt)


# ---- the whole expander_init_store ----------------------------------------------------------------------------------------------------------------------
def code_fingerprint(hb, n):
    """the finalized code's forms, and the codeword of one full-range message"""
    forms = hb.encode_forms()
    msg = hb.fill_splitmix(n, 99)
    out = hb.alloc(2 * n * 16)
    hb._chk(hb.lib.hobbit_memset(hb.ctx, V(out.ptr), 0, ctypes.c_size_t(2 * n * 16)))
    hb._chk(hb.lib.hobbit_encode_batch(hb.ctx, V(msg.ptr), V(out.ptr), ctypes.c_longlong(n), ctypes.c_size_t(1), ctypes.c_size_t(n), ctypes.c_size_t(2 * n)))
    return forms, hb.to_host(out, (2 * n, 2), np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [14, 67, 1000, 4096, 5000, 2 ** 16])
def test_graph_draw_against_expander_init_store(hb, n):
    libc.srandom(21)
    want_len = hb.expander_init_store(n)
    want_tail = draws(8)
    want_forms, want_cw = code_fingerprint(hb, n)
    libc.srandom(21)
    got_len = hb.graph_draw(n)
    got_tail = draws(8)
    got_forms, got_cw = code_fingerprint(hb, n)
    assert got_len == want_len and got_forms == want_forms
    assert np.array_equal(got_tail, want_tail)
    assert np.array_equal(got_cw, want_cw)
    for (dep, kind), (L, R, d, nbr, w) in hb._graph_levels.items():          # the store holds the host loop's arrays
        gl, gr, gd, pn, pw = ctypes.c_longlong(), ctypes.c_longlong(), ctypes.c_int(), V(), V()
        hb._chk(hb.lib.hobbit_graph_level_host(hb.ctx, dep, kind, ctypes.byref(gl), ctypes.byref(gr), ctypes.byref(gd), ctypes.byref(pn), ctypes.byref(pw)))
        assert (gl.value, gr.value, gd.value) == (L, R, d)
        assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(pn, ctypes.POINTER(ctypes.c_int64)), (L * d,)), nbr)
        assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(pw, ctypes.POINTER(ctypes.c_uint64)), (L * d, 2)), w)


@pytest.mark.gpu
@pytest.mark.parametrize("nbytes", [32, 64, 256])
def test_other_state_types_are_refused_with_a_live_context(hb, nbytes):
    buf_a = ctypes.create_string_buffer(256); buf_b = ctypes.create_string_buffer(256)
    prev = libc.initstate(11, buf_b, nbytes)
    try:
        want = draws(20)
        libc.initstate(11, buf_a, nbytes)
        b = hb.alloc(16 * 1000)
        assert hb.lib.hobbit_generate_randomness_dev(hb.ctx, ctypes.c_size_t(1000), V(b.ptr)) == ESTATE
        assert np.array_equal(draws(10), want[:10])
        ln = ctypes.c_longlong()
        assert hb.lib.hobbit_graph_draw(hb.ctx, ctypes.c_longlong(1000), ctypes.byref(ln)) == ESTATE
        assert np.array_equal(draws(10), want[10:])
    finally:
        libc.setstate(prev)


# ---- the C++ mirror -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("above", [True, False])
def test_mirror_same_with_the_device_path_on_and_off(above):
    """generate_randomness + expander_init_store + commit_standard of libhobbit_host.so from one seed, once with HOBBIT_HOST_LIBC_DEVICE=0 and once
    without: the same polynomial, root, next libc draw and contents of _C / D, above and below the sizes from which the mirror draws on the device"""
    from __graft_entry__ import build_host
    build_host()
    lib = ctypes.CDLL(os.path.join(PKG, "libhobbit_host.so"))
    rmin, gmin = ctypes.c_int(), ctypes.c_longlong()
    lib.hobbit_host_libc_stream_sizes(ctypes.byref(rmin), ctypes.byref(gmin))
    K = 4
    if above:
        trs = max(4096, gmin.value); N = max(1 << 18, rmin.value, 4 * K * trs)
        assert N & (N - 1) == 0 and trs & (trs - 1) == 0
    else:
        N, trs = 1 << 11, 64
        assert N < rmin.value and trs < gmin.value
    lib.hobbit_host_libc_stream.argtypes = [ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_uint, V, V, V, V]
    def counts():
        r, g = ctypes.c_longlong(), ctypes.c_longlong()
        lib.hobbit_host_libc_stream_counts(ctypes.byref(r), ctypes.byref(g))
        return r.value, g.value

    runs = []
    saved = os.environ.get("HOBBIT_HOST_LIBC_DEVICE")
    try:
        for off in (True, False):
            if off:
                os.environ["HOBBIT_HOST_LIBC_DEVICE"] = "0"
            else:
                os.environ.pop("HOBBIT_HOST_LIBC_DEVICE", None)
            poly = np.zeros((N, 2), np.uint64); root = np.zeros(32, np.uint8); nxt = ctypes.c_long(); dig = ctypes.c_uint64()
            before = counts()
            levels = lib.hobbit_host_libc_stream(N, K, trs, 31, poly.ctypes.data_as(V), root.ctypes.data_as(V), ctypes.byref(nxt), ctypes.byref(dig))
            took = tuple(b - a for a, b in zip(before, counts()))
            # the device path served both calls exactly when the switch is on and the sizes are above; otherwise the loops served both
            assert took == ((1, 1) if above and not off else (0, 0)), (above, off, took)
            runs.append((levels, poly, root, nxt.value, dig.value))
    finally:
        if saved is None:
            os.environ.pop("HOBBIT_HOST_LIBC_DEVICE", None)
        else:
            os.environ["HOBBIT_HOST_LIBC_DEVICE"] = saved
        lib.hobbit_host_close()
    a, b = runs
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]
    libc.srandom(31)                                      # and the polynomial is the host loop's, not merely the same twice
    want = np.zeros((1000, 2), np.uint64)
    _mod().load_library().hobbit_generate_randomness(ctypes.c_size_t(1000), want.ctypes.data_as(V))
    assert np.array_equal(a[1][:1000], want)
