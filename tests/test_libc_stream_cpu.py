"""The host side of include/hobbit_libcgen.h (no GPU): reading glibc's TYPE_3 generator as a 31-word window, jumping it ahead and writing it
back.  The yardstick is libc itself (srandom / rand / random through ctypes), never the code under test."""
import ctypes
import os
import re
import numpy as np
import pytest
from __graft_entry__ import load_package, build_hip, ROOT

libc = ctypes.CDLL(None)
libc.random.restype = ctypes.c_long
libc.initstate.restype = ctypes.c_void_p
libc.initstate.argtypes = [ctypes.c_uint, ctypes.c_void_p, ctypes.c_size_t]
libc.setstate.restype = ctypes.c_void_p
libc.setstate.argtypes = [ctypes.c_void_p]
V = ctypes.c_void_p
M32 = 0xFFFFFFFF
ESTATE = -5


@pytest.fixture(scope="module")
def mod():
    build_hip()
    return load_package()


@pytest.fixture(scope="module")
def lib(mod):
    return mod.load_library()


def draws(n):
    """n real libc draws, rand() and random() alternating (they share the generator)"""
    return [libc.random() if i & 1 else libc.rand() for i in range(n)]


def skip(n):
    rnd = libc.random
    for _ in range(n):
        rnd()


def window(lib):
    w = np.zeros(31, np.uint32)
    assert lib.hobbit_libc_window(w.ctypes.data_as(V)) == 0
    return w


def model(w, n):
    """the next n draws of a window by the recurrence r_i = r_{i-3} + r_{i-31} mod 2^32 in Python integers"""
    r = [int(v) for v in w]
    out = []
    for _ in range(n):
        v = (r[-3] + r[-31]) & M32
        r.append(v)
        out.append(v >> 1)
    return out


def test_library_exports_every_declared_symbol(mod, lib):
    src = open(os.path.join(ROOT, "include", "hobbit_libcgen.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = sorted(set(re.findall(r"\b(hobbit_[a-z0-9_]+)\s*\(", src)))
    assert len(decl) == 10 and sorted(mod.LIBCGEN_SYMBOLS) == decl
    for s in decl:
        assert hasattr(lib, s), "missing export " + s


@pytest.mark.parametrize("seed", [1, 777])
@pytest.mark.parametrize("d", [0, 1, 30, 31, 32, 10 ** 6])
def test_window_and_recurrence_give_the_next_draws(lib, seed, d):
    libc.srandom(seed); skip(d)
    want = draws(100)
    libc.srandom(seed); skip(d)
    w = window(lib)
    assert model(w, 100) == want
    assert draws(100) == want, "the snapshot disturbed the generator"


@pytest.mark.parametrize("k", [0, 1, 2, 30, 31, 32, 100, 2 ** 20 + 7, 10 ** 7])
def test_advance_against_real_calls(lib, k):
    libc.srandom(42); skip(k)
    want = draws(64)
    libc.srandom(42)
    assert lib.hobbit_libc_advance(ctypes.c_uint64(k)) == 0
    assert draws(64) == want


@pytest.mark.parametrize("a,b", [(2 ** 39 + 12345, 2 ** 39 - 999), (2 ** 62 + 77, 2 ** 62 - 5)])
def test_advance_composes_at_64_bit_offsets(lib, a, b):
    """advance(a) then advance(b) leaves the window of advance(a + b), for a + b near 2^40 and 2^63.  This is the ONLY check of offsets beyond what
    real calls can reach (test_advance_against_real_calls stops at 10^7); it shows consistency of the jump, and the small offsets pin its base."""
    libc.srandom(9)
    assert lib.hobbit_libc_advance(ctypes.c_uint64(a)) == 0 and lib.hobbit_libc_advance(ctypes.c_uint64(b)) == 0
    two = window(lib)
    libc.srandom(9)
    assert lib.hobbit_libc_advance(ctypes.c_uint64(a + b)) == 0
    one = window(lib)
    assert np.array_equal(one, two)
    libc.srandom(9); w0 = window(lib); out = np.zeros(31, np.uint32)
    lib.hobbit_libc_jump(w0.ctypes.data_as(V), ctypes.c_uint64(a + b), out.ctypes.data_as(V))
    assert np.array_equal(out, one)
    assert draws(4) == model(w0, 4), "hobbit_libc_jump moved the generator"


@pytest.mark.parametrize("d", [0, 5, 31, 1000])
def test_set_window_of_window_is_the_identity(lib, d):
    libc.srandom(3); skip(d)
    want = draws(100)
    libc.srandom(3); skip(d)
    w = window(lib)
    assert lib.hobbit_libc_set_window(w.ctypes.data_as(V)) == 0
    assert draws(50) == want[:50]
    w = window(lib)                                   # again, now that the library's own block is the active state
    assert lib.hobbit_libc_set_window(w.ctypes.data_as(V)) == 0
    assert draws(50) == want[50:]
    libc.srandom(3); skip(d)                         # and srandom on that block seeds as ever
    assert draws(100) == want


@pytest.mark.parametrize("nbytes", [32, 64, 256])
def test_other_state_types_are_refused_and_left_alone(lib, nbytes):
    """after initstate with a 32-, 64- or 256-byte buffer (TYPE_1, TYPE_2, TYPE_4) every call that reads the process generator returns HOBBIT_ESTATE
    and the draws that follow equal a control's"""
    buf_a = ctypes.create_string_buffer(256); buf_b = ctypes.create_string_buffer(256)
    prev = libc.initstate(11, buf_b, nbytes)
    try:
        skip(7)
        want = draws(40)
        libc.initstate(11, buf_a, nbytes)
        skip(7)
        w = np.zeros(31, np.uint32)
        assert lib.hobbit_libc_window(w.ctypes.data_as(V)) == ESTATE
        assert draws(10) == want[:10]
        assert lib.hobbit_libc_advance(ctypes.c_uint64(5)) == ESTATE
        assert draws(10) == want[10:20]
        assert lib.hobbit_libc_set_window(w.ctypes.data_as(V)) == ESTATE
        assert draws(10) == want[20:30]
        # (hobbit_generate_randomness_dev / hobbit_graph_draw need a context: tests/test_libc_stream.py)
        assert draws(10) == want[30:]
    finally:
        libc.setstate(prev)


def test_the_standalone_checker_of_the_header_passes(tmp_path):
    """scripts/libcgen_check.cpp -- the header against libc with no library in between -- builds with the host compiler of the mirror and passes"""
    import subprocess
    cxx = "g++"                                       # the compiler build_host() needs anyway
    exe = str(tmp_path / "libcgen_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", os.path.join(ROOT, "scripts", "libcgen_check.cpp"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "libcgen_check ok" in p.stdout, p.stdout + p.stderr
