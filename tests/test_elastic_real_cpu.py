"""The identities behind include/hobbit_elastic_real.h, checked with the oracle and Python integers alone (no GPU).

conj(a + bi) = a - bi is the Frobenius map of F_{p^2}, p = 2^61 - 1; a root of unity w of 2-power order divides p + 1 = 2^61, so conj(w) = 1/w.

  1  rows, any length L: the transform X of a base-field row of L/2 values, zero-padded, satisfies X[L - k] = conj(X[k]), and X[0 .. L/2] follow from
     ONE L/2-point transform Z of the row packed two reals to an element, pair by pair as k_real_unpack computes them:
         S = Z[k] + conj(Z[-k]), D = Z[k] - conj(Z[-k]), T = w^k (-i D):  X[k] = (S + T) / 2,  X[L/2 - k] = conj((S - T) / 2),  k = 0 .. L/4;
  2  columns, RS x expander: T(r, cols - c) = conj(T(r, c))                            (the encode itself: tests/test_real_symmetry_cpu.py);
  3  columns, RS x RS: T(r, cols - c) = conj(T((rows2 - r) mod rows2, c)), the column code being a transform of rows2 = 2 trs points.

half_ref below is csrc/hobbit_half.hpp's index function written once more in Python; the device function is checked through tests/test_elastic_real.py.
"""
import os
import re

import numpy as np
import pytest

P = (1 << 61) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conj(a):
    a = np.asarray(a, np.uint64).copy()
    im = a[..., 1]
    a[..., 1] = np.where(im == 0, 0, np.uint64(P) - im)
    return a


def widen(x):
    out = np.zeros(x.shape + (2,), np.uint64)
    out[..., 0] = x
    return out


def real_rows(h):
    """rows of h = L/2 reals: uniform, all p - 1, unit vectors at 0, 1, h - 1"""
    rows = [np.random.default_rng(h).integers(0, P, h, dtype=np.uint64), np.full(h, P - 1, np.uint64)]
    for pos in (0, 1, h - 1):
        e = np.zeros(h, np.uint64); e[pos] = 1
        rows.append(e)
    return rows


def cmul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


@pytest.mark.parametrize("i", range(5))
@pytest.mark.parametrize("logL", [3, 5, 12, 15])
def test_identity_1_rows_of_any_length(oracle, logL, i):
    L = 1 << logL; h = L // 2
    x = real_rows(h)[i]
    a = np.zeros((L, 2), np.uint64); a[:h, 0] = x
    X = oracle.fft(a)
    k = np.arange(1, L)
    assert np.array_equal(X[L - k], conj(X[k]))
    assert X[0, 1] == 0 and X[h, 1] == 0                       # columns 0 and cols/2 are base-field themselves
    z = np.zeros((h, 2), np.uint64); z[:h // 2, 0] = x[0::2]; z[:h // 2, 1] = x[1::2]       # the memory image of the reals, read as F
    assert z[:h // 2].tobytes() == x.tobytes()
    Z = oracle.fft(z)
    w = oracle.root_of_unity(logL); w = (int(w[0]), int(w[1]))
    inv2 = 1 << 60
    got = {}
    wk = (1, 0)
    for kk in range(h // 2 + 1):
        A = (int(Z[kk, 0]), int(Z[kk, 1])); Bz = Z[(h - kk) % h]; B = (int(Bz[0]), (P - int(Bz[1])) % P)
        S = ((A[0] + B[0]) % P, (A[1] + B[1]) % P); D = ((A[0] - B[0]) % P, (A[1] - B[1]) % P)
        T = cmul((D[1], (P - D[0]) % P), wk)                   # w^k (-i D)
        got[kk] = ((S[0] + T[0]) * inv2 % P, (S[1] + T[1]) * inv2 % P)
        if 2 * kk != h:
            got[h - kk] = ((S[0] - T[0]) * inv2 % P, (P - (S[1] - T[1]) * inv2 % P) % P)
        wk = cmul(wk, w)
    assert sorted(got) == list(range(h + 1))
    assert all(got[kk] == (int(X[kk, 0]), int(X[kk, 1])) for kk in range(h + 1))


def half_ref(r, c, cols, rows2, lin):
    """entry (r, c) of a chunk's full tensor -> (stored row, stored column <= cols/2, conjugate?)"""
    if c <= cols // 2:
        return r, c, False
    return (r if lin else (rows2 - r) % rows2), cols - c, True


def half_mirror_row(row, rows2, lin):
    return row if lin else (rows2 - row) % rows2


def chunk(B):
    return np.random.default_rng(B).integers(0, P, B, dtype=np.uint64)


@pytest.mark.parametrize("logB", [13, 14])
def test_identity_3_on_a_whole_chunk(oracle, logB):
    """row code, then the column transform of 2 trs points: every (r, c)"""
    B = 1 << logB; trs = B >> 11; rows2 = 2 * trs; cols = 4096
    T = oracle.compute_tensorcode(widen(chunk(B)), trs, 0)
    assert T.shape == (rows2, cols, 2)
    r = (rows2 - np.arange(rows2)) % rows2
    c = np.arange(1, cols)
    assert np.array_equal(T[:, cols - c], conj(T[r][:, c]))
    assert np.array_equal(T[:, 0], conj(T[r, 0])) and np.array_equal(T[:, cols // 2], conj(T[r, cols // 2]))     # columns 0 and cols/2 map to themselves
    assert not np.array_equal(T[1:, cols - c], conj(T[1:, c]))                                                   # ... and not without the row negation


@pytest.mark.parametrize("lin", [0, 1])
def test_index_function_against_the_identities(oracle, lin):
    """every (r, c) of a trs = 4 chunk is the stored entry half_ref names, conjugated where it says so"""
    B, trs, rows2, cols = 1 << 13, 4, 8, 4096
    if lin:
        oracle.rng_reset(); oracle.expander_init_store(trs)
    T = oracle.compute_tensorcode(widen(chunk(B)), trs, lin)
    stored = T[:, :cols // 2 + 1]
    for r in range(rows2):
        ref = [half_ref(r, c, cols, rows2, lin) for c in range(cols)]
        row = np.array([q[0] for q in ref]); col = np.array([q[1] for q in ref]); cj = np.array([q[2] for q in ref])
        assert col.max() <= cols // 2 and row.max() < rows2
        v = stored[row, col]
        assert np.array_equal(T[r], np.where(cj[:, None], conj(v), v)), r
        for sc in (1, 2, cols // 2 - 1):                       # the mirrored leaf of stored (r, sc) is the entry that half_ref sends back to it
            assert half_ref(half_mirror_row(r, rows2, lin), cols - sc, cols, rows2, lin) == (r, sc, True)


def test_header_and_symbol_list_agree():
    from __graft_entry__ import load_package
    mod = load_package()
    src = open(os.path.join(ROOT, "include", "hobbit_elastic_real.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = sorted(set(re.findall(r"\b(hobbit_[a-z0-9_]+)\s*\(", src)))
    assert len(decl) == 6 and sorted(mod.ELASTIC_REAL_SYMBOLS) == decl
    for other in (mod.ABI_SYMBOLS, mod.PARITY_SYMBOLS, mod.PARITY_LISTS_SYMBOLS, mod.WHIR_SYMBOLS, mod.BRAKINGBASE_SYMBOLS, mod.LONGCODES_SYMBOLS,
                  mod.LIBCGEN_SYMBOLS, mod.REAL_SYMBOLS, mod.ORION_SYMBOLS):
        assert not set(decl) & set(other)
    lib = mod.load_library()
    for s in decl:
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None, s
