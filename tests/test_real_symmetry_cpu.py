"""The two identities behind include/hobbit_real.h, checked with the oracle alone (no GPU).

conj(a + bi) = a - bi is the Frobenius map of F_{p^2}, p = 2^61 - 1.  A root of unity w of order 2^12 divides p + 1 = 2^61, so conj(w) = w^p = 1/w.

  rows     the transform X of a base-field row satisfies X[4096 - k] = conj(X[k]), and X[0 .. 2048] follow from ONE 2048-point transform Z of the
           row packed two reals to an element, z[j] = x[2j] + i x[2j+1]:
               E[k] = (Z[k] + conj(Z[-k])) / 2,  O[k] = (Z[k] - conj(Z[-k])) / (2i),  X[k] = E[k] + w^k O[k] (k < 2048),  X[2048] = E[0] - O[0];
  columns  the drawn expander graphs have base-field weights, so Enc(conj x) = conj(Enc x) -- and one weight with img != 0 breaks it, which is
           why hobbit_commit_standard_real refuses such graphs.

The arithmetic below is Python integers, the transforms and the encodes are the oracle's.
"""
import os
import re

import numpy as np
import pytest

from oracle.pyoracle import splitmix_field

P = (1 << 61) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def conj(a):
    a = np.asarray(a, np.uint64).copy()
    im = a[..., 1]
    a[..., 1] = np.where(im == 0, 0, np.uint64(P) - im)
    return a


def real_rows():
    rng = np.random.default_rng(2048)
    rows = [rng.integers(0, P, 2048, dtype=np.uint64), np.full(2048, P - 1, np.uint64), rng.integers(0, 1 << 33, 2048, dtype=np.uint64)]
    for pos in (0, 1, 2047):
        e = np.zeros(2048, np.uint64); e[pos] = 1
        rows.append(e)
    return rows


def transform4096(oracle, x):
    a = np.zeros((4096, 2), np.uint64); a[:2048, 0] = x
    return oracle.fft(a)


def cmul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


@pytest.mark.parametrize("i", range(6))
def test_transform_of_a_real_row_is_conjugate_symmetric(oracle, i):
    X = transform4096(oracle, real_rows()[i])
    k = np.arange(1, 4096)
    assert np.array_equal(X[4096 - k], conj(X[k]))
    assert X[0, 1] == 0 and X[2048, 1] == 0                    # columns 0 and cols/2 are base-field themselves


@pytest.mark.parametrize("i", range(6))
def test_unpacking_identity_gives_columns_0_to_2048(oracle, i):
    x = real_rows()[i]
    X = transform4096(oracle, x)
    z = np.zeros((2048, 2), np.uint64); z[:1024, 0] = x[0::2]; z[:1024, 1] = x[1::2]       # the memory image of the reals, read as F
    assert z[:1024].tobytes() == x.tobytes()
    Z = oracle.fft(z)
    w = oracle.root_of_unity(12)
    w = (int(w[0]), int(w[1]))
    inv2 = 1 << 60
    assert (2 * inv2) % P == 1
    wk = (1, 0)
    E0 = O0 = None
    for k in range(2048):
        A = (int(Z[k, 0]), int(Z[k, 1])); Bz = Z[(2048 - k) % 2048]; B = (int(Bz[0]), (P - int(Bz[1])) % P)
        S = ((A[0] + B[0]) % P, (A[1] + B[1]) % P); D = ((A[0] - B[0]) % P, (A[1] - B[1]) % P)
        E = (S[0] * inv2 % P, S[1] * inv2 % P)
        O = (D[1] * inv2 % P, (P - D[0]) % P * inv2 % P)       # D / (2i) = -i D / 2
        if k == 0:
            E0, O0 = E, O
        T = cmul(wk, O)
        assert ((E[0] + T[0]) % P, (E[1] + T[1]) % P) == (int(X[k, 0]), int(X[k, 1])), k
        wk = cmul(wk, w)
    assert ((E0[0] - O0[0]) % P, (E0[1] - O0[1]) % P) == (int(X[2048, 0]), int(X[2048, 1]))


@pytest.mark.parametrize("n", [16, 64, 1024])
def test_encode_commutes_with_conjugation_on_the_drawn_graphs(oracle, n):
    oracle.rng_reset(); oracle.expander_init_store(n)
    x = splitmix_field(n, 61 + n)
    assert (x[:, 1] != 0).any()
    y, ln = oracle.encode_monolithic(x)
    yc, lnc = oracle.encode_monolithic(conj(x))
    assert ln == lnc and n < ln <= 2 * n
    assert np.array_equal(yc, conj(y))


@pytest.mark.parametrize("n", [16, 64, 1024])
def test_one_weight_off_the_base_field_breaks_it(oracle, n):
    oracle.rng_reset(); oracle.expander_init_store(n)
    g = oracle.graph(0, 0)
    w = g["w"].copy()
    assert (w[:, 1] == 0).all()
    w[3, 1] = 5                                                 # one weight with img != 0
    oracle.graph_set_weights(0, 0, w)
    try:
        x = splitmix_field(n, 61 + n)
        y, _ = oracle.encode_monolithic(x)
        yc, _ = oracle.encode_monolithic(conj(x))
        assert not np.array_equal(yc, conj(y))
    finally:
        oracle.graph_set_weights(0, 0, g["w"])


def test_header_and_symbol_list_agree():
    from __graft_entry__ import load_package
    mod = load_package()
    src = open(os.path.join(ROOT, "include", "hobbit_real.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = sorted(set(re.findall(r"\b(hobbit_[a-z0-9_]+)\s*\(", src)))
    assert len(decl) == 8 and sorted(mod.REAL_SYMBOLS) == decl
