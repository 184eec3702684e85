"""The big-integer references of tests/adversarial.py for the circuit prover's operations, against the oracle (no GPU).

tests/test_circuit_prover_shapes.py compares the device with these references at the small shapes and with the oracle at the large
ones; this file is what makes the two the same yardstick: every reference, written from its formula with Python integers, agrees bit
for bit with the oracle's C restatement (which the committed fixtures pin to the reference) on uniform data and on the families
that sit at the edges of the field arithmetic, at one element, two, an odd count below a wave and a count that is no power of two."""
import numpy as np
import pytest
from adversarial import (families, selectors, to_py, from_py, py_err2p, py_err3p, py_err4p, py_batch_terms, py_axpy, py_axpy_i32, py_fingerprint,
                         py_prepare_matrix_cols, py_fold_rows, py_phi_g, py_cubic_claim, py_mul, py_add, P, LK_VALUES)
from oracle.pyoracle import splitmix_field

SIZES = [1, 2, 63, 300]
FAMS = ("uniform", "all_pm1", "zeros", "bits", "limbs")
FULL = np.array([0x123456789ABCDEF % P, 0x0FEDCBA987654321 % P], np.uint64)
SCALARS = {"zero": [0, 0], "one": [1, 0], "minus_one": [P - 1, 0], "full": FULL}


def tables(n, fam, count, seed=0):
    """`count` tables of n elements of one family (the seeded families differ from table to table)"""
    if fam == "uniform":
        return [splitmix_field(n, 40 + seed + j) for j in range(count)]
    return [families(n, seed=seed + j)[fam] for j in range(count)]


def const(a, n):
    return np.tile(np.asarray(a, np.uint64).reshape(1, 2), (n, 1))


@pytest.mark.parametrize("n", SIZES)
def test_error_term_references(oracle, n):
    """py_err2p / py_err3p / py_err4p against the oracle: every family in the fold tables and in the chunk tables, every selector
    family, and the lookup maps with every selector value"""
    lr = splitmix_field(2, 449)
    for fam in FAMS:
        f = tables(n, fam, 5, seed=n)
        for b, tag in ((tables(n, "uniform", 3, seed=9), "chunks uniform"), (tables(n, fam, 3, seed=5), "chunks " + fam)):
            what = "n=%d folds %s %s" % (n, fam, tag)
            P_ = [to_py(x) for x in b + f]
            assert np.array_equal(from_py(py_err2p(P_[0], P_[1], P_[3], P_[4])), oracle.err2p(b[0], b[1], f[0], f[1])), what
            for lookups in (False, True):
                for sname, g in selectors(n, lookups).items():
                    w = "%s selector %s lookups=%d" % (what, sname, lookups)
                    oracle.set_lookups(lr if lookups else None)
                    try:
                        want3 = oracle.err3p(b[0], g, f[0], f[1], f[2], f[4])
                        want4 = oracle.err4p(b[0], b[1], b[2], g, f[0], f[1], f[2], f[3])
                    finally:
                        oracle.set_lookups(None)
                    got3 = py_err3p(P_[0], g, P_[3], P_[4], P_[5], P_[7], to_py(lr) if lookups else None)
                    got4 = py_err4p(P_[0], P_[1], P_[2], g, P_[3], P_[4], P_[5], P_[6], lookups)
                    assert np.array_equal(from_py(got3), want3), w + " err3p"
                    assert np.array_equal(from_py(got4), want4), w + " err4p"


def test_selector_families_cover_every_lookup_value():
    s = selectors(300, lookups=True)
    assert set(s) == {"zeros", "ones", "alternate", "only_last", "thirds", "lk_cycle"} | {"lk_all_%s" % v for v in ("m1", 0, 1, 2, 3, 4)}
    assert sorted(set(s["lk_cycle"].tolist())) == list(LK_VALUES)
    assert s["only_last"].tolist() == [0] * 299 + [1] and s["alternate"][:4].tolist() == [0, 1, 0, 1] and s["thirds"][:4].tolist() == [1, 0, 0, 1]
    assert all(v.dtype == np.int32 and v.shape == (300,) for v in s.values())
    assert all(set(v.tolist()) <= {0, 1} for v in selectors(7).values()) and selectors(1)["only_last"].tolist() == [1]


@pytest.mark.parametrize("n", SIZES)
def test_batch_term_reference(oracle, n):
    for fam in FAMS:
        t = tables(n, fam, 3, seed=n) + tables(n, "uniform", 3, seed=n + 1)
        for order in ((0, 1, 2, 3, 4, 5), (3, 4, 5, 0, 1, 2)):               # the family in the chunks, then in the folds
            x = [t[i] for i in order]
            assert np.array_equal(from_py(py_batch_terms(*[to_py(v) for v in x])), oracle.batch_prod_terms(*x)), (n, fam, order)


@pytest.mark.parametrize("n", SIZES)
def test_fold_and_fingerprint_references(oracle, n):
    """py_axpy, py_axpy_i32 and py_fingerprint against the oracle's f_add / f_mul, every scalar with every family"""
    one = const([1, 0], n)
    for fam in FAMS:
        x, v, fr = tables(n, fam, 3, seed=n)
        y = splitmix_field(n, 77)
        for an, a in SCALARS.items():
            what = "n=%d %s a=%s" % (n, fam, an)
            ap = to_py(a)[0]
            ax = oracle.f_mul(const(a, n), x)
            assert np.array_equal(from_py(py_axpy(to_py(y), ap, to_py(x))), oracle.f_add(y, ax)), what
            assert np.array_equal(from_py(py_axpy(to_py(x), ap, to_py(x))), oracle.f_add(x, ax)), what + " onto itself"
            for sname, s in selectors(n).items():
                sv = np.stack([s.astype(np.uint64), np.zeros(n, np.uint64)], 1)
                assert np.array_equal(from_py(py_axpy_i32(to_py(x), ap, s)), oracle.f_add(x, oracle.f_mul(const(a, n), sv))), what + " sel " + sname
                assert np.array_equal(from_py(py_axpy_i32(to_py(x), ap, s, True)),
                                      oracle.f_add(x, oracle.f_mul(const(a, n), oracle.f_sub(one, sv)))), what + " 1 - sel " + sname
            base = oracle.f_add(oracle.f_add(x, one), oracle.f_mul(const(a, n), v))
            assert np.array_equal(from_py(py_fingerprint(to_py(x), to_py(v), ap)), base), what + " fingerprint"
            for bn, b in SCALARS.items():
                assert np.array_equal(from_py(py_fingerprint(to_py(x), to_py(v), ap, to_py(fr), to_py(b)[0])),
                                      oracle.f_add(base, oracle.f_mul(const(b, n), fr))), what + " fingerprint with freq, b=" + bn


@pytest.mark.parametrize("rows,cols,k", [(1, 7, 0), (2, 1, 1), (8, 5, 3), (8, 5, 2)])
def test_prepare_matrix_reference(oracle, rows, cols, k):
    """py_prepare_matrix_cols against the oracle's prepare_matrix of the transpose: with k = log2 rows the evaluation over the row index,
    with fewer challenges the first entry of the partial fold"""
    for fam in FAMS:
        M = tables(rows * cols, fam, 1, seed=rows + k)[0].reshape(rows, cols, 2)
        r = splitmix_field(k, 331) if k else np.zeros((0, 2), np.uint64)
        want = oracle.prepare_matrix(np.ascontiguousarray(M.transpose(1, 0, 2)), r) if k else M[0]
        assert np.array_equal(from_py(py_prepare_matrix_cols(M, r)), want), (rows, cols, k, fam)
    M = splitmix_field(8 * 5, 3).reshape(8, 5, 2)
    rt = to_py(splitmix_field(1, 4))[0]
    folded = py_fold_rows([to_py(row) for row in M], rt)
    assert len(folded) == 4 and folded[3][2] == py_add(to_py(M[6, 2])[0], py_mul(rt, tuple((int(b) - int(a)) % P for a, b in zip(M[6, 2], M[7, 2]))))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6])
def test_phi_g_reference(oracle, n):
    sp = np.array([0, 1, P - 1, (P + 1) // 2], np.uint64)
    special = np.stack([sp[np.arange(n) % 4], np.zeros(n, np.uint64)], 1)
    w = to_py(oracle.root_of_unity(n))[0]
    for pname, rx in (("uniform", splitmix_field(n, 320 + n)), ("zeros", np.zeros((n, 2), np.uint64)), ("ones", const([1, 0], n)), ("special", special)):
        for ifft in (False, True):
            for scale in ((1, 0), (7, 3), (P - 1, P - 1)):
                got = py_phi_g(to_py(rx), w, scale, ifft)
                assert np.array_equal(from_py(got), oracle.phi_g_init(rx, scale, ifft)), (n, pname, ifft, scale)
                if not ifft and n >= 1:
                    assert all(v == (0, 0) for v in got[1 << (n - 1):]), "the forward table's upper half stays zero"


@pytest.mark.parametrize("lens", [[1], [1, 1], [2], [2, 1], [1, 2, 4, 64], [8, 8], [32, 2, 1]])
def test_cubic_claim_reference(oracle, lens):
    """py_cubic_claim is round 0's p(0) + p(1) of the oracle's batched cubic sumcheck (for tables that start at length 1 the round
    polynomial is linear with the product at 0 and zero at 1)"""
    tot = sum(lens)
    for fam in FAMS:
        t = tables(tot, fam, 3, seed=tot)
        a = splitmix_field(len(lens), 503)
        claim = py_cubic_claim(*[to_py(x) for x in t], lens, to_py(a))
        if max(lens) >= 2:
            q0 = to_py(oracle.batch_3product_sumcheck(t[0], t[1], t[2], lens, a)["poly"][0])
            assert claim == tuple((q0[0][c] + q0[1][c] + q0[2][c] + 2 * q0[3][c]) % P for c in range(2)), (lens, fam)
        else:
            want = oracle.f_mul(oracle.f_mul(t[0], t[1]), t[2])
            acc = np.zeros((1, 2), np.uint64)
            for j in range(len(lens)):
                acc = oracle.f_add(acc, oracle.f_mul(a[j:j + 1], want[j:j + 1]))
            assert claim == to_py(acc)[0], (lens, fam)
