"""The leaf-chain index rule behind k_leaf_chain_half_rs and the surface of include/hobbit_real_rs.h, checked with the oracle alone (no GPU).

Under RS x RS the column code is a transform of rows2 = 2 trs points, so T(r, cols - c) = conj(T((rows2 - r) mod rows2, c)) (identity 3 of
tests/test_elastic_real_cpu.py).  A leaf (j, c) hashes the four entries T(4j + e, c), e = 0 .. 3.  For c > cols / 2 these are the conjugates of stored
rows (rows2 - 4j - e) mod rows2 of column cols - c; with G = rows2 / 4 groups and g = G - 1 - j that is, in hashing order,
    row 4 (g + 1) mod rows2   -- the first row of the NEXT stored group, wrapping to row 0 --   then rows 4g + 3, 4g + 2, 4g + 1.
leaf_rows below is that rule written once more in Python; the device kernel is checked through tests/test_commit_real_rs.py.
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


def leaf_rows(j, rows2):
    """stored rows of column cols - c whose conjugates leaf (j, c > cols/2) hashes, in hashing order"""
    G = rows2 // 4; g = G - 1 - j
    return [(4 * (g + 1)) % rows2, 4 * g + 3, 4 * g + 2, 4 * g + 1]


@pytest.mark.parametrize("cols", [8, 64])
@pytest.mark.parametrize("trs", [4, 8])
def test_leaf_index_rule_against_the_oracle(oracle, trs, cols):
    rows2 = 2 * trs; M = trs * cols // 2; hc = cols // 2
    x = np.random.default_rng(trs * cols).integers(0, P, M, dtype=np.uint64)
    T = oracle.compute_tensorcode(widen(x), trs, 0)
    assert T.shape == (rows2, cols, 2)
    ascending_holds = True
    for j in range(rows2 // 4):
        rows = leaf_rows(j, rows2)
        assert sorted(rows[1:]) == [r for r in range(4 * (rows2 // 4 - 1 - j) + 1, 4 * (rows2 // 4 - 1 - j) + 4)] and rows[0] % 4 == 0
        for c in range(hc + 1, cols):
            leaf = T[4 * j:4 * j + 4, c]
            assert np.array_equal(leaf, conj(T[rows, cols - c])), (j, c)
            ascending_holds &= np.array_equal(leaf, conj(T[sorted(rows), cols - c]))
    assert not ascending_holds                                 # the order matters: the same rows ascending are another leaf
    assert leaf_rows(0, rows2)[0] == 0                         # the wrap: the last stored group's mirror starts at row 0


def test_header_and_symbol_list_agree():
    from __graft_entry__ import load_package
    mod = load_package()
    src = open(os.path.join(ROOT, "include", "hobbit_real_rs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    decl = sorted(set(re.findall(r"\b(hobbit_[a-z0-9_]+)\s*\(", src)))
    assert len(decl) == 4 and sorted(mod.REAL_RS_SYMBOLS) == decl
    for other in (mod.ABI_SYMBOLS, mod.PARITY_SYMBOLS, mod.PARITY_LISTS_SYMBOLS, mod.WHIR_SYMBOLS, mod.BRAKINGBASE_SYMBOLS, mod.LONGCODES_SYMBOLS,
                  mod.LIBCGEN_SYMBOLS, mod.REAL_SYMBOLS, mod.ELASTIC_REAL_SYMBOLS, mod.ORION_SYMBOLS):
        assert not set(decl) & set(other)
    lib = mod.load_library()
    for s in decl:
        assert hasattr(lib, s) and getattr(lib, s).argtypes is not None, s
