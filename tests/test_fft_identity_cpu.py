"""The checkers of tests/test_fft_any_length.py, checked themselves on the CPU: the decimation-in-time identity and the sparse formula
(tests/fft_identity.py) must hold for the oracle's transform at 2^10 and 2^12 in both directions, and must notice a wrong transform."""
import numpy as np
import pytest
from oracle.pyoracle import splitmix_field
import fft_identity as fi


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("logn", [10, 12])
def test_dit_identity_holds_for_the_oracle_transform(oracle, logn, inverse):
    half = 1 << (logn - 1)
    e, o = splitmix_field(half, 11), splitmix_field(half, 12)
    B = fi.NumpyBackend(oracle, lambda a, inv: oracle.fft(a, inverse=inv))
    assert fi.dit_identity(B, oracle, logn, e, o, inverse) == (True, True)
    # the twiddles the identity was checked with are the powers of the direction's root
    w = fi.direction_root(oracle, logn, inverse)
    tw = fi.twiddles_by_doubling(B, oracle, half, w)
    for k in (0, 1, 2, 3, half // 2 + 1, half - 1):
        assert np.array_equal(tw[k], fi.f_pow_scalar(oracle, w, k)), k


@pytest.mark.parametrize("inverse", [False, True])
def test_dit_identity_notices_a_wrong_transform(oracle, inverse):
    logn = 10
    half = 1 << (logn - 1)
    e, o = splitmix_field(half, 13), splitmix_field(half, 14)

    def one_wrong_output(at):
        def fft(a, inv):
            r = oracle.fft(a, inverse=inv)
            if a.shape[0] == 1 << logn:
                r[at, 0] ^= np.uint64(1)
            return r
        return fi.NumpyBackend(oracle, fft)

    assert fi.dit_identity(one_wrong_output(5), oracle, logn, e, o, inverse) == (False, True)
    assert fi.dit_identity(one_wrong_output(half + 5), oracle, logn, e, o, inverse) == (True, False)
    # the other direction's transform, and a missing 1/len, fail both halves
    swapped = fi.NumpyBackend(oracle, lambda a, inv: oracle.fft(a, inverse=not inv))
    assert fi.dit_identity(swapped, oracle, logn, e, o, inverse) == (False, False)
    if inverse:
        unscaled = fi.NumpyBackend(oracle, lambda a, inv: oracle.f_mul(oracle.fft(a, inverse=True), np.tile(np.array([[a.shape[0], 0]], np.uint64), (a.shape[0], 1))))
        assert fi.dit_identity(unscaled, oracle, logn, e, o, True) == (False, False)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("logn", [10, 12])
def test_sparse_formula_matches_the_oracle_transform(oracle, logn, inverse):
    ln = 1 << logn
    pos, val, starts = fi.sparse_case(logn, logn)
    assert len(pos) == fi.N_ENTRIES and len(starts) == fi.N_WINDOWS and len(set(pos.tolist())) == len(pos)
    assert {0, 1, ln // 2, ln - 1} <= set(pos.tolist()) and (val == fi.P - 1).all(axis=1).any()
    x = np.zeros((ln, 2), np.uint64); x[pos.astype(np.int64)] = val
    want = oracle.fft(x, inverse=inverse)
    got = fi.sparse_expected(oracle, logn, pos, val, starts, inverse)
    for s, g in zip(starts, got):
        assert np.array_equal(g, want[s:s + fi.WINDOW]), s
    # and it is the direction's formula, not the other one's
    other = fi.sparse_expected(oracle, logn, pos, val, starts, not inverse)
    assert not np.array_equal(other, got)
