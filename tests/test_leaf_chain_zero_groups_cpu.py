"""The identity k_leaf_chain relies on for the all-zero leaf groups, pinned against the oracle's own commitments (no GPU).

An RS x expander codeword ends at row code.len of its 2 trs rows, so the leaf groups j >= zero_from = (code.len + 3) / 4 are zero in every
chunk of every column, and their leaves are all the same 32 bytes

    Z_K:   st_0 = 0^32,   st_{i+1} = H(H(0^64) | st_i),   i = 0 .. K-1

which depend on K and on nothing else.  The commit computes Z_K on the host (blake3_zero_group_leaf in csrc/hobbit_blake3.hpp) and stores it
into those leaves instead of hashing them.  Here: every leaf with j >= zero_from of the oracle's commit_standard equals that chain, computed
with the host references of tests/commit_refs.py; some leaf below zero_from does not; and the header's function, compiled into the stand-alone
tests/zero_chain_check.cpp with the address and undefined-behaviour sanitizers, agrees with a plain loop and with the same references."""
import os
import subprocess

import numpy as np
import pytest

import commit_refs as cr
from oracle.pyoracle import splitmix_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")
# the oracle's codeword lengths: trs -> code.len, so zero_from is 7, 28, 110, 441 and 1762
CODE_LEN = {16: 27, 64: 110, 256: 440, 1024: 1761, 4096: 7045}


def zero_group_leaf(K):
    """Z_K from the two host references: the chain over K all-zero groups, and the same from the inner digests"""
    z = cr.leaf_chain(np.zeros((K, 1, 4, 2), np.uint64))
    zd = cr.orc().blake3_64(np.zeros((1, 64), np.uint8))
    assert np.array_equal(z, cr.chain_digests(np.repeat(zd[None], K, axis=0)))
    return z[0]


@pytest.mark.parametrize("trs", sorted(CODE_LEN))
def test_codeword_lengths(oracle, trs):
    oracle.rng_reset()
    assert oracle.expander_init_store(trs) == CODE_LEN[trs]


@pytest.mark.parametrize("N,K,trs,lin", [(5 << 11, 5, 64, 1), (1 << 13, 2, 4096, 1)])
def test_leaves_of_the_zero_groups_are_the_k_fold_chain(oracle, N, K, trs, lin):
    oracle.rng_reset()
    code_len = oracle.expander_init_store(trs)
    assert code_len == CODE_LEN[trs]
    zero_from, half, M = (code_len + 3) // 4, trs // 2, N // K
    cols = 2 * M // trs
    assert 0 < zero_from < half
    levels, tensor = oracle.commit_standard(splitmix_field(N, 1800 + K + trs), K, trs, lin, want_tensor=True)
    assert not tensor[:, 4 * zero_from:].any() and tensor[:, 4 * zero_from - 4:4 * zero_from].any()       # (K, 2 trs, cols, 2): zero_from is exact
    leaves = levels[:M].reshape(half, cols, 32)                                                              # leaf order j * cols + c
    z = zero_group_leaf(K)
    assert (leaves[zero_from:] == z).all(), "a leaf of an all-zero group is not Z_K"
    assert not (leaves[:zero_from] == z).all(axis=2).any(), "a leaf below zero_from equals Z_K"
    if K > 1:
        assert not np.array_equal(z, zero_group_leaf(K - 1)), "Z_K does not depend on K"


def test_host_constant_under_sanitizers(tmp_path):
    exe = str(tmp_path / "zero_chain_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(PKG, "csrc"),
                           os.path.join(ROOT, "tests", "zero_chain_check.cpp"), "-o", exe])
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    assert out[0::2] == ["1", "2", "32"]
    for K, hx in zip((1, 2, 32), out[1::2]):
        assert hx == bytes(zero_group_leaf(K)).hex(), K
