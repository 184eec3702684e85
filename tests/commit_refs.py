"""Plain host references of everything the commitments are made of: the Merkle tree with either parent rule, its sibling paths, the
Our_PC leaf chain, the inner digests of the sharded commit, the Elastic_PC streaming leaves and shockwave_commit's column digests.

Built on nothing but the oracle's two compressions, blake3_64 and hash_md (pinned to the real reference by tests/golden/blake.npz and
merkle.npz); everything else is numpy indexing that states the layout in one line.  tests/test_commit_refs_cpu.py anchors each helper to
the oracle's own restatement of the same object; tests/test_commit_kernels.py compares the device with them."""
import numpy as np

_ORC = None


def orc():
    global _ORC
    if _ORC is None:
        from oracle import pyoracle
        pyoracle.build_oracle()
        _ORC = pyoracle.Oracle()
    return _ORC


def _h(a):
    return np.ascontiguousarray(a, np.uint8).reshape(-1, 32)


def tree(leaves, quirk):
    """flat levels over n = 2^d leaves, leaves first, 2n - 1 nodes: parent = H(L | L) of the even node under the quirk
    (src/merkle_tree.cpp:275-280), H(L | R) otherwise"""
    lv = [_h(leaves)]
    while lv[-1].shape[0] > 1:
        p = lv[-1]
        left = p[0::2]
        lv.append(orc().blake3_64(np.concatenate([left, left if quirk else p[1::2]], axis=1)))
    return np.concatenate(lv)


def paths(levels, n, pos):
    """sibling paths of leaves `pos` of a flat tree over n leaves, in one gather: level l starts at sum_{t<l} n >> t"""
    depth = n.bit_length() - 1
    off = np.concatenate([[0], np.cumsum([n >> t for t in range(depth)])])[:depth].astype(np.int64)
    pos = np.asarray(pos, np.int64)
    return levels[off[None, :] + ((pos[:, None] >> np.arange(depth)[None, :]) ^ 1)]


def _groups(chunk):
    """(cols, 2 trs, 2) codeword-major -> the 4-row groups in leaf order p = j * cols + c: (M, 4, 2)"""
    cols, rows2 = chunk.shape[0], chunk.shape[1]
    return np.ascontiguousarray(chunk.reshape(cols, rows2 // 4, 4, 2).transpose(1, 0, 2, 3)).reshape(-1, 4, 2)


def leaf_chain(T, start=None):
    """T: the device's codeword-major tensor (K, cols, 2 trs, 2).  Leaf p = j * cols + c chains hash_md(rows 4j .. 4j+3 of column c of
    chunk i, state) over i = 0 .. K-1 (src/Our_PC.cpp:162-166); `start` (leaf order) is the state in front of chunk 0, zeros if None"""
    T = np.asarray(T, np.uint64)
    M = T.shape[1] * (T.shape[2] // 4)
    leaf = np.zeros((M, 32), np.uint8) if start is None else _h(start).copy()
    for i in range(T.shape[0]):
        leaf = orc().hash_md(_groups(T[i]), leaf)
    return leaf


def slot_order(leaves, cols, half_trs):
    """leaf order p = j * cols + c -> the relay's slot order g = c * half_trs + j"""
    return np.ascontiguousarray(_h(leaves).reshape(half_trs, cols, 32).transpose(1, 0, 2)).reshape(-1, 32)


def inner_digests(T):
    """H(rows 4j .. 4j+3 of column c) of every chunk, leaf order: (K, M, 32)"""
    T = np.asarray(T, np.uint64)
    return np.stack([orc().blake3_64(_groups(T[i]).view(np.uint8).reshape(-1, 64)) for i in range(T.shape[0])])


def chain_digests(digests, start=None):
    """leaf[p] = H(dig_i[p] | leaf[p]) over i = 0 .. K-1 for digests (K, M, 32): leaf_chain from its inner digests"""
    digests = np.asarray(digests, np.uint8)
    leaf = np.zeros(digests.shape[1:], np.uint8) if start is None else _h(start).copy()
    for i in range(digests.shape[0]):
        leaf = orc().blake3_64(np.concatenate([digests[i], leaf], axis=1))
    return leaf


def elastic_leaves(tensors, shift):
    """tensors: row-major (2 trs, cols, 2) per chunk.  Per group of four, leaf[p] = hash_md(c0[p + shift], c1[p + shift], c2[p], c3[p],
    leaf[p]) with p = row * cols + col and zeros past the end (src/Elastic_PC.cpp:228-243; shift = 1 is the reference as built by GCC).
    A trailing group of fewer than four chunks is ignored."""
    flat = [np.asarray(t, np.uint64).reshape(-1, 2) for t in tensors]
    sh = (lambda v: np.concatenate([v[shift:], np.zeros((shift, 2), np.uint64)])) if shift else (lambda v: v)
    leaf = np.zeros((flat[0].shape[0], 32), np.uint8)
    for g in range(len(flat) // 4):
        c = flat[4 * g:4 * g + 4]
        leaf = orc().hash_md(np.ascontiguousarray(np.stack([sh(c[0]), sh(c[1]), c[2], c[3]], 1)), leaf)
    return leaf


def col_digests(enc, k, quirk):
    """shockwave_commit's level 0 (src/Virgo.cpp:143-151): the digest of column c of enc (k, W, 2) is the root of MT_commit_Blake over its k
    entries -- k / 4 leaves H(4 consecutive entries), then the tree with the given parent rule"""
    enc = np.asarray(enc, np.uint64)
    W = enc.shape[1]
    blocks = np.ascontiguousarray(enc.reshape(k // 4, 4, W, 2).transpose(2, 0, 1, 3)).view(np.uint8).reshape(-1, 64)
    nodes = orc().blake3_64(blocks).reshape(W, k // 4, 32)
    while nodes.shape[1] > 1:
        left = nodes[:, 0::2]
        blocks = np.concatenate([left, left if quirk else nodes[:, 1::2]], axis=2)
        nodes = orc().blake3_64(blocks.reshape(-1, 64)).reshape(W, -1, 32)
    return np.ascontiguousarray(nodes[:, 0])
