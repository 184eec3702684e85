"""The two kernels of csrc/hobbit_orion.hip on their own (include/hobbit_orion.h): the queried-column gather through an LDS tile, and the grid
of opening paths whose positions are computed on the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)
    yield h
    h.close()


@pytest.mark.parametrize("nrows,ld,nq", [(64, 64, 32), (70, 96, 1), (33, 40, 37), (256, 256, 128), (100, 131, 95)])
def test_gather(hb, nrows, ld, nq):
    """arr[q][c] = T[c][I[q]]: shapes that are and are not multiples of the 32 x 32 tile, the first and the last column, one column many times,
    and random ones"""
    g = np.random.default_rng(nrows + nq)
    T = g.integers(0, 1 << 61, (nrows, ld, 2), dtype=np.uint64)
    I = g.integers(0, ld, nq).astype(np.uint32)
    I[0] = ld - 1
    if nq > 4:
        I[1] = 0; I[2] = I[3] = I[nq - 1] = 7                            # boundary and duplicated indices
    got = hb.orion_gather(T, I)
    assert got.shape == (nq, nrows, 2)
    assert np.array_equal(got, T[:, I.astype(np.int64)].transpose(1, 0, 2))


def test_gather_refuses_an_index_past_the_row(hb):
    from __graft_entry__ import load_package
    T = np.zeros((8, 8, 2), np.uint64)
    with pytest.raises(load_package().HobbitError, match="rc=-2"):
        hb.orion_gather(T, np.array([0, 8], np.uint32))


@pytest.mark.parametrize("nq", [1, 3, 128])
@pytest.mark.parametrize("n,cols", [(1 << 14, 256), (1 << 9, 32)])
def test_grid_paths(hb, nq, n, cols):
    """pair (i, j) at index i nq + j is hobbit_merkle_paths' path of leaf (J[j] / 4) cols + I[i]; the corners of the grid are among the pairs"""
    g = np.random.default_rng(nq)
    leaves = g.integers(0, 256, (n, 32), dtype=np.uint8)
    dl = hb.alloc(64 * n)
    hb._chk(hb.lib.hobbit_memcpy_h2d(hb.ctx, dl.ptr, leaves.ctypes.data, leaves.nbytes))
    hb._chk(hb.lib.hobbit_merkle_levels(hb.ctx, dl.ptr, n, 0)); hb.sync()       # a conventional tree: every node differs from its sibling
    jmax = 4 * (n // cols)
    I = g.integers(0, cols, nq).astype(np.uint32); J = g.integers(0, jmax, nq).astype(np.uint32)
    I[0] = cols - 1; J[0] = jmax - 1
    if nq > 2:
        I[1] = 0; J[1] = 0; I[2] = I[0]; J[2] = 3
    depth = n.bit_length() - 1
    out = hb.orion_grid_paths(dl.ptr, n, cols, I, J)
    got = hb.to_host(out, (nq * nq, depth, 32), np.uint8)
    pos = ((J.astype(np.uint64) // 4)[None, :] * cols + I.astype(np.uint64)[:, None]).reshape(-1)
    want = np.zeros((nq * nq, depth, 32), np.uint8)
    hb._chk(hb.lib.hobbit_merkle_paths(hb.ctx, dl.ptr, n, pos.ctypes.data, len(pos), want.ctypes.data))
    assert pos.max() == n - 1
    assert np.array_equal(got, want)


def test_grid_paths_refuses_a_position_past_the_leaves(hb):
    from __graft_entry__ import load_package
    n, cols = 1 << 9, 32
    dl = hb.alloc(64 * n)
    for I, J in (([32], [0]), ([0], [64])):
        with pytest.raises(load_package().HobbitError, match="rc=-2"):
            hb.orion_grid_paths(dl.ptr, n, cols, np.array(I, np.uint32), np.array(J, np.uint32))
