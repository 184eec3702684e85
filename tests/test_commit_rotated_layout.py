"""The commit's rotated tensor layout (csrc/hobbit_rot.hpp): results stay what they were.

At trs = 4096 with rows of 4096 and a tensor of 64 MiB or more, hobbit_commit_standard's row FFT stores the codeword-major tensor itself and
rotates each column's message half inside its own ring; the encode's loader, the leaf chain, the gathers and the row reads go through the
rotated index, and hobbit_commitment_tensor_dev un-rotates once, in place, before the raw pointer leaves.  Nothing a caller can see may change.
The smallest shapes that take the path are N = K * 2^23 (512 MiB of tensor per chunk), K = 1, 2, 4.  For each:

  (a) root and all Merkle levels equal the tree over the leaves of the public, unrotated building blocks on the same polynomial:
      hobbit_tensorcode_chunks -> hobbit_leaf_chain -> hobbit_merkle_levels;
  (b) gathers and row reads, taken before any raw pointer was asked for, agree with hobbit_tensor_gather on that unrotated tensor;
  (c) hobbit_commitment_tensor_dev then returns a tensor byte-identical to the unrotated one, and (a), (b) still hold;
  (d) a second commit of another polynomial into the parked buffers gives that polynomial's tree, a third commit of the first polynomial the
      first tree again (the parked buffer is dirty and linear by then: the rotation is re-established);
  (e) K = 2: an opening verifies under tests/open_verifier.py and equals, array for array, the opening of a commitment that was un-rotated first.

That the path is taken at all (and not taken where it must not be) is read from the profiler's launch counts: no k_transpose in a rotated
commit, one k_unrotate_msg at the first raw pointer and none at the second.  The shape that must keep today's layout is trs = 1024 at 2^26,
against the real reference's root and level digests (tests/golden/bigroot_2e26.npz).
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
libc = ctypes.CDLL(None)
c_vp, c_sz = ctypes.c_void_p, ctypes.c_size_t
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TRS, COLS = 4096, 4096
PROBE_COLS = [0, 1, 255, 256, 4095]


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)
    h.rng_reset(); h.code_len = h.expander_init_store(TRS)
    yield h
    h.close()


class Unrotated:
    """tensor and tree of fill_splitmix(N, seed) from the public building blocks, none of which knows the rotation"""

    def __init__(self, hb, K, seed):
        self.hb, self.K, self.N, self.M = hb, K, K << 23, 1 << 23
        self.poly = hb.fill_splitmix(self.N, seed)
        self.tensor = hb.alloc(16 * 4 * self.N)
        hb._chk(hb.lib.hobbit_tensorcode_chunks(hb.ctx, c_vp(self.poly.ptr), c_sz(self.M), K, TRS, 1, c_vp(self.tensor.ptr)))
        lv = hb.alloc(64 * self.M)
        hb._chk(hb.lib.hobbit_memset(hb.ctx, c_vp(lv.ptr), 0, c_sz(32 * self.M)))           # hobbit_leaf_chain continues from what the leaves hold
        hb._chk(hb.lib.hobbit_leaf_chain(hb.ctx, c_vp(self.tensor.ptr), c_sz(self.M), K, TRS, 1, c_vp(lv.ptr)))
        hb._chk(hb.lib.hobbit_merkle_levels(hb.ctx, c_vp(lv.ptr), c_sz(self.M), 1))
        hb.sync()
        self.levels = hb.to_host(lv, (2 * self.M - 1, 32), np.uint8)
        lv.free()

    def gather(self, rows, cols):
        rows = np.ascontiguousarray(rows, np.uint32); cols = np.ascontiguousarray(cols, np.uint32)
        out = np.zeros((len(rows), self.K, 2), np.uint64)
        self.hb._chk(self.hb.lib.hobbit_tensor_gather(self.hb.ctx, c_vp(self.tensor.ptr), c_sz(self.M), self.K, TRS, rows.ctypes.data_as(c_vp),
                                                      cols.ctypes.data_as(c_vp), c_sz(len(rows)), out.ctypes.data_as(c_vp)))
        return out

    def free(self):
        self.poly.free(); self.tensor.free()


def launches(hb, fn):
    """fn() with every launch counted: {profile name: launches}"""
    hb.profile(True); hb.profile_reset()
    try:
        res = fn()
        hb.sync()
        rep = {k: v[1] for k, v in hb.profile_report().items()}
    finally:
        hb.profile(False); hb.profile_reset()
    return res, rep


def probe_rows(hb):
    rv = (hb.code_len + 3) & ~3                                 # rows_valid: the codeword's length rounded up to the leaf group
    assert TRS < hb.code_len < rv < 2 * TRS
    return [0, 7, 8, TRS - 1, TRS, rv - 1, rv, rv + 1, 2 * TRS - 1]


def check_reads(hb, c, ref):
    rows = probe_rows(hb)
    qr = np.repeat(rows, len(PROBE_COLS)); qc = np.tile(PROBE_COLS, len(rows))
    assert np.array_equal(c.gather(qr, qc), ref.gather(qr, qc))
    allc = np.arange(COLS)
    for chunk, r in ((0, 0), (ref.K - 1, 1), (0, TRS - 1), (ref.K - 1, TRS), (0, rows[5]), (0, rows[6])):
        assert np.array_equal(c.tensor_row(chunk, r), ref.gather(np.full(COLS, r), allc)[:, chunk]), (chunk, r)


@pytest.mark.parametrize("K", [1, 2, 4])
def test_rotated_commit_is_the_unrotated_commit(hb, K):
    ref = Unrotated(hb, K, 700 + K)
    N = ref.N
    c, rep = launches(hb, lambda: hb.commit_standard((ref.poly, N), K, TRS, 1))
    assert rep.get("k_fft4096", 0) >= 1 and "k_transpose" not in rep, rep        # the rotated path: the row FFT stores the tensor itself
    assert np.array_equal(c.levels(), ref.levels)                                 # (a)
    assert np.array_equal(c.root(), ref.levels[-1])
    _, rep = launches(hb, lambda: check_reads(hb, c, ref))                         # (b): through the rotated index
    assert "k_unrotate_msg" not in rep
    ptr, rep = launches(hb, lambda: hb.lib.hobbit_commitment_tensor_dev(c.h))     # (c)
    assert ptr and rep.get("k_unrotate_msg", 0) == 1, rep
    ptr2, rep = launches(hb, lambda: hb.lib.hobbit_commitment_tensor_dev(c.h))
    assert ptr2 == ptr and "k_unrotate_msg" not in rep and "k_zero_rows" not in rep
    for i in range(K):
        off = 16 * 4 * ref.M * i
        got = hb.to_host(ptr, (4 * ref.M, 2), np.uint64, offset=off)
        assert np.array_equal(got, hb.to_host(ref.tensor, (4 * ref.M, 2), np.uint64, offset=off)), i
        del got
    assert np.array_equal(c.levels(), ref.levels)
    check_reads(hb, c, ref)
    c.free()                                                                      # parks the (now linear) buffers
    other = Unrotated(hb, K, 900 + K)                                             # (d)
    assert not np.array_equal(other.levels[:64], ref.levels[:64])
    c2 = hb.commit_standard((other.poly, N), K, TRS, 1)
    assert np.array_equal(c2.levels(), other.levels)
    check_reads(hb, c2, other)
    c2.free(); other.free()
    c3 = hb.commit_standard((ref.poly, N), K, TRS, 1)
    assert np.array_equal(c3.levels(), ref.levels)
    check_reads(hb, c3, ref)
    c3.free(); ref.free()


def test_opening_of_a_rotated_commitment_verifies_and_equals_the_unrotated_one(hb):
    from test_open_verifier import device_aggregate, device_evaluators, verify_everything
    K, N, M = 2, 2 << 23, 1 << 23
    d = hb.fill_splitmix(N, 4242)
    x = splitmix_field(24, 7)
    c = hb.commit_standard((d, N), K, TRS, 1)
    libc.srandom(31); o, rep = launches(hb, lambda: hb.open_standard((d, N), c, x, 5900))
    assert "k_unrotate_msg" not in rep                                            # the opening read the rotated tensor
    assert o["checks"].tolist() == [1, 1, 1]
    assert (o["rows"] < TRS).sum() > 1000 and (o["rows"] >= TRS).sum() > 1000    # queries in the rotated half and in the parity half
    c.free()
    c = hb.commit_standard((d, N), K, TRS, 1)
    assert hb.lib.hobbit_commitment_tensor_dev(c.h)                               # un-rotated before the open
    libc.srandom(31); o2 = hb.open_standard((d, N), c, x, 5900)
    c.free()
    assert set(o) == set(o2)
    for k in o:
        if isinstance(o[k], dict):
            assert set(o[k]) == set(o2[k])
            for kk in o[k]:
                assert np.array_equal(o[k][kk], o2[k][kk]), (k, kk)
        else:
            assert np.array_equal(o[k], o2[k]), k
    d_aggr, _ = device_aggregate(hb, d, N, K, x)
    evalC, evalA, d_T = device_evaluators(hb, d_aggr, M, TRS)
    verify_everything(o, x, K, TRS, evalC, evalA)
    for b in (d, d_aggr, d_T):
        b.free()


def test_trs_1024_keeps_the_linear_layout(hb):
    """2^26, K = 32, trs = 1024 on test_PC's own inputs: the two-stream FFT + transpose path, no rotation to undo, the real reference's tree"""
    g = np.load(os.path.join(GOLD, "bigroot_2e26.npz"), allow_pickle=False)
    N, K, trs = 1 << 26, 32, 1024
    M = N // K
    hb.rng_reset()
    poly = hb.generate_randomness(N)
    hb.expander_init_store(trs)
    d = hb.to_device(poly); del poly
    try:
        c, rep = launches(hb, lambda: hb.commit_standard((d, N), K, trs, 1))
        assert rep.get("k_transpose", 0) >= 1, rep
        assert np.array_equal(c.root(), g["root"])
        lv = c.levels()
        off, sz, dgs = 0, M, []
        while sz >= 1:
            dgs.append(np.frombuffer(hashlib.sha256(lv[off:off + sz].tobytes()).digest(), np.uint8)); off += sz; sz //= 2
        assert np.array_equal(np.stack(dgs), g["level_dg"])
        ptr, rep = launches(hb, lambda: hb.lib.hobbit_commitment_tensor_dev(c.h))
        assert ptr and "k_unrotate_msg" not in rep
        c.free(); d.free()
    finally:
        hb.rng_reset(); hb.code_len = hb.expander_init_store(TRS)      # the module's graphs again, whatever order the tests run in
