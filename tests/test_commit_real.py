"""Base-field polynomials (include/hobbit_real.h): the row kernel, the half commitment, the aggregate, the opening and the driver against the
calls of hobbit_hip.h on the same polynomial widened to (x, 0).  All arithmetic is exact and canonical, so every comparison is byte for byte.

Shapes (N, K): (2^16, 4) trs 8, the identity code; (2^17, 4) trs 16, also against the oracle's root; (2^19, 4) trs 64; (2^23, 4) trs 1024, the
row-major scratch and the tiled transposes; (2^24, 2) trs 4096, the fat encode kernels and the rotated layout; (2^25, 2) trs 8192, the tiled steps.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import brakingbase_model as bm
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
libc = ctypes.CDLL(None)
c_vp, c_sz = ctypes.c_void_p, ctypes.c_size_t
P = (1 << 61) - 1
COLS = 4096
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")
EINVAL = "rc=-2"


@pytest.fixture(scope="module")
def mod():
    from __graft_entry__ import load_package
    return load_package()


@pytest.fixture(scope="module")
def hb(mod):
    h = mod.Hobbit(0)
    yield h
    h.close()


def widen(x):
    out = np.zeros(x.shape + (2,), np.uint64)
    out[..., 0] = x
    return out


def reals(n, seed):
    return np.random.default_rng(seed).integers(0, P, n, dtype=np.uint64)


def draw_graphs(hb, trs):
    hb.rng_reset()
    return hb.graph_draw(trs)


# ---- the row kernel ---------------------------------------------------------------------------------
def row_inputs(kind, rows):
    if kind == "uniform":
        return reals(rows * 2048, 11 + rows).reshape(rows, 2048)
    if kind == "all p-1":
        return np.full((rows, 2048), P - 1, np.uint64)
    if kind == "below 2^33":
        return np.random.default_rng(33 + rows).integers(0, 1 << 33, (rows, 2048), dtype=np.uint64)
    x = np.zeros((rows, 2048), np.uint64)                      # unit vectors at positions 0, 1, 2047
    for r in range(rows):
        x[r, (0, 1, 2047)[r % 3]] = 1
    return x


@pytest.mark.parametrize("rows", [3, 64])
@pytest.mark.parametrize("kind", ["uniform", "all p-1", "unit vectors", "below 2^33"])
def test_row_kernel_is_the_4096_point_transform_of_the_widened_row(hb, kind, rows):
    x = row_inputs(kind, rows)
    padded = np.zeros((rows, 4096, 2), np.uint64); padded[:, :2048, 0] = x
    want = hb.fft(padded)[:, :2049]
    got = hb.fft_real_rows(x)
    assert np.array_equal(got, want)
    if kind == "unit vectors":
        assert (got[0] == np.array([1, 0], np.uint64)).all()   # delta at 0: the all-ones row


def test_widen_real(hb):
    x = np.concatenate([reals(1000, 5), np.array([0, 1, P - 1], np.uint64)])
    assert np.array_equal(hb.widen_real(x), widen(x))


# ---- the half commitment ----------------------------------------------------------------------------
class Pair:
    """the half commitment of a real polynomial and the full commitment of the same polynomial widened, on graphs drawn for the shape"""

    def __init__(self, hb, logN, K, seed=None):
        self.hb, self.N, self.K = hb, 1 << logN, K
        self.M = self.N // K; self.trs = self.M // 2048
        self.code_len = draw_graphs(hb, self.trs)
        x = reals(self.N, seed or (1000 + logN))
        self.d_real = hb.to_device(x); del x
        self.d_wide = hb.alloc(16 * self.N)
        hb._chk(hb.lib.hobbit_widen_real(hb.ctx, c_vp(self.d_real.ptr), c_vp(self.d_wide.ptr), c_sz(self.N)))
        self.full = hb.commit_standard((self.d_wide, self.N), K, self.trs, 1)
        self.half = hb.commit_standard_real((self.d_real, self.N), K, self.trs, 1)

    def free(self):
        for c in (self.full, self.half):
            c.free()
        for b in (self.d_real, self.d_wide):
            b.free()


SHAPES = [(16, 4), (17, 4), (19, 4), (23, 4), (24, 2), (25, 2)]


@pytest.mark.parametrize("logN,K", SHAPES, ids=["2e%d-K%d" % s for s in SHAPES])
def test_half_commitment_equals_the_commitment_of_the_widened_polynomial(hb, oracle, logN, K):
    p = Pair(hb, logN, K)
    try:
        trs, M = p.trs, p.M
        assert p.half.is_half() and not p.full.is_half()
        assert np.array_equal(p.half.root(), p.full.root())
        assert np.array_equal(p.half.levels(), p.full.levels())
        ln = p.code_len                                        # the codeword's length (trs itself for the identity code of trs <= 13)
        assert trs <= ln < 2 * trs
        for chunk in (0, K - 1):
            for row in sorted({0, 1, trs - 1, trs, ln - 1, ln, 2 * trs - 1}):
                assert np.array_equal(p.half.tensor_row(chunk, row), p.full.tensor_row(chunk, row)), (chunk, row)
        rng = np.random.default_rng(logN)
        qr = rng.integers(0, 2 * trs, 512, dtype=np.uint32); qc = rng.integers(0, COLS, 512, dtype=np.uint32)
        edge = np.array([0, 1, COLS // 2 - 1, COLS // 2, COLS // 2 + 1, COLS - 1], np.uint32)
        groups = np.arange(0, 2 * trs, 4, dtype=np.uint32)     # every row group, at every edge column
        qr = np.concatenate([qr, np.repeat(groups, len(edge))]); qc = np.concatenate([qc, np.tile(edge, len(groups))])
        assert np.array_equal(p.half.gather(qr, qc), p.full.gather(qr, qc))
        assert np.array_equal(p.half.paths(qc, qr), p.full.paths(qc, qr))
        if (logN, K) == (17, 4):                               # ... and the oracle's root, on the oracle's graphs
            oracle.rng_reset(); oracle.expander_init_store(trs)
            hb.upload_graphs(trs, bm.graphs(oracle, trs))
            poly = widen(hb.to_host(p.d_real, (p.N,), np.uint64))
            want, _ = oracle.commit_standard(poly, K, trs, 1)
            c = hb.commit_standard_real((p.d_real, p.N), K, trs, 1)
            assert np.array_equal(c.levels(), want)
            c.free()
    finally:
        p.free()


def test_half_tensor_takes_at_most_half_plus_one_column(mod):
    """a context of its own: nothing parked, so the second commit of a kind allocates exactly its tensor and its levels"""
    hb = mod.Hobbit(0)
    try:
        N, K, trs = 1 << 17, 4, 16
        M = N // K
        draw_graphs(hb, trs)
        x = reals(N, 3)
        d_real = hb.to_device(x); d_wide = hb.to_device(widen(x))

        def live():
            a, b = c_sz(), c_sz()
            hb.lib.hobbit_mem_live(ctypes.byref(a), ctypes.byref(b))
            return b.value
        held = [hb.commit_standard((d_wide, N), K, trs, 1), hb.commit_standard_real((d_real, N), K, trs, 1)]       # tables and plans of both paths exist now
        b0 = live(); held.append(hb.commit_standard((d_wide, N), K, trs, 1))
        b1 = live(); held.append(hb.commit_standard_real((d_real, N), K, trs, 1))
        b2 = live()
        full_t, half_t = b1 - b0 - 64 * M, b2 - b1 - 64 * M
        print("tensor bytes: full %d, half %d" % (full_t, half_t))
        assert full_t == K * COLS * 2 * trs * 16
        assert 0 < half_t and half_t * COLS <= full_t * (COLS // 2 + 1)
        for c in held:
            c.free()
    finally:
        hb.close()


def test_refusals(hb, mod):
    N, K, trs = 1 << 17, 4, 16
    draw_graphs(hb, trs)
    d = hb.to_device(reals(N, 4))
    with pytest.raises(mod.HobbitError, match=EINVAL + ".*linear_time"):
        hb.commit_standard_real((d, N), K, trs, 0)
    with pytest.raises(mod.HobbitError, match=EINVAL + ".*4096"):
        hb.commit_standard_real((d, N), K, 32, 1)              # rows of 2048 points
    with pytest.raises(mod.HobbitError, match=EINVAL + ".*4096"):
        hb.commit_standard_real((d, N), 2 * K, trs, 1)         # rows of 2048 points the other way
    hb.rng_reset(); hb.expander_init_store(trs)                # the same graphs drawn on the host, to change one weight of
    w = hb._graph_levels[(0, 1)][4].copy()
    w[7, 1] = 1
    hb.rng_reset(); hb.expander_init_store(trs, weights={(0, 1): w})
    with pytest.raises(mod.HobbitError, match=EINVAL + ".*img != 0"):
        hb.commit_standard_real((d, N), K, trs, 1)
    c = hb.commit_standard((hb.to_device(widen(np.zeros(N, np.uint64))), N), K, trs, 1)       # the full form still takes such graphs
    c.free()
    draw_graphs(hb, trs)
    hb.commit_standard_real((d, N), K, trs, 1).free()          # and base-field graphs are accepted again
    d.free()


def test_raw_pointer_of_a_half_commitment_is_the_full_tensor(hb):
    p = Pair(hb, 17, 4)
    try:
        n_el = p.K * COLS * 2 * p.trs
        ptr = p.half.tensor_dev()
        assert ptr and ptr == p.half.tensor_dev()              # materialised once
        want = hb.to_host(p.full.tensor_dev(), (n_el, 2), np.uint64)
        assert np.array_equal(hb.to_host(ptr, (n_el, 2), np.uint64), want)
        assert np.array_equal(p.half.levels(), p.full.levels())          # the half form still answers
        assert np.array_equal(p.half.tensor_row(1, p.trs + 1), p.full.tensor_row(1, p.trs + 1))
    finally:
        p.free()


# ---- aggregate and opening ----------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 128])
def test_aggregate_real(hb, K):
    M = 3001                                                   # odd: more than one block, a ragged last one
    x = reals(K * M, K)
    x[:3] = (0, 1, P - 1)
    beta = splitmix_field(K, 77 + K)                           # full-range betas
    beta[0] = (P - 1, P - 1)
    assert np.array_equal(hb.aggregate_real(x, beta), hb.aggregate(widen(x), beta))


def same(a, b, where=""):
    assert set(a) == set(b), where
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k], where + k + "/")
        else:
            assert np.array_equal(a[k], b[k]), where + k


@pytest.mark.parametrize("logN,K", [(19, 4), (24, 2)], ids=["2e19-K4", "2e24-K2"])
def test_opening_of_a_half_commitment_is_the_opening_of_the_full_one(hb, logN, K):
    from test_open_verifier import device_aggregate, device_evaluators, verify_everything
    p = Pair(hb, logN, K)
    try:
        x = splitmix_field(logN, 7)
        libc.srandom(500 + logN)
        w0 = hb.libc_window()
        o_full = hb.open_standard((p.d_wide, p.N), p.full, x, 5900)
        w1 = hb.libc_window()
        hb.libc_set_window(w0)
        o_half = hb.open_standard_real((p.d_real, p.N), p.half, x, 5900)
        assert np.array_equal(hb.libc_window(), w1)            # the same draws
        assert o_half["checks"].tolist() == [1, 1, 1]
        assert (o_half["cols"] > COLS // 2).sum() > 1000 and (o_half["cols"] <= COLS // 2).sum() > 1000
        same(o_half, o_full)
        d_aggr, _ = device_aggregate(hb, p.d_wide, p.N, K, x)
        evalC, evalA, d_T = device_evaluators(hb, d_aggr, p.M, p.trs)
        verify_everything(o_half, x, K, p.trs, evalC, evalA)    # tests/open_verifier.verify_open and both shockwave proofs
        for b in (d_aggr, d_T):
            b.free()
    finally:
        p.free()


# ---- the driver ---------------------------------------------------------------------------------------
def _test_pc(args, timeout):
    exe = os.path.join(PKG, "host", "test_pc")
    return subprocess.run(["timeout", "-k", "10", str(timeout), exe] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT)


def test_driver_prints_the_same_root_and_proof_size():
    """host/test_pc real 20 32 and host/test_pc 20 4 32, each a fresh child process: the same root, the same Ps"""
    def root_and_ps(p):
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.splitlines()
        root = [l for l in lines if l.startswith("root ")]
        assert len(root) == 1 and ">>OK" in lines
        return root[0], lines[-1].split(",")[0]
    a = root_and_ps(_test_pc(("real", 20, 32), 120))
    b = root_and_ps(_test_pc((20, 4, 32), 120))
    assert a == b
    assert float(a[1]) == 3839.078125                          # the reference's stdout fingerprint of `./pigeon 20 4 32`
