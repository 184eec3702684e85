"""Base-field polynomials under RS x RS (include/hobbit_real_rs.h): the real row code up to 2^20 points, the half commitment, its readers, the
opening and the driver against the calls of hobbit_hip.h on the same polynomial widened to (x, 0).  All arithmetic is exact and canonical, so every
comparison is byte for byte.

Shapes (N, K, trs): (48, 3, 4) two leaf groups, the wrap to row 0, the shortest row code, odd K; (2^10, 4, 8); (2^17, 4, 16) k_fft_real4096 on a
small tensor; (2^23, 2, 2048) the 4096-point column transform; (2^18, 32, 128) and (2^20, 16, 128) test_PC option 1's own row size; (2^22, 4, 128)
the 2^13 .. 2^15 class; (2^23, 2, 128) chunk at a time; (2^24, 2, 128) the first length beyond hobbit_fft_real_rows_any.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
libc = ctypes.CDLL(None)
c_vp, c_sz = ctypes.c_void_p, ctypes.c_size_t
P = (1 << 61) - 1
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


def live(hb):
    a, b = c_sz(), c_sz()
    hb.lib.hobbit_mem_live(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


# ---- the row code -------------------------------------------------------------------------------------
def row_inputs(kind, rows, h):
    if kind == "uniform":
        return reals(rows * h, 11 + h % 1000).reshape(rows, h)
    if kind == "all p-1":
        return np.full((rows, h), P - 1, np.uint64)
    x = np.zeros((rows, h), np.uint64)                         # unit vectors at positions 0, 1, L/2 - 1
    for r in range(rows):
        x[r, (0, 1, h - 1)[r % 3]] = 1
    return x


KINDS = ["uniform", "all p-1", "unit vectors"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("logL", [3, 12, 16])
def test_row_code_equals_fft_real_rows_any_where_both_apply(hb, logL, kind):
    x = row_inputs(kind, 3, 1 << (logL - 1))
    assert np.array_equal(hb.fft_real_rows_len(x, logL), hb.fft_real_rows_any(x, logL))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("logL", [17, 18, 20])
def test_row_code_beyond_2e16_is_the_transform_of_the_widened_row(hb, logL, kind):
    L = 1 << logL; h = L // 2
    x = row_inputs(kind, 3, h)
    padded = np.zeros((3, L, 2), np.uint64); padded[:, :h, 0] = x
    want = hb.fft(padded)[:, :h + 1]
    got = hb.fft_real_rows_len(x, logL)
    assert np.array_equal(got, want)
    if kind == "unit vectors":
        assert (got[0] == np.array([1, 0], np.uint64)).all()   # delta at 0: the all-ones row


def test_row_code_range(hb, mod):
    for logL in (2, 21):
        with pytest.raises(mod.HobbitError, match=EINVAL + ".*\\[3,20\\]"):
            hb.fft_real_rows_len(np.zeros((1, 1 << (logL - 1)), np.uint64), logL)


# ---- the half commitment ------------------------------------------------------------------------------
class Pair:
    """the half commitment of a real polynomial and the full RS x RS commitment of the same polynomial widened"""

    def __init__(self, hb, N, K, trs, seed=None):
        self.hb, self.N, self.K, self.trs = hb, N, K, trs
        self.M = N // K; self.cols = 2 * self.M // trs; self.rows2 = 2 * trs
        x = reals(N, seed or (2000 + N % 9973))
        self.d_real = hb.to_device(x); del x
        self.d_wide = hb.alloc(16 * N)
        hb._chk(hb.lib.hobbit_widen_real(hb.ctx, c_vp(self.d_real.ptr), c_vp(self.d_wide.ptr), c_sz(N)))
        self.full = hb.commit_standard((self.d_wide, N), K, trs, 0)
        self.half = hb.commit_standard_real_rs((self.d_real, N), K, trs)

    def free(self):
        for c in (self.full, self.half):
            c.free()
        for b in (self.d_real, self.d_wide):
            b.free()


SHAPES = [(48, 3, 4), (1 << 10, 4, 8), (1 << 17, 4, 16), (1 << 23, 2, 2048), (1 << 18, 32, 128), (1 << 20, 16, 128), (1 << 22, 4, 128),
          (1 << 23, 2, 128), (1 << 24, 2, 128)]
ORACLE_SHAPES = [(48, 3, 4), (1 << 10, 4, 8), (1 << 18, 32, 128)]


@pytest.mark.parametrize("N,K,trs", SHAPES, ids=["N%d-K%d-trs%d" % s for s in SHAPES])
def test_half_commitment_equals_the_commitment_of_the_widened_polynomial(hb, oracle, N, K, trs):
    p = Pair(hb, N, K, trs)
    try:
        cols, rows2 = p.cols, p.rows2
        hc = cols // 2
        assert p.half.is_half() and not p.full.is_half()
        assert np.array_equal(p.half.root(), p.full.root())
        lv = p.half.levels()
        assert np.array_equal(lv, p.full.levels())
        for chunk in (0, K - 1):
            for row in sorted({0, 1, 3, 4, trs - 1, trs, rows2 - 4, rows2 - 1}):
                assert np.array_equal(p.half.tensor_row(chunk, row), p.full.tensor_row(chunk, row)), (chunk, row)
        rng = np.random.default_rng(N % 1000 + K)
        qr = rng.integers(0, rows2, 512, dtype=np.uint32); qc = rng.integers(0, cols, 512, dtype=np.uint32)
        edge = np.array([0, 1, hc - 1, hc, hc + 1, cols - 1], np.uint32)
        groups = np.arange(0, rows2, 4, dtype=np.uint32)       # every row group, at every edge column
        qr = np.concatenate([qr, np.repeat(groups, len(edge))]); qc = np.concatenate([qc, np.tile(edge, len(groups))])
        assert np.array_equal(p.half.gather(qr, qc), p.full.gather(qr, qc))
        assert np.array_equal(p.half.paths(qc, qr), p.full.paths(qc, qr))
        if (N, K, trs) in ORACLE_SHAPES:                       # ... and the oracle, so that a shared mistake of the two device forms cannot hide
            poly = widen(hb.to_host(p.d_real, (N,), np.uint64))
            want, _ = oracle.commit_standard(poly, K, trs, 0)
            assert np.array_equal(lv, want)
    finally:
        p.free()


def test_half_tensor_is_exactly_half_plus_one_column_per_chunk(mod):
    """a context of its own: nothing parked, so the second commit of a kind allocates exactly its tensor and its levels"""
    hb = mod.Hobbit(0)
    try:
        N, K, trs = 1 << 18, 32, 128
        M = N // K; cols = 2 * M // trs; rows2 = 2 * trs; hc = cols // 2
        x = reals(N, 3)
        d_real = hb.to_device(x); d_wide = hb.to_device(widen(x))
        held = [hb.commit_standard((d_wide, N), K, trs, 0), hb.commit_standard_real_rs((d_real, N), K, trs)]       # tables and workspaces of both paths exist now
        b0 = live(hb)[1]; held.append(hb.commit_standard((d_wide, N), K, trs, 0))
        b1 = live(hb)[1]; held.append(hb.commit_standard_real_rs((d_real, N), K, trs))
        b2 = live(hb)[1]
        full_t, half_t = b1 - b0 - 64 * M, b2 - b1 - 64 * M
        print("tensor bytes: full %d, half %d" % (full_t, half_t))
        assert full_t == K * cols * rows2 * 16
        assert half_t == (K * hc + K) * rows2 * 16
        for c in held:
            c.free()
    finally:
        hb.close()


def test_raw_pointer_of_a_half_commitment_is_the_full_tensor(hb):
    p = Pair(hb, 1 << 18, 32, 128)
    try:
        n_el = p.K * p.cols * p.rows2
        ptr = p.half.tensor_dev()
        assert ptr and ptr == p.half.tensor_dev()              # materialised once
        want = hb.to_host(p.full.tensor_dev(), (n_el, 2), np.uint64)
        assert np.array_equal(hb.to_host(ptr, (n_el, 2), np.uint64), want)
        assert np.array_equal(p.half.levels(), p.full.levels())          # the half form still answers
        assert np.array_equal(p.half.tensor_row(1, p.trs + 1), p.full.tensor_row(1, p.trs + 1))
    finally:
        p.free()


def test_commit_from_host_memory(hb):
    N, K, trs = 1 << 23, 2, 128                                # a tensor over 64 MiB: the upload runs group by group
    x = reals(N, 8)
    c, d = hb.commit_standard_real_rs_host(x, K, trs)
    want = hb.commit_standard_real_rs(x, K, trs)
    assert c.is_half() and np.array_equal(c.levels(), want.levels())
    assert np.array_equal(hb.to_host(d, (N,), np.uint64), x)
    for o in (c, want, d):
        o.free()


# ---- the opening --------------------------------------------------------------------------------------
def same(a, b, where=""):
    assert set(a) == set(b), where
    for k in a:
        if isinstance(a[k], dict):
            same(a[k], b[k], where + k + "/")
        elif a[k] is None or b[k] is None:
            assert a[k] is None and b[k] is None, where + k
        else:
            assert np.array_equal(a[k], b[k]), where + k


@pytest.mark.parametrize("N,K,trs", [(1 << 18, 32, 128), (1 << 23, 2, 128)], ids=["2e18-K32", "2e23-K2"])
def test_opening_from_a_real_polynomial_is_the_opening_of_the_widened_one(hb, oracle, N, K, trs):
    p = Pair(hb, N, K, trs)
    try:
        x = splitmix_field(N.bit_length() - 1, 7)
        libc.srandom(700 + K)
        w0 = hb.libc_window()
        o_full = hb.open_standard_rs((p.d_wide, N), p.full, x, 790)
        w1 = hb.libc_window()
        hb.libc_set_window(w0)
        o_half = hb.open_standard_rs_real((p.d_real, N), p.half, x, 790)
        assert np.array_equal(hb.libc_window(), w1)            # the same draws
        assert o_half["checks"].tolist() == [1, 1]
        qc = o_half["cols"]
        assert (qc > p.cols // 2).sum() >= 100 and (qc < p.cols // 2).sum() >= 100     # (790 uniform draws: 395 expected on each side)
        same(o_half, o_full)
        hb.libc_set_window(w0)
        o_mixed = hb.open_standard_rs_real((p.d_real, N), p.full, x, 790)             # the FULL commitment opened from the real polynomial
        assert np.array_equal(hb.libc_window(), w1)
        same(o_mixed, o_full)
        if K == 32:                                            # ... and the oracle's opening, from its own commitment
            poly = widen(hb.to_host(p.d_real, (N,), np.uint64))
            lv, T = oracle.commit_standard(poly, K, trs, 0, want_tensor=True)
            hb.libc_set_window(w0)
            want = oracle.open_standard_rs(poly, K, trs, x, 790, lv, T)
            assert want["checks"].tolist() == [1, 1]
            assert int(o_half["ncols"][0]) == int(want["ncols"][0]) and int(o_half["reply_len"][0]) == K
            for k in ("I", "rv0", "cf_root", "reply", "paths", "poly", "r", "vr", "fin", "rx"):
                assert np.array_equal(o_half[k], want[k]), k
            for k in want["sp_f"]:
                assert np.array_equal(o_half["sp_f"][k], want["sp_f"][k]), "sp_f/" + k
    finally:
        p.free()


# ---- refusals -----------------------------------------------------------------------------------------
def test_refusals_allocate_and_launch_nothing(hb, mod):
    d = hb.alloc(8 * (1 << 22) + 16)
    hb.sync()
    before = live(hb)
    bad = [((1 << 16), 4, 4096, 0, "4096"),                    # 2 trs > 4096
           (32, 4, 4, 0, "2\\^3"),                             # cols = 4
           (1 << 22, 1, 4, 0, "2\\^20"),                       # cols = 2^21
           (96, 2, 4, 0, "power of two"),                      # N / K = 48
           (1 << 10, 4, 8, 8, "aligned")]                      # a pointer offset by 8 bytes
    for N, K, trs, off, why in bad:
        with pytest.raises(mod.HobbitError, match=EINVAL + ".*" + why):
            hb.commit_standard_real_rs((d.ptr + off, N), K, trs)
        assert live(hb) == before, (N, K, trs)
    d.free()


def test_opening_refuses_an_rs_x_expander_commitment(hb, mod):
    N, K, trs = 1 << 17, 4, 16
    hb.rng_reset(); hb.graph_draw(trs)
    x = reals(N, 4)
    d = hb.to_device(x)
    c = hb.commit_standard_real((d, N), K, trs, 1)
    with pytest.raises(mod.HobbitError, match=EINVAL + ".*RS x expander"):
        hb.open_standard_rs_real((d, N), c, splitmix_field(17, 1), 790)
    c.free(); d.free()


# ---- the driver ---------------------------------------------------------------------------------------
def _test_pc(args, timeout):
    exe = os.path.join(PKG, "host", "test_pc")
    return subprocess.run(["timeout", "-k", "10", str(timeout), exe] + [str(a) for a in args], capture_output=True, text=True, cwd=ROOT)


def test_driver_prints_the_same_root_and_proof_size():
    """host/test_pc real_rs 20 32 and host/test_pc 20 1 32, each a fresh child process: the same root, the same Ps"""
    def root_and_ps(p):
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        lines = p.stdout.splitlines()
        root = [l for l in lines if l.startswith("root ")]
        assert len(root) == 1 and ">>OK" in lines
        return root[0], lines[-1].split(",")[0]
    a = root_and_ps(_test_pc(("real_rs", 20, 32), 120))
    b = root_and_ps(_test_pc((20, 1, 32), 120))
    assert a == b
