"""The 2-product sumcheck whose first table is a sum of eq tables given by its points (hobbit_sumcheck2_eq: the opening's P4).

The table sum_j a_j eq(r_j) is never built at the sizes that take two rounds per round trip: k_sc2_eq_double sums the dense table's quads
against two cache-sized factor tables per point, and the host rebuilds the round polynomials from four sums per point.  The reference
is the oracle's dense sumcheck2 on the table built on the CPU (precompute_beta and the oracle's field operations), bit for bit; once
per size the device's own dense path on the device's table is compared too.  Sizes are the smallest at which each path can go wrong:
host only, round by round, exactly one two-round trip and the bridge, the first folding launch, odd and even numbers of trips (the
bridge's buffers) and odd and even k (the split bit)."""
import ctypes
import numpy as np
import pytest
from adversarial import families, scatter_dense, with_kernels, graphs_from, P
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
PREV_R = np.array([312, 0], np.uint64)          # P4's transcript seed (src/PC_utils.cpp:362)
SC_KEYS = ("poly", "r", "vr", "fin")
SIZES = [2, 16, 1024, 1 << 11, 1 << 13, 1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 19, 1 << 20]
FULL_A = np.array([0x123456789ABCDEF % P, 0x0FEDCBA987654321 % P], np.uint64)
SCALARS = {"zero": [0, 0], "one": [1, 0], "minus_one": [P - 1, 0], "full": FULL_A}


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    mod = load_package()
    h = mod.Hobbit(0)          # raises if the HIP library or the GPU is missing: no fallback
    yield h
    h.close()


def same(got, want, what):
    for k in SC_KEYS:
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)


def eq_sum(oracle, points, scalars):
    """sum_j scalars[j] * precompute_beta(points[j]) with the oracle's field operations"""
    t = None
    for r, a in zip(points, scalars):
        b = oracle.precompute_beta(r)
        term = oracle.f_mul(np.tile(np.asarray(a, np.uint64), (b.shape[0], 1)), b)
        t = term if t is None else oracle.f_add(t, term)
    return t


def point_families(k, seed):
    """{name: (k, 2) uint64} (the second point of a pair is drawn with seed + 1)"""
    sp = np.array([0, 1, P - 1, (P + 1) // 2], np.uint64)
    pick = splitmix_field(k, 40 + seed)[:, 0] % np.uint64(4)
    special = np.stack([sp[pick], np.zeros(k, np.uint64)], 1)
    mixed = splitmix_field(k, 50 + seed)
    mixed[::3] = special[::3]
    return {"full": splitmix_field(k, 30 + seed), "all_zero": np.zeros((k, 2), np.uint64), "all_one": np.tile(np.array([[1, 0]], np.uint64), (k, 1)),
            "special": special, "mixed_in": mixed}


def eq_vs_oracle(hb, oracle, points, scalars, v2, what, profiled=False):
    want = oracle.sumcheck2(eq_sum(oracle, points, scalars), v2, PREV_R)
    run = lambda: hb.generate_2product_sumcheck_proof_eq(points, scalars, v2, PREV_R)
    got, names = with_kernels(hb, run) if profiled else (run(), None)
    same(got, want, what)
    return names, want


# ---- a. every size class ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_sumcheck2_eq_every_size(hb, oracle, n):
    """one and two points with full-range coordinates and scalars against the oracle; the device's dense path on the device's own table;
    and the path that ran: from 2^14 the eq kernel and not k_sc2_double, below it neither"""
    k = n.bit_length() - 1
    v2 = splitmix_field(n, 100 + k)
    pts = [splitmix_field(k, 10 + k), splitmix_field(k, 20 + k)]
    for T, sc in ((2, [SCALARS["one"], FULL_A]), (1, [FULL_A])):
        what = "n=2^%d T=%d" % (k, T)
        names, want = eq_vs_oracle(hb, oracle, pts[:T], sc, v2, what, profiled=True)
        assert "k_sc2_double" not in names, "%s: kernels %s" % (what, sorted(names))
        assert ("k_sc2_eq_double" in names) == (n >= 1 << 14), "%s: kernels %s" % (what, sorted(names))
    # (the last `want` is T = 1's) the device's dense path on a table the device built
    dev_tab = oracle.f_mul(np.tile(FULL_A, (n, 1)), hb.precompute_beta(pts[0]))
    same(hb.generate_2product_sumcheck_proof(dev_tab, v2, PREV_R), want, "n=2^%d dense on the device" % k)


# ---- b. points and scalars ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [15, 16])
def test_sumcheck2_eq_points_and_scalars(hb, oracle, k):
    """every point family with every scalar, T = 1 and T = 2 (the second point full-range, the same family, or the first point again):
    all-zero and all-one points leave one non-zero entry, at index 0 and at n - 1"""
    n = 1 << k
    v2 = splitmix_field(n, 200 + k)
    fam, fam2 = point_families(k, k), point_families(k, k + 1)
    for name, r in fam.items():
        if name in ("all_zero", "all_one"):
            t = oracle.precompute_beta(r)
            assert t.any(axis=1).sum() == 1 and t[0 if name == "all_zero" else n - 1].tolist() == [1, 0]
        for aname, a in SCALARS.items():
            what = "k=%d point %s a=%s" % (k, name, aname)
            eq_vs_oracle(hb, oracle, [r], [a], v2, what + " T=1")
            eq_vs_oracle(hb, oracle, [fam["full"], r], [SCALARS["one"], a], v2, what + " T=2 beside a full-range point")
        eq_vs_oracle(hb, oracle, [r, fam2[name]], [FULL_A, SCALARS["minus_one"]], v2, "k=%d both points %s" % (k, name))
        eq_vs_oracle(hb, oracle, [r, r], [SCALARS["one"], FULL_A], v2, "k=%d the two points equal, %s" % (k, name))


# ---- c. the dense table's families -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [14, 17])
def test_sumcheck2_eq_dense_families(hb, oracle, k):
    n = 1 << k
    fam = families(n, seed=k)
    pts = [splitmix_field(k, 300 + k), point_families(k, 7)["mixed_in"]]
    for f in ("all_pm1", "zeros", "bits"):
        eq_vs_oracle(hb, oracle, pts, [SCALARS["one"], FULL_A], fam[f], "k=%d v2=%s T=2" % (k, f))
        eq_vs_oracle(hb, oracle, pts[1:], [SCALARS["minus_one"]], fam[f], "k=%d v2=%s T=1" % (k, f))


# ---- d. what the launcher refuses ------------------------------------------------------------------------------------------------------
def test_sumcheck2_eq_bad_arguments(hb, oracle):
    """refused before anything is launched: n no power of two or below 2, T outside {1, 2}, null points or scalars"""
    lib, ctx = hb.lib, hb.ctx
    d = hb.to_device(splitmix_field(1 << 12, 1))
    pts = splitmix_field(12, 2); sc = splitmix_field(2, 3)
    out = [np.zeros((64, 3, 2), np.uint64), np.zeros((64, 2), np.uint64), np.zeros((2, 2), np.uint64), np.zeros(2, np.uint64)]
    o = [a.ctypes.data_as(ctypes.c_void_p) for a in out]
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pr = p(PREV_R)
    hb.profile(True); hb.profile_reset()
    try:
        for T, r1, r2, a, n, word in ((2, p(pts), p(pts), p(sc), 1000, b"power of two"), (2, p(pts), p(pts), p(sc), 1, b"power of two"),
                                      (2, p(pts), p(pts), p(sc), 0, b"power of two"), (1, p(pts), None, p(sc), 4095, b"power of two"),
                                      (0, p(pts), p(pts), p(sc), 4096, b"one or two"), (3, p(pts), p(pts), p(sc), 4096, b"one or two"),
                                      (-1, p(pts), p(pts), p(sc), 4096, b"one or two"), (1, None, p(pts), p(sc), 4096, b"null"),
                                      (2, p(pts), None, p(sc), 4096, b"null"), (2, None, None, p(sc), 4096, b"null"), (2, p(pts), p(pts), None, 4096, b"null")):
            assert lib.hobbit_sumcheck2_eq(ctx, T, r1, r2, a, d.ptr, n, pr, *o) < 0, (T, n)
            assert word in lib.hobbit_last_error(ctx), (T, n, lib.hobbit_last_error(ctx))
        assert not hb.profile_report(), "a refused call launched %s" % sorted(hb.profile_report())
    finally:
        hb.profile(False); hb.profile_reset()
    assert all(not a.any() for a in out)
    # the context is still usable afterwards, and T = 1 ignores a null second point
    got = hb.generate_2product_sumcheck_proof_eq([pts], [sc[0]], splitmix_field(1 << 12, 1), PREV_R)
    same(got, oracle.sumcheck2(eq_sum(oracle, [pts], [sc[0]]), splitmix_field(1 << 12, 1), PREV_R), "after the refusals")


# ---- e. the sparse round's list handling: lengths around the workgroup size ------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 255, 256, 257, 1023, 1024, 1025, 4099])
def test_sumcheck2_sparse_lengths_around_the_block(hb, oracle, m):
    """uniform lists of exactly m entries at n = 2^18 (the smallest sparse size): a partly filled wave, whole workgroups, one entry over"""
    n = 1 << 18
    rng = np.random.default_rng(8000 + m)
    idx = np.sort(rng.choice(n, m, replace=False)).astype(np.uint64)
    v1, val = splitmix_field(n, 810), splitmix_field(m, 811 + m)
    want = oracle.sumcheck2(v1, scatter_dense(n, idx, val), np.array([121, 0], np.uint64))
    same(hb.generate_2product_sumcheck_proof_sparse(v1, idx, val, np.array([121, 0], np.uint64)), want, "m=%d" % m)


# ---- f. the opening takes both forms -----------------------------------------------------------------------------------------------------
def test_open_uses_sparse_p3_and_eq_p4(hb, oracle):
    """the smallest opening whose big table (2 trs * 4096 = 2^18) takes the sparse P3 and the eq P4: the kernels that ran.  (The
    transcript is compared with the oracle's by the open tests.)"""
    N, K = 1 << 18, 4
    trs = N // (K << 11)
    libc = ctypes.CDLL(None)
    oracle.rng_reset(); poly = oracle.generate_randomness(N); oracle.expander_init_store(trs)
    x = oracle.generate_randomness(N.bit_length() - 1)
    hb.upload_graphs(trs, graphs_from(oracle, trs))
    c = hb.commit_standard(poly, K, trs, 1)
    libc.srandom(777)
    got, names = with_kernels(hb, lambda: hb.open_standard(poly, c, x, 1000, want_paths=False))
    c.free()
    assert got["checks"].tolist() == [1, 1, 1]
    assert "k_eq_final_axpy" not in names and "k_sc2_eq_double" in names and "k_sc2_sparse_round" in names, sorted(names)
