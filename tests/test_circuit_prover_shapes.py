"""The circuit prover's and the code proofs' entry points at every size class: the error terms and folds of the streaming sumcheck,
batch_prod, the batched cubic sumcheck, the multiplication tree, phiGInit, prepare_matrix, the parity matrix, prove_linear_code,
prove_fft, prove_fft_matrix, _whir_prove, shockwave_prove and the Merkle paths of an opening.

Each launcher switches form somewhere -- a grid capped at 1024 workgroups, a one-workgroup head, a sumcheck that stays on the host, a
cache rebuilt when a size changes -- and until now each was run with one uniform input at a handful of powers of two.  The shapes here
are the smallest on either side of every such switch, and the inputs include what a witness looks like (bits, zeros, constants, p - 1).
References: the big-integer restatements of tests/adversarial.py up to 300 elements (tests/test_circuit_refs_cpu.py proves them against
the oracle), the oracle above that.  Exact field and byte work: every comparison is np.array_equal.

On an MI355X the file's 116 cases take 13 s; the slowest three are test_error_terms_families_and_selectors[262145] (1.9 s: thirteen
families and seventeen selector arrays against the oracle), test_whir_prove_iteration_classes[21-5] (1.8 s) and
test_fingerprint_every_size[1048579] (0.9 s)."""
import contextlib
import ctypes
import numpy as np
import pytest
from adversarial import (families, selectors, graphs_from, set_weights, to_py, from_py, py_mul, py_add, py_err2p, py_err3p, py_err4p,
                         py_batch_terms, py_axpy, py_axpy_i32, py_fingerprint, py_prepare_matrix_cols, py_phi_g, py_cubic_claim, P)
from commit_refs import paths as expected_paths      # the sibling gather lives with the other commitment references
from oracle.pyoracle import splitmix_field
from test_sumcheck_eq import point_families
from test_sumcheck_shapes import open_case

pytestmark = pytest.mark.gpu
PY_MAX = 300                                    # up to here the reference is the big-integer one
FULL = np.array([0x123456789ABCDEF % P, 0x0FEDCBA987654321 % P], np.uint64)
SCALARS = {"zero": np.array([0, 0], np.uint64), "one": np.array([1, 0], np.uint64), "minus_one": np.array([P - 1, 0], np.uint64), "full": FULL}
LR = splitmix_field(2, 449)                     # lookup_rand
SC_KEYS = ("poly", "r", "vr", "fin")
libc = ctypes.CDLL(None)


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    mod = load_package()
    h = mod.Hobbit(0)          # raises if the HIP library or the GPU is missing: no fallback
    yield h
    h.close()


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def const(a, n):
    return np.tile(np.asarray(a, np.uint64).reshape(1, 2), (n, 1))


def back(hb, buf, n):
    return hb.to_host(buf, (n, 2), np.uint64)


def same(got, want, what, keys=None):
    for k in (keys or want):
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)


def field_sum(oracle, v):
    """the field sum of the rows of v, by halving with the oracle's f_add"""
    v = np.ascontiguousarray(v, np.uint64).reshape(-1, 2)
    while v.shape[0] > 1:
        if v.shape[0] % 2:
            v = np.concatenate([v, np.zeros((1, 2), np.uint64)])
        v = oracle.f_add(v[: v.shape[0] // 2], v[v.shape[0] // 2:])
    return v[0]


@contextlib.contextmanager
def lookup_mode(hb, oracle, on):
    """has_lookups on both sides, always switched off again"""
    if on:
        hb.set_lookups(LR); oracle.set_lookups(LR)
    try:
        yield
    finally:
        hb.set_lookups(None); oracle.set_lookups(None)


# ---- a. error terms ------------------------------------------------------------------------------------------------------------------
# run_err caps the grid at 1024 workgroups of 256 threads: one thread, either side of a wave (64) and of a workgroup (256), a length in
# the middle of the grid that is no power of two, the last length served in one pass (2^18) with its neighbours, and a length well into
# the second trip of k_err_terms' grid-stride loop
ERR_SIZES = [1, 2, 63, 64, 65, 255, 257, 5000, (1 << 18) - 1, 1 << 18, (1 << 18) + 1, (1 << 19) + 77]
ERR_FAMILY_SIZES = [257, (1 << 18) + 1]
NC = {2: 2, 3: 3, 4: 4, 13: 3}


def default_gate(n, lookups):
    return ((np.arange(n) * 7 + 3) % 6 - 1).astype(np.int32) if lookups else (np.arange(n) * 7 % 5 < 2).astype(np.int32)


class ErrTables:
    """three chunk tables b, four fold tables f and beta on the host and on the device"""

    def __init__(self, hb, b, f, beta):
        self.hb, self.b, self.f, self.beta, self.n = hb, b, f, beta, b[0].shape[0]
        self.db = [hb.to_device(x) for x in b]; self.df = [hb.to_device(x) for x in f]; self.dbeta = hb.to_device(beta)

    def device(self, kind, gate, K):
        """the typed entry point of `kind`, accumulating into K"""
        hb, n, b, f = self.hb, self.n, self.db, self.df
        g = hb.to_device(np.ascontiguousarray(gate, np.int32))
        if kind == 2:
            hb._chk(hb.lib.hobbit_compute2p_error_terms(hb.ctx, b[0].ptr, b[1].ptr, f[0].ptr, f[1].ptr, n, vp(K)))
        elif kind == 3:
            hb._chk(hb.lib.hobbit_compute3p_error_terms(hb.ctx, b[0].ptr, g.ptr, f[0].ptr, f[1].ptr, f[2].ptr, self.dbeta.ptr, n, vp(K)))
        else:
            hb._chk(hb.lib.hobbit_compute4p_error_terms(hb.ctx, b[0].ptr, b[1].ptr, b[2].ptr, g.ptr, f[0].ptr, f[1].ptr, f[2].ptr, f[3].ptr, n, vp(K)))
        return K

    def stream_fold(self, kind, gate, K):
        hb, b, f = self.hb, self.db, self.df
        t = {2: [b[0], b[1], f[0], f[1]], 3: [b[0], f[0], f[1], f[2], self.dbeta], 4: [b[0], b[1], b[2], f[0], f[1], f[2], f[3]], 13: b + f[:3]}[kind]
        ptrs = (ctypes.c_void_p * 8)(*[x.ptr for x in (t + [t[-1]] * 8)[:8]])
        g = hb.to_device(np.ascontiguousarray(gate, np.int32))
        hb._chk(hb.lib.hobbit_stream_fold(hb.ctx, kind, ptrs, g.ptr, self.n, vp(K)))
        return K

    def reference(self, oracle, kind, gate, lookups):
        b, f, beta = self.b, self.f, self.beta
        if self.n <= PY_MAX:
            pb, pf, pbe = [to_py(x) for x in b], [to_py(x) for x in f], to_py(beta)
            if kind == 2:
                return from_py(py_err2p(pb[0], pb[1], pf[0], pf[1]))
            if kind == 3:
                return from_py(py_err3p(pb[0], gate, pf[0], pf[1], pf[2], pbe, to_py(LR) if lookups else None))
            if kind == 4:
                return from_py(py_err4p(pb[0], pb[1], pb[2], gate, pf[0], pf[1], pf[2], pf[3], lookups))
            return from_py(py_batch_terms(pb[0], pb[1], pb[2], pf[0], pf[1], pf[2]))
        if kind == 2:
            return oracle.err2p(b[0], b[1], f[0], f[1])
        if kind == 3:
            return oracle.err3p(b[0], gate, f[0], f[1], f[2], beta)
        if kind == 4:
            return oracle.err4p(b[0], b[1], b[2], gate, f[0], f[1], f[2], f[3])
        return oracle.batch_prod_terms(b[0], b[1], b[2], f[0], f[1], f[2])


def uniform_err_tables(hb, n, seed):
    t = [splitmix_field(n, 600 + seed + i) for i in range(8)]
    return ErrTables(hb, t[:3], t[3:7], t[7])


@pytest.mark.parametrize("n", ERR_SIZES)
def test_error_terms_every_size(hb, oracle, n):
    """the three kinds with and without lookups on uniform tables; then a second call with other tables into the same h_K, which
    must hold the field sum of the two results (the reference's F& parameters)"""
    A, B = uniform_err_tables(hb, n, 0), uniform_err_tables(hb, n, 20)
    for lookups in (False, True):
        ga, gb = default_gate(n, lookups), default_gate(n, lookups)[::-1].copy()
        with lookup_mode(hb, oracle, lookups):
            for kind in (2, 3, 4):
                what = "n=%d kind %d lookups=%d" % (n, kind, lookups)
                K = np.zeros((NC[kind], 2), np.uint64)
                wa = A.reference(oracle, kind, ga, lookups)
                assert np.array_equal(A.device(kind, ga, K), wa), what
                wb = B.reference(oracle, kind, gb, lookups)
                assert np.array_equal(B.device(kind, gb, K), oracle.f_add(wa, wb)), what + ": second call into the same h_K"


@pytest.mark.parametrize("n", ERR_FAMILY_SIZES)
def test_error_terms_families_and_selectors(hb, oracle, n):
    """every input family in the fold tables (chunks uniform; the lookup maps only change the gate, so once, without them), and every
    selector family on uniform tables in both gate modes"""
    u = uniform_err_tables(hb, n, 40)
    fams = [families(n, seed=j) for j in range(5)]
    g = default_gate(n, False)
    for name in fams[0]:
        T = ErrTables(hb, u.b, [fams[j][name] for j in range(4)], fams[4][name])
        for kind in (2, 3, 4):
            K = np.zeros((NC[kind], 2), np.uint64)
            assert np.array_equal(T.device(kind, g, K), T.reference(oracle, kind, g, False)), "n=%d folds %s kind %d" % (n, name, kind)
    for lookups in (False, True):
        with lookup_mode(hb, oracle, lookups):
            for sname, g in selectors(n, lookups).items():
                for kind in (3, 4):
                    K = np.zeros((NC[kind], 2), np.uint64)
                    assert np.array_equal(u.device(kind, g, K), u.reference(oracle, kind, g, lookups)), "n=%d selector %s kind %d lookups=%d" % (n, sname, kind, lookups)


@pytest.mark.parametrize("n", [257, (1 << 18) + 1])
def test_stream_fold_every_kind(hb, oracle, n):
    """hobbit_stream_fold, kinds 2, 3, 4 and 13, accumulating into an h_K that starts non-zero"""
    T = uniform_err_tables(hb, n, 60)
    K0 = splitmix_field(4, 61)
    for lookups in (False, True):
        g = default_gate(n, lookups)
        with lookup_mode(hb, oracle, lookups):
            for kind in (2, 3, 4, 13):
                K = K0[:NC[kind]].copy()
                want = oracle.f_add(K0[:NC[kind]], T.reference(oracle, kind, g, lookups))
                assert np.array_equal(T.stream_fold(kind, g, K), want), "n=%d stream_fold kind %d lookups=%d" % (n, kind, lookups)


# ---- b. folds and the fingerprint ----------------------------------------------------------------------------------------------------
FOLD_SIZES = [1, 63, 257, 5000, (1 << 20) + 3]           # (the grid of these kernels is capped at 4096 workgroups: 2^20 + 3 takes a second trip)


class Running:
    """a device vector and its reference, updated side by side"""

    def __init__(self, hb, oracle, y):
        self.hb, self.oracle, self.n = hb, oracle, y.shape[0]
        self.small = self.n <= PY_MAX
        self.d = hb.to_device(y); self.ref = to_py(y) if self.small else y.copy()

    def check(self, what):
        got = back(self.hb, self.d, self.n)
        assert np.array_equal(got, from_py(self.ref) if self.small else self.ref), what

    def axpy(self, a, x):
        o = self.oracle
        self.ref = py_axpy(self.ref, to_py(a)[0], to_py(x)) if self.small else o.f_add(self.ref, o.f_mul(const(a, self.n), x))

    def axpy_i32(self, a, s, one_minus):
        o, n = self.oracle, self.n
        if self.small:
            self.ref = py_axpy_i32(self.ref, to_py(a)[0], s, one_minus)
        else:
            v = np.stack([s.astype(np.uint64), np.zeros(n, np.uint64)], 1)
            if one_minus:
                v = o.f_sub(const([1, 0], n), v)
            self.ref = o.f_add(self.ref, o.f_mul(const(a, n), v))


def fold_data(n):
    fam = families(n, seed=n % 89)
    return {"uniform": splitmix_field(n, 700), "all_pm1": fam["all_pm1"], "zeros": fam["zeros"], "bits": fam["bits"]}


@pytest.mark.parametrize("n", FOLD_SIZES)
def test_fold_axpy_and_aggregate(hb, oracle, n):
    """y += a x through hobbit_fold_axpy and hobbit_axpy_aggregate (the same fold under _aggregate's argument order), every scalar
    with every family, onto a running vector"""
    run = Running(hb, oracle, splitmix_field(n, 701))
    for name, x in fold_data(n).items():
        dx = hb.to_device(x)
        for an, a in SCALARS.items():
            hb._chk(hb.lib.hobbit_fold_axpy(hb.ctx, run.d.ptr, dx.ptr, vp(a), n))
            run.axpy(a, x); run.check("n=%d fold_axpy x=%s a=%s" % (n, name, an))
            hb._chk(hb.lib.hobbit_axpy_aggregate(hb.ctx, dx.ptr, vp(a), run.d.ptr, n))
            run.axpy(a, x); run.check("n=%d axpy_aggregate x=%s a=%s" % (n, name, an))
    for name, x in fold_data(n).items():                  # a family as the accumulator: p - 1 and 0 are where the sum wraps
        run = Running(hb, oracle, x)
        u = splitmix_field(n, 702); du = hb.to_device(u)
        hb._chk(hb.lib.hobbit_fold_axpy(hb.ctx, run.d.ptr, du.ptr, vp(FULL), n))
        run.axpy(FULL, u); run.check("n=%d fold_axpy onto %s" % (n, name))
        dc = hb.to_device(back(hb, run.d, n))
        hb._chk(hb.lib.hobbit_fold_axpy(hb.ctx, run.d.ptr, dc.ptr, vp(SCALARS["minus_one"]), n))        # y += -y
        assert not back(hb, run.d, n).any(), "n=%d y - y onto %s" % (n, name)


@pytest.mark.parametrize("n", FOLD_SIZES)
def test_fold_axpy_i32(hb, oracle, n):
    """y += a sel and y += a (1 - sel), every selector family with every scalar"""
    run = Running(hb, oracle, splitmix_field(n, 703))
    for sname, s in selectors(n).items():
        ds = hb.to_device(s)
        for one_minus in (0, 1):
            for an, a in SCALARS.items():
                hb._chk(hb.lib.hobbit_fold_axpy_i32(hb.ctx, run.d.ptr, ds.ptr, vp(a), one_minus, n))
                run.axpy_i32(a, s, bool(one_minus)); run.check("n=%d fold_axpy_i32 sel=%s one_minus=%d a=%s" % (n, sname, one_minus, an))


@pytest.mark.parametrize("n", FOLD_SIZES)
def test_fingerprint_every_size(hb, oracle, n):
    """addr + 1 + a value [+ b freq]: every family as addr and value (addr = p - 1 wraps on the + 1), every scalar"""
    data = fold_data(n); names = list(data)
    freq = splitmix_field(n, 704); dfreq = hb.to_device(freq); out = hb.alloc(16 * n)
    small = n <= PY_MAX
    for i, name in enumerate(names):
        addr, value = data[name], data[names[(i + 1) % len(names)]]
        da, dv = hb.to_device(addr), hb.to_device(value)
        for an, a in SCALARS.items():
            for bn, b in ((None, None), ("full", FULL), (an, a)):
                what = "n=%d addr=%s a=%s b=%s" % (n, name, an, bn)
                hb._chk(hb.lib.hobbit_fingerprint_map(hb.ctx, da.ptr, dv.ptr, dfreq.ptr if b is not None else None, vp(a), vp(b) if b is not None else None, out.ptr, n))
                if small:
                    want = from_py(py_fingerprint(to_py(addr), to_py(value), to_py(a)[0], to_py(freq) if b is not None else None, to_py(b)[0] if b is not None else None))
                else:
                    want = oracle.f_add(oracle.f_add(addr, const([1, 0], n)), oracle.f_mul(const(a, n), value))
                    if b is not None:
                        want = oracle.f_add(want, oracle.f_mul(const(b, n), freq))
                assert np.array_equal(back(hb, out, n), want), what


def test_folds_of_nothing(hb, oracle):
    """n = 0: success, nothing launched, nothing written"""
    y = splitmix_field(64, 705); d = hb.to_device(y); s = hb.to_device(np.ones(64, np.int32))
    K = splitmix_field(4, 706); K0 = K.copy()
    ptrs = (ctypes.c_void_p * 8)(*[d.ptr] * 8)
    hb.profile(True); hb.profile_reset()
    try:
        assert hb.lib.hobbit_fold_axpy(hb.ctx, d.ptr, d.ptr, vp(FULL), 0) == 0
        assert hb.lib.hobbit_axpy_aggregate(hb.ctx, d.ptr, vp(FULL), d.ptr, 0) == 0
        assert hb.lib.hobbit_fold_axpy_i32(hb.ctx, d.ptr, s.ptr, vp(FULL), 0, 0) == 0
        assert hb.lib.hobbit_fold_axpy_i32(hb.ctx, d.ptr, s.ptr, vp(FULL), 1, 0) == 0
        assert hb.lib.hobbit_fingerprint_map(hb.ctx, d.ptr, d.ptr, d.ptr, vp(FULL), vp(FULL), d.ptr, 0) == 0
        assert hb.lib.hobbit_fingerprint_map(hb.ctx, d.ptr, d.ptr, None, vp(FULL), None, d.ptr, 0) == 0
        for kind in (2, 3, 4, 13):
            assert hb.lib.hobbit_stream_fold(hb.ctx, kind, ptrs, s.ptr, 0, vp(K)) == 0
        hb.sync()
        assert not hb.profile_report(), "a call on nothing launched %s" % sorted(hb.profile_report())
    finally:
        hb.profile(False); hb.profile_reset()
    assert np.array_equal(back(hb, d, 64), y) and np.array_equal(K, K0)
    assert np.array_equal(hb.precompute_beta(splitmix_field(6, 2)), oracle.precompute_beta(splitmix_field(6, 2)))


# ---- c. batch_prod -------------------------------------------------------------------------------------------------------------------
BP_KEYS = ("rand", "Kf", "Kp", "f1", "f2", "f3")


def batch_prod_inputs(batches, n, seed=0):
    tb = [splitmix_field(batches * n, 420 + seed + i).reshape(batches, n, 2) for i in range(6)]
    return tb, splitmix_field(batches, 430 + seed), splitmix_field(batches, 431 + seed)


@pytest.mark.parametrize("batches,n", [(1, 1), (1, 257), (3, 1024), (2, (1 << 18) + 1), (5, 4096)])
def test_batch_prod_shapes(hb, oracle, batches, n):
    """one batch of one element, an odd length, the fixture's shape, a second trip of the error kernel's loop, five batches; Kf and
    K_partial start at zero here"""
    tb, a, rb = batch_prod_inputs(batches, n)
    r_last = np.array([1, 0], np.uint64)
    Kf, Kp = np.zeros(2, np.uint64), np.zeros((batches, 2), np.uint64)
    got = hb.batch_prod(*tb, r_last, a, rb, Kf, Kp)
    same(got, oracle.batch_prod(*tb, r_last, a, rb, Kf, Kp), "batches=%d n=%d" % (batches, n), BP_KEYS)
    if n <= 1024:
        # the three sums of each batch from their formula, through the typed kernel of batch_prod (stream_fold kind 13), and K_partial from them
        for j in range(batches):
            py = py_batch_terms(*[to_py(tb[i][j]) for i in (3, 4, 5, 0, 1, 2)])
            d = [hb.to_device(tb[i][j]) for i in (3, 4, 5, 0, 1, 2)]
            ptrs = (ctypes.c_void_p * 8)(*[x.ptr for x in d + d[:2]])
            K = np.zeros((3, 2), np.uint64)
            hb._chk(hb.lib.hobbit_stream_fold(hb.ctx, 13, ptrs, None, n, vp(K)))
            assert np.array_equal(K, from_py(py)), "batches=%d n=%d: sums of batch %d" % (batches, n, j)
            assert to_py(got["Kp"][j])[0] == py_mul(to_py(rb[j])[0], py[2]), "batches=%d n=%d: K_partial[%d]" % (batches, n, j)


def test_batch_prod_accumulators_and_zero_coefficients(hb, oracle):
    tb, a, rb = batch_prod_inputs(3, 1024, seed=50)
    Kf, Kp = splitmix_field(1, 432)[0], splitmix_field(3, 433)
    r_last = splitmix_field(1, 434)[0]
    same(hb.batch_prod(*tb, r_last, a, rb, Kf, Kp), oracle.batch_prod(*tb, r_last, a, rb, Kf, Kp), "Kf and K_partial start non-zero", BP_KEYS)
    z = np.zeros((3, 2), np.uint64)
    same(hb.batch_prod(*tb, r_last, z, rb, Kf, Kp), oracle.batch_prod(*tb, r_last, z, rb, Kf, Kp), "a all zero", BP_KEYS)
    fam = families(3 * 1024, seed=3)
    for name in ("all_pm1", "zeros", "bits"):
        t2 = [fam[name].reshape(3, 1024, 2)] * 3 + tb[3:]
        same(hb.batch_prod(*t2, r_last, a, rb, Kf, Kp), oracle.batch_prod(*t2, r_last, a, rb, Kf, Kp), "fold tables " + name, BP_KEYS)


# ---- d. the batched cubic sumcheck ---------------------------------------------------------------------------------------------------
# tables that start at length 1 and 2, a batch of one, equal lengths, a table long enough that k_sc3_poly fills 1024 workgroups (so that
# k_sc_reduce<4> takes four trips) beside tables that are scalars from the start, a batch of one on the device path, the fixture's list;
# and, beyond the list of the issue, 2^20: the first length at which k_sc3_poly's own grid-stride loop takes a second trip
B3_LISTS = [[1], [1, 1], [2], [2, 1], [1, 2, 4, 1024], [4096, 4096], [1 << 19, 2, 1], [1 << 17], [256, 64, 256, 4, 1024], [1 << 20, 2]]
B3_FAMILY_LISTS = ([1, 2, 4, 1024], [1 << 19, 2, 1])


def cubic_vs_oracle(hb, oracle, t, lens, a, what):
    got = hb.batch_3product_sumcheck(t[0], t[1], t[2], lens, a)
    same(got, oracle.batch_3product_sumcheck(t[0], t[1], t[2], lens, a), what, ("poly", "r", "vr"))
    if max(lens) >= 2:
        q0 = to_py(got["poly"][0])
        claim = tuple((q0[0][c] + q0[1][c] + q0[2][c] + 2 * q0[3][c]) % P for c in range(2))       # p(0) + p(1), p = c0 x^3 + c1 x^2 + c2 x + c3
        if sum(lens) <= 2048:
            want = py_cubic_claim(to_py(t[0]), to_py(t[1]), to_py(t[2]), lens, to_py(a))
        else:
            prod = oracle.f_mul(oracle.f_mul(t[0], t[1]), t[2])
            want, o = (0, 0), 0
            for j, ln in enumerate(lens):
                want = py_add(want, py_mul(to_py(a[j])[0], to_py(field_sum(oracle, prod[o:o + ln]))[0])); o += ln
        assert claim == want, what + ": round 0's claim"


@pytest.mark.parametrize("lens", B3_LISTS, ids=lambda l: "-".join(str(x) for x in l))
def test_batch_3product_sumcheck_lists(hb, oracle, lens):
    tot = sum(lens)
    t = [splitmix_field(tot, 500 + i) for i in range(3)]
    a = splitmix_field(len(lens), 503)
    cubic_vs_oracle(hb, oracle, t, lens, a, "lens=%s uniform" % lens)
    if lens in B3_FAMILY_LISTS:
        fam = [families(tot, seed=s) for s in (1, 2, 3)]
        for name in ("mix", "zeros", "all_pm1"):
            tf = [fam[0][name], np.ascontiguousarray(fam[1][name][::-1]), np.roll(fam[2][name], tot // 3, axis=0)]
            cubic_vs_oracle(hb, oracle, tf, lens, a, "lens=%s %s" % (lens, name))
            cubic_vs_oracle(hb, oracle, [tf[0], t[1], t[2]], lens, SCALARS["minus_one"][None].repeat(len(lens), 0), "lens=%s t1=%s a=-1" % (lens, name))


# ---- e. the multiplication tree ------------------------------------------------------------------------------------------------------
MT_PR = np.array([17, 5], np.uint64)


def mul_tree_vs_oracle(hb, oracle, x, px, what):
    if px is None and x.shape[0] > 1:
        hb.rng_reset()                              # r is drawn with generate_randomness: the same libc state on both sides
    got = hb.mul_tree(x, MT_PR, px)
    if px is None and x.shape[0] > 1:
        oracle.rng_reset()
    want = oracle.mul_tree(x, MT_PR, px)
    same(got, want, what)
    return got


# a tree of one layer; one vector with a tree deep enough for the device sumcheck (layers of up to 2^14); two vectors; many more vectors
# than elements (the eval_vector of the 1024 products), with the point given and drawn; the middle
@pytest.mark.parametrize("vectors,size,given", [(1, 2, False), (1, 1 << 15, False), (2, 2, True), (2, 1 << 16, True), (1024, 4, True), (1024, 4, False),
                                                (16, 2048, True)])
def test_mul_tree_shapes(hb, oracle, vectors, size, given):
    x = splitmix_field(vectors * size, 510 + vectors).reshape(vectors, size, 2)
    px = splitmix_field(max(1, vectors.bit_length() - 1), 520) if given else None
    got = mul_tree_vs_oracle(hb, oracle, x, px, "vectors=%d size=%d uniform" % (vectors, size))
    if vectors == 1:
        prod = (1, 0)
        for v in to_py(x[0]):
            prod = py_mul(prod, v)
        assert to_py(got["out_eval"])[0] == prod, "vectors=1 size=%d: out_eval is the product of the inputs" % size


def test_mul_tree_witness_like_inputs(hb, oracle):
    """a product tree over bits is almost all zeros from the second layer on; p - 1 everywhere with one zero planted kills one product"""
    vectors, size = 16, 2048
    px = splitmix_field(4, 521)
    bits = families(vectors * size, seed=5)["bits"].reshape(vectors, size, 2)
    mul_tree_vs_oracle(hb, oracle, bits, px, "bits")
    pm1 = np.full((vectors, size, 2), P - 1, np.uint64); pm1[5, 1000] = 0
    got = mul_tree_vs_oracle(hb, oracle, pm1, px, "p - 1 with one zero")
    ones = np.ones((1, 4096, 2), np.uint64); ones[:, :, 1] = 0
    got = mul_tree_vs_oracle(hb, oracle, ones, None, "all one, one vector")
    assert got["out_eval"].tolist() == [1, 0]
    ones[0, 4095] = 0
    assert mul_tree_vs_oracle(hb, oracle, ones, None, "all one and a zero, one vector")["out_eval"].tolist() == [0, 0]


# ---- f. code proofs ------------------------------------------------------------------------------------------------------------------
# hobbit_phi_g's forward table has n - 1 doubling levels and a closing left-only one: n = 1, 2 no head; 3 the first one-workgroup head
# (2 levels); 11 a head of 10; 12 the full head of 11 levels and nothing but the closing step after it; 13 the first doubling level by
# k_phi_step; 14 two of them; 19 levels of many workgroups.  The inverse table runs every level by k_phi_step.
@pytest.mark.parametrize("n", [1, 2, 3, 4, 11, 12, 13, 14, 19])
def test_phi_g_every_head_boundary(hb, oracle, n):
    pts = {"uniform": splitmix_field(n, 320 + n)}
    if n in (3, 12, 13):
        pf = point_families(n, n)
        pts.update({k: pf[k] for k in ("all_zero", "all_one", "special")})
    w = to_py(oracle.root_of_unity(n))[0]
    for pname, rx in pts.items():
        for ifft in (False, True):
            for scale in ((1, 0), (P - 5, 12345)):
                want = from_py(py_phi_g(to_py(rx), w, scale, ifft)) if n <= 6 else oracle.phi_g_init(rx, scale, ifft)
                assert np.array_equal(hb.phiGInit(rx, scale, ifft), want), "n=%d point %s ifft=%d scale=%s" % (n, pname, ifft, scale)


# rows = 1 and 2; a column count that is no power of two; k = log2 rows and k below it (the closing copy of row 0), k = 0 among them;
# more than one workgroup per fold; a matrix wider than the grid's 2^20 threads
@pytest.mark.parametrize("rows,cols,k", [(1, 7, 0), (2, 1, 1), (8, 5, 3), (8, 5, 2), (8, 5, 0), (256, 300, 8), (256, 300, 5), (4096, 64, 12), (16, 70000, 4)])
def test_prepare_matrix_cols_shapes(hb, oracle, rows, cols, k):
    fam = families(rows * cols, seed=rows)
    r = splitmix_field(k, 331) if k else np.zeros((0, 2), np.uint64)
    for name, flat in (("uniform", splitmix_field(rows * cols, 330)), ("all_pm1", fam["all_pm1"]), ("bits", fam["bits"]), ("neg_interleave", fam["neg_interleave"])):
        M = flat.reshape(rows, cols, 2)
        if rows * cols <= PY_MAX or k == 0:
            want = from_py(py_prepare_matrix_cols(M, r)) if k else M[0]
        else:
            want = oracle.prepare_matrix(np.ascontiguousarray(M.transpose(1, 0, 2)), r)        # k folds of each column, then its entry 0
        assert np.array_equal(hb.prepare_matrix_cols(M, r), want), "rows=%d cols=%d k=%d %s" % (rows, cols, k, name)


def code_case(hb, oracle, n, weights=None):
    """graphs for message length n drawn by the oracle and uploaded; returns the codeword length and size_a = the next power of two"""
    oracle.rng_reset(); ln = oracle.expander_init_store(n)
    lv = graphs_from(oracle, n)
    if weights is not None:
        lv = set_weights(oracle, lv, weights)
    assert hb.upload_graphs(n, lv) == ln
    return ln, max(2, 1 << (ln - 1).bit_length())


def parity_and_linear_code(hb, oracle, n, weights, what):
    ln, size_a = code_case(hb, oracle, n, weights)
    k = size_a.bit_length() - 1
    # the parity matrix at size_a, at twice that and at size_a again: the CSR cache is rebuilt on the way up and on the way down
    for sa in (size_a, 2 * size_a, size_a):
        beta = oracle.precompute_beta(splitmix_field(sa.bit_length() - 1, 300 + n))
        want, l2 = oracle.evaluate_parity_matrix(beta, n)
        assert l2 == ln
        assert np.array_equal(hb.evaluate_parity_matrix(beta, n), want), "%s: parity matrix at size_a=%d" % (what, sa)
    d, l3 = oracle.encode_monolithic(splitmix_field(n, 310 + n))
    assert l3 == ln
    cw = np.zeros((size_a, 2), np.uint64); cw[:ln] = d[:ln]
    r1 = splitmix_field(k, 777 + n)
    got = hb.prove_linear_code(cw, n, r1)
    same(got, oracle.prove_linear_code(cw, n, r1), what + ": prove_linear_code", SC_KEYS)
    assert oracle.claim_of(got["poly"][0]).tolist() == [0, 0], what + ": a codeword's claim is zero"
    bad = cw.copy(); bad[0, 0] = (int(bad[0, 0]) + 1) % P
    got = hb.prove_linear_code(bad, n, r1)
    same(got, oracle.prove_linear_code(bad, n, r1), what + ": prove_linear_code of a non-codeword", SC_KEYS)
    # n <= 13 has no level: the code is the identity, the parity matrix is empty and the claim is zero whatever the vector is
    assert (oracle.claim_of(got["poly"][0]).tolist() != [0, 0]) == (n > 13), what + ": the claim of a vector with entry 0 changed"
    assert bool(hb.evaluate_parity_matrix(beta, n).any()) == (n > 13)


# no level (5, 13), the smallest lengths with one (14, 15), lengths that are no power of two, the row sizes the commit uses (4096, 16384)
@pytest.mark.parametrize("n", [5, 13, 14, 15, 100, 2427, 4096, 6000, 16384])
def test_parity_matrix_and_linear_code(hb, oracle, n):
    parity_and_linear_code(hb, oracle, n, None, "n=%d" % n)


@pytest.mark.parametrize("n", [100, 4096])
def test_parity_matrix_and_linear_code_largest_weights(hb, oracle, n):
    parity_and_linear_code(hb, oracle, n, [P - 1, P - 1], "n=%d weights p-1" % n)


def proof_families(n):
    fam = families(n, seed=n % 83)
    return {"uniform": splitmix_field(n, 340), "bits": fam["bits"], "zeros": fam["zeros"], "neg_halves": fam["neg_halves"]}


# 1, 2: the smallest tables; 1024 / 2048: the last sumcheck that stays on the host and the first that does not; 2^14: the first with two
# rounds per trip; 2^17
@pytest.mark.parametrize("s", [1, 2, 256, 1024, 2048, 1 << 14, 1 << 17])
def test_prove_fft_sizes(hb, oracle, s):
    rr = splitmix_field((2 * s).bit_length() - 1, 341)
    for name, m in proof_families(s).items():
        same(hb.prove_fft(m, rr), oracle.prove_fft(m, rr), "s=%d %s" % (s, name), SC_KEYS)


@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 256), (2, 4), (16, 256), (256, 1 << 11), (32, 1 << 14)])
def test_prove_fft_matrix_shapes(hb, oracle, rows, cols):
    rr = splitmix_field((2 * cols).bit_length() - 1 + rows.bit_length() - 1, 351)
    for name, m in proof_families(rows * cols).items():
        M = m.reshape(rows, cols, 2)
        same(hb.prove_fft_matrix(M, rr), oracle.prove_fft_matrix(M, rr), "rows=%d cols=%d %s" % (rows, cols, name), SC_KEYS)


# ---- g. the inner PCS provers --------------------------------------------------------------------------------------------------------
def whir_vs_oracle(hb, oracle, p, x, what):
    libc.srandom(7); want = oracle.whir_prove(p, x); after_oracle = libc.rand()
    libc.srandom(7); got = hb.whir_prove(p, x); after_device = libc.rand()
    assert want["checks"].tolist() == [1, 1] and got["checks"].tolist() == [1, 1], what + ": the reference's two checks"
    same(got, want, what)
    assert after_device == after_oracle, what + ": the libc stream is left at another point"
    return int(want["iters"][0])


# _whir_prove takes 2, 3, 4, 5 iterations for logN in 9-12, 13-16, 17-20, 21-24: the upper edge of the first class and its neighbour,
# the middle of the second, the lower and upper edge of the third, the first five-iteration size
@pytest.mark.parametrize("logN,iters", [(11, 2), (12, 2), (14, 3), (15, 3), (17, 4), (20, 4), (21, 5)])
def test_whir_prove_iteration_classes(hb, oracle, logN, iters):
    assert whir_vs_oracle(hb, oracle, splitmix_field(1 << logN, 1), splitmix_field(logN, 2), "logN=%d" % logN) == iters


def test_whir_prove_witness_like_polynomials(hb, oracle):
    N = 1 << 14
    fam = families(N, seed=14)
    for name in ("zeros", "all_pm1", "bits", "const", "mix", "neg_halves"):
        whir_vs_oracle(hb, oracle, fam[name], splitmix_field(14, 3), "logN=14 " + name)
    whir_vs_oracle(hb, oracle, splitmix_field(N, 4), point_families(14, 5)["special"], "logN=14 special point")


def test_whir_prove_size_limits(hb, oracle):
    """below 2^9 (where the reference itself fails) and above 2^24: refused before anything is drawn or launched"""
    d = hb.to_device(splitmix_field(1 << 9, 1)); x = splitmix_field(25, 2)
    hb.profile(True); hb.profile_reset()
    try:
        libc.srandom(5); before = libc.rand(); libc.srandom(5)
        for N in (1 << 8, 1 << 25, 1000, 0):
            assert hb.lib.hobbit_whir_prove(hb.ctx, d.ptr, N, d.ptr, d.ptr, vp(x), None) < 0, N
            assert b"whir_prove" in hb.lib.hobbit_last_error(hb.ctx), N
        assert libc.rand() == before, "a refused call drew from the libc generator"
        hb.sync()
        assert not hb.profile_report(), "a refused call launched %s" % sorted(hb.profile_report())
    finally:
        hb.profile(False); hb.profile_reset()
    whir_vs_oracle(hb, oracle, splitmix_field(1 << 9, 6), splitmix_field(9, 7), "logN=9 after the refusals")


def shockwave_vs_oracle(hb, oracle, p, k, what, x=None):
    N = p.shape[0]
    enc, lv = oracle.shockwave_commit(p, k)
    x = splitmix_field(N.bit_length() - 1, 4) if x is None else x
    libc.srandom(9); want = oracle.shockwave_prove(p, enc, k, x, lv); after_oracle = libc.rand()
    libc.srandom(9); got = hb.shockwave_prove(p, enc, k, x, lv); after_device = libc.rand()
    has_whir = N // k > 256
    assert int(want["iters"][0] > 0) == has_whir and want["wchecks"].tolist() == ([1, 1] if has_whir else [0, 0]), what
    same(got, want, what)
    assert after_device == after_oracle, what + ": the libc stream is left at another point"
    return enc


# widths N / k: 128 and 256 (no WHIR proof), 512 (the smallest with one, 2 iterations), 4096 (2 iterations, upper edge), 4096 with 64 rows
@pytest.mark.parametrize("N,k", [(1 << 8, 2), (1 << 10, 4), (1 << 14, 32), (1 << 17, 32), (1 << 18, 64)])
def test_shockwave_prove_shapes(hb, oracle, N, k):
    shockwave_vs_oracle(hb, oracle, splitmix_field(N, 3), k, "N=2^%d k=%d" % (N.bit_length() - 1, k))


def test_shockwave_prove_witness_like_polynomials(hb, oracle):
    N, k = 1 << 14, 8
    fam = families(N, seed=15)
    for name in ("zeros", "all_pm1", "bits", "const", "mix", "neg_halves"):
        shockwave_vs_oracle(hb, oracle, fam[name], k, "N=2^14 k=8 " + name)
    # rows 1 and k - 1 zero: shockwave_commit's no-FFT shortcut made their code rows
    p = splitmix_field(N, 5).reshape(k, N // k, 2).copy(); p[1] = 0; p[k - 1] = 0
    enc = shockwave_vs_oracle(hb, oracle, p.reshape(-1, 2), k, "N=2^14 k=8 rows 1 and 7 zero")
    assert not enc[1].any() and not enc[k - 1].any() and enc[0].any()
    d_enc, d_lv = hb.shockwave_commit(p.reshape(-1, 2), k)
    assert np.array_equal(d_enc, enc), "the device's commitment of the same polynomial"


# ---- h. every Merkle path ------------------------------------------------------------------------------------------------------------


def test_merkle_paths_direct(hb, oracle):
    n = 1 << 12
    l0 = np.random.default_rng(2).integers(0, 256, (n, 32), dtype=np.uint8)
    levels = oracle.create_tree_blake(l0)
    assert np.array_equal(hb.create_tree_blake(l0), levels)
    pos = np.concatenate([[0, 1, n - 2, n - 1], np.random.default_rng(3).integers(0, n, 1000), [7, 7, 7]]).astype(np.uint64)
    assert len(set(pos.tolist())) < len(pos)
    d = hb.to_device(levels)
    out = np.zeros((len(pos), 12, 32), np.uint8)
    hb._chk(hb.lib.hobbit_merkle_paths(hb.ctx, d.ptr, n, vp(pos), len(pos), vp(out)))
    assert np.array_equal(out, expected_paths(levels, n, pos))
    for q in (0, 3, 500):
        assert np.array_equal(out[q], oracle.open_tree_blake(levels, n, int(pos[q]), 0, n)), q       # (the gather itself against open_tree_blake)


@pytest.mark.parametrize("N,K", [(1 << 18, 4), (1 << 20, 32)])
def test_open_standard_every_merkle_path(hb, oracle, N, K):
    """all 5900 paths of the opening, and all 240 of each inner shockwave proof, against one gather from the oracle's levels; the WHIR
    query paths (the trees of its layers stay inside the proof) whole against the oracle's"""
    queries = 5900
    trs, poly, x, lv, T = open_case(oracle, N, K)
    M = N // K; cols = 2 * M // trs
    libc.srandom(777); want = oracle.open_standard(poly, K, trs, x, queries, tensor=T)
    hb.upload_graphs(trs, graphs_from(oracle, trs))
    c = hb.commit_standard(poly, K, trs, 1)
    libc.srandom(777); got = hb.open_standard(poly, c, x, queries, want_paths=True)
    c.free()
    assert np.array_equal(got["I"], want["I"])
    pos = (got["I"][:, 1].astype(np.int64) // 4) * cols + got["I"][:, 0].astype(np.int64)
    assert len(np.unique(pos)) > 5000 and pos.max() < M
    assert np.array_equal(got["paths"], expected_paths(lv, M, pos)), "N=2^%d K=%d: the opening's paths" % (N.bit_length() - 1, K)
    q = queries // 2
    assert np.array_equal(got["paths"][q], oracle.open_tree_blake(lv, M, int(got["I"][q, 0]), int(got["I"][q, 1]), cols))
    # the two inner commitments, rebuilt as Oracle.open_standard builds them
    logK = K.bit_length() - 1
    aggr = oracle.aggregate(poly, oracle.precompute_beta(x[:logK]))
    C = oracle.compute_tensorcode(aggr, trs, 1).reshape(2 * trs, cols, 2)[trs:].reshape(-1, 2)
    for sp, vec in (("sp_c", C), ("sp_f", aggr)):
        W = 2 * vec.shape[0] // 32
        lv_sp = oracle.shockwave_commit(vec, 32)[1]
        assert np.array_equal(got[sp]["I"], want[sp]["I"]), sp
        assert np.array_equal(got[sp]["paths"], expected_paths(lv_sp, W, got[sp]["I"])), "N=2^%d K=%d: %s paths" % (N.bit_length() - 1, K, sp)
        for k in ("qn", "qidx", "qpaths"):
            assert np.array_equal(got[sp][k], want[sp][k]), (sp, k)
