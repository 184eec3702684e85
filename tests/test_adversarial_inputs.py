"""The lazy-reduction kernels on structured and worst-case inputs (tests/adversarial.py), bit-exact against the oracle.

The row FFT keeps its butterfly sums unreduced (up to 8p + 7 = 2^64 - 1) and folds them into [0, p + 7]; the device product takes
components up to p + 7; the expander encode keeps 96-bit sums and folds each output once.  Uniform inputs practically never reach the
edges of those bounds: the families here do (zeros and constants give exact multiples of p, bits / small integers / ramps give sums
B p + j, all-(p-1) under weights 2^32 - 1 gives the largest 96-bit sums).  Every assert names the family."""
import numpy as np
import pytest
import adversarial as A
from adversarial import FAT_CHAIN_4096, P, encode_with_kernels, families, graphs_from, set_weights
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)
    yield h
    h.close()


def _stack(fams):
    names = list(fams)
    return names, np.stack([fams[k] for k in names])


# ---- field primitive -----------------------------------------------------------------------------
def test_field_limb_edges_cross_product(hb, oracle):
    """f_binop add / sub / mul on every (re, im) x (re, im) combination of the limb-edge component values (39^4 pairs)"""
    a, b = A.cross_pairs(A.LIMB_EDGES)
    for op, fn in ((0, oracle.f_add), (1, oracle.f_sub), (2, oracle.f_mul)):
        got, want = hb.f_binop(op, a, b), fn(a, b)
        bad = np.nonzero((got != want).any(1))[0]
        assert bad.size == 0, (op, bad.size, a[bad[:4]].tolist(), b[bad[:4]].tolist())


def test_field_mul_lazy_input_range(hb, oracle):
    """The device product documents components up to p + 7 (fmul_lazy; the FFT feeds it folded octet sums in [0, p + 7]) and returns the
    canonical product: components in [p, p + 7] mixed with canonical edges, on both operands, against the oracle's product of the reduced
    values"""
    vals = A.LAZY_RANGE + [0, 1, 7, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 60, P - 1]
    a, b = A.cross_pairs(vals)
    red = lambda x: np.where(x >= np.uint64(P), x - np.uint64(P), x).astype(np.uint64)
    got, want = hb.f_binop(2, a, b), oracle.f_mul(red(a), red(b))
    bad = np.nonzero((got != want).any(1))[0]
    assert bad.size == 0, (bad.size, a[bad[:4]].tolist(), b[bad[:4]].tolist())


# ---- FFT -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn", list(range(1, 13)))
def test_fft_rows_families(hb, oracle, logn):
    """every LDS-resident length (generic radix-2/4, radix-8 with its radix-1/2/4 tail, FFT-4096), all families in one batch with a ragged
    row count (13 families + 2 repeats: never a multiple of the rows a workgroup owns), forward and inverse, every row against the oracle"""
    n = 1 << logn
    names, x = _stack(families(n, seed=logn))
    names += ["mix#2", "all_pm1#2"]; x = np.concatenate([x, x[[names.index("mix"), names.index("all_pm1")]]])
    for inv in (False, True):
        y = hb.fft(x, inverse=inv)
        for r, name in enumerate(names):
            assert np.array_equal(y[r], oracle.fft(x[r], inverse=inv)), (name, logn, "inverse" if inv else "forward")


@pytest.mark.parametrize("logn", [13, 14, 15, 16, 17, 18, 19, 20])
def test_fft_long_families(hb, oracle, logn):
    """the long forms (strided FFT-4096 + column pass: radix-2/4 up to R = 16, radix-8 columns from R = 32) on every family, batched"""
    names, x = _stack(families(1 << logn, seed=logn))
    y = hb.fft(x)
    for r, name in enumerate(names):
        assert np.array_equal(y[r], oracle.fft(x[r])), (name, logn)


def test_fft_2e22_five_pass_families(hb, oracle):
    """2^22: beyond the 2-D twiddle table, the five-pass form (transpose + FFT-4096 + twiddled transpose + rows + transpose)"""
    fams = families(1 << 22, seed=22)
    for name in ("zeros", "const", "bits", "near_diff", "mix"):
        assert np.array_equal(hb.fft(fams[name]), oracle.fft(fams[name])), name


@pytest.mark.parametrize("logc,trs", [(12, 16), (13, 16), (16, 4)])
def test_tensorcode_zero_padded_rows_families(hb, oracle, logc, trs):
    """the zero-padded-half source (RS row code = FFT of the message row followed by zeros): the padded FFT-4096 (logc 12), the long row form
    over strided padded FFT-4096s (13) and fft_long's padded source (16); every family as the message, RS columns (lin = 0)"""
    M = trs << (logc - 1)
    for name, msg in families(M, seed=logc).items():
        assert np.array_equal(hb.compute_tensorcode(msg, trs, 0), oracle.compute_tensorcode(msg, trs, 0)), (name, logc, trs)


# (kernel's profile name, logn, inverse): every place the two older kernels are still reached.  k_fft_rows, the generic radix-2/4 kernel: forward
# below the radix-8 lengths, and every inverse of 6 .. 11.  k_fft_cols, the radix-2/4 column pass of the two-factor form: R = 4, 8, 16 (the
# radix-8 column kernel shares the profile name but is built for R >= 32 only, so at these lengths the name is k_fft_cols's own).
OLDER_KERNELS = [("k_fft_rows", logn, False) for logn in range(1, 6)] + [("k_fft_rows", logn, True) for logn in range(6, 12)] + \
                [("k_fft_cols", logn, inv) for logn in (14, 15, 16) for inv in (False, True)]


@pytest.mark.parametrize("kernel,logn,inv", OLDER_KERNELS)
def test_fft_older_kernels_families(hb, oracle, kernel, logn, inv):
    """the generic radix-2/4 rows and the radix-2/4 column pass where they still run, every family in one batch, every row against the oracle;
    the profiler names the kernel that was launched"""
    names, x = _stack(families(1 << logn, seed=logn))
    hb.profile(True); hb.profile_reset()
    y = hb.fft_any(x, inverse=inv)
    rep = hb.profile_report()
    hb.profile(False)
    assert rep.get(kernel, (0, 0))[1] == 1, rep
    assert not any(k in rep for k in ("k_fft_r8", "k_transpose_tw", "k_fft_cols_wide") + (("k_fft4096", "k_fft4096_full", "k_fft_cols") if kernel == "k_fft_rows" else ())), rep
    for r, name in enumerate(names):
        assert np.array_equal(y[r], oracle.fft(x[r], inverse=inv)), (name, logn, "inverse" if inv else "forward")


# ---- expander encode -----------------------------------------------------------------------------
def _graphs(oracle, n, weights):
    oracle.rng_reset(); oracle.expander_init_store(n)
    lv = graphs_from(oracle, n)
    if weights is not None:
        lv = set_weights(oracle, lv, weights)
    return lv


WEIGHTS = {"drawn": None, "2^32-1": [(1 << 32) - 1, 0], "full_p-1": [P - 1, P - 1]}


def _oracle_encode(oracle, x):
    return [oracle.encode_monolithic(row) for row in x]


def _check_encode(got, wants, names, tag):
    for r, name in enumerate(names):
        want, ln = wants[r]
        assert np.array_equal(got[r][:ln], want[:ln]), (tag, name)
        assert not got[r][ln:].any(), (tag, name, "tail")


@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("n,modes", [(1024, ("out",)), (3000, ("out", "in")), (4000, ("out", "in")), (6000, ("out", "in")), (16384, ("out", "in"))])
def test_encode_families(hb, oracle, n, modes, wname):
    """single pass (1024), the A/B split (3000, 4000) and the tiled long code (6000, 16384), out of place and in place; every family as a
    message, under the drawn weights, every weight 2^32 - 1 (the 32-bit-weight kernels' largest 96-bit sums; all-(p-1) is one of the
    families) and every weight (p-1, p-1) (the full-range-weight kernels)"""
    lv = _graphs(oracle, n, WEIGHTS[wname])
    hb.upload_graphs(n, lv)
    names, x = _stack(families(n, seed=n))
    wants = _oracle_encode(oracle, x)
    for mode in modes:
        _check_encode(hb.encode_monolithic(x, in_place=(mode == "in")), wants, names, (n, wname, mode))


@pytest.mark.parametrize("wname", list(WEIGHTS))
def test_encode_4096_in_place_paths_families(hb, oracle, wname):
    """n = 4096 in place, the commit's form (the persistent k_enc_fat chain under 32-bit weights, the full-weight A/B split otherwise), and
    the out-of-place A/B split: both against the oracle, and against each other on every column"""
    lv = _graphs(oracle, 4096, WEIGHTS[wname])
    hb.upload_graphs(4096, lv)
    names, x = _stack(families(4096, seed=4096))
    wants = _oracle_encode(oracle, x)
    fullw = wname == "full_p-1"
    out, ran = encode_with_kernels(hb, x, in_place=False)
    assert ran == ({"k_encode_fullw_A", "k_encode_fullw_B"} if fullw else {"k_encode_A", "k_encode_B"}), (wname, ran)
    _check_encode(out, wants, names, (wname, "out"))
    got, ran = encode_with_kernels(hb, x, in_place=True)
    assert ran == ({"k_encode_fullw_A", "k_encode_fullw_B"} if fullw else FAT_CHAIN_4096), (wname, ran)
    _check_encode(got, wants, names, (wname, "in"))
    assert np.array_equal(got, out), wname


def _raise_in_degree(g, t, deg):
    """re-point edges of graph g (upload_graphs' form) at output t, in input order, until t has in-degree deg"""
    nbr = np.array(g["nbr"], np.int64).reshape(-1)
    have = int((nbr == t).sum())
    moved = np.flatnonzero(nbr != t)[:deg - have]
    nbr[moved] = t
    assert int((nbr == t).sum()) == deg
    return dict(g, nbr=nbr.reshape(np.shape(g["nbr"])))


# (level, in-degree one past the fat kernel's first register cap (hobbit_ctx.hpp FAT_*_CAP0), kernels in place)
FAT_FALLBACKS = {
    "C1_over_64": ((1, 0), 65, {"k_enc_fat_A", "k_encode_C1", "k_encode_M2", "k_enc_fat_D"}),
    "D0_over_28": ((0, 1), 29, {"k_enc_fat_A", "k_encode_B"}),
    "C0_over_72": ((0, 0), 73, {"k_encode_A", "k_encode_B"}),
}


@pytest.mark.parametrize("case", list(FAT_FALLBACKS))
def test_encode_4096_in_place_fat_fallbacks(hb, oracle, case):
    """n = 4096 in place with one output of a fat step past the kernel's register cap: that step falls back to the one-workgroup-per-column
    kernels, chosen from the graph alone; bit for bit the out-of-place A/B split on every column"""
    key, deg, kernels = FAT_FALLBACKS[case]
    oracle.rng_reset(); oracle.expander_init_store(4096)
    lv = graphs_from(oracle, 4096)
    lv[key] = _raise_in_degree(lv[key], 0, deg)
    hb.upload_graphs(4096, lv)
    x = np.concatenate([_stack(families(4096, seed=4096))[1], splitmix_field(300 * 4096, 4096).reshape(300, 4096, 2)])
    got, ran = encode_with_kernels(hb, x, in_place=True)
    assert ran == kernels, (case, ran)
    out, ran = encode_with_kernels(hb, x, in_place=False)
    assert ran == {"k_encode_A", "k_encode_B"}, (case, ran)
    assert np.array_equal(got, out), case
    assert not got[:, 7045:].any(), case


# ---- through the library -------------------------------------------------------------------------
@pytest.mark.parametrize("lin", [1, 0])
def test_commit_standard_2e20_families(hb, oracle, lin):
    """commit_standard at N = 2^20, K = 32 on witness-like polynomials (their rows reach the FFT's lazy states at 4096 points, the expander
    code's columns see runs of zeros and tiny values): every level and sampled tensor entries against oracle.commit_standard"""
    N, K = 1 << 20, 32
    trs = N // (K << 11)
    oracle.rng_reset(); oracle.expander_init_store(trs)
    hb.upload_graphs(trs, graphs_from(oracle, trs))
    fams = families(N, seed=20)
    rng = np.random.default_rng(20)
    rows = np.concatenate([[0, trs - 1, trs, 2 * trs - 1], rng.integers(0, 2 * trs, 60)]).astype(np.uint32)
    cols = np.concatenate([[0, 4095, 1, 2048], rng.integers(0, 4096, 60)]).astype(np.uint32)
    for name in ("bits", "small", "const", "zeros"):
        want_lv, T = oracle.commit_standard(fams[name], K, trs, lin, want_tensor=True)
        c = hb.commit_standard(fams[name], K, trs, lin)
        assert np.array_equal(c.levels(), want_lv), (name, lin)
        rep = c.gather(rows, cols)
        for q in range(rows.size):
            assert np.array_equal(rep[q], T[:, rows[q], cols[q]]), (name, lin, int(rows[q]), int(cols[q]))
        c.free()


SP_KEYS = ("I", "q1", "r1", "vr1", "fin1", "q2", "r2", "vr2", "fin2", "iters", "wq", "wa", "wroots", "wscal", "wchecks", "whir_root",
           "reply", "paths", "qn", "qidx", "qreply", "qpaths", "final_pb")


def test_open_standard_2e20_bits(hb, oracle):
    """open_standard at 2^20 on a bits polynomial (the opening's aggregations, inner FFT commitments and WHIR rounds on witness data),
    every transcript entry against the oracle as test_open_standard_vs_oracle does"""
    import ctypes
    libc = ctypes.CDLL(None)
    N, K = 1 << 20, 32
    trs = N // (K << 11)
    oracle.rng_reset(); oracle.expander_init_store(trs)
    poly = families(N, seed=21)["bits"]
    x = oracle.generate_randomness(20)
    lv, T = oracle.commit_standard(poly, K, trs, 1, want_tensor=True)
    libc.srandom(777); want = oracle.open_standard(poly, K, trs, x, 5900, tensor=T)
    hb.upload_graphs(trs, graphs_from(oracle, trs))
    c = hb.commit_standard(poly, K, trs, 1)
    assert np.array_equal(c.levels(), lv)
    libc.srandom(777); got = hb.open_standard(poly, c, x, 5900, want_paths=True)
    assert want["checks"].tolist() == [1, 1, 1] and got["checks"].tolist() == [1, 1, 1]
    for k in ("I", "scalars", "poly", "r", "vr", "fin", "roots", "reply"):
        assert np.array_equal(got[k], want[k]), k
    for q in range(0, 5900, 97):
        assert np.array_equal(got["paths"][q], oracle.open_tree_blake(lv, N // K, int(got["I"][q, 0]), int(got["I"][q, 1]), 4096)), q
    for sp in ("sp_c", "sp_f"):
        for k in SP_KEYS:
            assert np.array_equal(got[sp][k], want[sp][k]), (sp, k)
    c.free()


@pytest.mark.parametrize("logn", [10, 17])
def test_sumchecks_eval_beta_families(hb, oracle, logn):
    """sumcheck2 / sumcheck3, evaluate_vector and precompute_beta on the all-(p-1), zeros and bits tables (as tables and as points), at one
    single-launch and one multi-launch size"""
    n = 1 << logn
    fams = families(n, seed=logn)
    pts = families(logn, seed=logn)
    pr = np.array([33, 0], np.uint64)
    for name in ("all_pm1", "zeros", "bits"):
        v = fams[name]; w = fams["mix"]
        for k, val in oracle.sumcheck2(v, w, pr).items():
            assert np.array_equal(hb.generate_2product_sumcheck_proof(v, w, pr)[k], val), (name, "sumcheck2", k)
        got3 = hb.generate_3product_sumcheck_proof(v, v, w, pr)
        for k, val in oracle.sumcheck3(v, v, w, pr).items():
            assert np.array_equal(got3[k], val), (name, "sumcheck3", k)
        for rname in ("all_pm1", "zeros", "bits", "mix"):
            assert np.array_equal(hb.evaluate_vector(v, pts[rname]), oracle.evaluate_vector(v, pts[rname])), (name, rname, "evaluate_vector")
        assert np.array_equal(hb.precompute_beta(pts[name]), oracle.precompute_beta(pts[name])), (name, "precompute_beta")
