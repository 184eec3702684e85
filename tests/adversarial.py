"""Structured and worst-case F_{p^2} inputs for the lazy-reduction kernels (tests/test_adversarial_inputs.py, tests/test_oracle_selfcheck.py).

Uniform inputs (splitmix_field) almost never reach the states the hot kernels' hand-derived bounds are about: an FFT octet's fold landing in
[p, p + 7] needs two butterfly operands that differ by a small integer (chance ~2^-58 per fold for uniform data); the device product's
lazy-input range [p, p + 7] is not canonical at all; the expander encode's 96-bit sums are largest for all-(p-1) messages under weights
2^32 - 1.  Witness-like data -- bits, small integers, constants, ramps -- gets there at once.  Every family here is canonical (components
< p) so the oracle can take it as it is; each has a stated purpose (PURPOSE), and FAMILIES(n) returns them by name for the assert messages.
"""
import numpy as np

P = (1 << 61) - 1
U = np.uint64


def _splitmix(n, seed):
    from oracle.pyoracle import splitmix_field
    return splitmix_field(n, seed)


def _neg(x):
    """-x mod p, componentwise, canonical"""
    x = np.asarray(x, np.uint64)
    return np.where(x == 0, U(0), U(P) - x).astype(np.uint64)


# 31-bit limb split of the device product (x = x0 + 2^31 x1) and other component values at its edges; all canonical
LIMB_EDGES = [0, 1, 2, 3, 7, 8, 15, 16, 12345,
              (1 << 30) - 1, 1 << 30, (1 << 31) - 2, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 3 << 31, (1 << 32) - 1, 1 << 32, (1 << 33) - 1,
              1 << 33, (1 << 40) - 1, (1 << 45) + 1, 1 << 59, (1 << 60) - 1, 1 << 60, (1 << 60) + 1, (1 << 60) + (1 << 31) - 1,
              (1 << 60) + ((1 << 30) - 1) * (1 << 30), ((1 << 30) - 1) << 31, (((1 << 30) - 1) << 31) + 1, (((1 << 30) - 1) << 31) - 1,
              (1 << 61) - (1 << 32) + 1, 0x5555555555555555 & P, 0x0AAAAAAAAAAAAAAA, 0x1234567890ABCDEF & P, P - 8, P - 7, P - 2, P - 1]
assert len(set(LIMB_EDGES)) == len(LIMB_EDGES) >= 38 and all(0 <= v < P for v in LIMB_EDGES)
# the lazy input range the device product documents (fmul_lazy: components <= p + 7) and FFT octets feed it: p .. p + 7
LAZY_RANGE = [P + j for j in range(8)]

PURPOSE = {
    "zeros": "all zero: every lazy a - b is a + (B p - b) = B p exactly, which folds to p (the canonicalisation must map it to 0)",
    "all_pm1": "all (p-1, p-1): largest canonical components -- worst case of every unreduced sum (FFT levels, encode's 96-bit sums)",
    "const": "one constant: an FFT output of n c at 0 and exact zeros elsewhere, each reached as a multiple of p",
    "bits": "bits {0, 1} in re only (a witness): butterfly operands differ by 0 or 1, so a + B p - b lands on B p + j",
    "small": "small integers 0..15 in both components: sums B p + j, j < 16, at every level",
    "ramp": "x_i = i: neighbours differ by one, every first-level difference a small integer",
    "neg_interleave": "x, -x interleaved: pairwise cancellation, exact zeros reached through a + (p - a)",
    "neg_halves": "second half = -(first half): the DIT first stage (x_j, x_{j+n/2}) sums to exactly zero",
    "near_diff": "a large constant plus 0..7 by eighth of the row, so the stride-n/8 partners of an octet differ by 1..7 and a + B p - b lands on B p + j",
    "impulse_first": "(p-1, p-1) at position 0, zeros elsewhere",
    "impulse_last": "(p-1, p-1) at the last position, zeros elsewhere",
    "limbs": "components at the 31-bit limb split of the device product (2^31 - 1, (2^30 - 1) 2^31, 2^31, 2^32 - 1, 2^60, p - 1, ...)",
    "mix": "blocks of the small-integer families (bits, zeros, small, ramp, impulses) one after the other: a witness of mixed columns",
}


def families(n, seed=0):
    """{name: (n, 2) uint64}, every entry canonical"""
    i = np.arange(n, dtype=np.uint64)
    out = {}
    out["zeros"] = np.zeros((n, 2), np.uint64)
    out["all_pm1"] = np.full((n, 2), P - 1, np.uint64)
    out["const"] = np.tile(np.array([[0x0123456789ABCDEF % P, 42]], np.uint64), (n, 1))
    r = _splitmix(n, 3000 + seed)
    out["bits"] = np.stack([r[:, 0] & U(1), np.zeros(n, np.uint64)], 1)
    out["small"] = (r >> U(7)) & U(15)
    out["ramp"] = np.stack([i % U(P), np.zeros(n, np.uint64)], 1)
    x = _splitmix((n + 1) // 2, 1000 + seed)
    ni = np.empty((2 * x.shape[0], 2), np.uint64); ni[0::2] = x; ni[1::2] = _neg(x)
    out["neg_interleave"] = ni[:n].copy()
    hx = _splitmix(max(n // 2, 1), 2000 + seed)
    nh = np.zeros((n, 2), np.uint64)
    if n >= 2:
        nh[: n // 2] = hx[: n // 2]; nh[n // 2: n // 2 * 2] = _neg(hx[: n // 2])
    else:
        nh[:] = hx[:n]
    out["neg_halves"] = nh
    base = np.array([P - 20, (1 << 60) + 5], np.uint64)
    oc = (i * U(8)) // U(n)                            # which eighth of the row: the stride-n/8 partners of a radix-8 octet differ by 1..7
    out["near_diff"] = np.stack([base[0] + oc, base[1] + ((oc * U(3)) % U(8))], 1).astype(np.uint64)
    imp = np.zeros((n, 2), np.uint64); imp[0] = P - 1
    out["impulse_first"] = imp
    imp = np.zeros((n, 2), np.uint64); imp[-1] = P - 1
    out["impulse_last"] = imp
    L = np.array(LIMB_EDGES, np.uint64)
    out["limbs"] = np.stack([L[i % U(len(L))], L[(i * U(7) + U(3)) % U(len(L))]], 1)
    names = ["bits", "zeros", "small", "ramp", "impulse_first", "impulse_last"]     # small integers only: cut together they stay small
    blk = max(1, n // 16)
    mix = np.empty((n, 2), np.uint64)
    for b0 in range(0, n, blk):
        mix[b0:b0 + blk] = out[names[(b0 // blk) % len(names)]][b0:b0 + blk]
    out["mix"] = mix
    for k, v in out.items():
        assert v.shape == (n, 2) and v.dtype == np.uint64 and (v < U(P)).all(), k
    return out


def cross_pairs(values):
    """every (re, im) x (re, im) combination of `values`: (a, b) arrays of len(values)^4 elements"""
    v = np.asarray(values, np.uint64)
    m = len(v)
    g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 4)
    a = np.stack([v[g[:, 0]], v[g[:, 1]]], 1)
    b = np.stack([v[g[:, 2]], v[g[:, 3]]], 1)
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


# ---- plain Python big-integer references ------------------------------------------------------
def py_add(a, b):
    return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)


def py_sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def py_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def py_pow(x, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = py_mul(r, x)
        x = py_mul(x, x); e >>= 1
    return r


def py_dft(x, w):
    """X[k] = sum_j x[j] w^(jk), straight from the definition"""
    n = len(x)
    pw = [(1, 0)] * n
    for t in range(1, n):
        pw[t] = py_mul(pw[t - 1], w)
    out = []
    for k in range(n):
        s = (0, 0)
        for j in range(n):
            s = py_add(s, py_mul(x[j], pw[(j * k) % n]))
        out.append(s)
    return out


def to_py(a):
    return [(int(r), int(i)) for r, i in np.asarray(a, np.uint64).reshape(-1, 2)]


def from_py(v):
    return np.array(v, dtype=np.uint64).reshape(-1, 2)


# ---- big-integer restatements of the circuit prover's element-wise operations (tests/test_circuit_refs_cpu.py proves them against the
# oracle; tests/test_circuit_prover_shapes.py holds the device to them).  Tables are lists of (re, im) Python integers (to_py).
ONE, ZERO = (1, 0), (0, 0)


def py_sum(terms):
    s = ZERO
    for t in terms:
        s = py_add(s, t)
    return s


def py_gate3(s, lookup_rand=None):
    """compute3p_error_terms' gate: F(selector) without lookups; with them 0 and 4 -> 1, 2 -> lookup_rand[0], 3 -> lookup_rand[1], else 0"""
    s = int(s)
    if lookup_rand is None:
        return (s % P, 0)
    return ONE if s in (0, 4) else lookup_rand[0] if s == 2 else lookup_rand[1] if s == 3 else ZERO


def py_gate4(s, lookups=False):
    """compute4p_error_terms' gate: 1 - F(selector) without lookups, [selector == 1] with them"""
    s = int(s)
    return (1 if s == 1 else 0, 0) if lookups else py_sub(ONE, (s % P, 0))


def py_err2p(b1, b2, f1, f2):
    """K1 = sum b1 f2 + b2 f1, K2 = sum b1 b2 (src/sumcheck.cpp:374-379)"""
    n = len(b1)
    return [py_sum(py_add(py_mul(b1[i], f2[i]), py_mul(b2[i], f1[i])) for i in range(n)), py_sum(py_mul(b1[i], b2[i]) for i in range(n))]


def py_err3p(b1, gate, f1, f2, f3, beta, lookup_rand=None):
    """with g = the gate: K1 = sum f3 (b1 f2 + g f1) + beta f1 f2, K2 = sum beta (b1 f2 + g f1) + f3 b1 g, K3 = sum b1 g beta (:407-432)"""
    K = [ZERO, ZERO, ZERO]
    for j in range(len(b1)):
        g = py_gate3(gate[j], lookup_rand)
        t1 = py_add(py_mul(b1[j], f2[j]), py_mul(g, f1[j])); t2 = py_mul(b1[j], g)
        K[0] = py_add(K[0], py_add(py_mul(f3[j], t1), py_mul(py_mul(beta[j], f1[j]), f2[j])))
        K[1] = py_add(K[1], py_add(py_mul(beta[j], t1), py_mul(f3[j], t2)))
        K[2] = py_add(K[2], py_mul(t2, beta[j]))
    return K


def py_err4p(b1, b2, b3, gate, f1, f2, f3, f4, lookups=False):
    """the four coefficients of sum (f1 + x b1)(f2 + x b2)(f3 + x b3)(f4 + x g) above the constant one, lowest first (:381-405)"""
    K = [ZERO] * 4
    for i in range(len(b1)):
        g = py_gate4(gate[i], lookups)
        t1 = py_add(py_mul(f1[i], b2[i]), py_mul(f2[i], b1[i])); t2 = py_add(py_mul(f3[i], g), py_mul(f4[i], b3[i]))
        t3 = py_mul(b1[i], b2[i]); t4 = py_mul(g, b3[i]); t5 = py_mul(f1[i], f2[i]); t6 = py_mul(f3[i], f4[i])
        K[0] = py_add(K[0], py_add(py_mul(t1, t6), py_mul(t2, t5)))
        K[1] = py_add(K[1], py_add(py_add(py_mul(t1, t2), py_mul(t3, t6)), py_mul(t4, t5)))
        K[2] = py_add(K[2], py_add(py_mul(t1, t4), py_mul(t2, t3)))
        K[3] = py_add(K[3], py_mul(t3, t4))
    return K


def py_batch_terms(b1, b2, b3, f1, f2, f3):
    """the three sums of one batch_prod batch (:1093-1111): compute3p's with the third chunk b3 in beta's place and b2 in the gate's"""
    K = [ZERO, ZERO, ZERO]
    for k in range(len(b1)):
        t1 = py_add(py_mul(b1[k], f2[k]), py_mul(b2[k], f1[k])); t2 = py_mul(b1[k], b2[k])
        K[0] = py_add(K[0], py_add(py_mul(f3[k], t1), py_mul(py_mul(b3[k], f1[k]), f2[k])))
        K[1] = py_add(K[1], py_add(py_mul(b3[k], t1), py_mul(f3[k], t2)))
        K[2] = py_add(K[2], py_mul(t2, b3[k]))
    return K


def py_axpy(y, a, x):
    """y + a x"""
    return [py_add(y[i], py_mul(a, x[i])) for i in range(len(y))]


def py_axpy_i32(y, a, sel, one_minus=False):
    """y + a F(sel), or y + a (1 - F(sel))"""
    v = [py_sub(ONE, (int(s) % P, 0)) if one_minus else (int(s) % P, 0) for s in sel]
    return py_axpy(y, a, v)


def py_fingerprint(addr, value, a, freq=None, b=None):
    """addr + 1 + a value (+ b freq)"""
    out = [py_add(py_add(addr[i], ONE), py_mul(a, value[i])) for i in range(len(addr))]
    return out if freq is None else [py_add(out[i], py_mul(b, freq[i])) for i in range(len(out))]


def py_fold_rows(rows, r):
    """adjacent rows folded with r: row j = row 2j + r (row 2j+1 - row 2j)"""
    return [[py_add(a, py_mul(r, py_sub(b, a))) for a, b in zip(rows[2 * j], rows[2 * j + 1])] for j in range(len(rows) // 2)]


def py_prepare_matrix_cols(M, r):
    """M: (rows, cols, 2); the rows folded len(r) times (r[0] first), then row 0: column c's multilinear evaluation over the row index
    when len(r) = log2 rows, the first entry of its partial fold otherwise"""
    rows = [to_py(row) for row in np.asarray(M, np.uint64)]
    for rt in to_py(r) if len(r) else []:
        rows = py_fold_rows(rows, rt)
    return rows[0]


def py_phi_g(rx, w, scale=ONE, ifft=False):
    """phiGInit by its doubling recurrence: g[0] = scale; level i = 1, 2, ... with half = 2^(i-1), m = n - i and c = rx[m]:
    g[b ^ half] = g[b] ((1 - c) - c w^(b 2^m)), g[b] = g[b] ((1 - c) + c w^(b 2^m)) for b < half.  The inverse table (w -> 1 / w) runs
    levels 1 .. n; the forward table runs 1 .. n - 1 and closes with level n updating g[b] alone, so its upper half stays zero.
    w: the 2^n-th root of unity (oracle.root_of_unity(n))."""
    n = len(rx); N = 1 << n
    if ifft:
        w = py_pow(w, N - 1)
    pm = [ONE] * N
    for t in range(1, N):
        pm[t] = py_mul(pm[t - 1], w)
    g = [ZERO] * N; g[0] = scale
    for i in range(1, n + 1):
        half, m = 1 << (i - 1), n - i
        t1 = py_sub(ONE, rx[m])
        left_only = (i == n) and not ifft
        for b in range(half):
            t2 = py_mul(rx[m], pm[b << m])
            if not left_only:
                g[b ^ half] = py_mul(g[b], py_sub(t1, t2))
            g[b] = py_mul(g[b], py_add(t1, t2))
    return g


def py_cubic_claim(t1, t2, t3, lens, a):
    """sum_j a_j sum_i t1 t2 t3 over table j of the concatenated tables: round 0's p(0) + p(1) of the batched cubic sumcheck"""
    s, o = ZERO, 0
    for j, ln in enumerate(lens):
        s = py_add(s, py_mul(a[j], py_sum(py_mul(py_mul(t1[i], t2[i]), t3[i]) for i in range(o, o + int(ln)))))
        o += int(ln)
    return s


LK_VALUES = (-1, 0, 1, 2, 3, 4)        # every selector prove_gate_consistency_lookups hands the error terms over its three rewrites


def selectors(n, lookups=False):
    """{name: (n,) int32} gate selectors.  Without lookups they are 0 / 1 (the gate is F(s) or 1 - F(s)); lookups=True adds the lookup
    prover's values: all six in turn, and each alone (one branch of the selector map per array)."""
    i = np.arange(n)
    last = np.zeros(n, np.int32); last[-1] = 1
    out = {"zeros": np.zeros(n, np.int32), "ones": np.ones(n, np.int32), "alternate": (i % 2).astype(np.int32), "only_last": last,
           "thirds": (i % 3 == 0).astype(np.int32)}
    if lookups:
        out["lk_cycle"] = (i % 6 - 1).astype(np.int32)
        for v in LK_VALUES:
            out["lk_all_%s" % (("m%d" % -v) if v < 0 else v)] = np.full(n, v, np.int32)
    return out


def graphs_from(oracle, n):
    """the oracle's current expander graphs for message length n, {(dep, kind): dict(L, R, degree, nbr, w)} (Hobbit.upload_graphs' form)"""
    lv, dep, m = {}, 0, n
    while m > 13:
        for kind in (0, 1):
            lv[(dep, kind)] = oracle.graph(dep, kind)
        m = int(0.211 * m); dep += 1
    return lv


def encode_with_kernels(hb, x, in_place):
    """hb.encode_monolithic(x, in_place) under the profiler: the codewords and the names of the kernels that ran"""
    hb.profile(True); hb.profile_reset()
    try:
        y = hb.encode_monolithic(x, in_place=in_place)
        return y, set(hb.profile_report())
    finally:
        hb.profile(False); hb.profile_reset()


# n = 4096 in place with small weights: C_0, C_1 and D_0 by the persistent register-resident kernels, C_2 .. D_1 by k_encode_M2
FAT_CHAIN_4096 = {"k_enc_fat_A", "k_enc_fat_C1", "k_encode_M2", "k_enc_fat_D"}


def set_weights(oracle, lv, w):
    """every edge weight of every level set to the F element w, on the oracle and in lv (returned for upload_graphs)"""
    w = np.asarray(w, np.uint64).reshape(2)
    for key, g in lv.items():
        g["w"] = np.tile(w, (g["L"] * g["degree"], 1))
        oracle.graph_set_weights(key[0], key[1], g["w"])
    return lv


def py_encode(lv, src):
    """src/linear_code_encode.h:62-119 as a plain sum over the edge lists: codeword [x | Enc(C x) | D Enc(C x)], Python integers"""
    def rec(x, dep):
        n = len(x)
        if n <= 13:
            return list(x)
        C, D = lv[(dep, 0)], lv[(dep, 1)]
        s1 = [(0, 0)] * C["R"]
        for i in range(n):
            for d in range(C["degree"]):
                e = i * C["degree"] + d
                t = int(C["nbr"][e]); w = (int(C["w"][e, 0]), int(C["w"][e, 1]))
                s1[t] = py_add(s1[t], py_mul(w, x[i]))
        cw = rec(s1, dep + 1)
        z = [(0, 0)] * D["R"]
        for i in range(D["L"]):
            for d in range(D["degree"]):
                e = i * D["degree"] + d
                t = int(D["nbr"][e]); w = (int(D["w"][e, 0]), int(D["w"][e, 1]))
                z[t] = py_add(z[t], py_mul(cw[i], w))
        return list(x) + cw + z
    return rec(list(src), 0)


# ---- sorted index lists for the sparse 2-product sumcheck (tests/test_sumcheck_shapes.py) -------------------------------------------
# k_sc2_sparse_round cuts the list into 1024 slices of per = ceil(m / 1024) entries and regroups the entries into quads (index >> 2)
# that may straddle those slices; each list below puts the cut, the quads or the list length somewhere the opening's own lists never do.
SPARSE_PURPOSE = {
    "single_first": "m = 1 at index 0: one thread owns the whole list, quad 0",
    "single_last": "m = 1 at index n - 1: the last element of the last quad",
    "single_mid": "m = 1 at index n / 2 + 1",
    "one_quad_last": "the four indices of the last quad: one full quad, per = 1, each entry in another thread's slice",
    "full_quads": "all four entries of 300 consecutive quads from quad 777: m = 1200, per = 2, every quad cut across two slices",
    "odd_run": "2^16 + 3 consecutive indices from 4099: per = 65, slice boundaries at every phase of a quad",
    "powers_of_4": "4^j for every 4^j < n, and n - 1: loses entries at every fold, two entries long before the dense hand-over",
    "m_1023": "1023 uniform indices: one thread owns nothing",
    "m_1024": "1024 uniform indices: exactly one entry per thread",
    "m_1025": "1025 uniform indices: per = 2, half the threads own nothing",
    "open_like": "5900 draws with replacement, last write wins, values the powers of one scalar: the opening's own buff2",
    "max_spread": "n / 4 entries, one per quad at offset q % 4: the most entries that survive the first fold",
}


def open_like_list(n, queries=5900, seed=0):
    """(idx, val) as OpenRun::host_tables builds buff2 (src/PC_utils.cpp:331-336): position q drawn with replacement gets s^(q+1), the last
    write of a position wins; sorted by position"""
    rng = np.random.default_rng(9000 + seed)
    pos = rng.integers(0, n, queries)
    s = tuple(int(v) for v in _splitmix(1, 9100 + seed)[0])
    last, pw = {}, s
    for q in range(queries):
        last[int(pos[q])] = pw
        pw = py_mul(pw, s)
    idx = np.array(sorted(last), np.uint64)
    return idx, from_py([last[int(i)] for i in idx])


def sparse_lists(n, seed=0):
    """{name: strictly increasing uint64 indices < n} for a table of n >= 2^17 entries (SPARSE_PURPOSE); open_like's values come from open_like_list"""
    assert n >= 1 << 17 and n & (n - 1) == 0
    rng = np.random.default_rng(7000 + seed)
    out = {"single_first": [0], "single_last": [n - 1], "single_mid": [n // 2 + 1], "one_quad_last": [n - 4, n - 3, n - 2, n - 1]}
    out["full_quads"] = np.arange(4 * 777, 4 * (777 + 300))
    out["odd_run"] = np.arange(4099, 4099 + (1 << 16) + 3)
    p4 = [4 ** j for j in range(32) if 4 ** j < n]
    out["powers_of_4"] = sorted(set(p4 + [n - 1]))
    for m in (1023, 1024, 1025):
        out["m_%d" % m] = np.sort(rng.choice(n, m, replace=False))
    out["open_like"] = open_like_list(n, seed=seed)[0]
    q = np.arange(n // 4)
    out["max_spread"] = 4 * q + q % 4
    out = {k: np.ascontiguousarray(v, dtype=np.uint64) for k, v in out.items()}
    for k, v in out.items():
        assert k in SPARSE_PURPOSE and len(v) >= 1 and int(v[-1]) < n and (np.diff(v.astype(np.int64)) > 0).all(), k
    return out


def short_sparse_lists(n, seed=0):
    """the lists for tables short enough to be scattered at once: one entry at either end, every entry, and min(n / 2, 1000) uniform ones"""
    rng = np.random.default_rng(7500 + seed)
    out = {"single_first": [0], "single_last": [n - 1], "all": np.arange(n), "uniform": np.sort(rng.choice(n, min(n // 2, 1000), replace=False))}
    return {k: np.ascontiguousarray(v, dtype=np.uint64) for k, v in out.items()}


def pm1_with_zeros(m):
    """m values, all (p-1, p-1) but every seventh, which is exactly zero: a listed zero has to act as a zero"""
    v = np.full((m, 2), P - 1, np.uint64)
    v[6::7] = 0
    return v


def scatter_dense(n, idx, val):
    """the dense table the list stands for"""
    v = np.zeros((n, 2), np.uint64)
    v[np.asarray(idx, np.int64)] = val
    return v


def with_kernels(hb, fn):
    """fn() under the profiler: its result and the names of the kernels that ran"""
    hb.profile(True); hb.profile_reset()
    try:
        return fn(), set(hb.profile_report())
    finally:
        hb.profile(False); hb.profile_reset()


def gate_sumcheck_inputs(n):
    """six full-range tables (add, beta, L, R, O, mul: the folded selectors are full-range after the streaming phase), a[0..3] and the
    transcript seed of the degree-4 gate sumcheck"""
    from oracle.pyoracle import splitmix_field
    add = splitmix_field(n, 801); mul = splitmix_field(n, 802)
    tabs = [add, splitmix_field(n, 803), splitmix_field(n, 804), splitmix_field(n, 805), splitmix_field(n, 806), mul]
    return tabs, splitmix_field(4, 807), splitmix_field(1, 808)[0]
