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


# ---- the expander encode on graphs other than the drawn one (tests/test_encode_graphs.py, tests/test_encode_graph_families_cpu.py) -----------
# hobbit_graph_finalize chooses every kernel form of the encode from the shape and the in-degrees of the uploaded graphs.  expected_forms
# restates that choice in plain Python, expected_chain the launches launch_encode / launch_encode_long make of it, and the builders below put
# graphs at, just below and just above every rule in front of both.
def ctx_constants():
    """{name: [values]} of csrc/hobbit_ctx.hpp's NARROW_*, FAT_*, TILE_* tables and ENC_WIDE_MIN"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd", "csrc", "hobbit_ctx.hpp")).read()
    out = {}
    for name, val in re.findall(r"\b((?:NARROW|FAT|TILE)_[A-Z0-9_]+|ENC_WIDE_MIN)(?:\[[A-Z_]+\])? = (\{[0-9, ]+\}|[0-9]+)[,;]", src):
        out[name] = [int(v) for v in re.findall(r"[0-9]+", val)]
    return out


CTX = ctx_constants()
FAT = {   # step -> (level key, outputs per lane, consumer waves, register slots per position)
    "fatA": ((0, 0), CTX["FAT_A_NOUT"][0], CTX["FAT_A_CONS"][0], [CTX["FAT_A_CAP0"][0], CTX["FAT_A_CAP1"][0]]),
    "fatC1": ((1, 0), CTX["FAT_C1_NOUT"][0], CTX["FAT_C1_CONS"][0], [CTX["FAT_C1_CAP0"][0]]),
    "fatD": ((0, 1), CTX["FAT_D_NOUT"][0], CTX["FAT_D_CONS"][0], [CTX["FAT_D_CAP0"][0], CTX["FAT_D_CAP1"][0], CTX["FAT_D_CAP2"][0]]),
}
assert all(len(cap) == nout for _, nout, _, cap in FAT.values())
LEVEL_NAMES = {"C0": (0, 0), "C1": (1, 0), "C2": (2, 0), "C3": (3, 0), "D3": (3, 1), "D2": (2, 1), "D1": (1, 1), "D0": (0, 1)}


NARROW_LEVELS = [(2, 0), (3, 0), (3, 1), (2, 1), (1, 1)]              # C_2, C_3, D_3, D_2, D_1: steps 0 .. 4 of k_enc_narrow


def in_degrees(g):
    return np.bincount(np.asarray(g["nbr"], np.int64).reshape(-1), minlength=g["R"])


def code_plan(lv, n):
    """hobbit_graph_finalize's plan: the steps C_0 .. C_{D-1}, D_{D-1} .. D_0 as (level key, in_off, out_off), and cwlen[d], the length of
    the sub-codeword of depth d (cwlen[0]: the codeword)"""
    nd, off, D = [n], [0], 0
    while nd[D] > 13:
        g = lv[(D, 0)]
        assert g["L"] == nd[D]
        off.append(off[D] + nd[D]); nd.append(g["R"]); D += 1
    cwlen = [0] * (D + 1); cwlen[D] = nd[D]
    for d in range(D - 1, -1, -1):
        assert lv[(d, 1)]["L"] == cwlen[d + 1]
        cwlen[d] = nd[d] + cwlen[d + 1] + lv[(d, 1)]["R"]
    plan = [((d, 0), off[d], off[d] + nd[d]) for d in range(D)]
    plan += [((d, 1), off[d + 1], off[d + 1] + cwlen[d + 1]) for d in range(D - 1, -1, -1)]
    return plan, cwlen


def fat_verdict(g, nout, ncons, cap):
    """build_fat_step's decision for one level: (accepted, why, heaviest in-degree per position).  why: "ok", "shape" (more outputs than
    nout x lanes, or an input window over 64 KB) or "cap" (an output with more in-edges than its position has register slots: the outputs
    sorted heaviest first fill position 0 lane by lane, position 1 backwards, position 2 forwards)"""
    lanes = ncons * 64
    if g["R"] > nout * lanes or g["L"] * 16 > 65536:
        return False, "shape", None
    deg = np.sort(in_degrees(g))[::-1]
    top = [int(deg[j * lanes:(j + 1) * lanes].max()) if deg[j * lanes:(j + 1) * lanes].size else 0 for j in range(nout)]
    ok = all(top[j] <= cap[j] for j in range(nout))
    return ok, "ok" if ok else "cap", top


def narrow_verdict(lv, n):
    """build_narrow's decision: (accepted, why).  The code must have the five-step shape between C_1 and D_0 that the kernel was compiled
    for; then per step the outputs sorted heaviest first fill the step's positions, 64 / LPO outputs each, and none may have more in-edges
    than LPO x CAP"""
    plan, _ = code_plan(lv, n)
    S = CTX["NARROW_STEPS"][0]
    if len(plan) != S + 3:
        return False, "shape"
    x2 = plan[2][1]
    for s in range(S):
        key, in_off, out_off = plan[2 + s]
        if (lv[key]["L"], lv[key]["R"], in_off - x2, out_off - x2) != (CTX["NARROW_L"][s], CTX["NARROW_R"][s], CTX["NARROW_IN"][s], CTX["NARROW_OUT"][s]):
            return False, "shape"
    for s in range(S):
        deg = np.sort(in_degrees(lv[plan[2 + s][0]]))[::-1]
        nxt = 0
        for pos in range(CTX["NARROW_POS"][0]):
            if CTX["NARROW_STEP_OF"][pos] != s:
                continue
            lpo, cap = CTX["NARROW_LPO"][pos], CTX["NARROW_CAP"][pos]
            part = deg[nxt:nxt + 64 // lpo]
            if part.size and int(part.max()) > cap * lpo:
                return False, "cap at position %d" % pos
            nxt = min(deg.size, nxt + 64 // lpo)
        if nxt < deg.size:
            return False, "more outputs than positions"
    return True, "ok"


class Forms(dict):
    """expected_forms' result: equal to Hobbit.encode_forms() as a dict; size_class, nsteps and why ride along for expected_chain and the guards"""
    size_class = None; nsteps = 0; why = None


def expected_forms(lv, n):
    """what hobbit_graph_finalize decides for the graphs lv of message length n (and ensure_tiled at the first encode of a long code):
    Hobbit.encode_forms()'s dict after that encode.  .size_class: "single" (codeword <= 80 KB: one k_encode pass), "deep" (<= 160 KB: two
    passes, or the fat / narrow chain in place) or "tiled"; .why: per fat step and for narrow, the reason of the verdict; .top: per fat
    step the heaviest in-degree of each position"""
    plan, cwlen = code_plan(lv, n)
    ln = cwlen[0]
    small = all(not np.asarray(lv[k]["w"])[:, 1].any() and not (np.asarray(lv[k]["w"], np.uint64)[:, 0] >> U(32)).any() for k, _, _ in plan)
    f = Forms(small_weights=small, fatA=False, fatC1=False, fatD=False, narrow=False, tiled_pending=False, tiled_depth=0)
    f.nsteps = len(plan)
    f.size_class = "single" if ln * 16 <= 80 * 1024 else "deep" if ln * 16 <= 160 * 1024 else "tiled"
    f.why, f.top = {}, {}
    if small and len(plan) >= 4 and f.size_class == "deep":
        for name, (key, nout, ncons, cap) in FAT.items():
            f[name], f.why[name], f.top[name] = fat_verdict(lv[key], nout, ncons, cap)
        f["narrow"], f.why["narrow"] = narrow_verdict(lv, n)
    if f.size_class == "tiled":
        d = 0
        while d < len(cwlen) - 1 and cwlen[d] > CTX["TILE_MID_MAX"][0]:
            d += 1
        f["tiled_depth"] = d
    return f


def expected_chain(forms, in_place):
    """the profile names launch_encode / launch_encode_long run under for a code with these forms (csrc/hobbit_kernels.hip)"""
    fw = "" if forms["small_weights"] else "fullw_"
    if forms.size_class == "tiled":
        return {"k_enc_tiled_%sC" % fw, "k_encode_%slong_M" % fw, "k_enc_tiled_%sD" % fw}
    if forms.size_class == "single" or forms.nsteps < 2:
        return {"k_encode" if forms["small_weights"] else "k_encode_fullw"}
    if not forms["small_weights"]:
        return {"k_encode_fullw_A", "k_encode_fullw_B"}
    if not (forms["fatA"] and in_place):
        return {"k_encode_A", "k_encode_B"}
    if not forms["fatD"] or forms.nsteps < 5:
        return {"k_enc_fat_A", "k_encode_B"}
    return {"k_enc_fat_A", "k_enc_fat_C1" if forms["fatC1"] else "k_encode_C1", "k_encode_M2", "k_enc_fat_D"}


def encode_kernel_names():
    """every profile name in launch_encode_long and launch_encode (csrc/hobbit_kernels.hip), read from the source"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd", "csrc", "hobbit_kernels.hip")).read()
    a = src.index("static int launch_encode_long("); b = src.index("int launch_encode(", a); e = src.index("\n}\n", b)
    return set(re.findall(r'"(k_enc[a-zA-Z0-9_]*)"', src[a:e]))


def drawn_graphs(oracle, n, skip=None):
    """the graphs libc draws for message length n straight after rng_reset() -- or after generate_randomness(skip) -- on the oracle"""
    oracle.rng_reset()
    if skip is not None:
        oracle.generate_randomness(skip)
    oracle.expander_init_store(n)
    return graphs_from(oracle, n)


def set_graphs(oracle, lv):
    """the oracle's current graphs (same shapes) replaced by lv's edges"""
    for (dep, kind), g in lv.items():
        oracle.graph_set_edges(dep, kind, g["nbr"], g["w"])


def with_in_degrees(g, deg, seed):
    """g with the same L, R, degree and weights and its neighbours re-dealt: output t gets exactly deg[t] in-edges"""
    deg = np.asarray(deg, np.int64)
    assert deg.shape == (g["R"],) and (deg >= 0).all() and int(deg.sum()) == g["L"] * g["degree"], (deg.shape, int(deg.sum()))
    nbr = np.repeat(np.arange(g["R"], dtype=np.int64), deg)
    np.random.default_rng(seed).shuffle(nbr)
    return dict(g, nbr=nbr)


def heavy_degrees(R, E, k, h, seed, empty=()):
    """in-degrees summing to E: k outputs at h, the outputs in `empty` at 0, the rest as even as possible; which outputs are the heavy ones
    is drawn from seed"""
    free = np.setdiff1d(np.arange(R), np.asarray(empty, np.int64))
    free = free[np.random.default_rng(seed).permutation(free.size)]
    deg = np.zeros(R, np.int64)
    deg[free[:k]] = h
    rest, m = E - k * h, free.size - k
    assert rest >= 0 and m > 0
    deg[free[k:]] = rest // m
    deg[free[k:k + rest % m]] += 1
    return deg


def fitted_degrees(R, E, empty, room, seed):
    """in-degrees summing to E with the outputs in `empty` at 0, fitted to room[r], the register slots of the r-th heaviest output
    (non-increasing): every fed output gets the same share of its slots, so a step whose slots hold E edges at all accepts the graph"""
    free = np.setdiff1d(np.arange(R), np.asarray(empty, np.int64))
    free = free[np.random.default_rng(seed).permutation(free.size)]
    room = np.asarray(room, np.int64)[:free.size]
    assert room.size == free.size and (np.diff(room) <= 0).all() and E < int(room.sum())
    per = E * room // int(room.sum())
    per[:E - int(per.sum())] += 1
    assert (per <= room).all() and int(per.sum()) == E
    deg = np.zeros(R, np.int64); deg[free] = per
    return deg


def fat_room(step):
    """register slots by rank of in-degree for a fat step: cap[0] for the heaviest `lanes` outputs, cap[1] for the next, ..."""
    _, nout, ncons, cap = FAT[step]
    return np.repeat(cap, ncons * 64)


def narrow_room(s):
    """the same for narrow step s: LPO x CAP for the 64 / LPO outputs of each of its positions"""
    return np.concatenate([np.full(64 // CTX["NARROW_LPO"][p], CTX["NARROW_LPO"][p] * CTX["NARROW_CAP"][p])
                           for p in range(CTX["NARROW_POS"][0]) if CTX["NARROW_STEP_OF"][p] == s])


def empty_set(R):
    """outputs 0, R - 1 and every 7th"""
    return np.union1d(np.arange(0, R, 7), [R - 1])


def _hub(nbr, w, degree, i, a, b=None):
    """all edges of input i on output a; with b, the last one on b with weight 0"""
    nbr[i * degree:(i + 1) * degree] = a
    if b is not None:
        nbr[(i + 1) * degree - 1] = b; w[(i + 1) * degree - 1] = 0


def hubs(g, seed):
    """input 0: all edges but one on one output a, the last one with weight 0 on an output b that has no other in-edge (b's only record is
    (index 0, weight 0), what a padding slot looks like); input L - 1 the same on outputs c, d (the largest record offset); input L // 2
    with all its edges on one output e (a multi-edge).  a, c, e are the lightest outputs of g, so that the step keeps its form."""
    L, R, d = g["L"], g["R"], g["degree"]
    nbr = np.array(g["nbr"], np.int64).reshape(-1); w = np.array(g["w"], np.uint64).reshape(-1, 2)
    order = np.argsort(in_degrees(g), kind="stable")
    a, c, e, b, dd = (int(t) for t in order[:5])
    others = order[5:]
    for t in (b, dd):                                   # nobody else feeds b and d
        idx = np.flatnonzero(nbr == t)
        nbr[idx] = others[np.random.default_rng(seed + t).integers(0, others.size, idx.size)]
    _hub(nbr, w, d, 0, a, b); _hub(nbr, w, d, L - 1, c, dd); _hub(nbr, w, d, L // 2, e)
    out = dict(g, nbr=nbr, w=w)
    deg = in_degrees(out)
    assert deg[b] == 1 and deg[dd] == 1
    return out


def bank_clash(g):
    """input i sends all its edges to outputs t with (t // 16) % 16 == i % 16, dealt evenly: every record of such an output reads the bank
    quad i % 16, so the lanes of a 16-lane LDS group that own outputs of one class find no conflict-free slot order"""
    L, R, d = g["L"], g["R"], g["degree"]
    nbr = np.zeros((L, d), np.int64)
    for c in range(16):
        outs = np.flatnonzero((np.arange(R) // 16) % 16 == c); ins = np.arange(c, L, 16)
        E = ins.size * d
        deg = np.full(outs.size, E // outs.size, np.int64); deg[:E % outs.size] += 1
        tg = np.repeat(outs, deg)
        np.random.default_rng(160 + c).shuffle(tg)
        nbr[ins] = tg.reshape(ins.size, d)
    return dict(g, nbr=nbr.reshape(-1))


def tile_split(g, tile):
    """outputs below R / 2 fed only by inputs < tile, the others only by inputs >= tile (every slice of a tiled step has a tile without an
    edge); inputs 0 and tile - 1 with all their edges on one output each of the lower half, tile and L - 1 of the upper half"""
    L, R, d = g["L"], g["R"], g["degree"]
    assert tile < L
    rng = np.random.default_rng(5955)
    nbr = np.empty((L, d), np.int64)
    nbr[:tile] = rng.integers(0, R // 2, (tile, d)); nbr[tile:] = rng.integers(R // 2, R, (L - tile, d))
    nbr[0] = 3; nbr[tile - 1] = R // 2 - 1; nbr[tile] = R // 2; nbr[L - 1] = R - 1
    return dict(g, nbr=nbr.reshape(-1))


def _swap(lv, levels):
    """lv with the levels {key: graph} replaced"""
    out = dict(lv); out.update(levels)
    return out


def _set_weight(g, e, w):
    ww = np.array(g["w"], np.uint64).reshape(-1, 2); ww[e] = w
    return dict(g, w=ww)


# the six caps of the fat steps: family name -> (level, position, outputs at the cap so that the position's heaviest output sits on it)
CAP_CASES = {"C0_pos0": ("C0", "fatA", 0), "C0_pos1": ("C0", "fatA", 1), "C1_pos0": ("C1", "fatC1", 0),
             "D0_pos0": ("D0", "fatD", 0), "D0_pos1": ("D0", "fatD", 1), "D0_pos2": ("D0", "fatD", 2)}


FAMILIES_4096 = ["cap_exact_" + c for c in CAP_CASES] + ["cap_plus_one_" + c for c in CAP_CASES] + [
    "bank_clash", "empty_outputs", "narrow_empty_outputs", "hubs", "zero_weights", "one_big_weight_2^32", "one_big_weight_(1,1)"]       # graph_families(., 4096)


def cap_graph(g, step, pos, over, seed):
    """g's level re-dealt so that position pos of the fat step has its heaviest output exactly at the cap (over = 0) or one above (over = 1):
    pos x lanes + 1 outputs at that in-degree, the rest as even as possible -- or, where the rest would then be heavier than that (D_0's last
    position: its cap is below the mean in-degree), every output from that position on at it and the earlier ones as even as possible"""
    _, nout, ncons, cap = FAT[step]
    R, E, h, before = g["R"], g["L"] * g["degree"], cap[pos] + over, pos * ncons * 64
    if (E - (before + 1) * h) <= h * (R - before - 1):
        deg = heavy_degrees(R, E, before + 1, h, seed)
    else:
        deg = heavy_degrees(R, E, R - before, h, seed)
    assert np.sort(deg)[::-1][before] == h
    return with_in_degrees(g, deg, seed + 1)


def graph_families(lv0, n):
    """{name: (graphs, what the family is meant to select)} for the drawn graphs lv0 of n = 4096 (every family but tile_split) or n = 5955
    (tile_split).  Each family changes the levels it names and keeps the others as drawn.  The second entry: {form: value} that
    expected_forms must give (tests/test_encode_graph_families_cpu.py)."""
    lv0 = {k: dict(g) for k, g in lv0.items()}
    out = {}
    if n == 5955:
        out["tile_split"] = (_swap(lv0, {(0, 0): tile_split(lv0[(0, 0)], CTX["TILE_ELEMS"][0])}), {"tiled_depth": 1, "small_weights": True})
        return out
    assert n == 4096
    asdrawn = {"small_weights": True, "fatA": True, "fatC1": True, "fatD": True, "narrow": True}
    for i, (name, (lvl, step, pos)) in enumerate(CAP_CASES.items()):
        key = LEVEL_NAMES[lvl]
        out["cap_exact_" + name] = (_swap(lv0, {key: cap_graph(lv0[key], step, pos, 0, 100 + 10 * i)}), dict(asdrawn))
        out["cap_plus_one_" + name] = (_swap(lv0, {key: cap_graph(lv0[key], step, pos, 1, 105 + 10 * i)}), dict(asdrawn, **{step: False}))
    out["bank_clash"] = (_swap(lv0, {(0, 0): bank_clash(lv0[(0, 0)])}), dict(asdrawn))
    lv = {}
    for key, g in lv0.items():
        E, empty = g["L"] * g["degree"], empty_set(g["R"])
        fat = [k for k, v in FAT.items() if v[0] == key]
        deg = fitted_degrees(g["R"], E, empty, fat_room(fat[0]), 300) if fat else heavy_degrees(g["R"], E, 0, 0, 300, empty)
        lv[key] = with_in_degrees(g, deg, 301 + key[0] + 10 * key[1])
    out["empty_outputs"] = (lv, dict(asdrawn, narrow=False))       # (C_2's 31 fed outputs cannot hold its 1638 edges in the narrow slots)
    lv = dict(lv0)
    for st, key in enumerate(NARROW_LEVELS):                        # the narrow kernel's own zero outputs: the first and the last of every step
        g = lv0[key]
        lv[key] = with_in_degrees(g, fitted_degrees(g["R"], g["L"] * g["degree"], [0, g["R"] - 1], narrow_room(st), 320 + st), 330 + st)
    out["narrow_empty_outputs"] = (lv, dict(asdrawn))
    out["hubs"] = (_swap(lv0, {LEVEL_NAMES[k]: hubs(lv0[LEVEL_NAMES[k]], 400) for k in ("C0", "C1", "D0")}), dict(asdrawn))
    lv = {}
    for key, g in lv0.items():
        w = np.array(g["w"], np.uint64).reshape(-1, 2); w[0::3] = 0
        lv[key] = dict(g, w=w)
    out["zero_weights"] = (lv, dict(asdrawn))
    c2 = lv0[(2, 0)]
    nofat = {"small_weights": False, "fatA": False, "fatC1": False, "fatD": False, "narrow": False}
    out["one_big_weight_2^32"] = (_swap(lv0, {(2, 0): _set_weight(c2, 777, [1 << 32, 0])}), dict(nofat))
    out["one_big_weight_(1,1)"] = (_swap(lv0, {(2, 0): _set_weight(c2, 778, [1, 1])}), dict(nofat))
    return out


def encode_messages(n, nb, seed):
    """nb messages: the families (all_pm1 first: a batch of one is the worst case of the 96-bit sums, not the zero message), then uniform ones"""
    fam = families(n, seed=seed)
    fam = np.stack([fam["all_pm1"]] + [v for k, v in fam.items() if k != "all_pm1"])
    if nb <= len(fam):
        return np.ascontiguousarray(fam[:nb])
    return np.concatenate([fam, _splitmix((nb - len(fam)) * n, 6000 + seed).reshape(nb - len(fam), n, 2)])


# natural draws: (n, skip) -- the graphs libc draws for n after rng_reset() and generate_randomness(skip) (None: straight after the reset).
# 2977 / 2978 and 5954 / 5955 are the two sides of the LDS size classes; n = 4096 after two draws is a code with the narrow plan refused.
NATURAL = [(2977, None), (2978, None), (3000, None), (3333, None), (3500, None), (4000, None), (4095, None), (4097, None), (5954, None),
           (5955, None), (4096, 2)]
# the same draws with one weight of C_1 set to 2^32: the single-pass and the tiled chain in their general-weight forms
NATURAL_FULLW = [(2977, None, "2^32"), (5955, None, "2^32")]


def natural_graphs(oracle, case):
    lv = drawn_graphs(oracle, case[0], case[1])
    if len(case) > 2:
        lv = _swap(lv, {(1, 0): _set_weight(lv[(1, 0)], 5, [1 << 32, 0])})
    return lv


def natural_guard(forms):
    """forms: {case: expected_forms} over NATURAL.  The list as a whole still holds every kind of case it was chosen for (a libc whose
    draws differ would change which n is which)"""
    have = {"A refused by cap": False, "A refused by shape": False, "C1 refused": False, "a step exactly at a cap": False,
            "narrow refused with the fat steps accepted": False, "single pass": False, "tiled": False, "every fat step refused, two passes": False}
    for f in forms.values():
        have["single pass"] |= f.size_class == "single"
        have["tiled"] |= f.size_class == "tiled"
        if f.size_class != "deep":
            continue
        have["A refused by cap"] |= f.why["fatA"] == "cap"
        have["A refused by shape"] |= f.why["fatA"] == "shape"
        have["C1 refused"] |= f["fatA"] and f["fatD"] and not f["fatC1"]
        have["a step exactly at a cap"] |= any(f[s] and f.top[s][j] == FAT[s][3][j] for s in FAT if f.top[s] for j in range(FAT[s][1]))
        have["narrow refused with the fat steps accepted"] |= f["fatA"] and f["fatC1"] and f["fatD"] and not f["narrow"]
        have["every fat step refused, two passes"] |= not (f["fatA"] or f["fatC1"] or f["fatD"])
    assert all(have.values()), [k for k, v in have.items() if not v]
