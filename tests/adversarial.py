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
