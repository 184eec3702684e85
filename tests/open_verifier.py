"""The verifier's side of hobbit_open_standard (RS x expander, linear_time = 1) and of hobbit_shockwave_prove, in Python integers: no GPU, no
oracle call.  verify_open / verify_shockwave work on the dicts Hobbit.open_standard / Oracle.open_standard and Hobbit.shockwave_prove /
Oracle.shockwave_prove return, and raise Rejected with the failed relation's name (the names are the constants below).

Not covered here: the Merkle paths (the tree's left|left rule: tests/test_commit_kernels.py), the inside of the WHIR proofs (tests/test_whir_long.py),
the RS x RS and the Elastic openings.

The two ends of an opening and the end of a shockwave proof are evaluations of vectors the verifier would hold through the inner commitments;
the caller computes them (from the aggregate) and passes a function of the points.
"""
import numpy as np

P = (1 << 61) - 1


# ---- F_{p^2} (p = 2^61 - 1, i^2 = -1) in Python integers -----------------------------------------------------------------------------------------
def fi(a):
    return (int(a[0]), int(a[1]))


def fadd(a, b): return ((a[0] + b[0]) % P, (a[1] + b[1]) % P)
def fsub(a, b): return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)
def fmul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


ONE, ZERO = (1, 0), (0, 0)


def ev(q, x):
    """a polynomial's value, coefficients highest degree first (quadratics a, b, c; cubics a, b, c, d)"""
    v = ZERO
    for c in q:
        v = fadd(fmul(v, x), fi(c))
    return v


def claim(q):
    return fadd(ev(q, ZERO), ev(q, ONE))


def eq_at(r, idx):
    """precompute_beta(r)[idx] without the table: r[0] sits on the index's least significant bit"""
    v = ONE
    for j in range(len(r)):
        rj = fi(r[j])
        v = fmul(v, rj if (idx >> j) & 1 else fsub(ONE, rj))
    return v


def eq_points(u, v):
    """eq(u, v) = prod (u_j v_j + (1 - u_j)(1 - v_j))"""
    t = ONE
    for j in range(len(u)):
        uj, vj = fi(u[j]), fi(v[j])
        t = fmul(t, fadd(fmul(uj, vj), fmul(fsub(ONE, uj), fsub(ONE, vj))))
    return t


def powers_mle(s, r):
    """the multilinear extension of (s, s^2, s^3, ...) at r: s * prod ((1 - r_j) + r_j s^(2^j))"""
    v = p = s
    for j in range(len(r)):
        rj = fi(r[j])
        v = fmul(v, fadd(fsub(ONE, rj), fmul(rj, p)))
        p = fmul(p, p)
    return v


def inner(beta, row):
    t = ZERO
    for b, v in zip(beta, row):
        t = fadd(t, fmul(b, fi(v)))
    return t


# ---- rejection ------------------------------------------------------------------------------------------------------------------------------------
class Rejected(AssertionError):
    """one failed relation; .relation is its name, .what says where"""

    def __init__(self, relation, what=""):
        AssertionError.__init__(self, "%s: %s" % (what, relation) if what else relation)
        self.relation = relation
        self.what = what


def need(cond, relation, what=""):
    if not cond:
        raise Rejected(relation, what)


ROUNDS = "rounds"                   # q_i(0) + q_i(1) = q_{i-1}(r_{i-1}); q_last(r_last) = the product of the final values
P1_CLAIM = "p1_claim"               # P1's claimed sum is 0
P2_CLAIM = "p2_claim"               # P2's claim = P1.vr[1]
P2_POWERS = "p2_powers"             # P2.vr[0] = the multilinear extension of s0, s0^2, ... at P2's challenges
QUERY_RANGE = "query_range"         # every col < cols and every row < 2 trs (part of relation 5: no position outside the tensor)
P3_CLAIM = "p3_claim"               # P3's claim = sum over the distinct positions of w_p <eq(x[:log2 K]), reply[q_p]>
P3_WEIGHTS = "p3_weights"           # P3.vr[1] = sum_p w_p eq(P3.r)[p]
P4_CLAIM = "p4_claim"               # P4's claim = a P3.vr[0] + P2.vr[1]
P4_EQ = "p4_eq"                     # P4.vr[0] = eq(P2.r | P1.r, P4.r) + a eq(P3.r, P4.r)
P5_CLAIM = "p5_claim"               # P5's claim = y1
P4_END = "p4_end"                   # P4.vr[1] = (1 - rho) y1 + rho C~(P4.r[:-1]), rho = P4.r[-1]
P5_END = "p5_end"                   # P5.vr[1] = (1 - P5.r[-1]) aggr~(P5.r[:-1] | P4.r[logc : R3 - 1])
SP_P1_CLAIM = "sp_p1_claim"         # shockwave P1's claim = sum over the distinct columns of <eq(x[-log2 k:]), reply[i]>
SP_P1_WEIGHTS = "sp_p1_weights"     # vr1[1] = sum over the distinct columns of eq(r1)[I[i]]
SP_P2_CLAIM = "sp_p2_claim"         # shockwave P2's claim = vr1[0]
SP_P2_END = "sp_p2_end"             # vr2[1] = (1 - popped) row~(r2)
SP_WHIR = "sp_whir"                 # iters > 0: wchecks == [1, 1]


def check_rounds(poly, r, vr, what):
    """the verifier's round test of one sumcheck: q_i(0) + q_i(1) = q_{i-1}(r_{i-1}), and q_last(r_last) = the product of the final values"""
    poly = np.asarray(poly); r = np.asarray(r)
    need(len(poly) == len(r) and len(poly) >= 1, ROUNDS, what)
    for i in range(1, len(poly)):
        need(claim(poly[i]) == ev(poly[i - 1], fi(r[i - 1])), ROUNDS, "%s: round %d" % (what, i))
    prod = ONE
    for v in np.asarray(vr).reshape(-1, 2):
        prod = fmul(prod, fi(v))
    need(ev(poly[-1], fi(r[-1])) == prod, ROUNDS, what + ": final values")
    return claim(poly[0])


# ---- hobbit_open_standard -----------------------------------------------------------------------------------------------------------------------------
def open_shape(logN, K, trs):
    """cols, R1, logc, R3 and where P1 .. P5 begin in poly / r"""
    cols = 2 * ((1 << logN) // K) // trs
    R1 = (2 * trs).bit_length() - 1; logc = cols.bit_length() - 1; R3 = R1 + logc
    off = [0]
    for n in (R1, logc, R3, R3, logc):
        off.append(off[-1] + n)
    return cols, R1, logc, R3, off


def last_writes(I, cols):
    """position col + cols * row -> the last query there: the prover's buff2[I[q]] = pw, where the last write wins"""
    pos = {}
    for q in range(len(I)):
        pos[int(I[q][0]) + cols * int(I[q][1])] = q
    return pos


def open_points(o, x, K, trs):
    """the points of the two ends and of the two shockwave proofs: (P4.r[:-1], P5.r[:-1] | P4.r[logc : R3 - 1], sp_f's point)"""
    cols, R1, logc, R3, off = open_shape(len(x), K, trs)
    r4, r5 = o["r"][off[3]:off[4]], o["r"][off[4]:off[5]]
    pa = np.concatenate([r5[:-1], r4[logc:R3 - 1]])
    return np.ascontiguousarray(r4[:-1]), np.ascontiguousarray(pa), np.ascontiguousarray(np.concatenate([r5, r4[logc:R3 - 1]])[:-1])


def verify_open(o, x, K, trs, ends):
    """o: the opening; x: the point (log2 N elements); ends(pc, pa) -> (C~(pc), aggr~(pa)) as pairs of integers, C the parity half of the
    aggregate's tensor code (trs * cols entries, row-major).  Returns the five claimed sums."""
    cols, R1, logc, R3, off = open_shape(len(x), K, trs)
    logK = K.bit_length() - 1
    need(len(o["poly"]) == off[5] and len(o["r"]) == off[5], ROUNDS, "open: number of rounds")
    S = [dict(poly=o["poly"][off[i]:off[i + 1]], r=o["r"][off[i]:off[i + 1]], vr=[fi(v) for v in o["vr"][i]]) for i in range(5)]
    cl = [check_rounds(s["poly"], s["r"], o["vr"][i], "P%d" % (i + 1)) for i, s in enumerate(S)]
    rv0, s0, s2, a, y1 = [fi(v) for v in o["scalars"]]
    need(cl[0] == ZERO, P1_CLAIM)
    need(cl[1] == S[0]["vr"][1], P2_CLAIM)
    need(S[1]["vr"][0] == powers_mle(s0, S[1]["r"]), P2_POWERS)
    I = o["I"]
    for q in range(len(I)):
        need(int(I[q][0]) < cols and int(I[q][1]) < 2 * trs, QUERY_RANGE, "query %d" % q)
    pw, w = ONE, []
    for q in range(len(I)):
        pw = fmul(pw, s2); w.append(pw)                          # w_p = s2^(q_p + 1)
    beta = [eq_at(x[:logK], i) for i in range(K)]
    total = weights = ZERO
    for p, q in last_writes(I, cols).items():
        total = fadd(total, fmul(w[q], inner(beta, o["reply"][q])))
        weights = fadd(weights, fmul(w[q], eq_at(S[2]["r"], p)))
    need(cl[2] == total, P3_CLAIM)
    need(S[2]["vr"][1] == weights, P3_WEIGHTS)
    need(cl[3] == fadd(fmul(a, S[2]["vr"][0]), S[1]["vr"][1]), P4_CLAIM)
    r4, r5 = S[3]["r"], S[4]["r"]
    need(S[3]["vr"][0] == fadd(eq_points(np.concatenate([S[1]["r"], S[0]["r"]]), r4), fmul(a, eq_points(S[2]["r"], r4))), P4_EQ)
    need(cl[4] == y1, P5_CLAIM)
    pc, pa, _ = open_points(o, x, K, trs)
    Cv, Av = ends(pc, pa)
    rho = fi(r4[-1])
    need(S[3]["vr"][1] == fadd(fmul(fsub(ONE, rho), y1), fmul(rho, Cv)), P4_END)
    need(S[4]["vr"][1] == fmul(fsub(ONE, fi(r5[-1])), Av), P5_END)       # 1 - P5.r[-1]: prove_fft_matrix's zero padding
    return cl


def matrix_end(evaluate, x, k):
    """the end of a shockwave proof at x of a matrix of k rows, row-major: row~(r2) = matrix~(r2 | x[-log2 k:]), the row index being the high part
    of the flat index.  evaluate(point) -> matrix~(point) is the caller's (the oracle's or the device's evaluate_vector of that matrix)"""
    lk = k.bit_length() - 1
    xk = np.asarray(x)[len(x) - lk:]
    return lambda r2: fi(evaluate(np.ascontiguousarray(np.concatenate([r2, xk]))))


# ---- hobbit_shockwave_prove ---------------------------------------------------------------------------------------------------------------------------
def full_r2(sp):
    """prove_fft's last challenge is popped from r2 but still lies in the buffer behind the trimmed view"""
    r2 = sp["r2"]
    full = r2.base if r2.base is not None and len(r2.base) == len(sp["q2"]) else r2
    need(len(full) == len(sp["q2"]), ROUNDS, "the popped challenge is not behind the view")
    return full


def last_columns(I):
    """column -> the last query there"""
    return {int(c): i for i, c in enumerate(I)}


def verify_shockwave(sp, x, k, end, what="shockwave"):
    """sp: one shockwave proof of a (k, W / 2) matrix at x; end(r2) -> row~(r2) as a pair of integers, row = sum_j eq(x[-log2 k:])[j] matrix[j].
    Returns the claimed sums of P1 and P2."""
    lk = k.bit_length() - 1
    c1 = check_rounds(sp["q1"], sp["r1"], sp["vr1"], what + " P1")
    r2 = full_r2(sp)
    c2 = check_rounds(sp["q2"], r2, sp["vr2"], what + " P2")
    xk = x[len(x) - lk:]
    beta = [eq_at(xk, j) for j in range(k)]
    total = weights = ZERO
    for c, i in last_columns(sp["I"]).items():
        need(c < (1 << len(sp["r1"])), QUERY_RANGE, "%s: query %d" % (what, i))
        total = fadd(total, inner(beta, sp["reply"][i]))
        weights = fadd(weights, eq_at(sp["r1"], c))
    need(c1 == total, SP_P1_CLAIM, what)
    need(fi(sp["vr1"][1]) == weights, SP_P1_WEIGHTS, what)
    need(c2 == fi(sp["vr1"][0]), SP_P2_CLAIM, what)
    need(fi(sp["vr2"][1]) == fmul(fsub(ONE, fi(r2[-1])), end(np.ascontiguousarray(r2[:-1]))), SP_P2_END, what)
    if int(sp["iters"][0]):
        need(np.asarray(sp["wchecks"]).tolist() == [1, 1], SP_WHIR, what)
    return c1, c2
