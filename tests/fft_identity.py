"""Exact checks of a transform that is too long for a full CPU reference (tests/test_fft_any_length.py, tests/test_fft_identity_cpu.py).

Two checks, both bit for bit in F_{p^2}:

dit_identity   the decimation-in-time step.  With x the interleave of e and o (x[2j] = e[j], x[2j+1] = o[j]) and X, E, O their transforms,
               X[k] = E[k] + w^k O[k] and X[k + len/2] = E[k] - w^k O[k] for k < len/2, w the primitive len-th root of the direction.  An
               inverse transform carries 1/len, its halves 1/(len/2): the right-hand sides are then halved.  A length is checked against
               the length below it, so a chain of these steps rests on the longest length that a full reference still covers.
sparse_expected  X[k] = sum_j x_j w^(j k mod len) for an input with a few nonzero entries, evaluated at chosen outputs k with the oracle's
               field operations alone (square-and-multiply on the whole (entries x outputs) array of exponents).

dit_identity is written over a backend: an object with fft(a, logn, inverse), mul, add, sub (element-wise, returning new arrays),
const(n, value), interleave(e, o), equal(a, b) and slicing of the arrays it hands out.  NumpyBackend runs it on the CPU with the oracle's
operations and any transform (the CPU test pins the checker with it); the GPU test supplies one over device memory.
"""
import numpy as np

P = (1 << 61) - 1
N_ENTRIES, N_WINDOWS, WINDOW = 48, 16, 64


def f_pow_scalar(orc, w, e):
    """w^e for one element (2,) uint64"""
    acc = np.array([[1, 0]], np.uint64); b = np.asarray(w, np.uint64).reshape(1, 2)
    while e:
        if e & 1:
            acc = orc.f_mul(acc, b)
        b = orc.f_mul(b, b); e >>= 1
    return acc[0]


def direction_root(orc, logn, inverse):
    w = orc.root_of_unity(logn).reshape(1, 2)
    return (orc.f_inv(w) if inverse else w)[0]


def twiddles_by_doubling(B, orc, half, w):
    """tw[k] = w^k, k < half: tw[m:2m] = tw[:m] * w^m.  Element-wise products only; no transform code takes part."""
    tw = B.const(half, np.array([1, 0], np.uint64))
    wm = np.asarray(w, np.uint64).reshape(1, 2)                    # w^m
    m = 1
    while m < half:
        B.assign(tw, m, B.mul(tw[:m], B.const(m, wm[0])))
        wm = orc.f_mul(wm, wm); m *= 2
    return tw


def dit_identity(B, orc, logn, e, o, inverse):
    """(lower half holds, upper half holds) for the transform B.fft at length 2^logn; e, o: 2^(logn-1) elements each (left unchanged)"""
    half = 1 << (logn - 1)
    tw = twiddles_by_doubling(B, orc, half, direction_root(orc, logn, inverse))
    X = B.fft(B.interleave(e, o), logn, inverse)
    E = B.fft(B.copy(e), logn - 1, inverse)
    t = B.mul(tw, B.fft(B.copy(o), logn - 1, inverse))
    del tw
    lo, hi = B.add(E, t), B.sub(E, t)
    del E, t
    if inverse:
        inv2 = B.const(half, np.array([(P + 1) // 2, 0], np.uint64))
        lo, hi = B.mul(lo, inv2), B.mul(hi, inv2)
    return B.equal(X[:half], lo), B.equal(X[half:], hi)


class NumpyBackend:
    """(n, 2) uint64 arrays, the oracle's field operations, `fft(array, inverse) -> array` as the transform under test"""

    def __init__(self, orc, fft):
        self.orc, self._fft = orc, fft

    def fft(self, a, logn, inverse):
        assert a.shape[0] == 1 << logn
        return self._fft(a, inverse)

    def mul(self, a, b): return self.orc.f_mul(a, b)
    def add(self, a, b): return self.orc.f_add(a, b)
    def sub(self, a, b): return self.orc.f_sub(a, b)
    def const(self, n, v): return np.tile(np.asarray(v, np.uint64).reshape(1, 2), (n, 1))
    def copy(self, a): return a.copy()
    def equal(self, a, b): return bool(np.array_equal(a, b))

    def assign(self, dst, at, src):
        dst[at:at + src.shape[0]] = src

    def interleave(self, e, o):
        x = np.empty((2 * e.shape[0], 2), np.uint64); x[0::2] = e; x[1::2] = o
        return x


def sparse_case(logn, seed):
    """positions (sorted, distinct), values (n, 2) and output window starts for the sparse check at length 2^logn"""
    from oracle.pyoracle import splitmix_field
    ln = 1 << logn
    R = max(ln >> 12, 1)
    rnd = splitmix_field(256, 7000 + seed)[:, 0]
    pos = {p for p in (0, 1, 4095, 4096, R - 1, R, ln // 2, ln - 1) if 0 <= p < ln}
    i = 0
    while len(pos) < min(N_ENTRIES, ln):
        pos.add(int(rnd[i]) % ln); i += 1
    pos = np.array(sorted(pos), np.uint64)
    val = splitmix_field(len(pos), 7100 + seed)
    val[len(pos) // 2] = P - 1                                     # one (p-1, p-1)
    top = max(ln - WINDOW, 0)
    clip = lambda s: min(max(int(s), 0), top)
    starts = [0, top, clip(ln // 2 - WINDOW // 2)]
    for m in (1, 3, max(ln // 4096 - 1, 1)):
        starts.append(clip(m * 4096 - WINDOW // 2))                # straddling a multiple of 4096
    for m in (1, 5, 4095):
        starts.append(clip(m * R - WINDOW // 2))                   # straddling a multiple of R
    if logn >= 25:                                                 # the three-factor form's seams: multiples of S = len / 256
        S = ln >> 8
        starts += [clip(S - WINDOW // 2), clip(3 * S - WINDOW // 2), clip(255 * S - WINDOW // 2)]
    while len(starts) < N_WINDOWS:
        starts.append(clip(int(rnd[128 + len(starts)]) % ln))
    return pos, val, starts[:N_WINDOWS]


def sparse_expected(orc, logn, pos, val, starts, inverse):
    """X[k] for k in every window [s, s + WINDOW) (clipped to the length): (len(starts), window, 2) uint64"""
    ln = 1 << logn
    win = min(WINDOW, ln)
    ks = np.concatenate([np.arange(s, s + win, dtype=np.uint64) for s in starts])
    ex = (pos[:, None] * ks[None, :]) % np.uint64(ln)             # j, k < 2^28: the product fits 64 bits
    n, m = ex.shape
    acc = np.tile(np.array([[1, 0]], np.uint64), (n * m, 1))
    one = np.array([1, 0], np.uint64)
    wb = direction_root(orc, logn, inverse).reshape(1, 2)          # w^(2^bit)
    for bit in range(logn):
        sel = ((ex.reshape(-1) >> np.uint64(bit)) & np.uint64(1)).astype(bool)
        acc = orc.f_mul(acc, np.where(sel[:, None], wb, one[None, :]))
        wb = orc.f_mul(wb, wb)
    terms = orc.f_mul(acc, np.repeat(val, m, axis=0)).reshape(n, m, 2)
    out = terms[0]
    for j in range(1, n):
        out = orc.f_add(out, terms[j])
    if inverse:
        inv_len = orc.f_inv(np.array([[ln, 0]], np.uint64))
        out = orc.f_mul(out, np.tile(inv_len, (m, 1)))
    return out.reshape(len(starts), win, 2)
