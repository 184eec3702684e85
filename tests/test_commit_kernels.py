"""The kernels every commitment is made of, each at every launch form it has: the two BLAKE3 compressions, the tree (k_merkle_top / _sub /
_level, both parent rules, 1 .. 2^23 leaves), the sibling gather, the leaf chain through its three entry points (hobbit_leaf_chain,
hobbit_inner_digests + hobbit_chain_digests, hobbit_leaf_chain_relay over ragged slot ranges and in two hops), the Elastic_PC streaming
leaves in both argument orders, the inner commitments (shockwave_commit, change_form, whir_commit), whole commits below one workgroup,
and hobbit_aggregate on either side of its 64-coefficient slices.

Everything goes through the C ABI and is compared bit for bit, every output byte, with the plain host references of tests/commit_refs.py
(anchored to the oracle by tests/test_commit_refs_cpu.py) or with the oracle itself.  Every output buffer has a sentinel-filled slot
behind it that must come back untouched -- for a levels buffer that is the 2n-th hash slot.

On an MI355X the file's 173 cases take 7.8 s; the slowest three are test_merkle_levels_every_depth[23-1] (0.98 s: a 512 MiB levels buffer
against the host tree over 2^23 leaves), test_merkle_levels_every_depth[23-0] (0.82 s) and test_leaf_chain_entry_point[2097152-4-1]
(0.64 s: a 128 MiB tensor, two passes of the capped grid)."""
import ctypes
import numpy as np
import pytest
import commit_refs as cr
from adversarial import graphs_from
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
SENT = 0xA5
c_vp = ctypes.c_void_p


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    mod = load_package()
    h = mod.Hobbit(0)          # raises if the HIP library or the GPU is missing: no fallback
    h.lib.hobbit_verify_path_host.restype = ctypes.c_int
    h.lib.hobbit_elastic_free.restype = None
    h.cache = {}               # the last reference a family of cases shares (one entry per family)
    yield h
    h.cache.clear()
    h.close()


def vp(a):
    return a.ctypes.data_as(c_vp)


def rand_bytes(n, seed):
    return np.frombuffer(np.random.default_rng(seed).bytes(n), np.uint8)


class Guarded:
    """nbytes of device memory with a 64-byte sentinel slot behind them; the whole buffer starts as the sentinel unless `data` is given"""

    def __init__(self, hb, nbytes, data=None):
        self.hb, self.n = hb, int(nbytes)
        self.buf = hb.alloc(self.n + 64)
        self.ptr = self.buf.ptr
        hb._chk(hb.lib.hobbit_memset(hb.ctx, self.ptr, SENT, self.n + 64))
        if data is not None:
            data = np.ascontiguousarray(data)
            assert data.nbytes <= self.n
            if data.nbytes:
                hb._chk(hb.lib.hobbit_memcpy_h2d(hb.ctx, self.ptr, vp(data), data.nbytes))

    def zero(self):
        self.hb._chk(self.hb.lib.hobbit_memset(self.hb.ctx, self.ptr, 0, self.n))
        return self

    def host(self, shape, dtype=np.uint8, offset=0):
        return self.hb.to_host(self.buf, shape, dtype, offset)

    def intact(self, frm=None):
        """the bytes from `frm` (default: the end of the payload) to the end of the sentinel slot are still the sentinel"""
        frm = self.n if frm is None else int(frm)
        return bool((self.host((self.n + 64 - frm,), np.uint8, frm) == SENT).all())


def levels_of(hb, leaves, quirk):
    """hobbit_merkle_levels on a guarded buffer of 2n slots: (the 2n - 1 nodes, the buffer)"""
    n = leaves.shape[0]
    g = Guarded(hb, 64 * n, leaves)
    hb._chk(hb.lib.hobbit_merkle_levels(hb.ctx, g.ptr, n, quirk))
    assert g.intact(32 * (2 * n - 1)), "the 2n-th slot of the levels buffer was written"
    return g.host((2 * n - 1, 32)), g


# ---- a. flat hashes ------------------------------------------------------------------------------------------------------------------
# grid_for caps the grid at 4096 workgroups of 256: one thread, under a wave, over a workgroup, the last size in one pass and the first
# with a ragged second pass
FLAT_SIZES = [1, 63, 257, 1 << 20, (1 << 20) + 333]


def flat_inputs(n, width, seed):
    """random bytes with one all-zero and one all-0xFF block (H(0^64) is the constant k_leaf_chain substitutes for zero groups); for n = 1
    the three one after the other"""
    x = rand_bytes(n * width, seed).reshape(n, width).copy()
    if n >= 3:
        x[n // 2] = 0; x[n - 1] = 0xFF
        return [x]
    return [x, np.zeros_like(x), np.full_like(x, 0xFF)]


@pytest.mark.parametrize("n", FLAT_SIZES)
def test_blake3_64_every_size(hb, oracle, n):
    for x in flat_inputs(n, 64, n):
        d = hb.to_device(x); o = Guarded(hb, 32 * n)
        hb._chk(hb.lib.hobbit_blake3_64(hb.ctx, d.ptr, o.ptr, n))
        assert np.array_equal(o.host((n, 32)), oracle.blake3_64(x))
        assert o.intact()


@pytest.mark.parametrize("n", FLAT_SIZES)
def test_hash_md_every_size_out_of_place_and_in_place(hb, oracle, n):
    for x, prev in zip(flat_inputs(n, 64, 2 * n), flat_inputs(n, 32, 2 * n + 1)):
        want = oracle.hash_md(x.view(np.uint64).reshape(n, 4, 2), prev)
        d = hb.to_device(x); p = Guarded(hb, 32 * n, prev); o = Guarded(hb, 32 * n)
        hb._chk(hb.lib.hobbit_hash_md(hb.ctx, d.ptr, p.ptr, o.ptr, n))
        assert np.array_equal(o.host((n, 32)), want)
        assert np.array_equal(p.host((n, 32)), prev), "out of place: prev changed"
        assert o.intact() and p.intact()
        hb._chk(hb.lib.hobbit_hash_md(hb.ctx, d.ptr, p.ptr, p.ptr, n))          # in place, as the wrapper and the streaming commits call it
        assert np.array_equal(p.host((n, 32)), want)
        assert p.intact()


# ---- b. the tree: d = 0 writes nothing, d <= 11 k_merkle_top alone, 12 .. 22 k_merkle_sub with g = d - 11 then top, 23 one plain level in
# four passes of the capped grid, then sub with g = 11, then top ------------------------------------------------------------------------
def tree_leaves(hb, d):
    if hb.cache.get("tree_d") != d:
        hb.cache["tree_d"], hb.cache["tree_leaves"] = d, rand_bytes(32 << d, 100 + d).reshape(-1, 32)
    return hb.cache["tree_leaves"]


@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("d", range(24))
def test_merkle_levels_every_depth(hb, d, quirk):
    leaves = tree_leaves(hb, d)
    got, _ = levels_of(hb, leaves, quirk)
    assert np.array_equal(got[:1 << d], leaves), "level 0 changed"
    assert np.array_equal(got, cr.tree(leaves, quirk))


# ---- c. MT_commit_Blake --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [0, 1, 5, 11, 12, 13])
def test_mt_commit_blake_sizes(hb, oracle, d):
    n = 1 << d
    x = splitmix_field(4 * n, 300 + d)
    dx = hb.to_device(x); lv = Guarded(hb, 64 * n)
    hb._chk(hb.lib.hobbit_mt_commit_blake(hb.ctx, dx.ptr, 4 * n, lv.ptr))
    assert np.array_equal(lv.host((2 * n - 1, 32)), oracle.mt_commit_blake(x))
    assert lv.intact(32 * (2 * n - 1))


# ---- d. sibling paths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("n", [2, 4, 1 << 11, 1 << 13])
def test_merkle_paths_small_and_large_trees(hb, n, quirk):
    depth = n.bit_length() - 1
    leaves = rand_bytes(32 * n, 400 + n).reshape(n, 32)
    levels, g = levels_of(hb, leaves, quirk)
    assert np.array_equal(levels, cr.tree(leaves, quirk))
    rng = np.random.default_rng(n + quirk)
    for nq in (1, 7, 257):                                            # nq * depth is never a multiple of the 256-thread workgroup
        pos = rng.integers(0, n, nq).astype(np.uint64)
        pos[0] = n - 1
        if nq >= 7:
            pos[1] = 0; pos[2] = n - 1; pos[3] = pos[4] = pos[5]      # both ends and duplicates
        out = np.full((nq * depth * 32 + 64,), SENT, np.uint8)
        hb._chk(hb.lib.hobbit_merkle_paths(hb.ctx, g.ptr, n, vp(pos), nq, vp(out)))
        assert (out[nq * depth * 32:] == SENT).all()
        P = out[:nq * depth * 32].reshape(nq, depth, 32)
        assert np.array_equal(P, cr.paths(levels, n, pos)), nq
        if not quirk:                                                 # every path of a conventional tree walks to the root
            root = np.ascontiguousarray(levels[-1])
            for q in range(nq):
                p = int(pos[q])
                assert hb.lib.hobbit_verify_path_host(vp(np.ascontiguousarray(leaves[p])), p, vp(np.ascontiguousarray(P[q])), depth, vp(root), 0) == 1, (nq, q)
    for p in (0, n // 2, n - 1):
        out = np.full((depth * 32 + 64,), SENT, np.uint8)
        hb._chk(hb.lib.hobbit_merkle_path(hb.ctx, g.ptr, n, p, vp(out)))
        assert (out[depth * 32:] == SENT).all()
        assert np.array_equal(out[:depth * 32].reshape(1, depth, 32), cr.paths(levels, n, [p])), p


# ---- e. the leaf chain, three ways ---------------------------------------------------------------------------------------------------
# (M, trs, K).  The kernels run M / 256 workgroups on a grid capped at 4096 and rotate the block order inside runs of 8 only when the block
# count is a multiple of 8: under one block, 4 blocks (off), 8 (on), 9 (off), 2 columns of 2048 leaves, 32 blocks over 5 chunks, and 8192
# blocks = two passes of the capped grid
CHAIN_SHAPES = [(4, 4, 1), (64, 4, 3), (256, 64, 2), (1024, 4, 2), (2048, 4, 2), (2304, 4, 1), (4096, 4096, 2), (1 << 13, 4, 5), (1 << 21, 4, 1)]


class ChainCase:
    """a hobbit_fill_splitmix buffer read as a codeword-major tensor (K, cols, 2 trs), and its leaves on the host"""

    def __init__(self, hb, M, trs, K, T=None, lin=0, clean=None):
        self.hb, self.M, self.trs, self.K, self.lin = hb, M, trs, K, lin
        self.cols, self.half = 2 * M // trs, trs // 2
        if T is None:
            self.dev = hb.fill_splitmix(K * 4 * M, 900 + M + trs + K)
            self.T = hb.to_host(self.dev, (K, self.cols, 2 * trs, 2), np.uint64)
        else:
            self.T, self.dev = T, hb.to_device(T)
        self.clean = self.T if clean is None else clean               # what the leaves are the leaves of
        self.want = cr.leaf_chain(self.clean)
        self._dig = None

    @property
    def dig(self):
        if self._dig is None:
            self._dig = cr.inner_digests(self.clean)
        return self._dig

    def chunk_ptr(self, i):
        return self.dev.ptr + 64 * self.M * i

    def chain(self, i0, k, leaves):
        self.hb._chk(self.hb.lib.hobbit_leaf_chain(self.hb.ctx, self.chunk_ptr(i0), self.M, k, self.trs, self.lin, leaves.ptr))

    def relay(self, i0, k, b, cnt, s_in, s_out, leaves):
        self.hb._chk(self.hb.lib.hobbit_leaf_chain_relay(self.hb.ctx, self.chunk_ptr(i0), self.M, k, self.trs, self.lin, b, cnt, s_in, s_out, leaves))


def chain_case(hb, shape):
    if hb.cache.get("chain_shape") != shape:
        hb.cache["chain"] = None
        hb.cache["chain_shape"], hb.cache["chain"] = shape, ChainCase(hb, *shape)
    return hb.cache["chain"]


def check_leaf_chain(hb, c):
    """hobbit_leaf_chain continues from what d_leaves holds: from zeros, and from a given state with the chunks split over two calls"""
    M, K = c.M, c.K
    lv = Guarded(hb, 32 * M).zero()
    c.chain(0, K, lv)
    assert np.array_equal(lv.host((M, 32)), c.want), "zero start"
    assert lv.intact()
    s0 = rand_bytes(32 * M, 7 + M).reshape(M, 32)
    lv = Guarded(hb, 32 * M, s0)
    k1 = K // 2
    if k1:
        c.chain(0, k1, lv)
    c.chain(k1, K - k1, lv)
    assert np.array_equal(lv.host((M, 32)), cr.chain_digests(c.dig, s0)), "given start, two calls"        # (= leaf_chain(T, s0): the CPU file)
    assert lv.intact()


def check_digest_chain(hb, c, dev_ptr=None):
    """hobbit_inner_digests of all chunks (of c's buffer, or of the device copy of c.clean at dev_ptr), then hobbit_chain_digests onto
    zeroed leaves"""
    M, K = c.M, c.K
    dg = Guarded(hb, 32 * M * K)
    hb._chk(hb.lib.hobbit_inner_digests(hb.ctx, dev_ptr or c.dev.ptr, M, K, c.trs, dg.ptr))
    assert np.array_equal(dg.host((K, M, 32)), c.dig)
    assert dg.intact()
    lv = Guarded(hb, 32 * M).zero()
    hb._chk(hb.lib.hobbit_chain_digests(hb.ctx, dg.ptr, 32 * M, K, M, lv.ptr))
    assert np.array_equal(lv.host((M, 32)), c.want)
    assert lv.intact()


def ragged_ranges(M):
    cuts = sorted({0, 1, min(300, M - 1), M - 1, M})
    return [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]


def check_relay(hb, c):
    """slot ranges: [0, M) cut into ragged ranges with state_out and d_leaves given together, the leaves outside a range untouched; one
    whole range; and the K chunks in two hops, the first hop's state_out being the second's state_in"""
    M, K = c.M, c.K
    slots = cr.slot_order(c.want, c.cols, c.half)
    slot_of_leaf = (np.arange(M) % c.cols) * c.half + np.arange(M) // c.cols
    lv = Guarded(hb, 32 * M)
    expect = np.full((M, 32), SENT, np.uint8)
    ranges = ragged_ranges(M)
    for r, (b, cnt) in enumerate(ranges):
        so = Guarded(hb, 32 * cnt)
        c.relay(0, K, b, cnt, None, so.ptr, lv.ptr)
        assert np.array_equal(so.host((cnt, 32)), slots[b:b + cnt]), "state_out of [%d, %d)" % (b, b + cnt)
        assert so.intact()
        inside = (slot_of_leaf >= b) & (slot_of_leaf < b + cnt)
        expect[inside] = c.want[inside]
        if M <= 1 << 13 or r in (0, len(ranges) - 1):
            assert np.array_equal(lv.host((M, 32)), expect), "leaves after [%d, %d): slots outside the ranges so far must be untouched" % (b, b + cnt)
    assert lv.intact()
    lv = Guarded(hb, 32 * M)
    c.relay(0, K, 0, M, None, None, lv.ptr)
    assert np.array_equal(lv.host((M, 32)), c.want), "one whole range"
    assert lv.intact()
    if K > 1:
        k1 = K // 2
        s1 = Guarded(hb, 32 * M)
        c.relay(0, k1, 0, M, None, s1.ptr, None)
        assert np.array_equal(s1.host((M, 32)), cr.slot_order(cr.leaf_chain(c.clean[:k1]), c.cols, c.half)), "first hop's state_out"
        assert s1.intact()
        lv = Guarded(hb, 32 * M)
        c.relay(k1, K - k1, 0, M, s1.ptr, None, lv.ptr)
        assert np.array_equal(lv.host((M, 32)), c.want), "second hop's leaves"
        assert lv.intact()
        b, cnt = ranges[1] if len(ranges) > 1 else ranges[0]          # and a ragged range handed over
        so = Guarded(hb, 32 * cnt)
        c.relay(k1, K - k1, b, cnt, s1.ptr + 32 * b, so.ptr, None)
        assert np.array_equal(so.host((cnt, 32)), slots[b:b + cnt]), "second hop over a ragged range"
        assert so.intact()


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_leaf_chain_entry_point(hb, shape):
    check_leaf_chain(hb, chain_case(hb, shape))


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_inner_and_chain_digests(hb, shape):
    check_digest_chain(hb, chain_case(hb, shape))


@pytest.mark.parametrize("shape", CHAIN_SHAPES, ids=lambda s: "%d-%d-%d" % s)
def test_leaf_chain_relay_ranges_and_hops(hb, shape):
    check_relay(hb, chain_case(hb, shape))


@pytest.mark.parametrize("M,trs,K", [(1 << 10, 64, 2), (1 << 13, 4096, 2)])
def test_leaf_chain_linear_time_rows_past_the_codeword_are_not_read(hb, oracle, M, trs, K):
    """linear_time = 1: with len the codeword length and rv = (len + 3) & ~3, rows [len, rv) are zero and rows >= rv hold garbage.
    hobbit_leaf_chain and hobbit_leaf_chain_relay take linear_time and must give the leaves of the same buffer with those rows zero (the
    kernels' "not read" claim and the rounding of zero_from).  hobbit_inner_digests has no linear_time argument and reads every row it is
    given (hobbit_tensorcode_chunks writes those rows as zeros): it gets the buffer with the rows zero and must arrive at the same leaves."""
    oracle.rng_reset(); oracle.expander_init_store(trs)
    ln = hb.upload_graphs(trs, graphs_from(oracle, trs))
    rv = (ln + 3) & ~3
    assert trs < ln <= rv < 2 * trs
    cols = 2 * M // trs
    T = splitmix_field(K * 4 * M, 55 + trs).reshape(K, cols, 2 * trs, 2)
    T[:, :, ln:rv] = 0
    clean = T.copy(); clean[:, :, ln:] = 0
    assert T[:, :, rv:].any()
    c = ChainCase(hb, M, trs, K, T=T, lin=1, clean=clean)
    assert not np.array_equal(cr.leaf_chain(T), c.want)              # the garbage would show
    check_leaf_chain(hb, c)
    check_relay(hb, c)
    dclean = hb.to_device(clean)
    check_digest_chain(hb, c, dev_ptr=dclean.ptr)


# ---- f. Elastic_PC streaming leaves --------------------------------------------------------------------------------------------------
def elastic_case(hb, oracle, B, trs):
    """twelve distinct chunks, one of them all-zero, on the device, and their tensor codes from the oracle"""
    if hb.cache.get("elastic_shape") != (B, trs):
        chunks = [splitmix_field(B, 1200 + B + i) for i in range(12)]
        chunks[5] = np.zeros_like(chunks[5])
        tensors = [oracle.compute_tensorcode(c, trs, 0) for c in chunks]
        assert not tensors[5].any()
        hb.cache["elastic_shape"], hb.cache["elastic"] = (B, trs), ([hb.to_device(c) for c in chunks], tensors)
    return hb.cache["elastic"]


@pytest.mark.parametrize("order", [1, 0])
@pytest.mark.parametrize("B,trs", [(64, 4), (1 << 12, 64), (1 << 13, 4)])
def test_elastic_streaming_leaves(hb, oracle, B, trs, order):
    """hobbit_elastic_begin / push / finish with 4, 8 and 12 chunks in both argument orders (gcc_arg_order = 0 is shift == 0 in
    k_elastic_leaf / k_elastic_inner); finish after 6 pushes equals finish after 4; hobbit_elastic_push_inner per group followed by
    hobbit_chain_digests onto zeroed leaves gives the same level 0"""
    dev, tensors = elastic_case(hb, oracle, B, trs)
    lib, n = hb.lib, 4 * B
    want = {k: cr.elastic_leaves(tensors[:k], order) for k in (4, 8, 12)}
    assert np.array_equal(cr.elastic_leaves(tensors[:6], order), want[4])
    e = c_vp()
    hb._chk(lib.hobbit_elastic_begin(hb.ctx, B, trs, 0, order, ctypes.byref(e)))
    try:
        pushed = 0
        for upto in (4, 6, 8, 12):
            while pushed < upto:
                hb._chk(lib.hobbit_elastic_push(hb.ctx, e, dev[pushed].ptr)); pushed += 1
            lv = Guarded(hb, 64 * n)
            hb._chk(lib.hobbit_elastic_finish(hb.ctx, e, lv.ptr))
            assert np.array_equal(lv.host((2 * n - 1, 32)), cr.tree(want[upto - upto % 4], 1)), "finish after %d pushes" % upto
            assert lv.intact(32 * (2 * n - 1))
    finally:
        lib.hobbit_elastic_free(e)
    e = c_vp()
    hb._chk(lib.hobbit_elastic_begin(hb.ctx, B, trs, 0, order, ctypes.byref(e)))
    try:
        dg = Guarded(hb, 3 * 32 * n)
        for i in range(12):
            hb._chk(lib.hobbit_elastic_push_inner(hb.ctx, e, dev[i].ptr, dg.ptr + (i // 4) * 32 * n))
        lv = Guarded(hb, 32 * n).zero()
        hb._chk(lib.hobbit_chain_digests(hb.ctx, dg.ptr, 32 * n, 3, n, lv.ptr))
        assert np.array_equal(lv.host((n, 32)), want[12]), "push_inner + chain_digests"
        assert lv.intact() and dg.intact()
    finally:
        lib.hobbit_elastic_free(e)


# ---- g. inner commitments ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [2, 64, 4096])
@pytest.mark.parametrize("k", [4, 8, 16, 32, 64])
def test_shockwave_commit_shapes(hb, oracle, k, w):
    N, W = k * w, 2 * w
    poly = splitmix_field(N, 1500 + k + w)
    want_enc, want_lv = oracle.shockwave_commit(poly, k)
    d = hb.to_device(poly); enc = Guarded(hb, 16 * k * W); lv = Guarded(hb, 64 * W)
    hb._chk(hb.lib.hobbit_shockwave_commit(hb.ctx, d.ptr, N, k, enc.ptr, lv.ptr))
    assert np.array_equal(enc.host((k, W, 2), np.uint64), want_enc)
    assert np.array_equal(lv.host((2 * W - 1, 32)), want_lv)
    assert enc.intact() and lv.intact(32 * (2 * W - 1))


@pytest.mark.parametrize("logn", list(range(1, 17)) + [22])
def test_change_form_every_size(hb, oracle, logn):
    """blocks of more than 4096 elements go through k_change_form_level, the rest through k_change_form_tail in LDS (logn 12 | 13); the level
    kernel's capped grid takes a second pass from logn = 22"""
    n = 1 << logn
    poly = splitmix_field(n, 1600 + logn)
    d = Guarded(hb, 16 * n, poly)
    hb._chk(hb.lib.hobbit_change_form(hb.ctx, d.ptr, logn))
    assert np.array_equal(d.host((n, 2), np.uint64), oracle.change_form(poly))
    assert d.intact()


@pytest.mark.parametrize("logN", range(4, 15))
def test_whir_commit_every_size(hb, oracle, logN):
    """the 16-way regroup transposes 16 rows by 2 .. 2048 columns: every edge tile of k_transpose"""
    N = 1 << logN
    poly = splitmix_field(N, 1700 + logN)
    want_com, want_lv = oracle.whir_commit(poly)
    d = hb.to_device(poly); com = Guarded(hb, 32 * N); lv = Guarded(hb, 32 * N)
    hb._chk(hb.lib.hobbit_whir_commit(hb.ctx, d.ptr, N, com.ptr, lv.ptr))
    assert np.array_equal(com.host((2 * N, 2), np.uint64), want_com)
    assert np.array_equal(lv.host((N - 1, 32)), want_lv)
    assert com.intact() and lv.intact(32 * (N - 1))
    assert np.array_equal(hb.to_host(d, (N, 2), np.uint64), poly), "d_poly changed"


# ---- h. whole commits below the tested sizes: the commit's own k_leaf_chain<1> at under one block, rotation off and rotation on ------
@pytest.mark.parametrize("N,K,trs,lin", [(16, 1, 4, 0), (3 << 8, 3, 4, 0), (1 << 10, 4, 16, 0), (1 << 13, 2, 4096, 1), (5 << 11, 5, 64, 1)])
def test_commit_standard_small_shapes(hb, oracle, N, K, trs, lin):
    if lin:
        oracle.rng_reset(); oracle.expander_init_store(trs)
        hb.upload_graphs(trs, graphs_from(oracle, trs))
    poly = splitmix_field(N, 1800 + K + trs)
    want_lv, want_t = oracle.commit_standard(poly, K, trs, lin, want_tensor=True)
    c = hb.commit_standard(poly, K, trs, lin)
    try:
        M, cols = c.M, c.cols
        levels = c.levels()
        assert np.array_equal(levels, want_lv)
        assert np.array_equal(c.tensor(), want_t)
        assert np.array_equal(cr.tree(cr.leaf_chain(np.ascontiguousarray(want_t.transpose(0, 2, 1, 3))), 1), want_lv)
        qc = np.array([0, cols - 1, 0, cols - 1], np.uint32); qr = np.array([0, 0, 2 * trs - 1, 2 * trs - 1], np.uint32)
        assert np.array_equal(c.gather(qr, qc), np.stack([want_t[:, r, q] for r, q in zip(qr, qc)]))
        assert np.array_equal(c.paths(qc, qr), cr.paths(want_lv, M, (qr // 4).astype(np.int64) * cols + qc))
    finally:
        c.free()


# ---- i. hobbit_aggregate: the coefficients travel in slices of 64 per launch ---------------------------------------------------------
@pytest.mark.parametrize("M", [1, 255, 4097])
@pytest.mark.parametrize("K", [1, 63, 64, 65, 128, 200])
def test_aggregate_slices_of_64(hb, oracle, K, M):
    poly = splitmix_field(K * M, 1900 + K + M); beta = splitmix_field(K, 1901 + K)
    d = hb.to_device(poly); o = Guarded(hb, 16 * M)
    hb._chk(hb.lib.hobbit_aggregate(hb.ctx, d.ptr, K * M, vp(beta), K, o.ptr))
    assert np.array_equal(o.host((M, 2), np.uint64), oracle.aggregate(poly, beta))
    assert o.intact()
