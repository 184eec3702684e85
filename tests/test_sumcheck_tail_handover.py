"""The hand-over of the 2-product sumcheck's last tables to the host through the context's tail area.

The launch that produces the tables the host continues from also stores them into coherent pinned memory, and the round's mailbox post
tells the host they have landed; no copy command and no stream drain remain on that path.  Sizes, with SC_TAIL = 1024: 1024 runs every
round on the host (one launch that copies and posts), 2048 runs round 0 on the caller's tables without a fold (a copy launch in front
of the round's post), 4096 and 8192 run one and two single rounds (the fold launch writes the area), 16384 and 32768 take a two-round
trip and the bridge first.  Every form -- dense, sparse list, eq points -- is compared bit for bit with the oracle's sumcheck2 on the
table the form stands for.  A tail area read before its own post would hand the previous call's tables to the transcript: one context
runs 32768, 2048 and 4096 back to back on different inputs.  Tail areas are per context: two contexts on one device run from two threads."""
import threading
import numpy as np
import pytest
from adversarial import scatter_dense
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
PREV_R = np.array([33, 0], np.uint64)
SC_KEYS = ("poly", "r", "vr", "fin")
SIZES = [1024, 2048, 4096, 8192, 16384, 32768]
FULL_A = np.array([0x123456789ABCDEF, 0x0FEDCBA98765432], np.uint64)


def new_context():
    from __graft_entry__ import load_package
    return load_package().Hobbit(0)          # raises if the HIP library or the GPU is missing: no fallback


@pytest.fixture(scope="module")
def hb():
    h = new_context()
    yield h
    h.close()


@pytest.fixture(scope="module")
def dense_cases(oracle):
    """{(n, seed): (v1, v2, the oracle's proof)}: computed once, shared, never written to"""
    out = {}
    for n in SIZES:
        for seed in (0, 1):
            v1, v2 = splitmix_field(n, 900 + 2 * seed + n.bit_length()), splitmix_field(n, 950 + 2 * seed + n.bit_length())
            out[(n, seed)] = (v1, v2, oracle.sumcheck2(v1, v2, PREV_R))
    return out


def same(got, want, what):
    for k in SC_KEYS:
        assert np.array_equal(got[k], want[k]), "%s: %s differs" % (what, k)


@pytest.mark.parametrize("n", SIZES)
def test_dense_form(hb, dense_cases, n):
    v1, v2, want = dense_cases[(n, 0)]
    same(hb.generate_2product_sumcheck_proof(v1, v2, PREV_R), want, "dense n=%d" % n)


@pytest.mark.parametrize("n", SIZES)
def test_sparse_list_form(hb, oracle, n):
    """a list with entries at both ends and about a fifth of the positions in between"""
    v1 = splitmix_field(n, 700 + n.bit_length())
    idx = np.unique(np.concatenate([[0, n - 1], np.arange(3, n, 5)])).astype(np.uint64)
    val = splitmix_field(len(idx), 720 + n.bit_length())
    want = oracle.sumcheck2(v1, scatter_dense(n, idx, val), PREV_R)
    same(hb.generate_2product_sumcheck_proof_sparse(v1, idx, val, PREV_R), want, "sparse n=%d" % n)


@pytest.mark.parametrize("n", SIZES)
def test_eq_form(hb, oracle, n):
    """one and two points: the first table is sum_j a_j precompute_beta(r_j), built here with the oracle's field operations"""
    k = n.bit_length() - 1
    v2 = splitmix_field(n, 800 + k)
    pts = [splitmix_field(k, 810 + k), splitmix_field(k, 820 + k)]
    for T, sc in ((1, [FULL_A]), (2, [np.array([1, 0], np.uint64), FULL_A])):
        tab = None
        for r, a in zip(pts[:T], sc):
            b = oracle.precompute_beta(r)
            term = oracle.f_mul(np.tile(a, (b.shape[0], 1)), b)
            tab = term if tab is None else oracle.f_add(tab, term)
        want = oracle.sumcheck2(tab, v2, PREV_R)
        same(hb.generate_2product_sumcheck_proof_eq(pts[:T], sc, v2, PREV_R), want, "eq n=%d T=%d" % (n, T))


def test_tail_area_is_not_read_before_its_post(hb, dense_cases):
    """32768, then 2048, then 4096, back to back in one context on different inputs: each call's tail comes from its own tables.  The
    area still holds the previous call's 2048 elements per table when the next call starts."""
    for n, seed in ((32768, 1), (2048, 0), (4096, 1), (2048, 1), (1024, 0), (4096, 0)):
        v1, v2, want = dense_cases[(n, seed)]
        same(hb.generate_2product_sumcheck_proof(v1, v2, PREV_R), want, "back to back n=%d seed=%d" % (n, seed))


def test_two_contexts_two_threads(dense_cases):
    """two contexts on one device, each driven by its own thread at the same sizes on different inputs: each has a mailbox and a tail area
    of its own and gets its own results"""
    ctxs = [new_context(), new_context()]
    got, errs = [{}, {}], []

    def drive(t):
        try:
            for rep in range(3):
                for n in SIZES:
                    v1, v2, _ = dense_cases[(n, t)]
                    got[t][(n, rep)] = ctxs[t].generate_2product_sumcheck_proof(v1, v2, PREV_R)
        except Exception as e:          # (reported by the main thread)
            errs.append((t, repr(e)))

    try:
        threads = [threading.Thread(target=drive, args=(t,)) for t in (0, 1)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errs, errs
        for t in (0, 1):
            for (n, rep), g in got[t].items():
                same(g, dense_cases[(n, t)][2], "context %d n=%d repeat %d" % (t, n, rep))
    finally:
        for c in ctxs:
            c.close()
