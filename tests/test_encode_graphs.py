"""The recursive expander encode on graphs other than the one libc draws after rng_reset().

hobbit_graph_finalize chooses every kernel form from the uploaded graphs -- k_encode in one or two passes, k_enc_fat for C_0, C_1 and D_0,
k_enc_narrow for the five steps between them, k_enc_tiled, the general-weight twins -- and builds their tables on the host: lanes dealt by
in-degree in serpentine order, slots ordered by a matching against LDS bank quads, padding slots re-pointed, a width per wave, a refusal
when a cap is exceeded.  Every case here uploads its graphs and then holds the library to

  * Hobbit.encode_forms() == adversarial.expected_forms, the plain restatement of the selection rules (so a form that silently stopped
    being selected fails here, though its fallback computes the same codeword),
  * the profile names of an in-place and of an out-of-place encode == adversarial.expected_chain,
  * every column of both == the oracle's encode_monolithic under the same edges (oracle.graph_set_edges, pinned to the Python-integer
    sum by tests/test_encode_graph_families_cpu.py), rows [len, 2n) zero over a dirty buffer.

(a) natural draws on both sides of every size class and rule, (b) the synthetic families of adversarial.graph_families, (c) the same
graphs through the rows-innermost encode, (d) the commit on the two fallback chains no drawn graph selects at n = 4096.  The last test
checks that between them the in-place encodes ran under every profile name of launch_encode and launch_encode_long."""
import os
import numpy as np
import pytest
import adversarial as A
from adversarial import FAMILIES_4096

pytestmark = pytest.mark.gpu
N = 4096
OBSERVED = set()            # profile names of every in-place encode of this module


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)
    yield h
    h.close()


def _batches(n):
    """one column, and: n = 4096 -- every persistent workgroup of k_enc_fat_A takes one column and four take a second; else 70"""
    return (1, A.CTX["FAT_A_WGS"][0] + 4) if n == N else (1, 70)


def _upload(hb, oracle, lv, n, tag):
    """lv on the oracle (which holds graphs of the same shape) and on the device; the forms finalize chose against the restatement"""
    A.set_graphs(oracle, lv)
    want = A.expected_forms(lv, n)
    ln = hb.upload_graphs(n, lv)
    assert ln == A.code_plan(lv, n)[1][0]
    pending = want.size_class == "tiled"                                     # the tiled steps are built by the first encode
    assert hb.encode_forms() == dict(want, tiled_pending=pending, tiled_depth=0 if pending else want["tiled_depth"]), (tag, want.why, want.top)
    return want, ln


def _oracle_codewords(oracle, x, ln):
    out = np.empty((x.shape[0], 2 * x.shape[1], 2), np.uint64)
    for c in range(x.shape[0]):
        out[c], l = oracle.encode_monolithic(x[c])
        assert l == ln
    return out


def check_encode(hb, oracle, lv, n, tag, batches=None):
    want, ln = _upload(hb, oracle, lv, n, tag)
    batches = batches or _batches(n)
    x = A.encode_messages(n, max(batches), seed=n)
    ref = _oracle_codewords(oracle, x, ln)
    assert not ref[:, ln:].any() and ref[0, n:ln].any()
    for nb in batches:
        res = {}
        for in_place in (True, False):
            res[in_place], ran = A.encode_with_kernels(hb, x[:nb], in_place=in_place)
            assert ran == A.expected_chain(want, in_place), (tag, nb, in_place, ran)
            if in_place:
                OBSERVED.update(ran)
            assert hb.encode_forms() == want, (tag, nb, in_place)
        bad = np.flatnonzero((res[True] != res[False]).any(axis=(1, 2)))
        assert bad.size == 0, (tag, nb, "columns that differ between the in-place and the out-of-place encode", bad[:8].tolist(), bad.size)
        bad = np.flatnonzero((res[True] != ref[:nb]).any(axis=(1, 2)))
        assert bad.size == 0, (tag, nb, "columns that differ from the oracle", bad[:8].tolist(), bad.size,
                               "first rows", np.flatnonzero((res[True][bad[0]] != ref[bad[0]]).any(axis=1))[:8].tolist())
        assert not res[True][:, ln:].any() and not res[False][:, ln:].any(), (tag, nb, "rows [len, 2n) are not zero")
    return want


def _id(case):
    return "%d" % case[0] + ("" if case[1] is None else "_after_%d_draws" % case[1]) + ("" if len(case) < 3 else "_one_weight_" + case[2])


# ---- (a) natural draws ----------------------------------------------------------------------------------------------------------------------
def test_natural_draws_still_cover_every_rule(oracle):
    A.natural_guard({c: A.expected_forms(A.natural_graphs(oracle, c), c[0]) for c in A.NATURAL})


@pytest.mark.parametrize("case", A.NATURAL + A.NATURAL_FULLW, ids=_id)
def test_natural_draw(hb, oracle, case):
    check_encode(hb, oracle, A.natural_graphs(oracle, case), case[0], _id(case))


def test_drawn_4096_reports_every_register_form(hb, oracle):
    """the draw the benchmark runs on: all three fat steps and the narrow plan"""
    lv = A.drawn_graphs(oracle, N)
    want, _ = _upload(hb, oracle, lv, N, "4096")
    assert dict(want) == dict(small_weights=True, fatA=True, fatC1=True, fatD=True, narrow=True, tiled_pending=False, tiled_depth=0)


# ---- (b) synthetic families -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES_4096)
def test_family_4096(hb, oracle, name):
    lv, meant = A.graph_families(A.drawn_graphs(oracle, N), N)[name]
    want = check_encode(hb, oracle, lv, N, name)
    assert {k: want[k] for k in meant} == meant, (name, dict(want))


def test_family_tile_split(hb, oracle):
    lv, _ = A.graph_families(A.drawn_graphs(oracle, 5955), 5955)["tile_split"]
    check_encode(hb, oracle, lv, 5955, "tile_split")


# ---- (c) rows-innermost ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FAMILIES_4096 + ["drawn_3333", "drawn_4000"])
def test_rows_innermost(hb, oracle, name):
    """k_enc_ilv over the same graphs, in place: rows = 4 (the lanes of a wave own different outputs, with different trip counts) and
    rows = 64 (a wave's records are uniform), 8 messages, against the batch encode and the oracle"""
    if name.startswith("drawn_"):
        n = int(name[6:]); lv = A.drawn_graphs(oracle, n)
    else:
        n = N; lv = A.graph_families(A.drawn_graphs(oracle, N), N)[name][0]
    want, ln = _upload(hb, oracle, lv, n, name)
    x = A.encode_messages(n, 8, seed=n + 1)
    batch = hb.encode_monolithic(x, in_place=False)
    assert np.array_equal(batch, _oracle_codewords(oracle, x, ln)), name
    kname = "k_enc_ilv" if want["small_weights"] else "k_enc_ilv_fullw"
    for rows in (4, 64):
        for m0 in range(0, 8, rows):
            sel = (m0 + np.arange(rows)) % 8
            got, ran = A.with_kernels(hb, lambda: hb.encode_interleaved(np.ascontiguousarray(x[sel].transpose(1, 0, 2)), in_place=True))
            assert ran == {kname, "k_zero16"}, (name, rows, ran)                    # every step, then the zero tail
            assert got.shape == (2 * n, rows, 2)
            bad = np.flatnonzero((got.transpose(1, 0, 2) != batch[sel]).any(axis=(1, 2)))
            assert bad.size == 0, (name, rows, m0, "messages that differ from the batch encode", bad.tolist())


# ---- (d) the commit on a fallback chain -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cap_plus_one_D0_pos0", "cap_plus_one_C1_pos0"])
def test_commit_on_a_fallback_chain(hb, oracle, name):
    """commit_standard at N = 2^24, K = 2, trs = 4096 on a re-used, dirtied tensor buffer (as test_commit_unwritten_zero_tail_on_a_dirty_buffer
    does) under graphs whose in-place chain is {k_enc_fat_A, k_encode_B} -- which writes the whole zero tail whatever the commit asked for --
    or has k_encode_C1 in it: the levels are those of HOBBIT_COMMIT_SKIP_TAIL=0, and 16 columns gathered over all 8192 rows are the oracle's
    codewords of their own first 4096 rows with zeros behind"""
    Nn, K, trs = 1 << 24, 2, N
    lv = A.graph_families(A.drawn_graphs(oracle, N), N)[name][0]
    want, ln = _upload(hb, oracle, lv, N, name)
    chain = A.expected_chain(want, True)
    assert chain == ({"k_enc_fat_A", "k_encode_B"} if "D0" in name else {"k_enc_fat_A", "k_encode_C1", "k_encode_M2", "k_enc_fat_D"})
    d = hb.fill_splitmix(Nn, 6161)
    os.environ["HOBBIT_COMMIT_SKIP_TAIL"] = "0"
    try:
        c0 = hb.commit_standard((d, Nn), K, trs, 1)
        want_levels = c0.levels()
        ptr = hb.lib.hobbit_commitment_tensor_dev(c0.h)
        hb._chk(hb.lib.hobbit_fill_splitmix(hb.ctx, ptr, 4 * Nn, 98)); hb.sync()      # dirty the whole buffer, then park it for the next commit
        c0.free()
    finally:
        del os.environ["HOBBIT_COMMIT_SKIP_TAIL"]
    c, ran = A.with_kernels(hb, lambda: hb.commit_standard((d, Nn), K, trs, 1))
    assert chain <= ran and not (A.encode_kernel_names() - chain) & ran, (name, sorted(ran))
    assert hb.encode_forms() == want
    assert np.array_equal(c.levels(), want_levels), name
    cols = np.concatenate([[0, 1, c.cols - 2, c.cols - 1], 2 + np.random.default_rng(16).choice(c.cols - 4, 12, replace=False)])
    rows = np.arange(2 * trs)
    for col in cols:
        got = c.gather(rows, np.full(2 * trs, col))                      # (rows, K, 2)
        for i in range(K):
            cw, l = oracle.encode_monolithic(got[:trs, i])
            assert l == ln and got[:trs, i].any()
            assert np.array_equal(got[:, i], cw), (name, int(col), i, np.flatnonzero((got[:, i] != cw).any(axis=1))[:8].tolist())
    c.free()


# ---- every launch of launch_encode / launch_encode_long, in place ---------------------------------------------------------------------------
def test_every_encode_launch_ran_in_place(hb, oracle):
    """the union of the in-place kernel names this module saw is every profile name in launch_encode and launch_encode_long, the
    general-weight twins included.  (Run alone or out of order, it first encodes one column on the cases whose chain is still missing.)"""
    names = A.encode_kernel_names()
    cover = [("natural", c) for c in A.NATURAL + A.NATURAL_FULLW] + [("family", f) for f in ("cap_plus_one_D0_pos0", "one_big_weight_2^32")]
    for kind, c in cover:
        if names <= OBSERVED:
            break
        n = c[0] if kind == "natural" else N
        lv = A.natural_graphs(oracle, c) if kind == "natural" else A.graph_families(A.drawn_graphs(oracle, N), N)[c][0]
        if not A.expected_chain(A.expected_forms(lv, n), True) <= OBSERVED:
            check_encode(hb, oracle, lv, n, str(c), batches=(1,))
    assert OBSERVED == names, sorted(OBSERVED ^ names)
