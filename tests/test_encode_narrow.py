"""The five narrow steps C_2 .. D_1 of the n = 4096 encode in their persistent one-wave-per-column form (k_enc_narrow, launched under the
profile name k_encode_M2), in place, bit for bit against the out-of-place k_encode_A / k_encode_B split on every column and against the
oracle on the first, the middle and the last column.

A launch takes W = NARROW_WGS columns per round (one wave each) and a wave walks columns c, c + W, ...: the batch sizes put the loop's
edges -- no second column, a ragged last round, exactly one round, one column into the second -- in front of the kernel.  A wave keeps the
window [x_2 .. z_1] in LDS from column to column and orders its steps by program order alone, so a missing wait or a stale window shows as
one column's values inside another's: the zero / all-(p-1) batch is about that."""
import os
import re
import numpy as np
import pytest
from adversarial import FAT_CHAIN_4096, P, encode_with_kernels, families, graphs_from, set_weights
from oracle.pyoracle import splitmix_field

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096
LEN = 7045                                      # codeword length of n = 4096; rows [LEN, 2n) are zero
WEIGHTS = {"drawn": None, "2^32-1": [(1 << 32) - 1, 0], "full_p-1": [P - 1, P - 1]}


def _ctx_constants():
    """{name: [values]} of the kernel's NARROW_* tables (csrc/hobbit_ctx.hpp)"""
    src = open(os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd", "csrc", "hobbit_ctx.hpp")).read()
    out = {}
    for name, val in re.findall(r"\b(NARROW_[A-Z0-9_]+)(?:\[[A-Z_]+\])? = (\{[0-9, ]+\}|[0-9]+)[,;]", src):
        out[name] = [int(v) for v in re.findall(r"[0-9]+", val)]
    return out


C = _ctx_constants()
W = C["NARROW_WGS"][0]
assert W >= 64 and len(C["NARROW_LPO"]) == len(C["NARROW_CAP"]) == len(C["NARROW_STEP_OF"]) == C["NARROW_POS"][0]


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)
    yield h
    h.close()


def _drawn(oracle):
    oracle.rng_reset(); oracle.expander_init_store(N)
    return graphs_from(oracle, N)


@pytest.fixture(scope="module")
def big(hb, oracle):
    """3 W + 5 messages (the families first, uniform ones behind them) and their codewords by the out-of-place A/B split under the drawn
    graphs, computed once: every batch below is a prefix of it (columns are encoded independently)"""
    hb.upload_graphs(N, _drawn(oracle))
    fam = np.stack(list(families(N, seed=N).values()))
    nb = 3 * W + 5
    x = np.concatenate([fam, splitmix_field((nb - len(fam)) * N, 4097).reshape(nb - len(fam), N, 2)])
    out, ran = encode_with_kernels(hb, x, in_place=False)
    assert ran == {"k_encode_A", "k_encode_B"}, ran
    x.setflags(write=False); out.setflags(write=False)
    return x, out


@pytest.mark.parametrize("batch", ["1", "W-1", "W", "W+1", "3W+5"])
def test_narrow_batch_sizes(hb, oracle, big, batch):
    """fewer columns than resident waves, one short of a round, one round, one column into the second, three rounds and a ragged fourth"""
    x, out = big
    nb = {"1": 1, "W-1": W - 1, "W": W, "W+1": W + 1, "3W+5": 3 * W + 5}[batch]
    hb.upload_graphs(N, _drawn(oracle))
    assert hb.encode_forms()["narrow"] is True                   # k_encode_M2 below is k_enc_narrow, not its one-workgroup fallback
    got, ran = encode_with_kernels(hb, x[:nb], in_place=True)
    assert ran == FAT_CHAIN_4096, (batch, ran)
    bad = np.flatnonzero((got != out[:nb]).any(axis=(1, 2)))
    assert bad.size == 0, (batch, "columns that differ from the out-of-place result", bad[:8].tolist(), bad.size)
    for c in sorted({0, nb // 2, nb - 1}):
        want, ln = oracle.encode_monolithic(x[c])
        assert ln == LEN and np.array_equal(got[c][:ln], want[:ln]) and not got[c][ln:].any(), (batch, c)


@pytest.mark.parametrize("wname", list(WEIGHTS))
def test_narrow_families_and_weights(hb, oracle, wname):
    """every family as a message under the drawn weights, every weight 2^32 - 1 (the largest 96-bit sums: all-(p-1) is one of the families)
    and every weight (p-1, p-1), where the full-weight kernels must run and the narrow kernel must not"""
    lv = _drawn(oracle)
    if WEIGHTS[wname] is not None:
        lv = set_weights(oracle, lv, WEIGHTS[wname])
    hb.upload_graphs(N, lv)
    assert hb.encode_forms()["narrow"] is (wname != "full_p-1"), wname
    fams = families(N, seed=N)
    names, x = list(fams), np.stack(list(fams.values()))
    out, ran = encode_with_kernels(hb, x, in_place=False)
    fullw = wname == "full_p-1"
    assert ran == ({"k_encode_fullw_A", "k_encode_fullw_B"} if fullw else {"k_encode_A", "k_encode_B"}), (wname, ran)
    got, ran = encode_with_kernels(hb, x, in_place=True)
    assert ran == ({"k_encode_fullw_A", "k_encode_fullw_B"} if fullw else FAT_CHAIN_4096), (wname, ran)
    assert "k_encode_M2" in ran or fullw
    for r, name in enumerate(names):
        assert np.array_equal(got[r], out[r]), (wname, name)
    for r in sorted({0, len(names) // 2, len(names) - 1, names.index("all_pm1")}):
        want, ln = oracle.encode_monolithic(x[r])
        assert ln == LEN and np.array_equal(got[r][:ln], want[:ln]) and not got[r][ln:].any(), (wname, names[r])


def _raise_in_degree(g, t, deg):
    """re-point edges of graph g (upload_graphs' form) at output t, in input order, until t has in-degree deg"""
    nbr = np.array(g["nbr"], np.int64).reshape(-1)
    have = int((nbr == t).sum())
    moved = np.flatnonzero(nbr != t)[:deg - have]
    nbr[moved] = t
    assert int((nbr == t).sum()) == deg
    return dict(g, nbr=nbr.reshape(np.shape(g["nbr"])))


def _first_position_room(step):
    """in-edges the heaviest output of narrow step `step` may have: lanes per output x register slots of the step's first position"""
    p = C["NARROW_STEP_OF"].index(step)
    return C["NARROW_LPO"][p] * C["NARROW_CAP"][p]


# level -> narrow step (C_2, C_3, D_3, D_2, D_1 are steps 0 .. 4 of the kernel)
OVERFLOW = {"C2": ((2, 0), 0), "D1": ((1, 1), 4)}


@pytest.mark.parametrize("case", list(OVERFLOW))
def test_narrow_cap_overflow_falls_back(hb, oracle, case):
    """one output of a narrow level with one in-edge more than its lanes have register slots: the plan is refused at finalize and the steps
    run by the one-workgroup-per-column kernel under the same profile name; identical to the out-of-place split on every column"""
    key, step = OVERFLOW[case]
    lv = _drawn(oracle)
    lv[key] = _raise_in_degree(lv[key], 0, _first_position_room(step) + 1)
    hb.upload_graphs(N, lv)
    forms = hb.encode_forms()
    assert forms["narrow"] is False and forms["fatA"] and forms["fatC1"] and forms["fatD"], (case, forms)
    x = np.concatenate([np.stack(list(families(N, seed=N).values())), splitmix_field(100 * N, 4098).reshape(100, N, 2)])
    got, ran = encode_with_kernels(hb, x, in_place=True)
    assert ran == FAT_CHAIN_4096, (case, ran)
    out, ran = encode_with_kernels(hb, x, in_place=False)
    assert ran == {"k_encode_A", "k_encode_B"}, (case, ran)
    assert np.array_equal(got, out), case
    assert not got[:, LEN:].any(), case


def test_narrow_no_stale_window(hb, oracle):
    """zero and all-(p-1) messages: as two batches back to back in one context, and alternating by round inside one batch of 2 W + 3 columns,
    so that every wave meets zero, all-(p-1), zero in its window -- a zero column stays zero, an all-(p-1) column is the same everywhere"""
    hb.upload_graphs(N, _drawn(oracle))
    fams = families(N, seed=N)
    two = np.stack([fams["zeros"], fams["all_pm1"]])
    ref, _ = encode_with_kernels(hb, two, in_place=False)
    assert not ref[0].any() and ref[1].any()
    nb = W + 1
    assert hb.encode_forms()["narrow"] is True
    a, ran = encode_with_kernels(hb, np.broadcast_to(two[1], (nb, N, 2)), in_place=True)
    assert ran == FAT_CHAIN_4096, ran
    b, _ = encode_with_kernels(hb, np.broadcast_to(two[0], (nb, N, 2)), in_place=True)
    assert not b.any(), "a zero batch after an all-(p-1) batch carries non-zero values"
    assert (a == ref[1]).all(), "an all-(p-1) batch differs from the reference"
    del a, b
    nb = 2 * W + 3
    kind = (np.arange(nb) // W + 1) % 2                  # round 0: all-(p-1), round 1: zeros, round 2: all-(p-1)
    got, _ = encode_with_kernels(hb, two[kind], in_place=True)
    bad = np.flatnonzero((got != ref[kind]).any(axis=(1, 2)))
    assert bad.size == 0, ("columns with another column's values", bad[:8].tolist(), bad.size)
