"""Cross-check of the C restatement against the real reference build (oracle/_ref), on inputs beyond the
committed per-case fixtures.  The reference's answers were recorded once from oracle/_ref by
`python oracle/gen_golden.py oracle_vs_ref` (tests/golden/oracle_vs_ref.npz, large arrays as a SHA-256
digest plus sampled rows) and the CASES ones by gen_golden.py itself, so the check runs everywhere."""
import os
import numpy as np
import pytest
import golden_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def recorded(case):
    with np.load(os.path.join(GOLD, "oracle_vs_ref.npz"), allow_pickle=False) as z:
        pre = case + "__"
        return {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def assert_same(got, want, name):
    assert want and set(got) == set(want), (name, sorted(got), sorted(want))
    for k in want:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (name, k)


@pytest.mark.parametrize("name", ["field", "mimc", "blake", "merkle", "fft", "sumcheck", "elastic_open"])
def test_case_agrees(oracle, name):
    with np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False) as z:
        want = {k: z[k] for k in z.files}
    assert_same(golden_cases.CASES[name](oracle), want, name)


@pytest.mark.parametrize("n", list(golden_cases.VS_REF_GRAPH_SIZES))
def test_graph_and_encode_random_sizes(oracle, n):
    name = "graph_encode_n%d" % n
    assert_same(golden_cases.VS_REF_CASES[name](oracle), recorded(name), name)


def test_commit_2e18_full_tensor(oracle):
    assert_same(golden_cases.vs_ref_commit_2e18(oracle), recorded("commit_2e18"), "commit_2e18")


def test_elastic_open_passes_other_shape(oracle):
    """aggregate / compute_aggregation_reply of Elastic_PC::open (option 1) at a shape outside the fixtures"""
    assert_same(golden_cases.vs_ref_elastic_shape(oracle), recorded("elastic_shape"), "elastic_shape")
