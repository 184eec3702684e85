"""The inputs of tests/test_encode_graphs.py, checked without a device: the oracle's encode under replaced edges (graph_set_edges) against
the plain Python-integer sum over the edge lists (adversarial.py_encode) for every graph family, and every family against the restatement of
hobbit_graph_finalize's selection rules (adversarial.expected_forms): a family selects the form it was built to select.  These are
conditions on the inputs, not measurements -- when a cap in csrc/hobbit_ctx.hpp changes, the second test names the family to re-derive
instead of the device test quietly covering less."""
import numpy as np
import pytest
import adversarial as A

N = 4096
FAMILIES_4096 = A.FAMILIES_4096
CASES = [(N, f) for f in FAMILIES_4096] + [(5955, "tile_split")]


def _family(oracle, n, name):
    fams = A.graph_families(A.drawn_graphs(oracle, n), n)
    assert n != N or sorted(fams) == sorted(FAMILIES_4096)
    return fams[name]


def test_constants_are_read_from_the_header():
    for k in ("FAT_A_CAP0", "FAT_A_CAP1", "FAT_C1_CAP0", "FAT_D_CAP0", "FAT_D_CAP1", "FAT_D_CAP2", "FAT_A_WGS", "TILE_ELEMS", "TILE_MID_MAX",
              "ENC_WIDE_MIN", "NARROW_WGS", "NARROW_CAP", "NARROW_LPO"):
        assert A.CTX.get(k), k
    assert len(A.CTX["NARROW_CAP"]) == len(A.CTX["NARROW_LPO"]) == len(A.CTX["NARROW_STEP_OF"]) == A.CTX["NARROW_POS"][0]
    assert len(A.encode_kernel_names()) == 17, sorted(A.encode_kernel_names())


@pytest.mark.parametrize("n,name", CASES, ids=[c[1] for c in CASES])
def test_oracle_under_replaced_edges_is_the_plain_sum(oracle, n, name):
    """one column per family: the oracle's encode_monolithic after graph_set_edges equals py_encode over the same edge lists, the tail is
    zero, and putting the drawn edges back gives the drawn codeword again"""
    lv0 = A.drawn_graphs(oracle, n)
    x = A.encode_messages(n, 16, seed=n)[(0, 14, 15)[CASES.index((n, name)) % 3]]          # all (p-1, p-1), or a uniform message
    drawn, ln0 = oracle.encode_monolithic(x)
    lv, _ = A.graph_families(lv0, n)[name]
    for key, g in lv.items():
        assert (g["L"], g["R"], g["degree"]) == (lv0[key]["L"], lv0[key]["R"], lv0[key]["degree"])
        assert np.asarray(g["nbr"]).min() >= 0 and np.asarray(g["nbr"]).max() < g["R"]
    A.set_graphs(oracle, lv)
    got, ln = oracle.encode_monolithic(x)
    want = A.from_py(A.py_encode(lv, A.to_py(x)))
    assert ln == ln0 == len(want) == A.code_plan(lv, n)[1][0]
    assert np.array_equal(got[:ln], want) and not got[ln:].any()
    assert not np.array_equal(got, drawn)
    A.set_graphs(oracle, lv0)
    assert np.array_equal(oracle.encode_monolithic(x)[0], drawn)


def test_graph_set_edges_refuses_a_neighbour_out_of_range(oracle):
    lv0 = A.drawn_graphs(oracle, 100)
    g = lv0[(0, 1)]
    bad = np.array(g["nbr"]); bad[-1] = g["R"]
    with pytest.raises(ValueError):
        oracle.graph_set_edges(0, 1, bad, g["w"])
    assert np.array_equal(oracle.graph(0, 1)["nbr"], g["nbr"])
    with pytest.raises(AssertionError):
        oracle.graph_set_edges(0, 1, g["nbr"][:-1], g["w"][:-1])


@pytest.mark.parametrize("n,name", CASES, ids=[c[1] for c in CASES])
def test_family_selects_the_form_it_is_built_for(oracle, n, name):
    lv, want = _family(oracle, n, name)
    f = A.expected_forms(lv, n)
    assert {k: f[k] for k in want} == want, (name, dict(f), f.why, f.top)
    assert f.size_class == ("tiled" if n == 5955 else "deep")
    if name.startswith("cap_"):
        over = 0 if name.startswith("cap_exact_") else 1
        _, step, pos = A.CAP_CASES[name[len("cap_plus_one_" if over else "cap_exact_"):]]
        assert f.top[step][pos] == A.FAT[step][3][pos] + over, (name, f.top)                 # on the cap, or one above it
        assert all(t <= c for j, (t, c) in enumerate(zip(f.top[step], A.FAT[step][3])) if j < pos), (name, f.top)   # nothing refuses it earlier
    if name == "bank_clash":
        g = lv[(0, 0)]
        nbr = np.asarray(g["nbr"]).reshape(g["L"], g["degree"])
        assert ((nbr // 16) % 16 == (np.arange(g["L"]) % 16)[:, None]).all()
        assert sorted(set(A.in_degrees(g).tolist())) == [36, 48] and f.top["fatA"] == [48, 48]
    if name == "empty_outputs":
        for key, g in lv.items():
            deg = A.in_degrees(g)
            assert not deg[A.empty_set(g["R"])].any() and deg[0] == 0 and deg[-1] == 0 and (np.delete(deg, A.empty_set(g["R"])) > 0).all(), key
    if name == "narrow_empty_outputs":
        for key in A.NARROW_LEVELS:
            deg = A.in_degrees(lv[key])
            assert deg[0] == 0 and deg[-1] == 0 and (deg[1:-1] > 0).all(), key
    if name == "hubs":
        for key in [(0, 0), (1, 0), (0, 1)]:
            g = lv[key]; d = g["degree"]
            nbr = np.asarray(g["nbr"]).reshape(g["L"], d); w = np.asarray(g["w"]).reshape(g["L"], d, 2)
            for i in (0, g["L"] - 1):
                b = nbr[i, -1]
                assert len(set(nbr[i, :-1].tolist())) == 1 and not w[i, -1].any() and (nbr == b).sum() == 1, (key, i)
            assert len(set(nbr[g["L"] // 2].tolist())) == 1
    if name == "tile_split":
        g = lv[(0, 0)]; T = A.CTX["TILE_ELEMS"][0]
        nbr = np.asarray(g["nbr"]).reshape(g["L"], g["degree"])
        assert (nbr[:T] < g["R"] // 2).all() and (nbr[T:] >= g["R"] // 2).all()
        assert (lv[(0, 1)]["R"] + 63) // 64 > A.CTX["TILE_WAVES"][0] * A.CTX["TILE_MAXS"][0]      # D_0: two output groups


def test_natural_draws_still_cover_every_rule(oracle):
    A.natural_guard({c: A.expected_forms(A.natural_graphs(oracle, c), c[0]) for c in A.NATURAL})


def test_expected_chains_name_every_launch(oracle):
    """the cases of tests/test_encode_graphs.py, by the restatement alone: between them their in-place chains are every profile name of
    launch_encode and launch_encode_long"""
    seen = set()
    for c in A.NATURAL + A.NATURAL_FULLW:
        seen |= A.expected_chain(A.expected_forms(A.natural_graphs(oracle, c), c[0]), True)
    for n in (N, 5955):
        for name, (lv, _) in A.graph_families(A.drawn_graphs(oracle, n), n).items():
            seen |= A.expected_chain(A.expected_forms(lv, n), True)
    assert seen == A.encode_kernel_names(), sorted(seen ^ A.encode_kernel_names())
