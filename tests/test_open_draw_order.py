"""The opening takes the libc draws of both shockwave proofs early, with its other draws, under either schedule.

The reference's transcript is a function of the process-wide libc generator, so an opening has to consume the same number of draws in
the same order whichever schedule runs it: the overlapped one (the default; shockwave_prove(C_c) on a helper context from a second host
thread that is started early and parks until P4 has returned) and the serial one (HOBBIT_OPEN_THREADS=0).  After srand / srandom with a
fixed seed both must give every output array of the oracle's opening under that seed, both shockwave proofs included, and one rand() and
one random() taken straight after the call must return what they return after the oracle's.  A second opening on the same context in the
same process must do the same: the early-started thread leaves nothing behind.  Shape: the smallest of the opening's parity tests."""
import ctypes
import numpy as np
import pytest
from adversarial import graphs_from

pytestmark = pytest.mark.gpu
N, K, QUERIES, SEED = 1 << 18, 32, 5900, 4711
TRS = N // (K << 11)
OPEN_KEYS = ("I", "scalars", "poly", "r", "vr", "fin", "roots", "checks", "reply")


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)          # raises if the HIP library or the GPU is missing: no fallback
    yield h
    h.close()


def seeded(libc):
    libc.srand(SEED); libc.srandom(SEED)


def test_both_schedules_draw_alike(hb, oracle, monkeypatch):
    libc = ctypes.CDLL(None)
    oracle.rng_reset(); poly = oracle.generate_randomness(N); oracle.expander_init_store(TRS)
    x = oracle.generate_randomness(N.bit_length() - 1)
    lv, T = oracle.commit_standard(poly, K, TRS, 1, want_tensor=True)
    seeded(libc); want = oracle.open_standard(poly, K, TRS, x, QUERIES, tensor=T); want_after = (int(libc.rand()), int(libc.random()))
    hb.upload_graphs(TRS, graphs_from(oracle, TRS))
    c = hb.commit_standard(poly, K, TRS, 1)
    runs = []
    # default, serial, and the default again: the second and third openings of this context
    for name, env in (("overlapped", None), ("serial", "0"), ("overlapped, again", None), ("serial, again", "0")):
        with monkeypatch.context() as m:
            if env is None:
                m.delenv("HOBBIT_OPEN_THREADS", raising=False)
            else:
                m.setenv("HOBBIT_OPEN_THREADS", env)
            seeded(libc); got = hb.open_standard(poly, c, x, QUERIES, want_paths=True); after = (int(libc.rand()), int(libc.random()))
        runs.append((name, got, after))
    c.free()
    assert want["checks"].tolist() == [1, 1, 1]
    for name, got, after in runs:
        assert after == want_after, "%s: rand() / random() after the call %r, after the oracle's %r" % (name, after, want_after)
        for k in OPEN_KEYS:
            assert np.array_equal(got[k], want[k]), (name, k)
        for sp in ("sp_c", "sp_f"):
            assert set(want[sp]) <= set(got[sp]), (name, sp)
            for k in want[sp]:
                assert np.array_equal(got[sp][k], want[sp][k]), (name, sp, k)
    # every output array the library returns, those the oracle does not restate (the Merkle paths) included, is the same in every run
    _, first, _ = runs[0]
    for name, got, _ in runs[1:]:
        assert set(got) == set(first), name
        for k in first:
            if isinstance(first[k], dict):
                assert set(got[k]) == set(first[k]), (name, k)
                for kk in first[k]:
                    assert np.array_equal(got[k][kk], first[k][kk]), (name, k, kk)
            else:
                assert np.array_equal(got[k], first[k]), (name, k)
