"""The host-built twiddle tables of the FFT module (csrc/hobbit_fft_tables.hpp), checked on the host (no GPU).

Every table the library uploads is a pure function of (kind, logn, direction).  tests/fft_tables_check.cpp includes that header and is built
here as a stand-alone program, once plainly and once with the address and undefined-behaviour sanitizers.  For each kind, at its smallest and
one mid logn, in both directions, every entry is compared with its definition, computed by square-and-multiply from root_of_unity(logn):

  * plain roots (logn 0, 1, 2, 7): w^k;
  * radix-8 (logn 3, 5, 6, 7, 8, 11, and 12 = k_fft4096's): w_N2^(rev3(t) k N2 / (8h)) per pass, then the tail w_N^(q k); the table with
    neither (logn 3) is the one entry 1;
  * split (logn 25): hi[a] lo[b] = w^(a 2^14 + b) at the corners and at 400 fixed pseudo-random (a, b);
  * the 8th roots handed to the kernels: w8, w8^3, and w4 = -i forward, +i inverse.

The counts asserted below are the tables' sizes, worked out from the layouts.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")

RADIX8 = {3: 1, 5: 3 * 8, 6: 7 * 8, 7: 7 * 8 + 64, 8: 7 * 8 + 3 * 64, 11: 7 * 8 + 7 * 64 + 3 * 512}      # logn -> entries
WANT = {"roots": 1 + 1 + 2 + 64, "radix8": sum(RADIX8.values()), "radix8_4096": 7 * (8 + 64 + 512), "split": 9 + 400}


@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def tables_check(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fft_tables") / "fft_tables_check")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "fft_tables_check.cpp"), "-o", exe])
    return exe


def test_every_table_entry_matches_its_definition(tables_check):
    p = subprocess.run([tables_check], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    out = dict(line.split(None, 1) for line in p.stdout.splitlines())
    for kind, n in WANT.items():
        for d in ("fwd", "inv"):
            assert int(out["%s_%s" % (kind, d)]) == n, (kind, d, out)
    assert out["r8_roots"] == "ok"
