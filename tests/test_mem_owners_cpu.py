"""The memory owners of csrc/hobbit_mem.hpp (Buf, GrowBuf, Pool, Pooled) against a counting fake in place of HIP (no GPU).

tests/mem_owner_check.cpp compiles the real header with plain g++, HOBBIT_MEM_FAKE defined and its own mem::raw, under the address and
undefined-behaviour sanitizers, and checks: every allocation is freed exactly once on scope exit, moves / release / adopt hand over without
freeing, the grow-only buffer's wait-free-allocate order, the pool's exact-size reuse, its 48-buffer and 8 GiB caps, its drain-and-retry on a
failed allocation, and that a begin-shaped constructor that fails at any step leaves nothing live.  The header's live counter (the one behind
hobbit_mem_live) must agree with the fake's table after every step."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hobbit-space-efficient-zksnark-with-optimal-prover-time_amd")


def test_owners_under_sanitizers(tmp_path):
    exe = str(tmp_path / "mem_owner_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "mem_owner_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
