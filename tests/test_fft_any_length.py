"""hobbit_fft_any: the transform at every length up to 2^28, forward and inverse.

Up to 2^22 the oracle's CPU transform is the reference (1.7 s at 2^22; 21 s at 2^25, which no test can afford).  Above that, correctness
is carried by the exact decimation-in-time identity (tests/fft_identity.py) chained up from 2^22 -- every length against the length
below it, bit for bit, dense full-range inputs, all on the device -- and by an exact sparse check at chosen outputs.  The checkers
themselves are pinned on the CPU by tests/test_fft_identity_cpu.py.

The context runs its own stream: hb.sync() before torch touches what the library wrote, torch.cuda.synchronize() before the library
reads what torch wrote.  Nothing longer than a few windows is downloaded; comparisons return one boolean."""
import ctypes
import os
import numpy as np
import pytest
import torch
from adversarial import families, P
from oracle.pyoracle import splitmix_field
import fft_identity as fi

pytestmark = pytest.mark.gpu
EINVAL = -2


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    mod = load_package()
    h = mod.Hobbit(0)          # raises if the HIP library or the GPU is missing: no fallback
    yield h
    h.close()
    torch.cuda.empty_cache()


def dev_empty(n):
    return torch.empty((n, 2), dtype=torch.int64, device="cuda")


def dev_from(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def host_from(t):
    return t.cpu().numpy().view(np.uint64)


def dev_splitmix(hb, n, seed):
    t = dev_empty(n)
    torch.cuda.synchronize()
    hb._chk(hb.lib.hobbit_fill_splitmix(hb.ctx, t.data_ptr(), n, seed))
    hb.sync()
    return t


def dev_fft(hb, t, logn, inverse, batch=1):
    assert t.is_contiguous() and t.numel() == 2 * batch << logn
    torch.cuda.synchronize()
    hb.fft_any_dev(t.data_ptr(), logn, batch, inverse)
    hb.sync()
    return t


class DeviceBackend:
    """the backend of fft_identity.dit_identity over device memory: torch for layout and comparison, hobbit_f_binop for the field"""

    def __init__(self, hb):
        self.hb = hb

    def _binop(self, op, a, b):
        assert a.is_contiguous() and b.is_contiguous() and a.shape == b.shape
        out = torch.empty_like(a)
        torch.cuda.synchronize()
        self.hb._chk(self.hb.lib.hobbit_f_binop(self.hb.ctx, op, a.data_ptr(), b.data_ptr(), out.data_ptr(), a.shape[0]))
        self.hb.sync()
        return out

    def add(self, a, b): return self._binop(0, a, b)
    def sub(self, a, b): return self._binop(1, a, b)
    def mul(self, a, b): return self._binop(2, a, b)
    def fft(self, a, logn, inverse): return dev_fft(self.hb, a, logn, inverse)
    def copy(self, a): return a.clone()
    def equal(self, a, b): return bool(torch.equal(a, b))
    def interleave(self, e, o): return torch.stack([e, o], 1).reshape(-1, 2)

    def const(self, n, v):
        t = dev_empty(n)
        t[:, 0] = int(v[0]); t[:, 1] = int(v[1])
        return t

    def assign(self, dst, at, src):
        dst[at:at + src.shape[0]] = src


# ---- 1. the old call's bits ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logn,inverse", [(8, False), (12, False), (13, False), (17, False), (20, False), (22, False), (8, True), (12, True)])
def test_same_bits_as_fft_batch(hb, logn, inverse):
    x = splitmix_field(1 << logn, 100 + logn)
    assert np.array_equal(hb.fft_any(x, inverse=inverse), hb.fft(x, inverse=inverse))


# ---- 2. long inverse transforms against the oracle, one case per dispatch class of the two-factor form --------------------------------
@pytest.mark.parametrize("logn,names", [(13, None), (14, None), (16, None), (17, None), (19, None), (20, None),
                                        (21, ("mix", "all_pm1", "near_diff")), (22, ("mix", "all_pm1"))])
def test_long_inverse_matches_oracle(hb, oracle, logn, names):
    fam = families(1 << logn, seed=logn)
    names = list(fam) if names is None else list(names)
    got = hb.fft_any(np.stack([fam[k] for k in names]), inverse=True)
    for k, g in zip(names, got):
        assert np.array_equal(g, oracle.fft(fam[k], inverse=True)), "logn %d, family %s" % (logn, k)


@pytest.mark.parametrize("logn", [14, 17])
def test_long_inverse_batched_distinct_rows(hb, oracle, logn):
    x = splitmix_field(3 << logn, 200 + logn).reshape(3, 1 << logn, 2)
    got = hb.fft_any(x, inverse=True)
    for b in range(3):
        assert np.array_equal(got[b], oracle.fft(x[b], inverse=True)), b


# ---- 3. the decimation-in-time identity, dense, chained up from 2^22 -----------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("logn", [23, 24, 25, 26, 27, 28])
def test_dit_identity_dense(hb, oracle, logn, inverse):
    half = 1 << (logn - 1)
    e, o = dev_splitmix(hb, half, 300 + logn), dev_splitmix(hb, half, 400 + logn)
    assert fi.dit_identity(DeviceBackend(hb), oracle, logn, e, o, inverse) == (True, True)
    del e, o
    torch.cuda.empty_cache()


# ---- 4. a sparse input, exact at chosen outputs ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("logn", [22, 25, 26, 27, 28])
def test_sparse_input_exact_windows(hb, oracle, logn, inverse):
    ln = 1 << logn
    pos, val, starts = fi.sparse_case(logn, logn)
    R = ln >> 12
    assert {0, 1, 4095, 4096, R - 1, R, ln // 2, ln - 1} <= set(pos.tolist()) and len(pos) == 48 and len(starts) == 16
    x = torch.zeros((ln, 2), dtype=torch.int64, device="cuda")
    x[torch.from_numpy(pos.astype(np.int64)).cuda()] = dev_from(val)
    dev_fft(hb, x, logn, inverse)
    want = fi.sparse_expected(oracle, logn, pos, val, starts, inverse)
    for s, w in zip(starts, want):
        assert np.array_equal(host_from(x[s:s + fi.WINDOW]), w), "window at %d" % s
    if logn == 22:                                                    # the checker against the full reference, once
        xh = np.zeros((ln, 2), np.uint64); xh[pos.astype(np.int64)] = val
        assert np.array_equal(host_from(x), oracle.fft(xh, inverse=inverse))
    del x
    torch.cuda.empty_cache()


# ---- 5. worst-case values at the first length of the three-factor form, and round trips -------------------------------------------------
def dev_all_pm1(n):
    tile = dev_from(np.full((min(n, 1 << 20), 2), P - 1, np.uint64))
    return tile.repeat(n // tile.shape[0], 1)


@pytest.mark.parametrize("inverse", [False, True])
def test_dit_identity_all_pm1_2e25(hb, oracle, inverse):
    e = dev_all_pm1(1 << 24)
    assert fi.dit_identity(DeviceBackend(hb), oracle, 25, e, e.clone(), inverse) == (True, True)
    del e
    torch.cuda.empty_cache()


@pytest.mark.parametrize("logn", [25, 28])
def test_round_trip(hb, logn):
    for name, x in (("all_pm1", dev_all_pm1(1 << logn)), ("splitmix", dev_splitmix(hb, 1 << logn, 500 + logn))):
        y = x.clone()
        dev_fft(hb, y, logn, False)
        assert not torch.equal(y, x), name
        dev_fft(hb, y, logn, True)
        assert torch.equal(y, x), name
        del x, y
    torch.cuda.empty_cache()


def test_three_factor_form_runs_its_own_kernel(hb):
    x = dev_splitmix(hb, 1 << 25, 1)
    hb.profile(True); hb.profile_reset()
    dev_fft(hb, x, 25, False)
    rep = hb.profile_report()
    hb.profile(False)
    assert rep.get("k_fft_cols_wide", (0, 0))[1] == 1, rep


# ---- 6. the callers whose only limit was the transform length ----------------------------------------------------------------------------
@pytest.mark.parametrize("logN", [24, 26])
def test_whir_commit_long(hb, logN):
    N = 1 << logN; L = 2 * N
    poly = dev_splitmix(hb, N, 600)
    com = dev_empty(L); lv = torch.empty(32 * N, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hb._chk(hb.lib.hobbit_whir_commit(hb.ctx, poly.data_ptr(), N, com.data_ptr(), lv.data_ptr()))
    hb.sync()
    buf = torch.zeros((L, 2), dtype=torch.int64, device="cuda")
    buf[:N] = poly
    torch.cuda.synchronize()
    hb._chk(hb.lib.hobbit_change_form(hb.ctx, buf.data_ptr(), logN))    # in place on the first N elements
    hb.sync()
    dev_fft(hb, buf, logN + 1, False)
    want = buf.view(16, L // 16, 2).transpose(0, 1).contiguous().view(L, 2)   # buff[j*16 + kk] = poly_com[j + kk * L/16]
    assert torch.equal(com, want)
    lv2 = torch.empty_like(lv)
    torch.cuda.synchronize()
    hb._chk(hb.lib.hobbit_mt_commit_blake(hb.ctx, want.data_ptr(), L, lv2.data_ptr()))
    hb.sync()
    nodes = 2 * (L // 4) - 1
    assert torch.equal(lv[32 * (nodes - 1):32 * nodes], lv2[32 * (nodes - 1):32 * nodes])       # the root
    assert torch.equal(lv[:32 * nodes], lv2[:32 * nodes])
    del poly, com, lv, lv2, buf, want
    torch.cuda.empty_cache()


@pytest.mark.parametrize("logN", [26, 28])                     # rows of 2^25 and 2^27 points
def test_shockwave_commit_long(hb, logN):
    N, k = 1 << logN, 4
    w = N // k; W = 2 * w
    poly = dev_splitmix(hb, N, 700)
    enc = dev_empty(k * W); lv = torch.empty(64 * W, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hb._chk(hb.lib.hobbit_shockwave_commit(hb.ctx, poly.data_ptr(), N, k, enc.data_ptr(), lv.data_ptr()))
    hb.sync()
    buf = torch.zeros((k, W, 2), dtype=torch.int64, device="cuda")
    buf[:, :w] = poly.view(k, w, 2)
    dev_fft(hb, buf, logN - 1, False, batch=k)
    for i in range(k):
        assert torch.equal(enc.view(k, W, 2)[i], buf[i]), i
    del poly, enc, lv, buf
    torch.cuda.empty_cache()


# ---- 7. the host mirror ------------------------------------------------------------------------------------------------------------------
def test_host_mirror_fft(oracle):
    from __graft_entry__ import PKG, build_host
    build_host()
    lib = ctypes.CDLL(os.path.join(PKG, "libhobbit_host.so"))
    lib.hobbit_host_fft.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    P_ = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for logn, flag in ((13, 1), (16, 0)):
        x = splitmix_field(1 << logn, 800 + logn)
        y = x.copy()
        assert lib.hobbit_host_fft(P_(y), logn, flag) == 0
        assert np.array_equal(y, oracle.fft(x, inverse=bool(flag))), (logn, flag)
    x = np.tile(splitmix_field(1 << 20, 825), (32, 1))
    x[::4097, 1] = 12345                                               # not periodic
    y = x.copy()
    assert lib.hobbit_host_fft(P_(y), 25, 0) == 0
    assert not np.array_equal(y[:4096], x[:4096])
    assert lib.hobbit_host_fft(P_(y), 25, 1) == 0
    assert np.array_equal(y, x)
    assert lib.hobbit_host_fft(P_(y), 29, 0) == -1 and lib.hobbit_host_fft(P_(y), 0, 0) == -1


# ---- 8. refusals, before anything is allocated or launched --------------------------------------------------------------------------------
def test_invalid_arguments_launch_nothing(hb, oracle):
    ln = 1 << 13
    buf = torch.zeros((2 * (ln + 1), 2), dtype=torch.int64, device="cuda")     # even a wrongly accepted (13, batch 2, ld = len + 1) stays inside
    torch.cuda.synchronize()
    hb.profile(True); hb.profile_reset()
    call = lambda logn, batch, ld: hb.lib.hobbit_fft_any(hb.ctx, buf.data_ptr(), logn, batch, ld, 0)
    assert call(0, 1, 1) == EINVAL
    assert call(29, 1, 1 << 29) == EINVAL
    assert call(13, 2, ln + 1) == EINVAL
    assert call(28, 8, 1 << 28) == EINVAL
    hb.sync()
    rep = hb.profile_report()
    hb.profile(False)
    assert sum(c for _, c in rep.values()) == 0, rep
    assert not buf.any()
    r = splitmix_field(5, 900)
    assert np.array_equal(hb.precompute_beta(r), oracle.precompute_beta(r))
