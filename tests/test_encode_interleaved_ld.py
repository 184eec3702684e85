"""hobbit_encode_interleaved_ld (include/hobbit_orion.h): the rows-innermost encode in place on a matrix whose rows are `ld` apart, over its
first `width` messages only, neither a power of two -- against hobbit_encode_interleaved (k_enc_ilv, which needs both equal and a power of
two) and hobbit_encode_batch, bit for bit.

Per code n in {128, 1000, 4096, 8192} and per weight range (the drawn graphs: all weights below 2^32, k_enc_ilv_ld; one weight of C_0 set to
2^32: the general-weight form, k_enc_ilv_ld_fullw): widths {1, 63, 64, 65, len} (below, at and above one wave; the codeword length, the width
the Orion commitment runs), each at ld = width (so width = ld is every case's first), ld = the next power of two and ld = a multiple of 4
that is no power of two.  The matrix starts as a sentinel everywhere but the messages: entries [0, width) of all 2n rows must equal the
reference -- codeword, then zeros -- and entries [width, ld) must still hold the sentinel.  The grid order (strip) must not change a bit.

Everything stays on the device (torch tensors lent to the library by pointer, compared there): at n = 8192 the width-len matrix is 3 GB.
"""
import ctypes

import numpy as np
import pytest
import torch

import adversarial as A

pytestmark = pytest.mark.gpu
SENT = 0x0123456789ABCDEF
CODES = (128, 1000, 4096, 8192)
V, S, L = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_longlong


@pytest.fixture(scope="module")
def hb():
    from __graft_entry__ import load_package
    h = load_package().Hobbit(0)
    yield h
    h.close()


def pow2_at_least(v):
    return 1 << (v - 1).bit_length()


def lds_for(width):
    """ld = width, the next power of two, a multiple of 4 that is no power of two"""
    m4 = (width + 3) // 4 * 4 + 12
    while m4 & (m4 - 1) == 0:
        m4 += 4
    return sorted({width, pow2_at_least(width), m4})


def dev(shape):
    return torch.empty(shape + (2,), dtype=torch.int64, device="cuda")


@pytest.mark.parametrize("fullw", [False, True], ids=["small_weights", "full_range_weights"])
@pytest.mark.parametrize("n", CODES)
def test_strided_encode_equals_the_contiguous_ones(hb, oracle, n, fullw):
    lv = A.drawn_graphs(oracle, n)
    if fullw:
        lv = A._swap(lv, {(0, 0): A._set_weight(lv[(0, 0)], 5, [1 << 32, 0])})
    ln = hb.upload_graphs(n, lv)
    assert hb.encode_forms()["small_weights"] == (not fullw)
    assert n < ln < 2 * n
    R = pow2_at_least(ln)                                                # messages of the reference run: a power of two, as k_enc_ilv needs
    x = dev((n, R))
    hb._chk(hb.lib.hobbit_fill_splitmix(hb.ctx, x.data_ptr(), n * R, 4242 + n))
    fam = A.encode_messages(n, 8, seed=n + 2)                            # the worst cases of the 96-bit sums first
    x[:, :8] = torch.from_numpy(np.ascontiguousarray(fam.transpose(1, 0, 2)).view(np.int64)).cuda()
    ref = dev((2 * n, R)); ref.fill_(SENT)
    hb._chk(hb.lib.hobbit_encode_interleaved(hb.ctx, V(x.data_ptr()), V(ref.data_ptr()), L(n), ctypes.c_uint32(R))); hb.sync()
    assert not bool(ref[ln:].any()) and bool(ref[n:ln].any())
    # the batch encode of the first 65 and the last 3 messages of the widest case
    sel = list(range(65)) + [ln - 3, ln - 2, ln - 1]
    xb = x[:, sel].transpose(0, 1).contiguous(); yb = dev((len(sel), 2 * n)); yb.fill_(SENT)
    hb._chk(hb.lib.hobbit_encode_batch(hb.ctx, V(xb.data_ptr()), V(yb.data_ptr()), L(n), S(len(sel)), S(n), S(2 * n))); hb.sync()
    assert torch.equal(yb.transpose(0, 1), ref[:, sel]), "hobbit_encode_interleaved differs from hobbit_encode_batch"

    names = set()
    for width in (1, 63, 64, 65, ln):
        for ld in lds_for(width):
            for strip in ((None,) if width not in (65, ln) or ld != width else (None, 0, 64, 128, 256)):
                mat = dev((2 * n, ld)); mat.fill_(SENT)
                mat[:n, :width] = x[:, :width]
                hb.profile(True); hb.profile_reset()
                if strip is None:
                    hb._chk(hb.lib.hobbit_encode_interleaved_ld(hb.ctx, V(mat.data_ptr()), L(n), S(width), S(ld)))
                else:
                    hb._chk(hb.lib.hobbit_encode_interleaved_ld_order(hb.ctx, V(mat.data_ptr()), L(n), S(width), S(ld), ctypes.c_uint32(strip)))
                hb.sync(); names |= set(hb.profile_report()); hb.profile(False); hb.profile_reset()
                what = (n, fullw, width, ld, strip)
                assert torch.equal(mat[:, :width], ref[:, :width]), what
                assert bool((mat[:, width:] == SENT).all()), (what, "an entry at or past `width` was written")
                del mat
    assert names == {"k_enc_ilv_ld_fullw" if fullw else "k_enc_ilv_ld", "k_zero_rect"}, names


def test_refusals(hb, oracle):
    mod = hb.__class__
    hb.upload_graphs(128, A.drawn_graphs(oracle, 128))
    mat = dev((256, 64))
    p = V(mat.data_ptr())
    for n, width, ld, strip in ((128, 0, 64, 0), (128, 65, 64, 0), (0, 8, 64, 0), (128, 8, 64, 32), (128, 8, 64, 65)):
        assert hb.lib.hobbit_encode_interleaved_ld_order(hb.ctx, p, L(n), S(width), S(ld), ctypes.c_uint32(strip)) == -2, (n, width, ld, strip)
    assert hb.lib.hobbit_encode_interleaved_ld(hb.ctx, None, L(128), S(8), S(64)) == -2
    assert hb.lib.hobbit_encode_interleaved_ld(hb.ctx, p, L(128), S(1 << 23), S(1 << 23)) == -2          # 2 n width = 2^31
    assert hb.lib.hobbit_encode_interleaved_ld(hb.ctx, p, L(256), S(8), S(64)) == -5                     # graphs finalized for another n
    assert callable(mod.encode_interleaved_ld)
