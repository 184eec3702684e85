"""The ABI's stream contract (include/hobbit_hip.h, Conventions): calls that return nothing to h_* pointers are asynchronous, h_* inputs are
consumed before a call returns, work queued on one context runs in order, and a context may live on a caller's (non-blocking) stream.

The Python wrapper synchronises behind every call, so nothing else in the suite ever has two calls of one context in flight.  Here the calls go
through hb.lib / hb.ctx:

  1. pairs: every asynchronous entry point is issued twice back to back (A, B: different in every input) behind a backlog of unrelated work on
     the same stream, the h_* inputs are overwritten the moment each call returns, and both outputs must equal, bit for bit, those of A and B
     run alone with a sync after each.  What two queued calls of one context share -- pinned staging, the workspaces, the stage arena, the
     buffer pool, side / upload / helper streams, lazily built tables -- is exactly what such a pair breaks when it is not ordered.
  2. a context on a torch stream: ordering against torch's own work in both directions, a whole commit + open, and the stream's survival.
  3. two contexts on one device driven alternately by one host thread: process-global state.
  4. a guard (no GPU): every export of the header is classified, so a new one cannot slip past this file.
"""
import ctypes
import os
import re
import time
import numpy as np
import pytest

from oracle.pyoracle import splitmix_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = (1 << 61) - 1
SEED_A, SEED_B = 1100, 2300

# The backlog: BACKLOG_REPS element-wise products (hobbit_f_binop, op 2) over two 2^24-element buffers, queued in front of every pair so that the
# stream is still busy when B returns -- else the pair would have run one call after the other and tested nothing.
# Measured once on an MI355X (hobbit_timer_begin / hobbit_timer_end_ms around the backlog, time.perf_counter around A; B):
#   the backlog of 1000 products takes 159.5 ms on the device (159.40 .. 159.54 over three runs; 400 products: 62.4 ms);
#   the slowest pair to issue is fft_any-22-inv at 32.4 ms of host time (fft_any-22-fwd: 32.0 ms): a fresh context computes the 2^22 tables
#   on the host.  Every other pair takes the host under 2.1 ms (brakedown_commit-2e16), most under 0.1 ms.
# 159.5 ms >= 4 x 32.4 ms = 129.6 ms.  The `busy` assertion enforces the count from here on.
BACKLOG_REPS = 1000
BACKLOG_N = 1 << 24


# ---- 4. classification guard (runs anywhere) ----------------------------------------------------------------------------------------------------
# has a pair row (or an interleaved-stream / caller's-stream test) below
ASYNC_COVERED = {
    "hobbit_aggregate", "hobbit_eq_table", "hobbit_phi_g", "hobbit_prepare_matrix_cols", "hobbit_fold_axpy", "hobbit_fold_axpy_i32",
    "hobbit_axpy_aggregate", "hobbit_fingerprint_map", "hobbit_fft_any", "hobbit_fft_batch", "hobbit_encode_batch", "hobbit_encode_interleaved",
    "hobbit_tensorcode", "hobbit_commit_standard", "hobbit_commit_standard_host", "hobbit_open_standard", "hobbit_brakedown_commit",
    "hobbit_mt_commit_blake", "hobbit_merkle_levels", "hobbit_blake3_64", "hobbit_hash_md", "hobbit_leaf_chain", "hobbit_inner_digests",
    "hobbit_chain_digests", "hobbit_shockwave_commit", "hobbit_whir_commit", "hobbit_change_form", "hobbit_u64_bias_fold", "hobbit_parity_matrix",
    "hobbit_elastic_begin", "hobbit_elastic_push", "hobbit_elastic_finish", "hobbit_brakedown_stream_begin", "hobbit_brakedown_stream_push",
    "hobbit_brakedown_stream_finish", "hobbit_f_binop", "hobbit_ctx_create_on_stream", "hobbit_tensorcode_chunks",
}
# synchronise by contract: they write to an h_* output (or return when the data has arrived)
HOST_RETURNING = {
    "hobbit_memcpy_h2d", "hobbit_memcpy_d2h", "hobbit_timer_end_ms", "hobbit_merkle_path", "hobbit_merkle_paths", "hobbit_eval_vector",
    "hobbit_commitment_levels", "hobbit_commitment_root", "hobbit_commitment_tensor_row", "hobbit_commitment_gather", "hobbit_commitment_path",
    "hobbit_commitment_paths", "hobbit_brakedown_levels", "hobbit_brakedown_root", "hobbit_brakedown_tensor", "hobbit_brakedown_open",
    "hobbit_brakedown_stream_open_finish", "hobbit_whir_prove", "hobbit_shockwave_prove", "hobbit_tensor_gather", "hobbit_stream_fold",
    "hobbit_open_core", "hobbit_open_from_aggregate", "hobbit_elastic_open_finish", "hobbit_open_standard_rs", "hobbit_sumcheck2",
    "hobbit_sumcheck2_sparse", "hobbit_sumcheck2_eq", "hobbit_gate_sumcheck", "hobbit_sumcheck3", "hobbit_prove_linear_code", "hobbit_prove_fft",
    "hobbit_prove_fft_matrix", "hobbit_batch_3product_sumcheck", "hobbit_mul_tree", "hobbit_compute2p_error_terms", "hobbit_compute3p_error_terms",
    "hobbit_compute4p_error_terms", "hobbit_batch_prod", "hobbit_generate_claims_opt", "hobbit_sumcheck3_stream_batch",
    "hobbit_mul_tree_stream_shallow", "hobbit_gate_consistency_stream", "hobbit_gate_consistency_lookups_stream", "hobbit_sync", "hobbit_encode_forms",
}
EXEMPT = {
    "hobbit_ctx_create": "creates a context; nothing is queued yet",
    "hobbit_ctx_destroy": "waits for the context's streams and frees it",
    "hobbit_last_error": "accessor, host only",
    "hobbit_version": "accessor, host only",
    "hobbit_malloc": "allocation; queues nothing",
    "hobbit_mem_live": "accessor, host only",
    "hobbit_free": "returns a buffer to the pool or waits for the stream before it frees",
    "hobbit_memset": "one hipMemsetAsync with by-value arguments; used by the pair rows' setup",
    "hobbit_timer_begin": "records an event; measured with in this file, nothing shared",
    "hobbit_profile_enable": "switches host-side bookkeeping",
    "hobbit_profile_reset": "host-side bookkeeping",
    "hobbit_profile_get": "host-side bookkeeping, waits for its own events",
    "hobbit_profile_names": "host-side bookkeeping",
    "hobbit_mimc": "host only, no context",
    "hobbit_transcript_record": "host only, thread-local recorder",
    "hobbit_transcript_count": "host only",
    "hobbit_transcript_read": "host only",
    "hobbit_f_mul_host": "host only",
    "hobbit_f_inv_host": "host only",
    "hobbit_generate_randomness": "host only, libc generator",
    "hobbit_graph_reset": "frees the code's device tables after a wait; set-up call, not queued work",
    "hobbit_graph_upload": "set-up call: copies its host arrays before it returns (tests/test_gpu_parity.py uploads and encodes)",
    "hobbit_graph_finalize": "set-up call, returns the length to the host",
    "hobbit_commitment_free": "free function",
    "hobbit_commitment_num_leaves": "accessor",
    "hobbit_commitment_levels_dev": "accessor of a raw device pointer",
    "hobbit_commitment_tensor_dev": "accessor of a raw device pointer",
    "hobbit_brakedown_shape": "host only",
    "hobbit_brakedown_free": "free function",
    "hobbit_brakedown_dims": "accessor",
    "hobbit_brakedown_matrix_dev": "accessor of a raw device pointer",
    "hobbit_brakedown_levels_dev": "accessor of a raw device pointer",
    "hobbit_brakedown_stream_shape": "host only",
    "hobbit_brakedown_stream_device_bytes": "accessor",
    "hobbit_brakedown_stream_free": "free function",
    "hobbit_brakedown_stream_open_begin": "streaming opening, ends in the host-returning open_finish; covered with it in tests/test_brakedown_stream.py",
    "hobbit_brakedown_stream_open_aggregate_push": "streaming opening, see open_begin",
    "hobbit_brakedown_stream_open_reply_push": "streaming opening, see open_begin",
    "hobbit_brakedown_stream_open_device_bytes": "accessor",
    "hobbit_brakedown_stream_open_free": "free function",
    "hobbit_elastic_push_inner": "multi-GPU form of hobbit_elastic_push over the same kernels (tests/test_gpu_parity.py, sharded elastic commit)",
    "hobbit_elastic_free": "free function",
    "hobbit_elastic_open_begin": "streaming opening, ends in the host-returning open_finish",
    "hobbit_elastic_open_begin_lin": "streaming opening, ends in the host-returning open_finish",
    "hobbit_elastic_open_dims": "accessor",
    "hobbit_elastic_open_aggregate_push": "streaming opening, see open_begin",
    "hobbit_elastic_open_aggregate_finish": "streaming opening, see open_begin",
    "hobbit_elastic_open_reply_push": "streaming opening, see open_begin",
    "hobbit_elastic_open_free": "free function",
    "hobbit_leaf_chain_relay": "hobbit_leaf_chain with a slot range and a hand-over state, same kernels; hobbit_leaf_chain has the row",
    "hobbit_verify_path_host": "host only, no context",
    "hobbit_blake3_64_host": "host only, no context",
    "hobbit_read_mul_tree_layer": "callback-driven streaming reader: the source's writes order themselves (hobbit_memcpy_h2d)",
    "hobbit_read_mul_tree_data": "callback-driven streaming reader",
    "hobbit_set_lookups": "copies two elements into the context on the host",
    "hobbit_fill_splitmix": "one launch with by-value arguments; generates this file's inputs and is checked by their use",
}


def test_every_export_is_classified():
    """every function the header declares is in exactly one of ASYNC_COVERED, HOST_RETURNING, EXEMPT -- and nothing is listed that the header lacks"""
    with open(os.path.join(ROOT, "include", "hobbit_hip.h")) as f:
        names = set(m[:-1] for m in re.findall(r"hobbit_[a-z0-9_]+\(", f.read()))
    assert len(names) > 100
    sets = {"ASYNC_COVERED": ASYNC_COVERED, "HOST_RETURNING": HOST_RETURNING, "EXEMPT": set(EXEMPT)}
    for n in sorted(names):
        where = [k for k, s in sets.items() if n in s]
        assert len(where) == 1, "%s is in %s: classify it in tests/test_async_contract.py (and give an asynchronous call a pair row)" % (n, where or "no set")
    for k, s in sets.items():
        assert not (s - names), "%s lists names the header does not declare: %s" % (k, sorted(s - names))
    assert all(isinstance(r, str) and r for r in EXEMPT.values())


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------------
def _mod():
    from __graft_entry__ import load_package
    return load_package()


def F(n, seed):
    return splitmix_field(n, seed)


def rbytes(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def dirty(hb, nbytes):
    """a fresh device buffer pre-filled with a non-zero pattern: what a call does not write must not look like a result"""
    return hb.to_device(np.full(nbytes, 0xC3, np.uint8))


def scramble(*arrs):
    """overwrite host inputs the moment the call that was given them has returned"""
    for a in arrs:
        assert a.flags.c_contiguous and a.flags.writeable
        a.view(np.uint8)[...] = 0xEE


def same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), "%s: output %d differs" % (what, i)


_GRAPHS = {}


def graphs(oracle, n, weight=None):
    """the oracle's graphs for code length n from a fresh generator (optionally every weight set to `weight`), once per shape"""
    from adversarial import graphs_from, set_weights
    if (n, weight) not in _GRAPHS:
        oracle.rng_reset(); oracle.expander_init_store(n)
        lv = graphs_from(oracle, n)
        if weight is not None:
            lv = set_weights(oracle, lv, list(weight))
        _GRAPHS[(n, weight)] = lv
    return _GRAPHS[(n, weight)]


def oracle_graphs(oracle, n, weight=None):
    """put the oracle itself into the state `graphs` describes (its graphs are global)"""
    from adversarial import graphs_from, set_weights
    oracle.rng_reset(); oracle.expander_init_store(n)
    if weight is not None:
        set_weights(oracle, graphs_from(oracle, n), list(weight))


class Call:
    """one ABI call: issue() queues it and scrambles its h_* inputs, read() brings the outputs back (after a sync), want(oracle) is the
    oracle's answer for the same inputs (None: the oracle has no such operation)"""

    def __init__(self, issue, read, want=None, keep=()):
        self.issue, self.read, self.want, self.keep = issue, read, want, keep


class Row:
    def __init__(self, id, a, b, setup=None, fresh=False):
        self.id, self.a, self.b, self.setup, self.fresh = id, a, b, setup, fresh


@pytest.fixture(scope="module")
def ref():
    """the context of the reference runs: its own stream, a sync after every call"""
    h = _mod().Hobbit(0)
    yield h
    h.close()


@pytest.fixture(scope="module")
def stream():
    import torch
    return torch.cuda.Stream()


@pytest.fixture(scope="module")
def hs(stream):
    """the context of the contract runs, bound to a torch stream"""
    h = _mod().Hobbit(0, stream=stream.cuda_stream)
    yield h
    h.close()


@pytest.fixture(scope="module")
def backlog_bufs(ref):
    """two 2^24-element inputs and an output, owned by torch: no context's pool, workspace or arena knows them"""
    import torch
    t = [torch.empty((BACKLOG_N, 2), dtype=torch.int64, device="cuda") for _ in range(3)]
    for i in range(2):
        ref._chk(ref.lib.hobbit_fill_splitmix(ref.ctx, t[i].data_ptr(), BACKLOG_N, 77 + i))
    ref.sync()
    return t


def queue_backlog(hb, bufs, reps=BACKLOG_REPS):
    for _ in range(reps):
        hb._chk(hb.lib.hobbit_f_binop(hb.ctx, 2, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), BACKLOG_N))


HOST_MS = {}
# pairs in which a call may wait for the stream before it queues its work: row id -> what it waits for
MAY_WAIT = {
    "parity_matrix-64-other-size_a": "the CSR form of H^T is rebuilt for another size_a: the call drains the stream before it frees the old tables",
}


def run_pair(row, ref, hs, stream, bufs, oracle):
    """reference run (A, sync, B, sync), then the contract run (backlog, A, B, busy?, sync); both outputs bit for bit"""
    if row.setup:
        row.setup(ref, oracle)
    want = []
    for k, (mk, seed) in enumerate(((row.a, SEED_A), (row.b, SEED_B))):
        c = mk(ref, seed)
        c.issue(); ref.sync()
        want.append(c.read())
        if k == 0 and c.want is not None:
            same(want[0], c.want(oracle), row.id + ": A alone against the oracle")
        del c
    fresh = None
    if row.fresh:                               # lazily built tables are then built inside the unsynchronised pair
        fresh = hs = _mod().Hobbit(0, stream=stream.cuda_stream)
    try:
        import torch
        if row.setup:
            row.setup(hs, oracle)
        if not row.fresh:
            # the shapes once beforehand: a workspace that has to grow waits for the stream before it is freed (that wait is what orders it),
            # and the pair would then run behind an empty stream
            for mk in (row.a, row.b):
                w = mk(hs, SEED_B + 500); w.issue(); hs.sync(); del w
        calls = [row.a(hs, SEED_A), row.b(hs, SEED_B)]
        hs.sync()
        queue_backlog(hs, bufs)
        end_of_backlog = torch.cuda.Event(); end_of_backlog.record(stream)
        t0 = time.perf_counter()
        calls[0].issue(); calls[1].issue()
        HOST_MS[row.id] = (time.perf_counter() - t0) * 1e3
        busy = not stream.query()
        behind = not end_of_backlog.query()     # stronger: neither call waited for the stream, both sit in the queue behind the backlog
        hs.sync()
        got = [c.read() for c in calls]
        print("pair %-40s host %.3f ms busy %s behind-backlog %s" % (row.id, HOST_MS[row.id], busy, behind))
        same(got[0], want[0], row.id + ": A, unsynchronised")
        same(got[1], want[1], row.id + ": B, unsynchronised")
        assert busy, "backlog too short"
        assert behind or row.id in MAY_WAIT, "a call of this pair waited for the stream: asynchronous calls do not (or name the reason in MAY_WAIT)"
        del calls
    finally:
        if fresh is not None:
            fresh.close()


# ---- 1. the rows --------------------------------------------------------------------------------------------------------------------------------
def mk_aggregate(K, M=4096):
    def mk(hb, seed):
        poly, beta = F(K * M, seed), F(K, seed + 1); b0 = beta.copy()
        d, o = hb.to_device(poly), dirty(hb, 16 * M)

        def issue():
            hb._chk(hb.lib.hobbit_aggregate(hb.ctx, d.ptr, K * M, beta.ctypes.data, K, o.ptr)); scramble(beta)
        return Call(issue, lambda: [hb.to_host(o, (M, 2), np.uint64)], lambda orc: [orc.aggregate(poly, b0)], (d, o))
    return mk


def mk_f_binop(n, op):
    def mk(hb, seed):
        a, b = F(n, seed), F(n, seed + 1); da, db, o = hb.to_device(a), hb.to_device(b), dirty(hb, 16 * n)

        def issue():
            hb._chk(hb.lib.hobbit_f_binop(hb.ctx, op, da.ptr, db.ptr, o.ptr, n))
        return Call(issue, lambda: [hb.to_host(o, (n, 2), np.uint64)], lambda orc: [(orc.f_add, orc.f_sub, orc.f_mul)[op](a, b)], (da, db))
    return mk


def mk_tensorcode_chunks(N, K):
    trs = N // (K << 11); M = N // K

    def mk(hb, seed):
        d, t = hb.fill_splitmix(N, seed), dirty(hb, 64 * M * K)

        def issue():
            hb._chk(hb.lib.hobbit_tensorcode_chunks(hb.ctx, d.ptr, M, K, trs, 1, t.ptr))
        return Call(issue, lambda: [hb.to_host(t, (K, 2 * M // trs, 2 * trs, 2), np.uint64)], None, (d,))
    return mk


def mk_eq_table(k):
    def mk(hb, seed):
        r = F(k, seed); r0 = r.copy(); o = dirty(hb, 16 << k)

        def issue():
            hb._chk(hb.lib.hobbit_eq_table(hb.ctx, r.ctypes.data, k, o.ptr)); scramble(r)
        return Call(issue, lambda: [hb.to_host(o, (1 << k, 2), np.uint64)], lambda orc: [orc.precompute_beta(r0)])
    return mk


def mk_phi_g(n, ifft):
    def mk(hb, seed):
        rx, sc = F(n, seed), F(1, seed + 1).reshape(2).copy(); rx0, sc0 = rx.copy(), sc.copy(); o = dirty(hb, 16 << n)

        def issue():
            hb._chk(hb.lib.hobbit_phi_g(hb.ctx, rx.ctypes.data, n, sc.ctypes.data, ifft, o.ptr)); scramble(rx, sc)
        return Call(issue, lambda: [hb.to_host(o, (1 << n, 2), np.uint64)], lambda orc: [orc.phi_g_init(rx0, tuple(int(v) for v in sc0), bool(ifft))])
    return mk


def mk_prepare_matrix_cols(rows, cols, k):
    def mk(hb, seed):
        M, r = F(rows * cols, seed).reshape(rows, cols, 2), F(k, seed + 1); r0 = r.copy()
        d, o = hb.to_device(M), dirty(hb, 16 * cols)

        def issue():
            hb._chk(hb.lib.hobbit_prepare_matrix_cols(hb.ctx, d.ptr, rows, cols, r.ctypes.data, k, o.ptr)); scramble(r)
        # the oracle's prepare_matrix folds along each row of its argument: hand it the transpose
        return Call(issue, lambda: [hb.to_host(o, (cols, 2), np.uint64)], lambda orc: [orc.prepare_matrix(np.ascontiguousarray(M.transpose(1, 0, 2)), r0)], (d,))
    return mk


def _axpy(orc, acc, coeff, v):
    return orc.f_add(acc, orc.f_mul(np.repeat(coeff.reshape(1, 2), v.shape[0], 0), v))


def mk_fold_axpy(n, name):
    def mk(hb, seed):
        fold, buff, c = F(n, seed), F(n, seed + 1), F(1, seed + 2); c0 = c.copy()
        df, db = hb.to_device(fold), hb.to_device(buff)

        def issue():
            if name == "hobbit_fold_axpy":
                hb._chk(hb.lib.hobbit_fold_axpy(hb.ctx, df.ptr, db.ptr, c.ctypes.data, n))
            else:
                hb._chk(hb.lib.hobbit_axpy_aggregate(hb.ctx, db.ptr, c.ctypes.data, df.ptr, n))
            scramble(c)
        return Call(issue, lambda: [hb.to_host(df, (n, 2), np.uint64)], lambda orc: [_axpy(orc, fold, c0, buff)], (db,))
    return mk


def mk_fold_axpy_i32(n, one_minus):
    def mk(hb, seed):
        fold, c = F(n, seed), F(1, seed + 1); c0 = c.copy()
        sel = ((np.arange(n) * (seed % 7 + 3)) % 5 < 2).astype(np.int32)
        df, ds = hb.to_device(fold), hb.to_device(sel)

        def issue():
            hb._chk(hb.lib.hobbit_fold_axpy_i32(hb.ctx, df.ptr, ds.ptr, c.ctypes.data, one_minus, n)); scramble(c)

        def want(orc):
            s = np.zeros((n, 2), np.uint64); s[:, 0] = (1 - sel) if one_minus else sel
            return [_axpy(orc, fold, c0, s)]
        return Call(issue, lambda: [hb.to_host(df, (n, 2), np.uint64)], want, (ds,))
    return mk


def mk_fingerprint_map(n, with_freq):
    def mk(hb, seed):
        addr, value, freq, a, b = F(n, seed), F(n, seed + 1), F(n, seed + 2), F(1, seed + 3), F(1, seed + 4); a0, b0 = a.copy(), b.copy()
        da, dv, df, o = hb.to_device(addr), hb.to_device(value), hb.to_device(freq), dirty(hb, 16 * n)

        def issue():
            hb._chk(hb.lib.hobbit_fingerprint_map(hb.ctx, da.ptr, dv.ptr, df.ptr if with_freq else None, a.ctypes.data, b.ctypes.data, o.ptr, n)); scramble(a, b)

        def want(orc):
            one = np.zeros_like(addr); one[:, 0] = 1
            w = _axpy(orc, orc.f_add(addr, one), a0, value)
            return [_axpy(orc, w, b0, freq) if with_freq else w]
        return Call(issue, lambda: [hb.to_host(o, (n, 2), np.uint64)], want, (da, dv, df))
    return mk


def mk_fft(name, logn, inverse, batch, ld=None):
    n = 1 << logn; ld = ld or n

    def mk(hb, seed):
        d = hb.fill_splitmix(batch * ld, seed)              # the gaps between strided rows hold data too: they must stay as they are
        row0 = hb.to_host(d, (n, 2), np.uint64)

        def issue():
            hb._chk(getattr(hb.lib, name)(hb.ctx, d.ptr, logn, batch, ld, inverse))

        def want(orc):
            w = splitmix_field(batch * ld, seed).reshape(batch, ld, 2)
            for b in range(batch if logn <= 17 else 1):
                w[b, :n] = orc.fft(np.ascontiguousarray(w[b, :n]), inverse=bool(inverse))
            return w
        c = Call(issue, lambda: [hb.to_host(d, (batch, ld, 2), np.uint64)], None)
        if logn <= 17:
            c.want = lambda orc: [want(orc)]
        else:                                               # the first row only: the oracle's transform of three 2^22 rows takes too long
            c.want = None; c.row0_want = lambda orc: orc.fft(row0, inverse=bool(inverse))
        return c
    return mk


def mk_encode_batch(n, batch, in_place):
    def mk(hb, seed):
        src = F(batch * n, seed).reshape(batch, n, 2)
        if in_place:
            buf = np.full((batch, 2 * n, 2), 0x0123456789ABCDEF, np.uint64); buf[:, :n] = src
            dd = hb.to_device(buf); ds, lds = dd, 2 * n
        else:
            ds, dd, lds = hb.to_device(src), dirty(hb, 32 * n * batch), n

        def issue():
            hb._chk(hb.lib.hobbit_encode_batch(hb.ctx, ds.ptr, dd.ptr, n, batch, lds, 2 * n))
        c = Call(issue, lambda: [hb.to_host(dd, (batch, 2 * n, 2), np.uint64)], None, (ds,))
        c.first_want = lambda orc: orc.encode_monolithic(src[0])[0]
        return c
    return mk


def mk_encode_interleaved(n, rows):
    def mk(hb, seed):
        src = F(n * rows, seed).reshape(n, rows, 2)
        ds, dd = hb.to_device(src), dirty(hb, 32 * n * rows)

        def issue():
            hb._chk(hb.lib.hobbit_encode_interleaved(hb.ctx, ds.ptr, dd.ptr, n, rows))
        return Call(issue, lambda: [hb.to_host(dd, (2 * n, rows, 2), np.uint64)],
                    lambda orc: [np.stack([orc.encode_monolithic(np.ascontiguousarray(src[:, i]))[0] for i in range(rows)], 1)], (ds,))
    return mk


def mk_tensorcode(M, trs, lin):
    def mk(hb, seed):
        msg = F(M, seed); cols = 2 * M // trs
        d, o = hb.to_device(msg), dirty(hb, 64 * M)

        def issue():
            hb._chk(hb.lib.hobbit_tensorcode(hb.ctx, d.ptr, M, trs, lin, o.ptr))
        return Call(issue, lambda: [hb.to_host(o, (cols, 2 * trs, 2), np.uint64)],
                    lambda orc: [np.ascontiguousarray(orc.compute_tensorcode(msg, trs, lin).transpose(1, 0, 2))], (d,))
    return mk


def commit_outputs(hb, h, N, K, trs):
    """levels and four tensor rows of a commitment handle, which is freed"""
    c = _mod().Commitment(hb, h, N, K, trs)
    out = [c.levels()] + [c.tensor_row(i, r) for i, r in ((0, 0), (1, trs - 1), (K // 2, trs), (K - 1, 2 * trs - 1))]
    c.free()
    return out


def mk_commit_standard(N, K):
    trs = N // (K << 11)

    def mk(hb, seed):
        d = hb.fill_splitmix(N, seed); h = ctypes.c_void_p()

        def issue():
            hb._chk(hb.lib.hobbit_commit_standard(hb.ctx, d.ptr, N, K, trs, 1, ctypes.byref(h)))
        want = (lambda orc: [orc.commit_standard(splitmix_field(N, seed), K, trs, 1)[0]]) if N <= 1 << 18 else None
        c = Call(issue, lambda: commit_outputs(hb, h, N, K, trs), None, (d,))
        c.levels_want = want
        return c
    return mk


def mk_brakedown_commit(N, quirk):
    def mk(hb, seed):
        d = hb.fill_splitmix(N, seed); h = ctypes.c_void_p()

        def issue():
            hb._chk(hb.lib.hobbit_brakedown_commit(hb.ctx, d.ptr, N, quirk, ctypes.byref(h)))

        def read():
            c = _mod().BrakedownCommitment(hb, h, N)
            out = [c.levels(), c.tensor()]
            c.free()
            return out
        return Call(issue, read, None, (d,))
    return mk


def mk_mt_commit_blake(leaves):
    def mk(hb, seed):
        x = F(4 * leaves, seed); d, lv = hb.to_device(x), dirty(hb, 64 * leaves)

        def issue():
            hb._chk(hb.lib.hobbit_mt_commit_blake(hb.ctx, d.ptr, 4 * leaves, lv.ptr))
        return Call(issue, lambda: [hb.to_host(lv, (2 * leaves - 1, 32), np.uint8)], lambda orc: [orc.mt_commit_blake(x)], (d,))
    return mk


def mk_merkle_levels(n, quirk):
    def mk(hb, seed):
        buf = np.full((2 * n, 32), 0xC3, np.uint8); buf[:n] = rbytes((n, 32), seed); l0 = buf[:n].copy()
        lv = hb.to_device(buf)

        def issue():
            hb._chk(hb.lib.hobbit_merkle_levels(hb.ctx, lv.ptr, n, quirk))
        return Call(issue, lambda: [hb.to_host(lv, (2 * n - 1, 32), np.uint8)], (lambda orc: [orc.create_tree_blake(l0)]) if quirk else None)
    return mk


def mk_blake3_64(n):
    def mk(hb, seed):
        blocks = rbytes((n, 64), seed); d, o = hb.to_device(blocks), dirty(hb, 32 * n)

        def issue():
            hb._chk(hb.lib.hobbit_blake3_64(hb.ctx, d.ptr, o.ptr, n))
        return Call(issue, lambda: [hb.to_host(o, (n, 32), np.uint8)], lambda orc: [orc.blake3_64(blocks)], (d,))
    return mk


def mk_hash_md(n):
    def mk(hb, seed):
        x, prev = F(4 * n, seed).reshape(n, 4, 2), rbytes((n, 32), seed + 1)
        dx, dp, o = hb.to_device(x), hb.to_device(prev), dirty(hb, 32 * n)

        def issue():
            hb._chk(hb.lib.hobbit_hash_md(hb.ctx, dx.ptr, dp.ptr, o.ptr, n))
        return Call(issue, lambda: [hb.to_host(o, (n, 32), np.uint8)], lambda orc: [orc.hash_md(x, prev)], (dx, dp))
    return mk


def mk_leaf_chains(N, K, two_step):
    """hobbit_leaf_chain, or hobbit_inner_digests followed by hobbit_chain_digests, over the tensor of test_survey_named_exports, on top of
    leaves that already hold something"""
    trs = N // (K << 11); M = N // K

    def mk(hb, seed):
        d = hb.fill_splitmix(N, seed)
        t = hb.alloc(64 * M * K)
        hb._chk(hb.lib.hobbit_tensorcode_chunks(hb.ctx, d.ptr, M, K, trs, 1, t.ptr))
        lv = hb.to_device(rbytes((M, 32), seed + 1))            # (hobbit_memcpy_h2d waits for the tensor)
        dig = dirty(hb, 32 * M * K) if two_step else None

        def issue():
            if two_step:
                hb._chk(hb.lib.hobbit_inner_digests(hb.ctx, t.ptr, M, K, trs, dig.ptr))
                hb._chk(hb.lib.hobbit_chain_digests(hb.ctx, dig.ptr, 32 * M, K, M, lv.ptr))
            else:
                hb._chk(hb.lib.hobbit_leaf_chain(hb.ctx, t.ptr, M, K, trs, 1, lv.ptr))
        return Call(issue, lambda: [hb.to_host(lv, (M, 32), np.uint8)] + ([hb.to_host(dig, (K * M, 32), np.uint8)] if two_step else []), None, (d, t))
    return mk


def mk_shockwave_commit(N, k):
    W = 2 * N // k

    def mk(hb, seed):
        poly = F(N, seed); d, enc, lv = hb.to_device(poly), dirty(hb, 16 * k * W), dirty(hb, 64 * W)

        def issue():
            hb._chk(hb.lib.hobbit_shockwave_commit(hb.ctx, d.ptr, N, k, enc.ptr, lv.ptr))
        return Call(issue, lambda: [hb.to_host(enc, (k, W, 2), np.uint64), hb.to_host(lv, (2 * W - 1, 32), np.uint8)],
                    lambda orc: list(orc.shockwave_commit(poly, k)), (d,))
    return mk


def mk_whir_commit(N):
    def mk(hb, seed):
        poly = F(N, seed); d, com, lv = hb.to_device(poly), dirty(hb, 32 * N), dirty(hb, 32 * N)

        def issue():
            hb._chk(hb.lib.hobbit_whir_commit(hb.ctx, d.ptr, N, com.ptr, lv.ptr))
        return Call(issue, lambda: [hb.to_host(com, (2 * N, 2), np.uint64), hb.to_host(lv, (N - 1, 32), np.uint8)],
                    lambda orc: list(orc.whir_commit(poly)), (d,))
    return mk


def mk_change_form(logn):
    def mk(hb, seed):
        poly = F(1 << logn, seed); d = hb.to_device(poly)

        def issue():
            hb._chk(hb.lib.hobbit_change_form(hb.ctx, d.ptr, logn))
        return Call(issue, lambda: [hb.to_host(d, (1 << logn, 2), np.uint64)], lambda orc: [orc.change_form(poly)])
    return mk


def mk_u64_bias_fold(n, fold):
    def mk(hb, seed):
        rng = np.random.default_rng(seed)
        w = rng.integers(0, 1 << 62, n, dtype=np.uint64); bias = int(rng.integers(1, 1 << 61))      # w + bias < 2^63: no wrap-around
        d = hb.to_device(w)

        def issue():
            hb._chk(hb.lib.hobbit_u64_bias_fold(hb.ctx, d.ptr, n, ctypes.c_uint64(bias), fold))
        want = np.array([(int(x) + bias) % P if fold else int(x) + bias for x in w], np.uint64)
        return Call(issue, lambda: [hb.to_host(d, (n,), np.uint64)], lambda orc: [want])
    return mk


def mk_parity_matrix(n, size_a):
    def mk(hb, seed):
        beta = F(size_a, seed); d, o = hb.to_device(beta), dirty(hb, 16 * size_a)

        def issue():
            hb._chk(hb.lib.hobbit_parity_matrix(hb.ctx, d.ptr, size_a, n, o.ptr))
        return Call(issue, lambda: [hb.to_host(o, (size_a, 2), np.uint64)], lambda orc: [orc.evaluate_parity_matrix(beta, n)[0]], (d,))
    return mk


def code_setup(n, weight=None):
    def setup(hb, oracle):
        hb.upload_graphs(n, graphs(oracle, n, weight))
        oracle_graphs(oracle, n, weight)
    return setup


def _fft_rows():
    out = []
    for logn in (12, 13, 17, 22):
        for inv in (0, 1):
            out.append(Row("fft_any-%d-%s" % (logn, "inv" if inv else "fwd"), mk_fft("hobbit_fft_any", logn, inv, 3), mk_fft("hobbit_fft_any", logn, inv, 3), fresh=True))
    return out


ROWS = [
    Row("aggregate-K32", mk_aggregate(32), mk_aggregate(32)),
    Row("aggregate-K128", mk_aggregate(128), mk_aggregate(128)),
    Row("aggregate-K128-then-K32", mk_aggregate(128), mk_aggregate(32)),
    Row("f_binop-5000-mul-then-sub", mk_f_binop(5000, 2), mk_f_binop(5000, 1)),
    Row("tensorcode_chunks-2e18", mk_tensorcode_chunks(1 << 18, 32), mk_tensorcode_chunks(1 << 18, 32), code_setup(4)),
    Row("eq_table-13", mk_eq_table(13), mk_eq_table(13)),
    Row("eq_table-14", mk_eq_table(14), mk_eq_table(14)),
    Row("phi_g-13-fwd-then-inv", mk_phi_g(13, 0), mk_phi_g(13, 1)),
    Row("phi_g-13-inv-then-fwd", mk_phi_g(13, 1), mk_phi_g(13, 0)),
    Row("prepare_matrix_cols-64x256", mk_prepare_matrix_cols(64, 256, 6), mk_prepare_matrix_cols(64, 256, 6)),
    Row("fold_axpy-5000", mk_fold_axpy(5000, "hobbit_fold_axpy"), mk_fold_axpy(5000, "hobbit_fold_axpy")),
    Row("fold_axpy_i32-5000", mk_fold_axpy_i32(5000, 0), mk_fold_axpy_i32(5000, 1)),
    Row("axpy_aggregate-5000", mk_fold_axpy(5000, "hobbit_axpy_aggregate"), mk_fold_axpy(5000, "hobbit_axpy_aggregate")),
    Row("fingerprint_map-5000", mk_fingerprint_map(5000, 1), mk_fingerprint_map(5000, 0)),
] + _fft_rows() + [
    Row("fft_batch-12-strided", mk_fft("hobbit_fft_batch", 12, 0, 3, 4096 + 64), mk_fft("hobbit_fft_batch", 12, 1, 3, 4096 + 64), fresh=True),
    Row("encode_batch-4096-in-place-x300", mk_encode_batch(4096, 300, True), mk_encode_batch(4096, 300, True), code_setup(4096)),
    Row("encode_batch-3000", mk_encode_batch(3000, 3, False), mk_encode_batch(3000, 3, False), code_setup(3000)),
    Row("encode_interleaved-4096x4", mk_encode_interleaved(4096, 4), mk_encode_interleaved(4096, 4), code_setup(4096)),
    Row("tensorcode-64-expander", mk_tensorcode(1 << 17, 64, 1), mk_tensorcode(1 << 17, 64, 1), code_setup(64)),
    Row("tensorcode-64-rs", mk_tensorcode(1 << 17, 64, 0), mk_tensorcode(1 << 17, 64, 0)),
    Row("commit_standard-2e18", mk_commit_standard(1 << 18, 32), mk_commit_standard(1 << 18, 32), code_setup(4)),
    Row("commit_standard-2e22-piped", mk_commit_standard(1 << 22, 32), mk_commit_standard(1 << 22, 32), code_setup(64)),
    Row("brakedown_commit-2e16", mk_brakedown_commit(1 << 16, 1), mk_brakedown_commit(1 << 16, 0), code_setup(1 << 14)),
    Row("mt_commit_blake-1024", mk_mt_commit_blake(1024), mk_mt_commit_blake(1024)),
    Row("merkle_levels-1024", mk_merkle_levels(1024, 1), mk_merkle_levels(1024, 0)),
    Row("blake3_64-1024", mk_blake3_64(1024), mk_blake3_64(1024)),
    Row("hash_md-1024", mk_hash_md(1024), mk_hash_md(1024)),
    Row("leaf_chain-2e18", mk_leaf_chains(1 << 18, 32, False), mk_leaf_chains(1 << 18, 32, False), code_setup(4)),
    Row("inner_digests+chain_digests-2e18", mk_leaf_chains(1 << 18, 32, True), mk_leaf_chains(1 << 18, 32, True), code_setup(4)),
    Row("shockwave_commit-2e16", mk_shockwave_commit(1 << 16, 32), mk_shockwave_commit(1 << 16, 32)),
    Row("whir_commit-2e13", mk_whir_commit(1 << 13), mk_whir_commit(1 << 13)),
    Row("change_form-13", mk_change_form(13), mk_change_form(13)),
    Row("u64_bias_fold-add-then-fold", mk_u64_bias_fold(4096, 0), mk_u64_bias_fold(4096, 1)),
    Row("u64_bias_fold-fold-then-add", mk_u64_bias_fold(4096, 1), mk_u64_bias_fold(4096, 0)),
    Row("parity_matrix-64", mk_parity_matrix(64, 128), mk_parity_matrix(64, 128), code_setup(64)),
    Row("parity_matrix-64-other-size_a", mk_parity_matrix(64, 128), mk_parity_matrix(64, 256), code_setup(64)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=[r.id for r in ROWS])
def test_pair(row, ref, hs, stream, backlog_bufs, oracle):
    run_pair(row, ref, hs, stream, backlog_bufs, oracle)


PARTIAL = {
    "encode_batch-4096-in-place-x300": (code_setup(4096), mk_encode_batch(4096, 300, True), lambda c, out, orc: (out[0][0], c.first_want(orc))),
    "encode_batch-3000": (code_setup(3000), mk_encode_batch(3000, 3, False), lambda c, out, orc: (out[0][0], c.first_want(orc))),
    "fft_any-22-fwd": (None, mk_fft("hobbit_fft_any", 22, 0, 3), lambda c, out, orc: (out[0][0], c.row0_want(orc))),
    "fft_any-22-inv": (None, mk_fft("hobbit_fft_any", 22, 1, 3), lambda c, out, orc: (out[0][0], c.row0_want(orc))),
    "commit_standard-2e18": (code_setup(4), mk_commit_standard(1 << 18, 32), lambda c, out, orc: (out[0], c.levels_want(orc)[0])),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PARTIAL))
def test_pair_partial_oracle_checks(name, ref, oracle):
    """the rows whose oracle answer covers only part of the output (a first message, a first row, the levels): A alone against it"""
    setup, mk, pick = PARTIAL[name]
    if setup:
        setup(ref, oracle)
    c = mk(ref, SEED_A); c.issue(); ref.sync()
    got, want = pick(c, c.read(), oracle)
    assert np.array_equal(got, want)


# ---- commit, then the opening queued behind it ---------------------------------------------------------------------------------------------------
OPEN_KEYS = ("I", "scalars", "poly", "r", "vr", "fin", "roots", "reply", "paths", "checks")
SP_KEYS = ("I", "q1", "r1", "vr1", "fin1", "q2", "r2", "vr2", "fin2", "iters", "wq", "wa", "wroots", "wscal", "wchecks", "whir_root",
           "reply", "paths", "qn", "qidx", "qreply", "qpaths", "final_pb")
OPEN_N, OPEN_K, OPEN_Q = 1 << 20, 32, 5900
OPEN_TRS = OPEN_N // (OPEN_K << 11)


def same_opening(got, want, what):
    for k in OPEN_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k)
    for sp in ("sp_c", "sp_f"):
        for k in SP_KEYS:
            assert np.array_equal(got[sp][k], want[sp][k]), (what, sp, k)


def commit_and_open(hb, d, x, sync_between, before_open=None):
    """hobbit_commit_standard, then hobbit_open_standard; returns (levels, opening)"""
    libc = ctypes.CDLL(None)
    c = hb.commit_standard((d, OPEN_N), OPEN_K, OPEN_TRS, 1, sync=sync_between)
    if before_open is not None:
        before_open()
    xx = x.copy()
    libc.srandom(777); g = hb.open_standard((d, OPEN_N), c, xx, OPEN_Q)
    lv = c.levels(); c.free()
    return lv, g


@pytest.fixture(scope="module")
def opening(ref, oracle):
    """the own-stream context's commit (sync) + open at N = 2^20, K = 32, checked against the oracle once and shared"""
    libc = ctypes.CDLL(None)
    poly = splitmix_field(OPEN_N, 4242); x = splitmix_field(20, 4243)
    ref.upload_graphs(OPEN_TRS, graphs(oracle, OPEN_TRS)); oracle_graphs(oracle, OPEN_TRS)
    d = ref.to_device(poly)
    lv, g = commit_and_open(ref, d, x, True)
    wl, T = oracle.commit_standard(poly, OPEN_K, OPEN_TRS, 1, want_tensor=True)
    libc.srandom(777); w = oracle.open_standard(poly, OPEN_K, OPEN_TRS, x, OPEN_Q, tensor=T)
    assert np.array_equal(lv, wl)
    assert g["checks"].tolist() == [1, 1, 1] and w["checks"].tolist() == [1, 1, 1]
    for k in ("I", "scalars", "poly", "r", "vr", "fin", "roots", "reply"):
        assert np.array_equal(g[k], w[k]), k
    for sp in ("sp_c", "sp_f"):
        for k in SP_KEYS:
            assert np.array_equal(g[sp][k], w[sp][k]), (sp, k)
    return dict(poly=poly, x=x, levels=lv, open=g)


@pytest.mark.gpu
def test_open_queued_behind_commit(opening, hs, stream, backlog_bufs, oracle):
    """hobbit_open_standard issued the moment hobbit_commit_standard returned, the commit still queued behind the backlog.  The opening returns to
    the host, so the stream has drained when it comes back: `busy` is read between the two calls."""
    hs.upload_graphs(OPEN_TRS, graphs(oracle, OPEN_TRS))
    d = hs.to_device(opening["poly"])
    hs.sync(); queue_backlog(hs, backlog_bufs)
    busy = []
    lv, g = commit_and_open(hs, d, opening["x"], False, lambda: busy.append(not stream.query()))
    assert np.array_equal(lv, opening["levels"])
    same_opening(g, opening["open"], "open behind commit")
    assert busy[0], "backlog too short"


# ---- host commit twice: races on the upload stream, not the main one -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("logN", [22, 24])
def test_commit_standard_host_twice(logN, ref, hs, oracle):
    """two hobbit_commit_standard_host calls without a sync between them: the second refills the pinned staging pieces while the first call's last
    pieces may still be on the bus.  Each against hobbit_commit_standard of the same polynomial from device memory: the levels, and all of the
    d_poly it leaves behind.  (2^22: eight groups of 8 MiB, both staging pieces in use when the call returns; 2^24: eight groups of 32 MiB.)"""
    N, K = 1 << logN, 32; trs = N // (K << 11)
    for h in (ref, hs):
        h.upload_graphs(trs, graphs(oracle, trs))
    want, polys = [], []
    for seed in (SEED_A, SEED_B):
        d = ref.fill_splitmix(N, seed)
        c = ref.commit_standard((d, N), K, trs, 1)
        want.append(c.levels()); c.free()
        polys.append(ref.to_host(d, (N, 2), np.uint64))       # pageable, and the device generator is the host's (test_device_splitmix_matches_host)
        d.free()
    keep = [p.copy() for p in polys]
    dps = [hs.alloc(16 * N) for _ in range(2)]
    hs_ = [ctypes.c_void_p(), ctypes.c_void_p()]
    for i in range(2):
        hs._chk(hs.lib.hobbit_commit_standard_host(hs.ctx, polys[i].ctypes.data, dps[i].ptr, N, K, trs, 1, ctypes.byref(hs_[i])))
        scramble(polys[i])
    hs.sync()
    for i in range(2):
        c = _mod().Commitment(hs, hs_[i], N, K, trs)
        got = c.levels(); c.free()
        assert np.array_equal(hs.to_host(dps[i], (N, 2), np.uint64), keep[i]), "d_poly of call %d" % i
        assert np.array_equal(got, want[i]), "levels of call %d" % i


# ---- interleaved streaming objects ---------------------------------------------------------------------------------------------------------------
STREAM_B = 1 << 13


def _stream_commit(hb, kind, chunk_ptrs_a, chunk_ptrs_b, interleave, stream=None):
    """two streaming commits over eight chunks each on one context: A alone then B alone, or A, B, A, B, ...; returns their flat levels"""
    B = STREAM_B; lib = hb.lib
    nlev = (8 * B - 1) if kind == "elastic" else (4 * B - 1)

    def begin():
        h = ctypes.c_void_p()
        if kind == "elastic":
            hb._chk(lib.hobbit_elastic_begin(hb.ctx, B, B >> 11, 0, 1, ctypes.byref(h)))
        else:
            hb._chk(lib.hobbit_brakedown_stream_begin(hb.ctx, B, 1, ctypes.byref(h)))
        return h

    def push(h, p):
        hb._chk((lib.hobbit_elastic_push if kind == "elastic" else lib.hobbit_brakedown_stream_push)(hb.ctx, h, p))

    def finish(h, lv):
        if kind == "elastic":
            hb._chk(lib.hobbit_elastic_finish(hb.ctx, h, lv.ptr))
        else:
            hb._chk(lib.hobbit_brakedown_stream_finish(hb.ctx, h, 1, lv.ptr))

    free = lib.hobbit_elastic_free if kind == "elastic" else lib.hobbit_brakedown_stream_free
    lvs = [dirty(hb, 32 * (nlev + 1)) for _ in range(2)]
    if interleave:
        ha, hb_ = begin(), begin()
        for pa, pb in zip(chunk_ptrs_a, chunk_ptrs_b):
            push(ha, pa); push(hb_, pb)
        finish(ha, lvs[0]); finish(hb_, lvs[1])
        busy = not stream.query()
        hb.sync(); free(ha); free(hb_)
        assert busy, "backlog too short"
    else:
        for ptrs, lv in zip((chunk_ptrs_a, chunk_ptrs_b), lvs):
            h = begin()
            for p in ptrs:
                push(h, p)
            finish(h, lv); hb.sync(); free(h)
    return [hb.to_host(lv, (nlev, 32), np.uint8) for lv in lvs]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["elastic", "brakedown_stream"])
def test_interleaved_streaming_commits(kind, hs, stream, backlog_bufs, oracle):
    """two streaming commits alive on one context, their pushes alternating over eight distinct chunks each, no sync until both have finished:
    levels (the leaves first) equal those of each stream run alone"""
    B = STREAM_B
    if kind == "brakedown_stream":
        hs.upload_graphs(B, graphs(oracle, B))
    chunks = [[hs.fill_splitmix(B, 9000 + 100 * s + i) for i in range(8)] for s in range(2)]
    ptrs = [[c.ptr for c in cs] for cs in chunks]
    hs.sync()
    want = _stream_commit(hs, kind, ptrs[0], ptrs[1], False)
    assert not np.array_equal(want[0], want[1])
    hs.sync(); queue_backlog(hs, backlog_bufs)
    got = _stream_commit(hs, kind, ptrs[0], ptrs[1], True, stream)
    nleaf = (4 if kind == "elastic" else 2) * B
    for i in range(2):
        assert np.array_equal(got[i][:nleaf], want[i][:nleaf]), "leaves of stream %d" % i
        assert np.array_equal(got[i], want[i]), "levels of stream %d" % i


# ---- 2. a context on the caller's stream --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("logn", [17, 22])
def test_ordering_against_torch_work(logn, ref, hs, stream, backlog_bufs, oracle):
    """torch producer -> hobbit_fft_any -> torch consumer on one stream with no sync until the end: had the library run anywhere else, it would
    have read x before the copy, or torch would have cloned x before the transform"""
    import torch
    n = 1 << logn
    src_h = splitmix_field(n, 5150 + logn)
    want = oracle.fft(src_h) if logn == 17 else ref.fft_any(src_h)
    src = torch.from_numpy(src_h.view(np.int64)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        x = torch.full((n, 2), 0x3C3C3C3C, dtype=torch.int64, device="cuda")
        stream.synchronize()
        queue_backlog(hs, backlog_bufs)
        x.copy_(src, non_blocking=True)
        hs._chk(hs.lib.hobbit_fft_any(hs.ctx, x.data_ptr(), logn, 1, n, 0))
        y = x.clone()
        busy = not stream.query()
        stream.synchronize()
    assert np.array_equal(y.cpu().numpy().view(np.uint64), want)
    assert busy, "backlog too short"


@pytest.mark.gpu
def test_commit_and_open_on_callers_stream(opening, hs, oracle):
    """the whole commit + open on a torch stream (side stream, upload stream and both helper contexts joined to a non-blocking base stream) gives
    the own-stream context's bits"""
    hs.upload_graphs(OPEN_TRS, graphs(oracle, OPEN_TRS))
    d = hs.to_device(opening["poly"])
    lv, g = commit_and_open(hs, d, opening["x"], True)
    assert np.array_equal(lv, opening["levels"])
    same_opening(g, opening["open"], "caller's stream")


@pytest.mark.gpu
def test_commit_standard_host_on_callers_stream(ref, hs, oracle):
    N, K = 1 << 22, 32; trs = N // (K << 11)
    poly = splitmix_field(N, 6160)
    out = []
    for h in (ref, hs):
        h.upload_graphs(trs, graphs(oracle, trs))
        c, d = h.commit_standard_host(poly, K, trs, 1)
        out.append((c.levels(), h.to_host(d, (N, 2), np.uint64))); c.free()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[1][1], poly) and np.array_equal(out[0][1], poly)


@pytest.mark.gpu
def test_caller_keeps_the_stream():
    """hobbit_ctx_destroy leaves a caller's stream alone: torch work queued on it afterwards runs and gives the right bytes"""
    import torch
    s = torch.cuda.Stream()
    hb = _mod().Hobbit(0, stream=s.cuda_stream)
    a = splitmix_field(4096, 7); b = hb.fft_any(a); assert b.shape == a.shape
    hb.close()
    src = torch.arange(1 << 16, dtype=torch.int64, device="cuda"); torch.cuda.synchronize()
    with torch.cuda.stream(s):
        dst = torch.zeros_like(src); dst.copy_(src, non_blocking=True)
        s.synchronize()
    assert torch.equal(dst.cpu(), torch.arange(1 << 16, dtype=torch.int64))


# ---- 3. two contexts on one device, one host thread ----------------------------------------------------------------------------------------------
def _two_ctx_calls(hb, n_code, seed, inverse):
    """the calls one context makes in the alternation: encode, fft_any at 2^13, eq_table; returns Call objects (inputs ready, nothing queued)"""
    return [mk_encode_batch(n_code, 3, False)(hb, seed), mk_fft("hobbit_fft_any", 13, inverse, 1)(hb, seed + 10), mk_eq_table(13)(hb, seed + 20)]


@pytest.mark.gpu
def test_two_contexts_alternating(oracle):
    """context 1 (graphs for n = 4096) and context 2 (n = 3000, every weight 2^32 - 1), each on its own stream, called alternately without a sync:
    each result equals the same context run alone.  Catches process-global state: statics in csrc/, kernel attributes, tables cached outside
    the context."""
    mod = _mod()
    W = ((1 << 32) - 1, 0)

    def contexts():
        c1, c2 = mod.Hobbit(0), mod.Hobbit(0)
        c1.upload_graphs(4096, graphs(oracle, 4096)); c2.upload_graphs(3000, graphs(oracle, 3000, W))
        return c1, c2
    want = []
    for which in (0, 1):                                   # each context alone, in a process state where the other has made no call yet
        cs = contexts()
        calls = _two_ctx_calls(cs[which], (4096, 3000)[which], 31 + 50 * which, which)
        outs = []
        for c in calls:
            c.issue(); cs[which].sync(); outs.append(c.read())
        want.append(outs)
        del calls
        cs[0].close(); cs[1].close()
    c1, c2 = contexts()
    k1, k2 = _two_ctx_calls(c1, 4096, 31, 0), _two_ctx_calls(c2, 3000, 81, 1)
    c1.sync(); c2.sync()
    for a, b in zip(k1, k2):
        a.issue(); b.issue()
    c1.sync(); c2.sync()
    for i in range(3):
        same(k1[i].read(), want[0][i], "context 1, call %d" % i)
        same(k2[i].read(), want[1][i], "context 2, call %d" % i)
    oracle_graphs(oracle, 3000, W)
    assert np.array_equal(want[1][0][0][0], k2[0].first_want(oracle))
    del k1, k2
    c1.close(); c2.close()
