// hobbit_ctx.hpp -- context object behind the C ABI (include/hobbit_hip.h): device, stream,
// error string, per-kernel HIP-event profiler, cached twiddle tables and the uploaded expander
// graphs in their device (gather / sliced-ELL) form.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <tuple>
#include <vector>
#include "hobbit_field.hpp"
#include "hobbit_mem.hpp"
#include "../../include/hobbit_hip.h"
#include "../../include/hobbit_parity.h"

namespace hobbit {

// One SpMV step of the recursive expander encode, in gather form over the codeword buffer:
//   cw[out_off + t] = sum_e w_e * cw[in_off + idx_e],  t in [0, out_len)
// Outputs are ordered by in-degree and cut into slices of ENC_SW; a slice stores its edges k-major
// (edge k of its l-th output at slice_ptr + k*ENC_SW + l), padded with zero-weight records to a
// multiple of ENC_SPLIT past the slice's widest row (sorting keeps that within ~10 % of the real
// edge count: 76 288 records for the 69 084 edges of n = 4096, against 124 928 unsorted), so a
// wavefront reads 64 consecutive records per instruction and needs no per-lane bounds.
// slice_out maps (slice, l) back to the output index (0xFFFFFFFF = padding lane).
// slice geometry shared by the host preprocessing and k_encode (see hobbit_kernels.hip)
static constexpr uint32_t ENC_SW = 16;                 // outputs per slice
static constexpr uint32_t ENC_SPLIT = 64 / ENC_SW;     // lane groups sharing one output's edges
static constexpr uint32_t ENC_UNROLL = 4;              // edge records in flight per lane

struct EncStep {
    uint32_t in_off, out_off, out_len, n_slices;
    uint32_t slice_base;   // index of this step's first slice in slice_ptr/slice_width
    uint32_t sw;           // outputs per slice of this step: 64 (one output per lane, no cross-lane combine) for the wide steps,
                           // ENC_SW (lane groups share an output) for the narrow ones, where a slice per wave would leave waves idle
    uint32_t out_base;     // index of this step's first entry in slice_out (sw entries per slice)
};
static constexpr uint32_t ENC_WIDE_MIN = 128;          // steps with at least this many outputs use sw = 64 (one fold per lane and no cross-lane
                                                       // combine: the narrow form's per-slice fold + shuffles cost more than its shorter rows save --
                                                       // middle pass at 2^28: 2.61 ms at 512, 2.36 at 256, 2.28 at 128, 2.46 at 32)

struct HostGraph {          // one uploaded level (src/expanders.h:7-16)
    long long L = 0, R = 0;
    int degree = 0;
    std::vector<long long> nbr;
    std::vector<F> w;
};

// One WIDE SpMV step in "fat" form for the persistent encode kernels (hobbit_kernels.hip, k_enc_fat): a workgroup stays on its CU for the
// whole launch and walks the columns; every lane of its consumer waves owns the same number of outputs of the step for good, and the edge
// records of those outputs -- 32-bit weight, 16-bit byte offset of the input inside the step's window -- live in REGISTERS, loaded once per
// launch (position j of a lane has cap[j] register slots; a wave uses the first w[wave][j] of them, a multiple of 4; unused slots have
// weight 0).  Outputs are dealt to lanes in order of in-degree, serpentine over the positions, so that a lane's heavy output is paired
// with a light one.  Built by hobbit_graph_finalize when the step's degrees fit the caps the kernel was compiled for.
struct FatStep {
    bool ok = false;
    uint32_t in_off = 0, in_len = 0, out_off = 0, out_len = 0;
    mem::Buf<uint32_t> d_wt, d_ot, d_oidx, d_w;
};
// outputs per lane, consumer waves, register slots per position, workgroups per launch
static constexpr uint32_t FAT_A_NOUT = 2, FAT_A_CONS = 7, FAT_A_CAP0 = 72, FAT_A_CAP1 = 48, FAT_A_WGS = 256;          // C_0 of n = 4096: 864 outputs, in-degree 42.7 +- 6.5
static constexpr uint32_t FAT_C1_NOUT = 1, FAT_C1_CONS = 3, FAT_C1_CAP0 = 64, FAT_C1_WGS = 768;                       // C_1: 182 outputs, in-degree 42.7 (max ~62): three waves, a few workgroups per CU
static constexpr uint32_t FAT_D_NOUT = 3, FAT_D_CONS = 8, FAT_D_CAP0 = 28, FAT_D_CAP1 = 16, FAT_D_CAP2 = 12, FAT_D_WGS = 256;   // D_0: 1463 outputs, in-degree 12.2 +- 3.5

// The five NARROW steps C_2, C_3, D_3, D_2, D_1 of n = 4096 for the persistent one-wave-per-column kernel (hobbit_kernels.hip, k_enc_narrow):
// 6 612 edges on the 622-element window [x_2 .. z_1].  A step is a run of POSITIONS; in a position a lane works for one output, NARROW_LPO
// lanes share an output (lane = t * LPO + g: output t of the position, edges g, g + LPO, ... of it) and combine after one fold each; the
// position's outputs are the next 64 / LPO of the step in order of in-degree, heaviest first, and every lane has NARROW_CAP register slots
// for its share of the edges (weight 0 past the end).  The tables are the cheapest cover of the libc-drawn graphs' degrees (slots + about
// three per fold + one per combine round): 136 slots for the 103.3 edges per lane.  A record is the 32-bit weight (one register) and the
// input's place in the window: for the first four steps an 8-bit element index relative to the step's input (four to a register), for D_1
// a 16-bit byte offset (two to a register).  Built by hobbit_graph_finalize when the code has this shape and the degrees fit.
static constexpr uint32_t NARROW_STEPS = 5, NARROW_POS = 12;
static constexpr uint32_t NARROW_L[NARROW_STEPS] = {182, 38, 8, 65, 313}, NARROW_R[NARROW_STEPS] = {38, 8, 19, 66, 309};   // inputs / outputs per step
static constexpr uint32_t NARROW_IN[NARROW_STEPS] = {0, 182, 220, 182, 0}, NARROW_OUT[NARROW_STEPS] = {182, 220, 228, 247, 313};   // first input / output, window-relative
static constexpr uint32_t NARROW_WIN = 622, NARROW_X2 = 182;             // the window, and its head x_2 that the launch reads from the column
static constexpr uint32_t NARROW_STEP_OF[NARROW_POS] = {0, 0, 1, 2, 3, 3, 4, 4, 4, 4, 4, 4};
static constexpr uint32_t NARROW_LPO[NARROW_POS] = {8, 2, 8, 2, 4, 1, 8, 1, 1, 1, 1, 1};
static constexpr uint32_t NARROW_CAP[NARROW_POS] = {8, 24, 8, 6, 6, 14, 4, 20, 14, 12, 12, 8};
static constexpr uint32_t NARROW_BYTE_POS = 6;                           // positions [0, 6): 8-bit records; [6, 12) = D_1: 16-bit records
static constexpr uint32_t NARROW_SLOTS8 = 66, NARROW_SLOTS16 = 70, NARROW_SLOTS = NARROW_SLOTS8 + NARROW_SLOTS16;
static constexpr uint32_t NARROW_OREGS = (NARROW_SLOTS8 + 3) / 4 + NARROW_SLOTS16 / 2, NARROW_QREGS = NARROW_POS / 2;
static constexpr uint32_t NARROW_WGS = 2048;                             // one-wave workgroups per launch: two waves per SIMD (the 200 record registers)
struct NarrowPlan {
    bool ok = false;
    uint32_t x2_off = 0;                                                 // x_2's place in the column
    mem::Buf<uint32_t> d_wt, d_ot, d_q;                                  // slot-major [slot][lane]: weights, packed places, packed output byte offsets
};

// Long codes (codeword over 160 KB: n >= ~6000, tensor_row_size 8192 / 16384 of Our_PC): the outer steps C_0 .. C_{d-1} and D_{d-1} .. D_0,
// whose input windows are too long for one workgroup's LDS, run one launch each through k_enc_tiled (hobbit_kernels.hip); the sub-codeword of
// depth d (the first that fits TILE_MID_MAX) is encoded by one k_encode pass on its own window.  A tiled step cuts its input window into tiles
// of TILE_ELEMS elements (64 KB); its outputs keep one order (by in-degree) and 64-wide slices across tiles, and every (slice, tile) pair owns
// a k-major block of edge records whose input lies in that tile -- index relative to the tile start, padded with zero-weight records to a
// multiple of ENC_UNROLL -- so a lane carries its outputs' 96-bit sums in registers from tile to tile and folds once at the end.
static constexpr uint32_t TILE_ELEMS = 4096;            // 64 KB of LDS: two workgroups per CU
static constexpr uint32_t TILE_WAVES = 8, TILE_MAXS = 4; // waves per workgroup, slices per wave: a workgroup owns TILE_WAVES*TILE_MAXS*64 outputs
static constexpr uint32_t TILE_MID_MAX = 4096;          // longest sub-codeword left to the one-pass k_encode
struct TiledStep {
    uint32_t in_off, in_len, out_off, out_len;
    uint32_t ntiles, n_slices, groups;      // groups: workgroups per column (blockIdx.y), each TILE_WAVES*TILE_MAXS slices
    uint32_t tile_base;                     // index of (slice 0, tile 0) in tile_ptr / tile_width (slice-major, ntiles per slice)
    uint32_t out_base;                      // index of this step's first entry in tile_out (64 per slice)
};

// Brakedown's matrix (hobbit_brakedown_commit): `rows` codewords stored rows-innermost, element (i, c) at c*rows + i, so that one edge of a step
// gathers `rows` contiguous elements.  Every step of the code runs as one launch of k_enc_ilv over its outputs; step s keeps its outputs' in-edges
// as CSR: output t owns records [rowptr[ptr_base + t], rowptr[ptr_base + t + 1]) (input index relative to in_off, weight).
struct IlvStep { uint32_t in_off, out_off, out_len, ptr_base; };

struct PlanStep { const HostGraph *g; long long in_off, out_off; };

// One segment of the parity matrix' access lists (generate_access_idx, src/sumcheck.cpp:2622-2669; hobbit_parity_commit_device): entries
// [base, base + count) of the lists.  kind 0, the edges of one level: entry base + j is edge j of the level's forward records (record src + j
// of the forward form), idx1 = nbr + lvl, idx2 = j / degree + off.  kind 1, an identity run: idx1 = j + lvl, idx2 = j + off, weight p - 1,
// degree 1.  `cells`: the idx2 cells the segment covers (each `degree` times), [off, off + cells).
struct ParitySeg { uint32_t base, count, degree, lvl, off, kind, src, cells; };

struct DeviceCode {         // finalized code for one message length n
    long long n = 0, len = 0;
    bool small_weights = true;               // all weights real and < 2^32
    bool real_weights = true;                // no weight with img != 0 (recorded once, by hobbit_graph_finalize)
    std::vector<EncStep> steps;
    mem::Buf<EncStep> d_steps;
    mem::Buf<uint32_t> d_slice_ptr, d_slice_width, d_slice_out;   // per slice: offset, records per output, output ids
    mem::Buf<uint2> d_edges32;               // {idx, w32}          (small_weights)
    mem::Buf<uint32_t> d_eidx; mem::Buf<F> d_ew;     // general weights
    size_t n_edges_padded = 0, n_edges = 0;
    FatStep fatA, fatC1, fatD;               // first, second and last step in fat form (deep codes only: n = 4096)
    NarrowPlan narrow;                       // the five steps between them, one wave per column (n = 4096 with the degrees the kernel was compiled for)
    // long codes: steps [0, tiled_depth) and [nsteps - tiled_depth, nsteps) in tiled form (tiled_depth = 0: the codeword fits in LDS)
    uint32_t tiled_depth = 0;
    std::vector<TiledStep> tsteps;           // C_0 .. C_{d-1}, then D_{d-1} .. D_0 (the order of `steps`)
    mem::Buf<uint32_t> d_tile_ptr, d_tile_width, d_tile_out;
    mem::Buf<uint2> d_tile_e32;              // {index in the tile, w32}   (small_weights)
    mem::Buf<uint32_t> d_tile_eidx; mem::Buf<F> d_tile_ew;     // general weights
    size_t tile_records = 0;
    // Built on first use, not by hobbit_graph_finalize: the tiled steps (a long code through launch_encode: ensure_tiled) and the CSR steps of
    // the rows-innermost encode (ensure_ilv).  `plan` lists the steps in order (C_0 .. C_{D-1}, D_{D-1} .. D_0) over the uploaded graphs of
    // generation `graph_gen` (hobbit_ctx::graph_gen); `cwlen[d]`: length of the sub-codeword of depth d.
    std::vector<PlanStep> plan; std::vector<long long> cwlen; uint64_t graph_gen = 0; bool tiled_built = false;
    bool slices_built = false;               // the slice tables above: at the finalize for codewords up to 160 KB, with the tiled steps for longer ones
    bool ilv_built = false;
    std::vector<IlvStep> isteps;
    mem::Buf<uint32_t> d_ilv_ptr;
    mem::Buf<uint2> d_ilv_e32;               // {index relative to in_off, w32}   (small_weights)
    mem::Buf<uint32_t> d_ilv_eidx; mem::Buf<F> d_ilv_ew;       // general weights
    // The code's forward form (hobbit_parity_commit_device: ensure_fwd), built on first use: the neighbours and weights of every plan step
    // in list order (C_0 .. C_{D-1}, D_{D-1} .. D_0), and the segment table of the access lists (m entries in all)
    bool fwd_built = false;
    std::vector<ParitySeg> fwd_segs; size_t fwd_m = 0;
    mem::Buf<ParitySeg> d_fwd_segs;
    mem::Buf<uint32_t> d_fwd_nbr, d_fwd_w32;               // w32 under small_weights
    mem::Buf<F> d_fwd_w;                                     // general weights
    // H^T in CSR (evaluate_parity_matrix), built on first use
    mem::Buf<uint32_t> d_pm_rowptr, d_pm_idx; mem::Buf<F> d_pm_w; size_t pm_rows = 0;
};

struct ProfEntry { std::vector<std::pair<hipEvent_t, hipEvent_t>> ev; double ms = 0; long long launches = 0; };

}  // namespace hobbit

namespace hobbit { struct Mailbox { F vals[16]; uint32_t flag; uint32_t pad[3]; }; }

namespace hobbit { namespace fft {
struct R8Set { const F *t1 = nullptr, *t2, *t3; F w8, w8_3; int w4_plus_i; };    // k_fft4096's pass tables [7][8], [7][64], [7][512]; the direction's 8th roots
// dev: device tables by (kind of hobbit_fft_tables.hpp, logn, inverse); r8: per direction, filled with its pass tables
struct Tables { std::map<std::tuple<int, int, bool>, mem::Buf<F>> dev; R8Set r8[2]; };
}}

struct hobbit_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = false;
    // second stream + events: the layout change (HBM-bound) of one chunk group of a large linear tensor runs beside the next group's row FFT
    // (VALU-bound); a commitment with the rotated message half (hobbit_rot.hpp) has no layout change and does not use them.
    // Event slots: [0, 56) the commit pipeline's chunk groups (tensorcode_chunks clamps its group count to 56), 60-63 open_impl's cross-stream
    // fences, 64/65 the pipeline's opening / closing brackets.
    hipStream_t side = nullptr; hipEvent_t side_ev[66] = {};
    // commit_impl <-> launch_encode: "do not materialise the zero tail of the codewords" (asked / done); see hobbit_commitment::rows_valid
    bool enc_skip_tail = false, enc_tail_skipped = false;
    // host -> device streaming of a caller's pageable polynomial (hobbit_commit_standard_host): copy stream, two pinned staging pieces, events
    hipStream_t up_stream = nullptr; hobbit::mem::Buf<void, hobbit::mem::Pinned> up_pin[2]; hipEvent_t up_done[2] = {}; hipEvent_t up_ready[64] = {};
    static constexpr size_t UP_PIECE = (size_t)64 << 20;
    int up_init() {
        if (up_stream) return 0;
        if (hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking) != hipSuccess) { err = "upload stream create failed"; return HOBBIT_EHIP; }
        for (int i = 0; i < 2; i++) {
            if (up_pin[i].alloc_bytes(UP_PIECE)) { err = "upload staging hipHostMalloc failed"; return HOBBIT_ENOMEM; }
            if (hipEventCreateWithFlags(&up_done[i], hipEventDisableTiming) != hipSuccess) { err = "upload event create failed"; return HOBBIT_EHIP; }
        }
        for (auto &e : up_ready) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { err = "upload event create failed"; return HOBBIT_EHIP; }
        return 0;
    }
    int side_init() {
        if (side) return 0;
        if (hipStreamCreateWithFlags(&side, hipStreamNonBlocking) != hipSuccess) { err = "side stream create failed"; return HOBBIT_EHIP; }
        for (auto &e : side_ev) if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { err = "side event create failed"; return HOBBIT_EHIP; }
        return 0;
    }
    // helper context (own stream, scratch, staging, mailbox) for the one part of the open that is independent of what follows it:
    // shockwave_prove(C_c) runs there on a second host thread beside P5 and shockwave_prove(C_f) (open_impl)
    hobbit_ctx *helper = nullptr, *helper2 = nullptr;      // helper2: stream + scratch of the inner commitments, queued from the main thread
    std::string err;
    // profiler
    int prof_on = 0;
    std::map<std::string, hobbit::ProfEntry> prof;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    // every twiddle table of the FFT module (hobbit_fft.hip), built on first use and kept until the context goes
    hobbit::fft::Tables fft;
    // the jump tables of the libc-stream kernels (hobbit_libcgen.hip), built on first use
    hobbit::mem::Buf<uint32_t> libcgen_tab;
    // graphs
    std::map<std::pair<int, int>, hobbit::HostGraph> graphs;   // (dep, kind)
    uint64_t graph_gen = 0;                                     // bumped by every hobbit_graph_upload / hobbit_graph_reset
    hobbit::DeviceCode code;
    // the reference's globals has_lookups / lookup_rand[0..1] (src/main.cpp:67,70), set through hobbit_set_lookups
    bool has_lookups = false; hobbit::F lookup_rand[2];
    // Grow-only scratch (mem::GrowBuf: a request beyond the capacity waits for the stream, frees, then allocates).
    // workspace2: the row-major FFT output of a tensor code before its transpose (not asked for where the row FFT stores the tensor itself)
    // workspace3: arena of the open phase (tables that live across several sumchecks), kept between calls
    // workspace4: scratch of the inner-PCS provers (whir / shockwave), separate from the open arena that holds their inputs
    // workspace5: the caller's buffer of a three-factor transform (2^25 .. 2^28): its nested long transforms own workspace / workspace2
    hobbit::mem::GrowBuf<hobbit::mem::Device> ws[5];
    int grow(int k, size_t bytes, void **p, const char *msg) { if (ws[k].ensure(stream, bytes, p)) { err = msg; return HOBBIT_ENOMEM; } return 0; }
    int workspace2(size_t bytes, void **p) { return grow(1, bytes, p, "workspace2 hipMalloc failed"); }
    int workspace3(size_t bytes, void **p) { return grow(2, bytes, p, "workspace3 hipMalloc failed"); }
    int workspace4(size_t bytes, void **p) { return grow(3, bytes, p, "workspace4 hipMalloc failed"); }
    int workspace5(size_t bytes, void **p) { return grow(4, bytes, p, "workspace5 hipMalloc failed"); }
    // The buffers of short-lived objects come from and go back to a size-keyed pool (hobbit_mem.hpp); pool.stream is this context's stream.
    hobbit::mem::Pool pool;
    template <class T> int pool_get(size_t bytes, hobbit::mem::Pooled<T> &b) { if (b.get(pool, bytes)) { err = "device allocation failed"; return HOBBIT_ENOMEM; } return 0; }
    void pool_drain() { pool.drain(); }
    std::map<void *, size_t> large;              // live hobbit_malloc allocations too large for the pool (pointer -> size)
    // small pinned host buffer for the per-round coefficient read-back of the sumchecks
    hobbit::mem::GrowBuf<hobbit::mem::Pinned> pin;
    int pinned(size_t bytes, void **p) { if (pin.ensure(stream, bytes < 4096 ? 4096 : bytes, p)) { err = "hipHostMalloc failed"; return HOBBIT_ENOMEM; } return 0; }
    // Pinned staging arena of the open path.  hipMemcpyAsync to or from PAGEABLE host memory is not asynchronous on this runtime: a
    // device-to-host copy into a caller's buffer first waits for everything queued on the stream (rocprofv3: 100-170 us of GPU idle time
    // after every such copy, 2 ms per open).  So host inputs are copied here and uploaded from here, results land here and reach the
    // caller's buffers (`deferred`) after the closing synchronisation of the outermost library call (`stage_depth`).
    hobbit::mem::Buf<uint8_t, hobbit::mem::Pinned> stage; size_t stage_cap = 0, stage_off = 0; int stage_depth = 0;
    struct Deferred { void *dst; const void *src; size_t bytes; };
    std::vector<Deferred> deferred;
    void *stage_alloc(size_t bytes) {
        if (!stage) { if (stage.alloc((size_t)24 << 20)) return nullptr; stage_cap = (size_t)24 << 20; }
        const size_t a = (stage_off + 63) & ~(size_t)63;
        if (a + bytes > stage_cap) return nullptr;
        stage_off = a + bytes; return stage + a;
    }
    // one retired commitment's buffers, kept for the next commit of the same shape (a 2^28 commit
    // owns 16.5 GiB; re-allocating it per call would dominate a repeated-commit loop)
    hobbit::mem::Buf<hobbit::F> spare_tensor; hobbit::mem::Buf<uint8_t> spare_levels;
    // likewise one retired parity commitment's five device buffers (12.6 GiB at n = 2^20), for the next hobbit_parity_commit_device of the same
    // (P, n): the runtime releases freed buffers of this size in bursts, seconds long, inside a later allocation
    struct ParityBufs {
        hobbit::mem::Buf<uint32_t> d_u32;      // idx1 | idx2 | cnt1 | cnt2, P each
        hobbit::mem::Buf<hobbit::F> d_F;       // weight (P) | acc1 (2n) | acc2 (2n)
        hobbit::mem::Buf<hobbit::F> d_pw, d_enc; hobbit::mem::Buf<uint8_t> d_levels;
        bool whole() const { return d_u32 && d_F && d_pw && d_enc && d_levels; }
    };
    ParityBufs spare_parity; size_t spare_parity_P = 0; long long spare_parity_n = 0;

    // What is about order: drain the streams and the pool while the streams exist; the members' owners free afterwards, without waiting.
    ~hobbit_ctx() {
        delete helper; delete helper2;
        hipSetDevice(device);
        hipStreamSynchronize(stream);
        prof_collect();
        pool_drain();
        for (hipEvent_t e : ev_pool) hipEventDestroy(e);
        if (t0) hipEventDestroy(t0);
        if (t1) hipEventDestroy(t1);
        if (up_stream) {
            hipStreamSynchronize(up_stream);
            for (auto &e : up_done) if (e) hipEventDestroy(e);
            for (auto &e : up_ready) if (e) hipEventDestroy(e);
            hipStreamDestroy(up_stream);
        }
        if (side) { hipStreamSynchronize(side); for (auto &e : side_ev) if (e) hipEventDestroy(e); hipStreamDestroy(side); }
        if (owns_stream) hipStreamDestroy(stream);
    }
    int fail(int code, const std::string &msg) { err = msg; return code; }
    int hip(hipError_t e, const char *what) {
        if (e == hipSuccess) return 0;
        err = std::string(what) + ": " + hipGetErrorString(e);
        return HOBBIT_EHIP;
    }
    // prof_on: 0 off, 1 every launch, 2 only the commit's bulk kernels (a handful of launches per step: the event brackets then
    // cost nothing measurable, whereas bracketing the ~500 small launches of an open adds milliseconds of host time per step)
    std::vector<hipEvent_t> ev_pool;
    hipEvent_t ev_get() { if (!ev_pool.empty()) { hipEvent_t e = ev_pool.back(); ev_pool.pop_back(); return e; } hipEvent_t e; hipEventCreate(&e); return e; }
    static bool prof_bulk(const char *n) {
        return !strncmp(n, "k_leaf_chain", 12) || !strncmp(n, "k_fft4096", 9) || !strncmp(n, "k_encode", 8) || !strncmp(n, "k_enc_", 6) || !strcmp(n, "k_transpose") ||
               !strncmp(n, "k_inner_digests", 15) || !strncmp(n, "k_chain_digests", 15) || !strcmp(n, "k_aggregate");
    }
    bool prof_cur = false;
    void prof_begin(const char *name) {
        prof_cur = prof_on == 1 || (prof_on == 2 && prof_bulk(name));
        if (!prof_cur) return;
        hipEvent_t a = ev_get(), b = ev_get();
        hipEventRecord(a, stream);
        prof[name].ev.emplace_back(a, b);
    }
    void prof_end(const char *name) {
        if (!prof_cur) return;
        auto &e = prof[name]; hipEventRecord(e.ev.back().second, stream); e.launches++;
    }
    void prof_collect() {
        for (auto &kv : prof) {
            for (auto &p : kv.second.ev) {
                hipEventSynchronize(p.second);
                float ms = 0; hipEventElapsedTime(&ms, p.first, p.second);
                kv.second.ms += ms; ev_pool.push_back(p.first); ev_pool.push_back(p.second);
            }
            kv.second.ev.clear();
        }
    }
    // ---- mailbox: the one-workgroup reduction kernel of a sumcheck round writes its few coefficients straight into coherent pinned
    // host memory and then a sequence number; the host spins on that word (HOBBIT_MBOX=sync: sleeps in hipStreamSynchronize)
    // instead of queueing a copy and synchronising.
    // ---- tail area: behind the mailbox in the same coherent pinned allocation, two tables of TAIL_ELEMS elements.  The launch that
    // produces the tables a two-product sumcheck hands to the host (hobbit_kernels.hip, sumcheck2_impl) also stores them here, and the
    // round's post -- behind that launch in stream order -- tells the host they have landed: no copy command, no stream drain.
    static constexpr size_t TAIL_ELEMS = 2048, MBOX_BYTES = 4096, TAIL_BYTES = 2 * TAIL_ELEMS * sizeof(hobbit::F);
    hobbit::mem::Buf<hobbit::Mailbox, hobbit::mem::Pinned> mbox; hobbit::mem::Buf<unsigned> d_ticket; uint32_t mbox_seq = 0;
    hobbit::F *tail = nullptr;                   // tables at tail and tail + TAIL_ELEMS
    int mailbox(hobbit::Mailbox **m, unsigned **ticket) {
        if (!mbox) {
            if (mbox.alloc_bytes(MBOX_BYTES + TAIL_BYTES, hipHostMallocCoherent | hipHostMallocMapped)) { err = "mailbox hipHostMalloc failed"; return HOBBIT_ENOMEM; }
            memset((void *)mbox.get(), 0, MBOX_BYTES + TAIL_BYTES);
            tail = reinterpret_cast<hobbit::F *>(reinterpret_cast<uint8_t *>(mbox.get()) + MBOX_BYTES);
            if (d_ticket.alloc_bytes(256)) { err = "mailbox ticket alloc failed"; return HOBBIT_ENOMEM; }
            if (hipMemsetAsync(d_ticket, 0, 256, stream) != hipSuccess) { err = "mailbox ticket memset failed"; return HOBBIT_EHIP; }
        }
        *m = mbox; *ticket = d_ticket; return 0;
    }
    // wait until the kernel tagged `seq` has posted; bounded: gives up (error) once the stream has drained without the post
    // Drain the stream.  hipStreamSynchronize sleeps on an interrupt: in the rocprofv3 trace of an open nine such waits were each followed
    // by ~92 us of GPU idle time before the next kernel.  The default polls the stream's completion instead (a wait longer than 1 ms falls
    // back to the sleeping call; HOBBIT_SYNC=sleep: always sleep).  Alternating same-box runs of commit + open at 2^28: 39.45 / 39.75 ms
    // sleeping, 39.18 / 39.44 ms polling.  (The other configs of scripts/bench_configs.py do not move; what looked like a regression of
    // the 2^24 sumcheck there was the order of the runs -- the first process on a fresh box is the fast one whichever mode it uses.)
    int sync_mode = -1;
    // time this context's host thread spent waiting for the device (stream drains, mailbox spins): HOBBIT_TRACE=host prints it per stage,
    // the rest of a stage's time is host work the GPU may be waiting for
    uint64_t wait_ns = 0;
    struct WaitClock {
        hobbit_ctx *c; std::chrono::steady_clock::time_point t0;
        explicit WaitClock(hobbit_ctx *ctx) : c(ctx), t0(std::chrono::steady_clock::now()) {}
        ~WaitClock() { c->wait_ns += (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count(); }
    };
    int sync() {
        if (sync_mode < 0) { const char *e = getenv("HOBBIT_SYNC"); sync_mode = (e && !strcmp(e, "sleep")) ? 0 : 1; }
        WaitClock wc(this);
        if (sync_mode == 0) return hip(hipStreamSynchronize(stream), "stream sync");
        const auto t_start = wc.t0;
        for (uint32_t it = 1;; it++) {
            const hipError_t q = hipStreamQuery(stream);
            if (q == hipSuccess) return 0;
            if (q != hipErrorNotReady) return hip(q, "stream sync");
            if ((it & 0x3F) == 0 && std::chrono::steady_clock::now() - t_start > std::chrono::milliseconds(1)) return hip(hipStreamSynchronize(stream), "stream sync");
        }
    }
    int mbox_mode = -1;
    int mbox_wait(uint32_t seq) {
        if (mbox_mode < 0) { const char *e = getenv("HOBBIT_MBOX"); mbox_mode = (e && !strcmp(e, "sync")) ? 0 : 1; }
        WaitClock wc(this);
        if (mbox_mode == 0) {                    // sleep in the runtime; the post is complete when the kernel is
            int r = hip(hipStreamSynchronize(stream), "mailbox wait");
            if (r) return r;
            if (mbox->flag != seq) { err = "mailbox: kernel finished without posting"; return HOBBIT_EHIP; }
            return 0;
        }
        // the runtime queues launches lazily: a query makes it submit what is pending before we start spinning
        hipError_t q = hipStreamQuery(stream);
        if (q != hipSuccess && q != hipErrorNotReady) return hip(q, "mailbox wait");
        const auto t_start = std::chrono::steady_clock::now();
        for (uint64_t it = 1;; it++) {
            if (__atomic_load_n(&mbox->flag, __ATOMIC_ACQUIRE) == seq) return 0;
            if ((it & 0xFFFF) == 0) {
                if (std::chrono::steady_clock::now() - t_start > std::chrono::seconds(60)) { err = "mailbox: no post within 60 s (kernel hung?)"; return HOBBIT_EHIP; }
                q = hipStreamQuery(stream);
                if (q == hipSuccess) { if (__atomic_load_n(&mbox->flag, __ATOMIC_ACQUIRE) == seq) return 0; err = "mailbox: kernel finished without posting"; return HOBBIT_EHIP; }
                if (q != hipErrorNotReady) return hip(q, "mailbox wait");
            }
        }
    }
    // a caller may lend `workspace` another buffer for the calls it queues on a stream of its own (open_impl: the query answers on the
    // inner commitments' stream), so that they do not share scratch with what runs on the context's stream at the same time
    void *ws_lent = nullptr; size_t ws_lent_bytes = 0;
    int workspace(size_t bytes, void **p) {
        if (ws_lent) {
            if (bytes > ws_lent_bytes) { err = "lent workspace too small"; return HOBBIT_ESTATE; }
            *p = ws_lent; return 0;
        }
        return grow(0, bytes, p, "workspace hipMalloc failed");
    }
};

// A handle of the ABI while its constructor builds it: every early return frees it the way its *_free does; release() into *out at the end.
template <class H, void (*Free)(H *)> struct HandleFree { void operator()(H *h) const { Free(h); } };
template <class H, void (*Free)(H *)> using Handle = std::unique_ptr<H, HandleFree<H, Free>>;

// launch + optional per-kernel event bracket; checks the launch error
#define HB_LAUNCH(ctx, name, kern, grid, block, lds, ...)                                   \
    do {                                                                                     \
        (ctx)->prof_begin(name);                                                             \
        hipLaunchKernelGGL(kern, grid, block, lds, (ctx)->stream, __VA_ARGS__);              \
        (ctx)->prof_end(name);                                                               \
        hipError_t e__ = hipGetLastError();                                                  \
        if (e__ != hipSuccess) return (ctx)->hip(e__, name);                                 \
    } while (0)
#define HB_CHECK(ctx, call) do { int r__ = (ctx)->hip((call), #call); if (r__) return r__; } while (0)
#define HB_TRY(expr) do { int r__ = (expr); if (r__) return r__; } while (0)

namespace hobbit {
// Device buffers of one call (or one handle) taken through hobbit_malloc -- pooled up to its limit, from the runtime beyond -- and given back
// through hobbit_free on every way out
struct Scratch {
    hobbit_ctx *ctx; std::vector<void *> bufs;
    explicit Scratch(hobbit_ctx *c) : ctx(c) {}
    Scratch(const Scratch &) = delete;
    Scratch &operator=(const Scratch &) = delete;
    ~Scratch() { for (void *p : bufs) hobbit_free(ctx, p); }
    int get(size_t bytes, void **p) { HB_TRY(hobbit_malloc(ctx, bytes, p)); bufs.push_back(*p); return 0; }
};
using ParityHandle = Handle<hobbit_parity_commitment, hobbit_parity_commitment_free>;
}  // namespace hobbit
