// hobbit_capi.hip -- the extern "C" boundary declared in include/hobbit_hip.h.
// Host orchestration only: argument checks, graph preprocessing (reverse adjacency in sliced-ELL
// form), twiddle tables, and the launch sequences of tensor code / commit / open building blocks.
#include <algorithm>
#include <cstdio>
#include <chrono>
#include <cstring>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>
#include <functional>
#include "hobbit_kernels.hpp"
#include "hobbit_fft.hpp"
#include "hobbit_blake3.hpp"
#include "hobbit_libcgen.hpp"
#include "../../include/hobbit_whir.h"
#include "../../include/hobbit_real.h"
#include "../../include/hobbit_elastic_real.h"
#include "../../include/hobbit_real_rs.h"

using namespace hobbit;

// A hobbit_F pointer of the ABI is either a DEVICE pointer (handed on to the launchers as F *: 16-byte aligned by hobbit_malloc) or a HOST
// pointer (8-byte aligned: dereferenced only through HF, hobbit_field.hpp).  cF / mF give a thin pointer wrapper that converts to F * for
// the first use and indexes / dereferences as HF for the second -- host code never sees an F lvalue at an 8-byte-aligned address.
static inline CHP cF(const hobbit_F *p) { return CHP(reinterpret_cast<const HF *>(p)); }
static inline MHP mF(hobbit_F *p) { return MHP(reinterpret_cast<HF *>(p)); }
static_assert(sizeof(hobbit_F) == sizeof(F), "ABI field element must be 16 bytes");

struct hobbit_commitment {
    hobbit_ctx *ctx;
    size_t N, M; int K, trs, lin; uint32_t cols, rows2;
    mem::Buf<F> d_tensor; mem::Buf<uint8_t> d_levels;
    // Rows [rows_valid, rows2) of every column are zero by construction (an RS x expander codeword ends at `len`; rows_valid = len rounded up to the
    // leaf group) and were NOT written: the leaf chain, the gathers and the row reads answer them as zeros; hobbit_commitment_tensor_dev fills them
    // in before it hands the raw pointer out.  rows_valid == rows2: everything is in memory (RS x RS, shallow codes, HOBBIT_COMMIT_SKIP_TAIL=0).
    uint32_t rows_valid;
    // The message half (rows [0, trs)) of every column is rotated inside its own ring (hobbit_rot.hpp): msg_rot = trs - 1, else 0.  Written so by
    // the commit's row FFT where the shape has the rotated form (tensorcode_chunks); read through msg_rot_row by the encode's loader, the leaf
    // chain, the gathers and the row reads.  d_tensor never escapes except through hobbit_commitment_tensor_dev, which un-rotates it first, once.
    uint32_t msg_rot = 0;
    // A half commitment (hobbit_commit_standard_real; hobbit_half.hpp): d_tensor holds columns 0 .. cols / 2 of every chunk, K cols / 2 + K
    // codeword-major columns, and column c > cols / 2 is answered as the conjugate of column cols - c.  rows_valid and msg_rot hold for it as for
    // a full tensor.  Invariant: d_tensor of a half commitment never escapes; hobbit_commitment_tensor_dev materialises the full linear tensor
    // [K][cols][rows2] once into d_full, which the commitment owns, and hands that out from then on -- d_tensor, rows_valid and msg_rot stay as
    // they are, and every other reader keeps reading the half form.
    bool half = false;
    mem::Buf<F> d_full;
};

// Scope of one library call for the staging arena (hobbit_ctx.hpp): the outermost scope resets the arena on entry and, in finish(),
// synchronises the stream and hands the staged results to the caller's buffers; nested calls share the arena and defer to it.
struct StageScope {
    hobbit_ctx *ctx; bool top;
    explicit StageScope(hobbit_ctx *c) : ctx(c), top(c->stage_depth++ == 0) { if (top) { ctx->stage_off = 0; ctx->deferred.clear(); } }
    ~StageScope() { ctx->stage_depth--; if (top) ctx->deferred.clear(); }
    int finish() {
        if (!top) return 0;
        HB_TRY(ctx->sync());
        for (auto &d : ctx->deferred) memcpy(d.dst, d.src, d.bytes);
        ctx->deferred.clear();
        return 0;
    }
};
static int h2d_staged(hobbit_ctx *ctx, void *d, const void *h, size_t bytes) {
    if (!bytes) return 0;
    void *p = ctx->stage_depth > 0 ? ctx->stage_alloc(bytes) : nullptr;
    if (!p) { HB_CHECK(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream)); return 0; }     // pageable fallback (synchronous in effect)
    memcpy(p, h, bytes);
    HB_CHECK(ctx, hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}
static int d2h_staged(hobbit_ctx *ctx, void *h, const void *d, size_t bytes) {
    if (!bytes) return 0;
    void *p = ctx->stage_depth > 0 ? ctx->stage_alloc(bytes) : nullptr;
    if (!p) { HB_CHECK(ctx, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream)); return 0; }
    HB_CHECK(ctx, hipMemcpyAsync(p, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    ctx->deferred.push_back({h, p, bytes});
    return 0;
}
static int ilog2_exact(size_t n) { int l = 0; while (((size_t)1 << l) < n) l++; return ((size_t)1 << l) == n ? l : -1; }

namespace hobbit { TranscriptRec &transcript_rec() { static thread_local TranscriptRec t; return t; } }

extern "C" {

const char *hobbit_version(void) { return "hobbit-hip 0.1 (gfx950)"; }

// context creation runs under a parked libc generator: libcgen::Guard (hobbit_libcgen.hpp) says why
int hobbit_ctx_create_on_stream(int device, void *hip_stream, hobbit_ctx **out) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    libcgen::Guard rng_guard;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return HOBBIT_ENODEV;   // no CPU fallback, by design
    if (device < 0 || device >= ndev) return HOBBIT_ENODEV;
    if (hipSetDevice(device) != hipSuccess) return HOBBIT_ENODEV;
    hobbit_ctx *c = new hobbit_ctx();
    c->device = device;
    if (hip_stream) { c->stream = (hipStream_t)hip_stream; c->owns_stream = false; }
    else { if (hipStreamCreate(&c->stream) != hipSuccess) { delete c; return HOBBIT_EHIP; } c->owns_stream = true; }
    c->pool.stream = c->stream;
    hipEventCreate(&c->t0); hipEventCreate(&c->t1);
    {   // first allocation + first launch + first pinned allocation, still under the guard
        mem::Buf<hobbit_F> p; mem::Buf<void, mem::Pinned> hp;
        if (!p.alloc(256)) { hobbit_fill_splitmix(c, p, 256, 1); hipStreamSynchronize(c->stream); }
        (void)hp.alloc_bytes(4096);
    }
    *out = c;
    return 0;
}
int hobbit_ctx_create(int device, hobbit_ctx **out) { return hobbit_ctx_create_on_stream(device, nullptr, out); }

void hobbit_ctx_destroy(hobbit_ctx *ctx) { delete ctx; }     // the order of the teardown: ~hobbit_ctx
const char *hobbit_last_error(const hobbit_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }
int hobbit_sync(hobbit_ctx *ctx) { HB_TRY(ctx->sync()); return 0; }
// Temporaries of up to 256 MiB come from / go back to the context's size-keyed pool (the host mirror and the Python harness allocate
// and free a buffer per call); larger buffers go to the runtime directly and are released for real.
static const size_t HB_POOLED_MAX = (size_t)256 << 20;
int hobbit_malloc(hobbit_ctx *ctx, size_t bytes, void **d_ptr) {
    hipSetDevice(ctx->device);
    if (!bytes) bytes = 16;
    if (bytes <= HB_POOLED_MAX) {
        if (ctx->pool.lend(bytes, d_ptr)) return ctx->fail(HOBBIT_ENOMEM, "hipMalloc failed");
        return 0;
    }
    mem::Buf<void> b;
    if (b.alloc_bytes(bytes)) {
        ctx->pool_drain();
        if (b.alloc_bytes(bytes)) return ctx->fail(HOBBIT_ENOMEM, "hipMalloc failed");
    }
    ctx->large[b.get()] = bytes; *d_ptr = b.release();
    return 0;
}
int hobbit_free(hobbit_ctx *ctx, void *d_ptr) {
    if (!d_ptr) return 0;
    if (ctx->pool.take_back(d_ptr)) return 0;
    HB_TRY(ctx->sync());
    auto it = ctx->large.find(d_ptr);                        // (a pointer this context did not hand out is freed all the same, counted as 0 bytes)
    mem::Buf<void> b; b.adopt(d_ptr, it != ctx->large.end() ? it->second : 0);
    if (it != ctx->large.end()) ctx->large.erase(it);
    return 0;
}
void hobbit_mem_live(size_t *allocs, size_t *bytes) {
    if (allocs) *allocs = mem::live_allocs.load();
    if (bytes) *bytes = mem::live_bytes.load();
}
// Large transfers between the device and PAGEABLE host memory go through the context's two pinned 64 MiB staging pieces, the host side of
// each piece copied by a few threads while the other piece is on the bus: a plain hipMemcpy of 512 MB of Merkle levels into a std::vector ran at
// 4 GB/s (124 ms of the mirror's 277 ms commit at 2^28).  Both calls return when the data has arrived, like the plain ones.
static void par_memcpy(void *dst, const void *src, size_t n) {
    const int T = 8; std::thread th[T]; const size_t per = (n + T - 1) / T / 4096 * 4096 + 4096;
    for (int t = 0; t < T; t++) { const size_t lo = std::min(n, (size_t)t * per), hi = std::min(n, lo + per); th[t] = std::thread([=] { if (hi > lo) memcpy((char *)dst + lo, (const char *)src + lo, hi - lo); }); }
    for (int t = 0; t < T; t++) th[t].join();
}
static const size_t HB_STAGED_COPY_MIN = (size_t)32 << 20;
int hobbit_memcpy_h2d(hobbit_ctx *ctx, void *d, const void *h, size_t bytes) {
    if (bytes >= HB_STAGED_COPY_MIN && ctx->up_init() == 0) {
        HB_TRY(ctx->sync());                                            // ordered after what the context's stream has queued
        int piece = 0;
        for (size_t off = 0; off < bytes; off += hobbit_ctx::UP_PIECE, piece++) {
            const size_t n = std::min(hobbit_ctx::UP_PIECE, bytes - off); const int b = piece & 1;
            if (piece >= 2) HB_CHECK(ctx, hipEventSynchronize(ctx->up_done[b]));
            par_memcpy(ctx->up_pin[b], (const char *)h + off, n);
            HB_CHECK(ctx, hipMemcpyAsync((char *)d + off, ctx->up_pin[b], n, hipMemcpyHostToDevice, ctx->up_stream));
            HB_CHECK(ctx, hipEventRecord(ctx->up_done[b], ctx->up_stream));
        }
        HB_CHECK(ctx, hipStreamSynchronize(ctx->up_stream));
        return 0;
    }
    HB_CHECK(ctx, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream)); HB_TRY(ctx->sync()); return 0;
}
int hobbit_memcpy_d2h(hobbit_ctx *ctx, void *h, const void *d, size_t bytes) {
    if (bytes >= HB_STAGED_COPY_MIN && ctx->up_init() == 0) {
        HB_TRY(ctx->sync());
        const size_t np = (bytes + hobbit_ctx::UP_PIECE - 1) / hobbit_ctx::UP_PIECE;
        auto issue = [&](size_t p) -> int {
            const size_t off = p * hobbit_ctx::UP_PIECE, n = std::min(hobbit_ctx::UP_PIECE, bytes - off); const int b = (int)(p & 1);
            HB_CHECK(ctx, hipMemcpyAsync(ctx->up_pin[b], (const char *)d + off, n, hipMemcpyDeviceToHost, ctx->up_stream));
            HB_CHECK(ctx, hipEventRecord(ctx->up_done[b], ctx->up_stream));
            return 0;
        };
        HB_TRY(issue(0));
        for (size_t p = 0; p < np; p++) {
            if (p + 1 < np) HB_TRY(issue(p + 1));                       // the next piece crosses the bus while this one is copied out
            const size_t off = p * hobbit_ctx::UP_PIECE, n = std::min(hobbit_ctx::UP_PIECE, bytes - off);
            HB_CHECK(ctx, hipEventSynchronize(ctx->up_done[p & 1]));
            par_memcpy((char *)h + off, ctx->up_pin[p & 1], n);
        }
        return 0;
    }
    HB_CHECK(ctx, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream)); HB_TRY(ctx->sync()); return 0;
}
int hobbit_memset(hobbit_ctx *ctx, void *d, int value, size_t bytes) { HB_CHECK(ctx, hipMemsetAsync(d, value, bytes, ctx->stream)); return 0; }
int hobbit_timer_begin(hobbit_ctx *ctx) { HB_CHECK(ctx, hipEventRecord(ctx->t0, ctx->stream)); return 0; }
int hobbit_timer_end_ms(hobbit_ctx *ctx, float *ms) {
    HB_CHECK(ctx, hipEventRecord(ctx->t1, ctx->stream)); HB_CHECK(ctx, hipEventSynchronize(ctx->t1));
    HB_CHECK(ctx, hipEventElapsedTime(ms, ctx->t0, ctx->t1)); return 0;
}
int hobbit_profile_enable(hobbit_ctx *ctx, int on) { ctx->prof_on = on < 0 ? 0 : on > 2 ? 1 : on; return 0; }
int hobbit_profile_reset(hobbit_ctx *ctx) { hipStreamSynchronize(ctx->stream); ctx->prof_collect(); ctx->prof.clear(); return 0; }
int hobbit_profile_get(hobbit_ctx *ctx, const char *kernel, double *total_ms, long long *launches) {
    HB_TRY(ctx->sync());
    ctx->prof_collect();
    auto it = ctx->prof.find(kernel);
    if (it == ctx->prof.end()) { *total_ms = 0; *launches = 0; return 0; }
    *total_ms = it->second.ms; *launches = it->second.launches; return 0;
}
int hobbit_profile_names(hobbit_ctx *ctx, char *buf, size_t buflen) {
    std::string s;
    for (auto &kv : ctx->prof) { if (!s.empty()) s += ";"; s += kv.first; }
    if (s.size() + 1 > buflen) return ctx->fail(HOBBIT_EINVAL, "profile_names: buffer too small");
    memcpy(buf, s.c_str(), s.size() + 1); return 0;
}

// ---- transcript recorder (per calling thread) -------------------------------------------------------
void hobbit_transcript_record(int on) { TranscriptRec &t = transcript_rec(); if (on) t.w.clear(); t.on = on != 0; }
size_t hobbit_transcript_count(void) { return transcript_rec().w.size() / 6; }
size_t hobbit_transcript_read(uint64_t *out, size_t max_records) {
    TranscriptRec &t = transcript_rec();
    const size_t n = std::min(max_records, t.w.size() / 6);
    if (n) memcpy(out, t.w.data(), n * 6 * sizeof(uint64_t));
    return n;
}
// ---- host-side field helpers ------------------------------------------------------------------
void hobbit_mimc(const hobbit_F *x, const hobbit_F *k, hobbit_F *out) { *mF(out) = mimc_hash(*cF(x), *cF(k)); }
void hobbit_f_mul_host(const hobbit_F *a, const hobbit_F *b, hobbit_F *o, size_t n) { for (size_t i = 0; i < n; i++) mF(o)[i] = fmul(cF(a)[i], cF(b)[i]); }
void hobbit_f_inv_host(const hobbit_F *a, hobbit_F *o, size_t n) { for (size_t i = 0; i < n; i++) mF(o)[i] = finv(cF(a)[i]); }
void hobbit_generate_randomness(size_t n, hobbit_F *h_out) {       // src/utils.cpp:873-883
    F cst = fmake(0);
    for (size_t i = 0; i < n; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); mF(h_out)[i] = fadd(cst, fmake((uint64_t)rand())); }
}
int hobbit_f_binop(hobbit_ctx *ctx, int op, const hobbit_F *a, const hobbit_F *b, hobbit_F *o, size_t n) {
    if (op < 0 || op > 2) return ctx->fail(HOBBIT_EINVAL, "f_binop: op must be 0,1,2");
    if (!n) return 0;
    return launch_f_binop(ctx, op, cF(a), cF(b), mF(o), n);
}
int hobbit_fill_splitmix(hobbit_ctx *ctx, hobbit_F *o, size_t n, uint64_t seed) { if (!n) return 0; return launch_fill_splitmix(ctx, mF(o), n, seed); }

// ---- expander graphs --------------------------------------------------------------------------
int hobbit_graph_reset(hobbit_ctx *ctx) { ctx->graphs.clear(); ctx->graph_gen++; hipStreamSynchronize(ctx->stream); ctx->code = DeviceCode(); return 0; }
int hobbit_graph_upload(hobbit_ctx *ctx, int dep, int kind, long long L, long long R, int degree, const long long *nbr, const hobbit_F *w) {
    if (dep < 0 || dep >= 100 || (kind != 0 && kind != 1) || L <= 0 || R <= 0 || degree <= 0) return ctx->fail(HOBBIT_EINVAL, "graph_upload: bad dims");
    HostGraph g; g.L = L; g.R = R; g.degree = degree;
    g.nbr.assign(nbr, nbr + L * degree);
    g.w.resize((size_t)(L * degree)); for (size_t i = 0; i < g.w.size(); i++) g.w[i] = cF(w)[i];
    for (long long t : g.nbr) if (t < 0 || t >= R) return ctx->fail(HOBBIT_EINVAL, "graph_upload: neighbour out of range");
    ctx->graphs[{dep, kind}] = std::move(g);
    ctx->graph_gen++;
    return 0;
}
}  // extern "C"
namespace hobbit {
// in-edges of every output of a step, in input order: (input index, weight)
using InEdges = std::vector<std::vector<std::pair<uint32_t, F>>>;
static InEdges in_edges(const HostGraph &g) {
    InEdges rows((size_t)g.R);
    for (long long i = 0; i < g.L; i++)
        for (int j = 0; j < g.degree; j++) rows[g.nbr[i * g.degree + j]].push_back({(uint32_t)i, g.w[i * g.degree + j]});
    return rows;
}
// the outputs in order of in-degree, heaviest first (stable: equal in-degrees keep output order)
static std::vector<uint32_t> by_in_degree(const InEdges &rows) {
    std::vector<uint32_t> order(rows.size());
    for (size_t t = 0; t < order.size(); t++) order[t] = (uint32_t)t;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return rows[a].size() > rows[b].size(); });
    return order;
}
// a host table into a fresh device allocation (16 bytes for an empty one)
template <class T>
static int upload(hobbit_ctx *ctx, mem::Buf<T> *d, const std::vector<T> &h) {
    const size_t bytes = h.size() * sizeof(T);
    if (d->alloc_bytes(bytes ? bytes : 16)) return ctx->fail(HOBBIT_ENOMEM, "graph alloc failed");
    if (bytes) HB_CHECK(ctx, hipMemcpy(d->get(), h.data(), bytes, hipMemcpyHostToDevice));
    return 0;
}
// fat form of one step (hobbit_ctx.hpp FatStep): `nout` outputs per lane of `ncons` consumer waves, cap[j] register slots at position j.
// Leaves f.ok false when the step's degrees exceed the caps.
static int build_fat_step(hobbit_ctx *ctx, const PlanStep &p, uint32_t nout, uint32_t ncons, const uint32_t *cap, FatStep &f) {
    const HostGraph &g = *p.g;
    const size_t R = (size_t)g.R, lanes = (size_t)ncons * 64;
    if (R > nout * lanes || (size_t)g.L * 16 > 65536) return 0;
    const InEdges rows = in_edges(g);
    const std::vector<uint32_t> order = by_in_degree(rows);
    uint32_t base[4] = {0, 0, 0, 0}, tot = 0;
    for (uint32_t j = 0; j < nout; j++) { base[j] = tot; tot += cap[j]; }
    std::vector<uint32_t> wt((size_t)tot * lanes, 0), ot((size_t)(tot / 2) * lanes, 0), oidx((size_t)nout * lanes, 0xFFFFFFFFu), wid((size_t)ncons * nout, 0);
    // which output each (position, lane) owns, and the widths
    std::vector<int64_t> own((size_t)nout * lanes, -1);
    for (uint32_t j = 0; j < nout; j++)
        for (size_t l = 0; l < lanes; l++) {
            const size_t i = (j % 2 == 0) ? (size_t)j * lanes + l : (size_t)(j + 1) * lanes - 1 - l;      // serpentine: heavy with light
            if (i >= R) continue;
            const auto &row = rows[order[i]];
            if (row.size() > cap[j]) return 0;
            own[(size_t)j * lanes + l] = order[i]; oidx[(size_t)j * lanes + l] = order[i];
            uint32_t &w = wid[(l / 64) * nout + j];
            w = std::max(w, (uint32_t)((row.size() + 3) / 4 * 4));
        }
    // Slot order.  A lane's records are its own, so their order is free -- and the kernels turned out to be bound by LDS bank conflicts (SQ counters, round 3:
    // 65 % of the LDS-array cycles of k_enc_fat are conflict cycles with the edges in graph order).  A ds_read_b128 is served in four fixed groups of 16 lanes;
    // a 16-byte element covers one of 16 bank quads (index mod 16).  Per wave, position and group, slot after slot: a maximum matching of lanes to the quads
    // of their remaining edges (most constrained lanes first) -- a matched lane reads conflict-free, an unmatched one spends a padding slot if its row
    // is shorter than the wave's width, else takes any edge; padding slots point at a quad nobody else uses.
    static const int GROUPS[4][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
                                      {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59}, {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};
    auto put = [&](uint32_t j, size_t l, uint32_t k, uint32_t idx, F w) {
        const size_t slot = base[j] + k;
        wt[slot * lanes + l] = (uint32_t)w.re;
        ot[(slot / 2) * lanes + l] |= (idx * 16u) << (16 * (slot & 1));
    };
    for (uint32_t j = 0; j < nout; j++)
        for (uint32_t wv = 0; wv < ncons; wv++) {
            const uint32_t W = wid[wv * nout + j];
            for (int gi = 0; gi < 4; gi++) {
                std::vector<std::pair<uint32_t, F>> rem[16]; int slack[16];
                for (int q = 0; q < 16; q++) {
                    const size_t l = (size_t)wv * 64 + GROUPS[gi][q];
                    const int64_t t = own[(size_t)j * lanes + l];
                    if (t >= 0) rem[q] = rows[(size_t)t];
                    slack[q] = (int)W - (int)rem[q].size();
                }
                for (uint32_t k = 0; k < W; k++) {
                    int lane_of[16], quad_of[16]; for (int q = 0; q < 16; q++) { lane_of[q] = -1; quad_of[q] = -1; }
                    int ord[16]; for (int q = 0; q < 16; q++) ord[q] = q;
                    std::stable_sort(ord, ord + 16, [&](int a, int b) { return slack[a] < slack[b]; });
                    std::function<bool(int, bool *)> aug = [&](int q, bool *seen) -> bool {
                        for (auto &e : rem[q]) { const int r = e.first & 15; if (seen[r]) continue; seen[r] = true;
                            if (lane_of[r] < 0 || aug(lane_of[r], seen)) { lane_of[r] = q; quad_of[q] = r; return true; } }
                        return false;
                    };
                    for (int oq = 0; oq < 16; oq++) { const int q = ord[oq]; if (rem[q].empty()) continue; bool seen[16] = {false}; aug(q, seen); }
                    bool used[16] = {false};
                    for (int q = 0; q < 16; q++) if (quad_of[q] >= 0) used[quad_of[q]] = true;
                    for (int q = 0; q < 16; q++) {
                        const size_t l = (size_t)wv * 64 + GROUPS[gi][q];
                        if (rem[q].empty()) continue;
                        int pick = -1;
                        if (quad_of[q] >= 0) { for (size_t e = 0; e < rem[q].size(); e++) if ((int)(rem[q][e].first & 15) == quad_of[q]) { pick = (int)e; break; } }
                        else if (slack[q] > 0) { slack[q]--; continue; }                       // wait: a padding slot now (filled below), a real edge later
                        else pick = 0;                                                            // no room to wait: a conflict
                        put(j, l, k, rem[q][pick].first, rem[q][pick].second);
                        rem[q].erase(rem[q].begin() + pick);
                    }
                    // padding slots of this position (weight 0): a quad nobody reads
                    for (int q = 0; q < 16; q++) {
                        const size_t l = (size_t)wv * 64 + GROUPS[gi][q];
                        const size_t slot = base[j] + k;
                        if (wt[slot * lanes + l] != 0 || ((ot[(slot / 2) * lanes + l] >> (16 * (slot & 1))) & 0xFFFFu) != 0) continue;     // (a real edge with weight 0 and index 0 is re-pointed harmlessly: 0 * x)
                        int r = 0; while (r < 15 && used[r]) r++;
                        used[r] = true;
                        if ((uint32_t)r < (uint32_t)g.L) ot[(slot / 2) * lanes + l] |= ((uint32_t)r * 16u) << (16 * (slot & 1));
                    }
                }
                for (int q = 0; q < 16; q++) if (!rem[q].empty()) return 0;                      // (cannot happen: every lane places one edge per slot once its slack is spent)
            }
        }
    f.in_off = (uint32_t)p.in_off; f.in_len = (uint32_t)g.L; f.out_off = (uint32_t)p.out_off; f.out_len = (uint32_t)R;
    HB_TRY(upload(ctx, &f.d_wt, wt)); HB_TRY(upload(ctx, &f.d_ot, ot)); HB_TRY(upload(ctx, &f.d_oidx, oidx)); HB_TRY(upload(ctx, &f.d_w, wid));
    f.ok = true;
    return 0;
}
// Narrow form of the steps between C_1 and D_0 (hobbit_ctx.hpp NarrowPlan).  Leaves np.ok false when the code does not have the five-step shape the
// kernel was compiled for, or an output has more in-edges than the lanes of its position have slots: launch_encode then runs these steps as before.
static int build_narrow(hobbit_ctx *ctx, const std::vector<PlanStep> &plan, NarrowPlan &np) {
    if (plan.size() != NARROW_STEPS + 3) return 0;
    const long long x2 = plan[2].in_off;
    for (uint32_t s = 0; s < NARROW_STEPS; s++) {
        const PlanStep &p = plan[2 + s];
        if (p.g->L != (long long)NARROW_L[s] || p.g->R != (long long)NARROW_R[s] || p.in_off != x2 + NARROW_IN[s] || p.out_off != x2 + NARROW_OUT[s]) return 0;
    }
    std::vector<uint32_t> wt((size_t)NARROW_SLOTS * 64, 0), ot((size_t)NARROW_OREGS * 64, 0), q((size_t)NARROW_QREGS * 64, 0xFFFFFFFFu);
    uint32_t pos = 0, slot8 = 0, slot16 = 0, wslot = 0;
    for (uint32_t s = 0; s < NARROW_STEPS; s++) {
        const InEdges rows = in_edges(*plan[2 + s].g);
        const std::vector<uint32_t> order = by_in_degree(rows);
        size_t next = 0;
        for (; pos < NARROW_POS && NARROW_STEP_OF[pos] == s; pos++) {
            const uint32_t lpo = NARROW_LPO[pos], cap = NARROW_CAP[pos], cnt = 64 / lpo;
            const bool bytes = pos < NARROW_BYTE_POS;
            for (uint32_t t = 0; t < cnt && next + t < rows.size(); t++) {
                const uint32_t out = order[next + t];
                const auto &row = rows[out];
                if (row.size() > (size_t)cap * lpo) return 0;
                for (size_t e = 0; e < row.size(); e++) {                  // edge e of the output: slot e / lpo of lane group member e % lpo
                    const uint32_t lane = t * lpo + (uint32_t)(e % lpo), k = (uint32_t)(e / lpo);
                    wt[(size_t)(wslot + k) * 64 + lane] = (uint32_t)row[e].second.re;
                    if (bytes) { const uint32_t sl = slot8 + k; ot[(size_t)(sl >> 2) * 64 + lane] |= row[e].first << (8 * (sl & 3)); }
                    else { const uint32_t sl = slot16 + k; ot[(size_t)((NARROW_SLOTS8 + 3) / 4 + (sl >> 1)) * 64 + lane] |= ((NARROW_IN[s] + row[e].first) * 16u) << (16 * (sl & 1)); }
                }
                uint32_t &qq = q[(size_t)(pos >> 1) * 64 + t * lpo];       // the group's first lane stores the output
                qq = (qq & ~(0xFFFFu << (16 * (pos & 1)))) | (((NARROW_OUT[s] + out) * 16u) << (16 * (pos & 1)));
            }
            next = std::min(rows.size(), next + cnt);
            wslot += cap; (bytes ? slot8 : slot16) += cap;
        }
        if (next < rows.size()) return 0;
    }
    np.x2_off = (uint32_t)x2;
    HB_TRY(upload(ctx, &np.d_wt, wt)); HB_TRY(upload(ctx, &np.d_ot, ot)); HB_TRY(upload(ctx, &np.d_q, q));
    np.ok = true;
    return 0;
}
// The slice tables of k_encode (hobbit_ctx.hpp EncStep) from the plan hobbit_graph_finalize kept: built by the finalize for codes whose codeword
// fits LDS, by the first launch_encode (through ensure_tiled) for longer ones.
static int build_slices(hobbit_ctx *ctx) {
    DeviceCode &c = ctx->code;
    if (c.slices_built) return 0;
    const std::vector<PlanStep> &plan = c.plan;
    std::vector<uint32_t> slice_ptr, slice_width, slice_out, eidx; std::vector<uint2> e32; std::vector<F> ew;
    size_t pos = 0;
    for (auto &p : plan) {
        const HostGraph &g = *p.g;
        const InEdges rows = in_edges(g);
        EncStep s; s.in_off = (uint32_t)p.in_off; s.out_off = (uint32_t)p.out_off; s.out_len = (uint32_t)g.R;
        const uint32_t sw = (uint32_t)g.R >= ENC_WIDE_MIN ? 64u : ENC_SW, split = 64 / sw;
        // records per output are padded to the lane-group count, and for the wide steps to whole unrolled groups (no remainder loop)
        const uint32_t pad = sw == 64 ? ENC_UNROLL : split;
        s.sw = sw; s.out_base = (uint32_t)slice_out.size();
        s.n_slices = (uint32_t)((g.R + sw - 1) / sw); s.slice_base = (uint32_t)slice_ptr.size();
        const std::vector<uint32_t> order = by_in_degree(rows);
        for (uint32_t sl = 0; sl < s.n_slices; sl++) {
            size_t width = 0;
            for (uint32_t l = 0; l < sw; l++) { size_t q = (size_t)sl * sw + l; if (q < (size_t)g.R) width = std::max(width, rows[order[q]].size()); }
            width = (width + pad - 1) / pad * pad;
            slice_ptr.push_back((uint32_t)pos); slice_width.push_back((uint32_t)width);
            for (uint32_t l = 0; l < sw; l++) { size_t q = (size_t)sl * sw + l; slice_out.push_back(q < (size_t)g.R ? order[q] : 0xFFFFFFFFu); }
            for (size_t k = 0; k < width; k++)
                for (uint32_t l = 0; l < sw; l++) {
                    size_t q = (size_t)sl * sw + l;
                    uint32_t id = 0; F w = fmake(0);
                    if (q < (size_t)g.R && k < rows[order[q]].size()) { id = rows[order[q]][k].first; w = rows[order[q]][k].second; c.n_edges++; }
                    if (c.small_weights) e32.push_back(make_uint2(id, (uint32_t)w.re)); else { eidx.push_back(id); ew.push_back(w); }
                }
            pos += width * sw;
        }
        c.steps.push_back(s);
    }
    c.n_edges_padded = pos;
    // slice_ptr holds record offsets as 32 bits, and the plan's offsets (at most 2n) and the CSR pointers of ensure_ilv are 32-bit too
    if (pos >> 32) return ctx->fail(HOBBIT_EINVAL, "graph_finalize: more than 2^32 padded edge records");
    HB_TRY(upload(ctx, &c.d_steps, c.steps));
    HB_TRY(upload(ctx, &c.d_slice_ptr, slice_ptr));
    HB_TRY(upload(ctx, &c.d_slice_width, slice_width));
    HB_TRY(upload(ctx, &c.d_slice_out, slice_out));
    if (c.small_weights) HB_TRY(upload(ctx, &c.d_edges32, e32));
    else { HB_TRY(upload(ctx, &c.d_eidx, eidx)); HB_TRY(upload(ctx, &c.d_ew, ew)); }
    c.slices_built = true;
    return 0;
}
// Long codes (codeword over 160 KB): the outer steps whose windows do not fit in LDS, in tiled form (hobbit_ctx.hpp TiledStep).  Built by the
// first launch_encode of the finalized code, from the plan hobbit_graph_finalize kept.
int ensure_tiled(hobbit_ctx *ctx) {
    DeviceCode &c = ctx->code;
    if (c.tiled_built) return 0;
    if (c.graph_gen != ctx->graph_gen) return ctx->fail(HOBBIT_ESTATE, "encode: the graphs changed after hobbit_graph_finalize");
    HB_TRY(build_slices(ctx));
    const std::vector<PlanStep> &plan = c.plan;
    const std::vector<long long> &cwlen = c.cwlen;
    const uint32_t D = (uint32_t)cwlen.size() - 1;
    uint32_t d = 0;
    while (d < (uint32_t)D && cwlen[d] > TILE_MID_MAX) d++;
    c.tiled_depth = d;
    std::vector<uint32_t> tptr, twid, tout, teidx; std::vector<uint2> te32; std::vector<F> tew;
    for (size_t si = 0; si < plan.size(); si++) {
        if (si >= d && si < plan.size() - d) continue;
        const HostGraph &g = *plan[si].g;
        TiledStep t;
        t.in_off = (uint32_t)plan[si].in_off; t.in_len = (uint32_t)g.L; t.out_off = (uint32_t)plan[si].out_off; t.out_len = (uint32_t)g.R;
        t.ntiles = (t.in_len + TILE_ELEMS - 1) / TILE_ELEMS;
        t.n_slices = (t.out_len + 63) / 64;
        t.groups = (t.n_slices + TILE_WAVES * TILE_MAXS - 1) / (TILE_WAVES * TILE_MAXS);
        t.tile_base = (uint32_t)tptr.size(); t.out_base = (uint32_t)tout.size();
        // in-edges in input order, so that those of one tile are a contiguous run: tile k of output o is [beg(o, k), beg(o, k + 1))
        const InEdges rows = in_edges(g);
        auto beg = [&](uint32_t o, uint32_t k) {
            return (size_t)(std::lower_bound(rows[o].begin(), rows[o].end(), k * TILE_ELEMS, [](const std::pair<uint32_t, F> &e, uint32_t v) { return e.first < v; }) - rows[o].begin());
        };
        const std::vector<uint32_t> order = by_in_degree(rows);
        for (uint32_t sl = 0; sl < t.n_slices; sl++) {
            for (uint32_t l = 0; l < 64; l++) { const size_t q = (size_t)sl * 64 + l; tout.push_back(q < order.size() ? order[q] : 0xFFFFFFFFu); }
            for (uint32_t k = 0; k < t.ntiles; k++) {
                size_t lo[64], hi[64], width = 0;
                for (uint32_t l = 0; l < 64; l++) {
                    const size_t q = (size_t)sl * 64 + l;
                    lo[l] = hi[l] = 0;
                    if (q < order.size()) { lo[l] = beg(order[q], k); hi[l] = beg(order[q], k + 1); width = std::max(width, hi[l] - lo[l]); }
                }
                width = (width + ENC_UNROLL - 1) / ENC_UNROLL * ENC_UNROLL;
                tptr.push_back((uint32_t)c.tile_records); twid.push_back((uint32_t)width);
                for (size_t e = 0; e < width; e++)
                    for (uint32_t l = 0; l < 64; l++) {
                        uint32_t id = 0; F w = fmake(0);
                        if (lo[l] + e < hi[l]) { const auto &r = rows[order[(size_t)sl * 64 + l]][lo[l] + e]; id = r.first - k * TILE_ELEMS; w = r.second; }
                        if (c.small_weights) te32.push_back(make_uint2(id, (uint32_t)w.re)); else { teidx.push_back(id); tew.push_back(w); }
                    }
                c.tile_records += width * 64;
            }
        }
        c.tsteps.push_back(t);
    }
    HB_TRY(upload(ctx, &c.d_tile_ptr, tptr));
    HB_TRY(upload(ctx, &c.d_tile_width, twid));
    HB_TRY(upload(ctx, &c.d_tile_out, tout));
    if (c.small_weights) HB_TRY(upload(ctx, &c.d_tile_e32, te32));
    else { HB_TRY(upload(ctx, &c.d_tile_eidx, teidx)); HB_TRY(upload(ctx, &c.d_tile_ew, tew)); }
    c.tiled_built = true;
    return 0;
}
// The rows-innermost encode's steps (hobbit_ctx.hpp IlvStep): every step of the plan, its outputs' in-edges in input order (a counting sort by
// output), built by the first hobbit_encode_interleaved / hobbit_brakedown_commit of the finalized code.
int ensure_ilv(hobbit_ctx *ctx) {
    DeviceCode &c = ctx->code;
    if (c.ilv_built) return 0;
    if (c.graph_gen != ctx->graph_gen) return ctx->fail(HOBBIT_ESTATE, "encode: the graphs changed after hobbit_graph_finalize");
    std::vector<uint32_t> ptr; std::vector<uint2> e32; std::vector<uint32_t> eidx; std::vector<F> ew;
    size_t total = 0;
    for (const PlanStep &p : c.plan) total += (size_t)p.g->L * p.g->degree;
    if (total >= 0xFFFFFFFFu) return ctx->fail(HOBBIT_EINVAL, "encode_interleaved: too many edges");
    if (c.small_weights) e32.resize(total); else { eidx.resize(total); ew.resize(total); }
    size_t base = 0;
    c.isteps.clear();
    for (const PlanStep &p : c.plan) {
        const HostGraph &g = *p.g;
        const size_t R = (size_t)g.R, E = (size_t)g.L * g.degree;
        c.isteps.push_back({(uint32_t)p.in_off, (uint32_t)p.out_off, (uint32_t)R, (uint32_t)ptr.size()});
        std::vector<uint32_t> cnt(R + 1, 0);
        for (size_t e = 0; e < E; e++) cnt[(size_t)g.nbr[e] + 1]++;
        for (size_t t = 0; t < R; t++) cnt[t + 1] += cnt[t];
        for (size_t t = 0; t <= R; t++) ptr.push_back((uint32_t)(base + cnt[t]));
        for (long long i = 0; i < g.L; i++)                     // edges of input i in increasing i: each output's list is in input order
            for (int j = 0; j < g.degree; j++) {
                const size_t e = (size_t)i * g.degree + j, at = base + cnt[(size_t)g.nbr[e]]++;
                if (c.small_weights) e32[at] = make_uint2((uint32_t)i, (uint32_t)g.w[e].re); else { eidx[at] = (uint32_t)i; ew[at] = g.w[e]; }
            }
        base += E;
    }
    HB_TRY(upload(ctx, &c.d_ilv_ptr, ptr));
    if (c.small_weights) HB_TRY(upload(ctx, &c.d_ilv_e32, e32));
    else { HB_TRY(upload(ctx, &c.d_ilv_eidx, eidx)); HB_TRY(upload(ctx, &c.d_ilv_ew, ew)); }
    c.ilv_built = true;
    return 0;
}
// The segment table of the parity matrix' access lists (hobbit_ctx.hpp ParitySeg) from the finalized plan: the recursion of
// generate_access_idx (src/sumcheck.cpp:2622-2669) unrolled -- C-edges(d), C-identity(d) for d = 0 .. D-1, then D-edges(d), D-identity(d) for
// d = D-1 .. 0.  Depth d adds lvl_d = R_C(0) + .. + R_C(d-1) to every idx1 of its four segments (the reference's *lvl of depth d: the
// `+= R` at the end of a call reaches no list entry) and starts its idx2 at the plan's offsets.  Host only; *m: the entry count.
int parity_segments(hobbit_ctx *ctx, std::vector<ParitySeg> &segs, size_t *m) {
    const DeviceCode &c = ctx->code;
    if (c.graph_gen != ctx->graph_gen) return ctx->fail(HOBBIT_ESTATE, "parity_commit: the graphs changed after hobbit_graph_finalize");
    const size_t D = c.plan.size() / 2;
    std::vector<long long> lvl(D + 1, 0);
    for (size_t d = 0; d < D; d++) lvl[d + 1] = lvl[d] + c.plan[d].g->R;
    size_t base = 0, src = 0;
    bool fits = true;
    segs.clear();
    auto put = [&](const PlanStep &p, size_t d) {
        const HostGraph &g = *p.g;
        const size_t E = (size_t)g.L * (size_t)g.degree;
        fits = fits && base + E + (size_t)g.R < ((size_t)1 << 31) && lvl[d] < (1LL << 31) && p.out_off < (1LL << 31);
        segs.push_back({(uint32_t)base, (uint32_t)E, (uint32_t)g.degree, (uint32_t)lvl[d], (uint32_t)p.in_off, 0u, (uint32_t)src, (uint32_t)g.L});
        base += E; src += E;
        segs.push_back({(uint32_t)base, (uint32_t)g.R, 1u, (uint32_t)lvl[d], (uint32_t)p.out_off, 1u, 0u, (uint32_t)g.R});
        base += (size_t)g.R;
    };
    for (size_t d = 0; d < D; d++) put(c.plan[d], d);
    for (size_t d = D; d-- > 0;) put(c.plan[2 * D - 1 - d], d);
    if (!fits) return ctx->fail(HOBBIT_EINVAL, "parity_commit: list length outside the public witness' 8P layout");
    *m = base;
    return 0;
}
// The forward form behind hobbit_parity_commit_device, built by the first such commit of the finalized code: every level's neighbours (u32) and
// weights (u32 under small_weights, else F) in list order, and the segment table.  The index ranges are checked here from the table, in
// O(levels): hobbit_graph_upload bounds every neighbour by R.
int ensure_fwd(hobbit_ctx *ctx) {
    DeviceCode &c = ctx->code;
    if (c.fwd_built) return 0;
    std::vector<ParitySeg> segs; size_t m = 0;
    HB_TRY(parity_segments(ctx, segs, &m));
    const size_t S = 2 * (size_t)c.n;
    for (size_t s = 0; s < segs.size(); s += 2) {
        const size_t R = segs[s + 1].count;                     // the level's R: bound of its neighbours, length of its identity run
        if (segs[s].lvl + R > S || (size_t)segs[s].off + segs[s].cells > S || (size_t)segs[s + 1].off + R > S)
            return ctx->fail(HOBBIT_EINVAL, "parity_commit: list index beyond the 2n cells");
    }
    size_t total = 0;
    for (const PlanStep &p : c.plan) total += (size_t)p.g->L * (size_t)p.g->degree;
    std::vector<uint32_t> nbr(total), w32; std::vector<F> w;
    if (c.small_weights) w32.resize(total); else w.resize(total);
    size_t at = 0;
    for (const PlanStep &p : c.plan) {
        const HostGraph &g = *p.g;
        const size_t E = (size_t)g.L * (size_t)g.degree;
        for (size_t e = 0; e < E; e++) nbr[at + e] = (uint32_t)g.nbr[e];
        if (c.small_weights) for (size_t e = 0; e < E; e++) w32[at + e] = (uint32_t)g.w[e].re;
        else for (size_t e = 0; e < E; e++) w[at + e] = g.w[e];
        at += E;
    }
    HB_TRY(upload(ctx, &c.d_fwd_segs, segs));
    HB_TRY(upload(ctx, &c.d_fwd_nbr, nbr));
    if (c.small_weights) HB_TRY(upload(ctx, &c.d_fwd_w32, w32)); else HB_TRY(upload(ctx, &c.d_fwd_w, w));
    c.fwd_segs = segs; c.fwd_m = m; c.fwd_built = true;
    return 0;
}
int need_device_bytes(hobbit_ctx *ctx, size_t bytes, const char *what) {
    size_t free_b = 0, total_b = 0;
    hipSetDevice(ctx->device);
    HB_CHECK(ctx, hipMemGetInfo(&free_b, &total_b));
    if (free_b < bytes) {
        char msg[256];
        snprintf(msg, sizeof msg, "%s: needs about %.1f GiB of device memory, %.1f GiB are free", what, (double)bytes / 1073741824.0, (double)free_b / 1073741824.0);
        return ctx->fail(HOBBIT_ENOMEM, msg);
    }
    return 0;
}
}  // namespace hobbit
extern "C" {
int hobbit_graph_finalize(hobbit_ctx *ctx, long long n, long long *len_out) {
    hipStreamSynchronize(ctx->stream);
    ctx->code = DeviceCode();                                     // (the owners in it free their tables: the stream has drained)
    DeviceCode &c = ctx->code;
    const long long thr = 13;   // distance_threshold, src/parameter.h:5
    if (n <= 0 || n > (1LL << CODE_MAX_LOG)) return ctx->fail(HOBBIT_EINVAL, "graph_finalize: bad n");
    // level sizes and offsets
    std::vector<long long> nd{n}, off{0};
    int D = 0;
    while (nd[D] > thr) {
        auto it = ctx->graphs.find({D, 0});
        if (it == ctx->graphs.end() || it->second.L != nd[D]) return ctx->fail(HOBBIT_ESTATE, "graph_finalize: missing or mismatched _C level");
        off.push_back(off[D] + nd[D]); nd.push_back(it->second.R); D++;
    }
    std::vector<long long> cwlen(D + 1); cwlen[D] = nd[D];
    for (int d = D - 1; d >= 0; d--) {
        auto it = ctx->graphs.find({d, 1});
        if (it == ctx->graphs.end() || it->second.L != cwlen[d + 1]) return ctx->fail(HOBBIT_ESTATE, "graph_finalize: missing or mismatched D level");
        cwlen[d] = nd[d] + cwlen[d + 1] + it->second.R;
    }
    c.n = n; c.len = cwlen[0];
    if (c.len > 2 * n) return ctx->fail(HOBBIT_EINVAL, "graph_finalize: codeword longer than 2n");
    std::vector<PlanStep> &plan = c.plan;
    for (int d = 0; d < D; d++) plan.push_back({&ctx->graphs[{d, 0}], off[d], off[d] + nd[d]});
    for (int d = D - 1; d >= 0; d--) plan.push_back({&ctx->graphs[{d, 1}], off[d + 1], off[d + 1] + cwlen[d + 1]});
    c.small_weights = true;
    for (auto &p : plan) for (auto &w : p.g->w) if (w.im != 0 || w.re >> 32) { c.small_weights = false; break; }
    // base-field weights: Enc(conj x) = conj(Enc x), what a half commitment rests on (hobbit_commit_standard_real asks)
    c.real_weights = true;
    for (auto &p : plan) for (auto &w : p.g->w) if (w.im != 0) { c.real_weights = false; break; }
    // The slice tables of k_encode.  A code whose codeword fits LDS (up to 160 KB) gets them now; a longer one when its first launch_encode asks
    // for its tiled steps (ensure_tiled): the rows-innermost encode, the code proof and the parity matrix never read them, and at n = 2^21 they
    // were 3.2 s of a 3.2 s finalize
    if ((size_t)c.len * 16 <= 160 * 1024) HB_TRY(build_slices(ctx));
    // deep codes (n = 4096: the codeword does not leave room for two workgroups per CU): first, second and last step also in fat form
    if (c.small_weights && c.steps.size() >= 4 && (size_t)c.len * 16 > 80 * 1024 && (size_t)c.len * 16 <= 160 * 1024) {
        const uint32_t capA[3] = {FAT_A_CAP0, FAT_A_CAP1, 0}, capC1[3] = {FAT_C1_CAP0, 0, 0}, capD[3] = {FAT_D_CAP0, FAT_D_CAP1, FAT_D_CAP2};
        HB_TRY(build_fat_step(ctx, plan.front(), FAT_A_NOUT, FAT_A_CONS, capA, c.fatA));
        HB_TRY(build_fat_step(ctx, plan.back(), FAT_D_NOUT, FAT_D_CONS, capD, c.fatD));
        HB_TRY(build_fat_step(ctx, plan[1], FAT_C1_NOUT, FAT_C1_CONS, capC1, c.fatC1));
        HB_TRY(build_narrow(ctx, plan, c.narrow));
    }
    // the long codes' tiled steps and the rows-innermost CSR steps are built on first use from c.plan (ensure_tiled / ensure_ilv): a context
    // that only runs one of the two encodes does not pay for the other's plan
    c.cwlen = cwlen; c.graph_gen = ctx->graph_gen;
    if (len_out) *len_out = c.len;
    return 0;
}
// Which kernel forms hobbit_graph_finalize chose for the finalized code (include/hobbit_hip.h).  Host only: reads the code's flags.
int hobbit_encode_forms(hobbit_ctx *ctx, unsigned *flags, unsigned *tiled_depth) {
    const DeviceCode &c = ctx->code;
    if (!c.n || c.graph_gen != ctx->graph_gen) return ctx->fail(HOBBIT_ESTATE, "encode_forms: no finalized code (hobbit_graph_finalize)");
    const bool pending = (size_t)c.len * 16 > 160 * 1024 && !c.tiled_built;
    if (flags) *flags = (c.small_weights ? HOBBIT_FORM_SMALL_WEIGHTS : 0u) | (c.fatA.ok ? HOBBIT_FORM_FAT_A : 0u) | (c.fatC1.ok ? HOBBIT_FORM_FAT_C1 : 0u) |
                        (c.fatD.ok ? HOBBIT_FORM_FAT_D : 0u) | (c.narrow.ok ? HOBBIT_FORM_NARROW : 0u) | (pending ? HOBBIT_FORM_TILED_PENDING : 0u);
    if (tiled_depth) *tiled_depth = c.tiled_built ? c.tiled_depth : 0u;
    return 0;
}
int hobbit_encode_batch(hobbit_ctx *ctx, const hobbit_F *d_src, hobbit_F *d_dst, long long n, size_t batch, size_t ld_src, size_t ld_dst) {
    if (n <= 0 || ld_src < (size_t)n || ld_dst < (size_t)(2 * n)) return ctx->fail(HOBBIT_EINVAL, "encode_batch: bad n / leading dimensions");
    // in place (the messages already sit at the head of their codewords): nothing to copy, and the deep-code kernels apply
    const bool in_place = (const void *)d_src == (const void *)d_dst && ld_src == ld_dst;
    return launch_encode(ctx, cF(d_src), ld_src, mF(d_dst), ld_dst, n, batch, in_place ? 0 : 1);
}

// ---- BLAKE3 / Merkle --------------------------------------------------------------------------
int hobbit_blake3_64(hobbit_ctx *ctx, const uint8_t *d_in, uint8_t *d_out, size_t n) { return launch_blake3_64(ctx, d_in, d_out, n); }
int hobbit_hash_md(hobbit_ctx *ctx, const hobbit_F *d_xyzw, const uint8_t *d_prev, uint8_t *d_out, size_t n) { return launch_hash_md(ctx, cF(d_xyzw), d_prev, d_out, n); }
int hobbit_merkle_levels(hobbit_ctx *ctx, uint8_t *d_levels, size_t n, int quirk) {
    if (ilog2_exact(n) < 0) return ctx->fail(HOBBIT_EINVAL, "merkle_levels: n must be a power of two");
    return launch_merkle_levels(ctx, d_levels, n, quirk);
}
int hobbit_mt_commit_blake(hobbit_ctx *ctx, const hobbit_F *d_leafs, size_t N, uint8_t *d_levels) {
    if (N < 4 || ilog2_exact(N / 4) < 0 || N % 4) return ctx->fail(HOBBIT_EINVAL, "mt_commit_blake: N/4 must be a power of two");
    HB_TRY(launch_blake3_64(ctx, reinterpret_cast<const uint8_t *>(d_leafs), d_levels, N / 4));
    return launch_merkle_levels(ctx, d_levels, N / 4, 1);
}
static int paths_common(hobbit_ctx *ctx, const uint8_t *d_levels, size_t n, const uint64_t *h_pos, size_t nq, uint8_t *h_paths) {
    int depth = ilog2_exact(n);
    if (depth < 0) return ctx->fail(HOBBIT_EINVAL, "merkle_path: n must be a power of two");
    for (size_t q = 0; q < nq; q++) if (h_pos[q] >= n) return ctx->fail(HOBBIT_EINVAL, "merkle_path: position out of range");   // src/merkle_tree.cpp:310-313
    if (depth == 0 || nq == 0) return 0;
    StageScope sc(ctx);
    uint8_t *buf; size_t pbytes = nq * 8, obytes = nq * depth * 32;
    HB_TRY(ctx->workspace(pbytes + obytes + 64, (void **)&buf));     // (the staged read-back is queued right behind the kernel: later users of the workspace come after it)
    uint8_t *d_paths = buf; uint64_t *d_pos = reinterpret_cast<uint64_t *>(buf + ((obytes + 15) / 16) * 16);
    HB_TRY(h2d_staged(ctx, d_pos, h_pos, pbytes));
    HB_TRY(launch_merkle_paths(ctx, d_levels, n, d_pos, nq, depth, d_paths));
    HB_TRY(d2h_staged(ctx, h_paths, d_paths, obytes));
    return sc.finish();
}
int hobbit_merkle_path(hobbit_ctx *ctx, const uint8_t *d_levels, size_t n, size_t pos, uint8_t *h_path) {
    uint64_t p = pos; return paths_common(ctx, d_levels, n, &p, 1, h_path);
}
int hobbit_merkle_paths(hobbit_ctx *ctx, const uint8_t *d_levels, size_t n, const uint64_t *h_pos, size_t nq, uint8_t *h_paths) {
    return paths_common(ctx, d_levels, n, h_pos, nq, h_paths);
}

// ---- multilinear utilities --------------------------------------------------------------------
int hobbit_eq_table(hobbit_ctx *ctx, const hobbit_F *h_r, int k, hobbit_F *d_out) {
    if (k < 0 || k > 34) return ctx->fail(HOBBIT_EINVAL, "eq_table: bad k");
    return launch_eq_table(ctx, cF(h_r), k, mF(d_out));
}
// the evaluation left on the device: *d_res points at it (in ctx->workspace, or d_v itself for n = 1), valid until the workspace's next user
static int eval_vector_dev(hobbit_ctx *ctx, const hobbit_F *d_v, size_t n, const hobbit_F *h_r, const F **d_res) {
    int lg = ilog2_exact(n);
    if (lg < 0) return ctx->fail(HOBBIT_EINVAL, "eval_vector: n must be a power of two");
    if (lg == 0) { *d_res = cF(d_v); return 0; }
    F *ws; HB_TRY(ctx->workspace((n / 2 + n / 4 + 2) * sizeof(F), (void **)&ws));
    F *a = ws, *b = ws + n / 2;
    const F *src = cF(d_v);
    F *dst = a;
    // two levels per launch while the table is large, the last (up to 12) levels in one workgroup: 7 launches instead of 24 at n = 2^24
    int i = 0;
    while (lg - i > 12 || (lg - i > 1 && ((size_t)n >> i) > 4096)) {
        if (lg - i >= 2) { HB_TRY(launch_eval_fold2(ctx, src, dst, n >> (i + 2), cF(h_r)[i], cF(h_r)[i + 1])); i += 2; }
        else { HB_TRY(launch_eval_fold(ctx, src, dst, n >> (i + 1), cF(h_r)[i])); i += 1; }
        src = dst; dst = dst == a ? b : a;
    }
    if (i < lg) {
        std::vector<F> rt((size_t)(lg - i)); for (int q = i; q < lg; q++) rt[(size_t)(q - i)] = cF(h_r)[q];
        HB_TRY(launch_eval_tail(ctx, src, dst, n >> i, lg - i, rt.data()));
        src = dst;
    }
    *d_res = src; return 0;
}
int hobbit_eval_vector(hobbit_ctx *ctx, const hobbit_F *d_v, size_t n, const hobbit_F *h_r, hobbit_F *h_out) {
    const F *d_res; HB_TRY(eval_vector_dev(ctx, d_v, n, h_r, &d_res));
    return hobbit_memcpy_d2h(ctx, h_out, d_res, sizeof(F));       // a public call: h_out is final on return
}

// ---- tensor code / commit ---------------------------------------------------------------------
// Streams a caller's (pageable) host polynomial to the device in `groups` equal parts, each in 64 MiB pieces through two pinned staging buffers:
// piece p + 1 is copied into its buffer by a few host threads while piece p crosses PCIe; group g's last piece records ready[g] on the copy
// stream.  The commit's row-FFT loop waits for ready[g] and, once group g's kernels are queued, starts group g + 1 -- so the upload of one
// chunk group overlaps the device work of the previous one (hobbit_commit_standard_host).
struct Uploader {
    hobbit_ctx *ctx; const unsigned char *h; unsigned char *d; size_t group_bytes; int groups, started = 0, piece_no = 0;
    int start(int g) {
        if (g != started || g >= groups) return 0;
        started++;
        const unsigned char *src = h + (size_t)g * group_bytes; unsigned char *dst = d + (size_t)g * group_bytes;
        for (size_t off = 0; off < group_bytes; off += hobbit_ctx::UP_PIECE, piece_no++) {
            const size_t n = std::min(hobbit_ctx::UP_PIECE, group_bytes - off); const int b = piece_no & 1;
            // every refill waits for the piece's last transfer, the first two of a call included: an earlier hobbit_commit_standard_host on this
            // context returns with its last pieces still on the bus (an event that was never recorded returns at once)
            if (hipEventSynchronize(ctx->up_done[b]) != hipSuccess) return ctx->fail(HOBBIT_EHIP, "upload: staging buffer wait failed");
            unsigned char *pin = (unsigned char *)ctx->up_pin[b].get();
            par_memcpy(pin, src + off, n);
            HB_CHECK(ctx, hipMemcpyAsync(dst + off, pin, n, hipMemcpyHostToDevice, ctx->up_stream));
            HB_CHECK(ctx, hipEventRecord(ctx->up_done[b], ctx->up_stream));
        }
        HB_CHECK(ctx, hipEventRecord(ctx->up_ready[g], ctx->up_stream));
        return 0;
    }
    int wait(int g, hipStream_t s) { HB_TRY(start(g)); HB_CHECK(ctx, hipStreamWaitEvent(s, ctx->up_ready[g], 0)); return 0; }
    int all(hipStream_t s) { for (int g = 0; g < groups; g++) HB_TRY(wait(g, s)); return 0; }
};
// msg_rot (commit_impl only; default off): where every piece of the rotated form exists -- linear-time code, trs = 4096, rows of 4096, a tensor of
// 64 MiB or more, the fat in-place encode -- the tensor's message half is written rotated (hobbit_rot.hpp) and *msg_rot becomes the ring's mask;
// every other shape and every other caller gets today's linear tensor and *msg_rot = 0.
static int tensorcode_chunks(hobbit_ctx *ctx, const F *d_msg, size_t M, int K, int trs, int lin, F *d_out, Uploader *up = nullptr, uint32_t *msg_rot = nullptr) {
    if (msg_rot) *msg_rot = 0;
    if (trs <= 0 || M % (size_t)trs) return ctx->fail(HOBBIT_EINVAL, "tensorcode: trs must divide M");
    size_t half = M / trs, cols = 2 * half, rows2 = 2 * (size_t)trs;
    int logc = ilog2_exact(cols), logr = ilog2_exact(rows2);
    if (logc < 1 || logc > 24) return ctx->fail(HOBBIT_EINVAL, "tensorcode: row length 2M/trs must be a power of two <= 2^24");
    if (logr < 1) return ctx->fail(HOBBIT_EINVAL, "tensorcode: trs must be a power of two");
    // rows: RS encode = zero-padded FFT (src/PC_utils.cpp:75-84,105-107)
    const bool piped_shape = logc <= 12 && (size_t)K * trs * cols * sizeof(F) >= ((size_t)64 << 20);
    const bool rotated = msg_rot && lin && piped_shape && logc == 12 && trs == 4096 && encode_reads_rotated(ctx, trs);
    if (up && !piped_shape) { up->groups = 1; up->group_bytes = (size_t)K * M * sizeof(F); HB_TRY(up->all(ctx->stream)); up = nullptr; }
    if (logc > 15) {
        // very long rows (test_PC option 1 at 2^27 and beyond: tensor_row_size stays 128): one chunk at a time through the long transform
        F *rm; HB_TRY(ctx->workspace3((size_t)trs * cols * sizeof(F), (void **)&rm));
        for (int i = 0; i < K; i++) {
            HB_TRY(fft::any_rows(ctx, d_msg + (size_t)i * M, half, half, rm, logc, false, (size_t)trs));
            HB_TRY(launch_transpose(ctx, rm, (size_t)trs * cols, (uint32_t)trs, (uint32_t)cols, d_out + (size_t)i * cols * rows2, cols * rows2, rows2, 1));
        }
    } else if (logc > 12) {
        // long rows (Elastic_PC opt 2: 32768): R strided FFT-4096 per row + twiddle/R-point combine, then transpose
        const size_t nrows = (size_t)K * trs;
        F *Y, *rm;
        HB_TRY(ctx->workspace(nrows * cols * sizeof(F), (void **)&Y));
        HB_TRY(ctx->workspace2(nrows * cols * sizeof(F), (void **)&rm));
        HB_TRY(fft::rowcode_combine(ctx, d_msg, logc, (uint32_t)nrows, Y, rm));
        HB_TRY(launch_transpose(ctx, rm, (size_t)trs * cols, (uint32_t)trs, (uint32_t)cols, d_out, cols * rows2, rows2, (uint32_t)K));
    } else
    // Large tensors: FFT to a row-major scratch (coalesced stores) + tiled transpose; small ones write the
    // transposed layout directly (one launch less, the scattered stores stay in L2).
    if ((size_t)K * trs * cols * sizeof(F) >= ((size_t)64 << 20)) {
        const char *pp_env = getenv("HOBBIT_COMMIT_PIPE");
        int pipe = pp_env ? atoi(pp_env) : (K % 8 == 0 ? 8 : K % 4 == 0 ? 4 : K % 2 == 0 ? 2 : 0);
        if (pipe > 56) pipe = 56;                                    // side_ev[0 .. pipe) are this loop's; 60, 62, 63 belong to the opening (OpenRun), 61 is free, 64/65 to the brackets below
        if (rotated) {
            // A commitment's tensor (hobbit_rot.hpp): the row FFT stores the codeword-major layout itself, each column's message half rotated, so
            // that the 4096 stores of a row spread over the memory channels instead of meeting on one.  No row-major scratch, no transpose and no
            // side stream; the chunk groups remain because the upload of hobbit_commit_standard_host is waited for group by group.
            const int groups = pipe > 1 && K % pipe == 0 ? pipe : 1, per = K / groups;
            if (up) { up->groups = groups; up->group_bytes = (size_t)per * M * sizeof(F); }
            for (int g = 0; g < groups; g++) {
                const size_t c0 = (size_t)g * per;
                if (up) HB_TRY(up->wait(g, ctx->stream));
                HB_TRY(fft::rowcode_4096(ctx, d_msg + c0 * M, half, d_out + c0 * cols * rows2, 1, rows2, (uint32_t)per, (uint32_t)trs, M, cols * rows2, (uint32_t)trs - 1));
                if (up) HB_TRY(up->start(g + 1));                 // (host copy + PCIe of the next group, beside this group's kernel)
            }
            *msg_rot = (uint32_t)trs - 1;
            return launch_encode(ctx, d_out, rows2, d_out, rows2, trs, (size_t)K * cols, 0, *msg_rot);
        }
        F *rm; HB_TRY(ctx->workspace2((size_t)K * trs * cols * sizeof(F), (void **)&rm));
        // Two-stream pipeline over chunk groups (default on; HOBBIT_COMMIT_PIPE=0 turns it off, =G asks for G groups): group g's layout
        // change (HBM-bound, next to no VALU work) runs on the side stream while group g+1's row FFT (VALU-bound, one pass over the
        // data) runs on the main one.  Same kernels, same bytes, bit-identical tensor; DESIGN.md section 4 has the A/B.
        if (pipe > 1 && K % pipe == 0) {
            HB_TRY(ctx->side_init());
            const int per = K / pipe; hipStream_t mainS = ctx->stream;
            // every exit from this block -- also an error inside the group loop -- leaves the side stream joined: the caller may free or re-use
            // d_out / the scratch right away
            struct SideJoin { hobbit_ctx *c; hipStream_t m; bool done = false; ~SideJoin() { c->stream = m; if (!done) hipStreamSynchronize(c->side); } } join{ctx, mainS};
            HB_CHECK(ctx, hipEventRecord(ctx->side_ev[64], mainS)); HB_CHECK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_ev[64], 0));   // d_out / rm are free for the side stream
            if (up) { up->groups = pipe; up->group_bytes = (size_t)per * M * sizeof(F); }
            for (int g = 0; g < pipe; g++) {
                const size_t c0 = (size_t)g * per;
                if (up) HB_TRY(up->wait(g, mainS));
                HB_TRY(fft::rows(ctx, d_msg + c0 * M, half, (uint32_t)half, rm + c0 * trs * cols, cols, 1, logc, false, (uint32_t)per, (uint32_t)trs, M, (size_t)trs * cols));
                HB_CHECK(ctx, hipEventRecord(ctx->side_ev[g], mainS)); HB_CHECK(ctx, hipStreamWaitEvent(ctx->side, ctx->side_ev[g], 0));
                ctx->stream = ctx->side;
                const int rc = launch_transpose(ctx, rm + c0 * trs * cols, (size_t)trs * cols, (uint32_t)trs, (uint32_t)cols, d_out + c0 * cols * rows2, cols * rows2, rows2, (uint32_t)per);
                ctx->stream = mainS;
                if (rc) return rc;
                if (up) HB_TRY(up->start(g + 1));                 // (host copy + PCIe of the next group, beside this group's kernels)
            }
            HB_CHECK(ctx, hipEventRecord(ctx->side_ev[65], ctx->side)); HB_CHECK(ctx, hipStreamWaitEvent(mainS, ctx->side_ev[65], 0));
            join.done = true;
        } else {
            if (up) { up->groups = 1; up->group_bytes = (size_t)K * M * sizeof(F); HB_TRY(up->all(ctx->stream)); }
            HB_TRY(fft::rows(ctx, d_msg, half, (uint32_t)half, rm, cols, 1, logc, false, (uint32_t)K, (uint32_t)trs, M, (size_t)trs * cols));
            HB_TRY(launch_transpose(ctx, rm, (size_t)trs * cols, (uint32_t)trs, (uint32_t)cols, d_out, cols * rows2, rows2, (uint32_t)K));
        }
    } else
        HB_TRY(fft::rows(ctx, d_msg, half, (uint32_t)half, d_out, 1, rows2, logc, false, (uint32_t)K, (uint32_t)trs, M, cols * rows2));
    if (lin) {     // columns: expander code, in place on contiguous codewords (src/PC_utils.cpp:110-121)
        if (trs > 13 && ctx->code.n != trs) return ctx->fail(HOBBIT_ESTATE, "tensorcode: expander graphs for n = trs not finalized");
        if (trs <= 13 && ctx->code.n != trs) { long long l; HB_TRY(hobbit_graph_finalize(ctx, trs, &l)); }
        return launch_encode(ctx, d_out, rows2, d_out, rows2, trs, (size_t)K * cols, 0);
    }
    if (logr > 12) return ctx->fail(HOBBIT_EINVAL, "tensorcode: RSxRS needs 2*trs <= 4096");
    // columns: RS (src/PC_utils.cpp:92-101)
    return fft::rows(ctx, d_out, rows2, (uint32_t)trs, d_out, rows2, 1, logr, false, 1, (uint32_t)((size_t)K * cols), 0, 0);
}
int hobbit_tensorcode(hobbit_ctx *ctx, const hobbit_F *d_msg, size_t M, int trs, int linear_time, hobbit_F *d_out) {
    return tensorcode_chunks(ctx, cF(d_msg), M, 1, trs, linear_time, mF(d_out));
}

static int commit_impl(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, int K, int trs, int linear_time, hobbit_commitment **out, Uploader *up);
int hobbit_commit_standard(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, int K, int trs, int linear_time, hobbit_commitment **out) {
    return commit_impl(ctx, d_poly, N, K, trs, linear_time, out, nullptr);
}
int hobbit_commit_standard_host(hobbit_ctx *ctx, const hobbit_F *h_poly, hobbit_F *d_poly, size_t N, int K, int trs, int linear_time, hobbit_commitment **out) {
    if (!h_poly || !d_poly) return ctx->fail(HOBBIT_EINVAL, "commit_standard_host: null polynomial");
    HB_TRY(ctx->up_init());
    Uploader up{ctx, reinterpret_cast<const unsigned char *>(h_poly), reinterpret_cast<unsigned char *>(d_poly), 0, 0};
    const int rc = commit_impl(ctx, d_poly, N, K, trs, linear_time, out, &up);
    if (rc) hipStreamSynchronize(ctx->up_stream);                 // nothing of the caller's buffer is still being read on an error return
    return rc;
}
// A commitment's tensor (tbytes: its real size, full or half form) and levels: the parked pair of the last freed commitment where both sizes are the
// same to the byte, fresh allocations otherwise.
static int commit_buffers(hobbit_ctx *ctx, size_t tbytes, size_t M, mem::Buf<F> &tensor, mem::Buf<uint8_t> &levels) {
    if (ctx->spare_tensor && ctx->spare_tensor.bytes() == tbytes && ctx->spare_levels.bytes() == 64 * M) {
        tensor = std::move(ctx->spare_tensor); levels = std::move(ctx->spare_levels);
        return 0;
    }
    if (ctx->spare_tensor) {          // a parked commitment of another shape: release it BEFORE allocating (it can be 16.5 GiB)
        HB_TRY(ctx->sync());
        ctx->spare_tensor.reset(); ctx->spare_levels.reset();
    }
    if (tensor.alloc_bytes(tbytes) || levels.alloc_bytes(64 * M)) {
        ctx->pool_drain();                                    // give back what the pool parks, then once more
        tensor.reset();
        if (tensor.alloc_bytes(tbytes) || levels.alloc_bytes(64 * M)) return ctx->fail(HOBBIT_ENOMEM, "commit_standard: tensor allocation failed");
    }
    return 0;
}
static int commit_impl(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, int K, int trs, int linear_time, hobbit_commitment **out, Uploader *up) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    if (K <= 0 || N % (size_t)K) return ctx->fail(HOBBIT_EINVAL, "commit_standard: K must divide N");
    size_t M = N / K;
    if (trs < 4 || trs % 4 || M % (size_t)trs) return ctx->fail(HOBBIT_EINVAL, "commit_standard: trs must be a multiple of 4 dividing N/K");
    if (ilog2_exact(M) < 0) return ctx->fail(HOBBIT_EINVAL, "commit_standard: N/K must be a power of two");
    size_t cols = 2 * M / trs, rows2 = 2 * (size_t)trs;
    Handle<hobbit_commitment, hobbit_commitment_free> c(new hobbit_commitment());
    c->ctx = ctx; c->N = N; c->M = M; c->K = K; c->trs = trs; c->lin = linear_time; c->cols = (uint32_t)cols; c->rows2 = (uint32_t)rows2;
    HB_TRY(commit_buffers(ctx, (size_t)K * cols * rows2 * sizeof(F), M, c->d_tensor, c->d_levels));
    const char *st_env = getenv("HOBBIT_COMMIT_SKIP_TAIL");
    ctx->enc_skip_tail = linear_time && !(st_env && st_env[0] == '0'); ctx->enc_tail_skipped = false;
    int r = tensorcode_chunks(ctx, cF(d_poly), M, K, trs, linear_time, c->d_tensor, up, &c->msg_rot);
    c->rows_valid = (!r && ctx->enc_tail_skipped) ? std::min<uint32_t>((uint32_t)rows2, ((uint32_t)ctx->code.len + 3) & ~3u) : (uint32_t)rows2;
    ctx->enc_skip_tail = false; ctx->enc_tail_skipped = false;
    // leaf chain over the K chunks (src/Our_PC.cpp:155-167), then the tree (src/Our_PC.cpp:169);
    // rows >= the codeword length are zero in every chunk of an RS x expander tensor (RS x RS fills all 2*trs rows)
    if (!r) r = launch_leaf_chain(ctx, c->d_tensor, cols * rows2, K, (uint32_t)cols, (uint32_t)(trs / 2), c->d_levels,
                                       linear_time && ctx->code.n == trs ? (uint32_t)ctx->code.len : (uint32_t)rows2, c->msg_rot);
    if (!r) r = launch_merkle_levels(ctx, c->d_levels, M, 1);
    if (r) return r;
    *out = c.release();
    return 0;
}
// ---- base-field polynomials (include/hobbit_real.h) ---------------------------------------------
// commit_impl for a real polynomial: the same stages over columns 0 .. cols / 2 of every chunk (hobbit_half.hpp).  The row code stores the half
// tensor's layout itself -- rotated where the full commit's would be, plainly transposed for the small tensors that fit the cache -- and goes through
// a row-major scratch of 2049 columns and the tiled transpose for the large tensors that are not rotated; the encode sees K cols / 2 + K columns.
static int commit_real_impl(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, int K, int trs, int linear_time, hobbit_commitment **out, Uploader *up) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    if (!d_poly) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real: null polynomial");
    if (K <= 0 || N % (size_t)K) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real: K must divide N");
    const size_t M = N / K;
    if (trs < 4 || trs % 4 || M % (size_t)trs) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real: trs must be a multiple of 4 dividing N/K");
    if (ilog2_exact(M) < 0) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real: N/K must be a power of two");
    if (!linear_time) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real: only the RS x expander code (linear_time = 1) has the half form; RS x RS is not built");
    const size_t cols = 2 * M / trs, rows2 = 2 * (size_t)trs;
    if (cols != 4096) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real: the row code must have 4096 points, 2 (N/K) / trs == 4096");
    if (trs > 13 && ctx->code.n != trs) return ctx->fail(HOBBIT_ESTATE, "commit_standard_real: expander graphs for n = trs not finalized");
    if (trs <= 13 && ctx->code.n != trs) { long long l; HB_TRY(hobbit_graph_finalize(ctx, trs, &l)); }
    if (!ctx->code.real_weights)
        return ctx->fail(HOBBIT_EINVAL, "commit_standard_real: a weight of the finalized graphs has img != 0, so column cols - c is not the conjugate of column c");
    Handle<hobbit_commitment, hobbit_commitment_free> c(new hobbit_commitment());
    c->ctx = ctx; c->N = N; c->M = M; c->K = K; c->trs = trs; c->lin = 1; c->cols = (uint32_t)cols; c->rows2 = (uint32_t)rows2; c->half = true;
    const size_t hcols = half_ncols((uint32_t)cols, (uint32_t)K);
    HB_TRY(commit_buffers(ctx, hcols * rows2 * sizeof(F), M, c->d_tensor, c->d_levels));
    const bool piped_shape = (size_t)K * trs * cols * sizeof(F) >= ((size_t)64 << 20);            // the full commit's threshold: the same shapes rotate
    const bool rotated = piped_shape && trs == 4096 && encode_reads_rotated(ctx, trs);
    c->msg_rot = rotated ? (uint32_t)trs - 1 : 0;
    const int pipe = K % 8 == 0 ? 8 : K % 4 == 0 ? 4 : K % 2 == 0 ? 2 : 1, groups = up && piped_shape ? pipe : 1, per = K / groups;
    if (up) { up->groups = groups; up->group_bytes = (size_t)per * M * sizeof(uint64_t); }
    F *rm = nullptr;
    if (piped_shape && !rotated) HB_TRY(ctx->workspace2((size_t)K * trs * 2049 * sizeof(F), (void **)&rm));
    for (int g = 0; g < groups; g++) {
        const size_t c0 = (size_t)g * per;
        if (up) HB_TRY(up->wait(g, ctx->stream));
        if (rm) HB_TRY(fft::rowcode_real4096(ctx, d_poly + c0 * M, (size_t)per * trs, rm + c0 * trs * 2049, false, 0, 0, 0, 0));
        else HB_TRY(fft::rowcode_real4096(ctx, d_poly + c0 * M, (size_t)per * trs, c->d_tensor, true, (uint32_t)trs, (uint32_t)K, c->msg_rot, (uint32_t)c0));
        if (up) HB_TRY(up->start(g + 1));                 // (host copy + PCIe of the next group, beside this group's kernel)
    }
    if (rm) {       // columns 0 .. 2047 of every chunk into the main block, column 2048 into the strip
        HB_TRY(launch_transpose_ld(ctx, rm, (size_t)trs * 2049, 2049, (uint32_t)trs, 2048, c->d_tensor, 2048 * rows2, rows2, (uint32_t)K));
        HB_TRY(launch_transpose_ld(ctx, rm + 2048, (size_t)trs * 2049, 2049, (uint32_t)trs, 1, c->d_tensor + (size_t)K * 2048 * rows2, rows2, rows2, (uint32_t)K));
    }
    const char *st_env = getenv("HOBBIT_COMMIT_SKIP_TAIL");
    ctx->enc_skip_tail = !(st_env && st_env[0] == '0'); ctx->enc_tail_skipped = false;
    int r = launch_encode(ctx, c->d_tensor, rows2, c->d_tensor, rows2, trs, hcols, 0, c->msg_rot);
    c->rows_valid = (!r && ctx->enc_tail_skipped) ? std::min<uint32_t>((uint32_t)rows2, ((uint32_t)ctx->code.len + 3) & ~3u) : (uint32_t)rows2;
    ctx->enc_skip_tail = false; ctx->enc_tail_skipped = false;
    if (!r) r = launch_leaf_chain_half(ctx, c->d_tensor, K, (uint32_t)cols, (uint32_t)(trs / 2), c->d_levels, (uint32_t)ctx->code.len, c->msg_rot);
    if (!r) r = launch_merkle_levels(ctx, c->d_levels, M, 1);
    if (r) return r;
    *out = c.release();
    return 0;
}
int hobbit_commit_standard_real(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, int K, int trs, int linear_time, hobbit_commitment **out) {
    return commit_real_impl(ctx, d_poly, N, K, trs, linear_time, out, nullptr);
}
int hobbit_commit_standard_real_host(hobbit_ctx *ctx, const uint64_t *h_poly, uint64_t *d_poly, size_t N, int K, int trs, int linear_time, hobbit_commitment **out) {
    if (!h_poly || !d_poly) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_host: null polynomial");
    HB_TRY(ctx->up_init());
    Uploader up{ctx, reinterpret_cast<const unsigned char *>(h_poly), reinterpret_cast<unsigned char *>(d_poly), 0, 0};
    const int rc = commit_real_impl(ctx, d_poly, N, K, trs, linear_time, out, &up);
    if (rc) hipStreamSynchronize(ctx->up_stream);                 // nothing of the caller's buffer is still being read on an error return
    return rc;
}
// ---- base-field polynomials under RS x RS (include/hobbit_real_rs.h) -----------------------------
// commit_impl(linear_time = 0) for a real polynomial, as a half commitment.  Rows: the real row code straight into the half layout (fft::rowcode_real_half),
// all K chunks in one batch where the full form batches them (row codes up to 2^15 points), chunk by chunk beyond; never rotated.  Columns: the
// rows2-point transform in place over K cols / 2 + K columns, the call tensorcode_chunks makes over K cols.  Leaves: k_leaf_chain_half_rs.
static int commit_real_rs_impl(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, int K, int trs, hobbit_commitment **out, Uploader *up) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    if (!d_poly) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs: null polynomial");
    if ((uintptr_t)d_poly & 15) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs: the polynomial must be 16-byte aligned");
    if (K <= 0 || N % (size_t)K) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs: K must divide N");
    const size_t M = N / K;
    if (trs < 4 || trs % 4 || M % (size_t)trs) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs: trs must be a multiple of 4 dividing N/K");
    if (ilog2_exact(M) < 0) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs: N/K must be a power of two");
    const size_t cols = 2 * M / trs, rows2 = 2 * (size_t)trs;
    const int logc = ilog2_exact(cols), logr = ilog2_exact(rows2);
    if (logr < 0 || logr > 12) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs: the column code needs 2 trs a power of two <= 4096");
    if (logc < 3 || logc > 20) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs: the row code must have 2^3 .. 2^20 points, 8 <= 2 (N/K) / trs <= 2^20");
    if ((size_t)K * trs >> 20 && logc <= 15) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs: more than 2^20 rows in one batch");
    if (half_ncols((uint32_t)cols, (uint32_t)K) >> 31) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs: more than 2^31 stored columns");
    Handle<hobbit_commitment, hobbit_commitment_free> c(new hobbit_commitment());
    c->ctx = ctx; c->N = N; c->M = M; c->K = K; c->trs = trs; c->lin = 0; c->cols = (uint32_t)cols; c->rows2 = (uint32_t)rows2; c->half = true;
    c->rows_valid = (uint32_t)rows2; c->msg_rot = 0;
    const size_t hcols = half_ncols((uint32_t)cols, (uint32_t)K);
    HB_TRY(commit_buffers(ctx, hcols * rows2 * sizeof(F), M, c->d_tensor, c->d_levels));
    const bool big = (size_t)K * trs * cols * sizeof(F) >= ((size_t)64 << 20);
    const int pipe = K % 8 == 0 ? 8 : K % 4 == 0 ? 4 : K % 2 == 0 ? 2 : 1, groups = up && big ? pipe : 1, per = K / groups;
    if (up) { up->groups = groups; up->group_bytes = (size_t)per * M * sizeof(uint64_t); }
    for (int g = 0; g < groups; g++) {
        const size_t c0 = (size_t)g * per;
        if (up) HB_TRY(up->wait(g, ctx->stream));
        if (logc <= 15) HB_TRY(fft::rowcode_real_half(ctx, d_poly + c0 * M, logc, c->d_tensor, (uint32_t)trs, (uint32_t)K, (uint32_t)per, (uint32_t)c0));
        else for (int i = 0; i < per; i++)        // (very long rows: one chunk at a time through the long transform, as tensorcode_chunks does)
            HB_TRY(fft::rowcode_real_half(ctx, d_poly + (c0 + i) * M, logc, c->d_tensor, (uint32_t)trs, (uint32_t)K, 1, (uint32_t)(c0 + i)));
        if (up) HB_TRY(up->start(g + 1));                 // (host copy + PCIe of the next group, beside this group's kernels)
    }
    int r = fft::rows(ctx, c->d_tensor, rows2, (uint32_t)trs, c->d_tensor, rows2, 1, logr, false, 1, (uint32_t)hcols, 0, 0);
    if (!r) r = launch_leaf_chain_half_rs(ctx, c->d_tensor, K, (uint32_t)cols, (uint32_t)(trs / 2), c->d_levels);
    if (!r) r = launch_merkle_levels(ctx, c->d_levels, M, 1);
    if (r) return r;
    *out = c.release();
    return 0;
}
int hobbit_commit_standard_real_rs(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, int K, int trs, hobbit_commitment **out) {
    return commit_real_rs_impl(ctx, d_poly, N, K, trs, out, nullptr);
}
int hobbit_commit_standard_real_rs_host(hobbit_ctx *ctx, const uint64_t *h_poly, uint64_t *d_poly, size_t N, int K, int trs, hobbit_commitment **out) {
    if (!h_poly || !d_poly) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs_host: null polynomial");
    if (out) *out = nullptr;
    if ((uintptr_t)d_poly & 15) return ctx->fail(HOBBIT_EINVAL, "commit_standard_real_rs_host: the device polynomial must be 16-byte aligned");
    HB_TRY(ctx->up_init());
    Uploader up{ctx, reinterpret_cast<const unsigned char *>(h_poly), reinterpret_cast<unsigned char *>(d_poly), 0, 0};
    const int rc = commit_real_rs_impl(ctx, d_poly, N, K, trs, out, &up);
    if (rc) hipStreamSynchronize(ctx->up_stream);                 // nothing of the caller's buffer is still being read on an error return
    return rc;
}
int hobbit_commitment_is_half(const hobbit_commitment *c) { return c && c->half ? 1 : 0; }
int hobbit_widen_real(hobbit_ctx *ctx, const uint64_t *d_reals, hobbit_F *d_out, size_t n) {
    if (n && (!d_reals || !d_out)) return ctx->fail(HOBBIT_EINVAL, "widen_real: null argument");
    return launch_widen_real(ctx, d_reals, mF(d_out), n);
}
int hobbit_aggregate_real(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, const hobbit_F *h_beta, int K, hobbit_F *d_aggr) {
    if (K <= 0 || N % (size_t)K) return ctx->fail(HOBBIT_EINVAL, "aggregate_real: K must divide N");
    if (!d_poly || !h_beta || !d_aggr) return ctx->fail(HOBBIT_EINVAL, "aggregate_real: null argument");
    return launch_aggregate_real(ctx, d_poly, N / K, K, cF(h_beta), mF(d_aggr));
}

void hobbit_commitment_free(hobbit_commitment *c) {
    if (!c) return;
    hobbit_ctx *ctx = c->ctx;
    hipStreamSynchronize(ctx->stream);
    if (c->d_tensor && c->d_levels && !ctx->spare_tensor) {      // park the buffers for the next commit
        ctx->spare_tensor = std::move(c->d_tensor); ctx->spare_levels = std::move(c->d_levels);
    }
    delete c;
}
size_t hobbit_commitment_num_leaves(const hobbit_commitment *c) { return c->M; }
const uint8_t *hobbit_commitment_levels_dev(const hobbit_commitment *c) { return c->d_levels; }
const hobbit_F *hobbit_commitment_tensor_dev(const hobbit_commitment *c) {
    if (c->half) {                                        // the full linear tensor, materialised once into an allocation of the commitment's own
        hobbit_commitment *m = const_cast<hobbit_commitment *>(c);
        if (!m->d_full) {
            const size_t fbytes = (size_t)m->K * m->cols * m->rows2 * sizeof(F);
            if (need_device_bytes(m->ctx, fbytes, "commitment_tensor_dev (half commitment)") != 0) return nullptr;
            if (m->d_full.alloc_bytes(fbytes)) { m->ctx->fail(HOBBIT_ENOMEM, "commitment_tensor_dev: allocation of the full tensor failed"); return nullptr; }
            if (launch_half_expand(m->ctx, m->d_tensor, m->d_full, m->cols, m->K, m->rows2, m->rows_valid, m->msg_rot, m->lin) != 0 || m->ctx->sync() != 0) { m->d_full.reset(); return nullptr; }
        }
        return reinterpret_cast<const hobbit_F *>(m->d_full.get());
    }
    if (c->rows_valid < c->rows2 || c->msg_rot) {         // a raw pointer leaves the library: the implicit zeros become real ones and a rotated
        hobbit_commitment *m = const_cast<hobbit_commitment *>(c);      // message half a linear one, once, in place (one drain for both)
        if (launch_zero_rows(m->ctx, m->d_tensor, (size_t)m->K * m->cols, m->rows2, m->rows_valid) != 0 ||
            launch_unrotate_msg(m->ctx, m->d_tensor, (size_t)m->K * m->cols, m->rows2, m->msg_rot) != 0 || m->ctx->sync() != 0) return nullptr;
        m->rows_valid = m->rows2; m->msg_rot = 0;
    }
    return reinterpret_cast<const hobbit_F *>(c->d_tensor.get());
}
int hobbit_commitment_levels(hobbit_ctx *ctx, const hobbit_commitment *c, uint8_t *h_levels) { return hobbit_memcpy_d2h(ctx, h_levels, c->d_levels, 32 * (2 * c->M - 1)); }
int hobbit_commitment_root(hobbit_ctx *ctx, const hobbit_commitment *c, uint8_t *h_root) { return hobbit_memcpy_d2h(ctx, h_root, c->d_levels + 32 * (2 * c->M - 2), 32); }
int hobbit_commitment_tensor_row(hobbit_ctx *ctx, const hobbit_commitment *c, int chunk, int row, hobbit_F *h_out) {
    if (chunk < 0 || chunk >= c->K || row < 0 || (uint32_t)row >= c->rows2) return ctx->fail(HOBBIT_EINVAL, "tensor_row: index out of range");
    F *tmp; HB_TRY(ctx->workspace((size_t)c->cols * sizeof(F), (void **)&tmp));
    if (c->half) HB_TRY(launch_tensor_row_half(ctx, c->d_tensor, (uint32_t)chunk, c->K, c->rows2, c->cols, (uint32_t)row, tmp, c->rows_valid, c->msg_rot, c->lin));
    else HB_TRY(launch_tensor_row(ctx, c->d_tensor + (size_t)chunk * c->cols * c->rows2, c->rows2, c->cols, (uint32_t)row, tmp, c->rows_valid, c->msg_rot));
    return hobbit_memcpy_d2h(ctx, h_out, tmp, (size_t)c->cols * sizeof(F));
}
int hobbit_commitment_gather(hobbit_ctx *ctx, const hobbit_commitment *c, const uint32_t *h_rows, const uint32_t *h_cols, size_t nq, hobbit_F *h_reply) {
    for (size_t q = 0; q < nq; q++) if (h_rows[q] >= c->rows2 || h_cols[q] >= c->cols) return ctx->fail(HOBBIT_EINVAL, "gather: query out of range");
    if (!nq) return 0;
    StageScope sc(ctx);
    uint8_t *buf; size_t rb = ((nq * c->K * sizeof(F) + 15) / 16) * 16;
    HB_TRY(ctx->workspace(rb + 8 * nq + 64, (void **)&buf));
    F *d_reply = reinterpret_cast<F *>(buf); uint32_t *d_rows = reinterpret_cast<uint32_t *>(buf + rb), *d_cols = d_rows + nq;
    HB_TRY(h2d_staged(ctx, d_rows, h_rows, 4 * nq));
    HB_TRY(h2d_staged(ctx, d_cols, h_cols, 4 * nq));
    if (c->half) HB_TRY(launch_gather_half(ctx, c->d_tensor, c->cols, c->rows2, c->K, d_rows, d_cols, nq, d_reply, c->rows_valid, c->msg_rot, c->lin));
    else HB_TRY(launch_gather(ctx, c->d_tensor, (size_t)c->cols * c->rows2, c->rows2, c->K, d_rows, d_cols, nq, d_reply, c->rows_valid, c->msg_rot));
    HB_TRY(d2h_staged(ctx, h_reply, d_reply, nq * c->K * sizeof(F)));
    return sc.finish();
}
// the multi-GPU open's aggregate exchange: see k_u64_bias_fold
int hobbit_u64_bias_fold(hobbit_ctx *ctx, void *d_words, size_t n_words, uint64_t bias, int fold) {
    if (!d_words && n_words) return ctx->fail(HOBBIT_EINVAL, "u64_bias_fold: null buffer");
    if (!n_words) return 0;
    return launch_u64_bias_fold(ctx, reinterpret_cast<uint64_t *>(d_words), n_words, bias, fold);
}
// the same gather on a raw tensor shard (codeword-major, `nchunks` chunks of 4M F): the multi-GPU open's replies
int hobbit_tensor_gather(hobbit_ctx *ctx, const hobbit_F *d_tensor, size_t M, int nchunks, int trs, const uint32_t *h_rows, const uint32_t *h_cols, size_t nq, hobbit_F *h_reply) {
    if (nchunks <= 0 || trs <= 0 || M % (size_t)trs) return ctx->fail(HOBBIT_EINVAL, "tensor_gather: bad shard shape");
    const size_t cols = 2 * M / (size_t)trs, rows2 = 2 * (size_t)trs;
    for (size_t q = 0; q < nq; q++) if (h_rows[q] >= rows2 || h_cols[q] >= cols) return ctx->fail(HOBBIT_EINVAL, "tensor_gather: query out of range");
    if (!nq) return 0;
    uint8_t *buf; size_t rb = ((nq * nchunks * sizeof(F) + 15) / 16) * 16;
    HB_TRY(ctx->workspace(rb + 8 * nq + 64, (void **)&buf));
    F *d_reply = reinterpret_cast<F *>(buf); uint32_t *d_rows = reinterpret_cast<uint32_t *>(buf + rb), *d_cols = d_rows + nq;
    StageScope sc(ctx);
    HB_TRY(h2d_staged(ctx, d_rows, h_rows, 4 * nq));
    HB_TRY(h2d_staged(ctx, d_cols, h_cols, 4 * nq));
    HB_TRY(launch_gather(ctx, cF(d_tensor), cols * rows2, (uint32_t)rows2, nchunks, d_rows, d_cols, nq, d_reply, (uint32_t)rows2));
    return hobbit_memcpy_d2h(ctx, h_reply, d_reply, nq * nchunks * sizeof(F));
}
int hobbit_commitment_paths(hobbit_ctx *ctx, const hobbit_commitment *c, const uint32_t *h_cols, const uint32_t *h_rows, size_t nq, uint8_t *h_paths) {
    std::vector<uint64_t> pos(nq);
    for (size_t q = 0; q < nq; q++) pos[q] = (uint64_t)(h_rows[q] / 4) * c->cols + h_cols[q];   // src/merkle_tree.cpp:309
    return paths_common(ctx, c->d_levels, c->M, pos.data(), nq, h_paths);
}
int hobbit_commitment_path(hobbit_ctx *ctx, const hobbit_commitment *c, size_t col, size_t row, uint8_t *h_path) {
    uint32_t cc = (uint32_t)col, rr = (uint32_t)row;
    return hobbit_commitment_paths(ctx, c, &cc, &rr, 1, h_path);
}

// ---- Elastic_PC streaming commit (src/Elastic_PC.cpp:174-285) ----------------------------------
struct hobbit_elastic {
    hobbit_ctx *ctx; size_t B; int trs, lin, shift; uint32_t cols, rows2; size_t count;
    mem::Pooled<F> t[4]; mem::Pooled<uint8_t> state;
    bool real = false;              // hobbit_elastic_begin_real: t[] are half chunk tensors (hobbit_half.hpp), the chunks are base-field values
};
int hobbit_elastic_begin(hobbit_ctx *ctx, size_t B, int trs, int linear_time, int gcc_arg_order, hobbit_elastic **out) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    if (trs <= 0 || B % (size_t)trs || ilog2_exact(B) < 0) return ctx->fail(HOBBIT_EINVAL, "elastic_begin: B must be a power of two and trs divide it");
    Handle<hobbit_elastic, hobbit_elastic_free> e(new hobbit_elastic());
    e->ctx = ctx; e->B = B; e->trs = trs; e->lin = linear_time; e->shift = gcc_arg_order ? 1 : 0; e->count = 0;
    e->cols = (uint32_t)(2 * B / trs); e->rows2 = (uint32_t)(2 * trs);
    bool ok = true;
    for (int i = 0; i < 4 && ok; i++) ok = ctx->pool_get(4 * B * sizeof(F), e->t[i]) == 0;
    ok = ok && ctx->pool_get(4 * B * 32, e->state) == 0;
    if (!ok) return ctx->fail(HOBBIT_ENOMEM, "elastic_begin: allocation failed");
    HB_TRY(launch_zero(ctx, e->state, 4 * B * 32));       // buff_hash starts at zero (:186-193)
    *out = e.release();
    return 0;
}
int hobbit_elastic_push(hobbit_ctx *ctx, hobbit_elastic *e, const hobbit_F *d_chunk) {
    if (e->real) return ctx->fail(HOBBIT_ESTATE, "elastic_push: the handle takes base-field chunks (hobbit_elastic_push_real)");
    const int slot = (int)(e->count % 4);
    HB_TRY(tensorcode_chunks(ctx, cF(d_chunk), e->B, 1, e->trs, e->lin, e->t[slot]));   // an all-zero chunk encodes to zeros (:206-226)
    if (slot == 3) HB_TRY(launch_elastic_leaf(ctx, e->t[0], e->t[1], e->t[2], e->t[3], e->rows2, e->cols, e->shift, e->state));
    e->count++;
    return 0;
}
// Multi-GPU form of the push: the 4th chunk of a group writes the group's inner digests (4B x 32 B, the reference's leaf order) to
// d_digests instead of chaining them into the running leaves; the owner of each leaf range chains what it receives (hobbit_chain_digests).
int hobbit_elastic_push_inner(hobbit_ctx *ctx, hobbit_elastic *e, const hobbit_F *d_chunk, uint8_t *d_digests) {
    if (e->real) return ctx->fail(HOBBIT_ESTATE, "elastic_push_inner: the handle takes base-field chunks (hobbit_elastic_push_real)");
    const int slot = (int)(e->count % 4);
    HB_TRY(tensorcode_chunks(ctx, cF(d_chunk), e->B, 1, e->trs, e->lin, e->t[slot]));
    if (slot == 3) {
        if (!d_digests) return ctx->fail(HOBBIT_EINVAL, "elastic_push_inner: the 4th chunk of a group needs a digest buffer");
        HB_TRY(launch_elastic_inner(ctx, e->t[0], e->t[1], e->t[2], e->t[3], e->rows2, e->cols, e->shift, d_digests));
    }
    e->count++;
    return 0;
}
int hobbit_elastic_finish(hobbit_ctx *ctx, hobbit_elastic *e, uint8_t *d_levels) {
    HB_TRY(launch_elastic_finish(ctx, e->state, e->rows2, e->cols, d_levels));
    return launch_merkle_levels(ctx, d_levels, 4 * e->B, 1);                    // :277-283
}
void hobbit_elastic_free(hobbit_elastic *e) { delete e; }

// ---- the streaming commit on base-field chunks (include/hobbit_elastic_real.h) ---------------------------------
// The handle's four tensors are HALF chunk tensors: columns 0 .. cols / 2, codeword-major (hobbit_half.hpp).  The row code writes them
// (fft::real_rows_any), the column code runs over cols / 2 + 1 columns, and k_elastic_leaf_half answers the other columns as conjugates.
// RS x expander: the finalized graphs must have base-field weights, as for hobbit_commit_standard_real.
static int elastic_real_code(hobbit_ctx *ctx, int trs, int lin, const char *who) {
    if (!lin) return 0;
    if (trs > 13 && ctx->code.n != trs) return ctx->fail(HOBBIT_ESTATE, std::string(who) + ": expander graphs for n = trs not finalized");
    if (trs <= 13 && ctx->code.n != trs) { long long l; HB_TRY(hobbit_graph_finalize(ctx, trs, &l)); }
    if (!ctx->code.real_weights)
        return ctx->fail(HOBBIT_EINVAL, std::string(who) + ": a weight of the finalized graphs has img != 0, so column cols - c is not the conjugate of column c");
    return 0;
}
int hobbit_elastic_begin_real(hobbit_ctx *ctx, size_t B, int trs, int linear_time, int gcc_arg_order, hobbit_elastic **out) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    if (trs <= 0 || ilog2_exact((size_t)trs) < 0 || B % (size_t)trs || ilog2_exact(B) < 0) return ctx->fail(HOBBIT_EINVAL, "elastic_begin_real: B and trs must be powers of two, trs dividing B");
    const int logc = ilog2_exact(2 * B / (size_t)trs);
    if (logc < 3 || logc > 16) return ctx->fail(HOBBIT_EINVAL, "elastic_begin_real: the row code 2B/trs must have 2^3 .. 2^16 points");
    if (!linear_time && 2 * trs > 4096) return ctx->fail(HOBBIT_EINVAL, "elastic_begin_real: RSxRS needs 2*trs <= 4096");
    HB_TRY(elastic_real_code(ctx, trs, linear_time, "elastic_begin_real"));
    Handle<hobbit_elastic, hobbit_elastic_free> e(new hobbit_elastic());
    e->ctx = ctx; e->B = B; e->trs = trs; e->lin = linear_time; e->shift = gcc_arg_order ? 1 : 0; e->count = 0; e->real = true;
    e->cols = (uint32_t)(2 * B / trs); e->rows2 = (uint32_t)(2 * trs);
    bool ok = true;
    for (int i = 0; i < 4 && ok; i++) ok = ctx->pool_get((size_t)(e->cols / 2 + 1) * e->rows2 * sizeof(F), e->t[i]) == 0;
    ok = ok && ctx->pool_get(4 * B * 32, e->state) == 0;
    if (!ok) return ctx->fail(HOBBIT_ENOMEM, "elastic_begin_real: allocation failed");
    HB_TRY(launch_zero(ctx, e->state, 4 * B * 32));
    *out = e.release();
    return 0;
}
int hobbit_elastic_push_real(hobbit_ctx *ctx, hobbit_elastic *e, const uint64_t *d_chunk) {
    if (!e->real) return ctx->fail(HOBBIT_ESTATE, "elastic_push_real: the handle takes F chunks (hobbit_elastic_push)");
    if (!d_chunk) return ctx->fail(HOBBIT_EINVAL, "elastic_push_real: null chunk");
    HB_TRY(elastic_real_code(ctx, e->trs, e->lin, "elastic_push_real"));
    const int slot = (int)(e->count % 4);
    const uint32_t hcols = e->cols / 2 + 1;
    F *t = e->t[slot];
    HB_TRY(fft::real_rows_any(ctx, d_chunk, (size_t)e->trs, ilog2_exact(e->cols), t, true, (uint32_t)e->trs));
    if (e->lin) HB_TRY(launch_encode(ctx, t, e->rows2, t, e->rows2, e->trs, hcols, 0));
    else HB_TRY(fft::rows(ctx, t, e->rows2, (uint32_t)e->trs, t, e->rows2, 1, ilog2_exact(e->rows2), false, 1, hcols, 0, 0));
    if (slot == 3) HB_TRY(launch_elastic_leaf_half(ctx, e->t[0], e->t[1], e->t[2], e->t[3], e->rows2, e->cols, e->shift, e->lin, e->state));
    e->count++;
    return 0;
}
size_t hobbit_elastic_device_bytes(const hobbit_elastic *e) {
    size_t b = e->state.bytes();
    for (int i = 0; i < 4; i++) b += e->t[i].bytes();
    return b;
}

// ---- inner PCS commitments of the opening (src/Virgo.cpp:104-178) --------------------------------------
// rows zero-padded to twice their length and transformed: d_enc row i = FFT(row i of d_poly | zeros)
static int rs_rows(hobbit_ctx *ctx, const F *d_poly, size_t w, int k, F *d_enc) {
    const size_t W = 2 * w; const int lg = ilog2_exact(W);
    if (lg < 1) return ctx->fail(HOBBIT_EINVAL, "row length must be a power of two");
    if (lg > 27) return ctx->fail(HOBBIT_EINVAL, "rs_rows: encoded rows of at most 2^27 points");
    return fft::any_rows(ctx, d_poly, w, w, d_enc, lg, false, (size_t)k);
}
int hobbit_shockwave_commit(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, int k, hobbit_F *d_enc, uint8_t *d_levels) {
    if (k < 4 || k > 64 || ilog2_exact((size_t)k) < 0 || N % (size_t)k) return ctx->fail(HOBBIT_EINVAL, "shockwave_commit: k must be a power of two in [4,64] dividing N");
    const size_t w = N / k, W = 2 * w;
    HB_TRY(rs_rows(ctx, cF(d_poly), w, k, mF(d_enc)));          // an all-zero row transforms to zeros: the reference's skip is value-neutral (:133-141)
    HB_TRY(launch_col_digest(ctx, cF(d_enc), W, k, 1, d_levels));
    return launch_merkle_levels(ctx, d_levels, W, 1);
}
int hobbit_change_form(hobbit_ctx *ctx, hobbit_F *d_poly, int logn) {
    if (logn < 1 || logn > 30) return ctx->fail(HOBBIT_EINVAL, "change_form: bad logn");
    const size_t n = (size_t)1 << logn;
    F *tmp; HB_TRY(ctx->workspace2(n * sizeof(F), (void **)&tmp));
    F *cur = mF(d_poly), *nxt = tmp;
    int l = 0;
    for (; l < logn && (n >> l) > 4096; l++) { HB_TRY(launch_change_form_level(ctx, cur, nxt, n, n >> l)); std::swap(cur, nxt); }   // block size > 4096: one pass per level
    if (cur != mF(d_poly)) HB_TRY(launch_copy(ctx, d_poly, cur, n * sizeof(F)));
    if (l < logn) HB_TRY(launch_change_form_tail(ctx, mF(d_poly), n, (uint32_t)(n >> l)));                                           // the rest inside LDS
    return 0;
}
int hobbit_whir_commit(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, hobbit_F *d_com, uint8_t *d_levels) {
    const int logn = ilog2_exact(N);
    if (logn < 4 || logn > 26) return ctx->fail(HOBBIT_EINVAL, "whir_commit: N must be a power of two in [16, 2^26]");
    const size_t L = 2 * N;
    F *pc; HB_TRY(ctx->workspace4(2 * L * sizeof(F), (void **)&pc));      // (the open arena, workspace3, may hold d_poly)
    F *enc = pc + L;
    HB_TRY(launch_copy(ctx, pc, d_poly, N * sizeof(F)));
    HB_TRY(hobbit_change_form(ctx, reinterpret_cast<hobbit_F *>(pc), logn));
    HB_TRY(rs_rows(ctx, pc, N, 1, enc));                                        // resize(2N, 0) + _fft (:165-166)
    // buff[j*16 + kk] = poly_com[j + kk * L/16] (:168-173): a (16 x L/16) -> (L/16 x 16) transpose
    HB_TRY(launch_transpose_ld(ctx, enc, 0, L / 16, 16, (uint32_t)(L / 16), mF(d_com), 0, 16, 1));
    return hobbit_mt_commit_blake(ctx, d_com, L, d_levels);
}

// zero-pad `cur` elements to fsz, change_form, FFT, 16-way regroup, MT_commit_Blake -> root (one FRI layer of _whir_prove,
// src/Virgo.cpp:581-598).  fp: fsz F transient; keep: the regrouped codeword (fsz F) followed by its Merkle levels (fsz/2 hashes),
// which the next query round reads.
static int whir_fri_layer(hobbit_ctx *ctx, const F *d_poly, size_t cur, size_t fsz, F *fp, F *keep, uint8_t *d_root) {
    F *buf = keep; uint8_t *lv = reinterpret_cast<uint8_t *>(buf + fsz);
    HB_TRY(launch_zero(ctx, fp, fsz * sizeof(F)));
    HB_TRY(launch_copy(ctx, fp, d_poly, cur * sizeof(F)));
    HB_TRY(hobbit_change_form(ctx, reinterpret_cast<hobbit_F *>(fp), ilog2_exact(cur)));
    HB_TRY(fft::any_rows(ctx, fp, fsz, fsz, fp, ilog2_exact(fsz), false, 1));         // (2^25, 2^26: the first layer of hobbit_whir_prove_any)
    HB_TRY(launch_transpose_ld(ctx, fp, 0, fsz / 16, 16, (uint32_t)(fsz / 16), buf, 0, 16, 1));
    HB_TRY(hobbit_mt_commit_blake(ctx, reinterpret_cast<hobbit_F *>(buf), fsz, lv));
    HB_TRY(launch_copy(ctx, d_root, lv + 32 * (2 * (fsz / 4) - 2), 32));
    return 0;
}
// compute_zetas (src/Virgo.cpp:220-236), host side, libc draws in the reference's order
static void compute_zetas_host(std::vector<F> &z, std::vector<uint64_t> &ridx, int reps, int v, size_t Nq) {
    z.assign((size_t)reps * v, fmake(0)); ridx.clear();
    z[0] = fmake((uint64_t)random());
    const F omega = root_of_unity(ilog2_exact(Nq));
    for (int i = 1; i < reps; i++) { ridx.push_back((uint64_t)(rand() % (long)Nq)); z[(size_t)i * v] = fpow(omega, (u128)ridx.back()); }
    for (int i = 0; i < reps; i++) for (int j = 1; j < v; j++) z[(size_t)i * v + j] = fmul(z[(size_t)i * v + j - 1], z[(size_t)i * v + j - 1]);
}
// scratch elements hobbit_whir_prove carves from workspace4 AFTER the first 4N (left to a whir_commit of the same polynomial)
static constexpr size_t WHIR_DIN = 2048 + 128 + 64, WHIR_DRES = 1024;       // F elements: z (100 x <= 20) | pows (<= 100) | indices (<= 128 u64)
// The two forms of the proof.  hobbit_whir_prove: N <= 2^24, the out-of-domain step over `repeats` materialised eq tables.
// hobbit_whir_prove_any: N <= 2^26, that step from the two halves of every table (hobbit_whir.hip); its staging slot holds
// z (100 x <= 22) | pows | indices | the low halves of z (100 x WHIR_OOD_VL).  Plan, query answering and replay are shared.
struct WhirCfg {
    int max_log; bool split; const char *range;
    constexpr size_t zcap() const { return split ? 2304 : 2048; }
    constexpr size_t din() const { return zcap() + 128 + 64 + (split ? 128 * WHIR_OOD_VL : 0); }
    size_t ood_elems(size_t N) const { return split ? whir_ood_scratch_elems(std::max(ilog2_exact(N) - 4, 1), 100) : 2 * 100 * (N >> 4); }
};
static constexpr WhirCfg WHIR_TABLES = {24, false, "whir_prove: N must be a power of two in [2^9, 2^24]"},
                         WHIR_ANY = {26, true, "whir_prove_any: N must be a power of two in [2^9, 2^26]"};
static_assert(WHIR_TABLES.din() == WHIR_DIN, "hobbit_whir_prove's staging slot is what open_impl sizes the pinned buffer for");
static size_t whir_scratch_elems(size_t N, const WhirCfg &cfg = WHIR_TABLES) {
    return 2 * N /* poly, beta */ + cfg.ood_elems(N) /* out-of-domain step */ + N /* fp */ + 2 * N + N /* two kept layers */ + 64
           + 3 * 1024 /* partials */ + cfg.din() * 6 /* per-iteration inputs z | pows | query indices */ + WHIR_DRES /* coefficients, roots, y, finals */
           + 256 * 16 /* query replies */ + 8192 /* query paths: < 4096 hashes */ + 64;
}
// Every host-drawn input of one _whir_prove, taken from libc in the reference's order BEFORE anything is queued (none depends on device
// data): a caller can draw the plan of one proof, hand the proof to another thread / context and go on drawing for the next.
struct WhirIterPlan { F a[4]; bool last = false; int repeats = 0; std::vector<F> z, pw; std::vector<uint64_t> ridx; };
struct WhirPlan { std::vector<WhirIterPlan> it; int final_repeats = 0; size_t remaining = 0; bool final_round = false; std::vector<uint64_t> final_ridx; };
static int whir_plan(size_t N, WhirPlan &P, const WhirCfg &cfg = WHIR_TABLES) {
    const int k = 4, logN = ilog2_exact(N);
    if (logN < 9 || logN > cfg.max_log) return HOBBIT_EINVAL;
    int iter = 0, repeats = 100;
    for (;;) {
        if (iter >= 6) return HOBBIT_EINVAL;
        WhirIterPlan ip;
        for (int i = 0; i < k; i++) ip.a[i] = fmake((uint64_t)random());           // a.push_back(random()) (:561)
        iter++;
        const size_t cur = N >> (k * iter), fsz = (2 * N) >> iter;
        const int queries = (int)(100.0 / log2((double)fsz / (double)cur));
        if (logN - iter * k <= k) { ip.last = true; P.it.push_back(std::move(ip)); repeats = queries; P.remaining = (size_t)1 << (logN - iter * k); break; }
        const int v = logN - iter * k;
        compute_zetas_host(ip.z, ip.ridx, repeats, v, (2 * N) >> (iter + k));
        const F sch = fmake((uint64_t)random());
        ip.pw.resize(repeats); { F p = sch; for (int i = 0; i < repeats; i++) { ip.pw[i] = p; p = fmul(p, sch); } }
        ip.repeats = repeats;
        P.it.push_back(std::move(ip));
        repeats = queries;
    }
    P.final_repeats = repeats;
    {   // closing draws (:652-655) and the last query round's indices (:656), leaving the libc stream where the reference leaves it
        const int lr = ilog2_exact(P.remaining);
        F cst = fmake(0); for (int i = 0; i < lr; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); (void)rand(); }
        (void)cst;
        if (repeats > 0 && lr > 0) { std::vector<F> z; compute_zetas_host(z, P.final_ridx, repeats, lr, (2 * N) >> (iter * k)); P.final_round = true; }
    }
    return 0;
}
// _whir_prove (src/Virgo.cpp:519-686).  Nothing the host decides here depends on device data: the fold challenges, the out-of-domain
// points and the query indices are libc draws, and the running evaluation only feeds the reference's exit(-1) checks.  So the whole
// proof is queued without a single synchronisation -- host-drawn inputs go through one pinned staging slot per iteration (one
// async copy each), every result lands in a device result area -- and is read back once at the end, where the checks are replayed.
static int whir_prove_run(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_F *d_com, const uint8_t *d_com_levels, const hobbit_F *h_x, hobbit_whir_out *o,
                         const WhirPlan &plan, const WhirCfg &cfg = WHIR_TABLES) {
    const int k = 4, logN = ilog2_exact(N);
    if (logN < 9 || logN > cfg.max_log || !o) return ctx->fail(HOBBIT_EINVAL, cfg.range);
    const size_t DIN = cfg.din(), ZCAP = cfg.zcap();
    hobbit_F *h_qpoly = o->qpoly, *h_a = o->a, *h_scal = o->scal; uint8_t *h_fri_roots = o->fri_roots; int *h_checks = o->checks;
    StageScope sc(ctx);
    const size_t sz_front = 4 * N, sz_E = cfg.ood_elems(N) / 2;                  // (tables: two buffers of 100 N/16; split: one area, E0 onwards)
    F *base; HB_TRY(ctx->workspace4((sz_front + whir_scratch_elems(N, cfg)) * sizeof(F), (void **)&base));
    F *poly = base + sz_front, *beta = poly + N, *E0 = beta + N, *E1 = E0 + sz_E, *fp = E0 + cfg.ood_elems(N), *keepA = fp + N, *keepB = keepA + 2 * N, *part = keepB + N + 64,
      *din = part + 3 * 1024, *dres = din + DIN * 6, *d_rep = dres + WHIR_DRES;
    uint8_t *d_paths = reinterpret_cast<uint8_t *>(d_rep + 256 * 16);
    // result area: [0] eval0 | per iteration t (stride 128): 12 coefficients, root (2 F), y (100 F) | [900] final sum | [904..) final poly | beta
    auto res_it = [&](int t) { return dres + 8 + (size_t)t * 128; };
    F *res_fin = dres + 900;
    // pinned staging: one slot per iteration, laid out exactly like its device twin (z | pows | indices), then the read-back area
    uint8_t *pinb; HB_TRY(ctx->pinned((DIN * 6 + WHIR_DRES) * sizeof(F), (void **)&pinb));
    F *pin_in = reinterpret_cast<F *>(pinb), *pin_res = pin_in + DIN * 6;
    HB_TRY(launch_copy(ctx, poly, d_poly, N * sizeof(F)));
    HB_TRY(hobbit_eq_table(ctx, h_x, logN, reinterpret_cast<hobbit_F *>(beta)));
    HB_TRY(launch_dot(ctx, beta, poly, N, part, dres));                          // eval = <beta, poly> (:535-538)
    int iter = 0, repeats = 100, nq = 0; size_t remaining = 0;
    const F *prev = cF(d_com); const uint8_t *prev_lv = d_com_levels; size_t prev_sz = 2 * N;   // the layer the next query round reads
    std::vector<uint64_t> ridx;
    std::vector<F> a_all; std::vector<std::vector<F>> pw_all;                    // replayed after the read-back
    size_t q_tot = 0, path_off = 0; int q_round = 0;
    // _verify_iteration's prover part (:245-275): replies (16 regrouped elements per index) and open_tree_blake(tree, {r,0}, 0), into the
    // device reply / path areas; `d_idx`: the indices, already on the device
    auto answer = [&](const uint64_t *d_idx) -> int {
        const size_t n = ridx.size(); const int depth = ilog2_exact(prev_sz / 4);
        if (q_round >= 8 || q_tot + n > 256 || path_off + n * 32 * (size_t)depth > 8192 * sizeof(F)) return ctx->fail(HOBBIT_EINVAL, "whir_prove: query buffers too small");
        if (o->qn) o->qn[q_round] = (int32_t)n;
        q_round++;
        if (n && prev) {
            if (o->qidx) for (size_t i = 0; i < n; i++) o->qidx[q_tot + i] = (int32_t)ridx[i];
            if (o->qreply) HB_TRY(launch_gather_strided(ctx, prev, d_idx, n, 16, 16, 1, d_rep + 16 * q_tot));
            if (o->qpaths) HB_TRY(launch_merkle_paths(ctx, prev_lv, prev_sz / 4, d_idx, n, depth, d_paths + path_off));
        }
        q_tot += n; path_off += n * 32 * (size_t)depth;
        return 0;
    };
    for (;;) {
        if (iter >= 6 || (size_t)iter >= plan.it.size()) return ctx->fail(HOBBIT_EINVAL, "whir_prove: more iterations than the staging area / the plan holds");
        const WhirIterPlan &ip = plan.it[iter];
        for (int i = 0; i < k; i++) {
            const size_t L = N >> (iter * k + i + 1);
            const F a = ip.a[i];
            a_all.push_back(a);
            HB_TRY(launch_whir_round(ctx, poly, beta, L, a, part, res_it(iter) + 3 * i));
        }
        iter++;
        const size_t cur = N >> (k * iter), fsz = (2 * N) >> iter;
        F *keep = (iter & 1) ? keepA : keepB;                                    // layer sizes halve: odd layers need <= 2N, even <= N elements
        HB_TRY(whir_fri_layer(ctx, poly, cur, fsz, fp, keep, reinterpret_cast<uint8_t *>(res_it(iter - 1) + 12)));
        const int queries = (int)(100.0 / log2((double)fsz / (double)cur));
        if (logN - iter * k <= k) {
            if (!ip.last) return ctx->fail(HOBBIT_ESTATE, "whir_prove: plan out of step");
            repeats = queries; remaining = (size_t)1 << (logN - iter * k); break;
        }
        const int v = logN - iter * k;
        if (ip.last || ip.repeats != repeats) return ctx->fail(HOBBIT_ESTATE, "whir_prove: plan out of step");
        const std::vector<F> &z = ip.z; ridx = ip.ridx;
        const std::vector<F> &pw = ip.pw;
        pw_all.push_back(pw);
        // stage z | pows | indices of this iteration and ship them with one asynchronous copy
        F *pslot = pin_in + (size_t)(iter - 1) * DIN, *dslot = din + (size_t)(iter - 1) * DIN;
        if (z.size() > ZCAP || (size_t)repeats > 128 || ridx.size() > 128) return ctx->fail(HOBBIT_EINVAL, "whir_prove: staging slot too small");
        memcpy(pslot, z.data(), z.size() * sizeof(F)); memcpy(pslot + ZCAP, pw.data(), pw.size() * sizeof(F)); memcpy(pslot + ZCAP + 128, ridx.data(), ridx.size() * 8);
        const int vl = v < WHIR_OOD_VL ? v : WHIR_OOD_VL;
        if (cfg.split) for (int i = 0; i < repeats; i++) memcpy(pslot + ZCAP + 192 + (size_t)i * vl, z.data() + (size_t)i * v, (size_t)vl * sizeof(F));
        HB_CHECK(ctx, hipMemcpyAsync(dslot, pslot, DIN * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
        const F *dz = dslot, *dpw = dslot + ZCAP; const uint64_t *d_idx = reinterpret_cast<const uint64_t *>(dslot + ZCAP + 128);
        if (cfg.split) {
            // y = E poly, beta += pows^T E (:613-633) from the halves of the tables: poly and beta cross memory once each
            HB_TRY(launch_whir_ood(ctx, poly, beta, v, dz, dslot + ZCAP + 192, dpw, repeats, E0, res_it(iter - 1) + 16));
        } else {
            // the `repeats` eq tables side by side, then y = E poly, beta += pows^T E (:613-633)
            F *cE = E0, *nE = E1;
            const int hd = v < 11 ? v : 11;                                       // levels 0..hd-1 of every table in one launch
            HB_TRY(launch_eq_head_batched(ctx, cE, cur, dz, v, hd, repeats));
            for (int l = hd; l < v; l++) { HB_TRY(launch_eq_step_batched(ctx, cE, nE, (size_t)1 << l, cur, dz, v, l, repeats)); std::swap(cE, nE); }
            HB_TRY(launch_matvec_rows(ctx, cE, (size_t)repeats, cur, poly, res_it(iter - 1) + 16));
            HB_TRY(launch_vecmat(ctx, cE, (size_t)repeats, cur, dpw, nE));      // nE[0..cur) = sum_i pow_i E[i]   (uses ctx->workspace for partials)
            HB_TRY(launch_axpy(ctx, beta, nE, fmake(1), cur));
        }
        HB_TRY(answer(d_idx));                                                    // _verify_iteration(data, a, r, repeats, iter) (:634)
        prev = keep; prev_lv = reinterpret_cast<const uint8_t *>(keep + fsz); prev_sz = fsz;
        repeats = queries;
    }
    // final verification step (:641-651): sum = <final_poly, final_beta>
    HB_TRY(launch_dot(ctx, beta, poly, remaining, part, res_fin));
    HB_TRY(launch_copy(ctx, res_fin + 4, poly, remaining * sizeof(F)));
    HB_TRY(launch_copy(ctx, res_fin + 4 + remaining, beta, remaining * sizeof(F)));
    {   // the last query round (:656); its indices (and the closing draws in front of them, :652-655) are in the plan
        const int lr = ilog2_exact(remaining);
        if (remaining != plan.remaining || repeats != plan.final_repeats || plan.final_round != (repeats > 0 && lr > 0)) return ctx->fail(HOBBIT_ESTATE, "whir_prove: plan out of step");
        if (plan.final_round) {
            ridx = plan.final_ridx;
            if (ridx.size() > 128) return ctx->fail(HOBBIT_EINVAL, "whir_prove: staging slot too small");
            F *pslot = pin_in + (size_t)5 * DIN, *dslot = din + (size_t)5 * DIN;               // the last slot: only indices
            memcpy(pslot + ZCAP + 128, ridx.data(), ridx.size() * 8);
            HB_CHECK(ctx, hipMemcpyAsync(dslot + ZCAP + 128, pslot + ZCAP + 128, 128 * 8, hipMemcpyHostToDevice, ctx->stream));
            HB_TRY(answer(reinterpret_cast<const uint64_t *>(dslot + ZCAP + 128)));
        }
    }
    // the one read-back
    HB_CHECK(ctx, hipMemcpyAsync(pin_res, dres, WHIR_DRES * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    if (o->qreply && q_tot) HB_TRY(d2h_staged(ctx, o->qreply, d_rep, q_tot * 16 * sizeof(F)));
    if (o->qpaths && path_off) HB_TRY(d2h_staged(ctx, o->qpaths, d_paths, path_off));
    HB_TRY(ctx->sync());
    // replay: round checks ("Error in %d", :562-565), eval updates (:566, :631), final check (:648-651)
    F eval = pin_res[0];
    h_checks[0] = 1;
    for (int t = 0; t < iter; t++) {
        const F *r = pin_res + 8 + (size_t)t * 128;
        for (int i = 0; i < k; i++) {
            const F pa = r[3 * i], pb = r[3 * i + 1], pc = r[3 * i + 2], a = a_all[(size_t)t * k + i];
            if (!feq(fadd(fadd(pa, pb), fadd(pc, pc)), eval)) h_checks[0] = 0;
            eval = fadd(fmul(fadd(fmul(pa, a), pb), a), pc);
            mF(h_qpoly)[3 * nq] = pa; mF(h_qpoly)[3 * nq + 1] = pb; mF(h_qpoly)[3 * nq + 2] = pc; mF(h_a)[nq] = a; nq++;
        }
        memcpy(h_fri_roots + 32 * t, r + 12, 32);
        if (t < (int)pw_all.size()) for (size_t i = 0; i < pw_all[t].size(); i++) eval = fadd(eval, fmul(pw_all[t][i], r[16 + i]));
    }
    const F sum = pin_res[900];
    h_checks[1] = feq(sum, eval);
    mF(h_scal)[0] = eval; mF(h_scal)[1] = sum;
    if (o->final_pb) memcpy(o->final_pb, pin_res + 904, 2 * remaining * sizeof(F));
    if (o->iters) *o->iters = iter;
    return sc.finish();
}
int hobbit_whir_prove(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_F *d_com, const uint8_t *d_com_levels, const hobbit_F *h_x, hobbit_whir_out *o) {
    WhirPlan plan;
    if (whir_plan(N, plan) != 0) return ctx->fail(HOBBIT_EINVAL, "whir_prove: N must be a power of two in [2^9, 2^24]");
    return whir_prove_run(ctx, d_poly, N, d_com, d_com_levels, h_x, o, plan);
}
int hobbit_whir_prove_any(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_F *d_com, const uint8_t *d_com_levels, const hobbit_F *h_x, hobbit_whir_out *o) {
    WhirPlan plan;
    if (!o) return ctx->fail(HOBBIT_EINVAL, "whir_prove_any: NULL out");                                 // (before the plan: nothing is drawn)
    if (whir_plan(N, plan, WHIR_ANY) != 0) return ctx->fail(HOBBIT_EINVAL, WHIR_ANY.range);
    return whir_prove_run(ctx, d_poly, N, d_com, d_com_levels, h_x, o, plan, WHIR_ANY);
}
// shockwave_prove (src/Virgo.cpp:435-517), prover side
// workspace4 elements of one shockwave_prove: [0, nested) belongs to the nested whir_commit / whir_prove calls, its own vectors follow
// The nested proof's form by the aggregate's width: up to 2^24 the materialised out-of-domain tables (today's plan, scratch and code path,
// bit for bit), in (2^24, 2^26] the table-free step of hobbit_whir_prove_any (the parity opening of a code of 2^21: w = 2^25)
static const WhirCfg &shockwave_whir_cfg(size_t w) { return w > ((size_t)1 << WHIR_TABLES.max_log) ? WHIR_ANY : WHIR_TABLES; }
static size_t shockwave_nested_elems(size_t w) { return 4 * w + whir_scratch_elems(w, shockwave_whir_cfg(w)) + 64; }
static size_t shockwave_own_elems(size_t w, int k) {
    return w + 2 * w + 2 * w + 64 + 256 + 256 /* idx */ + 2 * w + 2 * w /* whir_commit outputs: com, levels */ + 240 * (size_t)k /* replies */ + 240 * 64 /* paths */ + 64;
}
// the libc draws of one shockwave_prove, in the reference's order: the 240 query columns (:463-467), then _whir_prove's (whir_plan)
struct ShockPlan { std::vector<uint64_t> I; bool committed = false; WhirPlan whir; };
static int shockwave_plan(size_t N, int k, ShockPlan &P) {
    if (k <= 0 || N % (size_t)k) return HOBBIT_EINVAL;
    const size_t w = N / k, W = 2 * w;
    P.I.resize(240);
    for (int i = 0; i < 240; i++) P.I[i] = (uint64_t)(rand() % (long)W);
    P.committed = w > 256;
    return P.committed ? whir_plan(w, P.whir, shockwave_whir_cfg(w)) : 0;
}
struct OpenTrace {
    // HOBBIT_TRACE=1: stage times with the stream drained at every mark (everything on one thread and stream); HOBBIT_TRACE=host: the host
    // thread's own time between marks, nothing drained, the production threads and streams
    bool on, drain; hobbit_ctx *ctx; std::chrono::steady_clock::time_point t0; const char *last; uint64_t w0;
    OpenTrace(hobbit_ctx *c) : on(getenv("HOBBIT_TRACE") != nullptr), drain(on && strcmp(getenv("HOBBIT_TRACE"), "host") != 0), ctx(c),
                               t0(std::chrono::steady_clock::now()), last("start"), w0(c->wait_ns) {}
    void mark(const char *name) {
        if (!on) return;
        if (drain) hipStreamSynchronize(ctx->stream);
        auto t1 = std::chrono::steady_clock::now();
        const double ms = std::chrono::duration<double, std::milli>(t1 - t0).count(), waited = 1e-6 * (double)(ctx->wait_ns - w0);
        if (drain) fprintf(stderr, "[hobbit open] %-28s %8.3f ms\n", name, ms);
        else fprintf(stderr, "[hobbit open] %-28s %8.3f ms  (waiting for the device %.3f, host work %.3f)\n", name, ms, waited, ms - waited);
        t0 = t1; w0 = ctx->wait_ns;
    }
};
static int shockwave_prove_run(hobbit_ctx *ctx, const hobbit_F *d_matrix, const hobbit_F *d_enc, const uint8_t *d_levels, size_t N, int k, const hobbit_F *h_x, int xlen,
                               hobbit_shockwave_out *o, const ShockPlan &plan) {
    const int lk = ilog2_exact((size_t)k);
    if (lk < 0 || k > 64 || N % (size_t)k || xlen < lk || !o) return ctx->fail(HOBBIT_EINVAL, "shockwave_prove: bad k / N / x");
    const size_t w = N / k, W = 2 * w;
    StageScope sc(ctx);
    OpenTrace tr(ctx); const bool helper_ctx = ctx->helper == nullptr && ctx->helper2 == nullptr; if (helper_ctx && !tr.drain) tr.on = false;   // (host mode: the main context's call only)
    std::vector<F> beta1((size_t)k); beta1[0] = fmake(1);
    for (int i = 0; i < lk; i++) for (size_t j = ((size_t)1 << i); j-- > 0;) { F t = fmul(cF(h_x)[xlen - lk + (lk - 1 - i)], beta1[j]); beta1[2 * j + 1] = t; beta1[2 * j] = fsub(beta1[j], t); }
    // workspace4 layout: [0, nested) belongs to the nested whir_commit / whir_prove calls (they carve from the start and never ask
    // for more than `nested`, so the buffer is not reallocated under us); our own vectors follow.
    const size_t nested = shockwave_nested_elems(w), own = shockwave_own_elems(w, k);
    F *base; HB_TRY(ctx->workspace4((nested + own) * sizeof(F), (void **)&base));
    F *mine = base + nested; F *aggr = mine, *at = aggr + w, *b1v = at + W, *dbeta = b1v + W, *ones = dbeta + 64; uint64_t *didx = reinterpret_cast<uint64_t *>(ones + 256);
    F *wcom = ones + 256 + 256; uint8_t *wlv = reinterpret_cast<uint8_t *>(wcom + 2 * w); F *d_rep = wcom + 4 * w;
    uint8_t *d_pth = reinterpret_cast<uint8_t *>(d_rep + 240 * (size_t)k);
    // (host vectors handed to asynchronous copies live to the end of this function, which ends synchronised)
    HB_TRY(h2d_staged(ctx, dbeta, beta1.data(), (size_t)k * sizeof(F)));
    HB_TRY(launch_vecmat(ctx, cF(d_matrix), (size_t)k, w, dbeta, aggr));        // aggr = beta1^T matrix (:444-456)
    HB_TRY(launch_vecmat(ctx, cF(d_enc), (size_t)k, W, dbeta, at));
    const bool committed = w > 256;
    if (committed) {                                                         // whir_commit(aggr, C) (:458-461)
        HB_TRY(hobbit_whir_commit(ctx, reinterpret_cast<hobbit_F *>(aggr), w, reinterpret_cast<hobbit_F *>(wcom), wlv));
        if (o->whir_root) HB_TRY(d2h_staged(ctx, o->whir_root, wlv + 32 * (w - 2), 32));
    }
    if (plan.I.size() != 240 || plan.committed != committed) return ctx->fail(HOBBIT_ESTATE, "shockwave_prove: plan out of step");
    const std::vector<uint64_t> &I = plan.I; std::vector<F> one(240, fmake(1));
    if (o->I) for (int i = 0; i < 240; i++) o->I[i] = (uint32_t)I[i];                                                // (:463-467)
    HB_TRY(launch_zero(ctx, b1v, W * sizeof(F)));
    HB_TRY(h2d_staged(ctx, ones, one.data(), 240 * sizeof(F)));
    HB_TRY(h2d_staged(ctx, didx, I.data(), 240 * 8));
    HB_TRY(launch_scatter(ctx, didx, ones, 240, b1v));
    if (o->reply) {                                                          // reply[i][j] = encoded_matrix[j][I[i]] (:468-472)
        HB_TRY(launch_gather_strided(ctx, cF(d_enc), didx, 240, (uint32_t)k, 1, W, d_rep));
        HB_TRY(d2h_staged(ctx, o->reply, d_rep, 240 * (size_t)k * sizeof(F)));
    }
    if (o->paths && d_levels) {                                              // open_tree_blake(data->MT, {I[i],0}, 0) (:503)
        const int depth = ilog2_exact(W);
        if (depth > 32) return ctx->fail(HOBBIT_EINVAL, "shockwave_prove: tree too deep for the path buffer");
        HB_TRY(launch_merkle_paths(ctx, d_levels, W, didx, 240, depth, d_pth));
        HB_TRY(d2h_staged(ctx, o->paths, d_pth, 240 * (size_t)depth * 32));
    }
    tr.mark("  sp: aggregate, whir_commit, queries");
    hobbit_F p33 = {33, 0};
    HB_TRY(hobbit_sumcheck2(ctx, reinterpret_cast<hobbit_F *>(at), reinterpret_cast<hobbit_F *>(b1v), W, &p33, o->q1, o->r1, o->vr1, o->fin1));         // (:477)
    tr.mark("  sp: sumcheck");
    HB_TRY(hobbit_prove_fft(ctx, reinterpret_cast<hobbit_F *>(aggr), w, o->r1, o->q2, o->r2, o->vr2, o->fin2));                                            // (:478)
    tr.mark("  sp: prove_fft");
    int iters = 0;
    // (:479) aggr.size()/2 > 256 is evaluated after prove_fft doubled aggr in place (src/sumcheck.cpp:2984-2985): the original width w
    if (committed) {
        // _whir_prove works on a copy of aggr inside its own scratch (from the start of workspace4): aggr and the commitment live beyond it
        hobbit_whir_out wo = {o->wq, o->wa, o->wroots, o->wscal, o->wchecks, &iters, o->wqidx, o->wqreply, o->wqpaths, o->wfinal, o->wqn};
        HB_TRY(whir_prove_run(ctx, reinterpret_cast<hobbit_F *>(aggr), w, reinterpret_cast<hobbit_F *>(wcom), wlv, o->r2, &wo, plan.whir, shockwave_whir_cfg(w)));   // (:480-481)
    }
    if (o->iters) *o->iters = iters;
    tr.mark("  sp: whir_prove");
    HB_TRY(ctx->sync());
    tr.mark("  sp: closing drain");
    return sc.finish();
}
int hobbit_shockwave_prove(hobbit_ctx *ctx, const hobbit_F *d_matrix, const hobbit_F *d_enc, const uint8_t *d_levels, size_t N, int k, const hobbit_F *h_x, int xlen,
                           hobbit_shockwave_out *o) {
    const int lk = ilog2_exact((size_t)k);
    if (lk < 0 || k > 64 || N % (size_t)k || xlen < lk || !o) return ctx->fail(HOBBIT_EINVAL, "shockwave_prove: bad k / N / x");
    ShockPlan plan;
    if (shockwave_plan(N, k, plan) != 0) return ctx->fail(HOBBIT_EINVAL, "shockwave_prove: bad k / N, or a width outside _whir_prove's range");
    return shockwave_prove_run(ctx, d_matrix, d_enc, d_levels, N, k, h_x, xlen, o, plan);
}

// ---- multi-GPU commit building blocks -------------------------------------------
int hobbit_tensorcode_chunks(hobbit_ctx *ctx, const hobbit_F *d_msg, size_t M, int nchunks, int trs, int linear_time, hobbit_F *d_out) {
    if (nchunks <= 0) return ctx->fail(HOBBIT_EINVAL, "tensorcode_chunks: nchunks must be positive");
    return tensorcode_chunks(ctx, cF(d_msg), M, nchunks, trs, linear_time, mF(d_out));
}
int hobbit_inner_digests(hobbit_ctx *ctx, const hobbit_F *d_tensor, size_t M, int nchunks, int trs, uint8_t *d_out) {
    if (trs < 4 || trs % 4 || M % (size_t)trs) return ctx->fail(HOBBIT_EINVAL, "inner_digests: trs must be a multiple of 4 dividing M");
    size_t cols = 2 * M / trs;
    return launch_inner_digests(ctx, cF(d_tensor), cols * 2 * (size_t)trs, nchunks, (uint32_t)cols, (uint32_t)(trs / 2), d_out);
}
int hobbit_chain_digests(hobbit_ctx *ctx, const uint8_t *d_digests, size_t stride_bytes, int K, size_t m, uint8_t *d_leaves) {
    if (K < 0 || stride_bytes % 16) return ctx->fail(HOBBIT_EINVAL, "chain_digests: bad K / stride");
    return launch_chain_digests(ctx, d_digests, stride_bytes, K, m, d_leaves);
}
int hobbit_leaf_chain_relay(hobbit_ctx *ctx, const hobbit_F *d_tensor, size_t M, int nchunks, int trs, int linear_time, size_t slot_begin, size_t slot_count,
                            const uint8_t *d_state_in, uint8_t *d_state_out, uint8_t *d_leaves) {
    if (trs < 4 || trs % 4 || M % (size_t)trs || nchunks <= 0) return ctx->fail(HOBBIT_EINVAL, "leaf_chain_relay: trs must be a multiple of 4 dividing M, nchunks positive");
    if (slot_begin + slot_count > M || (!d_state_out && !d_leaves)) return ctx->fail(HOBBIT_EINVAL, "leaf_chain_relay: slot range beyond the M leaves, or nowhere to write");
    const size_t cols = 2 * M / trs, rows2 = 2 * (size_t)trs;
    if (linear_time && ctx->code.n != trs) return ctx->fail(HOBBIT_ESTATE, "leaf_chain_relay: expander graphs for n = trs not finalized");
    return launch_leaf_chain_relay(ctx, cF(d_tensor), cols * rows2, nchunks, (uint32_t)cols, (uint32_t)(trs / 2), slot_begin, slot_count, d_state_in, d_state_out, d_leaves,
                                   linear_time ? (uint32_t)ctx->code.len : (uint32_t)rows2);
}
// A real check of an open_tree_blake path (the reference's verify_claim_opt_blake only does proof-size bookkeeping, in SHA3): walk the
// `depth` siblings from the leaf at `pos` to the root with create_tree_blake's parent rule (src/merkle_tree.cpp:275-280).  With the
// reference's left|left quirk a parent is H(L | L), L the even node of the pair: the running node at an even position, the sibling the
// path carries at an odd one -- so in the reference's tree only the path's even-side nodes are bound to the root; quirk == 0 checks an
// ordinary H(L | R) tree.  Returns 1 if the walk ends in `root`, 0 if not.  Host only.
int hobbit_verify_path_host(const uint8_t *leaf, uint64_t pos, const uint8_t *path, int depth, const uint8_t *root, int quirk_left_left) {
    if (!leaf || !root || depth < 0 || (depth && !path)) return 0;
    uint8_t node[32]; memcpy(node, leaf, 32);
    for (int l = 0; l < depth; l++, pos >>= 1) {
        const uint8_t *sib = path + 32 * (size_t)l;
        uint32_t m[16], h[8];
        const uint8_t *Lh = (pos & 1) ? sib : node, *Rh = quirk_left_left ? Lh : ((pos & 1) ? node : sib);
        memcpy(m, Lh, 32); memcpy(m + 8, Rh, 32);
        blake3_compress64(m, h);
        memcpy(node, h, 32);
    }
    return memcmp(node, root, 32) == 0;
}
int hobbit_fingerprint_map(hobbit_ctx *ctx, const hobbit_F *d_addr, const hobbit_F *d_value, const hobbit_F *d_freq, const hobbit_F *h_a, const hobbit_F *h_b, hobbit_F *d_out, size_t n) {
    if (!d_addr || !d_value || !h_a || !d_out || (d_freq && !h_b)) return ctx->fail(HOBBIT_EINVAL, "fingerprint_map: null argument");
    return launch_fingerprint(ctx, cF(d_addr), cF(d_value), d_freq ? cF(d_freq) : nullptr, *cF(h_a), d_freq ? *cF(h_b) : fmake(0), mF(d_out), n);
}
// SURVEY.md 8(b)'s export list by its own names: thin forms of what the library already has
int hobbit_leaf_chain(hobbit_ctx *ctx, const hobbit_F *d_tensor, size_t M, int nchunks, int trs, int linear_time, uint8_t *d_leaves) {
    if (trs < 4 || trs % 4 || M % (size_t)trs || nchunks <= 0 || !d_leaves) return ctx->fail(HOBBIT_EINVAL, "leaf_chain: trs must be a multiple of 4 dividing M, nchunks positive");
    const size_t cols = 2 * M / trs, rows2 = 2 * (size_t)trs;
    if (linear_time && ctx->code.n != trs) return ctx->fail(HOBBIT_ESTATE, "leaf_chain: expander graphs for n = trs not finalized");
    return launch_leaf_chain_relay(ctx, cF(d_tensor), cols * rows2, nchunks, (uint32_t)cols, (uint32_t)(trs / 2), 0, M, nullptr, nullptr, d_leaves,
                                   linear_time ? (uint32_t)ctx->code.len : (uint32_t)rows2, 1);
}
int hobbit_axpy_aggregate(hobbit_ctx *ctx, const hobbit_F *d_chunk, const hobbit_F *h_coeff, hobbit_F *d_acc, size_t n) {
    return hobbit_fold_axpy(ctx, d_acc, d_chunk, h_coeff, n);
}
int hobbit_stream_fold(hobbit_ctx *ctx, int kind, const hobbit_F *const *d_tables, const int32_t *d_gate, size_t n, hobbit_F *h_K) {
    if (!d_tables || !h_K) return ctx->fail(HOBBIT_EINVAL, "stream_fold: null argument");
    const int nt = kind == 2 ? 4 : kind == 3 ? 5 : kind == 4 ? 7 : kind == 13 ? 6 : 0, nc = kind == 2 ? 2 : kind == 4 ? 4 : 3;
    if (!nt) return ctx->fail(HOBBIT_EINVAL, "stream_fold: kind must be 2, 3, 4 (compute{2,3,4}p_error_terms) or 13 (one batch of batch_prod)");
    const F *t[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < nt; i++) t[i] = cF(d_tables[i]);
    F k[4];
    HB_TRY(launch_err_terms(ctx, kind, t, d_gate, n, k));
    for (int q = 0; q < nc; q++) mF(h_K)[q] = fadd(cF(h_K)[q], k[q]);
    return 0;
}
void hobbit_blake3_64_host(const uint8_t *in, uint8_t *out, size_t n) {
    for (size_t i = 0; i < n; i++) { uint32_t m[16], h[8]; memcpy(m, in + 64 * i, 64); blake3_compress64(m, h); memcpy(out + 32 * i, h, 32); }
}

// ---- code-membership / FFT-as-sumcheck (src/sumcheck.cpp:2888-2929, 2975-3027, 3223-3235) ---------
// host recursion of evaluate_parity_matrix, emitting (A index, beta index, weight) triples
static long long parity_triples(hobbit_ctx *ctx, std::vector<std::vector<std::pair<uint32_t, F>>> &rows, long long Offset, long long n, int dep, long long *lvl) {
    const long long thr = 13;
    if (n <= thr) return n;
    const HostGraph &C = ctx->graphs[{dep, 0}], &D = ctx->graphs[{dep, 1}];
    long long R = C.R;
    const F minus1 = fmake(P61 - 1);
    for (long long i = 0; i < n; i++)
        for (int d = 0; d < C.degree; d++) rows[i + Offset].push_back({(uint32_t)(C.nbr[i * C.degree + d] + *lvl), C.w[i * C.degree + d]});
    for (long long i = 0; i < R; i++) rows[i + Offset + n].push_back({(uint32_t)(*lvl + i), minus1});
    long long l = *lvl + R;
    long long L = parity_triples(ctx, rows, Offset + n, R, dep + 1, &l);
    R = D.R;
    for (long long i = 0; i < L; i++)
        for (int d = 0; d < D.degree; d++) rows[i + Offset + n].push_back({(uint32_t)(D.nbr[i * D.degree + d] + *lvl), D.w[i * D.degree + d]});
    for (long long i = 0; i < R; i++) rows[i + Offset + n + L].push_back({(uint32_t)(i + *lvl), minus1});
    *lvl += R;
    return n + L + R;
}
int hobbit_parity_matrix(hobbit_ctx *ctx, const hobbit_F *d_beta, size_t size_a, long long n, hobbit_F *d_A) {
    DeviceCode &c = ctx->code;
    if (c.n != n) return ctx->fail(HOBBIT_ESTATE, "parity_matrix: graphs for this n are not finalized");
    if (size_a < (size_t)c.len) return ctx->fail(HOBBIT_EINVAL, "parity_matrix: A must hold at least the codeword length");
    if (!c.d_pm_rowptr || c.pm_rows != size_a) {
        HB_TRY(ctx->sync());
        c.d_pm_rowptr.reset(); c.d_pm_idx.reset(); c.d_pm_w.reset();
        std::vector<std::vector<std::pair<uint32_t, F>>> rows(size_a);
        long long lvl = 0;
        parity_triples(ctx, rows, 0, n, 0, &lvl);
        std::vector<uint32_t> rp(size_a + 1, 0), idx; std::vector<F> w;
        for (size_t a = 0; a < size_a; a++) {
            rp[a + 1] = rp[a] + (uint32_t)rows[a].size();
            for (auto &e : rows[a]) { if (e.first >= size_a) return ctx->fail(HOBBIT_EINVAL, "parity_matrix: beta index out of range"); idx.push_back(e.first); w.push_back(e.second); }
        }
        if (c.d_pm_rowptr.alloc_bytes(rp.size() * 4) || c.d_pm_idx.alloc_bytes(idx.size() * 4 + 16) || c.d_pm_w.alloc_bytes(w.size() * sizeof(F) + 16))
            return ctx->fail(HOBBIT_ENOMEM, "parity_matrix: alloc failed");
        HB_CHECK(ctx, hipMemcpy(c.d_pm_rowptr, rp.data(), rp.size() * 4, hipMemcpyHostToDevice));
        if (!idx.empty()) { HB_CHECK(ctx, hipMemcpy(c.d_pm_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice)); HB_CHECK(ctx, hipMemcpy(c.d_pm_w, w.data(), w.size() * sizeof(F), hipMemcpyHostToDevice)); }
        c.pm_rows = size_a;
    }
    return launch_csr_gather(ctx, c.d_pm_rowptr, c.d_pm_idx, c.d_pm_w, cF(d_beta), mF(d_A), size_a);
}
int hobbit_phi_g(hobbit_ctx *ctx, const hobbit_F *h_rx, int n, const hobbit_F *h_scale, int is_ifft, hobbit_F *d_out) {
    if (n < 1 || n > 30) return ctx->fail(HOBBIT_EINVAL, "phi_g: n must be in [1,30]");
    const size_t N = (size_t)1 << n;
    const F *pm; HB_TRY(fft::roots(ctx, n, is_ifft != 0, &pm));      // phi_mul[k] = rou^k, k < N/2 (all that is indexed)
    F *g = mF(d_out);
    HB_TRY(launch_zero(ctx, g, N * sizeof(F)));
    const int last = is_ifft ? n : n - 1;
    int first = 1;
    if (!is_ifft && last >= 2) {                                       // the first levels in one workgroup: a level per launch is latency only up there
        const int hd = last < 11 ? last : 11;
        HB_TRY(launch_phi_head(ctx, g, n, hd, cF(h_rx), *cF(h_scale), pm));
        first = hd + 1;
    } else HB_TRY(launch_fill_F(ctx, g, 1, is_ifft && N > 1 ? 2 : 1, *cF(h_scale)));      // (a kernel argument: no upload to wait for)
    for (int i = first; i <= last; i++) HB_TRY(launch_phi_step(ctx, g, (size_t)1 << (i - 1), n - i, cF(h_rx)[n - i], pm, 0));
    if (!is_ifft) HB_TRY(launch_phi_step(ctx, g, (size_t)1 << (n - 1), 0, cF(h_rx)[0], pm, 1));
    return 0;
}
// arr[c] = multilinear evaluation over the ROW index of column c at r (prepare_matrix(transpose(M), r))
int hobbit_prepare_matrix_cols(hobbit_ctx *ctx, const hobbit_F *d_M, size_t rows, size_t cols, const hobbit_F *h_r, int k, hobbit_F *d_out) {
    if (ilog2_exact(rows) < 0 || k > ilog2_exact(rows)) return ctx->fail(HOBBIT_EINVAL, "prepare_matrix_cols: rows must be a power of two, k <= log2 rows");
    if (k == 0) { HB_TRY(launch_copy(ctx, d_out, d_M, cols * sizeof(F))); return 0; }
    F *ws; HB_TRY(ctx->workspace2((rows / 2 + rows / 4 + 1) * cols * sizeof(F), (void **)&ws));
    F *a = ws, *b = ws + (rows / 2) * cols;
    const F *src = cF(d_M); F *dst = a; size_t r = rows;
    for (int t = 0; t < k; t++) {
        F *o = (t == k - 1 && (r / 2) == 1) ? static_cast<F *>(mF(d_out)) : dst;
        HB_TRY(launch_fold_rows(ctx, src, o, r / 2, cols, cF(h_r)[t]));
        src = o; dst = dst == a ? b : a; r /= 2;
    }
    if (src != cF(d_out)) HB_TRY(launch_copy(ctx, d_out, src, cols * sizeof(F)));   // row 0 (src/utils.cpp:771-773)
    return 0;
}
int hobbit_prove_linear_code(hobbit_ctx *ctx, const hobbit_F *d_codeword, size_t size, long long n, const hobbit_F *h_r1, hobbit_F *h_qpoly,
                             hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_final) {
    int k = ilog2_exact(size);
    if (k < 1) return ctx->fail(HOBBIT_EINVAL, "prove_linear_code: size must be a power of two");
    F *tmp; HB_TRY(ctx->workspace2(2 * size * sizeof(F), (void **)&tmp));
    F *beta = tmp, *A = tmp + size;
    HB_TRY(hobbit_eq_table(ctx, h_r1, k, (hobbit_F *)beta));
    HB_TRY(hobbit_parity_matrix(ctx, (const hobbit_F *)beta, size, n, (hobbit_F *)A));
    return hobbit_sumcheck2(ctx, (const hobbit_F *)A, d_codeword, size, h_r1 + (k - 1), h_qpoly, h_r, h_vr, h_final);
}
int hobbit_prove_fft(hobbit_ctx *ctx, const hobbit_F *d_m, size_t s, const hobbit_F *h_r, hobbit_F *h_qpoly, hobbit_F *h_rr, hobbit_F *h_vr,
                     hobbit_F *h_final) {
    const size_t S = 2 * s; int k = ilog2_exact(S);
    if (k < 1) return ctx->fail(HOBBIT_EINVAL, "prove_fft: size must be a power of two");
    F *tmp; HB_TRY(ctx->workspace2(2 * S * sizeof(F), (void **)&tmp));
    F *mm = tmp, *FG = tmp + S;
    HB_TRY(launch_zero(ctx, mm + s, s * sizeof(F)));                       // m.resize(2*m.size(), 0)
    HB_TRY(launch_copy(ctx, mm, d_m, s * sizeof(F)));
    hobbit_F one = {1, 0};
    HB_TRY(hobbit_phi_g(ctx, h_r, k, &one, 0, (hobbit_F *)FG));
    return hobbit_sumcheck2(ctx, (const hobbit_F *)FG, (const hobbit_F *)mm, S, h_r + (k - 1), h_qpoly, h_rr, h_vr, h_final);
}
// h_prev: the transcript seed r[r.size()-1] (src/sumcheck.cpp:3012); recursive_prover_Spielman_stream hands prove_fft_matrix an r that is one
// entry longer than the k2 + k1 variables it uses (src/PC_utils.cpp:255-266), so the seed is not always h_r[k1 + k2 - 1]
static int prove_fft_matrix_seeded(hobbit_ctx *ctx, const hobbit_F *d_M, size_t rows, size_t cols, const hobbit_F *h_r, const hobbit_F *h_prev, hobbit_F *h_qpoly,
                                   hobbit_F *h_rr, hobbit_F *h_vr, hobbit_F *h_final);
int hobbit_prove_fft_matrix(hobbit_ctx *ctx, const hobbit_F *d_M, size_t rows, size_t cols, const hobbit_F *h_r, hobbit_F *h_qpoly, hobbit_F *h_rr,
                            hobbit_F *h_vr, hobbit_F *h_final) {
    const int k2 = ilog2_exact(2 * cols), k1 = ilog2_exact(rows);
    if (k2 < 1 || k1 < 0) return ctx->fail(HOBBIT_EINVAL, "prove_fft_matrix: rows and cols must be powers of two");
    return prove_fft_matrix_seeded(ctx, d_M, rows, cols, h_r, h_r + (k1 + k2 - 1), h_qpoly, h_rr, h_vr, h_final);
}
static int prove_fft_matrix_seeded(hobbit_ctx *ctx, const hobbit_F *d_M, size_t rows, size_t cols, const hobbit_F *h_r, const hobbit_F *h_prev, hobbit_F *h_qpoly,
                                   hobbit_F *h_rr, hobbit_F *h_vr, hobbit_F *h_final) {
    const size_t C2 = 2 * cols; int k2 = ilog2_exact(C2), k1 = ilog2_exact(rows);
    if (k2 < 1 || k1 < 0) return ctx->fail(HOBBIT_EINVAL, "prove_fft_matrix: rows and cols must be powers of two");
    // arr = prepare_matrix(transpose(M padded), r1): column evaluations, upper half zero; Fg1 = phiG(r2)
    F *tmp; HB_TRY(ctx->workspace(2 * C2 * sizeof(F), (void **)&tmp));
    F *arr = tmp, *Fg = tmp + C2;
    HB_TRY(launch_zero(ctx, arr + cols, cols * sizeof(F)));
    HB_TRY(hobbit_prepare_matrix_cols(ctx, d_M, rows, cols, h_r + k2, k1, (hobbit_F *)arr));
    hobbit_F one = {1, 0};
    HB_TRY(hobbit_phi_g(ctx, h_r, k2, &one, 0, (hobbit_F *)Fg));
    // sumcheck2 uses ctx->workspace itself: move the two tables to workspace2 first
    F *t2; HB_TRY(ctx->workspace2(2 * C2 * sizeof(F), (void **)&t2));
    HB_TRY(launch_copy(ctx, t2, tmp, 2 * C2 * sizeof(F)));
    return hobbit_sumcheck2(ctx, (const hobbit_F *)(t2 + C2), (const hobbit_F *)t2, C2, h_prev, h_qpoly, h_rr, h_vr, h_final);
}

// ---- open building blocks ---------------------------------------------------------------------
int hobbit_aggregate(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_F *h_beta, int K, hobbit_F *d_aggr) {
    if (K <= 0 || N % (size_t)K) return ctx->fail(HOBBIT_EINVAL, "aggregate: K must divide N");
    return launch_aggregate(ctx, cF(d_poly), N / K, K, cF(h_beta), mF(d_aggr));
}

// ---- streaming-sumcheck error terms and folds (src/sumcheck.cpp:374-432, 862-869, 1093-1136) ------
static inline void acc_K(hobbit_F *io, const F *k, int nc) { for (int q = 0; q < nc; q++) mF(io)[q] = fadd(cF(io)[q], k[q]); }
int hobbit_compute2p_error_terms(hobbit_ctx *ctx, const hobbit_F *d_b1, const hobbit_F *d_b2, const hobbit_F *d_f1, const hobbit_F *d_f2, size_t n, hobbit_F *h_K) {
    const F *t[8] = {cF(d_b1), cF(d_b2), cF(d_f1), cF(d_f2), nullptr, nullptr, nullptr, nullptr}; F k[4];
    HB_TRY(launch_err_terms(ctx, 2, t, nullptr, n, k)); acc_K(h_K, k, 2); return 0;
}
int hobbit_compute3p_error_terms(hobbit_ctx *ctx, const hobbit_F *d_b1, const int32_t *d_gate, const hobbit_F *d_f1, const hobbit_F *d_f2, const hobbit_F *d_f3,
                                 const hobbit_F *d_beta, size_t n, hobbit_F *h_K) {
    const F *t[8] = {cF(d_b1), cF(d_f1), cF(d_f2), cF(d_f3), cF(d_beta), nullptr, nullptr, nullptr}; F k[4];
    HB_TRY(launch_err_terms(ctx, 3, t, d_gate, n, k)); acc_K(h_K, k, 3); return 0;
}
int hobbit_compute4p_error_terms(hobbit_ctx *ctx, const hobbit_F *d_b1, const hobbit_F *d_b2, const hobbit_F *d_b3, const int32_t *d_gate, const hobbit_F *d_f1,
                                 const hobbit_F *d_f2, const hobbit_F *d_f3, const hobbit_F *d_f4, size_t n, hobbit_F *h_K) {
    const F *t[8] = {cF(d_b1), cF(d_b2), cF(d_b3), cF(d_f1), cF(d_f2), cF(d_f3), cF(d_f4), nullptr}; F k[4];
    HB_TRY(launch_err_terms(ctx, 4, t, d_gate, n, k)); acc_K(h_K, k, 4); return 0;
}
int hobbit_fold_axpy(hobbit_ctx *ctx, hobbit_F *d_fold, const hobbit_F *d_buff, const hobbit_F *h_rand, size_t n) {
    if (!n) return 0;
    return launch_axpy(ctx, mF(d_fold), cF(d_buff), *cF(h_rand), n);
}
int hobbit_fold_axpy_i32(hobbit_ctx *ctx, hobbit_F *d_fold, const int32_t *d_sel, const hobbit_F *h_rand, int one_minus, size_t n) {
    return launch_axpy_i32(ctx, mF(d_fold), d_sel, *cF(h_rand), one_minus, n);
}
int hobbit_batch_prod(hobbit_ctx *ctx, hobbit_F *d_f1, hobbit_F *d_f2, hobbit_F *d_f3, const hobbit_F *d_b1, const hobbit_F *d_b2, const hobbit_F *d_b3, int batches,
                      size_t n, const hobbit_F *h_r_last, const hobbit_F *h_a, const hobbit_F *h_rem_beta, hobbit_F *h_Kf, hobbit_F *h_Kp, hobbit_F *h_rand) {
    if (batches <= 0) return ctx->fail(HOBBIT_EINVAL, "batch_prod: batches must be positive");
    F K1 = fmake(0), K2 = fmake(0);
    std::vector<F> K3((size_t)batches);
    for (int j = 0; j < batches; j++) {
        const size_t o = (size_t)j * n;
        const F *t[8] = {cF(d_b1) + o, cF(d_b2) + o, cF(d_b3) + o, cF(d_f1) + o, cF(d_f2) + o, cF(d_f3) + o, nullptr, nullptr}; F k[4];
        HB_TRY(launch_err_terms(ctx, 13, t, nullptr, n, k));
        K1 = fadd(K1, fmul(cF(h_a)[j], k[0])); K2 = fadd(K2, fmul(cF(h_a)[j], k[1])); K3[j] = k[2];
    }
    F rnd = mimc_hash(K1, *cF(h_r_last));                  // mimc_hash(K, rand): argument order as in the reference (:1112-1116)
    rnd = mimc_hash(K2, rnd);
    for (int j = 0; j < batches; j++) rnd = mimc_hash(K3[j], rnd);
    const F x1 = rnd, x2 = fmul(rnd, x1), x3 = fmul(rnd, x2);
    F Kf = *cF(h_Kf);
    for (int j = 0; j < batches; j++) {
        mF(h_Kp)[j] = fadd(cF(h_Kp)[j], fmul(cF(h_rem_beta)[j], K3[j]));
        Kf = fadd(Kf, fmul(fmul(x3, cF(h_a)[j]), K3[j]));
    }
    Kf = fadd(Kf, fadd(fmul(x2, K2), fmul(x1, K1)));
    *mF(h_Kf) = Kf; *mF(h_rand) = rnd;
    const size_t tot = (size_t)batches * n;
    HB_TRY(launch_axpy(ctx, mF(d_f1), cF(d_b1), rnd, tot)); HB_TRY(launch_axpy(ctx, mF(d_f2), cF(d_b2), rnd, tot));
    return launch_axpy(ctx, mF(d_f3), cF(d_b3), rnd, tot);
}

// ---- batch_3product_sumcheck (src/sumcheck.cpp:275-372) -------------------------------------------------
static inline void cubic_of(const F &x0, const F &x1, const F &y0, const F &y1, const F &z0, const F &z1, F *p) {
    F dx = fsub(x1, x0), dy = fsub(y1, y0), dz = fsub(z1, z0);
    F qa = fmul(dx, dy), qb = fadd(fmul(dx, y0), fmul(x0, dy)), qc = fmul(x0, y0);
    p[0] = fadd(p[0], fmul(qa, dz)); p[1] = fadd(p[1], fadd(fmul(qa, z0), fmul(qb, dz)));
    p[2] = fadd(p[2], fadd(fmul(qb, z0), fmul(qc, dz))); p[3] = fadd(p[3], fmul(qc, z0));
}
int hobbit_batch_3product_sumcheck(hobbit_ctx *ctx, const hobbit_F *d_t1, const hobbit_F *d_t2, const hobbit_F *d_t3, const size_t *h_lens, int batches,
                                   const hobbit_F *h_a, hobbit_F *h_cpoly, hobbit_F *h_r, hobbit_F *h_vr) {
    if (batches <= 0) return ctx->fail(HOBBIT_EINVAL, "batch_3product_sumcheck: batches must be positive");
    size_t tot = 0, Lmax = 0;
    for (int j = 0; j < batches; j++) { if (ilog2_exact(h_lens[j]) < 0) return ctx->fail(HOBBIT_EINVAL, "batch_3product_sumcheck: lengths must be powers of two"); tot += h_lens[j]; Lmax = std::max(Lmax, h_lens[j]); }
    const int rounds = ilog2_exact(Lmax);
    // ping-pong copies of the three concatenated tables (inputs are preserved), partials, per-table coefficients
    F *ws; HB_TRY(ctx->workspace2((6 * tot + 4 * 1024 + 4 * (size_t)batches + 16) * sizeof(F), (void **)&ws));
    F *A = ws, *B = ws + 3 * tot, *part = B + 3 * tot, *coef = part + 4 * 1024;
    HB_TRY(launch_copy(ctx, A, d_t1, tot * sizeof(F)));
    HB_TRY(launch_copy(ctx, A + tot, d_t2, tot * sizeof(F)));
    HB_TRY(launch_copy(ctx, A + 2 * tot, d_t3, tot * sizeof(F)));
    std::vector<size_t> off(batches), len(batches); std::vector<char> set(batches, 0);
    std::vector<F> sc(3 * (size_t)batches);                          // host copies of tables that are down to one element
    { size_t o = 0; for (int j = 0; j < batches; j++) { off[j] = o; len[j] = h_lens[j]; o += h_lens[j]; } }
    F *pin; HB_TRY(ctx->pinned((4 * (size_t)batches + 3 * (size_t)batches) * sizeof(F), (void **)&pin));
    F *cur = A, *nxt = B;
    auto fetch_scalars = [&]() -> int {                             // read element 0 of every table that just reached length 1
        for (int j = 0; j < batches; j++) if (len[j] == 1 && set[j] == 0) {
            for (int t = 0; t < 3; t++) HB_CHECK(ctx, hipMemcpyAsync(pin + 4 * batches + 3 * j + t, cur + t * tot + off[j], sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
        }
        HB_TRY(ctx->sync());
        for (int j = 0; j < batches; j++) if (len[j] == 1 && set[j] == 0) { for (int t = 0; t < 3; t++) sc[3 * j + t] = pin[4 * batches + 3 * j + t]; set[j] = 2; }
        return 0;
    };
    HB_TRY(fetch_scalars());
    F rnd = fmake(312);
    for (int i = 0; i < rounds; i++) {
        for (int j = 0; j < batches; j++) if (len[j] >= 2) HB_TRY(launch_sc3_poly(ctx, cur + off[j], cur + tot + off[j], cur + 2 * tot + off[j], len[j] / 2, part, coef + 4 * j));
        HB_CHECK(ctx, hipMemcpyAsync(pin, coef, 4 * (size_t)batches * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
        HB_TRY(ctx->sync());
        F poly[4] = {fmake(0), fmake(0), fmake(0), fmake(0)};
        for (int j = 0; j < batches; j++) {
            F p[4] = {fmake(0), fmake(0), fmake(0), fmake(0)};
            if (len[j] >= 2) { for (int q = 0; q < 4; q++) p[q] = pin[4 * j + q]; }
            else {
                if (set[j] != 1) { for (int t = 0; t < 3; t++) mF(h_vr)[3 * j + t] = sc[3 * j + t]; set[j] = 1; }     // P.vr recorded the first time (:316-320)
                cubic_of(sc[3 * j], fmake(0), sc[3 * j + 1], fmake(0), sc[3 * j + 2], fmake(0), p);                      // linear_poly(-v, v)
            }
            for (int q = 0; q < 4; q++) poly[q] = fadd(poly[q], fmul(cF(h_a)[j], p[q]));
        }
        for (int q = 0; q < 4; q++) { rnd = mimc_hash(rnd, poly[q]); mF(h_cpoly)[4 * i + q] = poly[q]; }
        mF(h_r)[i] = rnd;
        for (int j = 0; j < batches; j++) {
            if (len[j] >= 2) { HB_TRY(launch_fold3(ctx, cur + off[j], cur + tot + off[j], cur + 2 * tot + off[j], nxt + off[j], nxt + tot + off[j], nxt + 2 * tot + off[j], len[j] / 2, rnd)); len[j] /= 2; }
            else { F om = fsub(fmake(1), rnd); for (int t = 0; t < 3; t++) sc[3 * j + t] = fmul(om, sc[3 * j + t]); }
        }
        std::swap(cur, nxt);
        // tables of length 1 were not copied by the fold: their scalars live on the host from now on
        HB_TRY(fetch_scalars());
    }
    for (int j = 0; j < batches; j++) if (set[j] != 1) for (int t = 0; t < 3; t++) mF(h_vr)[3 * j + t] = sc[3 * j + t];
    return 0;
}

// ---- prove_multiplication_tree_new (src/sumcheck.cpp:35-257), power-of-two vectors x size ---------------------
static int mul_tree_impl(hobbit_ctx *ctx, const hobbit_F *d_input, size_t vectors, size_t size, const hobbit_F *h_previous_r, const hobbit_F *h_prev_x,
                         hobbit_F *h_cpoly, hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_fin, hobbit_F *h_final_r, hobbit_F *h_out_eval, hobbit_F *h_final_eval, int *layers_out,
                         hobbit_F *h_output);
int hobbit_mul_tree(hobbit_ctx *ctx, const hobbit_F *d_input, size_t vectors, size_t size, const hobbit_F *h_previous_r, const hobbit_F *h_prev_x,
                    hobbit_F *h_cpoly, hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_fin, hobbit_F *h_final_r, hobbit_F *h_out_eval, hobbit_F *h_final_eval, int *layers_out) {
    return mul_tree_impl(ctx, d_input, vectors, size, h_previous_r, h_prev_x, h_cpoly, h_r, h_vr, h_fin, h_final_r, h_out_eval, h_final_eval, layers_out, nullptr);
}
// h_output (nullable): Proof.output = the `vectors` products (top layer of the tree)
static int mul_tree_impl(hobbit_ctx *ctx, const hobbit_F *d_input, size_t vectors, size_t size, const hobbit_F *h_previous_r, const hobbit_F *h_prev_x,
                         hobbit_F *h_cpoly, hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_fin, hobbit_F *h_final_r, hobbit_F *h_out_eval, hobbit_F *h_final_eval, int *layers_out,
                         hobbit_F *h_output) {
    const int depth = ilog2_exact(size), lv = ilog2_exact(vectors);
    if (depth < 1 || lv < 0) return ctx->fail(HOBBIT_EINVAL, "mul_tree: vectors and size must be powers of two (the host mirror pads as the reference does)");
    const size_t total = vectors * size;
    F *arena; HB_TRY(ctx->workspace3((3 * total + total + 16) * sizeof(F), (void **)&arena));    // in1 | in2 | transcript layers (sum = total each), beta
    F *in1 = arena, *in2 = arena + total, *tr = arena + 2 * total, *beta = arena + 3 * total;
    std::vector<size_t> lo(depth);
    { size_t o = 0, len = total; const F *src = cF(d_input);
      for (int i = 0; i < depth; i++) { len /= 2; lo[i] = o; HB_TRY(launch_mul_layer(ctx, src, len, in1 + o, in2 + o, tr + o)); src = tr + o; o += len; } }
    F previous_r = *cF(h_previous_r), sum;
    std::vector<F> r; int layers = 0; size_t qo = 0, ro = 0;
    if (h_output) HB_TRY(hobbit_memcpy_d2h(ctx, h_output, tr + lo[depth - 1], vectors * sizeof(F)));
    if (vectors == 1) {
        F top; HB_TRY(hobbit_memcpy_d2h(ctx, &top, tr + lo[depth - 1], sizeof(F)));
        previous_r = mimc_hash(previous_r, top); sum = top;
    } else {
        r.resize(lv);
        if (h_prev_x) memcpy((void *)r.data(), h_prev_x, sizeof(F) * lv);
        else { F cst = fmake(0); for (int i = 0; i < lv; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); r[i] = fadd(cst, fmake((uint64_t)rand())); } }   // generate_randomness
        HB_TRY(hobbit_eval_vector(ctx, reinterpret_cast<hobbit_F *>(tr + lo[depth - 1]), vectors, reinterpret_cast<hobbit_F *>(r.data()), reinterpret_cast<hobbit_F *>(&sum)));
        if (!h_prev_x) previous_r = mimc_hash(r[lv - 1], sum);
    }
    *mF(h_out_eval) = sum;
    for (int i = depth - 1; i >= 0; i--) {
        if (r.empty()) {
            F a, b; HB_TRY(hobbit_memcpy_d2h(ctx, &a, in1 + lo[i], sizeof(F))); HB_TRY(hobbit_memcpy_d2h(ctx, &b, in2 + lo[i], sizeof(F)));
            F num = mimc_hash(previous_r, a); previous_r = mimc_hash(num, b);
            sum = fadd(fmul(fsub(fmake(1), previous_r), a), fmul(previous_r, b));
            r.push_back(previous_r);
        } else {
            const int rl = (int)r.size(); const size_t n = (size_t)1 << rl;
            HB_TRY(hobbit_eq_table(ctx, reinterpret_cast<hobbit_F *>(r.data()), rl, reinterpret_cast<hobbit_F *>(beta)));
            HB_TRY(hobbit_sumcheck3(ctx, reinterpret_cast<hobbit_F *>(in1 + lo[i]), reinterpret_cast<hobbit_F *>(in2 + lo[i]), reinterpret_cast<hobbit_F *>(beta), n,
                                    reinterpret_cast<hobbit_F *>(&previous_r), h_cpoly + qo, h_r + ro, h_vr + 3 * layers, h_fin + layers));
            CHP q0 = cF(h_cpoly + qo);
            F claim = fadd(fadd(fadd(q0[0], q0[1]), fadd(q0[2], q0[3])), q0[3]);        // P.c_poly[0].eval(1) + eval(0)
            if (!feq(claim, sum)) printf("error %d\n", i);                              // the reference's own (non-fatal) check, :151,:203
            for (int t = 0; t < rl; t++) r[t] = cF(h_r + ro)[t];
            previous_r = cF(h_fin)[layers];
            sum = fadd(fmul(cF(h_vr)[3 * layers], fsub(fmake(1), previous_r)), fmul(cF(h_vr)[3 * layers + 1], previous_r));
            r.insert(r.begin(), previous_r);
            qo += 4 * (size_t)rl; ro += (size_t)rl; layers++;
        }
    }
    memcpy(h_final_r, r.data(), sizeof(F) * r.size()); *mF(h_final_eval) = sum;
    if (layers_out) *layers_out = layers;
    return 0;
}

// ---- Elastic_PC open, RS x RS (test_Elastic_PC option 1): src/Elastic_PC.cpp:625-726 ---------------------------------
// The stream stays with the host, as in the commit: pass 2 (aggregate, :316-347) and pass 3 (compute_aggregation_reply /
// update_reply, :487-533, 59-111) receive the chunks as device buffers, in stream order.
struct hobbit_elastic_open {
    hobbit_ctx *ctx; size_t N, B, K; int trs, queries; uint32_t cols, rows2;
    std::vector<F> beta; std::vector<uint32_t> qc, qr, ucols, qci; F rv0;
    size_t n_aggr, n_reply; bool committed;
    enum Form { NONE, FULL, REAL };                         // what a pass has been fed so far: F chunks or base-field chunks (include/hobbit_elastic_real.h), never both
    Form aggr_form = NONE, reply_form = NONE;
    int form(Form &pass, Form f, const char *who) {
        if (pass != NONE && pass != f) return ctx->fail(HOBBIT_ESTATE, std::string(who) + ": F chunks and base-field chunks may not be mixed within one pass");
        pass = f; return 0;
    }
    mem::Pooled<F> d_aggr, d_T, d_G, d_reply, d_encf; mem::Pooled<uint8_t> d_lvf; mem::Pooled<uint32_t> d_ucols; mem::Pooled<uint64_t> d_pick; mem::Pooled<int> d_nz;
    // option 2 (linear_time, RS x expander): the "remaining" columns (a queried parity row), the aggregate's row codes M, aux_commit and C_c
    bool lin; std::vector<uint32_t> rem; size_t np;
    mem::Pooled<F> d_M, d_aux, d_encc; mem::Pooled<uint8_t> d_lvc; mem::Pooled<uint32_t> d_rem;
    // the nine buffers both options use, of these sizes (capacities, not the distinct-column count), in this order
    int get9(const size_t (&sz)[9]) {
        return ctx->pool_get(sz[0], d_aggr) || ctx->pool_get(sz[1], d_T) || ctx->pool_get(sz[2], d_G) || ctx->pool_get(sz[3], d_reply) || ctx->pool_get(sz[4], d_encf) ||
               ctx->pool_get(sz[5], d_lvf) || ctx->pool_get(sz[6], d_ucols) || ctx->pool_get(sz[7], d_pick) || ctx->pool_get(sz[8], d_nz);
    }
};
// precompute_beta (src/utils.cpp:251-296) on the host for a handful of variables
static void host_eq_table(CHP r, int k, std::vector<F> &out) {
    out.assign((size_t)1 << k, fmake(0)); out[0] = fmake(1);
    for (int i = 0; i < k; i++) for (size_t j = ((size_t)1 << i); j-- > 0;) { F t = fmul(r[k - 1 - i], out[j]); out[2 * j + 1] = t; out[2 * j] = fsub(out[j], t); }
}
// ---- recursive_prover_RS (src/PC_utils.cpp:396-512): the aggregate (B elements, trs rows), its queries, C_f (encoded matrix + tree) -> P0, P2, P3, P5
// and shockwave_prove(C_f, r_x).  Shared by Elastic_PC::open option 1 and Our_PC's open_standard with linear_time == false.
static int rs_prover_dev(hobbit_ctx *ctx, const F *d_aggr, size_t B, size_t trs, const std::vector<uint32_t> &qc, const std::vector<uint32_t> &qr,
                         const std::vector<uint32_t> &ucols, const uint32_t *d_ucols, const F *d_encf, const uint8_t *d_lvf, hobbit_elastic_open_out *o) {
    const size_t half = B / trs, cols = 2 * half, rows2 = 2 * trs, nq = qc.size(), nc = ucols.size();
    const int logc = ilog2_exact(cols), logr = ilog2_exact(rows2), logt = logr - 1;
    if (logc < 1 || logc > 24 || logr < 2 || logr > 12) return ctx->fail(HOBBIT_EINVAL, "recursive_prover_RS: needs 2 <= 2*trs <= 4096 and a power-of-two row length");
    size_t np2 = 1; while (np2 < nc) np2 <<= 1;
    const int R0 = ilog2_exact(np2 * rows2);
    F *arena; HB_TRY(ctx->workspace3((2 * B + np2 * trs + 2 * np2 * rows2 + 2 * B + 4096 + 64) * sizeof(F), (void **)&arena));
    F *out1 = arena, *sel = out1 + 2 * B, *out3 = sel + np2 * trs, *bt = out3 + np2 * rows2, *b2 = bt + np2 * rows2, *stage = b2 + 2 * B;
    HB_TRY(fft::any_rows(ctx, d_aggr, half, half, out1, logc, false, trs));                                                   // out_1 (:406-420)
    HB_TRY(launch_zero(ctx, sel, (np2 * trs + 2 * np2 * rows2 + 2 * B) * sizeof(F)));                         // sel | out3 | bt | b2
    HB_TRY(launch_gather_cols(ctx, out1, cols, (uint32_t)trs, d_ucols, (uint32_t)nc, sel, trs));                                // selected_collumns (:422-431)
    HB_TRY(fft::rows(ctx, sel, trs, (uint32_t)trs, out3, rows2, 1, logr, false, 1, (uint32_t)nc, 0, 0));                            // out_3 (:436-452)
    std::vector<F> rq(nq);
    { F cst = fmake(0); for (size_t i = 0; i < nq; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); rq[i] = fadd(cst, fmake((uint64_t)rand())); } }   // r = generate_randomness(I.size()) (:459)
    {   // beta (:461-470): the sorted column walk is paired with the UNSORTED query rows, duplicates accumulate
        std::vector<uint32_t> cs(qc); std::sort(cs.begin(), cs.end());
        std::map<uint64_t, F> acc; size_t counter = 0;
        for (size_t i = 0; i < nq; i++) {
            if (ucols[counter] != cs[i]) counter++;
            const uint64_t at = counter * rows2 + qr[i];
            auto it = acc.find(at);
            if (it == acc.end()) acc[at] = rq[i]; else it->second = fadd(it->second, rq[i]);
        }
        uint8_t *pin; HB_TRY(ctx->pinned(std::max(nq * (sizeof(F) + 8) + 64, (size_t)2048 * sizeof(F)), (void **)&pin));
        F *pv = reinterpret_cast<F *>(pin); uint64_t *pi = reinterpret_cast<uint64_t *>(pin + nq * sizeof(F));
        size_t n = 0; for (auto &kv : acc) { pi[n] = kv.first; pv[n] = kv.second; n++; }
        F *dv = stage; uint64_t *di = reinterpret_cast<uint64_t *>(stage + nq);
        if (2 * nq > 4096) return ctx->fail(HOBBIT_EINVAL, "recursive_prover_RS: too many queries for the staging area");
        HB_CHECK(ctx, hipMemcpyAsync(dv, pv, n * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
        HB_CHECK(ctx, hipMemcpyAsync(di, pi, n * 8, hipMemcpyHostToDevice, ctx->stream));
        HB_TRY(launch_scatter(ctx, di, dv, n, bt));
    }
    hobbit_F p323 = {323, 0};
    hobbit_F *Q = o->qpoly, *Rr = o->r;
    HB_TRY(hobbit_sumcheck2(ctx, reinterpret_cast<hobbit_F *>(out3), reinterpret_cast<hobbit_F *>(bt), np2 * rows2, &p323, Q, Rr, o->vr, o->fin));          // P0 (:474)
    const hobbit_F *r0 = Rr; Q += 3 * R0; Rr += R0;
    HB_TRY(hobbit_prove_fft_matrix(ctx, reinterpret_cast<hobbit_F *>(sel), np2, trs, r0, Q, Rr, o->vr + 2, o->fin + 1));                                       // P2 (:480)
    { CHP q2 = cF(Q); o->checks[0] = feq(fadd(fadd(q2[0], q2[1]), fadd(q2[2], q2[2])), cF(o->vr)[0]); }                                                   // src/sumcheck.cpp:3016-3019
    const hobbit_F *r2 = Rr; Q += 3 * logr; Rr += logr;
    // r_point: P2.randomness[0] (its logr sumcheck challenges, then r1 = P0.r[logr..]) from index log2(trs) on (:482-485)
    std::vector<F> rpt; rpt.push_back(cF(r2)[logt]);
    for (int i = logr; i < R0; i++) rpt.push_back(cF(r0)[i]);
    std::vector<F> rb; host_eq_table(rpt.data(), (int)rpt.size(), rb);
    {   // beta[collumns[i] + j*cols] = r[i] (:489-496)
        uint8_t *pin; HB_TRY(ctx->pinned(2048 * sizeof(F), (void **)&pin));
        if (nc > 2048) return ctx->fail(HOBBIT_EINVAL, "recursive_prover_RS: more than 2048 distinct columns");
        HB_TRY(ctx->sync());                                    // (the staging buffer's previous contents have been consumed: sumcheck2 synchronised)
        memcpy(pin, rb.data(), nc * sizeof(F));
        HB_CHECK(ctx, hipMemcpyAsync(stage, pin, nc * sizeof(F), hipMemcpyHostToDevice, ctx->stream));
        HB_TRY(launch_spread_cols(ctx, d_ucols, stage, (uint32_t)nc, (uint32_t)trs, cols, b2));
    }
    HB_TRY(hobbit_sumcheck2(ctx, reinterpret_cast<hobbit_F *>(out1), reinterpret_cast<hobbit_F *>(b2), trs * cols, &p323, Q, Rr, o->vr + 4, o->fin + 2));     // P3 (:498)
    const hobbit_F *r3 = Rr; Q += 3 * (logt + logc); Rr += logt + logc;
    HB_TRY(hobbit_prove_fft_matrix(ctx, reinterpret_cast<const hobbit_F *>(d_aggr), trs, half, r3, Q, Rr, o->vr + 6, o->fin + 3));                               // P5 (:503)
    { CHP q5 = cF(Q); o->checks[1] = feq(fadd(fadd(q5[0], q5[1]), fadd(q5[2], q5[2])), cF(o->vr)[4]); }
    // r_x = P5.randomness[0]: its sumcheck challenges, then r1 = P3.r[logc .. logc + log2 trs) (src/sumcheck.cpp:3021-3023)
    std::vector<hobbit_F> rx((size_t)logc + (size_t)logt);
    memcpy(rx.data(), Rr, sizeof(hobbit_F) * (size_t)logc); memcpy(rx.data() + logc, r3 + logc, sizeof(hobbit_F) * (size_t)logt);
    if (o->rx) memcpy(o->rx, rx.data(), sizeof(hobbit_F) * rx.size());
    if (o->sp_f) HB_TRY(hobbit_shockwave_prove(ctx, reinterpret_cast<const hobbit_F *>(d_aggr), reinterpret_cast<const hobbit_F *>(d_encf), d_lvf, B, 32, rx.data(), (int)rx.size(), o->sp_f));   // (:507)
    return 0;
}
void hobbit_elastic_open_free(hobbit_elastic_open *e) { delete e; }

// ---- Elastic_PC open, RS x expander (test_Elastic_PC option 2, linear_time == true): src/Elastic_PC.cpp:625-726 with aggregate()'s linear_time
// branch (:348-413), update_reply_spielman (:431-485) and recursive_prover_Spielman_stream (src/PC_utils.cpp:168-270) ------------------------
// The reference AS BUILT (oracle/check_elastic_open2_determinism.py: the real reference returns the same bytes from fresh processes): for a
// queried column with a parity-row query update_reply_spielman copies the un-encoded column over the first tensor_row_size entries of buff2
// and leaves the rest as it was -- the parity of the last column that went through encode_monolithic in this chunk, zeros before any did.
// Per reply slot the begin function works out which column's codeword that is, once; the passes then encode every distinct column and gather.
static int elastic_open_begin_lin(hobbit_ctx *ctx, size_t N, size_t B, int trs, const hobbit_F *h_x, int queries, hobbit_elastic_open **out) {
    if (trs <= 0 || trs > 4096 || ilog2_exact(B) < 0 || ilog2_exact((size_t)trs) < 0 || B % (size_t)trs || 2 * B / (size_t)trs < 64 || 2 * B / (size_t)trs > ((size_t)1 << 24))
        return ctx->fail(HOBBIT_EINVAL, "elastic_open (linear_time): needs power-of-two B and trs <= 4096 with row codes of 64 .. 2^24 points (the reference: trs = B/2^14)");
    if (N % B || ilog2_exact(N / B) < 0 || queries <= 0 || !h_x) return ctx->fail(HOBBIT_EINVAL, "elastic_open: N/B must be a power of two");
    Handle<hobbit_elastic_open, hobbit_elastic_open_free> e(new hobbit_elastic_open());
    e->ctx = ctx; e->N = N; e->B = B; e->K = N / B; e->trs = trs; e->queries = queries; e->cols = (uint32_t)(2 * B / (size_t)trs); e->rows2 = (uint32_t)(2 * trs);
    e->n_aggr = e->n_reply = 0; e->committed = false; e->lin = true;
    host_eq_table(cF(h_x), ilog2_exact(e->K), e->beta);                                                     // precompute_beta(x1, beta) (:638-643)
    e->rv0 = fadd(fmake((uint64_t)random()), fmake((uint64_t)rand()));                                      // r_v[0] = generate_randomness(1)[0] (:645)
    const size_t nq = (size_t)queries;
    e->qc.resize(nq); e->qr.resize(nq);
    for (size_t q = 0; q < nq; q++) { e->qc[q] = (uint32_t)(rand() % (long)e->cols); e->qr[q] = (uint32_t)(rand() % (long)e->rows2); }   // (:650-655)
    e->ucols = e->qc; std::sort(e->ucols.begin(), e->ucols.end()); e->ucols.erase(std::unique(e->ucols.begin(), e->ucols.end()), e->ucols.end());
    const size_t nc = e->ucols.size();
    e->qci.resize(nq);
    std::vector<char> flag(nc, 0);                                                                          // a queried row >= tensor_row_size (:376-391, :462-468)
    for (size_t q = 0; q < nq; q++) {
        e->qci[q] = (uint32_t)(std::lower_bound(e->ucols.begin(), e->ucols.end(), e->qc[q]) - e->ucols.begin());
        if (e->qr[q] >= (uint32_t)trs) flag[e->qci[q]] = 1;
    }
    for (size_t c = 0; c < nc; c++) if (flag[c]) e->rem.push_back(e->ucols[c]);
    const size_t nr = e->rem.size();
    e->np = 1; while (e->np < nr * e->rows2) e->np <<= 1;
    // the parity a reply slot reads: its own column's when the column was encoded, else that of the last encoded column before it (row nc = zeros)
    std::vector<uint32_t> par(nc); { uint32_t last = (uint32_t)nc; for (size_t c = 0; c < nc; c++) { if (!flag[c]) last = (uint32_t)c; par[c] = last; } }
    // reply row `counter` is the counter-th query in (sorted column, then query order) (:476-478 over column_map)
    std::vector<uint32_t> start(nc + 1, 0), ord(nq);
    for (size_t q = 0; q < nq; q++) start[e->qci[q] + 1]++;
    for (size_t c = 0; c < nc; c++) start[c + 1] += start[c];
    { std::vector<uint32_t> fill(start.begin(), start.end() - 1); for (size_t q = 0; q < nq; q++) ord[fill[e->qci[q]]++] = (uint32_t)q; }
    std::vector<uint64_t> pick(nq);
    for (size_t k = 0; k < nq; k++) {
        const uint32_t q = ord[k], c = e->qci[q], row = e->qr[q];
        pick[k] = (uint64_t)(row < (uint32_t)trs ? c : par[c]) * e->rows2 + row;
    }
    const size_t sizes[9] = {B * sizeof(F), 2 * B * sizeof(F), (nc + 1) * e->rows2 * sizeof(F), e->K * nq * sizeof(F), 2 * B * sizeof(F),
                             64 * (2 * B / 32), nq * 4, nq * 8, e->K * sizeof(int)};
    if (e->get9(sizes) || ctx->pool_get(2 * B * sizeof(F), e->d_M) || ctx->pool_get(e->np * sizeof(F), e->d_aux) || ctx->pool_get(2 * e->np * sizeof(F), e->d_encc) ||
        ctx->pool_get(64 * (2 * e->np / 32), e->d_lvc) || ctx->pool_get((nr ? nr : 1) * 4, e->d_rem))
        return ctx->fail(HOBBIT_ENOMEM, "elastic_open_begin: allocation failed");
    HB_TRY(launch_zero(ctx, e->d_aggr, B * sizeof(F)));
    HB_TRY(launch_zero(ctx, e->d_nz, e->K * sizeof(int)));
    HB_TRY(launch_zero(ctx, e->d_G, (nc + 1) * e->rows2 * sizeof(F)));                                     // the zero row; the tails past the codeword length stay zero
    HB_CHECK(ctx, hipMemcpyAsync(e->d_ucols, e->ucols.data(), nc * 4, hipMemcpyHostToDevice, ctx->stream));
    HB_CHECK(ctx, hipMemcpyAsync(e->d_pick, pick.data(), nq * 8, hipMemcpyHostToDevice, ctx->stream));
    if (nr) HB_CHECK(ctx, hipMemcpyAsync(e->d_rem, e->rem.data(), nr * 4, hipMemcpyHostToDevice, ctx->stream));
    HB_TRY(ctx->sync());                                                        // `pick` is a local
    *out = e.release();
    return 0;
}
// recursive_prover_Spielman_stream(aggr_vector, aggr_tensor = d_M, aux_commit = d_aux, I) (src/PC_utils.cpp:168-270).  Transcripts P1, P2, P3, P5 back
// to back in o->qpoly / o->r (rounds log2 2trs, log2 cols, log2 np, log2 cols); o->scal = s[0], s2, y1; checks[0] = prove_fft_matrix's exit(-1) test.
static int spielman_stream_dev(hobbit_ctx *ctx, hobbit_elastic_open *e, hobbit_elastic_open_out *o) {
    const size_t B = e->B, trs = (size_t)e->trs, cols = e->cols, rows2 = e->rows2, half = cols / 2, nq = (size_t)e->queries, nr = e->rem.size(), np = e->np;
    const int logc = ilog2_exact(cols), R1 = ilog2_exact(rows2), logt = R1 - 1, R3 = ilog2_exact(np);
    if (!nr) return ctx->fail(HOBBIT_EINVAL, "elastic_open (linear_time): no queried parity row (the reference indexes an empty vector here)");
    if (nq > np) return ctx->fail(HOBBIT_EINVAL, "elastic_open (linear_time): more queries than padded aux_commit entries (the reference writes past its vector here)");
    if (!o->sp_c || !o->sp_f || !o->scal) return ctx->fail(HOBBIT_EINVAL, "elastic_open (linear_time): sp_c, sp_f and scal are required");
    if (o->cc_root) HB_TRY(hobbit_memcpy_d2h(ctx, o->cc_root, e->d_lvc + 32 * (2 * (2 * np / 32) - 2), 32));
    if (o->nrem) *o->nrem = (int)nr;
    F *arena; HB_TRY(ctx->workspace3((nr + 2 * rows2 + 2 * cols + np + 64) * sizeof(F), (void **)&arena));
    F *d_s = arena, *d_ac = d_s + nr, *d_b1 = d_ac + rows2, *d_ev = d_b1 + rows2, *d_sM = d_ev + cols, *d_b2 = d_sM + cols;
    StageScope sc(ctx);
    std::vector<F> sv(nr);
    sv[0] = fmake((uint64_t)random()); *mF(&o->scal[0]) = sv[0];                                           // s[0] = random() (:209-213)
    for (size_t i = 1; i < nr; i++) sv[i] = fmul(sv[i - 1], sv[0]);
    HB_TRY(h2d_staged(ctx, d_s, sv.data(), nr * sizeof(F)));
    HB_TRY(launch_vecmat(ctx, e->d_aux, nr, rows2, d_s, d_ac));                                             // aggr_c = sum_i s[i] codewords[i] (:214-219)
    std::vector<F> r1(R1);
    { F cst = fmake(0); for (int i = 0; i < R1; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); r1[i] = fadd(cst, fmake((uint64_t)rand())); } }   // prove_linear_code's generate_randomness
    hobbit_F *Q = o->qpoly, *Rr = o->r;
    hobbit_F *const Q1 = Q, *const Rr1 = Rr, *const Q2 = Q1 + 3 * R1, *const Rr2 = Rr1 + R1, *const Q3 = Q2 + 3 * logc, *const Rr3 = Rr2 + logc, *const Q5 = Q3 + 3 * R3,
             *const Rr5 = Rr3 + R3;
    if (ctx->code.n != e->trs) { long long l; HB_TRY(hobbit_graph_finalize(ctx, e->trs, &l)); }
    HB_TRY(hobbit_prove_linear_code(ctx, reinterpret_cast<hobbit_F *>(d_ac), rows2, (long long)trs, reinterpret_cast<const hobbit_F *>(r1.data()), Q1, Rr1, o->vr, o->fin));   // P1 (:221)
    HB_TRY(hobbit_eq_table(ctx, Rr1, R1, reinterpret_cast<hobbit_F *>(d_b1)));
    HB_TRY(launch_vecmat(ctx, e->d_M, trs, cols, d_b1, d_ev));                                              // evals[i] = sum_{j < trs} beta[j] M[j][i] (:226-230)
    HB_TRY(launch_zero(ctx, d_sM, cols * sizeof(F)));
    HB_TRY(launch_spread_cols(ctx, e->d_rem, d_s, (uint32_t)nr, 1, cols, d_sM));                            // sM[remaining_columns[j]] = s[j] (:231-234)
    hobbit_F p17 = {021, 0}, p121 = {121, 0};
    HB_TRY(hobbit_sumcheck2(ctx, reinterpret_cast<hobbit_F *>(d_sM), reinterpret_cast<hobbit_F *>(d_ev), cols, &p17, Q2, Rr2, o->vr + 2, o->fin + 1));   // P2 (:237)
    std::vector<F> pw(nq);
    F s2 = fmake((uint64_t)random()); *mF(&o->scal[1]) = s2;                                                // (:242)
    for (size_t i = 0; i < nq; i++) { pw[i] = s2; s2 = fmul(s2, s2); }                                      // buff2[i] = s2; s2 = s2*s2 (:243-246): repeated squares at 0 .. nq-1
    HB_TRY(launch_zero(ctx, d_b2, np * sizeof(F)));
    HB_TRY(h2d_staged(ctx, d_b2, pw.data(), nq * sizeof(F)));
    HB_TRY(hobbit_sumcheck2(ctx, reinterpret_cast<hobbit_F *>(e->d_aux.get()), reinterpret_cast<hobbit_F *>(d_b2), np, &p121, Q3, Rr3, o->vr + 4, o->fin + 2));   // P3 (:248)
    HB_TRY(hobbit_shockwave_prove(ctx, reinterpret_cast<hobbit_F *>(e->d_aux.get()), reinterpret_cast<hobbit_F *>(e->d_encc.get()), e->d_lvc, np, 32, Rr3, R3, o->sp_c));   // (:252)
    // r = P1.randomness[0] (all of it: the pop_back at :256 follows the copy) | P2.randomness[0]; evaluate_vector and prove_fft_matrix use its first
    // log2(trs * cols) entries, the transcript of P5 is seeded with its last one (:255-266)
    std::vector<hobbit_F> rcat((size_t)R1 + (size_t)logc);
    memcpy(rcat.data(), Rr1, sizeof(hobbit_F) * (size_t)R1); memcpy(rcat.data() + R1, Rr2, sizeof(hobbit_F) * (size_t)logc);
    F y1;
    HB_TRY(hobbit_eval_vector(ctx, reinterpret_cast<hobbit_F *>(e->d_M.get()), trs * cols, rcat.data(), reinterpret_cast<hobbit_F *>(&y1)));
    *mF(&o->scal[2]) = y1;
    HB_TRY(prove_fft_matrix_seeded(ctx, reinterpret_cast<const hobbit_F *>(e->d_aggr.get()), trs, half, rcat.data(), &rcat[rcat.size() - 1], Q5, Rr5, o->vr + 6, o->fin + 3));   // P5 (:266)
    { CHP q5 = cF(Q5); o->checks[0] = feq(fadd(fadd(q5[0], q5[1]), fadd(q5[2], q5[2])), y1); }      // src/sumcheck.cpp:3016-3019
    // P5.randomness[0] = its logc challenges | r1 = r[logc .. logc + log2 trs); pop_back (:268); shockwave_prove(C_f, .) (:269)
    std::vector<hobbit_F> rx((size_t)logc + (size_t)logt);
    memcpy(rx.data(), Rr5, sizeof(hobbit_F) * (size_t)logc); memcpy(rx.data() + logc, rcat.data() + logc, sizeof(hobbit_F) * (size_t)logt);
    rx.pop_back();
    if (o->rx) memcpy(o->rx, rx.data(), sizeof(hobbit_F) * rx.size());
    HB_TRY(hobbit_shockwave_prove(ctx, reinterpret_cast<const hobbit_F *>(e->d_aggr.get()), reinterpret_cast<const hobbit_F *>(e->d_encf.get()), e->d_lvf, B, 32, rx.data(), (int)rx.size(), o->sp_f));
    return sc.finish();
}
static int elastic_open_begin_lin(hobbit_ctx *ctx, size_t N, size_t B, int trs, const hobbit_F *h_x, int queries, hobbit_elastic_open **out);
int hobbit_elastic_open_begin_lin(hobbit_ctx *ctx, size_t N, size_t B, int trs, const hobbit_F *h_x, int queries, hobbit_elastic_open **out) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    return elastic_open_begin_lin(ctx, N, B, trs, h_x, queries, out);
}
int hobbit_elastic_open_begin(hobbit_ctx *ctx, size_t N, size_t B, int trs, const hobbit_F *h_x, int queries, hobbit_elastic_open **out) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    if (trs <= 0 || ilog2_exact(B) < 0 || ilog2_exact((size_t)trs) < 0 || B % (size_t)trs || 2 * B / (size_t)trs != 4096 || 2 * trs > 4096)
        return ctx->fail(HOBBIT_EINVAL, "elastic_open: needs trs = B/2^11 (4096-point row codes) and 2*trs <= 4096");
    if (N % B || ilog2_exact(N / B) < 0 || queries <= 0 || !h_x) return ctx->fail(HOBBIT_EINVAL, "elastic_open: N/B must be a power of two");
    Handle<hobbit_elastic_open, hobbit_elastic_open_free> e(new hobbit_elastic_open());
    e->ctx = ctx; e->N = N; e->B = B; e->K = N / B; e->trs = trs; e->queries = queries; e->cols = 4096; e->rows2 = (uint32_t)(2 * trs);
    e->n_aggr = e->n_reply = 0; e->committed = false; e->lin = false;
    host_eq_table(cF(h_x), ilog2_exact(e->K), e->beta);                                                     // precompute_beta(x1, beta) (:638-643)
    e->rv0 = fadd(fmake((uint64_t)random()), fmake((uint64_t)rand()));                                      // r_v[0] = generate_randomness(1)[0] (:645)
    e->qc.resize(queries); e->qr.resize(queries);
    for (int q = 0; q < queries; q++) { e->qc[q] = (uint32_t)(rand() % (long)e->cols); e->qr[q] = (uint32_t)(rand() % (long)e->rows2); }   // (:650-655)
    e->ucols = e->qc; std::sort(e->ucols.begin(), e->ucols.end()); e->ucols.erase(std::unique(e->ucols.begin(), e->ucols.end()), e->ucols.end());
    const size_t nc = e->ucols.size();
    e->qci.resize(queries); std::vector<uint64_t> pick(queries);
    for (int q = 0; q < queries; q++) {
        e->qci[q] = (uint32_t)(std::lower_bound(e->ucols.begin(), e->ucols.end(), e->qc[q]) - e->ucols.begin());
        pick[q] = (uint64_t)e->qci[q] * e->rows2 + e->qr[q];
    }
    const size_t sizes[9] = {B * sizeof(F), (size_t)trs * 4096 * sizeof(F), (size_t)queries * e->rows2 * sizeof(F), e->K * (size_t)queries * sizeof(F), 2 * B * sizeof(F),
                             64 * (2 * B / 32), (size_t)queries * 4, (size_t)queries * 8, e->K * sizeof(int)};
    if (e->get9(sizes)) return ctx->fail(HOBBIT_ENOMEM, "elastic_open_begin: allocation failed");
    HB_TRY(launch_zero(ctx, e->d_aggr, B * sizeof(F)));
    HB_TRY(launch_zero(ctx, e->d_nz, e->K * sizeof(int)));
    HB_CHECK(ctx, hipMemcpyAsync(e->d_ucols, e->ucols.data(), nc * 4, hipMemcpyHostToDevice, ctx->stream));
    HB_CHECK(ctx, hipMemcpyAsync(e->d_pick, pick.data(), (size_t)queries * 8, hipMemcpyHostToDevice, ctx->stream));
    HB_TRY(ctx->sync());                                                        // `pick` is a local
    *out = e.release();
    return 0;
}
void hobbit_elastic_open_dims(const hobbit_elastic_open *e, int *ncols, int *nrem, size_t *np) {
    if (ncols) *ncols = (int)e->ucols.size();
    if (nrem) *nrem = e->lin ? (int)e->rem.size() : 0;
    if (np) *np = e->lin ? e->np : 0;
}
int hobbit_elastic_open_aggregate_push(hobbit_ctx *ctx, hobbit_elastic_open *e, const hobbit_F *d_chunk) {
    if (e->n_aggr >= e->K || e->committed) return ctx->fail(HOBBIT_ESTATE, "elastic_open: more aggregate chunks than N/B");
    HB_TRY(e->form(e->aggr_form, hobbit_elastic_open::FULL, "elastic_open_aggregate_push"));
    HB_TRY(launch_axpy(ctx, e->d_aggr, cF(d_chunk), e->beta[e->n_aggr], e->B));                             // aggregated_vector[j] += beta1[i]*buff[j] (:330-333)
    e->n_aggr++;
    return 0;
}
// rows of a B-element vector (trs rows of B/trs) RS-encoded to twice their length
static int elastic_row_codes(hobbit_ctx *ctx, const F *d_v, size_t B, size_t trs, F *d_out) {
    const size_t half = B / trs; const int logc = ilog2_exact(2 * half);
    return fft::any_rows(ctx, d_v, half, half, d_out, logc, false, trs);
}
int hobbit_elastic_open_aggregate_finish(hobbit_ctx *ctx, hobbit_elastic_open *e) {
    if (e->n_aggr != e->K) return ctx->fail(HOBBIT_ESTATE, "elastic_open: aggregate pass incomplete");
    HB_TRY(hobbit_shockwave_commit(ctx, reinterpret_cast<hobbit_F *>(e->d_aggr.get()), e->B, 32, reinterpret_cast<hobbit_F *>(e->d_encf.get()), e->d_lvf));   // C_f (:343-346, :349)
    if (e->lin) {
        // aggregate()'s linear_time branch (:350-411): aggregated_tensor = the aggregate's rows RS-encoded; aux_commit = the expander codewords of
        // the queried columns that have a parity-row query; C_c = shockwave_commit(pad(aux_commit), 32)
        const uint32_t nr = (uint32_t)e->rem.size();
        if (ctx->code.n != e->trs) { long long l; HB_TRY(hobbit_graph_finalize(ctx, e->trs, &l)); }
        HB_TRY(elastic_row_codes(ctx, e->d_aggr, e->B, (size_t)e->trs, e->d_M));
        HB_TRY(launch_zero(ctx, e->d_aux, e->np * sizeof(F)));
        HB_TRY(launch_gather_cols(ctx, e->d_M, e->cols, (uint32_t)e->trs, e->d_rem, nr, e->d_aux, e->rows2));
        HB_TRY(launch_encode(ctx, e->d_aux, e->rows2, e->d_aux, e->rows2, e->trs, nr, 0));
        HB_TRY(hobbit_shockwave_commit(ctx, reinterpret_cast<hobbit_F *>(e->d_aux.get()), e->np, 32, reinterpret_cast<hobbit_F *>(e->d_encc.get()), e->d_lvc));
    }
    e->committed = true;
    return 0;
}
int hobbit_elastic_open_reply_push(hobbit_ctx *ctx, hobbit_elastic_open *e, const hobbit_F *d_chunk) {
    if (e->n_reply >= e->K) return ctx->fail(HOBBIT_ESTATE, "elastic_open: more reply chunks than N/B");
    HB_TRY(e->form(e->reply_form, hobbit_elastic_open::FULL, "elastic_open_reply_push"));
    const size_t i = e->n_reply, half = e->B / (size_t)e->trs; const uint32_t nc = (uint32_t)e->ucols.size();
    HB_TRY(launch_any_nonzero(ctx, cF(d_chunk), e->B, e->d_nz + i));                                       // an all-zero chunk appends nothing (:510-517)
    if (e->lin) {
        // update_reply_spielman (:431-485): rows RS-encoded, every distinct queried column expander-encoded into its row of d_G (the message half
        // is the column itself); d_pick holds, per reply slot, where the reference AS BUILT reads from (elastic_open_begin_lin)
        if (ctx->code.n != e->trs) { long long l; HB_TRY(hobbit_graph_finalize(ctx, e->trs, &l)); }
        HB_TRY(elastic_row_codes(ctx, cF(d_chunk), e->B, (size_t)e->trs, e->d_T));
        HB_TRY(launch_gather_cols(ctx, e->d_T, e->cols, (uint32_t)e->trs, e->d_ucols, nc, e->d_G, e->rows2));
        HB_TRY(launch_encode(ctx, e->d_G, e->rows2, e->d_G, e->rows2, e->trs, nc, 0));
        HB_TRY(launch_gather_strided(ctx, e->d_G, e->d_pick, (size_t)e->queries, 1, 1, 0, e->d_reply + i * (size_t)e->queries));
        e->n_reply++;
        return 0;
    }
    // update_reply (:59-111): rows to twice their length, then each queried column (trs entries, zero-padded) to 2*trs, its queried row kept
    HB_TRY(fft::rows(ctx, cF(d_chunk), half, (uint32_t)half, e->d_T, e->cols, 1, 12, false, 1, (uint32_t)e->trs, 0, 0));
    HB_TRY(launch_gather_cols(ctx, e->d_T, e->cols, (uint32_t)e->trs, e->d_ucols, nc, e->d_G, e->rows2));
    HB_TRY(fft::rows(ctx, e->d_G, e->rows2, (uint32_t)e->trs, e->d_G, e->rows2, 1, ilog2_exact(e->rows2), false, 1, nc, 0, 0));
    HB_TRY(launch_gather_strided(ctx, e->d_G, e->d_pick, (size_t)e->queries, 1, 1, 0, e->d_reply + i * (size_t)e->queries));
    e->n_reply++;
    return 0;
}
// The two passes on base-field chunks (include/hobbit_elastic_real.h).  Aggregate: F by F_p, 8 bytes read per coefficient.  Reply: the zero test on
// reals, the real row code into d_T as trs x (cols / 2 + 1) row-major, the conjugate-aware gather of the distinct queried columns -- before the
// column code a column c > cols / 2 is the entry-wise conjugate of column cols - c, whatever the column code is -- and from there the pass above.
int hobbit_elastic_open_aggregate_push_real(hobbit_ctx *ctx, hobbit_elastic_open *e, const uint64_t *d_chunk) {
    if (e->n_aggr >= e->K || e->committed) return ctx->fail(HOBBIT_ESTATE, "elastic_open: more aggregate chunks than N/B");
    if (!d_chunk) return ctx->fail(HOBBIT_EINVAL, "elastic_open_aggregate_push_real: null chunk");
    HB_TRY(e->form(e->aggr_form, hobbit_elastic_open::REAL, "elastic_open_aggregate_push_real"));
    HB_TRY(launch_axpy_real(ctx, e->d_aggr, d_chunk, e->beta[e->n_aggr], e->B));
    e->n_aggr++;
    return 0;
}
int hobbit_elastic_open_reply_push_real(hobbit_ctx *ctx, hobbit_elastic_open *e, const uint64_t *d_chunk) {
    if (e->n_reply >= e->K) return ctx->fail(HOBBIT_ESTATE, "elastic_open: more reply chunks than N/B");
    if (!d_chunk) return ctx->fail(HOBBIT_EINVAL, "elastic_open_reply_push_real: null chunk");
    const int logc = ilog2_exact(e->cols);
    if (logc < 3 || logc > 16) return ctx->fail(HOBBIT_EINVAL, "elastic_open_reply_push_real: the row code must have 2^3 .. 2^16 points");
    HB_TRY(e->form(e->reply_form, hobbit_elastic_open::REAL, "elastic_open_reply_push_real"));
    const size_t i = e->n_reply; const uint32_t nc = (uint32_t)e->ucols.size();
    HB_TRY(launch_any_nonzero_real(ctx, d_chunk, e->B, e->d_nz + i));
    if (e->lin && ctx->code.n != e->trs) { long long l; HB_TRY(hobbit_graph_finalize(ctx, e->trs, &l)); }
    HB_TRY(fft::real_rows_any(ctx, d_chunk, (size_t)e->trs, logc, e->d_T, false, 0));
    HB_TRY(launch_gather_cols_half(ctx, e->d_T, e->cols, (uint32_t)e->trs, e->d_ucols, nc, e->d_G, e->rows2));
    if (e->lin) HB_TRY(launch_encode(ctx, e->d_G, e->rows2, e->d_G, e->rows2, e->trs, nc, 0));
    else HB_TRY(fft::rows(ctx, e->d_G, e->rows2, (uint32_t)e->trs, e->d_G, e->rows2, 1, ilog2_exact(e->rows2), false, 1, nc, 0, 0));
    HB_TRY(launch_gather_strided(ctx, e->d_G, e->d_pick, (size_t)e->queries, 1, 1, 0, e->d_reply + i * (size_t)e->queries));
    e->n_reply++;
    return 0;
}
int hobbit_elastic_open_finish(hobbit_ctx *ctx, hobbit_elastic_open *e, const uint8_t *d_commit_levels, hobbit_elastic_open_out *o) {
    if (!o || !e->committed || e->n_reply != e->K) return ctx->fail(HOBBIT_ESTATE, "elastic_open_finish: the aggregate and reply passes must be complete");
    const size_t B = e->B, trs = (size_t)e->trs, cols = e->cols, nq = (size_t)e->queries, nc = e->ucols.size();
    if (o->cols) memcpy(o->cols, e->qc.data(), 4 * nq);
    if (o->rows) memcpy(o->rows, e->qr.data(), 4 * nq);
    if (o->rv0) *mF(o->rv0) = e->rv0;
    if (o->ncols) *o->ncols = (int)nc;
    if (o->cf_root) HB_CHECK(ctx, hipMemcpyAsync(o->cf_root, e->d_lvf + 32 * (2 * (2 * B / 32) - 2), 32, hipMemcpyDeviceToHost, ctx->stream));
    {   // replies: one entry per non-zero chunk, in stream order
        std::vector<int> nz(e->K); std::vector<F> rep(e->K * nq);
        HB_CHECK(ctx, hipMemcpyAsync(nz.data(), e->d_nz, e->K * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HB_CHECK(ctx, hipMemcpyAsync(rep.data(), e->d_reply, e->K * nq * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
        HB_TRY(ctx->sync());
        size_t filled = 0;
        for (size_t i = 0; i < e->K; i++) if (nz[i]) filled++;
        if (o->reply) { size_t f = 0; for (size_t i = 0; i < e->K; i++) if (nz[i]) { for (size_t q = 0; q < nq; q++) mF(o->reply)[q * filled + f] = rep[i * nq + q]; f++; } }
        if (o->reply_len) *o->reply_len = (int)filled;
    }
    if (o->paths && d_commit_levels) {                                                                      // open_tree_blake(Commitment_MT, I[i], 2B/trs) (:684-687)
        std::vector<uint64_t> pos(nq);
        for (size_t q = 0; q < nq; q++) pos[q] = (uint64_t)(e->qr[q] / 4) * cols + e->qc[q];
        HB_TRY(paths_common(ctx, d_commit_levels, 4 * B, pos.data(), nq, o->paths));
    }
    if (e->lin) return spielman_stream_dev(ctx, e, o);
    return rs_prover_dev(ctx, e->d_aggr, B, trs, e->qc, e->qr, e->ucols, e->d_ucols, e->d_encf, e->d_lvf, o);
}

// ---- Our_PC open_standard with linear_time == false (test_PC option 1; the circuit polynomial of prove_circuit_standard): src/Our_PC.cpp:604-692 ----
// r_v[0], _aggregate (aggregate + C_f, no C_c: :258-276), `queries` (790 in the reference) draws, replies out of the retained tensor, paths,
// recursive_prover_RS.  Output layout: hobbit_elastic_open_out (reply: queries x K).
// d_real: the polynomial as N reals of 8 bytes (hobbit_open_standard_rs_real), read by the aggregate alone; otherwise d_poly
static int open_rs_impl(hobbit_ctx *ctx, const hobbit_F *d_poly, const uint64_t *d_real, size_t N, const hobbit_commitment *c, const hobbit_F *h_x, int queries,
                        hobbit_elastic_open_out *o) {
    if (!c || !o || !h_x || queries <= 0 || (!d_poly && !d_real)) return ctx->fail(HOBBIT_EINVAL, "open_standard_rs: bad arguments");
    if (c->lin) return ctx->fail(HOBBIT_EINVAL, "open_standard_rs: the commitment is RS x expander (use hobbit_open_standard)");
    const int K = c->K; const size_t B = c->M, trs = (size_t)c->trs, cols = c->cols, rows2 = c->rows2, nq = (size_t)queries;
    const int logK = ilog2_exact((size_t)K);
    if (N != c->N || logK < 0) return ctx->fail(HOBBIT_EINVAL, "open_standard_rs: polynomial / commitment mismatch");
    std::vector<F> beta; host_eq_table(cF(h_x), logK, beta);                                                // precompute_beta(x1, beta) (:619-621)
    const F rv0 = fadd(fmake((uint64_t)random()), fmake((uint64_t)rand()));                                 // r_v[0] = generate_randomness(1)[0] (:623)
    mem::Pooled<F> d_aggr, d_encf; mem::Pooled<uint8_t> d_lvf; mem::Pooled<uint32_t> d_ucols;
    if (ctx->pool_get(B * sizeof(F), d_aggr) || ctx->pool_get(2 * B * sizeof(F), d_encf) || ctx->pool_get(64 * (2 * B / 32), d_lvf) || ctx->pool_get(nq * 4, d_ucols))
        return ctx->fail(HOBBIT_ENOMEM, "open_standard_rs: allocation failed");
    {
        if (d_real) HB_TRY(launch_aggregate_real(ctx, d_real, B, K, beta.data(), d_aggr));
        else HB_TRY(launch_aggregate(ctx, cF(d_poly), B, K, beta.data(), d_aggr));                          // _aggregate (:267-272)
        HB_TRY(hobbit_shockwave_commit(ctx, reinterpret_cast<hobbit_F *>(d_aggr.get()), B, 32, reinterpret_cast<hobbit_F *>(d_encf.get()), d_lvf));   // C_f (:274-275)
        std::vector<uint32_t> qc(nq), qr(nq);
        for (size_t q = 0; q < nq; q++) { qc[q] = (uint32_t)(rand() % (long)cols); qr[q] = (uint32_t)(rand() % (long)rows2); }      // (:634-638)
        std::vector<uint32_t> ucols(qc); std::sort(ucols.begin(), ucols.end()); ucols.erase(std::unique(ucols.begin(), ucols.end()), ucols.end());
        HB_TRY(hobbit_memcpy_h2d(ctx, d_ucols, ucols.data(), ucols.size() * 4));
        if (o->cols) memcpy(o->cols, qc.data(), 4 * nq);
        if (o->rows) memcpy(o->rows, qr.data(), 4 * nq);
        if (o->rv0) *mF(o->rv0) = rv0;
        if (o->ncols) *o->ncols = (int)ucols.size();
        if (o->cf_root) HB_TRY(hobbit_memcpy_d2h(ctx, o->cf_root, d_lvf + 32 * (2 * (2 * B / 32) - 2), 32));
        if (o->reply) HB_TRY(hobbit_commitment_gather(ctx, c, qr.data(), qc.data(), nq, o->reply));         // _compute_aggregation_reply (:291-305)
        if (o->reply_len) *o->reply_len = K;
        if (o->paths) HB_TRY(hobbit_commitment_paths(ctx, c, qc.data(), qr.data(), nq, o->paths));          // open_tree_blake(Commitment_MT, I[i], 2B/trs) (:643-645)
        return rs_prover_dev(ctx, d_aggr, B, trs, qc, qr, ucols, d_ucols, d_encf, d_lvf, o);                // (:651-653)
    }
}
int hobbit_open_standard_rs(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_commitment *c, const hobbit_F *h_x, int queries, hobbit_elastic_open_out *o) {
    if (!d_poly) return ctx->fail(HOBBIT_EINVAL, "open_standard_rs: bad arguments");
    return open_rs_impl(ctx, d_poly, nullptr, N, c, h_x, queries, o);
}
int hobbit_open_standard_rs_real(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, const hobbit_commitment *c, const hobbit_F *h_x, int queries, hobbit_elastic_open_out *o) {
    if (!d_poly) return ctx->fail(HOBBIT_EINVAL, "open_standard_rs_real: null polynomial");
    return open_rs_impl(ctx, nullptr, d_poly, N, c, h_x, queries, o);
}

// ---- streaming (space-efficient) provers over a caller-supplied chunk source -------------------------------------------------
struct StreamSrc { hobbit_chunk_source fn; void *user; };
static int src_next(hobbit_ctx *ctx, const StreamSrc &s, size_t n, const F **d) {
    const hobbit_F *p = nullptr;
    if (!s.fn || s.fn(s.user, n, &p) != 0 || (n && !p)) return ctx->fail(HOBBIT_EINVAL, "chunk source failed");
    *d = cF(p); return 0;
}
static int src_reset(hobbit_ctx *ctx, const StreamSrc &s) { const F *d; return src_next(ctx, s, 0, &d); }   // reset_stream (src/witness_stream.cpp:228-234)
// evaluate_vector (src/utils.cpp:789-802) on a handful of host values
static F host_eval_vector(std::vector<F> v, CHP r, int k) {
    for (int i = 0; i < k; i++) { size_t L = v.size() / 2; for (size_t j = 0; j < L; j++) v[j] = fadd(v[2 * j], fmul(r[i], fsub(v[2 * j + 1], v[2 * j]))); v.resize(L); }
    return v[0];
}
// read_mul_tree_layer (src/witness_stream.cpp:2413-2456, every stream but "wiring_consistency_check"): d_out[0..size) = products of
// 2^layer consecutive elements; one read of 2*size elements fills size/2^layer entries of each half.  layer >= 1.
static int dev_read_mul_tree_layer(hobbit_ctx *ctx, const StreamSrc &src, size_t size, int layer, F *d_out) {
    if (layer < 1 || ((size_t)1 << layer) > size) return ctx->fail(HOBBIT_EINVAL, "read_mul_tree_layer: needs 1 <= layer <= log2(size) (the reference indexes past its vector for layer 0)");
    const uint32_t seg = 1u << layer; const size_t per = size / seg;
    for (size_t counter = 0; counter < size / 2; counter += per) {
        const F *ch; HB_TRY(src_next(ctx, src, 2 * size, &ch));
        HB_TRY(launch_seg_prod(ctx, ch, seg, per, d_out + counter));
        HB_TRY(launch_seg_prod(ctx, ch + size, seg, per, d_out + counter + size / 2));
    }
    return 0;
}
// read_mul_tree_data (:2458-2510): V[0] = `size` products of 2^layer consecutive elements (lower half from the first half of every read,
// upper half from its second half), V[i] = products of 2^distance consecutive entries of V[i-1]
static int dev_read_mul_tree_data(hobbit_ctx *ctx, const StreamSrc &src, F *const *V, const size_t *vlen, int batches, size_t size, int layer, int distance) {
    const uint32_t seg = 1u << layer; const size_t per = size / (2 * (size_t)seg);
    if (!per) return ctx->fail(HOBBIT_EINVAL, "read_mul_tree_data: 2^layer too large for the read size");
    for (size_t counter = 0; counter < size / 2; counter += per) {
        const F *ch; HB_TRY(src_next(ctx, src, size, &ch));
        HB_TRY(launch_seg_prod(ctx, ch, seg, per, V[0] + counter));
        HB_TRY(launch_seg_prod(ctx, ch + size / 2, seg, per, V[0] + counter + size / 2));
    }
    for (int i = 1; i < batches; i++) HB_TRY(launch_seg_prod(ctx, V[i - 1], 1u << distance, vlen[i], V[i]));
    return 0;
}
int hobbit_read_mul_tree_layer(hobbit_ctx *ctx, hobbit_chunk_source source, void *user, size_t size, int layer, hobbit_F *d_out) {
    StreamSrc src{source, user};
    HB_TRY(src_reset(ctx, src));
    return dev_read_mul_tree_layer(ctx, src, size, layer, mF(d_out));
}
int hobbit_read_mul_tree_data(hobbit_ctx *ctx, hobbit_chunk_source source, void *user, size_t size, int layer, int distance, int batches, hobbit_F *d_out) {
    if (batches < 1 || batches > 16 || distance < 0) return ctx->fail(HOBBIT_EINVAL, "read_mul_tree_data: 1 <= batches <= 16");
    StreamSrc src{source, user};
    F *V[16]; size_t vlen[16]; size_t o = 0;
    for (int i = 0; i < batches; i++) { V[i] = mF(d_out) + o; vlen[i] = size >> (i * distance); o += vlen[i]; }
    HB_TRY(src_reset(ctx, src));
    return dev_read_mul_tree_data(ctx, src, V, vlen, batches, size, layer, distance);
}
// shared set-up of generate_claims_opt / the streaming 3-product sumcheck: per batch the table sizes and the eq table over the chunk index (host)
struct StreamPlan {
    int batches, logB; size_t size, nch, tot, vtot;
    size_t sz[16], off[16], vlen[16], voff[16]; int n_init[16]; std::vector<F> rb[16];
};
static int stream_plan(hobbit_ctx *ctx, StreamPlan &P, size_t fd_size, size_t B, CHP h_r, int rlen, int rstride, int batches, int distance, int layer_id) {
    if (batches < 1 || batches > 16 || distance < 1 || layer_id < 0) return ctx->fail(HOBBIT_EINVAL, "streaming sumcheck: bad batches / distance / layer");
    P.batches = batches; P.size = fd_size >> layer_id; P.logB = ilog2_exact(B);
    if (P.logB < 1 || ilog2_exact(P.size) < 0 || P.size < 4 * B) return ctx->fail(HOBBIT_EINVAL, "streaming sumcheck: needs power-of-two sizes with size >= 4*BUFFER_SPACE");
    P.nch = P.size / (4 * B); P.tot = P.vtot = 0;
    const int lhalf = ilog2_exact(P.size / 2);
    for (int i = 0; i < batches; i++) {
        const int n_init = P.logB - i * distance, n_rem = lhalf - i * distance - n_init;
        if (n_init < 1 || n_rem < 1 || n_init + n_rem > rlen) return ctx->fail(HOBBIT_EINVAL, "streaming sumcheck: challenge vector too short for this batch");
        P.n_init[i] = n_init;
        P.sz[i] = B >> (i * distance); P.vlen[i] = (4 * B) >> (i * distance); P.off[i] = P.tot; P.voff[i] = P.vtot; P.tot += P.sz[i]; P.vtot += P.vlen[i];
        host_eq_table(h_r + (size_t)i * rstride + n_init, n_rem, P.rb[i]);
    }
    return 0;
}
// generate_claims_opt (src/sumcheck.cpp:1014-1054): one challenge vector r for every batch
int hobbit_generate_claims_opt(hobbit_ctx *ctx, hobbit_chunk_source source, void *user, size_t fd_size, size_t B, const hobbit_F *h_r, int rlen, int batches, int layer_id,
                               int distance, hobbit_F *h_claims) {
    StreamSrc src{source, user}; StreamPlan P;
    HB_TRY(stream_plan(ctx, P, fd_size, B, cF(h_r), rlen, 0, batches, distance, layer_id));
    const size_t nres = 2 * P.nch * (size_t)batches;
    F *base; HB_TRY(ctx->workspace4((2 * P.vtot + P.tot + 1024 + nres + 64) * sizeof(F), (void **)&base));
    F *Vb = base, *EO = Vb + P.vtot, *beta = EO + P.vtot, *part = beta + P.tot, *dres = part + 1024;
    F *V[16]; for (int i = 0; i < batches; i++) V[i] = Vb + P.voff[i];
    for (int i = 0; i < batches; i++) HB_TRY(hobbit_eq_table(ctx, h_r, P.n_init[i], reinterpret_cast<hobbit_F *>(beta + P.off[i])));
    HB_TRY(src_reset(ctx, src));
    for (size_t c = 0; c < P.nch; c++) {
        HB_TRY(dev_read_mul_tree_data(ctx, src, V, P.vlen, batches, 4 * B, layer_id, distance));
        for (int j = 0; j < batches; j++) {
            F *E = EO + P.voff[j], *O = E + 2 * P.sz[j];                         // evens | odds, each 2*sz: [first half | second half]
            HB_TRY(launch_deinterleave(ctx, V[j], 2 * P.sz[j], E, O));
            HB_TRY(launch_dot_gen(ctx, beta + P.off[j], E, 1, O, P.sz[j], part, dres + (2 * c) * batches + j));
            HB_TRY(launch_dot_gen(ctx, beta + P.off[j], E + P.sz[j], 1, O + P.sz[j], P.sz[j], part, dres + (2 * c + 1) * batches + j));
        }
    }
    std::vector<F> res(nres);
    HB_TRY(hobbit_memcpy_d2h(ctx, res.data(), dres, nres * sizeof(F)));
    for (int j = 0; j < batches; j++) {
        F cl = fmake(0); const size_t hb = P.rb[j].size() / 2;
        for (size_t c = 0; c < P.nch; c++) { cl = fadd(cl, fmul(P.rb[j][c], res[(2 * c) * batches + j])); cl = fadd(cl, fmul(P.rb[j][c + hb], res[(2 * c + 1) * batches + j])); }
        mF(h_claims)[j] = cl;
    }
    return src_reset(ctx, src);
}
// generate_3product_sumcheck_beta_stream_batch_optimized (src/sumcheck.cpp:1150-1393)
int hobbit_sumcheck3_stream_batch(hobbit_ctx *ctx, hobbit_chunk_source source, void *user, size_t fd_size, size_t B, const hobbit_F *h_r, int rlen, int batches, int distance,
                                  int layer_id, const hobbit_F *h_old_claims, int n_old, hobbit_stream3_out *o) {
    if (!o || n_old > batches) return ctx->fail(HOBBIT_EINVAL, "sumcheck3_stream_batch: bad arguments");
    StreamSrc src{source, user}; StreamPlan P;
    HB_TRY(stream_plan(ctx, P, fd_size, B, cF(h_r), rlen, rlen, batches, distance, layer_id));
    const size_t nR = 2 * P.nch, half = P.rb[0].size() / 2, npe = 2 * (size_t)batches * nR;
    // device tables: V | evens/odds scratch | fold1,2,3 | buff1,2,3 (each `tot`, batch j at off[j]) | partials | results
    F *base; HB_TRY(ctx->workspace4((2 * P.vtot + 6 * P.tot + 1024 + npe + 2 * nR + 64) * sizeof(F), (void **)&base));
    F *Vb = base, *EO = Vb + P.vtot, *f1 = EO + P.vtot, *f2 = f1 + P.tot, *f3 = f2 + P.tot, *b1 = f3 + P.tot, *b2 = b1 + P.tot, *b3 = b2 + P.tot, *part = b3 + P.tot,
      *dres = part + 1024, *dR = dres + npe + 16;
    F *V[16]; for (int i = 0; i < batches; i++) V[i] = Vb + P.voff[i];
    for (int i = 0; i < batches; i++) HB_TRY(hobbit_eq_table(ctx, h_r + (size_t)i * rlen, P.n_init[i], reinterpret_cast<hobbit_F *>(b3 + P.off[i])));   // buff3 = beta(initial_r) (:1171)
    HB_TRY(launch_copy(ctx, f3, b3, P.tot * sizeof(F)));                                                       // fold_buff3 = buff3
    HB_TRY(src_reset(ctx, src));
    HB_TRY(dev_read_mul_tree_data(ctx, src, V, P.vlen, batches, 4 * B, layer_id, distance));                                                              // (:1187)
    std::vector<F> Kp(batches), a(batches);
    for (int i = 0; i < batches; i++) {                                              // fold_buff1/2 = the first half's pairs; K_partial = sum f1 f2 f3 (:1194-1202)
        HB_TRY(launch_deinterleave(ctx, V[i], P.sz[i], f1 + P.off[i], f2 + P.off[i]));
        HB_TRY(launch_dot_gen(ctx, f1 + P.off[i], f2 + P.off[i], 1, f3 + P.off[i], P.sz[i], part, dres + i));
    }
    HB_TRY(hobbit_memcpy_d2h(ctx, Kp.data(), dres, (size_t)batches * sizeof(F)));
    { F cst = fmake(0); for (int i = 0; i < batches; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); a[i] = fadd(cst, fmake((uint64_t)rand())); } }          // a = generate_randomness(batches)
    F Kf = fmake(0);
    std::vector<F> R; R.push_back(fmake(1));
    for (int i = 0; i < batches; i++) { Kf = fadd(Kf, fmul(a[i], Kp[i])); Kp[i] = fmul(Kp[i], P.rb[i][0]); }
    auto load_half = [&](int second) -> int {
        for (int j = 0; j < batches; j++) HB_TRY(launch_deinterleave(ctx, V[j] + (second ? 2 * P.sz[j] : 0), P.sz[j], b1 + P.off[j], b2 + P.off[j]));
        return 0;
    };
    auto batch_prod_step = [&](size_t idx) -> int {                                   // batch_prod (:1093-1136)
        F K1 = fmake(0), K2 = fmake(0); std::vector<F> K3(batches);
        for (int j = 0; j < batches; j++) {
            const size_t q = P.off[j];
            const F *t[8] = {b1 + q, b2 + q, b3 + q, f1 + q, f2 + q, f3 + q, nullptr, nullptr}; F k[4];
            HB_TRY(launch_err_terms(ctx, 13, t, nullptr, P.sz[j], k));
            K1 = fadd(K1, fmul(a[j], k[0])); K2 = fadd(K2, fmul(a[j], k[1])); K3[j] = k[2];
        }
        F rnd = mimc_hash(K1, R.back()); rnd = mimc_hash(K2, rnd);
        for (int j = 0; j < batches; j++) rnd = mimc_hash(K3[j], rnd);
        const F x1 = rnd, x2 = fmul(rnd, x1), x3 = fmul(rnd, x2);
        for (int j = 0; j < batches; j++) { Kp[j] = fadd(Kp[j], fmul(P.rb[j][idx], K3[j])); Kf = fadd(Kf, fmul(fmul(x3, a[j]), K3[j])); }
        Kf = fadd(Kf, fadd(fmul(x2, K2), fmul(x1, K1)));
        R.push_back(rnd);
        HB_TRY(launch_axpy(ctx, f1, b1, rnd, P.tot)); HB_TRY(launch_axpy(ctx, f2, b2, rnd, P.tot));
        return launch_axpy(ctx, f3, b3, rnd, P.tot);
    };
    HB_TRY(load_half(1)); HB_TRY(batch_prod_step(half));                              // (:1216-1222)
    for (size_t i = 1; i < P.nch; i++) {                                              // (:1223-1241)
        HB_TRY(dev_read_mul_tree_data(ctx, src, V, P.vlen, batches, 4 * B, layer_id, distance));
        HB_TRY(load_half(0)); HB_TRY(batch_prod_step(i));
        HB_TRY(load_half(1)); HB_TRY(batch_prod_step(i + half));
    }
    HB_TRY(src_reset(ctx, src));
    o->checks[0] = 1;
    for (int i = 0; i < n_old; i++) if (!feq(Kp[i], cF(h_old_claims)[i])) o->checks[0] = 0;                                                              // "Error in sumcheck 0" (printed only, :1246-1251)
    // P1 = batch_3product_sumcheck(fold_buff1, fold_buff2, fold_buff3, a) (:1264); "Error in sumcheck 1" (:1280-1283)
    std::vector<size_t> lens(batches); for (int i = 0; i < batches; i++) lens[i] = P.sz[i];
    HB_TRY(hobbit_batch_3product_sumcheck(ctx, reinterpret_cast<hobbit_F *>(f1), reinterpret_cast<hobbit_F *>(f2), reinterpret_cast<hobbit_F *>(f3), lens.data(), batches,
                                          reinterpret_cast<hobbit_F *>(a.data()), o->cpoly1, o->r1, o->vr1));
    { CHP q0 = cF(o->cpoly1); o->checks[1] = feq(fadd(fadd(fadd(q0[0], q0[1]), fadd(q0[2], q0[3])), q0[3]), Kf); }
    // Partial_Evals pass (:1303-1340): beta[k] over P1's first log2(sizes[k]) challenges
    for (int k = 0; k < batches; k++) HB_TRY(hobbit_eq_table(ctx, o->r1, ilog2_exact(P.sz[k]), reinterpret_cast<hobbit_F *>(b3 + P.off[k])));
    for (size_t i = 0; i < P.nch; i++) {
        HB_TRY(dev_read_mul_tree_data(ctx, src, V, P.vlen, batches, 4 * B, layer_id, distance));
        for (int k = 0; k < batches; k++) {
            const F *bt = b3 + P.off[k]; const size_t n = P.sz[k], h2 = P.vlen[k] / 2;
            F *p0 = dres + (size_t)(2 * k) * nR, *p1 = dres + (size_t)(2 * k + 1) * nR;
            HB_TRY(launch_dot_gen(ctx, bt, V[k], 2, nullptr, n, part, p0 + i));
            HB_TRY(launch_dot_gen(ctx, bt, V[k] + h2, 2, nullptr, n, part, p0 + i + nR / 2));
            HB_TRY(launch_dot_gen(ctx, bt, V[k] + 1, 2, nullptr, n, part, p1 + i));
            HB_TRY(launch_dot_gen(ctx, bt, V[k] + 1 + h2, 2, nullptr, n, part, p1 + i + nR / 2));
        }
    }
    HB_TRY(src_reset(ctx, src));
    std::vector<F> PE(npe);
    HB_TRY(hobbit_memcpy_d2h(ctx, PE.data(), dres, npe * sizeof(F)));
    std::vector<F> Rp(nR);                                                              // permute_partial_evals (:1137-1148): only R moves
    for (size_t i = 0; i < nR / 2; i++) { Rp[i] = R[2 * i]; Rp[nR / 2 + i] = R[2 * i + 1]; }
    if (o->R) memcpy(o->R, Rp.data(), nR * sizeof(F));
    std::vector<F> bb(2 * (size_t)batches), ae(nR, fmake(0));
    { F cst = fmake(0); for (size_t i = 0; i < bb.size(); i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); bb[i] = fadd(cst, fmake((uint64_t)rand())); } }   // b = generate_randomness(2*batches)
    for (size_t i = 0; i < bb.size(); i++) for (size_t j = 0; j < nR; j++) ae[j] = fadd(ae[j], fmul(bb[i], PE[i * nR + j]));
    HB_TRY(hobbit_memcpy_h2d(ctx, dR, Rp.data(), nR * sizeof(F)));
    HB_TRY(hobbit_memcpy_h2d(ctx, dR + nR, ae.data(), nR * sizeof(F)));
    hobbit_F zero = {0, 0};                                                             // previous_r = the local `rand`, never updated: F(0) (:1207, 1351)
    HB_TRY(hobbit_sumcheck2(ctx, reinterpret_cast<hobbit_F *>(dR), reinterpret_cast<hobbit_F *>(dR + nR), nR, &zero, o->qpoly2, o->r2, o->vr2, o->fin2));
    {   // "Error in sumcheck 2" (:1356-1365)
        F sum = fmake(0); CHP vr1 = cF(o->vr1), q2 = cF(o->qpoly2);
        for (int i = 0; i < batches; i++) { sum = fadd(sum, fmul(bb[2 * i], vr1[3 * i])); sum = fadd(sum, fmul(bb[2 * i + 1], vr1[3 * i + 1])); }
        o->checks[2] = feq(fadd(fadd(q2[0], q2[1]), fadd(q2[2], q2[2])), sum);
    }
    const int lR = ilog2_exact(nR);
    const F pad = fmake((uint64_t)random());                                            // (:1368)
    for (int i = 0; i < batches; i++) {
        MHP row = mF(o->new_r) + (size_t)i * o->new_r_ld; int n = 0;
        if (1 + P.n_init[i] + lR > o->new_r_ld) return ctx->fail(HOBBIT_EINVAL, "sumcheck3_stream_batch: new_r_ld too small");
        row[n++] = pad;
        for (int j = 0; j < P.n_init[i]; j++) row[n++] = cF(o->r1)[j];
        for (int j = 0; j < lR; j++) row[n++] = cF(o->r2)[j];
        const F e0 = host_eval_vector(std::vector<F>(PE.begin() + (size_t)(2 * i) * nR, PE.begin() + (size_t)(2 * i + 1) * nR), cF(o->r2), lR);
        const F e1 = host_eval_vector(std::vector<F>(PE.begin() + (size_t)(2 * i + 1) * nR, PE.begin() + (size_t)(2 * i + 2) * nR), cF(o->r2), lR);
        mF(o->new_claims)[i] = fadd(fmul(fsub(fmake(1), pad), e0), fmul(pad, e1));      // (:1383-1386)
    }
    return 0;
}
// prove_multiplication_tree_stream_shallow (src/sumcheck.cpp:1746-1915) without commit_layers / open_layers
int hobbit_mul_tree_stream_shallow(hobbit_ctx *ctx, hobbit_chunk_source source, void *user, size_t fd_size, size_t B, int vectors, size_t size, const hobbit_F *h_previous_r,
                                   int distance, const hobbit_F *h_prev_x, int naive, hobbit_mul_stream_out *o) {
    if (!o || vectors < 1 || distance < 1 || ilog2_exact((size_t)vectors) < 0 || ilog2_exact(size) < 0) return ctx->fail(HOBBIT_EINVAL, "mul_tree_stream_shallow: vectors and size must be powers of two");
    StreamSrc src{source, user};
    const size_t total = size * (size_t)vectors;
    if (o->n_steps) *o->n_steps = 0;
    if (total <= 2 * B) {                                                               // in memory (:1755-1774)
        HB_TRY(src_reset(ctx, src));
        const F *ch; HB_TRY(src_next(ctx, src, total, &ch));
        return mul_tree_impl(ctx, reinterpret_cast<const hobbit_F *>(ch), (size_t)vectors, size, h_previous_r, h_prev_x, o->cpoly, o->r, o->vr, o->fin, o->final_r, o->out_eval,
                             o->final_eval, o->layers, o->output);
    }
    int layers = ilog2_exact(total / (2 * B));
    if (layers < 0) return ctx->fail(HOBBIT_EINVAL, "mul_tree_stream_shallow: size*vectors/(2*BUFFER_SPACE) must be a power of two");
    if (layers % distance != 0 && layers > distance) layers = distance + layers - (layers % distance);       // (:1779-1793)
    if (o->stream_layers) *o->stream_layers = layers;
    const size_t n1 = fd_size >> layers;
    if (n1 < (size_t)vectors * 2) return ctx->fail(HOBBIT_EINVAL, "mul_tree_stream_shallow: product layer smaller than the vector count");
    F *buff1; HB_TRY(ctx->workspace4(n1 * sizeof(F), (void **)&buff1));
    HB_TRY(src_reset(ctx, src));
    HB_TRY(dev_read_mul_tree_layer(ctx, src, n1, layers, buff1));                       // (:1805-1810)
    HB_TRY(mul_tree_impl(ctx, reinterpret_cast<hobbit_F *>(buff1), (size_t)vectors, n1 / (size_t)vectors, h_previous_r, h_prev_x, o->cpoly, o->r, o->vr, o->fin, o->final_r,
                         o->out_eval, o->final_eval, o->layers, o->output));
    HB_TRY(src_reset(ctx, src));
    if (layers == 0) return 0;
    const int lt = ilog2_exact(n1);
    std::vector<hobbit_F> claims(16), nclaims(16);
    int steps = 0;
    auto run_step = [&](const hobbit_F *r, int rlen, int batches, int dist, int layer_id, int n_old) -> int {
        if (steps >= o->max_steps) return ctx->fail(HOBBIT_EINVAL, "mul_tree_stream_shallow: more streaming sumchecks than max_steps");
        hobbit_stream3_out *st = &o->steps[steps];
        HB_TRY(hobbit_sumcheck3_stream_batch(ctx, source, user, fd_size, B, r, rlen, batches, dist, layer_id, claims.data(), n_old, st));
        for (int i = 0; i < batches; i++) claims[i] = st->new_claims[i];
        steps++; if (o->n_steps) *o->n_steps = steps;
        return 0;
    };
    if (layers <= distance || naive) {                                                  // (:1849-1865)
        claims[0] = *o->final_eval;
        std::vector<hobbit_F> cur(o->final_r, o->final_r + lt);
        for (int i = layers - 1; i >= 0; i--) {
            HB_TRY(run_step(cur.data(), (int)cur.size(), 1, 1, i, 1));
            const hobbit_stream3_out *st = &o->steps[steps - 1];
            const int n = 1 + ilog2_exact(B) + ilog2_exact((fd_size >> i) / (2 * B));
            cur.assign(st->new_r, st->new_r + n);
        }
    } else {                                                                            // (:1866-1908)
        const int batches = layers / distance;
        const int want = ilog2_exact(total >> distance);
        std::vector<hobbit_F> r_temp(o->final_r, o->final_r + lt);
        { F cst = fmake(0); for (int i = 0; i < want - lt; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); F v = fadd(cst, fmake((uint64_t)rand())); r_temp.push_back(*reinterpret_cast<hobbit_F *>(&v)); } }
        HB_TRY(hobbit_generate_claims_opt(ctx, source, user, fd_size, B, r_temp.data(), (int)r_temp.size(), batches, distance - 1, distance, claims.data()));
        if (o->claims0) memcpy(o->claims0, claims.data(), sizeof(hobbit_F) * (size_t)batches);
        int ld = (int)r_temp.size();
        std::vector<hobbit_F> cur((size_t)batches * ld);
        for (int b = 0; b < batches; b++) memcpy(cur.data() + (size_t)b * ld, r_temp.data(), sizeof(hobbit_F) * (size_t)ld);
        for (int i = distance - 1; i >= 0; i--) {
            HB_TRY(run_step(cur.data(), ld, batches, distance, i, batches));
            const hobbit_stream3_out *st = &o->steps[steps - 1];
            ld = st->new_r_ld;
            cur.assign(st->new_r, st->new_r + (size_t)batches * ld);
        }
    }
    return 0;
}
// prove_gate_consistency (src/sumcheck.cpp:796-975) over a caller-supplied trace source (read_trace belongs to the witness generator)
int hobbit_gate_consistency_stream(hobbit_ctx *ctx, hobbit_trace_source source, void *user, size_t n_chunks, size_t B, const hobbit_F *h_r, hobbit_gate_stream_out *o) {
    const int logB = ilog2_exact(B), lR = ilog2_exact(n_chunks);
    if (!o || !source || logB < 1 || lR < 1) return ctx->fail(HOBBIT_EINVAL, "gate_consistency_stream: BUFFER_SPACE and the chunk count must be powers of two, chunks >= 2");
    auto next = [&](size_t n, const F **L, const F **R, const F **O, const int32_t **S) -> int {
        const hobbit_F *l = nullptr, *r = nullptr, *oo = nullptr; const int32_t *s = nullptr;
        if (source(user, n, &l, &r, &oo, &s) != 0 || (n && (!l || !r || !oo || !s))) return ctx->fail(HOBBIT_EINVAL, "trace source failed");
        *L = cF(l); *R = cF(r); *O = cF(oo); *S = s; return 0;
    };
    const F *bL, *bR, *bO; const int32_t *bS;
    F *base; HB_TRY(ctx->workspace4((8 * B + 1024 + 6 * n_chunks + 2 * n_chunks + 64) * sizeof(F), (void **)&base));
    F *beta = base, *fb = beta + B, *fL = fb + B, *fR = fL + B, *fO = fR + B, *fa = fO + B, *fm = fa + B, *tmp = fm + B, *part = tmp + B, *dres = part + 1024, *dR = dres + 6 * n_chunks + 16;
    HB_TRY(hobbit_eq_table(ctx, h_r, logB, reinterpret_cast<hobbit_F *>(beta)));
    HB_TRY(launch_copy(ctx, fb, beta, B * sizeof(F)));
    HB_TRY(next(0, &bL, &bR, &bO, &bS));
    HB_TRY(next(B, &bL, &bR, &bO, &bS));
    HB_TRY(launch_copy(ctx, fL, bL, B * sizeof(F)));
    HB_TRY(launch_copy(ctx, fR, bR, B * sizeof(F)));
    HB_TRY(launch_copy(ctx, fO, bO, B * sizeof(F)));
    HB_TRY(launch_i32_to_F(ctx, bS, 0, B, fa)); HB_TRY(launch_i32_to_F(ctx, bS, 1, B, fm));
    // Kf_O, Kf_L, Kf_R, Kf_M (:818-826)
    HB_TRY(launch_dot_gen(ctx, beta, fO, 1, nullptr, B, part, dres));
    HB_TRY(launch_dot_gen(ctx, beta, fL, 1, fa, B, part, dres + 1));
    HB_TRY(launch_dot_gen(ctx, beta, fR, 1, fa, B, part, dres + 2));
    HB_TRY(launch_f_binop(ctx, 2, fR, fL, tmp, B));
    HB_TRY(launch_dot_gen(ctx, beta, tmp, 1, fm, B, part, dres + 3));
    F K0[4]; HB_TRY(hobbit_memcpy_d2h(ctx, K0, dres, 4 * sizeof(F)));
    F KO = K0[0], KL = K0[1], KR = K0[2], KM = K0[3], rnd = fmake(0);
    std::vector<F> R; R.push_back(fmake(1));
    o->checks[0] = 1;
    for (size_t c = 1; c < n_chunks; c++) {
        HB_TRY(next(B, &bL, &bR, &bO, &bS));
        F k2[4], kl[4], kr[4], k4[4];
        { const F *t[8] = {bO, beta, fO, fb, nullptr, nullptr, nullptr, nullptr}; HB_TRY(launch_err_terms(ctx, 2, t, nullptr, B, k2)); }
        { const F *t[8] = {bL, fL, fa, fb, beta, nullptr, nullptr, nullptr}; HB_TRY(launch_err_terms(ctx, 3, t, bS, B, kl)); }
        { const F *t[8] = {bR, fR, fa, fb, beta, nullptr, nullptr, nullptr}; HB_TRY(launch_err_terms(ctx, 3, t, bS, B, kr)); }
        { const F *t[8] = {bL, bR, beta, fL, fR, fb, fm, nullptr}; HB_TRY(launch_err_terms(ctx, 4, t, bS, B, k4)); }
        if (!feq(fsub(fadd(fadd(k4[3], kl[2]), kr[2]), k2[1]), fmake(0))) o->checks[0] = 0;                 // "Error in gate consistency 1" (:840-843)
        rnd = mimc_hash(k2[0], rnd); rnd = mimc_hash(k2[1], rnd);
        rnd = mimc_hash(kl[0], rnd); rnd = mimc_hash(kl[1], rnd); rnd = mimc_hash(kl[2], rnd);
        rnd = mimc_hash(kr[0], rnd); rnd = mimc_hash(kr[1], rnd); rnd = mimc_hash(kr[2], rnd);
        R.push_back(rnd);
        const F x1 = rnd, x2 = fmul(rnd, x1), x3 = fmul(rnd, x2), x4 = fmul(rnd, x3);
        KO = fadd(KO, fadd(fmul(x1, k2[0]), fmul(x2, k2[1])));
        KL = fadd(KL, fadd(fadd(fmul(x1, kl[0]), fmul(x2, kl[1])), fmul(x3, kl[2])));
        KR = fadd(KR, fadd(fadd(fmul(x1, kr[0]), fmul(x2, kr[1])), fmul(x3, kr[2])));
        KM = fadd(KM, fadd(fadd(fmul(x1, k4[0]), fmul(x2, k4[1])), fadd(fmul(x3, k4[2]), fmul(x4, k4[3]))));
        HB_TRY(launch_axpy_i32(ctx, fa, bS, rnd, 0, B)); HB_TRY(launch_axpy(ctx, fL, bL, rnd, B)); HB_TRY(launch_axpy(ctx, fR, bR, rnd, B));      // (:862-869)
        HB_TRY(launch_axpy(ctx, fO, bO, rnd, B)); HB_TRY(launch_axpy_i32(ctx, fm, bS, rnd, 1, B)); HB_TRY(launch_axpy(ctx, fb, beta, rnd, B));
    }
    HB_TRY(next(0, &bL, &bR, &bO, &bS));                                                 // reset_stream(tr) (:871)
    memcpy(o->R, R.data(), n_chunks * sizeof(F));
    F a[4]; { F cst = fmake(0); for (int i = 0; i < 4; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); a[i] = fadd(cst, fmake((uint64_t)rand())); } }      // a = generate_randomness(4)
    memcpy(o->a, a, sizeof a);
    F sum = fadd(fadd(fmul(a[0], KL), fmul(a[1], KR)), fadd(fmul(a[2], KM), fmul(KO, a[3])));
    int chk2 = 0;
    HB_TRY(hobbit_gate_sumcheck(ctx, reinterpret_cast<hobbit_F *>(fa), reinterpret_cast<hobbit_F *>(fb), reinterpret_cast<hobbit_F *>(fL), reinterpret_cast<hobbit_F *>(fR),
                                reinterpret_cast<hobbit_F *>(fO), reinterpret_cast<hobbit_F *>(fm), B, reinterpret_cast<hobbit_F *>(a), reinterpret_cast<hobbit_F *>(&rnd),
                                reinterpret_cast<hobbit_F *>(&sum), o->poly, o->gr, o->fin6, &chk2));
    o->checks[1] = chk2;
    // Peval pass (:941-959): beta1 over the sumcheck challenges
    HB_TRY(hobbit_eq_table(ctx, o->gr, logB, reinterpret_cast<hobbit_F *>(tmp)));
    for (size_t c = 0; c < n_chunks; c++) {
        HB_TRY(next(B, &bL, &bR, &bO, &bS));
        HB_TRY(launch_dot_gen(ctx, tmp, bL, 1, nullptr, B, part, dres + 0 * n_chunks + c));
        HB_TRY(launch_dot_gen(ctx, tmp, bR, 1, nullptr, B, part, dres + 1 * n_chunks + c));
        HB_TRY(launch_dot_gen(ctx, tmp, bO, 1, nullptr, B, part, dres + 2 * n_chunks + c));
        HB_TRY(launch_dot_i32(ctx, tmp, bS, 0, B, part, dres + 3 * n_chunks + c));
        HB_TRY(launch_dot_i32(ctx, tmp, bS, 1, B, part, dres + 4 * n_chunks + c));
        HB_TRY(launch_dot_gen(ctx, tmp, beta, 1, nullptr, B, part, dres + 5 * n_chunks + c));
    }
    HB_TRY(hobbit_memcpy_d2h(ctx, o->Peval, dres, 6 * n_chunks * sizeof(F)));
    F b[6]; { F cst = fmake(0); for (int i = 0; i < 6; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); b[i] = fadd(cst, fmake((uint64_t)rand())); } }      // b = generate_randomness(6)
    memcpy(o->b, b, sizeof b);
    std::vector<F> pe(n_chunks, fmake(0));
    for (size_t j = 0; j < n_chunks; j++) for (int i = 0; i < 6; i++) pe[j] = fadd(pe[j], fmul(b[i], cF(o->Peval)[(size_t)i * n_chunks + j]));
    HB_TRY(hobbit_memcpy_h2d(ctx, dR, R.data(), n_chunks * sizeof(F)));
    HB_TRY(hobbit_memcpy_h2d(ctx, dR + n_chunks, pe.data(), n_chunks * sizeof(F)));
    HB_TRY(hobbit_sumcheck2(ctx, reinterpret_cast<hobbit_F *>(dR), reinterpret_cast<hobbit_F *>(dR + n_chunks), n_chunks, reinterpret_cast<hobbit_F *>(&rnd), o->q2, o->r2, o->vr2, o->fin2));
    {   // "Error in gate consistency 3" (:966-972); fin6 = add, beta, L, R, O, mul
        CHP f6 = cF(o->fin6), q2 = cF(o->q2);
        F sm = fadd(fadd(fmul(f6[2], b[0]), fmul(f6[3], b[1])), fadd(fmul(f6[4], b[2]), fmul(b[3], f6[0])));
        sm = fadd(sm, fadd(fmul(b[4], f6[5]), fmul(b[5], f6[1])));
        o->checks[2] = feq(fadd(fadd(q2[0], q2[1]), fadd(q2[2], q2[2])), sm);
    }
    return 0;
}

// has_lookups / lookup_rand (src/main.cpp:67,70,888,910): switches compute{3,4}p_error_terms to their lookup gate maps
int hobbit_set_lookups(hobbit_ctx *ctx, int on, const hobbit_F *h_lookup_rand) {
    if (on && !h_lookup_rand) return ctx->fail(HOBBIT_EINVAL, "set_lookups: lookup_rand[0..1] needed");
    ctx->has_lookups = on != 0;
    if (on) { ctx->lookup_rand[0] = cF(h_lookup_rand)[0]; ctx->lookup_rand[1] = cF(h_lookup_rand)[1]; }
    return 0;
}
// prove_gate_consistency_lookups (src/sumcheck.cpp:503-795) over a caller-supplied trace source; selectors 0 add, 1 mul, 2 lookup
int hobbit_gate_consistency_lookups_stream(hobbit_ctx *ctx, hobbit_trace_source source, void *user, size_t n_chunks, size_t B, const hobbit_F *h_r, hobbit_gate_lkp_stream_out *o) {
    const int logB = ilog2_exact(B), lR = ilog2_exact(n_chunks);
    if (!o || !source || logB < 1 || lR < 1) return ctx->fail(HOBBIT_EINVAL, "gate_consistency_lookups_stream: BUFFER_SPACE and the chunk count must be powers of two, chunks >= 2");
    if (!ctx->has_lookups) return ctx->fail(HOBBIT_EINVAL, "gate_consistency_lookups_stream: has_lookups is not set (hobbit_set_lookups)");
    auto next = [&](size_t n, const F **L, const F **R, const F **O, const int32_t **S) -> int {
        const hobbit_F *l = nullptr, *r = nullptr, *oo = nullptr; const int32_t *s = nullptr;
        if (source(user, n, &l, &r, &oo, &s) != 0 || (n && (!l || !r || !oo || !s))) return ctx->fail(HOBBIT_EINVAL, "trace source failed");
        *L = cF(l); *R = cF(r); *O = cF(oo); *S = s; return 0;
    };
    enum { AL, AR, TL, TR, TO, LK, LO, MU, BE };
    const F *bL, *bR, *bO; const int32_t *bS;
    const size_t nres = 8 * n_chunks + 16;
    F *base; HB_TRY(ctx->workspace4((13 * B + 1024 + nres + 2 * n_chunks + 64) * sizeof(F), (void **)&base));
    F *t[9]; for (int q = 0; q < 9; q++) t[q] = base + (size_t)q * B;
    F *beta = base + 9 * B, *blo = beta + B, *tmp = blo + B, *si = tmp + B, *part = si + B, *dres = part + 1024, *dR = dres + nres;
    int32_t *s2 = reinterpret_cast<int32_t *>(si), *s3 = s2 + B;                          // 2 B int32 <= B F
    const F one = fmake(1);
    HB_TRY(hobbit_eq_table(ctx, h_r, logB, reinterpret_cast<hobbit_F *>(beta)));
    HB_TRY(launch_copy(ctx, t[BE], beta, B * sizeof(F)));
    HB_TRY(next(0, &bL, &bR, &bO, &bS));
    HB_TRY(next(B, &bL, &bR, &bO, &bS));
    HB_TRY(launch_copy(ctx, t[TL], bL, B * sizeof(F)));
    HB_TRY(launch_copy(ctx, t[TR], bR, B * sizeof(F)));
    HB_TRY(launch_copy(ctx, t[TO], bO, B * sizeof(F)));
    // the selector tables of chunk 0 (:519-537) = one selector fold with rand = 1 over zeroed tables
    HB_TRY(launch_zero(ctx, t[AL], B * sizeof(F))); HB_TRY(launch_zero(ctx, t[AR], B * sizeof(F))); HB_TRY(launch_zero(ctx, t[LK], B * sizeof(F))); HB_TRY(launch_zero(ctx, t[MU], B * sizeof(F)));
    HB_TRY(launch_lkp_sel_fold(ctx, bS, one, t[AL], t[AR], t[LK], t[MU], B));
    HB_TRY(launch_lkp_prepare(ctx, bS, bL, bR, bO, nullptr, nullptr, t[LO], B));
    // Kf_O, Kf_L, Kf_R, Kf_lkp, Kf_M (:541-548)
    HB_TRY(launch_dot_gen(ctx, beta, t[TO], 1, nullptr, B, part, dres));
    HB_TRY(launch_dot_gen(ctx, beta, t[TL], 1, t[AL], B, part, dres + 1));
    HB_TRY(launch_dot_gen(ctx, beta, t[TR], 1, t[AR], B, part, dres + 2));
    HB_TRY(launch_dot_gen(ctx, beta, t[LO], 1, t[LK], B, part, dres + 3));
    HB_TRY(launch_f_binop(ctx, 2, t[TR], t[TL], tmp, B));
    HB_TRY(launch_dot_gen(ctx, beta, tmp, 1, t[MU], B, part, dres + 4));
    F K0[5]; HB_TRY(hobbit_memcpy_d2h(ctx, K0, dres, 5 * sizeof(F)));
    F KO = K0[0], KL = K0[1], KR = K0[2], KK = K0[3], KM = K0[4], rnd = fmake(0);
    o->checks[0] = feq(fsub(fsub(fadd(fadd(KM, KL), KR), KK), KO), fmake(0)) ? 1 : 0;   // (:549-552: the reference exits)
    o->checks[3] = 1;
    std::vector<F> R; R.push_back(fmake(1));
    for (size_t c = 1; c < n_chunks; c++) {
        HB_TRY(next(B, &bL, &bR, &bO, &bS));
        HB_TRY(launch_lkp_prepare(ctx, bS, bL, bR, bO, s2, s3, blo, B));
        F k2[4], kl[4], kr[4], kk[4], k4[4];
        { const F *tt[8] = {bO, beta, t[TO], t[BE], nullptr, nullptr, nullptr, nullptr}; HB_TRY(launch_err_terms(ctx, 2, tt, nullptr, B, k2)); }
        { const F *tt[8] = {bL, t[TL], t[AL], t[BE], beta, nullptr, nullptr, nullptr}; HB_TRY(launch_err_terms(ctx, 3, tt, bS, B, kl)); }
        { const F *tt[8] = {bR, t[TR], t[AR], t[BE], beta, nullptr, nullptr, nullptr}; HB_TRY(launch_err_terms(ctx, 3, tt, s2, B, kr)); }
        { const F *tt[8] = {blo, t[LO], t[LK], t[BE], beta, nullptr, nullptr, nullptr}; HB_TRY(launch_err_terms(ctx, 3, tt, s3, B, kk)); }
        { const F *tt[8] = {bL, bR, beta, t[TL], t[TR], t[BE], t[MU], nullptr}; HB_TRY(launch_err_terms(ctx, 4, tt, bS, B, k4)); }     // gate = [s == 1]: 2 and the reference's 4 agree
        if (!feq(fsub(fsub(fadd(fadd(k4[3], kl[2]), kr[2]), kk[2]), k2[1]), fmake(0))) o->checks[0] = 0;                                  // "Error in gate consistency 1" (:588-591)
        rnd = mimc_hash(k2[0], rnd); rnd = mimc_hash(k2[1], rnd);                                                                          // lookup and mul terms are NOT hashed (:593-600)
        rnd = mimc_hash(kl[0], rnd); rnd = mimc_hash(kl[1], rnd); rnd = mimc_hash(kl[2], rnd);
        rnd = mimc_hash(kr[0], rnd); rnd = mimc_hash(kr[1], rnd); rnd = mimc_hash(kr[2], rnd);
        R.push_back(rnd);
        const F x1 = rnd, x2 = fmul(rnd, x1), x3 = fmul(rnd, x2), x4 = fmul(rnd, x3);
        KO = fadd(KO, fadd(fmul(x1, k2[0]), fmul(x2, k2[1])));
        KK = fadd(KK, fadd(fadd(fmul(x1, kk[0]), fmul(x2, kk[1])), fmul(x3, kk[2])));
        KL = fadd(KL, fadd(fadd(fmul(x1, kl[0]), fmul(x2, kl[1])), fmul(x3, kl[2])));
        KR = fadd(KR, fadd(fadd(fmul(x1, kr[0]), fmul(x2, kr[1])), fmul(x3, kr[2])));
        KM = fadd(KM, fadd(fadd(fmul(x1, k4[0]), fmul(x2, k4[1])), fadd(fmul(x3, k4[2]), fmul(x4, k4[3]))));
        HB_TRY(launch_lkp_sel_fold(ctx, bS, rnd, t[AL], t[AR], t[LK], t[MU], B));                                                           // (:611-630)
        HB_TRY(launch_axpy(ctx, t[TL], bL, rnd, B)); HB_TRY(launch_axpy(ctx, t[TR], bR, rnd, B)); HB_TRY(launch_axpy(ctx, t[TO], bO, rnd, B));
        HB_TRY(launch_axpy(ctx, t[LO], blo, rnd, B)); HB_TRY(launch_axpy(ctx, t[BE], beta, rnd, B));
        // the reference's per-chunk self-check  sum fold_beta fold_mul fold_R fold_L == Kf_M  (:632-641)
        HB_TRY(launch_f_binop(ctx, 2, t[TR], t[TL], tmp, B));
        HB_TRY(launch_dot_gen(ctx, t[BE], tmp, 1, t[MU], B, part, dres));
        F sM; HB_TRY(hobbit_memcpy_d2h(ctx, &sM, dres, sizeof(F)));
        if (!feq(sM, KM)) o->checks[3] = 0;
    }
    HB_TRY(next(0, &bL, &bR, &bO, &bS));                                                 // reset_stream(tr) (:643)
    memcpy(o->R, R.data(), n_chunks * sizeof(F));
    F a[5]; { F cst = fmake(0); for (int i = 0; i < 5; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); a[i] = fadd(cst, fmake((uint64_t)rand())); } }      // a = generate_randomness(5)
    memcpy(o->a, a, sizeof a);
    { HB_TRY(launch_dot_gen(ctx, t[BE], t[LO], 1, t[LK], B, part, dres)); F sK; HB_TRY(hobbit_memcpy_d2h(ctx, &sK, dres, sizeof(F))); o->checks[4] = feq(sK, KK) ? 1 : 0; }   // (:646-652)
    F sum = fadd(fadd(fadd(fmul(a[0], KL), fmul(a[1], KR)), fadd(fmul(a[2], KM), fmul(KO, a[3]))), fmul(KK, a[4]));
    int chk2 = 0;
    HB_TRY(launch_gate_lkp_sumcheck(ctx, t, B, a, &rnd, &sum, mF(o->poly), mF(o->gr), mF(o->fin9), &chk2));
    o->checks[1] = chk2;
    // Peval pass (:736-764): beta1 over the sumcheck challenges; the selector columns as field tables through the same selector fold
    HB_TRY(hobbit_eq_table(ctx, o->gr, logB, reinterpret_cast<hobbit_F *>(tmp)));
    for (size_t c = 0; c < n_chunks; c++) {
        HB_TRY(next(B, &bL, &bR, &bO, &bS));
        HB_TRY(launch_zero(ctx, t[AL], B * sizeof(F))); HB_TRY(launch_zero(ctx, t[AR], B * sizeof(F))); HB_TRY(launch_zero(ctx, t[LK], B * sizeof(F))); HB_TRY(launch_zero(ctx, t[MU], B * sizeof(F)));
        HB_TRY(launch_lkp_sel_fold(ctx, bS, one, t[AL], t[AR], t[LK], t[MU], B));
        HB_TRY(launch_lkp_prepare(ctx, bS, bL, bR, bO, nullptr, nullptr, blo, B));
        const F *cols[8] = {bL, bR, bO, t[AL], t[AR], t[MU], t[LK], blo};
        for (int q = 0; q < 8; q++) HB_TRY(launch_dot_gen(ctx, tmp, cols[q], 1, nullptr, B, part, dres + (size_t)q * n_chunks + c));
    }
    HB_TRY(hobbit_memcpy_d2h(ctx, o->Peval, dres, 8 * n_chunks * sizeof(F)));
    F b[8]; { F cst = fmake(0); for (int i = 0; i < 8; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); b[i] = fadd(cst, fmake((uint64_t)rand())); } }      // b = generate_randomness(8)
    memcpy(o->b, b, sizeof b);
    std::vector<F> pe(n_chunks, fmake(0));
    for (size_t j = 0; j < n_chunks; j++) for (int i = 0; i < 8; i++) pe[j] = fadd(pe[j], fmul(b[i], cF(o->Peval)[(size_t)i * n_chunks + j]));
    HB_TRY(hobbit_memcpy_h2d(ctx, dR, R.data(), n_chunks * sizeof(F)));
    HB_TRY(hobbit_memcpy_h2d(ctx, dR + n_chunks, pe.data(), n_chunks * sizeof(F)));
    HB_TRY(hobbit_sumcheck2(ctx, reinterpret_cast<hobbit_F *>(dR), reinterpret_cast<hobbit_F *>(dR + n_chunks), n_chunks, reinterpret_cast<hobbit_F *>(&rnd), o->q2, o->r2, o->vr2, o->fin2));
    {   // "Error in gate consistency 3" (:783-789)
        CHP f9 = cF(o->fin9), q2 = cF(o->q2);
        F sm = fadd(fadd(fmul(f9[TL], b[0]), fmul(f9[TR], b[1])), fmul(f9[TO], b[2]));
        sm = fadd(sm, fmul(b[3], f9[AL])); sm = fadd(sm, fmul(b[4], f9[AR])); sm = fadd(sm, fmul(b[5], f9[MU]));
        sm = fadd(sm, fmul(b[6], f9[LK])); sm = fadd(sm, fmul(b[7], f9[LO]));
        o->checks[2] = feq(fadd(fadd(q2[0], q2[1]), fadd(q2[2], q2[2])), sm);
    }
    return 0;
}

// ---- Our_PC open without the inner shockwave/WHIR PCS -------------------------------------------
// open_standard (src/Our_PC.cpp:604-661) + recursive_prover_Spielman (src/PC_utils.cpp:271-385) minus
// shockwave_commit / shockwave_prove.  Host: libc draws in the reference's order, the transcript,
// challenge powers; device: everything that touches a table.
// With a commitment `c`: the aggregate is computed from d_poly (N = M K coefficients).  With c == NULL (multi-GPU open): d_poly is the
// M-element aggregate itself, summed by the caller from per-rank partials; dims = {K, trs}; replies and paths are the caller's business.
// One opening: what its stages share, and the stages in the reference's order (open_impl_body is the list).  Two schedules, chosen once:
//   serial      everything on the caller's thread and stream.  open_core, HOBBIT_OPEN_THREADS=0, a full per-kernel profile (mode 1) and
//               HOBBIT_TRACE=1 run it; the transcript recorder is per calling thread, so the tests against the reference's transcript need it.
//   overlapped  after the aggregate's tensor code the two inner commitments (needed only by the shockwave_prove calls at the very end) and behind
//               them the query answers (which feed nothing) go to helper2's stream, P1 -> P2 -> P3 -> P4 stay on the caller's thread and stream;
//               after P4, shockwave_prove(C_c) runs on the helper context from a second host thread beside P5 -> shockwave_prove(C_f).  Each
//               chain is a sequence of small dependent launches and host round trips that leaves the GPU mostly idle on its own.
//               Events: side_ev[62] tensor code final (main -> helper2), [63] inner commitments final, [60] query answers final (-> main),
//               [61] main stream at the end of P4 (-> helper: C).  The stream is never drained in mid-chain.
struct OpenRun {
    hobbit_ctx *ctx; const hobbit_F *d_poly; size_t N; const hobbit_commitment *c; const hobbit_F *h_x; int queries; hobbit_open_out *o; bool full, overlapped;
    OpenTrace tr; StageScope sc;
    int K, trs, logK, logc, R1, R3; size_t M, cols, rows2, big, nc_el;
    F *d_aggr, *BIG, *Mp, *C, *Tcm, *d_s, *d_ev, *d_ac, *d_b1, *tmpv, *encf, *encc; uint64_t *tmpi; uint8_t *lvf, *lvc;       // device arena
    std::vector<F> beta, sv, r1; std::vector<uint32_t> qc, qr; std::vector<uint64_t> Iv; F s2, a; size_t nnz = 0;      // host: beta over the chunk variables, the libc draws, buff2's length
    hobbit_F *Q1, *Q2, *Q3, *Q4, *Q5, *Rr1, *Rr2, *Rr3, *Rr4, *Rr5;                                                    // the output cursors of P1..P5
    F y1 = {}, *y1_pin = nullptr;                                          // y1 and the pinned slot its read-back lands in (y1_p5, finish)
    bool real_poly = false;                                                // d_poly holds N reals of 8 bytes (hobbit_open_standard_real): the aggregate reads them as such
    ShockPlan plan_c, plan_f;                                              // the libc draws of shockwave_prove(C_c) and (C_f), taken in libc_draws
    // overlapped only: the hand-over of the query answers; shockwave_prove(C_c) on the helper context.  Its thread is started in libc_draws,
    // while the GPU is busy, and parks on sp_cv until start_prove_cc lets it run (sp_go = 1) or the destructor sends it home (-1).
    std::thread q_thread, sp_thread; int sp_rc = 0;
    std::mutex sp_mu; std::condition_variable sp_cv; int sp_go = 0; bool cc_on_helper = false;
    void sp_signal(int go) { { std::lock_guard<std::mutex> lk(sp_mu); if (sp_go == 0) sp_go = go; } sp_cv.notify_one(); }
    OpenRun(hobbit_ctx *ctx_, const hobbit_F *d_poly_, size_t N_, const hobbit_commitment *c_, const hobbit_F *h_x_, int queries_, hobbit_open_out *o_, bool full_)
        : ctx(ctx_), d_poly(d_poly_), N(N_), c(c_), h_x(h_x_), queries(queries_), o(o_), full(full_), tr(ctx_), sc(ctx_) {
        const char *ot_env = getenv("HOBBIT_OPEN_THREADS");
        overlapped = full && o->sp_c && !(ot_env && ot_env[0] == '0') && ctx->prof_on != 1 && !tr.drain;
    }
    ~OpenRun() {            // every return path joins its threads; a worker still parked leaves without running
        if (sp_thread.joinable()) sp_signal(-1);
        for (std::thread *t : {&sp_thread, &q_thread}) if (t->joinable()) t->join();
    }
    int dims_beta_first_draw(const int *dims) {
        tr.mark("entry (stream drain)");
        if (c && !c->lin) return ctx->fail(HOBBIT_EINVAL, "open_core: only the RS x expander (linear_time) code is built");
        K = c ? c->K : dims[0]; trs = c ? c->trs : dims[1];
        if (K <= 0 || trs < 4 || N % (size_t)K) return ctx->fail(HOBBIT_EINVAL, "open: bad K / trs");
        M = N / (size_t)K; cols = 2 * M / (size_t)trs; rows2 = 2 * (size_t)trs; big = rows2 * cols; nc_el = (size_t)trs * cols;
        logK = ilog2_exact((size_t)K); logc = ilog2_exact(cols); R1 = ilog2_exact(rows2); R3 = R1 + logc;
        if (logK < 0 || (c && (M != c->M || cols != c->cols)) || logc != 12 || R1 < 0) return ctx->fail(HOBBIT_EINVAL, "open_core: needs K a power of two and 4096-point row codes");
        // beta over the chunk variables (precompute_beta, host: K <= 64 entries) and the r_v[0] draw (:619-623), the first libc draw of the call
        beta.resize((size_t)K); beta[0] = fmake(1);
        if (c) for (int i = 0; i < logK; i++) for (size_t j = ((size_t)1 << i); j-- > 0;) { F t = fmul(cF(h_x)[logK - 1 - i], beta[j]); beta[2 * j + 1] = t; beta[2 * j] = fsub(beta[j], t); }
        F rv0 = fmake((uint64_t)random()); rv0 = fadd(rv0, fmake((uint64_t)rand())); memcpy(&o->scalars[0], &rv0, sizeof(F));   // generate_randomness(1)
        return 0;
    }
    int size_scratch_and_lay_out_arena() {
        F *arena = nullptr;
        // + the two inner shockwave commitments kept for the later shockwave_prove: encoded matrices (2M and 2*trs*cols F) and their trees
        const size_t sw_el = 2 * M + 2 * nc_el + 2 * (2 * M / 32 + 2 * nc_el / 32) * 2 + 64;
        const size_t n_el = M + 2 * big + 2 * cols + 4 * rows2 + 2 * (size_t)queries + 128 + sw_el;
        HB_TRY(ctx->workspace3(n_el * sizeof(F), (void **)&arena));
        // size the shared scratch buffers once for the largest user below (the 4M-element sumchecks, the 32-row long FFTs of
        // the inner commitments): growing them step by step frees and re-maps device memory several times per call
        void *dummy;
        const size_t sc_need = (3 * big / 2 + 3 * 1024 + 64) * sizeof(F), fft_need = (size_t)2 * nc_el * sizeof(F);
        HB_TRY(ctx->workspace(std::max(sc_need, fft_need), &dummy));
        HB_TRY(ctx->workspace2(std::max(fft_need, (size_t)4 * rows2 * sizeof(F)), &dummy));
        // the same for the inner provers' scratch and the pinned staging buffer: no buffer is ever grown-and-freed after this point.
        // (Freeing device memory makes the driver unmap it later and pause the compute queues while it does: a 20+ ms stall that
        // lands in the NEXT call, measured on the second open of a process.)
        if (full) HB_TRY(ctx->workspace4((shockwave_nested_elems(nc_el / 32) + shockwave_own_elems(nc_el / 32, 32)) * sizeof(F), &dummy));
        HB_TRY(ctx->pinned(std::max((size_t)queries * (sizeof(F) + 8) + 4096, (WHIR_DIN * 6 + WHIR_DRES) * sizeof(F)), &dummy));
        tr.mark("scratch sizing");
        if (tr.on) fprintf(stderr, "[hobbit open] scratch at entry: ws %zu ws2 %zu ws3 %zu ws4 %zu pin %zu\n", ctx->ws[0].bytes(), ctx->ws[1].bytes(), ctx->ws[2].bytes(), ctx->ws[3].bytes(), ctx->pin.bytes());
        d_aggr = arena; BIG = d_aggr + M; Tcm = BIG + big; d_s = Tcm + big; d_ev = d_s + cols; d_ac = d_ev + cols; d_b1 = d_ac + rows2;
        Mp = BIG; C = BIG + nc_el;
        tmpv = d_b1 + rows2; tmpi = reinterpret_cast<uint64_t *>(tmpv + queries + 1);                 // the sparse buff2: (index, value) lists
        encf = d_b1 + rows2 + 2 * (size_t)queries + 64; encc = encf + 2 * M;                          // the inner commitments' encoded matrices ...
        lvf = reinterpret_cast<uint8_t *>(encc + 2 * nc_el); lvc = lvf + 64 * (2 * M / 32);           // ... and their trees
        Q1 = o->qpoly; Q2 = Q1 + 3 * R1; Q3 = Q2 + 3 * logc; Q4 = Q3 + 3 * R3; Q5 = Q4 + 3 * R3;
        Rr1 = o->r; Rr2 = Rr1 + R1; Rr3 = Rr2 + logc; Rr4 = Rr3 + R3; Rr5 = Rr4 + R3;
        tr.mark("beta + arena");
        return 0;
    }
    int aggregate_and_tensor_code() {
        if (c && real_poly) HB_TRY(hobbit_aggregate_real(ctx, reinterpret_cast<const uint64_t *>(d_poly), N, reinterpret_cast<const hobbit_F *>(beta.data()), K, reinterpret_cast<hobbit_F *>(d_aggr)));
        else if (c) HB_TRY(hobbit_aggregate(ctx, d_poly, N, reinterpret_cast<const hobbit_F *>(beta.data()), K, reinterpret_cast<hobbit_F *>(d_aggr)));   // _aggregate axpy (:258-272)
        else HB_TRY(launch_copy(ctx, d_aggr, d_poly, M * sizeof(F)));
        // compute_tensorcode(aggr) (:277): M' = row FFTs (row-major), codeword-major copy, expander encode, parity half back to row-major C
        tr.mark("beta, arena, aggregate");
        HB_TRY(fft::rows(ctx, d_aggr, cols / 2, (uint32_t)(cols / 2), Mp, cols, 1, logc, false, 1, (uint32_t)trs, 0, 0));
        tr.mark("row FFTs");
        HB_TRY(launch_transpose(ctx, Mp, 0, (uint32_t)trs, (uint32_t)cols, Tcm, 0, rows2, 1));
        tr.mark("transpose");
        if (ctx->code.n != trs) { long long l; HB_TRY(hobbit_graph_finalize(ctx, trs, &l)); }
        HB_TRY(launch_encode(ctx, Tcm, rows2, Tcm, rows2, trs, cols, 0));
        tr.mark("encode");
        HB_TRY(launch_transpose_ld(ctx, Tcm + trs, 0, rows2, (uint32_t)cols, (uint32_t)trs, C, 0, cols, 1));
        tr.mark("aggregate+tensorcode");
        return 0;
    }
    // _aggregate's inner commitments (src/Our_PC.cpp:274-287): C_f = shockwave_commit(aggr, 32), C_c = shockwave_commit(parity half, 32)
    int inner_commitments() {
        hobbit_F *aggr = reinterpret_cast<hobbit_F *>(d_aggr), *parity = reinterpret_cast<hobbit_F *>(C), *ef = reinterpret_cast<hobbit_F *>(encf), *ec = reinterpret_cast<hobbit_F *>(encc);
        if (overlapped) {
            for (hobbit_ctx **h : {&ctx->helper, &ctx->helper2}) if (!*h) {
                if (hobbit_ctx_create(ctx->device, h) != 0) return ctx->fail(HOBBIT_EHIP, "open: helper context creation failed");
                (*h)->sync_mode = ctx->sync_mode;
            }
            HB_TRY(ctx->side_init());
            hobbit_ctx *hc = ctx->helper2;
            HB_CHECK(ctx, hipEventRecord(ctx->side_ev[62], ctx->stream)); HB_CHECK(ctx, hipStreamWaitEvent(hc->stream, ctx->side_ev[62], 0));
            if (hobbit_shockwave_commit(hc, aggr, M, 32, ef, lvf) || hobbit_shockwave_commit(hc, parity, nc_el, 32, ec, lvc)) return ctx->fail(HOBBIT_EHIP, hc->err);
            HB_CHECK(ctx, hipEventRecord(ctx->side_ev[63], hc->stream));            // their roots are read in start_prove_cc, behind this event
        } else {
            HB_TRY(hobbit_shockwave_commit(ctx, aggr, M, 32, ef, lvf));
            HB_TRY(hobbit_shockwave_commit(ctx, parity, nc_el, 32, ec, lvc));
            HB_TRY(read_roots());
        }
        tr.mark("shockwave_commit C_f, C_c");
        return 0;
    }
    int read_roots() {      // (asynchronous: complete at the next of the many synchronisation points that follow)
        if (!o->roots) return 0;
        HB_TRY(d2h_staged(ctx, o->roots, lvf + 32 * (2 * (2 * M / 32) - 2), 32));
        return d2h_staged(ctx, o->roots + 32, lvc + 32 * (2 * (2 * nc_el / 32) - 2), 32);
    }
    // Every libc draw of the opening after r_v[0], in the reference's order -- queries (:633-641), s (src/PC_utils.cpp:293), r1
    // (prove_linear_code's generate_randomness, src/sumcheck.cpp:3225), s2 (:331), a (:342) -- none depends on device data, and nothing between
    // them draws.  Taken here, while the GPU still works through the aggregate's tensor code and inner commitments queued above: the GPU
    // never waits for the host later.  The reference's next draws after `a` are those of shockwave_prove(C_c) and then of shockwave_prove(C_f)
    // (P3, P4 and P5 draw nothing, and nothing else in those two proofs draws), and they depend on sizes alone: both plans are drawn here
    // too, in that order, under either schedule.  The overlapped schedule also starts the thread of shockwave_prove(C_c) here; it parks
    // until P4 has returned, so that neither the plan nor a thread start stands between P4 and y1.
    int libc_draws() {
        qc.resize(queries); qr.resize(queries); Iv.resize(queries); sv.resize(cols); r1.resize(R1);
        for (int q = 0; q < queries; q++) { qc[q] = (uint32_t)(rand() % (long)cols); qr[q] = (uint32_t)(rand() % (long)rows2); Iv[q] = qc[q] + cols * (uint64_t)qr[q]; }
        sv[0] = fmake((uint64_t)random()); o->scalars[1] = *reinterpret_cast<hobbit_F *>(&sv[0]);
        { F cst = fmake(0); for (int i = 0; i < R1; i++) { if (i % 100 == 0) cst = fmake((uint64_t)random()); r1[i] = fadd(cst, fmake((uint64_t)rand())); } }
        s2 = fmake((uint64_t)random()); o->scalars[2] = *reinterpret_cast<const hobbit_F *>(&s2);
        a = fmake((uint64_t)random()); o->scalars[3] = *reinterpret_cast<const hobbit_F *>(&a);
        if (o->cols) memcpy(o->cols, qc.data(), 4 * (size_t)queries);
        if (o->rows) memcpy(o->rows, qr.data(), 4 * (size_t)queries);
        if (full) {
            if (shockwave_plan(nc_el, 32, plan_c) != 0) return ctx->fail(HOBBIT_EINVAL, "open: C_c has no shockwave plan");
            if (shockwave_plan(M, 32, plan_f) != 0) return ctx->fail(HOBBIT_EINVAL, "open: C_f has no shockwave plan");
        }
        if (overlapped) {
            hobbit_ctx *hc = ctx->helper;
            try {       // (this object outlives the thread: its destructor releases and joins it)
                sp_thread = std::thread([this, hc] {
                    hipSetDevice(hc->device);
                    { std::unique_lock<std::mutex> lk(sp_mu); sp_cv.wait(lk, [this] { return sp_go != 0; }); if (sp_go < 0) return; }
                    sp_rc = shockwave_prove_run(hc, reinterpret_cast<hobbit_F *>(C), reinterpret_cast<hobbit_F *>(encc), lvc, nc_el, 32, Rr4, R3 - 1, o->sp_c, plan_c);
                });
                cc_on_helper = true;
            } catch (const std::exception &) { /* no thread: the proof runs on this context where the serial schedule runs it */ }
        }
        tr.mark("libc draws");
        return 0;
    }
    // replies (:291-305) and Merkle paths (:645-647) at the drawn positions.  Without a commitment (multi-GPU open) they are the caller's business.
    int query_answers() {
        if (c && overlapped) HB_TRY(query_answers_on_helper2());
        else if (c) {
            if (o->reply) HB_TRY(hobbit_commitment_gather(ctx, c, qr.data(), qc.data(), (size_t)queries, o->reply));
            if (o->paths) HB_TRY(hobbit_commitment_paths(ctx, c, qc.data(), qr.data(), (size_t)queries, o->paths));
        }
        tr.mark("queries: gather + paths queued");
        return 0;
    }
    // The answers feed nothing below: queued behind the inner commitments on helper2's stream (the staging arena stays this context's;
    // scratch is lent from helper2), off the chain P1 -> ... -> shockwave_prove(C_f).
    int query_answers_on_helper2() {
        hobbit_ctx *hc = ctx->helper2; const size_t n_def0 = ctx->deferred.size();
        const size_t lend = (size_t)queries * ((size_t)K * sizeof(F) + 8 + 32 * 40) + 4096;
        void *lp; if (hc->workspace2(lend, &lp) != 0) return ctx->fail(HOBBIT_ENOMEM, hc->err);      // (in stream order behind the commitments' last use of it)
        hipStream_t mainS = ctx->stream; int rc = 0;
        ctx->stream = hc->stream; ctx->ws_lent = lp; ctx->ws_lent_bytes = lend;
        if (o->reply) rc = hobbit_commitment_gather(ctx, c, qr.data(), qc.data(), (size_t)queries, o->reply);
        if (!rc && o->paths) rc = hobbit_commitment_paths(ctx, c, qc.data(), qr.data(), (size_t)queries, o->paths);
        ctx->stream = mainS; ctx->ws_lent = nullptr; ctx->ws_lent_bytes = 0;                         // restored before any return
        if (rc) return rc;
        HB_CHECK(ctx, hipEventRecord(ctx->side_ev[60], hc->stream));
        // The answers are 7 MB: handing them from the pinned staging arena to the caller's buffers at the closing synchronisation cost
        // 0.7 ms of single-threaded memcpy at the very end of the critical path.  They are final long before that, so a short-lived
        // thread waits for their event and copies them out while the main chain runs.
        if (ctx->deferred.size() == n_def0) return 0;
        std::vector<hobbit_ctx::Deferred> qdef(ctx->deferred.begin() + (long)n_def0, ctx->deferred.end());
        try {
            q_thread = std::thread([qdef, ev = ctx->side_ev[60], dev = ctx->device] {
                hipSetDevice(dev);
                if (hipEventSynchronize(ev) != hipSuccess) return;          // (the closing synchronisation reports the error)
                for (const auto &d : qdef) memcpy(d.dst, d.src, d.bytes);
            });
            ctx->deferred.resize(n_def0);                                   // the thread owns these hand-overs now
        } catch (const std::exception &) { /* no thread: the closing hand-over copies them */ }
        return 0;
    }
    int host_tables() {
        for (size_t i = 1; i < cols; i++) sv[i] = fmul(sv[i - 1], sv[0]);                                                   // s powers (:293-297)
        HB_TRY(h2d_staged(ctx, d_s, sv.data(), cols * sizeof(F)));
        // buff2: s2 powers at the queried positions, last write wins (:331-336).  P3 takes it as a sorted (index, value) list: 5900 non-zeros of 2^25.
        // (position, draw number) sorted as one key: the last draw of a position is the one whose power stays (a std::map here cost 0.6 ms of host time)
        std::vector<uint64_t> key((size_t)queries); std::vector<F> pws((size_t)queries);
        F pw = s2;
        for (int q = 0; q < queries; q++) { key[q] = (Iv[q] << 20) | (uint64_t)q; pws[q] = pw; pw = fmul(pw, s2); }
        std::sort(key.begin(), key.end());
        std::vector<uint64_t> idx; std::vector<F> val; idx.reserve((size_t)queries); val.reserve((size_t)queries);
        for (int q = 0; q < queries; q++)
            if (q + 1 == queries || (key[q + 1] >> 20) != (key[q] >> 20)) { idx.push_back(key[q] >> 20); val.push_back(pws[key[q] & 0xFFFFF]); }
        nnz = idx.size();
        HB_TRY(h2d_staged(ctx, tmpv, val.data(), val.size() * sizeof(F)));
        HB_TRY(h2d_staged(ctx, tmpi, idx.data(), idx.size() * 8));
        tr.mark("queries+gather+paths, host tables");
        return 0;
    }
    // aggr_c = [M' | C] . s (:298-309); P1 = prove_linear_code(aggr_c, trs) with r1 = generate_randomness(log2 2trs) (:310;
    // src/sumcheck.cpp:3223-3235); evals = beta(P1.r)^T [M' | C] (:311-320); P2 = sumcheck(s, evals, F(021) -- octal) (:322)
    int p1_evals_p2() {
        hobbit_F p17 = {021, 0};
        HB_TRY(launch_matvec_rows(ctx, BIG, rows2, cols, d_s, d_ac));
        HB_TRY(hobbit_prove_linear_code(ctx, reinterpret_cast<hobbit_F *>(d_ac), rows2, trs, reinterpret_cast<const hobbit_F *>(r1.data()), Q1, Rr1, o->vr, o->fin));
        HB_TRY(hobbit_eq_table(ctx, Rr1, R1, reinterpret_cast<hobbit_F *>(d_b1)));
        HB_TRY(launch_vecmat(ctx, BIG, rows2, cols, d_b1, d_ev));
        HB_TRY(hobbit_sumcheck2(ctx, reinterpret_cast<hobbit_F *>(d_s), reinterpret_cast<hobbit_F *>(d_ev), cols, &p17, Q2, Rr2, o->vr + 2, o->fin + 1));
        tr.mark("s, aggr_c, P1, evals, P2");
        return 0;
    }
    int p3() {              // P3 (:339) against the sparse buff2
        hobbit_F p121 = {121, 0};
        HB_TRY(launch_sumcheck2_sparse(ctx, BIG, tmpi, tmpv, nnz, big, *cF(&p121), mF(Q3), mF(Rr3), mF(o->vr + 4), mF(o->fin + 2)));
        tr.mark("buff2, P3");
        return 0;
    }
    // "Error recursion 1" (:323-326); a, beta(P2.r | P1.r) + a * beta(P3.r) (:342-349); P4 against [M' | C] (:362); "Error recursion 2" (:364-367)
    int p4() {
        { CHP q2 = cF(Q2); F c2 = fadd(fadd(q2[0], q2[1]), fadd(q2[2], q2[2])); o->checks[0] = feq(c2, cF(o->vr)[1]); }
        std::vector<hobbit_F> rcat(R3); hobbit_F p312 = {312, 0};
        memcpy(rcat.data(), Rr2, sizeof(hobbit_F) * logc); memcpy(rcat.data() + logc, Rr1, sizeof(hobbit_F) * R1);
        const F sc[2] = {fmake(1), a};             // beta(r) + a * beta(P3.r), never in memory: the sumcheck takes it by its two points
        HB_TRY(launch_sumcheck2_eq(ctx, 2, cF(rcat.data()), cF(Rr3), CHP(sc), BIG, big, *cF(&p312), mF(Q4), mF(Rr4), mF(o->vr + 6), mF(o->fin + 3)));
        { CHP q4 = cF(Q4); F c4 = fadd(fadd(q4[0], q4[1]), fadd(q4[2], q4[2])); F want = fadd(fmul(a, cF(o->vr)[4]), cF(o->vr)[3]); o->checks[1] = feq(c4, want); }
        tr.mark("betas, P4");
        return 0;
    }
    int prove_cc() {        // shockwave_prove(C_c, P4.r minus its last entry) (src/PC_utils.cpp:368), its draws taken in libc_draws
        HB_TRY(shockwave_prove_run(ctx, reinterpret_cast<hobbit_F *>(C), reinterpret_cast<hobbit_F *>(encc), lvc, nc_el, 32, Rr4, R3 - 1, o->sp_c, plan_c));
        tr.mark("shockwave_prove C_c");
        return 0;
    }
    // Overlapped, where the reference runs shockwave_prove(C_c): nothing after that proof depends on it and every challenge in it is a libc draw.
    // Its draws were taken in libc_draws, on the calling thread (ShockPlan); the proof runs on the helper context from the second host thread
    // parked there.  Nothing is drained: P4's challenges are host values, final when p4() has returned, and events order the device data for
    // the helper's stream -- side_ev[61] for C (this stream's, recorded here), side_ev[63] for encc and lvc (the commitments ran on helper2's).
    int start_prove_cc() {
        if (overlapped) {
            if (cc_on_helper) {
                hobbit_ctx *hc = ctx->helper;
                HB_CHECK(ctx, hipEventRecord(ctx->side_ev[61], ctx->stream)); HB_CHECK(ctx, hipStreamWaitEvent(hc->stream, ctx->side_ev[61], 0));
                HB_CHECK(ctx, hipStreamWaitEvent(hc->stream, ctx->side_ev[63], 0));
                sp_signal(1);
            }
            if (c) HB_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ctx->side_ev[60], 0));      // the query answers (their read-back is staged) ...
            HB_CHECK(ctx, hipStreamWaitEvent(ctx->stream, ctx->side_ev[63], 0));             // ... and the inner commitments are complete from here on
            HB_TRY(read_roots());
        }
        tr.mark("  helper released (events, no drain)");
        return 0;
    }
    // y1 = evaluate_vector(M', P4.r minus its last entry) (:372-373); P5 = prove_fft_matrix(initial tensor, r, y1) (:383)
    // Nothing on the chain needs y1 on the host: P5 takes P4.r, and y1 feeds only scalars[4] and the check against P5's first polynomial.
    // So it is read back like every other result of the opening -- a copy into the pinned staging arena queued behind the last fold, read
    // after the closing synchronisation -- and the check is made there (finish): no copy into pageable memory and no drain between P4 and P5.
    int y1_p5() {
        const F *d_y1;
        HB_TRY(eval_vector_dev(ctx, reinterpret_cast<hobbit_F *>(Mp), nc_el, Rr4, &d_y1));
        y1_pin = static_cast<F *>(ctx->stage_alloc(sizeof(F)));
        if (y1_pin) HB_CHECK(ctx, hipMemcpyAsync(y1_pin, d_y1, sizeof(F), hipMemcpyDeviceToHost, ctx->stream));      // (in stream order before P5 re-uses the workspace d_y1 lies in)
        else HB_TRY(hobbit_memcpy_d2h(ctx, reinterpret_cast<hobbit_F *>(&y1), d_y1, sizeof(F)));                    // arena full: the synchronous copy
        tr.mark("  y1 = evaluate_vector");
        HB_TRY(hobbit_prove_fft_matrix(ctx, reinterpret_cast<hobbit_F *>(d_aggr), (size_t)trs, cols / 2, Rr4, Q5, Rr5, o->vr + 8, o->fin + 4));
        tr.mark("y1, P5");
        return 0;
    }
    // the closing synchronisation and hand-over of the staged results, then y1 and the check that needs it: P5's claim against y1
    // (src/sumcheck.cpp:3016-3019)
    int finish() {
        HB_TRY(sc.finish());
        if (!sc.top) HB_TRY(ctx->sync());            // (inside another call's scope the drain is that call's: y1 is needed here)
        if (y1_pin) y1 = *y1_pin;
        o->scalars[4] = *reinterpret_cast<hobbit_F *>(&y1);
        CHP q5 = cF(Q5); const F c5 = fadd(fadd(q5[0], q5[1]), fadd(q5[2], q5[2]));
        o->checks[2] = feq(c5, y1);
        return 0;
    }
    // shockwave_prove(C_f, P5.randomness minus its last entry) (:384-385); P5.randomness = [sumcheck r | r1 = P4.r[logc .. logc+log2 trs)] (src/sumcheck.cpp:3021-3023)
    int prove_cf() {
        std::vector<hobbit_F> x5((size_t)logc + (size_t)(R1 - 1));
        memcpy(x5.data(), Rr5, sizeof(hobbit_F) * (size_t)logc); memcpy(x5.data() + logc, Rr4 + logc, sizeof(hobbit_F) * (size_t)(R1 - 1));
        HB_TRY(shockwave_prove_run(ctx, reinterpret_cast<hobbit_F *>(d_aggr), reinterpret_cast<hobbit_F *>(encf), lvf, M, 32, x5.data(), (int)x5.size() - 1, o->sp_f, plan_f));
        tr.mark("shockwave_prove C_f");
        return 0;
    }
};
static int open_impl_body(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_commitment *c, const int *dims, const hobbit_F *h_x, int queries, hobbit_open_out *o,
                          bool full, bool real_poly) {
    if ((!c && !dims) || !o || queries <= 0 || queries >= (1 << 20) || (full && (!o->sp_c || !o->sp_f))) return ctx->fail(HOBBIT_EINVAL, "open: bad arguments");
    if (!c && (o->reply || o->paths)) return ctx->fail(HOBBIT_EINVAL, "open_from_aggregate: replies and paths come from the tensor shards, not from here");
    OpenRun r(ctx, d_poly, N, c, h_x, queries, o, full);
    r.real_poly = real_poly;
    HB_TRY(r.dims_beta_first_draw(dims));
    HB_TRY(r.size_scratch_and_lay_out_arena());
    HB_TRY(r.aggregate_and_tensor_code());
    HB_TRY(r.inner_commitments());                   // overlapped: on helper2's stream
    HB_TRY(r.libc_draws());                          // both shockwave plans included; overlapped: the helper thread starts here and parks
    HB_TRY(r.query_answers());                       // overlapped: behind them on helper2's stream, handed over by a short-lived thread
    HB_TRY(r.host_tables());
    HB_TRY(r.p1_evals_p2());
    HB_TRY(r.p3());
    HB_TRY(r.p4());
    HB_TRY(r.start_prove_cc());                      // overlapped: helper2's work joins the main stream; shockwave_prove(C_c) on the helper context, second thread
    HB_TRY(r.y1_p5());
    if (!full) return r.finish();
    if (!r.cc_on_helper) HB_TRY(r.prove_cc());       // serial, or no helper thread: the reference runs it before P5; its draws were taken with the others, in the reference's order
    HB_TRY(r.prove_cf());
    if (r.cc_on_helper) {
        r.sp_thread.join();
        if (r.sp_rc) return ctx->fail(r.sp_rc, std::string("shockwave_prove(C_c) on the helper context: ") + ctx->helper->err);
    }
    if (r.tr.on) fprintf(stderr, "[hobbit open] scratch at exit:  ws %zu ws2 %zu ws3 %zu ws4 %zu pin %zu\n", ctx->ws[0].bytes(), ctx->ws[1].bytes(), ctx->ws[2].bytes(), ctx->ws[3].bytes(), ctx->pin.bytes());
    return r.finish();
}
static int open_impl(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_commitment *c, const int *dims, const hobbit_F *h_x, int queries, hobbit_open_out *o,
                     bool full, bool real_poly = false) {
    const int rc = open_impl_body(ctx, d_poly, N, c, dims, h_x, queries, o, full, real_poly);
    if (rc) {
        // an error return may leave work queued on the helper contexts' streams (inner commitments, query answers, their staged read-backs
        // into THIS context's arena): drain them before the caller -- or the next call's StageScope -- re-uses those buffers
        for (hobbit_ctx *h : {ctx->helper, ctx->helper2}) if (h) hipStreamSynchronize(h->stream);
        if (ctx->side) hipStreamSynchronize(ctx->side);
        hipStreamSynchronize(ctx->stream);
    }
    return rc;
}
int hobbit_open_core(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_commitment *c, const hobbit_F *h_x, int queries, hobbit_open_out *o) {
    if (!c) return ctx->fail(HOBBIT_EINVAL, "open_core: null commitment");
    return open_impl(ctx, d_poly, N, c, nullptr, h_x, queries, o, false);
}
int hobbit_open_standard(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, const hobbit_commitment *c, const hobbit_F *h_x, int queries, hobbit_open_out *o) {
    if (!c) return ctx->fail(HOBBIT_EINVAL, "open_standard: null commitment");
    return open_impl(ctx, d_poly, N, c, nullptr, h_x, queries, o, true);
}
// the same opening with the polynomial as N reals: only the aggregate reads it (k_aggregate_real), every later stage starts from the aggregate
int hobbit_open_standard_real(hobbit_ctx *ctx, const uint64_t *d_poly, size_t N, const hobbit_commitment *c, const hobbit_F *h_x, int queries, hobbit_open_out *o) {
    if (!c || !d_poly) return ctx->fail(HOBBIT_EINVAL, "open_standard_real: null commitment or polynomial");
    return open_impl(ctx, reinterpret_cast<const hobbit_F *>(d_poly), N, c, nullptr, h_x, queries, o, true, true);
}
int hobbit_open_from_aggregate(hobbit_ctx *ctx, const hobbit_F *d_aggr, size_t M, int K, int trs, int queries, hobbit_open_out *o) {
    const int dims[2] = {K, trs};
    return open_impl(ctx, d_aggr, M * (size_t)K, nullptr, dims, nullptr, queries, o, true);
}

int hobbit_sumcheck2(hobbit_ctx *ctx, const hobbit_F *d_v1, const hobbit_F *d_v2, size_t n, const hobbit_F *prev_r, hobbit_F *h_qpoly,
                     hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_final) {
    return launch_sumcheck2(ctx, cF(d_v1), cF(d_v2), n, *cF(prev_r), mF(h_qpoly), mF(h_r), mF(h_vr), mF(h_final));
}
int hobbit_sumcheck2_sparse(hobbit_ctx *ctx, const hobbit_F *d_v1, const uint64_t *d_idx, const hobbit_F *d_val, size_t m, size_t n, const hobbit_F *prev_r,
                            hobbit_F *h_qpoly, hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_final) {
    if (m > n) return ctx->fail(HOBBIT_EINVAL, "sumcheck2_sparse: more non-zeros than table entries");
    return launch_sumcheck2_sparse(ctx, cF(d_v1), d_idx, cF(d_val), m, n, *cF(prev_r), mF(h_qpoly), mF(h_r), mF(h_vr), mF(h_final));
}
int hobbit_sumcheck2_eq(hobbit_ctx *ctx, int T, const hobbit_F *h_r1, const hobbit_F *h_r2, const hobbit_F *h_a, const hobbit_F *d_v2, size_t n, const hobbit_F *prev_r,
                        hobbit_F *h_qpoly, hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_final) {
    if (!prev_r) return ctx->fail(HOBBIT_EINVAL, "sumcheck2_eq: null transcript seed");
    return launch_sumcheck2_eq(ctx, T, cF(h_r1), cF(h_r2), cF(h_a), cF(d_v2), n, *cF(prev_r), mF(h_qpoly), mF(h_r), mF(h_vr), mF(h_final));
}
int hobbit_gate_sumcheck(hobbit_ctx *ctx, const hobbit_F *d_add, const hobbit_F *d_beta, const hobbit_F *d_L, const hobbit_F *d_R, const hobbit_F *d_O, const hobbit_F *d_mul,
                         size_t n, const hobbit_F *h_a, hobbit_F *h_rand, hobbit_F *h_sum, hobbit_F *h_poly, hobbit_F *h_r, hobbit_F *h_final, int *h_check) {
    const F *tabs[6] = {cF(d_add), cF(d_beta), cF(d_L), cF(d_R), cF(d_O), cF(d_mul)};
    return launch_gate_sumcheck(ctx, tabs, n, cF(h_a), mF(h_rand), mF(h_sum), mF(h_poly), mF(h_r), mF(h_final), h_check);
}
int hobbit_sumcheck3(hobbit_ctx *ctx, const hobbit_F *d_v1, const hobbit_F *d_v2, const hobbit_F *d_v3, size_t n, const hobbit_F *prev_r,
                     hobbit_F *h_cpoly, hobbit_F *h_r, hobbit_F *h_vr, hobbit_F *h_final) {
    return launch_sumcheck3(ctx, cF(d_v1), cF(d_v2), cF(d_v3), n, *cF(prev_r), mF(h_cpoly), mF(h_r), mF(h_vr), mF(h_final));
}

// ---- Brakedown (src/Our_PC.cpp:197-236 commit_standard_brakedown, 432-520 open_brakedown_standard) --------------------------------------
int hobbit_encode_interleaved(hobbit_ctx *ctx, const hobbit_F *d_src, hobbit_F *d_dst, long long n, uint32_t rows) {
    if (n <= 0 || rows == 0 || (rows & (rows - 1)) || (size_t)2 * n * rows >= ((size_t)1 << 31))
        return ctx->fail(HOBBIT_EINVAL, "encode_interleaved: rows must be a power of two and 2 n rows < 2^31");
    if (ctx->code.n != n) return ctx->fail(HOBBIT_ESTATE, "encode_interleaved: graphs for this n are not finalized (hobbit_graph_finalize)");
    HB_TRY(ensure_ilv(ctx));
    return launch_encode_ilv(ctx, cF(d_src), mF(d_dst), rows);
}
struct hobbit_brakedown {
    hobbit_ctx *ctx;
    size_t N, B; uint32_t rows; long long len; int quirk;
    mem::Buf<F> d_mat; mem::Buf<uint8_t> d_levels;     // 2B columns x rows, element (i, c) at c * rows + i | flat levels over the 2B column digests
};
int hobbit_brakedown_shape(size_t N, size_t *B, uint32_t *rows) {
    const int n = ilog2_exact(N);
    if (n < 16 || n > 29) return HOBBIT_EINVAL;       // fewer than 4 rows below; B > 2^20 (the longest code hobbit_graph_finalize builds) above
    const size_t b = (size_t)1 << (n % 2 == 0 ? n / 2 + 6 : (n - 1) / 2 + 6);     // src/Our_PC.cpp:199-206
    if (B) *B = b;
    if (rows) *rows = (uint32_t)(N / b);
    return 0;
}
void hobbit_brakedown_free(hobbit_brakedown *c) {
    if (!c) return;
    hipStreamSynchronize(c->ctx->stream);
    delete c;
}
}  // extern "C"
// commit_standard_brakedown's body for `rows` messages of B elements (graphs for n = B finalized: the callers check); hobbit_brakedown_commit
// takes the shape from N, hobbit_brakingbase_commit (hobbit_brakingbase.hip) hands in B = N / K, rows = K
int hobbit::brakedown_commit_shape(hobbit_ctx *ctx, const F *d_poly, size_t B, uint32_t rows, int left_left_quirk, hobbit_brakedown **out) {
    *out = nullptr;
    HB_TRY(ensure_ilv(ctx));
    const size_t W = 2 * B;
    Handle<hobbit_brakedown, hobbit_brakedown_free> c(new hobbit_brakedown{ctx, B * rows, B, rows, ctx->code.len, left_left_quirk ? 1 : 0, {}, {}});
    if (c->d_mat.alloc(W * rows) || c->d_levels.alloc((2 * W - 1) * 32)) return ctx->fail(HOBBIT_ENOMEM, "brakedown_commit: device allocation failed");
    // row i of the message (poly[i B .. (i + 1) B)) becomes entry i of columns 0 .. B - 1; every row is then encoded in place (tensor[0][i])
    int r = launch_transpose(ctx, d_poly, 0, rows, (uint32_t)B, c->d_mat, 0, rows, 1);
    if (!r) r = launch_encode_ilv(ctx, c->d_mat, c->d_mat, rows);
    // MT_commit_Blake of every column -> level 0 (columns [len, 2B) are zero), then create_tree_blake over the 2B digests
    if (!r) r = launch_brakedown_digests(ctx, c->d_mat, rows, (size_t)c->len, W - (size_t)c->len, c->quirk, c->d_levels);
    if (!r) r = launch_merkle_levels(ctx, c->d_levels, W, c->quirk);
    if (r) return r;
    *out = c.release();
    return 0;
}
extern "C" {
int hobbit_brakedown_commit(hobbit_ctx *ctx, const hobbit_F *d_poly, size_t N, int left_left_quirk, hobbit_brakedown **out) {
    *out = nullptr;
    size_t B; uint32_t rows;
    if (hobbit_brakedown_shape(N, &B, &rows)) return ctx->fail(HOBBIT_EINVAL, "brakedown_commit: N must be 2^n with 16 <= n <= 29");
    if (ctx->code.n != (long long)B) return ctx->fail(HOBBIT_ESTATE, "brakedown_commit: graphs for n = B are not finalized (expander_init_store(B))");
    return brakedown_commit_shape(ctx, cF(d_poly), B, rows, left_left_quirk, out);
}
int hobbit_brakedown_dims(const hobbit_brakedown *c, size_t *B, uint32_t *rows, long long *len) {
    if (B) *B = c->B;
    if (rows) *rows = c->rows;
    if (len) *len = c->len;
    return 0;
}
const hobbit_F *hobbit_brakedown_matrix_dev(const hobbit_brakedown *c) { return reinterpret_cast<const hobbit_F *>(c->d_mat.get()); }
const uint8_t *hobbit_brakedown_levels_dev(const hobbit_brakedown *c) { return c->d_levels; }
int hobbit_brakedown_levels(hobbit_ctx *ctx, const hobbit_brakedown *c, uint8_t *h_levels) { return hobbit_memcpy_d2h(ctx, h_levels, c->d_levels, 32 * (4 * c->B - 1)); }
int hobbit_brakedown_root(hobbit_ctx *ctx, const hobbit_brakedown *c, uint8_t *h_root) { return hobbit_memcpy_d2h(ctx, h_root, c->d_levels + 32 * (4 * c->B - 2), 32); }
int hobbit_brakedown_tensor(hobbit_ctx *ctx, const hobbit_brakedown *c, size_t col_lo, size_t ncols, hobbit_F *h_out) {
    if (col_lo > 2 * c->B || ncols > 2 * c->B - col_lo) return ctx->fail(HOBBIT_EINVAL, "brakedown_tensor: columns out of range");
    if (!ncols) return 0;
    F *tmp; HB_TRY(ctx->workspace(ncols * c->rows * sizeof(F), (void **)&tmp));
    HB_TRY(launch_transpose(ctx, c->d_mat + col_lo * c->rows, 0, (uint32_t)ncols, c->rows, tmp, 0, ncols, 1));
    return hobbit_memcpy_d2h(ctx, h_out, tmp, ncols * c->rows * sizeof(F));
}
int hobbit_brakedown_open(hobbit_ctx *ctx, const hobbit_brakedown *c, const hobbit_F *h_x, const hobbit_F *h_r, const uint64_t *h_I, size_t nq,
                          hobbit_F *h_aggr_beta, hobbit_F *h_aggr_r, hobbit_F *h_reply, uint8_t *h_paths) {
    const size_t W = 2 * c->B, rows = c->rows;
    const int lr = ilog2_exact(rows), depth = ilog2_exact(W);
    for (size_t q = 0; q < nq; q++) if (h_I[q] >= W) return ctx->fail(HOBBIT_EINVAL, "brakedown_open: query out of range");
    StageScope sc(ctx);
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t b_rows = al(rows * sizeof(F)), b_aggr = al(c->B * sizeof(F)), b_rep = al(nq * rows * sizeof(F)), b_I = al(nq * 4), b_pos = al(nq * 8);
    uint8_t *ws;
    HB_TRY(ctx->workspace(2 * b_rows + 2 * b_aggr + b_rep + b_I + b_pos + al(nq * depth * 32) + 256, (void **)&ws));
    F *d_beta = reinterpret_cast<F *>(ws), *d_r = reinterpret_cast<F *>(ws + b_rows);
    F *d_ab = reinterpret_cast<F *>(ws + 2 * b_rows), *d_ar = reinterpret_cast<F *>(ws + 2 * b_rows + b_aggr);
    F *d_rep = reinterpret_cast<F *>(ws + 2 * b_rows + 2 * b_aggr);
    uint32_t *d_I = reinterpret_cast<uint32_t *>(ws + 2 * b_rows + 2 * b_aggr + b_rep);
    uint64_t *d_pos = reinterpret_cast<uint64_t *>(ws + 2 * b_rows + 2 * b_aggr + b_rep + b_I);
    uint8_t *d_paths = ws + 2 * b_rows + 2 * b_aggr + b_rep + b_I + b_pos;
    // beta1 = precompute_beta(x[0 .. log2 rows)); aggr_beta / aggr_r over the message columns j < B (src/Our_PC.cpp:447-457)
    if (h_aggr_beta || h_aggr_r) {
        HB_TRY(launch_eq_table(ctx, cF(h_x), lr, d_beta));
        HB_TRY(h2d_staged(ctx, d_r, h_r, rows * sizeof(F)));
        HB_TRY(launch_brakedown_aggr(ctx, c->d_mat, c->rows, c->B, d_beta, d_r, d_ab, d_ar));
        if (h_aggr_beta) HB_TRY(d2h_staged(ctx, h_aggr_beta, d_ab, c->B * sizeof(F)));
        if (h_aggr_r) HB_TRY(d2h_staged(ctx, h_aggr_r, d_ar, c->B * sizeof(F)));
    }
    if (nq && h_reply) {                                   // reply[q][i] = T[i][I[q]] (:462-468)
        std::vector<uint32_t> I32(h_I, h_I + nq);
        HB_TRY(h2d_staged(ctx, d_I, I32.data(), nq * 4));
        HB_TRY(launch_brakedown_reply(ctx, c->d_mat, c->rows, d_I, nq, d_rep));
        HB_TRY(d2h_staged(ctx, h_reply, d_rep, nq * rows * sizeof(F)));
    }
    if (nq && h_paths) {
        // open_tree_blake(MT, {0, I[q]}, 0) (:471-475) takes leaf (I[q] / 4) * 0 + 0: every path is leaf 0's
        std::vector<uint64_t> pos(nq);
        for (size_t q = 0; q < nq; q++) pos[q] = (h_I[q] / 4) * 0 + 0;
        HB_TRY(h2d_staged(ctx, d_pos, pos.data(), nq * 8));
        HB_TRY(launch_merkle_paths(ctx, c->d_levels, W, d_pos, nq, depth, d_paths));
        HB_TRY(d2h_staged(ctx, h_paths, d_paths, nq * depth * 32));
    }
    return sc.finish();
}

// ---- streaming Brakedown (src/Elastic_PC.cpp:112-172 commit_brakedown_stream, 287-313, 561-623 open_brakedown_stream) -------------------
// The host owns the stream and pushes B-element device chunks.  Both objects hold one group of four chunks as a 2B x 4 rows-innermost
// matrix and nothing that grows with the number of chunks pushed: `bytes` counts every device byte they allocate.
int hobbit_brakedown_stream_shape(size_t N, size_t *B, uint32_t *chunks) {
    const int n = ilog2_exact(N);
    if (n < 16 || n > 30) return HOBBIT_EINVAL;       // chunks <= 4 below ("Decrease buffer size", :113); B > 2^20 above
    const size_t b = (size_t)1 << ((n - 1) / 2 + 6);  // :785-791: n odd 2^(n/2+6), n even 2^((n-1)/2+6)
    if (B) *B = b;
    if (chunks) *chunks = (uint32_t)(N / b);
    return 0;
}
struct hobbit_brakedown_stream {
    hobbit_ctx *ctx; size_t B; long long len; int shift; size_t count; bool finished;
    mem::Pooled<F> d_mat; mem::Pooled<uint8_t> state;      // 2B columns x 4 rows | the 2B running leaves
};
void hobbit_brakedown_stream_free(hobbit_brakedown_stream *s) { delete s; }
int hobbit_brakedown_stream_begin(hobbit_ctx *ctx, size_t B, int gcc_arg_order, hobbit_brakedown_stream **out) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    if (ilog2_exact(B) < 0 || B > ((size_t)1 << 20)) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_begin: B must be a power of two, at most 2^20");
    if (ctx->code.n != (long long)B) return ctx->fail(HOBBIT_ESTATE, "brakedown_stream_begin: graphs for n = B are not finalized (expander_init_store(B))");
    HB_TRY(ensure_ilv(ctx));
    Handle<hobbit_brakedown_stream, hobbit_brakedown_stream_free> s(new hobbit_brakedown_stream{ctx, B, ctx->code.len, gcc_arg_order ? 1 : 0, 0, false, {}, {}});
    if (ctx->pool_get(8 * B * sizeof(F), s->d_mat) || ctx->pool_get(2 * B * 32, s->state)) return ctx->fail(HOBBIT_ENOMEM, "brakedown_stream_begin: allocation failed");
    HB_TRY(launch_zero(ctx, s->state, 2 * B * 32));       // buff_hash starts at zero (:125-130)
    *out = s.release();
    return 0;
}
size_t hobbit_brakedown_stream_device_bytes(const hobbit_brakedown_stream *s) { return s->d_mat.bytes() + s->state.bytes(); }
int hobbit_brakedown_stream_push(hobbit_ctx *ctx, hobbit_brakedown_stream *s, const hobbit_F *d_chunk) {
    if (s->finished) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_push: the commitment is finished");
    if (ctx->code.n != (long long)s->B) return ctx->fail(HOBBIT_ESTATE, "brakedown_stream_push: graphs for n = B are not finalized");
    const uint32_t slot = (uint32_t)(s->count % 4);
    HB_TRY(launch_bds_put(ctx, cF(d_chunk), s->B, slot, s->d_mat));
    if (slot == 3) {                                       // the group is complete: encode its four rows, chain them into the leaves (:139-150)
        HB_TRY(launch_encode_ilv(ctx, s->d_mat, s->d_mat, 4));
        HB_TRY(launch_bds_leaf(ctx, s->d_mat, (size_t)s->len, 2 * s->B, s->shift, s->state));
    }
    s->count++;
    return 0;
}
int hobbit_brakedown_stream_finish(hobbit_ctx *ctx, hobbit_brakedown_stream *s, int left_left_quirk, uint8_t *d_levels) {
    if (s->finished) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_finish: already finished");
    if (s->count % 4 || s->count <= 4) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_finish: the number of chunks must be a multiple of 4 above 4");
    HB_TRY(launch_copy(ctx, d_levels, s->state, 2 * s->B * 32));
    HB_TRY(launch_merkle_levels(ctx, d_levels, 2 * s->B, left_left_quirk ? 1 : 0));     // create_tree_blake(2B, ..) (:171)
    s->finished = true;
    return 0;
}

struct hobbit_brakedown_stream_open {
    hobbit_ctx *ctx; size_t B, chunks, nq; long long len; size_t n_aggr, n_reply;
    mem::Pooled<F> d_mat, d_ab, d_ar, d_w, d_reply; mem::Pooled<uint32_t> d_I;      // d_w: beta (chunks F) then r_v (chunks F)
};
void hobbit_brakedown_stream_open_free(hobbit_brakedown_stream_open *o) { delete o; }
int hobbit_brakedown_stream_open_begin(hobbit_ctx *ctx, size_t B, size_t chunks, const hobbit_F *h_beta, const hobbit_F *h_rv, const uint64_t *h_I, size_t nq,
                                       hobbit_brakedown_stream_open **out) {
    if (!out) return HOBBIT_EINVAL;
    *out = nullptr;
    if (ilog2_exact(B) < 0 || B > ((size_t)1 << 20)) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_open_begin: B must be a power of two, at most 2^20");
    if (chunks % 4 || chunks <= 4) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_open_begin: the number of chunks must be a multiple of 4 above 4");
    if (!h_beta || !h_rv || (nq && !h_I)) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_open_begin: null input");
    for (size_t q = 0; q < nq; q++) if (h_I[q] >= 2 * B) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_open_begin: query out of range");
    if (ctx->code.n != (long long)B) return ctx->fail(HOBBIT_ESTATE, "brakedown_stream_open_begin: graphs for n = B are not finalized (expander_init_store(B))");
    HB_TRY(ensure_ilv(ctx));
    Handle<hobbit_brakedown_stream_open, hobbit_brakedown_stream_open_free> o(new hobbit_brakedown_stream_open());
    o->ctx = ctx; o->B = B; o->chunks = chunks; o->nq = nq; o->len = ctx->code.len; o->n_aggr = o->n_reply = 0;
    if (ctx->pool_get(8 * B * sizeof(F), o->d_mat) || ctx->pool_get(B * sizeof(F), o->d_ab) || ctx->pool_get(B * sizeof(F), o->d_ar) || ctx->pool_get(2 * chunks * sizeof(F), o->d_w) ||
        ctx->pool_get((nq ? nq : 1) * chunks * sizeof(F), o->d_reply) || ctx->pool_get((nq ? nq : 1) * 4, o->d_I))
        return ctx->fail(HOBBIT_ENOMEM, "brakedown_stream_open_begin: allocation failed");
    StageScope sc(ctx);
    int r = h2d_staged(ctx, o->d_w, h_beta, chunks * sizeof(F));
    if (!r) r = h2d_staged(ctx, o->d_w + chunks, h_rv, chunks * sizeof(F));
    if (!r && nq) { std::vector<uint32_t> I32(h_I, h_I + nq); r = h2d_staged(ctx, o->d_I, I32.data(), nq * 4); }
    if (!r) r = launch_zero(ctx, o->d_ab, B * sizeof(F));
    if (!r) r = launch_zero(ctx, o->d_ar, B * sizeof(F));
    if (!r) r = sc.finish();
    if (r) return r;
    *out = o.release();
    return 0;
}
size_t hobbit_brakedown_stream_open_device_bytes(const hobbit_brakedown_stream_open *o) {
    return o->d_mat.bytes() + o->d_ab.bytes() + o->d_ar.bytes() + o->d_w.bytes() + o->d_reply.bytes() + o->d_I.bytes();
}
int hobbit_brakedown_stream_open_aggregate_push(hobbit_ctx *ctx, hobbit_brakedown_stream_open *o, const hobbit_F *d_chunk) {
    if (o->n_aggr >= o->chunks) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_open_aggregate_push: more chunks than the opening was begun with");
    const uint32_t slot = (uint32_t)(o->n_aggr % 4);
    HB_TRY(launch_bds_put(ctx, cF(d_chunk), o->B, slot, o->d_mat));
    if (slot == 3) HB_TRY(launch_bds_aggr(ctx, o->d_mat, o->B, o->d_w + (o->n_aggr - 3), o->d_w + o->chunks + (o->n_aggr - 3), o->d_ab, o->d_ar));
    o->n_aggr++;
    return 0;
}
int hobbit_brakedown_stream_open_reply_push(hobbit_ctx *ctx, hobbit_brakedown_stream_open *o, const hobbit_F *d_chunk) {
    if (o->n_reply >= o->chunks) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_open_reply_push: more chunks than the opening was begun with");
    if (ctx->code.n != (long long)o->B) return ctx->fail(HOBBIT_ESTATE, "brakedown_stream_open_reply_push: graphs for n = B are not finalized");
    const uint32_t slot = (uint32_t)(o->n_reply % 4);
    HB_TRY(launch_bds_put(ctx, cF(d_chunk), o->B, slot, o->d_mat));
    if (slot == 3) {
        HB_TRY(launch_encode_ilv(ctx, o->d_mat, o->d_mat, 4));
        HB_TRY(launch_bds_reply(ctx, o->d_mat, o->d_I, o->nq, o->chunks, o->n_reply - 3, o->d_reply));
    }
    o->n_reply++;
    return 0;
}
int hobbit_brakedown_stream_open_finish(hobbit_ctx *ctx, hobbit_brakedown_stream_open *o, const uint8_t *d_levels, hobbit_F *h_aggr_beta, hobbit_F *h_aggr_r,
                                        hobbit_F *h_reply, uint8_t *h_paths) {
    if ((h_aggr_beta || h_aggr_r) && o->n_aggr != o->chunks) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_open_finish: the aggregate pass is incomplete");
    if (h_reply && o->nq && o->n_reply != o->chunks) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_open_finish: the reply pass is incomplete");
    if (h_paths && o->nq && !d_levels) return ctx->fail(HOBBIT_EINVAL, "brakedown_stream_open_finish: paths need the commitment's levels");
    StageScope sc(ctx);
    if (h_aggr_beta) HB_TRY(d2h_staged(ctx, h_aggr_beta, o->d_ab, o->B * sizeof(F)));
    if (h_aggr_r) HB_TRY(d2h_staged(ctx, h_aggr_r, o->d_ar, o->B * sizeof(F)));
    if (h_reply && o->nq) HB_TRY(d2h_staged(ctx, h_reply, o->d_reply, o->nq * o->chunks * sizeof(F)));
    if (h_paths && o->nq) {
        // open_tree_blake(MT, {0, I[q]}, 0) (:583-587) takes leaf (I[q] / 4) * 0 + 0: every path is leaf 0's
        const size_t W = 2 * o->B; const int depth = ilog2_exact(W);
        std::vector<uint64_t> pos(o->nq, 0);
        uint8_t *buf; const size_t pb = ((o->nq * 8 + 255) / 256) * 256;
        HB_TRY(ctx->workspace(pb + o->nq * depth * 32 + 64, (void **)&buf));
        HB_TRY(h2d_staged(ctx, buf, pos.data(), o->nq * 8));
        HB_TRY(launch_merkle_paths(ctx, d_levels, W, reinterpret_cast<const uint64_t *>(buf), o->nq, depth, buf + pb));
        HB_TRY(d2h_staged(ctx, h_paths, buf + pb, o->nq * depth * 32));
    }
    return sc.finish();
}

}  // extern "C"
