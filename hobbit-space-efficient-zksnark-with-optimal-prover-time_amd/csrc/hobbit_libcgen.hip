// hobbit_libcgen.hip -- the libc random stream on the device (include/hobbit_libcgen.h; arithmetic and state layout: hobbit_libcgen.hpp).
//
// One workgroup covers SPAN consecutive draws, each of its LANES lanes a run of RUN consecutive ones:
//   1. the workgroup's window: the call's window carried on by (workgroup index) x (stride of the kernel), one application of the COARSE table's
//      x^(stride 2^b) per set bit b of the index, 31 lanes computing one word each over the window and its 30 following words in LDS;
//   2. lane l's window: one application of the LANE table's x^(l RUN) to the workgroup's window, in registers;
//   3. RUN draws over a 31-word ring in registers (unrolled, so every ring index is static), written to an LDS tile with an odd lane pitch
//      (ds_write_b32 has 32 banks: pitch 125 is conflict-free);
//   4. the kernel's output, each lane one element per sweep from the tile: consecutive lanes store consecutive 4, 8 or 16 bytes.
// The squarings are the host's (the tables are built once per context); no lane repeats them.  The draws cost a few instructions each and the
// kernels are bound by their stores; the tile (64 000 bytes) allows two workgroups per CU.
#include <vector>
#include "hobbit_kernels.hpp"
#include "hobbit_dev.hpp"
#include "hobbit_libcgen.hpp"
#include "../../include/hobbit_libcgen.h"
#include "../../include/hobbit_real.h"

using namespace hobbit;

namespace {
constexpr int DEG = libcgen::DEG;
constexpr uint32_t LANES = 128, RUN = 4 * DEG, PITCH = RUN + 1, SPAN = LANES * RUN, NBITS = 32;
// generate_randomness: 101 draws make 100 elements, so its workgroups step by whole groups and leave the tile's last SPAN - GR_DRAWS draws unused
constexpr uint32_t GR_GROUPS = SPAN / 101, GR_DRAWS = 101 * GR_GROUPS, GR_ELEMS = 100 * GR_GROUPS;
constexpr uint32_t GL_EDGES = SPAN / 2;                     // a graph level: two draws per edge
// ctx->libcgen_tab: lane table [31][LANES] | coarse table of stride SPAN [NBITS][31] | coarse table of stride GR_DRAWS [NBITS][31]
constexpr size_t TAB_LANE = 0, TAB_SPAN = (size_t)DEG * LANES, TAB_GR = TAB_SPAN + (size_t)NBITS * DEG, TAB_WORDS = TAB_GR + (size_t)NBITS * DEG;
static_assert(RUN % DEG == 0 && SPAN % 2 == 0 && LANES >= 2 * DEG, "libcgen kernel shape");

struct Window { uint32_t w[DEG]; };

// ext[31 + t] = ext[28 + t] + ext[t] for t < 30, every lane its own word from the window alone
__device__ __forceinline__ void extend_lds(uint32_t *ext, uint32_t t) {
    if (t < DEG - 1) {
        uint32_t s = ext[DEG - 3 + t % 3];
        for (uint32_t u = t % 3; u <= t; u += 3) s += ext[u];
        ext[DEG + t] = s;
    }
}
__device__ __forceinline__ uint32_t tile_at(const uint32_t *tile, uint32_t q) { return tile[q + q / RUN]; }

// draws [wg * stride, wg * stride + SPAN) of window w0 into the tile: draw q at tile[q + q / RUN].  Ends with a barrier.
__device__ __forceinline__ void wg_draws(const Window &w0, const uint32_t *__restrict__ coarse, const uint32_t *__restrict__ lane_tab, uint32_t wg, uint32_t *tile, uint32_t *ext) {
    const uint32_t t = threadIdx.x;
    if (t < DEG) {
        uint32_t v = 0;
#pragma unroll
        for (int j = 0; j < DEG; j++) if (t == (uint32_t)j) v = w0.w[j];
        ext[t] = v;
    }
    __syncthreads();
    for (int b = 0; b < (int)NBITS && (wg >> b) != 0; b++) {          // (uniform over the workgroup)
        if (!((wg >> b) & 1)) continue;
        extend_lds(ext, t);
        __syncthreads();
        uint32_t acc = 0;
        if (t < DEG) for (int j = 0; j < DEG; j++) acc += coarse[b * DEG + j] * ext[t + j];
        __syncthreads();
        if (t < DEG) ext[t] = acc;
        __syncthreads();
    }
    extend_lds(ext, t);
    __syncthreads();
    uint32_t e[2 * DEG - 1], r[DEG];
#pragma unroll
    for (int i = 0; i < 2 * DEG - 1; i++) e[i] = ext[i];
#pragma unroll
    for (int i = 0; i < DEG; i++) r[i] = 0;
#pragma unroll
    for (int j = 0; j < DEG; j++) {
        const uint32_t p = lane_tab[j * LANES + t];
#pragma unroll
        for (int i = 0; i < DEG; i++) r[i] += p * e[i + j];
    }
    uint32_t *mine = tile + t * PITCH;
#pragma unroll
    for (int it = 0; it < (int)(RUN / DEG); it++) {
#pragma unroll
        for (int j = 0; j < DEG; j++) { r[j] += r[(j + DEG - 3) % DEG]; mine[it * DEG + j] = r[j] >> 1; }
    }
    __syncthreads();
}

__global__ __launch_bounds__(LANES) void k_libc_draws(Window w0, const uint32_t *__restrict__ tab, uint32_t *__restrict__ out, uint64_t n) {
    __shared__ uint32_t tile[LANES * PITCH]; __shared__ uint32_t ext[64];
    wg_draws(w0, tab + TAB_SPAN, tab + TAB_LANE, blockIdx.x, tile, ext);
    const uint64_t base = (uint64_t)blockIdx.x * SPAN;
    const uint32_t cnt = (uint32_t)(n - base < SPAN ? n - base : SPAN);
    for (uint32_t q = threadIdx.x; q < cnt; q += LANES) out[base + q] = tile_at(tile, q);
}

// src/utils.cpp:873-883: element i = F(draw 101 (i / 100)) + F(draw 101 (i / 100) + 1 + i % 100); both below 2^31, so the sum needs no reduction
__global__ __launch_bounds__(LANES) void k_libc_randomness(Window w0, const uint32_t *__restrict__ tab, F *__restrict__ out, uint64_t n) {
    __shared__ uint32_t tile[LANES * PITCH]; __shared__ uint32_t ext[64];
    wg_draws(w0, tab + TAB_GR, tab + TAB_LANE, blockIdx.x, tile, ext);
    const uint64_t base = (uint64_t)blockIdx.x * GR_ELEMS;
    const uint32_t cnt = (uint32_t)(n - base < GR_ELEMS ? n - base : GR_ELEMS);
    for (uint32_t i = threadIdx.x; i < cnt; i += LANES) {
        const uint32_t g = i / 100, d = 101 * g;
        stF(out + base + i, fmake((uint64_t)tile_at(tile, d) + tile_at(tile, d + 1 + (i - 100 * g))));
    }
}

// the same elements as reals: img is 0 in this stream, so 8 bytes per value say everything (include/hobbit_real.h)
__global__ __launch_bounds__(LANES) void k_libc_randomness_real(Window w0, const uint32_t *__restrict__ tab, uint64_t *__restrict__ out, uint64_t n) {
    __shared__ uint32_t tile[LANES * PITCH]; __shared__ uint32_t ext[64];
    wg_draws(w0, tab + TAB_GR, tab + TAB_LANE, blockIdx.x, tile, ext);
    const uint64_t base = (uint64_t)blockIdx.x * GR_ELEMS;
    const uint32_t cnt = (uint32_t)(n - base < GR_ELEMS ? n - base : GR_ELEMS);
    for (uint32_t i = threadIdx.x; i < cnt; i += LANES) {
        const uint32_t g = i / 100, d = 101 * g;
        out[base + i] = (uint64_t)tile_at(tile, d) + tile_at(tile, d + 1 + (i - 100 * g));
    }
}

// src/expanders.h:20-47: edge e takes target = rand() % R, weight = random()
__global__ __launch_bounds__(LANES) void k_libc_graph_level(Window w0, const uint32_t *__restrict__ tab, uint32_t R, long long *__restrict__ nbr, F *__restrict__ wt, uint64_t edges) {
    __shared__ uint32_t tile[LANES * PITCH]; __shared__ uint32_t ext[64];
    wg_draws(w0, tab + TAB_SPAN, tab + TAB_LANE, blockIdx.x, tile, ext);
    const uint64_t base = (uint64_t)blockIdx.x * GL_EDGES;
    const uint32_t cnt = (uint32_t)(edges - base < GL_EDGES ? edges - base : GL_EDGES);
    for (uint32_t i = threadIdx.x; i < cnt; i += LANES) {
        nbr[base + i] = (long long)(tile_at(tile, 2 * i) % R);
        stF(wt + base + i, fmake((uint64_t)tile_at(tile, 2 * i + 1)));
    }
}

int tables(hobbit_ctx *ctx, const uint32_t **tab) {
    if (!ctx->libcgen_tab) {
        std::vector<uint32_t> h(TAB_WORDS);
        libcgen::lane_table(RUN, LANES, &h[TAB_LANE]); libcgen::coarse_table(SPAN, NBITS, &h[TAB_SPAN]); libcgen::coarse_table(GR_DRAWS, NBITS, &h[TAB_GR]);
        mem::Buf<uint32_t> d;
        if (d.alloc(TAB_WORDS)) return ctx->fail(HOBBIT_ENOMEM, "libc stream: table allocation failed");
        HB_CHECK(ctx, hipMemcpy(d.get(), h.data(), TAB_WORDS * sizeof(uint32_t), hipMemcpyHostToDevice));       // once per context
        ctx->libcgen_tab = std::move(d);
    }
    *tab = ctx->libcgen_tab.get();
    return 0;
}
// the window `first` draws on, as the kernels' argument; the workgroup count of `items` at `per` per workgroup
Window window_at(const uint32_t w[DEG], uint64_t first) { Window r; libcgen::jump(w, first, r.w); return r; }
int grid_of(hobbit_ctx *ctx, uint64_t items, uint32_t per, uint32_t *grid) {
    const uint64_t g = (items + per - 1) / per;
    if (g >= ((uint64_t)1 << 31)) return ctx->fail(HOBBIT_EINVAL, "libc stream: count beyond 2^31 workgroups");
    *grid = (uint32_t)g; return 0;
}
int launch_draws(hobbit_ctx *ctx, const uint32_t w[DEG], uint64_t first, size_t n, uint32_t *d_out) {
    const uint32_t *tab; uint32_t grid;
    HB_TRY(tables(ctx, &tab)); HB_TRY(grid_of(ctx, n, SPAN, &grid));
    HB_LAUNCH(ctx, "k_libc_draws", k_libc_draws, dim3(grid), dim3(LANES), 0, window_at(w, first), tab, d_out, (uint64_t)n);
    return 0;
}
int launch_randomness(hobbit_ctx *ctx, const uint32_t w[DEG], size_t n, F *d_out) {
    const uint32_t *tab; uint32_t grid;
    HB_TRY(tables(ctx, &tab)); HB_TRY(grid_of(ctx, n, GR_ELEMS, &grid));
    HB_LAUNCH(ctx, "k_libc_randomness", k_libc_randomness, dim3(grid), dim3(LANES), 0, window_at(w, 0), tab, d_out, (uint64_t)n);
    return 0;
}
int launch_randomness_real(hobbit_ctx *ctx, const uint32_t w[DEG], size_t n, uint64_t *d_out) {
    const uint32_t *tab; uint32_t grid;
    HB_TRY(tables(ctx, &tab)); HB_TRY(grid_of(ctx, n, GR_ELEMS, &grid));
    HB_LAUNCH(ctx, "k_libc_randomness_real", k_libc_randomness_real, dim3(grid), dim3(LANES), 0, window_at(w, 0), tab, d_out, (uint64_t)n);
    return 0;
}
int launch_graph_level(hobbit_ctx *ctx, const uint32_t w[DEG], uint64_t first, uint64_t edges, uint32_t R, long long *d_nbr, F *d_w) {
    const uint32_t *tab; uint32_t grid;
    HB_TRY(tables(ctx, &tab)); HB_TRY(grid_of(ctx, edges, GL_EDGES, &grid));
    HB_LAUNCH(ctx, "k_libc_graph_level", k_libc_graph_level, dim3(grid), dim3(LANES), 0, window_at(w, first), tab, R, d_nbr, d_w, edges);
    return 0;
}
bool level_dims_ok(long long L, long long R, int degree) { return L > 0 && R > 0 && R < (1LL << 31) && degree > 0 && degree <= 4096 && L <= (1LL << 40) / degree; }
const char *const NOT_TYPE3 = "the process generator is not glibc's TYPE_3 (initstate with another buffer size)";
}  // namespace

extern "C" {

int hobbit_libc_window(uint32_t w[31]) { return w && libcgen::snapshot(w) == 0 ? 0 : HOBBIT_ESTATE; }
int hobbit_libc_set_window(const uint32_t w[31]) {
    uint32_t cur[DEG];
    if (!w || libcgen::snapshot(cur) != 0) return HOBBIT_ESTATE;          // (a caller's state of another type is not replaced)
    return libcgen::write_back(w) == 0 ? 0 : HOBBIT_ESTATE;
}
int hobbit_libc_advance(uint64_t k) {
    uint32_t w[DEG];
    if (libcgen::snapshot(w) != 0) return HOBBIT_ESTATE;
    if (!k) return 0;
    libcgen::jump(w, k, w);
    return libcgen::write_back(w) == 0 ? 0 : HOBBIT_ESTATE;
}
void hobbit_libc_jump(const uint32_t w[31], uint64_t k, uint32_t out[31]) { libcgen::jump(w, k, out); }
void hobbit_libc_draws_shape(size_t *run_length, size_t *workgroup_span) { if (run_length) *run_length = RUN; if (workgroup_span) *workgroup_span = SPAN; }

int hobbit_libc_draws_dev(hobbit_ctx *ctx, const uint32_t w[31], uint64_t first, size_t n, uint32_t *d_out) {
    if (!w || (n && !d_out)) return ctx->fail(HOBBIT_EINVAL, "libc_draws_dev: null argument");
    if (!n) return 0;
    libcgen::Guard guard;                                                 // (a first launch loads this file's code object)
    return launch_draws(ctx, w, first, n, d_out);
}
int hobbit_libc_graph_level_dev(hobbit_ctx *ctx, const uint32_t w[31], uint64_t first, long long L, long long R, int degree, long long *d_nbr, hobbit_F *d_w) {
    if (!w || !d_nbr || !d_w) return ctx->fail(HOBBIT_EINVAL, "libc_graph_level_dev: null argument");
    if (!level_dims_ok(L, R, degree)) return ctx->fail(HOBBIT_EINVAL, "libc_graph_level_dev: bad dims (0 < R < 2^31)");
    libcgen::Guard guard;
    return launch_graph_level(ctx, w, first, (uint64_t)L * degree, (uint32_t)R, d_nbr, reinterpret_cast<F *>(d_w));
}
int hobbit_generate_randomness_dev(hobbit_ctx *ctx, size_t n, hobbit_F *d_out) {
    uint32_t w[DEG];
    if (libcgen::snapshot(w) != 0) return ctx->fail(HOBBIT_ESTATE, std::string("generate_randomness_dev: ") + NOT_TYPE3);
    if (!n) return 0;
    if (!d_out) return ctx->fail(HOBBIT_EINVAL, "generate_randomness_dev: null output");
    {
        libcgen::Guard guard;
        HB_TRY(launch_randomness(ctx, w, n, reinterpret_cast<F *>(d_out)));
    }
    libcgen::jump(w, (uint64_t)n + (n + 99) / 100, w);
    return libcgen::write_back(w) == 0 ? 0 : ctx->fail(HOBBIT_ESTATE, "generate_randomness_dev: setstate failed");
}
int hobbit_generate_randomness_real_dev(hobbit_ctx *ctx, size_t n, uint64_t *d_out) {
    uint32_t w[DEG];
    if (libcgen::snapshot(w) != 0) return ctx->fail(HOBBIT_ESTATE, std::string("generate_randomness_real_dev: ") + NOT_TYPE3);
    if (!n) return 0;
    if (!d_out) return ctx->fail(HOBBIT_EINVAL, "generate_randomness_real_dev: null output");
    {
        libcgen::Guard guard;
        HB_TRY(launch_randomness_real(ctx, w, n, d_out));
    }
    libcgen::jump(w, (uint64_t)n + (n + 99) / 100, w);
    return libcgen::write_back(w) == 0 ? 0 : ctx->fail(HOBBIT_ESTATE, "generate_randomness_real_dev: setstate failed");
}
int hobbit_graph_draw(hobbit_ctx *ctx, long long n, long long *codeword_len) {
    if (n <= 0 || n > (1LL << CODE_MAX_LOG)) return ctx->fail(HOBBIT_EINVAL, "graph_draw: bad n");
    uint32_t w[DEG];
    if (libcgen::snapshot(w) != 0) return ctx->fail(HOBBIT_ESTATE, std::string("graph_draw: ") + NOT_TYPE3);
    // src/expanders.h:78-92 with the doubles of src/parameter.h: C[dep] is n x (long long)(0.211 n) of degree 9, D[dep] is L x (long long)(n (1.72 - 1) - L) of
    // degree 12, L the codeword length of the level below; the recursion draws C[0], C[1], ... on its way down and D[last], ..., D[0] on its way up
    const double alpha = 0.211, r = 1.72;
    struct Level { int dep, kind; long long L, R; int degree; };
    std::vector<Level> order; std::vector<long long> nd{n};
    while (nd.back() > 13) { const long long m = nd.back(); order.push_back({(int)nd.size() - 1, 0, m, (long long)(alpha * m), 9}); nd.push_back((long long)(alpha * m)); }
    long long len = nd.back();
    for (int d = (int)nd.size() - 2; d >= 0; d--) { const long long R = (long long)(nd[d] * (r - 1) - len); order.push_back({d, 1, len, R, 12}); len = nd[d] + len + R; }
    for (const Level &l : order) if (!level_dims_ok(l.L, l.R, l.degree)) return ctx->fail(HOBBIT_EINVAL, "graph_draw: a level of this n has no nodes on one side");
    HB_TRY(hobbit_graph_reset(ctx));
    uint64_t first = 0;
    {
        libcgen::Guard guard;
        for (const Level &l : order) {
            const size_t E = (size_t)l.L * l.degree;
            Scratch sc(ctx);                                              // (one level's arrays at a time: 450 MB for C[0] of n = 2^21)
            void *d_nbr, *d_w;
            HB_TRY(sc.get(E * sizeof(long long), &d_nbr)); HB_TRY(sc.get(E * sizeof(F), &d_w));
            HB_TRY(launch_graph_level(ctx, w, first, E, (uint32_t)l.R, (long long *)d_nbr, (F *)d_w));
            HostGraph g; g.L = l.L; g.R = l.R; g.degree = l.degree; g.nbr.resize(E); g.w.resize(E);
            HB_TRY(hobbit_memcpy_d2h(ctx, g.nbr.data(), d_nbr, E * sizeof(long long)));
            HB_TRY(hobbit_memcpy_d2h(ctx, g.w.data(), d_w, E * sizeof(F)));
            ctx->graphs[{l.dep, l.kind}] = std::move(g);
            ctx->graph_gen++;
            first += 2 * (uint64_t)E;
        }
        long long got = 0;
        HB_TRY(hobbit_graph_finalize(ctx, n, &got));
        if (got != len) return ctx->fail(HOBBIT_ESTATE, "graph_draw: codeword length out of step with the level sizes");
    }
    libcgen::jump(w, first, w);
    if (libcgen::write_back(w) != 0) return ctx->fail(HOBBIT_ESTATE, "graph_draw: setstate failed");
    if (codeword_len) *codeword_len = len;
    return 0;
}
int hobbit_graph_level_host(hobbit_ctx *ctx, int dep, int kind, long long *L, long long *R, int *degree, const long long **h_nbr, const hobbit_F **h_w) {
    auto it = ctx->graphs.find({dep, kind});
    if (it == ctx->graphs.end()) return ctx->fail(HOBBIT_ESTATE, "graph_level_host: no such level in the graph store");
    const HostGraph &g = it->second;
    if (L) *L = g.L; if (R) *R = g.R; if (degree) *degree = g.degree;
    if (h_nbr) *h_nbr = g.nbr.data();
    if (h_w) *h_w = reinterpret_cast<const hobbit_F *>(g.w.data());
    return 0;
}

}  // extern "C"
