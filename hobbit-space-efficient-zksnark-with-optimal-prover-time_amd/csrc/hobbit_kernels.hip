// hobbit_kernels.hip -- gfx950 kernels of the HOBBIT prover hot path and their launchers.
//
// All kernels are integer (F_{p^2}, p = 2^61-1) or hash work: no MFMA.  The streaming kernels
// (fold, aggregate, leaf chain, tree levels) are HBM-bound and use 16-byte-per-lane coalesced
// accesses; the FFT and the expander encode keep a whole row / codeword in LDS (64 KB / <=110 KB
// of the CU's 160 KB; longer codewords stream their outer steps through 64 KB tiles, k_enc_tiled)
// and are bound by the v_mad_u64_u32 rate.
#include "hobbit_kernels.hpp"
#include "hobbit_dev.hpp"
#include "hobbit_blake3.hpp"
#include <vector>

namespace hobbit {
// ============================================================================================
// small utilities
// ============================================================================================
__global__ void k_f_binop(int op, const F *a, const F *b, F *o, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        F x = ldF(a + i), y = ldF(b + i);
        stF(o + i, op == 0 ? fadd(x, y) : op == 1 ? fsub(x, y) : fmul(x, y));
    }
}
__device__ __forceinline__ uint64_t splitmix(uint64_t seed, uint64_t idx) {
    uint64_t z = seed * 0x632BE59BD9B4E019ULL + idx * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
__global__ void k_fill_splitmix(F *o, size_t n, uint64_t seed) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        stF(o + i, fmake(splitmix(seed, 2 * i + 1) % P61, splitmix(seed, 2 * i + 2) % P61));
}

int launch_f_binop(hobbit_ctx *ctx, int op, const F *a, const F *b, F *o, size_t n) {
    HB_LAUNCH(ctx, "k_f_binop", k_f_binop, dim3(grid_for(n, 256)), dim3(256), 0, op, a, b, o, n);
    return 0;
}
// Multi-GPU aggregate exchange (parallel.sharded_open): the per-rank partial aggregates are summed by a plain 64-bit integer all-reduce -- field
// elements are < 2^61, so up to eight of them add up without leaving 64 bits -- and reduced mod p afterwards.  fold == 0: w += bias (the
// partials are shifted by -2^60 first, so that a SIGNED 64-bit sum cannot overflow either); fold != 0: w = (w + bias) mod p, canonical.
__global__ void k_u64_bias_fold(uint64_t *w, size_t n, uint64_t bias, int fold) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint64_t x = w[i] + bias;
        if (fold) { x = (x & P61) + (x >> 61); x = x >= P61 ? x - P61 : x; }
        w[i] = x;
    }
}
int launch_u64_bias_fold(hobbit_ctx *ctx, uint64_t *w, size_t n, uint64_t bias, int fold) {
    HB_LAUNCH(ctx, "k_u64_bias_fold", k_u64_bias_fold, dim3(grid_for(n, 256, 8192)), dim3(256), 0, w, n, bias, fold);
    return 0;
}
int launch_fill_splitmix(hobbit_ctx *ctx, F *o, size_t n, uint64_t seed) {
    HB_LAUNCH(ctx, "k_fill_splitmix", k_fill_splitmix, dim3(grid_for(n, 256)), dim3(256), 0, o, n, seed);
    return 0;
}

// ============================================================================================
// Expander encode (src/linear_code_encode.h:62-119), one workgroup per message, the whole
// codeword in LDS.  The recursion unrolls into a straight sequence of SpMV steps over one buffer
//   [x_0 | x_1 = C_0 x_0 | ... | x_D | z_{D-1} = D_{D-1} cw_D | ... | z_0 = D_0 cw_1]
// (the reference places the child codeword at dst+n and the D output behind it), executed in
// gather form (reverse adjacency: no atomics, deterministic, one writer per output).
// ============================================================================================
// Sliced-ELL geometry of one SpMV step: a slice is ENC_SW consecutive outputs; a wavefront owns a
// slice and splits each output's in-edges over ENC_SPLIT = 64/ENC_SW lane groups (lane l works on
// output l % ENC_SW, edges k = l / ENC_SW (mod ENC_SPLIT)), so one wave-instruction reads 64
// consecutive edge records (fully coalesced) and the per-lane dependent chain is ENC_SPLIT x
// shorter than one-lane-per-output.  The host pads every slice to a multiple of
// ENC_SPLIT*ENC_UNROLL edges per output with zero-weight records.
//
// SMALLW (all weights real and < 2^32, the only kind the reference ever draws, src/expanders.h:37):
// products are accumulated UNREDUCED in four 96-bit sums per output,
//     S_lo = sum w * lo32(a),  S_hi = sum w * hi32(a)        (for a = re and a = im)
// i.e. 4 v_mad_u64_u32 + 4 carry adds per edge and ONE Mersenne fold per output -- exact integer
// arithmetic, so the result is the same canonical element the reference's per-edge mod-p loop gives.
__device__ __forceinline__ void store8w(void *p, const uint32_t h[8]);
struct Acc96 { uint64_t lo; uint32_t hi; };
// a += w * x (32x32 -> 64 product into a 96-bit sum): one v_mad_u64_u32 whose carry-out feeds one
// v_addc (hipcc does not use the instruction's own carry output, hence the two-line asm).
__device__ __forceinline__ void acc96_mad(Acc96 &a, uint32_t w, uint32_t x) {
    asm("v_mad_u64_u32 %0, vcc, %2, %3, %0\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc" : "+v"(a.lo), "+v"(a.hi) : "v"(w), "v"(x) : "vcc");
}
// the four sums of one edge (re.lo, re.hi, im.lo, im.hi) in ONE asm statement: between separate statements hipcc pads every vcc hand-over with an s_nop
__device__ __forceinline__ void acc96_mad4(Acc96 &a, Acc96 &b, Acc96 &c, Acc96 &d, uint32_t w, const uint4 &x) {
    asm("v_mad_u64_u32 %0, vcc, %8, %9, %0\n\tv_addc_co_u32_e32 %1, vcc, 0, %1, vcc\n\t"
        "v_mad_u64_u32 %2, vcc, %8, %10, %2\n\tv_addc_co_u32_e32 %3, vcc, 0, %3, vcc\n\t"
        "v_mad_u64_u32 %4, vcc, %8, %11, %4\n\tv_addc_co_u32_e32 %5, vcc, 0, %5, vcc\n\t"
        "v_mad_u64_u32 %6, vcc, %8, %12, %6\n\tv_addc_co_u32_e32 %7, vcc, 0, %7, vcc"
        : "+v"(a.lo), "+v"(a.hi), "+v"(b.lo), "+v"(b.hi), "+v"(c.lo), "+v"(c.hi), "+v"(d.lo), "+v"(d.hi)
        : "v"(w), "v"(x.x), "v"(x.y), "v"(x.z), "v"(x.w) : "vcc");
}
__device__ __forceinline__ uint64_t acc_fold(const Acc96 &lo, const Acc96 &hi) {
    // value = lo + hi 2^32 with lo, hi 96-bit sums (any in-degree < 2^29).  No 128-bit arithmetic: 2^64 = 8 and 2^61 = 1 (mod p), so a 96-bit
    // sum {l, h} folds to fold61(l) + 8h < 2^61 + 2^36, and for the high sum b = b0 + 2^29 b1: b 2^32 = (b0 << 32) + b1.
    const uint64_t a = ((lo.lo & P61) + (lo.lo >> 61)) + ((uint64_t)lo.hi << 3);
    const uint64_t b = ((hi.lo & P61) + (hi.lo >> 61)) + ((uint64_t)hi.hi << 3);
    const uint64_t t = a + ((b & 0x1FFFFFFFull) << 32) + (b >> 29);                     // < 2^63
    const uint64_t r = (t & P61) + (t >> 61);                                            // <= p + 3
    return r >= P61 ? r - P61 : r;
}
__device__ __forceinline__ F shfl_xor_F(const F &a, int m) {
    F r;
    r.re = __shfl_xor((unsigned long long)a.re, m, 64);
    r.im = __shfl_xor((unsigned long long)a.im, m, 64);
    return r;
}

// A launch executes steps [s_lo, s_hi) of the encode on codeword indices [base, base + LDS extent):
// it loads [ld_lo, ld_hi) from the column in global memory, runs the steps (an output that falls
// outside the LDS window goes straight to global memory), and stores [st_lo, st_hi) (zeros past
// the codeword).  Small codes run as ONE pass; for n = 4096 (110 KB codeword, one workgroup per
// CU) the launcher splits the work into pass A = C_0 alone (64 KB message window, 2 workgroups per
// CU) and pass B = everything else (46 KB window, 3 per CU) so that one workgroup's global
// load/store overlaps another's gather loop.
struct EncPass { uint32_t base, ld_lo, ld_hi, s_lo, s_hi, st_lo, st_hi, direct_out; };
template <bool SMALLW>
__global__ void __launch_bounds__(1024)
k_encode(const F *__restrict__ src, size_t ld_src, F *__restrict__ dst, size_t ld_dst, uint32_t len, EncPass ps,
         const EncStep *__restrict__ steps, const uint32_t *__restrict__ slice_ptr,
         const uint32_t *__restrict__ slice_width, const uint32_t *__restrict__ slice_out, const uint2 *__restrict__ e32,
         const uint32_t *__restrict__ eidx, const F *__restrict__ ew) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *cw = reinterpret_cast<F *>(lds_raw) - ps.base;          // cw[i] addresses codeword index i
    const uint32_t b = blockIdx.x;
    const F *in = src + (size_t)b * ld_src;
    F *out = dst + (size_t)b * ld_dst;
    // window load: eight global loads per thread in flight before the first LDS store (one at a time cost a full memory round
    // trip per element: 7 400 of pass A's 27 000 cycles per column, measured with s_memtime stamps)
    for (uint32_t b0 = ps.ld_lo; b0 < ps.ld_hi; b0 += 8 * blockDim.x) {
        F v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const uint32_t i = b0 + u * blockDim.x + threadIdx.x; if (i < ps.ld_hi) v[u] = ldF(in + i); }
#pragma unroll
        for (int u = 0; u < 8; u++) { const uint32_t i = b0 + u * blockDim.x + threadIdx.x; if (i < ps.ld_hi) stF(&cw[i], v[u]); }
    }
    // (the barrier that publishes the window sits after the first step's first edge-record request: those loads do not touch LDS)
    // wave index as a scalar: the slice descriptors below then come through the scalar cache (s_load) instead of a per-lane
    // global load, and the slice loop is scalar control flow
    const uint32_t lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwaves = blockDim.x >> 6;
    for (uint32_t s = ps.s_lo; s < ps.s_hi; s++) {
        const EncStep sp = steps[s];
        const F *cin = cw + sp.in_off;
        const uint32_t sw = sp.sw, split = 64 / sw, tl = lane & (sw - 1);      // sw = 64: one output per lane; ENC_SW: lane groups share one
        if (SMALLW) {
            // slices of this wave: sl = wave, wave + nwaves, ...  The first group of edge records of the NEXT slice is requested
            // before the current slice's remainder / fold / shuffle / store, so its L2 latency is off the critical path.
            uint32_t sl = wave;
            bool have = sl < sp.n_slices;
            uint32_t nbase = 0, niters = 0;
            uint2 en[ENC_UNROLL];
            if (have) {
                nbase = slice_ptr[sp.slice_base + sl] + lane; niters = slice_width[sp.slice_base + sl] / split;
                if (niters >= ENC_UNROLL) {
#pragma unroll
                    for (int u = 0; u < ENC_UNROLL; u++) en[u] = e32[nbase + u * 64];
                }
            }
            if (s == ps.s_lo) __syncthreads();
            while (have) {
                const uint32_t base = nbase, iters = niters, cur = sl;
                Acc96 rl = {0, 0}, rh = {0, 0}, il = {0, 0}, ih = {0, 0};
                uint32_t j = 0;
                if (iters >= ENC_UNROLL) {
                    for (; j + ENC_UNROLL <= iters; j += ENC_UNROLL) {
                        uint2 e[ENC_UNROLL]; uint4 x[ENC_UNROLL];
#pragma unroll
                        for (int u = 0; u < ENC_UNROLL; u++) e[u] = en[u];
                        if (j + 2 * ENC_UNROLL <= iters) {     // prefetch the next full group of edge records
#pragma unroll
                            for (int u = 0; u < ENC_UNROLL; u++) en[u] = e32[base + (j + ENC_UNROLL + u) * 64];
                        }
#pragma unroll
                        for (int u = 0; u < ENC_UNROLL; u++) x[u] = *reinterpret_cast<const uint4 *>(cin + e[u].x);
#pragma unroll
                        for (int u = 0; u < ENC_UNROLL; u++) {
                            acc96_mad(rl, e[u].y, x[u].x); acc96_mad(rh, e[u].y, x[u].y);
                            acc96_mad(il, e[u].y, x[u].z); acc96_mad(ih, e[u].y, x[u].w);
                        }
                    }
                }
                sl += nwaves; have = sl < sp.n_slices;
                if (have) {                                   // next slice: descriptor + first record group in flight
                    nbase = slice_ptr[sp.slice_base + sl] + lane; niters = slice_width[sp.slice_base + sl] / split;
                    if (niters >= ENC_UNROLL) {
#pragma unroll
                        for (int u = 0; u < ENC_UNROLL; u++) en[u] = e32[nbase + u * 64];
                    }
                }
                for (; j < iters; j++) {                      // remainder (narrow steps only; rows are sorted by in-degree: at most ENC_UNROLL-1 records)
                    const uint2 e = e32[base + j * 64];
                    const uint4 x = *reinterpret_cast<const uint4 *>(cin + e.x);
                    acc96_mad(rl, e.y, x.x); acc96_mad(rh, e.y, x.y); acc96_mad(il, e.y, x.z); acc96_mad(ih, e.y, x.w);
                }
                F acc = fmake(acc_fold(rl, rh), acc_fold(il, ih));
                if (sw <= 16) acc = fadd(acc, shfl_xor_F(acc, 16));              // combine the lane groups (uniform branches)
                if (sw <= 32) acc = fadd(acc, shfl_xor_F(acc, 32));
                const uint32_t t = slice_out[sp.out_base + cur * sw + tl];       // outputs are sliced in order of in-degree
                if (lane < sw && t != 0xFFFFFFFFu) {
                    if (ps.direct_out) stF(out + sp.out_off + t, acc); else stF(&cw[sp.out_off + t], acc);
                }
            }
        } else {
            if (s == ps.s_lo) __syncthreads();
            for (uint32_t sl = wave; sl < sp.n_slices; sl += nwaves) {
                const uint32_t base = slice_ptr[sp.slice_base + sl] + lane;
                const uint32_t iters = slice_width[sp.slice_base + sl] / split;    // edge records per lane
                F acc = fmake(0);
                for (uint32_t j = 0; j < iters; j++) {
                    const uint32_t id = eidx[base + j * 64];
                    acc = fadd(acc, fmul(ldF(cin + id), ldF(ew + base + j * 64)));
                }
                if (sw <= 16) acc = fadd(acc, shfl_xor_F(acc, 16));
                if (sw <= 32) acc = fadd(acc, shfl_xor_F(acc, 32));
                const uint32_t t = slice_out[sp.out_base + sl * sw + tl];
                if (lane < sw && t != 0xFFFFFFFFu) {
                    if (ps.direct_out) stF(out + sp.out_off + t, acc); else stF(&cw[sp.out_off + t], acc);
                }
            }
        }
        __syncthreads();
    }
    for (uint32_t i = ps.st_lo + threadIdx.x; i < ps.st_hi; i += blockDim.x) stF(out + i, i < len ? ldF(&cw[i]) : fmake(0));
}

template <bool SMALLW>
static int launch_encode_pass(hobbit_ctx *ctx, const char *name, const F *src, size_t ld_src, F *dst, size_t ld_dst, size_t batch, EncPass ps,
                              uint32_t lds_elems, uint32_t block) {
    DeviceCode &c = ctx->code;
    hipFuncSetAttribute((const void *)k_encode<SMALLW>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    HB_LAUNCH(ctx, name, (k_encode<SMALLW>), dim3((unsigned)batch), dim3(block), (size_t)lds_elems * 16, src, ld_src, dst, ld_dst, (uint32_t)c.len, ps,
              c.d_steps, c.d_slice_ptr, c.d_slice_width, c.d_slice_out, c.d_edges32, c.d_eidx, c.d_ew);
    return 0;
}
static uint32_t block_for(const DeviceCode &c, uint32_t s_lo, uint32_t s_hi, uint32_t max_waves) {
    uint32_t widest = 1;
    for (uint32_t s = s_lo; s < s_hi; s++) widest = c.steps[s].n_slices > widest ? c.steps[s].n_slices : widest;
    return (widest >= max_waves ? max_waves : widest) * 64;
}

// ============================================================================================
// Wide SpMV steps of a deep code (n = 4096), persistent and register-resident (hobbit_ctx.hpp FatStep).
// One workgroup of NW fat waves and one loader wave per CU for the whole launch.  A lane owns NOUT outputs of the step for good and keeps
// their edge records -- 32-bit weight, 16-bit LDS byte offset -- in registers: the inner loop is one address add (SDWA word select), one
// ds_read_b128 and the 4 v_mad_u64_u32 + 4 v_addc of the unreduced 96-bit sums per edge; after the prologue no edge record, slice descriptor
// or index comes from memory.  The step's input window of the NEXT column streams into the second of two LDS buffers by LDS-DMA
// (global_load_lds_dwordx4, 1 KiB per wave-instruction, no registers) while the fat waves work on the current one; the loader wave issues
// all the pieces right after the one barrier per column that hands the buffers over (a wave's DMA pieces cost it ~100+ cycles each under
// load: with a dedicated loader the fat waves never stall on them -- 2.5 vs 3.3 ms for C_0 at 2^28 against every wave issuing its share;
// 2 / 4 / 6 pieces per fat wave beside the loader: 3.06 / 3.15 / 3.27 ms against 2.65 with the loader alone).  The outputs of column c
// are stored one iteration late, behind that barrier.
// (The one-workgroup-per-column k_encode re-reads 8 bytes of record per edge and column through L2 -- 40 GB per commit at 2^28 -- and its
// window load, barriers and slice loop do not overlap: DESIGN.md section 4.)
// ============================================================================================
template <int NOUT, int CAP0, int CAP1, int CAP2, int NW>
__global__ void __launch_bounds__((NW + 1) * 64)
k_enc_fat(F *__restrict__ tensor, size_t ld, uint32_t ncols, uint32_t in_off, uint32_t in_len, uint32_t out_off, uint32_t z_lo, uint32_t z_hi,
          const uint32_t *__restrict__ wt, const uint32_t *__restrict__ ot, const uint32_t *__restrict__ oidx, const uint32_t *__restrict__ wid, uint32_t rot_mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    constexpr int LANES = NW * 64, TOT = CAP0 + CAP1 + CAP2;
    constexpr int CAP[3] = {CAP0, CAP1, CAP2}, BASE[3] = {0, CAP0, CAP0 + CAP1};
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const uint32_t pieces = (in_len + 63) >> 6, win_bytes = pieces << 10;             // whole 1-KiB DMA pieces
    // [first_piece, end_piece): the pieces of a window this wave issues -- all of them for the loader (wave NW), none for a fat wave
    const bool loader = wave >= NW;
    const uint32_t first_piece = loader ? wave - NW : 0, end_piece = loader ? 0xFFFFFFFFu : 0;
    if (loader) {
        auto issue = [&](uint32_t c, uint32_t buf) {                                     // column c's window -> buffer buf
            const F *colp = tensor + (size_t)c * ld + in_off;
            if (rot_mask) {
                // A rotated message half (pass A of a commitment, hobbit_rot.hpp: in_off == 0, in_len == rot_mask + 1, whole pieces) is read through
                // its index; the LDS image is linear either way.  The column's rotation is wave-uniform and stays out of the piece loop: three vector
                // instructions per piece against the linear loop's four.  Every instruction of this wave waits for an issue slot among the fat
                // waves: five more per piece cost pass A 0.6 ms.
                const uint32_t rot = msg_rot_elems(c, rot_mask);
                for (uint32_t p = first_piece; p < pieces && p < end_piece; p++)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(colp + msg_rot_at((p << 6) + lane, rot, rot_mask)),
                                                     (__attribute__((address_space(3))) void *)(lds_raw + buf * win_bytes + (p << 10)), 16, 0, 0);
                return;
            }
            for (uint32_t p = first_piece; p < pieces && p < end_piece; p++) {
                uint32_t i = (p << 6) + lane; i = i < in_len ? i : in_len - 1;         // (the pad lanes of the last piece re-read the last element)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(colp + i),
                                                 (__attribute__((address_space(3))) void *)(lds_raw + buf * win_bytes + (p << 10)), 16, 0, 0);
            }
        };
        uint32_t c = blockIdx.x, it = 0;
        if (c < ncols) issue(c, 0);
        for (; c < ncols; c += gridDim.x, it++) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                             // this column's window has landed
            __builtin_amdgcn_s_barrier();                                                  // ... and the fat waves are done with the other buffer
            const uint32_t cn = c + gridDim.x;
            if (cn < ncols) issue(cn, (it + 1) & 1);
        }
        return;
    }
    // edge records into registers, once
    uint32_t w[TOT], o[TOT / 2], oi[NOUT], W[NOUT];
#pragma unroll
    for (int k = 0; k < TOT; k++) w[k] = wt[(size_t)k * LANES + threadIdx.x];
#pragma unroll
    for (int k = 0; k < TOT / 2; k++) o[k] = ot[(size_t)k * LANES + threadIdx.x];
#pragma unroll
    for (int j = 0; j < NOUT; j++) { oi[j] = oidx[(size_t)j * LANES + threadIdx.x]; W[j] = __builtin_amdgcn_readfirstlane(wid[wave * NOUT + j]); }
    F held[NOUT];                                                                        // the previous column's outputs, stored behind the next barrier
    F *hcol = nullptr;
    uint32_t it = 0;
    for (uint32_t c = blockIdx.x; c < ncols; c += gridDim.x, it++) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                 // (this wave's own loads and stores: the window is the loader's)
        __builtin_amdgcn_s_barrier();                                                      // this column's window has landed, and everyone is done with the other buffer
        if (hcol) {
#pragma unroll
            for (int j = 0; j < NOUT; j++) if (oi[j] != 0xFFFFFFFFu) stF(hcol + out_off + oi[j], held[j]);
            for (uint32_t i = z_lo + threadIdx.x; i < z_hi; i += LANES) stF(hcol + i, fmake(0));
        }
        const unsigned char *win = lds_raw + (it & 1) * win_bytes;
#pragma unroll
        for (int j = 0; j < NOUT; j++) {
            Acc96 rl = {0, 0}, rh = {0, 0}, il = {0, 0}, ih = {0, 0};
#pragma unroll
            for (int g = 0; g < CAP[j]; g += 4) {
                if ((uint32_t)g < W[j]) {                                                  // wave-uniform
                    uint4 x[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int k = BASE[j] + g + u;
                        const uint32_t off = (k & 1) ? (o[k >> 1] >> 16) : (o[k >> 1] & 0xFFFFu);
                        x[u] = *reinterpret_cast<const uint4 *>(win + off);
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) acc96_mad4(rl, rh, il, ih, w[BASE[j] + g + u], x[u]);
                }
            }
            held[j] = fmake(acc_fold(rl, rh), acc_fold(il, ih));
        }
        hcol = tensor + (size_t)c * ld;
    }
    if (hcol) {
#pragma unroll
        for (int j = 0; j < NOUT; j++) if (oi[j] != 0xFFFFFFFFu) stF(hcol + out_off + oi[j], held[j]);
        for (uint32_t i = z_lo + threadIdx.x; i < z_hi; i += LANES) stF(hcol + i, fmake(0));
    }
}
template <int NOUT, int CAP0, int CAP1, int CAP2, int NW>
static int launch_enc_fat(hobbit_ctx *ctx, const char *name, const FatStep &f, F *tensor, size_t ld, size_t ncols, uint32_t z_lo, uint32_t z_hi, uint32_t wgs,
                          uint32_t rot_mask = 0) {
    const size_t lds = (size_t)2 * ((f.in_len + 63) / 64) * 1024;
    auto kern = k_enc_fat<NOUT, CAP0, CAP1, CAP2, NW>;
    hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    const size_t grid = std::min(ncols, (size_t)wgs);
    HB_LAUNCH(ctx, name, kern, dim3((unsigned)grid), dim3((NW + 1) * 64), lds, tensor, ld, (uint32_t)ncols, f.in_off, f.in_len, f.out_off, z_lo, z_hi,
              f.d_wt, f.d_ot, f.d_oidx, f.d_w, rot_mask);
    return 0;
}

// ============================================================================================
// The five narrow steps C_2 .. D_1 of a deep code (n = 4096), persistent, register-resident and barrier-free (hobbit_ctx.hpp NarrowPlan).
// One wave owns one column at a time and walks columns c, c + gridDim.x, ...; its workgroup is that wave alone, with the 622-element window
// [x_2 .. z_1] in LDS.  The records of all five steps stay in registers for the whole launch (k_enc_fat's form: after the prologue no edge
// record, descriptor or index comes from memory), and the steps follow one another in program order: the LDS stores of a step, one
// lgkmcnt(0) wait, the gathers of the next.  Per position (hobbit_ctx.hpp) the inner loop is k_enc_fat's -- one operation for the address,
// one ds_read_b128, the 4 v_mad_u64_u32 + 4 v_addc of the unreduced 96-bit sums -- then one fold per lane, the xor-shuffle combine of the
// lanes that share an output, and the store into the window.  The next column's x_2 arrives by LDS-DMA in a staging area while the current
// column is worked on and is copied to the window's head when the columns change; the outputs [x_3 .. z_1] of a column leave as coalesced
// 16-byte stores from LDS at the start of the next iteration, so that the vmcnt(0) in front of the staging area never waits for a store
// just issued.
// ============================================================================================
static constexpr uint32_t NARROW_STAGE = 10240, NARROW_LDS = NARROW_STAGE + 3 * 1024;   // byte offset of the x_2 staging area (three 1-KiB DMA pieces), LDS per workgroup
static_assert(NARROW_WIN * 16 <= NARROW_STAGE && NARROW_X2 <= 3 * 64, "narrow window layout");
template <int P> struct NarrowPos {
    static constexpr int slot_base(int p) { int b = 0; for (int i = 0; i < p; i++) b += (int)NARROW_CAP[i]; return b; }
    static constexpr int LPO = NARROW_LPO[P], CAP = NARROW_CAP[P], WB = slot_base(P);
    static constexpr bool BYTES = P < (int)NARROW_BYTE_POS;
    static constexpr int SB = BYTES ? WB : WB - (int)NARROW_SLOTS8;                   // first slot among the records of its kind
    static constexpr int IN_BYTES = (int)NARROW_IN[NARROW_STEP_OF[P]] * 16;
    static constexpr bool STEP_END = P + 1 == (int)NARROW_POS || NARROW_STEP_OF[P + 1 < (int)NARROW_POS ? P + 1 : P] != NARROW_STEP_OF[P];
};
static_assert(NarrowPos<NARROW_BYTE_POS>::WB == NARROW_SLOTS8 && NarrowPos<NARROW_POS - 1>::WB + NarrowPos<NARROW_POS - 1>::CAP == NARROW_SLOTS, "narrow slot counts");
template <int P>
__device__ __forceinline__ void narrow_pos(unsigned char *lds, const uint32_t (&w)[NARROW_SLOTS], const uint32_t (&o)[NARROW_OREGS], const uint32_t (&q)[NARROW_QREGS]) {
    using NP = NarrowPos<P>;
    Acc96 rl = {0, 0}, rh = {0, 0}, il = {0, 0}, ih = {0, 0};
#pragma unroll
    for (int g = 0; g < NP::CAP; g += 4) {
        uint4 x[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (g + u >= NP::CAP) continue;
            const int k = NP::SB + g + u;
            if (NP::BYTES) x[u] = *reinterpret_cast<const uint4 *>(lds + NP::IN_BYTES + (((o[k >> 2] >> (8 * (k & 3))) & 0xFFu) << 4));
            else { const uint32_t r = o[(NARROW_SLOTS8 + 3) / 4 + (k >> 1)]; x[u] = *reinterpret_cast<const uint4 *>(lds + ((k & 1) ? (r >> 16) : (r & 0xFFFFu))); }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) if (g + u < NP::CAP) acc96_mad4(rl, rh, il, ih, w[NP::WB + g + u], x[u]);
    }
    F acc = fmake(acc_fold(rl, rh), acc_fold(il, ih));
#pragma unroll
    for (int m = 1; m < NP::LPO; m <<= 1) acc = fadd(acc, shfl_xor_F(acc, m));
    const uint32_t ob = (P & 1) ? (q[P >> 1] >> 16) : (q[P >> 1] & 0xFFFFu);
    if (ob != 0xFFFFu) stF(reinterpret_cast<F *>(lds + ob), acc);
    if (NP::STEP_END) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");            // this step's outputs are in the window before the next step gathers
}
template <int... P>
__device__ __forceinline__ void narrow_steps(unsigned char *lds, const uint32_t (&w)[NARROW_SLOTS], const uint32_t (&o)[NARROW_OREGS], const uint32_t (&q)[NARROW_QREGS],
                                             std::integer_sequence<int, P...>) {
    (narrow_pos<P>(lds, w, o, q), ...);
}
__global__ void __launch_bounds__(64)
k_enc_narrow(F *__restrict__ tensor, size_t ld, uint32_t ncols, uint32_t x2_off, const uint32_t *__restrict__ wt, const uint32_t *__restrict__ ot,
             const uint32_t *__restrict__ qt) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const uint32_t lane = threadIdx.x;
    auto issue = [&](uint32_t c) {                                                       // column c's x_2 -> the staging area
        const F *colp = tensor + (size_t)c * ld + x2_off;
#pragma unroll
        for (uint32_t p = 0; p < 3; p++) {
            uint32_t i = (p << 6) + lane; i = i < NARROW_X2 ? i : NARROW_X2 - 1;        // (the pad lanes of the last piece re-read the last element)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(colp + i),
                                             (__attribute__((address_space(3))) void *)(lds_raw + NARROW_STAGE + (p << 10)), 16, 0, 0);
        }
    };
    const uint32_t stride = gridDim.x;
    uint32_t c = blockIdx.x;
    if (c < ncols) issue(c);
    // edge records into registers, once
    uint32_t w[NARROW_SLOTS], o[NARROW_OREGS], q[NARROW_QREGS];
#pragma unroll
    for (uint32_t k = 0; k < NARROW_SLOTS; k++) w[k] = wt[k * 64 + lane];
#pragma unroll
    for (uint32_t k = 0; k < NARROW_OREGS; k++) o[k] = ot[k * 64 + lane];
#pragma unroll
    for (uint32_t k = 0; k < NARROW_QREGS; k++) q[k] = qt[k * 64 + lane];
    auto store_out = [&](F *col) {                                                       // [x_3 .. z_1] of the window -> the column
#pragma unroll
        for (uint32_t i0 = NARROW_X2; i0 < NARROW_WIN; i0 += 64) { const uint32_t i = i0 + lane; if (i < NARROW_WIN) stF(col + i, ldF(reinterpret_cast<const F *>(lds_raw) + i)); }
    };
    F *prev = nullptr;
    for (; c < ncols; c += stride) {
        // (the packed places are opaque to the compiler from one column to the next: it would otherwise hoist the 136 unpacked LDS addresses
        // out of the loop, one register each on top of the weights -- 322 registers, one wave per SIMD)
#pragma unroll
        for (uint32_t k = 0; k < NARROW_OREGS; k++) asm volatile("" : "+v"(o[k]));
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                 // this column's x_2 has landed in the staging area
        if (prev) store_out(prev);
#pragma unroll
        for (uint32_t p = 0; p < 3; p++) {
            const uint32_t i = (p << 6) + lane;
            if (i < NARROW_X2) stF(reinterpret_cast<F *>(lds_raw) + i, ldF(reinterpret_cast<const F *>(lds_raw + NARROW_STAGE) + i));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                               // x_2 is in the window, the staging area is free
        const uint32_t cn = c + stride;
        if (cn < ncols) issue(cn);
        narrow_steps(lds_raw, w, o, q, std::make_integer_sequence<int, NARROW_POS>());
        prev = tensor + (size_t)c * ld + x2_off;
    }
    if (prev) store_out(prev);
}
static int launch_enc_narrow(hobbit_ctx *ctx, const char *name, const NarrowPlan &np, F *tensor, size_t ld, size_t ncols) {
    const size_t grid = std::min(ncols, (size_t)NARROW_WGS);
    HB_LAUNCH(ctx, name, k_enc_narrow, dim3((unsigned)grid), dim3(64), (size_t)NARROW_LDS, tensor, ld, (uint32_t)ncols, np.x2_off, np.d_wt, np.d_ot, np.d_q);
    return 0;
}

// ============================================================================================
// Long codes (hobbit_ctx.hpp TiledStep): one SpMV step whose input window is longer than LDS, one workgroup per (column, output group).
// The window streams through LDS one 64 KB tile at a time; a wave owns up to TILE_MAXS slices of 64 outputs (one output per lane) and keeps
// their four unreduced 96-bit sums per output in registers across the tiles -- the same acc96_mad4 / acc_fold arithmetic as k_encode, one
// Mersenne fold per output -- and stores the outputs to the column at the end.  copy_in (out-of-place C_0): the workgroup of output group 0
// also writes the window to the destination column; [z_lo, z_hi): zeros it writes behind the codeword (D_0).
// ============================================================================================
template <bool SMALLW>
__global__ void __launch_bounds__(TILE_WAVES * 64)
k_enc_tiled(const F *__restrict__ src, size_t ld_src, F *__restrict__ dst, size_t ld_dst, TiledStep ts, const uint32_t *__restrict__ tile_ptr,
            const uint32_t *__restrict__ tile_width, const uint32_t *__restrict__ tile_out, const uint2 *__restrict__ e32,
            const uint32_t *__restrict__ eidx, const F *__restrict__ ew, uint32_t copy_in, uint32_t z_lo, uint32_t z_hi) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *tile = reinterpret_cast<F *>(lds_raw);
    const F *in = src + (size_t)blockIdx.x * ld_src + ts.in_off;
    F *out = dst + (size_t)blockIdx.x * ld_dst;
    const uint32_t grp = blockIdx.y, lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool copy = copy_in && grp == 0;
    Acc96 acc[TILE_MAXS][4];
    F accf[TILE_MAXS];
#pragma unroll
    for (uint32_t m = 0; m < TILE_MAXS; m++) {
        accf[m] = fmake(0);
#pragma unroll
        for (int q = 0; q < 4; q++) acc[m][q] = {0, 0};
    }
    for (uint32_t k = 0; k < ts.ntiles; k++) {
        const uint32_t lo = k * TILE_ELEMS, cnt = min(TILE_ELEMS, ts.in_len - lo);
        if (k) __syncthreads();                                  // every wave is done with the previous tile
        for (uint32_t b0 = 0; b0 < cnt; b0 += 4 * blockDim.x) {  // four global loads per thread in flight
            F v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) { const uint32_t i = b0 + u * blockDim.x + threadIdx.x; if (i < cnt) v[u] = ldF(in + lo + i); }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t i = b0 + u * blockDim.x + threadIdx.x;
                if (i < cnt) { stF(&tile[i], v[u]); if (copy) stF(out + ts.in_off + lo + i, v[u]); }
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t m = 0; m < TILE_MAXS; m++) {
            const uint32_t sl = (grp * TILE_MAXS + m) * TILE_WAVES + wave;        // wave-uniform
            if (sl >= ts.n_slices) continue;
            const uint32_t ti = ts.tile_base + sl * ts.ntiles + k;
            const uint32_t base = tile_ptr[ti] + lane, width = tile_width[ti];   // width: a multiple of ENC_UNROLL
            if (SMALLW) {
                for (uint32_t j = 0; j < width; j += ENC_UNROLL) {
                    uint2 e[ENC_UNROLL]; uint4 x[ENC_UNROLL];
#pragma unroll
                    for (int u = 0; u < ENC_UNROLL; u++) e[u] = e32[base + (j + u) * 64];
#pragma unroll
                    for (int u = 0; u < ENC_UNROLL; u++) x[u] = *reinterpret_cast<const uint4 *>(tile + e[u].x);
#pragma unroll
                    for (int u = 0; u < ENC_UNROLL; u++) acc96_mad4(acc[m][0], acc[m][1], acc[m][2], acc[m][3], e[u].y, x[u]);
                }
            } else {
                for (uint32_t j = 0; j < width; j++) accf[m] = fadd(accf[m], fmul(ldF(tile + eidx[base + j * 64]), ldF(ew + base + j * 64)));
            }
        }
    }
#pragma unroll
    for (uint32_t m = 0; m < TILE_MAXS; m++) {
        const uint32_t sl = (grp * TILE_MAXS + m) * TILE_WAVES + wave;
        if (sl >= ts.n_slices) continue;
        const uint32_t t = tile_out[ts.out_base + sl * 64 + lane];
        if (t != 0xFFFFFFFFu) stF(out + ts.out_off + t, SMALLW ? fmake(acc_fold(acc[m][0], acc[m][1]), acc_fold(acc[m][2], acc[m][3])) : accf[m]);
    }
    if (grp == 0)
        for (uint32_t i = z_lo + threadIdx.x; i < z_hi; i += blockDim.x) stF(out + i, fmake(0));
}

template <bool SMALLW>
static int launch_enc_tiled(hobbit_ctx *ctx, const char *name, const F *src, size_t ld_src, F *dst, size_t ld_dst, size_t batch, const TiledStep &ts,
                            uint32_t copy_in, uint32_t z_lo, uint32_t z_hi) {
    const DeviceCode &c = ctx->code;
    const uint32_t lds = std::min(ts.in_len, TILE_ELEMS) * 16;
    hipFuncSetAttribute((const void *)k_enc_tiled<SMALLW>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    // grid.x: columns, at most 2^31 - 1 per launch
    for (size_t b0 = 0; b0 < batch; b0 += 0x7FFFFFFFu) {
        const size_t nb = std::min<size_t>(batch - b0, 0x7FFFFFFFu);
        HB_LAUNCH(ctx, name, (k_enc_tiled<SMALLW>), dim3((unsigned)nb, ts.groups), dim3(TILE_WAVES * 64), lds, src + b0 * ld_src, ld_src, dst + b0 * ld_dst, ld_dst, ts,
                  c.d_tile_ptr, c.d_tile_width, c.d_tile_out, c.d_tile_e32, c.d_tile_eidx, c.d_tile_ew, copy_in, z_lo, z_hi);
    }
    return 0;
}

// Long codes: C_0 .. C_{d-1} tiled (C_0 reads the source; out of place it also copies the message), the sub-codeword of depth d as one k_encode
// pass on its window, D_{d-1} .. D_0 tiled (D_0 writes the zero tail).  Every launch reads what the one before it wrote to the destination.
static int launch_encode_long(hobbit_ctx *ctx, const F *src, size_t ld_src, F *dst, size_t ld_dst, size_t batch, int write_msg) {
    const DeviceCode &c = ctx->code;
    const uint32_t d = c.tiled_depth, nsteps = (uint32_t)c.steps.size(), nn = (uint32_t)c.n;
    uint32_t z_hi = 2 * nn;
    if (ctx->enc_skip_tail) { z_hi = std::min<uint32_t>(2 * nn, ((uint32_t)c.len + 3) & ~3u); ctx->enc_tail_skipped = true; }
    for (uint32_t j = 0; j < d; j++) {
        const F *s = j ? dst : src; const size_t ls = j ? ld_dst : ld_src;
        HB_TRY(c.small_weights ? launch_enc_tiled<true>(ctx, "k_enc_tiled_C", s, ls, dst, ld_dst, batch, c.tsteps[j], j == 0 && write_msg, 0, 0)
                               : launch_enc_tiled<false>(ctx, "k_enc_tiled_fullw_C", s, ls, dst, ld_dst, batch, c.tsteps[j], j == 0 && write_msg, 0, 0));
    }
    if (d < nsteps - d) {
        const EncStep &first = c.steps[d], &last = c.steps[nsteps - d - 1];
        const uint32_t w_lo = first.in_off, x_end = first.out_off, w_end = last.out_off + last.out_len;     // x_d = [w_lo, x_end), sub-codeword [w_lo, w_end)
        EncPass pm = {w_lo, w_lo, x_end, d, nsteps - d, x_end, w_end, 0};
        HB_TRY(c.small_weights ? launch_encode_pass<true>(ctx, "k_encode_long_M", dst, ld_dst, dst, ld_dst, batch, pm, w_end - w_lo, block_for(c, d, nsteps - d, 8))
                               : launch_encode_pass<false>(ctx, "k_encode_fullw_long_M", dst, ld_dst, dst, ld_dst, batch, pm, w_end - w_lo, block_for(c, d, nsteps - d, 8)));
    }
    for (uint32_t j = 0; j < d; j++) {
        const bool last = j + 1 == d;
        HB_TRY(c.small_weights ? launch_enc_tiled<true>(ctx, "k_enc_tiled_D", dst, ld_dst, dst, ld_dst, batch, c.tsteps[d + j], 0, last ? (uint32_t)c.len : 0, last ? z_hi : 0)
                               : launch_enc_tiled<false>(ctx, "k_enc_tiled_fullw_D", dst, ld_dst, dst, ld_dst, batch, c.tsteps[d + j], 0, last ? (uint32_t)c.len : 0, last ? z_hi : 0));
    }
    return 0;
}

// The in-place encode of a deep code reads its message in exactly one place, the loader wave of k_enc_fat's pass A (window [0, n)); C_1, the
// narrow steps, pass B and D_0 read and write the parity half [n, 2n) only.  That pass is the one form that follows a rotated message half.
bool encode_reads_rotated(const hobbit_ctx *ctx, long long n) {
    const DeviceCode &c = ctx->code;
    if (c.n != n || (size_t)c.len * 16 > 160 * 1024 || c.steps.size() < 2 || (size_t)c.len * 16 <= 80 * 1024) return false;
    if (!c.small_weights || !c.fatA.ok || c.fatA.in_off != 0 || c.fatA.in_len != (uint32_t)n) return false;
    if (c.fatD.ok && c.steps.size() >= 5 && (c.fatD.in_off < (uint32_t)n || (c.fatC1.ok && c.fatC1.in_off < (uint32_t)n))) return false;
    return true;
}
int launch_encode(hobbit_ctx *ctx, const F *src, size_t ld_src, F *dst, size_t ld_dst, long long n, size_t batch, int write_msg, uint32_t rot_mask) {
    DeviceCode &c = ctx->code;
    if (c.n != n) return ctx->fail(HOBBIT_ESTATE, "encode: graphs for this n are not finalized (hobbit_graph_finalize)");
    if (batch == 0) return 0;
    if (rot_mask && !(rot_mask == (uint32_t)n - 1 && src == dst && ld_src == ld_dst && !write_msg && encode_reads_rotated(ctx, n)))
        return ctx->fail(HOBBIT_ESTATE, "encode: a rotated message half needs the fat in-place form of this code");
    if ((size_t)c.len * 16 > 160 * 1024) {
        HB_TRY(ensure_tiled(ctx));
        if (!c.tiled_depth) return ctx->fail(HOBBIT_ESTATE, "encode: long code without its tiled steps (hobbit_graph_finalize)");
        return launch_encode_long(ctx, src, ld_src, dst, ld_dst, batch, write_msg);
    }
    const uint32_t nn = (uint32_t)n, nsteps = (uint32_t)c.steps.size();
    const bool split = nsteps >= 2 && (size_t)c.len * 16 > 80 * 1024;     // cannot co-schedule two workgroups per CU otherwise
    if (!split) {
        EncPass ps = {0, 0, nn, 0, nsteps, write_msg ? 0u : nn, 2 * nn, 0};
        uint32_t block = block_for(c, 0, nsteps, 16);
        return c.small_weights ? launch_encode_pass<true>(ctx, "k_encode", src, ld_src, dst, ld_dst, batch, ps, (uint32_t)c.len, block)
                               : launch_encode_pass<false>(ctx, "k_encode_fullw", src, ld_src, dst, ld_dst, batch, ps, (uint32_t)c.len, block);
    }
    // pass A: x_1 = C_0 x_0, outputs straight to the column in global memory
    const uint32_t r0 = c.steps[0].out_len;
    EncPass pa = {0, 0, nn, 0, 1, write_msg ? 0u : nn, write_msg ? nn : nn, 1};
    // pass B: the remaining steps on the window [n, len)
    EncPass pb = {nn, nn, nn + r0, 1, nsteps, nn + r0, 2 * nn, 0};
    // deep codes in place (the message is where the codeword goes): C_0 by the persistent register-resident kernel, then the rest as one
    // pass B unless D_0 fits that kernel too
    if (c.small_weights && c.fatA.ok && src == dst && ld_src == ld_dst && !write_msg) {
        HB_TRY((launch_enc_fat<FAT_A_NOUT, FAT_A_CAP0, FAT_A_CAP1, 0, FAT_A_CONS>(ctx, "k_enc_fat_A", c.fatA, dst, ld_dst, batch, 0, 0, FAT_A_WGS, rot_mask)));
        if (!c.fatD.ok || nsteps < 5)
            return launch_encode_pass<true>(ctx, "k_encode_B", dst, ld_dst, dst, ld_dst, batch, pb, (uint32_t)c.len - nn, block_for(c, 1, nsteps, 8));
        // C_1 alone -- 21 % of the edges on a 14 KB window: fat form, three workgroups per CU -- then the five short steps C_2 .. D_1 on the
        // 10 KB window [x_2 .. z_1], then D_0 in fat form (it also writes the zero tail).  The five steps run under the profile name
        // k_encode_M2 in one of two forms, chosen from the graph at finalize: k_enc_narrow, one persistent wave per column with every edge
        // record in registers and no barrier (the code's own five-step shape with the degrees the kernel was compiled for), or else the
        // one-workgroup-per-column k_encode with two-wave workgroups, sixteen per CU, which re-reads records and descriptors for every
        // column.  2^28: 2.44 ms for C_1 .. D_1 as one k_encode launch, 0.93 + 1.05 split, 0.63 + 1.05 with C_1 fat; the narrow form's
        // figures are in DESIGN.md section 4
        const EncStep &last = c.steps[nsteps - 1];
        const uint32_t r1 = c.steps[1].out_len, x2 = nn + r0;
        if (c.fatC1.ok) {
            HB_TRY((launch_enc_fat<FAT_C1_NOUT, FAT_C1_CAP0, 0, 0, FAT_C1_CONS>(ctx, "k_enc_fat_C1", c.fatC1, dst, ld_dst, batch, 0, 0, FAT_C1_WGS)));
        } else {
            EncPass p1 = {nn, nn, nn + r0, 1, 2, x2, x2, 1};
            HB_TRY(launch_encode_pass<true>(ctx, "k_encode_C1", dst, ld_dst, dst, ld_dst, batch, p1, r0, block_for(c, 1, 2, 8)));
        }
        if (c.narrow.ok) {
            HB_TRY(launch_enc_narrow(ctx, "k_encode_M2", c.narrow, dst, ld_dst, batch));
        } else {
            EncPass p2 = {x2, x2, x2 + r1, 2, nsteps - 1, x2 + r1, last.out_off, 0};
            HB_TRY(launch_encode_pass<true>(ctx, "k_encode_M2", dst, ld_dst, dst, ld_dst, batch, p2, last.out_off - x2, block_for(c, 2, nsteps - 1, 2)));
        }
        // the zero tail [len, 2n): a caller that answers those rows as zeros itself (commit_impl: leaf chain, gathers and row reads know the
        // codeword length) asks for the rows up to the next multiple of four only -- the leaf group that straddles the codeword's end is read whole
        uint32_t z_hi = 2 * nn;
        if (ctx->enc_skip_tail) { z_hi = std::min<uint32_t>(2 * nn, ((uint32_t)c.len + 3) & ~3u); ctx->enc_tail_skipped = true; }
        return launch_enc_fat<FAT_D_NOUT, FAT_D_CAP0, FAT_D_CAP1, FAT_D_CAP2, FAT_D_CONS>(ctx, "k_enc_fat_D", c.fatD, dst, ld_dst, batch, (uint32_t)c.len, z_hi,
                                                                                         FAT_D_WGS);
    }
    if (c.small_weights) {
        HB_TRY(launch_encode_pass<true>(ctx, "k_encode_A", src, ld_src, dst, ld_dst, batch, pa, nn, block_for(c, 0, 1, 16)));
        return launch_encode_pass<true>(ctx, "k_encode_B", dst, ld_dst, dst, ld_dst, batch, pb, (uint32_t)c.len - nn, block_for(c, 1, nsteps, 8));
    }
    HB_TRY(launch_encode_pass<false>(ctx, "k_encode_fullw_A", src, ld_src, dst, ld_dst, batch, pa, nn, block_for(c, 0, 1, 8)));
    return launch_encode_pass<false>(ctx, "k_encode_fullw_B", dst, ld_dst, dst, ld_dst, batch, pb, (uint32_t)c.len - nn, block_for(c, 1, nsteps, 8));
}

// ============================================================================================
// BLAKE3 / Merkle
// ============================================================================================
__device__ __forceinline__ void load16w(const void *p, uint32_t m[16]) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (int i = 0; i < 4; i++) { uint4 v = q[i]; m[4 * i] = v.x; m[4 * i + 1] = v.y; m[4 * i + 2] = v.z; m[4 * i + 3] = v.w; }
}
__device__ __forceinline__ void load8w(const void *p, uint32_t m[8]) {
    const uint4 *q = reinterpret_cast<const uint4 *>(p);
#pragma unroll
    for (int i = 0; i < 2; i++) { uint4 v = q[i]; m[4 * i] = v.x; m[4 * i + 1] = v.y; m[4 * i + 2] = v.z; m[4 * i + 3] = v.w; }
}
__device__ __forceinline__ void store8w(void *p, const uint32_t h[8]) {
    uint4 *q = reinterpret_cast<uint4 *>(p);
    q[0] = make_uint4(h[0], h[1], h[2], h[3]); q[1] = make_uint4(h[4], h[5], h[6], h[7]);
}

__global__ void k_blake3_64(const uint8_t *__restrict__ in, uint8_t *__restrict__ out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t m[16], h[8];
        load16w(in + 64 * i, m); blake3_compress64(m, h); store8w(out + 32 * i, h);
    }
}
// out[i] = H( H(xyzw[i]) | prev[i] )   (src/merkle_tree.cpp:62-87).  out may be prev (the streaming commits update their state in place): a
// thread reads prev[i] before it writes out[i] and touches no other entry, so neither of the two is declared __restrict__
__global__ void k_hash_md(const F *__restrict__ xyzw, const uint8_t *prev, uint8_t *out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t m[16], h[8];
        load16w(xyzw + 4 * i, m); blake3_compress64(m, h);
#pragma unroll
        for (int j = 0; j < 8; j++) m[j] = h[j];
        load8w(prev + 32 * i, m + 8);
        blake3_compress64(m, h); store8w(out + 32 * i, h);
    }
}
// level kernel: cur[i] = H(prev[2i] | prev[2i + (quirk ? 0 : 1)])   (src/merkle_tree.cpp:255-287)
__global__ void k_merkle_level(const uint8_t *__restrict__ prev, uint8_t *__restrict__ cur, size_t n_cur, int quirk) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n_cur; i += (size_t)gridDim.x * blockDim.x) {
        uint32_t m[16], h[8];
        load8w(prev + 64 * i, m);
        if (quirk) {
#pragma unroll
            for (int j = 0; j < 8; j++) m[8 + j] = m[j];
        } else load8w(prev + 64 * i + 32, m + 8);
        blake3_compress64(m, h); store8w(cur + 32 * i, h);
    }
}
// the last levels (n_cur <= 1024 nodes and everything above them) in ONE workgroup: a level per launch is pure launch latency
// up there (ten launches of a few microseconds of work each, and the opening builds about twenty small trees)
__global__ void __launch_bounds__(1024) k_merkle_top(const uint8_t *__restrict__ prev, uint8_t *__restrict__ cur, uint32_t n_cur, int quirk) {
    __shared__ uint32_t buf[2][1024 * 8];
    const uint32_t tid = threadIdx.x;
    uint32_t m[16], h[8];
    if (tid < n_cur) {
        load8w(prev + 64 * (size_t)tid, m);
        if (quirk) {
#pragma unroll
            for (int j = 0; j < 8; j++) m[8 + j] = m[j];
        } else load8w(prev + 64 * (size_t)tid + 32, m + 8);
        blake3_compress64(m, h); store8w(cur + 32 * (size_t)tid, h);
#pragma unroll
        for (int j = 0; j < 8; j++) buf[0][tid * 8 + j] = h[j];
    }
    uint32_t off = n_cur; int pb = 0;
    for (uint32_t sz = n_cur / 2; sz >= 1; sz /= 2) {
        __syncthreads();
        if (tid < sz) {
#pragma unroll
            for (int j = 0; j < 8; j++) m[j] = buf[pb][(2 * tid) * 8 + j];
#pragma unroll
            for (int j = 0; j < 8; j++) m[8 + j] = quirk ? m[j] : buf[pb][(2 * tid + 1) * 8 + j];
            blake3_compress64(m, h); store8w(cur + 32 * (size_t)(off + tid), h);
#pragma unroll
            for (int j = 0; j < 8; j++) buf[pb ^ 1][tid * 8 + j] = h[j];
        }
        off += sz; pb ^= 1;
    }
}
// `g` consecutive levels in one launch: a workgroup hashes 1024 nodes of the level that has `sz` nodes (from 2048 nodes of `prev`) and then
// the 512, 256, ... nodes above them that depend on nothing else, out of LDS -- the opening builds about eight trees of 2^19 .. 2^20
// leaves, and one launch per level was nine launches of a few microseconds each per tree.  sz must be a multiple of 1024, 1 <= g <= 11;
// `cur` points at the level of sz nodes, the levels above it follow in the flat layout.
__global__ void __launch_bounds__(1024) k_merkle_sub(const uint8_t *__restrict__ prev, uint8_t *__restrict__ cur, size_t sz, int g, int quirk) {
    __shared__ uint32_t buf[2][1024 * 8];
    const uint32_t tid = threadIdx.x;
    const size_t node = (size_t)blockIdx.x * 1024 + tid;
    uint32_t m[16], h[8];
    load8w(prev + 64 * node, m);
    if (quirk) {
#pragma unroll
        for (int j = 0; j < 8; j++) m[8 + j] = m[j];
    } else load8w(prev + 64 * node + 32, m + 8);
    blake3_compress64(m, h); store8w(cur + 32 * node, h);
#pragma unroll
    for (int j = 0; j < 8; j++) buf[0][tid * 8 + j] = h[j];
    size_t off = sz, lsz = sz; uint32_t width = 1024; int pb = 0;
    for (int lv = 1; lv < g; lv++) {
        width >>= 1; lsz >>= 1;
        __syncthreads();
        if (tid < width) {
#pragma unroll
            for (int j = 0; j < 8; j++) m[j] = buf[pb][(2 * tid) * 8 + j];
#pragma unroll
            for (int j = 0; j < 8; j++) m[8 + j] = quirk ? m[j] : buf[pb][(2 * tid + 1) * 8 + j];
            blake3_compress64(m, h); store8w(cur + 32 * (off + (size_t)blockIdx.x * width + tid), h);
#pragma unroll
            for (int j = 0; j < 8; j++) buf[pb ^ 1][tid * 8 + j] = h[j];
        }
        off += lsz; pb ^= 1;
    }
}
// Our_PC leaf chain over all K chunks (src/Our_PC.cpp:162-166).  The tensor is codeword-major
// ([chunk][col][2 trs]), so the 4 field elements of leaf (j, col) are 64 contiguous bytes.  One
// thread owns one leaf and keeps its Merkle-Damgard state in registers across the chunk loop:
// the tensor is read exactly once and the leaf array is written exactly once.
// Rows at or beyond the codeword length are zero in every chunk (the expander code fills 1.72 n of the 2 n rows), so the groups j >= zf
// (14 % of them at n = 4096) are neither read nor hashed here: the commit's chain starts from the zero state, so every such leaf is the same
// 32 bytes Z_K = blake3_zero_group_leaf(K), computed on the host and passed in as zk.  In leaf order j * cols + c those leaves are one
// contiguous tail of the leaf array, and every workgroup stores a slice of it with 16-byte stores before it starts hashing.
// The chain runs over the dense index idx in [0, cols * zf) of the other groups, c = idx / zf, j = idx % zf: a wavefront may straddle two
// columns, each lane still reads its own 64 contiguous bytes per chunk, and every workgroup costs the same, so no block order has to be
// arranged around the 8 XCDs.  (k_leaf_chain_relay below does NOT take this shortcut: it continues from a state its caller hands in, and
// what the chain of a zero group has absorbed before is not its to assume.)
struct ZeroDig { uint32_t w[8]; };
template <int NL>
__global__ void __launch_bounds__(256)
k_leaf_chain(const F *__restrict__ tensor, size_t chunk_stride, int K, uint32_t cols, uint32_t half_trs, uint8_t *__restrict__ leaves, uint32_t zf, ZeroDig zk,
             uint32_t rot_mask) {
    const uint32_t stride = gridDim.x * blockDim.x;
    // the leaves of the zero groups: 2 (half_trs - zf) cols stores of 16 bytes, ending exactly at the end of the leaf array
    {
        const size_t fill16 = 2 * (size_t)(half_trs - zf) * cols;
        uint4 *tail = reinterpret_cast<uint4 *>(leaves + 32 * (size_t)zf * cols);
        const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;     // stride is even: a thread stores the same half of Z_K every time
        const uint4 v = (t & 1) ? make_uint4(zk.w[4], zk.w[5], zk.w[6], zk.w[7]) : make_uint4(zk.w[0], zk.w[1], zk.w[2], zk.w[3]);
        for (size_t u = t; u < fill16; u += stride) tail[u] = v;
    }
    // NL leaves per thread (independent hash chains interleaved for instruction-level parallelism)
    const uint32_t total = cols * zf, per = (total + NL - 1) / NL;
    for (uint32_t b0 = blockIdx.x * blockDim.x; b0 < per; b0 += stride) {
        const uint32_t g0 = b0 + threadIdx.x;
        if (g0 >= per) continue;
        uint32_t st[NL][8];
        const F *p[NL];
        uint32_t g[NL], c[NL], j[NL];
#pragma unroll
        for (int l = 0; l < NL; l++) {
            g[l] = g0 + (uint32_t)l * per;
            const uint32_t gg = g[l] < total ? g[l] : total - 1;    // tail lanes recompute the last leaf (not stored)
#pragma unroll
            for (int q = 0; q < 8; q++) st[l][q] = 0;
            c[l] = gg / zf; j[l] = gg - c[l] * zf;
            // (c * 2trs + 4j; in a commitment's rotated message half the group sits at its rotated place, whole and aligned: hobbit_rot.hpp)
            p[l] = tensor + (size_t)c[l] * half_trs * 4 + msg_rot_row(4 * j[l], c[l], rot_mask);
        }
        for (int i = 0; i < K; i++) {
            uint32_t m[NL][16], h[NL][8];
#pragma unroll
            for (int l = 0; l < NL; l++) { load16w(p[l] + (size_t)i * chunk_stride, m[l]); blake3_compress64(m[l], h[l]); }
#pragma unroll
            for (int l = 0; l < NL; l++) {
#pragma unroll
                for (int q = 0; q < 8; q++) { m[l][q] = h[l][q]; m[l][8 + q] = st[l][q]; }
            }
#pragma unroll
            for (int l = 0; l < NL; l++) blake3_compress64(m[l], st[l]);
        }
#pragma unroll
        for (int l = 0; l < NL; l++)
            if (g[l] < total) store8w(leaves + 32 * ((size_t)j[l] * cols + c[l]), st[l]);
    }
}
// Multi-GPU commit by chain relay: the same chain over the K_local chunks of a rank's tensor shard, for the leaf slots
// g in [g_begin, g_begin + g_count) (slot g = col * half_trs + j: the order the shard is read in), starting from the state the previous
// rank handed over (state_in, 32 B per slot in slot order; NULL = the zero state of the first chunks) and leaving either the running
// state for the next rank (state_out, slot order: both sides of the hand-over are coalesced) or -- last rank -- the final leaves in the
// reference's leaf order j * cols + col.
__global__ void __launch_bounds__(256)
k_leaf_chain_relay(const F *__restrict__ tensor, size_t chunk_stride, int K, uint32_t cols, uint32_t half_trs, size_t g_begin, size_t g_count,
                   const uint8_t *__restrict__ state_in, uint8_t *__restrict__ state_out, uint8_t *leaves, uint32_t zero_from, ZeroDig zdig, int leaves_inout) {
    // This kernel still visits the all-zero groups (one compression per chunk for them, with the constant inner digest zdig = H(0^64), instead
    // of two).  Blocks are dealt round-robin over the 8 XCDs, and with 8 blocks per column the cheap all-zero groups of EVERY column would land
    // on one XCD (b % 8 == 7), which would idle while the other seven set the kernel's time.  Rotating the block index inside each run of 8 by
    // the run's number spreads the cheap blocks evenly.  The grid is capped: a block walks several runs of 8, and the pass number joins the
    // rotation, or it would meet the same position of every column it visits.  (The rotation permutes whole runs of 8 blocks: only when the
    // block count is a multiple of 8.)
    const bool rot = (gridDim.x & 7) == 0 && (((g_count + blockDim.x - 1) / blockDim.x) & 7) == 0;
    uint32_t pass = 0;
    for (size_t vb = blockIdx.x; vb * (size_t)blockDim.x < g_count; vb += gridDim.x, pass++) {
        const size_t bid = rot ? (vb & ~(size_t)7) | ((vb + (vb >> 3) + pass) & 7) : vb;
        const size_t t = bid * (size_t)blockDim.x + threadIdx.x;
        if (t >= g_count) continue;
        const size_t g = g_begin + t;
        uint32_t st[8];
        if (state_in) load8w(state_in + 32 * t, st);
        else if (leaves_inout) load8w(leaves + 32 * ((size_t)(g % half_trs) * cols + (size_t)(g / half_trs)), st);    // continue from the leaves already there (leaf order)
        else {
#pragma unroll
            for (int q = 0; q < 8; q++) st[q] = 0;
        }
        const F *p = tensor + g * 4;
        const bool zero = (uint32_t)(g % half_trs) >= zero_from;
        for (int i = 0; i < K; i++) {
            uint32_t m[16], h[8];
            if (zero) {
#pragma unroll
                for (int q = 0; q < 8; q++) h[q] = zdig.w[q];
            } else { load16w(p + (size_t)i * chunk_stride, m); blake3_compress64(m, h); }
#pragma unroll
            for (int q = 0; q < 8; q++) { m[q] = h[q]; m[8 + q] = st[q]; }
            blake3_compress64(m, st);
        }
        if (state_out) store8w(state_out + 32 * t, st);
        if (leaves) { const uint32_t c = (uint32_t)(g / half_trs), j = (uint32_t)(g % half_trs); store8w(leaves + 32 * ((size_t)j * cols + c), st); }
    }
}
int launch_leaf_chain_relay(hobbit_ctx *ctx, const F *tensor, size_t chunk_stride, int K, uint32_t cols, uint32_t half_trs, size_t g_begin, size_t g_count,
                            const uint8_t *state_in, uint8_t *state_out, uint8_t *leaves, uint32_t zero_rows_from, int leaves_inout) {
    if (!g_count) return 0;
    ZeroDig zd; { uint32_t z[16] = {0}; blake3_compress64(z, zd.w); }
    HB_LAUNCH(ctx, "k_leaf_chain_relay", k_leaf_chain_relay, dim3(grid_for(g_count, 256, 4096)), dim3(256), 0, tensor, chunk_stride, K, cols, half_trs, g_begin,
              g_count, state_in, state_out, leaves, (zero_rows_from + 3) / 4, zd, leaves_inout);
    return 0;
}
// Multi-GPU commit, step 1: inner digests H(t[4j..4j+3][c]) of the chunks a rank
// owns, written in the reference's LEAF ORDER (leaf = j*cols + c) so that a contiguous leaf range
// is a contiguous byte range to send: out[(i*M + j*cols + c)*32].
__global__ void k_inner_digests(const F *__restrict__ tensor, size_t chunk_stride, int nchunks, uint32_t cols, uint32_t half_trs,
                                uint8_t *__restrict__ out) {
    const size_t M = (size_t)cols * half_trs, total = M * nchunks;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const size_t i = g / M, rem = g % M;
        const uint32_t c = (uint32_t)(rem / half_trs), j = (uint32_t)(rem % half_trs);
        uint32_t m[16], h[8];
        load16w(tensor + i * chunk_stride + ((size_t)c * half_trs + j) * 4, m);
        blake3_compress64(m, h);
        store8w(out + 32 * (i * M + (size_t)j * cols + c), h);
    }
}
// step 2: Merkle-Damgard chain over the K chunks for a leaf range held in leaf order:
// leaf[p] = H(dig[K-1][p] | ... H(dig[0][p] | leaf[p]) ...), dig[i] at digests + i*stride
__global__ void k_chain_digests(const uint8_t *__restrict__ digests, size_t stride_bytes, int K, size_t m, uint8_t *__restrict__ leaves) {
    for (size_t p = blockIdx.x * (size_t)blockDim.x + threadIdx.x; p < m; p += (size_t)gridDim.x * blockDim.x) {
        uint32_t st[8], mm[16];
        load8w(leaves + 32 * p, st);
        for (int i = 0; i < K; i++) {
            load8w(digests + (size_t)i * stride_bytes + 32 * p, mm);
#pragma unroll
            for (int q = 0; q < 8; q++) mm[8 + q] = st[q];
            blake3_compress64(mm, st);
        }
        store8w(leaves + 32 * p, st);
    }
}
int launch_inner_digests(hobbit_ctx *ctx, const F *tensor, size_t chunk_stride, int nchunks, uint32_t cols, uint32_t half_trs, uint8_t *out) {
    size_t total = (size_t)cols * half_trs * nchunks;
    if (!total) return 0;
    HB_LAUNCH(ctx, "k_inner_digests", k_inner_digests, dim3(grid_for(total, 256, 1 << 20)), dim3(256), 0, tensor, chunk_stride, nchunks, cols, half_trs, out);
    return 0;
}
int launch_chain_digests(hobbit_ctx *ctx, const uint8_t *digests, size_t stride_bytes, int K, size_t m, uint8_t *leaves) {
    if (!m) return 0;
    HB_LAUNCH(ctx, "k_chain_digests", k_chain_digests, dim3(grid_for(m, 256, 1 << 20)), dim3(256), 0, digests, stride_bytes, K, m, leaves);
    return 0;
}
// Elastic_PC streaming commit (src/Elastic_PC.cpp:228-243): every 4th chunk the four stored tensors
// are hashed position-wise into the running leaves, leaf[p] = H( H(a|b|c|d) | leaf[p] ), p = row*cols+col.
// The call passes (ci0[counter], ci1[counter], ci2[counter++], tensor[j][k]) as arguments of ONE call;
// as built by GCC the first two are read at counter+1 -- `shift` = 1 reproduces that
// (a, b taken at p+1, zero past the end), 0 reads all four at p.  Tensors and the running leaf state
// are codeword-major (index g = col*rows2 + row) so every access is coalesced; k_elastic_finish
// permutes the state into the reference's leaf order once at the end.
__global__ void __launch_bounds__(256)
k_elastic_leaf(const F *__restrict__ t0, const F *__restrict__ t1, const F *__restrict__ t2, const F *__restrict__ t3, uint32_t rows2, uint32_t cols,
               int shift, uint8_t *__restrict__ state) {
    const size_t T = (size_t)rows2 * cols;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < T; g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t k = (uint32_t)(g / rows2), j = (uint32_t)(g % rows2);
        size_t gs = g; bool zero = false;
        if (shift) {
            if (k + 1 < cols) gs = g + rows2;                       // (j, k+1)
            else if (j + 1 < rows2) gs = (size_t)j + 1;             // wraps to (j+1, 0)
            else zero = true;                                       // p+1 == 4B: past the end
        }
        const F a = zero ? fmake(0) : ldF(t0 + gs), b = zero ? fmake(0) : ldF(t1 + gs), c = ldF(t2 + g), d = ldF(t3 + g);
        uint32_t m[16], h[8];
        m[0] = (uint32_t)a.re; m[1] = (uint32_t)(a.re >> 32); m[2] = (uint32_t)a.im; m[3] = (uint32_t)(a.im >> 32);
        m[4] = (uint32_t)b.re; m[5] = (uint32_t)(b.re >> 32); m[6] = (uint32_t)b.im; m[7] = (uint32_t)(b.im >> 32);
        m[8] = (uint32_t)c.re; m[9] = (uint32_t)(c.re >> 32); m[10] = (uint32_t)c.im; m[11] = (uint32_t)(c.im >> 32);
        m[12] = (uint32_t)d.re; m[13] = (uint32_t)(d.re >> 32); m[14] = (uint32_t)d.im; m[15] = (uint32_t)(d.im >> 32);
        blake3_compress64(m, h);
#pragma unroll
        for (int q = 0; q < 8; q++) m[q] = h[q];
        load8w(state + 32 * g, m + 8);
        blake3_compress64(m, h);
        store8w(state + 32 * g, h);
    }
}
// Multi-GPU streaming commit ("Elastic: groups of 4 consecutive chunks"): only the INNER digest H(c0, c1, c2, t3) of every
// position of one 4-chunk group, written in the reference's leaf order (p = j*cols + k) so that a rank's leaf range is one byte range
__global__ void __launch_bounds__(256)
k_elastic_inner(const F *__restrict__ t0, const F *__restrict__ t1, const F *__restrict__ t2, const F *__restrict__ t3, uint32_t rows2, uint32_t cols,
                int shift, uint8_t *__restrict__ out) {
    const size_t T = (size_t)rows2 * cols;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < T; g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t k = (uint32_t)(g / rows2), j = (uint32_t)(g % rows2);
        size_t gs = g; bool zero = false;
        if (shift) {
            if (k + 1 < cols) gs = g + rows2;
            else if (j + 1 < rows2) gs = (size_t)j + 1;
            else zero = true;
        }
        const F a = zero ? fmake(0) : ldF(t0 + gs), b = zero ? fmake(0) : ldF(t1 + gs), c = ldF(t2 + g), d = ldF(t3 + g);
        uint32_t m[16], h[8];
        m[0] = (uint32_t)a.re; m[1] = (uint32_t)(a.re >> 32); m[2] = (uint32_t)a.im; m[3] = (uint32_t)(a.im >> 32);
        m[4] = (uint32_t)b.re; m[5] = (uint32_t)(b.re >> 32); m[6] = (uint32_t)b.im; m[7] = (uint32_t)(b.im >> 32);
        m[8] = (uint32_t)c.re; m[9] = (uint32_t)(c.re >> 32); m[10] = (uint32_t)c.im; m[11] = (uint32_t)(c.im >> 32);
        m[12] = (uint32_t)d.re; m[13] = (uint32_t)(d.re >> 32); m[14] = (uint32_t)d.im; m[15] = (uint32_t)(d.im >> 32);
        blake3_compress64(m, h);
        store8w(out + 32 * ((size_t)j * cols + k), h);
    }
}
int launch_elastic_inner(hobbit_ctx *ctx, const F *t0, const F *t1, const F *t2, const F *t3, uint32_t rows2, uint32_t cols, int shift, uint8_t *out) {
    HB_LAUNCH(ctx, "k_elastic_inner", k_elastic_inner, dim3(grid_for((size_t)rows2 * cols, 256, 1 << 16)), dim3(256), 0, t0, t1, t2, t3, rows2, cols, shift, out);
    return 0;
}
__global__ void k_elastic_finish(const uint8_t *__restrict__ state, uint32_t rows2, uint32_t cols, uint8_t *__restrict__ leaves) {
    const size_t T = (size_t)rows2 * cols;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < T; g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t k = (uint32_t)(g / rows2), j = (uint32_t)(g % rows2);
        uint32_t h[8]; load8w(state + 32 * g, h);
        store8w(leaves + 32 * ((size_t)j * cols + k), h);
    }
}
int launch_elastic_leaf(hobbit_ctx *ctx, const F *t0, const F *t1, const F *t2, const F *t3, uint32_t rows2, uint32_t cols, int shift, uint8_t *state) {
    HB_LAUNCH(ctx, "k_elastic_leaf", k_elastic_leaf, dim3(grid_for((size_t)rows2 * cols, 256, 1 << 16)), dim3(256), 0, t0, t1, t2, t3, rows2, cols, shift, state);
    return 0;
}
int launch_elastic_finish(hobbit_ctx *ctx, const uint8_t *state, uint32_t rows2, uint32_t cols, uint8_t *leaves) {
    HB_LAUNCH(ctx, "k_elastic_finish", k_elastic_finish, dim3(grid_for((size_t)rows2 * cols, 256, 1 << 16)), dim3(256), 0, state, rows2, cols, leaves);
    return 0;
}
// ---- the streaming commit on base-field chunks (include/hobbit_elastic_real.h): k_elastic_leaf over four HALF chunk tensors (hobbit_half.hpp) ----
// position p + 1 of the full chunk tensor in leaf order p = r cols + c (k_elastic_leaf's `shift`); false past the end
__device__ __forceinline__ bool elastic_next(uint32_t &r, uint32_t &c, uint32_t rows2, uint32_t cols) {
    if (c + 1 < cols) { c++; return true; }
    if (r + 1 < rows2) { r++; c = 0; return true; }
    return false;
}
// entry (r, c) of the full chunk tensor out of its half tensor
__device__ __forceinline__ F half_ld(const F *__restrict__ t, uint32_t r, uint32_t c, uint32_t cols, uint32_t rows2, int lin) {
    const HalfRef h = half_ref(r, c, cols, rows2, lin);
    const F v = ldF(t + half_chunk_at(h.row, h.col, rows2));
    return h.conj ? fconj(v) : v;
}
// st = H( H(a | b | c | d) | st )
__device__ __forceinline__ void elastic_leaf_update(const F &a, const F &b, const F &c, const F &d, uint8_t *__restrict__ st) {
    uint32_t m[16], h[8];
    m[0] = (uint32_t)a.re; m[1] = (uint32_t)(a.re >> 32); m[2] = (uint32_t)a.im; m[3] = (uint32_t)(a.im >> 32);
    m[4] = (uint32_t)b.re; m[5] = (uint32_t)(b.re >> 32); m[6] = (uint32_t)b.im; m[7] = (uint32_t)(b.im >> 32);
    m[8] = (uint32_t)c.re; m[9] = (uint32_t)(c.re >> 32); m[10] = (uint32_t)c.im; m[11] = (uint32_t)(c.im >> 32);
    m[12] = (uint32_t)d.re; m[13] = (uint32_t)(d.re >> 32); m[14] = (uint32_t)d.im; m[15] = (uint32_t)(d.im >> 32);
    blake3_compress64(m, h);
#pragma unroll
    for (int q = 0; q < 8; q++) m[q] = h[q];
    load8w(st, m + 8);
    blake3_compress64(m, h);
    store8w(st, h);
}
// One thread per STORED entry (j, sc), sc <= cols / 2: it loads its entries of the last two tensors once and updates leaf (j, sc) and, for
// 0 < sc < cols / 2, the leaf of the full entry in column cols - sc that (j, sc) answers as its conjugate (half_mirror_row) -- one load, two
// leaves.  The first two tensors are read per leaf, at the leaf's own position p or with `shift` at p + 1, through half_ref.  The running state is k_elastic_leaf's, codeword-major over the
// FULL tensor, so k_elastic_finish is the same.  (256, 8): eight waves per SIMD as k_elastic_leaf has, i.e. at most 64 VGPRs.
__global__ void __launch_bounds__(256, 8)
k_elastic_leaf_half(const F *__restrict__ t0, const F *__restrict__ t1, const F *__restrict__ t2, const F *__restrict__ t3, uint32_t rows2, uint32_t cols,
                    int shift, int lin, uint8_t *__restrict__ state) {
    const uint32_t hc = cols / 2;
    const size_t T = (size_t)(hc + 1) * rows2;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < T; g += (size_t)gridDim.x * blockDim.x) {
        const uint32_t sc = (uint32_t)(g / rows2), j = (uint32_t)(g % rows2);
        const F c = ldF(t2 + g), d = ldF(t3 + g);
        // the first two tensors at the leaf's own position, or the next one: only c and d stay in registers across the two leaves
        auto first_two = [&](uint32_t r, uint32_t cc, F &a, F &b) {
            a = fmake(0); b = fmake(0);
            if (shift && !elastic_next(r, cc, rows2, cols)) return;
            a = half_ld(t0, r, cc, cols, rows2, lin); b = half_ld(t1, r, cc, cols, rows2, lin);
        };
        F a, b;
        first_two(j, sc, a, b);
        elastic_leaf_update(a, b, c, d, state + 32 * g);                                 // (the state index of (j, sc) is sc rows2 + j = g)
        if (sc > 0 && sc < hc) {
            const uint32_t cm = cols - sc, jm = half_mirror_row(j, rows2, lin);
            first_two(jm, cm, a, b);
            elastic_leaf_update(a, b, fconj(c), fconj(d), state + 32 * ((size_t)cm * rows2 + jm));
        }
    }
}
int launch_elastic_leaf_half(hobbit_ctx *ctx, const F *t0, const F *t1, const F *t2, const F *t3, uint32_t rows2, uint32_t cols, int shift, int lin, uint8_t *state) {
    HB_LAUNCH(ctx, "k_elastic_leaf_half", k_elastic_leaf_half, dim3(grid_for((size_t)rows2 * (cols / 2 + 1), 256, 1 << 16)), dim3(256), 0, t0, t1, t2, t3, rows2, cols,
              shift, lin, state);
    return 0;
}
// shockwave_commit column digests (src/Virgo.cpp:143-151): digest of column c = root of MT_commit_Blake over the
// k entries enc[0..k)[c] (k/4 leaves of 4 elements, then the tree with the configured parent rule), k <= 64
__global__ void __launch_bounds__(256)
k_col_digest(const F *__restrict__ enc, size_t W, int k, int quirk, uint8_t *__restrict__ out) {
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < W; c += (size_t)gridDim.x * blockDim.x) {
        const int leaves = k / 4;
        if (quirk) {
            // create_tree_blake's parent is H(left | left) (src/merkle_tree.cpp:275-280): the root is leaf 0 re-hashed log2(leaves)
            // times -- rows 0..3 of the column are all that reaches it.  1 + log2(leaves) compressions instead of 2*leaves - 1, in registers.
            uint32_t m[16], h[8];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const F v = ldF(enc + (size_t)e * W + c);
                m[4 * e] = (uint32_t)v.re; m[4 * e + 1] = (uint32_t)(v.re >> 32); m[4 * e + 2] = (uint32_t)v.im; m[4 * e + 3] = (uint32_t)(v.im >> 32);
            }
            blake3_compress64(m, h);
            for (int n = leaves; n > 1; n >>= 1) {
#pragma unroll
                for (int q = 0; q < 8; q++) { m[q] = h[q]; m[8 + q] = h[q]; }
                blake3_compress64(m, h);
            }
            store8w(out + 32 * c, h);
            continue;
        }
        uint32_t node[16][8];
        for (int l = 0; l < leaves; l++) {
            uint32_t m[16];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const F v = ldF(enc + (size_t)(4 * l + e) * W + c);
                m[4 * e] = (uint32_t)v.re; m[4 * e + 1] = (uint32_t)(v.re >> 32); m[4 * e + 2] = (uint32_t)v.im; m[4 * e + 3] = (uint32_t)(v.im >> 32);
            }
            blake3_compress64(m, node[l]);
        }
        for (int n = leaves / 2; n >= 1; n /= 2)
            for (int i = 0; i < n; i++) {
                uint32_t m[16];
#pragma unroll
                for (int q = 0; q < 8; q++) { m[q] = node[2 * i][q]; m[8 + q] = quirk ? node[2 * i][q] : node[2 * i + 1][q]; }
                blake3_compress64(m, node[i]);
            }
        store8w(out + 32 * c, node[0]);
    }
}
int launch_col_digest(hobbit_ctx *ctx, const F *enc, size_t W, int k, int quirk, uint8_t *out) {
    HB_LAUNCH(ctx, "k_col_digest", k_col_digest, dim3(grid_for(W, 256)), dim3(256), 0, enc, W, k, quirk, out);
    return 0;
}
// one level of change_form (src/Virgo.cpp:104-118): every block of S elements becomes [even entries | odd - even]
__global__ void k_change_form_level(const F *__restrict__ in, F *__restrict__ out, size_t n, size_t S) {
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < n / 2; g += (size_t)gridDim.x * blockDim.x) {
        const size_t blk = g / (S / 2), i = g % (S / 2), pos = blk * S;
        const F a = ldF(in + pos + 2 * i), b = ldF(in + pos + 2 * i + 1);
        stF(out + pos + i, a); stF(out + pos + S / 2 + i, fsub(b, a));
    }
}
// all levels with block size <= T (T a power of two <= 4096) at once: below that size the recursion stays inside one T-block, so a
// workgroup takes a T-block through LDS (in place, pairs staged in registers between the two barriers of a level)
__global__ void __launch_bounds__(256) k_change_form_tail(F *__restrict__ data, uint32_t T) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *s = reinterpret_cast<F *>(lds_raw);
    F *blk = data + (size_t)blockIdx.x * T;
    for (uint32_t i = threadIdx.x; i < T; i += 256) stF(&s[i], ldF(blk + i));
    __syncthreads();
    for (uint32_t S = T; S >= 2; S >>= 1) {
        F a[8], b[8];                                     // T/2 <= 2048 pairs over 256 threads
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t g = threadIdx.x + 256 * u;
            if (g < T / 2) { const uint32_t pos = (g / (S / 2)) * S, i = g % (S / 2); a[u] = ldF(&s[pos + 2 * i]); b[u] = ldF(&s[pos + 2 * i + 1]); }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t g = threadIdx.x + 256 * u;
            if (g < T / 2) { const uint32_t pos = (g / (S / 2)) * S, i = g % (S / 2); stF(&s[pos + i], a[u]); stF(&s[pos + S / 2 + i], fsub(b[u], a[u])); }
        }
        __syncthreads();
    }
    for (uint32_t i = threadIdx.x; i < T; i += 256) stF(blk + i, ldF(&s[i]));
}
int launch_change_form_tail(hobbit_ctx *ctx, F *data, size_t n, uint32_t T) {
    hipFuncSetAttribute((const void *)k_change_form_tail, hipFuncAttributeMaxDynamicSharedMemorySize, 65536);
    HB_LAUNCH(ctx, "k_change_form_tail", k_change_form_tail, dim3((unsigned)(n / T)), dim3(256), (size_t)T * 16, data, T);
    return 0;
}
int launch_change_form_level(hobbit_ctx *ctx, const F *in, F *out, size_t n, size_t S) {
    HB_LAUNCH(ctx, "k_change_form_level", k_change_form_level, dim3(grid_for(n / 2, 256)), dim3(256), 0, in, out, n, S);
    return 0;
}
// paths[q][l] = levels[off_l + (pos_q >> l) ^ 1]   (src/merkle_tree.cpp:308-324)
__global__ void k_merkle_paths(const uint8_t *__restrict__ levels, size_t n, const uint64_t *__restrict__ pos, size_t nq, int depth,
                               uint8_t *__restrict__ paths) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= nq * depth) return;
    size_t q = g / depth; int l = (int)(g % depth);
    size_t off = 0, sz = n;
    for (int t = 0; t < l; t++) { off += sz; sz >>= 1; }
    size_t p = (pos[q] >> l) ^ 1;
    const uint4 *s = reinterpret_cast<const uint4 *>(levels + 32 * (off + p));
    uint4 *d = reinterpret_cast<uint4 *>(paths + 32 * g);
    d[0] = s[0]; d[1] = s[1];
}

int launch_blake3_64(hobbit_ctx *ctx, const uint8_t *in, uint8_t *out, size_t n) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_blake3_64", k_blake3_64, dim3(grid_for(n, 256)), dim3(256), 0, in, out, n);
    return 0;
}
int launch_hash_md(hobbit_ctx *ctx, const F *xyzw, const uint8_t *prev, uint8_t *out, size_t n) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_hash_md", k_hash_md, dim3(grid_for(n, 256)), dim3(256), 0, xyzw, prev, out, n);
    return 0;
}
int launch_merkle_levels(hobbit_ctx *ctx, uint8_t *levels, size_t n, int quirk) {
    size_t off = 0, tot = n;
    for (size_t sz = n / 2; sz >= 1;) {
        if (sz <= 1024) {                                   // this level and all above it in one workgroup
            HB_LAUNCH(ctx, "k_merkle_top", k_merkle_top, dim3(1), dim3(1024), 0, levels + 32 * off, levels + 32 * tot, (uint32_t)sz, quirk);
            break;
        }
        // levels of more than 1024 nodes: up to 11 of them per launch (every workgroup's 1024 nodes carry their own ancestors), but only
        // while the level is small enough that the idle upper levels of a workgroup cost less than the launches they replace
        int wide = 0; for (size_t t = sz; t > 1024; t >>= 1) wide++;
        if (sz % 1024 == 0 && sz <= ((size_t)1 << 21) && (n & (n - 1)) == 0) {
            const int g = wide < 11 ? wide : 11;
            HB_LAUNCH(ctx, "k_merkle_level", k_merkle_sub, dim3((unsigned)(sz / 1024)), dim3(1024), 0, levels + 32 * off, levels + 32 * tot, sz, g, quirk);
            for (int lv = 0; lv < g; lv++) { off = tot; tot += sz; sz >>= 1; }
            continue;
        }
        HB_LAUNCH(ctx, "k_merkle_level", k_merkle_level, dim3(grid_for(sz, 256)), dim3(256), 0, levels + 32 * off, levels + 32 * tot, sz, quirk);
        off = tot; tot += sz; sz >>= 1;
    }
    return 0;
}
// zero_rows_from: first row index that is zero in EVERY chunk (the expander codeword length; 2*half_trs = none).  The chain starts from the
// zero state -- the commit, its one caller, always does -- and only that makes the leaves of the all-zero groups the constant Z_K.
int launch_leaf_chain(hobbit_ctx *ctx, const F *tensor, size_t chunk_stride, int K, uint32_t cols, uint32_t half_trs, uint8_t *leaves, uint32_t zero_rows_from,
                      uint32_t rot_mask) {
    constexpr int NL = 1;   // 2 interleaved chains measured no faster: the kernel sits at the VALU issue limit (profiles/r01_microbench.txt)
    if (((size_t)cols * half_trs) >> 32) return ctx->fail(HOBBIT_EINVAL, "leaf chain: more than 2^32 leaves");
    const uint32_t zf = std::min((zero_rows_from + 3) / 4, half_trs);
    ZeroDig zk = {};
    if (zf < half_trs) blake3_zero_group_leaf(K, zk.w);      // no zero group (RS x RS, or graphs not finalised for this trs): nothing is filled
    // Workgroups of 256 leaves over the dense range (28 192 at 2^28, K = 32), walked by a grid capped at 4096.  Measured in one job, kernel ms
    // per step, mean of three interleaved runs: 4096 8.74, 8192 8.73, 14 096 8.79, uncapped 8.71 -- one within the run-to-run
    // spread of the other -- and 4028 (7 equal passes) 8.84; in an earlier job 2048 9.04 and 3524 (8 equal passes) 9.00 against 4096 8.89.
    // Equal passes buy nothing: the hardware hands the next workgroup to whichever CU is free, so the cap stays where it was.
    HB_LAUNCH(ctx, "k_leaf_chain", k_leaf_chain<NL>, dim3(grid_for(((size_t)cols * zf + NL - 1) / NL, 256, 4096)), dim3(256), 0, tensor, chunk_stride, K, cols,
              half_trs, leaves, zf, zk, rot_mask);
    return 0;
}
int launch_merkle_paths(hobbit_ctx *ctx, const uint8_t *levels, size_t n, const uint64_t *d_pos, size_t nq, int depth, uint8_t *d_paths) {
    size_t total = nq * depth;
    if (!total) return 0;
    HB_LAUNCH(ctx, "k_merkle_paths", k_merkle_paths, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, levels, n, d_pos, nq, depth, d_paths);
    return 0;
}

// ============================================================================================
// eq table / aggregate / gather
// ============================================================================================
// one doubling step of precompute_beta (src/utils.cpp:251-296): new[2j] = old[j] - r*old[j]; new[2j+1] = r*old[j]
__global__ void k_eq_step(const F *__restrict__ old, F *__restrict__ nw, size_t m, F r) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) {
        F o = ldF(old + j), t = fmul(r, o);
        stF(nw + 2 * j, fsub(o, t)); stF(nw + 2 * j + 1, t);
    }
}
// two doubling steps in one pass (levels with challenges ra, then rb): old[j] -> new[4j .. 4j+3]; the intermediate level is never stored
__global__ void k_eq_step2(const F *__restrict__ old, F *__restrict__ nw, size_t m, F ra, F rb) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) {
        const F o = ldF(old + j), t = fmul(ra, o), x0 = fsub(o, t);
        const F u0 = fmul(rb, x0), u1 = fmul(rb, t);
        stF(nw + 4 * j, fsub(x0, u0)); stF(nw + 4 * j + 1, u0); stF(nw + 4 * j + 2, fsub(t, u1)); stF(nw + 4 * j + 3, u1);
    }
}
// the first h <= 12 doubling steps in ONE workgroup (table in LDS, pairs staged in registers between the two barriers of a level):
// up there a level per launch is a dozen launches of a few hundred nanoseconds of work each.  r.b[i] = challenge of level i.
struct EqHead { F b[12]; };
__global__ void __launch_bounds__(256) k_eq_head(EqHead r, int h, F *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *s = reinterpret_cast<F *>(lds_raw);
    if (threadIdx.x == 0) s[0] = fmake(1);
    __syncthreads();
    for (int i = 0; i < h; i++) {
        const uint32_t m = 1u << i;
        F o[8];
#pragma unroll
        for (int u = 0; u < 8; u++) { const uint32_t j = threadIdx.x + 256 * u; if (j < m) o[u] = ldF(&s[j]); }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t j = threadIdx.x + 256 * u;
            if (j < m) { const F t = fmul(r.b[i], o[u]); stF(&s[2 * j], fsub(o[u], t)); stF(&s[2 * j + 1], t); }
        }
        __syncthreads();
    }
    for (uint32_t j = threadIdx.x; j < (1u << h); j += 256) stF(out + j, ldF(&s[j]));
}
int launch_eq_table(hobbit_ctx *ctx, CHP h_r, int k, F *d_out) {
    // head in one workgroup, then ping-pong between d_out (final) and workspace so that the last step lands in d_out
    size_t n = (size_t)1 << k;
    F *tmp = nullptr;
    const int h = k < 12 ? k : 12, rest = k - h;
    if (rest > 0) HB_TRY(ctx->workspace(n / 2 * sizeof(F), (void **)&tmp));
    const int launches = rest / 2 + rest % 2;                       // one single step if `rest` is odd, then two levels per pass
    F *cur = (launches % 2 == 0) ? d_out : tmp;
    EqHead hd;
    for (int i = 0; i < 12; i++) hd.b[i] = i < h ? h_r[k - 1 - i] : fmake(0);
    static std::atomic<uint64_t> attr_set{0};
    set_lds_limit_once(ctx, (const void *)k_eq_head, 65536, attr_set);
    HB_LAUNCH(ctx, "k_eq_head", k_eq_head, dim3(1), dim3(256), ((size_t)16 << h), hd, h, cur);
    for (int i = h; i < k;) {
        F *nxt = cur == d_out ? tmp : d_out;
        size_t m = (size_t)1 << i;
        if ((k - i) % 2) { HB_LAUNCH(ctx, "k_eq_step", k_eq_step, dim3(grid_for(m, 256)), dim3(256), 0, cur, nxt, m, h_r[k - 1 - i]); i += 1; }
        else { HB_LAUNCH(ctx, "k_eq_step", k_eq_step2, dim3(grid_for(m, 256)), dim3(256), 0, cur, nxt, m, h_r[k - 1 - i], h_r[k - 2 - i]); i += 2; }
        cur = nxt;
    }
    return 0;
}
// aggr[j] = sum_i beta[i] * poly[i*M + j]   (src/Our_PC.cpp:258-272)
// K <= 64 coefficients passed by value in the kernel arguments (1 KB): no host buffer, no copy, no synchronisation
struct AggCoef { F b[64]; };
// a later slice of a sum over more than 64 chunks: aggr[j] += sum_i beta[i] * poly[i*M + j], continuing from what aggr holds
__global__ void k_aggregate_arg_acc(const F *__restrict__ poly, size_t M, int K, AggCoef beta, F *__restrict__ aggr) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < M; j += (size_t)gridDim.x * blockDim.x) {
        F acc = ldF(aggr + j);
        for (int i = 0; i < K; i++) acc = fadd(acc, fmul(beta.b[i], ldF(poly + (size_t)i * M + j)));
        stF(aggr + j, acc);
    }
}
__global__ void k_aggregate_arg(const F *__restrict__ poly, size_t M, int K, AggCoef beta, F *__restrict__ aggr) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < M; j += (size_t)gridDim.x * blockDim.x) {
        F acc = fmake(0);
        for (int i = 0; i < K; i++) acc = fadd(acc, fmul(beta.b[i], ldF(poly + (size_t)i * M + j)));
        stF(aggr + j, acc);
    }
}
int launch_aggregate(hobbit_ctx *ctx, const F *poly, size_t M, int K, CHP h_beta, F *aggr) {
    if (K <= 64) {
        AggCoef cf;
        for (int i = 0; i < 64; i++) cf.b[i] = i < K ? h_beta[i] : fmake(0);
        HB_LAUNCH(ctx, "k_aggregate", k_aggregate_arg, dim3(grid_for(M, 256)), dim3(256), 0, poly, M, K, cf, aggr);
        return 0;
    }
    // more chunks than fit the argument block: slices of 64, each with its coefficients in its own launch's arguments, the later ones continuing
    // the sum the earlier ones left in aggr -- the same additions in the same order i = 0 .. K-1 (canonical values survive the round trip through
    // memory unchanged).  Nothing the kernels read lives in a buffer a later call on this context could rewrite while they are still queued.
    for (int i0 = 0; i0 < K; i0 += 64) {
        const int k = K - i0 < 64 ? K - i0 : 64;
        AggCoef cf;
        for (int i = 0; i < 64; i++) cf.b[i] = i < k ? h_beta[i0 + i] : fmake(0);
        if (i0 == 0) HB_LAUNCH(ctx, "k_aggregate", k_aggregate_arg, dim3(grid_for(M, 256)), dim3(256), 0, poly, M, k, cf, aggr);
        else HB_LAUNCH(ctx, "k_aggregate", k_aggregate_arg_acc, dim3(grid_for(M, 256)), dim3(256), 0, poly + (size_t)i0 * M, M, k, cf, aggr);
    }
    return 0;
}
// reply[q*K + i] = tensor[i][col_q][row_q]   (src/Our_PC.cpp:291-305, codeword-major tensor)
// rows >= rows_valid of a column are zero BY CONSTRUCTION and may never have been written (a commitment's RS x expander tensor past its codeword
// length: commit_impl): they are answered as zero, not read
__global__ void k_gather(const F *__restrict__ tensor, size_t chunk_stride, uint32_t rows2, int K, const uint32_t *__restrict__ rows,
                         const uint32_t *__restrict__ cols, size_t nq, F *__restrict__ reply, uint32_t rows_valid, uint32_t rot_mask) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= nq * K) return;
    size_t q = g / K; int i = (int)(g % K);
    stF(reply + g, rows[q] < rows_valid ? ldF(tensor + (size_t)i * chunk_stride + (size_t)cols[q] * rows2 + msg_rot_row(rows[q], cols[q], rot_mask)) : fmake(0));
}
int launch_gather(hobbit_ctx *ctx, const F *tensor, size_t chunk_stride, uint32_t rows2, int K, const uint32_t *d_rows, const uint32_t *d_cols,
                  size_t nq, F *d_reply, uint32_t rows_valid, uint32_t rot_mask) {
    size_t total = nq * K;
    if (!total) return 0;
    HB_LAUNCH(ctx, "k_gather", k_gather, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, tensor, chunk_stride, rows2, K, d_rows, d_cols, nq, d_reply,
              rows_valid, rot_mask);
    return 0;
}
// the unwritten tails made real: rows [rows_valid, rows2) of every column := 0 (before a raw pointer to the tensor leaves the library)
__global__ void k_zero_rows(F *__restrict__ tensor, size_t ncols, uint32_t rows2, uint32_t rows_valid) {
    const uint32_t span = rows2 - rows_valid;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < ncols * span; g += (size_t)gridDim.x * blockDim.x)
        stF(tensor + (g / span) * rows2 + rows_valid + (g % span), fmake(0));
}
int launch_zero_rows(hobbit_ctx *ctx, F *tensor, size_t ncols, uint32_t rows2, uint32_t rows_valid) {
    if (rows_valid >= rows2 || !ncols) return 0;
    HB_LAUNCH(ctx, "k_zero_rows", k_zero_rows, dim3(grid_for(ncols * (rows2 - rows_valid), 256, 8192)), dim3(256), 0, tensor, ncols, rows2, rows_valid);
    return 0;
}
// row `row` of one chunk in the reference's row-major order: out[c] = tensor[c*rows2 + row]
__global__ void k_tensor_row(const F *__restrict__ chunk, uint32_t rows2, uint32_t cols, uint32_t row, F *__restrict__ out, uint32_t rows_valid, uint32_t rot_mask) {
    uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < cols) stF(out + c, row < rows_valid ? ldF(chunk + (size_t)c * rows2 + msg_rot_row(row, c, rot_mask)) : fmake(0));
}
int launch_tensor_row(hobbit_ctx *ctx, const F *chunk, uint32_t rows2, uint32_t cols, uint32_t row, F *d_out, uint32_t rows_valid, uint32_t rot_mask) {
    HB_LAUNCH(ctx, "k_tensor_row", k_tensor_row, dim3((cols + 255) / 256), dim3(256), 0, chunk, rows2, cols, row, d_out, rows_valid, rot_mask);
    return 0;
}
// A rotated message half made linear, in place (before a raw pointer to the tensor leaves the library).  One workgroup per column and pass:
// the rot_mask + 1 message rows (64 KiB at trs = 4096) come into LDS through the rotated index and go back in row order.
__global__ void __launch_bounds__(1024)
k_unrotate_msg(F *__restrict__ tensor, size_t ncols, uint32_t rows2, uint32_t rot_mask) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    F *s = reinterpret_cast<F *>(lds_raw);
    for (size_t c = blockIdx.x; c < ncols; c += gridDim.x) {
        F *col = tensor + c * rows2;
        for (uint32_t r = threadIdx.x; r <= rot_mask; r += blockDim.x) stF(&s[r], ldF(col + msg_rot_row(r, (uint32_t)c, rot_mask)));
        __syncthreads();                                            // the whole ring is in LDS before any of it is overwritten
        for (uint32_t r = threadIdx.x; r <= rot_mask; r += blockDim.x) stF(col + r, ldF(&s[r]));
        __syncthreads();
    }
}
int launch_unrotate_msg(hobbit_ctx *ctx, F *tensor, size_t ncols, uint32_t rows2, uint32_t rot_mask) {
    if (!rot_mask || !ncols) return 0;
    const size_t lds = ((size_t)rot_mask + 1) * sizeof(F);
    if ((rot_mask & (rot_mask + 1)) || rot_mask >= rows2 || lds > 64 * 1024) return ctx->fail(HOBBIT_EINVAL, "unrotate: the message ring must be a power of two of at most 4096 rows");
    hipFuncSetAttribute((const void *)k_unrotate_msg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    HB_LAUNCH(ctx, "k_unrotate_msg", k_unrotate_msg, dim3(grid_for(ncols, 1, 65536)), dim3(1024), lds, tensor, ncols, rows2, rot_mask);
    return 0;
}

// ============================================================================================
// The half form of a commitment's tensor (hobbit_half.hpp; include/hobbit_real.h): columns 0 .. cols / 2 of every chunk are in memory, column
// c > cols / 2 is the conjugate of column cols - c.  Kernels of their own beside k_leaf_chain, k_gather and k_tensor_row, which stay as they are.
// ============================================================================================
// the four elements of a leaf group conjugated in place: words 4e + 2, 4e + 3 are the imaginary part of element e
__device__ __forceinline__ void conj16w(uint32_t m[16]) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const uint64_t im = ((uint64_t)m[4 * e + 3] << 32) | m[4 * e + 2], v = im ? P61 - im : 0;
        m[4 * e + 2] = (uint32_t)v; m[4 * e + 3] = (uint32_t)(v >> 32);
    }
}
// k_leaf_chain (NL = 1) over a half tensor: the same dense index over all `cols` columns and the zf non-zero groups, the same fill of the zero
// groups' leaves.  Leaf (j, c) with c > cols / 2 reads the group of column cols - c -- the same contiguous, aligned 64 bytes per chunk, rotated by
// that column's batch index -- and conjugates it before hashing.
__global__ void __launch_bounds__(256)
k_leaf_chain_half(const F *__restrict__ tensor, uint32_t K, uint32_t cols, uint32_t half_trs, uint8_t *__restrict__ leaves, uint32_t zf, ZeroDig zk, uint32_t rot_mask) {
    const uint32_t stride = gridDim.x * blockDim.x, rows2 = 4 * half_trs;
    {
        const size_t fill16 = 2 * (size_t)(half_trs - zf) * cols;
        uint4 *tail = reinterpret_cast<uint4 *>(leaves + 32 * (size_t)zf * cols);
        const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;     // stride is even: a thread stores the same half of Z_K every time
        const uint4 v = (t & 1) ? make_uint4(zk.w[4], zk.w[5], zk.w[6], zk.w[7]) : make_uint4(zk.w[0], zk.w[1], zk.w[2], zk.w[3]);
        for (size_t u = t; u < fill16; u += stride) tail[u] = v;
    }
    const uint32_t total = cols * zf;
    for (uint32_t g = blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        const uint32_t c = g / zf, j = g - c * zf, sc = half_src_col(c, cols);
        const bool cj = half_is_conj(c, cols);
        // a column of the main block keeps its place and its rotation from chunk to chunk (hc columns on: a multiple of the rotation's period);
        // the strip's column of chunk i is batch column K hc + i, with a rotation of its own
        const bool strip = sc == cols / 2;
        const F *p0 = tensor + half_at(0, sc, 4 * j, cols, K, rows2, rot_mask);
        const size_t step = strip ? (size_t)rows2 : (size_t)(cols / 2) * rows2;
        uint32_t st[8];
#pragma unroll
        for (int q = 0; q < 8; q++) st[q] = 0;
        for (uint32_t i = 0; i < K; i++) {
            uint32_t m[16], h[8];
            load16w(strip && rot_mask ? tensor + half_at(i, sc, 4 * j, cols, K, rows2, rot_mask) : p0 + (size_t)i * step, m);
            if (cj) conj16w(m);
            blake3_compress64(m, h);
#pragma unroll
            for (int q = 0; q < 8; q++) { m[q] = h[q]; m[8 + q] = st[q]; }
            blake3_compress64(m, st);
        }
        store8w(leaves + 32 * ((size_t)j * cols + c), st);
    }
}
int launch_leaf_chain_half(hobbit_ctx *ctx, const F *tensor, int K, uint32_t cols, uint32_t half_trs, uint8_t *leaves, uint32_t zero_rows_from, uint32_t rot_mask) {
    if (((size_t)cols * half_trs) >> 32) return ctx->fail(HOBBIT_EINVAL, "leaf chain: more than 2^32 leaves");
    const uint32_t zf = std::min((zero_rows_from + 3) / 4, half_trs);
    ZeroDig zk = {};
    if (zf < half_trs) blake3_zero_group_leaf(K, zk.w);
    HB_LAUNCH(ctx, "k_leaf_chain_half", k_leaf_chain_half, dim3(grid_for((size_t)cols * zf, 256, 4096)), dim3(256), 0, tensor, (uint32_t)K, cols, half_trs, leaves, zf, zk,
              rot_mask);
    return 0;
}
// one element of the full tensor read from the half one: zero past rows_valid; column c > cols / 2 is answered through half_ref -- the conjugate of
// the same row of column cols - c under RS x expander (LIN = 1), of the negated row under RS x RS (LIN = 0, never rotated, every row valid)
template <int LIN>
__device__ __forceinline__ F half_load(const F *__restrict__ tensor, uint32_t i, uint32_t c, uint32_t r, uint32_t cols, uint32_t K, uint32_t rows2, uint32_t rows_valid,
                                       uint32_t rot_mask) {
    if (r >= rows_valid) return fmake(0);
    const HalfRef h = half_ref(r, c, cols, rows2, LIN);
    const F v = ldF(tensor + half_at(i, h.col, h.row, cols, K, rows2, rot_mask));
    return h.conj ? fconj(v) : v;
}
template <int LIN>
__global__ void k_gather_half(const F *__restrict__ tensor, uint32_t cols, uint32_t rows2, uint32_t K, const uint32_t *__restrict__ rows, const uint32_t *__restrict__ qcols,
                              size_t nq, F *__restrict__ reply, uint32_t rows_valid, uint32_t rot_mask) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= nq * K) return;
    const size_t q = g / K; const uint32_t i = (uint32_t)(g % K);
    stF(reply + g, half_load<LIN>(tensor, i, qcols[q], rows[q], cols, K, rows2, rows_valid, rot_mask));
}
int launch_gather_half(hobbit_ctx *ctx, const F *tensor, uint32_t cols, uint32_t rows2, int K, const uint32_t *d_rows, const uint32_t *d_cols, size_t nq, F *d_reply,
                       uint32_t rows_valid, uint32_t rot_mask, int lin) {
    const size_t total = nq * K;
    if (!total) return 0;
    if (lin) HB_LAUNCH(ctx, "k_gather_half", k_gather_half<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, tensor, cols, rows2, (uint32_t)K, d_rows, d_cols, nq, d_reply,
                       rows_valid, rot_mask);
    else HB_LAUNCH(ctx, "k_gather_half_rs", k_gather_half<0>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, tensor, cols, rows2, (uint32_t)K, d_rows, d_cols, nq, d_reply,
                   rows_valid, rot_mask);
    return 0;
}
template <int LIN>
__global__ void k_tensor_row_half(const F *__restrict__ tensor, uint32_t chunk, uint32_t K, uint32_t rows2, uint32_t cols, uint32_t row, F *__restrict__ out,
                                  uint32_t rows_valid, uint32_t rot_mask) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < cols) stF(out + c, half_load<LIN>(tensor, chunk, c, row, cols, K, rows2, rows_valid, rot_mask));
}
int launch_tensor_row_half(hobbit_ctx *ctx, const F *tensor, uint32_t chunk, int K, uint32_t rows2, uint32_t cols, uint32_t row, F *d_out, uint32_t rows_valid,
                           uint32_t rot_mask, int lin) {
    if (lin) HB_LAUNCH(ctx, "k_tensor_row_half", k_tensor_row_half<1>, dim3((cols + 255) / 256), dim3(256), 0, tensor, chunk, (uint32_t)K, rows2, cols, row, d_out, rows_valid, rot_mask);
    else HB_LAUNCH(ctx, "k_tensor_row_half_rs", k_tensor_row_half<0>, dim3((cols + 255) / 256), dim3(256), 0, tensor, chunk, (uint32_t)K, rows2, cols, row, d_out, rows_valid, rot_mask);
    return 0;
}
// The mirror that materialises the full linear tensor [K][cols][rows2] from the half one (hobbit_commitment_tensor_dev): one workgroup per
// full column and pass, reads and writes contiguous along the rows (RS x RS: the reads of a mirrored column run backwards); the implicit zeros
// become real ones and a rotated message half a linear one.
template <int LIN>
__global__ void __launch_bounds__(256)
k_half_expand(const F *__restrict__ tensor, F *__restrict__ full, uint32_t cols, uint32_t K, uint32_t rows2, uint32_t rows_valid, uint32_t rot_mask) {
    const size_t ncols = (size_t)K * cols;
    for (size_t gc = blockIdx.x; gc < ncols; gc += gridDim.x) {
        const uint32_t i = (uint32_t)(gc / cols), c = (uint32_t)(gc % cols);
        for (uint32_t r = threadIdx.x; r < rows2; r += blockDim.x) stF(full + gc * rows2 + r, half_load<LIN>(tensor, i, c, r, cols, K, rows2, rows_valid, rot_mask));
    }
}
int launch_half_expand(hobbit_ctx *ctx, const F *tensor, F *full, uint32_t cols, int K, uint32_t rows2, uint32_t rows_valid, uint32_t rot_mask, int lin) {
    if (lin) HB_LAUNCH(ctx, "k_half_expand", k_half_expand<1>, dim3(grid_for((size_t)K * cols, 1, 65536)), dim3(256), 0, tensor, full, cols, (uint32_t)K, rows2, rows_valid, rot_mask);
    else HB_LAUNCH(ctx, "k_half_expand_rs", k_half_expand<0>, dim3(grid_for((size_t)K * cols, 1, 65536)), dim3(256), 0, tensor, full, cols, (uint32_t)K, rows2, rows_valid, rot_mask);
    return 0;
}
// the 16 words a mirrored leaf hashes, from its stored group's 16 words m and the next group's first element n4
__device__ __forceinline__ void leaf_rs_mirror_words(const uint32_t m[16], const uint4 &n4, uint32_t w[16]) {
    w[0] = n4.x; w[1] = n4.y; w[2] = n4.z; w[3] = n4.w;
#pragma unroll
    for (int q = 0; q < 4; q++) { w[4 + q] = m[12 + q]; w[8 + q] = m[8 + q]; w[12 + q] = m[4 + q]; }
    conj16w(w);
}
// st = H( H(m) | st ); m is consumed
__device__ __forceinline__ void leaf_chain_step(uint32_t m[16], uint32_t st[8]) {
    uint32_t h[8];
    blake3_compress64(m, h);
#pragma unroll
    for (int q = 0; q < 8; q++) { m[q] = h[q]; m[8 + q] = st[q]; }
    blake3_compress64(m, st);
}
// The leaf chain over an RS x RS half tensor (include/hobbit_real_rs.h; DESIGN.md section 4, "Base-field polynomials under RS x RS").  The column
// code is a transform of rows2 points, so T(r, cols - c) = conj(T((rows2 - r) mod rows2, c)): leaf (j', cols - sc) hashes the conjugates of stored
// rows (rows2 - 4 j' - e) mod rows2, e = 0 .. 3, of column sc.  With G = rows2 / 4 groups and g = G - 1 - j' these are row 4 (g + 1) mod rows2 --
// the first row of the NEXT group, wrapping to row 0 -- and then rows 4g + 3, 4g + 2, 4g + 1.  One thread owns stored group (g, sc), sc <= cols / 2:
// per chunk it loads its 64 bytes and that one element beyond them and updates two chains, leaf (g, sc) and, for 0 < sc < cols / 2, leaf
// (G - 1 - g, cols - sc): 80 bytes per two leaves.  g is the fastest thread index; there are no zero groups (RS x RS fills all rows2 rows) and no rotation.
// 82 VGPRs, no scratch (forcing eight waves spilled 80 bytes); the per-leaf form -- one thread per leaf, 57 VGPRs -- measured 0.36 ms slower at
// (2^28, 32, 128) and was not kept.
__global__ void __launch_bounds__(256)
k_leaf_chain_half_rs(const F *__restrict__ tensor, uint32_t K, uint32_t cols, uint32_t G, uint8_t *__restrict__ leaves) {
    const uint32_t stride = gridDim.x * blockDim.x, rows2 = 4 * G, hc = cols / 2;
    const uint32_t total = (hc + 1) * G;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const uint32_t sc = t / G, g = t - sc * G;
        const bool strip = sc == hc, two = sc > 0 && sc < hc;
        const F *p0 = tensor + half_col(0, sc, cols, K) * rows2;
        const size_t step = strip ? (size_t)rows2 : (size_t)hc * rows2;
        const uint32_t nx = (4 * g + 4) & (rows2 - 1);
        uint32_t st[8], sm[8];
#pragma unroll
        for (int q = 0; q < 8; q++) st[q] = sm[q] = 0;
        for (uint32_t i = 0; i < K; i++) {
            const F *col = p0 + (size_t)i * step;
            uint32_t m[16], w[16];
            load16w(col + 4 * g, m);
            if (two) leaf_rs_mirror_words(m, *reinterpret_cast<const uint4 *>(col + nx), w);
            leaf_chain_step(m, st);
            if (two) leaf_chain_step(w, sm);
        }
        store8w(leaves + 32 * ((size_t)g * cols + sc), st);
        if (two) store8w(leaves + 32 * ((size_t)(G - 1 - g) * cols + (cols - sc)), sm);
    }
}
int launch_leaf_chain_half_rs(hobbit_ctx *ctx, const F *tensor, int K, uint32_t cols, uint32_t half_trs, uint8_t *leaves) {
    if (((size_t)cols * half_trs) >> 32) return ctx->fail(HOBBIT_EINVAL, "leaf chain: more than 2^32 leaves");
    if (!half_trs || (half_trs & (half_trs - 1))) return ctx->fail(HOBBIT_EINVAL, "leaf chain (RS x RS half form): 2 trs must be a power of two");
    HB_LAUNCH(ctx, "k_leaf_chain_half_rs", k_leaf_chain_half_rs, dim3(grid_for((size_t)(cols / 2 + 1) * half_trs, 256, 4096)), dim3(256), 0, tensor, (uint32_t)K, cols, half_trs,
              leaves);
    return 0;
}
// (x, 0) per coefficient: the F form of a real vector
__global__ void k_widen_real(const uint64_t *__restrict__ x, F *__restrict__ o, size_t n) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) stF(o + j, fmake(x[j]));
}
int launch_widen_real(hobbit_ctx *ctx, const uint64_t *x, F *o, size_t n) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_widen_real", k_widen_real, dim3(grid_for(n, 256)), dim3(256), 0, x, o, n);
    return 0;
}
// launch_aggregate over a real polynomial: aggr[j] = sum_i beta[i] * poly[i*M + j], each product two F_p products (beta.re x, beta.im x) -- what
// fmul(beta, (x, 0)) gives, canonical either way -- and half the bytes read.  ACC continues from what aggr holds (slices of 64 chunks).
template <bool ACC>
__global__ void k_aggregate_real(const uint64_t *__restrict__ poly, size_t M, int K, AggCoef beta, F *__restrict__ aggr) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < M; j += (size_t)gridDim.x * blockDim.x) {
        F acc = ACC ? ldF(aggr + j) : fmake(0);
        for (int i = 0; i < K; i++) { const uint64_t x = poly[(size_t)i * M + j]; acc = fadd(acc, fmake(mulp(beta.b[i].re, x), mulp(beta.b[i].im, x))); }
        stF(aggr + j, acc);
    }
}
int launch_aggregate_real(hobbit_ctx *ctx, const uint64_t *poly, size_t M, int K, CHP h_beta, F *aggr) {
    for (int i0 = 0; i0 < K; i0 += 64) {
        const int k = K - i0 < 64 ? K - i0 : 64;
        AggCoef cf;
        for (int i = 0; i < 64; i++) cf.b[i] = i < k ? h_beta[i0 + i] : fmake(0);
        if (i0 == 0) HB_LAUNCH(ctx, "k_aggregate_real", k_aggregate_real<false>, dim3(grid_for(M, 256)), dim3(256), 0, poly, M, k, cf, aggr);
        else HB_LAUNCH(ctx, "k_aggregate_real", k_aggregate_real<true>, dim3(grid_for(M, 256)), dim3(256), 0, poly + (size_t)i0 * M, M, k, cf, aggr);
    }
    return 0;
}
// multilinear evaluation fold step of evaluate_vector (src/utils.cpp:789-802): v'[j] = (1-r) v[2j] + r v[2j+1]
__global__ void k_eval_fold(const F *__restrict__ v, F *__restrict__ o, size_t L, F r) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x) {
        F a = ldF(v + 2 * j), b = ldF(v + 2 * j + 1);
        stF(o + j, fadd(a, fmul(r, fsub(b, a))));
    }
}
int launch_eval_fold(hobbit_ctx *ctx, const F *v, F *o, size_t L, F r) {
    HB_LAUNCH(ctx, "k_eval_fold", k_eval_fold, dim3(grid_for(L, 256)), dim3(256), 0, v, o, L, r);
    return 0;
}
// Two levels per launch (64 contiguous bytes per lane, the access pattern of k_sc2_double's fold): o[j] from v[4j .. 4j+3] with (r0, r1),
// level by level in the same order as two k_eval_fold launches -- the same field operations, half the launches, 2/3 of the traffic.
__global__ void k_eval_fold2(const F *__restrict__ v, F *__restrict__ o, size_t L, F r0, F r1) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x) {
        const F a = ldF(v + 4 * j), b = ldF(v + 4 * j + 1), c = ldF(v + 4 * j + 2), d = ldF(v + 4 * j + 3);
        const F x = fadd(a, fmul(r0, fsub(b, a))), y = fadd(c, fmul(r0, fsub(d, c)));
        stF(o + j, fadd(x, fmul(r1, fsub(y, x))));
    }
}
// The last levels (n <= 4096 elements) in one workgroup: the table lives in LDS, one barrier per level.
struct EvalTailR { F r[12]; };
__global__ void __launch_bounds__(1024) k_eval_tail(const F *__restrict__ v, F *__restrict__ o, uint32_t n, int levels, EvalTailR rr) {
    __shared__ F t[4096];
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) t[i] = ldF(v + i);
    __syncthreads();
    for (int l = 0; l < levels; l++) {
        const uint32_t L = n >> (l + 1);
        F out[2]; int cnt = 0;
        for (uint32_t j = threadIdx.x; j < L; j += blockDim.x) { const F a = t[2 * j], b = t[2 * j + 1]; out[cnt++] = fadd(a, fmul(rr.r[l], fsub(b, a))); }
        __syncthreads();
        cnt = 0;
        for (uint32_t j = threadIdx.x; j < L; j += blockDim.x) t[j] = out[cnt++];
        __syncthreads();
    }
    if (threadIdx.x == 0) stF(o, t[0]);
}
int launch_eval_fold2(hobbit_ctx *ctx, const F *v, F *o, size_t L, F r0, F r1) {
    HB_LAUNCH(ctx, "k_eval_fold", k_eval_fold2, dim3(grid_for(L, 256)), dim3(256), 0, v, o, L, r0, r1);
    return 0;
}
int launch_eval_tail(hobbit_ctx *ctx, const F *v, F *o, size_t n, int levels, const F *r) {
    if (n > 4096 || levels > 12 || ((size_t)1 << levels) != n) return ctx->fail(HOBBIT_EINVAL, "eval_tail: at most 4096 elements");
    EvalTailR rr; for (int i = 0; i < levels; i++) rr.r[i] = r[i];
    HB_LAUNCH(ctx, "k_eval_fold", k_eval_tail, dim3(1), dim3(1024), 0, v, o, (uint32_t)n, levels, rr);
    return 0;
}

// ============================================================================================
// code-membership / FFT-as-sumcheck tables
// ============================================================================================
// A = H^T beta (src/sumcheck.cpp:2888-2929) as one CSR gather: A[a] = sum_e w_e * beta[idx_e]
// (the "-= beta" identity terms are edges of weight -1)
__global__ void k_csr_gather(const uint32_t *__restrict__ rowptr, const uint32_t *__restrict__ idx, const F *__restrict__ w,
                             const F *__restrict__ x, F *__restrict__ y, size_t rows) {
    for (size_t a = blockIdx.x * (size_t)blockDim.x + threadIdx.x; a < rows; a += (size_t)gridDim.x * blockDim.x) {
        F acc = fmake(0);
        for (uint32_t e = rowptr[a]; e < rowptr[a + 1]; e++) acc = fadd(acc, fmul(ldF(x + idx[e]), ldF(w + e)));
        stF(y + a, acc);
    }
}
int launch_csr_gather(hobbit_ctx *ctx, const uint32_t *rowptr, const uint32_t *idx, const F *w, const F *x, F *y, size_t rows) {
    if (!rows) return 0;
    HB_LAUNCH(ctx, "k_csr_gather", k_csr_gather, dim3(grid_for(rows, 256)), dim3(256), 0, rowptr, idx, w, x, y, rows);
    return 0;
}
// one doubling level of phiGInit (src/utils.cpp:694-755): for b < half, l = b, r = b ^ half:
//   t2 = rx * pm[b << m];  g[r] = g[l] * ((1-rx) - t2);  g[l] = g[l] * ((1-rx) + t2)
// last_only (the non-inverse table's closing loop) updates g[l] alone.
__global__ void k_phi_step(F *__restrict__ g, size_t half, int m, F rx, const F *__restrict__ pm, int last_only) {
    const F t1 = fsub(fmake(1), rx);
    for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < half; b += (size_t)gridDim.x * blockDim.x) {
        const F t2 = fmul(rx, ldF(pm + (b << m))), gl = ldF(g + b);
        if (!last_only) stF(g + (b ^ half), fmul(gl, fsub(t1, t2)));
        stF(g + b, fmul(gl, fadd(t1, t2)));
    }
}
// levels 1..h (h <= 11) of the forward table in one workgroup: g[0] = scale, then h in-place doubling levels in LDS.  rx.b[i-1] = the
// challenge of level i (= h_rx[n - i]).
__global__ void __launch_bounds__(256) k_phi_head(F *__restrict__ g, int n, int h, EqHead rx, F scale, const F *__restrict__ pm) {
    __shared__ F s[2048];
    if (threadIdx.x == 0) s[0] = scale;
    __syncthreads();
    for (int i = 1; i <= h; i++) {
        const uint32_t half = 1u << (i - 1);
        const F r = rx.b[i - 1], t1 = fsub(fmake(1), r);
        for (uint32_t b = threadIdx.x; b < half; b += 256) {
            const F t2 = fmul(r, ldF(pm + ((size_t)b << (n - i)))), gl = ldF(&s[b]);
            stF(&s[b ^ half], fmul(gl, fsub(t1, t2)));
            stF(&s[b], fmul(gl, fadd(t1, t2)));
        }
        __syncthreads();
    }
    for (uint32_t j = threadIdx.x; j < (1u << h); j += 256) stF(g + j, ldF(&s[j]));
}
int launch_phi_head(hobbit_ctx *ctx, F *g, int n, int h, CHP h_rx, F scale, const F *pm) {
    if (h < 1 || h > 11 || h >= n) return ctx->fail(HOBBIT_EINVAL, "phi_head: 1 <= h <= min(11, n - 1)");
    EqHead rx;
    for (int i = 1; i <= 12; i++) rx.b[i - 1] = i <= h ? h_rx[n - i] : fmake(0);
    HB_LAUNCH(ctx, "k_phi_step", k_phi_head, dim3(1), dim3(256), 0, g, n, h, rx, scale, pm);
    return 0;
}
int launch_phi_step(hobbit_ctx *ctx, F *g, size_t half, int m, F rx, const F *pm, int last_only) {
    HB_LAUNCH(ctx, "k_phi_step", k_phi_step, dim3(grid_for(half, 256)), dim3(256), 0, g, half, m, rx, pm, last_only);
    return 0;
}
// prepare_matrix(transpose(M), r) step (src/utils.cpp:758-775): fold adjacent ROWS of a row-major matrix
__global__ void k_fold_rows(const F *__restrict__ in, F *__restrict__ out, size_t out_rows, size_t cols, F r) {
    const size_t total = out_rows * cols;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < total; g += (size_t)gridDim.x * blockDim.x) {
        const size_t j = g / cols, c = g % cols;
        const F a = ldF(in + (2 * j) * cols + c), b = ldF(in + (2 * j + 1) * cols + c);
        stF(out + g, fadd(a, fmul(r, fsub(b, a))));
    }
}
int launch_fold_rows(hobbit_ctx *ctx, const F *in, F *out, size_t out_rows, size_t cols, F r) {
    if (!out_rows || !cols) return 0;
    HB_LAUNCH(ctx, "k_fold_rows", k_fold_rows, dim3(grid_for(out_rows * cols, 256)), dim3(256), 0, in, out, out_rows, cols, r);
    return 0;
}

// ---- dense helpers of recursive_prover_Spielman (src/PC_utils.cpp:293-345) -------------------
// out[i] = sum_j v[j] * M[i][j]   (one workgroup per row; aggr_c = [M' | C] . s)
__global__ void __launch_bounds__(256) k_matvec_rows(const F *__restrict__ Mx, size_t cols, const F *__restrict__ v, F *__restrict__ out) {
    const F *row = Mx + (size_t)blockIdx.x * cols;
    F c[1] = {fmake(0)};
    for (size_t j = threadIdx.x; j < cols; j += blockDim.x) c[0] = fadd(c[0], fmul(ldF(v + j), ldF(row + j)));
    __shared__ F red[4];
    F sm = wave_sum(c[0]);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sm;
    __syncthreads();
    if (threadIdx.x == 0) stF(out + blockIdx.x, fadd(fadd(red[0], red[1]), fadd(red[2], red[3])));
}
// out[i] = sum_j v[j] * M[j][i]   (evals = beta^T [M' | C]): lanes run along i (coalesced), the row range is
// split over blockIdx.y into partial sums that a second launch adds up
__global__ void __launch_bounds__(256) k_vecmat(const F *__restrict__ Mx, size_t rows, size_t cols, const F *__restrict__ v, F *__restrict__ part) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= cols) return;
    const size_t per = (rows + gridDim.y - 1) / gridDim.y, j0 = blockIdx.y * per, j1 = j0 + per < rows ? j0 + per : rows;
    F acc = fmake(0);
    for (size_t j = j0; j < j1; j++) acc = fadd(acc, fmul(ldF(v + j), ldF(Mx + j * cols + i)));
    stF(part + (size_t)blockIdx.y * cols + i, acc);
}
__global__ void __launch_bounds__(256) k_colsum(const F *__restrict__ part, size_t nparts, size_t cols, F *__restrict__ out) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= cols) return;
    F acc = fmake(0);
    for (size_t p = 0; p < nparts; p++) acc = fadd(acc, ldF(part + p * cols + i));
    stF(out + i, acc);
}
__global__ void k_scatter(const uint64_t *__restrict__ idx, const F *__restrict__ val, size_t n, F *__restrict__ out) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g < n) stF(out + idx[g], ldF(val + g));
}
// y += a * x
__global__ void k_axpy(F *__restrict__ y, const F *__restrict__ x, F a, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) stF(y + i, fadd(ldF(y + i), fmul(a, ldF(x + i))));
}
int launch_matvec_rows(hobbit_ctx *ctx, const F *Mx, size_t rows, size_t cols, const F *v, F *out) {
    if (!rows) return 0;
    HB_LAUNCH(ctx, "k_matvec_rows", k_matvec_rows, dim3((unsigned)rows), dim3(256), 0, Mx, cols, v, out);
    return 0;
}
int launch_vecmat(hobbit_ctx *ctx, const F *Mx, size_t rows, size_t cols, const F *v, F *out) {
    // enough row slices to fill the chip: (cols/256) x nparts workgroups
    size_t nparts = 1;
    while (nparts < 256 && nparts * 2 <= rows && ((cols + 255) / 256) * nparts < 2048) nparts *= 2;
    F *part; HB_TRY(ctx->workspace(nparts * cols * sizeof(F), (void **)&part));
    HB_LAUNCH(ctx, "k_vecmat", k_vecmat, dim3((unsigned)((cols + 255) / 256), (unsigned)nparts), dim3(256), 0, Mx, rows, cols, v, part);
    HB_LAUNCH(ctx, "k_colsum", k_colsum, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, part, nparts, cols, out);
    return 0;
}
// out[q*m + j] = src[idx[q]*bmul + j*stride]: query replies (WHIR: 16 consecutive regrouped elements; shockwave: one column of k rows)
__global__ void k_gather_strided(const F *__restrict__ src, const uint64_t *__restrict__ idx, size_t nq, uint32_t m, size_t bmul, size_t stride, F *__restrict__ out) {
    size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= nq * m) return;
    size_t q = t / m, j = t % m;
    stF(out + t, ldF(src + idx[q] * bmul + j * stride));
}
int launch_gather_strided(hobbit_ctx *ctx, const F *src, const uint64_t *d_idx, size_t nq, uint32_t m, size_t bmul, size_t stride, F *out) {
    if (!nq) return 0;
    HB_LAUNCH(ctx, "k_gather_strided", k_gather_strided, dim3((unsigned)((nq * m + 255) / 256)), dim3(256), 0, src, d_idx, nq, m, bmul, stride, out);
    return 0;
}
int launch_scatter(hobbit_ctx *ctx, const uint64_t *idx, const F *val, size_t n, F *out) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_scatter", k_scatter, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, idx, val, n, out);
    return 0;
}
int launch_axpy(hobbit_ctx *ctx, F *y, const F *x, F a, size_t n) {
    HB_LAUNCH(ctx, "k_axpy", k_axpy, dim3(grid_for(n, 256)), dim3(256), 0, y, x, a, n);
    return 0;
}

// ============================================================================================
// Sumcheck (src/sumcheck.cpp:2391-2460 two-product, 1974-2058 three-product)
//
// Per round: one streaming kernel over the tables produces per-workgroup partial sums of the round
// polynomial's coefficients, a one-workgroup kernel reduces them to 3-4 field elements, and those
// 48-64 bytes go to the HOST, which runs the MiMC transcript (3-4 x 161 strictly sequential
// cubings: ~4 us on a CPU core, ~80 us on a GPU scalar unit -- measured 5.7 of 6.7 ms at n = 2^24
// with the transcript on the device) and passes the next challenge to the next launch as a kernel
// argument.  Once the tables are down to SC_TAIL elements the last rounds run on the host; the
// two-product sumcheck's tables reach it through the context's pinned tail area, stored by the
// launch that produces them and announced by the round's post (no copy command, no stream drain).
// Coefficient sums are exact field sums, so any reduction tree is bit-identical
// to the reference's sequential accumulation.
// ============================================================================================
static constexpr size_t SC_TAIL = 1024;      // table size at which the remaining rounds go to the host
static constexpr size_t SC_DOUBLE_MIN = 16 * SC_TAIL;      // tables at least this large take two rounds per round trip
static constexpr size_t SC_TAIL_AREA = hobbit_ctx::TAIL_ELEMS;      // elements per table of the context's tail area: the largest table handed to the host
static_assert(SC_TAIL_AREA == 2 * SC_TAIL, "the tail area holds the unfolded tables of the round that ends at SC_TAIL");

template <int NC>
__device__ __forceinline__ void block_reduce_store(F (&c)[NC], F *partials) {
    __shared__ F red[NC][16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int q = 0; q < NC; q++) { F s = wave_sum(c[q]); if (lane == 0) red[q][wv] = s; }
    __syncthreads();
    if (threadIdx.x < NC) {
        F s = red[threadIdx.x][0];
        for (int w = 1; w < nw; w++) s = fadd(s, red[threadIdx.x][w]);
        stF(partials + (size_t)blockIdx.x * NC + threadIdx.x, s);
    }
}
__device__ __forceinline__ void acc_quad(F (&c)[3], const F &x0, const F &x1, const F &y0, const F &y1) {
    // (dx t + x0)(dy t + y0): a = dx dy, b = dx y0 + x0 dy, c = x0 y0   (src/polynomial.cpp:133-135)
    F dx = fsub(x1, x0), dy = fsub(y1, y0);
    c[0] = fadd(c[0], fmul(dx, dy));
    c[1] = fadd(c[1], fadd(fmul(dx, y0), fmul(x0, dy)));
    c[2] = fadd(c[2], fmul(x0, y0));
}
// round 0 of the 2-product sumcheck: polynomial only (inputs are preserved)
__global__ void __launch_bounds__(256) k_sc2_poly(const F *__restrict__ v1, const F *__restrict__ v2, size_t L, F *__restrict__ partials) {
    F c[3] = {fmake(0), fmake(0), fmake(0)};
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x)
        acc_quad(c, ldF(v1 + 2 * j), ldF(v1 + 2 * j + 1), ldF(v2 + 2 * j), ldF(v2 + 2 * j + 1));
    block_reduce_store<3>(c, partials);
}
// rounds >= 1: fold the previous tables with the challenge just derived (4 -> 2 elements per
// thread and table) and accumulate this round's polynomial from the folded pair in registers.
__global__ void __launch_bounds__(256) k_sc2_fold_poly(const F *__restrict__ s1, const F *__restrict__ s2, F *__restrict__ d1, F *__restrict__ d2,
                                                       size_t L, F r, F *__restrict__ partials, F *__restrict__ tail) {
    F c[3] = {fmake(0), fmake(0), fmake(0)};
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x) {
        F a0 = ldF(s1 + 4 * j), a1 = ldF(s1 + 4 * j + 1), a2 = ldF(s1 + 4 * j + 2), a3 = ldF(s1 + 4 * j + 3);
        F b0 = ldF(s2 + 4 * j), b1 = ldF(s2 + 4 * j + 1), b2 = ldF(s2 + 4 * j + 2), b3 = ldF(s2 + 4 * j + 3);
        F x0 = fadd(a0, fmul(r, fsub(a1, a0))), x1 = fadd(a2, fmul(r, fsub(a3, a2)));
        F y0 = fadd(b0, fmul(r, fsub(b1, b0))), y1 = fadd(b2, fmul(r, fsub(b3, b2)));
        stF(d1 + 2 * j, x0); stF(d1 + 2 * j + 1, x1); stF(d2 + 2 * j, y0); stF(d2 + 2 * j + 1, y1);
        if (tail) {           // the launch whose output the host continues from (2 L <= SC_TAIL_AREA): the same elements into the context's tail area
            stF(tail + 2 * j, x0); stF(tail + 2 * j + 1, x1); stF(tail + SC_TAIL_AREA + 2 * j, y0); stF(tail + SC_TAIL_AREA + 2 * j + 1, y1);
        }
        acc_quad(c, x0, x1, y0, y1);
    }
    block_reduce_store<3>(c, partials);
}
// The paths that reach the host tail without a fold launch: both tables (len <= SC_TAIL_AREA elements each) into the tail area as they are
__global__ void __launch_bounds__(256) k_sc2_tail_copy(const F *__restrict__ s1, const F *__restrict__ s2, size_t len, F *__restrict__ tail) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < len; j += (size_t)gridDim.x * blockDim.x) {
        stF(tail + j, ldF(s1 + j)); stF(tail + SC_TAIL_AREA + j, ldF(s2 + j));
    }
}
// n <= SC_TAIL, where no round runs on the device and no reduction follows: ONE workgroup copies both tables and posts itself.  Every
// thread makes its stores visible at system scope before the barrier; thread 0 posts behind the barrier.
__global__ void __launch_bounds__(256) k_sc2_tail_copy_post(const F *__restrict__ s1, const F *__restrict__ s2, uint32_t len, F *__restrict__ tail, Mailbox *mb, uint32_t seq) {
    for (uint32_t j = threadIdx.x; j < len; j += blockDim.x) { stF(tail + j, ldF(s1 + j)); stF(tail + SC_TAIL_AREA + j, ldF(s2 + j)); }
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(&mb->flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Two rounds per transcript round trip.  For a quad (a0..a3) of the round-i tables, X(r, t) = x0(r) + t (x1(r) - x0(r)) with
// x0 = a0 + r (a1 - a0), x1 = a2 + r (a3 - a2) is bilinear in (r, t); G(r, t) = sum over quads of X(r, t) Y(r, t) is biquadratic and
// therefore fixed by its nine values on {0, 1, inf}^2 ("inf" = leading coefficient; leading coefficients multiply):
//   X(0,0) = a0, X(1,0) = a1, X(inf,0) = a1 - a0 | X(0,1) = a2, X(1,1) = a3, X(inf,1) = a3 - a2 | X(0,inf) = a2 - a0, X(1,inf) = a3 - a1,
//   X(inf,inf) = (a3 - a2) - (a1 - a0).
// Round i's polynomial is G(r, 0) + G(r, 1); after r = r_i the host has G(r_i, t) at t = 0, 1, inf: round i + 1's polynomial.  Nine
// products per quad instead of 2 x 4 + 4 over the two rounds, one round trip instead of two, and the tables are read once per two
// rounds: with FOLD the kernel first folds sixteen elements of the tables two levels up with (r0, r1) into the quad and stores it.
// Exact field sums: the coefficients are bit-identical to the reference's round-by-round ones (src/sumcheck.cpp:2391-2460).
// One thread per element of the round-i tables: with FOLD it folds the four elements 4g..4g+3 of the tables two levels up (64
// contiguous bytes per lane and table, the access pattern of k_sc2_fold_poly) into element g and stores it; the quad is the four
// adjacent lanes, which exchange values by DPP quad permutes.  Lane q of a quad owns X(q&1, q>>1) = a_q; lanes 1 and 3 also form the
// r = inf points, lanes 2 and 3 the t = inf points, lane 3 the (inf, inf) point.
template <int CTRL> __device__ __forceinline__ F quad_perm(const F &v) {
    F o; uint32_t w[4] = {(uint32_t)v.re, (uint32_t)(v.re >> 32), (uint32_t)v.im, (uint32_t)(v.im >> 32)};
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)w[k], CTRL, 0xF, 0xF, false);
    o.re = (uint64_t)w[0] | ((uint64_t)w[1] << 32); o.im = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
    return o;
}
template <bool FOLD>
__global__ void __launch_bounds__(256) k_sc2_double(const F *__restrict__ s1, const F *__restrict__ s2, F *__restrict__ d1, F *__restrict__ d2, size_t Q, F r0,
                                                    F r1, F *__restrict__ partials) {
    F acc0 = fmake(0), acc1 = fmake(0), acc2 = fmake(0), acc3 = fmake(0);
    const int q = threadIdx.x & 3;
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < 4 * Q; g += (size_t)gridDim.x * blockDim.x) {
        F a, b;
        if (FOLD) {
            const F *e = s1 + 4 * g, *h = s2 + 4 * g;
            F e0 = ldF(e), e1 = ldF(e + 1), e2 = ldF(e + 2), e3 = ldF(e + 3);
            F f0 = fadd(e0, fmul(r0, fsub(e1, e0))), f1 = fadd(e2, fmul(r0, fsub(e3, e2)));
            a = fadd(f0, fmul(r1, fsub(f1, f0)));
            F h0 = ldF(h), h1 = ldF(h + 1), h2 = ldF(h + 2), h3 = ldF(h + 3);
            F k0 = fadd(h0, fmul(r0, fsub(h1, h0))), k1 = fadd(h2, fmul(r0, fsub(h3, h2)));
            b = fadd(k0, fmul(r1, fsub(k1, k0)));
            stF(d1 + g, a); stF(d2 + g, b);
        } else { a = ldF(s1 + g); b = ldF(s2 + g); }
        acc0 = fadd(acc0, fmul(a, b));                                                   // (0,0) (1,0) (0,1) (1,1) on lanes 0..3
        const F an = quad_perm<0xA0>(a), bn = quad_perm<0xA0>(b);                        // lanes 1, 3 <- lanes 0, 2
        const F da = fsub(a, an), db = fsub(b, bn);                                      // lanes 1, 3: a1 - a0, a3 - a2
        acc1 = fadd(acc1, fmul(da, db));                                                 // (inf,0) on lane 1, (inf,1) on lane 3
        const F a2 = quad_perm<0x44>(a), b2 = quad_perm<0x44>(b);                        // lanes 2, 3 <- lanes 0, 1
        acc2 = fadd(acc2, fmul(fsub(a, a2), fsub(b, b2)));                               // (0,inf) on lane 2, (1,inf) on lane 3
        const F da2 = quad_perm<0x44>(da), db2 = quad_perm<0x44>(db);                    // lane 3 <- lane 1's differences
        acc3 = fadd(acc3, fmul(fsub(da, da2), fsub(db, db2)));                           // (inf,inf) on lane 3
    }
    const F z = fmake(0);
    F c[9] = {q == 0 ? acc0 : z, q == 1 ? acc0 : z, q == 1 ? acc1 : z, q == 2 ? acc0 : z, q == 3 ? acc0 : z, q == 3 ? acc1 : z,
              q == 2 ? acc2 : z, q == 3 ? acc2 : z, q == 3 ? acc3 : z};
    block_reduce_store<9>(c, partials);
}
// reduce the per-workgroup partials to NC coefficients
template <int NC>
__global__ void __launch_bounds__(256) k_sc_reduce(const F *__restrict__ partials, int nblocks, F *__restrict__ out) {
    F c[NC];
#pragma unroll
    for (int q = 0; q < NC; q++) c[q] = fmake(0);
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
        for (int q = 0; q < NC; q++) c[q] = fadd(c[q], ldF(partials + (size_t)b * NC + q));
    block_reduce_store<NC>(c, out);
}

// The same reduction, posting to the host mailbox: the NC coefficients go straight into coherent pinned host memory, then the
// launch's sequence number (system-scope release); the host spins on that word instead of queueing a 48-byte copy and sleeping
// in hipStreamSynchronize.  (Folding this into the round kernel itself -- last workgroup to arrive reduces -- needs an agent-scope
// release per workgroup, which on this 8-XCD part writes back each XCD's L2: measured 0.16 ms per launch, so it stays a kernel.)
template <int NC>
__global__ void __launch_bounds__(256) k_sc_reduce_post(const F *__restrict__ partials, int nblocks, Mailbox *mb, uint32_t seq) {
    F c[NC];
#pragma unroll
    for (int q = 0; q < NC; q++) c[q] = fmake(0);
    for (int b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
        for (int q = 0; q < NC; q++) c[q] = fadd(c[q], ldF(partials + (size_t)b * NC + q));
    __shared__ F red2[NC][16];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int q = 0; q < NC; q++) { F sm = wave_sum(c[q]); if (lane == 0) red2[q][wv] = sm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int q = 0; q < NC; q++) {
            F sm = red2[q][0];
            for (int w = 1; w < nw; w++) sm = fadd(sm, red2[q][w]);
            uint64_t *o = reinterpret_cast<uint64_t *>(&mb->vals[q]);
            __hip_atomic_store(o, sm.re, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); __hip_atomic_store(o + 1, sm.im, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __hip_atomic_store(&mb->flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// host tail of the 2-product sumcheck: tables a,b of size sz (not yet folded with `rnd` when
// pending_fold), continuing at round `round` exactly as src/sumcheck.cpp:2401-2452.  Folds in
// place: the caller hands it the context's tail area, where the device left the tables.
static void sc2_host_tail(F *a, F *b, size_t sz, F &rnd, bool pending_fold, int round, int rounds, MHP h_qpoly, MHP h_r) {
    auto fold = [&](F *v) { for (size_t j = 0; j < sz / 2; j++) v[j] = fadd(v[2 * j], fmul(rnd, fsub(v[2 * j + 1], v[2 * j]))); };
    if (pending_fold) { fold(a); fold(b); sz /= 2; }
    for (int i = round; i < rounds; i++) {
        F pa = fmake(0), pb = fmake(0), pc = fmake(0);
        for (size_t j = 0; j < sz / 2; j++) {
            F dx = fsub(a[2 * j + 1], a[2 * j]), dy = fsub(b[2 * j + 1], b[2 * j]);
            pa = fadd(pa, fmul(dx, dy)); pb = fadd(pb, fadd(fmul(dx, b[2 * j]), fmul(a[2 * j], dy))); pc = fadd(pc, fmul(a[2 * j], b[2 * j]));
        }
        rnd = mimc_hash(rnd, pa); rnd = mimc_hash(rnd, pb); rnd = mimc_hash(rnd, pc);
        h_r[i] = rnd; h_qpoly[3 * i] = pa; h_qpoly[3 * i + 1] = pb; h_qpoly[3 * i + 2] = pc;
        fold(a); fold(b); sz /= 2;
    }
}

// ---- streaming-sumcheck error terms (src/sumcheck.cpp:374-432, 1093-1136): fused multi-output dot products --
// KIND 2: compute2p (b1,b2,f1,f2) -> K1,K2;  KIND 3: compute3p (b1,gate,f1,f2,f3,beta) -> K1..K3;
// KIND 4: compute4p (b1,b2,b3,gate,f1..f4) -> K1..K4;  KIND 13: one batch of batch_prod (b1,b2,b3,f1,f2,f3) -> K1,K2,K3
struct ErrArgs { const F *t[8]; const int32_t *gate; int lk; F lr0, lr1; };
// compute3p_error_terms' selector -> gate map when has_lookups is set (src/sumcheck.cpp:413-427): 0 and 4 -> 1, 2 -> lookup_rand[0], 3 -> lookup_rand[1],
// everything else (1, and the -1 the caller parks addition gates at) -> 0
__device__ __forceinline__ F lk_gate3(int s, const F &lr0, const F &lr1) { return (s == 0 || s == 4) ? fmake(1) : s == 2 ? lr0 : s == 3 ? lr1 : fmake(0); }
template <int KIND, int NC>
__global__ void __launch_bounds__(256) k_err_terms(ErrArgs a, size_t n, F *__restrict__ partials) {
    F K[NC];
#pragma unroll
    for (int q = 0; q < NC; q++) K[q] = fmake(0);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        if (KIND == 2) {
            const F b1 = ldF(a.t[0] + i), b2 = ldF(a.t[1] + i), f1 = ldF(a.t[2] + i), f2 = ldF(a.t[3] + i);
            K[0] = fadd(K[0], fadd(fmul(b1, f2), fmul(b2, f1)));
            K[1] = fadd(K[1], fmul(b1, b2));
        } else if (KIND == 3) {
            const F b1 = ldF(a.t[0] + i), f1 = ldF(a.t[1] + i), f2 = ldF(a.t[2] + i), f3 = ldF(a.t[3] + i), be = ldF(a.t[4] + i);
            const F gate = a.lk ? lk_gate3(a.gate[i], a.lr0, a.lr1) : fmake((uint64_t)(int64_t)a.gate[i]);
            const F t1 = fadd(fmul(b1, f2), fmul(gate, f1)), t2 = fmul(b1, gate);
            K[0] = fadd(K[0], fadd(fmul(f3, t1), fmul(fmul(be, f1), f2)));
            K[1] = fadd(K[1], fadd(fmul(be, t1), fmul(f3, t2)));
            K[2] = fadd(K[2], fmul(t2, be));
        } else if (KIND == 4) {
            const F b1 = ldF(a.t[0] + i), b2 = ldF(a.t[1] + i), b3 = ldF(a.t[2] + i), f1 = ldF(a.t[3] + i), f2 = ldF(a.t[4] + i), f3 = ldF(a.t[5] + i),
                    f4 = ldF(a.t[6] + i);
            const F gate = a.lk ? fmake(a.gate[i] == 1 ? 1 : 0) : fsub(fmake(1), fmake((uint64_t)(int64_t)a.gate[i]));      // (:388-394)
            const F t1 = fadd(fmul(f1, b2), fmul(f2, b1)), t2 = fadd(fmul(f3, gate), fmul(f4, b3));
            const F t3 = fmul(b1, b2), t4 = fmul(gate, b3), t5 = fmul(f1, f2), t6 = fmul(f3, f4);
            K[0] = fadd(K[0], fadd(fmul(t1, t6), fmul(t2, t5)));
            K[1] = fadd(K[1], fadd(fadd(fmul(t1, t2), fmul(t3, t6)), fmul(t4, t5)));
            K[2] = fadd(K[2], fadd(fmul(t1, t4), fmul(t2, t3)));
            K[3] = fadd(K[3], fmul(t3, t4));
        } else {
            const F b1 = ldF(a.t[0] + i), b2 = ldF(a.t[1] + i), b3 = ldF(a.t[2] + i), f1 = ldF(a.t[3] + i), f2 = ldF(a.t[4] + i), f3 = ldF(a.t[5] + i);
            const F t1 = fadd(fmul(b1, f2), fmul(b2, f1)), t2 = fmul(b1, b2);
            K[0] = fadd(K[0], fadd(fmul(f3, t1), fmul(fmul(b3, f1), f2)));
            K[1] = fadd(K[1], fadd(fmul(b3, t1), fmul(f3, t2)));
            K[2] = fadd(K[2], fmul(t2, b3));
        }
    }
    block_reduce_store<NC>(K, partials);
}
// runs one error-term reduction; h_K receives the NC sums (not accumulated)
template <int KIND, int NC>
static int run_err(hobbit_ctx *ctx, const char *name, const ErrArgs &a, size_t n, MHP h_K) {
    const int MAXB = 1024;
    F *ws; HB_TRY(ctx->workspace(((size_t)MAXB * NC + NC + 4) * sizeof(F), (void **)&ws));
    F *part = ws, *coef = ws + (size_t)MAXB * NC;
    F *pin; HB_TRY(ctx->pinned(NC * sizeof(F), (void **)&pin));
    int nb = grid_for(n, 256, MAXB);
    HB_LAUNCH(ctx, name, (k_err_terms<KIND, NC>), dim3(nb), dim3(256), 0, a, n, part);
    HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce<NC>, dim3(1), dim3(256), 0, part, nb, coef);
    HB_CHECK(ctx, hipMemcpyAsync(pin, coef, NC * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    HB_TRY(ctx->sync());
    for (int q = 0; q < NC; q++) h_K[q] = pin[q];
    return 0;
}
int launch_err_terms(hobbit_ctx *ctx, int kind, const F *const *tables, const int32_t *gate, size_t n, MHP h_K) {
    ErrArgs a; for (int i = 0; i < 8; i++) a.t[i] = tables[i]; a.gate = gate; a.lk = ctx->has_lookups ? 1 : 0; a.lr0 = ctx->lookup_rand[0]; a.lr1 = ctx->lookup_rand[1];
    if (!n) { int nc = kind == 2 ? 2 : kind == 4 ? 4 : 3; for (int q = 0; q < nc; q++) h_K[q] = fmake(0); return 0; }
    switch (kind) {
        case 2: return run_err<2, 2>(ctx, "k_err2p", a, n, h_K);
        case 3: return run_err<3, 3>(ctx, "k_err3p", a, n, h_K);
        case 4: return run_err<4, 4>(ctx, "k_err4p", a, n, h_K);
        case 13: return run_err<13, 3>(ctx, "k_batch_prod_terms", a, n, h_K);
    }
    return ctx->fail(HOBBIT_EINVAL, "err_terms: unknown kind");
}
// fold[j] += rand * (F)sel[j]  or  rand * (1 - sel[j])   (src/sumcheck.cpp:863,867: gate selector folds)
__global__ void k_axpy_i32(F *__restrict__ y, const int32_t *__restrict__ sel, F a, int one_minus, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        F v = fmake((uint64_t)(int64_t)sel[i]);
        if (one_minus) v = fsub(fmake(1), v);
        stF(y + i, fadd(ldF(y + i), fmul(a, v)));
    }
}
int launch_axpy_i32(hobbit_ctx *ctx, F *y, const int32_t *sel, F a, int one_minus, size_t n) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_axpy_i32", k_axpy_i32, dim3(grid_for(n, 256)), dim3(256), 0, y, sel, a, one_minus, n);
    return 0;
}

// memory / lookup fingerprints of the wiring-consistency streams (src/witness_stream.cpp:2196, 2290-2305; src/main.cpp:1039-1044):
// out[i] = addr[i] + 1 + a * value[i] (+ b * freq[i])
__global__ void k_fingerprint(const F *__restrict__ addr, const F *__restrict__ value, const F *__restrict__ freq, F a, F b, F *__restrict__ out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        F v = fadd(fadd(ldF(addr + i), fmake(1)), fmul(a, ldF(value + i)));
        if (freq) v = fadd(v, fmul(b, ldF(freq + i)));
        stF(out + i, v);
    }
}
int launch_fingerprint(hobbit_ctx *ctx, const F *addr, const F *value, const F *freq, F a, F b, F *out, size_t n) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_fingerprint", k_fingerprint, dim3(grid_for(n, 256)), dim3(256), 0, addr, value, freq, a, b, out, n);
    return 0;
}

// ---- prove_gate_consistency_lookups (src/sumcheck.cpp:503-795) device pieces ---------------------------------------
// One chunk's selector rewrites (:568-585) and lookup output column: s2 = selectors for the R call (2 -> 3), s3 = for the lookup call
// (0 -> -1, 2 -> 4), blo = lookup_rand[0] L + lookup_rand[1] R - O on lookup rows, 0 elsewhere.
__global__ void k_lkp_prepare(const int32_t *__restrict__ S, const F *__restrict__ L, const F *__restrict__ R, const F *__restrict__ O, F lr0, F lr1,
                              int32_t *__restrict__ s2, int32_t *__restrict__ s3, F *__restrict__ blo, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int s = S[i];
        const bool lk = s != 0 && s != 1;
        if (s2) s2[i] = s == 2 ? 3 : s;
        if (s3) s3[i] = s == 0 ? -1 : s == 2 ? 4 : s;
        stF(blo + i, lk ? fsub(fadd(fmul(lr0, ldF(L + i)), fmul(lr1, ldF(R + i))), ldF(O + i)) : fmake(0));
    }
}
// the four selector-derived folds (:510-536 with rnd = 1 on zeroed tables, :614-625): add_L += rnd {1, 0, lr0}[s], add_R += rnd {1, 0, lr1}[s],
// lkp += rnd [s is a lookup], mul += rnd [s == 1]
__global__ void k_lkp_sel_fold(const int32_t *__restrict__ S, F rnd, F lr0, F lr1, F *__restrict__ aL, F *__restrict__ aR, F *__restrict__ lkp, F *__restrict__ mul, size_t n) {
    const F rl0 = fmul(rnd, lr0), rl1 = fmul(rnd, lr1);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int s = S[i];
        if (s == 1) stF(mul + i, fadd(ldF(mul + i), rnd));
        else if (s == 0) { stF(aL + i, fadd(ldF(aL + i), rnd)); stF(aR + i, fadd(ldF(aR + i), rnd)); }
        else { stF(lkp + i, fadd(ldF(lkp + i), rnd)); stF(aL + i, fadd(ldF(aL + i), rl0)); stF(aR + i, fadd(ldF(aR + i), rl1)); }
    }
}
int launch_lkp_prepare(hobbit_ctx *ctx, const int32_t *S, const F *L, const F *R, const F *O, int32_t *s2, int32_t *s3, F *blo, size_t n) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_lkp_prepare", k_lkp_prepare, dim3(grid_for(n, 256)), dim3(256), 0, S, L, R, O, ctx->lookup_rand[0], ctx->lookup_rand[1], s2, s3, blo, n);
    return 0;
}
int launch_lkp_sel_fold(hobbit_ctx *ctx, const int32_t *S, F rnd, F *aL, F *aR, F *lkp, F *mul, size_t n) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_lkp_sel_fold", k_lkp_sel_fold, dim3(grid_for(n, 256)), dim3(256), 0, S, rnd, ctx->lookup_rand[0], ctx->lookup_rand[1], aL, aR, lkp, mul, n);
    return 0;
}

// ---- _whir_prove (src/Virgo.cpp:519-686) device pieces -----------------------------------------------
// one fold round over the half split (j, j+L): quadratic coefficients of sum (dp t + p)(db t + b) and, in the same pass,
// poly[j] += a (poly[j+L] - poly[j]), beta[j] += a (beta[j+L] - beta[j])  (the challenge a = random() does not depend on
// the polynomial, so it is drawn before the pass)
__global__ void __launch_bounds__(256) k_whir_round(F *__restrict__ poly, F *__restrict__ beta, size_t L, F a, F *__restrict__ partials) {
    F c[3] = {fmake(0), fmake(0), fmake(0)};
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x) {
        const F p0 = ldF(poly + j), p1 = ldF(poly + j + L), b0 = ldF(beta + j), b1 = ldF(beta + j + L);
        const F d1 = fsub(p1, p0), d2 = fsub(b1, b0);
        c[0] = fadd(c[0], fmul(d1, d2)); c[1] = fadd(c[1], fadd(fmul(d1, b0), fmul(p0, d2))); c[2] = fadd(c[2], fmul(p0, b0));
        stF(poly + j, fadd(p0, fmul(a, d1))); stF(beta + j, fadd(b0, fmul(a, d2)));
    }
    block_reduce_store<3>(c, partials);
}
// <a, b> over n elements: per-workgroup partials (part: >= 1024 F), then one workgroup
__global__ void __launch_bounds__(256) k_dot(const F *__restrict__ a, const F *__restrict__ b, size_t n, F *__restrict__ partials) {
    F c[1] = {fmake(0)};
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) c[0] = fadd(c[0], fmul(ldF(a + j), ldF(b + j)));
    block_reduce_store<1>(c, partials);
}
int launch_dot(hobbit_ctx *ctx, const F *a, const F *b, size_t n, F *part, F *out) {
    int nb = grid_for(n, 256, 1024);
    HB_LAUNCH(ctx, "k_dot", k_dot, dim3(nb), dim3(256), 0, a, b, n, part);
    HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce<1>, dim3(1), dim3(256), 0, part, nb, out);
    return 0;
}
int launch_whir_round(hobbit_ctx *ctx, F *poly, F *beta, size_t L, F a, F *part, F *coef) {   // coef: 3 F of this round (device)
    int nb = grid_for(L, 256, 1024);
    HB_LAUNCH(ctx, "k_whir_round", k_whir_round, dim3(nb), dim3(256), 0, poly, beta, L, a, part);
    HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce<3>, dim3(1), dim3(256), 0, part, nb, coef);
    return 0;
}
// batched precompute_beta: reps tables of 2^v entries side by side (row stride ld); one doubling level per launch;
// z[p*v + (v-1-level)] is the challenge of table p at this level
__global__ void k_eq_step_batched(const F *__restrict__ old, F *__restrict__ nw, size_t m, size_t ld, const F *__restrict__ z, int v, int level) {
    const F *o = old + (size_t)blockIdx.y * ld; F *n = nw + (size_t)blockIdx.y * ld;
    const F r = ldF(z + (size_t)blockIdx.y * v + (v - 1 - level));
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < m; j += (size_t)gridDim.x * blockDim.x) {
        const F x = ldF(o + j), t = fmul(r, x);
        stF(n + 2 * j, fsub(x, t)); stF(n + 2 * j + 1, t);
    }
}
// the first h <= 11 levels of every table in one launch (one workgroup per table, table in LDS): a level per launch is latency only up there
__global__ void __launch_bounds__(256) k_eq_head_batched(F *__restrict__ out, size_t ld, const F *__restrict__ z, int v, int h) {
    __shared__ F s[2048];
    const F *zz = z + (size_t)blockIdx.x * v;
    if (threadIdx.x == 0) s[0] = fmake(1);
    __syncthreads();
    for (int i = 0; i < h; i++) {
        const uint32_t m = 1u << i;
        const F r = ldF(zz + (v - 1 - i));
        F o[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { const uint32_t j = threadIdx.x + 256 * u; if (j < m) o[u] = ldF(&s[j]); }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t j = threadIdx.x + 256 * u;
            if (j < m) { const F t = fmul(r, o[u]); stF(&s[2 * j], fsub(o[u], t)); stF(&s[2 * j + 1], t); }
        }
        __syncthreads();
    }
    F *n = out + (size_t)blockIdx.x * ld;
    for (uint32_t j = threadIdx.x; j < (1u << h); j += 256) stF(n + j, ldF(&s[j]));
}
int launch_eq_head_batched(hobbit_ctx *ctx, F *out, size_t ld, const F *z, int v, int h, int reps) {
    if (h < 0 || h > 11 || h > v) return ctx->fail(HOBBIT_EINVAL, "eq_head_batched: 0 <= h <= min(v, 11)");
    HB_LAUNCH(ctx, "k_eq_step_batched", k_eq_head_batched, dim3(reps), dim3(256), 0, out, ld, z, v, h);
    return 0;
}
int launch_eq_step_batched(hobbit_ctx *ctx, const F *old, F *nw, size_t m, size_t ld, const F *z, int v, int level, int reps) {
    HB_LAUNCH(ctx, "k_eq_step_batched", k_eq_step_batched, dim3(grid_for(m, 256, 256), reps), dim3(256), 0, old, nw, m, ld, z, v, level);
    return 0;
}
__global__ void k_fill_F(F *__restrict__ p, size_t stride, size_t n, F v) {
    size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g < n) stF(p + g * stride, v);
}
int launch_fill_F(hobbit_ctx *ctx, F *p, size_t stride, size_t n, F v) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_fill_F", k_fill_F, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, p, stride, n, v);
    return 0;
}

// ---- 2-product sumcheck whose SECOND table is sparse (the open's P3: 5900 non-zeros of 2^25, src/PC_utils.cpp:331-339) -------------------
// The round polynomials only see the quads in which the sparse table is non-zero, so the large levels need no dense pass over it and no
// products over the dense table: per round trip one plain 4 -> 1 fold of the dense table (k_sc2_fold4) and one pass over the LIST
// (k_sc2_sparse_round).  Everything the sumcheck does with the sparse table is linear in it, so the list is never regrouped: entry e keeps
// the caller's index x_e for good and stands, at level i, for the value v_e prod_{b < i} (x_e bit b ? r_b : 1 - r_b) at index x_e >> i
// (entries that meet in one index simply add up).  One thread per entry, any number of workgroups: with FOLD it multiplies its value by the
// weight of the two index bits just folded and stores it, then it gathers the four elements of its quad of the dense table and adds its
// share of the nine values of G(r, t) -- for the element at position p of the quad, b_p = v and the other three are zero in the sums
// k_sc2_double forms.  k_sc_reduce_post adds the workgroups' partials and posts them.  Exact field sums: the transcript is bit-identical
// to the dense kernels'.  Below SC_DOUBLE_MIN the list is summed into a dense table (k_scatter_counted) and the dense path takes over.
__global__ void __launch_bounds__(256) k_sc2_fold4(const F *__restrict__ s, F *__restrict__ d, size_t nout, F r0, F r1) {
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < nout; g += (size_t)gridDim.x * blockDim.x) {
        const F *e = s + 4 * g;
        const F e0 = ldF(e), e1 = ldF(e + 1), e2 = ldF(e + 2), e3 = ldF(e + 3);
        const F f0 = fadd(e0, fmul(r0, fsub(e1, e0))), f1 = fadd(e2, fmul(r0, fsub(e3, e2)));
        stF(d + g, fadd(f0, fmul(r1, fsub(f1, f0))));
    }
}
__device__ __forceinline__ F fkeep(bool c, const F &t) { const uint64_t m = 0 - (uint64_t)c; return fmake(t.re & m, t.im & m); }      // c ? t : 0, no select
// lvl: the level of `dense` (index x >> lvl); with FOLD the values come in at level lvl - 2
template <bool FOLD>
__global__ void __launch_bounds__(256) k_sc2_sparse_round(const uint64_t *__restrict__ idx, const F *val_in, F *val_out, uint32_t m, int lvl,
                                                           const F *__restrict__ dense, F r0, F r1, F *__restrict__ partials) {
    F c[9];
#pragma unroll
    for (int q = 0; q < 9; q++) c[q] = fmake(0);
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < m; e += gridDim.x * blockDim.x) {
        const uint64_t x = idx[e];
        F v = ldF(val_in + e);
        const uint64_t y = x >> lvl;
        const F *ap = dense + 4 * (y >> 2);
        const F a0 = ldF(ap), a1 = ldF(ap + 1), a2 = ldF(ap + 2), a3 = ldF(ap + 3);
        if (FOLD) {
            const uint32_t pp = (uint32_t)(x >> (lvl - 2)) & 3;      // position b0 + 2 b1 in the folded quad: weight (b0 ? r0 : 1 - r0) (b1 ? r1 : 1 - r1)
            v = fmul(v, fmul((pp & 1) ? r0 : fsub(fmake(1), r0), (pp & 2) ? r1 : fsub(fmake(1), r1)));
            stF(val_out + e, v);
        }
        const uint32_t p = (uint32_t)y & 3;
        const bool odd = p & 1, up = p & 2;
        const F nv = fneg(v);
        const F t0 = fmul(ldF(ap + p), v);                                                    // a_p b_p: (0,0) (1,0) (0,1) (1,1)
        c[0] = fadd(c[0], fkeep(p == 0, t0)); c[1] = fadd(c[1], fkeep(p == 1, t0)); c[3] = fadd(c[3], fkeep(p == 2, t0)); c[4] = fadd(c[4], fkeep(p == 3, t0));
        const F da01 = fsub(a1, a0), da23 = fsub(a3, a2);
        const F t1 = fmul(up ? da23 : da01, odd ? v : nv);                                    // (a1 - a0)(b1 - b0) | (a3 - a2)(b3 - b2)
        c[2] = fadd(c[2], fkeep(!up, t1)); c[5] = fadd(c[5], fkeep(up, t1));
        const F t2 = fmul(odd ? fsub(a3, a1) : fsub(a2, a0), up ? v : nv);                    // (a2 - a0)(b2 - b0) | (a3 - a1)(b3 - b1)
        c[6] = fadd(c[6], fkeep(!odd, t2)); c[7] = fadd(c[7], fkeep(odd, t2));
        c[8] = fadd(c[8], fmul(fsub(da23, da01), (odd != up) ? nv : v));                      // ((a3 - a2) - (a1 - a0)) ((b3 - b2) - (b1 - b0))
    }
    block_reduce_store<9>(c, partials);
}
// out[x >> lvl] = the sum of the entries that meet there (out zeroed by the caller).  The list is sorted, so they are consecutive: the first
// of a run adds it up.  (A run is one entry long through the opening; 2^lvl at the most.)
__global__ void __launch_bounds__(256) k_scatter_counted(const uint64_t *__restrict__ idx, const F *__restrict__ val, uint32_t m, int lvl, F *__restrict__ out) {
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < m; e += gridDim.x * blockDim.x) {
        const uint64_t y = idx[e] >> lvl;
        if (e && (idx[e - 1] >> lvl) == y) continue;
        F sm = ldF(val + e);
        for (uint32_t f = e + 1; f < m && (idx[f] >> lvl) == y; f++) sm = fadd(sm, ldF(val + f));
        stF(out + y, sm);
    }
}

// ---- 2-product sumcheck whose FIRST table is a sum of eq tables (the open's P4: eq(P2.r | P1.r) + a eq(P3.r) against [M' | C]) -----------------
// eq(r)[x] = prod_b (x_b ? r[b] : 1 - r[b]) and the sumcheck folds bit 0 first, so after i challenges c_0 .. c_{i-1} the folded table is
//   T_i[y] = sigma_i prod_{b >= i} (y_{b-i} ? r[b] : 1 - r[b]),    sigma_0 = 1,  sigma_{i+1} = sigma_i ((1 - r[i]) + c_i (2 r[i] - 1)):
// a host scalar times a shorter eq table.  The table is therefore never in memory.  More than that: the quad m of T_i is
//   (a0, a1, a2, a3) = A[m] (e0 f0, e1 f0, e0 f1, e1 f1),   e = (1 - r[i], r[i]),  f = (1 - r[i+1], r[i+1]),  A = T_{i+2} / its two folds,
// so X(rho, tau) = A[m] E(rho) F(tau) with E, F host scalars, and every one of the nine values of G(rho, tau) = sum_m X Y (see k_sc2_double) is
// E(rho) F(tau) times a combination of only FOUR sums over the dense table's quads (b0 .. b3),  W_p = sum_m A[m] b_p[m]:  one product per
// element and point where k_sc2_double spends four (k_sc2_double is at the VALU-issue limit, not at the memory's: DESIGN.md section 4).
// A[m] = sigma Lo[m mod 2^sh] Hi[m >> sh] with Hi = eq(r[s .. k-1]) and Lo = eq(r[i+2 .. s-1]) for a fixed split bit s: both a few thousand
// entries (cache-resident), built by ONE launch for every level the double rounds visit (k_eq_factors: each entry is its own product, no
// doubling passes); sigma is applied on the host, Hi once per run of equal m >> sh.  Only the dense table is read, and with FOLD folded and
// stored.  Exact field arithmetic throughout: the transcript is bit-identical to launch_sumcheck2 on the materialised table.
struct EqPts { F r[2][40]; };          // the points, entry b = the challenge of index bit b
__device__ __forceinline__ F eq_prod(const EqPts &p, int j, int from, int cnt, size_t x) {
    F v = fmake(1);
    for (int b = 0; b < cnt; b++) { const F rb = p.r[j][from + b]; v = fmul(v, ((x >> b) & 1) ? rb : fsub(fmake(1), rb)); }
    return v;
}
// blockIdx.y = table: per point first Hi (bits s .. k-1), then Lo of levels 2, 4, .., 2 nlev (bits level .. s-1), packed in that order
__global__ void __launch_bounds__(256) k_eq_factors(EqPts p, int k, int s, int nlev, F *__restrict__ out) {
    const int per = nlev + 1, j = blockIdx.y / per, t = blockIdx.y % per;
    size_t per_pt = (size_t)1 << (k - s), off = 0;
    for (int l = 1; l <= nlev; l++) { if (l == t) off = per_pt; per_pt += (size_t)1 << (s - 2 * l); }
    const int from = t == 0 ? s : 2 * t, cnt = t == 0 ? k - s : s - from;
    F *o = out + (size_t)j * per_pt + off;
    for (size_t x = blockIdx.x * (size_t)blockDim.x + threadIdx.x; x < ((size_t)1 << cnt); x += (size_t)gridDim.x * blockDim.x) stF(o + x, eq_prod(p, j, from, cnt, x));
}
// out[y] = sum_j al_j prod_{b < cnt} (y_b ? r_j[from + b] : 1 - r_j[from + b]): the folded table itself, for the levels that take the dense path
template <int T>
__global__ void __launch_bounds__(256) k_eq_sum_table(EqPts p, int from, int cnt, F al0, F al1, F *__restrict__ out) {
    for (size_t y = blockIdx.x * (size_t)blockDim.x + threadIdx.x; y < ((size_t)1 << cnt); y += (size_t)gridDim.x * blockDim.x) {
        F v = fmul(al0, eq_prod(p, 0, from, cnt, y));
        if (T == 2) v = fadd(v, fmul(al1, eq_prod(p, 1, from, cnt, y)));
        stF(out + y, v);
    }
}
// One lane per element of the level-i dense table (n4 = 4Q of them), as k_sc2_double; lane q of a quad sums A_j[m] b_q into its own W_{j,q}
// (a lane's q never changes: every stride is a multiple of four), so no lane exchange.  sh = s - (i + 2).  A workgroup walks spans of 256 U
// consecutive elements (n4 is a power of two >= SC_DOUBLE_MIN: spans never straddle its end), all of a span's loads issued before the first
// is used.  Partials: 4 T per workgroup, W_{j,p} at [4 j + p].
struct EqSide { const F *lo0, *lo1, *hi0, *hi1; };
template <bool FOLD, int T>
__global__ void __launch_bounds__(256) k_sc2_eq_double(EqSide eq, int sh, const F *__restrict__ s2, F *__restrict__ d2, size_t n4, F r0, F r1, F *__restrict__ partials) {
    constexpr int U = FOLD ? 2 : 4;
    F W0 = fmake(0), W1 = fmake(0), in0 = fmake(0), in1 = fmake(0), hv0 = fmake(0), hv1 = fmake(0);      // W_j = sum over finished runs; in_j: the current run's sum of Lo b
    size_t hcur = ~(size_t)0;
    const size_t lmask = ((size_t)1 << sh) - 1;
    for (size_t g0 = blockIdx.x * (size_t)(256 * U) + threadIdx.x; g0 < n4; g0 += (size_t)gridDim.x * (256 * U)) {
        F bv[U];
        if (FOLD) {
            F e[U][4];
#pragma unroll
            for (int u = 0; u < U; u++) { const F *h = s2 + 4 * (g0 + 256 * u); e[u][0] = ldF(h); e[u][1] = ldF(h + 1); e[u][2] = ldF(h + 2); e[u][3] = ldF(h + 3); }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const F k0 = fadd(e[u][0], fmul(r0, fsub(e[u][1], e[u][0]))), k1 = fadd(e[u][2], fmul(r0, fsub(e[u][3], e[u][2])));
                bv[u] = fadd(k0, fmul(r1, fsub(k1, k0)));
                stF(d2 + g0 + 256 * u, bv[u]);
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) bv[u] = ldF(s2 + g0 + 256 * u);
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const size_t m = (g0 + 256 * u) >> 2, h = m >> sh, l = m & lmask;
            if (h != hcur) {                                  // a new run: close the last one with its Hi (the first time with zeros)
                W0 = fadd(W0, fmul(hv0, in0)); in0 = fmake(0); hv0 = ldF(eq.hi0 + h);
                if (T == 2) { W1 = fadd(W1, fmul(hv1, in1)); in1 = fmake(0); hv1 = ldF(eq.hi1 + h); }
                hcur = h;
            }
            in0 = fadd(in0, fmul(ldF(eq.lo0 + l), bv[u]));
            if (T == 2) in1 = fadd(in1, fmul(ldF(eq.lo1 + l), bv[u]));
        }
    }
    W0 = fadd(W0, fmul(hv0, in0));
    if (T == 2) W1 = fadd(W1, fmul(hv1, in1));
    const int q = threadIdx.x & 3;
    const F z = fmake(0);
    F c[4 * T];
#pragma unroll
    for (int p = 0; p < 4; p++) { c[p] = q == p ? W0 : z; if (T == 2) c[4 + p] = q == p ? W1 : z; }
    block_reduce_store<4 * T>(c, partials);
}
struct EqSum { int T; CHP r[2]; F a[2]; };

static int sumcheck2_impl(hobbit_ctx *ctx, const F *v1, const F *v2, const uint64_t *sp_idx, const F *sp_val, size_t sp_m, const EqSum *eq, size_t n, F prev_r, MHP h_qpoly,
                          MHP h_r, MHP h_vr, MHP h_final);
int launch_sumcheck2(hobbit_ctx *ctx, const F *v1, const F *v2, size_t n, F prev_r, MHP h_qpoly, MHP h_r, MHP h_vr, MHP h_final) {
    return sumcheck2_impl(ctx, v1, v2, nullptr, nullptr, 0, nullptr, n, prev_r, h_qpoly, h_r, h_vr, h_final);
}
// v1 = sum_{j < T} a_j eq(r_j) given by its T <= 2 points (k = log2 n host entries each) and scalars; v2 dense on the device
int launch_sumcheck2_eq(hobbit_ctx *ctx, int T, CHP h_r1, CHP h_r2, CHP h_a, const F *v2, size_t n, F prev_r, MHP h_qpoly, MHP h_r, MHP h_vr, MHP h_final) {
    if (T < 1 || T > 2) return ctx->fail(HOBBIT_EINVAL, "sumcheck2_eq: one or two eq tables");
    if (!h_r1 || (T == 2 && !h_r2) || !h_a || !v2) return ctx->fail(HOBBIT_EINVAL, "sumcheck2_eq: null points, scalars or table");
    if (n > ((size_t)1 << 40)) return ctx->fail(HOBBIT_EINVAL, "sumcheck2_eq: n must be a power of two >= 2, at most 2^40");
    EqSum e; e.T = T; e.r[0] = h_r1; e.r[1] = T == 2 ? h_r2 : h_r1; e.a[0] = h_a[0]; e.a[1] = T == 2 ? (F)h_a[1] : fmake(0);
    return sumcheck2_impl(ctx, nullptr, v2, nullptr, nullptr, 0, &e, n, prev_r, h_qpoly, h_r, h_vr, h_final);
}
// v2 given as sp_m sorted, distinct (index, value) pairs on the device (every other entry zero)
int launch_sumcheck2_sparse(hobbit_ctx *ctx, const F *v1, const uint64_t *d_idx, const F *d_val, size_t m, size_t n, F prev_r, MHP h_qpoly, MHP h_r, MHP h_vr, MHP h_final) {
    if (!m || m > ((size_t)1 << 20)) return ctx->fail(HOBBIT_EINVAL, "sumcheck2_sparse: between 1 and 2^20 non-zeros");
    return sumcheck2_impl(ctx, v1, nullptr, d_idx, d_val, m, nullptr, n, prev_r, h_qpoly, h_r, h_vr, h_final);
}
static int sumcheck2_impl(hobbit_ctx *ctx, const F *v1, const F *v2, const uint64_t *sp_idx, const F *sp_val, size_t sp_m, const EqSum *eq, size_t n, F prev_r, MHP h_qpoly,
                          MHP h_r, MHP h_vr, MHP h_final) {
    int rounds = 0; while (((size_t)1 << rounds) < n) rounds++;
    if (((size_t)1 << rounds) != n || n < 2) return ctx->fail(HOBBIT_EINVAL, "sumcheck2: n must be a power of two >= 2");
    const int MAXB = 1024, EQ_MAXB = 2048;
    F rnd = prev_r;
    // the host's last rounds run in place in the context's tail area, where the device leaves their tables (hobbit_ctx.hpp)
    Mailbox *mb; unsigned *ticket; HB_TRY(ctx->mailbox(&mb, &ticket));
    F *const ta = ctx->tail, *const tb = ctx->tail + SC_TAIL_AREA;
    EqPts pts;
    if (eq) for (int j = 0; j < 2; j++) for (int b = 0; b < 40; b++) pts.r[j][b] = (j < eq->T && b < rounds) ? (F)eq->r[j][b] : fmake(0);
    // the eq-sum table itself, level `from` with scalars al: what the dense path reads where the table is short
    auto eq_table = [&](int from, const F *al, F *out) -> int {
        const size_t len = (size_t)1 << (rounds - from);
        if (eq->T == 2) HB_LAUNCH(ctx, "k_eq_sum_table", k_eq_sum_table<2>, dim3(grid_for(len, 256)), dim3(256), 0, pts, from, rounds - from, al[0], al[1], out);
        else HB_LAUNCH(ctx, "k_eq_sum_table", k_eq_sum_table<1>, dim3(grid_for(len, 256)), dim3(256), 0, pts, from, rounds - from, al[0], al[1], out);
        return 0;
    };
    if (n <= SC_TAIL) {                       // small instance: all rounds on the host
        if (eq) {
            F *dv1; HB_TRY(ctx->workspace(n * sizeof(F), (void **)&dv1));
            HB_TRY(eq_table(0, eq->a, dv1));
            v1 = dv1;
        }
        if (sp_idx) {
            F *dv2; HB_TRY(ctx->workspace(n * sizeof(F), (void **)&dv2));
            HB_TRY(launch_zero(ctx, dv2, n * sizeof(F)));
            HB_TRY(launch_scatter(ctx, sp_idx, sp_val, sp_m, dv2));
            v2 = dv2;
        }
        // no round runs on the device: one launch copies the tables into the tail area and posts, no copy command and no stream drain
        const uint32_t seq = ++ctx->mbox_seq;
        HB_LAUNCH(ctx, "k_sc2_tail_copy_post", k_sc2_tail_copy_post, dim3(1), dim3(256), 0, v1, v2, (uint32_t)n, ctx->tail, mb, seq);
        HB_TRY(ctx->mbox_wait(seq));
        sc2_host_tail(ta, tb, n, rnd, false, 0, rounds, h_qpoly, h_r);
    } else {
        size_t szA = n / 2, szB = n / 4;
        const bool sparse = sp_idx && n >= 16 * SC_DOUBLE_MIN;            // (shorter tables: scatter at once, dense path)
        const size_t sp_elems = sp_idx ? sp_m + (sparse ? 0 : n) : 0;      // the list's values at the current level (or a dense copy)
        // eq form: its own partials, the table where the dense path takes over (at most 4 SC_DOUBLE_MIN entries) and the factor tables
        const bool eq_double = eq && n >= SC_DOUBLE_MIN;
        const int eq_s = std::max(rounds - 12, (rounds + 1) / 2);               // split bit: Hi <= 4096 entries or both halves of k; every double level has i + 2 <= k - 12 <= s
        int eq_nlev = 0; while (eq_double && (n >> (2 * eq_nlev)) >= SC_DOUBLE_MIN) eq_nlev++;
        size_t eq_per_pt = (size_t)1 << (rounds - eq_s); for (int l = 1; l <= eq_nlev; l++) eq_per_pt += (size_t)1 << (eq_s - 2 * l);
        const size_t eq_elems = eq ? (size_t)EQ_MAXB * 8 + 4 + 4 * SC_DOUBLE_MIN + (eq_double ? 2 * eq_per_pt : 0) : 0;
        F *ws; HB_TRY(ctx->workspace((2 * szA + 2 * szB + (size_t)MAXB * 9 + 4 + sp_elems + eq_elems) * sizeof(F), (void **)&ws));
        F *A1 = ws, *A2 = A1 + szA, *B1 = A2 + szA, *B2 = B1 + szB, *part = B2 + szB;
        F *spw = part + (size_t)MAXB * 9 + 4;
        if (sp_idx && !sparse) {
            F *dv2 = spw + sp_m;
            HB_TRY(launch_zero(ctx, dv2, n * sizeof(F)));
            HB_TRY(launch_scatter(ctx, sp_idx, sp_val, sp_m, dv2));
            v2 = dv2;
        }
        F *eq_part = spw + sp_elems, *eq_tab = eq_part + (size_t)EQ_MAXB * 8 + 4, *eq_fac = eq_tab + 4 * SC_DOUBLE_MIN;
        F sig[2] = {fmake(1), fmake(1)}, eq_al[2] = {fmake(0), fmake(0)};        // sigma_{j,i}; a_j sigma_{j,i} of the last launch
        if (eq && !eq_double) { HB_TRY(eq_table(0, eq->a, eq_tab)); v1 = eq_tab; }      // round by round from the start: n < SC_DOUBLE_MIN entries
        if (eq_double)
            HB_LAUNCH(ctx, "k_eq_factors", k_eq_factors, dim3(grid_for((size_t)1 << std::max(eq_s, rounds - eq_s), 256, 64), eq->T * (eq_nlev + 1)), dim3(256), 0, pts, rounds,
                      eq_s, eq_nlev, eq_fac);
        const F *s1 = v1, *s2 = v2;
        F *d1 = A1, *d2 = A2;
        int i = 0;
        size_t cur = n;                       // size of the tables s1/s2 point at
        // ---- large tables: two rounds per round trip (k_sc2_double) ----
        if (n >= SC_DOUBLE_MIN) {
            const F *S1 = v1, *S2 = v2; size_t S_size = n;            // the materialised tables: level i - 2 (or the inputs)
            F *D1 = B1, *D2 = B2;                                     // T_2 has n/4 elements: fits B; later levels fit either
            bool pend = false; F pr0 = fmake(0), pr1 = fmake(0);      // (r_{i-2}, r_{i-1}): still to be applied to S
            const F *cval = sp_val;                                   // the sparse list's values at the level S1 is at
            while ((n >> i) >= SC_DOUBLE_MIN) {
                const size_t Q = (n >> i) / 4;
                const int nb = grid_for(4 * Q, 256, MAXB);
                const uint32_t seq = ++ctx->mbox_seq;
                if (sparse) {
                    const int nbs = grid_for(sp_m, 256, MAXB);
                    if (!pend) HB_LAUNCH(ctx, "k_sc2_sparse_round", k_sc2_sparse_round<false>, dim3(nbs), dim3(256), 0, sp_idx, cval, (F *)nullptr, (uint32_t)sp_m, i, S1, pr0, pr1, part);
                    else {
                        HB_LAUNCH(ctx, "k_sc2_fold4", k_sc2_fold4, dim3(grid_for(4 * Q, 256, 4096)), dim3(256), 0, S1, D1, 4 * Q, pr0, pr1);      // the dense table: level i - 2 -> level i
                        HB_LAUNCH(ctx, "k_sc2_sparse_round", k_sc2_sparse_round<true>, dim3(nbs), dim3(256), 0, sp_idx, cval, spw, (uint32_t)sp_m, i, (const F *)D1, pr0, pr1, part);
                        cval = spw;                                   // (each thread rewrites its own entry: in place from the second fold on)
                        S1 = D1; S_size = 4 * Q;
                        if (D1 == B1) { D1 = A1; D2 = A2; } else { D1 = B1; D2 = B2; }
                    }
                    HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce_post<9>, dim3(1), dim3(256), 0, part, nbs, mb, seq);
                } else if (eq) {
                    size_t lo_off = (size_t)1 << (rounds - eq_s); for (int l = 1; l <= i / 2; l++) lo_off += (size_t)1 << (eq_s - 2 * l);      // Lo of level i + 2
                    const F *f1 = eq->T == 2 ? eq_fac + eq_per_pt : eq_fac;
                    for (int j = 0; j < 2; j++) eq_al[j] = fmul(eq->a[j], sig[j]);
                    const EqSide es = {eq_fac + lo_off, f1 + lo_off, eq_fac, f1};
                    const int sh = eq_s - (i + 2), nbe = grid_for(4 * Q, pend ? 512 : 1024, EQ_MAXB);      // spans of 256 U elements
                    if (!pend) {
                        if (eq->T == 2) HB_LAUNCH(ctx, "k_sc2_eq_double", (k_sc2_eq_double<false, 2>), dim3(nbe), dim3(256), 0, es, sh, S2, (F *)nullptr, 4 * Q, pr0, pr1, eq_part);
                        else HB_LAUNCH(ctx, "k_sc2_eq_double", (k_sc2_eq_double<false, 1>), dim3(nbe), dim3(256), 0, es, sh, S2, (F *)nullptr, 4 * Q, pr0, pr1, eq_part);
                    } else {
                        if (eq->T == 2) HB_LAUNCH(ctx, "k_sc2_eq_double", (k_sc2_eq_double<true, 2>), dim3(nbe), dim3(256), 0, es, sh, S2, D2, 4 * Q, pr0, pr1, eq_part);
                        else HB_LAUNCH(ctx, "k_sc2_eq_double", (k_sc2_eq_double<true, 1>), dim3(nbe), dim3(256), 0, es, sh, S2, D2, 4 * Q, pr0, pr1, eq_part);
                        S2 = D2; S_size = 4 * Q;
                        if (D1 == B1) { D1 = A1; D2 = A2; } else { D1 = B1; D2 = B2; }
                    }
                    if (eq->T == 2) HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce_post<8>, dim3(1), dim3(256), 0, eq_part, nbe, mb, seq);
                    else HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce_post<4>, dim3(1), dim3(256), 0, eq_part, nbe, mb, seq);
                } else {
                if (!pend) HB_LAUNCH(ctx, "k_sc2_double", k_sc2_double<false>, dim3(nb), dim3(256), 0, S1, S2, (F *)nullptr, (F *)nullptr, Q, pr0, pr1, part);
                else {
                    HB_LAUNCH(ctx, "k_sc2_double", k_sc2_double<true>, dim3(nb), dim3(256), 0, S1, S2, D1, D2, Q, pr0, pr1, part);
                    S1 = D1; S2 = D2; S_size = 4 * Q;
                    if (D1 == B1) { D1 = A1; D2 = A2; } else { D1 = B1; D2 = B2; }
                }
                HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce_post<9>, dim3(1), dim3(256), 0, part, nb, mb, seq);
                }
                HB_TRY(ctx->mbox_wait(seq));
                F G[9]; for (int q = 0; q < 9; q++) G[q] = mb->vals[q];            // G(r, t) at (0,0) (1,0) (inf,0) | (0,1) (1,1) (inf,1) | (0,inf) (1,inf) (inf,inf)
                if (eq) {                                                           // posted: W_{j,p}.  G(rho, tau) = sum_j al_j E_j(rho) F_j(tau) S_j(rho, tau)
                    for (int q = 0; q < 9; q++) G[q] = fmake(0);
                    for (int j = 0; j < eq->T; j++) {
                        const F W[4] = {mb->vals[4 * j], mb->vals[4 * j + 1], mb->vals[4 * j + 2], mb->vals[4 * j + 3]};
                        const F d01 = fsub(W[1], W[0]), d23 = fsub(W[3], W[2]);
                        const F S[9] = {W[0], W[1], d01, W[2], W[3], d23, fsub(W[2], W[0]), fsub(W[3], W[1]), fsub(d23, d01)};
                        const F e1 = pts.r[j][i], e0 = fsub(fmake(1), e1), f1v = pts.r[j][i + 1], f0 = fsub(fmake(1), f1v);
                        const F E[3] = {e0, e1, fsub(e1, e0)}, Fv[3] = {fmul(eq_al[j], f0), fmul(eq_al[j], f1v), fmul(eq_al[j], fsub(f1v, f0))};
                        for (int tau = 0; tau < 3; tau++) for (int rho = 0; rho < 3; rho++) G[3 * tau + rho] = fadd(G[3 * tau + rho], fmul(fmul(E[rho], Fv[tau]), S[3 * tau + rho]));
                    }
                }
                // round i: G(r, 0) + G(r, 1) as (a, b, c) from its values at r = inf, 1, 0
                F p0[3]; p0[0] = fadd(G[2], G[5]); p0[2] = fadd(G[0], G[3]); p0[1] = fsub(fsub(fadd(G[1], G[4]), p0[0]), p0[2]);
                for (int q = 0; q < 3; q++) { rnd = mimc_hash(rnd, p0[q]); h_qpoly[3 * i + q] = p0[q]; }
                h_r[i] = rnd;
                const F r = rnd, rr = fmul(r, r);
                F v[3];                                                             // G(r_i, t) at t = 0, 1, inf
                for (int k = 0; k < 3; k++) { const F cc = G[3 * k], aa = G[3 * k + 2], bb = fsub(fsub(G[3 * k + 1], aa), cc); v[k] = fadd(cc, fadd(fmul(r, bb), fmul(rr, aa))); }
                const F p1[3] = {v[2], fsub(fsub(v[1], v[2]), v[0]), v[0]};         // round i + 1: (a, b, c)
                for (int q = 0; q < 3; q++) { rnd = mimc_hash(rnd, p1[q]); h_qpoly[3 * (i + 1) + q] = p1[q]; }
                h_r[i + 1] = rnd;
                if (eq) for (int j = 0; j < eq->T; j++) for (int b = 0; b < 2; b++) {              // sigma_{j,i+2}: the table's two index bits folded with (r_i, r_{i+1})
                    const F rho = pts.r[j][i + b], e0 = fsub(fmake(1), rho);
                    sig[j] = fmul(sig[j], fadd(e0, fmul(b ? rnd : r, fsub(rho, e0))));
                }
                pend = true; pr0 = r; pr1 = rnd; i += 2;
            }
            // bridge to the round-by-round loop: it expects s = T_{i-1} and rnd = r_{i-1}.  S = T_{i-2}: fold it once with r_{i-2}
            // (the polynomial this launch also sums is round i-1's, already known: its partials are not reduced).
            if (sparse) {                                             // the second table, dense from here on: level i - 2, beside S1 (n >= 16 SC_DOUBLE_MIN: S1 is A1 or B1)
                F *m2 = (S1 == A1) ? A2 : B2;
                HB_TRY(launch_zero(ctx, m2, S_size * sizeof(F)));
                HB_LAUNCH(ctx, "k_scatter_counted", k_scatter_counted, dim3(grid_for(sp_m, 256, MAXB)), dim3(256), 0, sp_idx, cval, (uint32_t)sp_m, i - 2, m2);
                S2 = m2;
            }
            if (eq) { HB_TRY(eq_table(i - 2, eq_al, eq_tab)); S1 = eq_tab; }      // the first table, dense from here on: level i - 2, S_size <= 2 SC_DOUBLE_MIN entries
            const bool at_A = eq ? S2 == A2 : S1 == A1;
            F *b1 = at_A ? B1 : A1, *b2 = at_A ? B2 : A2;
            const size_t L = S_size / 4;
            HB_LAUNCH(ctx, "k_sc2_fold_poly", k_sc2_fold_poly, dim3(grid_for(L, 256, MAXB)), dim3(256), 0, S1, S2, b1, b2, L, pr0, part, (F *)nullptr);   // (2 L >= 8 SC_TAIL: never the tail)
            s1 = b1; s2 = b2; cur = 2 * L;
            if (b1 == A1) { d1 = B1; d2 = B2; } else { d1 = A1; d2 = A2; }
        }
        for (;; i++) {
            size_t L = n >> (i + 1);          // pairs of the round-i tables
            int nb = grid_for(L, 256, MAXB);
            const uint32_t seq = ++ctx->mbox_seq;
            // The round whose tables the host continues from also lands them in the tail area, in front of the round's post: the fold launch
            // stores them there itself; round 0 on the caller's tables (SC_TAIL < n <= 2 SC_TAIL) has no fold launch and takes a copy launch.
            const bool last = 2 * L <= SC_TAIL_AREA || i == rounds - 1;      // the round-i tables (2 L elements each) are the host's: this round writes the tail area and ends the loop
            if (i == 0) {
                HB_LAUNCH(ctx, "k_sc2_poly", k_sc2_poly, dim3(nb), dim3(256), 0, s1, s2, L, part);
                if (last) HB_LAUNCH(ctx, "k_sc2_tail_copy", k_sc2_tail_copy, dim3(grid_for(cur, 256, 64)), dim3(256), 0, s1, s2, cur, ctx->tail);
            } else {
                HB_LAUNCH(ctx, "k_sc2_fold_poly", k_sc2_fold_poly, dim3(nb), dim3(256), 0, s1, s2, d1, d2, L, rnd, part, last ? ctx->tail : (F *)nullptr);
                s1 = d1; s2 = d2; cur = 2 * L;
                if (d1 == A1) { d1 = B1; d2 = B2; } else { d1 = A1; d2 = A2; }
            }
            HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce_post<3>, dim3(1), dim3(256), 0, part, nb, mb, seq);
            HB_TRY(ctx->mbox_wait(seq));                                  // the last workgroup posts the three coefficients to the host
            for (int q = 0; q < 3; q++) { const F cq = mb->vals[q]; rnd = mimc_hash(rnd, cq); h_qpoly[3 * i + q] = cq; }
            h_r[i] = rnd;
            if (last) break;                                    // the (unfolded) round-i tables are in the tail area: stored in front of the post that mbox_wait has just seen
        }
        sc2_host_tail(ta, tb, cur, rnd, true, i + 1, rounds, h_qpoly, h_r);
    }
    rnd = mimc_hash(rnd, ta[0]); rnd = mimc_hash(rnd, tb[0]);          // src/sumcheck.cpp:2444-2446
    h_vr[0] = ta[0]; h_vr[1] = tb[0]; *h_final = rnd;
    return 0;
}

// ---- degree-4 gate-consistency sumcheck (src/sumcheck.cpp:875-929) --------------------------------------
// Tables t[0..5] = fold_add, fold_beta, fold_L, fold_R, fold_O, fold_mul.  Per pair, twelve coefficient sums:
// c[0..3]  cubic   add * beta * (a0 L + a1 R)      (l1*l2*l3, src/polynomial.cpp:91-93,133-135)
// c[4..8]  quartic mul * beta * L * R              (cubic * linear, :99-101)
// c[9..11] quadratic beta * O
// The host combines them with a2, a3 (:899-903), hashes (mimc_hash(coefficient, rand): coefficient is the input) and folds.
template <int NT> struct GateTabsT { const F *s[NT]; F *d[NT]; };
HB_HD void cubic_acc(F *c, const F &b0, const F &d0, const F &b1, const F &d1, const F &b2, const F &d2) {     // (l1*l2)*l3
    F qa = fmul(d0, d1), qb = fadd(fmul(d0, b1), fmul(b0, d1)), qc = fmul(b0, b1);
    c[0] = fadd(c[0], fmul(qa, d2));
    c[1] = fadd(c[1], fadd(fmul(qa, b2), fmul(qb, d2)));
    c[2] = fadd(c[2], fadd(fmul(qb, b2), fmul(qc, d2)));
    c[3] = fadd(c[3], fmul(qc, b2));
}
HB_HD void quartic_acc(F *c, const F &bm, const F &dm, const F &bb, const F &db, const F &bl, const F &dl, const F &br, const F &dr) {   // ((mul*beta)*L)*R
    F ma = fmul(dm, db), mb = fadd(fmul(dm, bb), fmul(bm, db)), mc = fmul(bm, bb);
    F ka = fmul(ma, dl), kb = fadd(fmul(ma, bl), fmul(mb, dl)), kc = fadd(fmul(mb, bl), fmul(mc, dl)), kd = fmul(mc, bl);
    c[0] = fadd(c[0], fmul(ka, dr));
    c[1] = fadd(c[1], fadd(fmul(ka, br), fmul(kb, dr)));
    c[2] = fadd(c[2], fadd(fmul(kb, br), fmul(kc, dr)));
    c[3] = fadd(c[3], fadd(fmul(kc, br), fmul(kd, dr)));
    c[4] = fadd(c[4], fmul(kd, br));
}
HB_HD void quad_acc(F *c, const F &b0, const F &d0, const F &b1, const F &d1) {
    c[0] = fadd(c[0], fmul(d0, d1));
    c[1] = fadd(c[1], fadd(fmul(d0, b1), fmul(b0, d1)));
    c[2] = fadd(c[2], fmul(b0, b1));
}
// prove_gate_consistency / _standard: tables add, beta, L, R, O, mul; twelve sums
struct GateStd {
    static constexpr int NT = 6, NS = 12, NA = 4;
    static HB_HD void acc(F (&c)[12], const F (&b)[6], const F (&e)[6], const F &a0, const F &a1) {
        F d[6];
#pragma unroll
        for (int q = 0; q < 6; q++) d[q] = fsub(e[q], b[q]);
        const F l3a = fadd(fmul(a0, d[2]), fmul(a1, d[3])), l3b = fadd(fmul(a0, b[2]), fmul(a1, b[3]));
        cubic_acc(c, b[0], d[0], b[1], d[1], l3b, l3a);
        quartic_acc(c + 4, b[5], d[5], b[1], d[1], b[2], d[2], b[3], d[3]);
        quad_acc(c + 9, b[1], d[1], b[4], d[4]);
    }
    // combine the twelve sums into the quartic (a..e)  (:899-903)
    static void combine(const F *c, CHP a, F *p) {
        p[0] = fmul(a[2], c[4]);
        p[1] = fadd(fmul(a[2], c[5]), c[0]);
        p[2] = fadd(fadd(fmul(a[2], c[6]), c[1]), fmul(a[3], c[9]));
        p[3] = fadd(fadd(fmul(a[2], c[7]), c[2]), fmul(a[3], c[10]));
        p[4] = fadd(fadd(fmul(a[2], c[8]), c[3]), fmul(a[3], c[11]));
    }
};
// prove_gate_consistency_lookups (src/sumcheck.cpp:654-729): tables add_L, add_R, L, R, O, lkp, lkp_O, mul, beta; twenty sums:
// c[0..3] add_L*beta*L, c[4..7] add_R*beta*R, c[8..11] lkp*beta*lkp_O (cubics), c[12..16] mul*beta*L*R (quartic), c[17..19] beta*O
struct GateLkp {
    static constexpr int NT = 9, NS = 20, NA = 5;
    static HB_HD void acc(F (&c)[20], const F (&b)[9], const F (&e)[9], const F &, const F &) {
        F d[9];
#pragma unroll
        for (int q = 0; q < 9; q++) d[q] = fsub(e[q], b[q]);
        cubic_acc(c, b[0], d[0], b[8], d[8], b[2], d[2]);
        cubic_acc(c + 4, b[1], d[1], b[8], d[8], b[3], d[3]);
        cubic_acc(c + 8, b[5], d[5], b[8], d[8], b[6], d[6]);
        quartic_acc(c + 12, b[7], d[7], b[8], d[8], b[2], d[2], b[3], d[3]);
        quad_acc(c + 17, b[8], d[8], b[4], d[4]);
    }
    static void combine(const F *c, CHP a, F *p) {                       // (:689-704)
        F C[4];
        for (int k = 0; k < 4; k++) C[k] = fadd(fadd(fmul(a[0], c[k]), fmul(a[1], c[4 + k])), fmul(a[4], c[8 + k]));
        p[0] = fmul(a[2], c[12]);
        p[1] = fadd(fmul(a[2], c[13]), C[0]);
        p[2] = fadd(fadd(fmul(a[2], c[14]), C[1]), fmul(a[3], c[17]));
        p[3] = fadd(fadd(fmul(a[2], c[15]), C[2]), fmul(a[3], c[18]));
        p[4] = fadd(fadd(fmul(a[2], c[16]), C[3]), fmul(a[3], c[19]));
    }
};
// round 0: polynomial only
template <class G>
__global__ void __launch_bounds__(256) k_gate_poly(GateTabsT<G::NT> t, size_t L, F a0, F a1, F *__restrict__ partials) {
    F c[G::NS];
#pragma unroll
    for (int q = 0; q < G::NS; q++) c[q] = fmake(0);
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x) {
        F b[G::NT], e[G::NT];
#pragma unroll
        for (int q = 0; q < G::NT; q++) { b[q] = ldF(t.s[q] + 2 * j); e[q] = ldF(t.s[q] + 2 * j + 1); }
        G::acc(c, b, e, a0, a1);
    }
    block_reduce_store<G::NS>(c, partials);
}
// rounds >= 1: fold the previous tables (4 -> 2 elements per thread and table) and accumulate this round's sums
template <class G>
__global__ void __launch_bounds__(256) k_gate_fold_poly(GateTabsT<G::NT> t, size_t L, F r, F a0, F a1, F *__restrict__ partials) {
    F c[G::NS];
#pragma unroll
    for (int q = 0; q < G::NS; q++) c[q] = fmake(0);
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x) {
        F b[G::NT], e[G::NT];
#pragma unroll
        for (int q = 0; q < G::NT; q++) {
            F x0 = ldF(t.s[q] + 4 * j), x1 = ldF(t.s[q] + 4 * j + 1), x2 = ldF(t.s[q] + 4 * j + 2), x3 = ldF(t.s[q] + 4 * j + 3);
            b[q] = fadd(x0, fmul(r, fsub(x1, x0))); e[q] = fadd(x2, fmul(r, fsub(x3, x2)));
            stF(t.d[q] + 2 * j, b[q]); stF(t.d[q] + 2 * j + 1, e[q]);
        }
        G::acc(c, b, e, a0, a1);
    }
    block_reduce_store<G::NS>(c, partials);
}
// one transcript step: combine the sums into the quartic (a..e), hash, check against the running sum, evaluate
template <class G>
static bool gate_round_host(const F *c, CHP a, F &rnd, F &sum, MHP poly_out, MHP r_out) {
    F p[5];
    G::combine(c, a, p);
    for (int q = 0; q < 5; q++) { rnd = mimc_hash(p[q], rnd); poly_out[q] = p[q]; }
    F s01 = fadd(fadd(fadd(p[0], p[1]), fadd(p[2], p[3])), fadd(p[4], p[4]));
    bool ok = feq(s01, sum);                                              // "Error in gate consistency 2" (:909-912, :710-713)
    sum = fadd(fmul(fadd(fmul(fadd(fmul(fadd(fmul(p[0], rnd), p[1]), rnd), p[2]), rnd), p[3]), rnd), p[4]);
    *r_out = rnd;
    return ok;
}
// inputs are preserved (the reference folds in place and afterwards only reads element 0 of each table: h_final)
template <class G>
static int gate_sumcheck_impl(hobbit_ctx *ctx, const F *const *tabs, size_t n, CHP h_a, MHP h_rand, MHP h_sum, MHP h_poly, MHP h_r, MHP h_final, int *h_check) {
    constexpr int NT = G::NT, NS = G::NS;
    int rounds = 0; while (((size_t)1 << rounds) < n) rounds++;
    if (((size_t)1 << rounds) != n || n < 2) return ctx->fail(HOBBIT_EINVAL, "gate_sumcheck: n must be a power of two >= 2");
    const int MAXB = 512;
    F rnd = *h_rand, sum = *h_sum; bool ok = true;
    const F a0 = h_a[0], a1 = h_a[1];
    std::vector<F> host[NT];
    size_t cur = n; int i = 0; bool pending = false;
    if (n > SC_TAIL) {
        size_t szA = n / 2, szB = n / 4;
        F *ws; HB_TRY(ctx->workspace((NT * (szA + szB) + (size_t)MAXB * NS + NS + 4) * sizeof(F), (void **)&ws));
        F *A = ws, *B = A + NT * szA, *part = B + NT * szB, *coef = part + (size_t)MAXB * NS;
        F *pin; HB_TRY(ctx->pinned(NS * sizeof(F), (void **)&pin));
        GateTabsT<NT> t;
        for (int q = 0; q < NT; q++) { t.s[q] = tabs[q]; t.d[q] = A + (size_t)q * szA; }
        bool toA = true;
        for (;; i++) {
            size_t L = n >> (i + 1);
            int nb = grid_for(L, 256, MAXB);
            if (i == 0) HB_LAUNCH(ctx, "k_gate_poly", (k_gate_poly<G>), dim3(nb), dim3(256), 0, t, L, a0, a1, part);
            else {
                HB_LAUNCH(ctx, "k_gate_fold_poly", (k_gate_fold_poly<G>), dim3(nb), dim3(256), 0, t, L, rnd, a0, a1, part);
                cur = 2 * L; toA = !toA;
                for (int q = 0; q < NT; q++) { t.s[q] = t.d[q]; t.d[q] = toA ? A + (size_t)q * szA : B + (size_t)q * szB; }
            }
            HB_LAUNCH(ctx, "k_sc_reduce12", k_sc_reduce<NS>, dim3(1), dim3(256), 0, part, nb, coef);
            HB_CHECK(ctx, hipMemcpyAsync(pin, coef, NS * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
            HB_TRY(ctx->sync());
            ok &= gate_round_host<G>(pin, h_a, rnd, sum, h_poly + 5 * i, h_r + i);
            if (cur <= 2 * SC_TAIL || i == rounds - 1) break;
        }
        for (int q = 0; q < NT; q++) { host[q].resize(cur); HB_CHECK(ctx, hipMemcpyAsync(host[q].data(), t.s[q], cur * sizeof(F), hipMemcpyDeviceToHost, ctx->stream)); }
        HB_TRY(ctx->sync());
        pending = true; i++;
    } else {
        for (int q = 0; q < NT; q++) { host[q].resize(n); HB_CHECK(ctx, hipMemcpyAsync(host[q].data(), tabs[q], n * sizeof(F), hipMemcpyDeviceToHost, ctx->stream)); }
        HB_TRY(ctx->sync());
    }
    auto fold = [&]() { for (int q = 0; q < NT; q++) for (size_t j = 0; j < cur / 2; j++) host[q][j] = fadd(host[q][2 * j], fmul(rnd, fsub(host[q][2 * j + 1], host[q][2 * j]))); cur /= 2; };
    if (pending) fold();
    for (; i < rounds; i++) {
        F c[NS]; for (int q = 0; q < NS; q++) c[q] = fmake(0);
        for (size_t j = 0; j < cur / 2; j++) {
            F b[NT], e[NT];
            for (int q = 0; q < NT; q++) { b[q] = host[q][2 * j]; e[q] = host[q][2 * j + 1]; }
            G::acc(c, b, e, a0, a1);
        }
        ok &= gate_round_host<G>(c, h_a, rnd, sum, h_poly + 5 * i, h_r + i);
        fold();
    }
    for (int q = 0; q < NT; q++) h_final[q] = host[q][0];
    *h_rand = rnd; *h_sum = sum; *h_check = ok ? 1 : 0;
    return 0;
}
int launch_gate_sumcheck(hobbit_ctx *ctx, const F *const tabs[6], size_t n, CHP h_a, MHP h_rand, MHP h_sum, MHP h_poly, MHP h_r, MHP h_final, int *h_check) {
    return gate_sumcheck_impl<GateStd>(ctx, tabs, n, h_a, h_rand, h_sum, h_poly, h_r, h_final, h_check);
}
// tabs: add_L, add_R, L, R, O, lkp, lkp_O, mul, beta; h_a: 5 coefficients; h_final: the nine folded values in that order
int launch_gate_lkp_sumcheck(hobbit_ctx *ctx, const F *const tabs[9], size_t n, CHP h_a, MHP h_rand, MHP h_sum, MHP h_poly, MHP h_r, MHP h_final, int *h_check) {
    return gate_sumcheck_impl<GateLkp>(ctx, tabs, n, h_a, h_rand, h_sum, h_poly, h_r, h_final, h_check);
}

// 3-product: polynomial of the current tables and fold with the PRE-round challenge in one pass
__global__ void __launch_bounds__(256) k_sc3_poly_fold(const F *__restrict__ s1, const F *__restrict__ s2, const F *__restrict__ s3,
                                                       F *__restrict__ d1, F *__restrict__ d2, F *__restrict__ d3, size_t L,
                                                       F r, F *__restrict__ partials) {
    F c[4] = {fmake(0), fmake(0), fmake(0), fmake(0)};
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x) {
        F x0 = ldF(s1 + 2 * j), x1 = ldF(s1 + 2 * j + 1), y0 = ldF(s2 + 2 * j), y1 = ldF(s2 + 2 * j + 1), z0 = ldF(s3 + 2 * j), z1 = ldF(s3 + 2 * j + 1);
        F dx = fsub(x1, x0), dy = fsub(y1, y0), dz = fsub(z1, z0);
        // (l1*l2)*l3 with the reference's operator grouping (src/polynomial.cpp:91-93,133-135)
        F qa = fmul(dx, dy), qb = fadd(fmul(dx, y0), fmul(x0, dy)), qc = fmul(x0, y0);
        c[0] = fadd(c[0], fmul(qa, dz));
        c[1] = fadd(c[1], fadd(fmul(qa, z0), fmul(qb, dz)));
        c[2] = fadd(c[2], fadd(fmul(qb, z0), fmul(qc, dz)));
        c[3] = fadd(c[3], fmul(qc, z0));
        stF(d1 + j, fadd(x0, fmul(r, dx))); stF(d2 + j, fadd(y0, fmul(r, dy))); stF(d3 + j, fadd(z0, fmul(r, dz)));
    }
    block_reduce_store<4>(c, partials);
}
// cubic round polynomial only / fold only (batch_3product_sumcheck hashes first, then folds: src/sumcheck.cpp:327-352)
__global__ void __launch_bounds__(256) k_sc3_poly(const F *__restrict__ s1, const F *__restrict__ s2, const F *__restrict__ s3, size_t L, F *__restrict__ partials) {
    F c[4] = {fmake(0), fmake(0), fmake(0), fmake(0)};
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x) {
        F x0 = ldF(s1 + 2 * j), x1 = ldF(s1 + 2 * j + 1), y0 = ldF(s2 + 2 * j), y1 = ldF(s2 + 2 * j + 1), z0 = ldF(s3 + 2 * j), z1 = ldF(s3 + 2 * j + 1);
        F dx = fsub(x1, x0), dy = fsub(y1, y0), dz = fsub(z1, z0);
        F qa = fmul(dx, dy), qb = fadd(fmul(dx, y0), fmul(x0, dy)), qc = fmul(x0, y0);
        c[0] = fadd(c[0], fmul(qa, dz));
        c[1] = fadd(c[1], fadd(fmul(qa, z0), fmul(qb, dz)));
        c[2] = fadd(c[2], fadd(fmul(qb, z0), fmul(qc, dz)));
        c[3] = fadd(c[3], fmul(qc, z0));
    }
    block_reduce_store<4>(c, partials);
}
__global__ void __launch_bounds__(256) k_fold3(const F *__restrict__ s1, const F *__restrict__ s2, const F *__restrict__ s3, F *__restrict__ d1, F *__restrict__ d2,
                                               F *__restrict__ d3, size_t L, F r) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < L; j += (size_t)gridDim.x * blockDim.x) {
        F x0 = ldF(s1 + 2 * j), x1 = ldF(s1 + 2 * j + 1), y0 = ldF(s2 + 2 * j), y1 = ldF(s2 + 2 * j + 1), z0 = ldF(s3 + 2 * j), z1 = ldF(s3 + 2 * j + 1);
        stF(d1 + j, fadd(x0, fmul(r, fsub(x1, x0)))); stF(d2 + j, fadd(y0, fmul(r, fsub(y1, y0)))); stF(d3 + j, fadd(z0, fmul(r, fsub(z1, z0))));
    }
}
int launch_sc3_poly(hobbit_ctx *ctx, const F *s1, const F *s2, const F *s3, size_t L, F *part, F *coef) {
    int nb = grid_for(L, 256, 1024);
    HB_LAUNCH(ctx, "k_sc3_poly", k_sc3_poly, dim3(nb), dim3(256), 0, s1, s2, s3, L, part);
    HB_LAUNCH(ctx, "k_sc_reduce4", k_sc_reduce<4>, dim3(1), dim3(256), 0, part, nb, coef);
    return 0;
}
int launch_fold3(hobbit_ctx *ctx, const F *s1, const F *s2, const F *s3, F *d1, F *d2, F *d3, size_t L, F r) {
    HB_LAUNCH(ctx, "k_fold3", k_fold3, dim3(grid_for(L, 256)), dim3(256), 0, s1, s2, s3, d1, d2, d3, L, r);
    return 0;
}
// one layer of the multiplication tree (src/sumcheck.cpp:88-110): in1[j] = x[2j], in2[j] = x[2j+1], tr[j] = x[2j]*x[2j+1]
__global__ void __launch_bounds__(256) k_mul_layer(const F *__restrict__ x, size_t n_out, F *__restrict__ in1, F *__restrict__ in2, F *__restrict__ tr) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n_out; j += (size_t)gridDim.x * blockDim.x) {
        const F a = ldF(x + 2 * j), b = ldF(x + 2 * j + 1);
        stF(in1 + j, a); stF(in2 + j, b); stF(tr + j, fmul(a, b));
    }
}
int launch_mul_layer(hobbit_ctx *ctx, const F *x, size_t n_out, F *in1, F *in2, F *tr) {
    if (!n_out) return 0;
    HB_LAUNCH(ctx, "k_mul_layer", k_mul_layer, dim3(grid_for(n_out, 256)), dim3(256), 0, x, n_out, in1, in2, tr);
    return 0;
}

// host rounds of the 3-product sumcheck on tables of size sz (src/sumcheck.cpp:1981-2037)
static void sc3_host_tail(std::vector<F> &a, std::vector<F> &b, std::vector<F> &c3, F &rnd, int round, int rounds, MHP h_cpoly, MHP h_r) {
    size_t sz = a.size();
    for (int i = round; i < rounds; i++) {
        F pa = fmake(0), pb = fmake(0), pc = fmake(0), pd = fmake(0);
        for (size_t j = 0; j < sz / 2; j++) {
            F x0 = a[2 * j], y0 = b[2 * j], z0 = c3[2 * j];
            F dx = fsub(a[2 * j + 1], x0), dy = fsub(b[2 * j + 1], y0), dz = fsub(c3[2 * j + 1], z0);
            F qa = fmul(dx, dy), qb = fadd(fmul(dx, y0), fmul(x0, dy)), qc = fmul(x0, y0);
            pa = fadd(pa, fmul(qa, dz)); pb = fadd(pb, fadd(fmul(qa, z0), fmul(qb, dz)));
            pc = fadd(pc, fadd(fmul(qb, z0), fmul(qc, dz))); pd = fadd(pd, fmul(qc, z0));
            a[j] = fadd(x0, fmul(rnd, dx)); b[j] = fadd(y0, fmul(rnd, dy)); c3[j] = fadd(z0, fmul(rnd, dz));
        }
        h_r[i] = rnd;
        rnd = mimc_hash(rnd, pa); rnd = mimc_hash(rnd, pb); rnd = mimc_hash(rnd, pc); rnd = mimc_hash(rnd, pd);
        h_cpoly[4 * i] = pa; h_cpoly[4 * i + 1] = pb; h_cpoly[4 * i + 2] = pc; h_cpoly[4 * i + 3] = pd;
        sz /= 2;
    }
}
int launch_sumcheck3(hobbit_ctx *ctx, const F *v1, const F *v2, const F *v3, size_t n, F prev_r, MHP h_cpoly, MHP h_r, MHP h_vr, MHP h_final) {
    int rounds = 0; while (((size_t)1 << rounds) < n) rounds++;
    if (((size_t)1 << rounds) != n || n < 2) return ctx->fail(HOBBIT_EINVAL, "sumcheck3: n must be a power of two >= 2");
    const int MAXB = 1024;
    F rnd = prev_r;
    const F *s1 = v1, *s2 = v2, *s3 = v3;
    size_t cur = n;
    int i = 0;
    if (n > SC_TAIL) {
        size_t szA = n / 2, szB = n / 4;
        F *ws; HB_TRY(ctx->workspace((3 * szA + 3 * szB + (size_t)MAXB * 4 + 4) * sizeof(F), (void **)&ws));
        F *A = ws, *B = A + 3 * szA, *part = B + 3 * szB, *coef = part + (size_t)MAXB * 4;
        F *pin; HB_TRY(ctx->pinned(4 * sizeof(F), (void **)&pin));
        F *dst = A; size_t dsz = szA;
        for (; cur > SC_TAIL; i++) {
            size_t L = cur / 2;
            int nb = grid_for(L, 256, MAXB);
            HB_LAUNCH(ctx, "k_sc3_poly_fold", k_sc3_poly_fold, dim3(nb), dim3(256), 0, s1, s2, s3, dst, dst + dsz, dst + 2 * dsz, L, rnd, part);
            HB_LAUNCH(ctx, "k_sc_reduce4", k_sc_reduce<4>, dim3(1), dim3(256), 0, part, nb, coef);
            HB_CHECK(ctx, hipMemcpyAsync(pin, coef, 4 * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
            HB_TRY(ctx->sync());
            h_r[i] = rnd;                                           // randomness[i] = pre-round challenge
            for (int q = 0; q < 4; q++) { rnd = mimc_hash(rnd, pin[q]); h_cpoly[4 * i + q] = pin[q]; }
            s1 = dst; s2 = dst + dsz; s3 = dst + 2 * dsz; cur = L;
            if (dst == A) { dst = B; dsz = szB; } else { dst = A; dsz = szA; }
        }
    }
    std::vector<F> ta(cur), tb(cur), tc(cur);
    HB_CHECK(ctx, hipMemcpyAsync(ta.data(), s1, cur * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    HB_CHECK(ctx, hipMemcpyAsync(tb.data(), s2, cur * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    HB_CHECK(ctx, hipMemcpyAsync(tc.data(), s3, cur * sizeof(F), hipMemcpyDeviceToHost, ctx->stream));
    HB_TRY(ctx->sync());
    sc3_host_tail(ta, tb, tc, rnd, i, rounds, h_cpoly, h_r);
    rnd = mimc_hash(rnd, ta[0]); rnd = mimc_hash(rnd, tb[0]);      // v3[0] is not hashed (src/sumcheck.cpp:2043-2046)
    h_vr[0] = ta[0]; h_vr[1] = tb[0]; h_vr[2] = tc[0]; *h_final = rnd;
    return 0;
}

// ============================================================================================
// Elastic_PC open helpers (src/Elastic_PC.cpp:59-111 update_reply, :510-517 zero-chunk test; src/PC_utils.cpp:422-496)
// ============================================================================================
// *flag |= (some element of v is non-zero)
__global__ void k_any_nonzero(const F *__restrict__ v, size_t n, int *__restrict__ flag) {
    int nz = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { const F a = ldF(v + i); nz |= (a.re | a.im) != 0; }
    if (__any(nz) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
int launch_any_nonzero(hobbit_ctx *ctx, const F *v, size_t n, int *d_flag) {
    HB_LAUNCH(ctx, "k_any_nonzero", k_any_nonzero, dim3(grid_for(n, 256, 1024)), dim3(256), 0, v, n, d_flag);
    return 0;
}
// G[c*ldG + j] = T[j*ld + cols[c]], j < nrows: the queried columns of a row-major matrix, one per output row
__global__ void k_gather_cols(const F *__restrict__ T, size_t ld, uint32_t nrows, const uint32_t *__restrict__ cols, uint32_t ncols, F *__restrict__ G, size_t ldG) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)ncols * nrows) return;
    const uint32_t c = (uint32_t)(t / nrows), j = (uint32_t)(t % nrows);
    stF(G + (size_t)c * ldG + j, ldF(T + (size_t)j * ld + cols[c]));
}
int launch_gather_cols(hobbit_ctx *ctx, const F *T, size_t ld, uint32_t nrows, const uint32_t *d_cols, uint32_t ncols, F *G, size_t ldG) {
    if (!ncols || !nrows) return 0;
    HB_LAUNCH(ctx, "k_gather_cols", k_gather_cols, dim3((unsigned)(((size_t)ncols * nrows + 255) / 256)), dim3(256), 0, T, ld, nrows, d_cols, ncols, G, ldG);
    return 0;
}
// k_gather_cols on the row codes of base-field rows kept as columns 0 .. cols / 2 (row-major, cols / 2 + 1 elements per row): before the column
// code, column c > cols / 2 is the entry-wise conjugate of column cols - c (hobbit_half.hpp)
__global__ void k_gather_cols_half(const F *__restrict__ T, uint32_t cols, uint32_t nrows, const uint32_t *__restrict__ qcols, uint32_t ncols, F *__restrict__ G, size_t ldG) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)ncols * nrows) return;
    const uint32_t c = (uint32_t)(t / nrows), j = (uint32_t)(t % nrows), qc = qcols[c];
    const F v = ldF(T + (size_t)j * (cols / 2 + 1) + half_src_col(qc, cols));
    stF(G + (size_t)c * ldG + j, half_is_conj(qc, cols) ? fconj(v) : v);
}
int launch_gather_cols_half(hobbit_ctx *ctx, const F *T, uint32_t cols, uint32_t nrows, const uint32_t *d_cols, uint32_t ncols, F *G, size_t ldG) {
    if (!ncols || !nrows) return 0;
    HB_LAUNCH(ctx, "k_gather_cols_half", k_gather_cols_half, dim3((unsigned)(((size_t)ncols * nrows + 255) / 256)), dim3(256), 0, T, cols, nrows, d_cols, ncols, G, ldG);
    return 0;
}
// k_axpy and k_any_nonzero over base-field values: y += a * (x, 0), two F_p products per term
__global__ void k_axpy_real(F *__restrict__ y, const uint64_t *__restrict__ x, F a, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const uint64_t v = x[i];
        stF(y + i, fadd(ldF(y + i), fmake(mulp(a.re, v), mulp(a.im, v))));
    }
}
int launch_axpy_real(hobbit_ctx *ctx, F *y, const uint64_t *x, F a, size_t n) {
    HB_LAUNCH(ctx, "k_axpy_real", k_axpy_real, dim3(grid_for(n, 256)), dim3(256), 0, y, x, a, n);
    return 0;
}
__global__ void k_any_nonzero_real(const uint64_t *__restrict__ v, size_t n, int *__restrict__ flag) {
    int nz = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) nz |= v[i] != 0;
    if (__any(nz) && (threadIdx.x & 63) == 0) atomicOr(flag, 1);
}
int launch_any_nonzero_real(hobbit_ctx *ctx, const uint64_t *v, size_t n, int *d_flag) {
    HB_LAUNCH(ctx, "k_any_nonzero_real", k_any_nonzero_real, dim3(grid_for(n, 256, 1024)), dim3(256), 0, v, n, d_flag);
    return 0;
}
// out[cols[i] + j*ld] = vals[i], j < nrows: a column indicator weighted per column (recursive_prover_RS's second beta, src/PC_utils.cpp:489-496)
__global__ void k_spread_cols(const uint32_t *__restrict__ cols, const F *__restrict__ vals, uint32_t ncols, uint32_t nrows, size_t ld, F *__restrict__ out) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= (size_t)ncols * nrows) return;
    const uint32_t j = (uint32_t)(t / ncols), i = (uint32_t)(t % ncols);
    stF(out + (size_t)j * ld + cols[i], ldF(vals + i));
}
int launch_spread_cols(hobbit_ctx *ctx, const uint32_t *d_cols, const F *d_vals, uint32_t ncols, uint32_t nrows, size_t ld, F *out) {
    if (!ncols || !nrows) return 0;
    HB_LAUNCH(ctx, "k_spread_cols", k_spread_cols, dim3((unsigned)(((size_t)ncols * nrows + 255) / 256)), dim3(256), 0, d_cols, d_vals, ncols, nrows, ld, out);
    return 0;
}

// ============================================================================================
// Streaming provers: product layers of the stream (src/witness_stream.cpp:2413-2510 read_mul_tree_layer / read_mul_tree_data),
// partial evaluations (src/sumcheck.cpp:1327-1340, 949-959)
// ============================================================================================
// out[t] = prod_{j < seg} in[t*seg + j]
__global__ void k_seg_prod(const F *__restrict__ in, uint32_t seg, size_t n_out, F *__restrict__ out) {
    const size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (t >= n_out) return;
    const F *p = in + t * seg;
    F a = ldF(p);
    for (uint32_t j = 1; j < seg; j++) a = fmul(a, ldF(p + j));
    stF(out + t, a);
}
int launch_seg_prod(hobbit_ctx *ctx, const F *in, uint32_t seg, size_t n_out, F *out) {
    if (!n_out) return 0;
    HB_LAUNCH(ctx, "k_seg_prod", k_seg_prod, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, in, seg, n_out, out);
    return 0;
}
// a[j] = v[2j], b[j] = v[2j+1]
__global__ void k_deinterleave(const F *__restrict__ v, size_t n, F *__restrict__ a, F *__restrict__ b) {
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    stF(a + j, ldF(v + 2 * j)); stF(b + j, ldF(v + 2 * j + 1));
}
int launch_deinterleave(hobbit_ctx *ctx, const F *v, size_t n, F *a, F *b) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_deinterleave", k_deinterleave, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, v, n, a, b);
    return 0;
}
// sum_j a[j] * b[j*sb] (* c[j] when c != NULL)
__global__ void __launch_bounds__(256) k_dot_gen(const F *__restrict__ a, const F *__restrict__ b, size_t sb, const F *__restrict__ c, size_t n, F *__restrict__ partials) {
    F s[1] = {fmake(0)};
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
        F t = fmul(ldF(a + j), ldF(b + j * sb));
        if (c) t = fmul(t, ldF(c + j));
        s[0] = fadd(s[0], t);
    }
    block_reduce_store<1>(s, partials);
}
int launch_dot_gen(hobbit_ctx *ctx, const F *a, const F *b, size_t sb, const F *c, size_t n, F *part, F *out) {
    int nb = grid_for(n, 256, 1024);
    HB_LAUNCH(ctx, "k_dot_gen", k_dot_gen, dim3(nb), dim3(256), 0, a, b, sb, c, n, part);
    HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce<1>, dim3(1), dim3(256), 0, part, nb, out);
    return 0;
}
// sum_j a[j] * F(sel[j])  (one_minus: 1 - F(sel[j]))
__global__ void __launch_bounds__(256) k_dot_i32(const F *__restrict__ a, const int32_t *__restrict__ sel, int one_minus, size_t n, F *__restrict__ partials) {
    F s[1] = {fmake(0)};
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < n; j += (size_t)gridDim.x * blockDim.x) {
        F v = fmake((uint64_t)(int64_t)sel[j]);
        if (one_minus) v = fsub(fmake(1), v);
        s[0] = fadd(s[0], fmul(ldF(a + j), v));
    }
    block_reduce_store<1>(s, partials);
}
int launch_dot_i32(hobbit_ctx *ctx, const F *a, const int32_t *sel, int one_minus, size_t n, F *part, F *out) {
    int nb = grid_for(n, 256, 1024);
    HB_LAUNCH(ctx, "k_dot_i32", k_dot_i32, dim3(nb), dim3(256), 0, a, sel, one_minus, n, part);
    HB_LAUNCH(ctx, "k_sc_reduce", k_sc_reduce<1>, dim3(1), dim3(256), 0, part, nb, out);
    return 0;
}
// y[j] = F(sel[j]) or 1 - F(sel[j])
__global__ void k_i32_to_F(const int32_t *__restrict__ sel, int one_minus, size_t n, F *__restrict__ y) {
    const size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (j >= n) return;
    F v = fmake((uint64_t)(int64_t)sel[j]);
    if (one_minus) v = fsub(fmake(1), v);
    stF(y + j, v);
}
int launch_i32_to_F(hobbit_ctx *ctx, const int32_t *sel, int one_minus, size_t n, F *y) {
    if (!n) return 0;
    HB_LAUNCH(ctx, "k_i32_to_F", k_i32_to_F, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sel, one_minus, n, y);
    return 0;
}

// ============================================================================================
// Fill / copy as ordinary kernels.  The runtime's own hipMemsetAsync / device-to-device hipMemcpyAsync come with a 40-100 us idle gap in
// front of their internal kernels on this driver (rocprofv3 kernel trace of one open: 10 fills = 1.0 ms, 12 copies = 0.5 ms of GPU idle
// time); a plain launch has the usual 3-6 us.
// ============================================================================================
__global__ void k_zero16(uint4 *__restrict__ p, size_t n16) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = make_uint4(0, 0, 0, 0);
}
__global__ void k_copy16(uint4 *__restrict__ d, const uint4 *__restrict__ s, size_t n16) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}
int launch_zero(hobbit_ctx *ctx, void *p, size_t bytes) {
    if (!bytes) return 0;
    if ((bytes & 15) || ((uintptr_t)p & 15)) { hipError_t e = hipMemsetAsync(p, 0, bytes, ctx->stream); return e == hipSuccess ? 0 : ctx->hip(e, "hipMemsetAsync"); }
    HB_LAUNCH(ctx, "k_zero16", k_zero16, dim3(grid_for(bytes / 16, 256, 8192)), dim3(256), 0, reinterpret_cast<uint4 *>(p), bytes / 16);
    return 0;
}
int launch_copy(hobbit_ctx *ctx, void *d, const void *s, size_t bytes) {
    if (!bytes) return 0;
    if ((bytes & 15) || ((uintptr_t)d & 15) || ((uintptr_t)s & 15)) {
        hipError_t e = hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToDevice, ctx->stream); return e == hipSuccess ? 0 : ctx->hip(e, "hipMemcpyAsync");
    }
    HB_LAUNCH(ctx, "k_copy16", k_copy16, dim3(grid_for(bytes / 16, 256, 8192)), dim3(256), 0, reinterpret_cast<uint4 *>(d), reinterpret_cast<const uint4 *>(s), bytes / 16);
    return 0;
}

// ============================================================================================
// Brakedown (hobbit_brakedown_commit / _open): `rows` codewords of one code stored rows-innermost, element (i, c) at mat[c * rows + i]
// ============================================================================================
// One step of the encode over all rows at once (hobbit_ctx.hpp IlvStep): lane (t, i) owns output t of the step in row i and walks t's in-edge
// list; every edge gathers the `rows` contiguous inputs of its column, so a wave reads one 1 KB run per edge (rows >= 64) and the edge records
// are wave-uniform (scalar loads).  No LDS window: each step reads what the step before it wrote.  Same exact arithmetic as k_encode (four
// unreduced 96-bit sums per output and one fold; general weights: a canonical fmul / fadd per edge), so every codeword is bit-identical to
// hobbit_encode_batch's.
template <bool SMALLW>
__global__ void __launch_bounds__(256)
k_enc_ilv(F *__restrict__ mat, uint32_t rows, uint32_t lg_rows, IlvStep st, const uint32_t *__restrict__ ptr, const uint2 *__restrict__ e32,
          const uint32_t *__restrict__ eidx, const F *__restrict__ ew) {
    // 64-bit: a step of a code of 2^21 has up to 2^21 outputs, and hobbit_brakingbase_commit_any encodes up to 512 rows of them
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const uint32_t t = (uint32_t)(g >> lg_rows), i = (uint32_t)g & (rows - 1);
    if (t >= st.out_len) return;
    const F *in = mat + (size_t)st.in_off * rows + i;
    uint32_t beg = ptr[st.ptr_base + t], end = ptr[st.ptr_base + t + 1];
    if (rows >= 64) { beg = __builtin_amdgcn_readfirstlane(beg); end = __builtin_amdgcn_readfirstlane(end); }     // one output per wave
    F out;
    if (SMALLW) {
        Acc96 rl = {0, 0}, rh = {0, 0}, il = {0, 0}, ih = {0, 0};
        uint32_t e = beg;
        for (; e + 4 <= end; e += 4) {
            uint2 r[4]; uint4 x[4];
#pragma unroll
            for (int u = 0; u < 4; u++) r[u] = e32[e + u];
#pragma unroll
            for (int u = 0; u < 4; u++) x[u] = *reinterpret_cast<const uint4 *>(in + (size_t)r[u].x * rows);
#pragma unroll
            for (int u = 0; u < 4; u++) acc96_mad4(rl, rh, il, ih, r[u].y, x[u]);
        }
        for (; e < end; e++) {
            const uint2 r = e32[e];
            acc96_mad4(rl, rh, il, ih, r.y, *reinterpret_cast<const uint4 *>(in + (size_t)r.x * rows));
        }
        out = fmake(acc_fold(rl, rh), acc_fold(il, ih));
    } else {
        out = fmake(0);
        for (uint32_t e = beg; e < end; e++) out = fadd(out, fmul(ldF(in + (size_t)eidx[e] * rows), ldF(ew + e)));
    }
    stF(mat + (size_t)(st.out_off + t) * rows + i, out);
}
int launch_encode_ilv(hobbit_ctx *ctx, const F *src, F *dst, uint32_t rows) {
    const DeviceCode &c = ctx->code;
    uint32_t lg = 0; while ((1u << lg) < rows) lg++;
    if (src != dst) HB_TRY(launch_copy(ctx, dst, src, (size_t)c.n * rows * sizeof(F)));
    for (const IlvStep &st : c.isteps) {
        const size_t threads = (size_t)st.out_len * rows;
        if ((threads + 255) / 256 >> 31) return ctx->fail(HOBBIT_EINVAL, "encode_interleaved: a step of more than 2^39 outputs x rows");
        if (c.small_weights)
            HB_LAUNCH(ctx, "k_enc_ilv", k_enc_ilv<true>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, dst, rows, lg, st, c.d_ilv_ptr, c.d_ilv_e32,
                      c.d_ilv_eidx, c.d_ilv_ew);
        else
            HB_LAUNCH(ctx, "k_enc_ilv_fullw", k_enc_ilv<false>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, dst, rows, lg, st, c.d_ilv_ptr,
                      c.d_ilv_e32, c.d_ilv_eidx, c.d_ilv_ew);
    }
    return launch_zero(ctx, dst + (size_t)c.len * rows, (size_t)(2 * c.n - c.len) * rows * sizeof(F));    // the codewords' zero tail
}

// The same step on a matrix whose rows are `ld` apart, over its first `width` columns only (hobbit_encode_interleaved_ld): neither need be a
// power of two, so the thread index is split by a division and not by a shift.  The columns are cut into strips of `strip` (a multiple of 64,
// so a wave still owns one output and its edge records stay wave-uniform); the grid is STRIP-MAJOR: blocks [s * bps, (s + 1) * bps) walk every
// output of the step over the columns of strip s, so the workgroups in flight together gather from a window of in_len x strip elements and not
// from in_len x width.  strip >= width is the plain order of k_enc_ilv (all columns of a few outputs).  Arithmetic as k_enc_ilv, bit for bit.
template <bool SMALLW>
__global__ void __launch_bounds__(256)
k_enc_ilv_ld(F *__restrict__ mat, size_t ld, uint32_t width, uint32_t strip, uint32_t bps, IlvStep st, const uint32_t *__restrict__ ptr,
             const uint2 *__restrict__ e32, const uint32_t *__restrict__ eidx, const F *__restrict__ ew) {
    const uint32_t s = blockIdx.x / bps, item = (blockIdx.x - s * bps) * 256 + threadIdx.x;      // out_len * strip < 2^31 (the launcher)
    const uint32_t t = item / strip, col = s * strip + (item - t * strip);
    if (t >= st.out_len || col >= width) return;
    const F *in = mat + (size_t)st.in_off * ld + col;
    const uint32_t beg = __builtin_amdgcn_readfirstlane(ptr[st.ptr_base + t]), end = __builtin_amdgcn_readfirstlane(ptr[st.ptr_base + t + 1]);
    F out;
    if (SMALLW) {
        Acc96 rl = {0, 0}, rh = {0, 0}, il = {0, 0}, ih = {0, 0};
        uint32_t e = beg;
        for (; e + 4 <= end; e += 4) {
            uint2 r[4]; uint4 x[4];
#pragma unroll
            for (int u = 0; u < 4; u++) r[u] = e32[e + u];
#pragma unroll
            for (int u = 0; u < 4; u++) x[u] = *reinterpret_cast<const uint4 *>(in + (size_t)r[u].x * ld);
#pragma unroll
            for (int u = 0; u < 4; u++) acc96_mad4(rl, rh, il, ih, r[u].y, x[u]);
        }
        for (; e < end; e++) {
            const uint2 r = e32[e];
            acc96_mad4(rl, rh, il, ih, r.y, *reinterpret_cast<const uint4 *>(in + (size_t)r.x * ld));
        }
        out = fmake(acc_fold(rl, rh), acc_fold(il, ih));
    } else {
        out = fmake(0);
        for (uint32_t e = beg; e < end; e++) out = fadd(out, fmul(ldF(in + (size_t)eidx[e] * ld), ldF(ew + e)));
    }
    stF(mat + (size_t)(st.out_off + t) * ld + col, out);
}
// zeros into rows [row_lo, row_lo + nrows) x columns [col_lo, col_lo + ncols) of a matrix whose rows are ld apart
__global__ void k_zero_rect(F *__restrict__ mat, size_t ld, size_t row_lo, size_t nrows, size_t col_lo, size_t ncols) {
    const uint4 z = {0, 0, 0, 0};
    for (size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x; g < nrows * ncols; g += (size_t)gridDim.x * blockDim.x)
        *reinterpret_cast<uint4 *>(mat + (row_lo + g / ncols) * ld + col_lo + g % ncols) = z;
}
int launch_zero_rect(hobbit_ctx *ctx, F *mat, size_t ld, size_t row_lo, size_t nrows, size_t col_lo, size_t ncols) {
    if (!nrows || !ncols) return 0;
    HB_LAUNCH(ctx, "k_zero_rect", k_zero_rect, dim3(grid_for(nrows * ncols, 256, 1 << 16)), dim3(256), 0, mat, ld, row_lo, nrows, col_lo, ncols);
    return 0;
}
// in place on the 2n x ld matrix, columns [0, width); strip = 0: the plain order.  The caller has checked 2 n roundup64(width) < 2^31.
int launch_encode_ilv_ld(hobbit_ctx *ctx, F *mat, uint32_t width, size_t ld, uint32_t strip) {
    const DeviceCode &c = ctx->code;
    const uint32_t w64 = (width + 63) / 64 * 64;
    if (!strip || strip > w64) strip = w64;
    const uint32_t nstrips = (width + strip - 1) / strip;
    for (const IlvStep &st : c.isteps) {
        const uint32_t bps = (uint32_t)(((size_t)st.out_len * strip + 255) / 256);
        if (c.small_weights)
            HB_LAUNCH(ctx, "k_enc_ilv_ld", k_enc_ilv_ld<true>, dim3(nstrips * bps), dim3(256), 0, mat, ld, width, strip, bps, st, c.d_ilv_ptr, c.d_ilv_e32,
                      c.d_ilv_eidx, c.d_ilv_ew);
        else
            HB_LAUNCH(ctx, "k_enc_ilv_ld_fullw", k_enc_ilv_ld<false>, dim3(nstrips * bps), dim3(256), 0, mat, ld, width, strip, bps, st, c.d_ilv_ptr,
                      c.d_ilv_e32, c.d_ilv_eidx, c.d_ilv_ew);
    }
    return launch_zero_rect(ctx, mat, ld, (size_t)c.len, (size_t)(2 * c.n - c.len), 0, width);                // the codewords' zero tail
}

// Column digests of the matrix (MT_commit_Blake over the `rows` entries of column c, src/merkle_tree.cpp:193-221): leaf l = H(rows 4l..4l+3),
// which is 64 contiguous bytes here.  quirk (create_tree_blake's parent H(left | left), src/merkle_tree.cpp:275-280): the digest is leaf 0
// re-hashed log2(rows / 4) times, 1 + log2(rows / 4) compressions.  Otherwise the full tree over the rows / 4 leaves (rows <= 512), folded
// bottom-up through a stack of at most 8 pending nodes.  The codewords' zero tail makes the last columns all zero: the launcher hashes the first
// of them here and copies its digest to the rest (k_bd_fill).
__global__ void __launch_bounds__(256)
k_bd_digest(const F *__restrict__ mat, uint32_t rows, size_t ncols, int quirk, uint8_t *__restrict__ out) {
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < ncols; c += (size_t)gridDim.x * blockDim.x) {
        const uint32_t *col = reinterpret_cast<const uint32_t *>(mat + c * rows);
        const uint32_t leaves = rows / 4;
        uint32_t m[16], h[8];
        if (quirk) {
#pragma unroll
            for (int q = 0; q < 16; q++) m[q] = col[q];
            blake3_compress64(m, h);
            for (uint32_t n = leaves; n > 1; n >>= 1) {
#pragma unroll
                for (int q = 0; q < 8; q++) { m[q] = h[q]; m[8 + q] = h[q]; }
                blake3_compress64(m, h);
            }
            store8w(out + 32 * c, h);
            continue;
        }
        uint32_t stk[8][8]; int sp = 0;
        for (uint32_t l = 0; l < leaves; l++) {
            for (int q = 0; q < 16; q++) m[q] = col[16 * l + q];
            blake3_compress64(m, h);
            for (uint32_t k = l; k & 1; k >>= 1) {                // the pending left sibling of every completed subtree
                sp--;
                for (int q = 0; q < 8; q++) { m[q] = stk[sp][q]; m[8 + q] = h[q]; }
                blake3_compress64(m, h);
            }
            for (int q = 0; q < 8; q++) stk[sp][q] = h[q];
            sp++;
        }
        store8w(out + 32 * c, stk[0]);
    }
}
__global__ void k_bd_fill(uint8_t *__restrict__ out, size_t from, size_t n) {
    const uint4 *s = reinterpret_cast<const uint4 *>(out + 32 * (from - 1));
    const uint4 a = s[0], b = s[1];
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < n; c += (size_t)gridDim.x * blockDim.x) {
        uint4 *d = reinterpret_cast<uint4 *>(out + 32 * (from + c));
        d[0] = a; d[1] = b;
    }
}
// digests of columns [0, ncols) into out[0 .. ncols + nz): the last nz columns are zero, so their digest is computed once (column ncols) and copied
int launch_brakedown_digests(hobbit_ctx *ctx, const F *mat, uint32_t rows, size_t ncols, size_t nz, int quirk, uint8_t *out) {
    const size_t comp = ncols + (nz ? 1 : 0);
    HB_LAUNCH(ctx, "k_bd_digest", k_bd_digest, dim3(grid_for(comp, 256, 8192)), dim3(256), 0, mat, rows, comp, quirk, out);
    if (nz > 1) HB_LAUNCH(ctx, "k_bd_fill", k_bd_fill, dim3(grid_for(nz - 1, 256)), dim3(256), 0, out, comp, nz - 1);
    return 0;
}

// aggr_beta[j] = sum_i beta[i] T[i][j], aggr_r[j] = sum_i r[i] T[i][j] for j < B (src/Our_PC.cpp:452-457), both from ONE read of the message
// columns: G = min(rows, 64) lanes per column, each summing rows / G entries, then a butterfly over the G lanes.
__global__ void __launch_bounds__(256)
k_bd_aggr(const F *__restrict__ mat, uint32_t rows, uint32_t lg_g, size_t B, const F *__restrict__ beta, const F *__restrict__ r, F *__restrict__ ab,
          F *__restrict__ ar) {
    const uint32_t G = 1u << lg_g;
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x, j = g >> lg_g;
    const uint32_t sub = (uint32_t)g & (G - 1);
    F sb = fmake(0), sr = fmake(0);
    if (j < B)
        for (uint32_t i = sub; i < rows; i += G) {
            const F x = ldF(mat + j * rows + i);
            sb = fadd(sb, fmul(ldF(beta + i), x)); sr = fadd(sr, fmul(ldF(r + i), x));
        }
    for (uint32_t m = 1; m < G; m <<= 1) { sb = fadd(sb, shfl_xor_F(sb, (int)m)); sr = fadd(sr, shfl_xor_F(sr, (int)m)); }
    if (j < B && sub == 0) { stF(ab + j, sb); stF(ar + j, sr); }
}
int launch_brakedown_aggr(hobbit_ctx *ctx, const F *mat, uint32_t rows, size_t B, const F *beta, const F *r, F *aggr_beta, F *aggr_r) {
    uint32_t lg = 0; while ((1u << lg) < rows && lg < 6) lg++;
    const size_t threads = B << lg;
    HB_LAUNCH(ctx, "k_bd_aggr", k_bd_aggr, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, mat, rows, lg, B, beta, r, aggr_beta, aggr_r);
    return 0;
}
// reply[q][i] = T[i][I[q]] (src/Our_PC.cpp:462-468): one contiguous run of `rows` elements per query
__global__ void __launch_bounds__(256)
k_bd_reply(const F *__restrict__ mat, uint32_t rows, const uint32_t *__restrict__ I, size_t nq, F *__restrict__ reply) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= nq * rows) return;
    const size_t q = g / rows, i = g % rows;
    stF(reply + g, ldF(mat + (size_t)I[q] * rows + i));
}
int launch_brakedown_reply(hobbit_ctx *ctx, const F *mat, uint32_t rows, const uint32_t *d_I, size_t nq, F *reply) {
    if (!nq) return 0;
    HB_LAUNCH(ctx, "k_bd_reply", k_bd_reply, dim3((unsigned)((nq * rows + 255) / 256)), dim3(256), 0, mat, rows, d_I, nq, reply);
    return 0;
}

// ============================================================================================
// Streaming Brakedown (hobbit_brakedown_stream_*, src/Elastic_PC.cpp:112-172, 287-313): a group of four consecutive chunks is kept as a
// 2B x 4 matrix, rows-innermost (element (i, c) at mat[c * 4 + i]), so a column is one 64-byte line: the xyzw block of the leaf hash, the
// four summands of the aggregates and the four replies of a query.  The encode of a group is launch_encode_ilv at rows = 4.
// ============================================================================================
// the chunk into row `slot` of the message columns: mat[c * 4 + slot] = chunk[c]
__global__ void __launch_bounds__(256)
k_bds_put(const F *__restrict__ chunk, size_t B, uint32_t slot, F *__restrict__ mat) {
    for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < B; c += (size_t)gridDim.x * blockDim.x) stF(mat + 4 * c + slot, ldF(chunk + c));
}
int launch_bds_put(hobbit_ctx *ctx, const F *chunk, size_t B, uint32_t slot, F *mat) {
    HB_LAUNCH(ctx, "k_bds_put", k_bds_put, dim3(grid_for(B, 256, 1 << 16)), dim3(256), 0, chunk, B, slot, mat);
    return 0;
}
// leaf[j] = H( H(c0[j + shift] | c1[j + shift] | c2[j] | c3[j]) | leaf[j] ) for all W = 2B leaves (:145-149; shift = 1 is the call as built by
// GCC, see k_elastic_leaf): the first 32 bytes of column j + shift and the last 32 bytes of column j, two compressions, the state updated in
// place.  Columns from `len` on (the codewords' zero tail, and the one past the arrays that leaf 2B - 1 asks for) are taken as zero, not read.
__global__ void __launch_bounds__(256)
k_bds_leaf(const F *__restrict__ mat, size_t len, size_t W, int shift, uint8_t *__restrict__ state) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < W; j += (size_t)gridDim.x * blockDim.x) {
        const size_t ja = j + (shift ? 1 : 0);
        uint4 a = make_uint4(0, 0, 0, 0), b = a, c = a, d = a;
        if (ja < len) { const uint4 *p = reinterpret_cast<const uint4 *>(mat + 4 * ja); a = p[0]; b = p[1]; }
        if (j < len) { const uint4 *p = reinterpret_cast<const uint4 *>(mat + 4 * j + 2); c = p[0]; d = p[1]; }
        uint32_t m[16], h[8];
        m[0] = a.x; m[1] = a.y; m[2] = a.z; m[3] = a.w; m[4] = b.x; m[5] = b.y; m[6] = b.z; m[7] = b.w;
        m[8] = c.x; m[9] = c.y; m[10] = c.z; m[11] = c.w; m[12] = d.x; m[13] = d.y; m[14] = d.z; m[15] = d.w;
        blake3_compress64(m, h);
#pragma unroll
        for (int q = 0; q < 8; q++) m[q] = h[q];
        load8w(state + 32 * j, m + 8);
        blake3_compress64(m, h);
        store8w(state + 32 * j, h);
    }
}
int launch_bds_leaf(hobbit_ctx *ctx, const F *mat, size_t len, size_t W, int shift, uint8_t *state) {
    HB_LAUNCH(ctx, "k_bds_leaf", k_bds_leaf, dim3(grid_for(W, 256, 1 << 16)), dim3(256), 0, mat, len, W, shift, state);
    return 0;
}
// aggregate_brakedown (:287-299) for one group: ab[j] += sum_i beta[i] x[i][j], ar[j] += sum_i rv[i] x[i][j] over the group's four chunks,
// both from one read of message column j (beta / rv point at the group's four weights)
__global__ void __launch_bounds__(256)
k_bds_aggr(const F *__restrict__ mat, size_t B, const F *__restrict__ beta, const F *__restrict__ rv, F *__restrict__ ab, F *__restrict__ ar) {
    for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < B; j += (size_t)gridDim.x * blockDim.x) {
        F sb = ldF(ab + j), sr = ldF(ar + j);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const F x = ldF(mat + 4 * j + i);
            sb = fadd(sb, fmul(ldF(beta + i), x)); sr = fadd(sr, fmul(ldF(rv + i), x));
        }
        stF(ab + j, sb); stF(ar + j, sr);
    }
}
int launch_bds_aggr(hobbit_ctx *ctx, const F *mat, size_t B, const F *beta, const F *rv, F *ab, F *ar) {
    HB_LAUNCH(ctx, "k_bds_aggr", k_bds_aggr, dim3(grid_for(B, 256, 1 << 16)), dim3(256), 0, mat, B, beta, rv, ab, ar);
    return 0;
}
// compute_reply (:301-313) for one group: reply[q][first + i] = codeword_{first + i}[I[q]], i < 4: one 64-byte run per query
__global__ void __launch_bounds__(256)
k_bds_reply(const F *__restrict__ mat, const uint32_t *__restrict__ I, size_t nq, size_t chunks, size_t first, F *__restrict__ reply) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x, q = g >> 2;
    const uint32_t i = (uint32_t)g & 3;
    if (q < nq) stF(reply + q * chunks + first + i, ldF(mat + 4 * (size_t)I[q] + i));
}
int launch_bds_reply(hobbit_ctx *ctx, const F *mat, const uint32_t *d_I, size_t nq, size_t chunks, size_t first, F *reply) {
    if (!nq) return 0;
    HB_LAUNCH(ctx, "k_bds_reply", k_bds_reply, dim3((unsigned)((4 * nq + 255) / 256)), dim3(256), 0, mat, d_I, nq, chunks, first, reply);
    return 0;
}

}  // namespace hobbit
