// hobbit_whir.hip -- the out-of-domain step of _whir_prove (src/Virgo.cpp:613-633) without the eq tables (include/hobbit_whir.h).
//
// Per iteration: R points z_i in F^v, cur = 2^v folded coefficients,
//     y_i = <eq(z_i), poly>,      beta += sum_i pw_i eq(z_i).
// precompute_beta puts z[0] on the index's least significant bit, so with vl low variables
//     eq(z)[h 2^vl + l] = Ehi[i][h] Elo[i][l],      Ehi = eq(z[vl..v)) (2^(v-vl) entries),  Elo = eq(z[0..vl)) (2^vl entries),
// and both halves of the step are R cur products over tables that stay small:
//     A (k_whir_ood_y):     T[i][h] = sum_l Elo[i][l] poly[h][l],   y_i = sum_h Ehi[i][h] T[i][h]        -- poly read once
//     B (k_whir_ood_beta):  beta[h][l] += sum_i Ehi[i][h] (pw_i Elo[i][l])                               -- beta read and written once
// The materialised form (hobbit_whir_prove) writes and reads R tables of cur entries: 2 x 100 x N/16 elements of scratch, 13.4 GB at 2^26.
//
// vl = 4.  In A a lane owns one row h: its 16 coefficients sit in registers for all R points, every product has the Elo entry as its
// wave-uniform operand, read from LDS (R x 16 entries, at most 32 KB: one ds_read_b128 at one address per 16 multiply-adds), and the 16
// products of a row are summed lazily (hobbit_whir_acc.hpp).  224 VGPRs (the row with its limbs split once), 2 waves per SIMD; vl = 3 takes
// 130 and doubles the high table, vl = 5 needs 128 for the row alone.  The row loads are 256 B apart across lanes; at R x 17 products per
// row their cost does not show.  In B a lane owns 4 consecutive entries of beta (a coalesced 64 B) with four lazy sums over i: 104 VGPRs,
// 4 waves.  Neither kernel uses scratch memory (kernel-resource-usage remarks and measurements: DESIGN.md section 4).
#include <algorithm>
#include <vector>
#include "hobbit_kernels.hpp"
#include "hobbit_dev.hpp"
#include "hobbit_whir_acc.hpp"
#include "../../include/hobbit_whir.h"

using namespace hobbit;

namespace {

constexpr int OOD_WG = 256, OOD_Y_GRID = 1024, OOD_BETA_GRID = 2048;

// A.  One lane per row h of 2^VL coefficients.  blockIdx.y takes a slice of `per` points, so that few rows (a short polynomial: 4096
// rows at N = 2^20) still fill the chip; LDS holds the slice only: its Elo (per << VL entries), then one running y per wave and point (4 per).
// ypart[i * gridDim.x + blockIdx.x] = this workgroup's share of y_i.
template <int VL>
__global__ void __launch_bounds__(OOD_WG) k_whir_ood_y(const F *__restrict__ poly, const F *__restrict__ Elo, const F *__restrict__ Ehi, size_t rows, int R,
                                                       F *__restrict__ ypart) {
    extern __shared__ F ood_lds[];
    constexpr int CH = 1 << VL;
    const int per = (R + gridDim.y - 1) / gridDim.y, i0 = blockIdx.y * per, n = i0 >= R ? 0 : (i0 + per < R ? per : R - i0);
    F *sE = ood_lds, *ys = ood_lds + ((size_t)per << VL);
    for (int t = threadIdx.x; t < (n << VL); t += OOD_WG) stF(&sE[t], ldF(Elo + ((size_t)i0 << VL) + t));
    for (int t = threadIdx.x; t < 4 * per; t += OOD_WG) stF(&ys[t], fmake(0));
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (size_t base = (size_t)blockIdx.x * OOD_WG; base < rows; base += (size_t)gridDim.x * OOD_WG) {      // uniform over the workgroup
        const size_t h = base + threadIdx.x;
        const bool act = h < rows;
        F row[CH];
#pragma unroll
        for (int l = 0; l < CH; l++) row[l] = act ? ldF(poly + (h << VL) + l) : fmake(0);
        for (int i = 0; i < n; i++) {
            LazyAcc acc = lazy_zero();
#pragma unroll
            for (int l = 0; l < CH; l++) lazy_mad(acc, ldF(&sE[(i << VL) + l]), row[l]);
            const F e = act ? ldF(Ehi + (size_t)(i0 + i) * rows + h) : fmake(0);
            const F s = wave_sum(fmul(e, lazy_value(acc)));
            if (lane == 0) stF(&ys[wave * per + i], fadd(ldF(&ys[wave * per + i]), s));                   // a wave's own slots: no barrier
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += OOD_WG)
        stF(ypart + (size_t)(i0 + i) * gridDim.x + blockIdx.x, fadd(fadd(ldF(&ys[i]), ldF(&ys[per + i])), fadd(ldF(&ys[2 * per + i]), ldF(&ys[3 * per + i]))));
}
// y_i = sum of its nparts partial sums (one workgroup per point)
__global__ void __launch_bounds__(OOD_WG) k_whir_ood_ysum(const F *__restrict__ ypart, int nparts, F *__restrict__ y) {
    __shared__ F red[4];
    const F *p = ypart + (size_t)blockIdx.x * nparts;
    F a = fmake(0);
    for (int j = threadIdx.x; j < nparts; j += OOD_WG) a = fadd(a, ldF(p + j));
    a = wave_sum(a);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) stF(y + blockIdx.x, fadd(fadd(red[0], red[1]), fadd(red[2], red[3])));
}
// B.  One lane per CH consecutive entries of beta (CH divides 2^vl: they share h); LDS: pw_i Elo[i][l].
template <int CH>
__global__ void __launch_bounds__(OOD_WG) k_whir_ood_beta(F *__restrict__ beta, const F *__restrict__ Elo, const F *__restrict__ Ehi, const F *__restrict__ pw, int vl,
                                                          size_t rows, int R) {
    extern __shared__ F ood_lds[];
    F *sE = ood_lds;
    for (int t = threadIdx.x; t < (R << vl); t += OOD_WG) stF(&sE[t], fmul(ldF(pw + (t >> vl)), ldF(Elo + t)));
    __syncthreads();
    const size_t nT = (rows << vl) / CH;
    const uint32_t lmask = (1u << vl) - 1;
    for (size_t t = (size_t)blockIdx.x * OOD_WG + threadIdx.x; t < nT; t += (size_t)gridDim.x * OOD_WG) {
        const size_t e0 = t * CH, h = e0 >> vl;
        const uint32_t l0 = (uint32_t)e0 & lmask;
        LazyAcc acc[CH];
#pragma unroll
        for (int j = 0; j < CH; j++) acc[j] = lazy_zero();
        for (int i = 0; i < R; i++) {
            const F c = ldF(Ehi + (size_t)i * rows + h);
#pragma unroll
            for (int j = 0; j < CH; j++) lazy_mad(acc[j], c, ldF(&sE[(i << vl) + l0 + j]));
        }
#pragma unroll
        for (int j = 0; j < CH; j++) stF(beta + e0 + j, fadd(ldF(beta + e0 + j), lazy_value(acc[j])));
    }
}
// host values into device memory through the launch's own arguments: nothing a later call could rewrite while this one is still queued
struct ArgBlock { F v[240]; };
__global__ void k_put_F(ArgBlock a, F *__restrict__ dst, int n) {
    if ((int)threadIdx.x < n) stF(dst + threadIdx.x, a.v[threadIdx.x]);
}

}  // namespace

namespace hobbit {

size_t whir_ood_scratch_elems(int v, int R) {
    const int vl = v < WHIR_OOD_VL ? v : WHIR_OOD_VL;
    return 2048 + 2 * (size_t)R * ((size_t)1 << (v - vl)) + (size_t)R * OOD_Y_GRID;
}
// dz: R x v (point-major), dzlo: R x vl (the first vl entries of every point, packed), dpw: R -- all on the device; scratch: whir_ood_scratch_elems
int launch_whir_ood(hobbit_ctx *ctx, const F *poly, F *beta, int v, const F *dz, const F *dzlo, const F *dpw, int R, F *scratch, F *d_y) {
    if (v < 1 || v > 26 || R < 1 || R > 128) return ctx->fail(HOBBIT_EINVAL, "whir_ood: 1 <= v <= 26 and 1 <= R <= 128");
    const int vl = v < WHIR_OOD_VL ? v : WHIR_OOD_VL, vh = v - vl;
    const size_t rows = (size_t)1 << vh;
    F *Elo = scratch, *cE = scratch + 2048, *nE = cE + (size_t)R * rows, *ypart = nE + (size_t)R * rows;
    // the tables, by the batched eq kernels: level i of a table takes z[v - 1 - i], so the high table is the first vh levels of the full one
    HB_TRY(launch_eq_head_batched(ctx, Elo, (size_t)1 << vl, dzlo, vl, vl, R));
    const int hd = vh < 11 ? vh : 11;
    HB_TRY(launch_eq_head_batched(ctx, cE, rows, dz, v, hd, R));
    for (int l = hd; l < vh; l++) { HB_TRY(launch_eq_step_batched(ctx, cE, nE, (size_t)1 << l, rows, dz, v, l, R)); std::swap(cE, nE); }
    const int gy = (int)std::min<size_t>((rows + OOD_WG - 1) / OOD_WG, OOD_Y_GRID);
    int ny = OOD_Y_GRID / gy; ny = ny < 1 ? 1 : ny > R ? R : ny;                  // slices of the points: about OOD_Y_GRID workgroups in all
    ny = (R + (R + ny - 1) / ny - 1) / ((R + ny - 1) / ny);                       // no empty slice
    const size_t per = ((size_t)R + ny - 1) / ny;                                 // points per slice, as the kernel derives it from gridDim.y
    const size_t lds_y = ((per << vl) + 4 * per) * sizeof(F), lds_b = ((size_t)R << vl) * sizeof(F);
    switch (vl) {
        case 1: HB_LAUNCH(ctx, "k_whir_ood_y", k_whir_ood_y<1>, dim3(gy, ny), dim3(OOD_WG), lds_y, poly, Elo, cE, rows, R, ypart); break;
        case 2: HB_LAUNCH(ctx, "k_whir_ood_y", k_whir_ood_y<2>, dim3(gy, ny), dim3(OOD_WG), lds_y, poly, Elo, cE, rows, R, ypart); break;
        case 3: HB_LAUNCH(ctx, "k_whir_ood_y", k_whir_ood_y<3>, dim3(gy, ny), dim3(OOD_WG), lds_y, poly, Elo, cE, rows, R, ypart); break;
        default: HB_LAUNCH(ctx, "k_whir_ood_y", k_whir_ood_y<4>, dim3(gy, ny), dim3(OOD_WG), lds_y, poly, Elo, cE, rows, R, ypart); break;
    }
    HB_LAUNCH(ctx, "k_whir_ood_ysum", k_whir_ood_ysum, dim3(R), dim3(OOD_WG), 0, ypart, gy, d_y);
    if (vl >= 2) {
        const int gb = (int)std::min<size_t>((((rows << vl) / 4) + OOD_WG - 1) / OOD_WG, OOD_BETA_GRID);
        HB_LAUNCH(ctx, "k_whir_ood_beta", k_whir_ood_beta<4>, dim3(gb), dim3(OOD_WG), lds_b, beta, Elo, cE, dpw, vl, rows, R);
    } else {
        HB_LAUNCH(ctx, "k_whir_ood_beta", k_whir_ood_beta<1>, dim3(1), dim3(OOD_WG), lds_b, beta, Elo, cE, dpw, vl, rows, R);
    }
    return 0;
}

}  // namespace hobbit

extern "C" {

int hobbit_whir_ood(hobbit_ctx *ctx, const hobbit_F *d_poly, hobbit_F *d_beta, int v, const hobbit_F *h_z, const hobbit_F *h_pw, int R, hobbit_F *d_y) {
    if (!ctx) return HOBBIT_EINVAL;
    if (!d_poly || !d_beta || !h_z || !h_pw || !d_y) return ctx->fail(HOBBIT_EINVAL, "whir_ood: NULL argument");
    if (v < 1 || v > 26 || R < 1 || R > 128) return ctx->fail(HOBBIT_EINVAL, "whir_ood: 1 <= v <= 26 and 1 <= R <= 128");
    const int vl = v < WHIR_OOD_VL ? v : WHIR_OOD_VL;
    const CHP z(reinterpret_cast<const HF *>(h_z)), pw(reinterpret_cast<const HF *>(h_pw));
    // z | zlo | pw, consumed here: they travel in launch arguments
    std::vector<F> in; in.reserve((size_t)R * (v + vl + 1));
    for (size_t t = 0; t < (size_t)R * v; t++) in.push_back(F(z[t]));
    for (int i = 0; i < R; i++) for (int j = 0; j < vl; j++) in.push_back(F(z[(size_t)i * v + j]));
    for (int i = 0; i < R; i++) in.push_back(F(pw[i]));
    const size_t sc = whir_ood_scratch_elems(v, R);
    F *ws; HB_TRY(ctx->workspace((sc + in.size()) * sizeof(F), (void **)&ws));
    F *din = ws + sc;
    for (size_t off = 0; off < in.size(); off += 240) {
        const int n = (int)std::min<size_t>(240, in.size() - off);
        ArgBlock a;
        for (int t = 0; t < 240; t++) a.v[t] = t < n ? in[off + t] : fmake(0);
        HB_LAUNCH(ctx, "k_put_F", k_put_F, dim3(1), dim3(256), 0, a, din + off, n);
    }
    return launch_whir_ood(ctx, reinterpret_cast<const F *>(d_poly), reinterpret_cast<F *>(d_beta), v, din, din + (size_t)R * v, din + (size_t)R * (v + vl), R, ws,
                           reinterpret_cast<F *>(d_y));
}

}  // extern "C"
