// hobbit_dev.hpp -- the device and launch helpers that every kernel file shares (hobbit_kernels.hip, hobbit_fft.hip, hobbit_whir.hip)
#pragma once
#include <atomic>
#include "hobbit_ctx.hpp"

namespace hobbit {
// The dynamic-LDS limit is an attribute of the function ON ONE DEVICE: latched per device (bit = device ordinal), not per process -- a host that
// creates contexts on several devices from one process must set it on each (torchrun's one device per process never noticed).
static inline void set_lds_limit_once(hobbit_ctx *ctx, const void *kernel, int bytes, std::atomic<uint64_t> &done) {
    const uint64_t bit = 1ull << (ctx->device & 63);
    if (!(done.load(std::memory_order_relaxed) & bit)) { hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); done.fetch_or(bit); }
}
static inline int grid_for(size_t n, int block, int cap = 4096) {
    const size_t g = (n + block - 1) / block;
    return (int)(g < 1 ? 1 : g > (size_t)cap ? (size_t)cap : g);
}
__device__ __forceinline__ F ldF(const F *p) {
    const uint4 v = *reinterpret_cast<const uint4 *>(p);     // one global_load_dwordx4 / ds_read_b128
    F r; r.re = (uint64_t)v.x | ((uint64_t)v.y << 32); r.im = (uint64_t)v.z | ((uint64_t)v.w << 32); return r;
}
__device__ __forceinline__ void stF(F *p, const F &a) {
    uint4 v; v.x = (uint32_t)a.re; v.y = (uint32_t)(a.re >> 32); v.z = (uint32_t)a.im; v.w = (uint32_t)(a.im >> 32);
    *reinterpret_cast<uint4 *>(p) = v;
}
__device__ __forceinline__ F shfl_down_F(const F &a, int d) {
    F r;
    r.re = __shfl_down((unsigned long long)a.re, d, 64);
    r.im = __shfl_down((unsigned long long)a.im, d, 64);
    return r;
}
// sum over the 64 lanes of a wavefront; result valid in lane 0
__device__ __forceinline__ F wave_sum(F a) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) a = fadd(a, shfl_down_F(a, d));
    return a;
}
}  // namespace hobbit
