// hobbit_mem.hpp -- who owns device and pinned host memory behind the C ABI, in four types:
//   Buf<T, Where>   one raw allocation; frees in its destructor, never waits for a stream
//   GrowBuf<Where>  grow-only scratch: waits for the stream, frees, allocates -- in that order -- when a request passes its capacity
//   Pool            size-keyed free list; hands a parked buffer on without waiting, waits before a real free
//   Pooled<T>       one buffer of a Pool; goes back to it in its destructor
// Every raw call goes through the seam mem::raw (alloc, free, wait) and is counted on the way: hobbit_mem_live() reads the process-wide count of
// live allocations.  A stand-alone test defines HOBBIT_MEM_FAKE and declares mem::raw itself before it includes this header
// (tests/mem_owner_check.cpp): the header then needs neither the HIP headers nor a device.
#pragma once
#include <atomic>
#include <cstddef>
#include <map>
#include <utility>
#include "../../include/hobbit_hip.h"

namespace hobbit { namespace mem {

enum Where { Device, Pinned };

#ifndef HOBBIT_MEM_FAKE
}}
#include <hip/hip_runtime.h>
namespace hobbit { namespace mem { namespace raw {
using stream_t = hipStream_t;
inline void *alloc(Where w, size_t bytes, unsigned flags) {
    void *p = nullptr;
    return (w == Device ? hipMalloc(&p, bytes) : hipHostMalloc(&p, bytes, flags)) == hipSuccess ? p : nullptr;
}
inline void free(Where w, void *p) { if (w == Device) (void)hipFree(p); else (void)hipHostFree(p); }
inline void wait(stream_t s) { (void)hipStreamSynchronize(s); }
}
#endif

inline std::atomic<size_t> live_allocs{0}, live_bytes{0};     // atomic: shockwave_prove(C_c) allocates on a helper thread
inline void *take(Where w, size_t bytes, unsigned flags = 0) {
    void *p = raw::alloc(w, bytes, flags);
    if (p) { live_allocs++; live_bytes += bytes; }
    return p;
}
inline void give(Where w, void *p, size_t bytes) { raw::free(w, p); live_allocs--; live_bytes -= bytes; }

template <class T, Where W = Device>
class Buf {
    T *p_ = nullptr; size_t bytes_ = 0;
public:
    Buf() = default;
    Buf(Buf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    Buf &operator=(Buf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; } return *this; }
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() { reset(); }
    // n elements (pinned: `flags` of hipHostMalloc); drops what it held.  HOBBIT_ENOMEM and empty on failure.
    int alloc(size_t n, unsigned flags = 0) { return alloc_bytes(n * sizeof(T), flags); }
    int alloc_bytes(size_t bytes, unsigned flags = 0) {
        reset();
        p_ = static_cast<T *>(take(W, bytes, flags));
        if (!p_) return HOBBIT_ENOMEM;
        bytes_ = bytes; return 0;
    }
    void reset() { if (p_) give(W, (void *)p_, bytes_); p_ = nullptr; bytes_ = 0; }
    T *release() { T *p = p_; p_ = nullptr; bytes_ = 0; return p; }           // hand over: the caller frees (adopt() on the other side)
    void adopt(T *p, size_t bytes) { reset(); p_ = p; bytes_ = p ? bytes : 0; }
    operator T *() const { return p_; }
    T *operator->() const { return p_; }
    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }
};

template <Where W>
class GrowBuf {
    Buf<void, W> b_;
public:
    int ensure(raw::stream_t s, size_t bytes, void **p) {
        if (bytes > b_.bytes()) {
            if (b_) { raw::wait(s); b_.reset(); }
            if (b_.alloc_bytes(bytes)) return HOBBIT_ENOMEM;
        }
        *p = b_; return 0;
    }
    size_t bytes() const { return b_.bytes(); }
};

// Size-keyed free list for the device buffers of short-lived objects (a streaming commit or opening allocates five to nine buffers and
// releases them at its end: at the MLP config's shape the hipFree calls cost as much as the whole commit, 0.9 ms).  One stream per
// context, so a buffer handed back while kernels still read it is safe to hand out again: the next user is ordered behind them.
class Pool {
    std::multimap<size_t, void *> parked_; size_t parked_bytes_ = 0;
    std::map<void *, size_t> lent_;
public:
    static constexpr size_t MAX_PARKED = 48, MAX_BYTES = (size_t)8 << 30;
    raw::stream_t stream{};
    Pool() = default;
    Pool(const Pool &) = delete;
    Pool &operator=(const Pool &) = delete;
    ~Pool() { for (auto &kv : parked_) give(Device, kv.second, kv.first); }     // the owner drains (with the wait) while the stream still exists
    int get(size_t bytes, void **p) {
        auto it = parked_.find(bytes);
        if (it != parked_.end()) { *p = it->second; parked_bytes_ -= bytes; parked_.erase(it); return 0; }
        if (!(*p = take(Device, bytes))) {           // make room: drop everything parked, try once more
            drain();
            if (!(*p = take(Device, bytes))) return HOBBIT_ENOMEM;
        }
        return 0;
    }
    void put(size_t bytes, void *p) {
        if (!p) return;
        if (parked_.size() >= MAX_PARKED || parked_bytes_ + bytes > MAX_BYTES) { raw::wait(stream); give(Device, p, bytes); return; }
        parked_.emplace(bytes, p); parked_bytes_ += bytes;
    }
    void drain() {
        if (parked_.empty()) return;
        raw::wait(stream);
        for (auto &kv : parked_) give(Device, kv.second, kv.first);
        parked_.clear(); parked_bytes_ = 0;
    }
    // hobbit_malloc / hobbit_free hand out raw pointers: the pool remembers the sizes of those it lent
    int lend(size_t bytes, void **p) { if (get(bytes, p)) return HOBBIT_ENOMEM; lent_[*p] = bytes; return 0; }
    bool take_back(void *p) {
        auto it = lent_.find(p);
        if (it == lent_.end()) return false;
        const size_t bytes = it->second; lent_.erase(it); put(bytes, p); return true;
    }
    size_t parked() const { return parked_.size(); }
    size_t parked_bytes() const { return parked_bytes_; }
};

template <class T>
class Pooled {
    Pool *pool_ = nullptr; T *p_ = nullptr; size_t bytes_ = 0;
public:
    Pooled() = default;
    Pooled(Pooled &&o) noexcept : pool_(o.pool_), p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    Pooled &operator=(Pooled &&o) noexcept { if (this != &o) { reset(); pool_ = o.pool_; p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; } return *this; }
    Pooled(const Pooled &) = delete;
    Pooled &operator=(const Pooled &) = delete;
    ~Pooled() { reset(); }
    int get(Pool &pool, size_t bytes) {
        reset();
        void *p = nullptr;
        if (pool.get(bytes, &p)) return HOBBIT_ENOMEM;
        pool_ = &pool; p_ = static_cast<T *>(p); bytes_ = bytes; return 0;
    }
    void reset() { if (p_) pool_->put(bytes_, (void *)p_); p_ = nullptr; bytes_ = 0; }
    operator T *() const { return p_; }
    T *get() const { return p_; }
    size_t bytes() const { return bytes_; }
};

}}  // namespace hobbit::mem
