// device_block.h -- device memory of the library's stateful objects: a POOL of parked blocks, a BLOCK that owns what it holds, and
// CARVE, which cuts one block into aligned pieces.
// Why a pool: hipMalloc + hipFree of ~100 MB cost 0.5 ms of a 4.4-ms leaf call, hipFree of a few MB 0.2 ms, and a tree code (or the
// drop-in call) makes and destroys a plan (a context) per step.  The block of a finished object is parked, and the next object on
// that device that it is large enough for takes it.  Nothing in the library relies on fresh memory being zero.  There are two pools
// (kLeafPolicy, kCtxPolicy): the same code with four constants of policy.  nbx_release_cached() empties both.
// The part above the __HIPCC__ guard is plain C++ over {device, pointer, bytes} records with the allocate and free calls passed in
// (tests/test_device_block_cpu.py drives it with a counting allocator under ASan / UBSan).
#pragma once
#include <cstddef>
#include <mutex>
#include <vector>

namespace nbx_block {

struct Policy {
    size_t park_max;        // a larger block is freed at once
    size_t per_device;      // parked blocks kept per device
    bool evict_oldest;      // which one goes when there are more: the one parked first, or (false) the smallest
    bool take_near_fit;     // true: a parked block is taken only up to 4 x the bytes wanted + 1 MiB; false: any that is large enough
};
// Leaf plans: a call takes two blocks (the staged bodies; everything else), and the two largest are kept.
constexpr Policy kLeafPolicy = {(size_t)2 << 30, 2, false, false};
// Contexts.  1 GiB: a context's block carries the fp64 pass's sums (8 x dim x pad doubles: 201 MB at N = 2^20, 805 MB at 2^22), and a
// one-shot call per step at such sizes would otherwise allocate and free hundreds of MB each time; 288 GB of HBM do not miss two
// idle blocks.  A small context does not sit on a much larger block than it asked for.
constexpr Policy kCtxPolicy = {(size_t)1 << 30, 2, true, true};

// The allocate and free calls.  alloc answers 0, `out_of_memory`, or another code of the caller's (handed through as it is).
struct Backend {
    int (*alloc)(int device, size_t bytes, char** out);
    void (*free)(int device, char* p);
    void (*release_all_pools)();   // follows an out-of-memory answer, before the ONE retry: the parked blocks may be what is in the way
    int out_of_memory;
};

inline int alloc_retry(const Backend& b, int device, size_t bytes, char** out) {
    int e = b.alloc(device, bytes, out);
    if (e == b.out_of_memory) {
        b.release_all_pools();
        e = b.alloc(device, bytes, out);
    }
    return e;
}

class Pool {
public:
    Pool(const Policy& policy, const Backend& backend) : policy_(policy), backend_(backend) {}
    const Backend& backend() const { return backend_; }

    // The smallest parked block of `device` that holds `bytes` (and is not too large for them, Policy::take_near_fit), else a new
    // allocation.  *got: the bytes the block really has.
    int take(int device, size_t bytes, char** out, size_t* got) {
        {
            std::lock_guard<std::mutex> lock(mu_);
            size_t best = parked_.size();
            for (size_t i = 0; i < parked_.size(); ++i) {
                const Parked& a = parked_[i];
                if (a.device != device || a.bytes < bytes || (policy_.take_near_fit && a.bytes > 4 * bytes + ((size_t)1 << 20))) continue;
                if (best == parked_.size() || a.bytes < parked_[best].bytes) best = i;
            }
            if (best != parked_.size()) {
                *out = parked_[best].p;
                *got = parked_[best].bytes;
                parked_.erase(parked_.begin() + (long)best);
                return 0;
            }
        }
        *got = bytes;
        return alloc_retry(backend_, device, bytes, out);
    }

    void park(int device, char* p, size_t bytes) {   // nothing on the device uses p any more
        Parked evicted{device, p, bytes};
        if (bytes <= policy_.park_max) {
            std::lock_guard<std::mutex> lock(mu_);
            parked_.push_back(evicted);
            evicted.p = nullptr;
            size_t mine = 0, victim = parked_.size();
            for (size_t i = 0; i < parked_.size(); ++i) {
                if (parked_[i].device != device) continue;
                ++mine;
                if (victim == parked_.size() || (!policy_.evict_oldest && parked_[i].bytes < parked_[victim].bytes)) victim = i;
            }
            if (mine > policy_.per_device) {
                evicted = parked_[victim];
                parked_.erase(parked_.begin() + (long)victim);
            }
        }
        if (evicted.p) backend_.free(evicted.device, evicted.p);
    }

    void release_all() {
        std::vector<Parked> parked;
        {
            std::lock_guard<std::mutex> lock(mu_);
            parked.swap(parked_);
        }
        for (const Parked& a : parked) backend_.free(a.device, a.p);
    }

    size_t parked_count() {
        std::lock_guard<std::mutex> lock(mu_);
        return parked_.size();
    }

private:
    struct Parked { int device; char* p; size_t bytes; };
    const Policy policy_;
    const Backend backend_;
    std::mutex mu_;                // the pool's own: no other lock is held while it is
    std::vector<Parked> parked_;   // oldest first
};

// One device allocation and its owner: from a pool (given back to it: parked when the device is idle, freed otherwise) or a plain
// allocation (always freed).  Move-only; a block that was released or moved from holds nothing, so a second release frees nothing.
class Block {
public:
    Block() = default;
    Block(const Block&) = delete;
    Block& operator=(const Block&) = delete;
    Block(Block&& o) noexcept { steal(o); }
    Block& operator=(Block&& o) noexcept {
        if (this != &o) { release(false); steal(o); }
        return *this;
    }
    ~Block() { release(false); }

    explicit operator bool() const { return p_ != nullptr; }
    char* get() const { return p_; }
    size_t bytes() const { return bytes_; }   // what the block really has: a parked one may be larger than asked for
    template <typename T> T* as() const { return reinterpret_cast<T*>(p_); }

    // one of at least `bytes` from the pool (what the block held before is freed) ...
    int take(Pool& pool, int device, size_t bytes) { return hold(&pool, pool.backend(), device, bytes); }
    // ... or a plain allocation, which no pool ever sees
    int allocate(const Backend& b, int device, size_t bytes) { return hold(nullptr, b, device, bytes); }
    // A block of at least `bytes`: the one held when it is large enough, else that one parked and another taken.  The caller has
    // made sure that nothing on the device uses the block.
    int fit(Pool& pool, int device, size_t bytes) {
        if (p_ && bytes_ >= bytes) return 0;
        release(true);
        return take(pool, device, bytes);
    }
    void release(bool device_idle) {
        if (!p_) return;
        if (pool_ && device_idle) pool_->park(device_, p_, bytes_);
        else backend_->free(device_, p_);
        p_ = nullptr; bytes_ = 0;
    }

private:
    int hold(Pool* pool, const Backend& b, int device, size_t bytes) {
        release(false);
        const int e = pool ? pool->take(device, bytes, &p_, &bytes_) : b.alloc(device, bytes, &p_);
        if (e) { p_ = nullptr; bytes_ = 0; return e; }
        backend_ = &b; pool_ = pool; device_ = device;
        if (!pool) bytes_ = bytes;
        return 0;
    }
    void steal(Block& o) {
        backend_ = o.backend_; pool_ = o.pool_; device_ = o.device_; p_ = o.p_; bytes_ = o.bytes_;
        o.p_ = nullptr; o.bytes_ = 0;
    }
    const Backend* backend_ = nullptr;
    Pool* pool_ = nullptr;
    int device_ = 0;
    char* p_ = nullptr;
    size_t bytes_ = 0;
};

// One allocation cut into N pieces: each starts on a 256-byte boundary and has at least 256 bytes of slack behind it (the pair
// kernels' pad pair lies behind xp, for one).
constexpr size_t carve_span(size_t bytes) { return (bytes + 255) / 256 * 256 + 256; }
template <size_t N>
struct Carved {
    size_t off[N], total;
    template <typename T> T* at(char* base, size_t i) const { return reinterpret_cast<T*>(base + off[i]); }
};
template <size_t N>
Carved<N> carve(const size_t (&sizes)[N]) {
    Carved<N> c;
    c.total = 0;
    for (size_t i = 0; i < N; ++i) { c.off[i] = c.total; c.total += carve_span(sizes[i]); }
    return c;
}

}  // namespace nbx_block

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
namespace nbx_block {
Pool& leaf_pool();   // nbx_api.hip: the two pools over hipMalloc / hipFree
Pool& ctx_pool();
const Backend& hip_backend();
inline hipError_t take(Block& b, Pool& pool, int device, size_t bytes) { return (hipError_t)b.take(pool, device, bytes); }
inline hipError_t fit(Block& b, Pool& pool, int device, size_t bytes) { return (hipError_t)b.fit(pool, device, bytes); }
inline hipError_t allocate(Block& b, int device, size_t bytes) { return (hipError_t)b.allocate(hip_backend(), device, bytes); }
}  // namespace nbx_block
#endif
