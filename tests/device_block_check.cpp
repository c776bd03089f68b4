// device_block_check.cpp -- the plain-C++ part of csrc/device_block.h (the parked-block pool's policy, the owning Block, carve) driven
// by a counting allocator, under ASan / UBSan (tests/test_device_block_cpu.py builds and runs it).  Every "device" block is a host
// allocation, so a block freed twice or never is the sanitizers' finding as well as the counters'.
#include "../nbody-simulation-parallel_amd/csrc/device_block.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>

using namespace nbx_block;

namespace {

constexpr int kOom = 2;
constexpr size_t MiB = (size_t)1 << 20;

struct Fake {
    std::map<char*, int> live;     // block -> device
    std::map<char*, int> freed;    // block -> times freed
    int allocs = 0, frees = 0, releases = 0;
    int oom_left = 0;              // the next that many allocations answer out of memory
    Pool* pools[2] = {nullptr, nullptr};
} g;

// a "device allocation" is a byte of host memory: the sizes under test go up to GiB
int fake_alloc(int device, size_t, char** out) {
    ++g.allocs;
    *out = nullptr;
    if (g.oom_left > 0) { --g.oom_left; return kOom; }
    *out = static_cast<char*>(std::malloc(1));
    g.live[*out] = device;
    return 0;
}
void fake_free(int device, char* p) {
    ++g.frees;
    ++g.freed[p];
    if (!g.live.count(p) || g.live[p] != device) { std::printf("FAIL: freed %p, not a live block of device %d\n", (void*)p, device); std::exit(1); }
    g.live.erase(p);
    std::free(p);
}
void fake_release_all() {
    ++g.releases;
    for (Pool* pool : g.pools) if (pool) pool->release_all();
}
const Backend kFake = {fake_alloc, fake_free, fake_release_all, kOom};

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

char* fresh(Pool& pool, int device, size_t bytes) {   // a new allocation, the way an object gets one
    char* p = nullptr;
    size_t got = 0;
    CHECK(pool.take(device, bytes, &p, &got) == 0 && p && got == bytes);
    return p;
}

void leaf_policy() {
    Pool pool(kLeafPolicy, kFake);
    g = Fake();
    // three blocks parked on one device: the smallest is evicted and freed exactly once
    char* a = fresh(pool, 0, 30 * MiB);
    char* b = fresh(pool, 0, 10 * MiB);
    char* c = fresh(pool, 0, 20 * MiB);
    CHECK(g.allocs == 3);
    pool.park(0, a, 30 * MiB);
    pool.park(0, b, 10 * MiB);
    CHECK(g.frees == 0 && pool.parked_count() == 2);
    pool.park(0, c, 20 * MiB);
    CHECK(g.frees == 1 && g.freed[b] == 1 && pool.parked_count() == 2);
    // a take returns the smallest block that fits (and a much larger one than asked for is fine here)
    char* p = nullptr;
    size_t got = 0;
    CHECK(pool.take(0, 1 * MiB, &p, &got) == 0 && p == c && got == 20 * MiB && g.allocs == 3);
    CHECK(pool.take(0, 25 * MiB, &p, &got) == 0 && p == a && got == 30 * MiB && g.allocs == 3);
    CHECK(pool.parked_count() == 0);
    pool.park(0, a, 30 * MiB);
    pool.park(0, c, 20 * MiB);
    CHECK(pool.take(0, 31 * MiB, &p, &got) == 0 && p != a && p != c && got == 31 * MiB && g.allocs == 4);   // nothing fits: a new one
    char* const d = p;
    // a block above the cap is freed at once
    pool.park(0, d, kLeafPolicy.park_max + 1);
    CHECK(g.frees == 2 && g.freed[d] == 1 && pool.parked_count() == 2);
    char* const e = fresh(pool, 0, kLeafPolicy.park_max);   // the cap itself is parked; it is the largest now, so `c` goes
    pool.park(0, e, kLeafPolicy.park_max);
    CHECK(g.frees == 3 && g.freed[c] == 1 && pool.parked_count() == 2);
    // another device's blocks are not counted or taken
    char* const x = fresh(pool, 1, 50 * MiB);
    char* const y = fresh(pool, 1, 60 * MiB);
    pool.park(1, x, 50 * MiB);
    pool.park(1, y, 60 * MiB);
    CHECK(g.frees == 3 && pool.parked_count() == 4);
    CHECK(pool.take(2, 1 * MiB, &p, &got) == 0 && p != a && p != e && p != x && p != y && got == 1 * MiB);
    pool.park(2, p, 1 * MiB);
    CHECK(pool.take(1, 55 * MiB, &p, &got) == 0 && p == y);
    pool.park(1, y, 60 * MiB);
    // release-all frees each block once
    const int before = g.frees;
    pool.release_all();
    CHECK(g.frees == before + 5 && pool.parked_count() == 0 && g.live.empty());
    for (const auto& f : g.freed) CHECK(f.second == 1);
    pool.release_all();
    CHECK(g.frees == before + 5);
}

void ctx_policy() {
    Pool pool(kCtxPolicy, kFake);
    g = Fake();
    // the oldest block is evicted, whatever its size
    char* a = fresh(pool, 0, 30 * MiB);
    char* b = fresh(pool, 0, 10 * MiB);
    char* c = fresh(pool, 0, 20 * MiB);
    pool.park(0, a, 30 * MiB);
    pool.park(0, b, 10 * MiB);
    pool.park(0, c, 20 * MiB);
    CHECK(g.frees == 1 && g.freed[a] == 1 && pool.parked_count() == 2);
    // a parked block larger than 4 x want + 1 MiB is not taken (10 MiB against 4 x 2 + 1) ...
    char* p = nullptr;
    size_t got = 0;
    CHECK(pool.take(0, 2 * MiB, &p, &got) == 0 && p != b && p != c && got == 2 * MiB && g.allocs == 4 && pool.parked_count() == 2);
    char* const d = p;
    // ... at the bound it is, and among those that may be taken the smallest
    CHECK(pool.take(0, 2 * MiB + MiB / 4, &p, &got) == 0 && p == b && got == 10 * MiB && g.allocs == 4);
    pool.park(0, b, 10 * MiB);                      // c (20 MiB) is the older one now, b the newer
    CHECK(pool.take(0, 5 * MiB, &p, &got) == 0 && p == b && g.allocs == 4);
    pool.park(0, b, 10 * MiB);
    pool.park(0, d, 2 * MiB);                       // three again: c, the oldest (and the largest), goes
    CHECK(g.frees == 2 && g.freed[c] == 1 && pool.parked_count() == 2);
    pool.park(0, fresh(pool, 0, kCtxPolicy.park_max + 1), kCtxPolicy.park_max + 1);   // above the cap: freed at once
    CHECK(g.frees == 3 && pool.parked_count() == 2);
    pool.release_all();
    CHECK(g.frees == 5 && g.live.empty());
    for (const auto& f : g.freed) CHECK(f.second == 1);
}

// an allocator that reports out-of-memory: both pools are released, and the allocation is tried exactly once more
void out_of_memory(const Policy* policy) {
    Pool mine(*policy, kFake), other(policy == &kLeafPolicy ? kCtxPolicy : kLeafPolicy, kFake);
    g = Fake();
    g.pools[0] = &mine; g.pools[1] = &other;
    mine.park(0, fresh(mine, 0, 4 * MiB), 4 * MiB);
    other.park(0, fresh(other, 0, 4 * MiB), 4 * MiB);
    other.park(1, fresh(other, 1, 4 * MiB), 4 * MiB);
    CHECK(g.allocs == 3 && g.frees == 0);
    char* p = nullptr;
    size_t got = 0;
    g.oom_left = 1;
    CHECK(mine.take(0, 64 * MiB, &p, &got) == 0 && p && got == 64 * MiB);
    CHECK(g.allocs == 5 && g.releases == 1 && g.frees == 3 && mine.parked_count() == 0 && other.parked_count() == 0);
    for (const auto& f : g.freed) CHECK(f.second == 1);
    mine.park(0, p, 64 * MiB);
    g.oom_left = 2;                                 // still none after the release: the answer goes to the caller, no third attempt
    CHECK(mine.take(0, 65 * MiB, &p, &got) == kOom && p == nullptr);
    CHECK(g.allocs == 7 && g.releases == 2 && g.frees == 4 && g.live.empty());
    // the same for an object's block
    Block b;
    g.oom_left = 1;
    CHECK(b.take(mine, 0, MiB) == 0 && b && g.allocs == 9 && g.releases == 3);
    g.oom_left = 2;
    Block none;
    CHECK(none.take(mine, 0, MiB) == kOom && !none && none.get() == nullptr && none.bytes() == 0 && g.allocs == 11);
    b.release(false);
    CHECK(g.live.empty());
    g.pools[0] = g.pools[1] = nullptr;
}

void blocks(const Policy& policy) {
    Pool pool(policy, kFake);
    g = Fake();
    {
        Block b;
        CHECK(!b && b.bytes() == 0);
        b.release(true);
        b.release(false);
        CHECK(g.frees == 0);
        // released when the device is idle: parked; a second release frees nothing and parks nothing
        CHECK(b.take(pool, 0, 8 * MiB) == 0 && b && b.bytes() == 8 * MiB);
        char* const first = b.get();
        b.release(true);
        CHECK(!b && b.get() == nullptr && g.frees == 0 && pool.parked_count() == 1);
        b.release(true);
        b.release(false);
        CHECK(g.frees == 0 && pool.parked_count() == 1);
        // the parked block comes back, with the bytes it has; released when the device is not idle: freed, once
        CHECK(b.take(pool, 0, 6 * MiB) == 0 && b.get() == first && b.bytes() == 8 * MiB && g.allocs == 1);
        b.release(false);
        b.release(false);
        b.release(true);
        CHECK(g.frees == 1 && g.freed[first] == 1 && pool.parked_count() == 0);
        // a moved-from block holds nothing
        CHECK(b.take(pool, 0, 8 * MiB) == 0);
        char* const second = b.get();
        Block c(std::move(b));
        CHECK(!b && c.get() == second && c.bytes() == 8 * MiB);
        b.release(false);
        b.release(true);
        CHECK(g.frees == 1 && pool.parked_count() == 0);
        // fit: kept while large enough, else given back (the device is idle: parked) and another taken
        CHECK(c.fit(pool, 0, 5 * MiB) == 0 && c.get() == second && g.allocs == 2);
        CHECK(c.fit(pool, 0, 8 * MiB) == 0 && c.get() == second && g.allocs == 2);
        CHECK(c.fit(pool, 0, 9 * MiB) == 0 && c.get() != second && c.bytes() == 9 * MiB && g.allocs == 3 && g.frees == 1 && pool.parked_count() == 1);
        Block e;
        CHECK(e.fit(pool, 0, 7 * MiB) == 0 && e.get() == second && g.allocs == 3 && pool.parked_count() == 0);
        // move assignment frees what the target held, once, and empties the source
        char* const third = c.get();
        c = std::move(e);
        CHECK(g.frees == 2 && g.freed[third] == 1 && c.get() == second && !e);
        // a plain allocation is never parked
        Block plain;
        CHECK(plain.allocate(kFake, 0, 3 * MiB) == 0 && plain.bytes() == 3 * MiB && g.allocs == 4);
        char* const fourth = plain.get();
        plain.release(true);
        plain.release(true);
        CHECK(g.frees == 3 && g.freed[fourth] == 1 && pool.parked_count() == 0);
        // c still holds `second` here and goes out of scope holding it: freed by its destructor, b / e / plain free nothing
    }
    CHECK(g.frees == 4 && g.live.empty());
    for (const auto& f : g.freed) CHECK(f.second == 1);
}

void carved() {
    // the formula every caller used to write out: each piece rounded up to 256 bytes, 256 bytes of slack behind it
    const size_t sizes[12] = {0, 1, 255, 256, 257, 0, 0, 4096, 12345, 16 * 1000003, 8, 0};
    const auto cut = carve(sizes);
    size_t total = 0;
    for (int i = 0; i < 12; ++i) {
        CHECK(cut.off[i] == total && cut.off[i] % 256 == 0);
        total += (sizes[i] + 255) / 256 * 256 + 256;
    }
    CHECK(cut.total == total);
    CHECK(cut.off[1] == 256 && cut.off[2] == 768 && cut.off[3] == 1280 && cut.off[4] == 1792 && cut.off[5] == 2560 && cut.off[6] == 2816 && cut.off[7] == 3072);
    CHECK(carve_span(0) == 256 && carve_span(1) == 512 && carve_span(256) == 512 && carve_span(257) == 768);
    char* const base = reinterpret_cast<char*>((size_t)1 << 20);
    CHECK(reinterpret_cast<char*>(cut.at<double>(base, 8)) == base + cut.off[8]);
    const size_t one[1] = {0};
    CHECK(carve(one).total == 256 && carve(one).off[0] == 0);
}

}  // namespace

int main() {
    leaf_policy();
    ctx_policy();
    for (const Policy* policy : {&kLeafPolicy, &kCtxPolicy}) {
        out_of_memory(policy);
        blocks(*policy);
    }
    carved();
    std::printf("ok\n");
    return 0;
}
