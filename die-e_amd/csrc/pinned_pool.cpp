// pinned_pool.cpp -- pinned host memory for the delivered fragments.
// The arrays of a diee_fragments are page-locked so that the copies out of HBM are real asynchronous DMA (pageable
// destinations are staged by the runtime and block the host).  Pinning costs ~0.3 ms per MB, so blocks are kept when
// diee_free_fragments hands them back (up to option pinned_pool_mb, default 8192 MiB) and the next call takes them again.
#include "pinned_pool.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <unordered_map>
#include <vector>

namespace diee {

namespace {
struct PinnedPool {
    std::mutex m;
    std::multimap<size_t, void*> idle;                 // size -> block
    std::unordered_map<void*, size_t> out;             // blocks handed out
    size_t idle_bytes = 0;
    // process-wide: option pinned_pool_mb of any ctx (the environment's DIEE_PINNED_POOL_MB through it, read when a ctx is created)
    size_t cap = (size_t)8192 << 20;
    size_t cap_bytes() { std::lock_guard<std::mutex> lk(m); return cap; }
    void* acquire(size_t bytes) {
        bytes = (std::max<size_t>(bytes, 1) + 0xFFFFFull) & ~(size_t)0xFFFFFull;      // 1 MiB granules
        {
            std::lock_guard<std::mutex> lk(m);
            auto it = idle.lower_bound(bytes);
            if (it != idle.end() && it->first <= 2 * bytes + (64u << 20)) {
                void* p = it->second; const size_t sz = it->first;
                idle.erase(it); idle_bytes -= sz; out[p] = sz;
                return p;
            }
        }
        void* p = nullptr;
        if (hipHostMalloc(&p, bytes) != hipSuccess || !p) { (void)hipGetLastError(); return nullptr; }
        std::lock_guard<std::mutex> lk(m);
        out[p] = bytes;
        return p;
    }
    bool release(void* p) {                              // false: not one of ours
        if (!p) return true;
        size_t sz;
        {
            std::lock_guard<std::mutex> lk(m);
            auto it = out.find(p);
            if (it == out.end()) return false;
            sz = it->second; out.erase(it);
            if (idle_bytes + sz <= cap) { idle.emplace(sz, p); idle_bytes += sz; return true; }
        }
        (void)hipHostFree(p);
        return true;
    }
};
PinnedPool& pinned_pool() { static PinnedPool* pool = new PinnedPool(); return *pool; }   // (never destroyed: the HIP runtime may be gone first)
void give(void* q) { if (q && !pinned_pool().release(q)) free(q); }      // (a block of the pool, or the malloc fallback)
}  // namespace

bool pinned_release(void* p) { return pinned_pool().release(p); }
void pinned_pool_set_cap_mb(size_t mb) {
    PinnedPool& P = pinned_pool();
    std::vector<void*> drop;
    {
        std::lock_guard<std::mutex> lk(P.m);
        P.cap = mb << 20;
        while (P.idle_bytes > P.cap && !P.idle.empty()) {       // a lower cap gives idle blocks back at once, largest first
            auto it = std::prev(P.idle.end());
            drop.push_back(it->second); P.idle_bytes -= it->first; P.idle.erase(it);
        }
    }
    for (void* p : drop) (void)hipHostFree(p);
}
size_t pinned_pool_cap_mb() { return pinned_pool().cap_bytes() >> 20; }

void FragBufs::reserve(size_t rows) {
    if (rows <= cap) return;
    PinnedPool& P = pinned_pool();
    const size_t nc = std::max(rows, cap + cap / 2);
    // page-locked where the runtime grants it; a host that refuses to pin more (8 ranks x several GB each) gets pageable memory
    // instead -- the copies into it are staged by the runtime and block the host thread, the records are the same
    auto get = [&](size_t bytes) { void* q = P.acquire(bytes); return q ? q : malloc(std::max<size_t>(bytes, 1)); };
    int8_t* o = (int8_t*)get(nc); float* p = (float*)get(nc * 1352 * sizeof(float));
    float* st = (float*)get(nc * 144 * sizeof(float)); uint32_t* g = (uint32_t*)get(nc * sizeof(uint32_t));
    if (!o || !p || !st || !g) { give(o); give(p); give(st); give(g); throw std::bad_alloc(); }
    if (n) { memcpy(o, outcome, n); memcpy(p, ps, n * 1352 * sizeof(float)); memcpy(st, state, n * 144 * sizeof(float)); memcpy(g, game, n * sizeof(uint32_t)); }
    drop();
    outcome = o; ps = p; state = st; game = g; cap = nc;
}
void FragBufs::drop() { give(outcome); give(ps); give(state); give(game); outcome = nullptr; ps = nullptr; state = nullptr; game = nullptr; }
void FragBufs::release(diee_fragments* f) { f->n = (uint32_t)n; f->outcome = outcome; f->ps = ps; f->state = state; f->game = game; outcome = nullptr; ps = nullptr; state = nullptr; game = nullptr; cap = n = 0; }

}  // namespace diee
