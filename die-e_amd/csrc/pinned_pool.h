// pinned_pool.h -- page-locked host memory for the delivered fragments (pinned_pool.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/diee.h"

namespace diee {

bool pinned_release(void* p);             // back to the pool of page-locked blocks; false = not one of its blocks
void pinned_pool_set_cap_mb(size_t mb);   // option pinned_pool_mb (process-wide)
size_t pinned_pool_cap_mb();

struct FragBufs {          // host arrays of one diee_fragments until they are handed over: pinned, grown on demand
    int8_t* outcome = nullptr; float* ps = nullptr; float* state = nullptr; uint32_t* game = nullptr;
    size_t cap = 0, n = 0;                                     // rows
    FragBufs() = default;
    FragBufs(const FragBufs&) = delete;
    FragBufs& operator=(const FragBufs&) = delete;
    ~FragBufs() { drop(); }
    // room for `rows` rows, the first n kept.  The caller has drained the copy stream if n > 0 (copies into the old blocks).
    void reserve(size_t rows);
    void release(diee_fragments* f);
private:
    void drop();
};

}  // namespace diee
