// host_block.hpp -- the arrays of a host-pointer batched call (pnol_run_*_batch, capi.cpp) and
// their places in the one device block the call allocates.  Plain C++, no HIP: the layout is
// checked on its own by tests/cpp/host_block_check.cpp.
#pragma once

#include <cstddef>

namespace pnol {

enum : int { kHostIn = 1, kHostOut = 2 };   // copied to the device before the launch / back after it

struct HostArray {
    void* host;     // null: an optional array the caller left out (no room, no copy, null on the device)
    size_t count;   // items
    size_t elem;    // bytes per item: 8 (double, long long) or 4 (int)
    int dir;        // kHostIn | kHostOut
    size_t bytes() const { return host ? count * elem : 0; }
};

// off[i] = byte offset of array i in the block, the 8-byte items first (each in list order) so
// that every one of them is 8-byte aligned whatever the counts; returns the block's size
inline size_t host_block_carve(const HostArray* a, size_t na, size_t* off) {
    size_t total = 0;
    for (int wide = 1; wide >= 0; --wide)
        for (size_t i = 0; i < na; ++i)
            if ((a[i].elem % 8 == 0) == (wide == 1)) {
                off[i] = total;
                total += a[i].bytes();
            }
    return total;
}

}  // namespace pnol
