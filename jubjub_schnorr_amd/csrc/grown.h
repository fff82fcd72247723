// The capacity a grow-only buffer takes (device_owners.h grow_only, msig_scratch.h).  Plain C++.
#pragma once
#include <cstddef>

namespace jjs {

inline size_t grown(size_t want) {       // the smallest of 2^k, 1.5 * 2^k that holds `want`: what is retired stays below what is live
    size_t cap = 4096;
    while (cap < want) cap <<= 1;
    const size_t mid = cap / 4 * 3;
    return mid >= want ? mid : cap;
}

}  // namespace jjs
