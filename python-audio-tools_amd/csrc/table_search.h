// table_search.h — the one sorted-table lookup of the device code: "which
// track / stream / page owns unit x" over a table of first indices.
#pragma once
#include <hip/hip_runtime.h>

// Index of the last row of t[0, n) whose key is <= x.  Keys ascend, n >= 1
// (row 0 is the answer when every key is above x).  `key` is a member
// pointer (&Row::start); the index type follows n.
template <typename Row, typename K, typename N, typename X>
__device__ __forceinline__ N last_le(const Row *t, N n, X x, K Row::*key)
{
    N lo = 0, hi = n;
    while (hi - lo > 1) {
        const N mid = lo + ((hi - lo) >> 1);
        if (t[mid].*key <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
