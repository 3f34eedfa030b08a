// record_locks.h -- the lock order of every call on several records, and the size of an id table.  Standard C++ only: a stand-alone host program can include it
// (tests/host/record_locks_main.cpp).
#pragma once
#include <cstddef>
#include <functional>
#include <mutex>
#include <utility>

// One call's locks, taken in the one order every call uses: the owner (the covisibility graph, the keyframe-insertion handle), the keyframe store or stores with
// the lower address first, then the map.  Any of them may be null; the two stores may be one, which is then locked once.  The workspace lane is taken after these.
// Released on scope exit.
struct RecordLocks {
    std::unique_lock<std::mutex> lk_owner, lk_lo, lk_hi, lk_map;
    void take(std::mutex* owner, std::mutex* store_a, std::mutex* store_b, std::mutex* map)
    {
        std::mutex* lo = store_a ? store_a : store_b; std::mutex* hi = (store_a && store_b && store_b != store_a) ? store_b : nullptr;
        if (hi && std::less<std::mutex*>()(hi, lo)) std::swap(lo, hi);
        if (owner) lk_owner = std::unique_lock<std::mutex>(*owner);
        if (lo) lk_lo = std::unique_lock<std::mutex>(*lo);
        if (hi) lk_hi = std::unique_lock<std::mutex>(*hi);
        if (map) lk_map = std::unique_lock<std::mutex>(*map);
    }
};

// id -> value hash table of `entries` ids: the smallest power of two that is >= 64 and leaves the table at most half full
inline size_t id_table_capacity(long long entries)
{
    size_t cap = 64;
    while (cap < 2 * (size_t)(entries > 0 ? entries : 1)) cap <<= 1;
    return cap;
}
