// resize_plan.hpp — the host arithmetic of the online table resize (hdrf_index_resize, api_resize.hip;
// kernel in resize.hip).  No HIP in here: tests/cpp/resize_plan_test.cpp compiles it with g++ and checks
// the argument and load rule at their edges, and the property the kernel's locality rests on.
//
// tag_home (index_entry.hpp) takes the TOP log2cap bits of a multiplicative hash, so for every tag t
//     tag_home(t, k + d) >> d == tag_home(t, k)        (growing by d bits)
// and an entry whose home is slot h of a 2^k table has its home among the 2^d slots [h << d, (h + 1) << d)
// of a 2^(k+d) table — or, shrinking, at slot h >> d.  The mapping from old home to new home is
// monotone: a workgroup that walks one 256-slot tile of the old table writes into one contiguous
// region of the new one (plus what linear probing carried past a tile's end, in either table).
#pragma once
#include <stdint.h>

#include "table_walk.hpp"

namespace hdrf {

constexpr int kIndexMinLog2 = 10, kIndexMaxLog2 = 31;     // hdrf_open's bounds on cfg.index_log2

// What hdrf_index_resize answers before it allocates anything.
enum ResizeCheck {
    kResizeGo = 0,        // move the table
    kResizeSame = 1,      // new_log2 is the current size: nothing to do
    kResizeBadLog2 = 2,   // new_log2 outside [kIndexMinLog2, kIndexMaxLog2]
    kResizeTooFull = 3,   // the live entries would load the new table past 75 %
};

inline bool resize_log2_ok(int new_log2) { return new_log2 >= kIndexMinLog2 && new_log2 <= kIndexMaxLog2; }

// The load rule, a stated condition of the interface: at most 3/4 of the new table's slots.
// (entries <= 2^31 live slots of the old table: no overflow.)
inline bool resize_load_ok(uint64_t entries, int new_log2) { return entries * 4 <= 3 * (1ull << new_log2); }

// The argument check (before the count) ...
inline ResizeCheck resize_check_args(int cur_log2, int new_log2)
{
    if (!resize_log2_ok(new_log2)) return kResizeBadLog2;
    return new_log2 == cur_log2 ? kResizeSame : kResizeGo;
}
// ... and the whole decision once the live entries are known.
inline ResizeCheck resize_check(int cur_log2, int new_log2, uint64_t entries)
{
    const ResizeCheck a = resize_check_args(cur_log2, new_log2);
    if (a != kResizeGo) return a;
    return resize_load_ok(entries, new_log2) ? kResizeGo : kResizeTooFull;
}

// Workgroups of the rehash walk over the OLD table (and of the two counts, each over its own table):
// four per CU, one 256-slot tile each at least.
inline uint32_t resize_grid(int log2cap, int n_cu) { return walk_grid(log2cap, 4 * n_cu); }

// The device scratch of one call (ctx->d_rd): the counters of the two counts, then the rehash's error word.
constexpr uint64_t kResizeCntOld = 0, kResizeCntNew = 256, kResizeErr = 512, kResizeScratch = 768;

// Bytes each pass must move, for the speed script's rates (scripts/index_resize_speed.py).  The rehash
// reads the old table once and writes 64 B per live entry; its claims are one 8-B compare-and-swap per
// live entry on top (more where probes collide), reported apart because they are not streamed.
struct ResizeBytes {
    uint64_t count_old, clear, rehash_read, rehash_write, rehash_cas, count_new;
    uint64_t rehash() const { return rehash_read + rehash_write; }
};
inline ResizeBytes resize_bytes(int old_log2, int new_log2, uint64_t entries)
{
    ResizeBytes b;
    b.count_old = 64ull << old_log2;
    b.clear = 64ull << new_log2;
    b.rehash_read = 64ull << old_log2;
    b.rehash_write = entries * 64;
    b.rehash_cas = entries * 8;
    b.count_new = 64ull << new_log2;
    return b;
}

}  // namespace hdrf
