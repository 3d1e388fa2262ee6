// The host arithmetic of the online table resize (hdrf_amd/csrc/resize_plan.hpp), as a plain program
// (tests/test_index_resize.py compiles this with -fsanitize=address,undefined and runs it):
//   args     new_log2 9 and 32 are refused, 10 and 31 accepted, the current size is a no-op
//   load     the 75 % line at its edge: 768 entries fit 1024 slots, 769 do not; growing never trips it
//   homes    for 10^5 pseudo-random tags, every k in [10, 30] and d in {1, 2, 5}:
//            tag_home(t, k + d) >> d == tag_home(t, k), with index_entry.hpp's own tag_home — the
//            property the rehash kernel's locality rests on; and, from it, that homes stay in order
//   grid     one workgroup per tile up to 4 per CU, never more than the walk's bound
//   bytes    what the speed script divides by
#include <cstdio>

#include "../../hdrf_amd/csrc/index_entry.hpp"
#include "../../hdrf_amd/csrc/resize_plan.hpp"

using namespace hdrf;

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
            return 1;                                             \
        }                                                         \
    } while (0)

static uint64_t splitmix(uint64_t &s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

int main()
{
    // args
    CHECK(!resize_log2_ok(9) && resize_log2_ok(10) && resize_log2_ok(31) && !resize_log2_ok(32));
    CHECK(!resize_log2_ok(-1) && !resize_log2_ok(0) && !resize_log2_ok(64));
    CHECK(resize_check_args(10, 9) == kResizeBadLog2 && resize_check_args(31, 32) == kResizeBadLog2);
    CHECK(resize_check_args(10, 10) == kResizeSame && resize_check_args(31, 31) == kResizeSame);
    CHECK(resize_check_args(10, 11) == kResizeGo && resize_check_args(14, 10) == kResizeGo);
    CHECK(resize_check(14, 9, 0) == kResizeBadLog2 && resize_check(14, 32, 0) == kResizeBadLog2);
    CHECK(resize_check(10, 10, 1024) == kResizeSame);             // (a full table of the same size: still a no-op)
    // load: 3/4 of the new table's slots
    CHECK(resize_load_ok(768, 10) && !resize_load_ok(769, 10));
    CHECK(resize_check(14, 10, 768) == kResizeGo && resize_check(14, 10, 769) == kResizeTooFull);
    CHECK(resize_check(14, 10, 0) == kResizeGo);
    for (int k = kIndexMinLog2; k <= kIndexMaxLog2; k++) {
        const uint64_t slots = 1ull << k;
        CHECK(resize_load_ok(slots / 4 * 3, k) && !resize_load_ok(slots / 4 * 3 + 1, k));
        if (k < kIndexMaxLog2) CHECK(resize_check(k, k + 1, slots) == kResizeGo);      // a FULL table still grows
        if (k > kIndexMinLog2) CHECK(resize_check(k, k - 1, slots / 2) == kResizeTooFull);
    }
    CHECK(resize_load_ok(1ull << 31, 31) == false && resize_load_ok(3ull << 29, 31));
    // homes: growing by d bits refines a home, never reorders two
    uint64_t s = 20261021;
    const int ds[3] = {1, 2, 5};
    unsigned long long prev = 0;
    for (int i = 0; i < 100000; i++) {
        unsigned long long t = splitmix(s);
        if (i % 1000 == 0) t = i % 2000 ? ~0ull : 0ull;            // the extremes too
        if (i % 7 == 3) t |= 0xA5ull << 56;                        // an epoch in the top byte: no part of the home
        for (int k = 10; k <= 30; k++)
            for (int d : ds) {
                CHECK((tag_home(t, k + d) >> d) == tag_home(t, k));
                CHECK(tag_home(t, k) < (1ull << k));
                CHECK(tag_home(t & kTag56, k) == tag_home(t, k));
                if (i && tag_home(prev, k) < tag_home(t, k)) CHECK(tag_home(prev, k + d) < tag_home(t, k + d));
                if (i && tag_home(prev, k + d) <= tag_home(t, k + d)) CHECK(tag_home(prev, k) <= tag_home(t, k));
            }
        prev = t;
    }
    // grid: 4 workgroups per CU over the walked table, one tile each at least
    CHECK(resize_grid(10, 256) == 4);                              // 1024 slots: 4 tiles
    CHECK(resize_grid(18, 256) == 1024 && resize_grid(19, 256) == 1024 && resize_grid(31, 256) == 1024);
    CHECK(resize_grid(19, 256) * 2 == (1u << 19) / 256);           // 2^19: the smallest table with a second tile per workgroup
    CHECK(resize_grid(31, 100000) == kWalkMaxWgs && resize_grid(10, 0) == 1);
    // bytes
    const ResizeBytes b = resize_bytes(24, 25, 10000000);
    CHECK(b.count_old == (1ull << 30) && b.rehash_read == (1ull << 30) && b.clear == (2ull << 30) && b.count_new == (2ull << 30));
    CHECK(b.rehash_write == 640000000ull && b.rehash_cas == 80000000ull && b.rehash() == (1ull << 30) + 640000000ull);
    CHECK(kResizeCntOld % 256 == 0 && kResizeCntNew >= kResizeCntOld + 256 && kResizeErr >= kResizeCntNew + 256 &&
          kResizeScratch >= kResizeErr + 4);
    std::printf("PASS\n");
    return 0;
}
