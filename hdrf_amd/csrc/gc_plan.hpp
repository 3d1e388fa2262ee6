// gc_plan.hpp — the host arithmetic of the index garbage collection (hdrf_gc, api_gc.hip; kernels in
// gc.hip).  No HIP in here: tests/cpp/gc_plan_test.cpp compiles it with g++ and checks it against a
// per-digest model.
//
// The mark pass runs one lane per recipe digest over ALL live recipes laid end to end: recipe j owns
// the flat positions [first_j, first_j + n_j).  The host builds one job per recipe (the device address
// of its digests and first_j) plus a sentinel whose `first` is the total; a lane finds its recipe by
// binary search over `first` and its digest at dig + (i - first_j) * digest bytes.  Empty recipes get
// no job (they own no position).
#pragma once
#include <stdint.h>

#include <vector>

#include "table_walk.hpp"

#ifdef __HIPCC__
#define HDRF_GC_HD __host__ __device__   // gc_mark_kernel finds its recipe with the host's function
#else
#define HDRF_GC_HD
#endif

namespace hdrf {

constexpr uint32_t kGcTile = 256;            // lanes per workgroup of the mark / sweep launches
constexpr uint32_t kGcMaxGrid = 1u << 16;    // workgroups at most: the kernels stride over the rest

struct GcJob {
    uint64_t dig;        // device address of the recipe's digests (4-B aligned)
    uint64_t first;      // flat position of its first digest; the sentinel's is the total
};
static_assert(sizeof(GcJob) == 16, "GcJob is one 16-B load");

// The job list of a collection: add() every live recipe, then finish().
struct GcPlan {
    std::vector<GcJob> jobs;     // after finish(): njobs() jobs + the sentinel
    uint64_t total = 0;          // digests of all recipes
    uint64_t recipes = 0;        // recipes added, the empty ones included
    void add(uint64_t dig, uint32_t n)
    {
        recipes++;
        if (!n) return;
        jobs.push_back(GcJob{dig, total});
        total += n;
    }
    void finish() { jobs.push_back(GcJob{0, total}); }
    uint32_t njobs() const { return (uint32_t)jobs.size() - 1; }
};

// The job that owns flat position i < total: the last j < nj with jobs[j].first <= i (jobs[nj] is the
// sentinel).  nj >= 1.
HDRF_GC_HD inline uint32_t gc_find_job(const GcJob *jobs, uint32_t nj, uint64_t i)
{
    uint32_t lo = 0, hi = nj;                // invariant: jobs[lo].first <= i < jobs[hi].first
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (jobs[mid].first <= i) lo = mid; else hi = mid;
    }
    return lo;
}

// Workgroups of a launch of one lane per item over `items` items (0 items: no launch).
inline uint32_t gc_grid(uint64_t items)
{
    const uint64_t g = (items + kGcTile - 1) / kGcTile;
    return (uint32_t)(g < kGcMaxGrid ? g : kGcMaxGrid);
}

// Survivor rows the sweep may need: a kept entry is a marked table slot, one per distinct live digest
// at most, so neither the recipe digests nor the table's slots can be exceeded.
inline uint64_t gc_row_cap(uint64_t recipe_digests, uint64_t table_slots)
{
    return recipe_digests < table_slots ? recipe_digests : table_slots;
}

inline uint64_t gc_up256(uint64_t x) { return (x + 255) & ~255ull; }

// Where the pieces of one call live in the scratch (ctx->d_rd), each on a 256-B boundary:
// [jobs | container ids] are uploaded, the rest is cleared or written on the device.
struct GcLayout {
    uint64_t o_cnt, o_wg, o_jobs, o_cid, o_ccnt, o_seen, o_mark, o_dw, o_val, total;
};
constexpr uint64_t kGcCidBits = 1ull << 24;      // container ids are 3 bytes of the 11-byte value
inline GcLayout gc_layout(uint64_t njobs, uint64_t ncont, uint64_t table_slots, uint64_t rows, uint32_t hw,
                          uint32_t ccnt_bytes)
{
    GcLayout L;
    L.o_cnt = 0;
    L.o_wg = 256;                                // marked slots per sweep workgroup
    L.o_jobs = L.o_wg + gc_up256(kWalkMaxWgs * 4);
    L.o_cid = gc_up256(L.o_jobs + (njobs + 1) * sizeof(GcJob));
    L.o_ccnt = gc_up256(L.o_cid + ncont * 4);
    L.o_seen = gc_up256(L.o_ccnt + ncont * ccnt_bytes);
    L.o_mark = gc_up256(L.o_seen + kGcCidBits / 8);
    L.o_dw = gc_up256(L.o_mark + (table_slots + 31) / 32 * 4);
    L.o_val = gc_up256(L.o_dw + rows * hw * 4);
    L.total = gc_up256(L.o_val + rows * 11) + 256;
    return L;
}

}  // namespace hdrf
