// table_walk.hpp — the streaming pass over the whole index table that gc_sweep (gc.hip), cp_collect
// (compact.hip) and ix_rehash (resize.hip) share: persistent workgroups of 256 lanes, workgroup x takes the 256-slot tiles x,
// x + gridDim.x, ... of the table, one lane per 64-B entry.  A pass that appends rows runs after a
// counting pass with the same grid, which leaves in wg[x] the rows workgroup x will write: every
// workgroup then appends from a row base of its own through an LDS counter (one
// returning global atomic per wave on ONE counter held the sweep at the rate of that word).
//
// The grid's bound and its clamp are host arithmetic with no HIP in them (gc_plan.hpp and
// compact_plan.hpp size wg[] by the bound, and their tests are built with g++); the device part
// needs hipcc.
#pragma once
#include <stdint.h>

namespace hdrf {

constexpr uint32_t kWalkMaxWgs = 2048;       // persistent walk workgroups at most (one row-base word each)

// workgroups of a walk over 2^log2cap slots (log2cap >= 8: whole tiles only) when the caller asks for wgs
inline uint32_t walk_grid(int log2cap, int wgs)
{
    const uint64_t tiles = (1ull << log2cap) / 256;
    const uint64_t want = wgs < 1 ? 1 : (uint64_t)wgs < kWalkMaxWgs ? (uint64_t)wgs : kWalkMaxWgs;
    return (uint32_t)(want < tiles ? want : tiles);
}

}  // namespace hdrf

#ifdef __HIPCC__
#include "common.hpp"

namespace hdrf {

// This wave's share of the rows of the workgroups before this one (every lane holds it): the shares
// of a workgroup's four waves add up to its row base.  wg: the counting pass's output for this grid.
__device__ __forceinline__ uint32_t wg_row_base(const uint32_t *wg)
{
    unsigned long long before = 0;
    for (uint32_t y = threadIdx.x; y < blockIdx.x; y += 256u) before += wg[y];
    return (uint32_t)wave_sum_u64(before);
}

// The walk.  A wave reads its 64 entries of a tile as four fully coalesced 16-B loads per lane and
// turns them lane-major through LDS (16 KiB per workgroup); the next tile's loads are in flight while
// this one is classified.  body(slot, p0, p1, p2, p3): the lane's entry, as the four 16-B quarters of
// its 64 bytes (p0 = tag | mask, p1 = first | batch | ncopy, p2 = cid | start | stop | dig[0], p3 =
// dig[1..4]), once per tile.  Every lane of the workgroup calls it, in uniform control flow; body may
// not hold a barrier.
template <class F>
__device__ __forceinline__ void table_walk(const IndexEntry *tab, uint64_t nslots, F body)
{
    __shared__ uint4 s_e[4][256];                              // per wave: its 64 entries, 4 KiB
    const int t = (int)threadIdx.x, w = wave_id(), l = lane_id();
    const uint64_t tstride = (uint64_t)gridDim.x * 256u;
    // lane l's four 16-B pieces of the wave's 64 entries of a tile: piece k is bytes [(k * 64 + l) * 16, +16)
    auto fetch = [&](uint64_t tile, uint4 r[4]) {
        const uint8_t *wb = (const uint8_t *)(tab + tile + (uint64_t)w * 64);
#pragma unroll
        for (int k = 0; k < 4; k++) r[k] = ld16_nt(wb + (size_t)(k * 64 + l) * 16);
    };
    uint4 r[4] = {};
    if ((uint64_t)blockIdx.x * 256u < nslots) fetch((uint64_t)blockIdx.x * 256u, r);
    for (uint64_t tile = (uint64_t)blockIdx.x * 256u; tile < nslots; tile += tstride) {   // uniform
#pragma unroll
        for (int k = 0; k < 4; k++) s_e[w][k * 64 + l] = r[k];
        __syncthreads();
        const uint4 p0 = s_e[w][l * 4], p1 = s_e[w][l * 4 + 1], p2 = s_e[w][l * 4 + 2], p3 = s_e[w][l * 4 + 3];
        __syncthreads();                                       // (the next tile's stores come after every read)
        if (tile + tstride < nslots) fetch(tile + tstride, r); // in flight while this tile is classified
        body(tile + (uint64_t)t, p0, p1, p2, p3);
    }
}

}  // namespace hdrf
#endif
