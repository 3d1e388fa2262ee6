// common.hpp — shared device helpers and on-device layouts for libhdrf (gfx950 only).
//
// Data layout in HBM (one batch of up to 64 blocks):
//   block bytes          caller's device buffers (16-B aligned), `readable` bytes each
//   spec lists           [block][segment][SPEC_CAP] u32 cut offsets from the speculative walk
//   offsets              [block][cap_blk] u32 chunk END offsets (reference chunking() output)
//   digests              [block][cap_blk][H] bytes
//   chunk meta           [block][cap_blk] slot / flags / prefix
//   index table          2^k entries x 64 B, open addressing keyed by the first 8 digest bytes (index_entry.hpp)
//   container arena      slots x container_max bytes (raw containers, DataDeduplicator.maxSize)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "index_entry.hpp"

namespace hdrf {

#define HDRF_GLOBAL_FWD __attribute__((address_space(1)))
constexpr int kWave = 64;
constexpr int kMaxBatch = 64;        // one bit per block of the batch in IndexEntry::mask
// Lane walker (chunk.hip): one lane walks one speculative segment of seg_len bytes; a wave holds
// kWaveSegs segments plus a helper lane that walks the next wave's first segment.
constexpr int kWaveSegs = 63;
constexpr int kLaneOver = 8;         // overrun cuts a lane may record past its segment end
constexpr int kLdsCuts = 30;         // LDS list of every lane (u16 offsets from its segment start)
constexpr int kRepairCuts = 4096;    // a repair walk gives up after this many cuts ...
constexpr int kRepairBytes = 2 << 20;  // ... or this many bytes past its start
constexpr int kRqKeep = 16384;       // repair-queue entries whose cuts the count pass keeps (64 words each)
constexpr int kSegMinWin = 4;        // seg_len bounds, in units of window + 2 (702 B)
constexpr int kSegMaxWin = 20;        // seg_len / 702 + 2 + kLaneOver <= kLdsCuts

// (IndexEntry, its tag words and its digest / value codec: index_entry.hpp, shared with the host)
// nCopy (bits 0..7 of ncopy) without touching the SHA-224 digest byte above it
__device__ __forceinline__ void set_ncopy(IndexEntry *e, uint32_t n)
{
    *(HDRF_GLOBAL_FWD uint8_t *)&e->ncopy = (uint8_t)n;
}

// Per-batch block descriptor (device side).
struct BlockDesc {
    const uint8_t *data;
    uint64_t len;
    uint64_t readable;       // bytes readable from data (>= len)
    int32_t nseg;            // speculative lane segments [k*seg_len, min((k+1)*seg_len, len))
    int32_t seg_len;         // multiple of 702 (window + 2) so all-zero data syncs at once
    int32_t seg0;            // the block's first segment in the batch's flat spec / meta arrays
    int32_t wave0;           // the block's first lane-walker wave
};

// Speculative segment walk result (one per lane segment).
constexpr int kSyncEnd = -1;         // the chain ran to the block end without meeting the next one
constexpr int kSyncFail = -2;        // no shared cut within the overrun caps (no repair record)
constexpr int kSyncJump = -3;        // repaired: the chain continued and met segment k + jmp at its cut jj
constexpr int kSyncGiveUp = -4;      // repair found no shared cut within kRepairCuts / kRepairBytes
struct SegMeta {
    int32_t n_main;          // cuts < next segment start
    int32_t n_over;          // cuts >= next segment start (<= kLaneOver)
    int32_t sync;            // i | j << 16: overrun cut i == the next segment's cut j; or a kSync* status
    int32_t jmp;             // kSyncJump: target segment - this segment
    int32_t jj;              // kSyncJump: index of the shared cut in the target's list
    int32_t n_ext;           // kSyncJump: cuts of the repair walk, the shared cut included
    int32_t ext_dst;         // the repair's cuts go to offsets[ext_dst..] (-1: not on the block's path)
    int32_t cp_from;         // stitch plan: copy list[cp_from, cp_from + cp_n) to the block's offsets
    int32_t cp_n;
    int32_t cp_dst;          // unused
    int32_t pad[3];          // stitch scratch: piece size, repair-cut position in the piece; [2] unused (zero)
};

// Stitch path of one block (stitch_path_kernel): on-path jumps, the terminal segment, fallback flag.
struct PathInfo {
    int32_t nj, term, fb, pad;
};

// Per-block state after chunking/stitching.
struct BlockState {
    int32_t n_cuts;          // true boundaries before the drop-last rule (stitched + fallback)
    int32_t fail_dst;        // fallback writes from here (-1 = none); it starts at offsets[fail_dst - 1]
                             // (or at the block start, first-chunk rule, when fail_dst == 0)
    uint32_t fail_p0;        // unused (kept for the layout)
    int32_t n_chunks;        // final chunk count (offsets list length)
};

// Container stream state per storer range t (lastBlockID[t], file length, lastBlockID[t+4]).
struct AllocState {
    uint32_t id[4];
    uint32_t cur[4];         // open container length (file length)
    uint32_t pos[4];         // lastBlockID[t+4] (bufferBB.position() of the last storing block)
    uint32_t slot[4];        // arena slot of the open container
    uint32_t next_slot;
    uint32_t nclosed;        // containers closed so far (total)
    uint32_t exists[4];      // open container file exists
    uint32_t pad;
};

// Flush event inside one (block, range): container closes before chunk `chunk`.
struct FlushEv {
    int32_t chunk;
    uint32_t new_id;
    uint32_t new_slot;
    uint32_t base;           // range-relative prefix (X0 of `chunk`)
};

struct RangeState {          // per (block, range t)
    uint32_t id0, slot0, cur0;   // open container at the range start
    int32_t nflush;              // flush events of this (block, range)
    int32_t ev_begin;            // first event in the range-t event list
    int32_t c_begin, c_end;      // chunk range [n*t/nT, n*(t+1)/nT)
    uint32_t base;               // block prefix of new bytes before c_begin
    uint32_t total;              // new bytes in range
    int32_t active;              // storer t runs (storeSize != 0 and t < nThread)
};

// Node-global allocator scan (gx.hip / api_gx.hip hdrf_gx_flush_fn): one range's flush walk over
// a batch as a function of the open container's fill, with the batch's active blocks of range t
// laid end to end as one stream of new bytes.
struct FnBlock {             // per (range t, block b)
    uint32_t act, c0, c1, base;   // active (storeSize != 0 and t < nT), chunk range, pre[c0 - 1]
    uint64_t off, S;              // stream offset of the block's first new byte, new bytes
    uint32_t coff, pad;           // stream index of the block's first chunk
};
struct FnRange {             // per range t
    uint64_t any, S, base_last, S_last, nstream;
};

struct ClosedRec {           // a container closed during a batch
    uint32_t id, slot, len, range;
};

// ------------------------------------------------------------------------------------------
// Global-address-space views: pointers that arrive inside structs are generic (flat) to the
// compiler; flat loads also count in lgkmcnt and force vmcnt(0)-style waits.  Casting to
// address_space(1) yields global_load_* with precise vmcnt accounting.
#define HDRF_GLOBAL __attribute__((address_space(1)))
template <class T>
__device__ __forceinline__ const HDRF_GLOBAL T *gptr(const void *p)
{
    return (const HDRF_GLOBAL T *)(p);
}

typedef uint32_t u32x4v __attribute__((ext_vector_type(4)));
// 16-B global load (dword-aligned address is enough on gfx950)
__device__ __forceinline__ uint4 ld16(const void *p)
{
    const u32x4v v = *(const HDRF_GLOBAL u32x4v *)(p);
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ uint32_t ld4(const void *p) { return *(const HDRF_GLOBAL uint32_t *)(p); }
// streaming (nontemporal) 16-B load / store: bytes read or written once, kept from displacing
// the lines other stages re-read in L2 (granule maxima, SHA pairs, index entries, LZ4 windows)
__device__ __forceinline__ uint4 ld16_nt(const void *p)
{
    const u32x4v v = __builtin_nontemporal_load((const HDRF_GLOBAL u32x4v *)(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
template <bool NT>
__device__ __forceinline__ uint4 ld16_t(const void *p) { return NT ? ld16_nt(p) : ld16(p); }

__device__ __forceinline__ int lane_id() { return __lane_id(); }
// wave index inside the workgroup, as a provably wave-uniform (scalar) value
__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

__device__ __forceinline__ uint32_t rdlane(uint32_t v, int l)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, l);
}
__device__ __forceinline__ uint32_t rdfirst(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
}

// Wave-wide unsigned max (all lanes participate; result uniform).
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
    // row_ror:1,2,4,8 -> every lane holds its 16-lane row max
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x121, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x122, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x124, 0xf, 0xf, false));
    v = max(v, (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xf, 0xf, false));
    uint32_t a = max(rdlane(v, 0), rdlane(v, 16));
    uint32_t b = max(rdlane(v, 32), rdlane(v, 48));
    return max(a, b);
}

// Inclusive wave prefix sum (u32) via shuffles.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v)
{
    const int l = lane_id();
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        uint32_t t = __shfl_up(v, d, 64);
        if (l >= d) v += t;
    }
    return v;
}

// Wave-wide u64 sum (all lanes participate; every lane holds the result).
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// One step of a 1024-thread workgroup's running exclusive scan: use(off) gets the sum of the earlier
// steps' values and of this step's v over the threads below this one, then *s_carry advances by the
// step's total.  Every thread calls it, in uniform control flow; s_w: LDS [16], *s_carry: LDS, set
// behind a barrier before the first step and holding the grand total behind the last one.  use()
// stores what the offset yields, and it runs BEFORE the two barriers that move the carry: a store
// issued behind them is still in flight when the next step waits for its load, and the single
// workgroup of rd_scan, 138 dependent steps for a 128 MiB block, then ran 17 us longer per block.
template <class F>
__device__ __forceinline__ void wg1024_excl_scan(uint32_t v, uint32_t *s_w, unsigned long long *s_carry, F use)
{
    const int t = (int)threadIdx.x;
    const uint32_t incl = wave_incl_scan(v);
    if (lane_id() == 63) s_w[t >> 6] = incl;
    __syncthreads();
    uint32_t add = 0, tot = 0;
    for (int i = 0; i < 16; i++) {
        if (i < (t >> 6)) add += s_w[i];
        tot += s_w[i];
    }
    const unsigned long long carry = *s_carry;
    use(carry + add + incl - v);
    __syncthreads();
    if (t == 0) *s_carry = carry + tot;
    __syncthreads();
}

// Searches of an ascending list given by key(i) (a lambda: the list may sit in LDS, in memory, or in
// both, as gc_sweep's id list does).  find_sorted: the index in [lo, hi) whose key is v, or -1.
template <class K>
__device__ __forceinline__ int find_sorted(int lo, int hi, uint32_t v, K key)
{
    const int end = hi;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key(mid) < v) lo = mid + 1; else hi = mid;
    }
    return lo < end && key(lo) == v ? lo : -1;
}
// the place of container `cid` in the readable container list (sorted by id), or -1
__device__ __forceinline__ int find_cid(const uint32_t *cids, int ncont, uint32_t cid)
{
    return find_sorted(0, ncont, cid, [&](int m) { return cids[m]; });
}
// the last r in [0, n) with key(r) <= v (key(0) <= v)
template <class K>
__device__ __forceinline__ uint32_t last_le(uint32_t n, uint32_t v, K key)
{
    uint32_t lo = 0, hi = n - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (key(mid) <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ unsigned long long ballot64(bool p) { return __ballot(p); }

// this lane's rank among the lanes of mask m
__device__ __forceinline__ int wave_rank(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
}

// one slot of *counter for every lane of `m` (the lanes that call with want): one atomic per wave
__device__ __forceinline__ uint32_t wave_append(uint32_t *counter, bool want)
{
    const unsigned long long m = ballot64(want);
    if (!m) return 0u;
    uint32_t base = 0;
    if (lane_id() == (int)__builtin_ctzll(m)) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, (int)__builtin_ctzll(m), 64);
    return base + (uint32_t)wave_rank(m);
}

// Reserve one slot of counter counts[d] for every lane that wants one (256 threads; every thread of
// the workgroup calls it, in uniform control flow): the lanes count in LDS, then one global atomic
// per (workgroup, counter) takes the workgroup's slots (d < G <= 64; s_cnt / s_base: LDS [64]).  The
// node-global record regions are filled through G counters, one per owner rank: one returning
// atomic per chunk on those few addresses serialised at the memory side (gx_emit 30.8 ms and place
// part 1 ~20 ms per 4 GiB batch, profiles/r06_lb2_kernel_stats.csv), one per wave still ~1.5 ms.
__device__ __forceinline__ unsigned long long wg_reserve(unsigned long long *counts, int d, bool want, int G,
                                                         uint32_t *s_cnt, unsigned long long *s_base)
{
    const int t = (int)threadIdx.x;
    if (t < G) s_cnt[t] = 0u;
    __syncthreads();
    uint32_t li = 0;
    if (want) li = atomicAdd(&s_cnt[d], 1u);
    __syncthreads();
    if (t < G && s_cnt[t]) s_base[t] = atomicAdd(counts + t, (unsigned long long)s_cnt[t]);
    __syncthreads();
    return want ? s_base[d] + li : 0ull;
}


// Bounds-checked 16-B load (bytes >= avail read as 0).
__device__ __noinline__ uint4 load16_guard(const uint8_t *base, int64_t off, int64_t avail)
{
    if (off + 16 <= avail) return ld16(base + off);
    uint32_t w[4] = {0, 0, 0, 0};
    for (int i = 0; i < 16; i++)
        if (off + i < avail) w[i >> 2] |= (uint32_t)base[off + i] << (8 * (i & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __noinline__ uint32_t load4_guard(const uint8_t *base, int64_t off, int64_t avail)
{
    if (off + 4 <= avail) return ld4(base + off);
    uint32_t w = 0;
    for (int i = 0; i < 4; i++)
        if (off + i < avail) w |= (uint32_t)base[off + i] << (8 * i);
    return w;
}

// 16 output bytes from an arbitrarily aligned source: two aligned 16-B loads + a funnel shift by
// sh = src & 15 (uniform per run, since destination words are 16-B aligned within a run).
template <bool NT = false>
__device__ __forceinline__ uint4 load16_shift(const uint8_t *src_aligned, int sh)
{
    const uint4 x = ld16_t<NT>(src_aligned);
    if (sh == 0) return x;
    const uint4 y = ld16_t<NT>(src_aligned + 16);
    const uint32_t r = (uint32_t)(sh & 3);
#define AB(hi, lo) __builtin_amdgcn_alignbyte((hi), (lo), r)
    switch (sh >> 2) {                                   // uniform per run
    case 0: return make_uint4(AB(x.y, x.x), AB(x.z, x.y), AB(x.w, x.z), AB(y.x, x.w));
    case 1: return make_uint4(AB(x.z, x.y), AB(x.w, x.z), AB(y.x, x.w), AB(y.y, y.x));
    case 2: return make_uint4(AB(x.w, x.z), AB(y.x, x.w), AB(y.y, y.x), AB(y.z, y.y));
    default: return make_uint4(AB(y.x, x.w), AB(y.y, y.x), AB(y.z, y.y), AB(y.w, y.z));
    }
#undef AB
}

__device__ __forceinline__ void st16(void *p, uint4 v)
{
    u32x4v w = {v.x, v.y, v.z, v.w};
    *(HDRF_GLOBAL u32x4v *)p = w;
}
template <bool NT>
__device__ __forceinline__ void st16_t(void *p, uint4 v)
{
    u32x4v w = {v.x, v.y, v.z, v.w};
    if (NT) __builtin_nontemporal_store(w, (HDRF_GLOBAL u32x4v *)p);
    else *(HDRF_GLOBAL u32x4v *)p = w;
}
// streaming-knob bits (HDRF_NT): 1 = granule-max pass loads, 2 = place copy loads + stores
int stream_knobs();   // default 3 (measured +1.5 % on the config-2 bench); HDRF_NT=0 turns both off

}  // namespace hdrf
