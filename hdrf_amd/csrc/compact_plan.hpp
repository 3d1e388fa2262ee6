// compact_plan.hpp — the host arithmetic of container compaction (hdrf_compact, api_compact.hip;
// kernels in compact.hip).  No HIP in here: tests/cpp/compact_plan_test.cpp compiles it with g++ and
// checks it against a naive model.
//
// A call names up to kCpMax closed containers.  The collect pass turns every live index entry that
// names one of them into rows: an entry of up to kCpPiece bytes is one row, a longer one is cut into
// pieces of kCpPiece bytes, so that one chunk of max_chunk bytes is not one wave's work in the
// cover and gather passes.  Only an entry's first piece carries its table slot (the rewrite pass
// stores the entry's new start / stop through it).
#pragma once
#include <stdint.h>

#include "table_walk.hpp"

namespace hdrf {

constexpr int kCpMax = 16;                   // containers per call (HDRF_COMPACT_MAX)
constexpr uint32_t kCpPiece = 16384;         // bytes of a container one cover / gather wave handles
constexpr uint32_t kCpNoSlot = 0xffffffffu;  // CpRow::slot of the pieces after an entry's first

struct CpRow {
    uint32_t slot;       // table slot of the entry (first piece) or kCpNoSlot
    uint32_t cont;       // index of the container in the call's id list
    uint32_t a, b;       // the piece: old container bytes [a, b), 0 < b - a <= kCpPiece
};
static_assert(sizeof(CpRow) == 16, "CpRow is one 16-B store");

// What the collect pass needs to know of the call's containers, passed by value.
struct CpList {
    uint32_t n;
    uint32_t id[kCpMax];
    uint32_t valid[kCpMax];      // bytes the container holds; 0 for a row the host already refused
    uint32_t use[kCpMax];        // 1: eligible (its entries become rows)
};

struct CpCount {                 // per container of the call, zeroed by the caller
    unsigned long long chunks;   // live entries that name it
    unsigned long long bytes;    // sum of stop - start over the well-formed ones
    unsigned long long covered;  // set bits of its cover map (cover pass)
    unsigned long long moved;    // entries whose start changes (plan pass)
    uint32_t bad;                // an entry with stop <= start or stop > valid
    uint32_t pad;
};
static_assert(sizeof(CpCount) == 40, "CpCount layout");

// pieces of the well-formed range [start, stop): ceil((stop - start) / kCpPiece)
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint32_t cp_pieces(uint32_t start, uint32_t stop)
{
    return (stop - start + kCpPiece - 1) / kCpPiece;
}

// ---- eligibility, from the host maps ------------------------------------------------------------
enum CpHome { kCpArena = 1, kCpLoaded = 2 };
constexpr int kCpENotFound = -5, kCpEInval = -1;     // HDRF_E_NOTFOUND, HDRF_E_INVAL
// resident: the id has an arena slot (`closed`: it is closed, `pending`: retain_containers and not yet
// drained); loaded: hdrf_container_load made it readable.  A resident copy wins over a loaded one.
inline int cp_classify(bool resident, bool closed, bool pending, bool loaded)
{
    if (resident) return closed && !pending ? kCpArena : kCpEInval;
    return loaded ? kCpLoaded : kCpENotFound;
}

// The row's status once the device passes ran (0 compacted, 1 nothing to reclaim, 2 dead, -7
// inconsistent): c is the container's counters, len its bytes before.
constexpr int kCpEDevice = -7;                       // HDRF_E_DEVICE
inline int cp_status(const CpCount &c, uint64_t len)
{
    if (c.bad) return kCpEDevice;
    if (c.chunks == 0) return 2;
    if (c.covered != c.bytes || c.bytes > len) return kCpEDevice;    // overlapping ranges
    if (c.bytes == len) return 1;                    // disjoint ranges that add up to len tile [0, len)
    return 0;
}

// ---- scratch layout -----------------------------------------------------------------------------
inline uint64_t cp_up256(uint64_t x) { return (x + 255) & ~255ull; }
// words of one container's cover map: one bit per byte of container_max, plus a zero word that a
// lookup at position container_max (a chunk that ends there never asks) may not touch
inline uint64_t cp_map_words(uint32_t cmax) { return ((uint64_t)cmax + 31) / 32 + 1; }

// Where the pieces of one call live in the read-side scratch (ctx->d_rd), each on a 256-B boundary.
struct CpLayout {
    uint64_t o_cnt;      // kCpMax x CpCount, + the row total
    uint64_t o_wg;       // rows of each collect workgroup (kWalkMaxWgs words)
    uint64_t o_lz;       // compressor 2: ClosedRec[kCpMax], the count, two work words, file lengths, segment lengths
    uint64_t o_map;      // n x map words: the cover maps
    uint64_t o_pre;      // n x map words: set bits before each word
    uint64_t o_rows;     // `rows` x CpRow
    uint64_t map_stride; // bytes between two containers' maps (and prefix arrays)
    uint64_t total;
};
inline CpLayout cp_layout(uint32_t n, uint32_t cmax, uint64_t rows, uint32_t lz_segs)
{
    CpLayout L;
    L.o_cnt = 0;
    L.o_wg = cp_up256(L.o_cnt + (uint64_t)kCpMax * sizeof(CpCount) + 16);
    L.o_lz = cp_up256(L.o_wg + (uint64_t)kWalkMaxWgs * 4);
    // 16 B per ClosedRec, 256 B for the count and the work words, then the two length arrays
    const uint64_t lz_bytes = (uint64_t)kCpMax * 16 + 256 + cp_up256((uint64_t)kCpMax * 4) + (uint64_t)kCpMax * lz_segs * 4;
    L.o_map = cp_up256(L.o_lz + lz_bytes);
    L.map_stride = cp_up256(cp_map_words(cmax) * 4);
    L.o_pre = L.o_map + (uint64_t)n * L.map_stride;
    L.o_rows = L.o_pre + (uint64_t)n * L.map_stride;
    L.total = cp_up256(L.o_rows + rows * sizeof(CpRow)) + 256;
    return L;
}
// offsets inside the o_lz block
constexpr uint64_t kCpLzCount = (uint64_t)kCpMax * 16;           // the closed count (one word)
constexpr uint64_t kCpLzWork = kCpLzCount + 64;                  // launch_lz4's two work words
constexpr uint64_t kCpLzFileLen = kCpLzCount + 256;              // kCpMax file lengths
inline uint64_t cp_lz_seglen() { return kCpLzFileLen + cp_up256((uint64_t)kCpMax * 4); }

// The staging of a call (its own allocation, freed when the call returns): n images of container_max
// bytes, then under compressor 2 n Lz4Codec slots of lz_slot bytes; 256 B of slack behind each part.
struct CpStage {
    uint64_t o_img, o_lz, total;
};
inline CpStage cp_stage(uint32_t n, uint32_t cmax, uint64_t lz_slot)
{
    CpStage S;
    S.o_img = 0;
    S.o_lz = cp_up256((uint64_t)n * cmax + 256);
    S.total = S.o_lz + cp_up256((uint64_t)n * lz_slot + 256);
    return S;
}

}  // namespace hdrf
