// read_plan.hpp — the host arithmetic of the batched, ranged read (hdrf_read_batch, api_views.hip;
// kernels in readv.hip).  No HIP in here: tests/cpp/read_plan_test.cpp compiles it with g++ and checks
// it against per-byte models.
//
// A request is one byte range [offset, offset + length) of one block, clipped to the block
// (BlockSender's startOffset / length, DN/BlockSender.java:612-619).  Its clipped output is cut into
// tiles of T bytes, one wave each (rv_gather).  The tile seams sit at multiples of T counted from the
// 16-B line that holds the first destination byte, so every tile but a request's first starts on a
// 16-B aligned destination address, and its first and last tiles are short.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define HDRF_PLAN_HD __host__ __device__   // rv_gather computes its tile's span with the host's function
#else
#define HDRF_PLAN_HD
#endif

namespace hdrf {

constexpr uint32_t kReadTile = 16384;    // T: 4, 8 and 16 KiB were measured

// One request as the kernels see it (uploaded once per call).
struct ReadDesc {
    uint64_t dig;        // device address of the recipe's digests (4-B aligned): the recipe store, or scratch
    uint64_t out;        // device address of the first output byte (any alignment)
    uint32_t n;          // chunks of the recipe
    uint32_t row0;       // the request's first row in the chunk array
    uint32_t size;       // the recipe's BE32 size
    uint32_t off, len;   // the clipped range
    uint32_t tile0;      // the request's first output tile
};
static_assert(sizeof(ReadDesc) == 40, "ReadDesc is read as five 8-B words");

// status bits a kernel sets for a request (0: the gather may run)
constexpr int kReadNotFound = 1;   // a digest absent from the index, or an unreadable container in the range
constexpr int kReadDevice = 2;     // the chunk lengths do not add up to the recipe size

// Clip [offset, offset + length) to a block of `size` bytes: false when offset > size (HDRF_E_INVAL);
// otherwise *clen = the bytes the request returns (0 when offset == size or length == 0).
inline bool read_clip(uint64_t size, uint64_t offset, uint64_t length, uint64_t *clen)
{
    if (offset > size) return false;
    const uint64_t left = size - offset;              // no offset + length: it may wrap
    *clen = length < left ? length : left;
    return true;
}

// Tiles of a request of `len` output bytes whose first byte goes to destination address `dst`.
inline uint64_t read_tiles(uint64_t dst, uint64_t len, uint32_t T)
{
    return len ? ((dst & 15) + len + T - 1) / T : 0;
}

// Tile k of that request covers output bytes [*t0, *t1).
HDRF_PLAN_HD inline void read_tile_span(uint64_t dst, uint64_t len, uint32_t T, uint64_t k, uint64_t *t0, uint64_t *t1)
{
    const uint64_t a = dst & 15;
    const uint64_t e = (k + 1) * T - a;
    *t0 = k ? k * T - a : 0;
    *t1 = e < len ? e : len;
}

// Where the pieces of one call live in the read scratch (ctx->d_rd), each on a 256-B boundary:
// [descriptors | container ids | container bases | caller-supplied digests] are uploaded as one copy
// of `upload` bytes, then the status words (cleared on the device) and the chunk rows (device only).
struct ReadLayout {
    uint64_t o_desc, o_cid, o_base, o_dig, upload, o_status, o_rows, total;
};
inline uint64_t read_up256(uint64_t x) { return (x + 255) & ~255ull; }
inline ReadLayout read_layout(uint32_t nreq, uint32_t ncont, uint64_t dig_bytes, uint64_t rows, uint32_t row_bytes)
{
    ReadLayout L;
    L.o_desc = 0;
    L.o_cid = read_up256((uint64_t)nreq * sizeof(ReadDesc));
    L.o_base = read_up256(L.o_cid + (uint64_t)ncont * 4);
    L.o_dig = read_up256(L.o_base + (uint64_t)ncont * 8);
    L.upload = L.o_dig + dig_bytes;
    L.o_status = read_up256(L.upload);
    L.o_rows = read_up256(L.o_status + (uint64_t)nreq * 4);
    L.total = read_up256(L.o_rows + rows * row_bytes) + 256;
    return L;
}

// The prefix pass over a call's requests: add one request's rows and tiles, get its first row and tile.
// False when the rows no longer fit the kernels' 32-bit indices.
struct ReadPrefix {
    uint64_t rows = 0, tiles = 0;
    bool add(uint32_t n, uint64_t dst, uint64_t len, uint32_t T, uint32_t *row0, uint32_t *tile0)
    {
        *row0 = (uint32_t)rows;
        *tile0 = (uint32_t)tiles;
        rows += n;
        tiles += read_tiles(dst, len, T);
        return rows < (1ull << 31) && tiles < (1ull << 31);
    }
};

}  // namespace hdrf
