// The host arithmetic of the batched, ranged read (hdrf_amd/csrc/read_plan.hpp) against per-byte
// models (tests/test_read_batch.py compiles this with -fsanitize=address,undefined and runs it):
//   clipping   every (size, offset, length) of a small cube, plus the 64-bit edges, against a model
//              that walks the requested bytes one by one
//   tiles      for every destination alignment 0..15 and every length 0..3T+17 (T = 4096, 8192,
//              16384): the tiles of a request partition [0, len) exactly and in order, none is empty
//              or longer than T, and every tile but the first starts on a 16-B aligned destination
//   prefix     first rows / tiles of a mixed call, and the overflow guard
//   layout     the scratch regions are 256-B aligned, in order and disjoint
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../hdrf_amd/csrc/read_plan.hpp"

using namespace hdrf;

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
            return 1;                                             \
        }                                                         \
    } while (0)

// bytes of [offset, offset + length) that exist in a block of `size` bytes, one at a time
static bool model_clip(uint64_t size, uint64_t offset, uint64_t length, uint64_t *n)
{
    if (offset > size) return false;
    *n = 0;
    for (uint64_t i = 0; i < length; i++) {
        if (offset + i >= size) break;
        ++*n;
    }
    return true;
}

static int test_clip()
{
    for (uint64_t size = 0; size <= 12; size++)
        for (uint64_t off = 0; off <= 15; off++)
            for (uint64_t len = 0; len <= 15; len++) {
                uint64_t a = 99, b = 99;
                const bool ok = read_clip(size, off, len, &a), mok = model_clip(size, off, len, &b);
                CHECK(ok == mok);
                CHECK(ok == (off <= size));
                if (ok) CHECK(a == b);
                if (ok && (off == size || len == 0)) CHECK(a == 0);
            }
    uint64_t n = 0;
    const uint64_t big = ~0ull;
    CHECK(read_clip(10, 3, big, &n) && n == 7);                    // offset + length wraps
    CHECK(read_clip(10, 10, big, &n) && n == 0);
    CHECK(!read_clip(10, 11, 0, &n));
    CHECK(!read_clip(10, big, big, &n));
    CHECK(read_clip(big, big - 5, 100, &n) && n == 5);
    CHECK(read_clip(0, 0, 5, &n) && n == 0);                       // the empty block
    return 0;
}

static int test_tiles()
{
    for (uint32_t T : {4096u, 8192u, 16384u}) {
        std::vector<uint8_t> hit((size_t)3 * T + 17);
        for (uint64_t a = 0; a < 16; a++) {
            const uint64_t dst = 0x7f0000001000ull + a;
            for (uint64_t len = 0; len <= (uint64_t)3 * T + 17; len++) {
                const uint64_t nt = read_tiles(dst, len, T);
                CHECK((nt == 0) == (len == 0));
                // every byte counted as well near the tile seams and at a stride (all of them would be
                // 10^10 byte visits)
                const uint64_t m = (a + len) % T;
                const bool bytewise = len <= 64 || m <= 17 || m + 17 >= T || len % 509 == 0;
                if (bytewise) std::fill(hit.begin(), hit.begin() + (long)len, 0);
                uint64_t prev = 0;
                for (uint64_t k = 0; k < nt; k++) {
                    uint64_t t0, t1;
                    read_tile_span(dst, len, T, k, &t0, &t1);
                    CHECK(t0 == prev && t0 < t1 && t1 <= len && t1 - t0 <= T);
                    if (k) CHECK(((dst + t0) & 15) == 0);
                    if (k + 1 < nt && k) CHECK(t1 - t0 == T);
                    if (bytewise) for (uint64_t i = t0; i < t1; i++) hit[(size_t)i]++;
                    prev = t1;
                }
                CHECK(prev == len);                                // consecutive spans from 0 to len: a partition
                if (bytewise) for (uint64_t i = 0; i < len; i++) CHECK(hit[(size_t)i] == 1);
            }
        }
    }
    return 0;
}

static int test_prefix_and_layout()
{
    const uint32_t T = 8192;
    ReadPrefix px;
    uint32_t r0, t0;
    CHECK(px.add(5, 0x1000, 100, T, &r0, &t0) && r0 == 0 && t0 == 0);          // one tile
    CHECK(px.add(0, 0, 0, T, &r0, &t0) && r0 == 5 && t0 == 1);                 // a failed request: nothing
    CHECK(px.add(7, 0x100f, 2 * T, T, &r0, &t0) && r0 == 5 && t0 == 1);        // misaligned by 15: three tiles
    CHECK(px.add(1, 0x2000, 0, T, &r0, &t0) && r0 == 12 && t0 == 4);           // zero bytes: rows, no tile
    CHECK(px.rows == 13 && px.tiles == 4);
    CHECK(!px.add(0x7fffffffu, 0, 0, T, &r0, &t0));                            // rows past 2^31
    for (uint32_t nreq : {1u, 3u, 256u})
        for (uint32_t ncont : {0u, 1u, 70u})
            for (uint64_t dig : {0ull, 20ull, 28ull * 1000})
                for (uint64_t rows : {0ull, 1ull, 100000ull}) {
                    const ReadLayout L = read_layout(nreq, ncont, dig, rows, 16);
                    const uint64_t o[] = {L.o_desc, L.o_cid, L.o_base, L.o_dig, L.o_status, L.o_rows};
                    const uint64_t need[] = {(uint64_t)nreq * sizeof(ReadDesc), (uint64_t)ncont * 4, (uint64_t)ncont * 8, dig,
                                             (uint64_t)nreq * 4, rows * 16};
                    for (int i = 0; i < 6; i++) {
                        CHECK(o[i] % 256 == 0);
                        CHECK(o[i] + need[i] <= (i < 5 ? o[i + 1] : L.total));
                    }
                    CHECK(L.upload == L.o_dig + dig && L.upload <= L.o_status);
                }
    return 0;
}

int main()
{
    if (test_clip() || test_tiles() || test_prefix_and_layout()) return 1;
    std::printf("PASS\n");
    return 0;
}
