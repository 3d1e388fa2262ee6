// The host arithmetic of container compaction (hdrf_amd/csrc/compact_plan.hpp) against a naive model
// (tests/test_compact.py compiles this with -fsanitize=address,undefined and runs it):
//   pieces   cutting [start, stop) into kCpPiece pieces as the collect pass does covers every byte once
//   status   cp_status against a byte-by-byte model of the ranges: tiles / gaps / overlap / out of bounds
//   classify every combination of the host maps
//   layout   the scratch and staging regions are 256-B aligned, in order, disjoint and large enough
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hdrf_amd/csrc/compact_plan.hpp"

using namespace hdrf;

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
            return 1;                                             \
        }                                                         \
    } while (0)

struct Range { uint32_t start, stop; };

// the model: one counter per container byte
static int check_status(const std::vector<Range> &rs, uint32_t len, int want)
{
    std::vector<uint32_t> hits(len, 0);
    CpCount c;
    std::memset(&c, 0, sizeof c);
    for (const Range &r : rs) {
        c.chunks++;
        if (r.stop <= r.start || r.stop > len) { c.bad = 1; continue; }
        c.bytes += r.stop - r.start;
        // the rows of the range, as cp_collect cuts them
        const uint32_t np = cp_pieces(r.start, r.stop);
        uint64_t covered = 0;
        for (uint32_t k = 0; k < np; k++) {
            const uint32_t a = r.start + k * kCpPiece;
            const uint32_t b = r.stop - a > kCpPiece ? a + kCpPiece : r.stop;
            CHECK(a < b && b - a <= kCpPiece && b <= r.stop);
            if (k + 1 < np) CHECK(b - a == kCpPiece);
            for (uint32_t p = a; p < b; p++) hits[p]++;
            covered += b - a;
        }
        CHECK(covered == r.stop - r.start);
    }
    bool overlap = false;
    for (uint32_t p = 0; p < len; p++) {
        c.covered += hits[p] != 0;
        overlap |= hits[p] > 1;
    }
    int model;
    if (c.bad) model = -7;
    else if (rs.empty()) model = 2;
    else if (overlap) model = -7;
    else if (c.covered == len) model = 1;
    else model = 0;
    CHECK(model == want);
    CHECK(cp_status(c, len) == want);
    return 0;
}

int main()
{
    static_assert(sizeof(CpRow) == 16 && sizeof(CpCount) == 40, "device layouts");
    // pieces and status
    CHECK(cp_pieces(0, 1) == 1 && cp_pieces(5, 5 + kCpPiece) == 1 && cp_pieces(5, 6 + kCpPiece) == 2);
    CHECK(cp_pieces(0, 1000000) == (1000000 + kCpPiece - 1) / kCpPiece);
    if (check_status({}, 100, 2)) return 1;
    if (check_status({{0, 100}}, 100, 1)) return 1;
    if (check_status({{40, 100}, {0, 40}}, 100, 1)) return 1;
    if (check_status({{0, 40}, {41, 100}}, 100, 0)) return 1;
    if (check_status({{1, 100}}, 100, 0)) return 1;
    if (check_status({{0, 99}}, 100, 0)) return 1;
    if (check_status({{50, 51}}, 100, 0)) return 1;
    if (check_status({{0, 60}, {59, 100}}, 100, -7)) return 1;             // one byte shared
    if (check_status({{0, 60}, {0, 60}}, 100, -7)) return 1;
    if (check_status({{10, 20}, {12, 18}}, 100, -7)) return 1;             // nested: bytes < len, still overlap
    if (check_status({{0, 101}}, 100, -7)) return 1;
    if (check_status({{5, 5}}, 100, -7)) return 1;
    if (check_status({{9, 5}}, 100, -7)) return 1;
    if (check_status({{0, 3 * kCpPiece + 7}}, 3 * kCpPiece + 7, 1)) return 1;
    if (check_status({{31, 2 * kCpPiece + 31}, {2 * kCpPiece + 31, 2 * kCpPiece + 32}}, 3 * kCpPiece, 0)) return 1;
    if (check_status({{0, 1000000}}, 1 << 20, 0)) return 1;
    // eligibility
    for (int m = 0; m < 16; m++) {
        const bool resident = m & 1, closed = m & 2, pending = m & 4, loaded = m & 8;
        int want;
        if (resident) want = !closed || pending ? -1 : kCpArena;          // open or undrained: HDRF_E_INVAL
        else want = loaded ? kCpLoaded : -5;                              // HDRF_E_NOTFOUND
        CHECK(cp_classify(resident, closed, pending, loaded) == want);
    }
    // layouts
    for (uint32_t n : {1u, 3u, 16u})
        for (uint32_t cmax : {1000003u, 1u << 20, 1u << 21, 32u << 20, 0xffffffffu})
            for (uint64_t rows : {0ull, 1ull, 1000ull, 1ull << 22}) {
                const uint32_t segs = (uint32_t)(((uint64_t)cmax + 261099) / 261100);
                const CpLayout L = cp_layout(n, cmax, rows, segs);
                const uint64_t o[] = {L.o_cnt, L.o_wg, L.o_lz, L.o_map, L.o_pre, L.o_rows, L.total};
                for (int i = 0; i < 7; i++) CHECK(o[i] % 256 == 0);
                for (int i = 0; i + 1 < 7; i++) CHECK(o[i] < o[i + 1]);
                CHECK(L.o_wg - L.o_cnt >= kCpMax * sizeof(CpCount) + 4);       // counters + the error word
                CHECK(L.o_lz - L.o_wg >= kWalkMaxWgs * 4 && L.o_lz - L.o_wg >= kCpMax * 8);   // (the bases reuse it)
                CHECK(kCpLzCount >= kCpMax * 16 && kCpLzWork >= kCpLzCount + 4 && kCpLzFileLen >= kCpLzWork + 8);
                CHECK(cp_lz_seglen() >= kCpLzFileLen + kCpMax * 4);
                CHECK(L.o_map - L.o_lz >= cp_lz_seglen() + (uint64_t)kCpMax * segs * 4);
                CHECK(L.map_stride % 256 == 0 && L.map_stride >= cp_map_words(cmax) * 4);
                CHECK(cp_map_words(cmax) * 32 > cmax);                        // a bit for every byte, and one more
                CHECK(L.o_pre - L.o_map == n * L.map_stride && L.o_rows - L.o_pre == n * L.map_stride);
                CHECK(L.total - L.o_rows >= rows * sizeof(CpRow));
                for (uint64_t slot : {0ull, 1ull << 20}) {
                    const CpStage S = cp_stage(n, cmax, slot);
                    CHECK(S.o_img == 0 && S.o_lz % 256 == 0 && S.o_lz >= (uint64_t)n * cmax + 16);
                    CHECK(S.total >= S.o_lz + n * slot + 16);
                }
            }
    std::printf("PASS\n");
    return 0;
}
