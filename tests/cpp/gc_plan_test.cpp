// The host arithmetic of the index garbage collection (hdrf_amd/csrc/gc_plan.hpp) against a
// per-digest model (tests/test_gc.py compiles this with -fsanitize=address,undefined and runs it):
//   jobs     for 0, 1 and many recipes, empty ones among them and counts at the launch-tile edges:
//            every flat position belongs to exactly the recipe and the digest the model walks to, and
//            the digest address is dig + index * digest bytes, inside the recipe
//   grid     the mark launch visits every flat position exactly once, also past the grid cap
//   rows     the survivor capacity; the scratch regions are 256-B aligned, in order and disjoint
#include <cstdio>
#include <vector>

#include "../../hdrf_amd/csrc/gc_plan.hpp"

using namespace hdrf;

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
            return 1;                                             \
        }                                                         \
    } while (0)

struct Recipe { uint64_t dig; uint32_t n; };

// the model: walk the recipes in order, one digest at a time
static int check_plan(const std::vector<Recipe> &rs, uint32_t H)
{
    GcPlan plan;
    for (auto &r : rs) plan.add(r.dig, r.n);
    plan.finish();
    std::vector<std::pair<uint32_t, uint32_t>> owner;            // flat position -> (recipe, digest index)
    for (uint32_t j = 0; j < rs.size(); j++)
        for (uint32_t k = 0; k < rs[j].n; k++) owner.push_back({j, k});
    CHECK(plan.recipes == rs.size());
    CHECK(plan.total == owner.size());
    CHECK(plan.jobs.size() == (size_t)plan.njobs() + 1);
    CHECK(plan.jobs.back().first == plan.total);
    uint32_t nonempty = 0;
    for (auto &r : rs) nonempty += r.n != 0;
    CHECK(plan.njobs() == nonempty);
    for (uint32_t j = 0; j + 1 < plan.jobs.size(); j++) CHECK(plan.jobs[j].first < plan.jobs[j + 1].first);
    for (uint64_t i = 0; i < owner.size(); i++) {
        const uint32_t j = gc_find_job(plan.jobs.data(), plan.njobs(), i);
        CHECK(j < plan.njobs());
        const GcJob &jb = plan.jobs[j];
        const Recipe &want = rs[owner[i].first];
        CHECK(jb.dig == want.dig);                               // (the test's addresses are distinct)
        CHECK(i >= jb.first && i - jb.first == owner[i].second);
        const uint64_t addr = jb.dig + (i - jb.first) * H;
        CHECK(addr >= want.dig && addr + H <= want.dig + (uint64_t)want.n * H);
    }
    return 0;
}

static int test_jobs()
{
    for (uint32_t H : {20u, 28u}) {
        CHECK(check_plan({}, H) == 0);                           // no recipe
        CHECK(check_plan({{0x1000, 0}}, H) == 0);                // one empty recipe
        for (uint32_t n : {1u, 2u, 63u, 64u, 65u, 255u, 256u, 257u, 511u, 512u, 513u, 1000u})
            CHECK(check_plan({{0x7f0000000000ull, n}}, H) == 0);
        // many: empty ones first, last, adjacent and between; counts around the tile of 256
        std::vector<Recipe> rs;
        uint64_t a = 0x7f1000000000ull;
        const uint32_t counts[] = {0, 0, 1, 255, 0, 256, 1, 0, 0, 257, 3, 512, 0, 50, 1, 1, 0};
        for (uint32_t n : counts) { rs.push_back({a, n}); a += 0x100000; }
        CHECK(check_plan(rs, H) == 0);
        rs.clear();
        for (uint32_t j = 0; j < 700; j++) { rs.push_back({a, (j * 37u) % 11u}); a += 0x1000; }   // many small, some empty
        CHECK(check_plan(rs, H) == 0);
        rs.clear();
        for (uint32_t j = 0; j < 5; j++) { rs.push_back({a, 0}); a += 0x1000; }                    // only empty recipes
        CHECK(check_plan(rs, H) == 0);
    }
    return 0;
}

// the kernels' loop: lane (workgroup x, thread t) visits x * tile + t, then strides by grid * tile
static int test_grid()
{
    CHECK(gc_grid(0) == 0);
    const uint64_t full = (uint64_t)kGcMaxGrid * kGcTile;        // items of the largest grid's first round
    const uint64_t cases[] = {1, 255, 256, 257, 512, 513, 100000, full - 1, full, full + 1, full * 2 + 77};
    for (uint64_t items : cases) {
        const uint32_t g = gc_grid(items);
        CHECK(g >= 1 && g <= kGcMaxGrid);
        CHECK((uint64_t)g * kGcTile >= items || g == kGcMaxGrid);
        if (g > 1) CHECK((uint64_t)(g - 1) * kGcTile < items);   // no workgroup without work
        std::vector<uint8_t> hit((size_t)items, 0);
        const uint64_t stride = (uint64_t)g * kGcTile;
        for (uint64_t lane = 0; lane < stride; lane++)
            for (uint64_t i = lane; i < items; i += stride) hit[(size_t)i]++;
        for (uint64_t i = 0; i < items; i++) CHECK(hit[(size_t)i] == 1);
    }
    return 0;
}

static int test_rows_and_layout()
{
    CHECK(gc_row_cap(0, 1024) == 0);
    CHECK(gc_row_cap(5, 1024) == 5);
    CHECK(gc_row_cap(1024, 1024) == 1024);
    CHECK(gc_row_cap(1ull << 40, 1024) == 1024);
    for (uint64_t nj : {0ull, 1ull, 9000ull})
        for (uint64_t nc : {1ull, 3ull, 5000ull})
            for (uint64_t slots : {1024ull, 1ull << 16, 1ull << 24})
                for (uint64_t rows : {0ull, 1ull, 900ull, 1ull << 20})
                    for (uint32_t hw : {5u, 7u}) {
                        const GcLayout L = gc_layout(nj, nc, slots, rows, hw, 32);
                        const uint64_t o[] = {L.o_cnt, L.o_wg, L.o_jobs, L.o_cid, L.o_ccnt, L.o_seen, L.o_mark, L.o_dw, L.o_val};
                        const uint64_t need[] = {256, kWalkMaxWgs * 4, (nj + 1) * sizeof(GcJob), nc * 4, nc * 32,
                                                 kGcCidBits / 8, slots / 8, rows * hw * 4, rows * 11};
                        for (int i = 0; i < 9; i++) {
                            CHECK(o[i] % 256 == 0);
                            CHECK(o[i] + need[i] <= (i < 8 ? o[i + 1] : L.total));
                        }
                    }
    return 0;
}

int main()
{
    if (test_jobs() || test_grid() || test_rows_and_layout()) return 1;
    std::printf("PASS\n");
    return 0;
}
