// The hdrf_scheme.hpp pass-throughs of the scrub and the verified read (tests/test_scrub.py):
// a clean store scrubs clean and reads back verified; a second scheme restored from the first one's
// index, recipes and container files, with one byte of one file flipped, reports exactly the chunk
// that holds the byte, and the verified read of the block throws HDRF_E_CORRUPT.
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "hdrf_scheme.hpp"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
            return 1;                                             \
        }                                                         \
    } while (0)

int main()
{
    hdrf_cfg cfg;
    hdrf_default_cfg(&cfg);
    cfg.max_block_bytes = 4 << 20;
    cfg.max_batch_blocks = 2;
    cfg.index_log2 = 16;
    cfg.arena_slots = 16;
    cfg.container_max = 4 << 20;
    cfg.keep_recipes = 1;
    std::vector<uint8_t> block(600000);
    uint64_t x = 88172645463325252ull;                            // xorshift64: incompressible, no repeats
    for (auto &b : block) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b = (uint8_t)(x >> 32); }
    const uint64_t id = 77;
    std::vector<uint8_t> keys, vals, recipe;
    std::map<uint32_t, std::vector<uint8_t>> files;                // container id -> its file
    int64_t nrows = 0;
    {
        hdrf::HipReductionScheme s(&cfg);
        s.reduce(block.data(), block.size(), id);
        hdrf_scrub_stats st{};
        CHECK(s.scrub(-1, &st).empty());
        CHECK(st.bad == 0 && st.skipped == 0 && st.checked == st.entries && st.checked > 100);
        CHECK(st.bytes == (int64_t)block.size());
        CHECK(s.reconstruct_verified(id) == block);
        const int H = hdrf_digest_len(s.handle());
        nrows = hdrf_index_count(s.handle());
        keys.resize((size_t)nrows * H);
        vals.resize((size_t)nrows * 11);
        CHECK(hdrf_index_dump(s.handle(), keys.data(), vals.data(), nrows) == nrows);
        recipe = s.recipe(id);
        for (int64_t r = 0; r < nrows; r++) {                      // every container the rows name
            const uint8_t *v = &vals[(size_t)r * 11];
            const uint32_t c = ((uint32_t)v[1] << 16) | ((uint32_t)v[2] << 8) | v[3];
            if (files.count(c)) continue;
            int32_t closed = 0;
            const int64_t flen = hdrf_container_read(s.handle(), c, nullptr, 0, &closed);
            CHECK(flen > 0);
            files[c].resize((size_t)flen);
            CHECK(hdrf_container_read(s.handle(), c, files[c].data(), flen, &closed) == flen);
        }
    }
    hdrf::HipReductionScheme s(&cfg);                              // the restarted node, one file damaged
    CHECK(hdrf_index_load(s.handle(), keys.data(), vals.data(), nrows) == 0);
    CHECK(hdrf_recipe_load(s.handle(), id, recipe.data(), (int64_t)recipe.size()) == 0);
    CHECK(!files.empty());
    const uint32_t cid = files.begin()->first;
    const uint32_t pos = (uint32_t)files[cid].size() / 2;
    files[cid][pos] ^= 0x10;
    for (auto &kv : files)
        CHECK(hdrf_container_load(s.handle(), kv.first, kv.second.data(), (int64_t)kv.second.size(), 0) == 0);
    hdrf_scrub_stats st{};
    const std::vector<hdrf_bad_chunk> bad = s.scrub((int64_t)cid, &st);
    CHECK(bad.size() == 1 && st.bad == 1);
    CHECK(bad[0].container == cid && bad[0].start <= pos && pos < bad[0].stop && bad[0].why == 1);
    bool in_recipe = false;                                        // the bad digest is one of the block's
    const size_t H = (size_t)hdrf_digest_len(s.handle());
    for (size_t o = 4; o + H <= recipe.size(); o += H) in_recipe |= std::memcmp(&recipe[o], bad[0].digest, H) == 0;
    CHECK(in_recipe);
    bool threw = false;
    try {
        s.reconstruct_verified(id);
    } catch (const hdrf::Error &e) {
        threw = e.code == HDRF_E_CORRUPT;
    }
    CHECK(threw);
    CHECK(s.reconstruct(id).size() == block.size());              // unverified: bytes, no error
    std::printf("PASS\n");
    return 0;
}
