// The hdrf_scheme.hpp pass-through of container compaction (tests/test_compact.py): two blocks that
// share half their bytes are written, one is deleted and the index collected; the closed containers
// that lost chunks are compacted through the scheme.  A dry run changes nothing; the real run hands
// out files that are what hdrf_container_read returns afterwards, the sizes add up to the values of
// the index dump, and the block that remains reads back verified.
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

static std::vector<uint8_t> noise(uint64_t x, size_t n)
{
    std::vector<uint8_t> v(n);                                    // xorshift64: incompressible, no repeats
    for (auto &b : v) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; b = (uint8_t)(x >> 32); }
    return v;
}

static bool dump(hdrf_ctx *h, std::vector<uint8_t> &keys, std::vector<uint8_t> &vals)
{
    const int H = hdrf_digest_len(h);
    const int64_t n = hdrf_index_count(h);
    keys.assign((size_t)n * H, 0);
    vals.assign((size_t)n * 11, 0);
    return hdrf_index_dump(h, keys.data(), vals.data(), n) == n;
}

int main()
{
    hdrf_cfg cfg;
    hdrf_default_cfg(&cfg);
    cfg.max_block_bytes = 4 << 20;
    cfg.max_batch_blocks = 2;
    cfg.index_log2 = 16;
    cfg.arena_slots = 16;
    cfg.container_max = 1 << 20;
    cfg.keep_recipes = 1;
    const std::vector<uint8_t> shared = noise(88172645463325252ull, 1500000);
    std::vector<uint8_t> b1 = shared, b2 = noise(1234567ull, 1500000);
    const std::vector<uint8_t> own1 = noise(7654321ull, 1500000);
    b1.insert(b1.end(), own1.begin(), own1.end());
    b2.insert(b2.end(), shared.begin(), shared.end());
    hdrf::HipReductionScheme s(&cfg);
    s.reduce(b1.data(), b1.size(), 1);
    s.reduce(b2.data(), b2.size(), 2);
    CHECK(hdrf_block_delete(s.handle(), 1) == 0);
    std::vector<hdrf_gc_container> g(256);
    hdrf_gc_stats gs{};
    const int64_t ng = hdrf_gc(s.handle(), 0, &gs, g.data(), (int64_t)g.size());
    CHECK(ng > 0 && ng <= (int64_t)g.size() && gs.dropped > 0 && gs.kept > 0);
    std::vector<uint32_t> ids;
    for (int64_t i = 0; i < ng; i++) {
        int32_t closed = 0;
        if (g[i].dropped_bytes > 0 && hdrf_container_read(s.handle(), g[i].id, nullptr, 0, &closed) >= 0 && closed &&
            ids.size() < HDRF_COMPACT_MAX)
            ids.push_back(g[i].id);
    }
    CHECK(!ids.empty());
    std::vector<uint8_t> k0, v0, k1, v1;
    CHECK(dump(s.handle(), k0, v0));
    const std::vector<hdrf_compact_row> dry = s.compact(ids, nullptr, true);
    CHECK(dump(s.handle(), k1, v1) && k1 == k0 && v1 == v0);
    std::vector<std::vector<uint8_t>> files;
    const std::vector<hdrf_compact_row> rows = s.compact(ids, &files);
    CHECK(rows.size() == ids.size() && dry.size() == ids.size());
    size_t f = 0, compacted = 0;
    CHECK(dump(s.handle(), k1, v1) && k1 == k0);
    for (size_t i = 0; i < rows.size(); i++) {
        const hdrf_compact_row &r = rows[i];
        CHECK(r.id == ids[i] && r.status == dry[i].status && r.chunks == dry[i].chunks &&
              r.moved_chunks == dry[i].moved_chunks && r.new_bytes == dry[i].new_bytes && dry[i].data_off == -1);
        CHECK(r.status == 0 || r.status == 2);
        if (r.status != 0) continue;
        compacted++;
        CHECK(r.new_bytes > 0 && r.new_bytes < r.old_bytes && r.file_bytes == r.new_bytes);
        CHECK(f < files.size() && (int64_t)files[f].size() == r.file_bytes);
        std::vector<uint8_t> now((size_t)r.file_bytes);
        int32_t closed = 0;
        CHECK(hdrf_container_read(s.handle(), r.id, now.data(), r.file_bytes, &closed) == r.file_bytes && closed);
        CHECK(now == files[f]);
        f++;
        int64_t sum = 0, n = 0;                                    // the dump's values of this container tile the file
        for (size_t e = 0; e * 11 < v1.size(); e++) {
            const uint8_t *v = &v1[e * 11];
            const uint32_t c = ((uint32_t)v[1] << 16) | ((uint32_t)v[2] << 8) | v[3];
            if (c != r.id) continue;
            const uint32_t start = ((uint32_t)(v[10] & 0xF0) << 20) | ((uint32_t)v[4] << 16) | ((uint32_t)v[5] << 8) | v[6];
            const uint32_t stop = ((uint32_t)(v[10] & 0x0F) << 24) | ((uint32_t)v[7] << 16) | ((uint32_t)v[8] << 8) | v[9];
            CHECK(start < stop && stop <= (uint32_t)r.new_bytes);
            sum += stop - start;
            n++;
        }
        CHECK(sum == r.new_bytes && n == r.chunks);
    }
    CHECK(compacted > 0 && f == files.size());
    CHECK(s.reconstruct_verified(2) == b2);
    hdrf_scrub_stats st{};
    CHECK(s.scrub(-1, &st).empty() && st.bad == 0 && st.checked == st.entries);
    const std::vector<hdrf_compact_row> again = s.compact(ids, &files);
    for (const hdrf_compact_row &r : again) CHECK(r.status == 1 || r.status == 2);
    CHECK(files.empty());
    bool threw = false;
    try {
        s.compact({ids[0], ids[0]});
    } catch (const hdrf::Error &e) {
        threw = e.code == HDRF_E_INVAL;
    }
    CHECK(threw);
    std::printf("PASS\n");
    return 0;
}
