// The hdrf_scheme.hpp pass-through of the ranged read (tests/test_read_batch.py): ranges of two
// reduced blocks equal the slices of the bytes that were written, lengths past the end are clipped,
// a range that starts past the end throws HDRF_E_INVAL, and one hdrf_read_batch call serves ranges of
// both blocks into device memory.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hdrf_scheme.hpp"

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
            return 1;                                             \
        }                                                         \
    } while (0)

static std::vector<uint8_t> slice(const std::vector<uint8_t> &b, size_t off, size_t n)
{
    if (off > b.size()) off = b.size();
    if (n > b.size() - off) n = b.size() - off;
    return std::vector<uint8_t>(b.begin() + (long)off, b.begin() + (long)(off + n));
}

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
    std::vector<uint8_t> a(600000), b(300007);
    uint64_t x = 88172645463325252ull;                            // xorshift64: incompressible, no repeats
    for (auto &v : a) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = (uint8_t)(x >> 32); }
    for (auto &v : b) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = (uint8_t)(x >> 32); }
    hdrf::HipReductionScheme s(&cfg);
    s.reduce(a.data(), a.size(), 77);
    s.reduce(b.data(), b.size(), 78);
    const size_t shapes[][2] = {{0, 600000}, {0, 1}, {599999, 1}, {599997, 100}, {600000, 5}, {1234, 0},
                                {100001, 65536}, {17, 300000}};
    for (auto &sh : shapes) {
        CHECK(s.read_range(77, sh[0], sh[1]) == slice(a, sh[0], sh[1]));
        CHECK(s.read(78, sh[0] / 2, sh[1]) == slice(b, sh[0] / 2, sh[1]));
    }
    bool threw = false;
    try {
        s.read_range(77, 600001, 1);
    } catch (const hdrf::Error &e) {
        threw = e.code == HDRF_E_INVAL;
    }
    CHECK(threw);
    threw = false;
    try {
        s.read_range(4242, 0, 1);
    } catch (const hdrf::Error &e) {
        threw = e.code == HDRF_E_NOTFOUND;
    }
    CHECK(threw);
    // the batch call itself: three ranges, one of them failing, into one device buffer
    void *dev = nullptr;
    CHECK(hdrf_dev_alloc(s.handle(), 1 << 20, &dev) == 0);
    std::vector<uint8_t> fill(1 << 20, 0xA5), got(1 << 20);
    CHECK(hdrf_memcpy_h2d(s.handle(), dev, fill.data(), fill.size()) == 0);
    hdrf_read_req q[3] = {};
    q[0].block_id = 77; q[0].offset = 5; q[0].length = 200000; q[0].dev_out = (uint8_t *)dev + 3;
    q[1].block_id = 79; q[1].offset = 0; q[1].length = 10; q[1].dev_out = (uint8_t *)dev + 300000;
    q[2].block_id = 78; q[2].offset = 300000; q[2].length = 100; q[2].dev_out = (uint8_t *)dev + 400001;
    CHECK(hdrf_read_batch(s.handle(), 3, q) == HDRF_E_NOTFOUND);
    CHECK(q[0].result == 200000 && q[1].result == HDRF_E_NOTFOUND && q[2].result == 7);
    CHECK(hdrf_memcpy_d2h(s.handle(), got.data(), dev, got.size()) == 0);
    std::memcpy(fill.data() + 3, a.data() + 5, 200000);
    std::memcpy(fill.data() + 400001, b.data() + 300000, 7);
    CHECK(got == fill);
    CHECK(hdrf_dev_free(s.handle(), dev) == 0);
    std::printf("PASS\n");
    return 0;
}
