// The index entry's codec (hdrf_amd/csrc/index_entry.hpp) on the host (tests/test_scrub.py compiles
// this with -fsanitize=address,undefined and runs it):
//   digest   for SHA-1 (5 words) and SHA-224 (7 words): what a claim stores of a digest (the tag word
//            under all 56 tag bits, store_dig's words, then the nCopy byte) is matched by
//            entry_matches and turned back into the digest by entry_digest_words, whatever the epoch
//            and nCopy are; a digest that differs in one bit is not matched
//   value    encode_value against chunkMeta.getMeta stated byte by byte: nCopy, the low 24 bits of
//            the container id, of start and of stop, most significant byte first, and bits 24..27 of
//            start and stop in the two halves of the last byte
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../hdrf_amd/csrc/index_entry.hpp"

using namespace hdrf;

#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);      \
            return 1;                                             \
        }                                                         \
    } while (0)

static uint64_t rng_state = 0x243F6A8885A308D3ull;      // fixed seed
static uint32_t rnd()
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}

template <int HW>
static int check_digest(const uint32_t *dw, uint32_t epoch, uint32_t ncopy)
{
    const unsigned long long key = ((unsigned long long)epoch << 56) | kTag56;
    IndexEntry e;
    std::memset(&e, 0xA5, sizeof e);                    // whatever an older epoch left in the slot
    e.tag = tag_word(dw, key);                          // the claim: tag, digest words, then the value's nCopy
    store_dig<HW>(&e, dw);
    e.ncopy = (e.ncopy & ~0xffu) | (ncopy & 0xffu);     // (set_ncopy: the low byte alone)
    CHECK(tag_live(e.tag, key));
    CHECK(!tag_live(e.tag, key ^ (1ull << 56)));
    CHECK(entry_matches<HW>(e, dw));
    uint32_t back[HW];
    entry_digest_words<HW>(e.tag, e.ncopy, e.dig, back);
    for (int i = 0; i < HW; i++) CHECK(back[i] == dw[i]);
    CHECK((e.ncopy & 0xffu) == (ncopy & 0xffu));
    // one flipped bit in any word past the tag's seven bytes is another digest
    for (int i = 1; i < HW; i++) {
        uint32_t other[HW];
        std::memcpy(other, dw, sizeof other);
        other[i] ^= 1u << 31;
        CHECK(!entry_matches<HW>(e, other));
    }
    return 0;
}

template <int HW>
static int check_digests()
{
    std::vector<uint32_t> dw(HW);
    const uint32_t fills[2] = {0u, 0xffffffffu};
    for (uint32_t f : fills) {
        for (int i = 0; i < HW; i++) dw[i] = f;
        for (uint32_t epoch : {1u, 128u, 255u})
            for (uint32_t ncopy : {0u, 1u, 255u})
                if (check_digest<HW>(dw.data(), epoch, ncopy)) return 1;
    }
    for (int k = 0; k < 400; k++) {
        for (int i = 0; i < HW; i++) dw[i] = rnd();
        if (check_digest<HW>(dw.data(), 1 + rnd() % 255, rnd())) return 1;
    }
    return 0;
}

static int check_value(uint32_t ncopy, uint32_t cid, uint32_t start, uint32_t stop)
{
    uint8_t want[11];
    want[0] = (uint8_t)(ncopy % 256);
    for (int k = 0; k < 3; k++) {
        const uint32_t div = 1u << (8 * (2 - k));       // 65536, 256, 1
        want[1 + k] = (uint8_t)(cid / div % 256);
        want[4 + k] = (uint8_t)(start / div % 256);
        want[7 + k] = (uint8_t)(stop / div % 256);
    }
    want[10] = (uint8_t)(start / (1u << 24) % 16 * 16 + stop / (1u << 24) % 16);
    uint8_t got[11];
    std::memset(got, 0x5A, sizeof got);
    encode_value(ncopy, cid, start, stop, got);
    CHECK(std::memcmp(got, want, 11) == 0);
    return 0;
}

int main()
{
    if (check_digests<5>() || check_digests<7>()) return 1;
    const uint32_t edges[] = {0u, (1u << 24) - 1, 1u << 24, 1u << 25, (1u << 28) - 1};
    for (uint32_t start : edges)
        for (uint32_t stop : edges)
            for (uint32_t cid : {0u, 1u, 0x00ABCDEFu, 0x00ffffffu})
                for (uint32_t ncopy : {0u, 1u, 255u, 0x1280u})     // (bits 8..15 hold a SHA-224 digest byte)
                    if (check_value(ncopy, cid, start, stop)) return 1;
    for (int k = 0; k < 400; k++)
        if (check_value(rnd(), rnd() & 0xffffffu, rnd() >> 4, rnd() >> 4)) return 1;
    std::printf("PASS\n");
    return 0;
}
