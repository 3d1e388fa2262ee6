// index_entry.hpp — the 64-B entry of the fingerprint table and its codec, written once: how a digest
// is packed into an entry (tag_word, store_dig), compared with one (entry_matches) and recovered from
// one (entry_digest_words), and the 11-byte value an entry stands for (encode_value).  Host and device
// share every function; no HIP in here: tests/cpp/entry_codec_test.cpp compiles it with g++ and checks
// that the packing and its inverse agree.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define HDRF_ENTRY_HD __host__ __device__ __forceinline__
#define HDRF_ENTRY_UNROLL _Pragma("unroll")
#else
#define HDRF_ENTRY_HD inline
#define HDRF_ENTRY_UNROLL
#endif

namespace hdrf {

// Index entry: 64 B.  tag = the table generation ("epoch", 1..255) in bits 56..63 over the first 7
// digest bytes; an entry whose tag carries another epoch is EMPTY, so a fresh index (hdrf_reset)
// is one epoch bump instead of 2^k x 64 B of zero stores (a real clear only every 255 resets and
// at open).  `dig` holds digest bytes 8..27; the 8th digest byte lives in dig[4] (SHA-1: dig[3..4]
// hold bytes 0..7) or in ncopy bits 8..15 (SHA-224).  ncopy (bits 0..7) / cid / start / stop are
// the 11-byte Redis value (chunkMeta.getMeta, DN/chunkMeta.java:62-77) in unpacked form.
struct alignas(64) IndexEntry {
    unsigned long long tag;
    unsigned long long mask;    // batch-local: bit b = block b of the batch holds the digest
    unsigned long long first;   // batch-local: max over ((63-b)<<32 | chunk index)
    uint32_t batch;             // batch id that created the entry (ids only grow over a context's life)
    uint32_t ncopy;             // bits 0..7 nCopy, bits 8..15 digest byte 7 (SHA-224)
    uint32_t cid;
    uint32_t start;
    uint32_t stop;
    uint32_t dig[5];

};
static_assert(sizeof(IndexEntry) == 64, "IndexEntry must be one 64-B line");

// Tag key of a table: (epoch << 56) | the tag-bit mask (all ones except under the collision test
// hook, debug_tag_bits).  tag_word: the entry tag a digest must carry; tag_live: an entry of the
// current epoch; tag_home: the digest's home slot (independent of the epoch).
constexpr unsigned long long kTag56 = 0x00FFFFFFFFFFFFFFull;
HDRF_ENTRY_HD unsigned long long tag_word(const uint32_t *dw, unsigned long long key)
{
    return ((((unsigned long long)dw[0] | ((unsigned long long)dw[1] << 32)) & key) & kTag56) | (key & ~kTag56);
}
HDRF_ENTRY_HD bool tag_live(unsigned long long t, unsigned long long key)
{
    return ((t ^ key) >> 56) == 0;
}
HDRF_ENTRY_HD uint64_t tag_home(unsigned long long t, int log2cap)
{
    return ((t & kTag56) * 0x9E3779B97F4A7C15ull) >> (64 - log2cap);
}
// the full digest equals the entry's (the caller matched the tag word: bytes 0..6)
template <int HW>
HDRF_ENTRY_HD bool entry_matches(const IndexEntry &e, const uint32_t *dw)
{
    HDRF_ENTRY_UNROLL
    for (int i = 2; i < HW; i++)
        if (e.dig[i - 2] != dw[i]) return false;
    if (HW == 5) return e.dig[3] == dw[0] && e.dig[4] == dw[1];
    return ((e.ncopy >> 8) & 0xffu) == (dw[1] >> 24);
}
// a claimed entry's digest bytes (nCopy is written by the chunk that SETs the value).  Its inverse,
// given the tag the claim stored (tag_word under all 56 tag bits), is entry_digest_words.
template <int HW>
HDRF_ENTRY_HD void store_dig(IndexEntry *e, const uint32_t *dw)
{
    HDRF_ENTRY_UNROLL
    for (int i = 2; i < HW; i++) e->dig[i - 2] = dw[i];
    if (HW == 5) { e->dig[3] = dw[0]; e->dig[4] = dw[1]; }
    else e->ncopy = (dw[1] >> 24) << 8;
}
// The digest words (little-endian loads of the digest bytes) an entry stands for, from its fields:
// SHA-1 keeps bytes 0..7 in dig[3..4]; SHA-224 keeps bytes 0..6 in the tag and byte 7 in ncopy bits
// 8..15.  Fields, not an entry: gc_sweep holds them as the raw 16-B pieces of its table walk.
template <int HW>
HDRF_ENTRY_HD void entry_digest_words(unsigned long long tag, uint32_t ncopy, const uint32_t dig[5], uint32_t dw[HW])
{
    if (HW == 5) {
        dw[0] = dig[3]; dw[1] = dig[4];
    } else {
        const unsigned long long t = tag & kTag56;
        dw[0] = (uint32_t)t;
        dw[1] = (uint32_t)(t >> 32) | (((ncopy >> 8) & 0xffu) << 24);
    }
    HDRF_ENTRY_UNROLL
    for (int i = 2; i < HW; i++) dw[i] = dig[i - 2];
}
// the 11-byte value of an entry: chunkMeta.getMeta, DN/chunkMeta.java:62-77
HDRF_ENTRY_HD void encode_value(uint32_t ncopy, uint32_t cid, uint32_t start, uint32_t stop, uint8_t v[11])
{
    v[0] = (uint8_t)ncopy;
    v[1] = (uint8_t)(cid >> 16); v[2] = (uint8_t)(cid >> 8); v[3] = (uint8_t)cid;
    v[4] = (uint8_t)(start >> 16); v[5] = (uint8_t)(start >> 8); v[6] = (uint8_t)start;
    v[7] = (uint8_t)(stop >> 16); v[8] = (uint8_t)(stop >> 8); v[9] = (uint8_t)stop;
    v[10] = (uint8_t)(((start >> 20) & 0xF0) | ((stop >> 24) & 0x0F));
}

}  // namespace hdrf
