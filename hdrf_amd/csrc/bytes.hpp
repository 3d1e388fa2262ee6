// bytes.hpp — byte-granular device helpers: unaligned loads, byte stores and the wave-cooperative copy
// of the codec kernels (lz4.hip, snappy.hip, lzo.hip), the reads (read.hip, readv.hip) and the
// compaction (compact.hip).
#pragma once
#include "launchers.hpp"

namespace hdrf {

__device__ __forceinline__ uint32_t rd32u(const uint8_t *p)
{
    const uintptr_t a = (uintptr_t)p;
    const HDRF_GLOBAL uint32_t *q = gptr<uint32_t>((const void *)(a & ~(uintptr_t)3));
    return __builtin_amdgcn_alignbyte(q[1], q[0], (uint32_t)(a & 3));
}
// the 4 bytes at base + off, for a wave-uniform base: one global_load_dword with the base in SGPRs
// and a 32-bit lane offset (the amdhsa target runs with unaligned global access enabled, so the
// unaligned dword is a single load, against rd32u's aligned pair, 64-bit address and alignbyte)
__device__ __forceinline__ uint32_t ld32u(const uint8_t *base, uint32_t off)
{
    typedef uint32_t __attribute__((aligned(1))) u32u;
    return *gptr<u32u>((const void *)(base + off));
}
__device__ __forceinline__ uint32_t rd8(const uint8_t *p) { return *(const HDRF_GLOBAL uint8_t *)p; }
__device__ __forceinline__ void wr8(uint8_t *p, uint32_t v) { *(HDRF_GLOBAL uint8_t *)p = (uint8_t)v; }

// wave-cooperative copy of n bytes (any alignment on both sides; 16-B aligned destination words: head
// bytes up to the first one, 16-B words whose source is funnel-shifted, tail bytes).  NT: nontemporal
// loads and stores, for bytes that are touched once (compact.hip cp_gather).
template <bool NT = false>
__device__ inline void wave_copy(uint8_t *dst, const uint8_t *src, uint32_t n)
{
    const uint32_t l = (uint32_t)lane_id();
    uint32_t head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    if (head > n) head = n;
    if (l < head) wr8(dst + l, rd8(src + l));
    uint8_t *d = dst + head;
    const uint8_t *sp = src + head;
    const uint32_t n16 = (n - head) >> 4;
    const int sh = (int)((uintptr_t)sp & 15);
    const uint8_t *sa = sp - sh;
    uint32_t i = l;
    for (; i + 192 < n16; i += 256) {                 // four 16-B words per lane in flight
        const uint4 v0 = load16_shift<NT>(sa + 16 * (size_t)i, sh);
        const uint4 v1 = load16_shift<NT>(sa + 16 * (size_t)(i + 64), sh);
        const uint4 v2 = load16_shift<NT>(sa + 16 * (size_t)(i + 128), sh);
        const uint4 v3 = load16_shift<NT>(sa + 16 * (size_t)(i + 192), sh);
        st16_t<NT>(d + 16 * (size_t)i, v0);
        st16_t<NT>(d + 16 * (size_t)(i + 64), v1);
        st16_t<NT>(d + 16 * (size_t)(i + 128), v2);
        st16_t<NT>(d + 16 * (size_t)(i + 192), v3);
    }
    for (; i < n16; i += 64) st16_t<NT>(d + 16 * (size_t)i, load16_shift<NT>(sa + 16 * (size_t)i, sh));
    const uint32_t tb = head + 16 * n16;
    for (uint32_t k = tb + l; k < n; k += 64) wr8(dst + k, rd8(src + k));
}

__device__ __forceinline__ void put_be32(uint8_t *p, uint32_t v)
{
    wr8(p, v >> 24); wr8(p + 1, v >> 16); wr8(p + 2, v >> 8); wr8(p + 3, v);
}

}  // namespace hdrf
