// index_probe.hpp — the probe protocol of the fingerprint table (index_entry.hpp IndexEntry), written once.
//
// Every table of the project — the single-GPU index and the scratch table of the node-global front
// (index.hip), an owner's partition of the node-global index (gx.hip), and the readers (read.hip) —
// is open addressing over one layout: linear probing from tag_home, an entry is live when its tag
// carries the table's epoch, and the full digest tells apart entries that share a tag.  A batch
// enters its items (chunks, or the X1 records an owner received) in three steps:
//   claim  — one lane per item: probe by tag, CAS-claim a slot that is not live, stop on a tag hit
//   apply  — the items claim deferred: verify the full digest and record, or queue a tag collision
//   slow   — one thread: exact sequential re-probe of the queued collisions (astronomically rare
//            with 56 tag bits; the debug_tag_bits hook forces them)
// What an item records in the entry's batch-local fields (mask, first) is the caller's record policy:
//   struct R {
//       void init(IndexEntry *e) const;     // the claimer: the fields hold this item alone
//       void atomic(IndexEntry *e) const;   // add this item; other lanes record concurrently
//       void seq(IndexEntry *e) const;      // add this item; the slow path's single thread
//   };
// (index.hip BlockOccurrence, gx.hip OwnerRecord).  Loading the digest words and addressing the slot /
// flag arrays stay with the kernels, and so do the __restrict__ qualifiers: the helpers are inlined
// into kernels whose parameters carry them.  The readers' lookup body (probe_read_row: find, decode,
// locate the readable container) is here too, once for rd_lookup (read.hip) and rv_lookup (readv.hip).
#pragma once
#include "common.hpp"
#include "rd_chunk.hpp"

namespace hdrf {

// CAS-claim e for `tag` unless it is live.  t: the tag read from e; on false, the live tag that holds
// the slot.  An entry of an older epoch is empty: the CAS replaces the tag that was read.
__device__ __forceinline__ bool claim_if_empty(IndexEntry *e, unsigned long long &t, unsigned long long tag,
                                               unsigned long long key)
{
    bool mine = false;
    while (!tag_live(t, key)) {
        const unsigned long long old = atomicCAS(&e->tag, t, tag);
        if (old == t) { mine = true; break; }
        t = old;
    }
    return mine;
}

// ---- claim (parallel) ----------------------------------------------------------------------
// Returns false when the table is full (err |= 2, no slot).  Otherwise *slot is the claimed entry or
// the first entry carrying the tag, and *applied tells whether the item is recorded already.  It is
// when the digest is known to match: the claimer (its digest IS the entry's: it initialises the
// batch-local fields with its own item), or an entry created by an earlier batch of this epoch
// (batch in [bfirst, cur): its digest bytes are immutable).  Tag hits on entries created in this
// batch by another lane are deferred to apply (their digest bytes may not be visible yet) — and so
// is a stale `batch` of the previous epoch read between another lane's CAS and its batch store (such
// ids are < bfirst).
template <int HW, class R>
__device__ __forceinline__ bool probe_claim(IndexEntry *tab, int log2cap, uint32_t cur, uint32_t bfirst,
                                            unsigned long long key, const uint32_t *dw, const R &rec, int *err,
                                            uint32_t *slot, bool *applied)
{
    const unsigned long long tag = tag_word(dw, key);
    const uint64_t mask = (1ull << log2cap) - 1;
    uint64_t h = tag_home(tag, log2cap);
    bool mine = false;
    for (uint64_t probe = 0;; probe++) {
        if (probe > mask) { atomicOr(err, 2); return false; }     // table full
        IndexEntry *e = tab + h;
        unsigned long long t = __hip_atomic_load(&e->tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        mine = claim_if_empty(e, t, tag, key);
        if (mine) {
            e->batch = cur;
            rec.init(e);
            store_dig<HW>(e, dw);
            break;
        }
        if (t == tag) break;
        h = (h + 1) & mask;
    }
    *slot = (uint32_t)h;
    IndexEntry *e = tab + h;
    bool apply = false;
    if (!mine) {
        const uint32_t bt = e->batch;
        apply = bt >= bfirst && bt != cur && entry_matches<HW>(*e, dw);
        if (apply) rec.atomic(e);
    }
    *applied = mine || apply;
    return true;
}

// ---- apply (parallel): an item claim deferred, at the entry claim found -----------------------
// The full digest matches: record.  Otherwise the entry belongs to another digest with the same tag:
// the item joins the collision list (err |= 4 when the list is full).
template <int HW, class R>
__device__ __forceinline__ void probe_apply(IndexEntry *e, const uint32_t *dw, const R &rec, uint32_t item,
                                            uint32_t *coll, uint32_t *ncoll, int coll_cap, int *err)
{
    if (entry_matches<HW>(*e, dw)) {
        rec.atomic(e);
    } else {
        const uint32_t i = atomicAdd(ncoll, 1u);
        if ((int)i < coll_cap) coll[i] = item;
        else atomicOr(err, 4);
    }
}

// ---- slow (one thread): exact re-probe of a collided item, from the slot after the one claim found
// Returns false when the table is full; otherwise records the item and *slot is its entry.
template <int HW, class R>
__device__ __forceinline__ bool probe_slow(IndexEntry *tab, int log2cap, uint32_t cur, unsigned long long key,
                                           const uint32_t *dw, const R &rec, uint32_t *slot)
{
    const unsigned long long tag = tag_word(dw, key);
    const uint64_t mask = (1ull << log2cap) - 1;
    uint64_t h = (*slot + 1) & mask;
    for (uint64_t probe = 0;; probe++) {
        if (probe > mask) return false;
        IndexEntry *e = tab + h;
        if (!tag_live(e->tag, key)) {
            e->tag = tag; e->batch = cur; e->mask = 0; e->first = 0;
            store_dig<HW>(e, dw);
            break;
        }
        if (e->tag == tag && entry_matches<HW>(*e, dw)) break;
        h = (h + 1) & mask;
    }
    *slot = (uint32_t)h;
    rec.seq(tab + h);
    return true;
}

// ---- find (read-only): the entry holding the digest; nullptr when absent ------------------------
template <int HW>
__device__ __forceinline__ const IndexEntry *probe_find(const uint32_t *dw, const IndexEntry *tab, int log2cap,
                                                        unsigned long long key)
{
    const unsigned long long tag = tag_word(dw, key);
    const uint64_t mask = (1ull << log2cap) - 1;
    uint64_t h = tag_home(tag, log2cap);
    for (uint64_t probe = 0; probe <= mask; probe++) {
        const IndexEntry &e = tab[h];
        if (!tag_live(e.tag, key)) return nullptr;           // empty (or of an older epoch)
        if (e.tag == tag && entry_matches<HW>(e, dw)) return &e;
        h = (h + 1) & mask;
    }
    return nullptr;
}

// ---- find, for a reader (rd_lookup, rv_lookup): the digest's RdChunk row — where its bytes are and
// which entry of the readable container list (cids, sorted by id) holds them; the block offset is the
// scan's.  False when the digest is absent (the row is then empty); how a miss is reported, and whether
// a chunk without a readable container matters, stay with the kernels.
template <int HW>
__device__ __forceinline__ bool probe_read_row(const uint32_t *dw, const IndexEntry *tab, int log2cap,
                                               unsigned long long key, const uint32_t *cids, int ncont, RdChunk &r)
{
    r.slot = kRdNoSlot; r.start = 0; r.len = 0; r.off = 0;
    const IndexEntry *e = probe_find<HW>(dw, tab, log2cap, key);
    if (!e) return false;
    r.start = e->start;
    r.len = e->stop - e->start;                              // chunkMeta.length = blockStop - blockStart
    const int j = find_cid(cids, ncont, e->cid);
    if (j >= 0) r.slot = (uint32_t)j;
    return true;
}

// ---- claim the first empty slot of a tag's probe sequence (restore: digests are unique, nothing is
// looked up); nullptr when the table is full.  The caller fills the entry.
__device__ __forceinline__ IndexEntry *probe_claim_empty(IndexEntry *tab, int log2cap, unsigned long long key,
                                                         unsigned long long tag)
{
    const uint64_t mask = (1ull << log2cap) - 1;
    uint64_t h = tag_home(tag, log2cap);
    for (uint64_t probe = 0; probe <= mask; probe++, h = (h + 1) & mask) {
        unsigned long long t = tab[h].tag;
        if (claim_if_empty(tab + h, t, tag, key)) return tab + h;
    }
    return nullptr;
}

}  // namespace hdrf
