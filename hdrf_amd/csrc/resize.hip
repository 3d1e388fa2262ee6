// resize.hip — the online table resize on gfx950 (hdrf_index_resize, api_resize.hip).
//
// One pass moves every live entry of the old table into the new one, table to table and verbatim:
//   ix_rehash — table_walk.hpp's walk over the OLD table (persistent 256-lane workgroups, one lane per
//               64-B entry, the four coalesced 16-B quarters turned lane-major through LDS, read with
//               non-temporal loads).  A live entry claims the first empty slot of its tag's probe
//               sequence in the NEW table (index_probe.hpp probe_claim_empty: one device-scope
//               compare-and-swap on the tag word, performed at the memory side, more only where probes
//               collide) and its claimer stores the other 56 bytes as they were read: the 8-B mask and
//               three 16-B quarters, plain vector stores.  The tag is the stored tag, unchanged: the
//               epoch does not change.  No digest is decoded and nothing is looked up: entries that
//               share a tag (debug_tag_bits) each claim a slot of their own, and a later find tells them
//               apart by the full digest, as it does now.  A dead entry costs its read.
// tag_home takes the top bits of a multiplicative hash, so old home -> new home is monotone
// (resize_plan.hpp): the claims and stores of one old tile land in one contiguous region of the new table.
// The kernel has no digest width: an entry moves as 64 opaque bytes.
#include "index_probe.hpp"
#include "launchers.hpp"
#include "resize_plan.hpp"
#include "table_walk.hpp"

namespace hdrf {

// err |= 1: the new table had no empty slot for a live entry (the load rule makes that impossible;
// it is reported, not assumed).
__global__ void __launch_bounds__(256) ix_rehash_kernel(const IndexEntry *__restrict__ old_tab, uint64_t old_slots,
                                                        unsigned long long key, IndexEntry *__restrict__ new_tab,
                                                        int new_log2, uint32_t *__restrict__ err)
{
    table_walk(old_tab, old_slots, [&](uint64_t, uint4 p0, uint4 p1, uint4 p2, uint4 p3) {
        const unsigned long long tag = (unsigned long long)p0.x | ((unsigned long long)p0.y << 32);
        if (!tag_live(tag, key)) return;
        IndexEntry *e = probe_claim_empty(new_tab, new_log2, key, tag);
        if (!e) { atomicOr(err, 1u); return; }
        e->mask = (unsigned long long)p0.z | ((unsigned long long)p0.w << 32);
        st16(&e->first, p1);                                   // first | batch | ncopy
        st16(&e->cid, p2);                                     // cid | start | stop | dig[0]
        st16(&e->dig[1], p3);                                  // dig[1..4]
    });
}

hipError_t launch_index_rehash(const IndexEntry *old_tab, int old_log2, unsigned long long key, IndexEntry *new_tab,
                               int new_log2, uint32_t *err, int n_cu, hipStream_t st)
{
    if (!resize_log2_ok(old_log2) || !resize_log2_ok(new_log2)) return hipErrorInvalidValue;   // whole tiles only
    hipLaunchKernelGGL(ix_rehash_kernel, dim3(resize_grid(old_log2, n_cu)), dim3(256), 0, st, old_tab, 1ull << old_log2, key,
                       new_tab, new_log2, err);
    return hipGetLastError();
}

}  // namespace hdrf
