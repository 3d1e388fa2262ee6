// rd_chunk.hpp — the read row, written once: what the lookups (read.hip rd_lookup, readv.hip rv_lookup)
// produce, the gathers and the verified read's hash (verify.hip vf_hash) consume, and the host builds
// itself for a node-global fill (api_gx.hip) or reads back to name a corrupt chunk (api_views.hip).
// No HIP in here.
#pragma once
#include <stdint.h>

namespace hdrf {

constexpr uint32_t kRdNoSlot = 0xffffffffu;   // RdChunk::slot of a chunk without a readable container

struct RdChunk {
    uint32_t slot;       // index of the container in the readable list (kRdNoSlot: missing)
    uint32_t start, len;
    uint32_t off;        // offset in the rebuilt block
};
static_assert(sizeof(RdChunk) == 16, "RdChunk is one 16-B row of the read scratch");

}  // namespace hdrf
