// api_rx.hip — libhdrf C-ABI: the packet-granular receive path (hdrf_rx_begin, hdrf_append_packet,
// hdrf_rx_cancel, hdrf_submit_slot(s)).
//
// Writes the receive buffers (ctx->rx[], rx_used, host_copies) and, at hand-over, the next slot's
// copy_done event and rx_release mask; the batch itself goes through submit() (api.hip).
#include "ctx.hpp"

// ---- packet-granular receive (DN/BlockReceiver.java:877-896: each packet appended to bf1 as it
// arrives; :1258-1261 the finished block handed to the reducer) ------------------------------
// A packet is copied into the receive buffer's current pinned 4 MiB staging chunk (the caller may
// reuse the packet when the call returns); every full chunk goes H2D on stream C into the block's
// device buffer, overlapping the next packets and the kernels of the blocks in flight.  The two
// chunks alternate, waiting (host side) for a chunk's copy only before refilling it.  The packets
// of one block come from one receiver thread (the reference's BlockReceiver), so appends take
// only that buffer's state, not the context lock: receivers of different blocks copy in parallel.
// (touches only the receive buffer and stream C, so it runs without the context lock; the caller
// records an error under the lock)
static hipStream_t rx_stream(hdrf_ctx *ctx, const hdrf_ctx::Rx &r) { return r.st ? r.st : ctx->stC; }

// Packet bytes into the pinned staging chunk with non-temporal 16-B stores: the receiver thread does
// not read the destination lines first (a plain copy of a 64 KiB packet fetches them for ownership)
// and leaves nothing dirty in its caches for the copy engine's reads.  HDRF_RX_NT=0: std::memcpy.
static void copy_nt(uint8_t *dst, const uint8_t *src, uint64_t n)
{
    typedef long long v2 __attribute__((vector_size(16)));
    uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
    if (head > n) head = n;
    std::memcpy(dst, src, head);
    dst += head;
    src += head;
    n -= head;
    const uint64_t n64 = n >> 6;
    for (uint64_t i = 0; i < n64; i++) {
        v2 a, b, c, d;
        std::memcpy(&a, src + 64 * i, 16);
        std::memcpy(&b, src + 64 * i + 16, 16);
        std::memcpy(&c, src + 64 * i + 32, 16);
        std::memcpy(&d, src + 64 * i + 48, 16);
        __builtin_nontemporal_store(a, (v2 *)(dst + 64 * i));
        __builtin_nontemporal_store(b, (v2 *)(dst + 64 * i + 16));
        __builtin_nontemporal_store(c, (v2 *)(dst + 64 * i + 32));
        __builtin_nontemporal_store(d, (v2 *)(dst + 64 * i + 48));
    }
    std::memcpy(dst + 64 * n64, src + 64 * n64, n & 63);
    // Non-temporal stores are weakly ordered: fence them here, on the thread that wrote them, so
    // the staged bytes are visible before any later store of this thread (the hand-off of the block
    // to another thread that queues its last chunk's copy, e.g. hdrf_submit_slots from a submitter).
#if !defined(__HIP_DEVICE_COMPILE__)
    __builtin_ia32_sfence();
#endif
}

static bool rx_nt()
{
    static const bool on = env_int("HDRF_RX_NT", 1) != 0;
    return on;
}

static hipError_t rx_flush(hdrf_ctx *ctx, hdrf_ctx::Rx &r)
{
    if (r.fill == 0) return hipSuccess;
    const int c = r.cur;
    // the chunk's non-temporal stores are globally visible before the copy engine is told to read it
    std::atomic_thread_fence(std::memory_order_seq_cst);
    hipError_t e = hipMemcpyAsync(r.d + r.dst, r.h + (uint64_t)c * ctx->kRingChunk, r.fill, hipMemcpyHostToDevice,
                                  rx_stream(ctx, r));
    if (e == hipSuccess) e = hipEventRecord(r.ev[c], rx_stream(ctx, r));
    if (e != hipSuccess) return e;
    r.busy[c] = true;
    r.cur = c ^ 1;
    r.fill = 0;
    if (r.busy[r.cur]) {                               // refilling that chunk: its copy must have landed
        if ((e = hipEventSynchronize(r.ev[r.cur])) != hipSuccess) return e;
        r.busy[r.cur] = false;
    }
    return hipSuccess;
}

extern "C" int hdrf_rx_begin(hdrf_ctx *ctx, uint64_t block_id, int32_t *rx)
{
    HDRF_LOCK(ctx);
    if (!ctx || !rx) return HDRF_E_INVAL;
    if (ctx->G > 1) return set_err(ctx, HDRF_E_INVAL, "node-global context: use the hdrf_gx_* phases");
    for (int i = 0; i < hdrf_ctx::kRx; i++) {
        hdrf_ctx::Rx &r = ctx->rx[i];
        if (r.state.load() != 0) continue;
        if (!r.d) HIPCK(hipMalloc((void **)&r.d, (uint64_t)ctx->cfg.max_block_bytes + kSlack + 256));
        if (!r.h) {
            HIPCK(hipHostMalloc((void **)&r.h, 2 * ctx->kRingChunk));
            for (auto &e : r.ev) HIPCK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            static const bool own = env_int("HDRF_RX_STREAMS", 0) != 0;
            if (own) {
                HIPCK(hipStreamCreateWithFlags(&r.st, hipStreamNonBlocking));
                HIPCK(hipEventCreateWithFlags(&r.done, hipEventDisableTiming));
            }
        }
        r.len = 0;
        r.fill = 0;
        r.dst = 0;
        r.id = block_id;
        r.state.store(1);
        ctx->rx_used = true;                       // packet mode: drains on the copy engine
        ctx->host_copies = true;
        *rx = i;
        return 0;
    }
    return set_err(ctx, HDRF_E_CAPACITY, "every receive buffer holds a block being received or reduced (hdrf_wait_batch)");
}

extern "C" int hdrf_append_packet(hdrf_ctx *ctx, int32_t rx, const uint8_t *data, uint64_t len)
{
    if (!ctx) return HDRF_E_INVAL;
    if (rx < 0 || rx >= hdrf_ctx::kRx || ctx->rx[rx].state.load() != 1 || (len && !data)) {
        HDRF_LOCK(ctx);
        return set_err(ctx, HDRF_E_INVAL, "bad receive buffer or packet");
    }
    hdrf_ctx::Rx &r = ctx->rx[rx];
    if (len > (uint64_t)ctx->cfg.max_block_bytes - r.len) {       // r.len <= max_block_bytes: no wrap
        HDRF_LOCK(ctx);
        return set_err(ctx, HDRF_E_INVAL, "block larger than max_block_bytes");
    }
    while (len) {
        if (r.fill == 0) r.dst = r.len;
        const uint64_t n = std::min(len, ctx->kRingChunk - r.fill);
        if (rx_nt()) copy_nt(r.h + (uint64_t)r.cur * ctx->kRingChunk + r.fill, data, n);
        else std::memcpy(r.h + (uint64_t)r.cur * ctx->kRingChunk + r.fill, data, n);
        r.fill += n;
        r.len += n;
        data += n;
        len -= n;
        if (r.fill == ctx->kRingChunk) {
            const hipError_t e = rx_flush(ctx, r);
            if (e != hipSuccess) {
                HDRF_LOCK(ctx);
                return set_err(ctx, HDRF_E_HIP, std::string("packet copy: ") + hipGetErrorString(e));
            }
        }
    }
    return 0;
}

// A receive the DataNode abandons (client lost mid-block: the reference drops bf1): the buffer's
// staging copies are waited for and the buffer is free again.  The receiver thread must have
// stopped appending to it.
extern "C" int hdrf_rx_cancel(hdrf_ctx *ctx, int32_t rx)
{
    HDRF_LOCK(ctx);
    if (!ctx || rx < 0 || rx >= hdrf_ctx::kRx || ctx->rx[rx].state.load() != 1)
        return ctx ? set_err(ctx, HDRF_E_INVAL, "bad receive buffer (not receiving)") : HDRF_E_INVAL;
    hdrf_ctx::Rx &r = ctx->rx[rx];
    for (int c = 0; c < 2; c++)
        if (r.busy[c]) {
            HIPCK(hipEventSynchronize(r.ev[c]));
            r.busy[c] = false;
        }
    r.len = r.fill = r.dst = 0;
    r.cur = 0;
    r.state.store(0);
    return 0;
}

// n received blocks (receive buffers in arrival order) as ONE batch: the DataNode hands over every
// block whose last packet has arrived since its previous submit, so the batch's kernels, index and
// store passes are shared by those blocks instead of running once per block.
extern "C" int hdrf_submit_slots(hdrf_ctx *ctx, int32_t n, const int32_t *rxs)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (n < 1 || n > ctx->max_batch || !rxs) return set_err(ctx, HDRF_E_INVAL, "bad receive-buffer list");
    uint32_t mask = 0;
    for (int i = 0; i < n; i++) {
        const int32_t rx = rxs[i];
        if (rx < 0 || rx >= hdrf_ctx::kRx || ctx->rx[rx].state.load() != 1 || (mask >> rx & 1))
            return set_err(ctx, HDRF_E_INVAL, "bad receive buffer");
        mask |= 1u << rx;
    }
    if (ctx->nsub - ctx->nwait >= (uint64_t)kSlots)     // every submit pairs with one hdrf_wait_batch
        return set_err(ctx, HDRF_E_CAPACITY, "pipeline full: hdrf_wait_batch first");
    std::vector<const uint8_t *> p(n);
    std::vector<uint64_t> len(n), readable(n), id(n);
    for (int i = 0; i < n; i++) {
        hdrf_ctx::Rx &r = ctx->rx[rxs[i]];
        HIPCK(rx_flush(ctx, r));
        // (no slack fill: the kernels never depend on the bytes past a block's end, as for caller
        // buffers, and a fill kernel on the copy stream waited for CU slots and stalled the copies)
        if (r.st) {                                    // the batch's copies complete on stream C's clock
            HIPCK(hipEventRecord(r.done, r.st));
            HIPCK(hipStreamWaitEvent(ctx->stC, r.done, 0));
        }
        p[i] = r.d;
        len[i] = r.len;
        readable[i] = (uint64_t)ctx->cfg.max_block_bytes + kSlack + 256;
        id[i] = r.id;
    }
    Slot &S = ctx->sl[ctx->nsub % kSlots];
    HIPCK(hipEventRecord(S.copy_done, ctx->stC));
    if (int rc = submit(ctx, n, p.data(), len.data(), readable.data(), id.data(), true)) return rc;
    S.rx_release = mask;
    for (int i = 0; i < n; i++) ctx->rx[rxs[i]].state = 2;
    return 0;
}

extern "C" int hdrf_submit_slot(hdrf_ctx *ctx, int32_t rx)
{
    return hdrf_submit_slots(ctx, 1, &rx);
}
