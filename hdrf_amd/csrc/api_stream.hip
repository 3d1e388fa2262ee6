// api_stream.hip — libhdrf C-ABI: the stream codecs 0 (SnappyCodec), 3 (LzopCodec), 4 (Lz4Codec) and
// 5 (GzipCodec), write side (hdrf_stream_block*) and read side (hdrf_*_file_decode), and the two gzip
// stage probes.
//
// Every entry point drains the pipeline and works on stream A.  Writes only the grown scratch
// buffers (d_rd / rd_cap, d_stage / stage_cap), a streamed block's length (ctx->lengths) and
// lzop_mtime.
#include "ctx.hpp"

// Stream mode (compressor 4 / 0, DN/BlockReceiver.java:826-873,887-894,1238-1256): the block as
// codec.createOutputStream(file).write(packet) per received packet, then close().  The
// BlockCompressorStream decisions (hadoop-common 3.1.0) depend only on the write sizes, so the
// host plans the pieces (groups of buffered packets, or <= MAX_INPUT slices of one large write)
// and the GPU compresses all pieces of the block at once (one wave per piece), then frames them.
// BlockCompressorStream MAX_INPUT = bufferSize - compressionOverhead (256 KiB buffers): Lz4Codec
// overhead bufferSize/255 + 16, SnappyCodec bufferSize/6 + 32 (hadoop-common 3.1.0)
static int64_t stream_max_input(int codec)
{
    if (codec == 3) return 262144 - ((262144 >> 4) + 64 + 3);    // hadoop-lzo LzopOutputStream (LZO1X)
    return codec == 0 ? 262144 - (262144 / 6 + 32) : 262144 - (262144 / 255 + 16);
}

// hadoop-lzo LzopOutputStream.writeLzopHeader: magic, {version 0x1010, LZO library version 0x20a0
// (LZO 2.10), compat 0x0940, LZO1X_1 = method 1 / level 5, flags 0, mode 0x81a4, mtime, gmtdiff 0,
// no file name} and its Adler-32 (the reference's mtime is the wall clock: hdrf_set_lzop_mtime)
static size_t lzop_header(uint32_t mtime, uint8_t *dst)
{
    static const uint8_t magic[9] = {0x89, 'L', 'Z', 'O', 0x00, 0x0d, 0x0a, 0x1a, 0x0a};
    uint8_t h[25] = {0x10, 0x10, 0x20, 0xa0, 0x09, 0x40, 1, 5, 0, 0, 0, 0, 0, 0, 0x81, 0xa4,
                     (uint8_t)(mtime >> 24), (uint8_t)(mtime >> 16), (uint8_t)(mtime >> 8), (uint8_t)mtime, 0, 0, 0, 0, 0};
    uint32_t a = 1, b = 0;
    for (uint8_t c : h) { a = (a + c) % 65521u; b = (b + a) % 65521u; }
    const uint32_t ck = (b << 16) | a;
    std::memcpy(dst, magic, 9);
    std::memcpy(dst + 9, h, 25);
    dst[34] = (uint8_t)(ck >> 24); dst[35] = (uint8_t)(ck >> 16); dst[36] = (uint8_t)(ck >> 8); dst[37] = (uint8_t)ck;
    return 38;
}

// Stream-mode compressor 5 (GzipCodec, zlib level 6; DN/BlockReceiver.java:858-873,887-894): the
// file does not depend on the packet writes.  Stage 1 match pass, stage 2 lazy
// parse, stage 3 per-deflate-block trees + bits, stage 4 offsets / placement / CRC-32 trailer.
static int64_t stream_gzip(hdrf_ctx *ctx, uint64_t block_id, const uint8_t *dev_data, uint64_t len, uint8_t *out,
                           int64_t cap)
{
    if (len >= (1ull << 31)) return set_err(ctx, HDRF_E_INVAL, "gzip stream: len must be < 2^31");
    if (int rc = drain(ctx)) return rc;
    hipStream_t st = ctx->st;
    const int64_t n = (int64_t)len, maxblk = n / 16383 + 2, slot = 16384 * 6 + 2048;
    const int64_t bound = n + (n >> 3) + 1024;
    const size_t sz[] = {(size_t)(4 * n + 64), (size_t)(4 * n + 64), (size_t)(4 * n + 64), (size_t)(4 * n + 68),
                         (size_t)(40 * maxblk + 64), 64, gzip_tab_bytes(), gzip_block_state_bytes() * (size_t)maxblk,
                         (size_t)(slot * maxblk), (size_t)(24 * maxblk + 64), (size_t)(8 * maxblk + 72),
                         (size_t)(4 * ((n >> 16) + 2)), (size_t)(bound + 64), gzip_parse_scratch(n)};
    constexpr int kBufs = 14;
    uint64_t at[kBufs + 1] = {0};                      // one grown scratch (ctx->d_rd), 256-B aligned parts
    for (int i = 0; i < kBufs; i++) at[i + 1] = at[i] + ((sz[i] + 255) & ~(size_t)255);
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, at[kBufs])) return rc;
    uint8_t *B[kBufs];
    for (int i = 0; i < kBufs; i++) B[i] = ctx->d_rd + at[i];
    std::vector<uint8_t> tab(gzip_tab_bytes());
    gzip_host_tab(tab.data());
    int64_t cnt[2] = {0, 0}, flen = 0;
    hipError_t e = hipMemcpyAsync(B[6], tab.data(), tab.size(), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(B[12], 0, sz[12], st);
    if (e == hipSuccess) e = launch_gzip_match(dev_data, n, (uint32_t *)B[0], (uint32_t *)B[1], (uint32_t *)B[2], st);
    if (e == hipSuccess)
        e = launch_gzip_parse(dev_data, n, (const uint32_t *)B[1], (const uint32_t *)B[2], (uint32_t *)B[3],
                              (int64_t *)B[4], (int64_t *)B[5], B[13], st);
    if (e == hipSuccess) e = hipMemcpyAsync(cnt, B[5], 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess && (cnt[1] < 1 || cnt[1] > maxblk)) { return set_err(ctx, HDRF_E_DEVICE, "gzip parse block count"); }
    if (e == hipSuccess)
        e = launch_gzip_encode(dev_data, n, B[6], (const uint32_t *)B[3], (const int64_t *)B[4], (int)cnt[1], B[7], B[8],
                               slot, (int64_t *)B[9], (int64_t *)B[10], (uint32_t *)B[11], B[12], (int64_t *)B[5], st);
    if (e == hipSuccess) e = hipMemcpyAsync(&flen, B[5], 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { return set_err(ctx, HDRF_E_HIP, std::string("gzip stream: ") + hipGetErrorString(e)); }
    if (flen > bound) { return set_err(ctx, HDRF_E_DEVICE, "gzip stream exceeded its bound"); }
    if (!out || cap < flen) { return set_err(ctx, HDRF_E_CAPACITY, "stream file needs " + std::to_string(flen) + " bytes"); }
    e = hipMemcpy(out, B[12], (size_t)flen, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return set_err(ctx, HDRF_E_HIP, "gzip D2H");
    ctx->lengths[(uint32_t)block_id] = (int64_t)len;   // SET id -> BE32(len) (:1238-1256)
    return flen;
}

extern "C" int64_t hdrf_stream_block(hdrf_ctx *ctx, int32_t codec, uint64_t block_id, const uint8_t *dev_data,
                                     uint64_t len, uint64_t readable, const uint64_t *writes, int32_t nwrites,
                                     uint8_t *out, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (codec != 4 && codec != 0 && codec != 5 && codec != 3)
        return set_err(ctx, HDRF_E_UNSUPPORTED, "stream codec: 0 (SnappyCodec), 3 (LzopCodec), 4 (Lz4Codec) and 5 (GzipCodec)");
    if (nwrites < 0 || (nwrites && !writes) || (len && !dev_data) || readable < len + kSlack)
        return set_err(ctx, HDRF_E_INVAL, "bad stream arguments (readable must be >= len + 64)");
    if (codec == 5) {
        uint64_t sum = 0;
        for (int w = 0; w < nwrites; w++) sum += writes[w];
        if (sum != len) return set_err(ctx, HDRF_E_INVAL, "write sizes do not add up to the block length");
        return stream_gzip(ctx, block_id, dev_data, len, out, cap);
    }
    const int64_t kMaxIn = stream_max_input(codec);     // BlockCompressorStream MAX_INPUT_SIZE
    std::vector<LzPiece> pieces;
    std::vector<LzOut> outs;
    uint64_t off = 0, gs = 0, lim = 0;
    auto piece = [&](uint64_t src, uint64_t n, uint32_t hval, uint32_t hlen) {
        pieces.push_back(LzPiece{src, (uint32_t)n, 0});
        outs.push_back(LzOut{0, hval, hlen});
    };
    const bool lzop = codec == 3;
    for (int w = 0; w < nwrites; w++) {
        const uint64_t n = writes[w];
        if (lzop && n == 0) continue;
        if (lim > 0 && n + lim > (uint64_t)kMaxIn) { piece(gs, lim, (uint32_t)lim, 4); lim = 0; }   // finish()
        if (n > (uint64_t)kMaxIn) {                                                               // segmented write
            for (uint64_t o = 0; o < n; o += kMaxIn) {
                const uint64_t sl = std::min<uint64_t>(kMaxIn, n - o);
                // Lz4Codec/SnappyCodec: one BE32 raw length for the whole write; LZOP: every slice
                // is its own block [BE32 raw][BE32 stored]
                if (lzop) piece(off + o, sl, (uint32_t)sl, 4u);
                else piece(off + o, sl, (uint32_t)n, o == 0 ? 4u : 0u);
            }
            off += n;
            continue;
        }
        if (lim == 0) gs = off;
        lim += n;
        off += n;
    }
    if (off != len) return set_err(ctx, HDRF_E_INVAL, "write sizes do not add up to the block length");
    const bool trailer = lzop || lim == 0;             // close(): BE32 0 when nothing is buffered (LZOP: always)
    if (lim > 0) piece(gs, lim, (uint32_t)lim, 4);
    const int n = (int)pieces.size();
    const uint64_t stride = lzop ? lzo_piece_stride() : lz4_piece_stride();
    const uint64_t a_pieces = 0, a_outs = ((uint64_t)n * sizeof(LzPiece) + 255) & ~255ull;
    const uint64_t a_clen = a_outs + (((uint64_t)n * sizeof(LzOut) + 255) & ~255ull);
    const uint64_t a_stage = a_clen + (((uint64_t)n * 4 + 255) & ~255ull);
    const uint64_t a_file = a_stage + (((uint64_t)n * stride + 255) & ~255ull);   // keeps later arrays aligned
    // snappy: every group split into independent 64 KiB fragments (pieces[i].pad = first one)
    std::vector<LzPiece> frags;
    if (codec == 0)
        for (int i = 0; i < n; i++) {
            pieces[i].pad = (uint32_t)frags.size();
            for (uint64_t o = 0; o < pieces[i].len; o += 65536)
                frags.push_back(LzPiece{pieces[i].src + o, (uint32_t)std::min<uint64_t>(65536, pieces[i].len - o), 0});
        }
    const int nf = (int)frags.size();
    const uint64_t a_frags = a_file + (((uint64_t)n * (stride + 8) + 16 + 255) & ~255ull);
    const uint64_t a_fclen = a_frags + (((uint64_t)nf * sizeof(LzPiece) + 255) & ~255ull);
    const uint64_t a_fscr = a_fclen + (((uint64_t)nf * 4 + 255) & ~255ull);
    const uint64_t need = a_fscr + (uint64_t)nf * snappy_frag_stride() + 16;
    if (int rc = drain(ctx)) return rc;
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, need)) return rc;
    uint8_t *R = ctx->d_rd;
    hipStream_t st = ctx->st;
    std::vector<uint32_t> clen(n);
    if (n) {
        HIPCK(hipMemcpyAsync(R + a_pieces, pieces.data(), n * sizeof(LzPiece), hipMemcpyHostToDevice, st));
        if (codec == 4) {
            HIPCK(launch_lz4_stream((const LzPiece *)(R + a_pieces), n, dev_data, R + a_stage, (uint32_t *)(R + a_clen), st));
        } else if (codec == 3) {
            HIPCK(launch_lzo_stream((const LzPiece *)(R + a_pieces), n, dev_data, R + a_stage, (uint32_t *)(R + a_clen), st));
        } else {
            if (nf) HIPCK(hipMemcpyAsync(R + a_frags, frags.data(), nf * sizeof(LzPiece), hipMemcpyHostToDevice, st));
            HIPCK(launch_snappy_stream((const LzPiece *)(R + a_pieces), n, (const LzPiece *)(R + a_frags), nf, dev_data,
                                       R + a_fscr, (uint32_t *)(R + a_fclen), R + a_stage, stride,
                                       (uint32_t *)(R + a_clen), st));
        }
        HIPCK(hipMemcpyAsync(clen.data(), R + a_clen, n * 4, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
    }
    uint8_t hdr[64];
    const uint64_t hlen = lzop ? lzop_header(ctx->lzop_mtime, hdr) : 0;
    uint64_t pos = hlen;
    for (int i = 0; i < n; i++) {
        outs[i].dst = pos;
        pos += outs[i].hlen + 4 + clen[i];
    }
    const int64_t total = (int64_t)pos + (trailer ? 4 : 0);
    if (!out || cap < total) return set_err(ctx, HDRF_E_CAPACITY, "stream file needs " + std::to_string(total) + " bytes");
    if (hlen) std::memcpy(out, hdr, hlen);
    if (n) {
        HIPCK(hipMemcpyAsync(R + a_outs, outs.data(), n * sizeof(LzOut), hipMemcpyHostToDevice, st));
        HIPCK(launch_lz4_emit((const LzOut *)(R + a_outs), n, R + a_stage, (const uint32_t *)(R + a_clen), R + a_file, st));
        HIPCK(hipMemcpyAsync(out + hlen, R + a_file + hlen, pos - hlen, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
    }
    if (trailer) std::memset(out + pos, 0, 4);
    ctx->lengths[(uint32_t)block_id] = (int64_t)len;   // SET id -> BE32(len) (:1238-1256)
    return total;
}

// The same for a host-resident block (the DataNode's received bytes): staged H2D, then streamed
extern "C" int64_t hdrf_stream_block_host(hdrf_ctx *ctx, int32_t codec, uint64_t block_id, const uint8_t *data,
                                          uint64_t len, const uint64_t *writes, int32_t nwrites, uint8_t *out,
                                          int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx || (len && !data)) return HDRF_E_INVAL;
    if (codec != 4 && codec != 0 && codec != 5 && codec != 3)
        return set_err(ctx, HDRF_E_UNSUPPORTED, "stream codec: 0 (SnappyCodec), 3 (LzopCodec), 4 (Lz4Codec) and 5 (GzipCodec)");
    if (int rc = drain(ctx)) return rc;
    if (int rc = grow(ctx, &ctx->d_stage, &ctx->stage_cap, len + kSlack)) return rc;
    if (len) HIPCK(hipMemcpy(ctx->d_stage, data, len, hipMemcpyHostToDevice));
    return hdrf_stream_block(ctx, codec, block_id, ctx->d_stage, len, len + kSlack, writes, nwrites, out, cap);
}

// Hadoop codec file (BlockCompressorStream framing: [BE32 raw] ([BE32 clen] block)* groups)
// -> the compressed blocks it holds.  A group's raw length is sliced at the codec's MAX_INPUT
// (Lz4Codec 261,100, SnappyCodec 218,422), exactly as the stream wrote it; false if malformed.
bool host::plan_lz4_frame(const uint8_t *f, int64_t n, std::vector<LzDec> &items, uint64_t *raw_total, int codec)
{
    const uint64_t kMaxIn = (uint64_t)stream_max_input(codec);
    auto be32 = [&](int64_t i) { return ((uint64_t)f[i] << 24) | ((uint64_t)f[i + 1] << 16) | ((uint64_t)f[i + 2] << 8) | f[i + 3]; };
    int64_t i = 0;
    uint64_t o = 0;
    items.clear();
    while (i + 4 <= n) {
        const uint64_t total = be32(i);
        i += 4;
        uint64_t got = 0;
        while (got < total) {
            if (i + 4 > n) return false;
            const uint64_t c = be32(i);
            i += 4;
            if (i + (int64_t)c > n) return false;
            const uint64_t raw = std::min(kMaxIn, total - got);
            items.push_back(LzDec{(uint64_t)i, o + got, (uint32_t)c, (uint32_t)raw});
            i += (int64_t)c;
            got += raw;
        }
        o += total;
    }
    *raw_total = o;
    return i == n;
}

// decode a host-resident Lz4Codec file into device memory (dev_out, cap bytes); returns raw length
int64_t host::decode_file(hdrf_ctx *ctx, const uint8_t *file, int64_t flen, uint8_t *dev_out, int64_t cap, int codec)
{
    std::vector<LzDec> items;
    uint64_t raw = 0;
    if (flen < 0 || (flen && !file) || !plan_lz4_frame(file, flen, items, &raw, codec))
        return set_err(ctx, HDRF_E_INVAL, codec == 4 ? "malformed Lz4Codec frame" : "malformed SnappyCodec frame");
    if ((int64_t)raw > cap || (raw && !dev_out)) return set_err(ctx, HDRF_E_CAPACITY, "output capacity");
    if (items.empty()) return (int64_t)raw;
    const int n = (int)items.size();
    const uint64_t o_items = 0, o_err = ((uint64_t)n * sizeof(LzDec) + 255) & ~255ull, o_file = o_err + 256;
    if (int rc = drain(ctx)) return rc;
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, o_file + (uint64_t)flen + 64)) return rc;
    uint8_t *R = ctx->d_rd;
    hipStream_t st = ctx->st;
    HIPCK(hipMemcpyAsync(R + o_file, file, (size_t)flen, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(R + o_items, items.data(), (size_t)n * sizeof(LzDec), hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(R + o_err, 0, 4, st));
    if (codec == 4) HIPCK(launch_lz4_decode((const LzDec *)(R + o_items), n, R + o_file, dev_out, (int *)(R + o_err), st));
    else HIPCK(launch_snappy_decode((const LzDec *)(R + o_items), n, R + o_file, dev_out, (int *)(R + o_err), st));
    int err = 0;
    HIPCK(hipMemcpyAsync(&err, R + o_err, 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (err) return set_err(ctx, HDRF_E_INVAL, codec == 4 ? "corrupt LZ4 block in the Lz4Codec file"
                                                          : "corrupt snappy block in the SnappyCodec file");
    return (int64_t)raw;
}

// ---- LzopCodec read side (DN/DataConstructor.java:140-166): LzopInputStream ----------------
// header (magic, method LZO1X, Adler-32 / CRC-32 flags, optional file name; the header checksum is
// checked), then blocks [BE32 raw][BE32 stored][checksums per the flags][bytes] up to BE32 0; one
// wave per block decodes on the GPU (lzo.hip), stored == raw means the bytes are raw
static int64_t decode_lzop(hdrf_ctx *ctx, const uint8_t *f, int64_t n, uint8_t *dev_out, int64_t cap)
{
    static const uint8_t magic[9] = {0x89, 'L', 'Z', 'O', 0x00, 0x0d, 0x0a, 0x1a, 0x0a};
    auto be32 = [&](int64_t i) { return ((uint32_t)f[i] << 24) | ((uint32_t)f[i + 1] << 16) | ((uint32_t)f[i + 2] << 8) | f[i + 3]; };
    if (n < 9 + 29 || !f || std::memcmp(f, magic, 9) != 0) return set_err(ctx, HDRF_E_INVAL, "not an lzop file");
    const uint8_t *h = f + 9;
    const uint32_t flags = be32(9 + 8);
    const int fname = h[24];
    if ((h[6] != 1 && h[6] != 2 && h[6] != 3) || (flags & 0x40)) return set_err(ctx, HDRF_E_INVAL, "unsupported lzop header");
    int64_t pos = 9 + 25 + fname;
    if (pos + 4 > n) return set_err(ctx, HDRF_E_INVAL, "truncated lzop header");
    uint32_t a = 1, b = 0;
    for (int i = 0; i < 25 + fname; i++) { a = (a + h[i]) % 65521u; b = (b + a) % 65521u; }
    if (be32(pos) != ((b << 16) | a)) return set_err(ctx, HDRF_E_INVAL, "lzop header checksum mismatch");
    pos += 4;
    const int dck = ((flags & 1) != 0) + ((flags & 0x100) != 0), cck = ((flags & 2) != 0) + ((flags & 0x200) != 0);
    std::vector<LzDec> items;
    uint64_t raw = 0;
    for (;;) {
        if (pos + 4 > n) return set_err(ctx, HDRF_E_INVAL, "truncated lzop file");
        const uint32_t ul = be32(pos);
        pos += 4;
        if (ul == 0) break;
        if (pos + 4 > n) return set_err(ctx, HDRF_E_INVAL, "truncated lzop file");
        const uint32_t cl = be32(pos);
        pos += 4 + 4 * (int64_t)dck + (cl < ul ? 4 * (int64_t)cck : 0);
        if (cl > ul || pos + cl > n) return set_err(ctx, HDRF_E_INVAL, "malformed lzop block");
        items.push_back(LzDec{(uint64_t)pos, raw, cl, ul});
        pos += cl;
        raw += ul;
    }
    if (pos != n) return set_err(ctx, HDRF_E_INVAL, "bytes after the lzop end marker");
    if ((int64_t)raw > cap || (raw && !dev_out)) return set_err(ctx, HDRF_E_CAPACITY, "output capacity");
    if (items.empty()) return 0;
    const int m = (int)items.size();
    const uint64_t o_items = 0, o_err = ((uint64_t)m * sizeof(LzDec) + 255) & ~255ull, o_file = o_err + 256;
    if (int rc = drain(ctx)) return rc;
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, o_file + (uint64_t)n + 64)) return rc;
    uint8_t *R = ctx->d_rd;
    hipStream_t st = ctx->st;
    HIPCK(hipMemcpyAsync(R + o_file, f, (size_t)n, hipMemcpyHostToDevice, st));
    HIPCK(hipMemcpyAsync(R + o_items, items.data(), (size_t)m * sizeof(LzDec), hipMemcpyHostToDevice, st));
    HIPCK(hipMemsetAsync(R + o_err, 0, 4, st));
    HIPCK(launch_lzo_decode((const LzDec *)(R + o_items), m, R + o_file, dev_out, (int *)(R + o_err), st));
    int err = 0;
    HIPCK(hipMemcpyAsync(&err, R + o_err, 4, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    if (err) return set_err(ctx, HDRF_E_INVAL, "corrupt LZO1X block in the lzop file");
    return (int64_t)raw;
}

// ---- GzipCodec read side (DN/DataConstructor.java:194-218) -----------------------------------
// CRC-32 combination over GF(2) (zlib's crc32_combine: the CRC of A||B from crc(A), crc(B), |B|)
static uint32_t gf2_times(const uint32_t *mat, uint32_t vec)
{
    uint32_t sum = 0;
    for (int i = 0; vec; vec >>= 1, i++)
        if (vec & 1) sum ^= mat[i];
    return sum;
}
static void gf2_square(uint32_t *sq, const uint32_t *mat)
{
    for (int n = 0; n < 32; n++) sq[n] = gf2_times(mat, mat[n]);
}
// the operator "append len2 zero bytes" as a 32x32 matrix (columns)
static void crc_shift_op(uint32_t *op, int64_t len2)
{
    uint32_t odd[32], even[32];
    odd[0] = 0xEDB88320u;                     // x^1 (one zero bit)
    uint32_t row = 1;
    for (int n = 1; n < 32; n++) { odd[n] = row; row <<= 1; }
    gf2_square(even, odd);                    // 2 bits
    gf2_square(odd, even);                    // 4 bits
    for (int n = 0; n < 32; n++) op[n] = 1u << n;     // identity
    uint32_t *cur = odd, *nxt = even;         // cur: the operator for 8 * 2^k bits as k grows
    // start at one byte: square twice more (8 bits)
    gf2_square(nxt, cur);                     // 8 bits in nxt
    std::swap(cur, nxt);
    while (len2) {
        if (len2 & 1) {
            uint32_t t[32];
            for (int n = 0; n < 32; n++) t[n] = gf2_times(cur, op[n]);
            std::memcpy(op, t, sizeof t);
        }
        len2 >>= 1;
        if (!len2) break;
        gf2_square(nxt, cur);
        std::swap(cur, nxt);
    }
}
static uint32_t crc_combine_op(const uint32_t *op, uint32_t crc1, uint32_t crc2) { return gf2_times(op, crc1) ^ crc2; }

static int64_t decode_gzip(hdrf_ctx *ctx, const uint8_t *file, int64_t flen, uint8_t *dev_out, int64_t cap)
{
    if (flen < 0 || (flen && !file) || cap < 0 || (cap && !dev_out)) return set_err(ctx, HDRF_E_INVAL, "bad buffers");
    if (flen == 0) return 0;                  // an empty file decodes to nothing
    if (int rc = drain(ctx)) return rc;
    constexpr int64_t kPiece = 1 << 16;       // crc32_piece_kernel's piece
    hipStream_t st = ctx->st;
    uint32_t piece_op[32];
    crc_shift_op(piece_op, kPiece);
    CrcOp op1k;
    crc_shift_op(op1k.m, 1024);
    int64_t at = 0, out = 0;
    std::vector<uint32_t> crcs;
    while (at < flen) {
        // gzip member header (RFC 1952): ID1 ID2 CM FLG MTIME(4) XFL OS [XLEN extra] [name\0] [comment\0] [CRC16]
        if (flen - at < 18 || file[at] != 0x1f || file[at + 1] != 0x8b || file[at + 2] != 8)
            return set_err(ctx, HDRF_E_INVAL, "not a gzip member at offset " + std::to_string(at));
        const uint8_t flg = file[at + 3];
        int64_t h = at + 10;
        if (flg & 4) { if (h + 2 > flen) return set_err(ctx, HDRF_E_INVAL, "gzip header"); h += 2 + (file[h] | (file[h + 1] << 8)); }
        if (flg & 8) { while (h < flen && file[h]) h++; h++; }
        if (flg & 16) { while (h < flen && file[h]) h++; h++; }
        if (flg & 2) h += 2;
        if (h > flen) return set_err(ctx, HDRF_E_INVAL, "gzip header");
        // ---- 1. speculative chunk starts + per-chunk decode counts (inflate.hip) ----------------
        const int64_t slen = flen - h, nch = inflate_chunks(slen);
        const uint64_t o_file = 0, o_st = (o_file + (uint64_t)slen + 64 + 255) & ~255ull;
        const uint64_t o_info = o_st + (((uint64_t)nch * 8 + 255) & ~255ull);
        const uint64_t o_job = o_info + (((uint64_t)nch * 32 + 255) & ~255ull);
        const uint64_t o_misc = o_job + (((uint64_t)nch * 40 + 255) & ~255ull);
        const uint64_t o_crc = o_misc + 256, o_scr = (o_crc + 4 * ((uint64_t)(cap - out) / kPiece + 2) + 255) & ~255ull;
        if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, o_scr + 256)) return rc;
        uint8_t *R = ctx->d_rd;
        HIPCK(hipMemcpyAsync(R + o_file, file + h, (size_t)slen, hipMemcpyHostToDevice, st));
        HIPCK(launch_inflate_find(R + o_file, slen, (int64_t *)(R + o_st), (int64_t *)(R + o_info), st));
        std::vector<int64_t> starts((size_t)nch), info((size_t)nch * 4);
        HIPCK(hipMemcpyAsync(starts.data(), R + o_st, 8 * (size_t)nch, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(info.data(), R + o_info, 32 * (size_t)nch, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        // ---- 2. the chain of real block boundaries from chunk 0; output offsets ----------------
        std::vector<int64_t> jobs;
        int64_t n = 0, end_bit = -1;
        for (int64_t c = 0; c < nch;) {
            const int64_t *f = &info[(size_t)c * 4];
            if (f[2] < 0 || (f[2] <= c && !f[3])) return set_err(ctx, HDRF_E_INVAL, "corrupt deflate stream");
            jobs.insert(jobs.end(), {starts[(size_t)c], f[1], n, f[0], c});
            n += f[0];
            if (f[3]) { end_bit = f[1]; break; }
            c = f[2];
        }
        if (end_bit < 0) return set_err(ctx, HDRF_E_INVAL, "deflate stream without a final block");
        if (n > cap - out) return set_err(ctx, HDRF_E_CAPACITY, "output capacity");
        const int64_t end = h + (end_bit + 7) / 8;
        if (end + 8 > flen) return set_err(ctx, HDRF_E_INVAL, "gzip trailer missing");
        const uint32_t want_crc = (uint32_t)file[end] | ((uint32_t)file[end + 1] << 8) | ((uint32_t)file[end + 2] << 16) |
                                  ((uint32_t)file[end + 3] << 24);
        const uint32_t isize = (uint32_t)file[end + 4] | ((uint32_t)file[end + 5] << 8) | ((uint32_t)file[end + 6] << 16) |
                               ((uint32_t)file[end + 7] << 24);
        if (isize != (uint32_t)n) return set_err(ctx, HDRF_E_INVAL, "gzip ISIZE mismatch");
        // ---- 3. decode the chain's chunks in parallel, resolve cross-chunk window bytes --------
        if (n > 0) {
            const int nj = (int)(jobs.size() / 5);
            if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, o_scr + 4 * (uint64_t)n + 256)) return rc;
            if (ctx->d_rd != R) {                      // regrown: the file copy moves with it
                R = ctx->d_rd;
                HIPCK(hipMemcpyAsync(R + o_file, file + h, (size_t)slen, hipMemcpyHostToDevice, st));
            }
            uint32_t *scr = (uint32_t *)(R + o_scr);
            int *d_err = (int *)(R + o_misc);
            unsigned int *d_left = (unsigned int *)(R + o_misc + 8);
            HIPCK(hipMemcpyAsync(R + o_job, jobs.data(), 8 * jobs.size(), hipMemcpyHostToDevice, st));
            HIPCK(hipMemsetAsync(R + o_misc, 0, 16, st));
            HIPCK(launch_inflate_write(R + o_file, slen, (const int64_t *)(R + o_job), nj, scr, cap - out, d_err, st));
            int herr = 0;
            HIPCK(hipMemcpyAsync(&herr, d_err, 4, hipMemcpyDeviceToHost, st));
            HIPCK(hipStreamSynchronize(st));
            if (herr) return set_err(ctx, HDRF_E_INVAL, "corrupt deflate stream (chunk decode)");
            for (int pass = 0; nj > 1; pass++) {       // pointer jumping: chains halve every pass
                if (pass > 64) return set_err(ctx, HDRF_E_DEVICE, "window markers did not resolve");
                unsigned int left = 0;
                HIPCK(hipMemsetAsync(d_left, 0, 4, st));
                HIPCK(launch_inflate_resolve(scr, n, d_left, st));
                HIPCK(hipMemcpyAsync(&left, d_left, 4, hipMemcpyDeviceToHost, st));
                HIPCK(hipStreamSynchronize(st));
                if (!left) break;
            }
            HIPCK(launch_inflate_pack(scr, n, dev_out + out, st));
        }
        // CRC-32 of this member's output: 64 KiB pieces on the GPU, combined here
        const int64_t np = (n + kPiece - 1) / kPiece;
        uint32_t crc = 0;
        if (np) {
            HIPCK(launch_crc32_pieces(dev_out + out, n, op1k, (uint32_t *)(R + o_crc), st));
            crcs.resize((size_t)np);
            HIPCK(hipMemcpyAsync(crcs.data(), R + o_crc, 4 * (size_t)np, hipMemcpyDeviceToHost, st));
            HIPCK(hipStreamSynchronize(st));
            crc = crcs[0];
            for (int64_t i = 1; i < np; i++) {
                const int64_t len2 = std::min(kPiece, n - i * kPiece);
                if (len2 == kPiece) crc = crc_combine_op(piece_op, crc, crcs[(size_t)i]);
                else {
                    uint32_t op[32];
                    crc_shift_op(op, len2);
                    crc = crc_combine_op(op, crc, crcs[(size_t)i]);
                }
            }
        }
        if (crc != want_crc) return set_err(ctx, HDRF_E_INVAL, "gzip CRC-32 mismatch");
        out += n;
        at = end + 8;
    }
    return out;
}

// Read side for files: the Lz4Codec input stream DataConstructor opens for closed containers under
// compressor 2 (DN/DataConstructor.java:495-500) and for stream-mode blocks (:171-176).
extern "C" int64_t hdrf_lz4_file_decode(hdrf_ctx *ctx, const uint8_t *file, int64_t flen, uint8_t *dev_out, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    return decode_file(ctx, file, flen, dev_out, cap);
}

// The same for a stream-mode block file of codec 0 (SnappyCodec) or 4 (Lz4Codec): DataConstructor's
// compression-only decoders (DN/DataConstructor.java:102-220)
extern "C" int64_t hdrf_stream_file_decode(hdrf_ctx *ctx, int32_t codec, const uint8_t *file, int64_t flen,
                                           uint8_t *dev_out, int64_t cap)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (codec == 5) return decode_gzip(ctx, file, flen, dev_out, cap);
    if (codec == 3) return decode_lzop(ctx, file, flen, dev_out, cap);
    if (codec != 0 && codec != 4)
        return set_err(ctx, HDRF_E_UNSUPPORTED, "stream codec: 0 (SnappyCodec), 3 (LzopCodec), 4 (Lz4Codec), 5 (GzipCodec)");
    return decode_file(ctx, file, flen, dev_out, cap, codec);
}

extern "C" int hdrf_set_lzop_mtime(hdrf_ctx *ctx, uint32_t mtime)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    ctx->lzop_mtime = mtime;
    return 0;
}

// Compressor 5 stage 1 (gzip.hip): per-position longest_match answers for both chain limits.
extern "C" int hdrf_gzip_match_pass(hdrf_ctx *ctx, const uint8_t *dev_data, uint64_t len, uint32_t *dev_prev,
                                    uint32_t *dev_out128, uint32_t *dev_out32)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (len && (!dev_data || !dev_prev || !dev_out128 || !dev_out32)) return set_err(ctx, HDRF_E_INVAL, "null buffer");
    if (len >= (1ull << 31)) return set_err(ctx, HDRF_E_INVAL, "gzip match pass: len must be < 2^31");
    if (int rc = drain(ctx)) return rc;
    HIPCK(launch_gzip_match(dev_data, (int64_t)len, dev_prev, dev_out128, dev_out32, ctx->st));
    HIPCK(hipStreamSynchronize(ctx->st));
    return 0;
}

// Compressor 5 stage 2 (gzip.hip): the lazy parse over stage 1's answers.
extern "C" int hdrf_gzip_parse(hdrf_ctx *ctx, const uint8_t *dev_data, uint64_t len, const uint32_t *dev_m128,
                               const uint32_t *dev_m32, uint32_t *dev_syms, int64_t *dev_blks, int64_t *dev_cnt)
{
    HDRF_LOCK(ctx);
    if (!ctx) return HDRF_E_INVAL;
    if (!dev_syms || !dev_blks || !dev_cnt || (len && (!dev_data || !dev_m128 || !dev_m32)))
        return set_err(ctx, HDRF_E_INVAL, "null buffer");
    if (len >= (1ull << 31)) return set_err(ctx, HDRF_E_INVAL, "gzip parse: len must be < 2^31");
    if (int rc = drain(ctx)) return rc;
    if (int rc = grow(ctx, &ctx->d_rd, &ctx->rd_cap, gzip_parse_scratch((int64_t)len))) return rc;
    hipError_t e = launch_gzip_parse(dev_data, (int64_t)len, dev_m128, dev_m32, dev_syms, dev_blks, dev_cnt, ctx->d_rd,
                                     ctx->st);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->st);
    if (e != hipSuccess) return set_err(ctx, HDRF_E_HIP, std::string("gzip parse: ") + hipGetErrorString(e));
    return 0;
}
