// msw_rt_deflate.cpp -- BGZF deflate (include/msw_fastq.h, beside
// msw_bgzf_inflate): the argument checks, the stream-ordered scratch, the
// launches of a group of blocks, and the host-to-host form with pinned staging.
// The kernels: msw_deflate.hip, the CRC of msw_inflate.hip, the scan of msw_aln.hip.
#include "msw_runtime_internal.h"

#include "../../include/msw_fastq.h"
#include "msw_gz.h"

using namespace msw_detail;

namespace {

constexpr uint64_t kBlock = msw::kDeflateBlock, kSlot = msw::kDeflateSlot;
constexpr uint64_t kEofBytes = 28;
constexpr uint64_t kStoredOverhead = 18 + 5 + 8;  // header, stored block header, trailer
// Waves of one launch, each with a token buffer of kBlock words: four fit a
// CU's LDS, so 1024 fill the 256 CUs, and the token scratch stays at 255 MiB.
constexpr uint32_t kMaxWaves = 1024;
constexpr uint64_t kMaxGroupBytes = 2048ull << 20;  // a group's member sizes are scanned as u32
constexpr uint64_t kStage = 32ull << 20;            // pinned staging of the host form

uint64_t blocks_of(uint64_t len) { return (len + kBlock - 1) / kBlock; }

uint64_t scan_tmp_words(uint64_t count) {
    uint64_t w = 0;
    for (uint64_t c = (count + msw::kAlnScanTile - 1) / msw::kAlnScanTile; c > 1;
         c = (c + msw::kAlnScanTile - 1) / msw::kAlnScanTile)
        w += c;
    return w;
}

uint64_t align256(uint64_t v) { return (v + 255) & ~255ull; }

}  // namespace

extern "C" {

uint64_t msw_bgzf_deflate_bound(uint64_t len) { return len + blocks_of(len) * kStoredOverhead + kEofBytes; }

int msw_bgzf_deflate_device(msw_ctx* ctx, const uint8_t* data, uint64_t len, uint8_t* out, uint64_t cap,
                            uint64_t* out_len, uint32_t flags, void* stream) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (flags & ~MSW_BGZF_NO_EOF) return fail(MSW_E_INVALID, "BGZF deflate: unknown flag bits 0x%x", flags);
    if (!out || !out_len || (!data && len)) return fail(MSW_E_INVALID, "BGZF deflate: data/out/out_len is NULL");
    if (cap < msw_bgzf_deflate_bound(len))
        return fail(MSW_E_RANGE, "BGZF deflate: an output of %llu bytes is below the bound of %llu",
                    (unsigned long long)cap, (unsigned long long)msw_bgzf_deflate_bound(len));
    if (((uintptr_t)data | (uintptr_t)out) & 3) return fail(MSW_E_INVALID, "BGZF deflate: data and out are 4-byte aligned");
    int rc;
    if ((rc = set_device(ctx))) return rc;
    hipStream_t st = call_stream(ctx, stream);
    if (len == 0) {
        HIP_TRY(msw::launch_gz_finish(nullptr, nullptr, true, true, flags, out, out_len, st));
        return MSW_OK;
    }
    // blocks per group: the context's inflate group size bounds the slots
    const uint64_t nb = blocks_of(len);
    const uint64_t gb = std::min(nb, std::max<uint64_t>(1, std::min(ctx->opt.gz_group_bytes, kMaxGroupBytes) / kBlock));
    const uint32_t waves = (uint32_t)std::min<uint64_t>(gb, kMaxWaves);
    const uint64_t at_tokens = align256(gb * kSlot);
    const uint64_t at_sizes = at_tokens + align256((uint64_t)waves * kBlock * 4);
    const uint64_t at_scan = at_sizes + align256((gb + 1) * 4);
    const uint64_t at_base = at_scan + align256(scan_tmp_words(gb + 1) * 4);
    const uint64_t at_consts = at_base + 256;
    StreamTmp tmp(st);
    if ((rc = tmp.alloc(at_consts + sizeof(msw::GzCrcConsts)))) return rc;
    uint8_t* const base = (uint8_t*)tmp.p;
    uint8_t* const slots = base;
    uint32_t* const tokens = (uint32_t*)(base + at_tokens);
    uint32_t* const sizes = (uint32_t*)(base + at_sizes);
    uint32_t* const scan_tmp = (uint32_t*)(base + at_scan);
    uint64_t* const done = (uint64_t*)(base + at_base);  // bytes of the groups before
    msw::GzCrcConsts* const consts = (msw::GzCrcConsts*)(base + at_consts);
    static const msw::GzCrcConsts kConsts = msw::gz_crc_consts();
    HIP_TRY(hipMemcpyAsync(consts, &kConsts, sizeof(kConsts), hipMemcpyHostToDevice, st));
    for (uint64_t b0 = 0; b0 < nb; b0 += gb) {
        const uint32_t n = (uint32_t)std::min(gb, nb - b0);
        const uint8_t* src = data + b0 * kBlock;
        const uint64_t src_len = std::min(len - b0 * kBlock, (uint64_t)n * kBlock);
        const bool first = b0 == 0, last = b0 + n == nb;
        HIP_TRY(msw::launch_gz_deflate(src, src_len, n, waves, slots, sizes, tokens, st));
        HIP_TRY(msw::launch_gz_crc_put(src, src_len, (uint32_t)kBlock, n, consts, slots, (uint32_t)kSlot, sizes, st));
        HIP_TRY(msw::scan_in_place(sizes, (uint64_t)n + 1, scan_tmp, st));
        HIP_TRY(msw::launch_gz_gather(slots, sizes, n, first ? nullptr : done, out, st));
        HIP_TRY(msw::launch_gz_finish(sizes + n, done, first, last, flags, out, out_len, st));
    }
    return MSW_OK;
}

int msw_bgzf_deflate(msw_ctx* ctx, const uint8_t* data, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* out_len,
                     uint32_t flags) {
    if (!ctx) return fail(MSW_E_INVALID, "ctx is NULL");
    if (flags & ~MSW_BGZF_NO_EOF) return fail(MSW_E_INVALID, "BGZF deflate: unknown flag bits 0x%x", flags);
    if (!out || !out_len || (!data && len)) return fail(MSW_E_INVALID, "BGZF deflate: data/out/out_len is NULL");
    const uint64_t bound = msw_bgzf_deflate_bound(len);
    if (cap < bound)
        return fail(MSW_E_RANGE, "BGZF deflate: an output of %llu bytes is below the bound of %llu",
                    (unsigned long long)cap, (unsigned long long)bound);
    *out_len = 0;
    int rc;
    if ((rc = set_device(ctx))) return rc;
    hipStream_t st = ctx->compute;
    DeviceArena arena;
    const auto d_in = arena.take<uint8_t>(len);
    const auto d_out = arena.take<uint8_t>(bound);
    const auto d_len = arena.take<uint64_t>(1);
    if ((rc = arena.alloc())) return rc;
    uint8_t* stage = nullptr;
    if (hipHostMalloc((void**)&stage, kStage, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return fail(MSW_E_NOMEM, "hipHostMalloc(%llu B) failed (BGZF deflate staging)", (unsigned long long)kStage);
    }
    ChunkCopy cp(st);
    for (uint64_t p = 0; p < len && cp.ok(); p += kStage) {
        const uint64_t c = std::min(kStage, len - p);
        memcpy(stage, data + p, c);
        cp.up((uint8_t*)d_in + p, stage, c);
        cp.sync();  // the staging block is reused
    }
    if (cp.ok()) rc = msw_bgzf_deflate_device(ctx, d_in, len, d_out, bound, d_len, flags, st);
    uint64_t total = 0;
    if (!rc && cp.ok()) {
        cp.down(stage, d_len, sizeof(uint64_t));
        cp.sync();
        memcpy(&total, stage, sizeof(total));
    }
    if (!rc && cp.ok() && total > bound) rc = fail(MSW_E_DEVICE, "BGZF deflate: the output passed its bound");
    for (uint64_t p = 0; !rc && p < total && cp.ok(); p += kStage) {
        const uint64_t c = std::min(kStage, total - p);
        cp.down(stage, (uint8_t*)d_out + p, c);
        cp.sync();
        if (cp.ok()) memcpy(out + p, stage, c);
    }
    rc = cp.finish(rc, "BGZF deflate");
    (void)hipHostFree(stage);
    if (!rc) *out_len = total;
    return rc;
}

}  // extern "C"
