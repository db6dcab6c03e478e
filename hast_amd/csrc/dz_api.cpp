// dz_api.cpp -- the part of the C ABI that compresses device memory into gzip members (include/hast.h "deflate on the GPU").
// The routing stream's use of the same kernels is in fq_api.cpp (hast_fq_set_route_gz).
#include <hip/hip_runtime.h>

#include "dz_core.h"
#include "dz_device.h"
#include "hast_internal.h"

using namespace hast;

namespace hast {
namespace dz {

size_t slot_bytes(uint32_t max_pieces, uint32_t n_jobs) { return ((workspace_bytes(max_pieces) + 63) & ~(size_t)63) + n_jobs * (sizeof(Job) + sizeof(Result)); }
hipError_t slot_alloc(EncoderSlot *s, uint32_t max_pieces, uint32_t n_jobs) {
    *s = EncoderSlot{nullptr, slot_bytes(max_pieces, n_jobs), max_pieces, n_jobs};
    return dev_malloc(&s->d_work, s->bytes);
}
void slot_release(EncoderSlot *s, bool park) {
    park ? park_device(s->d_work, s->bytes, 3) : (void)hipFree(s->d_work);
    *s = EncoderSlot{};
}

static hast_status compress_one(const EncoderSlot &z, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, uint32_t flags, hipStream_t hs) {
    Result res;
    HAST_HIP_TRY(launch_job_one(z.job(), n_bytes, hs));
    HAST_HIP_TRY(launch_compress(z.job(), d_src, z.max_pieces, z.d_work, d_dst, cap, z.res(), flags, hs));
    HAST_HIP_TRY(hipMemcpyAsync(&res, z.res(), sizeof res, hipMemcpyDeviceToHost, hs));
    HAST_HIP_TRY(hipStreamSynchronize(hs));
    if (res.flags) return set_error(HAST_ERR_INVALID, "hast_dz_compress_device: the member did not fit its bound (flags %u)", res.flags);
    *n_out = (size_t)res.out_bytes[0];
    return HAST_OK;
}

// what the entry points share: one run of n_bytes from d_src, with encoder memory of its own, waited for.  flags: dz_core.h
static hast_status compress_call(hast_ctx *c, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, uint32_t flags, hast_stream stream) {
    if (!c || !d_dst || !n_out || (n_bytes && !d_src)) return set_error(HAST_ERR_INVALID, "null argument");
    const size_t need = (size_t)((flags & kBlocked) ? bound_blocked(n_bytes) : bound(n_bytes));
    if (cap < need) return set_error(HAST_ERR_INVALID, "hast_dz_compress_device: %zu bytes of room, %zu bytes of input can take %zu", cap, n_bytes, need);
    if (n_bytes / kPiece >= (1ull << 31)) return set_error(HAST_ERR_INVALID, "hast_dz_compress_device: input too large for one call");
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : ctx_stream_of(c);
    EncoderSlot z;
    *n_out = 0;
    HAST_HIP_TRY(hipSetDevice(hast_ctx_device(c)));
    HAST_HIP_TRY(slot_alloc(&z, (uint32_t)n_pieces(n_bytes)));
    const hast_status st = compress_one(z, d_src, n_bytes, d_dst, cap, n_out, flags, hs);
    (void)hipStreamSynchronize(hs);                         // (nothing of this call may still read the workspace)
    slot_release(&z, false);
    return st;
}

}  // namespace dz
}  // namespace hast

extern "C" {

size_t hast_dz_bound(size_t n_bytes) { return (size_t)dz::bound(n_bytes); }
size_t hast_dz_bound_blocked(size_t n_bytes) { return (size_t)dz::bound_blocked(n_bytes); }

hast_status hast_dz_compress_device_ex(hast_ctx *c, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, unsigned flags,
                                       hast_stream stream) {
    if (flags & ~(unsigned)HAST_DZ_LITERALS_ONLY) return set_error(HAST_ERR_INVALID, "hast_dz_compress_device_ex: unknown flags %#x", flags);
    return dz::compress_call(c, d_src, n_bytes, d_dst, cap, n_out, (flags & HAST_DZ_LITERALS_ONLY) ? dz::kLiteralsOnly : 0, stream);
}

hast_status hast_dz_compress_device(hast_ctx *c, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, hast_stream stream) {
    return hast_dz_compress_device_ex(c, d_src, n_bytes, d_dst, cap, n_out, 0, stream);
}

hast_status hast_dz_compress_blocked_device(hast_ctx *c, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, hast_stream stream) {
    return dz::compress_call(c, d_src, n_bytes, d_dst, cap, n_out, dz::kBlocked, stream);
}

}  // extern "C"
