// dz_api.cpp -- the part of the C ABI that compresses device memory into gzip members (include/hast.h "deflate on the GPU").
// The routing stream's use of the same kernels is in fq_api.cpp (hast_fq_set_route_gz).
#include <hip/hip_runtime.h>

#include "dz_core.h"
#include "dz_device.h"
#include "hast_internal.h"

using namespace hast;

#define DZ_HIP(expr)                                                                          \
    do {                                                                                      \
        const hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess) {                                                               \
            st = set_error(e_ == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
            goto out;                                                                         \
        }                                                                                     \
    } while (0)

extern "C" {

size_t hast_dz_bound(size_t n_bytes) { return (size_t)dz::bound(n_bytes); }

hast_status hast_dz_compress_device_ex(hast_ctx *c, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, unsigned flags,
                                       hast_stream stream) {
    if (!c || !d_dst || !n_out || (n_bytes && !d_src)) return set_error(HAST_ERR_INVALID, "null argument");
    if (flags & ~(unsigned)HAST_DZ_LITERALS_ONLY) return set_error(HAST_ERR_INVALID, "hast_dz_compress_device_ex: unknown flags %#x", flags);
    if (cap < dz::bound(n_bytes))
        return set_error(HAST_ERR_INVALID, "hast_dz_compress_device: %zu bytes of room, %zu bytes of input can take %zu", cap, n_bytes, (size_t)dz::bound(n_bytes));
    if (n_bytes / dz::kPiece >= (1ull << 31)) return set_error(HAST_ERR_INVALID, "hast_dz_compress_device: input too large for one member");
    hast_status st = HAST_OK;
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : ctx_stream_of(c);
    const uint32_t max_pieces = (uint32_t)dz::n_pieces(n_bytes);
    const size_t work_bytes = (dz::workspace_bytes(max_pieces) + 63) & ~(size_t)63;
    void *d_work = nullptr;
    dz::Job *d_job = nullptr;
    dz::Result *d_res = nullptr;
    dz::Result res;
    *n_out = 0;
    DZ_HIP(hipSetDevice(hast_ctx_device(c)));
    DZ_HIP(dev_malloc(&d_work, work_bytes + sizeof(dz::Job) + sizeof(dz::Result)));
    d_job = reinterpret_cast<dz::Job *>(static_cast<uint8_t *>(d_work) + work_bytes);
    d_res = reinterpret_cast<dz::Result *>(d_job + 1);
    DZ_HIP(dz::launch_job_one(d_job, n_bytes, hs));
    DZ_HIP(dz::launch_compress(d_job, d_src, max_pieces, d_work, d_dst, cap, d_res, (flags & HAST_DZ_LITERALS_ONLY) ? 1 : 0, hs));
    DZ_HIP(hipMemcpyAsync(&res, d_res, sizeof res, hipMemcpyDeviceToHost, hs));
    DZ_HIP(hipStreamSynchronize(hs));
    if (res.flags) st = set_error(HAST_ERR_INVALID, "hast_dz_compress_device: the member did not fit its bound (flags %u)", res.flags);
    else *n_out = (size_t)res.out_bytes[0];
out:
    if (d_work) {
        (void)hipStreamSynchronize(hs);                     // (nothing of this call may still read the workspace)
        (void)hipFree(d_work);
    }
    return st;
}

hast_status hast_dz_compress_device(hast_ctx *c, const uint8_t *d_src, size_t n_bytes, uint8_t *d_dst, size_t cap, size_t *n_out, hast_stream stream) {
    return hast_dz_compress_device_ex(c, d_src, n_bytes, d_dst, cap, n_out, 0, stream);
}

}  // extern "C"
