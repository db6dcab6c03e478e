// bz_device.h -- what bz_api.cpp (host) and bz_kernels.hip (device) share, and what gz_api.cpp calls when a hast_gz handle is a
// blocked-gzip stream: the per-member result, the kernel launchers, the stream behind hast_gz_open_blocked.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hast.h"
#include "bz_core.h"

namespace hast {
namespace bz {

struct MemberOut {               // what k_bz_inflate leaves per member
    uint32_t why;                // kBadNone, or kBad* | gz_core.h error code << 8
    uint32_t n_out;              // bytes produced (never more than the member's isize)
};

// a wave per member: d_w = the batch's input words (zero padding behind them), d_out = the batch's output; member i's bytes go to
// d_out + d_mem[i].out_off, at most d_mem[i].isize of them
hipError_t launch_inflate(const Member *d_mem, uint32_t n, const uint32_t *d_w, uint8_t *d_out, MemberOut *d_res, hipStream_t s);
// a workgroup per member: d_verdict[i] = 0 or why member i is refused (k_bz_inflate's reason, bytes produced != isize, CRC-32);
// d_first[0] = min(index of a refused member), d_first[1] = min(index << 8 | reason): both 0xFFFFFFFF from the caller
hipError_t launch_check(const Member *d_mem, uint32_t n, const uint8_t *d_out, const MemberOut *d_res, uint32_t *d_verdict, uint32_t *d_first, hipStream_t s);

// ---- the stream (bz_api.cpp) ---------------------------------------------------------------------------------------------------
struct Stream;
// HAST_ERR_UNSUPPORTED: not a regular file, empty, no BGZF member at its start, no room on the device; HAST_ERR_IO: cannot be read
hast_status stream_open(hast_ctx *ctx, const char *path, size_t batch_in_bytes, size_t batch_out_bytes, Stream **out);
hast_status stream_read(Stream *z, uint8_t *d_dst, size_t cap, size_t *n_out, hipStream_t hs);
void stream_stats(Stream *z, hast_gz_stats *gs, hast_gz_blocked_stats *bs);          // (either may be null)
void stream_close(Stream *z);

}  // namespace bz
}  // namespace hast
