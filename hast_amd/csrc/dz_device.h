// dz_device.h -- what dz_api.cpp / fq_api.cpp (host) and dz_kernels.hip (device) share: the description of a compression call as
// it lies in device memory, the workspace's size and the launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dz_core.h"
#include "fq_device.h"

namespace hast {
namespace dz {

// (Job and Result: dz_core.h)
// pieces a job of n_bytes in all can have at most, whatever its runs are
inline uint32_t max_pieces(uint64_t n_bytes) { return (uint32_t)(n_bytes / kPiece) + kMaxRuns; }
// most bytes the members of such a job take
inline uint64_t max_out_bytes(uint64_t n_bytes) { return n_bytes + 5ull * max_pieces(n_bytes) + (uint64_t)kMaxRuns * (kMemberHead + kMemberTail); }
// ... as blocked gzip: a frame per member, and a run's last member may be short
inline uint64_t max_out_bytes_blocked(uint64_t n_bytes) {
    return n_bytes + 5ull * max_pieces(n_bytes) + (uint64_t)kBlockedFrame * (n_bytes / kBlockedInput + kMaxRuns);
}
size_t workspace_bytes(uint32_t max_pieces);

// the encoder's device memory, one allocation: the workspace, behind it the Job and Result of n_jobs calls that take turns in it
struct EncoderSlot {
    uint8_t *d_work = nullptr;
    size_t bytes = 0;
    uint32_t max_pieces = 0, n_jobs = 0;
    Job *job(uint32_t i = 0) const { return reinterpret_cast<Job *>(d_work + bytes - n_jobs * (sizeof(Job) + sizeof(Result))) + i; }
    Result *res(uint32_t i = 0) const { return reinterpret_cast<Result *>(job(n_jobs)) + i; }
};
size_t slot_bytes(uint32_t max_pieces, uint32_t n_jobs);
hipError_t slot_alloc(EncoderSlot *s, uint32_t max_pieces, uint32_t n_jobs = 1);
void slot_release(EncoderSlot *s, bool park);  // parked at site 3 (hast_internal.h), or freed

hipError_t launch_job_one(Job *d_job, uint64_t n_bytes, hipStream_t s);                       // one run from offset 0, empty member for 0 bytes
hipError_t launch_job_from_route(Job *d_job, const RouteState *d_rs, hipStream_t s);          // the four runs of a routed block, as they lie in its d_out
// the two runs of a converted step of stage 02 (tx_feed.cpp): run 0 at offset 0, run 1 at second_off, d_run_bytes[0 .. 1] their sizes in device memory
hipError_t launch_job_from_tx(Job *d_job, const uint64_t *d_run_bytes, uint64_t second_off, hipStream_t s);
// the three runs of a binned view of stage 03 (rs_api.cpp): back to back from offset 0, d_run_bytes[0 .. 2] their sizes in device memory
hipError_t launch_job_from_bins(Job *d_job, const uint64_t *d_run_bytes, hipStream_t s);
// d_src + job.src_off[r] .. -> members from d_dst[0] on, never at or behind d_dst + cap; d_res says how long they are.
// flags: 0, or kLiteralsOnly | kBlocked (dz_core.h); blocked: every run becomes members of at most kBlockedPieces pieces
hipError_t launch_compress(const Job *d_job, const uint8_t *d_src, uint32_t max_pieces, void *d_work, uint8_t *d_dst, uint64_t cap, Result *d_res,
                           uint32_t flags, hipStream_t s);

}  // namespace dz
}  // namespace hast
