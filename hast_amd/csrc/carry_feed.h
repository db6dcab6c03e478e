// carry_feed.h -- the memory and the HIP calls of a carried-block feed (carry_plan.h) for hast_sq_feed and hast_rs: two device views,
// two pinned staging blocks, the upload stream.  Steps and carries run on the owner's stream.  WHO WAITS FOR WHOM:
//   * a step waits for the upload of its block (up_ev), unless the block was written on the device;
//   * a staging block is given out again once its upload, two blocks ago, has completed;
//   * THE UPLOAD RULE: carry() records an event behind its copy, and an upload waits for the last one recorded.  The upload of block n
//     writes the view block n-2 lay in; that block's step has been waited for, the carry out of it, which reads the view, need not be;
//   * a device block is written by the caller on the owner's stream: behind everything that still reads the view.
#pragma once
#include <hip/hip_runtime.h>

#include "carry_plan.h"
#include "hast_internal.h"

namespace hast {

struct CarryFeed {
    const char *name = "";                   // the owner's ABI prefix ("hast_rs") in the texts of hast_last_error()
    int device = 0;
    hipStream_t stream = nullptr, up_stream = nullptr;       // the owner's: steps and carries; ours: uploads
    carry::Plan plan;
    uint8_t *d_in[2] = {nullptr, nullptr}, *h_in[2] = {nullptr, nullptr};
    hipEvent_t up_ev[2] = {nullptr, nullptr}, carry_ev = nullptr;
    bool up_pending[2] = {false, false}, carry_pending = false;

    hipError_t create(const char *owner, int dev, hipStream_t owner_stream, size_t block) {
        name = owner, device = dev, stream = owner_stream, plan.block = block;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&carry_ev, hipEventDisableTiming);
        for (int i = 0; i < 2 && e == hipSuccess; ++i) {
            e = dev_malloc(&d_in[i], carry::room_of(block));
            if (e == hipSuccess) e = pinned_malloc(&h_in[i], block);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&up_ev[i], hipEventDisableTiming);
        }
        return e;
    }
    hast_status may_hand() {
        if (!plan.may_hand()) return set_error(HAST_ERR_INVALID, "%s: two blocks are waiting for %s_next", name, name);
        HAST_HIP_TRY(hipSetDevice(device));
        return HAST_OK;
    }
    // what = 1: the staging block; 2: the place of the new bytes in the view
    hast_status block(int what, uint8_t **buf) {
        if (hast_status st = may_hand()) return st;
        if (!buf) return set_error(HAST_ERR_INVALID, "null argument");
        const int slot = plan.submit_slot();
        if (what == 1 && up_pending[slot]) {
            HAST_HIP_TRY(hipEventSynchronize(up_ev[slot]));
            up_pending[slot] = false;
        }
        plan.hand(what);
        *buf = what == 1 ? h_in[slot] : d_in[slot] + plan.new_off();
        return HAST_OK;
    }
    hast_status submit(size_t n_bytes, bool allow_empty) {
        if (hast_status st = may_hand()) return st;
        if (!plan.may_submit(n_bytes, allow_empty)) return set_error(HAST_ERR_INVALID, "%s_submit: %zu bytes of a block of %zu", name, n_bytes, plan.block);
        const int slot = plan.submit_slot();
        if (!plan.submitted(n_bytes)) return HAST_OK;
        if (carry_pending) HAST_HIP_TRY(hipStreamWaitEvent(up_stream, carry_ev, 0));                 // the upload rule
        HAST_HIP_TRY(hipMemcpyAsync(d_in[slot] + plan.new_off(), h_in[slot], n_bytes, hipMemcpyHostToDevice, up_stream));
        HAST_HIP_TRY(hipEventRecord(up_ev[slot], up_stream));
        up_pending[slot] = true;
        return HAST_OK;
    }
    // in front of a step
    hast_status wait_step() {
        if (!plan.waiting()) return set_error(HAST_ERR_INVALID, "%s_next: no block submitted", name);
        HAST_HIP_TRY(hipSetDevice(device));
        if (!plan.on_device[plan.step_slot()]) HAST_HIP_TRY(hipStreamWaitEvent(stream, up_ev[plan.step_slot()], 0));
        return HAST_OK;
    }
    const uint8_t *at(const carry::View &v) const { return d_in[v.slot] + v.off; }
    // behind a step over view v: what it leaves goes in front of the next block's new bytes
    hast_status carry(const carry::View &v, size_t left, size_t consumed) {
        if (left) HAST_HIP_TRY(hipMemcpyAsync(d_in[v.slot ^ 1] + plan.left_off(left), at(v) + consumed, left, hipMemcpyDeviceToDevice, stream));
        HAST_HIP_TRY(hipEventRecord(carry_ev, stream));
        carry_pending = true;
        plan.tail = left;
        return HAST_OK;
    }
    hast_status take_tail(uint8_t *dst, size_t *n_bytes) {
        if (!dst || !n_bytes) return set_error(HAST_ERR_INVALID, "null argument");
        if (plan.waiting()) return set_error(HAST_ERR_INVALID, "%s_take_tail: a submitted block has not been framed", name);
        HAST_HIP_TRY(hipSetDevice(device));
        const carry::View v = plan.tail_view();
        if ((*n_bytes = v.bytes)) {
            HAST_HIP_TRY(hipMemcpyAsync(dst, at(v), v.bytes, hipMemcpyDeviceToHost, stream));
            HAST_HIP_TRY(hipStreamSynchronize(stream));
        }
        plan.drop_tail();
        return HAST_OK;
    }
    // waits for both streams; park: at site 3 (hast_internal.h), else the buffers are freed
    void release(bool park) {
        (void)hipSetDevice(device);
        if (up_stream) (void)hipStreamSynchronize(up_stream);
        if (stream) (void)hipStreamSynchronize(stream);
        for (int i = 0; i < 2; ++i) {
            park ? park_device(d_in[i], carry::room_of(plan.block), 3) : (void)hipFree(d_in[i]);
            park ? park_pinned(h_in[i], plan.block, 3) : (void)hipHostFree(h_in[i]);
            if (up_ev[i]) (void)hipEventDestroy(up_ev[i]);
        }
        if (carry_ev) (void)hipEventDestroy(carry_ev);
        if (up_stream) (void)hipStreamDestroy(up_stream);
    }
};

}  // namespace hast
