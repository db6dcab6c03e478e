// rows_api.cpp -- the part of the C ABI that makes `classify`'s output table on the GPU (include/hast.h "the output table on the GPU"):
// the steps of rows_kernels.hip in order, the memory they need, and the finished text's way back through pinned staging.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "hast_internal.h"
#include "rows_core.h"
#include "rows_device.h"

using namespace hast;

struct hast_rows {
    int device = 0;
    hipStream_t stream = nullptr;
    size_t n = 0;
    uint8_t *d_text[4] = {nullptr, nullptr, nullptr, nullptr};      // the table, the three lists
    uint32_t *d_order = nullptr;
    uint8_t *d_list_of = nullptr;
    hast_rows_info info = {};
    uint8_t *h_stage[2] = {nullptr, nullptr};                       // pinned, kStage bytes each: one copies while the other is emptied
    hipEvent_t staged[2] = {nullptr, nullptr};
};

namespace {

constexpr size_t kStage = 8u << 20;

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

// the arrays of a build that do not outlive it, in one allocation
struct Work {
    uint8_t *d = nullptr;
    uint64_t *hi = nullptr, *lo = nullptr, *keys_out = nullptr;
    uint32_t *id = nullptr, *id1 = nullptr, *meta = nullptr, *flags = nullptr;
    rows::TileBase *base = nullptr;
    void *sort_tmp = nullptr;
    size_t sort_tmp_bytes = 0;
};

hast_status build(hast_ctx *c, const uint8_t *d_text16, const uint64_t *d_counts, size_t n, uint64_t n0, uint64_t n1, double w0, double w1, int with_lists,
                  hast_rows **out) {
    if (!c || !out) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    if (n && (!d_text16 || !d_counts)) return set_error(HAST_ERR_INVALID, "null argument");
    if (n >> 32) return set_error(HAST_ERR_INVALID, "hast_rows_build: %zu rows, ids are 32 bits wide", n);
    if ((reinterpret_cast<uintptr_t>(d_text16) & 15) || (reinterpret_cast<uintptr_t>(d_counts) & 31))
        return set_error(HAST_ERR_INVALID, "hast_rows_build: text records must be 16-byte aligned, counters 32-byte aligned");
    HAST_HIP_TRY(hipSetDevice(ctx_device_of(c)));
    hast_rows *r = new hast_rows();
    r->device = ctx_device_of(c);
    r->stream = ctx_stream_of(c);
    r->n = n;
    r->info.n_rows = n;
    hipStream_t hs = r->stream;
    Work w;
    const size_t nt = rows::n_tiles(n);
    hipError_t e = !n ? hipSuccess : rows::sort_pass(nullptr, &w.sort_tmp_bytes, nullptr, nullptr, nullptr, nullptr, n, hs);
    auto fail = [&](const char *what) {
        const hast_status st = set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_rows_build: %s: %s", what, hipGetErrorString(e));
        (void)hipStreamSynchronize(hs);
        if (w.d) (void)hipFree(w.d);
        hast_rows_destroy(r);
        return st;
    };
    if (e != hipSuccess) return fail("sizing the sort");
    {
        const size_t b64 = up256(n * 8), b32 = up256(n * 4), b_base = up256((nt + 1) * sizeof(rows::TileBase)), b_tmp = up256(w.sort_tmp_bytes + 16);
        e = dev_malloc(&w.d, 3 * b64 + 3 * b32 + b_base + 256 + b_tmp);
        if (e != hipSuccess) return fail("workspace");
        uint8_t *p = w.d;
        w.hi = reinterpret_cast<uint64_t *>(p), p += b64;
        w.lo = reinterpret_cast<uint64_t *>(p), p += b64;
        w.keys_out = reinterpret_cast<uint64_t *>(p), p += b64;
        w.id = reinterpret_cast<uint32_t *>(p), p += b32;
        w.id1 = reinterpret_cast<uint32_t *>(p), p += b32;
        w.meta = reinterpret_cast<uint32_t *>(p), p += b32;
        w.base = reinterpret_cast<rows::TileBase *>(p), p += b_base;
        w.flags = reinterpret_cast<uint32_t *>(p), p += 256;
        w.sort_tmp = p;
    }
    e = dev_malloc(&r->d_order, up256(n * 4));
    if (e == hipSuccess) e = dev_malloc(&r->d_list_of, up256(n));
    for (int i = 0; i < 2 && e == hipSuccess; ++i) {
        e = pinned_malloc(&r->h_stage[i], kStage);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&r->staged[i], hipEventDisableTiming);
    }
    if (e != hipSuccess) return fail("the order, the lists by id and the staging buffers");

    // 1. a key, a call and the lengths per id
    double t0 = now_s();
    e = hipMemsetAsync(w.flags, 0, 256, hs);
    if (e == hipSuccess) e = rows::launch_key(d_text16, d_counts, n, n0, n1, w0, w1, w.hi, w.lo, w.id, w.meta, r->d_list_of, w.flags, hs);
    if (e == hipSuccess) e = hipStreamSynchronize(hs);
    if (e != hipSuccess) return fail("keys");
    r->info.keys_s = now_s() - t0;
    // 2. the ids by (hi, lo): stably by lo, then stably by hi
    t0 = now_s();
    if (n) {
        e = rows::sort_pass(w.sort_tmp, &w.sort_tmp_bytes, w.lo, w.keys_out, w.id, w.id1, n, hs);
        if (e == hipSuccess) e = rows::launch_gather(w.hi, w.id1, n, w.lo, hs);                          // (the low words are done with)
        if (e == hipSuccess) e = rows::sort_pass(w.sort_tmp, &w.sort_tmp_bytes, w.lo, w.keys_out, w.id1, r->d_order, n, hs);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(hs);
    if (e != hipSuccess) return fail("sort");
    r->info.sort_s = now_s() - t0;
    // 3. the offsets, the sizes, the text
    t0 = now_s();
    rows::TileBase total;
    uint32_t flags[2] = {0, 0};
    e = rows::launch_scan(r->d_order, w.meta, n, w.base, hs);
    if (e == hipSuccess) e = hipMemcpyAsync(&total, w.base + nt, sizeof total, hipMemcpyDeviceToHost, hs);
    if (e == hipSuccess) e = hipMemcpyAsync(flags, w.flags, sizeof flags, hipMemcpyDeviceToHost, hs);
    if (e == hipSuccess) e = hipStreamSynchronize(hs);
    if (e != hipSuccess) return fail("offsets");
    r->info.table_bytes = total.at[0];
    r->info.any_sep = flags[0] != 0;
    r->info.past_int = flags[1] != 0;
    e = dev_malloc(&r->d_text[0], up256(total.at[0] + 16));
    for (int l = 0; l < 3 && with_lists && e == hipSuccess; ++l) {
        r->info.list_bytes[l] = total.at[l + 1];
        e = dev_malloc(&r->d_text[l + 1], up256(total.at[l + 1] + 16));
    }
    if (e != hipSuccess) return fail("the text");
    e = rows::launch_write(d_text16, d_counts, r->d_order, w.meta, n, w.base, r->d_text[0], r->d_text[1], r->d_text[2], r->d_text[3], with_lists ? 1 : 0, hs);
    if (e == hipSuccess) e = hipStreamSynchronize(hs);
    if (e != hipSuccess) return fail("text");
    r->info.format_s = now_s() - t0;
    (void)hipFree(w.d);
    *out = r;
    return HAST_OK;
}

}  // namespace

extern "C" {

hast_status hast_rows_build_device(hast_ctx *c, const uint8_t *d_text16, const uint64_t *d_counts, size_t n, uint64_t n0, uint64_t n1, double w0, double w1,
                                   int with_lists, hast_rows **out) {
    return build(c, d_text16, d_counts, n, n0, n1, w0, w1, with_lists, out);
}

hast_status hast_rows_build(hast_ctx *c, hast_names *dict, size_t n, uint64_t n0, uint64_t n1, double w0, double w1, int with_lists, hast_rows **out) {
    if (!c || !dict || !out) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    size_t limit = 0;
    int device = 0;
    const uint8_t *d_text16 = names_texts_of(dict, &limit, &device);
    if (!d_text16) return set_error(HAST_ERR_INVALID, "hast_rows_build: not a dictionary (hast_names_create_dict)");
    if (device != ctx_device_of(c)) return set_error(HAST_ERR_INVALID, "hast_rows_build: the dictionary is on GPU %d, the context on GPU %d", device, ctx_device_of(c));
    const uint64_t *d_counts = ctx_counts_of(c);
    if (n > limit || n > ctx_n_barcodes(c) || (n && !d_counts))
        return set_error(HAST_ERR_INVALID, "hast_rows_build: %zu rows, the dictionary can hand out %zu ids and the context counts %zu barcodes", n, limit, ctx_n_barcodes(c));
    HAST_HIP_TRY(hipSetDevice(device));
    HAST_HIP_TRY(hipDeviceSynchronize());                  // (naming and commit kernels of any stream of this GPU: the texts and the counters are final)
    return build(c, d_text16, d_counts, n, n0, n1, w0, w1, with_lists, out);
}

hast_status hast_rows_get_info(hast_rows *r, hast_rows_info *info) {
    if (!r || !info) return set_error(HAST_ERR_INVALID, "null argument");
    *info = r->info;
    return HAST_OK;
}

hast_status hast_rows_read(hast_rows *r, int which, uint64_t offset, size_t n, void *host) {
    if (!r || (n && !host)) return set_error(HAST_ERR_INVALID, "null argument");
    if (which < 0 || which > 3) return set_error(HAST_ERR_INVALID, "hast_rows_read: text %d (0 = the table, 1..3 = the lists)", which);
    const uint64_t have = which ? r->info.list_bytes[which - 1] : r->info.table_bytes;
    if (offset > have || n > have - offset) return set_error(HAST_ERR_INVALID, "hast_rows_read: bytes [%llu, %llu) of %llu", (unsigned long long)offset,
                                                             (unsigned long long)(offset + n), (unsigned long long)have);
    if (!n) return HAST_OK;
    HAST_HIP_TRY(hipSetDevice(r->device));
    const uint8_t *src = r->d_text[which] + offset;
    uint8_t *dst = static_cast<uint8_t *>(host);
    const size_t pieces = (n + kStage - 1) / kStage;
    auto piece_bytes = [&](size_t k) { return std::min(kStage, n - k * kStage); };
    HAST_HIP_TRY(hipMemcpyAsync(r->h_stage[0], src, piece_bytes(0), hipMemcpyDeviceToHost, r->stream));
    HAST_HIP_TRY(hipEventRecord(r->staged[0], r->stream));
    for (size_t k = 0; k < pieces; ++k) {
        if (k + 1 < pieces) {                              // (its buffer was emptied a round ago)
            HAST_HIP_TRY(hipMemcpyAsync(r->h_stage[(k + 1) & 1], src + (k + 1) * kStage, piece_bytes(k + 1), hipMemcpyDeviceToHost, r->stream));
            HAST_HIP_TRY(hipEventRecord(r->staged[(k + 1) & 1], r->stream));
        }
        HAST_HIP_TRY(hipEventSynchronize(r->staged[k & 1]));
        memcpy(dst + k * kStage, r->h_stage[k & 1], piece_bytes(k));
    }
    return HAST_OK;
}

hast_status hast_rows_order(hast_rows *r, uint32_t *ids_in_row_order) {
    if (!r || (r->n && !ids_in_row_order)) return set_error(HAST_ERR_INVALID, "null argument");
    HAST_HIP_TRY(hipSetDevice(r->device));
    if (r->n) HAST_HIP_TRY(hipMemcpy(ids_in_row_order, r->d_order, r->n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return HAST_OK;
}

hast_status hast_rows_classes(hast_rows *r, uint8_t *cls_by_id) {
    if (!r || (r->n && !cls_by_id)) return set_error(HAST_ERR_INVALID, "null argument");
    HAST_HIP_TRY(hipSetDevice(r->device));
    if (r->n) HAST_HIP_TRY(hipMemcpy(cls_by_id, r->d_list_of, r->n, hipMemcpyDeviceToHost));
    return HAST_OK;
}

void hast_rows_destroy(hast_rows *r) {
    if (!r) return;
    (void)hipSetDevice(r->device);
    (void)hipStreamSynchronize(r->stream);
    for (uint8_t *p : r->d_text)
        if (p) (void)hipFree(p);
    if (r->d_order) (void)hipFree(r->d_order);
    if (r->d_list_of) (void)hipFree(r->d_list_of);
    for (int i = 0; i < 2; ++i) {
        if (r->h_stage[i]) (void)hipHostFree(r->h_stage[i]);
        if (r->staged[i]) (void)hipEventDestroy(r->staged[i]);
    }
    delete r;
}

}  // extern "C"
