// tx_api.cpp -- the part of the C ABI that converts stLFR read pairs into 10x FASTQ (include/hast.h "stage 02"): the map file and
// the conversion of host buffers, both tx_host.h's over the rules of tx_core.h, and the same conversion over device memory
// (hast_tx_create / hast_tx_pair_device: the kernels are tx_kernels.hip, what they decide per record tx_plan.h).  The hast_tx_map_*
// entries and hast_tx_pair_host are plain host code and touch no GPU.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <new>
#include <string>
#include <vector>

#include "hast_internal.h"
#include "tx_device.h"
#include "tx_host.h"

using namespace hast;

struct hast_tx_map {
    tx::Map map;
};

static_assert(sizeof(tx::TableSlot) == 48, "the table's slots are 48 bytes (tx_plan.h)");

// what hast_tx_pair_staged moves a step's bytes through, allocated at its first call: pinned staging and device buffers for both
// inputs of max_in bytes, device room for both runs (2 x max_in + 4 KB) and for their gzip members, and two slots of pinned memory
// for what comes back -- the slot of step n stays valid while step n + 1 runs, for whoever writes it out
struct TxStaging {
    size_t cap_out = 0, cap_gz = 0, cap_host = 0;
    uint8_t *h_in[2] = {nullptr, nullptr}, *d_in[2] = {nullptr, nullptr}, *d_out[2] = {nullptr, nullptr}, *d_gz[2] = {nullptr, nullptr};
    uint8_t *h_out[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};        // [slot][side]
    hipEvent_t ev[2] = {nullptr, nullptr};
    unsigned slot = 0;
};

struct hast_tx {
    hast_ctx *ctx = nullptr;
    const hast_tx_map *map = nullptr;        // the caller's (a paired feed converts a step on the host with it)
    TxStaging *io = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;            // the context's, when a call names none
    size_t max_in = 0;
    TxScratchPlan plan;
    uint8_t *d_scratch = nullptr;
    tx::TableSlot *d_table = nullptr;
    uint32_t n_slots = 0;
    TxDevState *h_st = nullptr;              // pinned
};

static void fill_info(const tx::Map &m, hast_tx_map_info *info) {
    if (!info) return;
    memset(info, 0, sizeof *info);
    info->n_keys = m.kv.size();
    info->device_ok = m.device_ok ? 1 : 0;
    snprintf(info->reason, sizeof info->reason, "%s", m.reason.c_str());
}

namespace hast {
TxParts tx_parts_of(const hast_tx *t) {
    return TxParts{t->ctx, t->device, t->max_in, t->map, reinterpret_cast<const TxDevState *>(t->d_scratch + t->plan.state)};
}
}  // namespace hast

extern "C" {

hast_status hast_tx_map_parse(const uint8_t *text, size_t n_bytes, hast_tx_map **out, hast_tx_map_info *info) {
    if (!out || (n_bytes && !text)) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    hast_tx_map *m = new (std::nothrow) hast_tx_map;
    if (!m) return set_error(HAST_ERR_OOM, "hast_tx_map_parse");
    tx::map_parse(text, n_bytes, m->map);
    fill_info(m->map, info);
    *out = m;
    return HAST_OK;
}

hast_status hast_tx_map_load(const char *path, hast_tx_map **out, hast_tx_map_info *info) {
    if (!path || !out) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    FILE *f = fopen(path, "rb");
    if (!f) return set_error(HAST_ERR_IO, "cannot open %s", path);
    std::vector<uint8_t> text;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.insert(text.end(), buf, buf + n);
    const bool bad = ferror(f) != 0;
    fclose(f);
    if (bad) return set_error(HAST_ERR_IO, "cannot read %s", path);
    return hast_tx_map_parse(text.data(), text.size(), out, info);
}

void hast_tx_map_destroy(hast_tx_map *m) { delete m; }

hast_status hast_tx_pair_host(const hast_tx_map *m, const uint8_t *r1, size_t n1, const uint8_t *r2, size_t n2, int final, hast_tx_state *state, uint8_t **out1,
                              uint8_t **out2, hast_tx_result *res) {
    if (!m || !state || !out1 || !out2 || !res || (n1 && !r1) || (n2 && !r2)) return set_error(HAST_ERR_INVALID, "null argument");
    if (final < 0 || final > 2) return set_error(HAST_ERR_INVALID, "hast_tx_pair_host: final = %d (0, 1 or 2)", final);
    *out1 = *out2 = nullptr;
    tx::State st;
    st.used = state->used;
    st.headers = state->headers;
    std::string o[2];
    size_t c1 = 0, c2 = 0;
    tx::pair_host(m->map, r1, n1, r2, n2, final, st, o[0], o[1], &c1, &c2);
    uint8_t *p[2];
    for (int s = 0; s < 2; ++s) {
        p[s] = static_cast<uint8_t *>(malloc(o[s].size() + 1));
        if (!p[s]) {
            if (s) free(p[0]);
            return set_error(HAST_ERR_OOM, "hast_tx_pair_host: %zu bytes of output", o[s].size());
        }
        memcpy(p[s], o[s].data(), o[s].size());
    }
    *out1 = p[0];
    *out2 = p[1];
    res->consumed1 = c1;
    res->consumed2 = c2;
    res->pairs = st.headers - state->headers;
    res->used = st.used - state->used;
    for (int s = 0; s < 2; ++s) res->out_bytes[s] = res->raw_bytes[s] = o[s].size();
    const uint8_t *in[2] = {r1, r2};
    const size_t n_in[2] = {n1, n2};
    for (int s = 0; s < 2; ++s) {
        uint64_t lines = 0;
        for (size_t i = 0; i < n_in[s]; ++i) lines += in[s][i] == '\n';
        res->lines[s] = lines > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)lines;
    }
    state->used = st.used;
    state->headers = st.headers;
    return HAST_OK;
}

void hast_tx_free(void *p) { free(p); }

hast_status hast_tx_create(hast_ctx *c, const hast_tx_map *m, size_t max_in_bytes, hast_tx **out) {
    if (!c || !m || !out) return set_error(HAST_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!m->map.device_ok) return set_error(HAST_ERR_UNSUPPORTED, "hast_tx_create: the map cannot go to the device: %s", m->map.reason.c_str());
    if (max_in_bytes < 1 || max_in_bytes > kTxMaxIn)
        return set_error(HAST_ERR_INVALID, "hast_tx_create: %zu bytes a side; offsets inside a step are 32 bits wide (at most %zu)", max_in_bytes, kTxMaxIn);
    hast_tx *t = new (std::nothrow) hast_tx;
    if (!t) return set_error(HAST_ERR_OOM, "hast_tx_create");
    std::vector<tx::TableSlot> table;
    tx::table_build(m->map, table);
    t->ctx = c;
    t->map = m;
    t->device = hast_ctx_device(c);
    t->stream = ctx_stream_of(c);
    t->max_in = max_in_bytes;
    t->plan = tx_scratch_plan(max_in_bytes);
    t->n_slots = (uint32_t)table.size();
    hipError_t e = hipSetDevice(t->device);
    if (e == hipSuccess) e = dev_malloc(&t->d_scratch, t->plan.total);
    if (e == hipSuccess) e = dev_malloc(&t->d_table, table.size() * sizeof(tx::TableSlot));
    if (e == hipSuccess) e = pinned_malloc(&t->h_st, sizeof(TxDevState));
    if (e == hipSuccess) e = hipMemcpyAsync(t->d_table, table.data(), table.size() * sizeof(tx::TableSlot), hipMemcpyHostToDevice, t->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
    if (e != hipSuccess) {
        const size_t total = t->plan.total;
        hast_tx_destroy(t);
        return set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_tx_create: %zu bytes of scratch: %s", total, hipGetErrorString(e));
    }
    *out = t;
    return HAST_OK;
}

hast_status hast_tx_pair_device(hast_tx *t, const uint8_t *d_r1, size_t n1, const uint8_t *d_r2, size_t n2, hast_tx_state *state, uint8_t *d_out1, size_t cap1,
                                uint8_t *d_out2, size_t cap2, hast_tx_result *res, hast_stream stream) {
    if (!t || !state || !res || (n1 && !d_r1) || (n2 && !d_r2) || (cap1 && !d_out1) || (cap2 && !d_out2)) return set_error(HAST_ERR_INVALID, "null argument");
    if (n1 > t->max_in || n2 > t->max_in)
        return set_error(HAST_ERR_INVALID, "hast_tx_pair_device: %zu and %zu bytes, the converter was created for %zu a side", n1, n2, t->max_in);
    hipStream_t hs = stream ? static_cast<hipStream_t>(stream) : t->stream;
    TxStepArgs a;
    a.d_in[0] = d_r1; a.d_in[1] = d_r2;
    a.n_in[0] = n1; a.n_in[1] = n2;
    a.d_out[0] = d_out1; a.d_out[1] = d_out2;
    a.cap[0] = cap1; a.cap[1] = cap2;
    a.used = state->used;
    a.d_table = t->d_table;
    a.n_slots = t->n_slots;
    HAST_HIP_TRY(hipSetDevice(t->device));
    HAST_HIP_TRY(launch_tx_step(a, t->d_scratch, t->plan, hs));
    HAST_HIP_TRY(hipMemcpyAsync(t->h_st, t->d_scratch + t->plan.state, sizeof(TxDevState), hipMemcpyDeviceToHost, hs));
    HAST_HIP_TRY(hipStreamSynchronize(hs));
    const TxDevState &s = *t->h_st;
    res->consumed1 = s.consumed[0];
    res->consumed2 = s.consumed[1];
    res->pairs = s.pairs;
    res->used = s.used;
    for (int side = 0; side < 2; ++side) {
        res->out_bytes[side] = res->raw_bytes[side] = s.out_bytes[side];
        res->lines[side] = s.lines[side];
    }
    if (s.refused)
        return set_error(HAST_ERR_UNSUPPORTED, "hast_tx_pair_device: the outputs take %llu and %llu bytes, the room is %zu and %zu",
                         (unsigned long long)s.out_bytes[0], (unsigned long long)s.out_bytes[1], cap1, cap2);
    state->used += s.used;
    state->headers += s.pairs;
    return HAST_OK;
}

static double wall() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static hipError_t staging_create(hast_tx *t) {
    TxStaging *io = new (std::nothrow) TxStaging;
    if (!io) return hipErrorOutOfMemory;
    t->io = io;                                                  // (hast_tx_destroy frees what a failure leaves)
    io->cap_out = 2 * t->max_in + 4096;
    io->cap_gz = hast_dz_bound(io->cap_out);
    io->cap_host = io->cap_out > io->cap_gz ? io->cap_out : io->cap_gz;
    hipError_t e = hipSuccess;
    for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        e = pinned_malloc(&io->h_in[s], t->max_in);
        if (e == hipSuccess) e = dev_malloc(&io->d_in[s], t->max_in + 64);
        if (e == hipSuccess) e = dev_malloc(&io->d_out[s], io->cap_out + 64);
        if (e == hipSuccess) e = dev_malloc(&io->d_gz[s], io->cap_gz + 64);
        for (int slot = 0; slot < 2 && e == hipSuccess; ++slot) e = pinned_malloc(&io->h_out[slot][s], io->cap_host);
        if (e == hipSuccess) e = hipEventCreate(&io->ev[s]);
    }
    return e;
}

static void staging_destroy(TxStaging *io) {
    if (!io) return;
    for (int s = 0; s < 2; ++s) {
        if (io->h_in[s]) (void)hipHostFree(io->h_in[s]);
        if (io->d_in[s]) (void)hipFree(io->d_in[s]);
        if (io->d_out[s]) (void)hipFree(io->d_out[s]);
        if (io->d_gz[s]) (void)hipFree(io->d_gz[s]);
        for (int slot = 0; slot < 2; ++slot)
            if (io->h_out[slot][s]) (void)hipHostFree(io->h_out[slot][s]);
        if (io->ev[s]) (void)hipEventDestroy(io->ev[s]);
    }
    delete io;
}

hast_status hast_tx_pair_staged(hast_tx *t, const uint8_t *r1, size_t n1, const uint8_t *r2, size_t n2, hast_tx_state *state, int gz, const uint8_t **out1,
                                const uint8_t **out2, hast_tx_result *res, hast_tx_times *times) {
    if (!t || !state || !out1 || !out2 || !res || !times || (n1 && !r1) || (n2 && !r2)) return set_error(HAST_ERR_INVALID, "null argument");
    *out1 = *out2 = nullptr;
    if (n1 > t->max_in || n2 > t->max_in)
        return set_error(HAST_ERR_UNSUPPORTED, "hast_tx_pair_staged: %zu and %zu bytes, the converter was created for %zu a side", n1, n2, t->max_in);
    HAST_HIP_TRY(hipSetDevice(t->device));
    if (!t->io) {
        const hipError_t e = staging_create(t);
        if (e != hipSuccess) {
            staging_destroy(t->io);
            t->io = nullptr;
            return set_error(e == hipErrorOutOfMemory ? HAST_ERR_OOM : HAST_ERR_HIP, "hast_tx_pair_staged: staging for %zu bytes a side: %s", t->max_in, hipGetErrorString(e));
        }
    }
    TxStaging &io = *t->io;
    const uint8_t *in[2] = {r1, r2};
    const size_t n_in[2] = {n1, n2};
    double t0 = wall();
    for (int s = 0; s < 2; ++s) {
        if (!n_in[s]) continue;
        memcpy(io.h_in[s], in[s], n_in[s]);
        HAST_HIP_TRY(hipMemcpyAsync(io.d_in[s], io.h_in[s], n_in[s], hipMemcpyHostToDevice, t->stream));
    }
    HAST_HIP_TRY(hipStreamSynchronize(t->stream));
    times->upload_s += wall() - t0;
    HAST_HIP_TRY(hipEventRecord(io.ev[0], t->stream));
    hast_tx_state after = *state;                                // (*state is the caller's only once the whole step has succeeded)
    const hast_status st = hast_tx_pair_device(t, io.d_in[0], n1, io.d_in[1], n2, &after, io.d_out[0], 2 * n1 + 4096, io.d_out[1], 2 * n2 + 4096, res, t->stream);
    HAST_HIP_TRY(hipEventRecord(io.ev[1], t->stream));
    HAST_HIP_TRY(hipEventSynchronize(io.ev[1]));
    float ms = 0;
    HAST_HIP_TRY(hipEventElapsedTime(&ms, io.ev[0], io.ev[1]));
    times->kernel_s += 1e-3 * ms;
    if (st != HAST_OK) return st;
    const unsigned slot = io.slot++ & 1;
    const uint8_t *d_from[2] = {io.d_out[0], io.d_out[1]};
    if (gz) {
        t0 = wall();
        for (int s = 0; s < 2; ++s) {
            if (!res->raw_bytes[s]) continue;                    // (an empty run is no member at all, as on the host route)
            size_t n_gz = 0;
            // (a failing encoder is never HAST_ERR_UNSUPPORTED: that status means "take hast_tx_pair_host", and this is trouble)
            if (hast_status zst = hast_dz_compress_device(t->ctx, io.d_out[s], (size_t)res->raw_bytes[s], io.d_gz[s], io.cap_gz, &n_gz, t->stream))
                return zst == HAST_ERR_UNSUPPORTED ? HAST_ERR_HIP : zst;
            res->out_bytes[s] = n_gz;
            d_from[s] = io.d_gz[s];
        }
        times->deflate_s += wall() - t0;
    }
    t0 = wall();
    for (int s = 0; s < 2; ++s)
        if (res->out_bytes[s]) HAST_HIP_TRY(hipMemcpyAsync(io.h_out[slot][s], d_from[s], (size_t)res->out_bytes[s], hipMemcpyDeviceToHost, t->stream));
    HAST_HIP_TRY(hipStreamSynchronize(t->stream));
    times->download_s += wall() - t0;
    *out1 = io.h_out[slot][0];
    *out2 = io.h_out[slot][1];
    *state = after;
    return HAST_OK;
}

void hast_tx_destroy(hast_tx *t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    staging_destroy(t->io);
    if (t->d_scratch) (void)hipFree(t->d_scratch);
    if (t->d_table) (void)hipFree(t->d_table);
    if (t->h_st) (void)hipHostFree(t->h_st);
    delete t;
}

int hast_tx_step_mode(int eof1, int eof2, const uint8_t *r1, size_t n1, const uint8_t *r2, size_t n2) {
    return tx::step_mode(eof1 != 0, eof2 != 0, r1, n1, r2, n2);
}

}  // extern "C"
