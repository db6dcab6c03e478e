// tx_api.cpp -- the part of the C ABI that converts stLFR read pairs into 10x FASTQ (include/hast.h "stage 02"): the map file and
// the conversion of host buffers, both tx_host.h's over the rules of tx_core.h.  Plain host code: nothing here touches a GPU.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <string>
#include <vector>

#include "hast_internal.h"
#include "tx_host.h"

using namespace hast;

struct hast_tx_map {
    tx::Map map;
};

static void fill_info(const tx::Map &m, hast_tx_map_info *info) {
    if (!info) return;
    memset(info, 0, sizeof *info);
    info->n_keys = m.kv.size();
    info->device_ok = m.device_ok ? 1 : 0;
    snprintf(info->reason, sizeof info->reason, "%s", m.reason.c_str());
}

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

int hast_tx_step_mode(int eof1, int eof2, const uint8_t *r1, size_t n1, const uint8_t *r2, size_t n2) {
    return tx::step_mode(eof1 != 0, eof2 != 0, r1, n1, r2, n2);
}

}  // extern "C"
