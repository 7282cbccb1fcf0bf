// The kw_rows handle (include/kwrows.h) as its two translation units share it: kwrows.hip builds the rows and
// their JSON cells, kwemit.hip renders the CSV lines from them.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/kwrows.h"
#include "kwhandle.hpp"

namespace rw {

using namespace kwh;   // Buf, ensure, scan_launch, SCAN_CHUNKS, ...

struct Tables {
    const int64_t *occ_off;
    const int32_t *occ_ti, *occ_rank, *occ_prev;
    const int64_t *occ_lo, *occ_hi;
    const uint8_t *invalid;
    const uint8_t *keys;
    const int64_t *key_off;
    uint32_t n_patterns;
};

struct Emit;   // kwemit.hip: the state of kw_rows_cells / kw_rows_emit

}  // namespace rw

struct kw_rows {
    int device = 0;
    std::string err;
    rw::Tables T{};
    void *d_tables = nullptr;          // one allocation holding every table
    int64_t n_occ = 0;
    int32_t n_patterns = 0, n_tickers = 0;
    rw::Buf date_us, date_ok, doc_off, cursor, tmp, rec, ecnt, ent_raw, ent, len, head, json, json_off, row_doc, row_ti;
    unsigned long long *tot = nullptr, *chunk = nullptr;
    int64_t n_rows = 0, n_bytes = 0;
    int64_t run_docs = 0;              // n_docs of the last kw_rows_run
    bool run_rows = false;             // the last run succeeded with the verdict KW_ROWS_OK: its rows can be rendered
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float ms[4] = {0, 0, 0, 0};
    bool have_run = false;
    rw::Emit *emit = nullptr;
};

namespace rw {

constexpr int BLOCK = 256;

// a buffer of at least `bytes` (contents are not kept when it grows)
inline int fit(kw_rows *h, Buf &b, size_t bytes) { return ensure(h, b, bytes, std::max<size_t>(256, bytes + bytes / 4)); }
// the blocks for `items` lanes
inline dim3 grid_of(uint64_t items) { return grid_for((long long)items, BLOCK, INT64_MAX); }
// kwemit.hip: frees what kw_rows_cells / kw_rows_emit allocated
void emit_destroy(kw_rows *h);

}  // namespace rw
