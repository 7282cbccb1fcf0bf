// The kw_rows handle (include/kwrows.h) as its two translation units share it: kwrows.hip builds the rows and
// their JSON cells, kwemit.hip renders the CSV lines from them.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/kwrows.h"

namespace rw {

struct Tables {
    const int64_t *occ_off;
    const int32_t *occ_ti, *occ_rank, *occ_prev;
    const int64_t *occ_lo, *occ_hi;
    const uint8_t *invalid;
    const uint8_t *keys;
    const int64_t *key_off;
    uint32_t n_patterns;
};

struct Buf {
    void *p = nullptr;
    size_t cap = 0;
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

#define RWCHK(h, x)                                                                    \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            (h)->err = std::string("HIP error ") + hipGetErrorString(e_) + " at " #x; \
            return KW_EHIP;                                                            \
        }                                                                              \
    } while (0)

namespace rw {

constexpr int BLOCK = 256;
constexpr int SCAN_CHUNKS = 512;

// a buffer of at least `bytes` (contents are not kept when it grows)
int ensure(kw_rows *h, Buf &b, size_t bytes);
// exclusive scan of a[0, m) in place; *d_grand (device) receives the total.  chunk: SCAN_CHUNKS words of scratch
void scan_launch(unsigned long long *a, int64_t m, unsigned long long *chunk, unsigned long long *d_grand,
                 hipStream_t st);
// kwemit.hip: frees what kw_rows_cells / kw_rows_emit allocated
void emit_destroy(kw_rows *h);

}  // namespace rw
