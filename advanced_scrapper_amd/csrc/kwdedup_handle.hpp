// libkwmatch: the kw_dedup handle (include/kwdedup.h), shared by dedup.hip (the keep-first run and its kept-rows
// machinery, the set-difference pass) and cdx.hip (the CDX and CSV parsers' row store and the CSV renderer, which
// reads the last run's kept rows).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <unordered_map>

#include "../../include/kwmatch.h"
#include "../../include/kwdedup.h"
#include "kwhandle.hpp"

namespace dd {

struct Scratch {
    uint4 *rowd;             // per kept row, what RowGen needs in one 16-byte load: x, y[7:0] = the raw start
                             //   (40 bits), y[31:8] = the normalised length (LEN_BIG: see len3); z, w = the plan:
                             //   z = the cut j (raw: the length; SLOW_ROW), w = 's' insertion << 31 | the ':80'
                             //   gap's raw position (NO_GAP) (a slow row: its slow-arena word)
    uint32_t *len3;          // per row: normalised length
    unsigned long long *table;
    uint2 *pairs;            // (row, an earlier row with its tag) of every kept row that found one, listed per
                             //   claim of TCLAIM groups: claim c's pairs at [c * 64 * TCLAIM, + pcount[c])
    uint32_t *pcount;        // pairs per claim
    uint32_t *recheck;       // rows compared with their tag's first row from the table (cnt[5] listed)
    uint32_t *collide;       // the CODE_COLLIDE rows (cnt[9] listed; a list longer than COLLIDE_CAP: the host
                             //   finds them by a scan of the codes)
    uint64_t mask;
    uint32_t epoch;          // this run's table epoch (1..255): a slot of another epoch is empty, so the table is
                             //   cleared only when it moves, grows or the epoch wraps (the memset cost 1.4 ms a run)
    unsigned long long *cnt;   // [0], [2], [3], [4]: rows per code but KEPT; [5] differing pairs;
                               // [7] the transform's next group of 64 rows; [9] CODE_COLLIDE rows listed;
                               // the set-difference pass: [11] rows listed for the host, [12] rows seen
    unsigned long long *gnext;   // &cnt[7]
    int weak;                // tests: hash h1 down to 4 bits (forces the collision path)
    int stats;               // KW_DEDUP_STATS: print the differing pairs (rows looked up in the table)
    int normalize;           // KW_DEDUP_NORMALIZE: apply :63-76; else keep-first over the raw strings
    uint2 *slow;             // rows (index, cut) for the byte-serial rewrite (capacity: every row)
    unsigned long long *nslow;   // [0] slow rows listed, [1] slow-arena words they may need, [2] words handed out
    uint64_t *sarena;        // the slow rows' normalised words (sized after the transform from nslow[1])
};

}  // namespace dd

struct kw_cdx_store;                            // the CDX row store and renderer state (cdx.hip)
void kw_cdx_store_destroy(kw_cdx_store *s);     // frees it (nullptr: nothing); the handle's device is current

struct kw_dedup {
    int device = 0;
    int cus = 256;
    int copy_bpc = 4, pairs_bpc = 4, copys_bpc = 16;   // resident blocks per CU of the statically divided kernels (one round of
                                       // blocks: a second partial round left CUs idle at the end)
    std::string err;
    void *d_buf = nullptr;
    size_t buf_bytes = 0;
    dd::Scratch S{};
    unsigned long long *tile_cnt = nullptr, *tile_bytes = nullptr, *totals = nullptr;
    unsigned long long *chunk_cnt = nullptr, *chunk_bytes = nullptr;   // the tile scan's chunk sums
    int64_t *kept_off = nullptr, *kept_row = nullptr;
    uint8_t *kept_bytes = nullptr;
    size_t kept_bytes_cap = 0;
    void *d_kept = nullptr;
    void *d_collide = nullptr;   // count + list of the CODE_COLLIDE rows
    void *d_sarena = nullptr;    // the slow rows' normalised words
    size_t sarena_bytes = 0;
    int64_t n = 0, n_kept = 0, n_kept_bytes = 0;
    void *table_at = nullptr;   // where the table was last cleared, its slots, the epoch of the last run
    uint64_t table_slots = 0;
    uint32_t epoch = 0;
    int64_t counts[4] = {0, 0, 0, 0};
    int64_t route[4] = {0, 0, 0, 0};   // the last run's slow rows, differing pairs, CODE_COLLIDE rows, rows listed
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool have_run = false;
    uint64_t run_serial = 0;       // kw_dedup_run calls so far (the renderer checks the kept rows are its run's)
    kw_cdx_store *cdx = nullptr;   // kw_cdx_* (cdx.hip)
    // the URLs the host's exact pass of the last run saw (normalised bytes) and the first row holding each
    std::unordered_map<std::string, uint32_t> collide_first;
    // kw_cdx_run_exclude: the run it belongs to (0: none), link rows, rows seen; then the kept buffers hold the
    // remaining rows
    bool no_compact = false;       // set around kw_cdx_run_exclude's kw_dedup_run: no kept rows wanted of it
    uint64_t ex_serial = 0;
    int64_t ex_links = 0, ex_seen = 0;
    int64_t ex_dup = 0;            // kw_cdx_run_exclude_unique: link rows whose first holder is an earlier link row
    hipEvent_t ex_ev[3] = {nullptr, nullptr, nullptr};
};

// dedup.hip: the set-difference pass over the last kw_dedup_run's rows (a raw run over the same arena, offsets and
// codes): the first m rows are the exclude rows; unique: repeats among the link rows are dropped too
int kw_dedup_exclude_pass(kw_dedup *h, const uint8_t *d_arena, int64_t m, uint8_t *d_code, bool unique, hipStream_t st);

// dedup.hip: after kw_dedup_exclude_pass over the same rows, out[0] = the distinct strings among the link rows coded
// KW_URL_SEEN, out[1] = the exclude rows the keep-first run coded KW_URL_KEPT
int kw_dedup_distinct_seen(kw_dedup *h, const uint8_t *d_arena, int64_t m, const uint8_t *d_code, int64_t *out,
                           hipStream_t st);
