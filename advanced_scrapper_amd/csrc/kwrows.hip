// libkwmatch: the per-ticker match cells built on the device (include/kwrows.h) -- the reference's per-article
// assembly (match_keywords.py:159-187) and json.dumps of the two dicts (:137-138), from hit records that are
// already in HBM.  The host form of the same rules is csrc/kwrows.c; tests/rows_rule.py restates the stages.
// csrc/kwemit.hip goes on from the rows to the finished CSV lines on the same handle (kwrows_handle.hpp).
//
// Stages of kw_rows_run (kernels exchange data only across launches; every size is found by a count pass and
// an exclusive scan, the buffers belong to the handle and grow on demand):
//   order    rw_count_kernel    records per document (documents without a date and doc >= n_docs count nothing)
//            scan_launch        the device scan of kwhandle.hpp (kwscan.hip)
//            rw_scatter_kernel  records into their document's segment (any order inside it)
//            rw_sort_kernel     a lane per record ranks it inside its segment by (field, pattern, pos): the
//                               segment is read by every lane that shares it (broadcast loads), so a document
//                               of m records costs m * m compares and any m is exact; config 2 has m ~ 4
//   expand   rw_groups_kernel   a lane per (doc, field, pattern) group head: over the pattern's occurrences, the
//                               period test and "first in-period occurrence per ticker" (occ_prev chains the
//                               earlier occurrences of the same ticker); pass 1 counts entries, pass 2 writes
//                               {doc, ticker, field, rank | pattern, first record, last record, position bytes}
//            rw_esort_kernel    a lane per entry ranks it inside its document by (ticker, field, rank)
//   render   rw_len_kernel      row heads and each entry's exact byte length (with the braces and separators
//                               it owns), then two scans: byte offsets and row numbers
//            rw_fill_kernel     a lane per entry writes its bytes, its row's doc / ticker and the row's offsets
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/kwrows.h"
#include "kwrows_handle.hpp"

namespace rw {

constexpr uint32_t NOPOS = KW_NOPOS;
// the run's counters (device, 64-bit words)
enum { T_VALID = 0, T_ENTRIES = 1, T_INVALID = 2, T_BADPAT = 3, T_BYTES = 4, T_ROWS = 5, T_WORDS = 8 };

// ---- order
// a record as one 16-byte word: x = doc, y = pattern, z = pos, w = field (kw_hit)
__device__ __forceinline__ bool rec_counts(const uint4 r, uint32_t n_docs, const uint8_t *__restrict__ date_ok)
{
    return r.x < n_docs && date_ok[r.x] != 0;
}

__global__ __launch_bounds__(BLOCK) void rw_count_kernel(const uint4 *__restrict__ hits, uint32_t n_hits,
                                                         uint32_t n_docs, const uint8_t *__restrict__ date_ok,
                                                         unsigned long long *__restrict__ doc_cnt)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_hits) return;
    const uint4 r = hits[i];
    if (rec_counts(r, n_docs, date_ok)) atomicAdd(&doc_cnt[r.x], 1ull);
}

__global__ __launch_bounds__(BLOCK) void rw_scatter_kernel(const uint4 *__restrict__ hits, uint32_t n_hits,
                                                           uint32_t n_docs, const uint8_t *__restrict__ date_ok,
                                                           const unsigned long long *__restrict__ doc_off,
                                                           uint32_t *__restrict__ cursor, uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_hits) return;
    const uint4 r = hits[i];
    if (!rec_counts(r, n_docs, date_ok)) return;
    out[doc_off[r.x] + atomicAdd(&cursor[r.x], 1u)] = r;   // < doc_off[r.x + 1]: the count pass saw this record
}

// (field, pattern, pos) of a before b
__device__ __forceinline__ bool rec_less(const uint4 a, const uint4 b)
{
    if (a.w != b.w) return a.w < b.w;
    if (a.y != b.y) return a.y < b.y;
    return a.z < b.z;
}

__global__ __launch_bounds__(BLOCK) void rw_sort_kernel(const uint4 *__restrict__ in,
                                                        const unsigned long long *__restrict__ tot,
                                                        const unsigned long long *__restrict__ doc_off,
                                                        uint4 *__restrict__ out)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= tot[T_VALID]) return;
    const uint4 r = in[i];
    const uint32_t s = (uint32_t)doc_off[r.x], e = (uint32_t)doc_off[r.x + 1];
    uint32_t rank = 0;
    for (uint32_t j = s; j < e; ++j) {
        const uint4 o = in[j];
        rank += (rec_less(o, r) || (!rec_less(r, o) && j < i)) ? 1u : 0u;
    }
    out[s + rank] = r;
}

// ---- expand
__device__ __forceinline__ bool in_period(const Tables &T, int64_t o, int64_t date)
{
    return T.occ_lo[o] <= date && date <= T.occ_hi[o];
}

// occurrence o of its pattern is an entry: in period, and no earlier occurrence of the same ticker is
__device__ __forceinline__ bool occ_is_entry(const Tables &T, int64_t o, int64_t date)
{
    if (!in_period(T, o, date)) return false;
    for (int32_t q = T.occ_prev[o]; q >= 0; q = T.occ_prev[q])
        if (in_period(T, q, date)) return false;
    return true;
}

__device__ __forceinline__ uint32_t digits10(uint32_t v)
{
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u
         : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}

// WRITE = false: ecnt[i] = entries of the group that record i heads (0 for the other records).
// WRITE = true: ecnt holds the scanned counts; the group's entries go to ent[2 * (ecnt[i] + k)], in table order.
template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void rw_groups_kernel(const uint4 *__restrict__ rec, unsigned long long *__restrict__ tot,
                                                          const unsigned long long *__restrict__ doc_off,
                                                          const int64_t *__restrict__ date_us, Tables T,
                                                          unsigned long long *__restrict__ ecnt, uint4 *__restrict__ ent)
{
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= tot[T_VALID]) return;
    const uint4 r = rec[i];
    const uint32_t s = (uint32_t)doc_off[r.x], e = (uint32_t)doc_off[r.x + 1];
    if (i != s) {
        const uint4 p = rec[i - 1];
        if (p.w == r.w && p.y == r.y) return;   // not a group head (ecnt[i] stays 0)
    }
    if (r.y >= T.n_patterns) {
        if (!WRITE) tot[T_BADPAT] = 1ull;
        return;
    }
    const int64_t date = date_us[r.x];
    const int64_t o0 = T.occ_off[r.y], o1 = T.occ_off[r.y + 1];
    if (!WRITE) {
        unsigned long long n = 0;
        for (int64_t o = o0; o < o1; ++o) n += occ_is_entry(T, o, date) ? 1ull : 0ull;
        if (n && T.invalid[r.y]) tot[T_INVALID] = 1ull;
        ecnt[i] = n;
    } else {
        if (ecnt[i + 1] == ecnt[i]) return;     // (ecnt has one word more than there are records)
        uint32_t ge = i, npos = 0, pbytes = 0;  // the group's end and the bytes of its positions, ", " included
        for (; ge < e; ++ge) {
            const uint4 q = rec[ge];
            if (q.w != r.w || q.y != r.y) break;
            if (q.z != NOPOS) { pbytes += digits10(q.z); ++npos; }
        }
        if (npos > 1) pbytes += 2u * (npos - 1u);
        unsigned long long at = ecnt[i];
        for (int64_t o = o0; o < o1; ++o) {
            if (!occ_is_entry(T, o, date)) continue;
            ent[2 * at] = make_uint4(r.x, (uint32_t)T.occ_ti[o], r.w, (uint32_t)T.occ_rank[o]);
            ent[2 * at + 1] = make_uint4(r.y, i, ge, pbytes);
            ++at;
        }
    }
}

// an entry's first word: x = doc, y = ticker, z = field, w = rank; its second: x = pattern, y / z = the group's
// records [y, z), w = the bytes of its positions
__device__ __forceinline__ bool ent_less(const uint4 a, const uint4 b)
{
    if (a.y != b.y) return (int32_t)a.y < (int32_t)b.y;
    if (a.z != b.z) return a.z < b.z;
    return (int32_t)a.w < (int32_t)b.w;
}

__global__ __launch_bounds__(BLOCK) void rw_esort_kernel(const uint4 *__restrict__ in, uint32_t n_ent,
                                                         const unsigned long long *__restrict__ doc_off,
                                                         const unsigned long long *__restrict__ eoff,
                                                         uint4 *__restrict__ out)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_ent) return;
    const uint4 a = in[2 * (size_t)j];
    const uint32_t s = (uint32_t)eoff[doc_off[a.x]], e = (uint32_t)eoff[doc_off[a.x + 1]];
    uint32_t rank = 0;
    for (uint32_t k = s; k < e; ++k) {
        const uint4 o = in[2 * (size_t)k];
        rank += (ent_less(o, a) || (!ent_less(a, o) && k < j)) ? 1u : 0u;
    }
    out[2 * (size_t)(s + rank)] = a;
    out[2 * (size_t)(s + rank) + 1] = in[2 * (size_t)j + 1];
}

// ---- render
// What entry j writes: [prefix] key ": [" positions "]" [suffix].  The prefix opens the row ("{", or "{}{" when
// the row has no text entry), separates entries (", ") or closes the text dict and opens the title dict ("}{");
// the suffix closes the row ("}", or "}{}" when the row has no title entry).
struct Piece {
    uint32_t prefix, suffix;   // 0 none, else the number of bytes (1: "{" / "}", 2: ", " / "}{", 3: "{}{" / "}{}")
    bool sep;                  // a 2-byte prefix is ", "
    bool row_head, row_last, title, first_title;
};

__device__ __forceinline__ Piece piece_of(const uint4 *__restrict__ ent, uint32_t j, uint32_t n_ent)
{
    const uint4 a = ent[2 * (size_t)j];
    Piece P;
    P.title = a.z != 0;
    P.row_head = true;
    P.row_last = true;
    bool prev_title = false;
    if (j > 0) {
        const uint4 p = ent[2 * (size_t)(j - 1)];
        P.row_head = p.x != a.x || p.y != a.y;
        prev_title = p.z != 0;
    }
    if (j + 1 < n_ent) {
        const uint4 q = ent[2 * (size_t)(j + 1)];
        P.row_last = q.x != a.x || q.y != a.y;
    }
    P.sep = false;
    if (P.row_head) P.prefix = P.title ? 3u : 1u;
    else if (P.title && !prev_title) P.prefix = 2u;
    else { P.prefix = 2u; P.sep = true; }
    P.first_title = P.title && (P.row_head || !prev_title);
    P.suffix = P.row_last ? (P.title ? 1u : 3u) : 0u;
    return P;
}

__global__ __launch_bounds__(BLOCK) void rw_len_kernel(const uint4 *__restrict__ ent, uint32_t n_ent, Tables T,
                                                       unsigned long long *__restrict__ len,
                                                       unsigned long long *__restrict__ head)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_ent) return;
    const Piece P = piece_of(ent, j, n_ent);
    const uint4 b = ent[2 * (size_t)j + 1];
    const unsigned long long key = (unsigned long long)(T.key_off[b.x + 1] - T.key_off[b.x]);
    len[j] = P.prefix + key + 4ull + b.w + P.suffix;   // 4: ": [" and "]"
    head[j] = P.row_head ? 1ull : 0ull;
}

__global__ __launch_bounds__(BLOCK) void rw_fill_kernel(const uint4 *__restrict__ ent, uint32_t n_ent,
                                                        const uint4 *__restrict__ rec, Tables T,
                                                        const unsigned long long *__restrict__ boff,
                                                        const unsigned long long *__restrict__ ridx,
                                                        const unsigned long long *__restrict__ tot,
                                                        uint8_t *__restrict__ out, int64_t *__restrict__ out_off,
                                                        int32_t *__restrict__ row_doc, int32_t *__restrict__ row_ti)
{
    const uint32_t j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= n_ent) return;
    const Piece P = piece_of(ent, j, n_ent);
    const uint4 a = ent[2 * (size_t)j], b = ent[2 * (size_t)j + 1];
    const unsigned long long start = boff[j];
    const unsigned long long r = ridx[j];   // exclusive scan of the heads: a head's own row, else the row + 1
    uint8_t *w = out + start;
    if (P.row_head) {
        row_doc[r] = (int32_t)a.x;
        row_ti[r] = (int32_t)a.y;
        out_off[2 * r] = (int64_t)start;
    }
    const unsigned long long row = P.row_head ? r : r - 1;
    if (P.prefix == 1u) *w++ = '{';
    else if (P.prefix == 3u) { *w++ = '{'; *w++ = '}'; *w++ = '{'; }
    else if (P.sep) { *w++ = ','; *w++ = ' '; }
    else { *w++ = '}'; *w++ = '{'; }
    if (P.first_title) out_off[2 * row + 1] = (int64_t)(w - out) - 1;   // the title dict's '{'
    const uint8_t *k = T.keys + T.key_off[b.x], *kend = T.keys + T.key_off[b.x + 1];
    while (k < kend) *w++ = *k++;
    *w++ = ':'; *w++ = ' '; *w++ = '[';
    bool first = true;
    for (uint32_t i = b.y; i < b.z; ++i) {
        uint32_t v = rec[i].z;
        if (v == NOPOS) continue;
        if (!first) { *w++ = ','; *w++ = ' '; }
        first = false;
        const uint32_t nd = digits10(v);
        for (uint32_t d = nd; d-- > 0;) { w[d] = (uint8_t)('0' + v % 10u); v /= 10u; }
        w += nd;
    }
    *w++ = ']';
    if (P.suffix == 1u) *w++ = '}';
    else if (P.suffix == 3u) {
        *w++ = '}';
        out_off[2 * row + 1] = (int64_t)(w - out);   // no title entry: the empty title dict starts here
        *w++ = '{'; *w++ = '}';
    }
    if (j + 1 == n_ent) out_off[2 * tot[T_ROWS]] = (int64_t)(w - out);
}

}  // namespace rw

extern "C" int kw_rows_create(int32_t device, const int64_t *occ_off, const int32_t *occ_ti, const int32_t *occ_rank,
                              const int64_t *occ_lo, const int64_t *occ_hi, const uint8_t *invalid_rx,
                              const uint8_t *keys, const int64_t *key_off, int32_t n_patterns, int32_t n_tickers,
                              kw_rows **out)
{
    using namespace rw;
    if (!out) return KW_EINVAL;
    kw_rows *h = new kw_rows();
    *out = h;
    h->device = device;
    h->n_patterns = n_patterns;
    h->n_tickers = n_tickers;
    if (n_patterns < 0 || n_tickers < 0 || !occ_off || !key_off || (n_patterns > 0 && !invalid_rx)) {
        h->err = "kw_rows_create: bad arguments";
        return KW_EINVAL;
    }
    if (occ_off[0] != 0 || key_off[0] != 0) { h->err = "kw_rows_create: offsets must start at 0"; return KW_EINVAL; }
    for (int32_t p = 0; p < n_patterns; ++p)
        if (occ_off[p + 1] < occ_off[p] || key_off[p + 1] < key_off[p]) {
            h->err = "kw_rows_create: offsets of pattern " + std::to_string(p) + " decrease";
            return KW_EINVAL;
        }
    const int64_t n_occ = occ_off[n_patterns], n_key = key_off[n_patterns];
    if (n_occ >= (int64_t)1 << 31) { h->err = "kw_rows_create: 2^31 occurrences or more"; return KW_EINVAL; }
    if (n_occ > 0 && (!occ_ti || !occ_rank || !occ_lo || !occ_hi)) { h->err = "kw_rows_create: bad arguments"; return KW_EINVAL; }
    if (n_key > 0 && !keys) { h->err = "kw_rows_create: bad arguments"; return KW_EINVAL; }
    h->n_occ = n_occ;
    // occ_prev[o]: the nearest earlier occurrence of o's pattern with o's ticker (-1: none)
    std::vector<int32_t> prev((size_t)n_occ, -1);
    {
        std::unordered_map<int32_t, int32_t> last;
        for (int32_t p = 0; p < n_patterns; ++p) {
            if (occ_off[p + 1] - occ_off[p] < 2) continue;
            last.clear();
            for (int64_t o = occ_off[p]; o < occ_off[p + 1]; ++o) {
                auto it = last.find(occ_ti[o]);
                if (it != last.end()) { prev[(size_t)o] = it->second; it->second = (int32_t)o; }
                else last.emplace(occ_ti[o], (int32_t)o);
            }
        }
    }
    KWCHK(h, hipSetDevice(device));
    const size_t np1 = (size_t)n_patterns + 1, no = (size_t)n_occ;
    const size_t sizes[9] = {np1 * 8, no * 4, no * 4, no * 4, no * 8, no * 8, (size_t)n_patterns, (size_t)n_key, np1 * 8};
    const void *src[9] = {occ_off, occ_ti, occ_rank, prev.data(), occ_lo, occ_hi, invalid_rx, keys, key_off};
    size_t at[10];
    at[0] = 0;
    for (int k = 0; k < 9; ++k) at[k + 1] = at[k] + align256(sizes[k]);
    KWCHK(h, hipMalloc(&h->d_tables, std::max<size_t>(256, at[9])));
    uint8_t *base = (uint8_t *)h->d_tables;
    for (int k = 0; k < 9; ++k)
        if (sizes[k]) KWCHK(h, hipMemcpy(base + at[k], src[k], sizes[k], hipMemcpyHostToDevice));
    h->T.occ_off = (const int64_t *)(base + at[0]);
    h->T.occ_ti = (const int32_t *)(base + at[1]);
    h->T.occ_rank = (const int32_t *)(base + at[2]);
    h->T.occ_prev = (const int32_t *)(base + at[3]);
    h->T.occ_lo = (const int64_t *)(base + at[4]);
    h->T.occ_hi = (const int64_t *)(base + at[5]);
    h->T.invalid = base + at[6];
    h->T.keys = base + at[7];
    h->T.key_off = (const int64_t *)(base + at[8]);
    h->T.n_patterns = (uint32_t)n_patterns;
    KWCHK(h, hipMalloc((void **)&h->tot, T_WORDS * 8));
    KWCHK(h, hipMalloc((void **)&h->chunk, SCAN_CHUNKS * 8));
    for (auto &e : h->ev) KWCHK(h, hipEventCreate(&e));
    return KW_OK;
}

extern "C" int kw_rows_run(kw_rows *h, const kw_hit *d_hits, int64_t n_hits, const int64_t *date_us,
                           const uint8_t *date_ok, int64_t n_docs, int64_t *n_rows, int64_t *n_bytes, int32_t *verdict,
                           void *stream)
{
    using namespace rw;
    typedef unsigned long long u64;
    if (!h) return KW_EINVAL;
    if (!n_rows || !n_bytes || !verdict || n_hits < 0 || n_docs < 0 || (n_hits > 0 && !d_hits) ||
        (n_docs > 0 && (!date_us || !date_ok))) {
        h->err = "kw_rows_run: bad arguments";
        return KW_EINVAL;
    }
    if (n_hits >= (int64_t)1 << 31 || n_docs >= (int64_t)1 << 31) {
        h->err = "kw_rows_run: 2^31 records or documents, or more";
        return KW_EINVAL;
    }
    if ((uintptr_t)d_hits & 15) { h->err = "kw_rows_run: d_hits must be 16-byte aligned"; return KW_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    h->have_run = false;
    h->run_rows = false;
    h->run_docs = n_docs;
    h->n_rows = h->n_bytes = 0;
    *n_rows = *n_bytes = 0;
    *verdict = KW_ROWS_OK;
    for (auto &m : h->ms) m = 0.f;
    if (n_hits == 0 || n_docs == 0) {
        h->have_run = h->run_rows = true;
        return KW_OK;
    }
    KWCHK(h, hipSetDevice(h->device));
    const uint32_t nh = (uint32_t)n_hits, nd = (uint32_t)n_docs;
    int rc;
    if ((rc = fit(h, h->date_us, (size_t)nd * 8)) || (rc = fit(h, h->date_ok, nd)) ||
        (rc = fit(h, h->doc_off, ((size_t)nd + 1) * 8)) || (rc = fit(h, h->cursor, (size_t)nd * 4)) ||
        (rc = fit(h, h->tmp, (size_t)nh * 16)) || (rc = fit(h, h->rec, (size_t)nh * 16)) ||
        (rc = fit(h, h->ecnt, ((size_t)nh + 1) * 8)))
        return rc;
    const uint4 *hits = (const uint4 *)d_hits;
    u64 *doc_off = (u64 *)h->doc_off.p, *ecnt = (u64 *)h->ecnt.p;
    uint4 *tmp = (uint4 *)h->tmp.p, *rec = (uint4 *)h->rec.p;
    const int64_t *d_date = (const int64_t *)h->date_us.p;
    const uint8_t *d_ok = (const uint8_t *)h->date_ok.p;

    KWCHK(h, hipEventRecord(h->ev[0], st));
    KWCHK(h, hipMemcpyAsync(h->date_us.p, date_us, (size_t)nd * 8, hipMemcpyHostToDevice, st));
    KWCHK(h, hipMemcpyAsync(h->date_ok.p, date_ok, nd, hipMemcpyHostToDevice, st));
    KWCHK(h, hipMemsetAsync(h->tot, 0, T_WORDS * 8, st));
    KWCHK(h, hipMemsetAsync(doc_off, 0, ((size_t)nd + 1) * 8, st));
    KWCHK(h, hipMemsetAsync(h->cursor.p, 0, (size_t)nd * 4, st));
    KWCHK(h, hipMemsetAsync(ecnt, 0, ((size_t)nh + 1) * 8, st));
    // order
    hipLaunchKernelGGL(rw_count_kernel, grid_of(nh), dim3(BLOCK), 0, st, hits, nh, nd, d_ok, doc_off);
    scan_launch(doc_off, (int64_t)nd + 1, h->chunk, h->tot + T_VALID, st);
    hipLaunchKernelGGL(rw_scatter_kernel, grid_of(nh), dim3(BLOCK), 0, st, hits, nh, nd, d_ok, (const u64 *)doc_off,
                       (uint32_t *)h->cursor.p, tmp);
    hipLaunchKernelGGL(rw_sort_kernel, grid_of(nh), dim3(BLOCK), 0, st, (const uint4 *)tmp, (const u64 *)h->tot,
                       (const u64 *)doc_off, rec);
    KWCHK(h, hipEventRecord(h->ev[1], st));
    // expand: count, scan, write, order
    hipLaunchKernelGGL(rw_groups_kernel<false>, grid_of(nh), dim3(BLOCK), 0, st, (const uint4 *)rec, h->tot,
                       (const u64 *)doc_off, d_date, h->T, ecnt, (uint4 *)nullptr);
    scan_launch(ecnt, (int64_t)nh + 1, h->chunk, h->tot + T_ENTRIES, st);
    u64 tot[T_WORDS];
    KWCHK(h, hipMemcpyAsync(tot, h->tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    if (tot[T_BADPAT]) {
        h->err = "kw_rows_run: a record's pattern index is beyond the tables";
        return KW_EINVAL;
    }
    if (tot[T_INVALID]) {
        *verdict = KW_ROWS_INVALID_REGEX;
        h->have_run = true;
        return KW_OK;
    }
    const u64 n_ent = tot[T_ENTRIES];
    if (n_ent >= 1ull << 31) { h->err = "kw_rows_run: 2^31 entries or more"; return KW_EOVERFLOW; }
    if (n_ent == 0) {
        h->have_run = h->run_rows = true;
        return KW_OK;
    }
    if ((rc = fit(h, h->ent_raw, (size_t)n_ent * 32)) || (rc = fit(h, h->ent, (size_t)n_ent * 32)) ||
        (rc = fit(h, h->len, (size_t)n_ent * 8)) || (rc = fit(h, h->head, (size_t)n_ent * 8)))
        return rc;
    uint4 *ent_raw = (uint4 *)h->ent_raw.p, *ent = (uint4 *)h->ent.p;
    u64 *len = (u64 *)h->len.p, *head = (u64 *)h->head.p;
    const uint32_t ne = (uint32_t)n_ent;
    hipLaunchKernelGGL(rw_groups_kernel<true>, grid_of(nh), dim3(BLOCK), 0, st, (const uint4 *)rec, h->tot,
                       (const u64 *)doc_off, d_date, h->T, ecnt, ent_raw);
    hipLaunchKernelGGL(rw_esort_kernel, grid_of(ne), dim3(BLOCK), 0, st, (const uint4 *)ent_raw, ne, (const u64 *)doc_off,
                       (const u64 *)ecnt, ent);
    KWCHK(h, hipEventRecord(h->ev[2], st));
    // render: size, then fill
    hipLaunchKernelGGL(rw_len_kernel, grid_of(ne), dim3(BLOCK), 0, st, (const uint4 *)ent, ne, h->T, len, head);
    scan_launch(len, (int64_t)ne, h->chunk, h->tot + T_BYTES, st);
    scan_launch(head, (int64_t)ne, h->chunk, h->tot + T_ROWS, st);
    KWCHK(h, hipMemcpyAsync(tot, h->tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    const u64 nb = tot[T_BYTES], nr = tot[T_ROWS];
    if ((rc = fit(h, h->json, (size_t)nb)) || (rc = fit(h, h->json_off, (size_t)(2 * nr + 1) * 8)) ||
        (rc = fit(h, h->row_doc, (size_t)nr * 4)) || (rc = fit(h, h->row_ti, (size_t)nr * 4)))
        return rc;
    hipLaunchKernelGGL(rw_fill_kernel, grid_of(ne), dim3(BLOCK), 0, st, (const uint4 *)ent, ne, (const uint4 *)rec, h->T,
                       (const u64 *)len, (const u64 *)head, (const u64 *)h->tot, (uint8_t *)h->json.p,
                       (int64_t *)h->json_off.p, (int32_t *)h->row_doc.p, (int32_t *)h->row_ti.p);
    KWCHK(h, hipEventRecord(h->ev[3], st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    for (int k = 0; k < 3; ++k) KWCHK(h, hipEventElapsedTime(&h->ms[k], h->ev[k], h->ev[k + 1]));
    KWCHK(h, hipEventElapsedTime(&h->ms[3], h->ev[0], h->ev[3]));
    h->n_rows = *n_rows = (int64_t)nr;
    h->n_bytes = *n_bytes = (int64_t)nb;
    h->have_run = h->run_rows = true;
    return KW_OK;
}

extern "C" int kw_rows_copy(kw_rows *h, int32_t *row_doc, int32_t *row_ti, uint8_t *json, int64_t *json_off)
{
    if (!h) return KW_EINVAL;
    if (!h->have_run) { h->err = "kw_rows_copy: no run"; return KW_ESTATE; }
    if (!json_off || (h->n_rows > 0 && (!row_doc || !row_ti)) || (h->n_bytes > 0 && !json)) {
        h->err = "kw_rows_copy: bad arguments";
        return KW_EINVAL;
    }
    if (h->n_rows == 0) {
        json_off[0] = 0;
        return KW_OK;
    }
    KWCHK(h, hipSetDevice(h->device));
    KWCHK(h, hipMemcpy(row_doc, h->row_doc.p, (size_t)h->n_rows * 4, hipMemcpyDeviceToHost));
    KWCHK(h, hipMemcpy(row_ti, h->row_ti.p, (size_t)h->n_rows * 4, hipMemcpyDeviceToHost));
    KWCHK(h, hipMemcpy(json, h->json.p, (size_t)h->n_bytes, hipMemcpyDeviceToHost));
    KWCHK(h, hipMemcpy(json_off, h->json_off.p, (size_t)(2 * h->n_rows + 1) * 8, hipMemcpyDeviceToHost));
    return KW_OK;
}

extern "C" int kw_rows_last_ms(kw_rows *h, float *ms, int32_t n)
{
    if (!h || !ms || n < 0) return KW_EINVAL;
    if (!h->have_run) { h->err = "kw_rows_last_ms: no run"; return KW_ESTATE; }
    for (int32_t k = 0; k < n && k < 4; ++k) ms[k] = h->ms[k];
    return KW_OK;
}

extern "C" const char *kw_rows_last_error(kw_rows *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" int kw_rows_destroy(kw_rows *h)
{
    if (!h) return KW_OK;
    (void)hipSetDevice(h->device);
    rw::emit_destroy(h);
    rw::Buf *bufs[] = {&h->date_us, &h->date_ok, &h->doc_off, &h->cursor, &h->tmp, &h->rec, &h->ecnt, &h->ent_raw,
                       &h->ent, &h->len, &h->head, &h->json, &h->json_off, &h->row_doc, &h->row_ti};
    for (rw::Buf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    if (h->d_tables) (void)hipFree(h->d_tables);
    if (h->tot) (void)hipFree(h->tot);
    if (h->chunk) (void)hipFree(h->chunk);
    for (auto &e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
    return KW_OK;
}
