// libkwmatch: the output sort on the device (include/kwsort.h) -- over the cells, flags and record spans an OK
// kw_ingest_parse of a per-ticker file's body left in device memory: the time_unix keys, the verdict of the take
// rule of kwsort.h, and the records laid out again in the order the host's np.argsort of the keys gives.
//
//   ks_rows_kernel    lane = row: the key from the time_unix cell (the canonical decimal form, inside int64), the
//                     FORM condition over the row's cells, the text / not-NA witnesses of the row's block and
//                     column, the record's bytes + 1 into the body's length.
//   ks_check_kernel   lane = row: a key that does not exceed the row before (not ascending); lane = block x column:
//                     the first one without a text witness that is not all NA.
//   ks_len_kernel     lane = order entry: its range check; the record's bytes + 1, scanned inside a tile of 256.
//   ks_scan_kernel    one block: the exclusive scan of the tiles' sums, the body's bytes.
//   ks_add_kernel     lane = order entry: the sum of the tiles before its own onto its offset.
//   ks_copy_kernel    lane = 16 body bytes, a wave = 1 to 16 KiB one after the other: the record of the wave's
//                     first byte by binary search in the scanned offsets, once; a KiB that lies inside one
//                     record's bytes is copied with one 16-byte load (at the source's own alignment) and one
//                     16-byte store a lane; in the others the lanes search on between the records of the KiB's
//                     first and last byte, and only a lane that holds a record's end goes byte by byte.
// kw_sort_keys synchronises once; kw_sort_gather twice (the body's size is known after the scan, and with it the
// range check's result: nothing is copied for a bad order).
//
// A file of several windows (kw_sort_begin / kw_sort_window / kw_sort_finish): ks_rows_kernel takes a row base and
// a text base, so a window's keys, offenders and witnesses land at the file's own row and block numbers and its
// spans at the store's positions; ks_check_kernel takes a row range, so a window's first key is held against the
// last key of the window before, and runs over the blocks once, at the end.  The state (Dev), the keys and the
// witnesses stay on the device from window to window, in buffers that keep their contents when they grow.
// kw_sort_gather_slab runs ks_copy_kernel over one slab's byte range of the scanned offsets; every position in
// the store and in the output is 64-bit.
//
// A file described by its write index (kw_sort_index_begin / kw_sort_index_window / kw_sort_index_finish): the
// records' lengths come from the host, nothing is parsed, and the route ends in the state a taken kw_sort_finish
// leaves, in front of the same gather.
//   ks_span_kernel      lane = record: its length (the terminator included), scanned inside a tile of 256 into rs;
//                       a length below 1 or above the body offends.
//   ks_span_add_kernel  lane = record: the sum of the tiles before its own (ks_scan_kernel) onto rs, re = the place
//                       of its terminator; a record that ends beyond the body offends.
//   ks_term_kernel      lane = record: the store's byte at re is '\n', or the index does not describe the body.
// The body arrives through two pinned slots of the handle, one asynchronous copy a window behind the last one.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/kwsort.h"
#include "kwdev.hpp"
#include "kwhandle.hpp"

namespace ks {

using namespace kwd;   // BLOCK, NONE and the primitives
using namespace kwh;
typedef unsigned long long u64;
constexpr int MAX_GRID = 2048;
constexpr uint32_t F_QUOTED = 1u, F_NA = 2u, F_TEXT = 4u, F_CANON = 8u;   // KWCSV_* (csrc/kwcsv.c)
constexpr int COL_BITS = 12;                                              // ncols <= 4096 (kw_ingest_create)

// a call's state on the device; copied to the host at each synchronisation
struct Dev {
    u64 first_key, first_form, first_dtype;   // the first offender of each condition (NONE)
    u64 body_bytes;                           // the rows' bytes + 1 each
    u64 total;                                // kw_sort_gather: the body's bytes
    int not_asc, bad_order;
    u64 first_len, first_term;                // the index route: the first row of a bad length, of a missing '\n' (NONE)
};

// The int64 a cell of the canonical decimal form `0` or `-?[1-9][0-9]*` holds; false for any other cell.
__device__ __forceinline__ bool parse_key(const uint8_t *__restrict__ s, long long len, long long *key)
{
    if (len < 1 || len > 20) return false;
    int i = 0;
    const bool neg = s[0] == '-';
    if (neg) i = 1;
    const int nd = (int)len - i;
    if (nd < 1 || nd > 19) return false;
    if (s[i] == '0') {
        if (nd != 1 || neg) return false;
        *key = 0;
        return true;
    }
    u64 mag = 0;   // (19 digits stay below 2^64)
    for (; i < (int)len; ++i) {
        const uint32_t d = (uint32_t)s[i] - '0';
        if (d > 9u) return false;
        mag = mag * 10ull + d;
    }
    if (mag > (1ull << 63) - (neg ? 0ull : 1ull)) return false;
    *key = (long long)(neg ? 0ull - mag : mag);
    return true;
}

__global__ __launch_bounds__(BLOCK) void ks_rows_kernel(const uint8_t *__restrict__ cells,
                                                        const long long *__restrict__ coff,
                                                        const uint8_t *__restrict__ cfl,
                                                        const long long *__restrict__ rs,
                                                        const long long *__restrict__ re, long long n, int ncols, int ti,
                                                        long long block_rows, long long *__restrict__ keys,
                                                        uint8_t *__restrict__ btext, uint8_t *__restrict__ bnonna,
                                                        Dev *__restrict__ D, long long base, long long tbase,
                                                        long long *__restrict__ srs, long long *__restrict__ sre)
{
    const long long rounds = (n + BLOCK - 1) / BLOCK;   // (every lane of a wave makes the same trips)
    for (long long q = blockIdx.x; q < rounds; q += gridDim.x) {
        const long long r = q * BLOCK + threadIdx.x;
        u64 ek = NONE, ef = NONE, bytes = 0;
        if (r < n) {
            const long long c0 = r * ncols;
            long long key = 0;
            {
                const long long c = c0 + ti, s = coff[c];
                if ((cfl[c] & (F_NA | F_QUOTED)) || !parse_key(cells + s, coff[c + 1] - s, &key)) ek = (u64)(base + r);
            }
            keys[base + r] = key;
            const long long blk = ((base + r) / block_rows) * ncols;
            for (int c = 0; c < ncols; ++c) {
                const uint32_t fl = cfl[c0 + c];
                if (ef == NONE && (!(fl & F_CANON) || ((fl & F_NA) && coff[c0 + c + 1] != coff[c0 + c])))
                    ef = ((u64)(base + r) << COL_BITS) | (u64)c;
                if (c != ti) {
                    if ((fl & F_TEXT) && !btext[blk + c]) btext[blk + c] = 1;
                    if (!(fl & F_NA) && !bnonna[blk + c]) bnonna[blk + c] = 1;
                }
            }
            bytes = (u64)(re[r] - rs[r] + 1);
            if (srs) {   // (a window: the record's span at its place in the store)
                srs[base + r] = tbase + rs[r];
                sre[base + r] = tbase + re[r];
            }
        }
        if (__any((ek & ef) != NONE)) {   // (rare: one atomic a wave and condition)
            ek = wave_min(ek);
            ef = wave_min(ef);
            if ((threadIdx.x & 63) == 0) {
                if (ek != NONE) atomicMin(&D->first_key, ek);
                if (ef != NONE) atomicMin(&D->first_form, ef);
            }
        }
        bytes = wave_sum(bytes);
        if ((threadIdx.x & 63) == 0 && bytes) atomicAdd(&D->body_bytes, bytes);
    }
}

__global__ __launch_bounds__(BLOCK) void ks_check_kernel(const long long *__restrict__ keys, long long r0, long long n,
                                                         const uint8_t *__restrict__ btext,
                                                         const uint8_t *__restrict__ bnonna, long long nbc, int ncols,
                                                         int ti, Dev *__restrict__ D)
{
    const long long step = (long long)gridDim.x * BLOCK, t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    for (long long r = r0 + t; r < n; r += step)   // (r0 >= 1: rows [r0, n) against the row before)
        if (keys[r] <= keys[r - 1] && !D->not_asc) D->not_asc = 1;
    for (long long i = t; i < nbc; i += step)
        if ((int)(i % ncols) != ti && !btext[i] && bnonna[i]) atomicMin(&D->first_dtype, (u64)i);
}

// A tile = BLOCK order entries: each one's range check and its record's bytes + 1, scanned inside the tile into
// doff; the tile's sum to tsum[tile].
__global__ __launch_bounds__(BLOCK) void ks_len_kernel(const long long *__restrict__ order, long long n, long long n_rows,
                                                       const long long *__restrict__ rs,
                                                       const long long *__restrict__ re, u64 *__restrict__ doff,
                                                       u64 *__restrict__ tsum, Dev *__restrict__ D)
{
    __shared__ u64 ws[BLOCK / 64];
    const long long ntiles = (n + BLOCK - 1) / BLOCK;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // (block-uniform trip count)
        const long long j = tile * BLOCK + threadIdx.x;
        u64 len = 0;
        if (j < n) {
            const long long o = order[j];
            if (o < 0 || o >= n_rows) {
                if (!D->bad_order) D->bad_order = 1;
            } else {
                len = (u64)(re[o] - rs[o] + 1);
            }
        }
        u64 total;
        const u64 before = block_scan(len, ws, &total);
        if (j < n) doff[j] = before;
        if (threadIdx.x == 0) tsum[tile] = total;
    }
}

// the exclusive scan of a[0, m) in place by one block (the tiles' sums: m = n / BLOCK); its sum to *total
__global__ __launch_bounds__(BLOCK) void ks_scan_kernel(u64 *__restrict__ a, long long m, u64 *__restrict__ total)
{
    __shared__ u64 ws[BLOCK / 64];
    u64 carry = 0;
    for (long long i0 = 0; i0 < m; i0 += BLOCK) {   // (block-uniform trip count)
        const long long i = i0 + threadIdx.x;
        u64 all;
        const u64 before = block_scan(i < m ? a[i] : 0ull, ws, &all);
        if (i < m) a[i] = carry + before;
        carry += all;
    }
    if (threadIdx.x == 0) *total = carry;
}

// doff[j] += the sum of the tiles before j's; doff[n] = the body's bytes
__global__ __launch_bounds__(BLOCK) void ks_add_kernel(u64 *__restrict__ doff, long long n, const u64 *__restrict__ tsum,
                                                       const u64 *__restrict__ total)
{
    const long long step = (long long)gridDim.x * BLOCK, t = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (t == 0) doff[n] = *total;
    for (long long j = t; j < n; j += step) doff[j] += tsum[j / BLOCK];
}

// ---- the index route: the records' spans from their lengths, not from a parse
// A tile = BLOCK records: each one's length (its terminator included), scanned inside the tile into rs; the tile's
// sum to tsum[tile].  A length below 1 or above the body's bytes offends and counts 0.
__global__ __launch_bounds__(BLOCK) void ks_span_kernel(const long long *__restrict__ lens, long long n, long long body,
                                                        long long *__restrict__ rs, u64 *__restrict__ tsum,
                                                        Dev *__restrict__ D)
{
    __shared__ u64 ws[BLOCK / 64];
    const long long ntiles = (n + BLOCK - 1) / BLOCK;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {   // (block-uniform trip count)
        const long long j = tile * BLOCK + threadIdx.x;
        u64 len = 0, bad = NONE;
        if (j < n) {
            const long long l = lens[j];
            if (l < 1 || l > body) bad = (u64)j; else len = (u64)l;
        }
        if (__any(bad != NONE)) {   // (rare: one atomic a wave)
            bad = wave_min(bad);
            if ((threadIdx.x & 63) == 0) atomicMin(&D->first_len, bad);
        }
        u64 total;
        const u64 before = block_scan(len, ws, &total);
        if (j < n) rs[j] = (long long)before;
        if (threadIdx.x == 0) tsum[tile] = total;
    }
}

// rs[j] += the sum of the tiles before j's: the bytes before record j; re[j] = the place of its last byte, the
// terminator.  A record that ends beyond the body offends: up to the first such row no sum has wrapped (every
// length counted lies in [1, body]), so the first offender is exact and the rows before it lie inside the store.
__global__ __launch_bounds__(BLOCK) void ks_span_add_kernel(const long long *__restrict__ lens, long long n,
                                                            long long body, long long *__restrict__ rs,
                                                            long long *__restrict__ re, const u64 *__restrict__ tsum,
                                                            Dev *__restrict__ D)
{
    const long long rounds = (n + BLOCK - 1) / BLOCK;   // (every lane of a wave makes the same trips)
    for (long long q = blockIdx.x; q < rounds; q += gridDim.x) {
        const long long j = q * BLOCK + threadIdx.x;
        u64 bad = NONE;
        if (j < n) {
            const long long l = lens[j];
            const u64 s = (u64)rs[j] + tsum[q];
            rs[j] = (long long)s;
            re[j] = (long long)(s + (u64)l - 1ull);
            if (l >= 1 && l <= body && s + (u64)l > (u64)body) bad = (u64)j;
        }
        if (__any(bad != NONE)) {
            bad = wave_min(bad);
            if ((threadIdx.x & 63) == 0) atomicMin(&D->first_len, bad);
        }
    }
}

// lane = record: the store's byte at the record's last place is its '\n', or the index does not describe the body
__global__ __launch_bounds__(BLOCK) void ks_term_kernel(const uint8_t *__restrict__ store,
                                                        const long long *__restrict__ re, long long n,
                                                        Dev *__restrict__ D)
{
    const long long rounds = (n + BLOCK - 1) / BLOCK;   // (every lane of a wave makes the same trips)
    for (long long q = blockIdx.x; q < rounds; q += gridDim.x) {
        const long long j = q * BLOCK + threadIdx.x;
        u64 bad = NONE;
        if (j < n && store[re[j]] != 0x0A) bad = (u64)j;
        if (__any(bad != NONE)) {   // (rare: one atomic a wave)
            bad = wave_min(bad);
            if ((threadIdx.x & 63) == 0) atomicMin(&D->first_term, bad);
        }
    }
}

typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));   // 16 bytes at any address

// A lane's 16 bytes from out position x0 < total, its record among [lo, l2] (doff[lo] <= x0, the record of the
// wave's last byte is l2): one 16-byte load where they lie inside one record's bytes, else byte by byte.
__device__ __forceinline__ uint4 copy_lane(const uint8_t *__restrict__ text, const long long *__restrict__ rs,
                                           const long long *__restrict__ order, const u64 *__restrict__ doff,
                                           u64 total, u64 x0, long long lo, long long l2)
{
    long long s = lo, hi = l2 + 1;   // the last record with doff[s] <= x0
    while (hi - s > 1) {
        const long long mid = (s + hi) >> 1;
        if (doff[mid] <= x0) s = mid; else hi = mid;
    }
    u64 seg_lo = doff[s], seg_end = doff[s + 1];
    const uint8_t *src = text + rs[order[s]];
    if (x0 + 16 < seg_end) {   // 16 bytes of one record (its '\n' stands at seg_end - 1)
        const u32x4_u v = *(const u32x4_u *)(src + (x0 - seg_lo));
        return make_uint4(v.x, v.y, v.z, v.w);
    }
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    #pragma unroll
    for (int k = 0; k < 16; ++k) {
        const u64 x = x0 + k;
        if (x < total) {
            while (x >= seg_end) {   // (x < total = doff[n]: s + 1 <= n - 1)
                ++s;
                seg_lo = seg_end;
                seg_end = doff[s + 1];
                src = text + rs[order[s]];
            }
            const uint32_t b = (x == seg_end - 1 ? 0x0Au : (uint32_t)src[x - seg_lo]) << (8 * (k & 3));
            if (k < 4) w0 |= b; else if (k < 8) w1 |= b; else if (k < 12) w2 |= b; else w3 |= b;
        }
    }
    return make_uint4(w0, w1, w2, w3);
}

// out[doff[j], doff[j + 1]) = the bytes of record order[j], then '\n'; doff[n] = the body's bytes (what follows
// them up to the next multiple of 16 is written as zeros).  Every order entry has passed ks_len_kernel's check.
// A wave lays out `iters` KiB one after the other: it searches the record of its first byte once, and from then
// on the record of a KiB's first byte is the record of the last KiB's last byte or the next one.
__global__ __launch_bounds__(BLOCK) void ks_copy_kernel(const uint8_t *__restrict__ text,
                                                        const long long *__restrict__ rs,
                                                        const long long *__restrict__ order,
                                                        const u64 *__restrict__ doff, long long n,
                                                        uint8_t *__restrict__ out, int iters, u64 x_lo, u64 x_hi)
{
    // the bytes [x_lo, total) of the body, total = min(x_hi, doff[n]), to out[0, total - x_lo): x_lo is a multiple
    // of 1024, and x_hi is one or lies at doff[n] or beyond
    const u64 total = x_hi < doff[n] ? x_hi : doff[n];
    const u64 wspan = (u64)iters << 10;
    const u64 nspans = total > x_lo ? (total - x_lo + wspan - 1) / wspan : 0;
    const u64 wv = (u64)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (a scalar)
    const u64 lane16 = (u64)(threadIdx.x & 63) << 4;
    out -= x_lo;                                  // (out + x: the place of the body's byte x)
    for (u64 sp = (u64)blockIdx.x * (BLOCK / 64) + wv; sp < nspans; sp += (u64)gridDim.x * (BLOCK / 64)) {
        u64 w0 = x_lo + sp * wspan;               // the first byte of the wave's next KiB (wave-uniform, as all below)
        // (a record may go on past a range's end: the whole KiBs stop at the range's end rounded up to a KiB, which
        // is the end itself unless the body ends there, and then no record goes on)
        const u64 tend = (total + 1023) & ~1023ull;
        const u64 send = w0 + wspan < tend ? w0 + wspan : tend, wend = send < total ? send : total;
        long long lo = 0, hi = n;                 // the last record with doff[lo] <= w0
        while (hi - lo > 1) {
            const long long mid = (lo + hi) >> 1;
            if (doff[mid] <= w0) lo = mid; else hi = mid;
        }
        u64 d0 = doff[lo], d1 = doff[lo + 1];
        const uint8_t *src0 = text + rs[order[lo]];
        while (w0 < wend) {
            if (w0 >= d1) {                       // (one step at most; w0 < total = doff[n]: lo + 1 <= n - 1)
                ++lo;
                d0 = d1;
                d1 = doff[lo + 1];
                src0 = text + rs[order[lo]];
            }
            if (w0 + 1024 < d1) {
                // whole KiBs inside the record's bytes (its '\n' stands at d1 - 1): one 16-byte load at the
                // source's own alignment and one aligned store a lane and KiB
                u64 m = (d1 - 1 - w0) >> 10;
                const u64 room = (send - w0) >> 10;
                if (m > room) m = room;
                const uint8_t *src = src0 + (w0 - d0) + lane16;
                uint8_t *dst = out + w0 + lane16;
                #pragma unroll 4
                for (u64 k = 0; k < m; ++k) {
                    const u32x4_u v = *(const u32x4_u *)(src + (k << 10));
                    *(uint4 *)(dst + (k << 10)) = make_uint4(v.x, v.y, v.z, v.w);
                }
                w0 += m << 10;
                continue;
            }
            // a KiB with a record's end in it: the record of its last byte, by a galloping search from lo
            const u64 wl = w0 + 1023 < total - 1 ? w0 + 1023 : total - 1;
            long long a = lo, step = 1;
            while (a + step < n && doff[a + step] <= wl) {
                a += step;
                step <<= 1;
            }
            long long b = a + step < n ? a + step : n;   // doff[a] <= wl < doff[b]
            while (b - a > 1) {
                const long long mid = (a + b) >> 1;
                if (doff[mid] <= wl) a = mid; else b = mid;
            }
            const u64 x0 = w0 + lane16;
            if (x0 < total) *(uint4 *)(out + x0) = copy_lane(text, rs, order, doff, total, x0, lo, a);
            if (a != lo) {
                lo = a;
                d0 = doff[lo];
                d1 = doff[lo + 1];
                src0 = text + rs[order[lo]];
            }
            w0 += 1024;
        }
    }
}


}  // namespace ks

struct kw_sort {
    int device = 0;
    std::string err;
    ks::Dev *D = nullptr;          // device
    ks::Dev *H = nullptr;          // pinned host copy
    ks::Buf keys, btext, bnonna, order, doff, tsum, out;
    void *h_keys = nullptr, *h_out = nullptr;   // pinned
    size_t h_keys_cap = 0, h_out_cap = 0;
    hipEvent_t ev[9] = {};
    float ms[4] = {0, 0, 0, 0};
    float ms_keys_copy = 0;
    // what the last taken kw_sort_keys or kw_sort_finish saw (kw_sort_gather, kw_sort_gather_begin)
    bool have = false;
    const uint8_t *text = nullptr;
    const int64_t *rs = nullptr, *re = nullptr;
    long long n_rows = 0;
    hipStream_t stream = nullptr;
    // a file of several windows (kw_sort_begin .. kw_sort_finish): the store of its body's text, its records'
    // spans in the store, and what the windows so far have added
    ks::Buf store, srs, sre;
    bool open = false;
    int time_col = 0, ncols = 0;
    long long block_rows = 0, expect = 0, used = 0, rows = 0;
    // the slabs of kw_sort_gather_begin: the last scan's shape, two device and two pinned host slabs in turn
    bool scanned = false;
    long long g_n = 0, slab_bytes = 0, n_slabs = 0, pre_k = -1;
    unsigned long long g_total = 0;
    int last_slot = 1;
    ks::Buf slab[2];
    void *h_slab[2] = {nullptr, nullptr};
    size_t h_slab_cap[2] = {0, 0};
    // the index route (kw_sort_index_begin .. kw_sort_index_finish): two pinned staging slots, each one's copy to the
    // store between its two events while `busy`; the records' lengths stand in `keys` until the spans are made
    bool iopen = false;
    void *h_stage[2] = {nullptr, nullptr};
    size_t h_stage_cap[2] = {0, 0};
    bool busy[2] = {false, false};
    hipEvent_t wev[2][2] = {};
};


namespace ks {

// a device buffer of at least `bytes` (contents are not kept when it grows)
static int fit(kw_sort *h, Buf &b, size_t bytes) { return ensure(h, b, bytes, bytes + bytes / 4 + 256); }

// a device buffer of at least `bytes` that keeps its first `keep` bytes when it grows (to twice the bytes asked
// for: a file's windows ask for a little more each); what a grown buffer holds beyond them is zero
static int fit_keep(kw_sort *h, Buf &b, size_t bytes, size_t keep, hipStream_t st)
{
    return ensure_keep(h, b, bytes, keep, 2 * bytes + 256, true, st);
}

static int fit_pinned(kw_sort *h, void **p, size_t *cap, size_t bytes)
{
    return ensure_pinned(h, p, cap, bytes, bytes + bytes / 4 + 4096);
}

// The cap on every launch grid of a call: MAX_GRID, or the tests' KW_TEST_SORT_GRID in [1, MAX_GRID] (read per
// call: the kernels' loops then make several trips on a small file).
static int grid_cap() { return (int)env_int("KW_TEST_SORT_GRID", 1, MAX_GRID, MAX_GRID); }

// The most bytes a store may hold: the tests' KW_TEST_SORT_STORE_MAX, else no cap of its own.
static long long store_cap() { return env_int("KW_TEST_SORT_STORE_MAX", 0, INT64_MAX, INT64_MAX); }

}  // namespace ks

using namespace ks;

extern "C" int kw_sort_create(int32_t device, kw_sort **out)
{
    if (!out) return KW_EINVAL;
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return KW_EHIP;
    kw_sort *h = new kw_sort();
    h->device = device;
    bool ok = hipMalloc((void **)&h->D, sizeof(Dev)) == hipSuccess &&
              hipHostMalloc((void **)&h->H, sizeof(Dev), hipHostMallocDefault) == hipSuccess;
    for (auto &e : h->ev)
        if (ok) ok = hipEventCreate(&e) == hipSuccess;
    for (auto &s : h->wev)
        for (auto &e : s)
            if (ok) ok = hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        kw_sort_destroy(h);
        return KW_EHIP;
    }
    *out = h;
    return KW_OK;
}

extern "C" int kw_sort_destroy(kw_sort *h)
{
    if (!h) return KW_OK;
    (void)hipSetDevice(h->device);
    Buf *bufs[] = {&h->keys,  &h->btext, &h->bnonna, &h->order,   &h->doff,   &h->tsum,
                   &h->out,   &h->store, &h->srs,    &h->sre,     &h->slab[0], &h->slab[1]};
    for (Buf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (void *p : h->h_slab)
        if (p) (void)hipHostFree(p);
    if (h->D) (void)hipFree(h->D);
    if (h->H) (void)hipHostFree(h->H);
    if (h->h_keys) (void)hipHostFree(h->h_keys);
    if (h->h_out) (void)hipHostFree(h->h_out);
    for (void *p : h->h_stage)
        if (p) (void)hipHostFree(p);
    for (auto &e : h->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &s : h->wev)
        for (auto &e : s)
            if (e) (void)hipEventDestroy(e);
    delete h;
    return KW_OK;
}

extern "C" const char *kw_sort_last_error(kw_sort *h) { return h ? h->err.c_str() : "null handle"; }

// the device's state as a file starts: no offender, no bytes
static int reset_state(kw_sort *h, hipStream_t st)
{
    Dev init;
    memset(&init, 0, sizeof(init));
    init.first_key = init.first_form = init.first_dtype = init.first_len = init.first_term = NONE;
    *h->H = init;   // (pinned: the copy below reads it in stream order; the last call's copy back has finished)
    KWCHK(h, hipMemcpyAsync(h->D, h->H, sizeof(Dev), hipMemcpyHostToDevice, st));
    return KW_OK;
}

// after ev[1]: the n keys and the state to the host; the copies' time to ms_keys_copy
static int fetch_state(kw_sort *h, long long n, hipStream_t st)
{
    KWCHK(h, hipMemcpyAsync(h->h_keys, h->keys.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipMemcpyAsync(h->H, h->D, sizeof(Dev), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipEventRecord(h->ev[2], st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipEventElapsedTime(&h->ms_keys_copy, h->ev[1], h->ev[2]));
    return KW_OK;
}

// the verdict of the fetched state: the first of KEY, FORM, DTYPE with an offender; true: KW_SORT_OK
static bool report(kw_sort *h, int32_t time_col, int32_t ncols, int64_t block_rows, const int64_t **keys,
                   int64_t *body_bytes, int32_t *verdict, int64_t *bad_row, int32_t *bad_col, int32_t *ascending)
{
    const Dev &R = *h->H;
    if (R.first_key != NONE) {
        *verdict = KW_SORT_KEY;
        *bad_row = (int64_t)R.first_key;
        *bad_col = time_col;
    } else if (R.first_form != NONE) {
        *verdict = KW_SORT_FORM;
        *bad_row = (int64_t)(R.first_form >> COL_BITS);
        *bad_col = (int32_t)(R.first_form & ((1u << COL_BITS) - 1u));
    } else if (R.first_dtype != NONE) {
        *verdict = KW_SORT_DTYPE;
        *bad_row = (int64_t)(R.first_dtype / (u64)ncols) * block_rows;
        *bad_col = (int32_t)(R.first_dtype % (u64)ncols);
    } else {
        *keys = (const int64_t *)h->h_keys;
        *body_bytes = (int64_t)R.body_bytes;
        *ascending = R.not_asc ? 0 : 1;
        return true;
    }
    return false;
}

extern "C" int kw_sort_keys(kw_sort *h, kw_ingest *ig, int32_t time_col, int64_t block_rows, const int64_t **keys,
                            int64_t *n_rows, int64_t *body_bytes, int32_t *verdict, int64_t *bad_row, int32_t *bad_col,
                            int32_t *ascending, void *stream)
{
    if (!h) return KW_EINVAL;
    h->have = h->scanned = h->open = h->iopen = false;
    if (!ig || !keys || !n_rows || !body_bytes || !verdict || !bad_row || !bad_col || !ascending || block_rows < 1) {
        h->err = "kw_sort_keys: bad arguments";
        return KW_EINVAL;
    }
    *keys = nullptr;
    *n_rows = *body_bytes = *bad_row = 0;
    *verdict = KW_SORT_OK;
    *bad_col = *ascending = 0;
    hipStream_t st = (hipStream_t)stream;
    KWCHK(h, hipSetDevice(h->device));
    KWCHK(h, hipEventRecord(h->ev[0], st));
    const int64_t *rs, *re, *coff;
    const uint8_t *text, *cells, *cfl;
    int64_t n, n_bytes, cell_bytes;
    int32_t ncols;
    if (kw_ingest_spans(ig, &rs, &re, &n, &ncols, &text, &n_bytes) != KW_OK ||
        kw_ingest_cells(ig, &cells, &coff, &cfl, &cell_bytes) != KW_OK) {
        h->err = std::string("kw_sort_keys: ") + kw_ingest_last_error(ig);
        return KW_ESTATE;
    }
    if (n < 1 || time_col < 0 || time_col >= ncols) {
        h->err = "kw_sort_keys: no rows, or no such column";
        return KW_EINVAL;
    }
    const long long nblk = (n + block_rows - 1) / block_rows, nbc = nblk * ncols;
    int rc;
    if ((rc = fit(h, h->keys, (size_t)n * 8)) || (rc = fit(h, h->btext, (size_t)nbc)) ||
        (rc = fit(h, h->bnonna, (size_t)nbc)) || (rc = fit_pinned(h, &h->h_keys, &h->h_keys_cap, (size_t)n * 8)))
        return rc;
    uint8_t *btext = (uint8_t *)h->btext.p, *bnonna = (uint8_t *)h->bnonna.p;
    const int gcap = grid_cap();
    if ((rc = reset_state(h, st))) return rc;
    KWCHK(h, hipMemsetAsync(btext, 0, (size_t)nbc, st));
    KWCHK(h, hipMemsetAsync(bnonna, 0, (size_t)nbc, st));
    hipLaunchKernelGGL(ks_rows_kernel, grid_for(n, BLOCK, gcap), dim3(BLOCK), 0, st, cells, (const long long *)coff, cfl,
                       (const long long *)rs, (const long long *)re, (long long)n, (int)ncols, (int)time_col,
                       (long long)block_rows, (long long *)h->keys.p, btext, bnonna, h->D, 0ll, 0ll,
                       (long long *)nullptr, (long long *)nullptr);
    hipLaunchKernelGGL(ks_check_kernel, grid_for(n > nbc ? n : nbc, BLOCK, gcap), dim3(BLOCK), 0, st,
                       (const long long *)h->keys.p, 1ll, (long long)n, (const uint8_t *)btext, (const uint8_t *)bnonna,
                       nbc, (int)ncols, (int)time_col, h->D);
    KWCHK(h, hipEventRecord(h->ev[1], st));
    if ((rc = fetch_state(h, n, st))) return rc;
    KWCHK(h, hipEventElapsedTime(&h->ms[0], h->ev[0], h->ev[1]));
    h->ms[1] = h->ms[2] = 0;
    h->ms[3] = h->ms_keys_copy;
    *n_rows = n;
    if (report(h, time_col, ncols, block_rows, keys, body_bytes, verdict, bad_row, bad_col, ascending)) {
        h->have = true;
        h->text = text;
        h->rs = rs;
        h->re = re;
        h->n_rows = n;
        h->stream = st;
    }
    return KW_OK;
}

// ------------------------------------------------------------------ a file of several windows
// The store of a file's body: expect_bytes and a lane's read past a record's end.  A store the handle has is kept
// when it is large enough.  KW_EOVERFLOW, with nothing allocated: see kw_sort_begin (kwsort.h).
static int reserve_store(kw_sort *h, int64_t expect_bytes, const char *who)
{
    if (expect_bytes > store_cap()) {
        h->err = std::string(who) + ": a store of " + std::to_string(expect_bytes) + " bytes is over the cap";
        return KW_EOVERFLOW;
    }
    const size_t want = (size_t)expect_bytes + 64;   // (a lane's 16-byte load may read past a record's end)
    if (h->store.cap < want) {
        // the store itself, and a quarter of it again for what is kept per row -- the key, the span, the order entry
        // and its offset, 40 bytes, at the 160 bytes and more of a per-ticker file's record -- and a margin for
        // the slabs; a store that is replaced gives its own bytes back first
        size_t free_b = 0, total_b = 0;
        KWCHK(h, hipMemGetInfo(&free_b, &total_b));
        const size_t need = want + want / 4 + ((size_t)64 << 20);
        if (need > free_b + h->store.cap) {
            h->err = std::string(who) + ": a store of " + std::to_string(expect_bytes) + " bytes does not fit in the " +
                     std::to_string(free_b) + " free bytes of the device";
            return KW_EOVERFLOW;
        }
        if (h->store.p) (void)hipFree(h->store.p);
        h->store.p = nullptr;
        h->store.cap = 0;
        if (hipMalloc(&h->store.p, want) != hipSuccess) {
            (void)hipGetLastError();
            h->store.p = nullptr;
            h->err = std::string(who) + ": no device memory for a store of " + std::to_string(expect_bytes) + " bytes";
            return KW_EOVERFLOW;
        }
        h->store.cap = want;
    }
    return KW_OK;
}

extern "C" int kw_sort_begin(kw_sort *h, int32_t time_col, int64_t block_rows, int64_t expect_bytes)
{
    if (!h) return KW_EINVAL;
    h->have = h->scanned = h->open = h->iopen = false;
    if (time_col < 0 || block_rows < 1 || expect_bytes < 1) {
        h->err = "kw_sort_begin: bad arguments";
        return KW_EINVAL;
    }
    KWCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = reserve_store(h, expect_bytes, "kw_sort_begin"))) return rc;
    h->time_col = time_col;
    h->block_rows = block_rows;
    h->expect = expect_bytes;
    h->used = h->rows = 0;
    h->ncols = 0;
    h->ms[0] = h->ms[1] = h->ms[2] = h->ms[3] = h->ms_keys_copy = 0;
    if ((rc = reset_state(h, nullptr))) return rc;
    KWCHK(h, hipStreamSynchronize(nullptr));
    h->open = true;
    return KW_OK;
}

extern "C" int kw_sort_window(kw_sort *h, kw_ingest *ig, int64_t consumed, void *stream)
{
    if (!h) return KW_EINVAL;
    if (!h->open) {
        h->err = "kw_sort_window: no kw_sort_begin";
        return KW_ESTATE;
    }
    h->open = false;   // (an error below ends the file)
    hipStream_t st = (hipStream_t)stream;
    KWCHK(h, hipSetDevice(h->device));
    const int64_t *rs, *re, *coff;
    const uint8_t *text, *cells, *cfl;
    int64_t n, n_bytes, cell_bytes;
    int32_t ncols;
    if (!ig || kw_ingest_spans(ig, &rs, &re, &n, &ncols, &text, &n_bytes) != KW_OK ||
        kw_ingest_cells(ig, &cells, &coff, &cfl, &cell_bytes) != KW_OK) {
        h->err = std::string("kw_sort_window: ") + (ig ? kw_ingest_last_error(ig) : "no ingest handle");
        return KW_ESTATE;
    }
    if (n < 1 || consumed < 1 || consumed > n_bytes || h->time_col >= ncols || (h->ncols && h->ncols != ncols)) {
        h->err = "kw_sort_window: no rows, bytes outside the text, or another shape than the file's first window";
        return KW_EINVAL;
    }
    if (consumed > h->expect - h->used) {
        h->err = "kw_sort_window: the store holds " + std::to_string(h->used) + " of " + std::to_string(h->expect) +
                 " bytes, the window has " + std::to_string(consumed);
        return KW_EOVERFLOW;
    }
    h->ncols = ncols;
    const long long base = h->rows, rows = base + n;
    const long long nbc = ((rows + h->block_rows - 1) / h->block_rows) * ncols;
    const long long nbc0 = ((base + h->block_rows - 1) / h->block_rows) * ncols;
    int rc;
    if ((rc = fit_keep(h, h->keys, (size_t)rows * 8, (size_t)base * 8, st)) ||
        (rc = fit_keep(h, h->srs, (size_t)rows * 8, (size_t)base * 8, st)) ||
        (rc = fit_keep(h, h->sre, (size_t)rows * 8, (size_t)base * 8, st)) ||
        (rc = fit_keep(h, h->btext, (size_t)nbc, (size_t)nbc0, st)) ||
        (rc = fit_keep(h, h->bnonna, (size_t)nbc, (size_t)nbc0, st)))
        return rc;
    uint8_t *btext = (uint8_t *)h->btext.p, *bnonna = (uint8_t *)h->bnonna.p;
    const int gcap = grid_cap();
    KWCHK(h, hipEventRecord(h->ev[0], st));
    // (the witnesses of the blocks this window opens: a buffer that did not grow holds an earlier file's)
    if (nbc > nbc0) {
        KWCHK(h, hipMemsetAsync(btext + nbc0, 0, (size_t)(nbc - nbc0), st));
        KWCHK(h, hipMemsetAsync(bnonna + nbc0, 0, (size_t)(nbc - nbc0), st));
    }
    hipLaunchKernelGGL(ks_rows_kernel, grid_for(n, BLOCK, gcap), dim3(BLOCK), 0, st, cells, (const long long *)coff, cfl,
                       (const long long *)rs, (const long long *)re, (long long)n, (int)ncols, h->time_col, h->block_rows,
                       (long long *)h->keys.p, btext, bnonna, h->D, base, h->used, (long long *)h->srs.p,
                       (long long *)h->sre.p);
    // (the first row of a later window against the last row of the window before)
    hipLaunchKernelGGL(ks_check_kernel, grid_for(n, BLOCK, gcap), dim3(BLOCK), 0, st, (const long long *)h->keys.p,
                       base > 0 ? base : 1ll, rows, (const uint8_t *)btext, (const uint8_t *)bnonna, 0ll, (int)ncols,
                       h->time_col, h->D);
    KWCHK(h, hipEventRecord(h->ev[1], st));
    KWCHK(h, hipMemcpyAsync((uint8_t *)h->store.p + h->used, text, (size_t)consumed, hipMemcpyDeviceToDevice, st));
    KWCHK(h, hipEventRecord(h->ev[2], st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    float a = 0, b = 0;
    KWCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
    KWCHK(h, hipEventElapsedTime(&b, h->ev[1], h->ev[2]));
    h->ms[0] += a;
    h->ms[3] += b;
    h->ms_keys_copy = h->ms[3];
    h->used += consumed;
    h->rows = rows;
    h->stream = st;
    h->open = true;
    return KW_OK;
}

extern "C" int kw_sort_finish(kw_sort *h, const int64_t **keys, int64_t *n_rows, int64_t *body_bytes, int32_t *verdict,
                              int64_t *bad_row, int32_t *bad_col, int32_t *ascending)
{
    if (!h) return KW_EINVAL;
    if (!h->open || h->rows < 1) {
        h->err = "kw_sort_finish: no kw_sort_begin, or no window since";
        h->open = false;
        return KW_ESTATE;
    }
    h->open = false;
    if (!keys || !n_rows || !body_bytes || !verdict || !bad_row || !bad_col || !ascending) {
        h->err = "kw_sort_finish: bad arguments";
        return KW_EINVAL;
    }
    *keys = nullptr;
    *n_rows = *body_bytes = *bad_row = 0;
    *verdict = KW_SORT_OK;
    *bad_col = *ascending = 0;
    hipStream_t st = h->stream;
    KWCHK(h, hipSetDevice(h->device));
    const long long n = h->rows, nbc = ((n + h->block_rows - 1) / h->block_rows) * h->ncols;
    int rc;
    if ((rc = fit_pinned(h, &h->h_keys, &h->h_keys_cap, (size_t)n * 8))) return rc;
    KWCHK(h, hipEventRecord(h->ev[0], st));
    hipLaunchKernelGGL(ks_check_kernel, grid_for(nbc, BLOCK, grid_cap()), dim3(BLOCK), 0, st, (const long long *)h->keys.p, 1ll,
                       0ll, (const uint8_t *)h->btext.p, (const uint8_t *)h->bnonna.p, nbc, h->ncols, h->time_col, h->D);
    KWCHK(h, hipEventRecord(h->ev[1], st));
    const float copies = h->ms[3];
    if ((rc = fetch_state(h, n, st))) return rc;
    float a = 0;
    KWCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
    h->ms[0] += a;
    h->ms[3] = h->ms_keys_copy = copies + h->ms_keys_copy;
    *n_rows = n;
    if (report(h, h->time_col, h->ncols, h->block_rows, keys, body_bytes, verdict, bad_row, bad_col, ascending)) {
        h->have = true;
        h->text = (const uint8_t *)h->store.p;
        h->rs = (const int64_t *)h->srs.p;
        h->re = (const int64_t *)h->sre.p;
        h->n_rows = n;
    }
    return KW_OK;
}

// ------------------------------------------------------------------ a file described by its write index
// the slot's copy to the store has finished: its time onto ms[3] (copies)
static int settle_slot(kw_sort *h, int slot)
{
    if (!h->busy[slot]) return KW_OK;
    h->busy[slot] = false;
    KWCHK(h, hipEventSynchronize(h->wev[slot][1]));
    float a = 0;
    KWCHK(h, hipEventElapsedTime(&a, h->wev[slot][0], h->wev[slot][1]));
    h->ms[3] += a;
    return KW_OK;
}

extern "C" int kw_sort_index_begin(kw_sort *h, const int64_t *lens, int64_t n_rows, int64_t body_bytes, int64_t *bad_row)
{
    if (!h) return KW_EINVAL;
    h->have = h->scanned = h->open = h->iopen = false;
    if (!lens || !bad_row || n_rows < 1 || body_bytes < 1) {
        h->err = "kw_sort_index_begin: bad arguments";
        return KW_EINVAL;
    }
    *bad_row = -1;
    KWCHK(h, hipSetDevice(h->device));
    int rc;
    // (a slot whose copy into the last file's store is still under way: the store may be replaced below)
    if ((rc = settle_slot(h, 0)) || (rc = settle_slot(h, 1))) return rc;
    if ((rc = reserve_store(h, body_bytes, "kw_sort_index_begin"))) return rc;
    const long long ntiles = (n_rows + BLOCK - 1) / BLOCK;
    if ((rc = fit(h, h->keys, (size_t)n_rows * 8)) || (rc = fit(h, h->srs, (size_t)n_rows * 8)) ||
        (rc = fit(h, h->sre, (size_t)n_rows * 8)) || (rc = fit(h, h->tsum, (size_t)ntiles * 8)))
        return rc;
    h->ms[0] = h->ms[1] = h->ms[2] = h->ms[3] = h->ms_keys_copy = 0;
    hipStream_t st = nullptr;
    const int gcap = grid_cap();
    const long long *d_lens = (const long long *)h->keys.p;
    KWCHK(h, hipEventRecord(h->ev[0], st));
    if ((rc = reset_state(h, st))) return rc;
    KWCHK(h, hipMemcpyAsync(h->keys.p, lens, (size_t)n_rows * 8, hipMemcpyHostToDevice, st));
    KWCHK(h, hipEventRecord(h->ev[1], st));
    hipLaunchKernelGGL(ks_span_kernel, grid_for(n_rows, BLOCK, gcap), dim3(BLOCK), 0, st, d_lens, (long long)n_rows,
                       (long long)body_bytes, (long long *)h->srs.p, (u64 *)h->tsum.p, h->D);
    hipLaunchKernelGGL(ks_scan_kernel, dim3(1), dim3(BLOCK), 0, st, (u64 *)h->tsum.p, ntiles, &h->D->total);
    hipLaunchKernelGGL(ks_span_add_kernel, grid_for(n_rows, BLOCK, gcap), dim3(BLOCK), 0, st, d_lens, (long long)n_rows,
                       (long long)body_bytes, (long long *)h->srs.p, (long long *)h->sre.p, (const u64 *)h->tsum.p,
                       h->D);
    KWCHK(h, hipEventRecord(h->ev[2], st));
    KWCHK(h, hipMemcpyAsync(h->H, h->D, sizeof(Dev), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipEventElapsedTime(&h->ms[3], h->ev[0], h->ev[1]));
    KWCHK(h, hipEventElapsedTime(&h->ms[0], h->ev[1], h->ev[2]));
    const Dev &R = *h->H;
    if (R.first_len != NONE || R.total != (u64)body_bytes) {
        // (with no offender every length was counted and every record ends inside the body: the sum is short)
        *bad_row = R.first_len != NONE ? (int64_t)R.first_len : n_rows;
        h->err = "kw_sort_index_begin: row " + std::to_string(*bad_row) +
                 (R.first_len == NONE       ? ": the lengths end before the body's " + std::to_string(body_bytes) + " bytes"
                  : lens[*bad_row] < 1      ? ": a length below 1"
                                            : ": the record ends beyond the body's " + std::to_string(body_bytes) + " bytes");
        return KW_EINVAL;
    }
    h->expect = body_bytes;
    h->used = 0;
    h->rows = n_rows;
    h->stream = st;
    h->iopen = true;
    return KW_OK;
}

extern "C" int kw_sort_index_stage(kw_sort *h, int32_t slot, int64_t n_bytes, uint8_t **host)
{
    if (!h) return KW_EINVAL;
    if (!host || slot < 0 || slot > 1 || n_bytes < 1) {
        h->err = "kw_sort_index_stage: bad arguments";
        return KW_EINVAL;
    }
    *host = nullptr;
    KWCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = settle_slot(h, slot)) || (rc = fit_pinned(h, &h->h_stage[slot], &h->h_stage_cap[slot], (size_t)n_bytes)))
        return rc;
    *host = (uint8_t *)h->h_stage[slot];
    return KW_OK;
}

extern "C" int kw_sort_index_window(kw_sort *h, int32_t slot, int64_t n_bytes, void *stream)
{
    if (!h) return KW_EINVAL;
    if (!h->iopen) {
        h->err = "kw_sort_index_window: no kw_sort_index_begin";
        return KW_ESTATE;
    }
    h->iopen = false;   // (an error below ends the file)
    if (slot < 0 || slot > 1 || n_bytes < 1 || (size_t)n_bytes > h->h_stage_cap[slot] || !h->h_stage[slot]) {
        h->err = "kw_sort_index_window: no such slot, or more bytes than it was staged for";
        return KW_EINVAL;
    }
    if (n_bytes > h->expect - h->used) {
        h->err = "kw_sort_index_window: the store holds " + std::to_string(h->used) + " of " +
                 std::to_string(h->expect) + " bytes, the window has " + std::to_string(n_bytes);
        return KW_EOVERFLOW;
    }
    hipStream_t st = (hipStream_t)stream;
    KWCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = settle_slot(h, slot))) return rc;
    KWCHK(h, hipEventRecord(h->wev[slot][0], st));
    KWCHK(h, hipMemcpyAsync((uint8_t *)h->store.p + h->used, h->h_stage[slot], (size_t)n_bytes, hipMemcpyHostToDevice, st));
    KWCHK(h, hipEventRecord(h->wev[slot][1], st));
    h->busy[slot] = true;
    h->used += n_bytes;
    h->stream = st;
    h->iopen = true;
    return KW_OK;
}

extern "C" int kw_sort_index_finish(kw_sort *h, int32_t *verdict, int64_t *bad_row)
{
    if (!h) return KW_EINVAL;
    if (!h->iopen || h->used != h->expect) {
        h->err = !h->iopen ? std::string("kw_sort_index_finish: no kw_sort_index_begin")
                           : "kw_sort_index_finish: the windows gave " + std::to_string(h->used) + " of the body's " +
                                 std::to_string(h->expect) + " bytes";
        h->iopen = false;
        return KW_ESTATE;
    }
    h->iopen = false;
    if (!verdict || !bad_row) {
        h->err = "kw_sort_index_finish: bad arguments";
        return KW_EINVAL;
    }
    *verdict = KW_INDEX_OK;
    *bad_row = -1;
    hipStream_t st = h->stream;
    KWCHK(h, hipSetDevice(h->device));
    KWCHK(h, hipEventRecord(h->ev[0], st));
    hipLaunchKernelGGL(ks_term_kernel, grid_for(h->rows, BLOCK, grid_cap()), dim3(BLOCK), 0, st, (const uint8_t *)h->store.p,
                       (const long long *)h->sre.p, h->rows, h->D);
    KWCHK(h, hipEventRecord(h->ev[1], st));
    KWCHK(h, hipMemcpyAsync(h->H, h->D, sizeof(Dev), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    int rc;
    if ((rc = settle_slot(h, 0)) || (rc = settle_slot(h, 1))) return rc;
    float a = 0;
    KWCHK(h, hipEventElapsedTime(&a, h->ev[0], h->ev[1]));
    h->ms[0] += a;
    h->ms_keys_copy = h->ms[3];
    if (h->H->first_term != NONE) {
        *verdict = KW_INDEX_TERM;
        *bad_row = (int64_t)h->H->first_term;
        return KW_OK;
    }
    h->have = true;
    h->text = (const uint8_t *)h->store.p;
    h->rs = (const int64_t *)h->srs.p;
    h->re = (const int64_t *)h->sre.p;
    h->n_rows = h->rows;
    return KW_OK;
}

// The order's range check, the records' lengths and their scan (ev[3] .. ev[5]); synchronises.  *total: the
// body's bytes; KW_EINVAL for an entry outside [0, n_rows).
static int gather_scan(kw_sort *h, const int64_t *order, int64_t n, u64 *total)
{
    hipStream_t st = h->stream;
    h->scanned = false;
    int rc;
    const long long ntiles = (n + BLOCK - 1) / BLOCK;
    if ((rc = fit(h, h->order, (size_t)n * 8)) || (rc = fit(h, h->doff, (size_t)(n + 1) * 8)) ||
        (rc = fit(h, h->tsum, (size_t)ntiles * 8)))
        return rc;
    const int gcap = grid_cap();
    h->H->total = 0;
    h->H->bad_order = 0;
    KWCHK(h, hipEventRecord(h->ev[3], st));
    KWCHK(h, hipMemcpyAsync(h->D, h->H, sizeof(Dev), hipMemcpyHostToDevice, st));
    KWCHK(h, hipMemcpyAsync(h->order.p, order, (size_t)n * 8, hipMemcpyHostToDevice, st));
    KWCHK(h, hipEventRecord(h->ev[4], st));
    hipLaunchKernelGGL(ks_len_kernel, grid_for(n, BLOCK, gcap), dim3(BLOCK), 0, st, (const long long *)h->order.p, (long long)n,
                       h->n_rows, (const long long *)h->rs, (const long long *)h->re, (u64 *)h->doff.p, (u64 *)h->tsum.p,
                       h->D);
    hipLaunchKernelGGL(ks_scan_kernel, dim3(1), dim3(BLOCK), 0, st, (u64 *)h->tsum.p, ntiles, &h->D->total);
    hipLaunchKernelGGL(ks_add_kernel, grid_for(n, BLOCK, gcap), dim3(BLOCK), 0, st, (u64 *)h->doff.p, (long long)n,
                       (const u64 *)h->tsum.p, (const u64 *)&h->D->total);
    KWCHK(h, hipEventRecord(h->ev[5], st));
    KWCHK(h, hipMemcpyAsync(h->H, h->D, sizeof(Dev), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    if (h->H->bad_order) {
        h->err = "kw_sort_gather: an order entry outside [0, n_rows)";
        return KW_EINVAL;
    }
    *total = h->H->total;
    float a = 0;
    KWCHK(h, hipEventElapsedTime(&a, h->ev[3], h->ev[4]));
    KWCHK(h, hipEventElapsedTime(&h->ms[1], h->ev[4], h->ev[5]));
    h->ms[2] = 0;
    h->ms[3] = h->ms_keys_copy + a;
    return KW_OK;
}

// The body's bytes [x_lo, x_hi) (x_lo a multiple of 1024, x_hi one or the body's size) to d_out, then to h_out, on
// the stream: ev[6] .. ev[8].  No synchronisation.
static int gather_range(kw_sort *h, long long n, u64 x_lo, u64 x_hi, void *d_out, void *h_out)
{
    hipStream_t st = h->stream;
    const int gcap = grid_cap();
    KWCHK(h, hipEventRecord(h->ev[6], st));
    // the KiB a wave lays out: one while the range gives every wave of a full grid something to do, up to 16 beyond
    const long long kib = (long long)((x_hi - x_lo + 1023) >> 10), waves = (long long)gcap * (BLOCK / 64);
    long long iters = (kib + waves - 1) / waves;
    iters = iters < 1 ? 1 : (iters > 16 ? 16 : iters);
    const long long spans = (kib + iters - 1) / iters;
    hipLaunchKernelGGL(ks_copy_kernel, grid_for(spans * 64, BLOCK, gcap), dim3(BLOCK), 0, st, h->text,
                       (const long long *)h->rs, (const long long *)h->order.p, (const u64 *)h->doff.p, n,
                       (uint8_t *)d_out, (int)iters, x_lo, x_hi);
    KWCHK(h, hipEventRecord(h->ev[7], st));
    KWCHK(h, hipMemcpyAsync(h_out, d_out, (size_t)(x_hi - x_lo), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipEventRecord(h->ev[8], st));
    return KW_OK;
}

// after the stream that ran gather_range was synchronised: its times onto ms[2] (gather) and ms[3] (copies)
static int gather_times(kw_sort *h)
{
    float a = 0, b = 0;
    KWCHK(h, hipEventElapsedTime(&a, h->ev[6], h->ev[7]));
    KWCHK(h, hipEventElapsedTime(&b, h->ev[7], h->ev[8]));
    h->ms[2] += a;
    h->ms[3] += b;
    return KW_OK;
}

extern "C" int kw_sort_gather(kw_sort *h, const int64_t *order, int64_t n, const uint8_t **out, int64_t *out_bytes)
{
    if (!h) return KW_EINVAL;
    if (!h->have) {
        h->err = "kw_sort_gather: no kw_sort_keys or kw_sort_finish that was taken";
        return KW_ESTATE;
    }
    if (!order || !out || !out_bytes || n < 1 || n > h->n_rows) {
        h->err = "kw_sort_gather: bad arguments";
        return KW_EINVAL;
    }
    *out = nullptr;
    *out_bytes = 0;
    KWCHK(h, hipSetDevice(h->device));
    u64 total = 0;
    int rc;
    if ((rc = gather_scan(h, order, n, &total))) return rc;
    if (total >= 1ull << 31) {
        h->err = "kw_sort_gather: the body holds " + std::to_string(total) + " bytes";
        return KW_EOVERFLOW;
    }
    if ((rc = fit(h, h->out, (size_t)total + 32)) ||
        (rc = fit_pinned(h, &h->h_out, &h->h_out_cap, (size_t)total + 16)) ||
        (rc = gather_range(h, n, 0, total, h->out.p, h->h_out)))
        return rc;
    KWCHK(h, hipStreamSynchronize(h->stream));
    KWCHK(h, hipGetLastError());
    if ((rc = gather_times(h))) return rc;
    *out = (const uint8_t *)h->h_out;
    *out_bytes = (int64_t)total;
    return KW_OK;
}

extern "C" int kw_sort_gather_begin(kw_sort *h, const int64_t *order, int64_t n, int64_t slab_bytes,
                                    int64_t *total_bytes, int64_t *n_slabs)
{
    if (!h) return KW_EINVAL;
    if (!h->have) {
        h->err = "kw_sort_gather_begin: no kw_sort_keys or kw_sort_finish that was taken";
        return KW_ESTATE;
    }
    h->scanned = false;
    if (!order || !total_bytes || !n_slabs || n < 1 || n > h->n_rows || slab_bytes < 1024 || slab_bytes % 1024 ||
        slab_bytes >= 1ll << 31) {
        h->err = "kw_sort_gather_begin: bad arguments";
        return KW_EINVAL;
    }
    *total_bytes = *n_slabs = 0;
    KWCHK(h, hipSetDevice(h->device));
    u64 total = 0;
    int rc;
    if ((rc = gather_scan(h, order, n, &total))) return rc;
    for (int s = 0; s < 2; ++s)
        if ((rc = fit(h, h->slab[s], (size_t)slab_bytes + 32)) ||
            (rc = fit_pinned(h, &h->h_slab[s], &h->h_slab_cap[s], (size_t)slab_bytes)))
            return rc;
    h->g_n = n;
    h->g_total = total;
    h->slab_bytes = slab_bytes;
    h->n_slabs = (long long)((total + (u64)slab_bytes - 1) / (u64)slab_bytes);
    h->pre_k = -1;
    h->last_slot = 1;
    h->scanned = true;
    *total_bytes = (int64_t)total;
    *n_slabs = h->n_slabs;
    return KW_OK;
}

extern "C" int kw_sort_gather_slab(kw_sort *h, int64_t k, const uint8_t **out, int64_t *out_bytes)
{
    if (!h) return KW_EINVAL;
    if (!h->have || !h->scanned) {
        h->err = "kw_sort_gather_slab: no kw_sort_gather_begin that succeeded";
        return KW_ESTATE;
    }
    if (!out || !out_bytes || k < 0 || k >= h->n_slabs) {
        h->err = "kw_sort_gather_slab: bad arguments";
        return KW_EINVAL;
    }
    *out = nullptr;
    *out_bytes = 0;
    KWCHK(h, hipSetDevice(h->device));
    const u64 sb = (u64)h->slab_bytes;
    auto hi_of = [&](long long j) { return (u64)(j + 1) * sb < h->g_total ? (u64)(j + 1) * sb : h->g_total; };
    int rc;
    // the slab this call asks for: laid out ahead by the call before, or now, into the slab the caller gave up
    const int slot = 1 - h->last_slot;
    if (h->pre_k != k) {
        if (h->pre_k >= 0) {   // (another one is under way into this slab)
            KWCHK(h, hipStreamSynchronize(h->stream));
            if ((rc = gather_times(h))) return rc;
        }
        if ((rc = gather_range(h, h->g_n, (u64)k * sb, hi_of(k), h->slab[slot].p, h->h_slab[slot]))) return rc;
    }
    h->pre_k = -1;
    KWCHK(h, hipStreamSynchronize(h->stream));
    KWCHK(h, hipGetLastError());
    if ((rc = gather_times(h))) return rc;
    *out = (const uint8_t *)h->h_slab[slot];
    *out_bytes = (int64_t)(hi_of(k) - (u64)k * sb);
    h->last_slot = slot;
    // the next slab, into the other one, while the caller writes this one out
    if (k + 1 < h->n_slabs) {
        if ((rc = gather_range(h, h->g_n, (u64)(k + 1) * sb, hi_of(k + 1), h->slab[1 - slot].p, h->h_slab[1 - slot])))
            return rc;
        h->pre_k = k + 1;
    }
    return KW_OK;
}

extern "C" int kw_sort_last_ms(kw_sort *h, float *ms, int32_t n)
{
    if (!h || !ms || n < 0) return KW_EINVAL;
    for (int k = 0; k < n && k < 4; ++k) ms[k] = h->ms[k];
    return KW_OK;
}
