// libkwmatch: CDX listings and quoted CSV files parsed into the dedup's row store and the kept rows rendered as CSV,
// on the device (include/kwdedup.h, kw_cdx_*, kw_csv_append and its windowed form kw_csv_stream_*).
//
// Reference: yahoo_links_selenium.py:59 (read_csv of a listing), :82 / :176 (to_csv), :164-167 (read_csv of the
// part CSVs); the rule under which a text is taken at all is restated in tests/cdx_rule.py.
//
//   cx_lines_kernel<false>  one block a tile of TILE bytes, 16 bytes a lane in one coalesced load: '\n', '"',
//                           '\r' and NUL bytes as 16-bit masks; a byte starts a row when it is not '\n' and the
//                           byte before it is (or it is the text's first), so blank-line runs and lines longer
//                           than a tile need nothing special.  Rows per tile; the first '"' / '\r' / NUL position.
//   scan_launch             the device scan of kwhandle.hpp (kwscan.hip), used for the rows per tile, the URL
//                           lengths and the CSV line lengths.
//   cx_lines_kernel<true>   the same masks again: every row's start position, at its rank.
//   cx_parse_kernel         lane = row, 8 bytes a step with per-byte masks: fields counted, the timestamp and URL
//                           cells located, UTF-8 validated (bytewise only in words with a byte >= 0x80), ':'
//                           looked for in the URL cell, the digits parsed.  The first offending line by atomicMin
//                           of (line start, condition).
//   cx_off_kernel           the rows' arena offsets from the scanned URL lengths.
//   cx_fill_kernel          destination-major copy: a lane owns one aligned 16-byte chunk of the output, finds
//                           the segment (row / CSV line) under it by binary search in the offsets (narrowed per
//                           block), gathers its bytes and stores them at once.  With ArenaGen it compacts the
//                           URL cells into the arena, with CsvGen it writes the CSV.
//   cx_linelen_kernel       lane = kept row: decimal digits of the timestamp, the URL's length, whether it holds
//                           a ',' (then it is quoted).
//
//   cx_sel_*                the surviving rows rendered in a given order into several files (kw_cdx_csv_select_*; the
//                           link list's refresh and split, experiental/drop.py and split.py): the order's indices and
//                           the files' bounds checked, the lines' lengths gathered through the order, scan_launch, then
//                           cx_fill_kernel with SelGen; described above the kernels.
//
//   cv_*                    quoted CSV, one column out (kw_csv_append, the scraper's resume filter:
//                           constant_rate_scrapper.py:312-360; the rule is restated in tests/resume_rule.py): the
//                           same tiles and masks with quote state carried across them; described above the kernels.
//
// Kernels hand data to each other only across launches.  All byte work: the roofline is HBM bandwidth.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "kwdedup_handle.hpp"
#include "kwdev.hpp"

namespace cx {

using namespace kwd;   // BLOCK, TILE, NONE and the primitives
using namespace kwh;
constexpr int HEADER_LEN = 14;       // "date_time,url\n"
__constant__ const char HEADER[HEADER_LEN + 2] = "date_time,url\n";
static const char HEADER_HOST[HEADER_LEN + 2] = "date_time,url\n";

// priorities of the line conditions inside one line (the low 3 bits of Errs::line)
enum { P_HEADER = 0, P_UTF8 = 1, P_FIELDS = 2, P_TS = 3, P_URL = 4 };

struct Errs {
    unsigned long long quote, cr, nul;   // position of the first such byte (NONE)
    unsigned long long line;             // min over offending lines of (line start << 3 | condition) (NONE)
};

struct Dialect {
    uint32_t delim;
    int ts_col, url_col, skip, exact;
};

__device__ __forceinline__ uint64_t eq8(uint64_t v, uint64_t pat)
{
    const uint64_t d = v ^ pat;
    return ~(((d & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | d) & 0x8080808080808080ull;
}
// The text's rows: a row starts at a byte that is not '\n' and follows a '\n' (or starts the text).
// WRITE = false: rows per tile into tile_cnt, the first '"', '\r', NUL into errs.
// WRITE = true:  tile_cnt holds the tiles' exclusive prefix; every row's start goes to row_start at its rank.
template <bool WRITE>
__global__ __launch_bounds__(BLOCK) void cx_lines_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t ntiles,
                                                         unsigned long long *__restrict__ tile_cnt,
                                                         Errs *__restrict__ errs, int64_t *__restrict__ row_start)
{
    __shared__ unsigned long long ws[BLOCK / 64];
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t p = tile * TILE + (int64_t)threadIdx.x * 16;
        uint32_t starts = 0;
        unsigned long long eq = NONE, ec = NONE, ez = NONE;
        if (p < n) {
            // (the text is readable up to the next multiple of 16 past n: kw_cdx_append's contract)
            const uint4 v = *(const uint4 *)(text + p);
            const uint32_t valid = n - p >= 16 ? 0xFFFFu : (1u << (int)(n - p)) - 1u;
            const uint32_t nl = mask16(v, 0x0Au) & valid;
            const uint32_t prev_nl = (p == 0 || text[p - 1] == 0x0A) ? 1u : 0u;
            starts = ~nl & ((nl << 1) | prev_nl) & valid;
            if (!WRITE) {
                const uint32_t q = mask16(v, 0x22u) & valid, c = mask16(v, 0x0Du) & valid, z = mask16(v, 0u) & valid;
                if (q) eq = (unsigned long long)p + __builtin_ctz(q);
                if (c) ec = (unsigned long long)p + __builtin_ctz(c);
                if (z) ez = (unsigned long long)p + __builtin_ctz(z);
            }
        }
        if (!WRITE) {
            if (__any((eq & ec & ez) != NONE)) {   // (rare: one atomic a wave and condition)
                eq = wave_min(eq);
                ec = wave_min(ec);
                ez = wave_min(ez);
                if ((threadIdx.x & 63) == 0) {
                    if (eq != NONE) atomicMin(&errs->quote, eq);
                    if (ec != NONE) atomicMin(&errs->cr, ec);
                    if (ez != NONE) atomicMin(&errs->nul, ez);
                }
            }
        }
        unsigned long long total;
        const unsigned long long before = block_scan((unsigned long long)__popc(starts), ws, &total);
        if (!WRITE) {
            if (threadIdx.x == 0) tile_cnt[tile] = total;
        } else {
            unsigned long long r = tile_cnt[tile] + before;
            while (starts) {
                row_start[r++] = p + __builtin_ctz(starts);
                starts &= starts - 1u;
            }
        }
    }
}

// One row: fields, cells, UTF-8, digits.  Row r of the text starts at row_start[r] and ends before the next
// '\n' (or at n).  With D.skip row 0 is the header line; rows are written at r - D.skip.
__global__ __launch_bounds__(BLOCK) void cx_parse_kernel(const uint8_t *__restrict__ text, int64_t n,
                                                         const int64_t *__restrict__ row_start, int64_t n_lines,
                                                         Dialect D, int64_t *__restrict__ ts_out,
                                                         int64_t *__restrict__ url_pos,
                                                         unsigned long long *__restrict__ url_len,
                                                         Errs *__restrict__ errs)
{
    constexpr uint64_t ONES = 0x0101010101010101ull, HI = 0x8080808080808080ull;
    for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < n_lines; r += (int64_t)gridDim.x * BLOCK) {
        const int64_t s = row_start[r];
        if (D.skip && r == 0) {
            // the header: the text's first HEADER_LEN - 1 bytes, then '\n' or the end
            bool ok = s == 0 && n >= HEADER_LEN - 1 && (n == HEADER_LEN - 1 || text[HEADER_LEN - 1] == 0x0A);
            for (int k = 0; ok && k < HEADER_LEN - 1; ++k) ok = text[k] == (uint8_t)HEADER[k];
            if (!ok) atomicMin(&errs->line, (unsigned long long)P_HEADER);
            continue;
        }
        int f = 0, need = 0;
        uint32_t lo = 0x80u, hi = 0xBFu;
        bool bad8 = false, colon = false;
        int64_t ts_s = D.ts_col == 0 ? s : -1, ts_e = -1, u_s = D.url_col == 0 ? s : -1, u_e = -1, end = -1;
        for (int64_t w = s & ~(int64_t)7; end < 0; w += 8) {
            if (w >= n) { end = n; break; }
            // (aligned 8 bytes at w < n: inside the text's readable 16-byte granule)
            const uint64_t v = *(const uint64_t *)(text + w);
            const int b0 = w < s ? (int)(s - w) : 0;
            const int b1 = n - w >= 8 ? 8 : (int)(n - w);
            const uint64_t from = ~((1ull << (8 * b0)) - 1ull);
            const uint64_t nlm = eq8(v, 0x0Aull * ONES) & from & (b1 == 8 ? ~0ull : (1ull << (8 * b1)) - 1ull);
            const int e = nlm ? (__builtin_ctzll(nlm) >> 3) : b1;   // the row's bytes of this word: [b0, e)
            const uint64_t in = HI & from & (e == 8 ? ~0ull : (1ull << (8 * e)) - 1ull);
            if (need || (v & in)) {
                for (int k = b0; k < e; ++k) {
                    const uint32_t c = (uint32_t)(v >> (8 * k)) & 0xFFu;
                    if (need) {
                        if (c < lo || c > hi) bad8 = true;
                        --need;
                        lo = 0x80u; hi = 0xBFu;
                    } else if (c >= 0x80u) {
                        if (c >= 0xC2u && c <= 0xDFu) need = 1;
                        else if (c == 0xE0u) { need = 2; lo = 0xA0u; }
                        else if (c == 0xEDu) { need = 2; hi = 0x9Fu; }
                        else if (c >= 0xE1u && c <= 0xEFu) need = 2;
                        else if (c == 0xF0u) { need = 3; lo = 0x90u; }
                        else if (c >= 0xF1u && c <= 0xF3u) need = 3;
                        else if (c == 0xF4u) { need = 3; hi = 0x8Fu; }
                        else bad8 = true;
                    }
                }
            }
            uint64_t ev = (eq8(v, (uint64_t)D.delim * ONES) | eq8(v, 0x3Aull * ONES)) & in;
            while (ev) {
                const int k = __builtin_ctzll(ev) >> 3;
                ev &= ev - 1ull;
                const int64_t pos = w + k;
                if (((uint32_t)(v >> (8 * k)) & 0xFFu) == D.delim) {
                    if (f == D.ts_col) ts_e = pos;
                    if (f == D.url_col) u_e = pos;
                    ++f;
                    if (f == D.ts_col) ts_s = pos + 1;
                    if (f == D.url_col) u_s = pos + 1;
                } else {
                    colon |= f == D.url_col;
                }
            }
            if (nlm) end = w + e;
        }
        if (need) bad8 = true;
        if (f == D.ts_col) ts_e = end;
        if (f == D.url_col) u_e = end;
        const int fields = f + 1;
        const int least = (D.ts_col > D.url_col ? D.ts_col : D.url_col) + 1;
        int cond = -1;
        int64_t ts = 0;
        if (bad8) cond = P_UTF8;
        else if (D.exact ? fields != D.exact : fields < least) cond = P_FIELDS;
        else {
            const int64_t tl = ts_e - ts_s;
            bool ok = tl >= 1 && tl <= 18;
            for (int64_t k = ts_s; ok && k < ts_e; ++k) {
                const uint32_t c = text[k];
                ok = c >= 0x30u && c <= 0x39u;
                ts = ts * 10 + (int64_t)(c - 0x30u);
            }
            if (!ok) cond = P_TS;
            else if (!colon) cond = P_URL;
        }
        if (cond >= 0) {
            atomicMin(&errs->line, ((unsigned long long)s << 3) | (unsigned long long)cond);
            continue;
        }
        const int64_t o = r - D.skip;
        ts_out[o] = ts;
        url_pos[o] = u_s;
        url_len[o] = (unsigned long long)(u_e - u_s);
    }
}

// off[r] = base + the scanned URL lengths (r < m), off[m] = base + their total
__global__ __launch_bounds__(BLOCK) void cx_off_kernel(int64_t *__restrict__ off, const unsigned long long *__restrict__ excl,
                                                       const unsigned long long *__restrict__ grand, int64_t m, int64_t base)
{
    for (int64_t r = (int64_t)blockIdx.x * BLOCK + threadIdx.x; r <= m; r += (int64_t)gridDim.x * BLOCK)
        off[r] = base + (int64_t)(r < m ? excl[r] : *grand);
}

// '\n' bytes in text[0, end): the line number of a position
__global__ __launch_bounds__(BLOCK) void cx_count_nl_kernel(const uint8_t *__restrict__ text, int64_t end,
                                                            unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long ws[BLOCK / 64];
    unsigned long long c = 0;
    for (int64_t p = ((int64_t)blockIdx.x * BLOCK + threadIdx.x) * 16; p < end; p += (int64_t)gridDim.x * BLOCK * 16) {
        const uint4 v = *(const uint4 *)(text + p);
        const uint32_t valid = end - p >= 16 ? 0xFFFFu : (1u << (int)(end - p)) - 1u;
        c += (unsigned long long)__popc(mask16(v, 0x0Au) & valid);
    }
    unsigned long long total;
    (void)block_scan(c, ws, &total);
    if (threadIdx.x == 0 && total) atomicAdd(out, total);
}

// largest s in [a, b) with off[s] <= p (off[a] <= p)
__device__ __forceinline__ int64_t seg_find(const int64_t *__restrict__ off, int64_t a, int64_t b, int64_t p)
{
    while (b - a > 1) {
        const int64_t mid = a + ((b - a) >> 1);
        if (off[mid] <= p) a = mid; else b = mid;
    }
    return a;
}

// Destination-major write of m segments: segment s is out[off[s], off[s + 1]) and its byte j is
// g.byte(g.open(s), j).  out is 16-byte aligned; a lane owns the aligned 16-byte chunk c (bytes outside
// [off[0], off[m]) are left alone: the first and the last chunk are written bytewise when partial).
template <class Gen>
__global__ __launch_bounds__(BLOCK) void cx_fill_kernel(uint8_t *__restrict__ out, const int64_t *__restrict__ off,
                                                        int64_t m, Gen g)
{
    __shared__ int64_t rng[2];
    const int64_t lo = off[0], hi = off[m];
    const int64_t c0 = lo >> 4, c1 = (hi + 15) >> 4;
    for (int64_t cb = c0 + (int64_t)blockIdx.x * BLOCK; cb < c1; cb += (int64_t)gridDim.x * BLOCK) {
        __syncthreads();   // rng free again
        if (threadIdx.x == 0) {   // the block's chunks lie under segments [rng[0], rng[1]]
            const int64_t pf = cb * 16 > lo ? cb * 16 : lo;
            const int64_t pe = (cb + BLOCK) * 16 < hi ? (cb + BLOCK) * 16 : hi;
            rng[0] = seg_find(off, 0, m, pf);
            rng[1] = seg_find(off, rng[0], m, pe - 1);
        }
        __syncthreads();
        const int64_t c = cb + threadIdx.x;
        int64_t p = c * 16 > lo ? c * 16 : lo;
        const int64_t e = c * 16 + 16 < hi ? c * 16 + 16 : hi;
        if (p >= e) continue;   // (every thread still reaches both barriers of the next round: none inside)
        const int64_t p0 = p;
        int64_t s = seg_find(off, rng[0], rng[1] + 1, p);
        uint64_t a = 0, b = 0;
        while (p < e) {
            const int64_t so = off[s], se = off[s + 1];
            if (se <= p) { ++s; continue; }   // (an empty segment)
            const auto ctx = g.open(s);
            const int64_t stop = se < e ? se : e;
            for (int64_t j = p - so; p < stop; ++p, ++j) {
                const uint64_t x = g.byte(ctx, j);
                const int k = (int)(p - c * 16);
                if (k < 8) a |= x << (8 * k); else b |= x << (8 * (k - 8));
            }
            ++s;
        }
        if (e - p0 == 16) {
            *(uint4 *)(out + c * 16) = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
        } else {
            for (int64_t q = p0; q < e; ++q) {
                const int k = (int)(q - c * 16);
                out[q] = (uint8_t)(k < 8 ? a >> (8 * k) : b >> (8 * (k - 8)));
            }
        }
    }
}

// segment r (a row being appended) = its URL cell in the text
struct ArenaGen {
    const uint8_t *text;
    const int64_t *url_pos;
    __device__ __forceinline__ const uint8_t *open(int64_t s) const { return text + url_pos[s]; }
    __device__ __forceinline__ uint64_t byte(const uint8_t *src, int64_t j) const { return src[j]; }
};

__device__ __forceinline__ int dec_digits(int64_t v)   // v in [0, 10^18)
{
    int d = 1;
    for (int64_t t = 10; d < 18 && v >= t; t *= 10) ++d;
    return d;
}

// segment 0 = the header line, segment k + 1 = kept row k: decimal(ts) ',' ['"'] url ['"'] '\n'
struct CsvGen {
    const int64_t *ts, *kept_row, *kept_off;
    const uint8_t *kept_bytes, *quoted;
    struct Ctx {
        int64_t ts, ulen;
        const uint8_t *url;
        int nd, q;
    };
    __device__ __forceinline__ Ctx open(int64_t s) const
    {
        Ctx c{0, 0, nullptr, 0, 0};
        if (s == 0) { c.nd = -1; return c; }
        const int64_t k = s - 1;
        c.ts = ts[kept_row[k]];
        c.nd = dec_digits(c.ts);
        c.url = kept_bytes + kept_off[k];
        c.ulen = kept_off[k + 1] - kept_off[k];
        c.q = quoted[k];
        return c;
    }
    __device__ __forceinline__ uint64_t byte(const Ctx &c, int64_t j) const
    {
        if (c.nd < 0) return (uint64_t)(uint8_t)HEADER[j];
        if (j < c.nd) {
            int64_t v = c.ts;
            for (int t = c.nd - 1 - (int)j; t > 0; --t) v /= 10;
            return (uint64_t)(0x30 + v % 10);
        }
        j -= c.nd;
        if (j == 0) return 0x2Cull;
        j -= 1;
        if (c.q) {
            if (j == 0 || j == c.ulen + 1) return 0x22ull;
            j -= 1;
        }
        return j < c.ulen ? (uint64_t)c.url[j] : 0x0Aull;
    }
};

// seglen[0] = the header's length, seglen[k + 1] = the length of kept row k's line; quoted[k] = its URL has a ','
__global__ __launch_bounds__(BLOCK) void cx_linelen_kernel(int64_t n_kept, const int64_t *__restrict__ ts,
                                                           const int64_t *__restrict__ kept_row,
                                                           const int64_t *__restrict__ kept_off,
                                                           const uint8_t *__restrict__ kept_bytes,
                                                           unsigned long long *__restrict__ seglen,
                                                           uint8_t *__restrict__ quoted)
{
    constexpr uint64_t ONES = 0x0101010101010101ull;
    for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < n_kept; k += (int64_t)gridDim.x * BLOCK) {
        const int64_t b = kept_off[k], e = kept_off[k + 1];
        bool comma = false;
        // (aligned 8 bytes under [b, e): inside the kept bytes and their padding)
        for (int64_t w = b & ~(int64_t)7; w < e && !comma; w += 8) {
            const uint64_t v = *(const uint64_t *)(kept_bytes + w);
            const int b0 = w < b ? (int)(b - w) : 0;
            const int b1 = e - w >= 8 ? 8 : (int)(e - w);
            const uint64_t in = ~((1ull << (8 * b0)) - 1ull) & (b1 == 8 ? ~0ull : (1ull << (8 * b1)) - 1ull);
            comma = (eq8(v, 0x2Cull * ONES) & in) != 0;
        }
        quoted[k] = comma ? 1 : 0;
        seglen[k + 1] = (unsigned long long)(dec_digits(ts[kept_row[k]]) + 1 + (e - b) + (comma ? 2 : 0) + 1);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) seglen[0] = HEADER_LEN;
}

// ---- the surviving rows rendered in a given order into several files (kw_cdx_csv_select_*)
//
// order[0, n_order) indexes the last run's surviving rows; seg[0 .. n_seg] bounds the files in it.  The output is a
// list of m = n_order + n_seg lines: file s is its header line (line seg[s] + s) and then one line a selected row
// (order position j of file s is line j + s + 1).  src[line] = -1 for a header, else the surviving row's index with
// bit 62 set when its URL is quoted; len[line] its bytes, scanned in place by scan_launch into the lines' offsets.
// The copy is cx_fill_kernel<SelGen>: a lane owns 16 bytes of the output, so the stores are full and coalesced
// whatever the order; the gather is on the read side.
constexpr int64_t SEL_QUOTED = (int64_t)1 << 62;

struct SelErrs {
    unsigned long long seg;     // the first s with a bad bound seg[s] (NONE)
    unsigned long long order;   // the first j with order[j] outside [0, n_kept) (NONE)
};

// lane = bound s: seg[0] = 0, seg[n_seg] = n_order, ascending; file s's header line.  A bound is only ever used as
// an index after it was found inside [0, n_order].
__global__ __launch_bounds__(BLOCK) void cx_sel_seg_kernel(const int64_t *__restrict__ seg, int64_t n_seg, int64_t n_order,
                                                           unsigned long long *__restrict__ len, int64_t *__restrict__ src,
                                                           SelErrs *__restrict__ errs)
{
    for (int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x; s <= n_seg; s += (int64_t)gridDim.x * BLOCK) {
        const int64_t b = seg[s];
        bool ok = b >= 0 && b <= n_order;
        if (s == 0) ok = ok && b == 0;
        if (s == n_seg) ok = ok && b == n_order;
        if (s > 0) ok = ok && b >= seg[s - 1];
        if (!ok) { atomicMin(&errs->seg, (unsigned long long)s); continue; }
        if (s < n_seg) {
            len[b + s] = HEADER_LEN;
            src[b + s] = -1;
        }
    }
}

// lane = order position j: the index checked, the file found, the line's length (as cx_linelen_kernel)
__global__ __launch_bounds__(BLOCK) void cx_sel_len_kernel(const int64_t *__restrict__ order, int64_t n_order,
                                                           const int64_t *__restrict__ seg, int64_t n_seg, int64_t n_kept,
                                                           const int64_t *__restrict__ ts, int64_t row_base,
                                                           const int64_t *__restrict__ kept_row,
                                                           const int64_t *__restrict__ kept_off,
                                                           const uint8_t *__restrict__ kept_bytes,
                                                           unsigned long long *__restrict__ len, int64_t *__restrict__ src,
                                                           SelErrs *__restrict__ errs)
{
    constexpr uint64_t ONES = 0x0101010101010101ull;
    for (int64_t j = (int64_t)blockIdx.x * BLOCK + threadIdx.x; j < n_order; j += (int64_t)gridDim.x * BLOCK) {
        const int64_t s = seg_find(seg, 0, n_seg, j);   // (in [0, n_seg) whatever seg holds: line < n_order + n_seg)
        const int64_t line = j + s + 1;
        const int64_t k = order[j];
        if (k < 0 || k >= n_kept) {   // (never read as an address)
            atomicMin(&errs->order, (unsigned long long)j);
            len[line] = 0;
            src[line] = -1;
            continue;
        }
        const int64_t b = kept_off[k], e = kept_off[k + 1];
        bool comma = false;
        for (int64_t w = b & ~(int64_t)7; w < e && !comma; w += 8) {
            const uint64_t v = *(const uint64_t *)(kept_bytes + w);
            const int b0 = w < b ? (int)(b - w) : 0;
            const int b1 = e - w >= 8 ? 8 : (int)(e - w);
            const uint64_t in = ~((1ull << (8 * b0)) - 1ull) & (b1 == 8 ? ~0ull : (1ull << (8 * b1)) - 1ull);
            comma = (eq8(v, 0x2Cull * ONES) & in) != 0;
        }
        len[line] = (unsigned long long)(dec_digits(ts[row_base + kept_row[k]]) + 1 + (e - b) + (comma ? 2 : 0) + 1);
        src[line] = comma ? (k | SEL_QUOTED) : k;
    }
}

// seg_bytes[s] = the bytes of file s, from the scanned line offsets (off[m] = the total)
__global__ __launch_bounds__(BLOCK) void cx_sel_bytes_kernel(const int64_t *__restrict__ seg, int64_t n_seg,
                                                             const int64_t *__restrict__ off,
                                                             int64_t *__restrict__ seg_bytes)
{
    for (int64_t s = (int64_t)blockIdx.x * BLOCK + threadIdx.x; s < n_seg; s += (int64_t)gridDim.x * BLOCK)
        seg_bytes[s] = off[seg[s + 1] + s + 1] - off[seg[s] + s];
}

// line l = a header (src[l] < 0) or surviving row src[l]: as CsvGen
struct SelGen {
    const int64_t *ts, *kept_row, *kept_off;
    const uint8_t *kept_bytes;
    const int64_t *src;
    int64_t row_base;
    __device__ __forceinline__ CsvGen::Ctx open(int64_t l) const
    {
        CsvGen::Ctx c{0, 0, nullptr, 0, 0};
        const int64_t v = src[l];
        if (v < 0) { c.nd = -1; return c; }
        const int64_t k = v & (SEL_QUOTED - 1);
        c.ts = ts[row_base + kept_row[k]];
        c.nd = dec_digits(c.ts);
        c.url = kept_bytes + kept_off[k];
        c.ulen = kept_off[k + 1] - kept_off[k];
        c.q = (v & SEL_QUOTED) ? 1 : 0;
        return c;
    }
    __device__ __forceinline__ uint64_t byte(const CsvGen::Ctx &c, int64_t j) const { return CsvGen{}.byte(c, j); }
};

__global__ __launch_bounds__(BLOCK) void cx_sel_ts_kernel(int64_t n_kept, const int64_t *__restrict__ ts, int64_t row_base,
                                                          const int64_t *__restrict__ kept_row, int64_t *__restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * BLOCK + threadIdx.x; k < n_kept; k += (int64_t)gridDim.x * BLOCK)
        out[k] = ts[row_base + kept_row[k]];
}

// ---- quoted CSV, one column out (kw_csv_append; the rule: DESIGN.md §7, tests/resume_rule.py)
//
//   cv_quotes_kernel    a tile's '"' bytes counted (their exclusive scan over the tiles carries the quote parity
//                       into every tile, however many tiles a quoted cell spans); the first NUL; UTF-8 validated by
//                       the lanes whose 16 bytes hold a byte >= 0x80 (from the code point boundary before them).
//   cv_tile_kernel<M>   the tile's masks again with the carried parity: a lane's in-quote mask is the prefix xor of
//                       its '"' mask on the parity before it (a block scan of the lanes' '"' counts).  Outside quotes
//                       a '\n' ends a record, a ',' ends a field; a record of no bytes but its terminator is
//                       skipped.  COUNT: record ends, delimiters and record starts per tile, the quote discipline
//                       and the '\r' rule.  ENDS (after the scans): every record's start, its end and the delimiters
//                       before its end, at the record's rank.  CELLS: a delimiter's rank within its record from the
//                       count at the end of the record before it; the two that bound the column give the cell.
//   cv_rows_kernel      lane = record: the field count from the two delimiter counts, the cell without its outer
//                       quotes, ':' looked for and '"' / '\n' / '\r' refused 8 bytes a step.
//   cv_last_end_kernel  a window of a stream (kw_csv_stream_window): the position after the last '\n' outside quotes,
//                       from the same masks and carried parity; every pass after it runs over the bytes before it.
//   then scan_launch, cx_off_kernel and cx_fill_kernel<ArenaGen> as kw_cdx_append.
enum { CV_COUNT = 0, CV_ENDS = 1, CV_CELLS = 2 };

// positions of the first offenders (NONE), in the words after a parse's four totals
struct CsvErrs {
    unsigned long long nul, utf8, quote, cr, fields, url;
};

__global__ __launch_bounds__(BLOCK) void cv_quotes_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t ntiles,
                                                          unsigned long long *__restrict__ tile_q,
                                                          CsvErrs *__restrict__ errs)
{
    quotes_tiles(text, n, ntiles, tile_q, &errs->nul, &errs->utf8);
}

struct CsvArgs {
    const uint8_t *text;
    int64_t n, ntiles;
    unsigned long long *tile_q, *tile_e, *tile_d;   // per tile: '"' bytes, record ends, delimiters (scanned)
    unsigned long long *n_starts;                   // COUNT: the records that are not zero-length
    CsvErrs *errs;
    int64_t *rec_start, *end_pos, *end_dcnt, *cell_start, *cell_end;
    int64_t cap;                                    // entries of the per-record arrays
    int url_col;
    int r0;                                         // the first record that is a row: 1 when record 0 is the header
};

template <int MODE>
__global__ __launch_bounds__(BLOCK) void cv_tile_kernel(CsvArgs A)
{
    __shared__ unsigned long long ws[BLOCK / 64];
    const uint8_t *__restrict__ text = A.text;
    const int64_t n = A.n;
    for (int64_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        const int64_t p = tile * TILE + (int64_t)threadIdx.x * 16;
        uint32_t valid = 0, q = 0, cm = 0, nl = 0, cr = 0;
        // the bytes around the lane's 16: the text is preceded by (virtual) line ends, 0x100 stands for its end
        uint32_t prev1 = 0x0Au, prev2 = 0x0Au, next = 0x100u;
        if (p < n) {
            const uint4 v = *(const uint4 *)(text + p);
            valid = n - p >= 16 ? 0xFFFFu : (1u << (int)(n - p)) - 1u;
            q = mask16(v, 0x22u) & valid;
            cm = mask16(v, 0x2Cu) & valid;
            nl = mask16(v, 0x0Au) & valid;
            cr = mask16(v, 0x0Du) & valid;
            if (p > 0) { prev1 = text[p - 1]; prev2 = text[p - 2]; }
            if (p + 16 < n) next = text[p + 16];
        }
        unsigned long long total;
        const unsigned long long qb = block_scan((unsigned long long)__popc(q), ws, &total);
        const uint32_t inpar = (uint32_t)((A.tile_q[tile] + qb) & 1ull);
        uint32_t incl = q;   // bit k: the parity of the '"' bytes in bits 0..k
        incl ^= incl << 1;
        incl ^= incl << 2;
        incl ^= incl << 4;
        incl ^= incl << 8;
        const uint32_t sb = ((incl << 1) ^ (inpar ? 0xFFFFu : 0u)) & valid;   // bit k: byte k lies inside quotes
        const uint32_t pnl = ((nl << 1) | (prev1 == 0x0Au ? 1u : 0u)) & 0xFFFFu;   // the byte before is '\n'
        const uint32_t pcr = ((cr << 1) | (prev1 == 0x0Du ? 1u : 0u)) & 0xFFFFu;
        const uint32_t pn2 = ((nl << 2) | (prev1 == 0x0Au ? 2u : 0u) | (prev2 == 0x0Au ? 1u : 0u)) & 0xFFFFu;
        // a record end that is not zero-length, a record start, a delimiter
        const uint32_t E = nl & ~sb & ~(pnl | (pcr & pn2));
        const uint32_t ST = valid & ~sb & pnl & ~nl & ~cr;
        const uint32_t DL = cm & ~sb;
        if (MODE == CV_COUNT) {
            const uint32_t pcm = ((cm << 1) | (prev1 == 0x2Cu ? 1u : 0u)) & 0xFFFFu;
            const uint32_t pq = ((q << 1) | (prev1 == 0x22u ? 1u : 0u)) & 0xFFFFu;
            const uint32_t top = 0x8000u;
            const uint32_t ncm = (cm >> 1) | (next == 0x2Cu ? top : 0u), nnl = (nl >> 1) | (next == 0x0Au ? top : 0u);
            const uint32_t ncr = (cr >> 1) | (next == 0x0Du ? top : 0u), nq = (q >> 1) | (next == 0x22u ? top : 0u);
            const uint32_t eot = (p < n && n - p <= 16) ? 1u << (int)(n - p - 1) : 0u;   // the text's last byte
            const uint32_t bad_q = ((q & ~sb) & ~(pcm | pnl | pq)) | ((q & sb) & ~(ncm | nnl | ncr | nq | eot));
            const uint32_t bad_c = cr & ~sb & ~nnl;
            unsigned long long eq = NONE, ec = NONE;
            if (bad_q) eq = (unsigned long long)p + __builtin_ctz(bad_q);
            if (bad_c) ec = (unsigned long long)p + __builtin_ctz(bad_c);
            if (__any((eq & ec) != NONE)) {
                eq = wave_min(eq);
                ec = wave_min(ec);
                if ((threadIdx.x & 63) == 0) {
                    if (eq != NONE) atomicMin(&A.errs->quote, eq);
                    if (ec != NONE) atomicMin(&A.errs->cr, ec);
                }
            }
            (void)block_scan((unsigned long long)__popc(E) | ((unsigned long long)__popc(DL) << 16) |
                                 ((unsigned long long)__popc(ST) << 32),
                             ws, &total);
            if (threadIdx.x == 0) {
                A.tile_e[tile] = total & 0xFFFFull;
                A.tile_d[tile] = (total >> 16) & 0xFFFFull;
                if (total >> 32) atomicAdd(A.n_starts, total >> 32);
            }
        } else {
            const unsigned long long before =
                block_scan((unsigned long long)__popc(E) | ((unsigned long long)__popc(DL) << 32), ws, &total);
            const int64_t ce = (int64_t)(A.tile_e[tile] + (before & 0xFFFFFFFFull));   // record ends before the lane
            const int64_t cd = (int64_t)(A.tile_d[tile] + (before >> 32));             // delimiters before it
            uint32_t todo = MODE == CV_ENDS ? (E | ST) : DL;
            while (todo) {
                const int k = __builtin_ctz(todo);
                todo &= todo - 1u;
                const uint32_t below = (1u << k) - 1u;
                const int64_t r = ce + __popc(E & below);   // the record the byte belongs to
                if (r >= A.cap) continue;                   // (cannot happen in a text that passed COUNT)
                if (MODE == CV_ENDS) {
                    if ((E >> k) & 1u) {
                        A.end_pos[r] = p + k;
                        A.end_dcnt[r] = cd + __popc(DL & below);
                    } else {
                        A.rec_start[r] = p + k;
                    }
                } else if (r >= A.r0) {
                    // the delimiter ends field f
                    const int64_t f = cd + __popc(DL & below) - (r > 0 ? A.end_dcnt[r - 1] : 0);
                    if (f == A.url_col - 1) A.cell_start[r] = p + k + 1;
                    if (f == A.url_col) A.cell_end[r] = p + k;
                }
            }
        }
    }
}

// The windowed form (kw_csv_stream_window): the position after the last '\n' outside quotes, as a maximum over the
// lanes (0: none).  tile_q holds the tiles' scanned '"' counts, so the parity is cv_tile_kernel's.
__global__ __launch_bounds__(BLOCK) void cv_last_end_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t ntiles,
                                                            const unsigned long long *__restrict__ tile_q,
                                                            unsigned long long *__restrict__ last)
{
    __shared__ unsigned long long ws[BLOCK / 64];
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t p = tile * TILE + (int64_t)threadIdx.x * 16;
        uint32_t valid = 0, q = 0, nl = 0;
        if (p < n) {
            const uint4 v = *(const uint4 *)(text + p);
            valid = n - p >= 16 ? 0xFFFFu : (1u << (int)(n - p)) - 1u;
            q = mask16(v, 0x22u) & valid;
            nl = mask16(v, 0x0Au) & valid;
        }
        unsigned long long total;
        const unsigned long long qb = block_scan((unsigned long long)__popc(q), ws, &total);
        const uint32_t inpar = (uint32_t)((tile_q[tile] + qb) & 1ull);
        uint32_t incl = q;
        incl ^= incl << 1;
        incl ^= incl << 2;
        incl ^= incl << 4;
        incl ^= incl << 8;
        const uint32_t sb = ((incl << 1) ^ (inpar ? 0xFFFFu : 0u)) & valid;
        const uint32_t ends = nl & ~sb;
        unsigned long long e = ends ? (unsigned long long)p + (unsigned long long)(32 - __builtin_clz(ends)) : 0ull;
        if (__any(e != 0ull)) {
            for (int d = 32; d >= 1; d >>= 1) {
                const unsigned long long y = __shfl_xor(e, d, 64);
                e = y > e ? y : e;
            }
            if ((threadIdx.x & 63) == 0) atomicMax(last, e);
        }
    }
}

// Record r >= r0 (r0 = 1: record 0 is the header): [rec_start[r], its end); the records past n_ends end with the
// text.  The cell's position and length go to cell_start[r] / cell_end[r] (their own lane's entries).
__global__ __launch_bounds__(BLOCK) void cv_rows_kernel(const uint8_t *__restrict__ text, int64_t n, int64_t r0,
                                                        int64_t n_rec, int64_t n_ends, int64_t n_delims, int n_fields,
                                                        int url_col,
                                                        const int64_t *__restrict__ rec_start,
                                                        const int64_t *__restrict__ end_pos,
                                                        const int64_t *__restrict__ end_dcnt, int64_t *cell_start,
                                                        int64_t *cell_end, CsvErrs *__restrict__ errs)
{
    constexpr uint64_t ONES = 0x0101010101010101ull;
    for (int64_t r = r0 + (int64_t)blockIdx.x * BLOCK + threadIdx.x; r < n_rec; r += (int64_t)gridDim.x * BLOCK) {
        const int64_t s = rec_start[r];
        int64_t e = n, dc = n_delims;
        if (r < n_ends) {
            e = end_pos[r];
            dc = end_dcnt[r];
            if (e > s && text[e - 1] == 0x0Du) --e;   // "\r\n"
        }
        if (dc - (r > 0 ? end_dcnt[r - 1] : 0) + 1 != (int64_t)n_fields) {
            atomicMin(&errs->fields, (unsigned long long)s);
            continue;
        }
        int64_t b = url_col == 0 ? s : cell_start[r];
        int64_t c = url_col == n_fields - 1 ? e : cell_end[r];
        if (c - b >= 2 && text[b] == 0x22u) { ++b; --c; }   // (a quoted cell ends with its closing quote)
        bool colon = false, bad = false;
        // (aligned 8 bytes under [b, c), c <= n: inside the text's readable 16-byte granule)
        for (int64_t w = b & ~(int64_t)7; w < c; w += 8) {
            const uint64_t v = *(const uint64_t *)(text + w);
            const int b0 = w < b ? (int)(b - w) : 0;
            const int b1 = c - w >= 8 ? 8 : (int)(c - w);
            const uint64_t in = ~((1ull << (8 * b0)) - 1ull) & (b1 == 8 ? ~0ull : (1ull << (8 * b1)) - 1ull);
            colon |= (eq8(v, 0x3Aull * ONES) & in) != 0;
            bad |= ((eq8(v, 0x22ull * ONES) | eq8(v, 0x0Aull * ONES) | eq8(v, 0x0Dull * ONES)) & in) != 0;
        }
        if (bad || !colon) {
            atomicMin(&errs->url, (unsigned long long)s);
            continue;
        }
        cell_start[r] = b;
        cell_end[r] = c - b;
    }
}

}  // namespace cx

using namespace cx;

struct kw_cdx_store {
    // the rows: arena (URL bytes; 64 readable bytes past n_bytes), off (n + 1), ts (n)
    uint8_t *arena = nullptr;
    size_t arena_cap = 0;
    int64_t *off = nullptr, *ts = nullptr;
    size_t rows_cap = 0;
    int64_t n = 0, n_bytes = 0;
    uint8_t *code = nullptr;
    size_t code_cap = 0;
    // append scratch
    void *d_tiles = nullptr;
    size_t tiles_bytes = 0;
    void *d_rows = nullptr;
    size_t rows_bytes = 0;
    // render
    void *d_csv = nullptr;       // segment offsets (n_kept + 2) + quoted flags
    size_t csv_scratch = 0;
    int64_t csv_bytes = 0, csv_kept = 0;
    uint64_t run_serial = 0;     // the kw_dedup_run kw_cdx_run made (0: none since the store changed)
    bool csv_ready = false;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float ms[3] = {0.f, 0.f, 0.f};
    // select render (kw_cdx_csv_select_*)
    uint64_t sel_serial = 0;     // the kw_dedup_run of the last kw_cdx_run / _run_exclude / _run_exclude_unique over
                                 //   this store (0: none since the store changed)
    void *d_sel = nullptr;       // line offsets (m + 1), line sources (m), scan chunks, the error words
    size_t sel_scratch = 0;
    int64_t sel_lines = 0, sel_bytes = 0;
    bool sel_ready = false;
    float sel_ms[2] = {0.f, 0.f};
    // the windowed CSV append (kw_csv_stream_*): the header arguments, the rows and bytes kw_csv_stream_begin noted,
    // the file position of the next window's first byte
    bool stream_open = false, stream_first = false, stream_final = false, stream_bad = false;
    std::string stream_header;
    int32_t stream_col = 0, stream_fields = 0;
    int64_t stream_n0 = 0, stream_bytes0 = 0, stream_pos = 0;
};

void kw_cdx_store_destroy(kw_cdx_store *s)
{
    if (!s) return;
    if (s->arena) (void)hipFree(s->arena);
    if (s->off) (void)hipFree(s->off);
    if (s->ts) (void)hipFree(s->ts);
    if (s->code) (void)hipFree(s->code);
    if (s->d_tiles) (void)hipFree(s->d_tiles);
    if (s->d_rows) (void)hipFree(s->d_rows);
    if (s->d_csv) (void)hipFree(s->d_csv);
    if (s->d_sel) (void)hipFree(s->d_sel);
    for (auto &e : s->ev)
        if (e) (void)hipEventDestroy(e);
    delete s;
}

static int store_get(kw_dedup *h, kw_cdx_store **out)
{
    if (!h->cdx) {
        kw_cdx_store *s = new kw_cdx_store();
        h->cdx = s;
        for (auto &e : s->ev) KWCHK(h, hipEventCreate(&e));
    }
    *out = h->cdx;
    return KW_OK;
}

// a scratch buffer of at least `bytes`
static int scratch_fit(kw_dedup *h, void **buf, size_t *have, size_t bytes)
{
    return ensure(h, buf, have, bytes, bytes + bytes / 4);
}

// a store buffer of at least `need` bytes that keeps its first `used` bytes
static int grow_keep(kw_dedup *h, void **buf, size_t *cap, size_t need, size_t used, hipStream_t st)
{
    return ensure_keep(h, buf, cap, need, used, std::max(need, *cap * 2), false, st);
}

// the blocks for `items` lanes, 16 a CU at most
static int cus_grid(const kw_dedup *h, int64_t items) { return (int)grid_for(items, BLOCK, (int64_t)h->cus * 16).x; }

// the line (the '\n' bytes before it) of byte position pos
static int line_of(kw_dedup *h, const uint8_t *d_text, int64_t pos, unsigned long long *d_cnt, hipStream_t st,
                   int64_t *line)
{
    unsigned long long c = 0;
    KWCHK(h, hipMemsetAsync(d_cnt, 0, 8, st));
    if (pos > 0) {
        hipLaunchKernelGGL(cx_count_nl_kernel, dim3(cus_grid(h, (pos + 15) / 16)), dim3(BLOCK), 0, st, d_text, pos, d_cnt);
        KWCHK(h, hipGetLastError());
    }
    KWCHK(h, hipMemcpyAsync(&c, d_cnt, 8, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    *line = (int64_t)c;
    return KW_OK;
}

extern "C" int kw_cdx_tile_bytes(void) { return TILE; }

extern "C" int kw_cdx_begin(kw_dedup *h)
{
    if (!h) return KW_EINVAL;
    kw_cdx_store *s = nullptr;
    int rc = store_get(h, &s);
    if (rc) return rc;
    s->n = s->n_bytes = 0;
    s->stream_open = false;
    s->run_serial = 0;
    s->csv_ready = false;
    s->sel_serial = 0;
    s->sel_ready = false;
    s->ms[0] = s->ms[1] = s->ms[2] = 0.f;
    return KW_OK;
}

extern "C" int kw_cdx_append(kw_dedup *h, const uint8_t *d_text, int64_t n_bytes, const kw_cdx_dialect *d,
                             int64_t *n_rows, int32_t *verdict, int64_t *bad_line, void *stream)
{
    if (!h) return KW_EINVAL;
    if (!d || !n_rows || !verdict || !bad_line || n_bytes < 0 || (n_bytes > 0 && !d_text)) {
        h->err = "kw_cdx_append: bad arguments";
        return KW_EINVAL;
    }
    if (((uintptr_t)d_text & 15) != 0) { h->err = "kw_cdx_append: the text must be 16-byte aligned"; return KW_EINVAL; }
    if ((d->delim != ' ' && d->delim != ',') || d->ts_col < 0 || d->url_col < 0 || d->ts_col == d->url_col ||
        d->ts_col > 1023 || d->url_col > 1023 || d->skip_lines < 0 || d->skip_lines > 1 || d->exact_fields < 0 ||
        (d->exact_fields && d->exact_fields <= std::max(d->ts_col, d->url_col))) {
        h->err = "kw_cdx_append: unsupported dialect";
        return KW_EINVAL;
    }
    KWCHK(h, hipSetDevice(h->device));
    kw_cdx_store *s = nullptr;
    int rc = store_get(h, &s);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    *n_rows = 0;
    *verdict = KW_CDX_OK;
    *bad_line = -1;
    const Dialect D{(uint32_t)d->delim, d->ts_col, d->url_col, d->skip_lines, d->exact_fields};
    if (n_bytes == 0) {
        if (D.skip) { *verdict = KW_CDX_HEADER; *bad_line = 0; }
        return KW_OK;
    }
    // ---- rows per tile, the byte conditions
    const int64_t ntiles = (n_bytes + TILE - 1) / TILE;
    rc = scratch_fit(h, &s->d_tiles, &s->tiles_bytes, align256(8 * (size_t)ntiles) + align256(8 * SCAN_CHUNKS) + 256);
    if (rc) return rc;
    unsigned long long *tile_cnt = (unsigned long long *)s->d_tiles;
    unsigned long long *chunk = (unsigned long long *)((uint8_t *)s->d_tiles + align256(8 * (size_t)ntiles));
    unsigned long long *small = chunk + align256(8 * SCAN_CHUNKS) / 8;   // [0] a scan's total, [1] a line count, [4..8) Errs
    Errs *errs = (Errs *)(small + 4);
    KWCHK(h, hipMemsetAsync(small, 0xFF, 64, st));
    KWCHK(h, hipEventRecord(s->ev[0], st));
    const int tgrid = (int)std::min<int64_t>(ntiles, (int64_t)h->cus * 16);
    hipLaunchKernelGGL(cx_lines_kernel<false>, dim3(tgrid), dim3(BLOCK), 0, st, d_text, n_bytes, ntiles, tile_cnt, errs,
                       (int64_t *)nullptr);
    scan_launch(tile_cnt, ntiles, chunk, small, st);
    KWCHK(h, hipGetLastError());
    unsigned long long hs[8];
    KWCHK(h, hipMemcpyAsync(hs, small, sizeof(hs), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    const int64_t n_lines = (int64_t)hs[0];
    for (int k = 0; k < 3; ++k) {
        if (hs[4 + k] == NONE) continue;
        *verdict = KW_CDX_QUOTE + k;
        return line_of(h, d_text, (int64_t)hs[4 + k], small + 1, st, bad_line);
    }
    if (n_lines == 0) {
        if (D.skip) { *verdict = KW_CDX_HEADER; *bad_line = 0; }
        return KW_OK;
    }
    const int64_t n_new = n_lines - D.skip;
    if (s->n + n_new >= ((int64_t)1 << 32)) { h->err = "kw_cdx_append: more than 2^32 - 1 rows"; return KW_EUNSUPPORTED; }
    // ---- row starts, the rows parsed (timestamps straight into the store, past its rows)
    {
        size_t cap = s->rows_cap * 8, cap2 = s->rows_cap * 8;
        const size_t need = 8 * ((size_t)(s->n + n_new) + 1);
        rc = grow_keep(h, (void **)&s->off, &cap, need, 8 * ((size_t)s->n + 1), st);
        if (!rc) rc = grow_keep(h, (void **)&s->ts, &cap2, cap, 8 * (size_t)s->n, st);
        if (rc) return rc;
        s->rows_cap = cap / 8;
    }
    rc = scratch_fit(h, &s->d_rows, &s->rows_bytes, 3 * align256(8 * ((size_t)n_lines + 1)));
    if (rc) return rc;
    int64_t *row_start = (int64_t *)s->d_rows;
    int64_t *url_pos = (int64_t *)((uint8_t *)s->d_rows + align256(8 * ((size_t)n_lines + 1)));
    unsigned long long *url_len = (unsigned long long *)((uint8_t *)s->d_rows + 2 * align256(8 * ((size_t)n_lines + 1)));
    hipLaunchKernelGGL(cx_lines_kernel<true>, dim3(tgrid), dim3(BLOCK), 0, st, d_text, n_bytes, ntiles, tile_cnt, errs,
                       row_start);
    hipLaunchKernelGGL(cx_parse_kernel, dim3(cus_grid(h, n_lines)), dim3(BLOCK), 0, st, d_text, n_bytes,
                       (const int64_t *)row_start, n_lines, D, s->ts + s->n, url_pos, url_len, errs);
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipEventRecord(s->ev[1], st));
    KWCHK(h, hipMemcpyAsync(hs, small, sizeof(hs), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    if (hs[7] != NONE) {
        static const int32_t codes[5] = {KW_CDX_HEADER, KW_CDX_UTF8, KW_CDX_FIELDS, KW_CDX_TS, KW_CDX_URL};
        *verdict = codes[std::min<unsigned long long>(hs[7] & 7, 4)];
        return line_of(h, d_text, (int64_t)(hs[7] >> 3), small + 1, st, bad_line);
    }
    // ---- compaction: the URL lengths scanned, the offsets, the URL cells copied into the arena
    int64_t total = 0;
    if (n_new > 0) {
        scan_launch(url_len, n_new, chunk, small, st);
        KWCHK(h, hipGetLastError());
        KWCHK(h, hipMemcpyAsync(hs, small, 8, hipMemcpyDeviceToHost, st));
        KWCHK(h, hipStreamSynchronize(st));
        total = (int64_t)hs[0];
        rc = grow_keep(h, (void **)&s->arena, &s->arena_cap, (size_t)(s->n_bytes + total) + 64, (size_t)s->n_bytes, st);
        if (rc) return rc;
        hipLaunchKernelGGL(cx_off_kernel, dim3(cus_grid(h, n_new + 1)), dim3(BLOCK), 0, st, s->off + s->n,
                           (const unsigned long long *)url_len, (const unsigned long long *)small, n_new, s->n_bytes);
        if (total > 0)
            hipLaunchKernelGGL(cx_fill_kernel<ArenaGen>, dim3(cus_grid(h, (total + 31) / 16)), dim3(BLOCK), 0, st, s->arena,
                               (const int64_t *)(s->off + s->n), n_new, ArenaGen{d_text, url_pos});
        KWCHK(h, hipGetLastError());
    }
    KWCHK(h, hipEventRecord(s->ev[2], st));
    KWCHK(h, hipStreamSynchronize(st));
    float a = 0.f, b = 0.f;
    KWCHK(h, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
    KWCHK(h, hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
    s->ms[0] += a;
    s->ms[1] += b;
    s->n += n_new;
    s->n_bytes += total;
    s->run_serial = 0;
    s->csv_ready = false;
    s->sel_serial = 0;
    s->sel_ready = false;
    *n_rows = n_new;
    return KW_OK;
}

// a header line kw_csv_append can be given: no '"' or line break, n_fields names, the column among them
static bool csv_header_ok(const char *header_line, int32_t url_col, int32_t n_fields)
{
    const size_t hl = strlen(header_line);
    int commas = 0;
    bool plain = hl >= 1 && hl <= 255;
    for (size_t k = 0; k < hl && plain; ++k) {
        const char c = header_line[k];
        commas += c == ',';
        plain = c != '"' && c != '\n' && c != '\r';
    }
    return plain && n_fields == commas + 1 && url_col >= 0 && url_col < n_fields;
}

// The cap on the tile kernels' launch grids: the device's, or the tests' KW_TEST_CSV_GRID in [1, 2048] (read per call:
// the kernels' loops then make several trips on a text of a few tiles).
static int csv_grid_cap(const kw_dedup *h) { return (int)env_int("KW_TEST_CSV_GRID", 1, 2048, h->cus * 16); }

// How csv_parse reads a text: the whole file (kw_csv_append), or one window of a stream (kw_csv_stream_window).
struct CsvMode {
    bool window;   // a window: only the bytes before *consumed are judged, a window without rows is not refused
    bool first;    // the text starts with the header line (record 0)
    bool final;    // the text's end is the file's end
};

// kw_csv_append's parse over d_text[0, n_win).  A window (M.window) first finds *consumed, the position after the last
// '\n' outside quotes (n_win when final), and then runs every pass over [0, *consumed) alone; positions are the text's.
static int csv_parse(kw_dedup *h, kw_cdx_store *s, const uint8_t *d_text, int64_t n_win, const char *header_line,
                     int32_t url_col, int32_t n_fields, CsvMode M, int64_t *consumed, int64_t *n_rows,
                     int32_t *verdict, int64_t *bad_pos, hipStream_t st)
{
    int rc;
    const size_t hl = strlen(header_line);
    *n_rows = 0;
    *verdict = KW_CSV_OK;
    *bad_pos = -1;
    *consumed = 0;
    auto refuse = [&](int32_t v, int64_t pos) { *verdict = v; *bad_pos = pos; return KW_OK; };
    if (n_win == 0) return (M.first && M.final) ? refuse(KW_CSV_HEADER, 0) : KW_OK;
    if (M.window && M.first && !M.final && n_win < (int64_t)hl + 1) return KW_OK;   // (not yet the header line)
    // ---- '"' bytes per tile, the byte conditions
    int64_t n_bytes = n_win;
    int64_t ntiles = (n_bytes + TILE - 1) / TILE;
    const size_t tw = align256(8 * (size_t)ntiles);
    rc = scratch_fit(h, &s->d_tiles, &s->tiles_bytes, 3 * tw + align256(8 * SCAN_CHUNKS) + 256);
    if (rc) return rc;
    unsigned long long *tile_q = (unsigned long long *)s->d_tiles;
    unsigned long long *tile_e = (unsigned long long *)((uint8_t *)s->d_tiles + tw);
    unsigned long long *tile_d = (unsigned long long *)((uint8_t *)s->d_tiles + 2 * tw);
    unsigned long long *chunk = (unsigned long long *)((uint8_t *)s->d_tiles + 3 * tw);
    // small: the totals [0] '"' bytes, [1] record ends, [2] delimiters, [3] record starts, then CsvErrs; [12] a
    // scan's total; [13] a window's consumed bytes
    unsigned long long *small = chunk + align256(8 * SCAN_CHUNKS) / 8;
    CsvErrs *errs = (CsvErrs *)(small + 4);
    KWCHK(h, hipMemsetAsync(small, 0, 32, st));
    KWCHK(h, hipMemsetAsync(small + 4, 0xFF, sizeof(CsvErrs), st));
    KWCHK(h, hipMemsetAsync(small + 13, 0, 8, st));
    KWCHK(h, hipEventRecord(s->ev[0], st));
    const int gcap = csv_grid_cap(h);
    int tgrid = (int)std::min<int64_t>(ntiles, (int64_t)gcap);
    hipLaunchKernelGGL(cv_quotes_kernel, dim3(tgrid), dim3(BLOCK), 0, st, d_text, n_bytes, ntiles, tile_q, errs);
    scan_launch(tile_q, ntiles, chunk, small, st);
    if (M.window && !M.final)
        hipLaunchKernelGGL(cv_last_end_kernel, dim3(tgrid), dim3(BLOCK), 0, st, d_text, n_bytes, ntiles,
                           (const unsigned long long *)tile_q, small + 13);
    KWCHK(h, hipGetLastError());
    unsigned long long hs[14];
    uint8_t head[260] = {0};
    KWCHK(h, hipMemcpyAsync(hs, small, sizeof(hs), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipMemcpyAsync(head, d_text, (size_t)std::min<int64_t>(n_bytes, (int64_t)hl + 2), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    if (M.window && !M.final) {
        // only the records that end inside the window are judged: every pass below runs over [0, consumed)
        if (hs[13] > (unsigned long long)n_win) { h->err = "kw_csv_stream_window: a record end past the window"; return KW_ESTATE; }
        n_bytes = (int64_t)hs[13];
        if (n_bytes == 0) return KW_OK;   // (no record ends here: the caller comes back with more bytes)
        ntiles = (n_bytes + TILE - 1) / TILE;
        tgrid = (int)std::min<int64_t>(ntiles, (int64_t)gcap);
    }
    const size_t hn = (size_t)std::min<int64_t>(n_bytes, (int64_t)hl + 2);
    if (hs[4] != NONE && (int64_t)hs[4] < n_bytes) return refuse(KW_CSV_NUL, (int64_t)hs[4]);
    if (hs[5] != NONE && (int64_t)hs[5] < n_bytes) return refuse(KW_CSV_UTF8, (int64_t)hs[5]);
    if (M.first && !(hn > hl && memcmp(head, header_line, hl) == 0 &&
                     (head[hl] == '\n' || (head[hl] == '\r' && hn > hl + 1 && head[hl + 1] == '\n'))))
        return refuse(KW_CSV_HEADER, 0);
    // (a window that is not final ends after a '\n' outside quotes)
    const bool ends_quoted = (!M.window || M.final) && (hs[0] & 1ull) != 0;
    const int64_t r0 = M.first ? 1 : 0;
    *consumed = n_bytes;
    // ---- record ends, delimiters and record starts per tile; the quote discipline, the '\r' rule
    CsvArgs A{};
    A.text = d_text;
    A.n = n_bytes;
    A.ntiles = ntiles;
    A.tile_q = tile_q;
    A.tile_e = tile_e;
    A.tile_d = tile_d;
    A.n_starts = small + 3;
    A.errs = errs;
    A.url_col = url_col;
    A.r0 = (int)r0;
    hipLaunchKernelGGL(cv_tile_kernel<CV_COUNT>, dim3(tgrid), dim3(BLOCK), 0, st, A);
    scan_launch(tile_e, ntiles, chunk, small + 1, st);
    scan_launch(tile_d, ntiles, chunk, small + 2, st);
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipMemcpyAsync(hs, small, sizeof(hs), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    if (hs[6] != NONE || ends_quoted) return refuse(KW_CSV_QUOTE, hs[6] != NONE ? (int64_t)hs[6] : n_bytes);
    if (hs[7] != NONE) return refuse(KW_CSV_CR, (int64_t)hs[7]);
    const int64_t n_ends = (int64_t)hs[1], n_delims = (int64_t)hs[2], n_rec = (int64_t)hs[3];
    if (n_rec < r0 || n_ends > n_rec || n_ends < n_rec - 1) {   // (the header is a record; the last may end with the text)
        h->err = "kw_csv_append: record starts and ends do not pair up";
        return KW_ESTATE;
    }
    const int64_t n_new = n_rec - r0;
    if (n_new == 0 && M.window) return KW_OK;   // (blank lines, or the header alone: kw_csv_stream_end tests the total)
    if (n_new == 0 || s->n + n_new >= ((int64_t)1 << 32)) return refuse(KW_CSV_ROWS, n_bytes);
    // ---- the records located, their cells checked
    const size_t rw = align256(8 * ((size_t)n_rec + 1));
    rc = scratch_fit(h, &s->d_rows, &s->rows_bytes, 5 * rw);
    if (rc) return rc;
    A.rec_start = (int64_t *)s->d_rows;
    A.end_pos = (int64_t *)((uint8_t *)s->d_rows + rw);
    A.end_dcnt = (int64_t *)((uint8_t *)s->d_rows + 2 * rw);
    A.cell_start = (int64_t *)((uint8_t *)s->d_rows + 3 * rw);
    A.cell_end = (int64_t *)((uint8_t *)s->d_rows + 4 * rw);
    A.cap = n_rec + 1;
    KWCHK(h, hipMemsetAsync(s->d_rows, 0, 5 * rw, st));   // (an entry nobody wrote is an empty cell at 0, not a wild one)
    hipLaunchKernelGGL(cv_tile_kernel<CV_ENDS>, dim3(tgrid), dim3(BLOCK), 0, st, A);
    hipLaunchKernelGGL(cv_tile_kernel<CV_CELLS>, dim3(tgrid), dim3(BLOCK), 0, st, A);
    hipLaunchKernelGGL(cv_rows_kernel, dim3(std::min(cus_grid(h, n_new), gcap)), dim3(BLOCK), 0, st, d_text, n_bytes, r0,
                       n_rec, n_ends, n_delims, (int)n_fields, (int)url_col, (const int64_t *)A.rec_start,
                       (const int64_t *)A.end_pos, (const int64_t *)A.end_dcnt, A.cell_start, A.cell_end, errs);
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipEventRecord(s->ev[1], st));
    KWCHK(h, hipMemcpyAsync(hs, small, sizeof(hs), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    if (hs[8] != NONE) return refuse(KW_CSV_FIELDS, (int64_t)hs[8]);
    if (hs[9] != NONE) return refuse(KW_CSV_URL, (int64_t)hs[9]);
    // ---- compaction (as kw_cdx_append): the cell lengths scanned, the offsets, the cells copied into the arena
    {
        size_t cap = s->rows_cap * 8, cap2 = s->rows_cap * 8;
        const size_t need = 8 * ((size_t)(s->n + n_new) + 1);
        rc = grow_keep(h, (void **)&s->off, &cap, need, 8 * ((size_t)s->n + 1), st);
        if (!rc) rc = grow_keep(h, (void **)&s->ts, &cap2, cap, 8 * (size_t)s->n, st);
        if (rc) return rc;
        s->rows_cap = cap / 8;
    }
    const int64_t *url_pos = A.cell_start + r0;
    unsigned long long *url_len = (unsigned long long *)(A.cell_end + r0);
    unsigned long long *grand = small + 12;
    KWCHK(h, hipMemsetAsync(s->ts + s->n, 0, 8 * (size_t)n_new, st));
    scan_launch(url_len, n_new, chunk, grand, st);
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipMemcpyAsync(hs, grand, 8, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    const int64_t total = (int64_t)hs[0];
    rc = grow_keep(h, (void **)&s->arena, &s->arena_cap, (size_t)(s->n_bytes + total) + 64, (size_t)s->n_bytes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(cx_off_kernel, dim3(cus_grid(h, n_new + 1)), dim3(BLOCK), 0, st, s->off + s->n,
                       (const unsigned long long *)url_len, (const unsigned long long *)grand, n_new, s->n_bytes);
    hipLaunchKernelGGL(cx_fill_kernel<ArenaGen>, dim3(cus_grid(h, (total + 31) / 16)), dim3(BLOCK), 0, st, s->arena,
                       (const int64_t *)(s->off + s->n), n_new, ArenaGen{d_text, url_pos});
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipEventRecord(s->ev[2], st));
    KWCHK(h, hipStreamSynchronize(st));
    float a = 0.f, b = 0.f;
    KWCHK(h, hipEventElapsedTime(&a, s->ev[0], s->ev[1]));
    KWCHK(h, hipEventElapsedTime(&b, s->ev[1], s->ev[2]));
    s->ms[0] += a;
    s->ms[1] += b;
    s->n += n_new;
    s->n_bytes += total;
    s->run_serial = 0;
    s->csv_ready = false;
    s->sel_serial = 0;
    s->sel_ready = false;
    *n_rows = n_new;
    return KW_OK;
}

extern "C" int kw_csv_append(kw_dedup *h, const uint8_t *d_text, int64_t n_bytes, const char *header_line,
                             int32_t url_col, int32_t n_fields, int64_t *n_rows, int32_t *verdict, int64_t *bad_pos,
                             void *stream)
{
    if (!h) return KW_EINVAL;
    if (!header_line || !n_rows || !verdict || !bad_pos || n_bytes < 0 || (n_bytes > 0 && !d_text)) {
        h->err = "kw_csv_append: bad arguments";
        return KW_EINVAL;
    }
    if (((uintptr_t)d_text & 15) != 0) { h->err = "kw_csv_append: the text must be 16-byte aligned"; return KW_EINVAL; }
    if (!csv_header_ok(header_line, url_col, n_fields)) {
        h->err = "kw_csv_append: unsupported header line or column";
        return KW_EINVAL;
    }
    KWCHK(h, hipSetDevice(h->device));
    kw_cdx_store *s = nullptr;
    int rc = store_get(h, &s);
    if (rc) return rc;
    if (s->stream_open) { h->err = "kw_csv_append: a kw_csv_stream is open"; return KW_ESTATE; }
    int64_t consumed = 0;
    return csv_parse(h, s, d_text, n_bytes, header_line, url_col, n_fields, CsvMode{false, true, true}, &consumed, n_rows,
                     verdict, bad_pos, (hipStream_t)stream);
}

// ---- the windowed form: kw_csv_stream_begin / _window / _end (the contract: include/kwdedup.h)
static void store_changed(kw_cdx_store *s)
{
    s->run_serial = 0;
    s->csv_ready = false;
    s->sel_serial = 0;
    s->sel_ready = false;
}

extern "C" int kw_csv_stream_begin(kw_dedup *h, const char *header_line, int32_t url_col, int32_t n_fields)
{
    if (!h) return KW_EINVAL;
    if (!header_line || !csv_header_ok(header_line, url_col, n_fields)) {
        h->err = "kw_csv_stream_begin: unsupported header line or column";
        return KW_EINVAL;
    }
    kw_cdx_store *s = nullptr;
    int rc = store_get(h, &s);
    if (rc) return rc;
    if (s->stream_open) { h->err = "kw_csv_stream_begin: a stream is open"; return KW_ESTATE; }
    s->stream_open = true;
    s->stream_first = true;
    s->stream_final = s->stream_bad = false;
    s->stream_header = header_line;
    s->stream_col = url_col;
    s->stream_fields = n_fields;
    s->stream_n0 = s->n;
    s->stream_bytes0 = s->n_bytes;
    s->stream_pos = 0;
    return KW_OK;
}

extern "C" int kw_csv_stream_window(kw_dedup *h, const uint8_t *d_text, int64_t n_bytes, int32_t final, int64_t *consumed,
                                    int64_t *n_rows, int32_t *verdict, int64_t *bad_pos, void *stream)
{
    if (!h) return KW_EINVAL;
    if (!consumed || !n_rows || !verdict || !bad_pos || n_bytes < 0 || (n_bytes > 0 && !d_text)) {
        h->err = "kw_csv_stream_window: bad arguments";
        return KW_EINVAL;
    }
    if (((uintptr_t)d_text & 15) != 0) { h->err = "kw_csv_stream_window: the text must be 16-byte aligned"; return KW_EINVAL; }
    kw_cdx_store *s = h->cdx;
    if (!s || !s->stream_open || s->stream_final || s->stream_bad) {
        h->err = "kw_csv_stream_window: no open stream, or one that has had its final or a refused window";
        return KW_ESTATE;
    }
    KWCHK(h, hipSetDevice(h->device));
    const int rc = csv_parse(h, s, d_text, n_bytes, s->stream_header.c_str(), s->stream_col, s->stream_fields,
                             CsvMode{true, s->stream_first, final != 0}, consumed, n_rows, verdict, bad_pos,
                             (hipStream_t)stream);
    if (rc != KW_OK || *verdict != KW_CSV_OK) {
        s->stream_bad = true;   // (kw_csv_stream_end puts the store back)
        *consumed = 0;
        if (rc == KW_OK) *bad_pos += s->stream_pos;
        return rc;
    }
    if (*consumed > 0) s->stream_first = false;
    s->stream_pos += *consumed;
    s->stream_final = final != 0;
    return KW_OK;
}

extern "C" int kw_csv_stream_end(kw_dedup *h, int32_t commit, int64_t *n_rows_total)
{
    if (!h) return KW_EINVAL;
    kw_cdx_store *s = h->cdx;
    if (!s || !s->stream_open) { h->err = "kw_csv_stream_end: no open stream"; return KW_ESTATE; }
    s->stream_open = false;
    if (n_rows_total) *n_rows_total = 0;
    const int64_t added = s->n - s->stream_n0;
    const bool keep = commit != 0 && !s->stream_bad && s->stream_final && added > 0;
    if (!keep) {
        // off[stream_n0] still holds stream_bytes0: the rows noted by kw_csv_stream_begin are the store again
        s->n = s->stream_n0;
        s->n_bytes = s->stream_bytes0;
        store_changed(s);
        if (commit != 0 && !s->stream_bad && !s->stream_final) {
            h->err = "kw_csv_stream_end: commit before the final window";
            return KW_ESTATE;
        }
        return (commit != 0 && !s->stream_bad) ? KW_CSV_ROWS : KW_OK;
    }
    if (n_rows_total) *n_rows_total = added;
    return KW_OK;
}

static int run_exclude(kw_dedup *h, int64_t n_exclude, bool unique, void *stream)
{
    if (!h) return KW_EINVAL;
    KWCHK(h, hipSetDevice(h->device));
    kw_cdx_store *s = nullptr;
    int rc = store_get(h, &s);
    if (rc) return rc;
    if (n_exclude < 0 || n_exclude > s->n) { h->err = "kw_cdx_run_exclude: n_exclude outside the store"; return KW_EINVAL; }
    rc = scratch_fit(h, (void **)&s->code, &s->code_cap, (size_t)s->n + 64);
    if (rc) return rc;
    s->csv_ready = false;
    s->run_serial = 0;   // (the kept-rows buffers will hold the remaining rows: nothing for kw_cdx_csv_* to render)
    s->sel_ready = false;
    s->sel_serial = 0;
    h->no_compact = true;   // (the run's own kept rows would be thrown away: the pass compacts the link rows)
    rc = kw_dedup_run(h, s->arena, s->off, s->n, 0, s->code, stream);
    h->no_compact = false;
    if (rc) return rc;
    rc = kw_dedup_exclude_pass(h, s->arena, n_exclude, s->code, unique, (hipStream_t)stream);
    if (rc) return rc;
    s->sel_serial = h->run_serial;
    return KW_OK;
}

extern "C" int kw_cdx_run_exclude(kw_dedup *h, int64_t n_exclude, void *stream)
{
    return run_exclude(h, n_exclude, false, stream);
}

extern "C" int kw_cdx_run_exclude_unique(kw_dedup *h, int64_t n_exclude, void *stream)
{
    return run_exclude(h, n_exclude, true, stream);
}

extern "C" int kw_cdx_exclude_distinct_seen(kw_dedup *h, int64_t *n_distinct_seen, int64_t *n_exclude_kept, void *stream)
{
    if (!h || !n_distinct_seen || !n_exclude_kept) return KW_EINVAL;
    kw_cdx_store *s = h->cdx;
    if (!s || h->ex_serial == 0 || h->ex_serial != h->run_serial || s->sel_serial != h->run_serial) {
        h->err = "kw_cdx_exclude_distinct_seen: the last run was not kw_cdx_run_exclude";
        return KW_ESTATE;
    }
    KWCHK(h, hipSetDevice(h->device));
    int64_t out[2] = {0, 0};
    const int rc = kw_dedup_distinct_seen(h, s->arena, s->n - h->ex_links, s->code, out, (hipStream_t)stream);
    if (rc) return rc;
    *n_distinct_seen = out[0];
    *n_exclude_kept = out[1];
    return KW_OK;
}

extern "C" int kw_cdx_exclude_codes(kw_dedup *h, uint8_t *d_code, void *stream)
{
    if (!h) return KW_EINVAL;
    kw_cdx_store *s = h->cdx;
    if (!s || h->ex_serial == 0 || h->ex_serial != h->run_serial) {
        h->err = "kw_cdx_exclude_codes: the last run was not kw_cdx_run_exclude";
        return KW_ESTATE;
    }
    KWCHK(h, hipSetDevice(h->device));
    if (h->ex_links > 0) {
        if (!d_code) { h->err = "kw_cdx_exclude_codes: bad arguments"; return KW_EINVAL; }
        KWCHK(h, hipMemcpyAsync(d_code, s->code + (s->n - h->ex_links), (size_t)h->ex_links, hipMemcpyDeviceToDevice,
                                (hipStream_t)stream));
    }
    return KW_OK;
}

extern "C" int kw_cdx_rows(kw_dedup *h, int64_t *n_rows, int64_t *n_bytes)
{
    if (!h || !n_rows || !n_bytes) return KW_EINVAL;
    *n_rows = h->cdx ? h->cdx->n : 0;
    *n_bytes = h->cdx ? h->cdx->n_bytes : 0;
    return KW_OK;
}

extern "C" int kw_cdx_store_copy(kw_dedup *h, uint8_t *d_arena, int64_t *d_off, int64_t *d_ts, void *stream)
{
    if (!h) return KW_EINVAL;
    KWCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    kw_cdx_store *s = h->cdx;
    if (!s || s->n == 0) {
        if (d_off) KWCHK(h, hipMemsetAsync(d_off, 0, 8, st));
        return KW_OK;
    }
    if (d_arena && s->n_bytes) KWCHK(h, hipMemcpyAsync(d_arena, s->arena, (size_t)s->n_bytes, hipMemcpyDeviceToDevice, st));
    if (d_off) KWCHK(h, hipMemcpyAsync(d_off, s->off, 8 * ((size_t)s->n + 1), hipMemcpyDeviceToDevice, st));
    if (d_ts) KWCHK(h, hipMemcpyAsync(d_ts, s->ts, 8 * (size_t)s->n, hipMemcpyDeviceToDevice, st));
    return KW_OK;
}

extern "C" int kw_cdx_run(kw_dedup *h, int32_t flags, void *stream)
{
    if (!h) return KW_EINVAL;
    KWCHK(h, hipSetDevice(h->device));
    kw_cdx_store *s = nullptr;
    int rc = store_get(h, &s);
    if (rc) return rc;
    rc = scratch_fit(h, (void **)&s->code, &s->code_cap, (size_t)s->n + 64);
    if (rc) return rc;
    s->csv_ready = false;
    s->run_serial = 0;
    s->sel_ready = false;
    s->sel_serial = 0;
    rc = kw_dedup_run(h, s->arena, s->off, s->n, flags, s->code, stream);
    if (rc) return rc;
    s->run_serial = h->run_serial;
    s->sel_serial = h->run_serial;
    return KW_OK;
}

extern "C" int kw_cdx_csv_size(kw_dedup *h, int64_t *n_bytes, void *stream)
{
    if (!h || !n_bytes) return KW_EINVAL;
    kw_cdx_store *s = h->cdx;
    if (!s || s->run_serial == 0 || s->run_serial != h->run_serial) {
        h->err = "kw_cdx_csv_size: the last run was not kw_cdx_run over this store";
        return KW_ESTATE;
    }
    KWCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    s->csv_kept = h->n_kept;
    s->ms[2] = 0.f;
    if (h->n_kept == 0) {
        s->csv_bytes = HEADER_LEN;
    } else {
        const size_t nk = (size_t)h->n_kept;
        int rc = scratch_fit(h, &s->d_csv, &s->csv_scratch, align256(8 * (nk + 2)) + align256(nk) + align256(8 * SCAN_CHUNKS) + 256);
        if (rc) return rc;
        unsigned long long *seg = (unsigned long long *)s->d_csv;
        uint8_t *quoted = (uint8_t *)s->d_csv + align256(8 * (nk + 2));
        unsigned long long *chunk = (unsigned long long *)(quoted + align256(nk));
        unsigned long long *grand = chunk + align256(8 * SCAN_CHUNKS) / 8;
        KWCHK(h, hipEventRecord(s->ev[3], st));
        hipLaunchKernelGGL(cx_linelen_kernel, dim3(cus_grid(h, h->n_kept)), dim3(BLOCK), 0, st, h->n_kept,
                           (const int64_t *)s->ts, (const int64_t *)h->kept_row, (const int64_t *)h->kept_off,
                           (const uint8_t *)h->kept_bytes, seg, quoted);
        scan_launch(seg, h->n_kept + 1, chunk, grand, st);
        KWCHK(h, hipGetLastError());
        KWCHK(h, hipMemcpyAsync(seg + nk + 1, grand, 8, hipMemcpyDeviceToDevice, st));
        unsigned long long tot = 0;
        KWCHK(h, hipMemcpyAsync(&tot, grand, 8, hipMemcpyDeviceToHost, st));
        KWCHK(h, hipEventRecord(s->ev[4], st));
        KWCHK(h, hipStreamSynchronize(st));
        KWCHK(h, hipEventElapsedTime(&s->ms[2], s->ev[3], s->ev[4]));
        s->csv_bytes = (int64_t)tot;
    }
    s->csv_ready = true;
    *n_bytes = s->csv_bytes;
    return KW_OK;
}

extern "C" int kw_cdx_csv_copy(kw_dedup *h, uint8_t *d_out, void *stream)
{
    if (!h) return KW_EINVAL;
    kw_cdx_store *s = h->cdx;
    if (!s || !s->csv_ready || s->run_serial != h->run_serial) {
        h->err = "kw_cdx_csv_copy: no kw_cdx_csv_size since the last kw_cdx_run";
        return KW_ESTATE;
    }
    if (!d_out || ((uintptr_t)d_out & 15) != 0) { h->err = "kw_cdx_csv_copy: d_out must be 16-byte aligned"; return KW_EINVAL; }
    KWCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if (s->csv_kept == 0) {
        KWCHK(h, hipMemcpyAsync(d_out, HEADER_HOST, HEADER_LEN, hipMemcpyHostToDevice, st));
        KWCHK(h, hipStreamSynchronize(st));
        return KW_OK;
    }
    const size_t nk = (size_t)s->csv_kept;
    const uint8_t *quoted = (const uint8_t *)s->d_csv + align256(8 * (nk + 2));
    KWCHK(h, hipEventRecord(s->ev[3], st));
    hipLaunchKernelGGL(cx_fill_kernel<CsvGen>, dim3(cus_grid(h, (s->csv_bytes + 31) / 16)), dim3(BLOCK), 0, st, d_out,
                       (const int64_t *)s->d_csv, s->csv_kept + 1,
                       CsvGen{(const int64_t *)s->ts, (const int64_t *)h->kept_row, (const int64_t *)h->kept_off,
                              (const uint8_t *)h->kept_bytes, quoted});
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipEventRecord(s->ev[4], st));
    KWCHK(h, hipStreamSynchronize(st));
    float w = 0.f;
    KWCHK(h, hipEventElapsedTime(&w, s->ev[3], s->ev[4]));
    s->ms[2] += w;
    return KW_OK;
}

extern "C" int kw_cdx_last_ms(kw_dedup *h, float *ms, int32_t k)
{
    if (!h || !ms || k < 0) return KW_EINVAL;
    for (int i = 0; i < k && i < 3; ++i) ms[i] = h->cdx ? h->cdx->ms[i] : 0.f;
    return KW_OK;
}

// ---- the surviving rows in a given order, into several files (kw_cdx_selected_ts, kw_cdx_csv_select_*)

// the last run over this store and the store row of surviving row 0's row index: kw_cdx_run's kept rows carry store
// rows, the exclude runs' remaining rows carry indices among the link rows
static int select_state(kw_dedup *h, const char *who, kw_cdx_store **out, int64_t *row_base)
{
    kw_cdx_store *s = h->cdx;
    if (!s || s->sel_serial == 0 || s->sel_serial != h->run_serial) {
        h->err = std::string(who) + ": no kw_cdx_run, kw_cdx_run_exclude or kw_cdx_run_exclude_unique over this store";
        return KW_ESTATE;
    }
    *out = s;
    *row_base = (h->ex_serial != 0 && h->ex_serial == h->run_serial) ? s->n - h->ex_links : 0;
    return KW_OK;
}

extern "C" int kw_cdx_selected_ts(kw_dedup *h, int64_t *d_ts, void *stream)
{
    if (!h) return KW_EINVAL;
    kw_cdx_store *s = nullptr;
    int64_t base = 0;
    if (int rc = select_state(h, "kw_cdx_selected_ts", &s, &base)) return rc;
    if (h->n_kept == 0) return KW_OK;
    if (!d_ts) { h->err = "kw_cdx_selected_ts: bad arguments"; return KW_EINVAL; }
    KWCHK(h, hipSetDevice(h->device));
    hipLaunchKernelGGL(cx_sel_ts_kernel, dim3(cus_grid(h, h->n_kept)), dim3(BLOCK), 0, (hipStream_t)stream, h->n_kept,
                       (const int64_t *)s->ts, base, (const int64_t *)h->kept_row, d_ts);
    KWCHK(h, hipGetLastError());
    return KW_OK;
}

// d_sel: off (m + 1 words), src (m words), the scan's chunks and grand total, the error words
static void select_carve(kw_cdx_store *s, size_t m, unsigned long long **off, int64_t **src, unsigned long long **chunk,
                         unsigned long long **grand, SelErrs **errs)
{
    uint8_t *p = (uint8_t *)s->d_sel;
    *off = (unsigned long long *)p;
    p += align256(8 * (m + 1));
    *src = (int64_t *)p;
    p += align256(8 * m);
    *chunk = (unsigned long long *)p;
    p += align256(8 * SCAN_CHUNKS);
    *grand = (unsigned long long *)p;
    *errs = (SelErrs *)(p + 64);
}

extern "C" int kw_cdx_csv_select_size(kw_dedup *h, const int64_t *d_order, int64_t n_order, const int64_t *d_seg,
                                      int64_t n_seg, int64_t *d_seg_bytes, int64_t *n_bytes, void *stream)
{
    if (!h) return KW_EINVAL;
    kw_cdx_store *s = nullptr;
    int64_t base = 0;
    if (int rc = select_state(h, "kw_cdx_csv_select_size", &s, &base)) return rc;
    s->sel_ready = false;
    if (!n_bytes || n_order < 0 || n_seg < 0 || (n_order > 0 && (!d_order || n_seg == 0)) ||
        (n_seg > 0 && (!d_seg || !d_seg_bytes))) {
        h->err = "kw_cdx_csv_select_size: bad arguments";
        return KW_EINVAL;
    }
    KWCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    s->sel_ms[0] = s->sel_ms[1] = 0.f;
    const int64_t m = n_order + n_seg;
    s->sel_lines = m;
    s->sel_bytes = 0;
    if (m > 0) {
        int rc = scratch_fit(h, &s->d_sel, &s->sel_scratch,
                             align256(8 * ((size_t)m + 1)) + align256(8 * (size_t)m) + align256(8 * SCAN_CHUNKS) + 256);
        if (rc) return rc;
        unsigned long long *off, *chunk, *grand;
        int64_t *src;
        SelErrs *errs;
        select_carve(s, (size_t)m, &off, &src, &chunk, &grand, &errs);
        KWCHK(h, hipEventRecord(s->ev[3], st));
        KWCHK(h, hipMemsetAsync(errs, 0xFF, sizeof(SelErrs), st));
        hipLaunchKernelGGL(cx_sel_seg_kernel, dim3(cus_grid(h, n_seg + 1)), dim3(BLOCK), 0, st, d_seg, n_seg, n_order, off,
                           src, errs);
        if (n_order > 0)
            hipLaunchKernelGGL(cx_sel_len_kernel, dim3(cus_grid(h, n_order)), dim3(BLOCK), 0, st, d_order, n_order, d_seg,
                               n_seg, h->n_kept, (const int64_t *)s->ts, base, (const int64_t *)h->kept_row,
                               (const int64_t *)h->kept_off, (const uint8_t *)h->kept_bytes, off, src, errs);
        KWCHK(h, hipGetLastError());
        SelErrs e;
        KWCHK(h, hipMemcpyAsync(&e, errs, sizeof(e), hipMemcpyDeviceToHost, st));
        KWCHK(h, hipStreamSynchronize(st));
        if (e.seg != NONE) {
            h->err = "kw_cdx_csv_select_size: d_seg[" + std::to_string(e.seg) + "] is not an ascending bound from 0 to n_order";
            return KW_EINVAL;
        }
        if (e.order != NONE) {
            int64_t v = 0;
            KWCHK(h, hipMemcpy(&v, d_order + e.order, 8, hipMemcpyDeviceToHost));
            h->err = "kw_cdx_csv_select_size: d_order[" + std::to_string(e.order) + "] = " + std::to_string(v) +
                     " is outside the " + std::to_string(h->n_kept) + " surviving rows";
            return KW_EINVAL;
        }
        scan_launch(off, m, chunk, grand, st);
        KWCHK(h, hipGetLastError());
        KWCHK(h, hipMemcpyAsync(off + m, grand, 8, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(cx_sel_bytes_kernel, dim3(cus_grid(h, n_seg)), dim3(BLOCK), 0, st, d_seg, n_seg,
                           (const int64_t *)off, d_seg_bytes);
        KWCHK(h, hipGetLastError());
        unsigned long long tot = 0;
        KWCHK(h, hipMemcpyAsync(&tot, grand, 8, hipMemcpyDeviceToHost, st));
        KWCHK(h, hipEventRecord(s->ev[4], st));
        KWCHK(h, hipStreamSynchronize(st));
        KWCHK(h, hipEventElapsedTime(&s->sel_ms[0], s->ev[3], s->ev[4]));
        s->sel_bytes = (int64_t)tot;
    }
    s->sel_ready = true;
    *n_bytes = s->sel_bytes;
    return KW_OK;
}

extern "C" int kw_cdx_csv_select_copy(kw_dedup *h, uint8_t *d_out, void *stream)
{
    if (!h) return KW_EINVAL;
    kw_cdx_store *s = nullptr;
    int64_t base = 0;
    if (int rc = select_state(h, "kw_cdx_csv_select_copy", &s, &base)) return rc;
    if (!s->sel_ready) { h->err = "kw_cdx_csv_select_copy: no kw_cdx_csv_select_size since the last run"; return KW_ESTATE; }
    if (s->sel_bytes == 0) return KW_OK;
    if (!d_out || ((uintptr_t)d_out & 15) != 0) { h->err = "kw_cdx_csv_select_copy: d_out must be 16-byte aligned"; return KW_EINVAL; }
    KWCHK(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *off, *chunk, *grand;
    int64_t *src;
    SelErrs *errs;
    select_carve(s, (size_t)s->sel_lines, &off, &src, &chunk, &grand, &errs);
    KWCHK(h, hipEventRecord(s->ev[3], st));
    hipLaunchKernelGGL(cx_fill_kernel<SelGen>, dim3(cus_grid(h, (s->sel_bytes + 31) / 16)), dim3(BLOCK), 0, st, d_out,
                       (const int64_t *)off, s->sel_lines,
                       SelGen{(const int64_t *)s->ts, (const int64_t *)h->kept_row, (const int64_t *)h->kept_off,
                              (const uint8_t *)h->kept_bytes, (const int64_t *)src, base});
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipEventRecord(s->ev[4], st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipEventElapsedTime(&s->sel_ms[1], s->ev[3], s->ev[4]));
    return KW_OK;
}

extern "C" int kw_cdx_select_last_ms(kw_dedup *h, float *ms, int32_t k)
{
    if (!h || !ms || k < 0) return KW_EINVAL;
    for (int i = 0; i < k && i < 2; ++i) ms[i] = h->cdx ? h->cdx->sel_ms[i] : 0.f;
    return KW_OK;
}
