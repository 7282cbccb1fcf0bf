// libkwmatch: the article ingest on the device (include/kwingest.h) -- raw article-CSV bytes in device memory
// become the tokenized cells (kwcsv_parse's layout), the matcher's arena (kwcsv_pack's) and the date arrays
// (kwcsv_dates_iso's) of csrc/kwcsv.c, wherever the take rule of kwingest.h holds.
//
//   ig_quotes_kernel   a tile's '"' bytes counted (their exclusive scan over the tiles carries the quote parity
//                      into every tile); the first NUL; UTF-8 validated by the lanes that hold a byte >= 0x80.
//   ig_tile_kernel<0>  the tile's masks with the carried parity (a lane's in-quote mask is the prefix xor of its
//                      '"' mask on the parity before it): per tile the record ends, the delimiters and the kept
//                      bytes; the quote discipline and the '\r' rule.
//   ig_tile_kernel<1>  after the scans: every cell's end offset (a delimiter's or a record end's rank is its cell,
//                      the kept bytes before it its offset), the field count of every taken record from the two
//                      ranks at its end, blank records, `consumed`, a cell's QUOTED / needs-quotes bits (one
//                      atomicOr a wave where the wave lies in one cell), and the kept bytes through LDS into
//                      16-byte stores.
//   ig_finish_kernel   one thread: n_rows, consumed, the verdict in rule order.  The kernels after it return at
//                      once unless the verdict is OK (the offsets of a refused text are not all written).
//   ig_flags_kernel    lane = cell: CANON, the NA compare, the text witness, the columns' witnesses.
//   ig_rows_kernel     lane = row: the date cell by the ISO rule, the two arena segment lengths.
//   ig_stamps_kernel   lane = row, once a zone table is set (kw_ingest_zone): time_unix from the date arrays by the
//                      rule of kwstamps.h, the table staged in LDS.
//   ig_gather_kernel   lane = 16 arena bytes: the segment by binary search in the scanned offsets.
//   ig_spans_kernel    on request (kw_ingest_spans), after an OK parse: the tile masks once more, for every taken
//                      record's first byte and the byte after its last.
// One host synchronisation a parse; every buffer is sized from n_bytes and max_rows before the first launch.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/kwingest.h"
#define KWST_FN __device__ __forceinline__ static
#include "../../include/kwstamps.h"
#include "kwdev.hpp"
#include "kwhandle.hpp"

namespace ig {

using namespace kwd;   // BLOCK, TILE, NONE and the primitives
using namespace kwh;
typedef unsigned long long u64;
constexpr int MAX_GRID = 2048;
constexpr uint32_t F_QUOTED = 1u, F_NA = 2u, F_TEXT = 4u, F_CANON = 8u;   // KWCSV_* (csrc/kwcsv.c)
constexpr uint32_t W_QUOTED = 1u, W_NEEDQ = 2u;                           // the tile pass's bits of a cell
constexpr int ARENA_PAD = 64;
constexpr int MAX_NA = 64, MAX_NA_LEN = 16;

struct Errs {
    u64 nul, utf8, quote, cr, blank, fields;   // position of the first offender (NONE)
};

// the parse's state on the device; copied to the host once, at the end
struct Dev {
    Errs errs;
    u64 tot_q, tot_e, tot_d, tot_k;            // '"' bytes, records, delimiters, kept bytes of the whole text
    u64 mark;                                  // the position after the last taken record's '\n'
    long long n_rows, consumed, cell_bytes, arena_bytes, col_bytes, bad_pos;
    int verdict, witness[6], pad;
};

struct Args {
    const uint8_t *text;
    long long n, ntiles, max_rows, cells_cap;
    int final_, ncols;
    u64 *tq, *te, *td, *tk;                    // per tile, scanned
    Dev *D;
    long long *coff;
    uint32_t *cflw;
    uint8_t *cells;
};

__global__ __launch_bounds__(BLOCK) void ig_quotes_kernel(const uint8_t *__restrict__ text, long long n, long long ntiles,
                                                          u64 *__restrict__ tq, Dev *__restrict__ D)
{
    // (the text is readable up to the next multiple of 16 past n: kw_ingest_parse's contract)
    quotes_tiles(text, n, ntiles, tq, &D->errs.nul, &D->errs.utf8);
}

// Block b: the exclusive scan of a[b][0, m) in place (m from *m_dev when given), its total to total[b].  With
// `verdict` given, a refused text's scan writes a total of 0 and reads nothing (its values were not written).
struct ScanArgs {
    u64 *a[3];
    u64 *total[3];
    long long m;
    const long long *m_dev;
    int m_mul, m_add;          // m = *m_dev * m_mul + m_add
    const int *verdict;
};

__global__ __launch_bounds__(BLOCK) void ig_scan_kernel(ScanArgs S)
{
    __shared__ u64 ws[BLOCK / 64];
    u64 *__restrict__ a = S.a[blockIdx.x];
    if (S.verdict && *S.verdict != KW_INGEST_OK) {   // (block-uniform)
        if (threadIdx.x == 0) *S.total[blockIdx.x] = 0;
        return;
    }
    const long long m = S.m_dev ? *S.m_dev * S.m_mul + S.m_add : S.m;
    u64 carry = 0;
    for (long long i0 = 0; i0 < m; i0 += BLOCK) {   // (block-uniform trip count)
        const long long i = i0 + threadIdx.x;
        const u64 x = i < m ? a[i] : 0ull;
        u64 total;
        const u64 before = block_scan(x, ws, &total);
        if (i < m) a[i] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) *S.total[blockIdx.x] = carry;
}

// the masks of a lane's 16 bytes (bit k = byte p + k)
struct Lane {
    uint32_t valid, q, cm, nl, cr;
    uint32_t sb;            // the byte lies inside quotes (the parity of the '"' before it)
    uint32_t E, DL, K;      // a record end that is not zero-length; a delimiter; a kept byte
    uint32_t open, need;    // an opening quote; a kept ',', '"' or '\n'
    uint32_t bad_q, bad_c;
    uint32_t vE;            // the final text's end ends a record after this lane's last byte
};

__device__ __forceinline__ Lane lane_masks(const uint8_t *__restrict__ text, long long n, long long p, int final_,
                                           uint4 v, uint32_t inpar)
{
    Lane L;
    // the bytes around the lane's 16: the text is preceded by (virtual) line ends, 0x100 stands for its end
    uint32_t prev1 = 0x0Au, prev2 = 0x0Au, next = 0x100u;
    L.valid = n - p >= 16 ? 0xFFFFu : (1u << (int)(n - p)) - 1u;
    L.q = mask16(v, 0x22u) & L.valid;
    L.cm = mask16(v, 0x2Cu) & L.valid;
    L.nl = mask16(v, 0x0Au) & L.valid;
    L.cr = mask16(v, 0x0Du) & L.valid;
    if (p > 0) prev1 = text[p - 1];
    if (p > 1) prev2 = text[p - 2];
    if (p + 16 < n) next = text[p + 16];
    uint32_t incl = L.q;   // bit k: the parity of the '"' bytes in bits 0..k
    incl ^= incl << 1;
    incl ^= incl << 2;
    incl ^= incl << 4;
    incl ^= incl << 8;
    L.sb = ((incl << 1) ^ (inpar ? 0xFFFFu : 0u)) & L.valid;
    const uint32_t q = L.q, cm = L.cm, nl = L.nl, cr = L.cr, sb = L.sb;
    const uint32_t pnl = ((nl << 1) | (prev1 == 0x0Au ? 1u : 0u)) & 0xFFFFu;   // the byte before is '\n'
    const uint32_t pcr = ((cr << 1) | (prev1 == 0x0Du ? 1u : 0u)) & 0xFFFFu;
    const uint32_t pn2 = ((nl << 2) | (prev1 == 0x0Au ? 2u : 0u) | (prev2 == 0x0Au ? 1u : 0u)) & 0xFFFFu;
    const uint32_t pcm = ((cm << 1) | (prev1 == 0x2Cu ? 1u : 0u)) & 0xFFFFu;
    const uint32_t pq = ((q << 1) | (prev1 == 0x22u ? 1u : 0u)) & 0xFFFFu;
    const uint32_t top = 0x8000u;
    const uint32_t ncm = (cm >> 1) | (next == 0x2Cu ? top : 0u), nnl = (nl >> 1) | (next == 0x0Au ? top : 0u);
    const uint32_t ncr = (cr >> 1) | (next == 0x0Du ? top : 0u), nq = (q >> 1) | (next == 0x22u ? top : 0u);
    const uint32_t eot = n - p <= 16 ? 1u << (int)(n - p - 1) : 0u;   // the text's last byte
    L.E = nl & ~sb & ~(pnl | (pcr & pn2));
    L.DL = cm & ~sb;
    const uint32_t pair2 = q & ~sb & pq;           // the second '"' of a pair: kept
    L.open = q & ~sb & ~pq;
    L.K = L.valid & ~(L.DL | (nl & ~sb) | (cr & ~sb) | (q & ~pair2));
    L.need = (cm & sb) | (nl & sb) | pair2;
    L.bad_q = ((q & ~sb) & ~(pcm | pnl | pq)) | ((q & sb) & ~(ncm | nnl | ncr | nq | eot));
    L.bad_c = cr & ~sb & ~nnl & ~(final_ ? 0u : eot);
    L.vE = 0;
    if (final_ && eot) {
        const uint32_t after = ((sb ^ q) & eot) ? 1u : 0u;   // the text ends inside quotes
        if (!after && !(nl & ~sb & eot)) L.vE = 1;
    }
    return L;
}

// a record ending at byte `end` (its '\n', or the text's length) is spaces and tabs only: its first byte (NONE)
__device__ u64 blank_record(const uint8_t *__restrict__ text, long long end)
{
    long long j = end - 1;
    if (j >= 0 && text[j] == 0x0Du) --j;
    if (j < 0 || (text[j] != 0x20u && text[j] != 0x09u)) return NONE;
    while (j >= 0 && (text[j] == 0x20u || text[j] == 0x09u)) --j;
    if (j < 0 || text[j] == 0x0Au) return (u64)(j + 1);
    return NONE;
}

template <int MODE>
__global__ __launch_bounds__(BLOCK) void ig_tile_kernel(Args A)
{
    __shared__ u64 ws[BLOCK / 64];
    __shared__ uint4 lbuf[TILE / 16 + 1];
    uint8_t *lbytes = (uint8_t *)lbuf;
    const uint8_t *__restrict__ text = A.text;
    const long long n = A.n;
    const int lane = threadIdx.x & 63;
    long long n_take = 0;
    if (MODE == 1) {
        const u64 found = A.D->tot_e;
        n_take = found < (u64)A.max_rows ? (long long)found : A.max_rows;
    }
    for (long long tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        const long long p = tile * TILE + (long long)threadIdx.x * 16;
        const bool in = p < n;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (in) v = *(const uint4 *)(text + p);
        const uint32_t qraw = in ? mask16(v, 0x22u) & (n - p >= 16 ? 0xFFFFu : (1u << (int)(n - p)) - 1u) : 0u;
        u64 total;
        const u64 qb = block_scan((u64)__popc(qraw), ws, &total);
        Lane L{};
        if (in) L = lane_masks(text, n, p, A.final_, v, (uint32_t)((A.tq[tile] + qb) & 1ull));
        const u64 packed = (u64)(__popc(L.E) + L.vE) | ((u64)__popc(L.DL) << 20) | ((u64)__popc(L.K) << 40);
        const u64 before = block_scan(packed, ws, &total);
        if (MODE == 0) {
            u64 eq = NONE, ec = NONE;
            if (L.bad_q) eq = (u64)p + __builtin_ctz(L.bad_q);
            if (L.bad_c) ec = (u64)p + __builtin_ctz(L.bad_c);
            if (__any((eq & ec) != NONE)) {
                eq = wave_min(eq);
                ec = wave_min(ec);
                if (lane == 0) {
                    if (eq != NONE) atomicMin(&A.D->errs.quote, eq);
                    if (ec != NONE) atomicMin(&A.D->errs.cr, ec);
                }
            }
            if (threadIdx.x == 0) {
                A.te[tile] = total & 0xFFFFFull;
                A.td[tile] = (total >> 20) & 0xFFFFFull;
                A.tk[tile] = total >> 40;
            }
            continue;
        }
        const long long ce = (long long)(A.te[tile] + (before & 0xFFFFFull));          // records ended before the lane
        const long long cd = (long long)(A.td[tile] + ((before >> 20) & 0xFFFFFull));   // delimiters before it
        const u64 kbase = A.tk[tile];
        const uint32_t kin = (uint32_t)(before >> 40);                                  // kept bytes before it, in the tile
        const long long c0 = ce + cd;                                                   // the cell of the lane's first byte
        const uint32_t ends = L.E | L.DL;
        // every cell end: its offset; every taken record's end: its field count, blank records, `consumed`
        {
            uint32_t todo = ends;
            while (todo || L.vE) {
                int k;
                uint32_t below;
                bool is_end;
                if (todo) {
                    k = __builtin_ctz(todo);
                    todo &= todo - 1u;
                    below = (1u << k) - 1u;
                    is_end = (L.E >> k) & 1u;
                } else {
                    k = 16;
                    below = 0xFFFFu;
                    is_end = true;
                    L.vE = 0;
                }
                const long long cell = c0 + __popc(ends & below);
                if (cell < A.cells_cap) A.coff[cell + 1] = (long long)(kbase + kin + __popc(L.K & below));
                if (is_end) {
                    const long long r = ce + __popc(L.E & below);
                    if (r < n_take) {
                        const long long d = cd + __popc(L.DL & below);
                        const long long at = k == 16 ? n : p + k;
                        if (d != (r + 1) * (long long)(A.ncols - 1)) atomicMin(&A.D->errs.fields, (u64)at);
                        const u64 bl = blank_record(text, at);
                        if (bl != NONE) atomicMin(&A.D->errs.blank, bl);
                        if (r == n_take - 1) A.D->mark = (u64)(k == 16 ? n : p + k + 1);
                    }
                }
            }
        }
        // a cell's QUOTED / needs-quotes bits
        {
            const uint32_t m0 = ends ? (1u << __builtin_ctz(ends)) - 1u : 0xFFFFu;
            const uint32_t bits0 = ((L.open & m0) ? W_QUOTED : 0u) | ((L.need & m0) ? W_NEEDQ : 0u);
            const bool ev = bits0 != 0 && c0 < A.cells_cap;
            const u64 em = __ballot(ev);
            if (em) {   // (wave-uniform)
                const int lead = __ffsll((long long)em) - 1;
                const long long cl = __shfl(c0, lead, 64);
                if (__all(!ev || c0 == cl)) {
                    uint32_t b = ev ? bits0 : 0u;
                    for (int d = 32; d >= 1; d >>= 1) b |= __shfl_xor(b, d, 64);
                    if (lane == lead) atomicOr(&A.cflw[cl], b);
                } else if (ev) {
                    atomicOr(&A.cflw[c0], bits0);
                }
            }
            uint32_t todo = ends;
            while (todo) {   // the cells that start inside the lane
                const int k = __builtin_ctz(todo);
                todo &= todo - 1u;
                const uint32_t seg = ~((2u << k) - 1u) & (todo ? (1u << __builtin_ctz(todo)) - 1u : 0xFFFFu);
                const uint32_t b = ((L.open & seg) ? W_QUOTED : 0u) | ((L.need & seg) ? W_NEEDQ : 0u);
                const long long cell = c0 + __popc(ends & ((2u << k) - 1u));
                if (b && cell < A.cells_cap) atomicOr(&A.cflw[cell], b);
            }
        }
        // the kept bytes: compacted in LDS at the output's own 16-byte phase, then stored 16 bytes a lane
        const uint32_t sh = (uint32_t)(kbase & 15ull);
        {
            uint32_t o = sh + kin;
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            if (L.K == 0xFFFFu) {
                #pragma unroll
                for (int k = 0; k < 16; ++k) lbytes[o + k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            } else {
                #pragma unroll
                for (int k = 0; k < 16; ++k)
                    if ((L.K >> k) & 1u) lbytes[o++] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
            }
        }
        __syncthreads();
        {
            const uint32_t span = sh + (uint32_t)(total >> 40);
            uint8_t *__restrict__ dst = A.cells + (kbase - sh);   // 16-byte aligned
            for (uint32_t c = threadIdx.x; c * 16 < span; c += BLOCK) {
                const uint32_t lo = c * 16 < sh ? sh : c * 16, hi = c * 16 + 16 < span ? c * 16 + 16 : span;
                if (hi - lo == 16) {
                    *(uint4 *)(dst + c * 16) = lbuf[c];
                } else {
                    for (uint32_t j = lo; j < hi; ++j) dst[j] = lbytes[j];
                }
            }
        }
        __syncthreads();   // lbuf free again
    }
}

__global__ void ig_finish_kernel(Dev *__restrict__ D, const long long *__restrict__ coff, long long n, int final_,
                                 long long max_rows, int ncols)
{
    if (threadIdx.x || blockIdx.x) return;
    const u64 found = D->tot_e;
    const bool fewer = found < (u64)max_rows;
    long long n_rows = fewer ? (long long)found : max_rows;
    const bool to_end = final_ && fewer;
    const long long consumed = to_end ? n : (n_rows ? (long long)D->mark : 0);
    const u64 limit = (u64)consumed;
    int verdict = KW_INGEST_OK;
    u64 pos = 0;
    u64 eq = D->errs.quote;
    if (eq >= limit) eq = NONE;
    if (eq == NONE && to_end && (D->tot_q & 1ull)) eq = (u64)n;   // the final text ends inside quotes
    if (D->errs.nul < limit) { verdict = KW_INGEST_NUL; pos = D->errs.nul; }
    else if (D->errs.utf8 < limit) { verdict = KW_INGEST_UTF8; pos = D->errs.utf8; }
    else if (eq != NONE) { verdict = KW_INGEST_QUOTE; pos = eq; }
    else if (D->errs.cr < limit) { verdict = KW_INGEST_CR; pos = D->errs.cr; }
    else if (D->errs.blank != NONE) { verdict = KW_INGEST_BLANK; pos = D->errs.blank; }
    else if (D->errs.fields != NONE) { verdict = KW_INGEST_FIELDS; pos = D->errs.fields; }
    else if (n_rows >= (1ll << 31) || n_rows * ncols >= (1ll << 31)) { verdict = KW_INGEST_ROWS; pos = 0; }
    D->verdict = verdict;
    D->bad_pos = (long long)pos;
    if (verdict != KW_INGEST_OK) n_rows = 0;
    D->n_rows = n_rows;
    D->consumed = verdict == KW_INGEST_OK ? consumed : 0;
    D->cell_bytes = n_rows ? coff[n_rows * ncols] : 0;
    D->arena_bytes = 0;
}

// Every taken record's byte span, as kwcsv_parse's rspan gives it.  A record with bytes starts at a byte outside
// quotes that follows a '\n' outside quotes (or the text's start) and is neither '\n' nor '\r' (outside quotes a
// '\r' is followed by '\n': the CR rule, so either begins a record of no bytes); the records that ended before it
// are its rank.  A record ends where ig_tile_kernel counts its end, before the '\r' of a "\r\n".  Runs on the
// scanned tile counts (tq, te) the parse left.
__global__ __launch_bounds__(BLOCK) void ig_spans_kernel(Args A, long long *__restrict__ rs, long long *__restrict__ re)
{
    __shared__ u64 ws[BLOCK / 64];
    if (A.D->verdict != KW_INGEST_OK) return;
    const uint8_t *__restrict__ text = A.text;
    const long long n = A.n, n_take = A.D->n_rows;
    for (long long tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        const long long p = tile * TILE + (long long)threadIdx.x * 16;
        const bool in = p < n;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (in) v = *(const uint4 *)(text + p);
        const uint32_t qraw = in ? mask16(v, 0x22u) & (n - p >= 16 ? 0xFFFFu : (1u << (int)(n - p)) - 1u) : 0u;
        u64 total;
        const u64 qb = block_scan((u64)__popc(qraw), ws, &total);
        Lane L{};
        if (in) L = lane_masks(text, n, p, A.final_, v, (uint32_t)((A.tq[tile] + qb) & 1ull));
        const u64 before = block_scan((u64)(__popc(L.E) + L.vE), ws, &total);
        if (!in) continue;   // (after the block's scans)
        const long long ce = (long long)(A.te[tile] + before);   // records ended before the lane
        const uint32_t pnl = ((L.nl << 1) | ((p == 0 || text[p - 1] == 0x0Au) ? 1u : 0u)) & 0xFFFFu;
        uint32_t todo = L.valid & ~L.sb & pnl & ~L.nl & ~L.cr;
        while (todo) {
            const int k = __builtin_ctz(todo);
            todo &= todo - 1u;
            const long long r = ce + __popc(L.E & ((1u << k) - 1u));
            if (r < n_take) rs[r] = p + k;
        }
        todo = L.E;
        while (todo || L.vE) {
            long long at, r;
            if (todo) {
                const int k = __builtin_ctz(todo);
                todo &= todo - 1u;
                at = p + k;
                r = ce + __popc(L.E & ((1u << k) - 1u));
            } else {
                at = n;
                r = ce + __popc(L.E);
                L.vE = 0;
            }
            if (r < n_take) re[r] = (at > 0 && text[at - 1] == 0x0Du) ? at - 1 : at;
        }
    }
}

// kwcsv_text_witness (csrc/kwcsv.c)
__device__ bool text_witness(const uint8_t *__restrict__ s, long long n)
{
    long long a = 0, b = n;
    while (a < b && (s[a] == ' ' || s[a] == '\t')) ++a;
    while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\t')) --b;
    if (a == b) return true;
    const uint8_t *t = s + a;
    const long long m = b - a;
    if (m <= 9) {   // the longest literal: a sign and "infinity"
        if (ieq(t, m, "true", 4) || ieq(t, m, "false", 5)) return false;
        const int sg = (t[0] == '+' || t[0] == '-') ? 1 : 0;
        if (ieq(t + sg, m - sg, "inf", 3) || ieq(t + sg, m - sg, "infinity", 8)) return false;
    }
    for (long long k = 0; k < m; ++k) {
        const uint8_t c = t[k];
        if (!((c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E')) return true;
    }
    return false;
}

struct Cols {
    int c[6];
};

__global__ __launch_bounds__(BLOCK) void ig_flags_kernel(Dev *__restrict__ D, const uint8_t *__restrict__ cells,
                                                         const long long *__restrict__ coff,
                                                         const uint32_t *__restrict__ cflw, uint8_t *__restrict__ cfl,
                                                         int ncols, Cols C, const uint8_t *__restrict__ na,
                                                         const int *__restrict__ na_off, int n_na)
{
    if (D->verdict != KW_INGEST_OK) return;
    const long long nc = D->n_rows * ncols;
    for (long long c = (long long)blockIdx.x * BLOCK + threadIdx.x; c < nc; c += (long long)gridDim.x * BLOCK) {
        const long long s = coff[c], len = coff[c + 1] - s;
        const uint8_t *__restrict__ t = cells + s;
        const uint32_t w = cflw[c];
        uint32_t fl = (w & W_QUOTED) ? F_QUOTED : 0u;
        if (((w & W_NEEDQ) != 0) == ((w & W_QUOTED) != 0)) fl |= F_CANON;
        bool isna = false;
        if (len <= MAX_NA_LEN) {
            for (int k = 0; k < n_na && !isna; ++k) {
                const int a = na_off[k], b = na_off[k + 1];
                if (b - a != (int)len) continue;
                bool same = true;
                for (int i = 0; i < (int)len && same; ++i) same = na[a + i] == t[i];
                isna = same;
            }
        }
        if (isna) {
            fl |= F_NA;
        } else if (text_witness(t, len)) {
            fl |= F_TEXT;
            const int col = (int)(c % ncols);
            for (int k = 0; k < 6; ++k)
                if (C.c[k] == col && D->witness[k] == 0) D->witness[k] = 1;
        }
        cfl[c] = (uint8_t)fl;
    }
}

__device__ __forceinline__ long long days_from_civil(long long y, long long m, long long d)
{
    y -= m <= 2;
    const long long era = (y >= 0 ? y : y - 399) / 400;
    const long long yoe = y - era * 400;
    const long long doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const long long doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + doe - 719468;
}

constexpr int DATE_MAX = 35;   // the longest native date cell: 19 + '.' + 9 digits + sign + HH ':' MM

// One date cell by the ISO rule of kwingest.h (kwcsv_dates_iso's answer).  The cell's bytes are read once, each
// under its own `i < len` (nothing past the cell's end), into registers; the calendar test reads the first 19,
// the tail machine the other 16 at most, a byte a step (kwcsv_dates_iso's states).
__device__ __forceinline__ void date_iso(const uint8_t *__restrict__ s, int len, long long &us, uint8_t &kind, int &off_s)
{
    us = 0;
    kind = 0;
    off_s = 0;
    if (len < 19 || len > DATE_MAX) return;
    int b[DATE_MAX];
#pragma unroll
    for (int i = 0; i < DATE_MAX; ++i) b[i] = i < len ? (int)s[i] : 0;
    bool ok = b[4] == '-' && b[7] == '-' && (b[10] == ' ' || b[10] == 'T') && b[13] == ':' && b[16] == ':';
#pragma unroll
    for (int i = 0; i < 19; ++i)
        if (i != 4 && i != 7 && i != 10 && i != 13 && i != 16) ok = ok && b[i] >= '0' && b[i] <= '9';
    if (!ok) return;
#define IG_D2(i) ((long long)(b[i] - '0') * 10 + (b[(i) + 1] - '0'))
    const long long y = IG_D2(0) * 100 + IG_D2(2), mo = IG_D2(5), d = IG_D2(8), hh = IG_D2(11), mi = IG_D2(14), ss = IG_D2(17);
#undef IG_D2
    if (y < 1000 || mo < 1 || mo > 12 || hh >= 24 || mi >= 60 || ss >= 60) return;
    const bool leap = (y % 4 == 0) && (y % 100 != 0 || y % 400 == 0);
    const long long md = mo == 2 ? (leap ? 29 : 28) : ((mo == 4 || mo == 6 || mo == 9 || mo == 11) ? 30 : 31);
    if (d < 1 || d > md) return;
    // st: 0 after the seconds; 1 after '.'; 2 in the fraction; 3 after the sign; 4 after H; 5 after HH; 6 after
    // HH':'; 7 after M; 8 done ('Z' or MM); 9 refused
    int st = 0, nf = 0, sign = 1, frac = 0, oh = 0, om = 0;
#pragma unroll
    for (int i = 19; i < DATE_MAX; ++i) {
        if (i < len) {
            const int ch = b[i], dg = ch - '0';
            const bool isd = ch >= '0' && ch <= '9';
            const int zone = ch == 'Z' ? 8 : (ch == '+' || ch == '-') ? 3 : 9;
            int nx = 9;
            if (st == 0) {
                nx = ch == '.' ? 1 : zone;
            } else if (st == 1 || st == 2) {
                if (isd) {
                    ++nf;
                    if (nf <= 6) frac = frac * 10 + dg;
                    nx = nf <= 9 ? 2 : 9;
                } else {
                    nx = st == 2 ? zone : 9;
                }
            } else if (st == 3) {
                oh = dg * 10;
                nx = isd ? 4 : 9;
            } else if (st == 4) {
                oh += dg;
                nx = isd ? 5 : 9;
            } else if (st == 5) {
                if (isd) om = dg * 10;
                nx = isd ? 7 : (ch == ':' ? 6 : 9);
            } else if (st == 6) {
                om = dg * 10;
                nx = isd ? 7 : 9;
            } else if (st == 7) {
                om += dg;
                nx = isd ? 8 : 9;
            }
            st = nx;
            if (st == 3) sign = ch == '-' ? -1 : 1;
        }
    }
    if (!(st == 0 || st == 2 || st == 5 || st == 8) || oh > 23 || om > 59) return;
    const bool aware = st == 5 || st == 8;
    const int off = aware ? sign * (oh * 3600 + om * 60) : 0;
    int f = frac;   // the first min(nf, 6) digits as microseconds
#pragma unroll
    for (int k = 1; k < 6; ++k)
        if (nf <= k) f *= 10;
    us = ((days_from_civil(y, mo, d) * 86400) + hh * 3600 + mi * 60 + ss - off) * 1000000 + f;
    off_s = off;
    kind = aware ? 3 : nf ? 4 : 1;
}

// lane = row: the date cell by the ISO rule (kwcsv_dates_iso); the lengths of the row's two arena segments
__global__ __launch_bounds__(BLOCK) void ig_rows_kernel(const Dev *__restrict__ D, const uint8_t *__restrict__ cells,
                                                        const long long *__restrict__ coff,
                                                        const uint8_t *__restrict__ cfl, int ncols, Cols C,
                                                        long long *__restrict__ us, uint8_t *__restrict__ kind,
                                                        int *__restrict__ off_s, u64 *__restrict__ aoff)
{
    if (D->verdict != KW_INGEST_OK) return;
    const long long nr = D->n_rows;
    if (blockIdx.x == 0 && threadIdx.x == 0) aoff[2 * nr] = 0;
    for (long long r = (long long)blockIdx.x * BLOCK + threadIdx.x; r < nr; r += (long long)gridDim.x * BLOCK) {
        for (int k = 0; k < 2; ++k) {
            const long long c = r * ncols + C.c[k];
            aoff[2 * r + k] = (cfl[c] & F_NA) ? 3ull : (u64)(coff[c + 1] - coff[c]);
        }
        const long long c = r * ncols + C.c[2];
        long long v = 0;
        uint8_t kd = 2;
        int off = 0;
        if (!(cfl[c] & F_NA)) {
            const long long lo = coff[c], len = coff[c + 1] - lo;
            date_iso(cells + lo, len > DATE_MAX ? DATE_MAX + 1 : (int)len, v, kd, off);
        }
        us[r] = v;
        kind[r] = kd;
        off_s[r] = off;
    }
}

// lane = row: time_unix of the row's date under the zone table zat[zn + 1] / zoff[zn] (kwstamps.h: the solve's up to
// four utcoff lookups are ten-step binary searches over the table's copy in LDS, staged once a block; 64-bit integer
// arithmetic only).  stamps[r] and native[r] for every taken row; a block without rows stages nothing.
__global__ __launch_bounds__(BLOCK) void ig_stamps_kernel(const Dev *__restrict__ D, const long long *__restrict__ us,
                                                          const uint8_t *__restrict__ kind,
                                                          const int64_t *__restrict__ zat, const int32_t *__restrict__ zoff,
                                                          int zn, int64_t *__restrict__ stamps, uint8_t *__restrict__ native)
{
    __shared__ int64_t s_at[KWST_CAPACITY];
    __shared__ int32_t s_off[KWST_CAPACITY];
    if (D->verdict != KW_INGEST_OK) return;
    const long long nr = D->n_rows;
    if ((long long)blockIdx.x * BLOCK >= nr) return;   // (the whole block)
    for (int k = threadIdx.x; k < zn; k += BLOCK) {
        s_at[k] = zat[k];
        s_off[k] = zoff[k];
    }
    __syncthreads();
    kwst_zone z;
    z.at = s_at;
    z.off = s_off;
    z.n = zn;
    z.lo = zat[0] + KWST_MARGIN;
    z.hi = zat[zn] - KWST_MARGIN;
    for (long long r = (long long)blockIdx.x * BLOCK + threadIdx.x; r < nr; r += (long long)gridDim.x * BLOCK) {
        int64_t v;
        const int nat = kwst_row(&z, (int64_t)us[r], (int)kind[r], &v);
        stamps[r] = v;
        native[r] = (uint8_t)nat;
    }
}

// lane = row: the length and the flags of column col's cell
__global__ __launch_bounds__(BLOCK) void ig_collen_kernel(const Dev *__restrict__ D, const long long *__restrict__ coff,
                                                          const uint8_t *__restrict__ cfl, int ncols, int col,
                                                          u64 *__restrict__ off, uint8_t *__restrict__ fl)
{
    const long long nr = D->n_rows;
    if (blockIdx.x == 0 && threadIdx.x == 0) off[nr] = 0;
    for (long long r = (long long)blockIdx.x * BLOCK + threadIdx.x; r < nr; r += (long long)gridDim.x * BLOCK) {
        const long long c = r * ncols + col;
        off[r] = (u64)(coff[c + 1] - coff[c]);
        fl[r] = cfl[c];
    }
}

// Segments laid end to end: lane = 16 output bytes of dst[0, total + pad) (the pad zero).  ARENA: segment s is
// row s / 2's article_text (s even) or title cell, an NA cell "nan"; else segment s is row s's cell of column col.
template <bool ARENA>
__global__ __launch_bounds__(BLOCK) void ig_gather_kernel(const Dev *__restrict__ D, const uint8_t *__restrict__ cells,
                                                          const long long *__restrict__ coff,
                                                          const uint8_t *__restrict__ cfl, int ncols, int ct, int ci,
                                                          const u64 *__restrict__ off, uint8_t *__restrict__ dst, int pad)
{
    if (D->verdict != KW_INGEST_OK) return;
    const long long nseg = ARENA ? 2 * D->n_rows : D->n_rows;
    const u64 total = off[nseg];
    const u64 span = total + (u64)pad;
    for (u64 i = (u64)blockIdx.x * BLOCK + threadIdx.x; i * 16 < span; i += (u64)gridDim.x * BLOCK) {
        const u64 x0 = i * 16;
        uint32_t w[4] = {0, 0, 0, 0};
        if (x0 < total) {
            long long lo = 0, hi = nseg;   // the last segment with off[s] <= x0
            while (hi - lo > 1) {
                const long long mid = (lo + hi) >> 1;
                if (off[mid] <= x0) lo = mid; else hi = mid;
            }
            long long s = lo - 1;
            u64 seg_end = 0, seg_lo = 0;
            const uint8_t *src = nullptr;
            for (int j = 0; j < 16; ++j) {
                const u64 x = x0 + j;
                if (x >= total) break;
                while (s < 0 || x >= seg_end) {
                    ++s;
                    seg_lo = off[s];
                    seg_end = off[s + 1];
                    const long long cell = ARENA ? (s >> 1) * ncols + ((s & 1) ? ci : ct) : s * ncols + ct;
                    src = (ARENA && (cfl[cell] & F_NA)) ? nullptr : cells + coff[cell];
                }
                const u64 k = x - seg_lo;
                const uint32_t b = src ? src[k] : (uint32_t)(k == 1 ? 'a' : 'n');
                w[j >> 2] |= b << (8 * (j & 3));
            }
        }
        *(uint4 *)(dst + x0) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace ig

struct kw_ingest {
    int device = 0;
    std::string err;
    int ncols = 0;
    ig::Cols cols{};
    uint8_t *d_na = nullptr;
    int *d_na_off = nullptr;
    int n_na = 0;
    ig::Dev *D = nullptr;          // device
    ig::Dev *H = nullptr;          // pinned host copy
    ig::Buf tiles, cells, coff, cflw, cfl, arena, aoff, us, kind, doff, col_buf, col_off, col_fl;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [4], [5]: around the stamps kernel
    float ms[5] = {0, 0, 0, 0, 0};
    bool have = false;             // an OK parse whose buffers stand
    ig::Buf zat, zoff, stamps, native;   // the zone table (kw_ingest_zone) and the rows' stamps under it
    int zn = 0;                    // the table's entries, 0: none
    bool have_stamps = false;      // the last OK parse computed stamps
    void *stage[2] = {nullptr, nullptr};   // pinned staging windows (kw_ingest_stage)
    size_t stage_cap[2] = {0, 0};
    ig::Buf text;                  // kw_ingest_upload's device copy of a window
    hipStream_t stream = nullptr;  // the last parse's
    const uint8_t *ptext = nullptr;   // the last parse's text, its bytes and its final flag (kw_ingest_spans)
    long long pn = 0;
    int pfinal = 0;
    ig::Buf spans;                 // the taken records' starts, then their ends
    bool have_spans = false;
};

namespace ig {

// a buffer of at least `bytes` (contents are not kept when it grows; it grows by half again at least)
static int fit(kw_ingest *h, Buf &b, size_t bytes) { return ensure(h, b, bytes, bytes + bytes / 2 + 256); }

// The cap on every launch grid of a call: MAX_GRID, or the tests' KW_TEST_INGEST_GRID in [1, MAX_GRID] (read per
// call: the kernels' loops then make several trips on a small text).
static int grid_cap() { return (int)env_int("KW_TEST_INGEST_GRID", 1, MAX_GRID, MAX_GRID); }

}  // namespace ig

using namespace ig;

extern "C" int kw_ingest_tile_bytes(void) { return TILE; }

extern "C" int kw_ingest_create(int32_t device, int32_t ncols, const int32_t *cols, const uint8_t *na,
                                const int32_t *na_off, int32_t n_na, kw_ingest **out)
{
    if (!out) return KW_EINVAL;
    *out = nullptr;
    if (!cols || !na_off || n_na < 0 || n_na > MAX_NA || ncols < 6 || ncols > 4096 || (n_na > 0 && !na)) return KW_EINVAL;
    for (int a = 0; a < 6; ++a) {
        if (cols[a] < 0 || cols[a] >= ncols) return KW_EINVAL;
        for (int b = 0; b < a; ++b)
            if (cols[a] == cols[b]) return KW_EINVAL;
    }
    if (na_off[0] != 0) return KW_EINVAL;
    for (int k = 0; k < n_na; ++k)
        if (na_off[k + 1] < na_off[k] || na_off[k + 1] - na_off[k] > MAX_NA_LEN) return KW_EINVAL;
    if (hipSetDevice(device) != hipSuccess) return KW_EHIP;
    kw_ingest *h = new kw_ingest();
    h->device = device;
    h->ncols = ncols;
    h->n_na = n_na;
    for (int a = 0; a < 6; ++a) h->cols.c[a] = cols[a];
    const size_t nab = (size_t)na_off[n_na];
    bool ok = hipMalloc((void **)&h->d_na, nab + 16) == hipSuccess &&
              hipMalloc((void **)&h->d_na_off, ((size_t)n_na + 1) * 4) == hipSuccess &&
              hipMalloc((void **)&h->D, sizeof(Dev)) == hipSuccess &&
              hipHostMalloc((void **)&h->H, sizeof(Dev), hipHostMallocDefault) == hipSuccess;
    if (ok && nab) ok = hipMemcpy(h->d_na, na, nab, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) ok = hipMemcpy(h->d_na_off, na_off, ((size_t)n_na + 1) * 4, hipMemcpyHostToDevice) == hipSuccess;
    for (auto &e : h->ev)
        if (ok) ok = hipEventCreate(&e) == hipSuccess;
    if (!ok) {
        kw_ingest_destroy(h);
        return KW_EHIP;
    }
    *out = h;
    return KW_OK;
}

extern "C" int kw_ingest_destroy(kw_ingest *h)
{
    if (!h) return KW_OK;
    (void)hipSetDevice(h->device);
    Buf *bufs[] = {&h->tiles, &h->cells, &h->coff, &h->cflw, &h->cfl, &h->arena, &h->aoff, &h->us, &h->kind, &h->doff,
                   &h->col_buf, &h->col_off, &h->col_fl, &h->spans, &h->zat, &h->zoff, &h->stamps, &h->native};
    for (Buf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    if (h->d_na) (void)hipFree(h->d_na);
    if (h->d_na_off) (void)hipFree(h->d_na_off);
    if (h->D) (void)hipFree(h->D);
    if (h->H) (void)hipHostFree(h->H);
    for (void *p : h->stage)
        if (p) (void)hipHostFree(p);
    if (h->text.p) (void)hipFree(h->text.p);
    for (auto &e : h->ev)
        if (e) (void)hipEventDestroy(e);
    delete h;
    return KW_OK;
}

extern "C" const char *kw_ingest_last_error(kw_ingest *h) { return h ? h->err.c_str() : "null handle"; }

extern "C" int kw_ingest_parse(kw_ingest *h, const uint8_t *d_text, int64_t n_bytes, int32_t final_, int64_t max_rows,
                               int64_t *n_rows, int64_t *consumed, int32_t *verdict, int64_t *bad_pos, void *stream)
{
    if (!h) return KW_EINVAL;
    h->have = false;
    h->have_spans = false;
    h->have_stamps = false;
    if (!n_rows || !consumed || !verdict || !bad_pos || n_bytes < 0 || n_bytes >= (int64_t)1 << 31 || max_rows < 1 ||
        (n_bytes > 0 && !d_text) || ((uintptr_t)d_text & 15u)) {
        h->err = "kw_ingest_parse: bad arguments";
        return KW_EINVAL;
    }
    *n_rows = *consumed = 0;
    *verdict = KW_INGEST_OK;
    *bad_pos = 0;
    hipStream_t st = (hipStream_t)stream;
    h->stream = st;
    KWCHK(h, hipSetDevice(h->device));
    const long long n = n_bytes, ncols = h->ncols;
    const long long ntiles = (n + TILE - 1) / TILE;
    // a record has ncols - 1 delimiters at least: the text holds at most n / ncols + 1 records that pass
    long long rows_cap = n / ncols + 1;
    if (rows_cap > max_rows) rows_cap = max_rows;
    const long long cells_cap = rows_cap * ncols;
    int rc;
    if ((rc = fit(h, h->tiles, (size_t)(ntiles + 1) * 4 * 8)) || (rc = fit(h, h->cells, (size_t)n + 32)) ||
        (rc = fit(h, h->coff, (size_t)(cells_cap + 1) * 8)) || (rc = fit(h, h->cflw, (size_t)cells_cap * 4)) ||
        (rc = fit(h, h->cfl, (size_t)cells_cap)) ||
        (rc = fit(h, h->arena, (size_t)n + 6 * (size_t)rows_cap + ARENA_PAD + 32)) ||
        (rc = fit(h, h->aoff, (size_t)(2 * rows_cap + 1) * 8)) || (rc = fit(h, h->us, (size_t)rows_cap * 8)) ||
        (rc = fit(h, h->kind, (size_t)rows_cap)) || (rc = fit(h, h->doff, (size_t)rows_cap * 4)))
        return rc;
    const int zn = h->zn;
    if (zn && ((rc = fit(h, h->stamps, (size_t)rows_cap * 8)) || (rc = fit(h, h->native, (size_t)rows_cap)))) return rc;
    Dev init;
    memset(&init, 0, sizeof(init));
    init.errs.nul = init.errs.utf8 = init.errs.quote = init.errs.cr = init.errs.blank = init.errs.fields = NONE;
    *h->H = init;   // (pinned: the copy below reads it in stream order; the last parse's copy back has finished)
    Args A;
    A.text = d_text;
    A.n = n;
    A.ntiles = ntiles;
    A.max_rows = max_rows;
    A.cells_cap = cells_cap;
    A.final_ = final_ ? 1 : 0;
    A.ncols = (int)ncols;
    A.tq = (u64 *)h->tiles.p;
    A.te = A.tq + (ntiles + 1);
    A.td = A.te + (ntiles + 1);
    A.tk = A.td + (ntiles + 1);
    A.D = h->D;
    A.coff = (long long *)h->coff.p;
    A.cflw = (uint32_t *)h->cflw.p;
    A.cells = (uint8_t *)h->cells.p;
    const int gcap = grid_cap();
    const dim3 tgrid((unsigned)(ntiles < 1 ? 1 : (ntiles > gcap ? gcap : ntiles)));

    KWCHK(h, hipEventRecord(h->ev[0], st));
    KWCHK(h, hipMemcpyAsync(h->D, h->H, sizeof(Dev), hipMemcpyHostToDevice, st));
    KWCHK(h, hipMemsetAsync(A.coff, 0, 8, st));
    KWCHK(h, hipMemsetAsync(A.cflw, 0, (size_t)cells_cap * 4, st));
    // classify
    hipLaunchKernelGGL(ig_quotes_kernel, tgrid, dim3(BLOCK), 0, st, d_text, n, ntiles, A.tq, h->D);
    {
        ScanArgs S{};
        S.a[0] = A.tq;
        S.total[0] = &h->D->tot_q;
        S.m = ntiles;
        hipLaunchKernelGGL(ig_scan_kernel, dim3(1), dim3(BLOCK), 0, st, S);
    }
    KWCHK(h, hipEventRecord(h->ev[1], st));
    // cells
    hipLaunchKernelGGL(ig_tile_kernel<0>, tgrid, dim3(BLOCK), 0, st, A);
    {
        ScanArgs S{};
        S.a[0] = A.te; S.a[1] = A.td; S.a[2] = A.tk;
        S.total[0] = &h->D->tot_e; S.total[1] = &h->D->tot_d; S.total[2] = &h->D->tot_k;
        S.m = ntiles;
        hipLaunchKernelGGL(ig_scan_kernel, dim3(3), dim3(BLOCK), 0, st, S);
    }
    hipLaunchKernelGGL(ig_tile_kernel<1>, tgrid, dim3(BLOCK), 0, st, A);
    hipLaunchKernelGGL(ig_finish_kernel, dim3(1), dim3(64), 0, st, h->D, (const long long *)A.coff, n, A.final_,
                       (long long)max_rows, (int)ncols);
    hipLaunchKernelGGL(ig_flags_kernel, grid_for(cells_cap, BLOCK, gcap), dim3(BLOCK), 0, st, h->D, (const uint8_t *)A.cells,
                       (const long long *)A.coff, (const uint32_t *)A.cflw, (uint8_t *)h->cfl.p, (int)ncols, h->cols,
                       (const uint8_t *)h->d_na, (const int *)h->d_na_off, h->n_na);
    KWCHK(h, hipEventRecord(h->ev[2], st));
    // arena + dates
    hipLaunchKernelGGL(ig_rows_kernel, grid_for(rows_cap, BLOCK, gcap), dim3(BLOCK), 0, st, (const Dev *)h->D,
                       (const uint8_t *)A.cells, (const long long *)A.coff, (const uint8_t *)h->cfl.p, (int)ncols, h->cols,
                       (long long *)h->us.p, (uint8_t *)h->kind.p, (int *)h->doff.p, (u64 *)h->aoff.p);
    if (zn) {
        KWCHK(h, hipEventRecord(h->ev[4], st));
        hipLaunchKernelGGL(ig_stamps_kernel, grid_for(rows_cap, BLOCK, gcap), dim3(BLOCK), 0, st, (const Dev *)h->D,
                           (const long long *)h->us.p, (const uint8_t *)h->kind.p, (const int64_t *)h->zat.p,
                           (const int32_t *)h->zoff.p, zn, (int64_t *)h->stamps.p, (uint8_t *)h->native.p);
        KWCHK(h, hipEventRecord(h->ev[5], st));
    }
    {
        ScanArgs S{};
        S.a[0] = (u64 *)h->aoff.p;
        S.total[0] = (u64 *)&h->D->arena_bytes;
        S.m_dev = &h->D->n_rows;
        S.verdict = &h->D->verdict;
        S.m_mul = 2;
        S.m_add = 1;
        hipLaunchKernelGGL(ig_scan_kernel, dim3(1), dim3(BLOCK), 0, st, S);
    }
    hipLaunchKernelGGL(ig_gather_kernel<true>, grid_for((n + 6 * rows_cap + ARENA_PAD) / 16 + 1, BLOCK, gcap), dim3(BLOCK), 0,
                       st, (const Dev *)h->D, (const uint8_t *)A.cells, (const long long *)A.coff, (const uint8_t *)h->cfl.p,
                       (int)ncols, h->cols.c[0], h->cols.c[1], (const u64 *)h->aoff.p, (uint8_t *)h->arena.p, ARENA_PAD);
    KWCHK(h, hipEventRecord(h->ev[3], st));
    KWCHK(h, hipMemcpyAsync(h->H, h->D, sizeof(Dev), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    for (int k = 0; k < 3; ++k) KWCHK(h, hipEventElapsedTime(&h->ms[k], h->ev[k], h->ev[k + 1]));
    KWCHK(h, hipEventElapsedTime(&h->ms[3], h->ev[0], h->ev[3]));
    h->ms[4] = 0.f;
    if (zn) KWCHK(h, hipEventElapsedTime(&h->ms[4], h->ev[4], h->ev[5]));
    *verdict = h->H->verdict;
    *bad_pos = h->H->bad_pos;
    *n_rows = h->H->n_rows;
    *consumed = h->H->consumed;
    h->have = h->H->verdict == KW_INGEST_OK;
    h->have_stamps = h->have && zn > 0;
    h->ptext = d_text;
    h->pn = n;
    h->pfinal = A.final_;
    return KW_OK;
}

extern "C" int kw_ingest_stage(kw_ingest *h, int32_t slot, int64_t n_bytes, uint8_t **host)
{
    if (!h) return KW_EINVAL;
    if (!host || slot < 0 || slot > 1 || n_bytes < 0 || n_bytes >= (int64_t)1 << 31) {
        h->err = "kw_ingest_stage: bad arguments";
        return KW_EINVAL;
    }
    KWCHK(h, hipSetDevice(h->device));
    const size_t nb = (size_t)n_bytes;
    const int rc = ensure_pinned(h, &h->stage[slot], &h->stage_cap[slot], nb, nb + nb / 4 + 4096);
    if (rc) return rc;
    *host = (uint8_t *)h->stage[slot];
    return KW_OK;
}

extern "C" int kw_ingest_upload(kw_ingest *h, int32_t slot, int64_t start, int64_t n_bytes, const uint8_t **d_text,
                                void *stream)
{
    if (!h) return KW_EINVAL;
    if (!d_text || slot < 0 || slot > 1 || start < 0 || n_bytes < 0 || (size_t)(start + n_bytes) > h->stage_cap[slot]) {
        h->err = "kw_ingest_upload: bad arguments";
        return KW_EINVAL;
    }
    KWCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = fit(h, h->text, (size_t)n_bytes + 16))) return rc;
    if (n_bytes)
        KWCHK(h, hipMemcpyAsync(h->text.p, (const uint8_t *)h->stage[slot] + start, (size_t)n_bytes,
                                hipMemcpyHostToDevice, (hipStream_t)stream));
    *d_text = (const uint8_t *)h->text.p;
    return KW_OK;
}

#define IG_NEED_PARSE(h, name)                                               \
    do {                                                                     \
        if (!(h)) return KW_EINVAL;                                          \
        if (!(h)->have) { (h)->err = name ": no parse that was taken"; return KW_ESTATE; } \
    } while (0)

extern "C" int kw_ingest_cells(kw_ingest *h, const uint8_t **d_cells, const int64_t **d_coff, const uint8_t **d_cfl,
                               int64_t *cell_bytes)
{
    IG_NEED_PARSE(h, "kw_ingest_cells");
    if (!d_cells || !d_coff || !d_cfl || !cell_bytes) { h->err = "kw_ingest_cells: bad arguments"; return KW_EINVAL; }
    *d_cells = (const uint8_t *)h->cells.p;
    *d_coff = (const int64_t *)h->coff.p;
    *d_cfl = (const uint8_t *)h->cfl.p;
    *cell_bytes = h->H->cell_bytes;
    return KW_OK;
}

extern "C" int kw_ingest_arena(kw_ingest *h, const uint8_t **d_arena, const int64_t **d_off, int64_t *arena_bytes)
{
    IG_NEED_PARSE(h, "kw_ingest_arena");
    if (!d_arena || !d_off || !arena_bytes) { h->err = "kw_ingest_arena: bad arguments"; return KW_EINVAL; }
    *d_arena = (const uint8_t *)h->arena.p;
    *d_off = (const int64_t *)h->aoff.p;
    *arena_bytes = h->H->arena_bytes;
    return KW_OK;
}

// the date arrays of the last parse into host arrays (off_s may be null)
static int copy_dates(kw_ingest *h, size_t nr, int64_t *us, uint8_t *kind, int32_t *off_s)
{
    KWCHK(h, hipSetDevice(h->device));
    KWCHK(h, hipMemcpyAsync(us, h->us.p, nr * 8, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipMemcpyAsync(kind, h->kind.p, nr, hipMemcpyDeviceToHost, h->stream));
    if (off_s) KWCHK(h, hipMemcpyAsync(off_s, h->doff.p, nr * 4, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipStreamSynchronize(h->stream));
    return KW_OK;
}

extern "C" int kw_ingest_dates(kw_ingest *h, int64_t *us, uint8_t *kind)
{
    IG_NEED_PARSE(h, "kw_ingest_dates");
    const size_t nr = (size_t)h->H->n_rows;
    if (nr && (!us || !kind)) { h->err = "kw_ingest_dates: bad arguments"; return KW_EINVAL; }
    if (!nr) return KW_OK;
    const int rc = copy_dates(h, nr, us, kind, nullptr);
    if (rc) return rc;
    for (size_t r = 0; r < nr; ++r)   // kwcsv_dates knows the 19-byte layout alone: the ISO rule's other kinds are its 0
        if (kind[r] > 2) { kind[r] = 0; us[r] = 0; }
    return KW_OK;
}

extern "C" int kw_ingest_dates_iso(kw_ingest *h, int64_t *us, uint8_t *kind, int32_t *off_s)
{
    IG_NEED_PARSE(h, "kw_ingest_dates_iso");
    const size_t nr = (size_t)h->H->n_rows;
    if (nr && (!us || !kind || !off_s)) { h->err = "kw_ingest_dates_iso: bad arguments"; return KW_EINVAL; }
    if (!nr) return KW_OK;
    return copy_dates(h, nr, us, kind, off_s);
}

extern "C" int kw_ingest_zone(kw_ingest *h, const int64_t *at, const int32_t *off, int32_t n_trans)
{
    if (!h) return KW_EINVAL;
    if (n_trans < 0 || n_trans > KWST_CAPACITY || (n_trans > 0 && (!at || !off))) {
        h->err = "kw_ingest_zone: bad arguments";
        return KW_EINVAL;
    }
    for (int32_t k = 0; k < n_trans; ++k)
        if (at[k] >= at[k + 1]) { h->err = "kw_ingest_zone: the instants do not ascend"; return KW_EINVAL; }
    if (n_trans > 0 && (at[0] > INT64_MAX - KWST_MARGIN || at[n_trans] < INT64_MIN + KWST_MARGIN)) {
        h->err = "kw_ingest_zone: bad arguments";
        return KW_EINVAL;
    }
    h->zn = 0;
    if (n_trans == 0) return KW_OK;
    KWCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = fit(h, h->zat, ((size_t)n_trans + 1) * 8)) || (rc = fit(h, h->zoff, (size_t)n_trans * 4))) return rc;
    KWCHK(h, hipMemcpy(h->zat.p, at, ((size_t)n_trans + 1) * 8, hipMemcpyHostToDevice));
    KWCHK(h, hipMemcpy(h->zoff.p, off, (size_t)n_trans * 4, hipMemcpyHostToDevice));
    h->zn = n_trans;
    return KW_OK;
}

extern "C" int kw_ingest_stamps(kw_ingest *h, int64_t *stamps, uint8_t *native)
{
    IG_NEED_PARSE(h, "kw_ingest_stamps");
    if (!h->have_stamps) { h->err = "kw_ingest_stamps: the parse had no zone table"; return KW_ESTATE; }
    const size_t nr = (size_t)h->H->n_rows;
    if (nr && (!stamps || !native)) { h->err = "kw_ingest_stamps: bad arguments"; return KW_EINVAL; }
    if (!nr) return KW_OK;
    KWCHK(h, hipSetDevice(h->device));
    KWCHK(h, hipMemcpyAsync(stamps, h->stamps.p, nr * 8, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipMemcpyAsync(native, h->native.p, nr, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipStreamSynchronize(h->stream));
    return KW_OK;
}

extern "C" int kw_ingest_stamps_device(kw_ingest *h, const int64_t **d_stamps)
{
    IG_NEED_PARSE(h, "kw_ingest_stamps_device");
    if (!h->have_stamps) { h->err = "kw_ingest_stamps_device: the parse had no zone table"; return KW_ESTATE; }
    if (!d_stamps) { h->err = "kw_ingest_stamps_device: bad arguments"; return KW_EINVAL; }
    *d_stamps = (const int64_t *)h->stamps.p;
    return KW_OK;
}

extern "C" int kw_ingest_column_flags(kw_ingest *h, int32_t *witness)
{
    IG_NEED_PARSE(h, "kw_ingest_column_flags");
    if (!witness) { h->err = "kw_ingest_column_flags: bad arguments"; return KW_EINVAL; }
    for (int k = 0; k < 6; ++k) witness[k] = h->H->witness[k] ? 1 : 0;
    return KW_OK;
}

extern "C" int kw_ingest_copy_cells(kw_ingest *h, uint8_t *cells, int64_t *coff, uint8_t *cfl)
{
    IG_NEED_PARSE(h, "kw_ingest_copy_cells");
    const size_t nc = (size_t)h->H->n_rows * (size_t)h->ncols, nb = (size_t)h->H->cell_bytes;
    if (!coff || (nc && !cfl) || (nb && !cells)) { h->err = "kw_ingest_copy_cells: bad arguments"; return KW_EINVAL; }
    KWCHK(h, hipSetDevice(h->device));
    if (nb) KWCHK(h, hipMemcpyAsync(cells, h->cells.p, nb, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipMemcpyAsync(coff, h->coff.p, (nc + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    if (nc) KWCHK(h, hipMemcpyAsync(cfl, h->cfl.p, nc, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipStreamSynchronize(h->stream));
    return KW_OK;
}

extern "C" int kw_ingest_copy_arena(kw_ingest *h, uint8_t *arena, int64_t *off)
{
    IG_NEED_PARSE(h, "kw_ingest_copy_arena");
    const size_t nr = (size_t)h->H->n_rows, nb = (size_t)h->H->arena_bytes + ARENA_PAD;
    if (!arena || !off) { h->err = "kw_ingest_copy_arena: bad arguments"; return KW_EINVAL; }
    KWCHK(h, hipSetDevice(h->device));
    KWCHK(h, hipMemcpyAsync(arena, h->arena.p, nb, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipMemcpyAsync(off, h->aoff.p, (2 * nr + 1) * 8, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipStreamSynchronize(h->stream));
    return KW_OK;
}

extern "C" int kw_ingest_copy_column(kw_ingest *h, int32_t col, uint8_t *bytes, int64_t cap, int64_t *off, uint8_t *fl)
{
    IG_NEED_PARSE(h, "kw_ingest_copy_column");
    const long long nr = h->H->n_rows;
    if (col < 0 || col >= h->ncols || !off || cap < 0 || (nr && !fl) || (cap > 0 && !bytes)) {
        h->err = "kw_ingest_copy_column: bad arguments";
        return KW_EINVAL;
    }
    off[0] = 0;
    if (!nr) return KW_OK;
    hipStream_t st = h->stream;
    KWCHK(h, hipSetDevice(h->device));
    int rc;
    if ((rc = fit(h, h->col_off, (size_t)(nr + 1) * 8)) || (rc = fit(h, h->col_fl, (size_t)nr)) ||
        (rc = fit(h, h->col_buf, (size_t)h->H->cell_bytes + 32)))
        return rc;
    const int gcap = grid_cap();
    hipLaunchKernelGGL(ig_collen_kernel, grid_for(nr, BLOCK, gcap), dim3(BLOCK), 0, st, (const Dev *)h->D,
                       (const long long *)h->coff.p, (const uint8_t *)h->cfl.p, h->ncols, (int)col, (u64 *)h->col_off.p,
                       (uint8_t *)h->col_fl.p);
    {
        ScanArgs S{};
        S.a[0] = (u64 *)h->col_off.p;
        S.total[0] = (u64 *)&h->D->col_bytes;
        S.m = nr + 1;
        hipLaunchKernelGGL(ig_scan_kernel, dim3(1), dim3(BLOCK), 0, st, S);
    }
    hipLaunchKernelGGL(ig_gather_kernel<false>, grid_for(h->H->cell_bytes / 16 + 1, BLOCK, gcap), dim3(BLOCK), 0, st,
                       (const Dev *)h->D, (const uint8_t *)h->cells.p, (const long long *)h->coff.p,
                       (const uint8_t *)h->cfl.p, h->ncols, (int)col, 0, (const u64 *)h->col_off.p, (uint8_t *)h->col_buf.p, 0);
    KWCHK(h, hipMemcpyAsync(off, h->col_off.p, (size_t)(nr + 1) * 8, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipMemcpyAsync(fl, h->col_fl.p, (size_t)nr, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    const int64_t nb = off[nr];
    if (nb > cap) { h->err = "kw_ingest_copy_column: the column holds " + std::to_string(nb) + " bytes"; return KW_EOVERFLOW; }
    if (nb) KWCHK(h, hipMemcpy(bytes, h->col_buf.p, (size_t)nb, hipMemcpyDeviceToHost));
    return KW_OK;
}

extern "C" int kw_ingest_spans(kw_ingest *h, const int64_t **d_start, const int64_t **d_end, int64_t *n_rows,
                               int32_t *ncols, const uint8_t **d_text, int64_t *n_bytes)
{
    IG_NEED_PARSE(h, "kw_ingest_spans");
    if (!d_start || !d_end || !n_rows || !ncols || !d_text || !n_bytes) {
        h->err = "kw_ingest_spans: bad arguments";
        return KW_EINVAL;
    }
    const long long nr = h->H->n_rows;
    if (!h->have_spans) {
        KWCHK(h, hipSetDevice(h->device));
        int rc;
        if ((rc = fit(h, h->spans, (size_t)(2 * nr + 2) * 8))) return rc;
        if (nr) {
            Args A{};
            A.text = h->ptext;
            A.n = h->pn;
            A.ntiles = (h->pn + TILE - 1) / TILE;
            A.final_ = h->pfinal;
            A.ncols = h->ncols;
            A.tq = (u64 *)h->tiles.p;
            A.te = A.tq + (A.ntiles + 1);
            A.D = h->D;
            const int gcap = grid_cap();
            const dim3 tgrid((unsigned)(A.ntiles < 1 ? 1 : (A.ntiles > gcap ? gcap : A.ntiles)));
            hipLaunchKernelGGL(ig_spans_kernel, tgrid, dim3(BLOCK), 0, h->stream, A, (long long *)h->spans.p,
                               (long long *)h->spans.p + nr);
            KWCHK(h, hipGetLastError());
        }
        h->have_spans = true;
    }
    *d_start = (const int64_t *)h->spans.p;
    *d_end = (const int64_t *)h->spans.p + nr;
    *n_rows = nr;
    *ncols = h->ncols;
    *d_text = h->ptext;
    *n_bytes = h->pn;
    return KW_OK;
}

extern "C" int kw_ingest_copy_spans(kw_ingest *h, int64_t *start, int64_t *end)
{
    IG_NEED_PARSE(h, "kw_ingest_copy_spans");
    const int64_t *ds, *de;
    const uint8_t *dt;
    int64_t nr, nb;
    int32_t nc;
    int rc;
    if ((rc = kw_ingest_spans(h, &ds, &de, &nr, &nc, &dt, &nb))) return rc;
    if (!nr) return KW_OK;
    if (!start || !end) { h->err = "kw_ingest_copy_spans: bad arguments"; return KW_EINVAL; }
    KWCHK(h, hipMemcpyAsync(start, ds, (size_t)nr * 8, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipMemcpyAsync(end, de, (size_t)nr * 8, hipMemcpyDeviceToHost, h->stream));
    KWCHK(h, hipStreamSynchronize(h->stream));
    KWCHK(h, hipGetLastError());
    return KW_OK;
}

extern "C" int kw_ingest_last_ms(kw_ingest *h, float *ms, int32_t n)
{
    if (!h || !ms || n < 0) return KW_EINVAL;
    for (int k = 0; k < n && k < 5; ++k) ms[k] = h->ms[k];
    return KW_OK;
}
