// libkwmatch: the per-ticker CSV rows rendered on the device (include/kwrows.h, kw_rows_cells / kw_rows_emit) --
// the reference's append_to_csv (match_keywords.py:128-146) for the rows of the last kw_rows_run, byte for byte what
// kwcsv_emit_mt (csrc/kwcsv.c) writes: the JSON cells never leave the device, the finished lines arrive in pinned
// host memory.  tests/emit_rule.py restates the rule.
//
// Stages of kw_rows_emit (kernels exchange data only across launches; sizes come from a measure pass and an
// exclusive scan, rw::scan_launch; the buffers belong to the handle and grow on demand):
//   order    em_count_kernel    rows per KB ticker (the first n_rows_use rows)
//            em_scatter_kernel  rows into their ticker's segment (any order inside it); marks the articles that
//                               have a rendered row
//            em_sort_kernel     a lane per row ranks it inside its segment by row number (m rows of a ticker cost
//                               m * m compares, any m is exact): the stable order by ticker; the rows' document,
//                               ticker and time stamp in that order
//   measure  em_measure_kernel  a wave per (article, cell) of the marked articles: the count of '"', whether the
//                               cell is quoted, '\r', NUL, the text-witness rule (kwcsv_text_witness) -> the cell's
//                               rendered length and the article's flag bits
//            em_rowlen_kernel   a wave per row: the rendered lengths of its two JSON cells, its line length, its
//                               flags; then the scan that gives line_off
//   fill     em_render_kernel   a wave per (article, cell) writes the cell in QUOTE_MINIMAL form into scratch: an
//                               article's cells are rendered once, as the host emitter does, and its rows copy
//                               them.  Byte i of a quoted cell lands at 1 + i + (the '"' before i): a wave64
//                               ballot, the popcount of the lower lanes, and a carry from step to step.  A cell
//                               is never split over waves, so no carry crosses a workgroup.
//            em_fill_kernel     a workgroup per row: the stamp's digits, the two scratch parts (copied as aligned
//                               32-bit stores whatever the two alignments are: two aligned loads and a byte
//                               shift per store), the two JSON cells (a wave each, the ballot form above)
//   copy     the lines, line_off, flags and the rows' document / ticker / stamp to pinned host buffers
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/kwrows.h"
#include "kwdev.hpp"
#include "kwrows_handle.hpp"

namespace rw {

using kwd::ieq;
constexpr uint32_t BAD = 0xFFFFFFFFu;
constexpr uint8_t CELL_NA = 2;          // KWCSV_NA (csrc/kwcsv.c)
constexpr size_t SCRATCH_PAD = 16;      // the shifted copy reads up to 3 bytes past a part's end
// the emit's counters (device, 64-bit words)
enum { E_BAD = 0, E_NUL = 1, E_SCRATCH = 2, E_BYTES = 3, E_TROWS = 4, E_WORDS = 8 };


struct Emit {
    Buf c_buf, c_off, c_fl;             // the chunk's tokenized cells
    const uint8_t *b_cells = nullptr;   // kw_rows_cells_device: the caller's device buffers instead
    const int64_t *b_coff = nullptr;
    const uint8_t *b_cfl = nullptr;
    bool borrowed = false;
    int64_t cells_docs = -1;
    int32_t ncols = 0;
    Buf stamps, tcnt, tcur, seg, ord, used, dfl, slen, cq, llen, jl, flags, o_doc, o_ti, o_stamp, scratch, out;
    unsigned long long *tot = nullptr;
    Buf p_out, p_off, p_flags, p_doc, p_ti, p_stamp;   // pinned host memory
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // [5]: the fill's start
    float ms[4] = {0, 0, 0, 0};
    bool have = false;
};

// ---- what a wave learns about one cell (every member is wave-uniform)
struct CellStat {
    unsigned long long nq;     // '"' bytes
    bool trig, cr, nul;        // holds ',', '"' or '\n'; holds '\r'; holds NUL
    bool other;                // a non-blank byte that no number holds (not 0-9 + - . e E)
    long long nonblank, first, last;   // non-blank bytes, the first and the last of them (-1: none)
};

__device__ __forceinline__ CellStat wave_stat(const uint8_t *__restrict__ s, long long n, int lane)
{
    CellStat S;
    S.nq = 0;
    S.trig = S.cr = S.nul = S.other = false;
    S.nonblank = 0;
    S.first = S.last = -1;
    for (long long i0 = 0; i0 < n; i0 += 64) {   // (wave-uniform trip count)
        const long long i = i0 + lane;
        const bool in = i < n;
        const uint8_t c = in ? s[i] : (uint8_t)' ';
        const unsigned long long mq = __ballot(in && c == '"');
        const unsigned long long mt = __ballot(in && (c == ',' || c == '\n'));
        const unsigned long long mcr = __ballot(in && c == '\r');
        const unsigned long long mz = __ballot(in && c == 0);
        const unsigned long long mnb = __ballot(in && c != ' ' && c != '\t');
        const bool cls = (c >= '0' && c <= '9') || c == '+' || c == '-' || c == '.' || c == 'e' || c == 'E';
        const unsigned long long mo = __ballot(in && c != ' ' && c != '\t' && !cls);
        S.nq += (unsigned long long)__popcll(mq);
        S.trig |= (mq | mt) != 0;
        S.cr |= mcr != 0;
        S.nul |= mz != 0;
        S.other |= mo != 0;
        if (mnb) {
            if (S.first < 0) S.first = i0 + (__ffsll((long long)mnb) - 1);
            S.last = i0 + 63 - __clzll((long long)mnb);
            S.nonblank += __popcll(mnb);
        }
    }
    return S;
}

// kwcsv_text_witness (csrc/kwcsv.c) of a non-NA cell whose bytes gave S
__device__ __forceinline__ bool text_witness(const uint8_t *__restrict__ s, const CellStat &S)
{
    if (S.first < 0) return true;                      // empty, or blanks only: no number
    const uint8_t *t = s + S.first;
    const long long m = S.last - S.first + 1;
    if (m <= 9) {                                      // the longest literal: a sign and "infinity"
        if (ieq(t, m, "true", 4) || ieq(t, m, "false", 5)) return false;
        const int sg = (t[0] == '+' || t[0] == '-') ? 1 : 0;
        if (ieq(t + sg, m - sg, "inf", 3) || ieq(t + sg, m - sg, "infinity", 8)) return false;
    }
    return S.other || S.nonblank != m;                 // a byte no number holds (a blank between others is one)
}

// a cell in QUOTE_MINIMAL form by one wave: dst gets n bytes as they are, or n + nq + 2 when quoted
__device__ __forceinline__ void wave_put(uint8_t *__restrict__ dst, const uint8_t *__restrict__ s, long long n,
                                         bool quoted, int lane)
{
    if (!quoted) {
        for (long long i = lane; i < n; i += 64) dst[i] = s[i];
        return;
    }
    if (lane == 0) dst[0] = '"';
    long long carry = 0;                               // the '"' of the earlier steps
    for (long long i0 = 0; i0 < n; i0 += 64) {         // (wave-uniform trip count)
        const long long i = i0 + lane;
        const bool in = i < n;
        const uint8_t c = in ? s[i] : (uint8_t)0;
        const bool q = in && c == '"';
        const unsigned long long mq = __ballot(q);
        const int before = __popcll(mq & ((1ull << lane) - 1ull));
        if (in) {
            uint8_t *o = dst + 1 + i + carry + before;
            o[0] = c;
            if (q) o[1] = '"';
        }
        carry += __popcll(mq);
    }
    if (lane == 0) dst[1 + n + carry] = '"';
}

// n bytes by one workgroup, dst and src of any alignment: aligned 32-bit stores, each from two aligned loads.
// Reads at most 3 bytes before src (down to its 4-byte boundary) and 3 after src + n.
__device__ __forceinline__ void block_copy(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, long long n)
{
    const int tid = threadIdx.x;
    long long head = (long long)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
    if (head > n) head = n;
    if (tid < head) dst[tid] = src[tid];
    const long long nw = (n - head) >> 2;
    uint32_t *d4 = (uint32_t *)(dst + head);
    const uint8_t *s = src + head;
    const uint32_t sh = (uint32_t)((uintptr_t)s & 3u);
    const uint32_t *sa = (const uint32_t *)(s - sh);
    if (sh == 0) {
        for (long long w = tid; w < nw; w += BLOCK) d4[w] = sa[w];
    } else {
        const uint32_t down = 8u * sh, up = 32u - down;
        for (long long w = tid; w < nw; w += BLOCK) d4[w] = (sa[w] >> down) | (sa[w + 1] << up);
    }
    const long long done = head + 4 * nw;
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

__device__ __forceinline__ unsigned long long stamp_abs(long long v)
{
    return v < 0 ? (unsigned long long)(-(v + 1)) + 1ull : (unsigned long long)v;
}

__device__ __forceinline__ int stamp_len(long long v)   // the bytes of v as a signed decimal
{
    unsigned long long u = stamp_abs(v);
    int nd = v < 0 ? 1 : 0;
    do { ++nd; u /= 10ull; } while (u);
    return nd;
}

// ---- order
__global__ __launch_bounds__(BLOCK) void em_count_kernel(const int32_t *__restrict__ row_ti, uint32_t n_use,
                                                         uint32_t n_tickers, unsigned long long *__restrict__ tcnt,
                                                         unsigned long long *__restrict__ tot)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_use) return;
    const uint32_t t = (uint32_t)row_ti[r];
    if (t >= n_tickers) { tot[E_BAD] = 1ull; return; }
    atomicAdd(&tcnt[t], 1ull);
}

__global__ __launch_bounds__(BLOCK) void em_scatter_kernel(const int32_t *__restrict__ row_ti,
                                                           const int32_t *__restrict__ row_doc, uint32_t n_use,
                                                           uint32_t n_tickers, uint32_t n_docs,
                                                           const unsigned long long *__restrict__ toff,
                                                           uint32_t *__restrict__ tcur, uint32_t *__restrict__ seg,
                                                           uint8_t *__restrict__ used, unsigned long long *__restrict__ tot)
{
    const uint32_t r = blockIdx.x * BLOCK + threadIdx.x;
    if (r >= n_use) return;
    const uint32_t t = (uint32_t)row_ti[r], d = (uint32_t)row_doc[r];
    if (t >= n_tickers) return;
    if (d >= n_docs) { tot[E_BAD] = 1ull; return; }
    seg[toff[t] + atomicAdd(&tcur[t], 1u)] = r;   // < toff[t + 1]: the count pass saw this row
    used[d] = 1;
}

// slot k of seg (preset to BAD) -> the row's place in the stable order by ticker; slots no row fills stay BAD
__global__ __launch_bounds__(BLOCK) void em_sort_kernel(const uint32_t *__restrict__ seg, uint32_t n_use,
                                                        const int32_t *__restrict__ row_ti,
                                                        const int32_t *__restrict__ row_doc,
                                                        const unsigned long long *__restrict__ toff,
                                                        const int64_t *__restrict__ stamps, uint32_t *__restrict__ ord,
                                                        int32_t *__restrict__ o_doc, int32_t *__restrict__ o_ti,
                                                        int64_t *__restrict__ o_stamp)
{
    const uint32_t k = blockIdx.x * BLOCK + threadIdx.x;
    if (k >= n_use) return;
    const uint32_t r = seg[k];
    if (r >= n_use) {          // fewer rows than slots (a row was refused): such slots are the last ones
        ord[k] = BAD;
        return;
    }
    const uint32_t t = (uint32_t)row_ti[r];
    const uint32_t s = (uint32_t)toff[t], e = (uint32_t)toff[t + 1];
    uint32_t rank = 0;
    for (uint32_t j = s; j < e; ++j) rank += seg[j] < r ? 1u : 0u;
    const int32_t d = row_doc[r];
    ord[s + rank] = r;
    o_doc[s + rank] = d;
    o_ti[s + rank] = (int32_t)t;
    o_stamp[s + rank] = stamps[d];
}

// ---- measure
// out column of chunk cell c (0 date_time, 1..5 title .. article_text): 0, 3..7
__device__ __forceinline__ int out_col(int c) { return c == 0 ? 0 : c + 2; }

struct Cols { int32_t c[6]; };

__global__ __launch_bounds__(BLOCK) void em_measure_kernel(const uint8_t *__restrict__ buf, const int64_t *__restrict__ off,
                                                           const uint8_t *__restrict__ fl, int32_t ncols, Cols cols,
                                                           uint32_t n_docs, const uint8_t *__restrict__ used,
                                                           unsigned long long *__restrict__ slen, uint8_t *__restrict__ cq,
                                                           uint32_t *__restrict__ dfl, unsigned long long *__restrict__ tot)
{
    const uint64_t w = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (w >= (uint64_t)n_docs * 6) return;
    const uint32_t d = (uint32_t)(w / 6);
    const int c = (int)(w % 6);
    if (!used[d]) return;                                   // (slen stays 0)
    const int64_t cell = (int64_t)d * ncols + cols.c[c];
    const unsigned long long comma = c >= 2 ? 1ull : 0ull;  // title .. article_text stand joined by ','
    if (fl[cell] & CELL_NA) {                               // NaN: written empty, its bytes are not looked at
        if (lane == 0) {
            atomicOr(&dfl[d], 1u << (8 + out_col(c)));
            slen[w] = comma;
            cq[w] = 0;
        }
        return;
    }
    const uint8_t *s = buf + off[cell];
    const long long n = off[cell + 1] - off[cell];
    const CellStat S = wave_stat(s, n, lane);
    if (lane != 0) return;
    uint32_t bits = 0;
    if (S.cr) bits |= 1u << 16;
    if (text_witness(s, S)) bits |= 1u << out_col(c);
    atomicOr(&dfl[d], bits);
    if (S.nul) tot[E_NUL] = 1ull;
    slen[w] = comma + (unsigned long long)n + (S.trig ? S.nq + 2ull : 0ull);
    cq[w] = S.trig ? 1 : 0;
}

__global__ __launch_bounds__(BLOCK) void em_rowlen_kernel(const uint32_t *__restrict__ ord, uint32_t n_use, uint32_t n_docs,
                                                          const int32_t *__restrict__ row_doc,
                                                          const int64_t *__restrict__ stamps,
                                                          const unsigned long long *__restrict__ soff,
                                                          const uint32_t *__restrict__ dfl,
                                                          const uint8_t *__restrict__ json, const int64_t *__restrict__ json_off,
                                                          unsigned long long *__restrict__ llen,
                                                          unsigned long long *__restrict__ jl, uint32_t *__restrict__ flags,
                                                          unsigned long long *__restrict__ tot)
{
    const uint64_t k = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (k >= n_use) return;
    const uint32_t r = ord[k];
    if (r >= n_use) {                                       // (llen, jl and flags stay 0)
        if (lane == 0) tot[E_BAD] = 1ull;
        return;
    }
    const uint32_t d = (uint32_t)row_doc[r];
    if (d >= n_docs) return;
    uint32_t bits = dfl[d] | 6u;                            // the JSON cells are text witnesses
    unsigned long long len = (unsigned long long)stamp_len(stamps[d]) + 1ull + (soff[6ull * d + 1] - soff[6ull * d]);
    for (int c = 0; c < 2; ++c) {
        const long long a = json_off[2ull * r + c], n = json_off[2ull * r + c + 1] - a;
        const CellStat S = wave_stat(json + a, n, lane);
        const unsigned long long m = (unsigned long long)n + (S.trig ? S.nq + 2ull : 0ull);
        if (S.cr) bits |= 1u << 16;
        if (S.nul && lane == 0) tot[E_NUL] = 1ull;
        if (lane == 0) jl[2 * k + c] = m;
        len += 1ull + m;
    }
    len += 1ull + (soff[6ull * d + 6] - soff[6ull * d + 1]) + 1ull;
    if (lane == 0) {
        llen[k] = len;
        flags[k] = bits;
    }
}

// ---- fill
__global__ __launch_bounds__(BLOCK) void em_render_kernel(const uint8_t *__restrict__ buf, const int64_t *__restrict__ off,
                                                          const uint8_t *__restrict__ fl, int32_t ncols, Cols cols,
                                                          uint32_t n_docs, const uint8_t *__restrict__ used,
                                                          const unsigned long long *__restrict__ soff,
                                                          const uint8_t *__restrict__ cq, uint8_t *__restrict__ scratch)
{
    const uint64_t w = ((uint64_t)blockIdx.x * BLOCK + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63;
    if (w >= (uint64_t)n_docs * 6) return;
    const uint32_t d = (uint32_t)(w / 6);
    const int c = (int)(w % 6);
    if (!used[d]) return;
    uint8_t *o = scratch + soff[w];
    if (c >= 2) {
        if (lane == 0) o[0] = ',';
        ++o;
    }
    const int64_t cell = (int64_t)d * ncols + cols.c[c];
    if (fl[cell] & CELL_NA) return;
    wave_put(o, buf + off[cell], off[cell + 1] - off[cell], cq[w] != 0, lane);   // (exactly soff[w + 1] - soff[w] bytes)
}

__global__ __launch_bounds__(BLOCK) void em_fill_kernel(const uint32_t *__restrict__ ord, uint32_t n_use, uint32_t n_docs,
                                                        const int32_t *__restrict__ row_doc,
                                                        const int64_t *__restrict__ stamps,
                                                        const unsigned long long *__restrict__ soff,
                                                        const uint8_t *__restrict__ scratch,
                                                        const uint8_t *__restrict__ json, const int64_t *__restrict__ json_off,
                                                        const unsigned long long *__restrict__ jl,
                                                        const unsigned long long *__restrict__ loff, uint8_t *__restrict__ out)
{
    const uint32_t k = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t r = ord[k];
    if (r >= n_use) return;
    const uint32_t d = (uint32_t)row_doc[r];
    if (d >= n_docs) return;
    const long long v = stamps[d];
    const int nd = stamp_len(v);
    const unsigned long long a0 = soff[6ull * d], b0 = soff[6ull * d + 1], b1 = soff[6ull * d + 6];
    const long long la = (long long)(b0 - a0), lb = (long long)(b1 - b0);
    const long long j0 = json_off[2ull * r], j1 = json_off[2ull * r + 1], j2 = json_off[2ull * r + 2];
    const long long m0 = (long long)jl[2ull * k], m1 = (long long)jl[2ull * k + 1];
    uint8_t *o = out + loff[k];
    uint8_t *pa = o + nd + 1, *pj0 = pa + la + 1, *pj1 = pj0 + m0 + 1, *pb = pj1 + m1 + 1;
    if (tid == 0) {
        unsigned long long u = stamp_abs(v);
        uint8_t *p = o + nd;
        do { *--p = (uint8_t)('0' + u % 10ull); u /= 10ull; } while (u);
        if (v < 0) *--p = '-';
        o[nd] = ',';
        pa[la] = ',';
        pj0[m0] = ',';
        pj1[m1] = ',';
        pb[lb] = '\n';
    }
    if (wv == 0) wave_put(pj0, json + j0, j1 - j0, m0 != j1 - j0, lane);
    if (wv == 1) wave_put(pj1, json + j1, j2 - j1, m1 != j2 - j1, lane);
    block_copy(pa, scratch + a0, la);
    block_copy(pb, scratch + b0, lb);
}

static int fit_pinned(kw_rows *h, Buf &b, size_t bytes)
{
    return ensure_pinned(h, &b.p, &b.cap, bytes, std::max<size_t>(256, bytes + bytes / 4));
}

static int emit_state(kw_rows *h)
{
    if (h->emit) return KW_OK;
    KWCHK(h, hipSetDevice(h->device));
    Emit *E = new Emit();
    h->emit = E;
    KWCHK(h, hipMalloc((void **)&E->tot, E_WORDS * 8));
    for (auto &e : E->ev) KWCHK(h, hipEventCreate(&e));
    return KW_OK;
}

void emit_destroy(kw_rows *h)
{
    Emit *E = h->emit;
    if (!E) return;
    Buf *bufs[] = {&E->c_buf, &E->c_off, &E->c_fl, &E->stamps, &E->tcnt, &E->tcur, &E->seg, &E->ord, &E->used, &E->dfl,
                   &E->slen, &E->cq, &E->llen, &E->jl, &E->flags, &E->o_doc, &E->o_ti, &E->o_stamp, &E->scratch, &E->out};
    for (Buf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    Buf *pins[] = {&E->p_out, &E->p_off, &E->p_flags, &E->p_doc, &E->p_ti, &E->p_stamp};
    for (Buf *p : pins)
        if (p->p) (void)hipHostFree(p->p);
    if (E->tot) (void)hipFree(E->tot);
    for (auto &e : E->ev)
        if (e) (void)hipEventDestroy(e);
    delete E;
    h->emit = nullptr;
}

}  // namespace rw

extern "C" int kw_rows_cells(kw_rows *h, const uint8_t *cells, const int64_t *coff, const uint8_t *cfl, int64_t n_docs,
                             int32_t ncols, void *stream)
{
    using namespace rw;
    if (!h) return KW_EINVAL;
    if (h->emit) h->emit->cells_docs = -1;
    if (!coff || n_docs < 0 || ncols < 1 || n_docs >= (int64_t)1 << 31 || (n_docs > 0 && !cfl)) {
        h->err = "kw_rows_cells: bad arguments";
        return KW_EINVAL;
    }
    const int64_t nc = n_docs * ncols;
    if (nc >= (int64_t)1 << 34) { h->err = "kw_rows_cells: 2^34 cells or more"; return KW_EINVAL; }
    if (coff[0] < 0) { h->err = "kw_rows_cells: a negative offset"; return KW_EINVAL; }
    for (int64_t i = 0; i < nc; ++i)       // every later read of the cell bytes is inside [0, coff[nc])
        if (coff[i + 1] < coff[i]) { h->err = "kw_rows_cells: offsets decrease at cell " + std::to_string(i); return KW_EINVAL; }
    const int64_t nb = coff[nc];
    if (nb > 0 && !cells) { h->err = "kw_rows_cells: bad arguments"; return KW_EINVAL; }
    int rc;
    if ((rc = emit_state(h))) return rc;
    Emit *E = h->emit;
    hipStream_t st = (hipStream_t)stream;
    KWCHK(h, hipSetDevice(h->device));
    if ((rc = fit(h, E->c_buf, (size_t)nb)) || (rc = fit(h, E->c_off, (size_t)(nc + 1) * 8)) ||
        (rc = fit(h, E->c_fl, (size_t)nc)))
        return rc;
    if (nb) KWCHK(h, hipMemcpyAsync(E->c_buf.p, cells, (size_t)nb, hipMemcpyHostToDevice, st));
    KWCHK(h, hipMemcpyAsync(E->c_off.p, coff, (size_t)(nc + 1) * 8, hipMemcpyHostToDevice, st));
    if (nc) KWCHK(h, hipMemcpyAsync(E->c_fl.p, cfl, (size_t)nc, hipMemcpyHostToDevice, st));
    KWCHK(h, hipStreamSynchronize(st));    // the caller's arrays are free again
    E->cells_docs = n_docs;
    E->ncols = ncols;
    E->borrowed = false;
    return KW_OK;
}

namespace rw {

// kw_rows_cells' offset checks on device-resident offsets: bad[0] = 1 + the first cell whose offsets decrease
// (1 + nc for a negative coff[0]), 0 when they are in order
__global__ __launch_bounds__(BLOCK) void em_coff_check_kernel(const int64_t *__restrict__ coff, uint64_t nc,
                                                              unsigned long long *__restrict__ bad)
{
    if (blockIdx.x == 0 && threadIdx.x == 0 && coff[0] < 0) atomicMax(bad, (unsigned long long)nc + 1ull);
    for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < nc; i += (uint64_t)gridDim.x * BLOCK)
        if (coff[i + 1] < coff[i]) atomicMax(bad, (unsigned long long)(nc - i));   // (max of nc - i: the first such cell)
}

}  // namespace rw

extern "C" int kw_rows_cells_device(kw_rows *h, const uint8_t *d_cells, const int64_t *d_coff, const uint8_t *d_cfl,
                                    int64_t n_docs, int32_t ncols, void *stream)
{
    using namespace rw;
    if (!h) return KW_EINVAL;
    if (h->emit) h->emit->cells_docs = -1;
    if (!d_coff || n_docs < 0 || ncols < 1 || n_docs >= (int64_t)1 << 31 || (n_docs > 0 && (!d_cfl || !d_cells))) {
        h->err = "kw_rows_cells_device: bad arguments";
        return KW_EINVAL;
    }
    const int64_t nc = n_docs * ncols;
    if (nc >= (int64_t)1 << 34) { h->err = "kw_rows_cells_device: 2^34 cells or more"; return KW_EINVAL; }
    int rc;
    if ((rc = emit_state(h))) return rc;
    Emit *E = h->emit;
    hipStream_t st = (hipStream_t)stream;
    KWCHK(h, hipSetDevice(h->device));
    // every later read of the cell bytes must lie inside [0, coff[nc]): the offsets are checked where they are
    unsigned long long bad = 0;
    KWCHK(h, hipMemsetAsync(E->tot, 0, 8, st));
    const uint64_t blocks = ((uint64_t)nc + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(em_coff_check_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks))), dim3(BLOCK),
                       0, st, d_coff, (uint64_t)nc, E->tot);
    KWCHK(h, hipMemcpyAsync(&bad, E->tot, 8, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    if (bad == (unsigned long long)nc + 1ull) { h->err = "kw_rows_cells_device: a negative offset"; return KW_EINVAL; }
    if (bad) {
        h->err = "kw_rows_cells_device: offsets decrease at cell " + std::to_string((unsigned long long)nc - bad);
        return KW_EINVAL;
    }
    E->b_cells = d_cells;
    E->b_coff = d_coff;
    E->b_cfl = d_cfl;
    E->cells_docs = n_docs;
    E->ncols = ncols;
    E->borrowed = true;
    return KW_OK;
}

// kw_rows_emit (stamp_by_doc: a host array, uploaded) and kw_rows_emit_stamps_device (d_stamp_by_doc: borrowed)
static int emit_rows(const char *who, kw_rows *h, const int32_t *cols, const int64_t *stamp_by_doc, const int64_t *d_stamp_by_doc,
                     int64_t n_docs, int64_t n_rows_use, int64_t *n_out_bytes, int32_t *verdict, void *stream)
{
    using namespace rw;
    typedef unsigned long long u64;
    if (!h) return KW_EINVAL;
    if (h->emit) h->emit->have = false;
    if (!cols || !n_out_bytes || !verdict || (n_docs > 0 && !stamp_by_doc && !d_stamp_by_doc)) {
        h->err = std::string(who) + ": bad arguments";
        return KW_EINVAL;
    }
    *n_out_bytes = 0;
    *verdict = KW_EMIT_OK;
    Emit *E = h->emit;
    if (!h->have_run || !h->run_rows) { h->err = std::string(who) + ": no run that left rows"; return KW_ESTATE; }
    if (!E || E->cells_docs < 0) { h->err = std::string(who) + ": no cells (kw_rows_cells)"; return KW_ESTATE; }
    if (n_docs != h->run_docs || n_docs != E->cells_docs) {
        h->err = std::string(who) + ": n_docs differs from the run's or the cells'";
        return KW_ESTATE;
    }
    for (int c = 0; c < 6; ++c)
        if (cols[c] < 0 || cols[c] >= E->ncols) { h->err = std::string(who) + ": a column index outside the cells"; return KW_EINVAL; }
    if (n_rows_use < 0 || n_rows_use > h->n_rows) { h->err = std::string(who) + ": n_rows_use outside [0, n_rows]"; return KW_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    KWCHK(h, hipSetDevice(h->device));
    for (auto &m : E->ms) m = 0.f;
    const uint32_t nu = (uint32_t)n_rows_use, nd = (uint32_t)n_docs, nt = (uint32_t)h->n_tickers;
    int rc;
    if ((rc = fit_pinned(h, E->p_out, 1)) || (rc = fit_pinned(h, E->p_off, ((size_t)nu + 1) * 8)) ||
        (rc = fit_pinned(h, E->p_flags, (size_t)nu * 4)) || (rc = fit_pinned(h, E->p_doc, (size_t)nu * 4)) ||
        (rc = fit_pinned(h, E->p_ti, (size_t)nu * 4)) || (rc = fit_pinned(h, E->p_stamp, (size_t)nu * 8)))
        return rc;
    ((int64_t *)E->p_off.p)[0] = 0;
    if (nu == 0) {
        E->have = true;
        return KW_OK;
    }
    const size_t ncell = (size_t)nd * 6;
    if ((!d_stamp_by_doc && (rc = fit(h, E->stamps, (size_t)nd * 8))) || (rc = fit(h, E->tcnt, ((size_t)nt + 1) * 8)) ||
        (rc = fit(h, E->tcur, (size_t)nt * 4)) || (rc = fit(h, E->seg, (size_t)nu * 4)) ||
        (rc = fit(h, E->ord, (size_t)nu * 4)) || (rc = fit(h, E->used, nd)) ||
        (rc = fit(h, E->dfl, (size_t)nd * 4)) || (rc = fit(h, E->slen, (ncell + 1) * 8)) ||
        (rc = fit(h, E->cq, ncell)) || (rc = fit(h, E->llen, ((size_t)nu + 1) * 8)) ||
        (rc = fit(h, E->jl, (size_t)nu * 16)) || (rc = fit(h, E->flags, (size_t)nu * 4)) ||
        (rc = fit(h, E->o_doc, (size_t)nu * 4)) || (rc = fit(h, E->o_ti, (size_t)nu * 4)) ||
        (rc = fit(h, E->o_stamp, (size_t)nu * 8)))
        return rc;
    Cols C;
    for (int c = 0; c < 6; ++c) C.c[c] = cols[c];
    const int32_t *row_doc = (const int32_t *)h->row_doc.p, *row_ti = (const int32_t *)h->row_ti.p;
    const uint8_t *json = (const uint8_t *)h->json.p;
    const int64_t *json_off = (const int64_t *)h->json_off.p;
    const uint8_t *cbuf = E->borrowed ? E->b_cells : (const uint8_t *)E->c_buf.p;
    const uint8_t *cfl = E->borrowed ? E->b_cfl : (const uint8_t *)E->c_fl.p;
    const int64_t *coff = E->borrowed ? E->b_coff : (const int64_t *)E->c_off.p;
    const int64_t *stamps = d_stamp_by_doc ? d_stamp_by_doc : (const int64_t *)E->stamps.p;
    u64 *tcnt = (u64 *)E->tcnt.p, *slen = (u64 *)E->slen.p, *llen = (u64 *)E->llen.p, *jl = (u64 *)E->jl.p;
    uint32_t *seg = (uint32_t *)E->seg.p, *ord = (uint32_t *)E->ord.p, *dfl = (uint32_t *)E->dfl.p;
    uint8_t *used = (uint8_t *)E->used.p, *cq = (uint8_t *)E->cq.p;

    KWCHK(h, hipEventRecord(E->ev[0], st));
    if (!d_stamp_by_doc) KWCHK(h, hipMemcpyAsync(E->stamps.p, stamp_by_doc, (size_t)nd * 8, hipMemcpyHostToDevice, st));
    KWCHK(h, hipMemsetAsync(E->tot, 0, E_WORDS * 8, st));
    KWCHK(h, hipMemsetAsync(tcnt, 0, ((size_t)nt + 1) * 8, st));
    if (nt) KWCHK(h, hipMemsetAsync(E->tcur.p, 0, (size_t)nt * 4, st));
    KWCHK(h, hipMemsetAsync(seg, 0xFF, (size_t)nu * 4, st));
    KWCHK(h, hipMemsetAsync(used, 0, nd, st));
    KWCHK(h, hipMemsetAsync(dfl, 0, (size_t)nd * 4, st));
    KWCHK(h, hipMemsetAsync(slen, 0, (ncell + 1) * 8, st));
    KWCHK(h, hipMemsetAsync(llen, 0, ((size_t)nu + 1) * 8, st));
    KWCHK(h, hipMemsetAsync(jl, 0, (size_t)nu * 16, st));
    KWCHK(h, hipMemsetAsync(E->flags.p, 0, (size_t)nu * 4, st));
    KWCHK(h, hipMemsetAsync(E->o_doc.p, 0, (size_t)nu * 4, st));
    KWCHK(h, hipMemsetAsync(E->o_ti.p, 0, (size_t)nu * 4, st));
    KWCHK(h, hipMemsetAsync(E->o_stamp.p, 0, (size_t)nu * 8, st));
    // order
    hipLaunchKernelGGL(em_count_kernel, grid_of(nu), dim3(BLOCK), 0, st, row_ti, nu, nt, tcnt, E->tot);
    scan_launch(tcnt, (int64_t)nt + 1, h->chunk, E->tot + E_TROWS, st);
    hipLaunchKernelGGL(em_scatter_kernel, grid_of(nu), dim3(BLOCK), 0, st, row_ti, row_doc, nu, nt, nd, (const u64 *)tcnt,
                       (uint32_t *)E->tcur.p, seg, used, E->tot);
    hipLaunchKernelGGL(em_sort_kernel, grid_of(nu), dim3(BLOCK), 0, st, (const uint32_t *)seg, nu, row_ti, row_doc,
                       (const u64 *)tcnt, stamps, ord, (int32_t *)E->o_doc.p, (int32_t *)E->o_ti.p, (int64_t *)E->o_stamp.p);
    KWCHK(h, hipEventRecord(E->ev[1], st));
    // measure
    hipLaunchKernelGGL(em_measure_kernel, grid_of((uint64_t)ncell * 64), dim3(BLOCK), 0, st, cbuf, coff, cfl, E->ncols, C, nd,
                       (const uint8_t *)used, slen, cq, dfl, E->tot);
    scan_launch(slen, (int64_t)ncell + 1, h->chunk, E->tot + E_SCRATCH, st);
    hipLaunchKernelGGL(em_rowlen_kernel, grid_of((uint64_t)nu * 64), dim3(BLOCK), 0, st, (const uint32_t *)ord, nu, nd, row_doc,
                       stamps, (const u64 *)slen, (const uint32_t *)dfl, json, json_off, llen, jl, (uint32_t *)E->flags.p,
                       E->tot);
    scan_launch(llen, (int64_t)nu + 1, h->chunk, E->tot + E_BYTES, st);
    KWCHK(h, hipEventRecord(E->ev[2], st));
    u64 tot[E_WORDS];
    KWCHK(h, hipMemcpyAsync(tot, E->tot, sizeof(tot), hipMemcpyDeviceToHost, st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    if (tot[E_BAD]) { h->err = std::string(who) + ": a row's ticker or document is beyond the tables"; return KW_EINVAL; }
    for (int k = 0; k < 2; ++k) KWCHK(h, hipEventElapsedTime(&E->ms[k], E->ev[k], E->ev[k + 1]));
    if (tot[E_NUL]) {
        *verdict = KW_EMIT_NUL;
        E->have = true;
        return KW_OK;
    }
    const u64 nbytes = tot[E_BYTES];
    if ((rc = fit(h, E->scratch, (size_t)tot[E_SCRATCH] + SCRATCH_PAD)) || (rc = fit(h, E->out, (size_t)nbytes)) ||
        (rc = fit_pinned(h, E->p_out, (size_t)nbytes)))
        return rc;
    // fill (timed from here: the buffers above may just have grown)
    KWCHK(h, hipEventRecord(E->ev[5], st));
    hipLaunchKernelGGL(em_render_kernel, grid_of((uint64_t)ncell * 64), dim3(BLOCK), 0, st, cbuf, coff, cfl, E->ncols, C, nd,
                       (const uint8_t *)used, (const u64 *)slen, (const uint8_t *)cq, (uint8_t *)E->scratch.p);
    hipLaunchKernelGGL(em_fill_kernel, dim3(nu), dim3(BLOCK), 0, st, (const uint32_t *)ord, nu, nd, row_doc, stamps,
                       (const u64 *)slen, (const uint8_t *)E->scratch.p, json, json_off, (const u64 *)jl, (const u64 *)llen,
                       (uint8_t *)E->out.p);
    KWCHK(h, hipEventRecord(E->ev[3], st));
    // copy
    KWCHK(h, hipMemcpyAsync(E->p_out.p, E->out.p, (size_t)nbytes, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipMemcpyAsync(E->p_off.p, llen, ((size_t)nu + 1) * 8, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipMemcpyAsync(E->p_flags.p, E->flags.p, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipMemcpyAsync(E->p_doc.p, E->o_doc.p, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipMemcpyAsync(E->p_ti.p, E->o_ti.p, (size_t)nu * 4, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipMemcpyAsync(E->p_stamp.p, E->o_stamp.p, (size_t)nu * 8, hipMemcpyDeviceToHost, st));
    KWCHK(h, hipEventRecord(E->ev[4], st));
    KWCHK(h, hipStreamSynchronize(st));
    KWCHK(h, hipGetLastError());
    KWCHK(h, hipEventElapsedTime(&E->ms[2], E->ev[5], E->ev[3]));
    KWCHK(h, hipEventElapsedTime(&E->ms[3], E->ev[3], E->ev[4]));
    *n_out_bytes = (int64_t)nbytes;
    E->have = true;
    return KW_OK;
}

extern "C" int kw_rows_emit(kw_rows *h, const int32_t *cols, const int64_t *stamp_by_doc, int64_t n_docs,
                            int64_t n_rows_use, int64_t *n_out_bytes, int32_t *verdict, void *stream)
{
    return emit_rows("kw_rows_emit", h, cols, stamp_by_doc, nullptr, n_docs, n_rows_use, n_out_bytes, verdict, stream);
}

extern "C" int kw_rows_emit_stamps_device(kw_rows *h, const int32_t *cols, const int64_t *d_stamp_by_doc, int64_t n_docs,
                                          int64_t n_rows_use, int64_t *n_out_bytes, int32_t *verdict, void *stream)
{
    return emit_rows("kw_rows_emit_stamps_device", h, cols, nullptr, d_stamp_by_doc, n_docs, n_rows_use, n_out_bytes, verdict, stream);
}

extern "C" int kw_rows_emit_result(kw_rows *h, const uint8_t **out, const int64_t **line_off, const uint32_t **flags,
                                   const int32_t **row_doc, const int32_t **row_ti, const int64_t **stamps)
{
    if (!h) return KW_EINVAL;
    if (!out || !line_off || !flags || !row_doc || !row_ti || !stamps) {
        h->err = "kw_rows_emit_result: bad arguments";
        return KW_EINVAL;
    }
    rw::Emit *E = h->emit;
    if (!E || !E->have) { h->err = "kw_rows_emit_result: no emit"; return KW_ESTATE; }
    *out = (const uint8_t *)E->p_out.p;
    *line_off = (const int64_t *)E->p_off.p;
    *flags = (const uint32_t *)E->p_flags.p;
    *row_doc = (const int32_t *)E->p_doc.p;
    *row_ti = (const int32_t *)E->p_ti.p;
    *stamps = (const int64_t *)E->p_stamp.p;
    return KW_OK;
}

extern "C" int kw_rows_copy_index(kw_rows *h, int32_t *row_doc, int32_t *row_ti)
{
    if (!h) return KW_EINVAL;
    if (!h->have_run) { h->err = "kw_rows_copy_index: no run"; return KW_ESTATE; }
    if (h->n_rows > 0 && (!row_doc || !row_ti)) { h->err = "kw_rows_copy_index: bad arguments"; return KW_EINVAL; }
    if (h->n_rows == 0) return KW_OK;
    KWCHK(h, hipSetDevice(h->device));
    KWCHK(h, hipMemcpy(row_doc, h->row_doc.p, (size_t)h->n_rows * 4, hipMemcpyDeviceToHost));
    KWCHK(h, hipMemcpy(row_ti, h->row_ti.p, (size_t)h->n_rows * 4, hipMemcpyDeviceToHost));
    return KW_OK;
}

extern "C" int kw_rows_emit_last_ms(kw_rows *h, float *ms, int32_t n)
{
    if (!h || !ms || n < 0) return KW_EINVAL;
    if (!h->emit || !h->emit->have) { h->err = "kw_rows_emit_last_ms: no emit"; return KW_ESTATE; }
    for (int32_t k = 0; k < n && k < 4; ++k) ms[k] = h->emit->ms[k];
    return KW_OK;
}
