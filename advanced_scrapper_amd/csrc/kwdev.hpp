// libkwmatch: the device primitives the handles beside the matcher share (kwingest, kwsort, cdx, dedup, kwemit).
// The library is built without relocatable device code, so everything here is inline in the unit that calls it; a
// shared __global__ kernel lives in one unit behind a host launcher instead (kwscan.hip, declared in kwhandle.hpp).
// The matcher's own wave helpers (kwmatch*.hpp) are shaped by its hot path and are not these.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace kwd {

constexpr int BLOCK = 256;           // threads of every block that calls block_scan
constexpr int TILE = BLOCK * 16;     // bytes of text a block classifies at once
constexpr unsigned long long NONE = ~0ull;

__device__ __forceinline__ uint32_t eq4(uint32_t v, uint32_t pat)   // 0x80 in exactly the bytes equal to pat's
{
    const uint32_t d = v ^ pat;
    return ~(((d & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | d) & 0x80808080u;
}
__device__ __forceinline__ uint32_t bits4(uint32_t m) { return (((m >> 7) & 0x01010101u) * 0x01020408u) >> 24; }
__device__ __forceinline__ uint32_t mask16(uint4 v, uint32_t c)     // bit k set iff byte k of the 16 equals c
{
    const uint32_t pat = c * 0x01010101u;
    return bits4(eq4(v.x, pat)) | (bits4(eq4(v.y, pat)) << 4) | (bits4(eq4(v.z, pat)) << 8) | (bits4(eq4(v.w, pat)) << 12);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long x)
{
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long y = __shfl_xor(x, d, 64);
        x = y < x ? y : x;
    }
    return x;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long x)
{
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}

// exclusive scan of one value a thread over a block of BLOCK; *total: the block's sum (ws: BLOCK / 64 words of LDS)
__device__ __forceinline__ unsigned long long block_scan(unsigned long long x, unsigned long long *ws,
                                                         unsigned long long *total)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    unsigned long long inc = x;
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long y = __shfl_up(inc, d, 64);
        if (lane >= d) inc += y;
    }
    __syncthreads();   // ws free again
    if (lane == 63) ws[wv] = inc;
    __syncthreads();
    unsigned long long before = 0, all = 0;
    for (int k = 0; k < BLOCK / 64; ++k) {
        const unsigned long long s = ws[k];
        if (k < wv) before += s;
        all += s;
    }
    *total = all;
    return before + inc - x;
}

// s[0, m) equals lit (lower case) without regard to ASCII case
__device__ __forceinline__ bool ieq(const uint8_t *__restrict__ s, long long m, const char *lit, int len)
{
    if (m != len) return false;
    for (int i = 0; i < len; ++i) {
        uint8_t c = s[i];
        if (c >= 'A' && c <= 'Z') c = (uint8_t)(c + 32);
        if (c != (uint8_t)lit[i]) return false;
    }
    return true;
}

// The first byte a strict UTF-8 decoder stops at among the code points that start in [p, p + 16): from the code
// point boundary at or before p (a continuation byte at p belongs to a lead at most 3 bytes back; four continuation
// bytes in a row hold an error at or before p, which its own lane reports).  Not forced inline: the quote kernels
// call it from the few lanes that hold a byte >= 0x80.
inline __device__ unsigned long long utf8_lane(const uint8_t *__restrict__ text, long long n, long long p)
{
    long long q = p;
    if ((text[p] & 0xC0u) == 0x80u) {
        int back = 1;
        while (back <= 3 && p - back >= 0 && (text[p - back] & 0xC0u) == 0x80u) ++back;
        if (back > 3 || p - back < 0) return (unsigned long long)p;
        q = p - back;
    }
    const long long stop = p + 16 < n ? p + 16 : n;
    while (q < stop) {
        const uint32_t c = text[q];
        if (c < 0x80u) { ++q; continue; }
        int need;
        uint32_t lo = 0x80u, hi = 0xBFu;
        if (c >= 0xC2u && c <= 0xDFu) need = 1;
        else if (c == 0xE0u) { need = 2; lo = 0xA0u; }
        else if (c == 0xEDu) { need = 2; hi = 0x9Fu; }
        else if (c >= 0xE1u && c <= 0xEFu) need = 2;
        else if (c == 0xF0u) { need = 3; lo = 0x90u; }
        else if (c >= 0xF1u && c <= 0xF3u) need = 3;
        else if (c == 0xF4u) { need = 3; hi = 0x8Fu; }
        else return (unsigned long long)q;
        for (int k = 1; k <= need; ++k) {
            if (q + k >= n) return (unsigned long long)q;
            const uint32_t b = text[q + k];
            if (b < lo || b > hi) return (unsigned long long)q;
            lo = 0x80u; hi = 0xBFu;
        }
        q += need + 1;
    }
    return NONE;
}

// The body of a quote-count kernel over tiles of TILE bytes: a tile's '"' bytes to tile_q[tile] (their exclusive scan
// over the tiles carries the quote parity into every tile); the first NUL and the first byte a strict UTF-8 decoder
// stops at by atomicMin into *first_nul and *first_utf8.  The text is readable up to the next multiple of 16 past n.
__device__ __forceinline__ void quotes_tiles(const uint8_t *__restrict__ text, long long n, long long ntiles,
                                             unsigned long long *__restrict__ tile_q, unsigned long long *first_nul,
                                             unsigned long long *first_utf8)
{
    __shared__ unsigned long long ws[BLOCK / 64];
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long p = tile * TILE + (long long)threadIdx.x * 16;
        uint32_t q = 0;
        unsigned long long ez = NONE, e8 = NONE;
        if (p < n) {
            const uint4 v = *(const uint4 *)(text + p);
            const uint32_t valid = n - p >= 16 ? 0xFFFFu : (1u << (int)(n - p)) - 1u;
            q = mask16(v, 0x22u) & valid;
            const uint32_t z = mask16(v, 0u) & valid;
            const uint32_t hb = (bits4(v.x & 0x80808080u) | (bits4(v.y & 0x80808080u) << 4) |
                                 (bits4(v.z & 0x80808080u) << 8) | (bits4(v.w & 0x80808080u) << 12)) & valid;
            if (z) ez = (unsigned long long)p + __builtin_ctz(z);
            if (hb) e8 = utf8_lane(text, n, p);
        }
        if (__any((ez & e8) != NONE)) {   // (rare: one atomic a wave and condition)
            ez = wave_min(ez);
            e8 = wave_min(e8);
            if ((threadIdx.x & 63) == 0) {
                if (ez != NONE) atomicMin(first_nul, ez);
                if (e8 != NONE) atomicMin(first_utf8, e8);
            }
        }
        unsigned long long total;
        (void)block_scan((unsigned long long)__popc(q), ws, &total);
        if (threadIdx.x == 0) tile_q[tile] = total;
    }
}

}  // namespace kwd
