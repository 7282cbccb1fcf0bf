// libkwmatch: the host plumbing the handles beside the matcher share (kw_ingest, kw_sort, kw_dedup with its CDX
// store, kw_rows with its emitter): the HIP error check, buffers that grow, test overrides in a range, launch grids,
// and the one device scan (kwscan.hip).  `h` is any handle with a `std::string err`.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/kwmatch.h"
#include "kwenv.hpp"

#define KWCHK(h, x)                                                                    \
    do {                                                                               \
        hipError_t e_ = (x);                                                           \
        if (e_ != hipSuccess) {                                                        \
            (h)->err = std::string("HIP error ") + hipGetErrorString(e_) + " at " #x; \
            return KW_EHIP;                                                            \
        }                                                                              \
    } while (0)

namespace kwh {

struct Buf {
    void *p = nullptr;
    size_t cap = 0;
};

// A device buffer of at least `bytes`; one that has to grow is allocated anew with `want` bytes (the handle's own
// growth rule, want >= bytes) and its contents are not kept.
template <class H>
int ensure(H *h, void **p, size_t *cap, size_t bytes, size_t want)
{
    if (*cap >= bytes && *p) return KW_OK;
    if (*p) (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    KWCHK(h, hipMalloc(p, want));
    *cap = want;
    return KW_OK;
}
template <class H>
int ensure(H *h, Buf &b, size_t bytes, size_t want) { return ensure(h, &b.p, &b.cap, bytes, want); }

// The same for a buffer that keeps its first `keep` bytes when it grows; with zero_rest what it holds beyond them
// is zero.  The old buffer is freed after the stream has made the copy.
template <class H>
int ensure_keep(H *h, void **p, size_t *cap, size_t bytes, size_t keep, size_t want, bool zero_rest, hipStream_t st)
{
    if (*cap >= bytes && *p) return KW_OK;
    void *np = nullptr;
    KWCHK(h, hipMalloc(&np, want));
    if (keep > *cap) keep = *cap;
    const bool copy = *p && keep;
    hipError_t e = hipSuccess;
    if (copy) e = hipMemcpyAsync(np, *p, keep, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && zero_rest) e = hipMemsetAsync((uint8_t *)np + keep, 0, want - keep, st);
    if (e == hipSuccess && (copy || zero_rest)) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipFree(np);
        KWCHK(h, e);
    }
    if (*p) (void)hipFree(*p);
    *p = np;
    *cap = want;
    return KW_OK;
}
template <class H>
int ensure_keep(H *h, Buf &b, size_t bytes, size_t keep, size_t want, bool zero_rest, hipStream_t st)
{
    return ensure_keep(h, &b.p, &b.cap, bytes, keep, want, zero_rest, st);
}

// a pinned host buffer of at least `bytes` (contents are not kept when it grows)
template <class H>
int ensure_pinned(H *h, void **p, size_t *cap, size_t bytes, size_t want)
{
    if (*cap >= bytes && *p) return KW_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    KWCHK(h, hipHostMalloc(p, want, hipHostMallocDefault));
    *cap = want;
    return KW_OK;
}

// the integer `name` holds in [lo, hi] (read per call through kw_env: the tests' and developers' gate), else fallback
static inline long long env_int(const char *name, long long lo, long long hi, long long fallback)
{
    if (const char *e = kw_env(name)) {
        char *end = nullptr;
        const long long v = strtoll(e, &end, 10);
        if (end != e && *end == '\0' && v >= lo && v <= hi) return v;
    }
    return fallback;
}

// blocks of `block` threads for `items` lanes: at least one, at most cap
static inline dim3 grid_for(long long items, int block, long long cap)
{
    long long g = (items + block - 1) / block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return dim3((unsigned)g);
}

static inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// kwscan.hip: the exclusive scan of a[0, m) in place, in two levels; *d_grand (device) receives the total.
// chunk: SCAN_CHUNKS words of device scratch.  Launches three kernels on st and does not synchronise.
constexpr int SCAN_CHUNKS = 512;
void scan_launch(unsigned long long *a, int64_t m, unsigned long long *chunk, unsigned long long *d_grand, hipStream_t st);

}  // namespace kwh
