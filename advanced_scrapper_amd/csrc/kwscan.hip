// libkwmatch: the device scan of kwhandle.hpp -- the exclusive scan of m 64-bit counts in place, in two levels:
// chunk c = values [c * per, (c + 1) * per); the chunk sums, their scan in one block, each chunk from its prefix.
// The CDX / CSV store (cdx.hip), the match rows (kwrows.hip) and the emitter (kwemit.hip) size everything with it.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kwdev.hpp"
#include "kwhandle.hpp"

namespace kwd {

__global__ __launch_bounds__(BLOCK) void scan_sums_kernel(const unsigned long long *__restrict__ a, int64_t m,
                                                          int64_t per, unsigned long long *__restrict__ chunk)
{
    __shared__ unsigned long long ws[BLOCK / 64];
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    unsigned long long s = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) s += a[i];
    unsigned long long total;
    (void)block_scan(s, ws, &total);
    if (threadIdx.x == 0) chunk[blockIdx.x] = total;
}

// one block: the chunk sums' exclusive scan in place (nchunk <= SCAN_CHUNKS = 2 * BLOCK), the grand total
__global__ __launch_bounds__(BLOCK) void scan_chunks_kernel(unsigned long long *__restrict__ chunk, int nchunk,
                                                            unsigned long long *__restrict__ grand)
{
    __shared__ unsigned long long ws[BLOCK / 64];
    const int i0 = 2 * (int)threadIdx.x, i1 = i0 + 1;
    const unsigned long long x0 = i0 < nchunk ? chunk[i0] : 0ull, x1 = i1 < nchunk ? chunk[i1] : 0ull;
    unsigned long long total;
    const unsigned long long before = block_scan(x0 + x1, ws, &total);
    if (i0 < nchunk) chunk[i0] = before;
    if (i1 < nchunk) chunk[i1] = before + x0;
    if (threadIdx.x == 0) *grand = total;
}

__global__ __launch_bounds__(BLOCK) void scan_apply_kernel(unsigned long long *__restrict__ a, int64_t m, int64_t per,
                                                           const unsigned long long *__restrict__ chunk)
{
    __shared__ unsigned long long ws[BLOCK / 64];
    const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < m ? lo + per : m;
    unsigned long long carry = chunk[blockIdx.x];
    for (int64_t i0 = lo; i0 < hi; i0 += BLOCK) {   // (block-uniform trip count)
        const int64_t i = i0 + threadIdx.x;
        const unsigned long long x = i < hi ? a[i] : 0ull;
        unsigned long long total;
        const unsigned long long before = block_scan(x, ws, &total);
        if (i < hi) a[i] = carry + before;
        carry += total;
    }
}

}  // namespace kwd

static_assert(kwh::SCAN_CHUNKS == 2 * kwd::BLOCK, "scan_chunks_kernel scans two chunk sums a thread");

void kwh::scan_launch(unsigned long long *a, int64_t m, unsigned long long *chunk, unsigned long long *d_grand,
                      hipStream_t st)
{
    using namespace kwd;
    const int64_t nchunk = std::max<int64_t>(1, std::min<int64_t>(SCAN_CHUNKS, (m + 4 * BLOCK - 1) / (4 * BLOCK)));
    const int64_t per = std::max<int64_t>(1, (m + nchunk - 1) / nchunk);
    hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)nchunk), dim3(BLOCK), 0, st, (const unsigned long long *)a, m,
                       per, chunk);
    hipLaunchKernelGGL(scan_chunks_kernel, dim3(1), dim3(BLOCK), 0, st, chunk, (int)nchunk, d_grand);
    hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nchunk), dim3(BLOCK), 0, st, a, m, per,
                       (const unsigned long long *)chunk);
}
