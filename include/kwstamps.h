/*
 * kwstamps.h -- time_unix of the ISO rule's date rows from the integer date arrays, in any local time zone: the
 * one statement of the rule that the host routine (kwcsv_stamps_local, csrc/kwcsv.c) and the device kernel
 * (ig_stamps_kernel, csrc/kwingest.hip) both compile.  tests/stamps_rule.py restates it in Python; DESIGN.md §7.
 *
 * The zone table: ascending instants at[0..n] and UTC offsets off[0..n-1] in seconds, off[i] valid on
 * [at[i], at[i+1]); 1 <= n <= KWST_CAPACITY.  It answers for instants in [at[0] + KWST_MARGIN, at[n] - KWST_MARGIN)
 * only: a row whose solve probes an instant outside is not native (the caller asks timestamp() itself).  A process
 * in UTC has the one entry (INT64_MIN, INT64_MAX, 0).
 *
 * A naive datetime's timestamp() solves t = local(u) for u, local(u) = u + utcoff(u), t the wall clock read as UTC
 * (CPython's local_to_seconds with fold = 0); kwst_solve is that algorithm over the table.  By kind (kwingest.h):
 *   1   the solved u
 *   4   timestamp() is the double u + frac / 1e6 and int() rounds toward zero: the solved u when the fraction is
 *       zero, or when u >= 0 and the instant's microseconds are below 2^52 (the double then never reaches u + 1)
 *   3   floor(us / 10^6) when the fraction is zero or 0 <= us < 2^52; no table is read
 *   0, 2  never native
 * 64-bit integer arithmetic only.
 */
#ifndef KWSTAMPS_H
#define KWSTAMPS_H

#include <stdint.h>

#ifndef KWST_FN
#define KWST_FN static inline
#endif

#define KWST_CAPACITY 1024
#define KWST_MARGIN 172800            /* two days */
#define KWST_BOUND ((int64_t)1 << 52)

typedef struct {
    const int64_t *at;
    const int32_t *off;
    int32_t n;
    int64_t lo, hi;                   /* at[0] + KWST_MARGIN, at[n] - KWST_MARGIN */
} kwst_zone;

/* utcoff(x) into *o; 0 when x lies outside the table's range.  Ten steps whatever n is: the last i with at[i] <= x. */
KWST_FN int kwst_off(const kwst_zone *z, int64_t x, int64_t *o)
{
    if (x < z->lo || x >= z->hi) return 0;
    int32_t i = 0;
    for (int32_t step = KWST_CAPACITY / 2; step >= 1; step >>= 1)
        if (i + step < z->n && z->at[i + step] <= x) i += step;
    *o = z->off[i];
    return 1;
}

/* t = local(u) solved for u into *u; 0 when a probe leaves the table. */
KWST_FN int kwst_solve(const kwst_zone *z, int64_t t, int64_t *u)
{
    int64_t a, b, o;
    if (!kwst_off(z, t, &a)) return 0;
    const int64_t u1 = t - a;
    if (!kwst_off(z, u1, &o)) return 0;
    const int64_t t1 = u1 + o;
    if (t1 == t) {
        if (!kwst_off(z, u1 - 86400, &b)) return 0;
        if (a == b) { *u = u1; return 1; }
    } else {
        b = t1 - u1;
    }
    const int64_t u2 = t - b;
    if (!kwst_off(z, u2, &o)) return 0;
    if (u2 + o == t) *u = u2;
    else if (t1 == t) *u = u1;
    else *u = u1 > u2 ? u1 : u2;      /* t lies in a gap */
    return 1;
}

/* One row: its time_unix into *stamp (0 when not native); returns native (1 = the value is final). */
KWST_FN int kwst_row(const kwst_zone *z, int64_t us, int kind, int64_t *stamp)
{
    *stamp = 0;
    if (kind != 1 && kind != 3 && kind != 4) return 0;
    int64_t t = us / 1000000;
    int64_t frac = us - t * 1000000;
    if (frac < 0) { --t; frac += 1000000; }
    if (kind == 3) {
        if (frac != 0 && (us < 0 || us >= KWST_BOUND)) return 0;
        *stamp = t;
        return 1;
    }
    int64_t u;
    if (!kwst_solve(z, t, &u)) return 0;
    if (frac != 0 && (u < 0 || u > KWST_BOUND / 1000000 || u * 1000000 + frac >= KWST_BOUND)) return 0;   /* (no overflow) */
    *stamp = u;
    return 1;
}

#endif
