// The scanline form of the polygon fill for one edge, shared by the kernels of raster.hip and by host code that
// restates them.  Fixed point with 8 fractional bits: pixel (r, c) has its centre at (256 c + 128, 256 r + 128).  All integer.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ __forceinline__
#else
#define RS_HD inline
#endif

// the first centre row (or column) at or behind the coordinate y: ceil((y - 128) / 256)
RS_HD int rs_first_centre(int y) { return (y + 127) >> 8; }

// An edge between the centre rows [ra, rb): q is c* of the current row, the first column it toggles,
//     c* = ceil((N - 128 D) / (256 D)) = floor((N + 128 D - 1) / (256 D)),   N = x0 D + (x1 - x0)(Yc - y0),   D = y1 - y0 > 0,
// kept with its remainder rem in [0, den), den = 256 D.  From one row to the next N grows by 256 (x1 - x0) = sq den + sr with
// sq = floor((x1 - x0) / D) and 0 <= sr < den, so a step is two additions and a carry: no product and no division per row.
// With |coordinate| <= 2^28: D, |x1 - x0| <= 2^29, |N| < 2^59, den <= 2^37, |q| <= 2^20 + 1.
struct RsEdge {
    long long rem, sr, den;
    int ra, rb, q, sq;
};

// false: the edge crosses no centre row of [rlo, rhi) (horizontal edges never do)
RS_HD bool rs_edge_setup(int x0, int y0, int x1, int y1, int rlo, int rhi, RsEdge& e) {
    if (y0 == y1) return false;
    if (y0 > y1) {
        int t = x0; x0 = x1; x1 = t;
        t = y0; y0 = y1; y1 = t;
    }
    const int ra = rs_first_centre(y0), rb = rs_first_centre(y1);          // y0 <= Yc < y1
    e.ra = ra > rlo ? ra : rlo;
    e.rb = rb < rhi ? rb : rhi;
    if (e.ra >= e.rb) return false;
    const long long D = (long long)y1 - y0, dx = (long long)x1 - x0;
    e.den = 256 * D;
    if (dx == 0) {                                                         // c* = ceil((x0 - 128) / 256) on every row
        e.q = rs_first_centre(x0);
        e.rem = 0;
        e.sq = 0;
        e.sr = 0;
        return true;
    }
    const long long Yc = 256ll * e.ra + 128;
    const long long M = (long long)x0 * D + dx * (Yc - y0) + 128 * D - 1;
    long long q = M / e.den, rem = M - q * e.den;
    if (rem < 0) { --q; rem += e.den; }                                    // floor semantics
    long long sq = dx / D;
    if (sq * D > dx) --sq;
    e.q = (int)q;
    e.rem = rem;
    e.sq = (int)sq;
    e.sr = 256 * (dx - sq * D);
    return true;
}

RS_HD void rs_edge_step(RsEdge& e) {
    e.q += e.sq;
    e.rem += e.sr;
    if (e.rem >= e.den) { ++e.q; e.rem -= e.den; }
}
