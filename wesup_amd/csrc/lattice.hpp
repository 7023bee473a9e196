// The two lattices of the inference tools, each index computation stated once.
// The patch lattice of an (H, W) slide under patch size p (slide.hip, classmap.hip): ceil(H / p) rows of n_w = ceil(W / p) patches,
// patch k (row-major) with its corner at (k / n_w * p, k % n_w * p).
// The window lattice of an image (tiles.hip, classmap.hip): sorted corners tops[n_h] x lefts[n_w] in device memory, made by the caller.
#pragma once
#include "common.hpp"

// n_w and the last patch's index; false when a size is outside what the kernels index (include/wesup_hip.h: 1 <= H, W, p <= 2^30
// and fewer than 2^31 patches)
static inline bool sd_lattice(int H, int W, int p, int* n_w, int* last) {
    const int LIM = 1 << 30;
    if (H <= 0 || W <= 0 || p <= 0 || H > LIM || W > LIM || p > LIM) return false;
    const long nh = ((long)H + p - 1) / p, nw = ((long)W + p - 1) / p;
    if (nh * nw > 0x7fffffffl) return false;
    *n_w = (int)nw;
    *last = (int)(nh * nw - 1);
    return true;
}

// Pixel idx of the padded p x p patches first .. first + count - 1 (x fastest, then y, then the patch): n the patch's place in the
// pass, (y, x) inside the patch, (Y, X) in the slide.  skip: the patch lies past the end of the lattice or the pixel beyond the
// slide -- never written.  With a patch list slot first + n names patch list[first + n]: a slot at or beyond
// n_list is skipped, and so is a list value outside [0, last], which sets bad and never becomes an address.
struct PatchPixel {
    int n, y, x;
    long Y, X;
    bool skip, bad;
};
__device__ __forceinline__ PatchPixel patch_pixel(long idx, int p, int first, int n_w, int last, int H, int W,
                                                  const int32_t* __restrict__ list = nullptr, int n_list = 0) {
    const long pp = (long)p * p;
    PatchPixel q;
    q.n = (int)(idx / pp);
    const long r = idx - (long)q.n * pp;
    q.y = (int)(r / p);
    q.x = (int)(r - (long)q.y * p);
    int k = first + q.n;
    bool off = false;
    q.bad = false;
    if (list) {
        off = k >= n_list;
        k = off ? 0 : list[k];
        q.bad = k < 0 || k > last;
        if (q.bad) k = 0;
    }
    const int ky = k / n_w, kx = k - ky * n_w;
    q.Y = (long)ky * p + q.y;
    q.X = (long)kx * p + q.x;
    q.skip = off || q.bad || k > last || q.Y >= H || q.X >= W;
    return q;
}

// The eight views of a square p x p window (infer_tile.apply_view / invert_view): v = r + 4 f, a left-right mirror first when f,
// then r counter-clockwise quarter turns.  A view list comes by value: n_views and one word of four bits per view, the first view
// in the lowest bits.  views_ok: 1 <= n_views <= 8, every index below 8, none twice -- asked on the host, before a launch.
#define WESUP_MAX_VIEWS 8
static inline bool views_ok(int n_views, uint32_t views) {
    if (n_views < 1 || n_views > WESUP_MAX_VIEWS) return false;
    unsigned seen = 0;
    for (int t = 0; t < n_views; ++t) {
        const unsigned v = (views >> (4 * t)) & 15u;
        if (v > 7u || (seen >> v) & 1u) return false;
        seen |= 1u << v;
    }
    return true;
}
__device__ __forceinline__ int view_at(uint32_t views, int t) { return (int)((views >> (4 * t)) & 7u); }

struct ViewPixel {
    int y, x;
};
// forward: the pixel of the upright window that pixel (y, x) of view v shows -- apply_view(a, v)[y][x] = a[s.y][s.x]
__device__ __forceinline__ ViewPixel view_source(int v, int p, int y, int x) {
    const int r = v & 3, m = p - 1;
    ViewPixel s;
    s.y = r == 0 ? y : r == 1 ? x : r == 2 ? m - y : m - x;
    s.x = r == 0 ? x : r == 1 ? m - y : r == 2 ? m - x : y;
    if (v & 4) s.x = m - s.x;
    return s;
}
// inverse: where pixel (y, x) of the upright window lies in view v -- invert_view(b, v)[y][x] = b[q.y][q.x]
__device__ __forceinline__ ViewPixel view_inverse(int v, int p, int y, int x) {
    const int r = v & 3, m = p - 1;
    const int w = (v & 4) ? m - x : x;
    ViewPixel q;
    q.y = r == 0 ? y : r == 1 ? m - w : r == 2 ? m - y : w;
    q.x = r == 0 ? w : r == 1 ? y : r == 2 ? m - w : m - y;
    return q;
}
__device__ __forceinline__ bool view_inside(const ViewPixel q, int p) { return q.y >= 0 && q.y < p && q.x >= 0 && q.x < p; }

// [i0, i1): the windows of one axis of a sorted window lattice that cover pos, 0 <= pos - tops[i] < p; n comparisons.  The caller
// tests every offset again before it makes an address of it (an unsorted lattice gives wrong numbers, never a fault).
struct Covering {
    int i0, i1;
};
__device__ __forceinline__ Covering covering(const int32_t* __restrict__ tops, int n, int pos, int p) {
    Covering r = {n, 0};
    for (int i = 0; i < n; ++i) {
        const int d = pos - tops[i];
        if (d >= 0 && d < p) {
            r.i0 = i < r.i0 ? i : r.i0;
            r.i1 = i + 1;
        }
    }
    return r;
}
