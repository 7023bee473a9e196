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
// slide -- never written.
struct PatchPixel {
    int n, y, x;
    long Y, X;
    bool skip;
};
__device__ __forceinline__ PatchPixel patch_pixel(long idx, int p, int first, int n_w, int last, int H, int W) {
    const long pp = (long)p * p;
    PatchPixel q;
    q.n = (int)(idx / pp);
    const long r = idx - (long)q.n * pp;
    q.y = (int)(r / p);
    q.x = (int)(r - (long)q.y * p);
    const int k = first + q.n;
    const int ky = k / n_w, kx = k - ky * n_w;
    q.Y = (long)ky * p + q.y;
    q.X = (long)kx * p + q.x;
    q.skip = k > last || q.Y >= H || q.X >= W;
    return q;
}

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
