// The patch lattice of an (H, W) slide under patch size p (slide.hip, classmap.hip): ceil(H / p) rows of n_w = ceil(W / p) patches,
// patch k (row-major) with its corner at (k / n_w * p, k % n_w * p).
#pragma once

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
