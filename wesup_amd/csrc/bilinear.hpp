// Bilinear interpolation with align_corners=True: the one statement of the source coordinates, shared by every kernel that
// resamples (spatial.hip: side outputs; pixel.hip: images, probability planes, the per-resolution fc maps; slide.hip: patches).
// At the end of the file: the align_corners=False ("half pixel") coordinates of F.interpolate's default, for slide.hip.
#pragma once
#include "common.hpp"

// torch: scale = (in-1)/(out-1) (float); src = scale*dst; i0 = min(int(src), in-1); i1 = i0 + (i0 < in-1);
// l1 = clamp(src - i0, 0, 1); l0 = 1 - l1.
struct Lerp {
    int i0, i1;
    float l0, l1;
};
__device__ __forceinline__ Lerp lerp_of(int dst, float scale, int in) {
    // torch rounds the product before it takes the fraction: no contraction of it into the subtraction below (an fma there
    // moves l1 by up to half an ulp of src, 2e-6 at src = 36)
#pragma clang fp contract(off)
    Lerp r;
    const float src = scale * (float)dst;
    r.i0 = min((int)src, in - 1);
    r.i1 = r.i0 + ((r.i0 < in - 1) ? 1 : 0);
    r.l1 = fminf(fmaxf(src - (float)r.i0, 0.f), 1.f);
    r.l0 = 1.f - r.l1;
    return r;
}
static inline float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

// torch with align_corners=False: scale = in/out (float); src = max(scale*(dst + 0.5) - 0.5, 0); the rest as above
// (area_pixel_compute_source_index + compute_source_index_and_lambda).  At in == out src is dst exactly: l1 = 0.
__device__ __forceinline__ Lerp lerp_half_pixel(int dst, float scale, int in) {
#pragma clang fp contract(off)
    Lerp r;
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
    r.i0 = min((int)src, in - 1);
    r.i1 = r.i0 + ((r.i0 < in - 1) ? 1 : 0);
    r.l1 = fminf(fmaxf(src - (float)r.i0, 0.f), 1.f);
    r.l0 = 1.f - r.l1;
    return r;
}
static inline float hp_scale(int in, int out) { return (float)in / (float)out; }
