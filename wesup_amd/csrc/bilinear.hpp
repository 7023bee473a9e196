// Bilinear interpolation with align_corners=True: the one statement of the source coordinates, shared by every kernel that
// resamples (spatial.hip: side outputs; pixel.hip: images, probability planes, the per-resolution fc maps; slide.hip: patches).
// Behind them: the align_corners=False ("half pixel") coordinates of F.interpolate's default, for slide.hip.  At the end of the
// file: the blend of the four neighbours, in the two forms whose bits results depend on, and the step into a running mean, each
// rounding written out.
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

// ---- the blend: ly.l0 * (lx.l0 * v00 + lx.l1 * v01) + ly.l1 * (lx.l0 * v10 + lx.l1 * v11), every fused step an explicit fmaf
// and no contraction beyond it, so that the bits are the source's and not a compiler's pick.  The kernels that use one form are
// bit-equal to each other (tests/test_slide_gpu.py) and to a recording (tests/golden/resize_bits.npz); against torch's
// F.interpolate both stay within a few fp32 roundings (tests/test_pixel_resolution_gpu.py).  upsample_fwd_kernel (spatial.hip)
// keeps the plain expression: the compiler fuses its four lanes in two different ways, neither form below.

// An image on its way INTO the network -- to_tensor + F.interpolate(img, size) of pixel_infer.py / the patch resize of
// test_dp2019_pipeline.py: px_image_resize_kernel (pixel.hip), sd_gather_kernel (slide.hip).  Three fused steps.  Also the
// F.interpolate of the fc maps in px_gather_kernel (pixel.hip), which is held to a tolerance only.
__device__ __forceinline__ float blend_image(const Lerp ly, const Lerp lx, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
    const float a = __builtin_fmaf(lx.l0, v00, lx.l1 * v01), b = __builtin_fmaf(lx.l0, v10, lx.l1 * v11);
    return __builtin_fmaf(ly.l0, a, ly.l1 * b);
}
// A prediction plane on its way BACK to the image's size -- F.interpolate(pred[..., 1], size) of pixel_infer.py and of the
// patch stitch: px_plane_resize_kernel (pixel.hip, times alpha), sd_scatter_kernel<1> (slide.hip).  The rows fused, the sum of
// the two rows not.
__device__ __forceinline__ float blend_plane(const Lerp ly, const Lerp lx, float v00, float v01, float v10, float v11) {
#pragma clang fp contract(off)
    const float a = __builtin_fmaf(lx.l1, v01, lx.l0 * v00), b = __builtin_fmaf(lx.l1, v11, lx.l0 * v10);
    return ly.l0 * a + ly.l1 * b;
}
// A plane into the running mean over the scales -- out = (accumulate ? out : 0) + alpha * blend_plane: px_plane_resize_kernel
// (pixel.hip) and every plane of cm_planes_resize_kernel (classmap.hip).  The product by alpha is rounded, and the add onto out is
// a second rounding: no contraction of the two into one fma.
__device__ __forceinline__ float blend_plane_times(const Lerp ly, const Lerp lx, float alpha, float v00, float v01, float v10,
                                                   float v11) {
#pragma clang fp contract(off)
    return alpha * blend_plane(ly, lx, v00, v01, v10, v11);
}
__device__ __forceinline__ float add_rounded_product(float out, float product) {
#pragma clang fp contract(off)
    return out + product;
}
