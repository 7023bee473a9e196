// Whole-image multi-scale pixel inference: the two resizes at the ends of a scale -- uint8 image down to the
// network input, class-1 probability back up and into the mean over the scales -- and the gather that makes the first fc
// layer's output from per-resolution products.  All three are memory movement with a few multiply-adds per element: no LDS,
// no atomics, no workspace, deterministic.  Coordinates (lerp_of / ac_scale) and blends (blend_image, blend_plane): bilinear.hpp.
#include "common.hpp"
#include "bilinear.hpp"

#define PX_BLOCK 256
#define PX_MAX_BLOCKS 4096     // grid-stride above this (cdna_hip_programming.md, guideline 11)

namespace {

// out[c][y][x] = bilinear_ac(img[.][.][c] / 255.f)(y, x): to_tensor followed by F.interpolate.  One thread per output pixel and
// all three planes (the 12 bytes of its four corners sit in two short runs); stores of neighbouring lanes are neighbours.
__global__ __launch_bounds__(PX_BLOCK) void px_image_resize_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int H,
                                                                   int W, int h, int w, float sh, float sw) {
    const long total = (long)h * w;
    for (long idx = (long)blockIdx.x * PX_BLOCK + threadIdx.x; idx < total; idx += (long)gridDim.x * PX_BLOCK) {
        const int y = (int)(idx / w), x = (int)(idx - (long)y * w);
        const Lerp ly = lerp_of(y, sh, H), lx = lerp_of(x, sw, W);
        const uint8_t* r0 = img + (long)ly.i0 * W * 3;
        const uint8_t* r1 = img + (long)ly.i1 * W * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v00 = (float)r0[lx.i0 * 3 + c] / 255.f, v01 = (float)r0[lx.i1 * 3 + c] / 255.f;
            const float v10 = (float)r1[lx.i0 * 3 + c] / 255.f, v11 = (float)r1[lx.i1 * 3 + c] / 255.f;
            out[c * total + idx] = blend_image(ly, lx, v00, v01, v10, v11);
        }
    }
}

// out[Y][X] = (accumulate ? out[Y][X] : 0) + alpha * bilinear_ac(in)(Y, X); in[y][x] sits at in[(y * w + x) * stride]
// (stride 2: class 1 of an (h, w, 2) prediction, read in place)
__global__ __launch_bounds__(PX_BLOCK) void px_plane_resize_kernel(const float* __restrict__ in, float* __restrict__ out, int h, int w,
                                                                   int H, int W, int stride, float alpha, int accumulate, float sh,
                                                                   float sw) {
    const long total = (long)H * W;
    for (long idx = (long)blockIdx.x * PX_BLOCK + threadIdx.x; idx < total; idx += (long)gridDim.x * PX_BLOCK) {
        const int Y = (int)(idx / W), X = (int)(idx - (long)Y * W);
        const Lerp ly = lerp_of(Y, sh, h), lx = lerp_of(X, sw, w);
        const float* r0 = in + (long)ly.i0 * w * stride;
        const float* r1 = in + (long)ly.i1 * w * stride;
        const float v = blend_plane_times(ly, lx, alpha, r0[(long)lx.i0 * stride], r0[(long)lx.i1 * stride], r1[(long)lx.i0 * stride],
                                          r1[(long)lx.i1 * stride]);
        out[idx] = accumulate ? add_rounded_product(out[idx], v) : v;
    }
}

// ---- the per-resolution gather: out = ReLU(bias + P0 + sum_r bilinear_ac(P_r)), every level interpolated straight to (H, W).
// A block owns PG_TY rows x PG_TX columns of pixels times a slab of 64 channel quads: a wave is one row of the tile, its lanes
// the quads (16 B each, 1 KB per wave access).  A wave walks its row from left to right and keeps, per level, the two coarse
// columns it is between (top and bottom corner, 4 float4) in registers: a corner is fetched when the walk first reaches it and
// serves every pixel between it and the next one (2^r of them at level r) instead of being fetched per pixel.  Over 16 pixels
// that is about 18 + 10 + 6 + 4 fetches for the four levels where a block per pixel makes 256; the rows of the tile and the
// neighbouring tiles find the same coarse rows in L2.  Every output element reads only its own element of P0, so out may be P0.
#define PG_TX 16
#define PG_TY 4
struct PixLevels {
    const float* p[4];
    int h[4], w[4];
    float sh[4], sw[4];
};
}  // namespace
WESUP_NO_PADDING(PixLevels, 4 * 8 + 4 * 4 * 4);
namespace {

__device__ __forceinline__ float4 fma_bilerp(float4 acc, const Lerp ly, const Lerp lx, float4 a0, float4 a1, float4 b0, float4 b1) {
    acc.x += blend_image(ly, lx, a0.x, a1.x, b0.x, b1.x);
    acc.y += blend_image(ly, lx, a0.y, a1.y, b0.y, b1.y);
    acc.z += blend_image(ly, lx, a0.z, a1.z, b0.z, b1.z);
    acc.w += blend_image(ly, lx, a0.w, a1.w, b0.w, b1.w);
    return acc;
}

template <int NL>
__global__ __launch_bounds__(PX_BLOCK) void px_gather_kernel(const float* p0, const float* __restrict__ bias, float* out,
                                                             const PixLevels L, int B, int H, int W, int C4, int tiles_x,
                                                             int tiles_y, int slabs) {
    constexpr int NA = NL > 0 ? NL : 1;
    int bid = blockIdx.x;
    const int slab = bid % slabs;
    bid /= slabs;
    const int tx = bid % tiles_x;
    bid /= tiles_x;
    const int ty = bid % tiles_y;
    const int b = bid / tiles_y;
    const int q = slab * 64 + (threadIdx.x & 63);
    const int Y = ty * PG_TY + (threadIdx.x >> 6);
    if (b >= B || q >= C4 || Y >= H) return;
    const int X0 = tx * PG_TX, X1 = min(X0 + PG_TX, W);
    const long N = (long)C4 * 4;
    const float4 bv = ld4(bias + 4 * q);
    Lerp ly[NA];
    const float* top[NA];
    const float* bot[NA];
    int c0[NA], c1[NA];
    float4 a0[NA], a1[NA], b0[NA], b1[NA];
#pragma unroll
    for (int r = 0; r < NL; ++r) {
        ly[r] = lerp_of(Y, L.sh[r], L.h[r]);
        const float* base = L.p[r] + (long)b * L.h[r] * L.w[r] * N + 4 * q;
        top[r] = base + (long)ly[r].i0 * L.w[r] * N;
        bot[r] = base + (long)ly[r].i1 * L.w[r] * N;
        c0[r] = c1[r] = -1;
        a0[r] = a1[r] = b0[r] = b1[r] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const long row = ((long)b * H + Y) * W;
    for (int X = X0; X < X1; X += 4) {
        float4 v[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (X + j < X1) v[j] = ld4(p0 + (row + X + j) * N + 4 * q);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (X + j >= X1) break;
            float4 acc = make_float4(bv.x + v[j].x, bv.y + v[j].y, bv.z + v[j].z, bv.w + v[j].w);
#pragma unroll
            for (int r = 0; r < NL; ++r) {
                const Lerp lx = lerp_of(X + j, L.sw[r], L.w[r]);
                // (the column indices depend on the pixel alone: these branches are the same in every lane of the wave)
                if (lx.i0 != c0[r]) {
                    if (lx.i0 == c1[r]) {
                        a0[r] = a1[r];
                        b0[r] = b1[r];
                    } else {
                        a0[r] = ld4(top[r] + (long)lx.i0 * N);
                        b0[r] = ld4(bot[r] + (long)lx.i0 * N);
                    }
                    c0[r] = lx.i0;
                }
                if (lx.i1 != c1[r]) {
                    if (lx.i1 == c0[r]) {
                        a1[r] = a0[r];
                        b1[r] = b0[r];
                    } else {
                        a1[r] = ld4(top[r] + (long)lx.i1 * N);
                        b1[r] = ld4(bot[r] + (long)lx.i1 * N);
                    }
                    c1[r] = lx.i1;
                }
                acc = fma_bilerp(acc, ly[r], lx, a0[r], a1[r], b0[r], b1[r]);
            }
            st4(out + (row + X + j) * N + 4 * q, relu4(acc));
        }
    }
}

}  // namespace

extern "C" int wesup_image_resize_u8(const uint8_t* img, float* out, int H, int W, int h, int w, void* stream) {
    if (!img || !out || H <= 0 || W <= 0 || h <= 0 || w <= 0) return WESUP_ERR_INVALID;
    WESUP_LAUNCH(px_image_resize_kernel, dim3(grid_stride_blocks((long)h * w, PX_BLOCK, PX_MAX_BLOCKS)), dim3(PX_BLOCK), 0,
                 (hipStream_t)stream, img, out, H, W, h, w, ac_scale(H, h), ac_scale(W, w));
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_plane_resize_acc(const float* in, float* out, int h, int w, int H, int W, int stride, float alpha,
                                      int accumulate, void* stream) {
    if (!in || !out || h <= 0 || w <= 0 || H <= 0 || W <= 0 || stride <= 0) return WESUP_ERR_INVALID;
    WESUP_LAUNCH(px_plane_resize_kernel, dim3(grid_stride_blocks((long)H * W, PX_BLOCK, PX_MAX_BLOCKS)), dim3(PX_BLOCK), 0,
                 (hipStream_t)stream, in, out, h, w, H, W, stride, alpha, accumulate ? 1 : 0, ac_scale(h, H), ac_scale(w, W));
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_pixel_gather_fwd(const float* p0, const float* bias, float* out, const WesupCoarseMap* levels /* host */,
                                      int n_levels, int B, int H, int W, int N, void* stream) {
    if (!p0 || !bias || !out || n_levels < 0 || n_levels > 4 || (n_levels && !levels) || B <= 0 || H <= 0 || W <= 0 || N <= 0 ||
        (N % 4) || (((uintptr_t)p0 | (uintptr_t)bias | (uintptr_t)out) & 15))
        return WESUP_ERR_INVALID;
    PixLevels L = {};
    for (int r = 0; r < n_levels; ++r) {
        if (!levels[r].p || levels[r].h <= 0 || levels[r].w <= 0 || (((uintptr_t)levels[r].p) & 15)) return WESUP_ERR_INVALID;
        L.p[r] = levels[r].p;
        L.h[r] = levels[r].h;
        L.w[r] = levels[r].w;
        L.sh[r] = ac_scale(levels[r].h, H);
        L.sw[r] = ac_scale(levels[r].w, W);
    }
    const int C4 = N / 4, slabs = ceil_div(C4, 64), tiles_x = ceil_div(W, PG_TX), tiles_y = ceil_div(H, PG_TY);
    const long blocks = (long)B * tiles_y * tiles_x * slabs;
    if (blocks >= (1l << 31)) return WESUP_ERR_INVALID;
    const dim3 grid((unsigned)blocks), block(PX_BLOCK);
    hipStream_t st = (hipStream_t)stream;
    switch (n_levels) {
    case 0: WESUP_LAUNCH(px_gather_kernel<0>, grid, block, 0, st, p0, bias, out, L, B, H, W, C4, tiles_x, tiles_y, slabs); break;
    case 1: WESUP_LAUNCH(px_gather_kernel<1>, grid, block, 0, st, p0, bias, out, L, B, H, W, C4, tiles_x, tiles_y, slabs); break;
    case 2: WESUP_LAUNCH(px_gather_kernel<2>, grid, block, 0, st, p0, bias, out, L, B, H, W, C4, tiles_x, tiles_y, slabs); break;
    case 3: WESUP_LAUNCH(px_gather_kernel<3>, grid, block, 0, st, p0, bias, out, L, B, H, W, C4, tiles_x, tiles_y, slabs); break;
    default: WESUP_LAUNCH(px_gather_kernel<4>, grid, block, 0, st, p0, bias, out, L, B, H, W, C4, tiles_x, tiles_y, slabs); break;
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
