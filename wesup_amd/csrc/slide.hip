// Whole-slide evaluation on the device (the reference's test_dp2019_pipeline.py): the two ends of a patch's trip
// through the network and the pixel counts of the score.  A slide is cut into a lattice of p x p patches, n_h = ceil(H / p) rows
// of n_w = ceil(W / p); patch k (row-major) has its corner at (k / n_w * p, k % n_w * p) and texels beyond the slide are 0 -- the
// reference pads the slide with zeros before it cuts.  The gather cuts patches and resizes them to the network's input in one
// pass, the scatter resizes a patch's prediction back and pastes it into the slide-size map, the scores kernel counts.  All three
// are memory movement: no LDS beyond the block reduction of the counts, no workspace, deterministic (integer atomics only).
// Every offset that involves H * W is a long: a slide may be larger than 2^31 bytes.
// The gather and the scatter also walk a list of patches instead of consecutive indices (the *_list entries; the list is
// tissue.hip's): the same kernels with the list as one more argument, null for the plain entries.
#include "common.hpp"
#include "bilinear.hpp"
#include "lattice.hpp"

#define SD_BLOCK 256
#define SD_MAX_BLOCKS 4096     // grid-stride above this (cdna_hip_programming.md, guideline 11)

namespace {

// out[n][c][y][x] = bilinear(patch_k / 255.f)(y, x), k = min(first + n, last): one thread per output pixel and all three planes,
// x fastest across lanes (the three plane stores of a wave are 256 contiguous bytes each).  The neighbour indices are clamped
// at the PATCH border (lerp_of on p texels); a texel beyond the slide border reads as 0 -- pad, then resize.  With a patch list
//  k = list[min(first + n, n_list - 1)]; a list value outside [0, last] leaves its slot unwritten.
template <int AC>
__global__ __launch_bounds__(SD_BLOCK) void sd_gather_kernel(const uint8_t* __restrict__ img, float* __restrict__ out, int H, int W,
                                                             int n_w, int last, int p, int h, int w, int first, int count,
                                                             float sh, float sw, const int32_t* __restrict__ list, int n_list) {
    const long plane = (long)h * w;
    const long total = (long)count * plane;
    for (long idx = (long)blockIdx.x * SD_BLOCK + threadIdx.x; idx < total; idx += (long)gridDim.x * SD_BLOCK) {
        const int n = (int)(idx / plane);
        const long r = idx - (long)n * plane;
        const int y = (int)(r / w), x = (int)(r - (long)y * w);
        int k = first + n;
        if (list) {
            k = list[k > n_list - 1 ? n_list - 1 : k];
            if (k < 0 || k > last) continue;
        }
        k = k > last ? last : k;
        const int ky = k / n_w, kx = k - ky * n_w;
        const Lerp ly = AC ? lerp_of(y, sh, p) : lerp_half_pixel(y, sh, p);
        const Lerp lx = AC ? lerp_of(x, sw, p) : lerp_half_pixel(x, sw, p);
        const long gy0 = (long)ky * p + ly.i0, gy1 = (long)ky * p + ly.i1;
        const long gx0 = (long)kx * p + lx.i0, gx1 = (long)kx * p + lx.i1;
        const bool in00 = gy0 < H && gx0 < W, in01 = gy0 < H && gx1 < W;
        const bool in10 = gy1 < H && gx0 < W, in11 = gy1 < H && gx1 < W;
        const uint8_t* r0 = img + gy0 * W * 3;
        const uint8_t* r1 = img + gy1 * W * 3;
        float* dst = out + (long)n * 3 * plane + r;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v00 = in00 ? (float)r0[gx0 * 3 + c] / 255.f : 0.f, v01 = in01 ? (float)r0[gx1 * 3 + c] / 255.f : 0.f;
            const float v10 = in10 ? (float)r1[gx0 * 3 + c] / 255.f : 0.f, v11 = in11 ? (float)r1[gx1 * 3 + c] / 255.f : 0.f;
            dst[c * plane] = blend_image(ly, lx, v00, v01, v10, v11);
        }
    }
}

// out[Y][X] = 255 * rintf(v) for the slide pixels inside the patches first .. first + count - 1; v = the nearest texel of the
// patch's (h, w) prediction (MODE 0: torch's floorf(dst * scale) index) or its align_corners bilinear value (MODE 1: the
// arithmetic of px_plane_resize_kernel at alpha = 1).  One thread per pixel of the padded lattice, x fastest (patch_pixel,
// lattice.hpp): a wave writes 64 neighbouring bytes (row starts are not aligned: W is any number).  Pixels of the lattice beyond
// the slide, and patches past the end of the lattice, are never written.
template <int MODE>
__global__ __launch_bounds__(SD_BLOCK) void sd_scatter_kernel(const float* __restrict__ pred, uint8_t* __restrict__ out, int H, int W,
                                                              int n_w, int last, int p, int h, int w, int stride, int first,
                                                              int count, float sh, float sw, const int32_t* __restrict__ list,
                                                              int n_list) {
    const long total = (long)count * p * p;
    for (long idx = (long)blockIdx.x * SD_BLOCK + threadIdx.x; idx < total; idx += (long)gridDim.x * SD_BLOCK) {
        const PatchPixel q = patch_pixel(idx, p, first, n_w, last, H, W, list, n_list);
        if (q.skip) continue;
        const float* src = pred + (long)q.n * h * w * stride;
        float v;
        if (MODE == 0) {
            const int sy = min((int)floorf((float)q.y * sh), h - 1), sx = min((int)floorf((float)q.x * sw), w - 1);
            v = src[((long)sy * w + sx) * stride];
        } else {
            const Lerp ly = lerp_of(q.y, sh, h), lx = lerp_of(q.x, sw, w);
            const float* r0 = src + (long)ly.i0 * w * stride;
            const float* r1 = src + (long)ly.i1 * w * stride;
            v = blend_plane(ly, lx, r0[(long)lx.i0 * stride], r0[(long)lx.i1 * stride], r1[(long)lx.i0 * stride],
                            r1[(long)lx.i1 * stride]);
        }
        out[q.Y * W + q.X] = (uint8_t)(int)(255.f * rintf(v));      // rintf: half to even, torch.round
    }
}

// ---- scores: out4 += {#(s == g), #(s > 0 && g > 0), #(s > 0), #(g > 0)} over uint8 maps, after x -> 255 - x on both with
// `flip` = 0xffffffff (255 - x is ~x on a byte: equality is unchanged, "> 0" becomes "!= 255").  Four bytes at a time: bit 7 of
// every byte of nz(x) says that the byte is non-zero, a popcount counts them.
__device__ __forceinline__ unsigned nz_bytes(unsigned x) { return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u; }

struct Counts {
    unsigned eq, inter, s, g;
};
__device__ __forceinline__ void count_word(Counts& c, unsigned s, unsigned g, unsigned flip) {
    const unsigned ns = nz_bytes(s ^ flip), ng = nz_bytes(g ^ flip);
    c.eq += 4u - (unsigned)__popc(nz_bytes(s ^ g));
    c.inter += (unsigned)__popc(ns & ng);
    c.s += (unsigned)__popc(ns);
    c.g += (unsigned)__popc(ng);
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// nvec: whole 16-byte chunks (0 when a pointer is not 16-byte aligned); the n - 16 * nvec bytes behind them go one at a time.
// Per thread 32-bit counts (<= 16 per chunk; a thread sees n / 2^20 bytes at the full grid), per wave and block 64-bit sums,
// one 64-bit atomic add per count and block: integers, so the order of the blocks cannot matter.
__global__ __launch_bounds__(SD_BLOCK) void sd_scores_kernel(const uint8_t* __restrict__ S, const uint8_t* __restrict__ G,
                                                             unsigned long long* __restrict__ out4, long n, long nvec,
                                                             unsigned flip) {
    Counts c = {0u, 0u, 0u, 0u};
    const long tid = (long)blockIdx.x * SD_BLOCK + threadIdx.x, nthreads = (long)gridDim.x * SD_BLOCK;
    const uint4* S4 = reinterpret_cast<const uint4*>(S);
    const uint4* G4 = reinterpret_cast<const uint4*>(G);
    for (long i = tid; i < nvec; i += nthreads) {
        const uint4 s = S4[i], g = G4[i];
        count_word(c, s.x, g.x, flip);
        count_word(c, s.y, g.y, flip);
        count_word(c, s.z, g.z, flip);
        count_word(c, s.w, g.w, flip);
    }
    for (long i = nvec * 16 + tid; i < n; i += nthreads) {
        const unsigned s = (unsigned)S[i] ^ (flip & 0xffu), g = (unsigned)G[i] ^ (flip & 0xffu);
        c.eq += s == g ? 1u : 0u;
        c.inter += (s && g) ? 1u : 0u;
        c.s += s ? 1u : 0u;
        c.g += g ? 1u : 0u;
    }
    __shared__ unsigned long long part[SD_BLOCK / 64][4];
    const unsigned long long v[4] = {wave_sum(c.eq), wave_sum(c.inter), wave_sum(c.s), wave_sum(c.g)};
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) part[wave][j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long t = 0;
#pragma unroll
        for (int wv = 0; wv < SD_BLOCK / 64; ++wv) t += part[wv][threadIdx.x];
        if (t) atomicAdd(&out4[threadIdx.x], t);
    }
}

}  // namespace

// list == NULL: the consecutive patches first .. first + count - 1; otherwise the slots first .. of list[n_list]
static int sd_gather(const uint8_t* img, float* out, int H, int W, int p, int h, int w, int align_corners, int first, int count,
                     const int32_t* list, int n_list, void* stream) {
    int n_w = 0, last = 0;
    if (!img || !out || h <= 0 || w <= 0 || first < 0 || count < 1 || (align_corners != 0 && align_corners != 1) ||
        !sd_lattice(H, W, p, &n_w, &last) || (long)first + count > 0x7fffffffl)
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_stride_blocks((long)count * h * w, SD_BLOCK, SD_MAX_BLOCKS)), block(SD_BLOCK);
    if (align_corners) {
        WESUP_LAUNCH(sd_gather_kernel<1>, grid, block, 0, st, img, out, H, W, n_w, last, p, h, w, first, count, ac_scale(p, h),
                     ac_scale(p, w), list, n_list);
    } else {
        WESUP_LAUNCH(sd_gather_kernel<0>, grid, block, 0, st, img, out, H, W, n_w, last, p, h, w, first, count, hp_scale(p, h),
                     hp_scale(p, w), list, n_list);
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

static int sd_scatter(const float* pred, uint8_t* out, int H, int W, int p, int h, int w, int stride, int mode, int first, int count,
                      const int32_t* list, int n_list, void* stream) {
    int n_w = 0, last = 0;
    if (!pred || !out || h <= 0 || w <= 0 || stride < 1 || first < 0 || count < 1 || (mode != 0 && mode != 1) ||
        !sd_lattice(H, W, p, &n_w, &last) || (long)first + count > 0x7fffffffl)
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_stride_blocks((long)count * p * p, SD_BLOCK, SD_MAX_BLOCKS)), block(SD_BLOCK);
    if (mode == 0) {
        WESUP_LAUNCH(sd_scatter_kernel<0>, grid, block, 0, st, pred, out, H, W, n_w, last, p, h, w, stride, first, count,
                     hp_scale(h, p), hp_scale(w, p), list, n_list);
    } else {
        WESUP_LAUNCH(sd_scatter_kernel<1>, grid, block, 0, st, pred, out, H, W, n_w, last, p, h, w, stride, first, count,
                     ac_scale(h, p), ac_scale(w, p), list, n_list);
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_patch_gather_resize(const uint8_t* img, float* out, int H, int W, int p, int h, int w, int align_corners,
                                         int first, int count, void* stream) {
    return sd_gather(img, out, H, W, p, h, w, align_corners, first, count, nullptr, 0, stream);
}

extern "C" int wesup_patch_gather_resize_list(const uint8_t* img, float* out, int H, int W, int p, int h, int w, int align_corners,
                                              int first, int count, const int32_t* list, int n_list, void* stream) {
    if (!list || n_list < 1) return WESUP_ERR_INVALID;
    return sd_gather(img, out, H, W, p, h, w, align_corners, first, count, list, n_list, stream);
}

extern "C" int wesup_patch_scatter_u8(const float* pred, uint8_t* out, int H, int W, int p, int h, int w, int stride, int mode,
                                      int first, int count, void* stream) {
    return sd_scatter(pred, out, H, W, p, h, w, stride, mode, first, count, nullptr, 0, stream);
}

extern "C" int wesup_patch_scatter_u8_list(const float* pred, uint8_t* out, int H, int W, int p, int h, int w, int stride, int mode,
                                           int first, int count, const int32_t* list, int n_list, void* stream) {
    if (!list || n_list < 1) return WESUP_ERR_INVALID;
    return sd_scatter(pred, out, H, W, p, h, w, stride, mode, first, count, list, n_list, stream);
}

extern "C" int wesup_mask_scores(const uint8_t* S, const uint8_t* G, int64_t* out4, long n, int negative, void* stream) {
    if (!S || !G || !out4 || n <= 0 || (((uintptr_t)out4) & 7)) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (wesup_fill_words_(out4, 0u, 8, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    const bool aligned = ((((uintptr_t)S) | ((uintptr_t)G)) & 15) == 0;
    const long nvec = aligned ? n / 16 : 0;
    const long work = nvec + (n - nvec * 16);
    WESUP_LAUNCH(sd_scores_kernel, dim3(grid_stride_blocks(work, SD_BLOCK, SD_MAX_BLOCKS)), dim3(SD_BLOCK), 0, st, S, G,
                 reinterpret_cast<unsigned long long*>(out4), n, nvec, negative ? 0xffffffffu : 0u);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
