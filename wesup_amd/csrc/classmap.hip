// Class maps for models of more than two classes: the four steps behind the networks of infer_tile.py,
// pixel_infer.py and slide.py that exist for one plane in tiles.hip, pixel.hip and slide.hip -- the merge over the covering
// windows, the resize back to the image's size, the paste into the slide-size map and the scoring -- as per-pixel reductions over
// the C values of a pixel, 2 <= C <= WESUP_MAX_CLASSES.  The index code and the roundings are the one-plane kernels' own: the
// lattice walks of lattice.hpp, the blends of bilinear.hpp.  The two-class kernels stay as they are; nothing here is reached for C = 2
// by the tools.
//
// A pixel's class is the FIRST MAXIMUM over ascending c, compared with a strict > (np.argmax on data without NaNs.  No comparison
// with a NaN is true: a NaN behind the first entry is never the maximum, and a row whose first entry is NaN gives class 0).
// Per-class values live in registers: arrays are indexed by unrolled constants only, under a compile-time bound
// CMAX >= C with every use guarded by c < C, as cls_row (loss.hip) does -- a run-time index would put them in scratch.  A class
// index that comes in as data (a vote, a painted map, a label byte) is never used as an address: it is compared, and one outside
// [0, C) is not counted and sets the status word (wesup_seg_confusion's convention).
//
// All kernels are byte-bound: every input byte is read once, as float4 / uint4 where C % 4 == 0 (or the maps are 16-byte aligned).
// No workspace, no float atomics, deterministic.
#include "common.hpp"
#include "bilinear.hpp"
#include "lattice.hpp"

#define CM_BLOCK 256
#define CM_MAX_BLOCKS 4096     // grid-stride above this (cdna_hip_programming.md, guideline 11)

namespace {

inline bool cm_range(int C) { return C >= 2 && C <= WESUP_MAX_CLASSES; }

// first maximum of v[0 .. C)
template <int CMAX, typename T>
__device__ __forceinline__ int first_max(const T (&v)[CMAX], int C) {
    T best = v[0];
    int bi = 0;
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C && v[c] > best) {
            best = v[c];
            bi = c;
        }
    return bi;
}

// use(c, src[c]) for the C values of a pixel, one contiguous run, in ascending c: float4 per class quad with VEC4 (C % 4 == 0, src
// 16-byte aligned).  c is a constant once the loop is unrolled, so use may index a register array with it.
template <int CMAX, bool VEC4, typename Use>
__device__ __forceinline__ void load_classes(const float* __restrict__ src, int C, Use use) {
    if constexpr (VEC4) {
#pragma unroll
        for (int c = 0; c + 3 < CMAX; c += 4)
            if (c < C) {
                const float4 q = ld4(src + c);
                use(c, q.x);
                use(c + 1, q.y);
                use(c + 2, q.z);
                use(c + 3, q.w);
            }
    } else {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) use(c, src[c]);
    }
}

// the four neighbours of a bilinear sample in an [h][w][C] map: the C values of each are one contiguous run
struct Corners {
    const float *p00, *p01, *p10, *p11;
};
__device__ __forceinline__ Corners corners_of(const float* in, const Lerp ly, const Lerp lx, int w, int C) {
    return {in + ((long)ly.i0 * w + lx.i0) * C, in + ((long)ly.i0 * w + lx.i1) * C, in + ((long)ly.i1 * w + lx.i0) * C,
            in + ((long)ly.i1 * w + lx.i1) * C};
}

// ---- 1. merge: out[y][x] = first maximum over c of the mean over the covering windows and their views (the plain
// entry is the one-view case V = 1, views = 0, and UPRIGHT is that case at compile time, as in tiles.hip).  One thread per PIXEL:
// the covering windows are found once (covering, lattice.hpp: tl_merge_kernel's search), every covering window (ascending,
// row-major) contributes its V views in list order, each read through view_inverse (lattice.hpp) at an offset tested to lie in
// [0, p); the C values of a window pixel are one contiguous run, and the (H, W, C) fp64 tensor is never formed.  VOTES = 0: pred
// [N][V][p][p][C] probabilities in VIEW space; per class tl_merge_kernel's arithmetic -- adds onto 0.0 in fp64, one IEEE division
// by the number of values, covering windows x V -- then the argmax of the quotients (two sums may round to one quotient: the
// division is not skipped).  VOTES = 1: pred [N][V][p][p] class indices as floats; integer counts per class (a vote is compared
// with every c, it never indexes), the first maximum of the counts.  infer_tile.combine_views_to_classes
// (combine_patches_to_classes for one upright view) bit for bit.
template <int CMAX, bool VEC4, bool VOTES, bool UPRIGHT>
__global__ __launch_bounds__(CM_BLOCK) void cm_merge_kernel(const float* __restrict__ pred, const int32_t* __restrict__ tops,
                                                            const int32_t* __restrict__ lefts, uint8_t* __restrict__ out,
                                                            int32_t* __restrict__ status, int H, int W, int C, int n_h, int n_w,
                                                            int p, int n_views, uint32_t views) {
    const int V = UPRIGHT ? 1 : n_views;
    const long total = (long)H * W;
    for (long idx = (long)blockIdx.x * CM_BLOCK + threadIdx.x; idx < total; idx += (long)gridDim.x * CM_BLOCK) {
        const int y = (int)(idx / W), x = (int)(idx - (long)y * W);
        const Covering rows = covering(tops, n_h, y, p), cols = covering(lefts, n_w, x, p);
        double acc[CMAX];
        int votes[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) {
            acc[c] = 0.0;
            votes[c] = 0;
        }
        int cnt = 0;
        bool bad = false;
        for (int i = rows.i0; i < rows.i1; ++i) {
            const int dy = y - tops[i];
            if (dy < 0 || dy >= p) continue;         // (an unsorted lattice: never an address outside the window)
            for (int j = cols.i0; j < cols.i1; ++j) {
                const int dx = x - lefts[j];
                if (dx < 0 || dx >= p) continue;
                const long slot = (long)(i * n_w + j) * V;
                for (int t = 0; t < V; ++t) {
                    const ViewPixel q = view_inverse(UPRIGHT ? 0 : view_at(views, t), p, dy, dx);
                    if (!view_inside(q, p)) continue;
                    const long at = ((slot + t) * p + q.y) * p + q.x;
                    if constexpr (VOTES) {
                        const float v = rintf(pred[at]);
                        if (v >= 0.f && v < (float)C) {
#pragma unroll
                            for (int c = 0; c < CMAX; ++c)
                                if (c < C) votes[c] += (v == (float)c) ? 1 : 0;
                        } else bad = true;           // (a NaN lands here too)
                    } else {
                        load_classes<CMAX, VEC4>(pred + at * C, C, [&](int c, float v) { acc[c] += (double)v; });
                    }
                    ++cnt;
                }
            }
        }
        int cls;
        if constexpr (VOTES) {
            cls = first_max<CMAX>(votes, C);
            if (bad) atomicOr(status, 1);
        } else {
            const double n = (double)cnt;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) acc[c] = acc[c] / n;
            cls = first_max<CMAX>(acc, C);
        }
        out[idx] = (uint8_t)cls;
    }
}

// ---- 2. resize: out[Y][X][c] = (accumulate ? out[Y][X][c] : 0) + alpha * bilinear_ac(in[..][..][c])(Y, X), every plane the
// bits of px_plane_resize_kernel on in[..., c]: the same two functions (blend_plane_times, add_rounded_product: bilinear.hpp) state
// the product by alpha and the add onto out as two roundings in both kernels.  One thread per output pixel: the coordinates and the
// four corner addresses are worked out once, the four corner vectors are read once (float4 per class quad with VEC4) and serve
// all C planes.
template <int CMAX, bool VEC4>
__global__ __launch_bounds__(CM_BLOCK) void cm_planes_resize_kernel(const float* __restrict__ in, float* __restrict__ out, int h,
                                                                    int w, int H, int W, int C, float alpha, int accumulate,
                                                                    float sh, float sw) {
    const long total = (long)H * W;
    for (long idx = (long)blockIdx.x * CM_BLOCK + threadIdx.x; idx < total; idx += (long)gridDim.x * CM_BLOCK) {
        const int Y = (int)(idx / W), X = (int)(idx - (long)Y * W);
        const Lerp ly = lerp_of(Y, sh, h), lx = lerp_of(X, sw, w);
        const Corners k = corners_of(in, ly, lx, w, C);
        float* dst = out + idx * C;
        if constexpr (VEC4) {
#pragma unroll
            for (int c = 0; c + 3 < CMAX; c += 4)
                if (c < C) {
                    const float4 a = ld4(k.p00 + c), b = ld4(k.p01 + c), d = ld4(k.p10 + c), e = ld4(k.p11 + c);
                    float4 v = make_float4(blend_plane_times(ly, lx, alpha, a.x, b.x, d.x, e.x),
                                           blend_plane_times(ly, lx, alpha, a.y, b.y, d.y, e.y),
                                           blend_plane_times(ly, lx, alpha, a.z, b.z, d.z, e.z),
                                           blend_plane_times(ly, lx, alpha, a.w, b.w, d.w, e.w));
                    if (accumulate) {
                        const float4 o = ld4(dst + c);
                        v = make_float4(add_rounded_product(o.x, v.x), add_rounded_product(o.y, v.y), add_rounded_product(o.z, v.z),
                                        add_rounded_product(o.w, v.w));
                    }
                    st4(dst + c, v);
                }
        } else {
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float v = blend_plane_times(ly, lx, alpha, k.p00[c], k.p01[c], k.p10[c], k.p11[c]);
                    dst[c] = accumulate ? add_rounded_product(dst[c], v) : v;
                }
        }
    }
}

// ---- 3. argmax: out[r] = first maximum of in[r][0 .. C).  One thread per row, rows read as float4 with VEC4.
template <int CMAX, bool VEC4>
__global__ __launch_bounds__(CM_BLOCK) void cm_argmax_kernel(const float* __restrict__ in, uint8_t* __restrict__ out, long n, int C) {
    for (long r = (long)blockIdx.x * CM_BLOCK + threadIdx.x; r < n; r += (long)gridDim.x * CM_BLOCK) {
        float v[CMAX];
        load_classes<CMAX, VEC4>(in + r * C, C, [&](int c, float x) { v[c] = x; });
        out[r] = (uint8_t)first_max<CMAX>(v, C);
    }
}

// ---- 4. paste: sd_scatter_kernel's lattice walk (patch_pixel, lattice.hpp: one thread per pixel of the padded lattice, x fastest;
// pixels beyond the slide and patches past the end of the lattice are never written) with a class index as the pasted byte.
// MODE 0: pred [count][h][w] class indices as floats, the nearest texel (torch's floorf(dst * scale)); an index outside [0, C)
// pastes 0 and sets status.  MODE 1: pred [count][h][w][C] probabilities, per class cm_planes_resize_kernel's value at alpha = 1
// (1.f * v is v), then the first maximum.
template <int CMAX, bool VEC4, int MODE>
__global__ __launch_bounds__(CM_BLOCK) void cm_scatter_kernel(const float* __restrict__ pred, uint8_t* __restrict__ out,
                                                              int32_t* __restrict__ status, int H, int W, int n_w, int last, int p,
                                                              int h, int w, int C, int first, int count, float sh, float sw,
                                                              const int32_t* __restrict__ list, int n_list) {
    const long total = (long)count * p * p;
    bool bad = false;
    for (long idx = (long)blockIdx.x * CM_BLOCK + threadIdx.x; idx < total; idx += (long)gridDim.x * CM_BLOCK) {
        const PatchPixel q = patch_pixel(idx, p, first, n_w, last, H, W, list, n_list);
        bad = bad || q.bad;                          // (a list value outside the lattice: skipped, told in status)
        if (q.skip) continue;
        int cls = 0;
        if constexpr (MODE == 0) {
            const int sy = min((int)floorf((float)q.y * sh), h - 1), sx = min((int)floorf((float)q.x * sw), w - 1);
            const float v = rintf(pred[((long)q.n * h + sy) * w + sx]);
            if (v >= 0.f && v < (float)C) cls = (int)v;
            else bad = true;                         // (a NaN lands here too)
        } else {
            const Lerp ly = lerp_of(q.y, sh, h), lx = lerp_of(q.x, sw, w);
            const Corners k = corners_of(pred + (long)q.n * h * w * C, ly, lx, w, C);
            float v[CMAX];
            if constexpr (VEC4) {
#pragma unroll
                for (int c = 0; c + 3 < CMAX; c += 4)
                    if (c < C) {
                        const float4 a = ld4(k.p00 + c), b = ld4(k.p01 + c), d = ld4(k.p10 + c), e = ld4(k.p11 + c);
                        v[c] = blend_plane(ly, lx, a.x, b.x, d.x, e.x);
                        v[c + 1] = blend_plane(ly, lx, a.y, b.y, d.y, e.y);
                        v[c + 2] = blend_plane(ly, lx, a.z, b.z, d.z, e.z);
                        v[c + 3] = blend_plane(ly, lx, a.w, b.w, d.w, e.w);
                    }
            } else {
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < C) v[c] = blend_plane(ly, lx, k.p00[c], k.p01[c], k.p10[c], k.p11[c]);
            }
            cls = first_max<CMAX>(v, C);
        }
        out[q.Y * W + q.X] = (uint8_t)cls;
    }
    if (bad) atomicOr(status, 1);
}

// ---- 5. confusion of two label maps: conf[g][s] += 1 per byte pair.  A wave counts into its own table in LDS (integer adds,
// C * C <= 256 cells), the block adds its four tables up and adds the non-zero cells to the 64-bit table in global memory:
// integers, so no order of lanes, waves or blocks can change the result.  nvec: whole 16-byte chunks (0 when a pointer is not
// 16-byte aligned); the bytes behind them go one at a time.  A thread sees at most n / 2^20 bytes at the full grid and the entry
// bounds n, so a 32-bit cell cannot wrap.  A byte outside [0, C) is remembered in a register and costs its thread one atomic on
// the status word at the end, however many there are (a x 255 mask handed over by mistake is all of them).
#define CM_CELLS (WESUP_MAX_CLASSES * WESUP_MAX_CLASSES)
__device__ __forceinline__ bool cm_count(unsigned* tab, unsigned s, unsigned g, unsigned C) {      // true: not counted
    if (s < C && g < C) {
        atomicAdd(&tab[g * C + s], 1u);
        return false;
    }
    return true;
}
__device__ __forceinline__ bool cm_count_word(unsigned* tab, unsigned s, unsigned g, unsigned C) {
    bool bad = false;
#pragma unroll
    for (int b = 0; b < 4; ++b) bad |= cm_count(tab, (s >> (8 * b)) & 0xffu, (g >> (8 * b)) & 0xffu, C);
    return bad;
}
__global__ __launch_bounds__(CM_BLOCK) void cm_confusion_kernel(const uint8_t* __restrict__ S, const uint8_t* __restrict__ G,
                                                                unsigned long long* __restrict__ conf, int32_t* __restrict__ status,
                                                                long n, long nvec, int C) {
    __shared__ unsigned tab[CM_BLOCK / 64][CM_CELLS];
    for (int e = threadIdx.x; e < (CM_BLOCK / 64) * CM_CELLS; e += CM_BLOCK) (&tab[0][0])[e] = 0u;
    __syncthreads();
    unsigned* mine = tab[threadIdx.x >> 6];
    const long tid = (long)blockIdx.x * CM_BLOCK + threadIdx.x, nthreads = (long)gridDim.x * CM_BLOCK;
    const uint4* S4 = reinterpret_cast<const uint4*>(S);
    const uint4* G4 = reinterpret_cast<const uint4*>(G);
    bool bad = false;
    for (long i = tid; i < nvec; i += nthreads) {
        const uint4 s = S4[i], g = G4[i];
        bad |= cm_count_word(mine, s.x, g.x, (unsigned)C);
        bad |= cm_count_word(mine, s.y, g.y, (unsigned)C);
        bad |= cm_count_word(mine, s.z, g.z, (unsigned)C);
        bad |= cm_count_word(mine, s.w, g.w, (unsigned)C);
    }
    for (long i = nvec * 16 + tid; i < n; i += nthreads) bad |= cm_count(mine, S[i], G[i], (unsigned)C);
    if (bad) atomicOr(status, 1);
    __syncthreads();
    if (threadIdx.x < C * C) {
        unsigned long long t = 0;
#pragma unroll
        for (int wv = 0; wv < CM_BLOCK / 64; ++wv) t += tab[wv][threadIdx.x];
        if (t) atomicAdd(&conf[threadIdx.x], t);
    }
}

inline bool aligned16(const void* a) { return (((uintptr_t)a) & 15) == 0; }

}  // namespace

// CMAX in {2, 4, 8, 16} and, where the kernel has both forms, float4 reads for C % 4 == 0 on 16-byte aligned tensors
#define CM_DISPATCH(C, vec, LAUNCH)                              \
    do {                                                         \
        if ((C) <= 2) { LAUNCH(2, false); }                      \
        else if ((C) <= 4) { if (vec) { LAUNCH(4, true); } else { LAUNCH(4, false); } }   \
        else if ((C) <= 8) { if (vec) { LAUNCH(8, true); } else { LAUNCH(8, false); } }   \
        else { if (vec) { LAUNCH(16, true); } else { LAUNCH(16, false); } }               \
    } while (0)

// (called with n_views = 1, views = 0 by the plain entry)
static int cm_merge(const float* pred, const int32_t* tops, const int32_t* lefts, uint8_t* out, int32_t* status, int H, int W, int C,
                    int n_h, int n_w, int p, int n_views, uint32_t views, int votes, void* stream) {
    if (!pred || !tops || !lefts || !out || !status || p < 1 || p > H || p > W || !cm_range(C) || n_h < 1 || n_w < 1 ||
        !views_ok(n_views, views) || (long)n_h * n_w * n_views > 0x7fffffffl || (votes != 0 && votes != 1))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (wesup_fill_words_(status, 0u, 1, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    const dim3 grid(grid_stride_blocks((long)H * W, CM_BLOCK, CM_MAX_BLOCKS)), block(CM_BLOCK);
    const bool vec = !votes && (C % 4 == 0) && aligned16(pred), upright = n_views == 1 && views == 0;
#define CM_M(CMAX, V, VOTES, UP)                                                                                                   \
    WESUP_LAUNCH((cm_merge_kernel<CMAX, V, VOTES, UP>), grid, block, 0, st, pred, tops, lefts, out, status, H, W, C, n_h, n_w, p, \
                 n_views, views)
#define CM_L(CMAX, V)                                                                            \
    if (votes) {                                                                                 \
        if (upright) CM_M(CMAX, false, true, true);                                              \
        else CM_M(CMAX, false, true, false);                                                     \
    } else if (upright) CM_M(CMAX, V, false, true);                                              \
    else CM_M(CMAX, V, false, false)
    CM_DISPATCH(C, vec, CM_L);
#undef CM_L
#undef CM_M
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_window_merge_classes(const float* pred, const int32_t* tops, const int32_t* lefts, uint8_t* out,
                                          int32_t* status, int H, int W, int C, int n_h, int n_w, int p, int votes, void* stream) {
    return cm_merge(pred, tops, lefts, out, status, H, W, C, n_h, n_w, p, 1, 0u, votes, stream);
}

extern "C" int wesup_window_merge_classes_views(const float* pred, const int32_t* tops, const int32_t* lefts, uint8_t* out,
                                                int32_t* status, int H, int W, int C, int n_h, int n_w, int p, int n_views,
                                                uint32_t views, int votes, void* stream) {
    return cm_merge(pred, tops, lefts, out, status, H, W, C, n_h, n_w, p, n_views, views, votes, stream);
}

extern "C" int wesup_planes_resize_acc(const float* in, float* out, int h, int w, int H, int W, int C, float alpha, int accumulate,
                                       void* stream) {
    if (!in || !out || h <= 0 || w <= 0 || H <= 0 || W <= 0 || !cm_range(C)) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_stride_blocks((long)H * W, CM_BLOCK, CM_MAX_BLOCKS)), block(CM_BLOCK);
    const bool vec = (C % 4 == 0) && aligned16(in) && aligned16(out);
    const float sh = ac_scale(h, H), sw = ac_scale(w, W);
    const int acc = accumulate ? 1 : 0;
#define CM_L(CMAX, V) WESUP_LAUNCH((cm_planes_resize_kernel<CMAX, V>), grid, block, 0, st, in, out, h, w, H, W, C, alpha, acc, sh, sw)
    CM_DISPATCH(C, vec, CM_L);
#undef CM_L
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_class_argmax_u8(const float* in, uint8_t* out, long n, int C, void* stream) {
    if (!in || !out || n <= 0 || !cm_range(C)) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_stride_blocks(n, CM_BLOCK, CM_MAX_BLOCKS)), block(CM_BLOCK);
    const bool vec = (C % 4 == 0) && aligned16(in);
#define CM_L(CMAX, V) WESUP_LAUNCH((cm_argmax_kernel<CMAX, V>), grid, block, 0, st, in, out, n, C)
    CM_DISPATCH(C, vec, CM_L);
#undef CM_L
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

// list == NULL: the consecutive patches first .. first + count - 1; otherwise the slots first .. of list[n_list]
static int cm_scatter(const float* pred, uint8_t* out, int32_t* status, int H, int W, int p, int h, int w, int C, int mode, int first,
                      int count, const int32_t* list, int n_list, void* stream) {
    int n_w = 0, last = 0;
    if (!pred || !out || !status || h <= 0 || w <= 0 || !cm_range(C) || first < 0 || count < 1 || (mode != 0 && mode != 1) ||
        !sd_lattice(H, W, p, &n_w, &last) || (long)first + count > 0x7fffffffl)
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_stride_blocks((long)count * p * p, CM_BLOCK, CM_MAX_BLOCKS)), block(CM_BLOCK);
    const bool vec = mode == 1 && (C % 4 == 0) && aligned16(pred);
    const float sh = mode == 0 ? hp_scale(h, p) : ac_scale(h, p), sw = mode == 0 ? hp_scale(w, p) : ac_scale(w, p);
    if (mode == 0) {                                 // (one index per texel: nothing is held per class)
        WESUP_LAUNCH((cm_scatter_kernel<2, false, 0>), grid, block, 0, st, pred, out, status, H, W, n_w, last, p, h, w, C, first,
                     count, sh, sw, list, n_list);
    } else {
#define CM_L(CMAX, V)                                                                                                              \
    WESUP_LAUNCH((cm_scatter_kernel<CMAX, V, 1>), grid, block, 0, st, pred, out, status, H, W, n_w, last, p, h, w, C, first, count, sh, \
                 sw, list, n_list)
        CM_DISPATCH(C, vec, CM_L);
#undef CM_L
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_patch_scatter_classes_u8(const float* pred, uint8_t* out, int32_t* status, int H, int W, int p, int h, int w,
                                              int C, int mode, int first, int count, void* stream) {
    return cm_scatter(pred, out, status, H, W, p, h, w, C, mode, first, count, nullptr, 0, stream);
}

extern "C" int wesup_patch_scatter_classes_u8_list(const float* pred, uint8_t* out, int32_t* status, int H, int W, int p, int h,
                                                   int w, int C, int mode, int first, int count, const int32_t* list, int n_list,
                                                   void* stream) {
    if (!list || n_list < 1) return WESUP_ERR_INVALID;
    return cm_scatter(pred, out, status, H, W, p, h, w, C, mode, first, count, list, n_list, stream);
}

extern "C" int wesup_label_confusion(const uint8_t* S, const uint8_t* G, int64_t* conf, int32_t* status, long n, int C,
                                     void* stream) {
    if (!S || !G || !conf || !status || n <= 0 || n > (1l << 40) || !cm_range(C) || (((uintptr_t)conf) & 7))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    int rc = wesup_fill_words_(conf, 0u, (size_t)2 * C * C, st);
    if (rc == WESUP_OK) rc = wesup_fill_words_(status, 0u, 1, st);
    if (rc != WESUP_OK) return rc;
    const long nvec = (aligned16(S) && aligned16(G)) ? n / 16 : 0;
    const long work = nvec + (n - nvec * 16);
    WESUP_LAUNCH(cm_confusion_kernel, dim3(grid_stride_blocks(work, CM_BLOCK, CM_MAX_BLOCKS)), dim3(CM_BLOCK), 0, st, S, G,
                 reinterpret_cast<unsigned long long*>(conf), status, n, nvec, C);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
