// Window inference on images larger than the network input, the two ends of it that used to run on the host:
// cutting an (H, W, 3) uint8 image into the fp32 windows the network reads, and merging the per-window predictions into one
// map by the mean over the covering windows.  Both kernels are pure memory movement: no LDS, no atomics, no workspace.
//
// The window lattice (infer_tile.window_grid) is two sorted int32 arrays on the device, tops[n_h] and lefts[n_w]; window k
// (row-major) has its corner at (tops[k / n_w], lefts[k % n_w]).  The arrays are made by the caller: neither kernel trusts
// them with an address.  The gather clamps a corner into the image, the merge only ever reads pred at offsets it has itself
// tested to lie in [0, p), so a wrong lattice gives wrong numbers (NaN where no window covers a pixel), never a fault.
#include "common.hpp"
#include "lattice.hpp"

#define TL_BLOCK 256
#define TL_MAX_BLOCKS 4096     // grid-stride above this (cdna_hip_programming.md, guideline 11)

namespace {

// What ATen makes of uint8 -> float -> div_(255.) on the device: the division by a host scalar is a multiplication by the
// fp32 reciprocal (1.f / 255.f rounded once, on the host), which differs from x / 255.f in the last bit for some bytes.
// tests/test_tiles_gpu.py holds all 256 values to infer_tile._to_tensor bit for bit.
__device__ __forceinline__ float byte_to_unit(uint8_t v) { return (float)v * (1.0f / 255.0f); }

// A window is read under one of the eight views of lattice.hpp: the slot axis of a pass is windows x views, slot
// s is window s / V under view views[s % V]; the plain entries are the one-view case V = 1, views = 0, for which a (N,1,p,p[,C])
// buffer is the (N,p,p[,C]) buffer.  UPRIGHT is that case at compile time -- the same body with the view arithmetic folded away
// (view 0 maps a pixel to itself), which is what keeps the plain entries at their speed (profiles/window_fold_micro.txt).

// out[n][c][y][x] = unit(window pixel view_source(v, y, x)) for the slots first .. first + count - 1, the last slot repeated
// past the end of the lattice: the bits of _to_tensor(apply_view(window, v)).  One thread makes VEC pixels along the OUTPUT's x of
// all three planes, one VEC-wide store per plane, so the stores stay contiguous whatever the view.  VEC = 4 needs p % 4 == 0
// (16-byte aligned stores).  The reads of a thread's VEC pixels step along the image's x for an even r (backwards under a half
// turn or a mirror) and along its y, one image row apart, for an odd r; upright they are 3 * VEC neighbouring bytes, and
// neighbouring lanes read neighbouring bytes.  A source pixel is tested to lie inside the window before it becomes an address,
// like everything else here (upright it is (y, x + i) itself, inside by the thread's own index arithmetic).
template <int VEC, bool UPRIGHT>
__global__ __launch_bounds__(TL_BLOCK) void tl_gather_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ tops,
                                                             const int32_t* __restrict__ lefts, float* __restrict__ out, int H,
                                                             int W, int n_h, int n_w, int p, int n_views, uint32_t views, int first,
                                                             int count) {
    const int V = UPRIGHT ? 1 : n_views;
    const int pv = p / VEC;
    const long per_win = (long)p * pv;
    const long total = (long)count * per_win;
    const long plane = (long)p * p;
    const int last = n_h * n_w * V - 1;
    for (long idx = (long)blockIdx.x * TL_BLOCK + threadIdx.x; idx < total; idx += (long)gridDim.x * TL_BLOCK) {
        const int n = (int)(idx / per_win);
        const int r = (int)(idx - (long)n * per_win);
        const int y = r / pv, x = (r - y * pv) * VEC;
        int s = first + n;
        s = s > last ? last : s;
        const int k = s / V, v = UPRIGHT ? 0 : view_at(views, s - k * V);
        const int wi = k / n_w, wj = k - wi * n_w;
        int top = tops[wi], left = lefts[wj];
        top = top < 0 ? 0 : (top > H - p ? H - p : top);
        left = left < 0 ? 0 : (left > W - p ? W - p : left);
        const uint8_t* win = img + ((long)top * W + left) * 3;
        float val[3][VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
            const ViewPixel q = view_source(v, p, y, x + i);
            const bool in = UPRIGHT || view_inside(q, p);
            // (upright q is (y, x + i): written as a constant offset from one address, the thread's 3 * VEC bytes become one load)
            const uint8_t* src = UPRIGHT ? win + ((long)y * W + x) * 3 + i * 3 : win + ((long)q.y * W + q.x) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) val[c][i] = in ? byte_to_unit(src[c]) : 0.f;
        }
        float* dst = out + (long)n * 3 * plane + (long)y * p + x;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (VEC == 4) st4(dst + c * plane, make_float4(val[c][0], val[c][1], val[c][2], val[c][3]));
            else dst[c * plane] = val[c][0];
        }
    }
}

// pred [N][V][p][p][C], every prediction in the space of its view -> out[y][x][c] = mean over the covering windows and their
// views, in fp64.  One thread per output element (c fastest: loads and stores of neighbouring lanes are neighbours).  The lattice
// is sorted, so the covering windows are a range of rows times a range of columns: n_h + n_w comparisons find it (covering,
// lattice.hpp).  Per covering window (ascending, row-major) its views in list order, each read through view_inverse at an offset
// tested to lie in [0, p); the values are added as doubles onto 0.0 and divided once by their number, covering windows x V -- the
// order and the operations of infer_tile.combine_views_to_image (combine_patches_to_image for one upright view), hence its result
// bit for bit (adds and one IEEE division: nothing to contract).
template <bool UPRIGHT>
__global__ __launch_bounds__(TL_BLOCK) void tl_merge_kernel(const float* __restrict__ pred, const int32_t* __restrict__ tops,
                                                            const int32_t* __restrict__ lefts, double* __restrict__ out, int H,
                                                            int W, int C, int n_h, int n_w, int p, int n_views, uint32_t views,
                                                            int round_first) {
    const int V = UPRIGHT ? 1 : n_views;
    const long total = (long)H * W * C;
    const long WC = (long)W * C;
    for (long idx = (long)blockIdx.x * TL_BLOCK + threadIdx.x; idx < total; idx += (long)gridDim.x * TL_BLOCK) {
        const int y = (int)(idx / WC);
        const int r = (int)(idx - (long)y * WC);
        const int x = r / C, c = r - x * C;
        const Covering rows = covering(tops, n_h, y, p), cols = covering(lefts, n_w, x, p);
        double acc = 0.0;
        int cnt = 0;
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
                    float v = pred[(((slot + t) * p + q.y) * p + q.x) * C + c];
                    if (round_first) v = rintf(v);   // half to even: torch.round / np.round
                    acc += (double)v;
                    ++cnt;
                }
            }
        }
        out[idx] = acc / (double)cnt;
    }
}

}  // namespace

// (called with n_views = 1, views = 0 by the plain entries)
static int tl_gather(const uint8_t* img, const int32_t* tops, const int32_t* lefts, float* out, int H, int W, int n_h, int n_w, int p,
                     int n_views, uint32_t views, int first, int count, void* stream) {
    if (!img || !tops || !lefts || !out || p < 1 || p > H || p > W || n_h < 1 || n_w < 1 || first < 0 || count < 1 ||
        !views_ok(n_views, views) || (long)n_h * n_w * n_views > 0x7fffffffl)
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = p % 4 == 0, upright = n_views == 1 && views == 0;
    const dim3 grid(grid_stride_blocks((long)count * p * (p / (vec ? 4 : 1)), TL_BLOCK, TL_MAX_BLOCKS)), block(TL_BLOCK);
#define TL_L(VEC, UP) \
    WESUP_LAUNCH((tl_gather_kernel<VEC, UP>), grid, block, 0, st, img, tops, lefts, out, H, W, n_h, n_w, p, n_views, views, first, count)
    if (vec) {
        if (upright) TL_L(4, true);
        else TL_L(4, false);
    } else {
        if (upright) TL_L(1, true);
        else TL_L(1, false);
    }
#undef TL_L
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

static int tl_merge(const float* pred, const int32_t* tops, const int32_t* lefts, double* out, int H, int W, int C, int n_h, int n_w,
                    int p, int n_views, uint32_t views, int round_first, void* stream) {
    if (!pred || !tops || !lefts || !out || p < 1 || p > H || p > W || C < 1 || n_h < 1 || n_w < 1 || !views_ok(n_views, views) ||
        (long)n_h * n_w * n_views > 0x7fffffffl)
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(grid_stride_blocks((long)H * W * C, TL_BLOCK, TL_MAX_BLOCKS)), block(TL_BLOCK);
    const int rf = round_first ? 1 : 0;
    if (n_views == 1 && views == 0)
        WESUP_LAUNCH(tl_merge_kernel<true>, grid, block, 0, st, pred, tops, lefts, out, H, W, C, n_h, n_w, p, n_views, views, rf);
    else WESUP_LAUNCH(tl_merge_kernel<false>, grid, block, 0, st, pred, tops, lefts, out, H, W, C, n_h, n_w, p, n_views, views, rf);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_window_gather(const uint8_t* img, const int32_t* tops, const int32_t* lefts, float* out, int H, int W,
                                   int n_h, int n_w, int p, int first, int count, void* stream) {
    return tl_gather(img, tops, lefts, out, H, W, n_h, n_w, p, 1, 0u, first, count, stream);
}

extern "C" int wesup_window_gather_views(const uint8_t* img, const int32_t* tops, const int32_t* lefts, float* out, int H, int W,
                                         int n_h, int n_w, int p, int n_views, uint32_t views, int first, int count, void* stream) {
    return tl_gather(img, tops, lefts, out, H, W, n_h, n_w, p, n_views, views, first, count, stream);
}

extern "C" int wesup_window_merge(const float* pred, const int32_t* tops, const int32_t* lefts, double* out, int H, int W, int C,
                                  int n_h, int n_w, int p, int round_first, void* stream) {
    return tl_merge(pred, tops, lefts, out, H, W, C, n_h, n_w, p, 1, 0u, round_first, stream);
}

extern "C" int wesup_window_merge_views(const float* pred, const int32_t* tops, const int32_t* lefts, double* out, int H, int W,
                                        int C, int n_h, int n_w, int p, int n_views, uint32_t views, int round_first,
                                        void* stream) {
    return tl_merge(pred, tops, lefts, out, H, W, C, n_h, n_w, p, n_views, views, round_first, stream);
}
