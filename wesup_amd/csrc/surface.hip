// Surface-distance metrics on the GPU: an exact, uncapped squared Euclidean distance map, the 4-neighbour border
// of a mask, and the reductions HD, HD95, ASSD and NSD are made of.  Integer arithmetic on integer data wherever a value is
// compared, held to the numpy restatement in wesup_amd/surface.py bit for bit (tests/test_surface_gpu.py); the two sums of square
// roots are float64 with one owner and a fixed order each, no floating-point atomic, so two runs give the same bits.
//
// The distance map, three launches whatever the data:
//   1. edt_bits_kernel    one thread per column and chunk of ED_CHUNK = 64 rows: the chunk's background pixels as the bits of one
//                         64-bit word.  Lanes along x, so every row read is coalesced.
//   2. edt_column_kernel  the same thread turns its word into the 64 column distances of its rows: the nearest background pixel
//                         above row r is the highest set bit at or below r, the nearest below the lowest at or above it; a chunk
//                         without one on that side takes it from the nearest chunk word that has a bit (at most H / 64 words each
//                         way).  Stored squared, ED_NONE where the column has no background at all.
//   3. edt_row_kernel     d2(x) = min over x' of (x - x')^2 + g2(x'): the scan runs outward in |dx| and stops as soon as dx^2
//                         reaches the best value so far -- no candidate further out can be smaller.  O(W) per pixel at worst
//                         (one background pixel in a corner), O(distance) otherwise.  The row is read through the cache: a wave's
//                         64 lanes read 64 consecutive words that slide by one per step, and a row of the widest legal image does
//                         not fit the LDS.
// Every legal candidate fits int32: (H-1)^2 + (W-1)^2 < ED_NONE is a condition of the entry; sums with an ED_NONE term are taken in
// unsigned arithmetic (below 2^32) and clamped.
//
// The statistics of an image pair, for B pairs at once:
//   ss_partial_kernel     walks the pixels: counts, maxima, counts within the tolerance and the float64 sums of the roots per
//                         direction, per thread in index order, folded by a fixed tree in LDS, one partial row per block; and the
//                         key array of the pair for the order statistics, d2 at the border pixels and ED_NONE elsewhere (2 HW keys:
//                         the padding sorts behind every real key, so ranks below n_p + n_g never see it).
//   ss_final_kernel       one block per pair folds the partial rows by the same tree, writes the block and derives the two ranks
//                         from n_p + n_g -- on the device, so nothing is read back before the selection.
//   (radix select)        the stain module's, on the keys as bit patterns (stain.hip, wesup_select_i32).
//   ss_widen_kernel       the two selected keys into the block as int64.
#include <math.h>
#include <string.h>
#include "common.hpp"

#define ED_CHUNK WESUP_EDT_CHUNK
#define ED_COLS WESUP_EDT_COLS
#define ED_SEG WESUP_EDT_SEG
#define ED_ROWS WESUP_EDT_ROWS
#define ED_NONE WESUP_EDT_NONE
#define SS_BLOCK 256
#define SS_MAX_BLOCKS 256               // partial rows per pair at most
#define SS_INTS 6                       // n_p, n_g, max_pg, max_gp, within_p, within_g
#define SS_ROW 8                        // ... and the two sums: 8-byte slots of a partial row
#define SS_STATS WESUP_SURFACE_STATS

static_assert(ED_CHUNK == 64, "a chunk of the column pass is the bits of one 64-bit word");
static_assert(ED_SEG * ED_ROWS == 256 && ED_COLS == 256, "256-thread blocks");
static_assert(SS_STATS == SS_ROW + 2, "the block: a partial row's eight quantities and the two order statistics");

namespace {

__global__ __launch_bounds__(ED_COLS) void edt_bits_kernel(const uint8_t* __restrict__ mask, unsigned long long* __restrict__ zb,
                                                           int H, int W, int nch, int invert) {
    const int x = blockIdx.x * ED_COLS + threadIdx.x, c = blockIdx.y;
    if (x >= W) return;
    const int y0 = c * ED_CHUNK;
    const int rows = min(ED_CHUNK, H - y0);
    const uint8_t* m = mask + (long)blockIdx.z * H * W + (long)y0 * W + x;
    unsigned long long z = 0ull;
#pragma unroll 8
    for (int r = 0; r < rows; ++r) {
        const bool fg = (m[(long)r * W] != 0) != (invert != 0);
        if (!fg) z |= 1ull << r;
    }
    zb[((long)blockIdx.z * nch + c) * W + x] = z;               // rows past H: not background
}

__global__ __launch_bounds__(ED_COLS) void edt_column_kernel(const unsigned long long* __restrict__ zb, int32_t* __restrict__ g2,
                                                             int H, int W, int nch) {
    const int x = blockIdx.x * ED_COLS + threadIdx.x, c = blockIdx.y;
    if (x >= W) return;
    const unsigned long long* zc = zb + (long)blockIdx.z * nch * W + x;
    const unsigned long long z = zc[(long)c * W];
    const int y0 = c * ED_CHUNK;
    const int rows = min(ED_CHUNK, H - y0);
    int above = -1, below = -1;                                 // rows of the nearest background pixels outside the chunk
    for (int cc = c - 1; cc >= 0; --cc) {
        const unsigned long long v = zc[(long)cc * W];
        if (v) { above = cc * ED_CHUNK + 63 - __clzll((long long)v); break; }
    }
    for (int cc = c + 1; cc < nch; ++cc) {
        const unsigned long long v = zc[(long)cc * W];
        if (v) { below = cc * ED_CHUNK + __ffsll(v) - 1; break; }
    }
    int32_t* out = g2 + (long)blockIdx.z * H * W + (long)y0 * W + x;
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        const unsigned long long lo = z & (~0ull >> (63 - r)), hi = z >> r;
        const int ya = lo ? y0 + 63 - __clzll((long long)lo) : above;
        const int yb = hi ? y + __ffsll(hi) - 1 : below;
        int d = 0x7fffffff;
        if (ya >= 0) d = y - ya;
        if (yb >= 0) d = min(d, yb - y);
        out[(long)r * W] = d == 0x7fffffff ? ED_NONE : d * d;   // d <= H - 1 <= 46340: the square fits
    }
}

__global__ __launch_bounds__(256) void edt_row_kernel(const int32_t* __restrict__ g2, int32_t* __restrict__ d2, int H, int W) {
    const int x = blockIdx.x * ED_SEG + (threadIdx.x & (ED_SEG - 1));
    const int y = blockIdx.y * ED_ROWS + threadIdx.x / ED_SEG;
    if (x >= W || y >= H) return;
    const long base = ((long)blockIdx.z * H + y) * W;
    const int32_t* row = g2 + base;
    unsigned best = (unsigned)row[x];
    const int reach = max(x, W - 1 - x);
    for (int dx = 1; dx <= reach; ++dx) {
        const unsigned dd = (unsigned)dx * (unsigned)dx;
        if (dd >= best) break;
        unsigned a = (unsigned)ED_NONE;                         // outside the image: not background
        if (x - dx >= 0) a = (unsigned)row[x - dx];
        if (x + dx < W) a = min(a, (unsigned)row[x + dx]);
        best = min(best, dd + a);                               // dd < best <= 2^31 - 1 and a <= 2^31 - 1: no wrap
    }
    d2[base + x] = (int32_t)min(best, (unsigned)ED_NONE);
}

__global__ __launch_bounds__(256) void border_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ out, int H, int W) {
    const int x = blockIdx.x * ED_SEG + (threadIdx.x & (ED_SEG - 1));
    const int y = blockIdx.y * ED_ROWS + threadIdx.x / ED_SEG;
    if (x >= W || y >= H) return;
    const long base = (long)blockIdx.z * H * W;
    const uint8_t* m = mask + base;
    const long p = (long)y * W + x;
    int v = 0;
    if (m[p] != 0)
        v = y == 0 || x == 0 || y == H - 1 || x == W - 1 || m[p - W] == 0 || m[p + W] == 0 || m[p - 1] == 0 || m[p + 1] == 0;
    out[base + p] = (uint8_t)v;
}

// the eight quantities of a partial row, folded over the 256 threads of a block by a fixed tree: thread 0 holds the result
struct SsAcc {
    long v[SS_INTS];
    double s[2];
};
__device__ __forceinline__ void ss_fold(SsAcc& a, long (*li)[SS_BLOCK], double (*ld)[SS_BLOCK]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < SS_INTS; ++k) li[k][t] = a.v[k];
    ld[0][t] = a.s[0];
    ld[1][t] = a.s[1];
    __syncthreads();
    for (int s = SS_BLOCK / 2; s >= 1; s >>= 1) {
        if (t < s) {
            li[0][t] += li[0][t + s];
            li[1][t] += li[1][t + s];
            li[2][t] = max(li[2][t], li[2][t + s]);
            li[3][t] = max(li[3][t], li[3][t + s]);
            li[4][t] += li[4][t + s];
            li[5][t] += li[5][t + s];
            ld[0][t] += ld[0][t + s];
            ld[1][t] += ld[1][t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < SS_INTS; ++k) a.v[k] = li[k][0];
    a.s[0] = ld[0][0];
    a.s[1] = ld[1][0];
}

// grid (blocks, B).  partial [B][blocks][SS_ROW] 8-byte slots, keys [B][2 HW]
__global__ __launch_bounds__(SS_BLOCK) void ss_partial_kernel(const uint8_t* __restrict__ bp, const uint8_t* __restrict__ bg,
                                                              const int32_t* __restrict__ d_to_g, const int32_t* __restrict__ d_to_p,
                                                              long HW, long t2, int32_t* __restrict__ keys, long* __restrict__ partial) {
    __shared__ long li[SS_INTS][SS_BLOCK];
    __shared__ double ld[2][SS_BLOCK];
    const long base = (long)blockIdx.y * HW;
    bp += base; bg += base; d_to_g += base; d_to_p += base;
    int32_t* kp = keys + 2 * base;
    int32_t* kg = kp + HW;
    SsAcc a;
#pragma unroll
    for (int k = 0; k < SS_INTS; ++k) a.v[k] = 0;
    a.s[0] = a.s[1] = 0.0;
    const long stride = (long)gridDim.x * SS_BLOCK;
    for (long i = (long)blockIdx.x * SS_BLOCK + threadIdx.x; i < HW; i += stride) {
        int vp = ED_NONE, vg = ED_NONE;
        if (bp[i] != 0) {
            vp = d_to_g[i];
            a.v[0] += 1;
            a.v[2] = max(a.v[2], (long)vp);
            a.v[4] += (long)vp <= t2;
            a.s[0] += sqrt((double)vp);
        }
        if (bg[i] != 0) {
            vg = d_to_p[i];
            a.v[1] += 1;
            a.v[3] = max(a.v[3], (long)vg);
            a.v[5] += (long)vg <= t2;
            a.s[1] += sqrt((double)vg);
        }
        kp[i] = vp;
        kg[i] = vg;
    }
    ss_fold(a, li, ld);
    if (threadIdx.x == 0) {
        long* row = partial + ((long)blockIdx.y * gridDim.x + blockIdx.x) * SS_ROW;
#pragma unroll
        for (int k = 0; k < SS_INTS; ++k) row[k] = a.v[k];
        row[6] = __double_as_longlong(a.s[0]);
        row[7] = __double_as_longlong(a.s[1]);
    }
}

// grid (1, B).  stats [B][SS_STATS] 8-byte slots, ranks [B][2]
__global__ __launch_bounds__(SS_BLOCK) void ss_final_kernel(const long* __restrict__ partial, int blocks, long q_frac_bits,
                                                            long* __restrict__ stats, long* __restrict__ ranks) {
    __shared__ long li[SS_INTS][SS_BLOCK];
    __shared__ double ld[2][SS_BLOCK];
    const int b = blockIdx.y, t = threadIdx.x;
    SsAcc a;
#pragma unroll
    for (int k = 0; k < SS_INTS; ++k) a.v[k] = 0;
    a.s[0] = a.s[1] = 0.0;
    if (t < blocks) {
        const long* row = partial + ((long)b * blocks + t) * SS_ROW;
#pragma unroll
        for (int k = 0; k < SS_INTS; ++k) a.v[k] = row[k];
        a.s[0] = __longlong_as_double(row[6]);
        a.s[1] = __longlong_as_double(row[7]);
    }
    ss_fold(a, li, ld);
    if (t == 0) {
        long* out = stats + (long)b * SS_STATS;
#pragma unroll
        for (int k = 0; k < SS_INTS; ++k) out[k] = a.v[k];
        out[6] = 0;
        out[7] = 0;
        out[8] = __double_as_longlong(a.s[0]);
        out[9] = __double_as_longlong(a.s[1]);
        const long n = a.v[0] + a.v[1];
        long k = 0, k1 = 0;
        if (n > 0) {
            k = (long)floor((double)(n - 1) * __longlong_as_double(q_frac_bits));      // the host's float64 product
            k = k < 0 ? 0 : (k > n - 1 ? n - 1 : k);
            k1 = k + 1 < n ? k + 1 : n - 1;
        }
        ranks[2 * b] = k;
        ranks[2 * b + 1] = k1;
    }
}

__global__ void ss_widen_kernel(const int32_t* __restrict__ sel, long* __restrict__ stats, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    long* out = stats + (long)b * SS_STATS;
    const bool any = out[0] + out[1] > 0;
    out[6] = any ? (long)sel[2 * b] : 0;
    out[7] = any ? (long)sel[2 * b + 1] : 0;
}

// the shapes split.hip's entries take ...
inline bool bad_image(int B, int H, int W) {
    return B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || (long)H * W >= (1l << 30) ||
           (long)B * H * W >= (1l << 40);
}
// ... whose largest possible squared distance stays below ED_NONE
inline bool bad_edt(int B, int H, int W) {
    return bad_image(B, H, W) || (long)(H - 1) * (H - 1) + (long)(W - 1) * (W - 1) >= (long)ED_NONE;
}
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
inline dim3 pixel_grid(int B, int H, int W) { return dim3(ceil_div(W, ED_SEG), ceil_div(H, ED_ROWS), B); }

struct EdtLayout { size_t bits, g2, total; };
inline EdtLayout edt_layout(int B, int H, int W) {
    EdtLayout L;
    L.bits = 0;
    L.g2 = align_up((size_t)B * ceil_div(H, ED_CHUNK) * W * 8, 256);
    L.total = L.g2 + align_up((size_t)B * H * W * 4, 256);
    return L;
}

struct StatsLayout { size_t partial, ranks, sel, keys, select, total; };
inline unsigned ss_blocks(long HW) { return grid_stride_blocks(HW, SS_BLOCK, SS_MAX_BLOCKS); }
inline StatsLayout stats_layout(int B, int H, int W) {
    const long HW = (long)H * W;
    StatsLayout L;
    size_t o = 0;
    L.partial = o; o += align_up((size_t)B * ss_blocks(HW) * SS_ROW * 8, 256);
    L.ranks = o; o += align_up((size_t)B * 2 * 8, 256);
    L.sel = o; o += align_up((size_t)B * 2 * 4, 256);
    L.keys = o; o += align_up((size_t)B * 2 * HW * 4, 256);
    L.select = o; o += align_up(wesup_select_workspace_bytes_(2 * HW, B), 256);
    L.total = o;
    return L;
}

}  // namespace

extern "C" size_t wesup_edt_full_workspace_bytes(int B, int H, int W) {
    if (bad_edt(B, H, W)) return 0;
    return edt_layout(B, H, W).total;
}

extern "C" int wesup_edt_full(const uint8_t* mask, int32_t* d2, int B, int H, int W, int invert, void* ws, size_t ws_bytes,
                              void* stream) {
    if (!mask || !d2 || !ws || bad_edt(B, H, W) || (invert != 0 && invert != 1) || ((uintptr_t)ws & 7) || ((uintptr_t)d2 & 3))
        return WESUP_ERR_INVALID;
    const EdtLayout L = edt_layout(B, H, W);
    if (ws_bytes < L.total) return WESUP_ERR_INVALID;
    const size_t np = (size_t)B * H * W;
    if (overlap(mask, np, d2, 4 * np) || overlap(mask, np, ws, L.total) || overlap(d2, 4 * np, ws, L.total)) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* zb = (unsigned long long*)((char*)ws + L.bits);
    int32_t* g2 = (int32_t*)((char*)ws + L.g2);
    const int nch = ceil_div(H, ED_CHUNK);
    const dim3 cgrid(ceil_div(W, ED_COLS), nch, B);
    WESUP_LAUNCH(edt_bits_kernel, cgrid, dim3(ED_COLS), 0, st, mask, zb, H, W, nch, invert);
    WESUP_LAUNCH(edt_column_kernel, cgrid, dim3(ED_COLS), 0, st, (const unsigned long long*)zb, g2, H, W, nch);
    WESUP_LAUNCH(edt_row_kernel, pixel_grid(B, H, W), dim3(256), 0, st, (const int32_t*)g2, d2, H, W);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_mask_border(const uint8_t* mask, uint8_t* out, int B, int H, int W, void* stream) {
    if (!mask || !out || bad_image(B, H, W)) return WESUP_ERR_INVALID;
    const size_t np = (size_t)B * H * W;
    if (overlap(mask, np, out, np)) return WESUP_ERR_INVALID;
    WESUP_LAUNCH(border_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, mask, out, H, W);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_surface_stats_workspace_bytes(int B, int H, int W) {
    if (bad_edt(B, H, W)) return 0;
    return stats_layout(B, H, W).total;
}

extern "C" int wesup_surface_stats(const uint8_t* border_p, const uint8_t* border_g, const int32_t* d2_to_g, const int32_t* d2_to_p,
                                   void* stats, int B, int H, int W, long t2, long q_frac_bits, void* ws, size_t ws_bytes,
                                   void* stream) {
    if (!border_p || !border_g || !d2_to_g || !d2_to_p || !stats || !ws || bad_edt(B, H, W) || t2 < 0) return WESUP_ERR_INVALID;
    if (((uintptr_t)stats & 7) || ((uintptr_t)ws & 15) || ((uintptr_t)d2_to_g & 3) || ((uintptr_t)d2_to_p & 3)) return WESUP_ERR_INVALID;
    double qf;
    memcpy(&qf, &q_frac_bits, sizeof qf);
    if (!(qf >= 0.0 && qf <= 1.0)) return WESUP_ERR_INVALID;
    const StatsLayout L = stats_layout(B, H, W);
    if (ws_bytes < L.total) return WESUP_ERR_INVALID;
    const size_t np = (size_t)B * H * W, nst = (size_t)B * SS_STATS * 8;
    if (overlap(stats, nst, ws, L.total) || overlap(border_p, np, ws, L.total) || overlap(border_g, np, ws, L.total) ||
        overlap(d2_to_g, 4 * np, ws, L.total) || overlap(d2_to_p, 4 * np, ws, L.total) || overlap(stats, nst, border_p, np) ||
        overlap(stats, nst, border_g, np) || overlap(stats, nst, d2_to_g, 4 * np) || overlap(stats, nst, d2_to_p, 4 * np))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W;
    const unsigned blocks = ss_blocks(HW);
    char* w = (char*)ws;
    long* partial = (long*)(w + L.partial);
    long* ranks = (long*)(w + L.ranks);
    int32_t* sel = (int32_t*)(w + L.sel);
    int32_t* keys = (int32_t*)(w + L.keys);
    WESUP_LAUNCH(ss_partial_kernel, dim3(blocks, B), dim3(SS_BLOCK), 0, st, border_p, border_g, d2_to_g, d2_to_p, HW, t2, keys,
                 partial);
    WESUP_LAUNCH(ss_final_kernel, dim3(1, B), dim3(SS_BLOCK), 0, st, (const long*)partial, (int)blocks, q_frac_bits, (long*)stats,
                 ranks);
    // non-negative int32 keys as the bit patterns of floats: the select's key map is a pure bit map on them (wesup_select_i32)
    wesup_select_launch_((const float*)keys, 2 * HW, 2 * HW, (const long*)ranks, 2, 2, (float*)sel, 2, B, w + L.select, st);
    WESUP_LAUNCH(ss_widen_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, st, (const int32_t*)sel, (long*)stats, B);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
