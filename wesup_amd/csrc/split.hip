// Splitting touching objects of a predicted mask on the GPU: a capped squared distance map, label growth from
// seeds and the one-pixel cut between grown labels.  Everything here is integer arithmetic on integer data and is held to the
// numpy restatement in wesup_amd/split.py bit for bit (tests/test_split_gpu.py).
//
// Every per-pixel kernel runs on the same grid: blocks of 256 threads = SP_ROWS rows of SP_SEG pixels, one wave per row, lanes
// along x; grid (ceil(W / SP_SEG), ceil(H / SP_ROWS), B).
//   1. sp_column_kernel  g[p] = distance to the nearest background pixel of p's column within dmax (the largest d with d^2 < cap),
//                        255 when there is none: one byte per pixel.  Reads of row y +- d are coalesced.
//   2. sp_row_kernel     D2[p] = min(cap, min over dx of dx^2 + g(y, x + dx)^2) from a row segment of g staged in LDS with a halo
//                        of dmax on either side (up to 254: wider than the segment, so the staging loop walks the whole staged
//                        range and asks every cell whether it lies inside the image); the scan runs outward in |dx| and stops as
//                        soon as dx^2 reaches the best value so far.  O(radius) per pixel.
//   3. sp_grow_kernel    temporal blocking of the synchronous growth rounds: a block stages a SP_TILE^2 tile and a halo of SP_HALO
//                        cells in LDS and runs T <= SP_HALO rounds there.  After t rounds the outer t rings of the staged region
//                        are stale (their neighbours outside the region were never seen); the tile itself, SP_HALO >= T cells in,
//                        is exact and is the only part written back.  A launch reads one label map and writes another, so no block
//                        sees a neighbour's half-finished round.
//   4. sp_cut_kernel     a pixel of label a is cleared when one of its eight neighbours carries a label 0 < b < a.
#include "common.hpp"

#define SP_SEG 64              // WESUP_SPLIT_SEG: pixels of a row per wave
#define SP_ROWS 4              // WESUP_SPLIT_ROWS
#define SP_MAX_REACH 254       // offsets d with d^2 < 65025
#define SP_TILE 32             // WESUP_SPLIT_TILE
#define SP_HALO 8              // WESUP_SPLIT_HALO = the most rounds of one launch
#define SP_SIDE (SP_TILE + 2 * SP_HALO)
#define SP_CELLS (SP_SIDE * SP_SIDE)
#define SP_PER (SP_CELLS / 256)

static_assert(SP_SEG == WESUP_SPLIT_SEG && SP_ROWS == WESUP_SPLIT_ROWS && SP_TILE == WESUP_SPLIT_TILE &&
              SP_HALO == WESUP_SPLIT_HALO, "include/wesup_hip.h names the tile constants");
static_assert(SP_SEG * SP_ROWS == 256 && SP_CELLS % 256 == 0 && SP_HALO % 2 == 0, "256-thread blocks, whole cells per thread");

namespace {

__global__ __launch_bounds__(256) void sp_column_kernel(const uint8_t* __restrict__ mask, uint8_t* __restrict__ g, int H, int W,
                                                        int dmax) {
    const int x = blockIdx.x * SP_SEG + (threadIdx.x & (SP_SEG - 1));
    const int y = blockIdx.y * SP_ROWS + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const long base = (long)blockIdx.z * H * W;
    const uint8_t* m = mask + base;
    const long p = (long)y * W + x;
    int v = 0;
    if (m[p] != 0) {
        v = 255;
        for (int d = 1; d <= dmax; ++d) {
            const bool up = y - d >= 0 && m[p - (long)d * W] == 0;
            const bool dn = y + d < H && m[p + (long)d * W] == 0;
            if (up || dn) { v = d; break; }
        }
    }
    g[base + p] = (uint8_t)v;
}

__global__ __launch_bounds__(256) void sp_row_kernel(const uint8_t* __restrict__ g, int32_t* __restrict__ d2, int H, int W, int cap,
                                                     int dmax) {
    __shared__ uint8_t gs[SP_ROWS][SP_SEG + 2 * SP_MAX_REACH + 4];
    const int lane = threadIdx.x & (SP_SEG - 1), r = threadIdx.x >> 6;
    const int x0 = blockIdx.x * SP_SEG, y = blockIdx.y * SP_ROWS + r;
    const long row = ((long)blockIdx.z * H + y) * W;
    const int span = SP_SEG + 2 * dmax;
    for (int i = lane; i < span; i += SP_SEG) {
        const int xx = x0 - dmax + i;
        gs[r][i] = (y < H && xx >= 0 && xx < W) ? g[row + xx] : (uint8_t)255;        // outside the image: not background
    }
    __syncthreads();
    const int x = x0 + lane;
    if (x >= W || y >= H) return;
    const int c = lane + dmax;
    const int g0 = gs[r][c];
    int best = min(cap, g0 * g0);
    for (int dx = 1; dx <= dmax && dx * dx < best; ++dx) {
        const int a = min((int)gs[r][c - dx], (int)gs[r][c + dx]);
        best = min(best, dx * dx + a * a);
    }
    d2[row + x] = best;
}

// cells: -1 background or outside the image, 0 foreground without a label, > 0 a label
__global__ __launch_bounds__(256) void sp_grow_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ in,
                                                      int32_t* __restrict__ out, int32_t* __restrict__ changed, int H, int W,
                                                      int T, int round0) {
    __shared__ int buf[2][SP_CELLS];
    const int tid = threadIdx.x;
    const int ty0 = blockIdx.y * SP_TILE - SP_HALO, tx0 = blockIdx.x * SP_TILE - SP_HALO;
    const long base = (long)blockIdx.z * H * W;
    unsigned was_zero = 0;
#pragma unroll
    for (int k = 0; k < SP_PER; ++k) {
        const int i = tid + k * 256;
        const int sy = i / SP_SIDE, sx = i - sy * SP_SIDE;
        const int y = ty0 + sy, x = tx0 + sx;
        int v = -1;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const long p = base + (long)y * W + x;
            if (mask[p] != 0) v = max(in[p], 0);
        }
        buf[0][i] = v;
        if (v == 0) was_zero |= 1u << k;
    }
    int cur = 0;
    if (__syncthreads_or(was_zero != 0)) {
        int quiet = 0;
        for (int t = 0; t < T; ++t) {
            const bool eight = ((round0 + t) & 1) == 0;     // odd rounds: 4-neighbourhood, even rounds: 8-neighbourhood
            const int* src = buf[cur];
            int* dst = buf[cur ^ 1];
            int took = 0;
#pragma unroll
            for (int k = 0; k < SP_PER; ++k) {
                const int i = tid + k * 256;
                int v = src[i];
                if (v == 0) {
                    const int sy = i / SP_SIDE, sx = i - sy * SP_SIDE;
                    const bool u = sy > 0, d = sy < SP_SIDE - 1, l = sx > 0, rr = sx < SP_SIDE - 1;
                    unsigned m = 0xffffffffu;                // no positive neighbour yet: above every label, 2^31 - 1 included
                    int n;
                    if (u) { n = src[i - SP_SIDE]; if (n > 0) m = min(m, (unsigned)n); }
                    if (d) { n = src[i + SP_SIDE]; if (n > 0) m = min(m, (unsigned)n); }
                    if (l) { n = src[i - 1]; if (n > 0) m = min(m, (unsigned)n); }
                    if (rr) { n = src[i + 1]; if (n > 0) m = min(m, (unsigned)n); }
                    if (eight) {
                        if (u && l) { n = src[i - SP_SIDE - 1]; if (n > 0) m = min(m, (unsigned)n); }
                        if (u && rr) { n = src[i - SP_SIDE + 1]; if (n > 0) m = min(m, (unsigned)n); }
                        if (d && l) { n = src[i + SP_SIDE - 1]; if (n > 0) m = min(m, (unsigned)n); }
                        if (d && rr) { n = src[i + SP_SIDE + 1]; if (n > 0) m = min(m, (unsigned)n); }
                    }
                    if (m != 0xffffffffu) { v = (int)m; took = 1; }
                }
                dst[i] = v;
            }
            cur ^= 1;
            // (the barrier of the round.)  Two rounds in a row without a new label, one of either kind: the staged region is at its
            // own fixed point and the remaining rounds would copy it
            if (__syncthreads_or(took)) quiet = 0;
            else if (++quiet == 2) break;
        }
    }
    const int* fin = buf[cur];
    int grew = 0;
#pragma unroll
    for (int k = 0; k < SP_PER; ++k) {
        const int i = tid + k * 256;
        const int sy = i / SP_SIDE, sx = i - sy * SP_SIDE;
        const int y = ty0 + sy, x = tx0 + sx;
        if (sy < SP_HALO || sy >= SP_HALO + SP_TILE || sx < SP_HALO || sx >= SP_HALO + SP_TILE || y >= H || x >= W) continue;
        const int v = fin[i];
        out[base + (long)y * W + x] = v > 0 ? v : 0;
        if (((was_zero >> k) & 1u) && v > 0) grew = 1;
    }
    if (__syncthreads_or(grew) && tid == 0) *changed = 1;   // a plain store: every block that writes writes the same word
}

__global__ __launch_bounds__(256) void sp_cut_kernel(const uint8_t* __restrict__ mask, const int32_t* __restrict__ labels,
                                                     uint8_t* __restrict__ out, int H, int W) {
    const int x = blockIdx.x * SP_SEG + (threadIdx.x & (SP_SEG - 1));
    const int y = blockIdx.y * SP_ROWS + (threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const long base = (long)blockIdx.z * H * W;
    const int32_t* lab = labels + base;
    const long p = (long)y * W + x;
    int v = 0;
    if (mask[base + p] != 0) {
        v = 1;
        const int a = lab[p];
        if (a > 0) {
            for (int dy = -1; dy <= 1; ++dy) {
                const int yy = y + dy;
                if (yy < 0 || yy >= H) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const int xx = x + dx;
                    if (xx < 0 || xx >= W) continue;
                    const int b = lab[(long)yy * W + xx];
                    if (b > 0 && b < a) v = 0;
                }
            }
        }
    }
    out[base + p] = (uint8_t)v;
}

inline bool bad_image(int B, int H, int W) {
    return B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || (long)H * W >= (1l << 30) ||
           (long)B * H * W >= (1l << 40);
}
// na bytes at a and nb bytes at b share a byte
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}
inline dim3 pixel_grid(int B, int H, int W) { return dim3(ceil_div(W, SP_SEG), ceil_div(H, SP_ROWS), B); }

}  // namespace

extern "C" size_t wesup_edt_sq_workspace_bytes(int B, int H, int W) {
    if (bad_image(B, H, W)) return 0;
    return align_up((size_t)B * H * W, 256);                                    // the column distances, one byte per pixel
}

extern "C" int wesup_edt_sq(const uint8_t* mask, int32_t* d2, int B, int H, int W, int cap, void* ws, size_t ws_bytes,
                            void* stream) {
    if (!mask || !d2 || !ws || bad_image(B, H, W) || cap < 1 || cap > 255 * 255) return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_edt_sq_workspace_bytes(B, H, W)) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    int dmax = 0;
    while ((dmax + 1) * (dmax + 1) < cap) ++dmax;           // offsets with d^2 < cap: at most SP_MAX_REACH
    uint8_t* g = (uint8_t*)ws;
    WESUP_LAUNCH(sp_column_kernel, pixel_grid(B, H, W), dim3(256), 0, st, mask, g, H, W, dmax);
    WESUP_LAUNCH(sp_row_kernel, pixel_grid(B, H, W), dim3(256), 0, st, (const uint8_t*)g, d2, H, W, cap, dmax);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_label_grow_workspace_bytes(int B, int H, int W) {
    if (bad_image(B, H, W)) return 0;
    return align_up((size_t)B * H * W * 4, 256);                                // the other label map of the ping-pong
}

extern "C" int wesup_label_grow(const uint8_t* mask, const int32_t* seeds, int32_t* labels, int32_t* changed, int B, int H, int W,
                                int first_round, int launches, int rounds, void* ws, size_t ws_bytes, void* stream) {
    if (!mask || !seeds || !labels || !changed || !ws || bad_image(B, H, W) || first_round < 1 || launches < 1 ||
        launches > 65536 || rounds < 2 || rounds > SP_HALO || (rounds & 1))
        return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_label_grow_workspace_bytes(B, H, W)) return WESUP_ERR_INVALID;
    // a launch reads one map while its blocks write another: seeds, labels and the workspace are three maps, none of them the mask
    const size_t nm = (size_t)B * H * W, nl = 4 * nm;
    if (overlap(seeds, nl, labels, nl) || overlap(seeds, nl, ws, nl) || overlap(labels, nl, ws, nl) ||
        overlap(mask, nm, labels, nl) || overlap(mask, nm, ws, nl) || overlap(changed, 4, labels, nl) ||
        overlap(changed, 4, ws, nl))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(ceil_div(W, SP_TILE), ceil_div(H, SP_TILE), B);
    const int32_t* src = seeds;
    for (int i = 0; i < launches; ++i) {
        int32_t* dst = ((launches - 1 - i) & 1) ? (int32_t*)ws : labels;        // the last launch writes `labels`
        // the word reports the LAST launch alone: a launch holds a round of either kind, so one that changed nothing stands at
        // the fixed point whatever the launches before it did
        if (i == launches - 1 && wesup_fill_words_(changed, 0u, 1, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
        // (rounds is even: the parity of the first round of every launch is that of first_round)
        WESUP_LAUNCH(sp_grow_kernel, grid, dim3(256), 0, st, mask, src, dst, changed, H, W, rounds, first_round & 1);
        src = dst;
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_label_cut(const uint8_t* mask, const int32_t* labels, uint8_t* out, int B, int H, int W, void* stream) {
    if (!mask || !labels || !out || bad_image(B, H, W)) return WESUP_ERR_INVALID;
    const size_t np = (size_t)B * H * W;
    if (overlap(mask, np, out, np) || overlap(labels, 4 * np, out, np)) return WESUP_ERR_INVALID;
    WESUP_LAUNCH(sp_cut_kernel, pixel_grid(B, H, W), dim3(256), 0, (hipStream_t)stream, mask, labels, out, H, W);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
