// Polygon fill on the GPU: general polygons in fixed point -> label maps and class maps, equal to
// wesup_amd/raster.py:fill_host bit for bit (tests/test_raster_gpu.py).  Integer arithmetic only; the two places where threads
// meet on one word (a tile's toggle bits in LDS, a pixel's label) use an integer xor and an integer maximum, whose results do not
// depend on the order.
//
// A pixel's centre is (256 c + 128, 256 r + 128).  An edge with y0 < y1 toggles, in every centre row y0 <= Yc < y1, the columns
// from c* on (raster.hpp); a feature covers the pixels toggled an odd number of times; a pixel's label is 1 + its largest
// covering feature.  Clamping c* to the left edge of a rectangle keeps the parity inside it, so a feature's bounding box is cut
// into tiles of RS_TILE_ROWS x RS_TILE_COLS pixels, aligned to the image, that are filled on their own.
//
// wesup_polygon_fill, six launches whatever the data, seven with values (F = 0: two, three with values), no read-back:
//   two fills (labels, the status word)
//   rs_box_kernel      a block per feature: its CSR offsets, image index and vertices are checked (a bad feature sets the status
//                      bit and owns no tile: nothing of it is read again), its bounding box is reduced over the block, clipped to
//                      the image and cut into tiles; the tile count goes to the scan
//   rs_scan_blocks, rs_scan_small    the features' first tiles (64-bit, two levels: the block scan and the one-block scan of
//                      scan.hpp; the fill adds the block's offset itself) and the tile total
//   rs_fill_kernel     a fixed grid striding over the tiles: the tile's feature by bisection; the tile's toggle bits, 64 rows of
//                      one 64-bit word, zeroed in LDS; the block's threads walk the feature's edges ring by ring and xor one bit
//                      per crossed centre row; one thread per row turns the toggles into the parity prefix by six shifts; each
//                      wave then takes rows of 64 pixels, 256 contiguous bytes, and raises the labels of the set bits by atomicMax
//   rs_values_kernel   out8 = values[label - 1], 0 where the label is 0
#include "common.hpp"
#include "raster.hpp"
#include "scan.hpp"

#define RS_TILE_ROWS WESUP_RASTER_TILE_ROWS
#define RS_TILE_COLS WESUP_RASTER_TILE_COLS
#define RS_BLOCK WESUP_RASTER_BLOCK
#define RS_SCAN 1024
#define RS_FILL_BLOCKS 4096             // the fill kernel's grid: 256 CUs x 8 resident blocks of 256 threads, twice
#define RS_MAX_BLOCKS 65536             // the grid of the kernels that stride over features or pixels
#define RS_COORD_MAX (1 << 28)
#define RS_HDR_BYTES 256                // the tile total, 8 bytes at 0

static_assert(RS_TILE_COLS == 64, "a tile row is one 64-bit word and one wave's row segment");
static_assert(RS_TILE_ROWS <= RS_BLOCK && RS_BLOCK % 64 == 0 && 2 * RS_TILE_ROWS <= RS_BLOCK, "one thread per row word");

namespace {

typedef unsigned long long u64;

// box [F]: {first tile column, first tile row, tile columns, image}; cnt [F]: the feature's tiles
__global__ __launch_bounds__(RS_BLOCK) void rs_box_kernel(const int32_t* __restrict__ verts, const int32_t* __restrict__ ring_first,
                                                          const int32_t* __restrict__ ffr, const int32_t* __restrict__ fimg,
                                                          int4* __restrict__ box, u64* __restrict__ cnt, int32_t* __restrict__ status,
                                                          int B, int H, int W, int F, int R, int V) {
    __shared__ int sh[5][RS_BLOCK / 64];
    const int tid = threadIdx.x;
    for (int f = blockIdx.x; f < F; f += gridDim.x) {
        const int k0 = ffr[f], k1 = ffr[f + 1], img = fimg[f];
        int lb = k0 < 0 || k1 < k0 || k1 > R || (unsigned)img >= (unsigned)B;
        if (!lb)
            for (int k = k0 + tid; k < k1; k += RS_BLOCK) {
                const int a = ring_first[k], b = ring_first[k + 1];
                lb |= a < 0 || b < a || b > V;
            }
        const bool bad = __syncthreads_or(lb);                              // (also orders the last round's reads of sh before the writes below)
        int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = (int)0x80000000, ymax = (int)0x80000000, oob = 0;
        if (!bad && k1 > k0) {                                              // monotone offsets: the feature's vertices are one range inside [0, V)
            const int v0 = ring_first[k0], v1 = ring_first[k1];
            for (int i = v0 + tid; i < v1; i += RS_BLOCK) {
                const int2 p = ((const int2*)verts)[i];
                oob |= p.x < -RS_COORD_MAX || p.x > RS_COORD_MAX || p.y < -RS_COORD_MAX || p.y > RS_COORD_MAX;
                xmin = min(xmin, p.x);
                ymin = min(ymin, p.y);
                xmax = max(xmax, p.x);
                ymax = max(ymax, p.y);
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            xmin = min(xmin, __shfl_xor(xmin, off));
            ymin = min(ymin, __shfl_xor(ymin, off));
            xmax = max(xmax, __shfl_xor(xmax, off));
            ymax = max(ymax, __shfl_xor(ymax, off));
            oob |= __shfl_xor(oob, off);
        }
        if ((tid & 63) == 0) {
            const int w = tid >> 6;
            sh[0][w] = xmin; sh[1][w] = ymin; sh[2][w] = xmax; sh[3][w] = ymax; sh[4][w] = oob;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < RS_BLOCK / 64; ++w) {
                xmin = min(xmin, sh[0][w]);
                ymin = min(ymin, sh[1][w]);
                xmax = max(xmax, sh[2][w]);
                ymax = max(ymax, sh[3][w]);
                oob |= sh[4][w];
            }
            int4 bx = make_int4(0, 0, 0, 0);
            u64 n = 0;
            if (bad || oob) atomicOr(status, 1);
            else if (xmin <= xmax) {
                // the centres a feature can cover: ymin <= Yc < ymax and xmin <= Xc < xmax (behind xmax every crossing counts: even)
                const int r0 = max(0, rs_first_centre(ymin)), r1 = min(H, rs_first_centre(ymax));
                const int c0 = max(0, rs_first_centre(xmin)), c1 = min(W, rs_first_centre(xmax));
                if (r0 < r1 && c0 < c1) {
                    const int ty0 = r0 / RS_TILE_ROWS, nty = (r1 - 1) / RS_TILE_ROWS - ty0 + 1;
                    const int tx0 = c0 / RS_TILE_COLS, ntx = (c1 - 1) / RS_TILE_COLS - tx0 + 1;
                    bx = make_int4(tx0, ty0, ntx, img);
                    n = (u64)ntx * (u64)nty;
                }
            }
            box[f] = bx;
            cnt[f] = n;
        }
    }
}

// cnt [n] -> its exclusive scan inside every block of RS_SCAN, bsum [blocks] the blocks' totals
__global__ __launch_bounds__(RS_SCAN) void rs_scan_blocks(u64* __restrict__ cnt, u64* __restrict__ bsum, int n) {
    __shared__ u64 sh[RS_SCAN];
    const long i = (long)blockIdx.x * RS_SCAN + threadIdx.x;
    u64 tot;
    const u64 e = scan::block_scan<u64, RS_SCAN>(i < n ? cnt[i] : 0ull, sh, &tot);
    if (i < n) cnt[i] = e;
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(RS_SCAN) void rs_scan_small(u64* __restrict__ v, int n, u64* __restrict__ total_out) {
    u64 run;
    scan::scan_small<u64, RS_SCAN>(v, n, &run);
    if (threadIdx.x == 0) *total_out = run;
}

__global__ __launch_bounds__(RS_BLOCK) void rs_fill_kernel(const int32_t* __restrict__ verts, const int32_t* __restrict__ ring_first,
                                                           const int32_t* __restrict__ ffr, const int4* __restrict__ box,
                                                           const u64* __restrict__ first, const u64* __restrict__ bsum,
                                                           const u64* __restrict__ total_p, int32_t* __restrict__ labels, int H, int W,
                                                           int F) {
    __shared__ unsigned bits[RS_TILE_ROWS * 2];
    __shared__ u64 cover[RS_TILE_ROWS];
    const int tid = threadIdx.x;
    const u64 total = *total_p;
    const int2* __restrict__ v = (const int2*)verts;
    for (u64 t = blockIdx.x; t < total; t += gridDim.x) {
        // the last feature whose first tile is at or before t: it owns t, the features without tiles in front of it do not
        int lo = 0, hi = F - 1;
        while (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            if (bsum[mid / RS_SCAN] + first[mid] <= t) lo = mid;
            else hi = mid - 1;
        }
        const int f = lo;
        const int4 bx = box[f];
        const unsigned j = (unsigned)(t - (bsum[f / RS_SCAN] + first[f]));
        const int ntx = bx.z > 0 ? bx.z : 1;
        const int r0 = (bx.y + (int)(j / (unsigned)ntx)) * RS_TILE_ROWS, c0 = (bx.x + (int)(j % (unsigned)ntx)) * RS_TILE_COLS;
        const int r1 = min(H, r0 + RS_TILE_ROWS), c1 = min(W, c0 + RS_TILE_COLS);
        if (tid < RS_TILE_ROWS * 2) bits[tid] = 0u;
        __syncthreads();
        const int k0 = ffr[f], k1 = ffr[f + 1];
        for (int k = k0; k < k1; ++k) {
            const int a = ring_first[k], n = ring_first[k + 1] - a;
            for (int i = tid; i < n; i += RS_BLOCK) {
                const int2 p = v[a + i], q = v[a + (i + 1 == n ? 0 : i + 1)];
                if (min(p.x, q.x) > 256 * c1 - 128) continue;              // every c* of the edge is at or behind c1
                RsEdge e;
                if (!rs_edge_setup(p.x, p.y, q.x, q.y, r0, r1, e)) continue;
                for (int r = e.ra; r < e.rb; ++r) {
                    if (e.q < c1) {
                        const int c = max(e.q, c0) - c0;
                        atomicXor(&bits[(r - r0) * 2 + (c >> 5)], 1u << (c & 31));
                    }
                    rs_edge_step(e);
                }
            }
        }
        __syncthreads();
        if (tid < RS_TILE_ROWS) {
            u64 x = (u64)bits[2 * tid] | ((u64)bits[2 * tid + 1] << 32);
            x ^= x << 1;
            x ^= x << 2;
            x ^= x << 4;
            x ^= x << 8;
            x ^= x << 16;
            x ^= x << 32;
            cover[tid] = x;
        }
        __syncthreads();
        const int lane = tid & 63;
        int32_t* __restrict__ img = labels + (long)bx.w * H * W;
        if (r0 < r1 && c0 + lane < c1)
            for (int rr = tid >> 6; rr < r1 - r0; rr += RS_BLOCK / 64)
                if ((cover[rr] >> lane) & 1ull) atomicMax(&img[(long)(r0 + rr) * W + c0 + lane], f + 1);
        __syncthreads();
    }
}

__global__ __launch_bounds__(RS_BLOCK) void rs_values_kernel(const int32_t* __restrict__ labels, const uint8_t* __restrict__ values,
                                                             uint8_t* __restrict__ out8, long n, int F) {
    for (long i = (long)blockIdx.x * RS_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * RS_BLOCK) {
        const int l = labels[i];
        out8[i] = (l > 0 && l <= F) ? values[l - 1] : (uint8_t)0;
    }
}

// H, W <= 2^21: every vertex lies within +-2^20 pixels, and 256 W stays an int
inline bool bad_shape(int B, int H, int W) {
    return B <= 0 || H <= 0 || W <= 0 || H > (1 << 21) || W > (1 << 21) || (long)B * H * W >= (1l << 31);
}
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

struct Layout { size_t hdr, box, cnt, bsum, total; };
inline Layout layout(int F) {
    Layout L;
    size_t o = 0;
    L.hdr = o; o += RS_HDR_BYTES;
    L.box = o; o += align_up((size_t)F * 16, 256);
    L.cnt = o; o += align_up((size_t)F * 8, 256);
    L.bsum = o; o += align_up((size_t)ceil_div(F > 0 ? F : 1, RS_SCAN) * 8, 256);
    L.total = o;
    return L;
}

}  // namespace

extern "C" int wesup_raster_limit(int which) {
    return which == 0 ? RS_TILE_ROWS : which == 1 ? RS_TILE_COLS : which == 2 ? RS_BLOCK : which == 3 ? RS_COORD_MAX
         : which == 4 ? WESUP_RASTER_FRAC_BITS : which == 5 ? RS_FILL_BLOCKS : -1;
}

extern "C" size_t wesup_polygon_fill_workspace_bytes(int B, int H, int W, int F) {
    if (bad_shape(B, H, W) || F < 0 || F > 0x7fffffff - RS_SCAN) return 0;
    return layout(F).total;
}

extern "C" int wesup_polygon_fill(const int32_t* verts, const int32_t* ring_first, const int32_t* feature_first_ring,
                                  const int32_t* feature_image, const uint8_t* values, int32_t* labels, uint8_t* out8,
                                  int32_t* status, int B, int H, int W, int F, int R, int V, void* ws, size_t ws_bytes, void* stream) {
    if (!ring_first || !feature_first_ring || !labels || !status || !ws || bad_shape(B, H, W)) return WESUP_ERR_INVALID;
    if (F < 0 || R < 0 || V < 0 || F > 0x7fffffff - RS_SCAN || R == 0x7fffffff) return WESUP_ERR_INVALID;
    if ((F > 0 && !feature_image) || (V > 0 && !verts)) return WESUP_ERR_INVALID;
    if ((values != nullptr) != (out8 != nullptr) && !(F == 0 && out8)) return WESUP_ERR_INVALID;
    if (((uintptr_t)ws & 15) || ((uintptr_t)verts & 7) || ((uintptr_t)ring_first & 3) || ((uintptr_t)feature_first_ring & 3) ||
        ((uintptr_t)feature_image & 3) || ((uintptr_t)labels & 3) || ((uintptr_t)status & 3))
        return WESUP_ERR_INVALID;
    const Layout L = layout(F);
    if (ws_bytes < L.total) return WESUP_ERR_INVALID;
    const size_t N = (size_t)B * H * W;
    const void* ops[9] = {verts, ring_first, feature_first_ring, feature_image, values, labels, out8, status, ws};
    const size_t len[9] = {(size_t)V * 8, ((size_t)R + 1) * 4, ((size_t)F + 1) * 4, (size_t)F * 4, (size_t)F, N * 4, N, 4, L.total};
    for (int i = 0; i < 9; ++i)
        for (int j = i + 1; j < 9; ++j)
            if (ops[i] && ops[j] && len[i] && len[j] && overlap(ops[i], len[i], ops[j], len[j])) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    if (wesup_fill_words_(labels, 0u, N, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (wesup_fill_words_(status, 0u, 1, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (F > 0) {
        int4* box = (int4*)(w + L.box);
        u64* cnt = (u64*)(w + L.cnt);
        u64* bsum = (u64*)(w + L.bsum);
        u64* total = (u64*)(w + L.hdr);
        const int nblk = ceil_div(F, RS_SCAN);
        WESUP_LAUNCH(rs_box_kernel, dim3(F < RS_MAX_BLOCKS ? F : RS_MAX_BLOCKS), dim3(RS_BLOCK), 0, st, verts, ring_first,
                     feature_first_ring, feature_image, box, cnt, status, B, H, W, F, R, V);
        WESUP_LAUNCH(rs_scan_blocks, dim3(nblk), dim3(RS_SCAN), 0, st, cnt, bsum, F);
        WESUP_LAUNCH(rs_scan_small, dim3(1), dim3(RS_SCAN), 0, st, bsum, nblk, total);
        WESUP_LAUNCH(rs_fill_kernel, dim3(RS_FILL_BLOCKS), dim3(RS_BLOCK), 0, st, verts, ring_first, feature_first_ring,
                     (const int4*)box, (const u64*)cnt, (const u64*)bsum, (const u64*)total, labels, H, W, F);
    }
    if (out8)
        WESUP_LAUNCH(rs_values_kernel, dim3(grid_stride_blocks((long)N, RS_BLOCK, RS_MAX_BLOCKS)), dim3(RS_BLOCK), 0, st,
                     (const int32_t*)labels, values, out8, (long)N, F);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
