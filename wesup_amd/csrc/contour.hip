// Object outlines on the GPU: the ordered boundary rings of a label map, equal to the sequential tracer
// wesup_amd/contour.py:trace_host word for word (tests/test_contour_gpu.py).  Integer arithmetic only; the two places where
// threads meet on one word (a ring's bounding box and area) use integer atomics, whose result does not depend on the order.
//
// A crack is a unit edge between a pixel of label l > 0 and a 4-neighbour of another label (or the outside), directed with
// the pixel on its left; side = direction: 0 N (going west), 1 W (south), 2 S (east), 3 E (north), so d - 1 is the right turn
// and d + 1 the left turn.  Everything a crack needs from the map is the 2 x 2 pixels around one of its end points:
//   leaving a vertex:   west  SW && !NW    south SE && !SW    east NE && !SE    north NW && !NE      (X: pixel X has label l)
//   arriving at it:     west  SE && !NE    south NE && !NW    east NW && !SW    north SW && !SE
// the successor is the first of right, straight, left that leaves the crack's end point; the crack's start is a corner
// unless a crack arrives there straight and nothing leaves to that crack's right (then that crack is the predecessor).
//
// wesup_contour_count, two launches: the header fill and
//   ct_mask_kernel     per pixel the four crack bits and the four corner bits in one byte; the block's crack count for the scan;
//                      per-image cracks and corners by integer atomics, one pair per block.
// wesup_contour_trace, 18 + ceil(log2 n_cracks) launches whatever the data (n = n_cracks):
//   two fills (header, n_rings), ct_mask_kernel, sc_small (block counts), ct_check_kernel (the totals against n_cracks / n_corners: every later
//   kernel returns at once unless they agree, so no index ever passes a capacity)
//   ct_pfx_kernel      per pixel the compact index of its first crack: cracks are numbered in slot order
//   ct_link_kernel     per crack {successor, successor, 1, 0} and its slot
//   ct_double_kernel   x ceil(log2 n): element {nxt, m, off} of crack e describes the 2^k steps after e: where they end, the
//                      smallest crack index among them and the step at which it first occurs.  Two elements combine into the
//                      next power; once 2^k covers the ring m is the leader and off the distance to it (the ring length at the
//                      leader itself).  One 16-byte element per crack and round, read once in order and once through nxt.
//   ct_ring_kernel     position in the ring, and the scan key of the leaders: (1 << 32) | length
//   sc_block_sums, sc_small, sc_apply    ring ids and the rings' first crack in ring order, one 64-bit scan (the three passes of
//                      scan.hpp here and below; ct_pfx_kernel above is its apply pass over the crack counts)
//   ct_check2_kernel   rings against ring_cap
//   ct_place_kernel    ring order: the crack of every place, the corner flag of every place; the leaders start their records
//   sc_block_sums, sc_small, sc_apply    vertex indices: the scan of the corner flags in ring order
//   ct_emit_kernel     one thread per place: vertices, bounding boxes, areas; a wave inside one ring folds first
//
// wesup_contour_simplify, seven launches whatever the data: the exact Douglas-Peucker of contour.py:simplify_host
//   fill (counts), sp_validate_kernel (the records' vertex ranges; every later kernel is a no-op unless they are consecutive)
//   sp_simplify_kernel one block per ring, the blocks striding over the rings: anchors, then level after level every vertex of a
//                      live piece measures itself against the piece's chord, the piece's maximum by a 64-bit atomicMax, the tie
//                      rule by a 64-bit atomicMin, split or retire; the live vertices are kept as a compact list, so a level
//                      costs what is still live.  State in LDS up to SP_LDS_N vertices, in the workspace above.
//   sc_block_sums, sc_small, sc_apply    the scan of the keep flags: the output index of every kept vertex
//   sp_emit_kernel     kept vertices to their places, every record's first vertex, the total
#include "common.hpp"
#include "scan.hpp"

#define CT_SCAN 1024
#define CT_BLOCK 256
#define CT_RING WESUP_CONTOUR_RING
#define CT_HDR_WORDS 64                 // words 0 ok, 1 corners found, 2 ok2; 8-byte totals at words 4 cracks, 6 rings << 32 | cracks, 8 corners

static_assert(CT_RING == 12, "a ring record: ten words and one int64");

namespace {

typedef unsigned long long u64;

struct Quad { bool nw, ne, sw, se; };

__device__ __forceinline__ int lab_at(const int32_t* __restrict__ img, int H, int W, int r, int c) {
    return ((unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W) ? img[(long)r * W + c] : 0;      // l > 0 never equals it
}
__device__ __forceinline__ Quad quad_at(const int32_t* __restrict__ img, int H, int W, int vx, int vy, int l) {
    Quad q;
    q.nw = lab_at(img, H, W, vy - 1, vx - 1) == l;
    q.ne = lab_at(img, H, W, vy - 1, vx) == l;
    q.sw = lab_at(img, H, W, vy, vx - 1) == l;
    q.se = lab_at(img, H, W, vy, vx) == l;
    return q;
}
__device__ __forceinline__ bool leaves(const Quad q, int d) {
    return d == 0 ? (q.sw && !q.nw) : d == 1 ? (q.se && !q.sw) : d == 2 ? (q.ne && !q.se) : (q.nw && !q.ne);
}
__device__ __forceinline__ bool arrives(const Quad q, int d) {
    return d == 0 ? (q.se && !q.ne) : d == 1 ? (q.ne && !q.nw) : d == 2 ? (q.nw && !q.sw) : (q.sw && !q.se);
}
__device__ __forceinline__ void crack_ends(int r, int c, int d, int& x0, int& y0, int& x1, int& y1) {
    x0 = c + (d == 0 || d == 3);
    y0 = r + (d >= 2);
    x1 = c + (d >= 2);
    y1 = r + (d == 1 || d == 2);
}

// grid (nblk, B).  maskb [B][HW]: bits 0..3 the cracks N W S E, bits 4..7 their corner flags
__global__ __launch_bounds__(CT_SCAN) void ct_mask_kernel(const int32_t* __restrict__ labels, uint8_t* __restrict__ maskb,
                                                          u64* __restrict__ bsum, int32_t* __restrict__ counts,
                                                          int32_t* __restrict__ corners_total, int H, int W, int nblk) {
    __shared__ int sh[2][CT_SCAN / 64];
    const int b = blockIdx.y, blk = blockIdx.x, tid = threadIdx.x;
    const int HW = H * W;
    const int p = blk * CT_SCAN + tid;
    const int32_t* img = labels + (long)b * HW;
    int nc = 0, nk = 0;
    if (p < HW) {
        const int r = p / W, c = p - r * W;
        const int l = img[p];
        unsigned m = 0;
        if (l > 0) {
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const int nr = r + (d == 2) - (d == 0), ncol = c + (d == 3) - (d == 1);
                if (lab_at(img, H, W, nr, ncol) == l) continue;
                int x0, y0, x1, y1;
                crack_ends(r, c, d, x0, y0, x1, y1);
                const Quad q = quad_at(img, H, W, x0, y0, l);
                const bool corner = !(arrives(q, d) && !leaves(q, (d + 3) & 3));
                m |= (1u << d) | ((unsigned)corner << (4 + d));
            }
        }
        maskb[(long)b * HW + p] = (uint8_t)m;
        nc = __popc(m & 15u);
        nk = __popc(m >> 4);
    }
    for (int off = 32; off > 0; off >>= 1) {
        nc += __shfl_xor(nc, off);
        nk += __shfl_xor(nk, off);
    }
    if ((tid & 63) == 0) { sh[0][tid >> 6] = nc; sh[1][tid >> 6] = nk; }
    __syncthreads();
    if (tid == 0) {
        int a = 0, k = 0;
        for (int i = 0; i < CT_SCAN / 64; ++i) { a += sh[0][i]; k += sh[1][i]; }
        bsum[(long)b * nblk + blk] = (u64)a;
        if (a) atomicAdd(counts + 2 * b, a);
        if (k) atomicAdd(counts + 2 * b + 1, k);
        if (k && corners_total) atomicAdd(corners_total, k);
    }
}

// the 64-bit scan in three kernels (scan.hpp); gate: a header word, every launch behind a check is a no-op unless the check passed (NULL: none)
__global__ __launch_bounds__(CT_SCAN) void sc_block_sums(const int32_t* __restrict__ gate, const u64* __restrict__ vals,
                                                               u64* __restrict__ bsum, int n) {
    if (gate && *gate == 0) return;
    const u64 tot = scan::scan_block_total<u64, CT_SCAN>([vals](long i) { return vals[i]; }, n);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(CT_SCAN) void sc_small(const int32_t* __restrict__ gate, u64* __restrict__ v, int n,
                                                          u64* __restrict__ total_out) {
    if (gate && *gate == 0) return;
    u64 run;
    scan::scan_small<u64, CT_SCAN>(v, n, &run);
    if (threadIdx.x == 0) *total_out = run;
}
__global__ __launch_bounds__(CT_SCAN) void sc_apply(const int32_t* __restrict__ gate, u64* __restrict__ vals,
                                                          const u64* __restrict__ bsum, int n) {
    if (gate && *gate == 0) return;
    scan::scan_apply<u64, CT_SCAN>([vals](long i) { return vals[i]; }, [vals](long i, u64 x) { vals[i] = x; }, bsum[blockIdx.x], n);
}

// hdr[0] = 1 when the map holds exactly the cracks and corners the caller sized its buffers for
__global__ void ct_check_kernel(int32_t* __restrict__ hdr, int32_t* __restrict__ status, int n_cracks, int n_corners) {
    const u64 cracks = *(const u64*)(hdr + 4);
    if (cracks == (u64)n_cracks && hdr[1] == n_corners) hdr[0] = 1;
    else atomicOr(status, 1);
}
__global__ void ct_check2_kernel(int32_t* __restrict__ hdr, int32_t* __restrict__ status, int ring_cap) {
    if (hdr[0] == 0) return;
    const u64 rings = *(const u64*)(hdr + 6) >> 32;
    if (rings <= (u64)ring_cap) hdr[2] = 1;
    else atomicOr(status, 1);
}

// grid (nblk, B): pfx [B][HW], the compact index of the pixel's first crack: the apply pass of the scan whose block sums
// ct_mask_kernel made
__global__ __launch_bounds__(CT_SCAN) void ct_pfx_kernel(const uint8_t* __restrict__ maskb, const u64* __restrict__ bsum,
                                                         int32_t* __restrict__ pfx, int HW, int nblk) {
    const uint8_t* m = maskb + (long)blockIdx.y * HW;
    int32_t* out = pfx + (long)blockIdx.y * HW;
    scan::scan_apply<int, CT_SCAN>([m](long p) { return __popc(m[p] & 15u); }, [out](long p, int x) { out[p] = x; },
                                   (int)bsum[(long)blockIdx.y * nblk + blockIdx.x], HW);
}

// grid (ceil(HW / CT_BLOCK), B)
__global__ __launch_bounds__(CT_BLOCK) void ct_link_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ labels,
                                                           const uint8_t* __restrict__ maskb, const int32_t* __restrict__ pfx,
                                                           int4* __restrict__ elem, int32_t* __restrict__ slot, int H, int W, int n) {
    if (hdr[0] == 0) return;
    const int b = blockIdx.y;
    const int HW = H * W;
    const int p = blockIdx.x * CT_BLOCK + threadIdx.x;
    if (p >= HW) return;
    const long base = (long)b * HW;
    const unsigned m = maskb[base + p] & 15u;
    if (!m) return;
    const int32_t* img = labels + base;
    const int l = img[p];
    const int r = p / W, c = p - r * W;
    int e = pfx[base + p];
    for (int d = 0; d < 4; ++d) {
        if (!((m >> d) & 1u)) continue;
        int x0, y0, x1, y1;
        crack_ends(r, c, d, x0, y0, x1, y1);
        const Quad q = quad_at(img, H, W, x1, y1, l);
        const int rt = (d + 3) & 3;
        const int t = leaves(q, rt) ? rt : leaves(q, d) ? d : ((d + 1) & 3);
        const int sr = y1 - (t >= 2), sc = x1 - (t == 0 || t == 3);         // west SW, south SE, east NE, north NW
        int nx = e;
        if ((unsigned)sr < (unsigned)H && (unsigned)sc < (unsigned)W) {
            const long sp = base + (long)sr * W + sc;
            nx = pfx[sp] + __popc(maskb[sp] & ((1u << t) - 1u));
        }
        if ((unsigned)nx >= (unsigned)n) nx = e;                             // (cannot happen on a checked map: keeps every index inside)
        if ((unsigned)e < (unsigned)n) {
            elem[e] = make_int4(nx, nx, 1, 0);
            slot[e] = (int)(4 * (base + p)) + d;
        }
        ++e;
    }
}

__global__ __launch_bounds__(CT_BLOCK) void ct_double_kernel(const int32_t* __restrict__ hdr, const int4* __restrict__ src,
                                                             int4* __restrict__ dst, int n, int step) {
    if (hdr[0] == 0) return;
    const long e = (long)blockIdx.x * CT_BLOCK + threadIdx.x;
    if (e >= n) return;
    const int4 a = src[e];
    const int4 b = src[a.x];
    int4 o = make_int4(b.x, a.y, a.z, 0);
    if (b.y < a.y) { o.y = b.y; o.z = step + b.z; }
    dst[e] = o;
}

__global__ __launch_bounds__(CT_BLOCK) void ct_ring_kernel(const int32_t* __restrict__ hdr, const int4* __restrict__ fin,
                                                           int32_t* __restrict__ pos, u64* __restrict__ rk, int n) {
    if (hdr[0] == 0) return;
    const long e = (long)blockIdx.x * CT_BLOCK + threadIdx.x;
    if (e >= n) return;
    const int4 a = fin[e];
    const bool leader = a.y == (int)e;
    const int len = leader ? a.z : fin[a.y].z;
    pos[e] = leader ? 0 : len - a.z;
    rk[e] = leader ? ((1ull << 32) | (u64)(unsigned)len) : 0ull;
}

__device__ __forceinline__ int corner_of(const uint8_t* __restrict__ maskb, int s) { return (maskb[s >> 2] >> (4 + (s & 3))) & 1; }

__global__ __launch_bounds__(CT_BLOCK) void ct_place_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ labels,
                                                            const uint8_t* __restrict__ maskb, const int4* __restrict__ fin,
                                                            const int32_t* __restrict__ slot, const int32_t* __restrict__ pos,
                                                            const u64* __restrict__ rk, int32_t* __restrict__ ord,
                                                            u64* __restrict__ cf, int32_t* __restrict__ rings,
                                                            int32_t* __restrict__ n_rings, int HW, int n, int ring_cap) {
    if (hdr[2] == 0) return;
    const long e = (long)blockIdx.x * CT_BLOCK + threadIdx.x;
    if (e >= n) return;
    const int4 a = fin[e];
    const u64 s = rk[a.y];
    const unsigned q = (unsigned)s + (unsigned)pos[e];
    const int sl = slot[e];
    if (q < (unsigned)n) {
        ord[q] = (int)e;
        cf[q] = (u64)corner_of(maskb, sl);
    }
    const unsigned ring = (unsigned)(s >> 32);
    if (a.y == (int)e && ring < (unsigned)ring_cap) {
        const int P = sl >> 2;
        const int b = P / HW;
        int32_t* rec = rings + (long)ring * CT_RING;
        rec[0] = b;
        rec[1] = labels[P];
        rec[2] = 0;
        rec[3] = 0;
        rec[4] = a.z;
        rec[5] = 0x7fffffff;
        rec[6] = 0x7fffffff;
        rec[7] = (int)0x80000000;
        rec[8] = (int)0x80000000;
        rec[9] = sl - 4 * b * HW;
        rec[10] = 0;
        rec[11] = 0;
        atomicAdd(n_rings + b, 1);
    }
}

// one thread per place of the ring order
__global__ __launch_bounds__(CT_BLOCK) void ct_emit_kernel(const int32_t* __restrict__ hdr, const int4* __restrict__ fin,
                                                           const int32_t* __restrict__ slot, const u64* __restrict__ rk,
                                                           const int32_t* __restrict__ ord, const u64* __restrict__ cf,
                                                           const uint8_t* __restrict__ maskb, int32_t* __restrict__ rings,
                                                           int32_t* __restrict__ verts, int HW, int W, int n, int n_corners,
                                                           int ring_cap) {
    if (hdr[2] == 0) return;
    const long q = (long)blockIdx.x * CT_BLOCK + threadIdx.x;
    const bool valid = q < n;
    int ring = -1, x0 = 0x7fffffff, y0 = 0x7fffffff, x1 = (int)0x80000000, y1 = (int)0x80000000;
    int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = (int)0x80000000, by1 = (int)0x80000000;
    long long area = 0;
    if (valid) {
        const int e = ord[q];
        const int4 a = fin[e];
        const u64 s = rk[a.y];
        const int sl = slot[e];
        const int P = sl >> 2, d = sl & 3;
        const int p = P % HW;
        const int r = p / W, c = p - r * W;
        crack_ends(r, c, d, x0, y0, x1, y1);
        area = -((long long)x0 * y1 - (long long)x1 * y0);
        bx0 = bx1 = x0;
        by0 = by1 = y0;
        ring = (int)(unsigned)(s >> 32);
        if ((unsigned)ring >= (unsigned)ring_cap) ring = -1;
        const u64 v = cf[q];
        if (corner_of(maskb, sl) && v < (u64)n_corners) {
            verts[2 * v] = x0;
            verts[2 * v + 1] = y0;
        }
        if (a.y == e && ring >= 0) {                                     // the leader: the ring's place 0
            const long qe = q + a.z;
            const u64 vend = qe < n ? cf[qe] : *(const u64*)(hdr + 8);
            int32_t* rec = rings + (long)ring * CT_RING;
            rec[2] = (int)v;
            rec[3] = (int)(vend - v);
        }
    }
    const int first = __shfl(ring, 0);
    if (__all(!valid || ring == first)) {
        for (int off = 32; off > 0; off >>= 1) {
            bx0 = min(bx0, __shfl_xor(bx0, off));
            by0 = min(by0, __shfl_xor(by0, off));
            bx1 = max(bx1, __shfl_xor(bx1, off));
            by1 = max(by1, __shfl_xor(by1, off));
            area += __shfl_xor(area, off);
        }
        if ((threadIdx.x & 63) != 0) ring = -1;
    }
    if (ring >= 0) {
        int32_t* rec = rings + (long)ring * CT_RING;
        atomicMin(rec + 5, bx0);
        atomicMin(rec + 6, by0);
        atomicMax(rec + 7, bx1);
        atomicMax(rec + 8, by1);
        atomicAdd((u64*)(rec + 10), (u64)area);
    }
}

inline bool bad_shape(int B, int H, int W) {
    return B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long)H * W >= (1l << 29) || 4l * B * ((long)H * W) >= (1l << 31);
}
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

struct Layout { size_t hdr, counts, maskb, pfx, bsum_p, elem_a, elem_b, slot, pos, rk, cf, ord, bsum_c, total; };
inline Layout layout(int B, int H, int W, long n) {
    const size_t N = (size_t)B * H * W;
    const size_t nblk_p = (size_t)B * ceil_div(H * W, CT_SCAN), nblk_c = (size_t)((n + CT_SCAN - 1) / CT_SCAN);
    Layout L;
    size_t o = 0;
    L.hdr = o; o += align_up(CT_HDR_WORDS * 4, 256);
    L.counts = o; o += align_up((size_t)B * 2 * 4, 256);
    L.maskb = o; o += align_up(N, 256);
    L.pfx = o; o += align_up(N * 4, 256);
    L.bsum_p = o; o += align_up(nblk_p * 8, 256);
    L.elem_a = o; o += align_up((size_t)n * 16, 256);
    L.elem_b = o; o += align_up((size_t)n * 16, 256);
    L.slot = o; o += align_up((size_t)n * 4, 256);
    L.pos = o; o += align_up((size_t)n * 4, 256);
    L.rk = o; o += align_up((size_t)n * 8, 256);
    L.cf = o; o += align_up((size_t)n * 8, 256);
    L.ord = o; o += align_up((size_t)n * 4, 256);
    L.bsum_c = o; o += align_up(nblk_c * 8, 256);
    L.total = o;
    return L;
}

}  // namespace

extern "C" size_t wesup_contour_trace_workspace_bytes(int B, int H, int W, int n_cracks) {
    if (bad_shape(B, H, W) || n_cracks < 0 || (long)n_cracks > 4l * B * H * W) return 0;
    return layout(B, H, W, n_cracks).total;
}

extern "C" size_t wesup_contour_workspace_bytes(int B, int H, int W) {
    if (bad_shape(B, H, W)) return 0;
    return layout(B, H, W, 4l * B * H * W).total;
}

extern "C" int wesup_contour_count(const int32_t* labels, int32_t* counts, int B, int H, int W, void* ws, size_t ws_bytes,
                                   void* stream) {
    if (!labels || !counts || !ws || bad_shape(B, H, W) || ((uintptr_t)ws & 15) || ((uintptr_t)labels & 3) || ((uintptr_t)counts & 3))
        return WESUP_ERR_INVALID;
    const Layout L = layout(B, H, W, 0);
    if (ws_bytes < L.total) return WESUP_ERR_INVALID;
    const size_t nl = (size_t)B * H * W * 4, nc = (size_t)B * 2 * 4;
    if (overlap(labels, nl, counts, nc) || overlap(labels, nl, ws, L.total) || overlap(counts, nc, ws, L.total))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    const int nblk = ceil_div(H * W, CT_SCAN);
    if (wesup_fill_words_(counts, 0u, (size_t)B * 2, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    WESUP_LAUNCH(ct_mask_kernel, dim3(nblk, B), dim3(CT_SCAN), 0, st, labels, (uint8_t*)(w + L.maskb), (u64*)(w + L.bsum_p), counts,
                 (int32_t*)nullptr, H, W, nblk);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_contour_trace(const int32_t* labels, int32_t* rings, int32_t* verts, int32_t* n_rings, int32_t* status, int B,
                                   int H, int W, int n_cracks, int n_corners, int ring_cap, void* ws, size_t ws_bytes,
                                   void* stream) {
    if (!labels || !rings || !verts || !n_rings || !status || !ws || bad_shape(B, H, W)) return WESUP_ERR_INVALID;
    if (n_cracks < 0 || n_corners < 0 || ring_cap < 0 || (long)n_cracks > 4l * B * H * W) return WESUP_ERR_INVALID;
    if (((uintptr_t)ws & 15) || ((uintptr_t)labels & 3) || ((uintptr_t)rings & 7) || ((uintptr_t)verts & 3) ||
        ((uintptr_t)n_rings & 3) || ((uintptr_t)status & 3))
        return WESUP_ERR_INVALID;
    const Layout L = layout(B, H, W, n_cracks);
    if (ws_bytes < L.total) return WESUP_ERR_INVALID;
    // an empty capacity still names a word: the overlap test takes every operand as at least one element long
    const size_t nl = (size_t)B * H * W * 4, nr = (size_t)(ring_cap > 0 ? ring_cap : 1) * CT_RING * 4,
                 nv = (size_t)(n_corners > 0 ? n_corners : 1) * 8, nn = (size_t)B * 4;
    const void* ops[6] = {labels, rings, verts, n_rings, status, ws};
    const size_t len[6] = {nl, nr, nv, nn, 4, L.total};
    for (int i = 0; i < 6; ++i)
        for (int j = i + 1; j < 6; ++j)
            if (overlap(ops[i], len[i], ops[j], len[j])) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    int32_t* hdr = (int32_t*)(w + L.hdr);
    int32_t* cnt = (int32_t*)(w + L.counts);
    uint8_t* maskb = (uint8_t*)(w + L.maskb);
    int32_t* pfx = (int32_t*)(w + L.pfx);
    u64* bsum_p = (u64*)(w + L.bsum_p);
    int4* ea = (int4*)(w + L.elem_a);
    int4* eb = (int4*)(w + L.elem_b);
    int32_t* slot = (int32_t*)(w + L.slot);
    int32_t* pos = (int32_t*)(w + L.pos);
    u64* rk = (u64*)(w + L.rk);
    u64* cf = (u64*)(w + L.cf);
    int32_t* ord = (int32_t*)(w + L.ord);
    u64* bsum_c = (u64*)(w + L.bsum_c);
    const int HW = H * W, n = n_cracks;
    const int nblk = ceil_div(HW, CT_SCAN);
    // the header and the per-image counts lie next to each other: one fill
    if (wesup_fill_words_(w + L.hdr, 0u, (L.maskb - L.hdr) / 4, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (wesup_fill_words_(n_rings, 0u, (size_t)B, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    WESUP_LAUNCH(ct_mask_kernel, dim3(nblk, B), dim3(CT_SCAN), 0, st, labels, maskb, bsum_p, cnt, hdr + 1, H, W, nblk);
    WESUP_LAUNCH(sc_small, dim3(1), dim3(CT_SCAN), 0, st, (const int32_t*)nullptr, bsum_p, B * nblk, (u64*)(hdr + 4));
    WESUP_LAUNCH(ct_check_kernel, dim3(1), dim3(1), 0, st, hdr, status, n_cracks, n_corners);
    if (n > 0) {
        const unsigned gc = (unsigned)((n + CT_BLOCK - 1) / CT_BLOCK), gs = (unsigned)((n + CT_SCAN - 1) / CT_SCAN);
        WESUP_LAUNCH(ct_pfx_kernel, dim3(nblk, B), dim3(CT_SCAN), 0, st, (const uint8_t*)maskb, (const u64*)bsum_p, pfx, HW, nblk);
        WESUP_LAUNCH(ct_link_kernel, dim3(ceil_div(HW, CT_BLOCK), B), dim3(CT_BLOCK), 0, st, (const int32_t*)hdr, labels,
                     (const uint8_t*)maskb, (const int32_t*)pfx, ea, slot, H, W, n);
        int4 *src = ea, *dst = eb;
        for (int k = 0; (1l << k) < (long)n; ++k) {
            WESUP_LAUNCH(ct_double_kernel, dim3(gc), dim3(CT_BLOCK), 0, st, (const int32_t*)hdr, (const int4*)src, dst, n, 1 << k);
            int4* t = src; src = dst; dst = t;
        }
        const int4* fin = src;
        WESUP_LAUNCH(ct_ring_kernel, dim3(gc), dim3(CT_BLOCK), 0, st, (const int32_t*)hdr, fin, pos, rk, n);
        WESUP_LAUNCH(sc_block_sums, dim3(gs), dim3(CT_SCAN), 0, st, (const int32_t*)hdr, (const u64*)rk, bsum_c, n);
        WESUP_LAUNCH(sc_small, dim3(1), dim3(CT_SCAN), 0, st, (const int32_t*)hdr, bsum_c, (int)gs, (u64*)(hdr + 6));
        WESUP_LAUNCH(sc_apply, dim3(gs), dim3(CT_SCAN), 0, st, (const int32_t*)hdr, rk, (const u64*)bsum_c, n);
        WESUP_LAUNCH(ct_check2_kernel, dim3(1), dim3(1), 0, st, hdr, status, ring_cap);
        WESUP_LAUNCH(ct_place_kernel, dim3(gc), dim3(CT_BLOCK), 0, st, (const int32_t*)hdr, labels, (const uint8_t*)maskb, fin,
                     (const int32_t*)slot, (const int32_t*)pos, (const u64*)rk, ord, cf, rings, n_rings, HW, n, ring_cap);
        WESUP_LAUNCH(sc_block_sums, dim3(gs), dim3(CT_SCAN), 0, st, (const int32_t*)(hdr + 2), (const u64*)cf, bsum_c, n);
        WESUP_LAUNCH(sc_small, dim3(1), dim3(CT_SCAN), 0, st, (const int32_t*)(hdr + 2), bsum_c, (int)gs, (u64*)(hdr + 8));
        WESUP_LAUNCH(sc_apply, dim3(gs), dim3(CT_SCAN), 0, st, (const int32_t*)(hdr + 2), cf, (const u64*)bsum_c, n);
        WESUP_LAUNCH(ct_emit_kernel, dim3(gc), dim3(CT_BLOCK), 0, st, (const int32_t*)hdr, fin, (const int32_t*)slot,
                     (const u64*)rk, (const int32_t*)ord, (const u64*)cf, (const uint8_t*)maskb, rings, verts, HW, W, n, n_corners,
                     ring_cap);
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

// ---------------------------------------------------------------------------------------------- simplification
#define SP_BLOCK 1024
#define SP_LDS_N 896                    // vertices of a ring whose state lives in LDS: 64 bytes each, 56 KiB of the 64 KiB a block may declare
#define SP_MAX_BLOCKS 1024
#define SP_HDR_WORDS 64                 // words 0 ok; the 8-byte total of kept vertices at word 2
#define SP_SPAN 32768
#define SP_NONE 0xffffffffffffffffull

namespace {

// one block, striding over the records: first vertices consecutive from 0 to V, every ring of at least one vertex
__global__ __launch_bounds__(SP_BLOCK) void sp_validate_kernel(const int32_t* __restrict__ rings, int R, int V,
                                                               int32_t* __restrict__ hdr, int32_t* __restrict__ counts) {
    __shared__ int bad;
    if (threadIdx.x == 0) bad = 0;
    __syncthreads();
    int b = 0;
    for (int r = threadIdx.x; r < R; r += SP_BLOCK) {
        const long fv = rings[(long)r * CT_RING + 2], n = rings[(long)r * CT_RING + 3];
        const long prev = r ? (long)rings[(long)(r - 1) * CT_RING + 2] + rings[(long)(r - 1) * CT_RING + 3] : 0l;
        if (n < 1 || fv < 0 || fv + n > V || fv != prev) b = 1;
        if (r == R - 1 && fv + n != V) b = 1;
    }
    if (b) atomicOr(&bad, 1);
    __syncthreads();
    if (threadIdx.x == 0) {
        hdr[0] = bad ? 0 : 1;
        hdr[2] = 0;
        hdr[3] = 0;
        if (bad) counts[3] = 1;
    }
}

// a ring's state, in LDS or in the workspace: the code below is the same
struct SpState {
    const int32_t* px;                  // x at px[stride * k], y at py[stride * k]
    const int32_t* py;
    int stride;
    int32_t *lo, *hi;                   // per vertex: the ends of its piece, positions 0 .. n (n is vertex 0 again)
    u64 *best, *tie;                    // per piece, at its lo: the largest D; (|2k - lo - hi| << 32) | k of the winner
    int32_t* list;                      // the live vertices
    long par;                           // best, tie and list of the odd levels lie this many elements behind those of the even ones
    u64* dl;                            // D of the live vertex at this place of the list
};

struct SpShared {
    u64 akey, area_all, area_k;
    int bb_all[4], bb_k[4];
    int nkept, nact[2];
};

__device__ __forceinline__ u64 sp_cross(int xa, int ya, int xb, int yb) {               // one term of area2: -(xa yb - xb ya)
    return (u64)(-((long long)xa * yb - (long long)xb * ya));
}

__device__ __forceinline__ void sp_ring(const SpState S, SpShared& sh, int n, u64 tol2, u64* __restrict__ keep) {
    const int tid = threadIdx.x;
    const int a1 = (int)(0xffffffffu - (unsigned)sh.akey);                              // (read after the caller's barrier)
    // pieces 0 .. a1 and a1 .. n; every other vertex is live
    for (int k = tid; k < n; k += SP_BLOCK) {
        const bool anchor = k == 0 || k == a1;
        keep[k] = anchor ? 1ull : 0ull;
        if (anchor) {
            S.best[k] = 0;
            S.tie[k] = SP_NONE;
        } else {
            S.lo[k] = k < a1 ? 0 : a1;
            S.hi[k] = k < a1 ? a1 : n;
            S.list[k - 1 - (k > a1 && a1 > 0)] = k;
        }
    }
    if (tid == 0) {
        sh.nact[0] = n - 1 - (a1 > 0);
        sh.nact[1] = 0;
        sh.nkept = 1 + (a1 > 0);
        sh.area_k = 0;
        const int x0 = S.px[0], y0 = S.py[0], x1 = S.px[(long)S.stride * a1], y1 = S.py[(long)S.stride * a1];
        sh.bb_k[0] = min(x0, x1); sh.bb_k[1] = min(y0, y1); sh.bb_k[2] = max(x0, x1); sh.bb_k[3] = max(y0, y1);
    }
    __syncthreads();
    int p = 0;
    // at most n levels: a level with live vertices keeps at least one more vertex or retires them all, and ends the loop then
    for (int level = 0; level < n; ++level, p ^= 1) {
        const int cnt = sh.nact[p];
        if (cnt == 0) break;
        const int32_t* lst = S.list + p * S.par;
        u64 *best = S.best + p * S.par, *tie = S.tie + p * S.par;
        u64 *best_n = S.best + (p ^ 1) * S.par, *tie_n = S.tie + (p ^ 1) * S.par;
        int32_t* lst_n = S.list + (p ^ 1) * S.par;
        for (int i0 = 0; i0 < cnt; i0 += SP_BLOCK) {
            const int i = i0 + tid;
            const bool valid = i < cnt;
            int l = -1;
            u64 D = 0;
            if (valid) {
                const int k = lst[i], h = S.hi[k];
                l = S.lo[k];
                const int hv = h == n ? 0 : h;
                const long long ax = S.px[(long)S.stride * l], ay = S.py[(long)S.stride * l];
                const long long bx = S.px[(long)S.stride * hv], by = S.py[(long)S.stride * hv];
                const long long qx = S.px[(long)S.stride * k], qy = S.py[(long)S.stride * k];
                const long long ux = bx - ax, uy = by - ay, vx = qx - ax, vy = qy - ay;
                const u64 L = (u64)(ux * ux + uy * uy), da = (u64)(vx * vx + vy * vy);
                if (L == 0) D = da;
                else {
                    const long long t = vx * ux + vy * uy;
                    if (t <= 0) D = da * L;
                    else if ((u64)t >= L) D = (u64)((qx - bx) * (qx - bx) + (qy - by) * (qy - by)) * L;
                    else {
                        const long long c = vx * uy - vy * ux;
                        D = (u64)(c * c);
                    }
                }
                S.dl[i] = D;
            }
            // a wave inside one piece folds first: the early levels of a long ring would otherwise meet on one word
            const int first = __shfl(l, 0);
            if (__all(!valid || l == first)) {
                for (int off = 32; off > 0; off >>= 1) {
                    const u64 o = __shfl_xor(D, off);
                    D = o > D ? o : D;
                }
                if ((tid & 63) == 0 && valid) atomicMax(&best[l], D);
            } else if (valid) atomicMax(&best[l], D);
        }
        __syncthreads();
        for (int i = tid; i < cnt; i += SP_BLOCK) {
            const int k = lst[i], l = S.lo[k], h = S.hi[k];
            if (S.dl[i] == best[l]) {
                const int a = 2 * k - l - h;
                atomicMin(&tie[l], ((u64)(unsigned)(a < 0 ? -a : a) << 32) | (u64)(unsigned)k);
            }
        }
        if (tid == 0) sh.nact[p ^ 1] = 0;
        __syncthreads();
        for (int i0 = 0; i0 < cnt; i0 += SP_BLOCK) {
            const int i = i0 + tid;
            bool live = false;
            int k = 0;
            if (i < cnt) {
                k = lst[i];
                const int l = S.lo[k], h = S.hi[k];
                const int hv = h == n ? 0 : h;
                const int ax = S.px[(long)S.stride * l], ay = S.py[(long)S.stride * l];
                const int bx = S.px[(long)S.stride * hv], by = S.py[(long)S.stride * hv];
                const long long ux = (long long)bx - ax, uy = (long long)by - ay;
                const u64 L = (u64)(ux * ux + uy * uy);
                if (best[l] > ((tol2 * (L ? L : 1ull)) >> 8)) {
                    const int m = (int)(unsigned)tie[l];
                    if (k == m) {
                        const int mx = S.px[(long)S.stride * k], my = S.py[(long)S.stride * k];
                        keep[k] = 1ull;
                        best_n[l] = 0; tie_n[l] = SP_NONE;
                        best_n[k] = 0; tie_n[k] = SP_NONE;
                        atomicAdd(&sh.area_k, sp_cross(ax, ay, mx, my) + sp_cross(mx, my, bx, by) - sp_cross(ax, ay, bx, by));
                        atomicAdd(&sh.nkept, 1);
                        atomicMin(&sh.bb_k[0], mx); atomicMin(&sh.bb_k[1], my);
                        atomicMax(&sh.bb_k[2], mx); atomicMax(&sh.bb_k[3], my);
                    } else {
                        if (k < m) S.hi[k] = m; else S.lo[k] = m;
                        live = true;
                    }
                }
            }
            // the survivors go to the other list: one atomic per wave, the order inside the list does not matter
            const u64 mask = __ballot(live);
            if (mask) {
                const int lane = tid & 63, leader = __ffsll((long long)mask) - 1;
                int base = 0;
                if (lane == leader) base = atomicAdd(&sh.nact[p ^ 1], __popcll(mask));
                base = __shfl(base, leader);
                if (live) lst_n[base + __popcll(mask & ((1ull << lane) - 1ull))] = k;
            }
        }
        __syncthreads();
    }
    __syncthreads();
}

__global__ __launch_bounds__(SP_BLOCK) void sp_simplify_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ rings,
                                                               const int32_t* __restrict__ verts, int R, u64 tol2,
                                                               int32_t* __restrict__ rings_out, int32_t* __restrict__ flags,
                                                               int32_t* __restrict__ counts, u64* __restrict__ keep,
                                                               int32_t* __restrict__ g_lo, int32_t* __restrict__ g_hi,
                                                               u64* __restrict__ g_best, u64* __restrict__ g_tie,
                                                               int32_t* __restrict__ g_list, u64* __restrict__ g_dl, long V) {
    __shared__ SpShared sh;
    __shared__ u64 s_best[2][SP_LDS_N], s_tie[2][SP_LDS_N], s_dl[SP_LDS_N];
    __shared__ int32_t s_x[SP_LDS_N], s_y[SP_LDS_N], s_lo[SP_LDS_N], s_hi[SP_LDS_N], s_list[2][SP_LDS_N];
    if (hdr[0] == 0) return;
    const int tid = threadIdx.x;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        const int32_t* rec = rings + (long)r * CT_RING;
        const long fv = rec[2];
        const int n = rec[3];
        const long long a2_in = (long long)(((u64)(unsigned)rec[11] << 32) | (u64)(unsigned)rec[10]);
        const bool oversize = n > 4 && ((long)rec[7] - rec[5] >= SP_SPAN || (long)rec[8] - rec[6] >= SP_SPAN);
        const bool work = n > 4 && !oversize;
        const bool in_lds = work && n <= SP_LDS_N;
        const int32_t* P = verts + 2 * fv;
        if (tid == 0) {
            sh.akey = 0;
            sh.area_all = 0;
            sh.bb_all[0] = sh.bb_all[1] = 0x7fffffff;
            sh.bb_all[2] = sh.bb_all[3] = (int)0x80000000;
        }
        __syncthreads();
        // every vertex once: the ring as traced (bounding box, area2), the far anchor
        {
            const int x0 = P[0], y0 = P[1];
            u64 key = 0, area = 0;
            int bx0 = 0x7fffffff, by0 = 0x7fffffff, bx1 = (int)0x80000000, by1 = (int)0x80000000;
            for (int k = tid; k < n; k += SP_BLOCK) {
                const int x = P[2 * k], y = P[2 * k + 1];
                const int kn = k + 1 == n ? 0 : k + 1;
                area += sp_cross(x, y, P[2 * kn], P[2 * kn + 1]);
                bx0 = min(bx0, x); by0 = min(by0, y); bx1 = max(bx1, x); by1 = max(by1, y);
                if (work) {
                    const long long dx = (long long)x - x0, dy = (long long)y - y0;
                    const u64 kk = ((u64)(dx * dx + dy * dy) << 32) | (u64)(0xffffffffu - (unsigned)k);      // < 2^31: the spans are below 2^15
                    key = kk > key ? kk : key;
                    if (in_lds) { s_x[k] = x; s_y[k] = y; }
                } else keep[fv + k] = 1ull;
            }
            for (int off = 32; off > 0; off >>= 1) {
                const u64 ok = __shfl_xor(key, off);
                key = ok > key ? ok : key;
                area += __shfl_xor(area, off);
                bx0 = min(bx0, __shfl_xor(bx0, off)); by0 = min(by0, __shfl_xor(by0, off));
                bx1 = max(bx1, __shfl_xor(bx1, off)); by1 = max(by1, __shfl_xor(by1, off));
            }
            if ((tid & 63) == 0 && (long)(tid & ~63) < n) {
                atomicMax(&sh.akey, key);
                atomicAdd(&sh.area_all, area);
                atomicMin(&sh.bb_all[0], bx0); atomicMin(&sh.bb_all[1], by0);
                atomicMax(&sh.bb_all[2], bx1); atomicMax(&sh.bb_all[3], by1);
            }
        }
        __syncthreads();
        bool as_traced = true;
        if (work) {
            SpState S;
            if (in_lds) {
                S.px = s_x; S.py = s_y; S.stride = 1;
                S.lo = s_lo; S.hi = s_hi;
                S.best = s_best[0]; S.tie = s_tie[0]; S.list = s_list[0]; S.par = SP_LDS_N;
                S.dl = s_dl;
                sp_ring(S, sh, n, tol2, keep + fv);
            } else {
                S.px = P; S.py = P + 1; S.stride = 2;
                S.lo = g_lo + fv; S.hi = g_hi + fv;
                S.best = g_best + fv; S.tie = g_tie + fv; S.list = g_list + fv; S.par = V;
                S.dl = g_dl + fv;
                sp_ring(S, sh, n, tol2, keep + fv);
            }
            const long long ak = (long long)sh.area_k;
            as_traced = sh.nkept < 3 || ak == 0 || a2_in == 0 || (ak > 0) != (a2_in > 0);       // orientation is never lost
            if (as_traced)
                for (int k = tid; k < n; k += SP_BLOCK) keep[fv + k] = 1ull;
        }
        if (tid == 0) {
            const int flag = oversize ? 2 : (work && as_traced) ? 1 : 0;
            const u64 area = as_traced ? sh.area_all : sh.area_k;
            const int* bb = as_traced ? sh.bb_all : sh.bb_k;
            int32_t* out = rings_out + (long)r * CT_RING;
            out[0] = rec[0]; out[1] = rec[1];
            out[3] = as_traced ? n : sh.nkept;
            out[4] = rec[4];
            out[5] = bb[0]; out[6] = bb[1]; out[7] = bb[2]; out[8] = bb[3];
            out[9] = rec[9];
            out[10] = (int)(unsigned)area; out[11] = (int)(unsigned)(area >> 32);
            flags[r] = flag;
            if (flag) atomicAdd(counts + flag, 1);
        }
        __syncthreads();
    }
}

// grid over max(V, R): scan[k] is the number of kept vertices in front of k
__global__ __launch_bounds__(CT_BLOCK) void sp_emit_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ rings,
                                                           const int32_t* __restrict__ verts, const u64* __restrict__ scan,
                                                           int32_t* __restrict__ rings_out, int32_t* __restrict__ verts_out,
                                                           int32_t* __restrict__ counts, int R, int V) {
    if (hdr[0] == 0) return;
    const long k = (long)blockIdx.x * CT_BLOCK + threadIdx.x;
    const u64 total = *(const u64*)(hdr + 2);
    if (k < V) {
        const u64 s = scan[k], e = k + 1 < V ? scan[k + 1] : total;
        if (e != s && s < (u64)V) {
            verts_out[2 * s] = verts[2 * k];
            verts_out[2 * s + 1] = verts[2 * k + 1];
        }
    }
    if (k < R) rings_out[k * CT_RING + 2] = (int)scan[rings[k * CT_RING + 2]];
    if (k == 0) counts[0] = (int)total;
}

struct SpLayout { size_t hdr, keep, bsum, lo, hi, best, tie, list, dl, total; };
inline SpLayout sp_layout(long V) {
    const size_t v = (size_t)V;
    SpLayout L;
    size_t o = 0;
    L.hdr = o; o += align_up(SP_HDR_WORDS * 4, 256);
    L.keep = o; o += align_up(v * 8, 256);
    L.bsum = o; o += align_up(((v + CT_SCAN - 1) / CT_SCAN) * 8, 256);
    L.lo = o; o += align_up(v * 4, 256);
    L.hi = o; o += align_up(v * 4, 256);
    L.best = o; o += align_up(2 * v * 8, 256);
    L.tie = o; o += align_up(2 * v * 8, 256);
    L.list = o; o += align_up(2 * v * 4, 256);
    L.dl = o; o += align_up(v * 8, 256);
    L.total = o;
    return L;
}
inline bool sp_bad_sizes(int R, int V) { return R < 0 || V < 0 || V > (1 << 28) || R > V; }

}  // namespace

extern "C" size_t wesup_contour_simplify_workspace_bytes(int R, int V) {
    if (sp_bad_sizes(R, V)) return 0;
    return sp_layout(V).total;
}

extern "C" int wesup_contour_simplify(const int32_t* rings, int R, const int32_t* verts, int V, int tol_q4, int32_t* rings_out,
                                      int32_t* verts_out, int32_t* flags, int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
    if (!rings || !verts || !rings_out || !verts_out || !flags || !counts || !ws || sp_bad_sizes(R, V)) return WESUP_ERR_INVALID;
    if (tol_q4 < 0 || tol_q4 > WESUP_SIMPLIFY_TOL_MAX) return WESUP_ERR_INVALID;
    if (((uintptr_t)ws & 15) || ((uintptr_t)rings & 7) || ((uintptr_t)rings_out & 7) || ((uintptr_t)verts & 3) ||
        ((uintptr_t)verts_out & 3) || ((uintptr_t)flags & 3) || ((uintptr_t)counts & 3))
        return WESUP_ERR_INVALID;
    const SpLayout L = sp_layout(V);
    if (ws_bytes < L.total) return WESUP_ERR_INVALID;
    const size_t nr = (size_t)(R > 0 ? R : 1) * CT_RING * 4, nv = (size_t)(V > 0 ? V : 1) * 8, nf = (size_t)(R > 0 ? R : 1) * 4;
    const void* ops[7] = {rings, verts, rings_out, verts_out, flags, counts, ws};
    const size_t len[7] = {nr, nv, nr, nv, nf, WESUP_SIMPLIFY_COUNTS * 4, L.total};
    for (int i = 0; i < 7; ++i)
        for (int j = i + 1; j < 7; ++j)
            if (overlap(ops[i], len[i], ops[j], len[j])) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    int32_t* hdr = (int32_t*)(w + L.hdr);
    u64* keep = (u64*)(w + L.keep);
    u64* bsum = (u64*)(w + L.bsum);
    if (wesup_fill_words_(counts, 0u, (size_t)WESUP_SIMPLIFY_COUNTS, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    WESUP_LAUNCH(sp_validate_kernel, dim3(1), dim3(SP_BLOCK), 0, st, rings, R, V, hdr, counts);
    if (R > 0) {
        const unsigned gs = (unsigned)((V + CT_SCAN - 1) / CT_SCAN);
        const int big = V > R ? V : R;
        WESUP_LAUNCH(sp_simplify_kernel, dim3(R < SP_MAX_BLOCKS ? R : SP_MAX_BLOCKS), dim3(SP_BLOCK), 0, st, (const int32_t*)hdr,
                     rings, verts, R, (u64)tol_q4 * (u64)tol_q4, rings_out, flags, counts, keep, (int32_t*)(w + L.lo),
                     (int32_t*)(w + L.hi), (u64*)(w + L.best), (u64*)(w + L.tie), (int32_t*)(w + L.list), (u64*)(w + L.dl), (long)V);
        WESUP_LAUNCH(sc_block_sums, dim3(gs), dim3(CT_SCAN), 0, st, (const int32_t*)hdr, (const u64*)keep, bsum, V);
        WESUP_LAUNCH(sc_small, dim3(1), dim3(CT_SCAN), 0, st, (const int32_t*)hdr, bsum, (int)gs, (u64*)(hdr + 2));
        WESUP_LAUNCH(sc_apply, dim3(gs), dim3(CT_SCAN), 0, st, (const int32_t*)hdr, keep, (const u64*)bsum, V);
        WESUP_LAUNCH(sp_emit_kernel, dim3((unsigned)((big + CT_BLOCK - 1) / CT_BLOCK)), dim3(CT_BLOCK), 0, st, (const int32_t*)hdr,
                     rings, verts, (const u64*)keep, rings_out, verts_out, counts, R, V);
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
