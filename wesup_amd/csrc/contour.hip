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
//   sc_block_sums, sc_small, sc_apply    ring ids and the rings' first crack in ring order, one 64-bit scan
//   ct_check2_kernel   rings against ring_cap
//   ct_place_kernel    ring order: the crack of every place, the corner flag of every place; the leaders start their records
//   sc_block_sums, sc_small, sc_apply    vertex indices: the scan of the corner flags in ring order
//   ct_emit_kernel     one thread per place: vertices, bounding boxes, areas; a wave inside one ring folds first
#include "common.hpp"

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

// exclusive scan of CT_SCAN values, one per thread
template <typename T>
__device__ __forceinline__ T block_scan(T v, T* sh, T* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < CT_SCAN; off <<= 1) {
        const T t = (tid >= off) ? sh[tid - off] : (T)0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const T incl = sh[tid];
    *total = sh[CT_SCAN - 1];
    __syncthreads();
    return incl - v;
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

// the 64-bit scan in three kernels; gate: a header word, every launch behind a check is a no-op unless the check passed (NULL: none)
__global__ __launch_bounds__(CT_SCAN) void sc_block_sums(const int32_t* __restrict__ gate, const u64* __restrict__ vals,
                                                               u64* __restrict__ bsum, int n) {
    __shared__ u64 sh[CT_SCAN];
    if (gate && *gate == 0) return;
    const long i = (long)blockIdx.x * CT_SCAN + threadIdx.x;
    u64 tot;
    block_scan<u64>(i < n ? vals[i] : 0ull, sh, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(CT_SCAN) void sc_small(const int32_t* __restrict__ gate, u64* __restrict__ v, int n,
                                                          u64* __restrict__ total_out) {
    __shared__ u64 sh[CT_SCAN];
    if (gate && *gate == 0) return;
    u64 run = 0;
    for (int i0 = 0; i0 < n; i0 += CT_SCAN) {
        const int i = i0 + threadIdx.x;
        u64 tot;
        const u64 e = block_scan<u64>(i < n ? v[i] : 0ull, sh, &tot);
        if (i < n) v[i] = run + e;
        run += tot;
    }
    if (threadIdx.x == 0) *total_out = run;
}
__global__ __launch_bounds__(CT_SCAN) void sc_apply(const int32_t* __restrict__ gate, u64* __restrict__ vals,
                                                          const u64* __restrict__ bsum, int n) {
    __shared__ u64 sh[CT_SCAN];
    if (gate && *gate == 0) return;
    const long i = (long)blockIdx.x * CT_SCAN + threadIdx.x;
    u64 tot;
    const u64 e = block_scan<u64>(i < n ? vals[i] : 0ull, sh, &tot);
    if (i < n) vals[i] = bsum[blockIdx.x] + e;
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

// grid (nblk, B): pfx [B][HW], the compact index of the pixel's first crack
__global__ __launch_bounds__(CT_SCAN) void ct_pfx_kernel(const uint8_t* __restrict__ maskb, const u64* __restrict__ bsum,
                                                         int32_t* __restrict__ pfx, int HW, int nblk) {
    __shared__ int sh[CT_SCAN];
    const int b = blockIdx.y, blk = blockIdx.x;
    const int p = blk * CT_SCAN + threadIdx.x;
    const int v = p < HW ? __popc(maskb[(long)b * HW + p] & 15u) : 0;
    int tot;
    const int e = block_scan<int>(v, sh, &tot);
    if (p < HW) pfx[(long)b * HW + p] = (int)bsum[(long)b * nblk + blk] + e;
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
