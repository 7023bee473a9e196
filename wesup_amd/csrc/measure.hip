// Object measurements on the GPU: per label of an int32 label map the moments up to order two, the bounding box,
// the border-pixel classes of the 4-neighbourhood perimeter estimator, the bit-quad counts, the maximum of a distance map and
// the exact convex hull of the pixel corners with its area and its Feret pair -- equal to wesup_amd/measure.py:measure_host word
// for word and vertex for vertex (tests/test_measure_gpu.py).  Integer arithmetic only; where threads meet on one word they use
// integer atomics (add, min, max), whose result does not depend on the order.
//
// The hull comes from row profiles, not from the points: with L[r] / R[r] the smallest column / the largest column + 1 of a label
// in row r, the only corners that can be hull vertices are, per lattice line y in rmin .. rmax + 1, the left candidate
// (min(L[y-1], L[y]), y) and the right candidate (max(R[y-1], R[y]), y) -- h + 1 lines for a label h rows high, lines between two
// empty rows have none.  The left side of the hull is the lower convex envelope of x over y of the left candidates: a candidate
// is a strict vertex iff the largest slope dx / dy from the candidates before it is smaller than the smallest slope to those after
// it (fractions compared by cross-multiplication; a chain's two ends always are); the right side is the same with -x.  That is
// O(h^2) tests per label.  The vertices are ordered left chain top down, then right chain bottom up: counter-clockwise on screen
// from the smallest (y, x).
//
// wesup_measure_profile_count, 5 launches: two fills, ms_box_init, ms_moments, ms_offsets; count = the sum of h + 1 over the labels.
// wesup_object_measure, 19 launches whatever the data (9 when n_prof == 0):
//   fills (status; header + accumulators), ms_box_init
//   ms_moments_kernel   a thread folds runs of equal labels within a row over MS_PIX consecutive pixels, a wave that ends inside one
//                       label folds once more, then one add per entry: into the block's table in LDS when L + 1 <= MS_LDS_LABELS
//                       (flushed with one global atomic per non-empty entry and block), else to global memory
//   ms_local_kernel     one thread per pixel corner: the pixel's maximum of d2 (atomicMax on d2 << 32 | ~pixel: the first pixel in
//                       raster order wins; a wave inside one label folds first), its border class, and the corner's 2 x 2 pattern
//                       of every distinct label among its four pixels
//   ms_offsets_kernel   candidates h + 1 and hull blocks ceil((h + 1) / CHUNK) of every label, both scanned (one block, two block
//                       scans of scan.hpp per round from one read of the boxes)
//   ms_check_kernel     the candidates against n_prof: every later kernel returns at once unless they fit
//   two fills, ms_rows_kernel   L[r] / R[r] of every (label, row) by int32 atomicMin / atomicMax from the ends of runs only
//   ms_cand_kernel      the two candidates of every line
//   fill, ms_hull_kernel   a block per (label, chunk of CHUNK candidates), found by binary search in the scanned block counts;
//                       all candidates of the label stream through LDS; flags and packed coordinates in output order
//   ms_flag_sums, ms_scan_small, ms_flag_apply   the vertex index of every flag, one scan over 2 n_prof flags (the passes of scan.hpp)
//   ms_check2_kernel    the vertices against vert_cap
//   ms_emit_kernel      the vertices
//   ms_final_kernel     a block per label: area2, the Feret pair in two passes over the vertex pairs, and the row of the table
// Nothing is written to table or hull_verts unless both checks pass; status gets bit 0 per image for a label outside [0, L] and
// bit 1 on every image when a capacity is short.
#include "common.hpp"
#include "scan.hpp"

#define MS_BLOCK 256
#define MS_PIX 8                          // consecutive pixels per thread
#define MS_MAX_BLOCKS 1024                // blocks per image of the moments kernel: bounds the flushes of the private tables
#define MS_LDS_LABELS 512                 // 6 x 64-bit sums and 4 x 32-bit box words per label: 32 KB
#define MS_CHUNK WESUP_MEASURE_HULL_CHUNK
#define MS_WORDS WESUP_MEASURE_WORDS
#define MS_SCAN 1024
#define MS_ACC 13                         // 64-bit accumulators per label: 0-5 sums, 6 the d2 key, 7-9 border classes, 10-12 quads
#define MS_HDR_WORDS 64                   // words 0 ok, 2 ok2, 8 vertices; 8-byte totals at words 4 candidates, 6 hull blocks
#define MS_MAX_SIDE 32768
#define MS_MAX_LABELS (1 << 20)
#define MS_MAX_ENTRIES (1l << 26)
#define MS_MAX_PROF (1 << 29)
#define MS_NONE 0x7fffffff

static_assert(MS_CHUNK == MS_BLOCK, "a hull block holds one candidate per thread");
static_assert(MS_WORDS == 24, "the row of the table");

namespace {

typedef unsigned long long u64;
typedef long long i64;

__device__ __forceinline__ int lab_at(const int32_t* __restrict__ img, int H, int W, int r, int c) {
    return ((unsigned)r < (unsigned)H && (unsigned)c < (unsigned)W) ? img[(long)r * W + c] : -1;      // a label l >= 1 never equals it
}
__device__ __forceinline__ bool border_at(const int32_t* __restrict__ img, int H, int W, int r, int c, int l) {
    return lab_at(img, H, W, r - 1, c) != l || lab_at(img, H, W, r + 1, c) != l || lab_at(img, H, W, r, c - 1) != l ||
           lab_at(img, H, W, r, c + 1) != l;
}

__global__ __launch_bounds__(MS_BLOCK) void ms_box_init_kernel(int32_t* __restrict__ box, long n_e, int H, int W) {
    for (long e = (long)blockIdx.x * MS_BLOCK + threadIdx.x; e < n_e; e += (long)gridDim.x * MS_BLOCK)
        *reinterpret_cast<int4*>(box + 4 * e) = make_int4(H, W, -1, -1);
}

struct Run { u64 cnt, sr, sc, srr, src, scc; int r0, c0, r1, c1; };

// a run of cnt pixels of row r from column c0 to c1, sc / scc the sums of their columns and squared columns
__device__ __forceinline__ Run make_run(u64 cnt, int r, u64 sc, u64 scc, int c0, int c1) {
    Run q;
    q.cnt = cnt; q.sr = cnt * (u64)r; q.sc = sc; q.srr = cnt * (u64)r * (u64)r; q.src = (u64)r * sc; q.scc = scc;
    q.r0 = q.r1 = r; q.c0 = c0; q.c1 = c1;
    return q;
}
__device__ __forceinline__ void add_run(u64* __restrict__ sums, int32_t* __restrict__ bx, const Run& q) {
    atomicAdd(sums, q.cnt); atomicAdd(sums + 1, q.sr); atomicAdd(sums + 2, q.sc);
    atomicAdd(sums + 3, q.srr); atomicAdd(sums + 4, q.src); atomicAdd(sums + 5, q.scc);
    atomicMin(bx, q.r0); atomicMin(bx + 1, q.c0); atomicMax(bx + 2, q.r1); atomicMax(bx + 3, q.c1);
}

// grid (blocks, B).  acc [B][L+1][MS_ACC], box [B][L+1][4]; the LDS table: [L+1][6] sums, then [L+1][4] box words
template <bool LDS>
__global__ __launch_bounds__(MS_BLOCK) void ms_moments_kernel(const int32_t* __restrict__ labels, u64* __restrict__ acc,
                                                              int32_t* __restrict__ box, int32_t* __restrict__ status, long HW,
                                                              int W, int L) {
    extern __shared__ u64 ms_tab[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = L + 1;
    int32_t* tbox = reinterpret_cast<int32_t*>(ms_tab + 6 * (LDS ? n : 0));
    if (LDS) {
        for (int i = tid; i < 6 * n; i += MS_BLOCK) ms_tab[i] = 0;
        for (int i = tid; i < 4 * n; i += MS_BLOCK) tbox[i] = (i & 2) ? -1 : MS_NONE;
        __syncthreads();
    }
    const int32_t* lab = labels + (long)b * HW;
    u64* gacc = acc + (long)b * n * MS_ACC;
    int32_t* gbox = box + (long)b * n * 4;
    int bad = 0;
    const long step = (long)gridDim.x * MS_BLOCK * MS_PIX;
    for (long base = (long)blockIdx.x * MS_BLOCK * MS_PIX; base < HW; base += step) {          // uniform over the block
        const long p0 = base + (long)tid * MS_PIX;
        const long p1 = min(HW, p0 + MS_PIX);
        int key = -1, krow = 0, c0 = 0, c1 = 0;
        u64 cnt = 0, sc = 0, scc = 0;
        if (p0 < HW) {
            int row = (int)(p0 / W);
            int col = (int)(p0 - (long)row * W);
            for (long p = p0; p < p1; ++p) {
                const int l = lab[p];
                if (l < 0 || l > L) bad = 1;
                const int k = (l >= 1 && l <= L) ? l : -1;
                if (k != key || row != krow) {
                    if (key >= 0) {
                        const Run q = make_run(cnt, krow, sc, scc, c0, c1);
                        if (LDS) add_run(ms_tab + 6 * key, tbox + 4 * key, q);
                        else add_run(gacc + (long)key * MS_ACC, gbox + 4 * key, q);
                    }
                    key = k; krow = row; c0 = col;
                    cnt = sc = scc = 0;
                }
                if (k >= 0) {
                    ++cnt;
                    sc += (u64)col;
                    scc += (u64)col * (u64)col;
                    c1 = col;
                }
                if (++col == W) { col = 0; ++row; }
            }
        }
        // the pending run: a wave whose pending runs all belong to one label adds once
        Run q = make_run(cnt, krow, sc, scc, c0, c1);
        if (key < 0) { q = make_run(0, 0, 0, 0, 0, 0); q.r0 = q.c0 = MS_NONE; q.r1 = q.c1 = -1; }
        const u64 have = __ballot(key >= 0);
        if (have) {
            const int k0 = __shfl(key, __ffsll((long long)have) - 1);
            if (__all(key < 0 || key == k0)) {
                for (int off = 32; off > 0; off >>= 1) {
                    q.cnt += __shfl_xor(q.cnt, off); q.sr += __shfl_xor(q.sr, off); q.sc += __shfl_xor(q.sc, off);
                    q.srr += __shfl_xor(q.srr, off); q.src += __shfl_xor(q.src, off); q.scc += __shfl_xor(q.scc, off);
                    q.r0 = min(q.r0, __shfl_xor(q.r0, off)); q.c0 = min(q.c0, __shfl_xor(q.c0, off));
                    q.r1 = max(q.r1, __shfl_xor(q.r1, off)); q.c1 = max(q.c1, __shfl_xor(q.c1, off));
                }
                key = (tid & 63) == 0 ? k0 : -1;
            }
            if (key >= 0) {
                if (LDS) add_run(ms_tab + 6 * key, tbox + 4 * key, q);
                else add_run(gacc + (long)key * MS_ACC, gbox + 4 * key, q);
            }
        }
    }
    if (bad) atomicOr(&status[b], 1);
    if (LDS) {
        __syncthreads();
        for (int k = tid; k < n; k += MS_BLOCK) {
            if (ms_tab[6 * k] == 0) continue;
            for (int i = 0; i < 6; ++i) atomicAdd(gacc + (long)k * MS_ACC + i, ms_tab[6 * k + i]);
            atomicMin(gbox + 4 * k, tbox[4 * k]); atomicMin(gbox + 4 * k + 1, tbox[4 * k + 1]);
            atomicMax(gbox + 4 * k + 2, tbox[4 * k + 2]); atomicMax(gbox + 4 * k + 3, tbox[4 * k + 3]);
        }
    }
}

__device__ __forceinline__ int border_class(int v) {
    switch (v) {
        case 5: case 7: case 15: case 17: case 25: case 27: return 0;
        case 21: case 33: return 1;
        case 13: case 23: return 2;
        default: return -1;
    }
}

// grid (ceil((H+1)(W+1) / MS_BLOCK), B): thread = lattice point (x, y) and, inside the image, pixel (y, x)
__global__ __launch_bounds__(MS_BLOCK) void ms_local_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ d2,
                                                            u64* __restrict__ acc, int H, int W, int L) {
    const int b = blockIdx.y;
    const long HW = (long)H * W;
    const long t = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    const int32_t* img = labels + (long)b * HW;
    u64* gacc = acc + (long)b * (L + 1) * MS_ACC;
    const bool in_lattice = t < (long)(H + 1) * (W + 1);
    const int y = in_lattice ? (int)(t / (W + 1)) : 0;
    const int x = in_lattice ? (int)(t - (long)y * (W + 1)) : 0;
    int ke = -1;
    u64 key = 0;
    if (in_lattice && y < H && x < W) {
        const int l = img[(long)y * W + x];
        if (l >= 1 && l <= L) {
            if (d2) {
                ke = l;
                key = ((u64)(unsigned)d2[(long)b * HW + (long)y * W + x] << 32) | (u64)(~(unsigned)(y * W + x));
            }
            if (border_at(img, H, W, y, x, l)) {
                int v = 1;
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dx = -1; dx <= 1; ++dx) {
                        if (dy == 0 && dx == 0) continue;
                        if (lab_at(img, H, W, y + dy, x + dx) == l && border_at(img, H, W, y + dy, x + dx, l))
                            v += (dy == 0 || dx == 0) ? 2 : 10;
                    }
                const int cls = border_class(v);
                if (cls >= 0) atomicAdd(gacc + (long)l * MS_ACC + 7 + cls, 1ull);
            }
        }
    }
    // the maximum of d2: every thread of the wave is here
    const u64 have = __ballot(ke >= 0);
    if (have) {
        const int k0 = __shfl(ke, __ffsll((long long)have) - 1);
        if (__all(ke < 0 || ke == k0)) {
            for (int off = 32; off > 0; off >>= 1) key = max(key, __shfl_xor(key, off));
            ke = (threadIdx.x & 63) == 0 ? k0 : -1;
        }
        if (ke >= 0) {
            u64* word = gacc + (long)ke * MS_ACC + 6;
            if (key > __atomic_load_n(word, __ATOMIC_RELAXED)) atomicMax(word, key);         // (the word only grows: a stale read asks for an atomic too many, never one too few)
        }
    }
    if (in_lattice) {
        const int q[4] = {lab_at(img, H, W, y - 1, x - 1), lab_at(img, H, W, y - 1, x), lab_at(img, H, W, y, x - 1),
                          lab_at(img, H, W, y, x)};                                             // NW NE SW SE
        if (q[0] == q[1] && q[1] == q[2] && q[2] == q[3]) return;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int l = q[i];
            if (l < 1 || l > L) continue;
            bool seen = false;
#pragma unroll
            for (int j = 0; j < i; ++j) seen = seen || q[j] == l;
            if (seen) continue;
            const int cnt = (q[0] == l) + (q[1] == l) + (q[2] == l) + (q[3] == l);
            int w = -1;
            if (cnt == 1) w = 10;
            else if (cnt == 3) w = 11;
            else if (cnt == 2 && ((q[0] == l && q[3] == l) || (q[1] == l && q[2] == l))) w = 12;
            if (w >= 0) atomicAdd(gacc + (long)l * MS_ACC + w, 1ull);
        }
    }
}

// one block: offc / offk [n_e + 1], the exclusive scans of the candidates and of the hull blocks of every entry
__global__ __launch_bounds__(MS_SCAN) void ms_offsets_kernel(const int32_t* __restrict__ box, u64* __restrict__ offc,
                                                             u64* __restrict__ offk, int32_t* __restrict__ hdr,
                                                             i64* __restrict__ count_out, long n_e) {
    __shared__ u64 sh[MS_SCAN];
    u64 runc = 0, runk = 0;
    for (long e0 = 0; e0 < n_e; e0 += MS_SCAN) {
        const long e = e0 + threadIdx.x;
        u64 c = 0;
        if (e < n_e) {
            const int4 bx = *reinterpret_cast<const int4*>(box + 4 * e);
            if (bx.z >= bx.x) c = (u64)(bx.z - bx.x + 2);
        }
        const u64 k = (c + MS_CHUNK - 1) / MS_CHUNK;
        u64 totc, totk;
        const u64 ec = scan::block_scan<u64, MS_SCAN>(c, sh, &totc);
        const u64 ek = scan::block_scan<u64, MS_SCAN>(k, sh, &totk);
        if (e < n_e) { offc[e] = runc + ec; offk[e] = runk + ek; }
        runc += totc;
        runk += totk;
    }
    if (threadIdx.x == 0) {
        offc[n_e] = runc;
        offk[n_e] = runk;
        *reinterpret_cast<u64*>(hdr + 4) = runc;
        *reinterpret_cast<u64*>(hdr + 6) = runk;
        if (count_out) *count_out = (i64)runc;
    }
}

__global__ void ms_check_kernel(int32_t* __restrict__ hdr, int32_t* __restrict__ status, int B, int n_prof) {
    if (*reinterpret_cast<const u64*>(hdr + 4) <= (u64)n_prof) hdr[0] = 1;
    else for (int b = 0; b < B; ++b) atomicOr(status + b, 2);
}
__global__ void ms_check2_kernel(int32_t* __restrict__ hdr, int32_t* __restrict__ status, int B, int vert_cap) {
    if (hdr[0] == 0) return;
    if (hdr[8] <= vert_cap) hdr[2] = 1;
    else for (int b = 0; b < B; ++b) atomicOr(status + b, 2);
}

// grid (ceil(HW / (MS_BLOCK MS_PIX)), B): lrow / rrow [n_prof], slot offc[e] + r - rmin of label entry e
__global__ __launch_bounds__(MS_BLOCK) void ms_rows_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ labels,
                                                           const int32_t* __restrict__ box, const u64* __restrict__ offc,
                                                           int32_t* __restrict__ lrow, int32_t* __restrict__ rrow, long HW, int W,
                                                           int L, int n_prof) {
    if (hdr[0] == 0) return;
    const int b = blockIdx.y;
    const long p0 = ((long)blockIdx.x * MS_BLOCK + threadIdx.x) * MS_PIX;
    if (p0 >= HW) return;
    const long p1 = min(HW, p0 + MS_PIX);
    const int32_t* lab = labels + (long)b * HW;
    const long e0 = (long)b * (L + 1);
    int row = (int)(p0 / W);
    int col = (int)(p0 - (long)row * W);
    long p = p0;
    while (p < p1) {
        const int l = lab[p];
        const int c0 = col;
        long q = p + 1;
        int c1 = col;
        while (q < p1 && c1 + 1 < W && lab[q] == l) { ++q; ++c1; }                    // the run [c0, c1] of row `row`
        if (l >= 1 && l <= L) {
            const bool starts = !(p == p0 && c0 > 0 && lab[p - 1] == l);            // not the tail of the previous thread's run
            const bool ends = !(q == p1 && c1 + 1 < W && q < HW && lab[q] == l);
            const long e = e0 + l;
            const long slot = (long)offc[e] + (row - box[4 * e]);
            if (slot >= 0 && slot < n_prof) {
                if (starts) atomicMin(lrow + slot, c0);
                if (ends) atomicMax(rrow + slot, c1 + 1);
            }
        }
        col = c1 + 1;
        if (col == W) { col = 0; ++row; }
        p = q;
    }
}

// the last entry whose offset is <= i: the entry that holds element i (entries without elements share their successor's offset)
__device__ __forceinline__ long find_entry(const u64* __restrict__ off, long n_e, u64 i) {
    long lo = 0, hi = n_e - 1;
    while (lo < hi) {
        const long mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// candl / candr [n_prof]: the candidates of line i - offc[e] of entry e; MS_NONE / -1 between two empty rows
__global__ __launch_bounds__(MS_BLOCK) void ms_cand_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ box,
                                                           const u64* __restrict__ offc, const int32_t* __restrict__ lrow,
                                                           const int32_t* __restrict__ rrow, int32_t* __restrict__ candl,
                                                           int32_t* __restrict__ candr, long n_e) {
    if (hdr[0] == 0) return;
    const long i = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (i >= (long)*reinterpret_cast<const u64*>(hdr + 4)) return;
    const long e = find_entry(offc, n_e, (u64)i);
    const long s = (long)offc[e];
    const int k = (int)(i - s);
    const int h = box[4 * e + 2] - box[4 * e] + 1;
    int xl = MS_NONE, xr = -1;
    if (k >= 1) { xl = lrow[i - 1]; xr = rrow[i - 1]; }
    if (k < h) { xl = min(xl, lrow[i]); xr = max(xr, rrow[i]); }
    candl[i] = xl;
    candr[i] = xr;
}

// grid (an upper bound of the hull blocks): block j is chunk j - offk[e] of entry e.  seqf / seqxy [2 n_prof]: of entry e with
// candidates [s, s + cnt) the places 2 s .. 2 s + cnt - 1 are the left chain top down, the next cnt the right chain bottom up
__global__ __launch_bounds__(MS_BLOCK) void ms_hull_kernel(const int32_t* __restrict__ hdr, const int32_t* __restrict__ box,
                                                           const u64* __restrict__ offc, const u64* __restrict__ offk,
                                                           const int32_t* __restrict__ candl, const int32_t* __restrict__ candr,
                                                           uint8_t* __restrict__ seqf, uint32_t* __restrict__ seqxy, long n_e,
                                                           int n_prof) {
    __shared__ int shl[MS_CHUNK], shr[MS_CHUNK];
    if (hdr[0] == 0) return;
    const u64 j = blockIdx.x;
    if (j >= *reinterpret_cast<const u64*>(hdr + 6)) return;
    const long e = find_entry(offk, n_e, j);
    const long s = (long)offc[e];
    const int cnt = (int)(offc[e + 1] - offc[e]);
    const int tid = threadIdx.x;
    const int ki = (int)(j - offk[e]) * MS_CHUNK + tid;
    const bool valid = ki < cnt && s + cnt <= n_prof;
    const int xl = valid ? candl[s + ki] : MS_NONE, xr = valid ? candr[s + ki] : -1;
    // the largest slope from before and the smallest to after as fractions n / d, d > 0; has*: one was seen
    i64 lbn = 0, lbd = 1, lan = 0, lad = 1, rbn = 0, rbd = 1, ran = 0, rad = 1;
    bool hlb = false, hla = false, hrb = false, hra = false;
    for (int t0 = 0; t0 < cnt; t0 += MS_CHUNK) {
        const int tj = t0 + tid;
        shl[tid] = tj < cnt ? candl[s + tj] : MS_NONE;
        shr[tid] = tj < cnt ? candr[s + tj] : -1;
        __syncthreads();
        const int m = min(MS_CHUNK, cnt - t0);
        for (int jj = 0; jj < m; ++jj) {
            const int kj = t0 + jj;
            const int yl = shl[jj], yr = shr[jj];
            if (yr < 0 || kj == ki) continue;                                   // a line without candidates (both or none exist)
            if (kj < ki) {
                const i64 d = ki - kj, nl = xl - yl, nr = yr - xr;              // right chain: the same test on -x
                if (!hlb || nl * lbd > lbn * d) { lbn = nl; lbd = d; hlb = true; }
                if (!hrb || nr * rbd > rbn * d) { rbn = nr; rbd = d; hrb = true; }
            } else {
                const i64 d = kj - ki, nl = yl - xl, nr = xr - yr;
                if (!hla || nl * lad < lan * d) { lan = nl; lad = d; hla = true; }
                if (!hra || nr * rad < ran * d) { ran = nr; rad = d; hra = true; }
            }
        }
        __syncthreads();
    }
    if (!valid) return;
    const bool there = xr >= 0;
    const bool fl = there && (!hlb || !hla || lbn * lad < lan * lbd);
    const bool fr = there && (!hrb || !hra || rbn * rad < ran * rbd);
    const unsigned y = (unsigned)(box[4 * e] + ki);
    const long ql = 2 * s + ki, qr = 2 * s + cnt + (cnt - 1 - ki);
    seqf[ql] = fl;
    seqf[qr] = fr;
    seqxy[ql] = (y << 16) | (unsigned)(there ? xl : 0);
    seqxy[qr] = (y << 16) | (unsigned)(there ? xr : 0);
}

// the scan of the flags in three kernels (scan.hpp)
__global__ __launch_bounds__(MS_SCAN) void ms_flag_sums_kernel(const int32_t* __restrict__ hdr, const uint8_t* __restrict__ seqf,
                                                               int* __restrict__ bsum, long n) {
    if (hdr[0] == 0) return;
    const int tot = scan::scan_block_total<int, MS_SCAN>([seqf](long i) { return (int)seqf[i]; }, n);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}
__global__ __launch_bounds__(MS_SCAN) void ms_scan_small_kernel(int32_t* __restrict__ hdr, int* __restrict__ v, int n) {
    if (hdr[0] == 0) return;
    int run;
    scan::scan_small<int, MS_SCAN>(v, n, &run);
    if (threadIdx.x == 0) hdr[8] = run;
}
__global__ __launch_bounds__(MS_SCAN) void ms_flag_apply_kernel(const int32_t* __restrict__ hdr, const uint8_t* __restrict__ seqf,
                                                                const int* __restrict__ bsum, int* __restrict__ seqi, long n) {
    if (hdr[0] == 0) return;
    scan::scan_apply<int, MS_SCAN>([seqf](long i) { return (int)seqf[i]; }, [seqi](long i, int x) { seqi[i] = x; }, bsum[blockIdx.x],
                                   n);
}

__global__ __launch_bounds__(MS_BLOCK) void ms_emit_kernel(const int32_t* __restrict__ hdr, const uint8_t* __restrict__ seqf,
                                                           const uint32_t* __restrict__ seqxy, const int* __restrict__ seqi,
                                                           int32_t* __restrict__ verts, long n, int vert_cap) {
    if (hdr[2] == 0) return;
    const long q = (long)blockIdx.x * MS_BLOCK + threadIdx.x;
    if (q >= n || !seqf[q]) return;
    const int v = seqi[q];
    if ((unsigned)v >= (unsigned)vert_cap) return;
    const uint32_t xy = seqxy[q];
    verts[2 * (long)v] = (int)(xy & 0xffffu);
    verts[2 * (long)v + 1] = (int)(xy >> 16);
}

template <typename T, typename F>
__device__ __forceinline__ T block_reduce(T v, T* sh, F f) {
    for (int off = 32; off > 0; off >>= 1) v = f(v, __shfl_xor(v, off));
    __syncthreads();                                                            // (sh may still be read from the reduction before)
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    T r = sh[0];
    for (int i = 1; i < MS_BLOCK / 64; ++i) r = f(r, sh[i]);
    return r;
}

// grid (L + 1, B): the row of label blockIdx.x
__global__ __launch_bounds__(MS_BLOCK) void ms_final_kernel(const int32_t* __restrict__ hdr, const u64* __restrict__ acc,
                                                            const int32_t* __restrict__ box, const u64* __restrict__ offc,
                                                            const int* __restrict__ seqi, const int32_t* __restrict__ verts,
                                                            i64* __restrict__ table, int W, int L, long n2, int vert_cap,
                                                            int has_d2) {
    __shared__ i64 sh[MS_BLOCK / 64];
    if (hdr[2] == 0) return;
    const int l = blockIdx.x, tid = threadIdx.x;
    const long e = (long)blockIdx.y * (L + 1) + l;
    i64* row = table + e * MS_WORDS;
    const int4 bx = *reinterpret_cast<const int4*>(box + 4 * e);
    if (l == 0 || bx.z < bx.x) {                                                // background, or an absent label
        if (tid < MS_WORDS) row[tid] = (l != 0 && tid >= 6 && tid < 10) ? (i64)(tid == 6 ? bx.x : tid == 7 ? bx.y : -1) : 0;
        return;
    }
    const long s = (long)offc[e], cnt = (long)(offc[e + 1] - offc[e]);
    const int total_v = hdr[8];
    const int v0 = seqi[2 * s];
    const int v1 = 2 * (s + cnt) < n2 ? seqi[2 * (s + cnt)] : total_v;
    int nv = v1 - v0;
    if (v0 < 0 || nv < 0 || (long)v0 + nv > vert_cap) nv = 0;                    // (cannot happen behind the checks: keeps every index inside)
    const int32_t* pv = verts + 2 * (long)v0;
    i64 area = 0, best = 0;
    for (int i = tid; i < nv; i += MS_BLOCK) {
        const int k = i + 1 < nv ? i + 1 : 0;
        const i64 xi = pv[2 * i], yi = pv[2 * i + 1], xk = pv[2 * k], yk = pv[2 * k + 1];
        area -= xi * yk - xk * yi;
        for (int j = i + 1; j < nv; ++j) {
            const i64 dx = pv[2 * j] - xi, dy = pv[2 * j + 1] - yi;
            best = max(best, dx * dx + dy * dy);
        }
    }
    area = block_reduce<i64>(area, sh, [](i64 a, i64 c) { return a + c; });
    best = block_reduce<i64>(best, sh, [](i64 a, i64 c) { return a > c ? a : c; });
    u64 pair = ~0ull;
    for (int i = tid; i < nv; i += MS_BLOCK) {
        const i64 xi = pv[2 * i], yi = pv[2 * i + 1];
        const u64 li = (u64)(yi * (W + 1) + xi);
        for (int j = i + 1; j < nv; ++j) {
            const i64 xj = pv[2 * j], yj = pv[2 * j + 1];
            if ((xj - xi) * (xj - xi) + (yj - yi) * (yj - yi) != best) continue;
            const u64 lj = (u64)(yj * (W + 1) + xj);
            pair = min(pair, li < lj ? (li << 32) | lj : (lj << 32) | li);
        }
    }
    pair = (u64)block_reduce<i64>((i64)pair, sh, [](i64 a, i64 c) { return (u64)a < (u64)c ? a : c; });
    if (nv < 2) pair = 0;
    const u64* a = acc + e * MS_ACC;
    if (tid < 6) row[tid] = (i64)a[tid];
    else if (tid < 10) row[tid] = tid == 6 ? bx.x : tid == 7 ? bx.y : tid == 8 ? bx.z : bx.w;
    else if (tid < 16) row[tid] = (i64)a[tid - 3];
    else if (tid == 16) row[16] = area;
    else if (tid == 17) row[17] = nv;
    else if (tid == 18) row[18] = best;
    else if (tid == 19) row[19] = (i64)(pair >> 32);
    else if (tid == 20) row[20] = (i64)(pair & 0xffffffffull);
    else if (tid == 21) row[21] = has_d2 ? (i64)(a[6] >> 32) : 0;
    else if (tid == 22) row[22] = has_d2 ? (i64)(~(unsigned)a[6]) : 0;
    else if (tid == 23) row[23] = v0;
}

inline bool bad_shape(int B, int H, int W, int L) {
    return B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > MS_MAX_SIDE || W > MS_MAX_SIDE || L < 0 || L + 1 > MS_MAX_LABELS ||
           (long)B * (L + 1) > MS_MAX_ENTRIES || (long)B * H * W >= (1l << 40);
}
inline bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

struct Layout { size_t hdr, acc, box, offc, offk, lrow, rrow, candl, candr, seqf, seqxy, seqi, bsum, total; };
inline Layout layout(int B, int L, long n_prof) {
    const size_t n_e = (size_t)B * (L + 1), n = (size_t)n_prof;
    Layout Y;
    size_t o = 0;
    Y.hdr = o; o += align_up(MS_HDR_WORDS * 4, 256);
    Y.acc = o; o += align_up(n_e * MS_ACC * 8, 256);
    Y.box = o; o += align_up(n_e * 16, 256);
    Y.offc = o; o += align_up((n_e + 1) * 8, 256);
    Y.offk = o; o += align_up((n_e + 1) * 8, 256);
    Y.lrow = o; o += align_up(n * 4, 256);
    Y.rrow = o; o += align_up(n * 4, 256);
    Y.candl = o; o += align_up(n * 4, 256);
    Y.candr = o; o += align_up(n * 4, 256);
    Y.seqf = o; o += align_up(2 * n, 256);
    Y.seqxy = o; o += align_up(2 * n * 4, 256);
    Y.seqi = o; o += align_up(2 * n * 4, 256);
    Y.bsum = o; o += align_up(((2 * n + MS_SCAN - 1) / MS_SCAN) * 4, 256);
    Y.total = o;
    return Y;
}

// the launches both entries start with: accumulators, boxes, moments, offsets
int measure_front(const int32_t* labels, int32_t* status, i64* count_out, int B, int H, int W, int L, char* w, const Layout& Y,
                  hipStream_t st) {
    const long n_e = (long)B * (L + 1), HW = (long)H * W;
    if (wesup_fill_words_(w + Y.hdr, 0u, (Y.box - Y.hdr) / 4, st) != WESUP_OK) return WESUP_ERR_LAUNCH;          // header and accumulators
    WESUP_LAUNCH(ms_box_init_kernel, dim3(grid_stride_blocks(n_e, MS_BLOCK, 4096)), dim3(MS_BLOCK), 0, st, (int32_t*)(w + Y.box), n_e,
                 H, W);
    const unsigned gx = grid_stride_blocks((HW + MS_PIX - 1) / MS_PIX, MS_BLOCK, MS_MAX_BLOCKS);
    if (L + 1 <= MS_LDS_LABELS)
        WESUP_LAUNCH(ms_moments_kernel<true>, dim3(gx, B), dim3(MS_BLOCK), (size_t)(L + 1) * 64, st, labels, (u64*)(w + Y.acc),
                     (int32_t*)(w + Y.box), status, HW, W, L);
    else
        WESUP_LAUNCH(ms_moments_kernel<false>, dim3(gx, B), dim3(MS_BLOCK), 0, st, labels, (u64*)(w + Y.acc), (int32_t*)(w + Y.box),
                     status, HW, W, L);
    WESUP_LAUNCH(ms_offsets_kernel, dim3(1), dim3(MS_SCAN), 0, st, (const int32_t*)(w + Y.box), (u64*)(w + Y.offc), (u64*)(w + Y.offk),
                 (int32_t*)(w + Y.hdr), count_out, n_e);
    return WESUP_OK;
}

}  // namespace

extern "C" int wesup_measure_limit(int which) {
    return which == 0 ? MS_LDS_LABELS : which == 1 ? MS_CHUNK : which == 2 ? MS_WORDS : which == 3 ? MS_MAX_SIDE
         : which == 4 ? MS_MAX_LABELS : which == 5 ? MS_MAX_PROF : -1;
}

extern "C" size_t wesup_measure_workspace_bytes(int B, int H, int W, int L, int n_prof) {
    if (bad_shape(B, H, W, L) || n_prof < 0 || n_prof > MS_MAX_PROF) return 0;
    return layout(B, L, n_prof).total;
}

extern "C" int wesup_measure_profile_count(const int32_t* labels, int64_t* count, int32_t* status, int B, int H, int W, int L,
                                           void* ws, size_t ws_bytes, void* stream) {
    if (!labels || !count || !status || !ws || bad_shape(B, H, W, L)) return WESUP_ERR_INVALID;
    if (((uintptr_t)ws & 15) || ((uintptr_t)labels & 3) || ((uintptr_t)count & 7) || ((uintptr_t)status & 3)) return WESUP_ERR_INVALID;
    const Layout Y = layout(B, L, 0);
    if (ws_bytes < Y.total) return WESUP_ERR_INVALID;
    const void* ops[4] = {labels, count, status, ws};
    const size_t len[4] = {(size_t)B * H * W * 4, 8, (size_t)B * 4, Y.total};
    for (int i = 0; i < 4; ++i)
        for (int j = i + 1; j < 4; ++j)
            if (overlap(ops[i], len[i], ops[j], len[j])) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (wesup_fill_words_(status, 0u, (size_t)B, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (measure_front(labels, status, (i64*)count, B, H, W, L, (char*)ws, Y, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_object_measure(const int32_t* labels, const int32_t* d2, int64_t* table, int32_t* hull_verts, int32_t* status,
                                    int B, int H, int W, int L, int n_prof, int vert_cap, void* ws, size_t ws_bytes, void* stream) {
    if (!labels || !table || !hull_verts || !status || !ws || bad_shape(B, H, W, L)) return WESUP_ERR_INVALID;
    if (n_prof < 0 || n_prof > MS_MAX_PROF || vert_cap < 0) return WESUP_ERR_INVALID;
    if (((uintptr_t)ws & 15) || ((uintptr_t)labels & 3) || ((uintptr_t)d2 & 3) || ((uintptr_t)table & 7) ||
        ((uintptr_t)hull_verts & 3) || ((uintptr_t)status & 3))
        return WESUP_ERR_INVALID;
    const Layout Y = layout(B, L, n_prof);
    if (ws_bytes < Y.total) return WESUP_ERR_INVALID;
    // an empty capacity still names a word: the overlap test takes every operand as at least one element long
    const size_t nl = (size_t)B * H * W * 4;
    const void* ops[6] = {labels, table, hull_verts, status, ws, d2};
    const size_t len[6] = {nl, (size_t)B * (L + 1) * MS_WORDS * 8, (size_t)(vert_cap > 0 ? vert_cap : 1) * 8, (size_t)B * 4, Y.total, nl};
    for (int i = 0; i < (d2 ? 6 : 5); ++i)
        for (int j = i + 1; j < (d2 ? 6 : 5); ++j)
            if (!(i == 0 && j == 5) && overlap(ops[i], len[i], ops[j], len[j])) return WESUP_ERR_INVALID;      // (both are only read)
    hipStream_t st = (hipStream_t)stream;
    char* w = (char*)ws;
    int32_t* hdr = (int32_t*)(w + Y.hdr);
    u64* acc = (u64*)(w + Y.acc);
    int32_t* box = (int32_t*)(w + Y.box);
    u64* offc = (u64*)(w + Y.offc);
    u64* offk = (u64*)(w + Y.offk);
    int32_t* lrow = (int32_t*)(w + Y.lrow);
    int32_t* rrow = (int32_t*)(w + Y.rrow);
    int32_t* candl = (int32_t*)(w + Y.candl);
    int32_t* candr = (int32_t*)(w + Y.candr);
    uint8_t* seqf = (uint8_t*)(w + Y.seqf);
    uint32_t* seqxy = (uint32_t*)(w + Y.seqxy);
    int* seqi = (int*)(w + Y.seqi);
    int* bsum = (int*)(w + Y.bsum);
    const long n_e = (long)B * (L + 1), HW = (long)H * W, n2 = 2l * n_prof;
    if (wesup_fill_words_(status, 0u, (size_t)B, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (measure_front(labels, status, (i64*)nullptr, B, H, W, L, w, Y, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    const long lattice = (long)(H + 1) * (W + 1);
    WESUP_LAUNCH(ms_local_kernel, dim3((unsigned)((lattice + MS_BLOCK - 1) / MS_BLOCK), B), dim3(MS_BLOCK), 0, st, labels, d2, acc, H, W, L);
    WESUP_LAUNCH(ms_check_kernel, dim3(1), dim3(1), 0, st, hdr, status, B, n_prof);
    if (n_prof > 0) {
        const unsigned gp = (unsigned)((n_prof + MS_BLOCK - 1) / MS_BLOCK), gs = (unsigned)((n2 + MS_SCAN - 1) / MS_SCAN);
        if (wesup_fill_words_(lrow, (unsigned)MS_NONE, (size_t)n_prof, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
        if (wesup_fill_words_(rrow, 0xffffffffu, (size_t)n_prof, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
        WESUP_LAUNCH(ms_rows_kernel, dim3((unsigned)((HW + MS_BLOCK * MS_PIX - 1) / (MS_BLOCK * MS_PIX)), B), dim3(MS_BLOCK), 0, st,
                     (const int32_t*)hdr, labels, (const int32_t*)box, (const u64*)offc, lrow, rrow, HW, W, L, n_prof);
        WESUP_LAUNCH(ms_cand_kernel, dim3(gp), dim3(MS_BLOCK), 0, st, (const int32_t*)hdr, (const int32_t*)box, (const u64*)offc,
                     (const int32_t*)lrow, (const int32_t*)rrow, candl, candr, n_e);
        if (wesup_fill_words_(seqf, 0u, (size_t)((n2 + 3) / 4), st) != WESUP_OK) return WESUP_ERR_LAUNCH;
        // hull blocks: ceil(c / CHUNK) <= c / CHUNK + 1 summed over the present labels, of which there are at most n_e and n_prof / 2
        const long present = n_e < n_prof / 2 ? n_e : n_prof / 2;
        WESUP_LAUNCH(ms_hull_kernel, dim3((unsigned)(n_prof / MS_CHUNK + present + 1)), dim3(MS_BLOCK), 0, st, (const int32_t*)hdr,
                     (const int32_t*)box, (const u64*)offc, (const u64*)offk, (const int32_t*)candl, (const int32_t*)candr, seqf,
                     seqxy, n_e, n_prof);
        WESUP_LAUNCH(ms_flag_sums_kernel, dim3(gs), dim3(MS_SCAN), 0, st, (const int32_t*)hdr, (const uint8_t*)seqf, bsum, n2);
        WESUP_LAUNCH(ms_scan_small_kernel, dim3(1), dim3(MS_SCAN), 0, st, hdr, bsum, (int)gs);
        WESUP_LAUNCH(ms_flag_apply_kernel, dim3(gs), dim3(MS_SCAN), 0, st, (const int32_t*)hdr, (const uint8_t*)seqf, (const int*)bsum,
                     seqi, n2);
    }
    WESUP_LAUNCH(ms_check2_kernel, dim3(1), dim3(1), 0, st, hdr, status, B, vert_cap);
    if (n_prof > 0)
        WESUP_LAUNCH(ms_emit_kernel, dim3((unsigned)((n2 + MS_BLOCK - 1) / MS_BLOCK)), dim3(MS_BLOCK), 0, st, (const int32_t*)hdr,
                     (const uint8_t*)seqf, (const uint32_t*)seqxy, (const int*)seqi, hull_verts, n2, vert_cap);
    WESUP_LAUNCH(ms_final_kernel, dim3(L + 1, B), dim3(MS_BLOCK), 0, st, (const int32_t*)hdr, (const u64*)acc, (const int32_t*)box,
                 (const u64*)offc, (const int*)seqi, (const int32_t*)hull_verts, (i64*)table, W, L, n2, vert_cap, d2 ? 1 : 0);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
