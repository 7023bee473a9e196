// Mask post-processing and the integer half of the GlaS challenge metrics on the GPU: connected components,
// small-region clean-up, binary morphology with scipy's conventions, the contingency table of two label maps, per-label pixel
// lists and the squared directed Hausdorff distance of object pairs.  Everything here is integer arithmetic on integer data:
// the results do not depend on the order of the atomics or on the run, and are held to scipy / numpy bit for bit
// (tests/test_regions_gpu.py).  The float formulas of the metrics stay on the host (utils/metrics.py).
//
// Connected components (4- or 8-connected) by union-find, root = smallest pixel index of the component = its first pixel in
// raster order:
//   1. rg_tile_kernel    one block per 16 x 16 tile: union-find in LDS, then parent[p] = global index of the tile-local root;
//   2. rg_border_kernel  unions only across tile borders, in global memory, with atomicMin (as uf_union of slic.hip);
//   3. rg_flatten_kernel parent[p] = root (and the root flags / the areas per root);
//   4. the three-kernel scan of the root flags (scan.hpp) and the relabel: ids 1..n in raster order of the first pixel.
// Parents only ever decrease, so every find / union loop terminates.  Merge, flatten and renumber are separate launches: the
// kernel boundary makes one XCD's writes visible to the others.  Inside the merge kernel a load of parent[] may be stale; it is
// then an OLDER parent of that pixel, i.e. still a member of the same tree with an index >= the current one, and the atomicMin
// returns the true previous value, from which the union continues -- the loads are agent-scope atomic loads all the same (they
// bypass the CU's L1, which no other CU's store refreshes).
#include "common.hpp"
#include "scan.hpp"

#define RG_TILE 16
#define RG_SCAN 1024
#define RG_CHUNK 2048          // pixels per block of the counting sort
#define RG_MAX_LABELS 16384    // cursor table of the placement kernel: 64 KB of LDS
#define RG_MAX_FP 1024         // footprint cells
#define RG_HD_PIX 4            // pixels of a per lane in the Hausdorff kernel
#define RG_HD_BLOCK 256
#define RG_HD_TILE 1024        // boundary pixels of b staged per pass

namespace {

// ---------------------------------------------------------------------------------------------------- union-find
__device__ __forceinline__ int lds_find(volatile int* par, int a) {
    while (true) {
        const int p = par[a];
        if (p == a) return a;
        a = p;
    }
}
__device__ __forceinline__ void lds_union(int* par, int a, int b) {
    a = lds_find(par, a);
    b = lds_find(par, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(&par[a], b);
        if (old == a) break;
        a = lds_find(par, old);
        b = lds_find(par, b);
    }
}
__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_find(const int* par, int a) {
    while (true) {
        const int p = g_load(&par[a]);
        if (p == a) return a;
        a = p;
    }
}
__device__ __forceinline__ void g_union(int* par, int a, int b) {
    a = g_find(par, a);
    b = g_find(par, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }      // a > b: hang the larger root under the smaller
        const int old = atomicMin(&par[a], b);
        if (old == a) break;                                // a was a root and now points to b
        a = g_find(par, old);                               // a had been re-parented: union(old, b) restores either lost link
        b = g_find(par, b);
    }
}

// pixels of the pass: (mask != 0) == value.  parent = -1 for the others.
__global__ __launch_bounds__(256) void rg_tile_kernel(const uint8_t* __restrict__ mask, int* __restrict__ parent, int H, int W,
                                                      int conn8, int value) {
    __shared__ int par[RG_TILE * RG_TILE];
    __shared__ uint8_t on_s[RG_TILE * RG_TILE];
    const int b = blockIdx.z, tid = threadIdx.x;
    const int ty0 = blockIdx.y * RG_TILE, tx0 = blockIdx.x * RG_TILE;
    const int ly = tid >> 4, lx = tid & 15, y = ty0 + ly, x = tx0 + lx;
    const bool inside = y < H && x < W;
    const long idx = ((long)b * H + y) * W + x;
    const bool on = inside && ((mask[idx] != 0) == (value != 0));
    on_s[tid] = on ? 1 : 0;
    par[tid] = tid;
    __syncthreads();
    if (on) {
        if (lx > 0 && on_s[tid - 1]) lds_union(par, tid, tid - 1);
        if (ly > 0 && on_s[tid - RG_TILE]) lds_union(par, tid, tid - RG_TILE);
        if (conn8 && ly > 0) {
            if (lx > 0 && on_s[tid - RG_TILE - 1]) lds_union(par, tid, tid - RG_TILE - 1);
            if (lx < RG_TILE - 1 && on_s[tid - RG_TILE + 1]) lds_union(par, tid, tid - RG_TILE + 1);
        }
    }
    __syncthreads();
    if (inside) {
        int r = -1;
        if (on) {
            const int l = lds_find(par, tid);               // smallest local index = smallest global index of the tile's part
            r = (ty0 + (l >> 4)) * W + tx0 + (l & 15);
        }
        parent[idx] = r;
    }
}
__global__ void rg_border_kernel(int* __restrict__ parent, int H, int W, int B, int conn8) {
    const long HW = (long)H * W;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * HW) return;
    const int b = (int)(idx / HW);
    const int p = (int)(idx - (long)b * HW);
    const int y = p / W, x = p - y * W;
    const bool ex = (x & (RG_TILE - 1)) == 0, ey = (y & (RG_TILE - 1)) == 0, exr = (x & (RG_TILE - 1)) == RG_TILE - 1;
    if (!(ex || ey || (conn8 && exr))) return;
    int* par = parent + (long)b * HW;
    if (par[p] < 0) return;                                 // (-1 never changes: a plain load is exact)
    if (ex && x > 0 && par[p - 1] >= 0) g_union(par, p, p - 1);
    if (ey && y > 0 && par[p - W] >= 0) g_union(par, p, p - W);
    if (conn8 && y > 0) {
        if ((ex || ey) && x > 0 && par[p - W - 1] >= 0) g_union(par, p, p - W - 1);
        if ((exr || ey) && x + 1 < W && par[p - W + 1] >= 0) g_union(par, p, p - W + 1);
    }
}
// parent[p] = root; flags[p] = p is a root (flags != NULL); area[root] += 1 (area != NULL, zeroed by the caller); 256 threads
__global__ void rg_flatten_kernel(int* __restrict__ parent, int32_t* __restrict__ flags, int32_t* __restrict__ area, long HW,
                                  int B) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * HW) return;
    const long b = idx / HW;
    const int p = (int)(idx - b * HW);
    int* par = parent + b * HW;
    int r = par[p];
    if (r >= 0) {
        while (true) {                                      // (another thread may already have flattened a link: still an ancestor)
            const int q = par[r];
            if (q == r) break;
            r = q;
        }
        par[p] = r;
    }
    if (flags) flags[idx] = (r == p) ? 1 : 0;
    if (area) {
        // one add per (wave, root): the lanes of equal root count themselves with ballots (all pixels of the background adding 1 to
        // one word serialise otherwise: 4 ms at 522 x 775)
        const int lane = threadIdx.x & 63;
        unsigned long long rem = __ballot(r >= 0);
        while (rem) {
            const int leader = __ffsll((long long)rem) - 1;
            const int rb = __shfl((int)b, leader), rr = __shfl(r, leader);
            const unsigned long long m = __ballot(r == rr && (int)b == rb);
            if (lane == leader) atomicAdd(&area[(long)rb * HW + rr], __popcll(m));
            rem &= ~m;
        }
    }
}

// the scan of the root flags in three kernels (scan.hpp), grid (nblk, B)
__global__ __launch_bounds__(RG_SCAN) void rg_scan_block_sums(const int32_t* __restrict__ flags, int32_t* __restrict__ bsum,
                                                              long HW, int nblk) {
    const int32_t* f = flags + (long)blockIdx.y * HW;
    const int s = scan::scan_block_total<int, RG_SCAN>([f](long p) { return f[p]; }, HW);
    if (threadIdx.x == 0) bsum[(long)blockIdx.y * nblk + blockIdx.x] = s;
}
// in-place exclusive scan of n values per image (block b), total -> total_out[b]
__global__ __launch_bounds__(RG_SCAN) void rg_scan_small(int32_t* __restrict__ vals, int32_t* __restrict__ total_out, int n,
                                                         int stride, int total_stride) {
    int run;
    scan::scan_small<int, RG_SCAN>(vals + (long)blockIdx.x * stride, n, &run);
    if (threadIdx.x == 0 && total_out) total_out[(long)blockIdx.x * total_stride] = run;
}
// flags -> exclusive prefix, in place
__global__ __launch_bounds__(RG_SCAN) void rg_scan_apply(int32_t* __restrict__ flags, const int32_t* __restrict__ bsum, long HW,
                                                         int nblk) {
    int32_t* f = flags + (long)blockIdx.y * HW;
    scan::scan_apply<int, RG_SCAN>([f](long p) { return f[p]; }, [f](long p, int x) { f[p] = x; },
                                   bsum[(long)blockIdx.y * nblk + blockIdx.x], HW);
}
__global__ void rg_relabel_kernel(const int* __restrict__ parent, const int32_t* __restrict__ newid, int32_t* __restrict__ labels,
                                  long HW, int B) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * HW) return;
    const long b = idx / HW;
    const int r = parent[idx];
    labels[idx] = r < 0 ? 0 : newid[b * HW + r] + 1;
}
// one pass of remove_small_regions: pixels of a component of the pass smaller than min_size take the other value
__global__ void rg_small_apply_kernel(const uint8_t* __restrict__ in, const int* __restrict__ parent,
                                      const int32_t* __restrict__ area, uint8_t* __restrict__ out, long HW, int B, int min_size,
                                      int value) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * HW) return;
    const long b = idx / HW;
    const int r = parent[idx];
    uint8_t v = in[idx] != 0 ? 1 : 0;
    if (r >= 0 && area[b * HW + r] < min_size) v = value ? 0 : 1;
    out[idx] = v;
}

// ---------------------------------------------------------------------------------------------------- morphology
__device__ __forceinline__ int reflect_idx(int i, int n) {          // scipy mode 'reflect': (d c b a | a b c d | d c b a)
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - 1 - i;
}
// erosion: min over the footprint cells (j, k) of in[y + j - fh/2][x + k - fw/2]; dilation: max over the mirrored footprint,
// which is the same offsets negated (scipy.ndimage.grey_dilation, also for even sizes)
__global__ __launch_bounds__(256) void rg_morph_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out,
                                                       const uint8_t* __restrict__ fp, int H, int W, int B, int fh, int fw,
                                                       int dilate) {
    __shared__ int offs[RG_MAX_FP];
    __shared__ int noff;
    if (threadIdx.x == 0) noff = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < fh * fw; i += 256)
        if (fp[i]) {
            int dy = i / fw - fh / 2, dx = i % fw - fw / 2;
            if (dilate) { dy = -dy; dx = -dx; }
            offs[atomicAdd(&noff, 1)] = (int)(((unsigned)dy << 16) | ((unsigned)dx & 0xffffu));          // (min / max: the order of the cells does not matter)
        }
    __syncthreads();
    const long HW = (long)H * W;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= B * HW) return;
    const long b = idx / HW;
    const int p = (int)(idx - b * HW);
    const int y = p / W, x = p - y * W;
    const uint8_t* src = in + b * HW;
    const int n = noff;
    int acc = dilate ? 0 : 1;
    for (int o = 0; o < n; ++o) {
        const int w = offs[o];                              // wave-uniform address: a broadcast
        const int yy = reflect_idx(y + (w >> 16), H), xx = reflect_idx(x + (int)(short)(w & 0xffff), W);
        const int v = src[(long)yy * W + xx] != 0;
        acc = dilate ? (acc | v) : (acc & v);
    }
    out[idx] = (uint8_t)acc;
}

// ---------------------------------------------------------------------------------------------------- contingency table
// eight consecutive pixels per thread: equal (s, g) pairs in a row (the usual case inside an object) are added once
__global__ void rg_contingency_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ G, int32_t* __restrict__ table,
                                      int32_t* __restrict__ status, int HW, int nS, int nG) {
    const int b = blockIdx.y;
    const long p0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (p0 >= HW) return;
    const int32_t* s = S + (long)b * HW;
    const int32_t* g = G + (long)b * HW;
    int32_t* t = table + (long)b * (nS + 1) * (nG + 1);
    const int p1 = (int)min((long)HW, p0 + 8);
    int key = -1, run = 0, bad = 0;
    for (int p = (int)p0; p < p1; ++p) {
        const int a = s[p], c = g[p];
        if (a < 0 || a > nS || c < 0 || c > nG) { bad = 1; continue; }
        const int k = a * (nG + 1) + c;
        if (k == key) ++run;
        else {
            if (run) atomicAdd(&t[key], run);
            key = k;
            run = 1;
        }
    }
    if (run) atomicAdd(&t[key], run);
    if (bad) atomicOr(&status[b], 1);
}

// ---------------------------------------------------------------------------------------------------- label sort
// key = label, or -1 unless the pixel has a 4-neighbour outside its object or outside the image
__global__ void rg_boundary_key_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ key, int H, int W, int B) {
    const long HW = (long)H * W;
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * HW) return;
    const long b = idx / HW;
    const int p = (int)(idx - b * HW);
    const int y = p / W, x = p - y * W;
    const int32_t* lab = labels + b * HW;
    const int l = lab[p];
    bool edge = x == 0 || y == 0 || x == W - 1 || y == H - 1;
    if (!edge) edge = lab[p - 1] != l || lab[p + 1] != l || lab[p - W] != l || lab[p + W] != l;
    key[idx] = (edge && l > 0) ? l : -1;
}
// per chunk of RG_CHUNK pixels: histogram of the keys in [0, L]  -> hist[b][chunk][L + 1]; status |= 1 for a key > L
__global__ __launch_bounds__(256) void rg_hist_kernel(const int32_t* __restrict__ key, int32_t* __restrict__ hist,
                                                      int32_t* __restrict__ status, int HW, int L, int nchunk) {
    extern __shared__ int32_t lh[];
    const int b = blockIdx.y, g = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i <= L; i += 256) lh[i] = 0;
    __syncthreads();
    const int p0 = g * RG_CHUNK, p1 = min(HW, p0 + RG_CHUNK);
    int bad = 0;
    for (int q = p0 + tid; q < p1; q += 256) {
        const int l = key[(long)b * HW + q];
        if (l > L) bad = 1;
        else if (l >= 0) atomicAdd(&lh[l], 1);
    }
    if (bad) atomicOr(&status[b], 1);
    __syncthreads();
    int32_t* oh = hist + ((long)b * nchunk + g) * (L + 1);
    for (int i = tid; i <= L; i += 256) oh[i] = lh[i];
}
// per label: exclusive scan over the chunks (in place), total -> start[b][l]
__global__ void rg_chunk_scan_kernel(int32_t* __restrict__ hist, int32_t* __restrict__ start, int L, int nchunk) {
    const int b = blockIdx.y;
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > L) return;
    int32_t* h = hist + (long)b * nchunk * (L + 1) + l;
    int run = 0;
    for (int g = 0; g < nchunk; ++g) {
        const int v = h[(long)g * (L + 1)];
        h[(long)g * (L + 1)] = run;
        run += v;
    }
    start[(long)b * (L + 2) + l] = run;
}
// stable placement, one wave per chunk (the form of sp_place_kernel in superpixel.hip): a cursor per label in LDS, the lanes of
// equal label rank themselves with ballots
__global__ __launch_bounds__(64) void rg_place_kernel(const int32_t* __restrict__ key, const int32_t* __restrict__ chunk_base,
                                                      const int32_t* __restrict__ start, int HW, int L, int nchunk,
                                                      int32_t* __restrict__ pix) {
    extern __shared__ int32_t cur[];
    const int b = blockIdx.y, g = blockIdx.x, lane = threadIdx.x;
    const int32_t* base = chunk_base + ((long)b * nchunk + g) * (L + 1);
    const int32_t* st = start + (long)b * (L + 2);
    for (int i = lane; i <= L; i += 64) cur[i] = st[i] + base[i];
    __syncthreads();
    const int p0 = g * RG_CHUNK, p1 = min(HW, p0 + RG_CHUNK);
    for (int s = p0; s < p1; s += 64) {
        const int p = s + lane;
        int l = (p < p1) ? key[(long)b * HW + p] : -1;
        if (l > L) l = -1;
        unsigned long long rem = __ballot(l >= 0);
        int pos = -1;
        while (rem) {
            const int leader = __ffsll((long long)rem) - 1;
            const int ll = __shfl(l, leader);
            const unsigned long long m = __ballot(l == ll);
            const int c0 = cur[ll];
            if (l == ll) pos = c0 + __popcll(m & ((1ull << lane) - 1ull));
            __syncthreads();
            if (lane == leader) cur[ll] = c0 + __popcll(m);
            __syncthreads();
            rem &= ~m;
        }
        if (l >= 0 && pos >= 0 && pos < HW) pix[(long)b * HW + pos] = p;
    }
}

// ---------------------------------------------------------------------------------------------------- directed Hausdorff
// d2[pair] = max over the pixels p of object a (map X) of min over the pixels q of object b (map Y) of |p - q|^2.  A pixel of a
// that lies in b contributes 0; for every other pixel the nearest pixel of b is a boundary pixel of b (walk from q towards p: the
// last pixel inside b on that path has a 4-neighbour outside b and is not farther), so the minimum runs over b's boundary list
// only.  One block per (pair, chunk of a's pixels); b's boundary is staged in LDS as y << 16 | x and read at a wave-uniform address.
// Exact prune between the LDS passes: when no running minimum of the block exceeds the pair's current maximum, the block cannot
// raise it.
__global__ __launch_bounds__(RG_HD_BLOCK) void rg_hausdorff_kernel(const int32_t* __restrict__ pairs,
                                                                   const int32_t* __restrict__ startA,
                                                                   const int32_t* __restrict__ pixA,
                                                                   const int32_t* __restrict__ labelsB,
                                                                   const int32_t* __restrict__ bstartB,
                                                                   const int32_t* __restrict__ bpixB, int32_t* __restrict__ d2,
                                                                   int W, int HW, int LA, int LB) {
    __shared__ unsigned bq[RG_HD_TILE];
    __shared__ int wmax[RG_HD_BLOCK / 64];
    const int pair = blockIdx.x, tid = threadIdx.x;
    const int a = pairs[2 * pair], b = pairs[2 * pair + 1];
    if (a < 1 || a > LA || b < 1 || b > LB) {
        if (blockIdx.y == 0 && tid == 0) d2[pair] = -1;
        return;
    }
    const int a0 = startA[a], a1 = min(startA[a + 1], HW);
    const int c0 = a0 + blockIdx.y * (RG_HD_BLOCK * RG_HD_PIX);
    if (c0 >= a1) return;
    const int b0 = max(bstartB[b], 0), b1 = min(bstartB[b + 1], HW);
    int py[RG_HD_PIX], px[RG_HD_PIX], best[RG_HD_PIX];
#pragma unroll
    for (int k = 0; k < RG_HD_PIX; ++k) {
        const int i = c0 + k * RG_HD_BLOCK + tid;
        py[k] = px[k] = 0;
        best[k] = 0;                                        // (no pixel, or a pixel inside b: contributes 0)
        if (i < a1) {
            const int p = pixA[i];
            if ((unsigned)p < (unsigned)HW) {
                py[k] = p / W;
                px[k] = p - py[k] * W;
                if (labelsB[p] != b) best[k] = 0x7fffffff;
            }
        }
    }
    for (int t0 = b0; t0 < b1; t0 += RG_HD_TILE) {
        const int n = min(RG_HD_TILE, b1 - t0);
        __syncthreads();
        for (int i = tid; i < n; i += RG_HD_BLOCK) {
            const int q = bpixB[t0 + i];
            const int qy = q / W;
            bq[i] = ((unsigned)qy << 16) | (unsigned)(q - qy * W);
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const unsigned q = bq[i];
            const int qy = (int)(q >> 16), qx = (int)(q & 0xffffu);
#pragma unroll
            for (int k = 0; k < RG_HD_PIX; ++k) {
                const int dy = py[k] - qy, dx = px[k] - qx;
                best[k] = min(best[k], dy * dy + dx * dx);
            }
        }
        if (t0 + RG_HD_TILE < b1) {
            int m = 0;
#pragma unroll
            for (int k = 0; k < RG_HD_PIX; ++k) m = max(m, best[k]);
            const int cur = g_load(&d2[pair]);
            if (!__syncthreads_or(m > cur)) return;
        }
    }
    int m = 0;
#pragma unroll
    for (int k = 0; k < RG_HD_PIX; ++k) m = max(m, best[k]);
    if (b1 <= b0) m = 0;                                    // (an object without pixels: nothing to measure against)
    for (int off = 32; off > 0; off >>= 1) m = max(m, __shfl_xor(m, off));
    if ((tid & 63) == 0) wmax[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < RG_HD_BLOCK / 64; ++i) m = max(m, wmax[i]);
        if (m > 0) atomicMax(&d2[pair], m);
    }
}

inline bool bad_image(int B, int H, int W) {
    return B <= 0 || B > 65535 || H <= 0 || W <= 0 || (long)H * W >= (1l << 30) || (long)B * H * W >= (1l << 40) ||
           ceil_div(H, RG_TILE) > 65535;
}

// tile + border: parent[] holds a forest of every image's components of the pass
int label_roots(const uint8_t* mask, int* parent, int B, int H, int W, int conn8, int value, hipStream_t st) {
    const long tot = (long)B * H * W;
    WESUP_LAUNCH(rg_tile_kernel, dim3(ceil_div(W, RG_TILE), ceil_div(H, RG_TILE), B), dim3(256), 0, st, mask, parent, H, W, conn8,
                 value);
    WESUP_LAUNCH(rg_border_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, parent, H, W, B, conn8);
    return WESUP_OK;
}

}  // namespace

extern "C" size_t wesup_cc_label_workspace_bytes(int B, int H, int W) {
    if (bad_image(B, H, W)) return 0;
    const size_t HW = (size_t)H * W, nblk = (HW + RG_SCAN - 1) / RG_SCAN;
    return 2 * align_up(B * HW * 4, 256) + align_up(B * nblk * 4, 256);        // parent, root flags / new ids, block sums
}

extern "C" int wesup_cc_label(const uint8_t* mask, int32_t* labels, int32_t* n_labels, int B, int H, int W, int connectivity,
                              int value, void* ws, size_t ws_bytes, void* stream) {
    if (!mask || !labels || !n_labels || !ws || bad_image(B, H, W) || (connectivity != 4 && connectivity != 8))
        return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_cc_label_workspace_bytes(B, H, W)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W, tot = (long)B * HW;
    const int nblk = (int)((HW + RG_SCAN - 1) / RG_SCAN);
    const size_t plane = align_up((size_t)tot * 4, 256);
    char* w = (char*)ws;
    int* parent = (int*)w;        w += plane;
    int32_t* flags = (int32_t*)w; w += plane;
    int32_t* bsum = (int32_t*)w;
    const unsigned pb = (unsigned)((tot + 255) / 256);
    label_roots(mask, parent, B, H, W, connectivity == 8, value != 0, st);
    WESUP_LAUNCH(rg_flatten_kernel, dim3(pb), dim3(256), 0, st, parent, flags, (int32_t*)nullptr, HW, B);
    WESUP_LAUNCH(rg_scan_block_sums, dim3(nblk, B), dim3(RG_SCAN), 0, st, flags, bsum, HW, nblk);
    WESUP_LAUNCH(rg_scan_small, dim3(B), dim3(RG_SCAN), 0, st, bsum, n_labels, nblk, nblk, 1);
    WESUP_LAUNCH(rg_scan_apply, dim3(nblk, B), dim3(RG_SCAN), 0, st, flags, bsum, HW, nblk);
    WESUP_LAUNCH(rg_relabel_kernel, dim3(pb), dim3(256), 0, st, parent, flags, labels, HW, B);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_remove_small_regions_workspace_bytes(int B, int H, int W) {
    if (bad_image(B, H, W)) return 0;
    return 2 * align_up((size_t)B * H * W * 4, 256);                            // parent, area per root
}

extern "C" int wesup_remove_small_regions(const uint8_t* mask, uint8_t* out, int B, int H, int W, int min_size, void* ws,
                                          size_t ws_bytes, void* stream) {
    if (!mask || !out || !ws || bad_image(B, H, W) || min_size < 0) return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_remove_small_regions_workspace_bytes(B, H, W)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W, tot = (long)B * HW;
    int* parent = (int*)ws;
    int32_t* area = (int32_t*)((char*)ws + align_up((size_t)tot * 4, 256));
    const unsigned pb = (unsigned)((tot + 255) / 256);
    for (int pass = 0; pass < 2; ++pass) {                  // erase small foreground regions, then fill small holes of the result
        const uint8_t* src = pass == 0 ? mask : out;
        const int value = pass == 0 ? 1 : 0;
        if (wesup_fill_words_(area, 0u, (size_t)tot, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
        label_roots(src, parent, B, H, W, 1, value, st);
        WESUP_LAUNCH(rg_flatten_kernel, dim3(pb), dim3(256), 0, st, parent, (int32_t*)nullptr, area, HW, B);
        WESUP_LAUNCH(rg_small_apply_kernel, dim3(pb), dim3(256), 0, st, src, parent, area, out, HW, B, min_size, value);
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_binary_morph_workspace_bytes(int B, int H, int W, int op) {
    if (bad_image(B, H, W) || op < 0 || op > 2) return 0;
    return op == 2 ? align_up((size_t)B * H * W, 256) : 256;                    // the eroded map of an opening
}

extern "C" int wesup_binary_morph(const uint8_t* mask, uint8_t* out, const uint8_t* footprint, int B, int H, int W, int fh, int fw,
                                  int op, void* ws, size_t ws_bytes, void* stream) {
    if (!mask || !out || !footprint || mask == out || bad_image(B, H, W) || fh <= 0 || fw <= 0 || fh > 255 || fw > 255 ||
        (long)fh * fw > RG_MAX_FP || op < 0 || op > 2)
        return WESUP_ERR_INVALID;
    if (op == 2 && !ws) return WESUP_ERR_INVALID;
    if (op == 2 && ws_bytes < wesup_binary_morph_workspace_bytes(B, H, W, op)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long tot = (long)B * H * W;
    const unsigned pb = (unsigned)((tot + 255) / 256);
    if (op == 2) {
        uint8_t* tmp = (uint8_t*)ws;
        WESUP_LAUNCH(rg_morph_kernel, dim3(pb), dim3(256), 0, st, mask, tmp, footprint, H, W, B, fh, fw, 0);
        WESUP_LAUNCH(rg_morph_kernel, dim3(pb), dim3(256), 0, st, (const uint8_t*)tmp, out, footprint, H, W, B, fh, fw, 1);
    } else {
        WESUP_LAUNCH(rg_morph_kernel, dim3(pb), dim3(256), 0, st, mask, out, footprint, H, W, B, fh, fw, op);
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_contingency(const int32_t* S, const int32_t* G, int32_t* table, int32_t* status, int B, int HW, int nS, int nG,
                                 void* stream) {
    if (!S || !G || !table || !status || B <= 0 || B > 65535 || HW <= 0 || nS < 0 || nG < 0 ||
        ((long)nS + 1) * ((long)nG + 1) > (1l << 26))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (wesup_fill_words_(table, 0u, (size_t)B * (nS + 1) * (nG + 1), st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (wesup_fill_words_(status, 0u, (size_t)B, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    WESUP_LAUNCH(rg_contingency_kernel, dim3(ceil_div(ceil_div(HW, 8), 256), B), dim3(256), 0, st, S, G, table, status, HW, nS, nG);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_label_sort_workspace_bytes(int B, int H, int W, int L) {
    if (bad_image(B, H, W) || L < 0 || L >= RG_MAX_LABELS) return 0;
    const size_t HW = (size_t)H * W, nchunk = (HW + RG_CHUNK - 1) / RG_CHUNK;
    return align_up(B * HW * 4, 256) + align_up(B * nchunk * (L + 1) * 4, 256);   // boundary keys, chunk histograms
}

// start / bstart [B][L + 2]: the pixels of label l are pix[start[l] .. start[l + 1]); bpix holds the boundary pixels of the
// labels >= 1 the same way (entries past bstart[L + 1] are not written)
extern "C" int wesup_label_sort(const int32_t* labels, int32_t* start, int32_t* pix, int32_t* bstart, int32_t* bpix,
                                int32_t* status, int B, int H, int W, int L, void* ws, size_t ws_bytes, void* stream) {
    if (!labels || !start || !pix || !bstart || !bpix || !status || !ws || bad_image(B, H, W) || L < 0 || L >= RG_MAX_LABELS)
        return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_label_sort_workspace_bytes(B, H, W, L)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    const long tot = (long)B * HW;
    const int nchunk = ceil_div(HW, RG_CHUNK);
    int32_t* bkey = (int32_t*)ws;
    int32_t* hist = (int32_t*)((char*)ws + align_up((size_t)tot * 4, 256));
    const size_t lds = (size_t)(L + 1) * 4;
    if (wesup_fill_words_(status, 0u, (size_t)B, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    WESUP_LAUNCH(rg_boundary_key_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, labels, bkey, H, W, B);
    for (int pass = 0; pass < 2; ++pass) {
        const int32_t* key = pass == 0 ? labels : bkey;
        int32_t* s = pass == 0 ? start : bstart;
        int32_t* o = pass == 0 ? pix : bpix;
        WESUP_LAUNCH(rg_hist_kernel, dim3(nchunk, B), dim3(256), lds, st, key, hist, status, HW, L, nchunk);
        WESUP_LAUNCH(rg_chunk_scan_kernel, dim3(ceil_div(L + 1, 256), B), dim3(256), 0, st, hist, s, L, nchunk);
        WESUP_LAUNCH(rg_scan_small, dim3(B), dim3(RG_SCAN), 0, st, s, s + (L + 1), L + 1, L + 2, L + 2);
        WESUP_LAUNCH(rg_place_kernel, dim3(nchunk, B), dim3(64), lds, st, key, (const int32_t*)hist, (const int32_t*)s, HW, L,
                     nchunk, o);
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

// one image pair: the pixel lists of map X (start / pix of wesup_label_sort), the label map of Y and its boundary lists
extern "C" int wesup_directed_hausdorff_sq(const int32_t* pairs, const int32_t* start_x, const int32_t* pix_x,
                                           const int32_t* labels_y, const int32_t* bstart_y, const int32_t* bpix_y, int32_t* d2,
                                           int P, int H, int W, int LX, int LY, void* stream) {
    if (!pairs || !start_x || !pix_x || !labels_y || !bstart_y || !bpix_y || !d2 || P < 0 || H <= 0 || W <= 0 || H > 32767 ||
        W > 32767 || (long)H * W > 65535l * (RG_HD_BLOCK * RG_HD_PIX) || LX < 0 || LY < 0)
        return WESUP_ERR_INVALID;
    if (P == 0) return WESUP_OK;
    hipStream_t st = (hipStream_t)stream;
    const int HW = H * W;
    if (wesup_fill_words_(d2, 0u, (size_t)P, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    WESUP_LAUNCH(rg_hausdorff_kernel, dim3(P, ceil_div(HW, RG_HD_BLOCK * RG_HD_PIX)), dim3(RG_HD_BLOCK), 0, st, pairs, start_x,
                 pix_x, labels_y, bstart_y, bpix_y, d2, W, HW, LX, LY);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
