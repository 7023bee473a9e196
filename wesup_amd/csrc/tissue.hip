// Tissue selection for whole-slide evaluation: which patches of slide.hip's lattice are worth a forward pass.
// One read of the resident uint8 slide gives a 256-bin histogram of a pixel value per patch (tis_hist_kernel, the hot path); the
// rest works on those histograms: their sum, Otsu's threshold over it, the tissue pixels of every patch (a prefix or suffix sum of
// its histogram) and the ordered list of the patches kept.  The host statement of every step is wesup_amd/slide.py
// (pixel_value, patch_histograms, otsu_threshold, select_patches); the kernels equal it bit for bit.  Integers throughout -- adds
// in LDS and global memory in any order give the same cells -- except the six fp64 operations of an Otsu score, done by one
// thread per threshold in a fixed order without contraction.  No workspace, no host sync.
#include "common.hpp"
#include "lattice.hpp"

#define TIS_BLOCK 256
#define TIS_WAVES (TIS_BLOCK / 64)
#define TIS_COPIES (2 * TIS_WAVES)   // LDS histograms per block: one per wave and lane parity
#define TIS_MAX_BLOCKS WESUP_TISSUE_MAX_BLOCKS
#define TIS_ITEM_PIXELS WESUP_TISSUE_ITEM_PIXELS
static_assert(WESUP_TISSUE_LIST_CHUNK == TIS_BLOCK, "the compaction walks the patches one block of threads at a time");

namespace {

// the pixel value of DESIGN.md 3.19: CH 0 luma (77 R + 150 G + 29 B + 128) >> 8, CH 1 chroma max - min; 0 .. 255 either way
template <int CH>
__device__ __forceinline__ unsigned tis_value(unsigned r, unsigned g, unsigned b) {
    if (CH == 0) return (77u * r + 150u * g + 29u * b + 128u) >> 8;
    return max(r, max(g, b)) - min(r, min(g, b));
}

// One value per lane (negative: none) into the wave's LDS histogram.  Glass puts every lane on one bin, where 64 LDS adds to
// one address run one after the other: the lanes that hold the first lane's value are counted by a ballot and added by one lane;
// only the others add for themselves (noise: nearly all of them, spread over the bins and the two parity copies).
// Every lane of the wave calls this (ballot, shuffle).
__device__ __forceinline__ void tis_add(unsigned* mine, unsigned* even, int v, int lane) {
    const unsigned long long have = __ballot(v >= 0);
    if (have == 0ull) return;
    const int lead = __ffsll((long long)have) - 1;
    const int f = __shfl(v, lead, 64);
    const unsigned long long same = __ballot(v == f);
    if (lane == lead) atomicAdd(&even[f], (unsigned)__popcll(same));
    else if (v >= 0 && v != f) atomicAdd(&mine[v], 1u);
}

// bytes o .. o + 3 of the image as a little-endian word, o a multiple of 4 on a 4-byte aligned base; bytes at nb and beyond
// read as 0 and are never addressed
__device__ __forceinline__ unsigned tis_word(const uint8_t* __restrict__ img, long o, long nb) {
    if (o + 4 <= nb) return *reinterpret_cast<const unsigned*>(img + o);
    unsigned v = 0;
    for (int i = 0; i < 4; ++i)
        if (o + i < nb) v |= (unsigned)img[o + i] << (8 * i);
    return v;
}

// hist[k][v] += 1 for every slide pixel of patch k.  An item is `rows` rows of one patch (about TIS_ITEM_PIXELS pixels: a
// 1000-pixel patch is 125 items, the 3 x 3 lattice of a 3000 x 2600 slide about a thousand); the blocks stride over the items.
// Inside an item a thread takes four neighbouring pixels of a row, 12 bytes.  A row starts at any byte (W * 3 is any number), so
// on a 4-byte aligned image (ALIGNED) the thread reads the four aligned words that cover them and shifts the pixels out
// (v_alignbit); the fourth word is the neighbour's first and comes from the cache.  Otherwise it reads the 12 bytes one by one.
// No word or byte outside [0, 3 H W) is addressed.  A block counts into TIS_COPIES histograms in LDS and adds their non-zero cells
// to the patch's row of hist after every item: an item has at most rows * p <= max(TIS_ITEM_PIXELS, p) < 2^32 pixels.
template <int CH, bool ALIGNED>
__global__ __launch_bounds__(TIS_BLOCK) void tis_hist_kernel(const uint8_t* __restrict__ img, unsigned* __restrict__ hist, int H, int W,
                                                           int n_w, int p, int rows, int chunks, long items) {
    __shared__ unsigned lds[TIS_COPIES][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned* even = lds[2 * wave];
    unsigned* mine = lds[2 * wave + (lane & 1)];
    for (int c = 0; c < TIS_COPIES; ++c) lds[c][tid] = 0u;
    __syncthreads();
    const long nb = (long)H * W * 3;
    for (long item = blockIdx.x; item < items; item += gridDim.x) {
        const int k = (int)(item / chunks), chunk = (int)(item - (long)k * chunks);
        const int ky = k / n_w, kx = k - ky * n_w;
        const long y0 = (long)ky * p + (long)chunk * rows, x0 = (long)kx * p;
        const long yp = min((long)ky * p + p, (long)H);                       // the patch's rows end here
        const int nr = (int)max(0l, min(y0 + rows, yp) - y0);                // rows of this item inside the slide
        const int nx = (int)(min(x0 + p, (long)W) - x0);                     // pixels of a row, >= 1
        const int quads = (nx + 3) >> 2;
        const long work = (long)nr * quads;
        for (long base = 0; base < work; base += TIS_BLOCK) {                 // (the same trip count for every lane of a wave)
            const long idx = base + tid;
            int left = 0;                                                    // pixels of this thread: 0 .. 4
            unsigned u0 = 0, u1 = 0, u2 = 0;                                 // their 12 bytes
            if (idx < work) {
                const int r = (int)(idx / quads), q = (int)(idx - (long)r * quads);
                left = min(4, nx - 4 * q);
                const long b0 = ((y0 + r) * W + x0 + 4 * q) * 3;             // first byte
                if (ALIGNED) {
                    const long a0 = b0 & ~3l;
                    const unsigned sh = 8u * (unsigned)(b0 - a0);
                    const long end = b0 + 3 * left;                          // one past the last byte wanted
                    const unsigned w0 = tis_word(img, a0, nb), w1 = a0 + 4 < end ? tis_word(img, a0 + 4, nb) : 0u;
                    const unsigned w2 = a0 + 8 < end ? tis_word(img, a0 + 8, nb) : 0u;
                    const unsigned w3 = a0 + 12 < end ? tis_word(img, a0 + 12, nb) : 0u;
                    u0 = __funnelshift_r(w0, w1, sh);
                    u1 = __funnelshift_r(w1, w2, sh);
                    u2 = __funnelshift_r(w2, w3, sh);
                } else {
                    const int nbytes = 3 * left;
                    for (int i = 0; i < 12; ++i) {
                        const unsigned byte = i < nbytes ? (unsigned)img[b0 + i] : 0u;
                        if (i < 4) u0 |= byte << (8 * i);
                        else if (i < 8) u1 |= byte << (8 * (i - 4));
                        else u2 |= byte << (8 * (i - 8));
                    }
                }
            }
            const int v0 = (int)tis_value<CH>(u0 & 255u, (u0 >> 8) & 255u, (u0 >> 16) & 255u);
            const int v1 = (int)tis_value<CH>(u0 >> 24, u1 & 255u, (u1 >> 8) & 255u);
            const int v2 = (int)tis_value<CH>((u1 >> 16) & 255u, u1 >> 24, u2 & 255u);
            const int v3 = (int)tis_value<CH>((u2 >> 8) & 255u, (u2 >> 16) & 255u, u2 >> 24);
            tis_add(mine, even, left > 0 ? v0 : -1, lane);
            tis_add(mine, even, left > 1 ? v1 : -1, lane);
            tis_add(mine, even, left > 2 ? v2 : -1, lane);
            tis_add(mine, even, left > 3 ? v3 : -1, lane);
        }
        __syncthreads();
        unsigned sum = 0;
        for (int c = 0; c < TIS_COPIES; ++c) {
            sum += lds[c][tid];
            lds[c][tid] = 0u;
        }
        if (sum) atomicAdd(&hist[(long)k * 256 + tid], sum);
        __syncthreads();
    }
}

// total[v] += sum over a block's patches of hist[k][v]: thread = bin, one 64-bit integer add per bin and block
__global__ __launch_bounds__(TIS_BLOCK) void tis_total_kernel(const unsigned* __restrict__ hist, unsigned long long* __restrict__ total,
                                                            int n) {
    unsigned long long s = 0;
    for (int k = blockIdx.x; k < n; k += gridDim.x) s += hist[(long)k * 256 + threadIdx.x];
    if (s) atomicAdd(&total[threadIdx.x], s);
}

// info = {t, n_keep (tis_list_kernel's), n, flat, 0, 0, 0, 0}.  threshold >= 0: t is given.  Otherwise Otsu over total, as
// slide.otsu_threshold states it: thread t scores threshold t; w0, s0, N, S, D = w0 (N - w0) are integers below 2^64 (the entry
// bounds N = H W by 2^32), num = |S w0 - s0 N| is formed exactly in 128 bits, and q = x * x / (double)D with
// x = (double)hi * 2^64 + (double)lo takes six fp64 operations, each rounded once (__dmul_rn and its kin are never contracted).
// Thread 0 then walks t = 0 .. 254 upwards and keeps the first largest q under a strict >; no t with D > 0: t = -1, a flat slide.
__global__ __launch_bounds__(256) void tis_threshold_kernel(const unsigned long long* __restrict__ total, int32_t* __restrict__ info,
                                                           int threshold, int n) {
    __shared__ unsigned long long h[256];
    __shared__ double q[256];
    __shared__ int ok[256];
    const int t = threadIdx.x;
    if (t >= 4 && t < 8) info[t] = 0;
    if (t == 2) info[2] = n;
    if (threshold >= 0) {
        if (t == 0) info[0] = threshold;
        if (t == 3) info[3] = 0;
        return;
    }
    h[t] = total[t];
    __syncthreads();
    unsigned long long N = 0, S = 0, w0 = 0, s0 = 0;
    for (int i = 0; i < 256; ++i) {
        const unsigned long long c = h[i];
        N += c;
        S += (unsigned long long)i * c;
        if (i <= t) {
            w0 += c;
            s0 += (unsigned long long)i * c;
        }
    }
    const unsigned long long D = w0 * (N - w0);
    ok[t] = (t < 255 && D != 0ull) ? 1 : 0;
    double score = 0.0;
    if (ok[t]) {
        const unsigned long long alo = S * w0, ahi = __umul64hi(S, w0), blo = s0 * N, bhi = __umul64hi(s0, N);
        const bool a_ge = ahi > bhi || (ahi == bhi && alo >= blo);
        const unsigned long long xl = a_ge ? alo : blo, xh = a_ge ? ahi : bhi, yl = a_ge ? blo : alo, yh = a_ge ? bhi : ahi;
        const unsigned long long lo = xl - yl, hi = xh - yh - (xl < yl ? 1ull : 0ull);        // subtract with a borrow
        const double x = __dadd_rn(__dmul_rn((double)hi, 18446744073709551616.0), (double)lo);
        score = __ddiv_rn(__dmul_rn(x, x), (double)D);
    }
    q[t] = score;
    __syncthreads();
    if (t == 0) {
        int best = -1;
        double bq = 0.0;
        for (int i = 0; i < 255; ++i)
            if (ok[i] && (best < 0 || q[i] > bq)) {
                best = i;
                bq = q[i];
            }
        info[0] = best;
        info[3] = best < 0 ? 1 : 0;
    }
}

// tissue: luma v <= t, chroma v > t, t = -1 every pixel
template <int CH>
__device__ __forceinline__ bool tis_tissue(int v, int t) {
    return t < 0 || (CH == 0 ? v <= t : v > t);
}

// counts[k] = the tissue pixels of patch k: the bins of hist[k] on the tissue side of t.  One wave per patch.
template <int CH>
__global__ __launch_bounds__(TIS_BLOCK) void tis_counts_kernel(const unsigned* __restrict__ hist, const int32_t* __restrict__ info,
                                                             unsigned* __restrict__ counts, int n) {
    const int t = info[0];
    const int lane = threadIdx.x & 63;
    for (long k = (long)blockIdx.x * TIS_WAVES + (threadIdx.x >> 6); k < n; k += (long)gridDim.x * TIS_WAVES) {
        unsigned s = 0;
        for (int v = lane; v < 256; v += 64)
            if (tis_tissue<CH>(v, t)) s += hist[k * 256 + v];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) counts[k] = s;
    }
}

// list[0 .. n_keep) = the kept patches in ascending order, info[1] = n_keep.  Kept: counts[k] >= 1 and
// counts[k] * 10^6 >= min_ppm * area_k, area_k the patch's pixels inside the slide (a flat slide counts every pixel: all kept).
// One block walks the patches TIS_BLOCK at a time: a ballot and a popcount rank a kept patch inside its wave, the waves' totals
// inside the chunk, `base` carries the count over the chunk edges.  list beyond n_keep is left as it is.
__global__ __launch_bounds__(TIS_BLOCK) void tis_list_kernel(const unsigned* __restrict__ counts, int32_t* __restrict__ info,
                                                           int32_t* __restrict__ list, int H, int W, int n_w, int p, int min_ppm,
                                                           int n) {
    __shared__ int wave_kept[TIS_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (long start = 0; start < n; start += TIS_BLOCK) {
        const long k = start + threadIdx.x;
        bool keep = false;
        if (k < n) {
            const int ky = (int)(k / n_w), kx = (int)(k - (long)ky * n_w);
            const long ah = min((long)ky * p + p, (long)H) - (long)ky * p, aw = min((long)kx * p + p, (long)W) - (long)kx * p;
            const unsigned long long c = counts[k];
            keep = c >= 1ull && c * 1000000ull >= (unsigned long long)min_ppm * (unsigned long long)(ah * aw);
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(m);
        __syncthreads();
        int before = base, all = 0;
        for (int wv = 0; wv < TIS_WAVES; ++wv) {
            if (wv < wave) before += wave_kept[wv];
            all += wave_kept[wv];
        }
        if (keep) list[before + __popcll(m & ((1ull << lane) - 1ull))] = (int32_t)k;
        base += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) info[1] = base;
}

// out[Y][X] = 255 where the pixel is tissue under info[0], else 0
template <int CH>
__global__ __launch_bounds__(TIS_BLOCK) void tis_mask_kernel(const uint8_t* __restrict__ img, const int32_t* __restrict__ info,
                                                           uint8_t* __restrict__ out, long n) {
    const int t = info[0];
    for (long i = (long)blockIdx.x * TIS_BLOCK + threadIdx.x; i < n; i += (long)gridDim.x * TIS_BLOCK) {
        const uint8_t* px = img + 3 * i;
        out[i] = tis_tissue<CH>((int)tis_value<CH>(px[0], px[1], px[2]), t) ? 255 : 0;
    }
}

// the lattice of the tissue entries: slide.hip's, a patch of at most 65535 (a cell of hist is a uint32) and at most 2^32 pixels
// (Otsu's D = w0 (N - w0) stays below 2^64)
inline bool tis_lattice(int H, int W, int p, int* n_w, int* last) {
    return sd_lattice(H, W, p, n_w, last) && p <= 65535 && (long)H * W <= (1l << 32);
}

}  // namespace

extern "C" int wesup_patch_value_hist(const uint8_t* img, uint32_t* hist, int H, int W, int p, int channel, void* stream) {
    int n_w = 0, last = 0;
    if (!img || !hist || (channel != 0 && channel != 1) || !tis_lattice(H, W, p, &n_w, &last) || (((uintptr_t)hist) & 3))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)last + 1;
    if (wesup_fill_words_(hist, 0u, (size_t)n * 256, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    const int rows = TIS_ITEM_PIXELS / p > 1 ? TIS_ITEM_PIXELS / p : 1;
    const int chunks = (p + rows - 1) / rows;
    const long items = n * chunks;
    const dim3 grid((unsigned)(items > TIS_MAX_BLOCKS ? TIS_MAX_BLOCKS : items)), block(TIS_BLOCK);
    const bool aligned = (((uintptr_t)img) & 3) == 0;
#define TIS_L(CH, AL) WESUP_LAUNCH((tis_hist_kernel<CH, AL>), grid, block, 0, st, img, hist, H, W, n_w, p, rows, chunks, items)
    if (channel == 0) {
        if (aligned) TIS_L(0, true);
        else TIS_L(0, false);
    } else {
        if (aligned) TIS_L(1, true);
        else TIS_L(1, false);
    }
#undef TIS_L
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_tissue_select(const uint32_t* hist, int H, int W, int p, int channel, int threshold, int min_ppm, int32_t* info,
                                   int64_t* total, uint32_t* counts, int32_t* list, void* stream) {
    int n_w = 0, last = 0;
    if (!hist || !info || !total || !counts || !list || (channel != 0 && channel != 1) || threshold < -1 || threshold > 254 ||
        min_ppm < 0 || min_ppm > 1000000 || !tis_lattice(H, W, p, &n_w, &last) || (((uintptr_t)total) & 7))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const int n = last + 1;
    if (wesup_fill_words_(total, 0u, 512, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    WESUP_LAUNCH(tis_total_kernel, dim3(grid_stride_blocks((n + 15) / 16, 1, 256)), dim3(TIS_BLOCK), 0, st, hist,
                 reinterpret_cast<unsigned long long*>(total), n);
    WESUP_LAUNCH(tis_threshold_kernel, dim3(1), dim3(256), 0, st, reinterpret_cast<const unsigned long long*>(total), info, threshold, n);
    const dim3 cgrid(grid_stride_blocks(n, TIS_WAVES, TIS_MAX_BLOCKS)), block(TIS_BLOCK);
    if (channel == 0) WESUP_LAUNCH(tis_counts_kernel<0>, cgrid, block, 0, st, hist, (const int32_t*)info, counts, n);
    else WESUP_LAUNCH(tis_counts_kernel<1>, cgrid, block, 0, st, hist, (const int32_t*)info, counts, n);
    WESUP_LAUNCH(tis_list_kernel, dim3(1), block, 0, st, (const unsigned*)counts, info, list, H, W, n_w, p, min_ppm, n);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_tissue_mask_u8(const uint8_t* img, const int32_t* info, uint8_t* out, int H, int W, int channel, void* stream) {
    if (!img || !info || !out || H <= 0 || W <= 0 || H > (1 << 30) || W > (1 << 30) || (channel != 0 && channel != 1))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long n = (long)H * W;
    const dim3 grid(grid_stride_blocks(n, TIS_BLOCK, TIS_MAX_BLOCKS)), block(TIS_BLOCK);
    if (channel == 0) WESUP_LAUNCH(tis_mask_kernel<0>, grid, block, 0, st, img, info, out, n);
    else WESUP_LAUNCH(tis_mask_kernel<1>, grid, block, 0, st, img, info, out, n);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
