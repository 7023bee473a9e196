// Painted object comparisons (reference scripts/paint_masks.py): which ground-truth object a predicted object
// takes its colour from, decided over the contingency table of the two labelled maps (regions.hip), and the palette paint of a
// label map.  Integer arithmetic on integer data: the results are held to the host functions of wesup_amd/paint.py exactly
// (tests/test_paint_gpu.py).
//
// Matching: ground-truth object g is a candidate for predicted object p when p covers more than half of it, 2 * C[p][g] > area[g]
// with area[g] the sum of column g; p takes the candidate of the largest area, the lowest g among equal areas, and
// max(nS, nG) + p when it has none.
//   1. pm_colsum_kernel  area[g] (64-bit) = sum over the image's rows of column g: a thread per column (coalesced across a row), a
//                        chunk of rows per block, one integer atomic per (chunk, column);
//   2. pm_match_kernel   one wave per row: the lanes scan the columns 64 apart, each keeps its best (area, g), and a butterfly of
//                        shuffles reduces the 64 pairs under the same order.
// Painting: four consecutive pixels per thread -- one 16-byte load of labels, 12 bytes of interleaved RGB as three whole words.
// The groups are cut on the FLAT pixel index of the batch, so that a group's bytes start on a word whatever H * W is; a group that
// straddles two images (or the end) is written byte by byte, each image's block writing its own pixels only.
#include "common.hpp"

#define PM_ROWS 64             // rows of the table per block of the column sums
#define PM_LUT_LDS 2048        // colour tables up to this many entries are staged in LDS (8 KB), longer ones read from memory
#define PM_MAX_BLOCKS 2048     // per image: the rest of the groups by grid stride (the staging is paid once per block)

namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void pm_colsum_kernel(const int32_t* __restrict__ table, const int32_t* __restrict__ nS_dev,
                                                        const int32_t* __restrict__ nG_dev, u64* __restrict__ area, int nS,
                                                        int nG, int colblk) {
    const int b = blockIdx.y;
    const int chunk = blockIdx.x / colblk;
    const int g = (blockIdx.x - chunk * colblk) * 256 + threadIdx.x;
    const int rows = min(max(nS_dev[b], 0), nS) + 1, cols = min(max(nG_dev[b], 0), nG) + 1;
    const int r0 = chunk * PM_ROWS, r1 = min(r0 + PM_ROWS, rows);
    if (g >= cols || r0 >= r1) return;
    const int32_t* t = table + (long)b * (nS + 1) * (nG + 1) + g;
    u64 s = 0;
    for (int r = r0; r < r1; ++r) s += (u64)(unsigned)max(t[(long)r * (nG + 1)], 0);
    if (s) atomicAdd(&area[(long)b * (nG + 1) + g], s);
}

__global__ __launch_bounds__(256) void pm_match_kernel(const int32_t* __restrict__ table, const int32_t* __restrict__ nS_dev,
                                                       const int32_t* __restrict__ nG_dev, const u64* __restrict__ area,
                                                       int32_t* __restrict__ match, int nS, int nG) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int p = blockIdx.x * 4 + (threadIdx.x >> 6);                   // wave-uniform
    if (p > nS) return;
    const int rows = min(max(nS_dev[b], 0), nS), cols = min(max(nG_dev[b], 0), nG);
    int32_t* out = match + (long)b * (nS + 1);
    if (p == 0 || p > rows) {
        if (lane == 0) out[p] = 0;
        return;
    }
    const int32_t* row = table + ((long)b * (nS + 1) + p) * (nG + 1);
    const u64* ar = area + (long)b * (nG + 1);
    u64 best_a = 0;
    int best_g = 0;                                                      // 0: no candidate (a candidate has area >= 1)
    for (int g = 1 + lane; g <= cols; g += 64) {
        const u64 c = (u64)(unsigned)max(row[g], 0), a = ar[g];
        if (2 * c > a && a > best_a) {                                   // ascending g per lane: > keeps the lowest g of equal areas
            best_a = a;
            best_g = g;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const u64 oa = __shfl_xor(best_a, off);
        const int og = __shfl_xor(best_g, off);
        if (og != 0 && (best_g == 0 || oa > best_a || (oa == best_a && og < best_g))) {
            best_a = oa;
            best_g = og;
        }
    }
    if (lane == 0) out[p] = best_g != 0 ? best_g : max(rows, cols) + p;
}

// STAGED: the image's colour table sits in LDS (n_lut * 4 bytes), otherwise it is read from memory
template <bool STAGED>
__device__ __forceinline__ unsigned pm_colour(int l, const unsigned* __restrict__ lut, const unsigned* lut_s, int n_lut, int& bad) {
    if ((unsigned)l >= (unsigned)n_lut) {                                // never an index: the pixel is black
        bad = 1;
        return 0u;
    }
    return (STAGED ? lut_s[l] : lut[l]) & 0xffffffu;
}

template <bool VEC, bool STAGED>
__global__ __launch_bounds__(256) void pm_paint_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ lut_all,
                                                       uint8_t* __restrict__ out, int32_t* __restrict__ status, int HW_, int n_lut) {
    extern __shared__ unsigned lut_s[];
    const int b = blockIdx.y;
    const long HW = HW_;
    const unsigned* lut = reinterpret_cast<const unsigned*>(lut_all) + (long)b * n_lut;
    if (STAGED) {
        for (int i = threadIdx.x; i < n_lut; i += 256) lut_s[i] = lut[i];
        __syncthreads();
    }
    const long n_lo = (long)b * HW, n_hi = n_lo + HW;                    // the image's flat pixels
    const long k_hi = (n_hi + 3) >> 2;                                   // groups k cover the flat pixels 4k .. 4k + 3
    int bad = 0;
    for (long k = (n_lo >> 2) + (long)blockIdx.x * 256 + threadIdx.x; k < k_hi; k += (long)gridDim.x * 256) {
        const long n0 = k * 4;
        if (VEC && n0 >= n_lo && n0 + 4 <= n_hi) {
            const int4 l = *reinterpret_cast<const int4*>(labels + n0);
            const unsigned c0 = pm_colour<STAGED>(l.x, lut, lut_s, n_lut, bad);
            const unsigned c1 = pm_colour<STAGED>(l.y, lut, lut_s, n_lut, bad);
            const unsigned c2 = pm_colour<STAGED>(l.z, lut, lut_s, n_lut, bad);
            const unsigned c3 = pm_colour<STAGED>(l.w, lut, lut_s, n_lut, bad);
            uint3 w;                                                     // r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
            w.x = c0 | (c1 << 24);
            w.y = (c1 >> 8) | (c2 << 16);
            w.z = (c2 >> 16) | (c3 << 8);
            *reinterpret_cast<uint3*>(out + n0 * 3) = w;
        } else {
            const long q0 = max(n0, n_lo), q1 = min(n0 + 4, n_hi);
            for (long q = q0; q < q1; ++q) {
                const unsigned c = pm_colour<STAGED>(labels[q], lut, lut_s, n_lut, bad);
                out[q * 3] = (uint8_t)c;
                out[q * 3 + 1] = (uint8_t)(c >> 8);
                out[q * 3 + 2] = (uint8_t)(c >> 16);
            }
        }
    }
    if (bad) atomicOr(&status[b], 1);
}

inline bool bad_table(int B, int nS, int nG) {
    return B <= 0 || B > 65535 || nS < 0 || nG < 0 || ((long)nS + 1) * ((long)nG + 1) > (1l << 26) ||
           (long)B * ((long)nS + 1) * ((long)nG + 1) >= (1l << 40);
}

}  // namespace

extern "C" size_t wesup_object_match_workspace_bytes(int B, int nG) {
    if (B <= 0 || B > 65535 || nG < 0 || nG >= (1 << 26)) return 0;
    return align_up((size_t)B * ((size_t)nG + 1) * 8, 256);                     // the column sums
}

extern "C" int wesup_object_match(const int32_t* table, const int32_t* nS_dev, const int32_t* nG_dev, int32_t* match, int B,
                                  int nS, int nG, void* ws, size_t ws_bytes, void* stream) {
    if (!table || !nS_dev || !nG_dev || !match || !ws || bad_table(B, nS, nG)) return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_object_match_workspace_bytes(B, nG)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    u64* area = (u64*)ws;
    if (wesup_fill_words_(area, 0u, (size_t)B * (nG + 1) * 2, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    // (chunks of rows) x (blocks of columns) flattened into grid.x: either factor alone can pass 65535, the product stays below 2^21
    const int chunks = ceil_div(nS + 1, PM_ROWS), colblk = ceil_div(nG + 1, 256);
    WESUP_LAUNCH(pm_colsum_kernel, dim3(chunks * colblk, B), dim3(256), 0, st, table, nS_dev, nG_dev, area, nS, nG, colblk);
    WESUP_LAUNCH(pm_match_kernel, dim3(ceil_div(nS + 1, 4), B), dim3(256), 0, st, table, nS_dev, nG_dev, (const u64*)area, match,
                 nS, nG);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_label_paint(const int32_t* labels, const int32_t* lut, uint8_t* out, int32_t* status, int B, int HW,
                                 int n_lut, void* stream) {
    if (!labels || !lut || !out || !status || B <= 0 || B > 65535 || HW <= 0 || HW >= (1 << 30) || n_lut <= 0 ||
        n_lut > (1 << 26))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (wesup_fill_words_(status, 0u, (size_t)B, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    const bool staged = n_lut <= PM_LUT_LDS;
    const size_t lds = staged ? (size_t)n_lut * 4 : 0;
    const unsigned nblk = grid_stride_blocks((HW + 3) / 4 + 1, 256, PM_MAX_BLOCKS);
    const bool vec = ((uintptr_t)labels & 15) == 0 && ((uintptr_t)out & 3) == 0;
    auto kern = vec ? (staged ? pm_paint_kernel<true, true> : pm_paint_kernel<true, false>)
                    : (staged ? pm_paint_kernel<false, true> : pm_paint_kernel<false, false>);
    WESUP_LAUNCH(kern, dim3(nblk, B), dim3(256), lds, st, labels, lut, out, status, HW, n_lut);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
