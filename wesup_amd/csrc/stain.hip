// Macenko stain normalisation and stain jitter of H&E images (Macenko et al., ISBI 2009), and the exact order
// statistics its percentiles need.  fp32 / fp64 VALU only, no matrix instruction, no floating-point atomic: counts are integer
// LDS atomics (exact), every sum has one owner and a fixed order, so two runs give the same bits.  A fit is one chain of
// launches without a host read-back; its result stays in a 64-byte device block per image that the apply pass reads.
//
//   sel_hist_kernel       radix select, one pass of 8 bits from the top: per block a 256-bin histogram of the pass's digit among
//                         the keys that carry a rank's prefix (ranks that still share a prefix share a histogram), written as
//                         one partial row per block.  Keys are the order-preserving uint32 image of the float.
//   sel_pick_kernel       one block: folds the partial rows in block order, a wave per rank scans the 256 bins to the rank's
//                         digit, keeps the prefix and the residual rank in the workspace; the last pass writes the floats.
//   st_moments_kernel     table OD of every sampled pixel, tissue test, count / 3 sums / 6 second moments in fp64 per thread,
//                         wave and block fold, one partial row per block.
//   st_eigen_kernel       one block per image: partial rows in a fixed order, covariance, cyclic Jacobi (fixed sweeps), sign rules,
//                         the ranks of the two angle percentiles.
//   st_phi_kernel         phi = atan2(OD . v1, OD . v0) of every sampled tissue pixel (fp64, rounded once); +inf elsewhere.
//   st_vectors_kernel     interpolated angles, stain vectors, H/E ordering, the 2 x 3 pseudo-inverse, validity.
//   st_conc_kernel        both concentrations of every sampled pixel (fp64 dot of the block's float pinv, rounded once).
//   st_final_kernel       maxC; the block.
//   st_apply_kernel       c = pinv OD;  c' = c (maxC_d / maxC_s) a + b;  OD' = HE_d c' + keep (OD - HE_s c);
//                         v' = rint(clamp(Io exp(-OD') - 1, 0, 255)): four pixels (three aligned dwords) per thread and trip.
#include <math.h>
#include "common.hpp"

#define SEL_BLOCK WESUP_SELECT_BLOCK
#define SEL_MAX_BLOCKS WESUP_SELECT_MAX_BLOCKS
#define SEL_MAX_RANKS WESUP_SELECT_MAX_RANKS
#define ST_MOM 10                       // count, sum r g b, sum rr rg rb gg gb bb
#define ST_MOM_BLOCKS 256               // partial rows per image at most
#define ST_MAP_BLOCKS 2048              // phi / concentration / apply blocks per image at most
#define ST_JACOBI_SWEEPS 12
#define ST_PARALLEL_DET 1e-6            // |det(HE^T HE)| = sin^2 of the angle between the stain vectors
#define ST_MIN_MAXC 1e-6
#define ST_MAX_SAMPLES (1L << 24)       // n_tissue travels as a float

namespace {

// ---------------------------------------------------------------- radix select
struct SelState {                       // per array of a batch, in the workspace
    long rank[SEL_MAX_RANKS];           // residual rank among the keys that carry the prefix
    unsigned prefix[SEL_MAX_RANKS];     // the bits fixed so far, in place (low bits 0)
    int alias[SEL_MAX_RANKS];           // the first rank with the same prefix: the owner of the histogram
    long pad_[2];
};
static_assert(sizeof(SelState) == 80, "SelState layout");
#define SEL_STATE_BYTES 256

__device__ __forceinline__ unsigned sel_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// pass p looks at bits [24 - 8 p, 32 - 8 p).  grid (blocks, batch).
__global__ __launch_bounds__(SEL_BLOCK) void sel_hist_kernel(const float* __restrict__ keys, long key_stride, long n, int n_ranks,
                                                             int pass, const SelState* __restrict__ state, long state_stride,
                                                             unsigned* __restrict__ partial, long partial_stride) {
    __shared__ unsigned hist[SEL_MAX_RANKS][256];
    __shared__ unsigned s_prefix[SEL_MAX_RANKS];
    __shared__ int s_owner[SEL_MAX_RANKS];
    const int b = blockIdx.y;
    keys += (size_t)b * key_stride;
    const SelState* st = (const SelState*)((const char*)state + (size_t)b * state_stride);
    for (int t = threadIdx.x; t < SEL_MAX_RANKS * 256; t += SEL_BLOCK) (&hist[0][0])[t] = 0u;
    if (threadIdx.x < SEL_MAX_RANKS) {
        const int r = threadIdx.x;
        // pass 0: nothing fixed yet, every rank reads histogram 0
        s_prefix[r] = pass == 0 ? 0u : st->prefix[r];
        s_owner[r] = r < n_ranks && (pass == 0 ? r == 0 : st->alias[r] == r);
    }
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const unsigned himask = pass == 0 ? 0u : ~((1u << (shift + 8)) - 1u);
    unsigned pre[SEL_MAX_RANKS];
    int own[SEL_MAX_RANKS];
    // runs of one digit (the top byte of angles in a narrow range) are counted in a register and flushed when the digit changes
    int last[SEL_MAX_RANKS];
    unsigned cnt[SEL_MAX_RANKS];
#pragma unroll
    for (int r = 0; r < SEL_MAX_RANKS; ++r) { pre[r] = s_prefix[r]; own[r] = s_owner[r]; last[r] = -1; cnt[r] = 0u; }
    auto count = [&](float f) {
        const unsigned k = sel_key(f);
        const int digit = (int)((k >> shift) & 255u);
#pragma unroll
        for (int r = 0; r < SEL_MAX_RANKS; ++r) {
            if (own[r] && (k & himask) == pre[r]) {
                if (digit == last[r]) ++cnt[r];
                else {
                    if (cnt[r]) atomicAdd(&hist[r][last[r]], cnt[r]);
                    last[r] = digit;
                    cnt[r] = 1u;
                }
            }
        }
    };
    const long stride = (long)gridDim.x * SEL_BLOCK;
    long i = (long)blockIdx.x * SEL_BLOCK + threadIdx.x;
    for (; i + 3 * stride < n; i += 4 * stride) {                          // four loads in flight
        const float f0 = keys[i], f1 = keys[i + stride], f2 = keys[i + 2 * stride], f3 = keys[i + 3 * stride];
        count(f0); count(f1); count(f2); count(f3);
    }
    for (; i < n; i += stride) count(keys[i]);
#pragma unroll
    for (int r = 0; r < SEL_MAX_RANKS; ++r)
        if (cnt[r]) atomicAdd(&hist[r][last[r]], cnt[r]);
    __syncthreads();
    unsigned* row = partial + (size_t)b * partial_stride + (size_t)blockIdx.x * (SEL_MAX_RANKS * 256);
    for (int t = threadIdx.x; t < SEL_MAX_RANKS * 256; t += SEL_BLOCK) row[t] = (&hist[0][0])[t];
}

// grid (1, batch), 4 * 256 threads: the partial rows of every histogram in use are added per bin, then a wave per rank picks.
__global__ __launch_bounds__(SEL_MAX_RANKS * 256) void sel_pick_kernel(long n, const long* __restrict__ ranks, long rank_stride,
                                                                        int n_ranks, int pass, int blocks, SelState* __restrict__ state,
                                                                        long state_stride, const unsigned* __restrict__ partial,
                                                                        long partial_stride, float* __restrict__ out, long out_stride) {
    __shared__ unsigned long long total[SEL_MAX_RANKS][256], quarter[4][256];
    __shared__ int s_owner[SEL_MAX_RANKS];
    __shared__ unsigned s_prefix[SEL_MAX_RANKS];
    const int b = blockIdx.y;
    SelState* st = (SelState*)((char*)state + (size_t)b * state_stride);
    const int r = threadIdx.x >> 8, d = threadIdx.x & 255;
    if (threadIdx.x < SEL_MAX_RANKS) s_owner[threadIdx.x] = pass == 0 ? 0 : st->alias[threadIdx.x];
    __syncthreads();
    // every owner's histogram in turn: the quarter r of the threads adds the rows r, r + 4, ... of bin d, sixteen loads in flight
    // (one thread per bin over all rows waits for 256 loads one after the other: 60 us), then the four quarters are added
    for (int o = 0; o < n_ranks; ++o) {
        if (s_owner[o] != o) continue;
        const unsigned* col = partial + (size_t)b * partial_stride + (size_t)o * 256 + d;
        unsigned long long sum = 0;
        int k = r;
        for (; k + 60 < blocks; k += 64) {
            unsigned v[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) v[j] = col[(size_t)(k + 4 * j) * (SEL_MAX_RANKS * 256)];
#pragma unroll
            for (int j = 0; j < 16; ++j) sum += v[j];
        }
        for (; k < blocks; k += 4) sum += col[(size_t)k * (SEL_MAX_RANKS * 256)];
        quarter[r][d] = sum;
        __syncthreads();
        if (r == 0) total[o][d] = (quarter[0][d] + quarter[1][d]) + (quarter[2][d] + quarter[3][d]);
        __syncthreads();
    }
    // rank q is settled by the first wave of its 256 threads: lane l owns bins 4 l .. 4 l + 3, a shuffle scan gives the count below
    // its bins, the one lane whose bins straddle the rank walks them
    const int q = r, lane = threadIdx.x & 255;
    if (q < n_ranks && lane < 64) {
        long rank;
        unsigned prefix;
        if (pass == 0) {
            rank = ranks[(size_t)b * rank_stride + q];
            rank = rank < 0 ? 0 : (rank > n - 1 ? n - 1 : rank);            // a rank outside the array is taken to its end
            prefix = 0u;
        } else {
            rank = st->rank[q];
            prefix = st->prefix[q];
        }
        const unsigned long long* h = total[s_owner[q]] + 4 * lane;
        const unsigned long long mine = h[0] + h[1] + h[2] + h[3];
        unsigned long long incl = mine;
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long up = __shfl_up(incl, off);
            if (lane >= off) incl += up;
        }
        unsigned long long below = incl - mine;
        // (the counts under a prefix sum to the keys that carry it, so a lane always takes the rank; the last lane takes it anyway)
        const bool take = (below <= (unsigned long long)rank && (unsigned long long)rank < incl) ||
                          (lane == 63 && (unsigned long long)rank >= incl);
        if (take) {
            int e = 0;
            for (; e < 3; ++e) {
                if (below + h[e] > (unsigned long long)rank) break;
                below += h[e];
            }
            prefix |= (unsigned)(4 * lane + e) << (24 - 8 * pass);
            st->rank[q] = rank - (long)below;
            st->prefix[q] = prefix;
            s_prefix[q] = prefix;
            if (pass == 3) out[(size_t)b * out_stride + q] = sel_unkey(prefix);
        }
    }
    __syncthreads();
    if (threadIdx.x < n_ranks) {                                            // owners for the next pass
        const int me = threadIdx.x;
        int a = me;
        for (int e = 0; e < me; ++e)
            if (s_prefix[e] == s_prefix[me]) { a = e; break; }
        st->alias[me] = a;
    }
}

inline unsigned sel_blocks(long n) { return grid_stride_blocks(n, SEL_BLOCK, SEL_MAX_BLOCKS); }
inline size_t sel_ws_bytes(long n, int batch) {
    return (size_t)batch * (SEL_STATE_BYTES + (size_t)sel_blocks(n) * SEL_MAX_RANKS * 256 * sizeof(unsigned));
}

// `batch` arrays of n keys each, `n_ranks` ranks each; ws holds sel_ws_bytes(n, batch).  Eight launches.
void sel_launch(const float* keys, long key_stride, long n, const long* ranks, long rank_stride, int n_ranks, float* out,
                long out_stride, int batch, void* ws, hipStream_t st) {
    const unsigned blocks = sel_blocks(n);
    SelState* state = (SelState*)ws;
    unsigned* partial = (unsigned*)((char*)ws + (size_t)batch * SEL_STATE_BYTES);
    const long pstride = (long)blocks * SEL_MAX_RANKS * 256;
    for (int pass = 0; pass < 4; ++pass) {
        WESUP_LAUNCH(sel_hist_kernel, dim3(blocks, batch), dim3(SEL_BLOCK), 0, st, keys, key_stride, n, n_ranks, pass,
                     (const SelState*)state, (long)SEL_STATE_BYTES, partial, pstride);
        WESUP_LAUNCH(sel_pick_kernel, dim3(1, batch), dim3(SEL_MAX_RANKS * 256), 0, st, n, ranks, rank_stride, n_ranks, pass,
                     (int)blocks, state, (long)SEL_STATE_BYTES, (const unsigned*)partial, pstride, out, out_stride);
    }
}

// ---------------------------------------------------------------- the fit
struct StainScratch {                   // per image, in the workspace (ops.stain_fit(return_stages=True) reads eig)
    double eig[6];                      // V[c][k]: the two leading eigenvectors of the tissue OD covariance, as columns
    double frac[3];                     // interpolation weights: phi_lo, phi_hi, maxC
    double he[6];                       // HE[c][k] as the block's floats
    double n_tissue;
    long ranks_phi[4];                  // lo, lo + 1, hi, hi + 1
    long ranks_c[2];
    float sel_phi[4];
    float sel_c[4];                     // [k][2]
    float pinv[6];                      // pinv[k][c] as in the block
    int valid;
    int pad_;
};
static_assert(sizeof(StainScratch) == 16 * 8 + 6 * 8 + 8 * 4 + 6 * 4 + 8, "StainScratch layout");
#define ST_SCRATCH_BYTES 256
static_assert(sizeof(StainScratch) <= ST_SCRATCH_BYTES, "StainScratch fits its slot");

struct StainGeom {
    int H, W, stride, hs, ws;           // hs x ws sampled rows and columns
    int pad_;
    long ns;                            // hs * ws
};
static_assert(sizeof(StainGeom) == 32, "StainGeom has no padding");

__device__ __forceinline__ void od_table(float* T, float io) {
    // a uint8 channel has 256 values: OD = -log((v + 1) / Io), in double, rounded once
    for (int v = threadIdx.x; v < 256; v += blockDim.x) T[v] = (float)(-log((double)(v + 1) / (double)io));
    __syncthreads();
}

__device__ __forceinline__ const uint8_t* sample_ptr(const uint8_t* img, const StainGeom& g, int b, long s) {
    const unsigned y = (unsigned)s / (unsigned)g.ws, x = (unsigned)s - y * (unsigned)g.ws;      // s < 2^24: a 32-bit division
    return img + ((size_t)b * g.H * g.W + (size_t)y * g.stride * g.W + (size_t)x * g.stride) * 3;
}

__global__ __launch_bounds__(256) void st_moments_kernel(const uint8_t* __restrict__ img, double* __restrict__ partial, StainGeom g,
                                                         float io, float beta) {
    __shared__ float T[256];
    __shared__ double red[4][ST_MOM];
    od_table(T, io);
    const int b = blockIdx.y;
    double m[ST_MOM];
#pragma unroll
    for (int j = 0; j < ST_MOM; ++j) m[j] = 0.0;
    auto add = [&](unsigned pr, unsigned pg, unsigned pb) {
        const float fr = T[pr], fg = T[pg], fb = T[pb];
        if (fr >= beta && fg >= beta && fb >= beta) {
            const double r = fr, gg = fg, bb = fb;
            m[0] += 1.0; m[1] += r; m[2] += gg; m[3] += bb;
            m[4] += r * r; m[5] += r * gg; m[6] += r * bb; m[7] += gg * gg; m[8] += gg * bb; m[9] += bb * bb;
        }
    };
    const long step = (long)gridDim.x * 256;
    long s = (long)blockIdx.x * 256 + threadIdx.x;
    for (; s + 3 * step < g.ns; s += 4 * step) {                           // four samples in flight, added in the order of the plain loop
        const uint8_t *p0 = sample_ptr(img, g, b, s), *p1 = sample_ptr(img, g, b, s + step), *p2 = sample_ptr(img, g, b, s + 2 * step),
                      *p3 = sample_ptr(img, g, b, s + 3 * step);
        const unsigned v[12] = {p0[0], p0[1], p0[2], p1[0], p1[1], p1[2], p2[0], p2[1], p2[2], p3[0], p3[1], p3[2]};
        add(v[0], v[1], v[2]); add(v[3], v[4], v[5]); add(v[6], v[7], v[8]); add(v[9], v[10], v[11]);
    }
    for (; s < g.ns; s += step) {
        const uint8_t* p = sample_ptr(img, g, b, s);
        add(p[0], p[1], p[2]);
    }
#pragma unroll
    for (int j = 0; j < ST_MOM; ++j) {
        double v = m[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = v;
    }
    __syncthreads();
    if (threadIdx.x < ST_MOM) {
        const int j = threadIdx.x;
        partial[((size_t)b * gridDim.x + blockIdx.x) * ST_MOM + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    }
}

__device__ void jacobi3(double a[3][3], double v[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < ST_JACOBI_SWEEPS; ++sweep) {
        for (int p = 0; p < 2; ++p) {
            for (int q = p + 1; q < 3; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {                            // A <- A J
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq;
                    a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {                            // A <- J^T A
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk;
                    a[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq;
                    v[k][q] = s * vkp + c * vkq;
                }
            }
        }
    }
}

__device__ __forceinline__ void percentile_ranks(double q, long n, long* lo, long* hi, double* frac) {
    const double pos = q * (double)(n - 1) / 100.0;
    const double f = floor(pos);
    long l = (long)f;
    if (l < 0) l = 0;
    if (l > n - 1) l = n - 1;
    *lo = l;
    *hi = l + 1 > n - 1 ? n - 1 : l + 1;
    *frac = pos - f;
}

// grid (B), 64 threads
__global__ __launch_bounds__(64) void st_eigen_kernel(const double* __restrict__ partial, int mom_blocks, double* __restrict__ moments,
                                                      char* __restrict__ scratch, long ns, float alpha, int min_tissue) {
    __shared__ double mom[ST_MOM];
    const int b = blockIdx.x;
    // the partial rows in a fixed order: lane l adds rows l, l + 64, ..., then the lanes fold pairwise
    for (int j = 0; j < ST_MOM; ++j) {
        double s = 0.0;
        for (int k = threadIdx.x; k < mom_blocks; k += 64) s += partial[((size_t)b * mom_blocks + k) * ST_MOM + j];
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
        if (threadIdx.x == 0) {
            mom[j] = s;
            moments[(size_t)b * ST_MOM + j] = s;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    StainScratch* sc = (StainScratch*)(scratch + (size_t)b * ST_SCRATCH_BYTES);
    const double n = mom[0];
    double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    int i0 = 0, i1 = 1;
    const int enough = n >= (double)min_tissue;
    if (enough) {
        const double mean[3] = {mom[1] / n, mom[2] / n, mom[3] / n};
        const double s2[3][3] = {{mom[4], mom[5], mom[6]}, {mom[5], mom[7], mom[8]}, {mom[6], mom[8], mom[9]}};
        double a[3][3];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) a[i][j] = (s2[i][j] - n * mean[i] * mean[j]) / (n - 1.0);
        jacobi3(a, v);
        const double e[3] = {a[0][0], a[1][1], a[2][2]};
        // the two largest eigenvalues, the larger first (ties: the lower index first)
        i0 = 0;
        for (int i = 1; i < 3; ++i) if (e[i] > e[i0]) i0 = i;
        i1 = i0 == 0 ? 1 : 0;
        for (int i = 0; i < 3; ++i) if (i != i0 && e[i] > e[i1]) i1 = i;
    }
    double c0[3] = {v[0][i0], v[1][i0], v[2][i0]}, c1[3] = {v[0][i1], v[1][i1], v[2][i1]};
    if (c0[0] + c0[1] + c0[2] < 0.0) { c0[0] = -c0[0]; c0[1] = -c0[1]; c0[2] = -c0[2]; }
    int big = 0;                                                            // the second: its largest component positive
    for (int i = 1; i < 3; ++i) if (fabs(c1[i]) > fabs(c1[big])) big = i;
    if (c1[big] < 0.0) { c1[0] = -c1[0]; c1[1] = -c1[1]; c1[2] = -c1[2]; }
    for (int c = 0; c < 3; ++c) { sc->eig[2 * c] = c0[c]; sc->eig[2 * c + 1] = c1[c]; }
    sc->n_tissue = n;
    sc->valid = enough;
    const long nt = n < 1.0 ? 1 : (long)n;
    percentile_ranks((double)alpha, nt, &sc->ranks_phi[0], &sc->ranks_phi[1], &sc->frac[0]);
    percentile_ranks(100.0 - (double)alpha, nt, &sc->ranks_phi[2], &sc->ranks_phi[3], &sc->frac[1]);
    percentile_ranks(99.0, ns, &sc->ranks_c[0], &sc->ranks_c[1], &sc->frac[2]);
}

__global__ __launch_bounds__(256) void st_phi_kernel(const uint8_t* __restrict__ img, const char* __restrict__ scratch,
                                                     float* __restrict__ phi, StainGeom g, float io, float beta) {
    __shared__ float T[256];
    od_table(T, io);
    const int b = blockIdx.y;
    const StainScratch* sc = (const StainScratch*)(scratch + (size_t)b * ST_SCRATCH_BYTES);
    const double v00 = sc->eig[0], v01 = sc->eig[1], v10 = sc->eig[2], v11 = sc->eig[3], v20 = sc->eig[4], v21 = sc->eig[5];
    float* out = phi + (size_t)b * g.ns;
    const long step = (long)gridDim.x * 256;
    for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < g.ns; s += step) {
        const uint8_t* p = sample_ptr(img, g, b, s);
        const float fr = T[p[0]], fg = T[p[1]], fb = T[p[2]];
        float key = __uint_as_float(0x7f800000u);                           // not tissue: after every angle
        if (fr >= beta && fg >= beta && fb >= beta) {
            const double t0 = (double)fr * v00 + (double)fg * v10 + (double)fb * v20;
            const double t1 = (double)fr * v01 + (double)fg * v11 + (double)fb * v21;
            key = (float)atan2(t1, t0);
        }
        out[s] = key;
    }
}

// grid (B), 64 threads
__global__ __launch_bounds__(64) void st_vectors_kernel(char* __restrict__ scratch) {
    if (threadIdx.x != 0) return;
    StainScratch* sc = (StainScratch*)(scratch + (size_t)blockIdx.x * ST_SCRATCH_BYTES);
    const double lo = (double)sc->sel_phi[0] + ((double)sc->sel_phi[1] - (double)sc->sel_phi[0]) * sc->frac[0];
    const double hi = (double)sc->sel_phi[2] + ((double)sc->sel_phi[3] - (double)sc->sel_phi[2]) * sc->frac[1];
    int valid = sc->valid && isfinite(lo) && isfinite(hi);
    double a[3], c[3];
    if (valid) {
        const double cl = cos(lo), sl = sin(lo), ch = cos(hi), sh = sin(hi);
        for (int k = 0; k < 3; ++k) {
            a[k] = sc->eig[2 * k] * cl + sc->eig[2 * k + 1] * sl;
            c[k] = sc->eig[2 * k] * ch + sc->eig[2 * k + 1] * sh;
        }
    } else {
        for (int k = 0; k < 3; ++k) a[k] = c[k] = 0.0;
    }
    // the larger red component is H
    const int swap = !(a[0] > c[0]);
    double he[6];
    for (int k = 0; k < 3; ++k) {
        he[2 * k] = (double)(float)(swap ? c[k] : a[k]);
        he[2 * k + 1] = (double)(float)(swap ? a[k] : c[k]);
    }
    // pinv = (HE^T HE)^-1 HE^T of the ROUNDED vectors: what the block says is what the concentrations are made with
    double g00 = 0, g01 = 0, g11 = 0;
    for (int k = 0; k < 3; ++k) { g00 += he[2 * k] * he[2 * k]; g01 += he[2 * k] * he[2 * k + 1]; g11 += he[2 * k + 1] * he[2 * k + 1]; }
    const double det = g00 * g11 - g01 * g01;
    valid = valid && fabs(det) >= ST_PARALLEL_DET;
    for (int k = 0; k < 3; ++k) {
        sc->he[2 * k] = valid ? he[2 * k] : 0.0;
        sc->he[2 * k + 1] = valid ? he[2 * k + 1] : 0.0;
        sc->pinv[k] = valid ? (float)((g11 * he[2 * k] - g01 * he[2 * k + 1]) / det) : 0.f;
        sc->pinv[3 + k] = valid ? (float)((g00 * he[2 * k + 1] - g01 * he[2 * k]) / det) : 0.f;
    }
    sc->valid = valid;
}

__global__ __launch_bounds__(256) void st_conc_kernel(const uint8_t* __restrict__ img, const char* __restrict__ scratch,
                                                      float* __restrict__ conc, StainGeom g, float io) {
    __shared__ float T[256];
    od_table(T, io);
    const int b = blockIdx.y;
    const StainScratch* sc = (const StainScratch*)(scratch + (size_t)b * ST_SCRATCH_BYTES);
    double pv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) pv[k] = (double)sc->pinv[k];
    float* c0 = conc + (size_t)b * 2 * g.ns;
    float* c1 = c0 + g.ns;
    const long step = (long)gridDim.x * 256;
    for (long s = (long)blockIdx.x * 256 + threadIdx.x; s < g.ns; s += step) {
        const uint8_t* p = sample_ptr(img, g, b, s);
        const double r = T[p[0]], gg = T[p[1]], bb = T[p[2]];
        c0[s] = (float)(pv[0] * r + pv[1] * gg + pv[2] * bb);
        c1[s] = (float)(pv[3] * r + pv[4] * gg + pv[5] * bb);
    }
}

// grid (B), 64 threads
__global__ __launch_bounds__(64) void st_final_kernel(const char* __restrict__ scratch, float* __restrict__ blocks) {
    if (threadIdx.x != 0) return;
    const StainScratch* sc = (const StainScratch*)(scratch + (size_t)blockIdx.x * ST_SCRATCH_BYTES);
    float* blk = blocks + (size_t)blockIdx.x * WESUP_STAIN_BLOCK;
    float maxc[2];
    int valid = sc->valid;
    for (int k = 0; k < 2; ++k) {
        const double lo = sc->sel_c[2 * k], hi = sc->sel_c[2 * k + 1];
        maxc[k] = (float)(lo + (hi - lo) * sc->frac[2]);
        valid = valid && maxc[k] >= (float)ST_MIN_MAXC;                     // (false for a NaN)
    }
    for (int k = 0; k < 6; ++k) {
        blk[k] = valid ? (float)sc->he[k] : 0.f;
        blk[6 + k] = valid ? sc->pinv[k] : 0.f;
    }
    blk[12] = valid ? maxc[0] : 0.f;
    blk[13] = valid ? maxc[1] : 0.f;
    blk[14] = (float)sc->n_tissue;
    blk[15] = valid ? 1.f : 0.f;
}

inline StainGeom make_geom(int H, int W, int stride) {
    StainGeom g;
    g.H = H; g.W = W; g.stride = stride;
    g.hs = (H + stride - 1) / stride;
    g.ws = (W + stride - 1) / stride;
    g.pad_ = 0;
    g.ns = (long)g.hs * g.ws;
    return g;
}

struct FitLayout {
    size_t partial, moments, scratch, phi, conc, sel, total;
    unsigned mom_blocks;
};
inline FitLayout fit_layout(int B, const StainGeom& g) {
    FitLayout L;
    L.mom_blocks = grid_stride_blocks(g.ns, 256, ST_MOM_BLOCKS);
    size_t o = 0;
    L.partial = o; o += align_up((size_t)B * L.mom_blocks * ST_MOM * sizeof(double), 256);
    L.moments = o; o += align_up((size_t)B * ST_MOM * sizeof(double), 256);
    L.scratch = o; o += (size_t)B * ST_SCRATCH_BYTES;
    L.phi = o; o += align_up((size_t)B * g.ns * sizeof(float), 256);
    L.conc = o; o += align_up((size_t)B * 2 * g.ns * sizeof(float), 256);
    L.sel = o; o += sel_ws_bytes(g.ns, B);
    L.total = o;
    return L;
}
inline int fit_shape_ok(int B, int H, int W, int stride) {
    if (B < 1 || H < 1 || W < 1 || stride < 1 || B > 65535) return 0;
    const long hs = (H + (long)stride - 1) / stride, ws = (W + (long)stride - 1) / stride;
    return hs * ws <= ST_MAX_SAMPLES;
}

// ---------------------------------------------------------------- apply
struct ApplyCoef {                      // per image, uniform over a block
    float p[6];                         // pinv_s[k][c]
    float hs[6];                        // HE_s[c][k]
    float hd[6];                        // HE_d[c][k]
    float sa[2], sb[2];                 // c' = c sa + b:  sa = (maxC_d / maxC_s) a
    float keep;
    int valid;
};

__device__ __forceinline__ void apply_pixel(uint8_t& r, uint8_t& g, uint8_t& b, const float* T, const ApplyCoef& k, float io) {
    const float od[3] = {T[r], T[g], T[b]};
    // explicit multiplies and fused multiply-adds: nothing is left to the compiler's contraction, so HE_d c' and HE_s c are the
    // same bits when the operands are (the identity jitter gives the image back)
    const float c0 = fmaf(k.p[2], od[2], fmaf(k.p[1], od[1], __fmul_rn(k.p[0], od[0])));
    const float c1 = fmaf(k.p[5], od[2], fmaf(k.p[4], od[1], __fmul_rn(k.p[3], od[0])));
    const float d0 = fmaf(c0, k.sa[0], k.sb[0]);
    const float d1 = fmaf(c1, k.sa[1], k.sb[1]);
    uint8_t o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float fit = fmaf(k.hs[2 * c + 1], c1, __fmul_rn(k.hs[2 * c], c0));
        const float dst = fmaf(k.hd[2 * c + 1], d1, __fmul_rn(k.hd[2 * c], d0));
        const float odn = fmaf(k.keep, __fsub_rn(od[c], fit), dst);
        float v = fmaf(io, expf(-odn), -1.f);
        v = fminf(fmaxf(v, 0.f), 255.f);
        o[c] = (uint8_t)(int)rintf(v);
    }
    r = o[0]; g = o[1]; b = o[2];
}

struct alignas(4) Pix4 { unsigned w[3]; };     // four pixels: twelve bytes at a 4-byte boundary

// grid (blocks, B), 256 threads.  Image b starts at byte 3 b HW of img / out; `head` pixels in front of the first 4-byte boundary
// that is also a pixel boundary (both buffers share the phase, or everything is head) and the pixels behind the last whole group
// of four go one by one, spread over the grid like the groups.
__global__ __launch_bounds__(256) void st_apply_kernel(const uint8_t* img, uint8_t* out, const float* __restrict__ src_blocks,
                                                       const float* __restrict__ dst_blocks, int dst_stride,
                                                       const float* __restrict__ jitter, float keep, long HW, float io, int wide) {
    __shared__ float T[256];
    od_table(T, io);
    const int b = blockIdx.y;
    const float* sb = src_blocks + (size_t)b * WESUP_STAIN_BLOCK;
    const float* db = dst_blocks + (size_t)b * dst_stride;
    ApplyCoef k;
#pragma unroll
    for (int i = 0; i < 6; ++i) { k.hs[i] = sb[i]; k.p[i] = sb[6 + i]; k.hd[i] = db[i]; }
    k.valid = sb[15] != 0.f && db[15] != 0.f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const float a = jitter ? jitter[(size_t)b * 4 + 2 * i] : 1.f, bb = jitter ? jitter[(size_t)b * 4 + 2 * i + 1] : 0.f;
        const float ratio = k.valid ? db[12 + i] / sb[12 + i] : 1.f;
        k.sa[i] = __fmul_rn(ratio, a);
        k.sb[i] = bb;
    }
    k.keep = keep;
    const uint8_t* in_b = img + (size_t)b * HW * 3;
    uint8_t* out_b = out + (size_t)b * HW * 3;
    long head = wide ? (long)((uintptr_t)in_b & 3) : HW;
    if (head > HW) head = HW;
    const long groups = (HW - head) / 4;
    const long tail0 = head + groups * 4;
    const Pix4* in4 = (const Pix4*)(in_b + head * 3);
    Pix4* out4 = (Pix4*)(out_b + head * 3);
    const long step = (long)gridDim.x * 256;
    for (long gidx = (long)blockIdx.x * 256 + threadIdx.x; gidx < groups; gidx += step) {
        Pix4 q = in4[gidx];
        if (k.valid) {
            uint8_t by[12];
#pragma unroll
            for (int j = 0; j < 12; ++j) by[j] = (uint8_t)(q.w[j >> 2] >> (8 * (j & 3)));
#pragma unroll
            for (int j = 0; j < 4; ++j) apply_pixel(by[3 * j], by[3 * j + 1], by[3 * j + 2], T, k, io);
#pragma unroll
            for (int w = 0; w < 3; ++w)
                q.w[w] = (unsigned)by[4 * w] | ((unsigned)by[4 * w + 1] << 8) | ((unsigned)by[4 * w + 2] << 16) | ((unsigned)by[4 * w + 3] << 24);
        }
        out4[gidx] = q;
    }
    // head and tail, a pixel per thread over the whole grid: at most six pixels on the dword path, the whole image on the byte path
    const long rest = head + (HW - tail0);
    for (long t = (long)blockIdx.x * 256 + threadIdx.x; t < rest; t += step) {
        const long px = t < head ? t : tail0 + (t - head);
        uint8_t r = in_b[3 * px], g = in_b[3 * px + 1], bl = in_b[3 * px + 2];
        if (k.valid) apply_pixel(r, g, bl, T, k, io);
        out_b[3 * px] = r; out_b[3 * px + 1] = g; out_b[3 * px + 2] = bl;
    }
}

}  // namespace

// the select for the other modules of the library (common.hpp; csrc/surface.hip)
size_t wesup_select_workspace_bytes_(long n, int batch) { return sel_ws_bytes(n, batch); }
void wesup_select_launch_(const float* keys, long key_stride, long n, const long* ranks, long rank_stride, int n_ranks, float* out,
                          long out_stride, int batch, void* ws, hipStream_t st) {
    sel_launch(keys, key_stride, n, ranks, rank_stride, n_ranks, out, out_stride, batch, ws, st);
}

// ---------------------------------------------------------------- entries
extern "C" size_t wesup_select_f32_workspace_bytes(long n) {
    if (n < 1) return 0;
    return sel_ws_bytes(n, 1);
}

extern "C" int wesup_select_f32(const float* keys, long n, const long* ranks, int n_ranks, float* out, void* ws, size_t ws_bytes,
                                void* stream) {
    if (!keys || !ranks || !out || !ws || n < 1 || n_ranks < 1 || n_ranks > SEL_MAX_RANKS) return WESUP_ERR_INVALID;
    if (((uintptr_t)keys & 3) || ((uintptr_t)ranks & 7) || ((uintptr_t)out & 3) || ((uintptr_t)ws & 15)) return WESUP_ERR_INVALID;
    if (ws_bytes < sel_ws_bytes(n, 1)) return WESUP_ERR_WORKSPACE;
    sel_launch(keys, n, n, ranks, n_ranks, n_ranks, out, n_ranks, 1, ws, (hipStream_t)stream);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_stain_fit_workspace_bytes(int B, int H, int W, int stride) {
    if (!fit_shape_ok(B, H, W, stride)) return 0;
    return fit_layout(B, make_geom(H, W, stride)).total;
}

extern "C" size_t wesup_stain_fit_stage_offset(int B, int H, int W, int stride, int stage) {
    if (!fit_shape_ok(B, H, W, stride)) return 0;
    const FitLayout L = fit_layout(B, make_geom(H, W, stride));
    switch (stage) {
        case WESUP_STAIN_STAGE_MOMENTS: return L.moments;
        case WESUP_STAIN_STAGE_SCRATCH: return L.scratch;
        case WESUP_STAIN_STAGE_PHI: return L.phi;
        case WESUP_STAIN_STAGE_CONC: return L.conc;
        default: return 0;
    }
}

extern "C" int wesup_stain_fit(const uint8_t* img, float* blocks, int B, int H, int W, int stride, float io, float alpha, float beta,
                               int min_tissue, void* ws, size_t ws_bytes, void* stream) {
    if (!img || !blocks || !ws || !fit_shape_ok(B, H, W, stride)) return WESUP_ERR_INVALID;
    if (!(io > 1.f) || !(alpha >= 0.f && alpha <= 50.f) || !(beta >= 0.f) || min_tissue < 2) return WESUP_ERR_INVALID;
    if (((uintptr_t)blocks & 3) || ((uintptr_t)ws & 15)) return WESUP_ERR_INVALID;
    const StainGeom g = make_geom(H, W, stride);
    const FitLayout L = fit_layout(B, g);
    if (ws_bytes < L.total) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    double* partial = (double*)(base + L.partial);
    double* moments = (double*)(base + L.moments);
    char* scratch = base + L.scratch;
    float* phi = (float*)(base + L.phi);
    float* conc = (float*)(base + L.conc);
    void* sel = base + L.sel;
    const unsigned map_blocks = grid_stride_blocks(g.ns, 256, ST_MAP_BLOCKS);
    const long sstride = ST_SCRATCH_BYTES / 8, fstride = ST_SCRATCH_BYTES / 4;
    WESUP_LAUNCH(st_moments_kernel, dim3(L.mom_blocks, B), dim3(256), 0, st, img, partial, g, io, beta);
    WESUP_LAUNCH(st_eigen_kernel, dim3(B), dim3(64), 0, st, (const double*)partial, (int)L.mom_blocks, moments, scratch, g.ns, alpha,
                 min_tissue);
    WESUP_LAUNCH(st_phi_kernel, dim3(map_blocks, B), dim3(256), 0, st, img, (const char*)scratch, phi, g, io, beta);
    // the two angle percentiles: four ranks of one array per image
    sel_launch(phi, g.ns, g.ns, (const long*)(scratch + offsetof(StainScratch, ranks_phi)), sstride, 4,
               (float*)(scratch + offsetof(StainScratch, sel_phi)), fstride, B, sel, st);
    WESUP_LAUNCH(st_vectors_kernel, dim3(B), dim3(64), 0, st, scratch);
    WESUP_LAUNCH(st_conc_kernel, dim3(map_blocks, B), dim3(256), 0, st, img, (const char*)scratch, conc, g, io);
    // the 99th percentile of both concentrations: per stain a batch of B arrays with the same two ranks
    for (int k = 0; k < 2; ++k)
        sel_launch(conc + (size_t)k * g.ns, 2 * g.ns, g.ns, (const long*)(scratch + offsetof(StainScratch, ranks_c)), sstride, 2,
                   (float*)(scratch + offsetof(StainScratch, sel_c)) + 2 * k, fstride, B, sel, st);
    WESUP_LAUNCH(st_final_kernel, dim3(B), dim3(64), 0, st, (const char*)scratch, blocks);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" int wesup_stain_apply(const uint8_t* img, uint8_t* out, const float* src_blocks, const float* dst_blocks, int dst_stride,
                                 const float* jitter, float keep_residual, int B, int H, int W, float io, void* stream) {
    if (!img || !out || !src_blocks || !dst_blocks || B < 1 || B > 65535 || H < 1 || W < 1) return WESUP_ERR_INVALID;
    if (dst_stride != 0 && dst_stride != WESUP_STAIN_BLOCK) return WESUP_ERR_INVALID;
    if (!(io > 1.f) || !(keep_residual == keep_residual)) return WESUP_ERR_INVALID;
    if (((uintptr_t)src_blocks & 3) || ((uintptr_t)dst_blocks & 3) || ((uintptr_t)jitter & 3)) return WESUP_ERR_INVALID;
    const long HW = (long)H * W;
    // in place, or apart: a partial overlap would read what another thread has written
    if (out != img) {
        const size_t bytes = (size_t)B * HW * 3;
        if ((uintptr_t)out < (uintptr_t)img + bytes && (uintptr_t)img < (uintptr_t)out + bytes) return WESUP_ERR_INVALID;
    }
    // the dword path needs image b of both buffers at the same phase of the 4-byte grid: 3 HW bytes per image
    const int same_phase = (((uintptr_t)img ^ (uintptr_t)out) & 3) == 0;
    const int wide = same_phase ? 1 : 0;
    const unsigned blocks = grid_stride_blocks(wide ? (HW + 3) / 4 : HW, 256, ST_MAP_BLOCKS);
    WESUP_LAUNCH(st_apply_kernel, dim3(blocks, B), dim3(256), 0, (hipStream_t)stream, img, out, src_blocks, dst_blocks, dst_stride,
                 jitter, keep_residual, HW, io, wide);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

// Non-negative int32 keys through the same passes.  A key 0 .. 2^31 - 1 read as a float has its sign bit clear, and sel_key maps
// such a pattern u to u | 0x80000000: a pure bit map that keeps the integer order of every one of them, the patterns above
// 0x7F800000 (NaNs to a float reader) included; sel_unkey clears the bit again.  Between the load and the store the value only
// passes through bit casts and integer instructions, so no NaN is quieted on the way.
extern "C" size_t wesup_select_i32_workspace_bytes(long n) { return wesup_select_f32_workspace_bytes(n); }

extern "C" int wesup_select_i32(const int32_t* keys, long n, const long* ranks, int n_ranks, int32_t* out, void* ws, size_t ws_bytes,
                                void* stream) {
    return wesup_select_f32((const float*)keys, n, ranks, n_ranks, (float*)out, ws, ws_bytes, stream);
}
