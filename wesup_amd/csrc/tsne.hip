// Exact t-SNE of superpixel features (the reference's plot_tsne.py hands model.sp_features to
// sklearn.manifold.TSNE): squared distances, the per-row perplexity search with the joint probabilities, and the gradient
// iterations.  fp32 VALU throughout, no matrix instruction, no floating-point atomic: every sum has one owner and a fixed order,
// so two runs give the same bits.
//
//   ts_sqdist_kernel      d2[i][j] = sum_k (x[i][k] - x[j][k])^2 from differences in ascending k (never the Gram form: ReLU
//                         features of one cluster are close together and |a|^2 + |b|^2 - 2ab cancels).  (a - b)^2 and (b - a)^2
//                         are the same bits, so the matrix is bit-symmetric and its diagonal exactly 0.
//   ts_search_kernel      a block per row: scikit-learn's search for beta_i (start at 1, double / halve while a bound is
//                         infinite, bisect otherwise, at most 100 steps, stop at |H - log perplexity| <= 1e-5) on distances
//                         shifted by the row's smallest off-diagonal one, then the conditional row C[i][:] and its sum.
//   ts_total_kernel       one block adds the row sums in a fixed order.
//   ts_symmetrise_kernel  P = max((C + C^T) / total, eps) in place: a 64 x 64 tile and its mirror per block, every pair
//                         computed once and written to both places; the diagonal 0.
//   ts_pair_kernel        a block owns 16 rows (4 per wave) of one column slab; y of a 256-column chunk is staged in LDS, the
//                         lanes of a wave walk the columns (coalesced reads of P), a butterfly of shuffles folds the 64 lanes.
//                         Per row and slab: att (2), rep (2), z and -- in the last iteration of a call -- sum p log p, sum p log num.
//   ts_update_kernel      every block adds all z partials in the same order (Z), a thread per row adds the row's slab partials
//                         in slab order, g = 4 (att - rep / Z), the delta-bar-delta update; in the last iteration block 0 walks
//                         all rows once more for |g| and the KL divergence.
#include <math.h>
#include "common.hpp"

#define TS_EPS 2.220446049250313e-16f   // scikit-learn's MACHINE_EPSILON (the double's): a normal number in fp32 too
#define TS_TILE 64                      // sqdist and symmetrise: a 64 x 64 tile of the matrix per block
#define TS_KC 32                        // sqdist: feature columns per LDS stage
#define TS_ROWS 16                      // pair pass: rows per block ...
#define TS_RPW 4                        // ... of which each of the 4 waves owns this many
#define TS_CHUNK 256                    // pair pass: columns of y staged in LDS at a time
#define TS_SLAB_ALIGN 64                // a column slab is a multiple of this wide
#define TS_TARGET_BLOCKS 1024           // pair pass: split the columns into slabs until there are about this many blocks
#define TS_PARTS 7                      // att.x att.y rep.x rep.y z plogp plognum
#define TS_MAX_ITERS 65536
#define TS_SEARCH_STEPS 100
#define TS_SEARCH_TOL 1e-5f

namespace {

__device__ __forceinline__ float wave_sum(float v) {
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float wave_min(float v) {
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
    return v;
}
// sum over the 256 threads of a block, the same bits in every thread: lanes by butterfly, then the four waves in order
__device__ __forceinline__ float block_sum(float v, float* red /* 4 floats of LDS */) {
    v = wave_sum(v);
    __syncthreads();                                                     // red's readers of the call before
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
__device__ __forceinline__ float block_min(float v, float* red) {
    v = wave_min(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

__global__ __launch_bounds__(256) void ts_sqdist_kernel(const float* __restrict__ x, float* __restrict__ d2, int n, int d) {
    __shared__ float xi[TS_TILE][TS_KC + 1], xj[TS_TILE][TS_KC + 1];
    const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const int i0 = blockIdx.y * TS_TILE, j0 = blockIdx.x * TS_TILE;
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
    for (int k0 = 0; k0 < d; k0 += TS_KC) {
        for (int t = threadIdx.x; t < TS_TILE * TS_KC; t += 256) {
            const int r = t / TS_KC, k = t % TS_KC;
            const int gi = i0 + r, gj = j0 + r, gk = k0 + k;
            // past the last feature both sides hold 0: the step adds (0 - 0)^2 and leaves the sum's bits alone
            xi[r][k] = (gi < n && gk < d) ? x[(long)gi * d + gk] : 0.f;
            xj[r][k] = (gj < n && gk < d) ? x[(long)gj * d + gk] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < TS_KC; ++k) {
            float a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = xi[ty * 4 + r][k];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = xj[tx + 16 * c][k];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float df = a[r] - b[c];
                    acc[r][c] = fmaf(df, df, acc[r][c]);
                }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int i = i0 + ty * 4 + r, j = j0 + tx + 16 * c;
            if (i < n && j < n) d2[(long)i * n + j] = i == j ? 0.f : acc[r][c];
        }
}

__global__ __launch_bounds__(256) void ts_search_kernel(const float* __restrict__ d2, float* __restrict__ c, float* __restrict__ beta_out,
                                                        float* __restrict__ rowsum, int n, float log_perp) {
    __shared__ float red[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const float* row = d2 + (long)i * n;
    float m = INFINITY;
    for (int j = tid; j < n; j += 256)
        if (j != i) m = fminf(m, row[j]);
    m = block_min(m, red);
    // every thread of the block holds the same S, SD and so takes the same branches: the loop is block-uniform
    float beta = 1.f, lo = -INFINITY, hi = INFINITY, beta_used = 1.f, s_used = 1.f;
    for (int step = 0; step < TS_SEARCH_STEPS; ++step) {
        float s = 0.f, sd = 0.f;
        for (int j = tid; j < n; j += 256)
            if (j != i) {
                const float dd = row[j] - m;
                const float e = expf(-beta * dd);
                s += e;
                sd = fmaf(dd, e, sd);
            }
        s = block_sum(s, red);                                           // >= 1: the nearest neighbour contributes exp(0)
        sd = block_sum(sd, red);
        beta_used = beta;
        s_used = s;
        const float diff = logf(s) + beta * sd / s - log_perp;
        if (fabsf(diff) <= TS_SEARCH_TOL) break;
        if (diff > 0.f) {
            lo = beta;
            beta = hi == INFINITY ? beta * 2.f : (beta + hi) * 0.5f;
        } else {
            hi = beta;
            beta = lo == -INFINITY ? beta * 0.5f : (beta + lo) * 0.5f;
        }
    }
    float rs = 0.f;
    float* crow = c + (long)i * n;
    for (int j = tid; j < n; j += 256) {
        float v = 0.f;
        if (j != i) v = expf(-beta_used * (row[j] - m)) / s_used;
        crow[j] = v;
        rs += v;
    }
    rs = block_sum(rs, red);
    if (tid == 0) {
        rowsum[i] = rs;
        beta_out[i] = beta_used;
    }
}

// total[0] = max(sum of (C + C^T), eps) = max(2 * sum of the row sums, eps)
__global__ __launch_bounds__(256) void ts_total_kernel(const float* __restrict__ rowsum, float* __restrict__ total, int n) {
    __shared__ float red[4];
    float s = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) s += rowsum[j];
    s = block_sum(s, red);
    if (threadIdx.x == 0) total[0] = fmaxf(2.f * s, TS_EPS);
}

__global__ __launch_bounds__(256) void ts_symmetrise_kernel(float* __restrict__ p, const float* __restrict__ total, int n) {
    __shared__ float A[TS_TILE][TS_TILE + 1], B[TS_TILE][TS_TILE + 1];
    const int bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;                                                 // the mirror tile's block writes this one
    const int i0 = bi * TS_TILE, j0 = bj * TS_TILE;
    const float tot = total[0];
    for (int t = threadIdx.x; t < TS_TILE * TS_TILE; t += 256) {
        const int r = t / TS_TILE, q = t % TS_TILE;
        A[r][q] = (i0 + r < n && j0 + q < n) ? p[(long)(i0 + r) * n + j0 + q] : 0.f;
        B[r][q] = (j0 + r < n && i0 + q < n) ? p[(long)(j0 + r) * n + i0 + q] : 0.f;
    }
    __syncthreads();
    float v[TS_TILE * TS_TILE / 256];
#pragma unroll
    for (int u = 0; u < TS_TILE * TS_TILE / 256; ++u) {
        const int t = threadIdx.x + u * 256, r = t / TS_TILE, q = t % TS_TILE;
        v[u] = (i0 + r == j0 + q) ? 0.f : fmaxf((A[r][q] + B[q][r]) / tot, TS_EPS);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TS_TILE * TS_TILE / 256; ++u) {
        const int t = threadIdx.x + u * 256, r = t / TS_TILE, q = t % TS_TILE;
        A[r][q] = v[u];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < TS_TILE * TS_TILE; t += 256) {
        const int r = t / TS_TILE, q = t % TS_TILE;
        if (i0 + r < n && j0 + q < n) p[(long)(i0 + r) * n + j0 + q] = A[r][q];
        // (on the diagonal tile the mirror is the tile itself: A[q][r] was computed from the same two addends, a + b == b + a)
        if (bi != bj && j0 + r < n && i0 + q < n) p[(long)(j0 + r) * n + i0 + q] = A[q][r];
    }
}

template <bool LAST>
__global__ __launch_bounds__(256) void ts_pair_kernel(const float* __restrict__ p, const float2* __restrict__ y, float* __restrict__ part,
                                                      int n, int slab_w, float ex) {
    __shared__ float2 ys[TS_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i_base = blockIdx.x * TS_ROWS + wave * TS_RPW;             // wave-uniform
    const int c_begin = blockIdx.y * slab_w, c_end = min(n, c_begin + slab_w);
    int ir[TS_RPW];
    float2 yi[TS_RPW];
    const float* prow[TS_RPW];
    float ax[TS_RPW], ay[TS_RPW], rx[TS_RPW], ry[TS_RPW], z[TS_RPW], ka[TS_RPW], kb[TS_RPW];
#pragma unroll
    for (int r = 0; r < TS_RPW; ++r) {
        ir[r] = min(i_base + r, n - 1);                                  // rows past the end repeat the last one and are not written
        yi[r] = y[ir[r]];
        prow[r] = p + (long)ir[r] * n;
        ax[r] = ay[r] = rx[r] = ry[r] = z[r] = ka[r] = kb[r] = 0.f;
    }
    for (int c0 = c_begin; c0 < c_end; c0 += TS_CHUNK) {
        const int len = min(TS_CHUNK, c_end - c0);
        __syncthreads();                                                 // the chunk before has been consumed
        for (int t = tid; t < len; t += 256) ys[t] = y[c0 + t];
        __syncthreads();
        for (int t = lane; t < len; t += 64) {
            const float2 yj = ys[t];
            const int j = c0 + t;
#pragma unroll
            for (int r = 0; r < TS_RPW; ++r) {
                const float pv = prow[r][j];
                const float dx = yi[r].x - yj.x, dy = yi[r].y - yj.y;
                const float num = 1.f / (1.f + (dx * dx + dy * dy));
                const float w = ex * pv * num;                           // p[i][i] = 0 and y_i - y_i = 0: the diagonal adds nothing
                ax[r] = fmaf(w, dx, ax[r]);
                ay[r] = fmaf(w, dy, ay[r]);
                const float n2 = num * num;
                rx[r] = fmaf(n2, dx, rx[r]);
                ry[r] = fmaf(n2, dy, ry[r]);
                const bool off = j != ir[r];
                z[r] += off ? num : 0.f;
                if (LAST) {
                    const float pc = fmaxf(pv, TS_EPS);
                    ka[r] += off ? pc * logf(pc) : 0.f;
                    kb[r] += off ? pc * logf(num) : 0.f;
                }
            }
        }
    }
    float* out = part + (long)blockIdx.y * TS_PARTS * n;
#pragma unroll
    for (int r = 0; r < TS_RPW; ++r) {
        const float s0 = wave_sum(ax[r]), s1 = wave_sum(ay[r]), s2 = wave_sum(rx[r]), s3 = wave_sum(ry[r]), s4 = wave_sum(z[r]);
        float s5 = 0.f, s6 = 0.f;
        if (LAST) {
            s5 = wave_sum(ka[r]);
            s6 = wave_sum(kb[r]);
        }
        const int i = i_base + r;
        if (lane == 0 && i < n) {
            out[0 * (long)n + i] = s0;
            out[1 * (long)n + i] = s1;
            out[2 * (long)n + i] = s2;
            out[3 * (long)n + i] = s3;
            out[4 * (long)n + i] = s4;
            if (LAST) {
                out[5 * (long)n + i] = s5;
                out[6 * (long)n + i] = s6;
            }
        }
    }
}

// a row's gradient from its slab partials, slabs in ascending order
__device__ __forceinline__ float2 ts_row_grad(const float* __restrict__ part, int n, int slabs, int i, float Z) {
    float a0 = 0.f, a1 = 0.f, r0 = 0.f, r1 = 0.f;
    for (int s = 0; s < slabs; ++s) {
        const float* q = part + (long)s * TS_PARTS * n + i;
        a0 += q[0];
        a1 += q[n];
        r0 += q[2 * (long)n];
        r1 += q[3 * (long)n];
    }
    return make_float2(4.f * (a0 - r0 / Z), 4.f * (a1 - r1 / Z));
}

template <bool LAST>
__global__ __launch_bounds__(256) void ts_update_kernel(const float* __restrict__ part, float2* __restrict__ y, float2* __restrict__ upd,
                                                        float2* __restrict__ gains, float* __restrict__ stats, int n, int slabs,
                                                        float momentum, float lr, float min_gain, int apply) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    float zs = 0.f;
    for (int s = 0; s < slabs; ++s) {
        const float* q = part + ((long)s * TS_PARTS + 4) * n;
        for (int t = tid; t < n; t += 256) zs += q[t];
    }
    const float Z = block_sum(zs, red);                                  // the same additions in the same order in every block
    const int i = blockIdx.x * 256 + tid;
    if (apply && i < n) {
        const float2 g = ts_row_grad(part, n, slabs, i, Z);
        float2 u = upd[i], ga = gains[i], yy = y[i];
        ga.x = fmaxf(u.x * g.x < 0.f ? ga.x + 0.2f : ga.x * 0.8f, min_gain);
        ga.y = fmaxf(u.y * g.y < 0.f ? ga.y + 0.2f : ga.y * 0.8f, min_gain);
        u.x = momentum * u.x - lr * (g.x * ga.x);
        u.y = momentum * u.y - lr * (g.y * ga.y);
        yy.x += u.x;
        yy.y += u.y;
        gains[i] = ga;
        upd[i] = u;
        y[i] = yy;
    }
    if (LAST && blockIdx.x == 0) {                                       // (reads the partials only: no block writes them here)
        float g2 = 0.f, ka = 0.f, kb = 0.f;
        for (int t = tid; t < n; t += 256) {
            const float2 g = ts_row_grad(part, n, slabs, t, Z);
            g2 = fmaf(g.x, g.x, fmaf(g.y, g.y, g2));
            for (int s = 0; s < slabs; ++s) {
                const float* q = part + (long)s * TS_PARTS * n + t;
                ka += q[5 * (long)n];
                kb += q[6 * (long)n];
            }
        }
        g2 = block_sum(g2, red);
        ka = block_sum(ka, red);
        kb = block_sum(kb, red);
        if (tid == 0) {
            stats[0] = ka - kb + logf(Z);
            stats[1] = sqrtf(g2);
            stats[2] = Z;
            stats[3] = ka;
        }
    }
}

// column slabs of the pair pass: enough of them for about TS_TARGET_BLOCKS blocks, each a multiple of TS_SLAB_ALIGN wide
inline void ts_slabs(int n, int* slabs, int* slab_w) {
    const int rb = ceil_div(n, TS_ROWS);
    int s = ceil_div(TS_TARGET_BLOCKS, rb);
    const int most = ceil_div(n, TS_SLAB_ALIGN);
    if (s > most) s = most;
    if (s < 1) s = 1;
    const int w = ceil_div(ceil_div(n, s), TS_SLAB_ALIGN) * TS_SLAB_ALIGN;
    *slab_w = w;
    *slabs = ceil_div(n, w);
}

inline bool ts_bad_n(int n) { return n < 2 || n > WESUP_TSNE_MAX_N; }

}  // namespace

extern "C" int wesup_tsne_sqdist(const float* x, int n, int d, float* d2, void* stream) {
    if (!x || !d2 || ts_bad_n(n) || d < 1 || d > WESUP_TSNE_MAX_D) return WESUP_ERR_INVALID;
    const int nb = ceil_div(n, TS_TILE);
    WESUP_LAUNCH(ts_sqdist_kernel, dim3(nb, nb), dim3(256), 0, (hipStream_t)stream, x, d2, n, d);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_tsne_affinities_workspace_bytes(int n) {
    if (ts_bad_n(n)) return 0;
    return align_up(((size_t)n + 1) * 4, 256);                                  // the row sums, then their total
}

extern "C" int wesup_tsne_affinities(const float* d2, int n, float perplexity, float* p, float* beta, void* ws, size_t ws_bytes,
                                     void* stream) {
    if (!d2 || !p || !beta || !ws || ts_bad_n(n) || !(perplexity > 0.f) || !(perplexity < (float)n)) return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_tsne_affinities_workspace_bytes(n)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    float* rowsum = (float*)ws;
    float* total = rowsum + n;
    WESUP_LAUNCH(ts_search_kernel, dim3(n), dim3(256), 0, st, d2, p, beta, rowsum, n, logf(perplexity));
    WESUP_LAUNCH(ts_total_kernel, dim3(1), dim3(256), 0, st, (const float*)rowsum, total, n);
    const int nb = ceil_div(n, TS_TILE);
    WESUP_LAUNCH(ts_symmetrise_kernel, dim3(nb, nb), dim3(256), 0, st, p, (const float*)total, n);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_tsne_iterate_workspace_bytes(int n) {
    if (ts_bad_n(n)) return 0;
    int slabs, slab_w;
    ts_slabs(n, &slabs, &slab_w);
    return align_up((size_t)slabs * TS_PARTS * (size_t)n * 4, 256);
}

extern "C" int wesup_tsne_iterate(const float* p, float* y, float* upd, float* gains, float* stats, int n, int iters,
                                  float exaggeration, float momentum, float lr, float min_gain, void* ws, size_t ws_bytes,
                                  void* stream) {
    if (!p || !y || !upd || !gains || !stats || !ws || ts_bad_n(n) || iters < 0 || iters > TS_MAX_ITERS || !(exaggeration > 0.f) ||
        !(momentum >= 0.f) || !(lr > 0.f) || !(min_gain >= 0.f))
        return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_tsne_iterate_workspace_bytes(n)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int slabs, slab_w;
    ts_slabs(n, &slabs, &slab_w);
    float* part = (float*)ws;
    const dim3 pgrid(ceil_div(n, TS_ROWS), slabs), ugrid(ceil_div(n, 256));
    const float2* yc = (const float2*)y;
    if (iters == 0) {                                                    // KL, |g| and Z of y as it stands; nothing moves
        WESUP_LAUNCH(ts_pair_kernel<true>, pgrid, dim3(256), 0, st, p, yc, part, n, slab_w, exaggeration);
        WESUP_LAUNCH(ts_update_kernel<true>, ugrid, dim3(256), 0, st, (const float*)part, (float2*)y, (float2*)upd, (float2*)gains,
                     stats, n, slabs, momentum, lr, min_gain, 0);
    }
    for (int it = 0; it < iters; ++it) {
        if (it + 1 == iters) {
            WESUP_LAUNCH(ts_pair_kernel<true>, pgrid, dim3(256), 0, st, p, yc, part, n, slab_w, exaggeration);
            WESUP_LAUNCH(ts_update_kernel<true>, ugrid, dim3(256), 0, st, (const float*)part, (float2*)y, (float2*)upd,
                         (float2*)gains, stats, n, slabs, momentum, lr, min_gain, 1);
        } else {
            WESUP_LAUNCH(ts_pair_kernel<false>, pgrid, dim3(256), 0, st, p, yc, part, n, slab_w, exaggeration);
            WESUP_LAUNCH(ts_update_kernel<false>, ugrid, dim3(256), 0, st, (const float*)part, (float2*)y, (float2*)upd,
                         (float2*)gains, stats, n, slabs, momentum, lr, min_gain, 1);
        }
    }
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
