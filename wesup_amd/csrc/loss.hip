// Head and loss kernels: classifier + softmax, label propagation over the superpixel affinity
// exp(-|fi-fj|^2), semi-supervised cross entropy, fused SGD, segmentation metric sums.
// All reductions are fixed-order (no float atomics): results are bitwise reproducible.
#include "common.hpp"

// block-wide sum of `v` over 256 threads, fixed tree order; result valid in all threads
__device__ __forceinline__ float block_sum256(float v, float* sh) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
#pragma unroll
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) sh[tid] += sh[tid + off];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

// ------------------------------------------------------------------ classifier Linear(D,C) + Softmax(dim=1), 2 <= C <= WESUP_MAX_CLASSES
// One body per operation.  Two classes -- the training step -- are instantiated with the class count as a compile-time constant
// (cls_row<2, .>, the <2> forms of the backward bodies), more classes with the run-time count; the two-class entries call the _c
// entries with C = 2, which launch the two-class instantiations.
// One row: logits by fmaf in ascending k, the maximum subtracted, the exponentials summed in ascending class order, one
// reciprocal.  The logits live in registers: z[] is indexed by unrolled constants only, CMAX >= C bounds it at compile time.
// W: [C][D] and bias [C], in LDS (classifier_fwd_c_kernel) or global memory (its form for a table beyond the LDS, and prop_body's
// tail) -- the arithmetic is the same.
template <int CMAX, bool VEC4>
__device__ __forceinline__ void cls_row(const float* __restrict__ f, const float* W, const float* bias, float* __restrict__ out,
                                        int D, int C, bool st4_ok = false) {
    float z[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) z[c] = (c < C) ? bias[c] : 0.f;
    if constexpr (VEC4) {
        for (int k = 0; k < D; k += 4) {
            const float4 v = ld4(f + k);
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float4 w = ld4(W + c * D + k);
                    z[c] = fmaf(v.x, w.x, z[c]);
                    z[c] = fmaf(v.y, w.y, z[c]);
                    z[c] = fmaf(v.z, w.z, z[c]);
                    z[c] = fmaf(v.w, w.w, z[c]);
                }
        }
    } else {
        for (int k = 0; k < D; ++k) {
            const float v = f[k];
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) z[c] = fmaf(v, W[c * D + k], z[c]);
        }
    }
    float m = z[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C) m = fmaxf(m, z[c]);
    z[0] = expf(z[0] - m);
    float s = z[0];
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C) {
            z[c] = expf(z[c] - m);
            s += z[c];
        }
    const float inv = 1.f / s;
    if (CMAX >= 4 && st4_ok) {                      // (C % 4 == 0, out 16-byte aligned)
#pragma unroll
        for (int c = 0; c + 3 < CMAX; c += 4)
            if (c < C) st4(out + c, make_float4(z[c] * inv, z[c + 1] * inv, z[c + 2] * inv, z[c + 3] * inv));
    } else {
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) out[c] = z[c] * inv;
    }
}
// Streaming form (pixel inference runs it with R = B*H*W): Wc and bc staged in LDS once per block (every lane reads the same
// address: a broadcast), a thread per row, rows read as float4 where D % 4 == 0, at most 2048 blocks that stride over the rows.
// LDS = false: no staging, cls_row reads Wc / bc themselves (a table larger than the LDS a kernel gets without asking).
template <int CMAX, bool VEC4, bool LDS = true>
__global__ __launch_bounds__(256) void classifier_fwd_c_kernel(const float* __restrict__ feat, const float* __restrict__ Wc,
                                                               const float* __restrict__ bc, float* __restrict__ pred, int R,
                                                               int D, int C, int st4_ok) {
    extern __shared__ __align__(16) float shw[];                  // [C][D] | [C]
    if constexpr (LDS) {
        for (int e = threadIdx.x; e < C * D; e += 256) shw[e] = Wc[e];
        if (threadIdx.x < C) shw[C * D + threadIdx.x] = bc[threadIdx.x];
        __syncthreads();
    }
    for (long r = (long)blockIdx.x * 256 + threadIdx.x; r < R; r += (long)gridDim.x * 256) {
        if constexpr (LDS) cls_row<CMAX, VEC4>(feat + r * D, shw, shw + C * D, pred + r * C, D, C, st4_ok != 0);
        else cls_row<CMAX, false>(feat + r * D, Wc, bc, pred + r * C, D, C, st4_ok != 0);
    }
}
#define CLS_C_MAX_D 512                             // (C * D + C floats of LDS: 32 KB at C = 16)
#define CLS_LDS_DEFAULT (64 * 1024)                 // (the dynamic LDS a kernel gets without asking)
static inline bool cls_c_range(int C) { return C >= 2 && C <= WESUP_MAX_CLASSES; }
template <int CMAX>
static int classifier_fwd_c_launch(const float* feat, const float* Wc, const float* bc, float* pred, int R, int D, int C,
                                   hipStream_t st) {
    const bool vec = (D % 4 == 0) && (((uintptr_t)feat & 15) == 0);
    const int st4_ok = (C % 4 == 0) && (((uintptr_t)pred & 15) == 0);
    const int blocks = min(ceil_div(R, 256), 2048);
    const size_t lds = ((size_t)C * D + C) * sizeof(float);
    if (CMAX == 2 && lds > CLS_LDS_DEFAULT)         // D >= 8192: wesup_classifier_fwd alone takes any D, the _c entry D <= 512
        WESUP_LAUNCH((classifier_fwd_c_kernel<2, false, false>), dim3(blocks), dim3(256), 0, st, feat, Wc, bc, pred, R, D, C, st4_ok);
    else if (vec)
        WESUP_LAUNCH((classifier_fwd_c_kernel<CMAX, true>), dim3(blocks), dim3(256), lds, st, feat, Wc, bc, pred, R, D, C, st4_ok);
    else
        WESUP_LAUNCH((classifier_fwd_c_kernel<CMAX, false>), dim3(blocks), dim3(256), lds, st, feat, Wc, bc, pred, R, D, C, st4_ok);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
// two classes, any D > 0 (models/wesup.py:229-232,292)
extern "C" int wesup_classifier_fwd(const float* feat, const float* Wc, const float* bc, float* pred, int R, int D,
                                    void* stream) {
    if (!feat || !Wc || !bc || !pred || R <= 0 || D <= 0) return WESUP_ERR_INVALID;
    return classifier_fwd_c_launch<2>(feat, Wc, bc, pred, R, D, 2, (hipStream_t)stream);
}
extern "C" int wesup_classifier_fwd_c(const float* feat, const float* Wc, const float* bc, float* pred, int R, int D, int C,
                                      void* stream) {
    if (!feat || !Wc || !bc || !pred || R <= 0 || D <= 0 || D > CLS_C_MAX_D || !cls_c_range(C)) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (C <= 2) return classifier_fwd_c_launch<2>(feat, Wc, bc, pred, R, D, C, st);
    if (C <= 4) return classifier_fwd_c_launch<4>(feat, Wc, bc, pred, R, D, C, st);
    if (C <= 8) return classifier_fwd_c_launch<8>(feat, Wc, bc, pred, R, D, C, st);
    return classifier_fwd_c_launch<WESUP_MAX_CLASSES>(feat, Wc, bc, pred, R, D, C, st);
}

// backward, C classes: dz_c = p_c (dp_c - sum_j dp_j p_j); dfeat = (sum_c dz_c Wc[c][k] + extra) masked by feat > 0; partial
// dWc / dbc per 64 rows, reduced in fixed order.  The class sums are written with their fused multiply-adds spelled out: the
// first product, then fmaf in ascending class order.  Left to the compiler (-ffp-contract=fast) either product of a sum of two
// may become the addend, and the instantiations -- unfused and fused (head_bwd_body), two classes and C -- which must agree bit
// for bit, are contracted separately.  No per-thread array: a row's dpred waits in its LDS row of dz.
// CT: the class count where it is a compile-time constant (2: the training step), 0: the run-time C.  CT sizes a row of dz.
#define CLS_ROWS 64
static constexpr int cls_dz_width(int CT) { return CT ? CT : WESUP_MAX_CLASSES; }
__device__ __forceinline__ void cls_dz_row(const float* __restrict__ p, float* dzrow, int C) {
    float s = dzrow[0] * p[0];
    for (int c = 1; c < C; ++c) s = fmaf(dzrow[c], p[c], s);
    for (int c = 0; c < C; ++c) dzrow[c] = p[c] * (dzrow[c] - s);
}
// dfeat of the block's rows and the block's partial sums, from dz[CLS_ROWS][cls_dz_width(CT)] in LDS (behind a __syncthreads).
// nrow: how many of the block's CLS_ROWS rows exist (their dz beyond is zero); a constant where the caller knows it, so that the
// loops over the rows carry no test and their loads go out together.
template <int CT>
__device__ __forceinline__ void cls_bwd_tail(const float* __restrict__ feat, const float* __restrict__ Wc,
                                             const float* __restrict__ extra, float* __restrict__ dfeat,
                                             float* __restrict__ part, const float (*dz)[cls_dz_width(CT)], long r0, int nrow, int D,
                                             int C) {
    const int tid = threadIdx.x;
    float* pout = part + (long)blockIdx.x * (C * D + C);
    for (int e = tid; e < nrow * D; e += 256) {
        const int rr = e / D, k = e - rr * D;
        const long r = r0 + rr;
        float g = dz[rr][0] * Wc[k];
        for (int c = 1; c < C; ++c) g = fmaf(dz[rr][c], Wc[c * D + k], g);
        if (extra) g += extra[r * D + k];
        dfeat[r * D + k] = feat[r * D + k] > 0.f ? g : 0.f;
    }
    for (int e = tid; e < C * D + C; e += 256) {
        float s = 0.f;
        if (e < C * D) {
            const int c = e / D, k = e - c * D;
            for (int rr = 0; rr < nrow; ++rr) s = fmaf(dz[rr][c], feat[(r0 + rr) * D + k], s);
        } else {
            const int c = e - C * D;
            for (int rr = 0; rr < CLS_ROWS; ++rr) s += dz[rr][c];
        }
        pout[e] = s;
    }
}
template <int CT>
__global__ __launch_bounds__(256) void classifier_bwd_c_kernel(const float* __restrict__ feat, const float* __restrict__ Wc,
                                                               const float* __restrict__ pred, const float* __restrict__ dpred,
                                                               const float* __restrict__ extra, float* __restrict__ dfeat,
                                                               float* __restrict__ part, int R, int D, int C_rt) {
    __shared__ float dz[CLS_ROWS][cls_dz_width(CT)];
    const int C = CT ? CT : C_rt;
    const long r0 = (long)blockIdx.x * CLS_ROWS;
    const int tid = threadIdx.x;
    if (tid < CLS_ROWS) {
        const long r = r0 + tid;
        if (r < R) {
            for (int c = 0; c < C; ++c) dz[tid][c] = dpred[r * C + c];
            cls_dz_row(pred + r * C, dz[tid], C);
        } else {
            for (int c = 0; c < C; ++c) dz[tid][c] = 0.f;
        }
    }
    __syncthreads();
    cls_bwd_tail<CT>(feat, Wc, extra, dfeat, part, dz, r0, (int)min((long)CLS_ROWS, R - r0), D, C);
}
// dWc / dbc: the blocks' partial sums added in ascending block order.  (Two plain kernels: the recorded two-class step names
// classifier_bwd_reduce.)
__device__ __forceinline__ void cls_reduce(const float* __restrict__ part, float* __restrict__ dWc, float* __restrict__ dbc,
                                           int nblk, int D, int C) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= C * D + C) return;
    float s = 0.f;
    for (int b = 0; b < nblk; ++b) s += part[(long)b * (C * D + C) + e];
    if (e < C * D) dWc[e] = s;
    else dbc[e - C * D] = s;
}
__global__ void classifier_bwd_reduce(const float* __restrict__ part, float* __restrict__ dWc, float* __restrict__ dbc,
                                      int nblk, int D) {
    cls_reduce(part, dWc, dbc, nblk, D, 2);
}
__global__ void classifier_bwd_c_reduce(const float* __restrict__ part, float* __restrict__ dWc, float* __restrict__ dbc,
                                        int nblk, int D, int C) {
    cls_reduce(part, dWc, dbc, nblk, D, C);
}
static void cls_reduce_launch(const void* ws, float* dWc, float* dbc, int R, int D, int C, hipStream_t st) {
    const dim3 grid(ceil_div(C * D + C, 64));
    const int nblk = ceil_div(R, CLS_ROWS);
    if (C == 2) WESUP_LAUNCH(classifier_bwd_reduce, grid, dim3(64), 0, st, (const float*)ws, dWc, dbc, nblk, D);
    else WESUP_LAUNCH(classifier_bwd_c_reduce, grid, dim3(64), 0, st, (const float*)ws, dWc, dbc, nblk, D, C);
}
extern "C" size_t wesup_classifier_bwd_c_workspace_bytes(int R, int D, int C) {
    if (R <= 0 || D <= 0 || !cls_c_range(C)) return 0;
    return (size_t)ceil_div(R, CLS_ROWS) * (C * D + C) * sizeof(float);
}
extern "C" int wesup_classifier_bwd_c(const float* feat, const float* Wc, const float* pred, const float* dpred,
                                      const float* dfeat_extra, float* dfeat, float* dWc, float* dbc, int R, int D, int C,
                                      void* ws, size_t ws_bytes, void* stream) {
    if (!feat || !Wc || !pred || !dpred || !dfeat || !dWc || !dbc || !ws || R <= 0 || D <= 0 || !cls_c_range(C))
        return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_classifier_bwd_c_workspace_bytes(R, D, C)) return WESUP_ERR_WORKSPACE;
    const dim3 grid(ceil_div(R, CLS_ROWS));
    hipStream_t st = (hipStream_t)stream;
    if (C == 2) WESUP_LAUNCH(classifier_bwd_c_kernel<2>, grid, dim3(256), 0, st, feat, Wc, pred, dpred, dfeat_extra, dfeat, (float*)ws, R, D, C);
    else WESUP_LAUNCH(classifier_bwd_c_kernel<0>, grid, dim3(256), 0, st, feat, Wc, pred, dpred, dfeat_extra, dfeat, (float*)ws, R, D, C);
    cls_reduce_launch(ws, dWc, dbc, R, D, C, st);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
// two classes: the _c entries with C = 2
extern "C" size_t wesup_classifier_bwd_workspace_bytes(int R, int D) { return wesup_classifier_bwd_c_workspace_bytes(R, D, 2); }
extern "C" int wesup_classifier_bwd(const float* feat, const float* Wc, const float* pred, const float* dpred,
                                    const float* dfeat_extra, float* dfeat, float* dWc, float* dbc, int R, int D,
                                    void* ws, size_t ws_bytes, void* stream) {
    return wesup_classifier_bwd_c(feat, Wc, pred, dpred, dfeat_extra, dfeat, dWc, dbc, R, D, 2, ws, ws_bytes, stream);
}

// ------------------------------------------------------------------ label propagation (models/wesup.py:99-139)
// One launch: a block owns PROP_ROWS consecutive rows of an image.  It first writes what every row has whatever happens next --
// y_all = the row's own labels (labelled rows) or zeros, src_idx = -1, max_sim = 0 (a launch of its own until round 5) -- and
// then, for its unlabelled rows, one wave per row: lanes stride over the labelled rows j (staged in LDS 256 at a time, row stride
// D+1 floats so that lanes hit distinct banks).  d_ij = sum_k (f_j,k - f_i,k)^2 as a direct difference in ascending k (not
// |a|^2+|b|^2-2ab: near-ties must not flip); W = expf(-d); the row maximum takes the FIRST (lowest) labelled index on ties, as
// torch.max(dim=1) does; propagate iff W > threshold (strict).
#define PROP_TILE 256
#define PROP_ROWS 16
// Dynamic LDS of a block for a feature width D: the labelled tile [PROP_TILE][D+1] and the block's own rows [PROP_ROWS][D] --
// 1088 D + 1024 bytes.  Up to D = 59 that fits the 64 KiB a kernel gets without asking; from D = 60 (66 304 B) the entry raises
// the kernel's limit, once, to the CU's 160 KiB, which holds D <= WESUP_HEAD_MAX_D = 149 (163 136 B; D = 150 needs 164 224 B and
// is refused before any launch).  From D = 60 on a CU holds one block at a time; nothing changes for the step's D = 32 (35 840 B).
#define PROP_LDS_DEFAULT (64 * 1024)
#define PROP_LDS_MAX (160 * 1024)
static constexpr size_t prop_lds_bytes(int D) {
    return ((size_t)PROP_TILE * ((size_t)D + 1) + (size_t)PROP_ROWS * (size_t)D) * sizeof(float);
}
static_assert(prop_lds_bytes(WESUP_HEAD_MAX_D) <= PROP_LDS_MAX && prop_lds_bytes(WESUP_HEAD_MAX_D + 1) > PROP_LDS_MAX,
              "WESUP_HEAD_MAX_D (include/wesup_hip.h) is the largest D whose propagation tile fits the CU's LDS");
// (the body of prop_kernel and of prop_c_kernel, its form for a classifier of more than two classes: GENERIC only chooses the
// classifier tail, everything else is the same code)
template <bool GENERIC>
__device__ __forceinline__ void prop_body(float* sh, const float* __restrict__ feat, const float* __restrict__ sp_labels,
                                          const int32_t* __restrict__ n_sp, const int32_t* __restrict__ n_l,
                                          float thr, int enable, float* __restrict__ y_all, int32_t* __restrict__ src_idx,
                                          float* __restrict__ max_sim, int Kmax, int D, int C,
                                          const float* __restrict__ Wc, const float* __restrict__ bc,
                                          float* __restrict__ pred) {
    float* fl = sh;                               // [PROP_TILE][D+1]
    float* fi = sh + PROP_TILE * (D + 1);         // [PROP_ROWS][D]
    const int b = blockIdx.y;
    const int nl = n_l[b], ns = n_sp[b];
    const int i_blk = blockIdx.x * PROP_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int e = tid; e < PROP_ROWS * C; e += 256) {
        const int r = i_blk + e / C;
        if (r < Kmax) y_all[((long)b * Kmax + i_blk) * C + e] = (r < nl) ? sp_labels[((long)b * Kmax + i_blk) * C + e] : 0.f;
    }
    if (tid < PROP_ROWS && i_blk + tid < Kmax) {
        src_idx[(long)b * Kmax + i_blk + tid] = -1;
        max_sim[(long)b * Kmax + i_blk + tid] = 0.f;
    }
    // wesup_head_fwd / wesup_head_fwd_c: the classifier + softmax of this block's rows rides along (classifier_fwd_c_kernel's
    // arithmetic, cls_row: a launch of its own on the chain between the fc layers and the loss otherwise).  prop_kernel writes two
    // columns per row whatever the label width C, prop_c_kernel C columns.
    // prop_kernel's tail is cls_row<2, false> typed out, the one two-class body that is kept: as a call the compiler schedules its
    // end with one more s_nop, the propagation loops behind it start 4 bytes later and wesup_head_fwd takes 2.5 % longer at the
    // step's shape (Measured).  Its bits are held to cls_row's by the fused-against-unfused tests.
    if (pred && tid < PROP_ROWS && i_blk + tid < Kmax) {
        const long r = (long)b * Kmax + i_blk + tid;
        if constexpr (GENERIC) {
            cls_row<WESUP_MAX_CLASSES, false>(feat + r * D, Wc, bc, pred + r * C, D, C);
        } else {
            float z0 = bc[0], z1 = bc[1];
            const float* f = feat + r * D;
            for (int k = 0; k < D; ++k) {
                const float v = f[k];
                z0 = fmaf(v, Wc[k], z0);
                z1 = fmaf(v, Wc[D + k], z1);
            }
            const float m = fmaxf(z0, z1);
            const float e0 = expf(z0 - m), e1 = expf(z1 - m);
            const float inv = 1.f / (e0 + e1);
            pred[2 * r] = e0 * inv;
            pred[2 * r + 1] = e1 * inv;
        }
    }
    // rows of this block that take part in the propagation: unlabelled and present (uniform per block)
    if (!enable || nl <= 0 || i_blk + PROP_ROWS <= nl || i_blk >= ns) return;
    __syncthreads();                              // (the defaults above are written before a propagated row overwrites its own)
    const float* fb = feat + (long)b * Kmax * D;
    for (int e = tid; e < PROP_ROWS * D; e += 256) {
        const int rr = e / D, k = e - rr * D;
        fi[e] = (i_blk + rr < ns) ? fb[(long)(i_blk + rr) * D + k] : 0.f;
    }
    float best_w[PROP_ROWS / 4];
    int best_j[PROP_ROWS / 4];
#pragma unroll
    for (int q = 0; q < PROP_ROWS / 4; ++q) {
        best_w[q] = -1.f;
        best_j[q] = 0x7fffffff;
    }
    for (int j0 = 0; j0 < nl; j0 += PROP_TILE) {
        const int nj = min(PROP_TILE, nl - j0);
        __syncthreads();
        for (int e = tid; e < nj * D; e += 256) {
            const int jj = e / D, k = e - jj * D;
            fl[jj * (D + 1) + k] = fb[(long)(j0 + jj) * D + k];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PROP_ROWS / 4; ++q) {
            const int i = i_blk + wave * (PROP_ROWS / 4) + q;
            if (i < nl || i >= ns) continue;      // (wave-uniform: a labelled or absent row)
            const float* f_i = fi + (wave * (PROP_ROWS / 4) + q) * D;
            for (int jj = lane; jj < nj; jj += 64) {
                const float* f_j = fl + jj * (D + 1);
                float d = 0.f;
                for (int k = 0; k < D; ++k) {
                    const float t = f_j[k] - f_i[k];
                    d = fmaf(t, t, d);
                }
                const float w = expf(-d);
                if (w > best_w[q]) {              // strict: earlier j wins ties inside a lane
                    best_w[q] = w;
                    best_j[q] = j0 + jj;
                }
            }
        }
    }
#pragma unroll
    for (int q = 0; q < PROP_ROWS / 4; ++q) {
        float w = best_w[q];
        int j = best_j[q];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ow = __shfl_xor(w, off);
            const int oj = __shfl_xor(j, off);
            if (ow > w || (ow == w && oj < j)) {
                w = ow;
                j = oj;
            }
        }
        const int i = i_blk + wave * (PROP_ROWS / 4) + q;
        if (lane == 0 && i >= nl && i < ns) {
            max_sim[(long)b * Kmax + i] = w;
            src_idx[(long)b * Kmax + i] = j;
            if (w > thr)
                for (int c = 0; c < C; ++c)
                    y_all[((long)b * Kmax + i) * C + c] = sp_labels[((long)b * Kmax + j) * C + c];
        }
    }
}
__global__ __launch_bounds__(256) void prop_kernel(const float* __restrict__ feat, const float* __restrict__ sp_labels,
                                                   const int32_t* __restrict__ n_sp, const int32_t* __restrict__ n_l,
                                                   float thr, int enable, float* __restrict__ y_all, int32_t* __restrict__ src_idx,
                                                   float* __restrict__ max_sim, int Kmax, int D, int C,
                                                   const float* __restrict__ Wc, const float* __restrict__ bc,
                                                   float* __restrict__ pred) {
    extern __shared__ float sh[];
    prop_body<false>(sh, feat, sp_labels, n_sp, n_l, thr, enable, y_all, src_idx, max_sim, Kmax, D, C, Wc, bc, pred);
}
__global__ __launch_bounds__(256) void prop_c_kernel(const float* __restrict__ feat, const float* __restrict__ sp_labels,
                                                     const int32_t* __restrict__ n_sp, const int32_t* __restrict__ n_l,
                                                     float thr, int enable, float* __restrict__ y_all, int32_t* __restrict__ src_idx,
                                                     float* __restrict__ max_sim, int Kmax, int D, int C,
                                                     const float* __restrict__ Wc, const float* __restrict__ bc,
                                                     float* __restrict__ pred) {
    extern __shared__ float sh[];
    prop_body<true>(sh, feat, sp_labels, n_sp, n_l, thr, enable, y_all, src_idx, max_sim, Kmax, D, C, Wc, bc, pred);
}
// The launch of the four entries below.  About that size first: WESUP_ERR_INVALID beyond the CU's LDS, the kernel's dynamic-LDS
// limit raised (once per kernel) where the default does not hold it.
template <bool GENERIC>
static int prop_launch(const float* feat, const float* Wc, const float* bc, float* pred, const float* sp_labels,
                       const int32_t* n_sp, const int32_t* n_l, float threshold, int enable, float* y_all, int32_t* src_idx,
                       float* max_sim, int B, int Kmax, int D, int C, void* stream) {
    constexpr auto kernel = GENERIC ? prop_c_kernel : prop_kernel;
    const size_t lds = prop_lds_bytes(D);
    if (lds > PROP_LDS_MAX) return WESUP_ERR_INVALID;
    if (lds > PROP_LDS_DEFAULT) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                                           hipFuncAttributeMaxDynamicSharedMemorySize, PROP_LDS_MAX);
        if (attr != hipSuccess) return WESUP_ERR_LAUNCH;
    }
    WESUP_LAUNCH(kernel, dim3(ceil_div(Kmax, PROP_ROWS), B), dim3(256), lds, (hipStream_t)stream, feat, sp_labels, n_sp, n_l,
                 threshold, enable, y_all, src_idx, max_sim, Kmax, D, C, Wc, bc, pred);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
extern "C" int wesup_propagate(const float* feat, const float* sp_labels, const int32_t* n_sp, const int32_t* n_l,
                               float threshold, int enable, float* y_all, int32_t* src_idx, float* max_sim, int B,
                               int Kmax, int D, int C, void* stream) {
    if (!feat || !sp_labels || !n_sp || !n_l || !y_all || !src_idx || !max_sim || B <= 0 || Kmax <= 0 || D <= 0 ||
        D > WESUP_HEAD_MAX_D || C <= 0)
        return WESUP_ERR_INVALID;
    return prop_launch<false>(feat, nullptr, nullptr, nullptr, sp_labels, n_sp, n_l, threshold, enable, y_all, src_idx, max_sim, B,
                              Kmax, D, C, stream);
}
// classifier + softmax (wesup_classifier_fwd_c) and label propagation (wesup_propagate) of the same features in ONE launch: both
// read feat, neither reads the other's result.  Bit-identical to the two entries.  wesup_head_fwd: pred (B*Kmax, 2), labels of any
// width C; wesup_head_fwd_c: pred (B*Kmax, C), and prop_kernel again where C = 2.
extern "C" int wesup_head_fwd(const float* feat, const float* Wc, const float* bc, float* pred, const float* sp_labels,
                              const int32_t* n_sp, const int32_t* n_l, float threshold, int enable, float* y_all,
                              int32_t* src_idx, float* max_sim, int B, int Kmax, int D, int C, void* stream) {
    if (!feat || !Wc || !bc || !pred || !sp_labels || !n_sp || !n_l || !y_all || !src_idx || !max_sim || B <= 0 || Kmax <= 0 ||
        D <= 0 || D > WESUP_HEAD_MAX_D || C <= 0)
        return WESUP_ERR_INVALID;
    return prop_launch<false>(feat, Wc, bc, pred, sp_labels, n_sp, n_l, threshold, enable, y_all, src_idx, max_sim, B, Kmax, D, C,
                              stream);
}
extern "C" int wesup_head_fwd_c(const float* feat, const float* Wc, const float* bc, float* pred, const float* sp_labels,
                                const int32_t* n_sp, const int32_t* n_l, float threshold, int enable, float* y_all,
                                int32_t* src_idx, float* max_sim, int B, int Kmax, int D, int C, void* stream) {
    if (!feat || !Wc || !bc || !pred || !sp_labels || !n_sp || !n_l || !y_all || !src_idx || !max_sim || B <= 0 || Kmax <= 0 ||
        D <= 0 || D > WESUP_HEAD_MAX_D || !cls_c_range(C))
        return WESUP_ERR_INVALID;
    return (C == 2 ? prop_launch<false> : prop_launch<true>)(feat, Wc, bc, pred, sp_labels, n_sp, n_l, threshold, enable, y_all,
                                                             src_idx, max_sim, B, Kmax, D, C, stream);
}

// ------------------------------------------------------------------ loss (models/wesup.py:66-96, 492-531)
__device__ __forceinline__ float ce_row(const float* p, const float* y, int C, float eps, float* ysum,
                                        const float* cw = nullptr) {
    float s = 0.f, ys = 0.f;
    for (int c = 0; c < C; ++c) {
        const float yc = y[c];
        ys += yc;
        // torch.clamp keeps a NaN (models/wesup.py:83), fminf/fmaxf would swallow it and a NaN prediction would end
        // in a finite loss instead of the ValueError of models/base.py:202-203
        const float pc = (p[c] != p[c]) ? p[c] : fminf(fmaxf(p[c], eps), 1.f - eps);
        const float ce = -yc * logf(pc);
        s += cw ? ce * cw[c] : ce;               // models/wesup.py:93-94
    }
    *ysum = ys;
    return s;
}
__global__ __launch_bounds__(256) void loss_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ y_all,
                                                       const int32_t* __restrict__ n_sp, const int32_t* __restrict__ n_l,
                                                       float eps, float prop_weight, float* __restrict__ terms, int Kmax,
                                                       int C) {
    __shared__ float sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int ns = n_sp[b], nl = n_l[b];
    float sup = 0.f, supc = 0.f, pro = 0.f, proc = 0.f, plab = 0.f;
    for (int r = tid; r < ns; r += 256) {
        float ys;
        const float ce = ce_row(pred + ((long)b * Kmax + r) * C, y_all + ((long)b * Kmax + r) * C, C, eps, &ys);
        if (r < nl) {
            sup += ce;
            supc += (ys > 0.f) ? 1.f : 0.f;
        } else {
            pro += ce;
            proc += (ys > 0.f) ? 1.f : 0.f;
            plab += ys;
        }
    }
    sup = block_sum256(sup, sh);
    supc = block_sum256(supc, sh);
    pro = block_sum256(pro, sh);
    proc = block_sum256(proc, sh);
    plab = block_sum256(plab, sh);
    if (tid == 0) {
        float l = (supc > 0.f) ? sup / supc : 0.f;
        if (nl < ns && proc > 0.f) l += prop_weight * (pro / proc);
        float* t = terms + (long)b * 8;
        t[0] = sup; t[1] = supc; t[2] = pro; t[3] = proc; t[4] = plab; t[5] = l; t[6] = 0.f; t[7] = 0.f;
    }
}
__global__ void loss_mean_kernel(const float* __restrict__ terms, float* __restrict__ loss, int B) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float s = 0.f;
        for (int b = 0; b < B; ++b) s += terms[(long)b * 8 + 5];
        loss[0] = s / (float)B;
    }
}
extern "C" int wesup_loss_fwd(const float* pred, const float* y_all, const int32_t* n_sp, const int32_t* n_l, float eps,
                              float prop_weight, float* terms, float* loss, int B, int Kmax, int C, void* stream) {
    if (!pred || !y_all || !n_sp || !n_l || !terms || B <= 0 || Kmax <= 0 || C <= 0) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    WESUP_LAUNCH(loss_fwd_kernel, dim3(B), dim3(256), 0, st, pred, y_all, n_sp, n_l, eps, prop_weight, terms, Kmax, C);
    // (loss == NULL: the caller forms the mean of terms[b][5] itself -- the step runner does, on the host, from the block it
    // reads back anyway: one launch less on the chain between forward and backward)
    if (loss) WESUP_LAUNCH(loss_mean_kernel, dim3(1), dim3(64), 0, st, (const float*)terms, loss, B);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
// d loss / d pred: -y/p where eps <= p <= 1-eps (torch.clamp passes the gradient on the closed interval)
__global__ void loss_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ y_all,
                                const int32_t* __restrict__ n_sp, const int32_t* __restrict__ n_l,
                                const float* __restrict__ terms, const float* __restrict__ dloss, float eps,
                                float prop_weight, float* __restrict__ dpred, int B, int Kmax, int C, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long br = idx / C;
    const int b = br / Kmax, r = br - (long)b * Kmax;
    const int ns = n_sp[b], nl = n_l[b];
    float g = 0.f;
    if (r < ns) {
        const float* t = terms + (long)b * 8;
        float coef;
        if (r < nl) coef = (t[1] > 0.f) ? 1.f / t[1] : 0.f;
        else coef = (nl < ns && t[3] > 0.f) ? prop_weight / t[3] : 0.f;
        const float p = pred[idx];
        if (p >= eps && p <= 1.f - eps) g = dloss[0] * (1.f / (float)B) * coef * (-y_all[idx] / p);
    }
    dpred[idx] = g;
}
extern "C" int wesup_loss_bwd(const float* pred, const float* y_all, const int32_t* n_sp, const int32_t* n_l,
                              const float* terms, const float* dloss, float eps, float prop_weight, float* dpred, int B,
                              int Kmax, int C, void* stream) {
    if (!pred || !y_all || !n_sp || !n_l || !terms || !dloss || !dpred || B <= 0 || Kmax <= 0 || C <= 0)
        return WESUP_ERR_INVALID;
    const long total = (long)B * Kmax * C;
    WESUP_LAUNCH(loss_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, pred,
                       y_all, n_sp, n_l, terms, dloss, eps, prop_weight, dpred, B, Kmax, C, total);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

// Loss, its gradient and the classifier's backward in ONE launch (wesup_loss_fwd + wesup_loss_bwd + wesup_classifier_bwd_c's first
// kernel: three launches on the chain between the fc layers' forward and backward).  A block owns CLS_ROWS = 64 rows of one image
// (Kmax % 64 == 0).  The per-image sums the gradient needs are a reduction over the whole image: every block of an image forms
// them ITSELF, with loss_fwd_kernel's loop and tree -- the same numbers in every block, no hand-off between blocks; the image's
// first block writes them to terms.  Then dpred of the block's rows (loss_bwd_kernel's expression) and classifier_bwd_c_kernel's
// body on them.  Bit-identical to the three entries.  (The body of head_bwd_kernel, CT = 2, and of head_bwd_c_kernel, CT = 0.)
template <int CT>
__device__ __forceinline__ void head_bwd_body(float* sh, float (*dz)[cls_dz_width(CT)], const float* __restrict__ feat,
                                              const float* __restrict__ Wc, const float* __restrict__ pred,
                                              const float* __restrict__ y_all, const int32_t* __restrict__ n_sp,
                                              const int32_t* __restrict__ n_l, const float* __restrict__ dloss, float eps,
                                              float prop_weight, float* __restrict__ terms, float* __restrict__ dpred,
                                              float* __restrict__ dfeat, float* __restrict__ part, int B, int Kmax, int D,
                                              int C_rt) {
    const int C = CT ? CT : C_rt;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * CLS_ROWS;                 // first row (of B * Kmax, an int) of this block
    const int b = r0 / Kmax, i0 = r0 - b * Kmax;
    const int ns = n_sp[b], nl = n_l[b];
    float sup = 0.f, supc = 0.f, pro = 0.f, proc = 0.f, plab = 0.f;
    for (int r = tid; r < ns; r += 256) {
        float ys;
        const float ce = ce_row(pred + ((long)b * Kmax + r) * C, y_all + ((long)b * Kmax + r) * C, C, eps, &ys);
        if (r < nl) {
            sup += ce;
            supc += (ys > 0.f) ? 1.f : 0.f;
        } else {
            pro += ce;
            proc += (ys > 0.f) ? 1.f : 0.f;
            plab += ys;
        }
    }
    sup = block_sum256(sup, sh);
    supc = block_sum256(supc, sh);
    pro = block_sum256(pro, sh);
    proc = block_sum256(proc, sh);
    plab = block_sum256(plab, sh);
    if (tid == 0 && i0 == 0) {
        float l = (supc > 0.f) ? sup / supc : 0.f;
        if (nl < ns && proc > 0.f) l += prop_weight * (pro / proc);
        float* t = terms + (long)b * 8;
        t[0] = sup; t[1] = supc; t[2] = pro; t[3] = proc; t[4] = plab; t[5] = l; t[6] = 0.f; t[7] = 0.f;
    }
    // dpred of the block's rows, then dz = p * (dp - sum_c dp_c p_c)
    if (tid < CLS_ROWS) {
        const int r = i0 + tid;                           // row inside the image (< Kmax)
        const long gr = (long)r0 + tid;
        float coef = 0.f;
        if (r < ns) {
            if (r < nl) coef = (supc > 0.f) ? 1.f / supc : 0.f;
            else coef = (nl < ns && proc > 0.f) ? prop_weight / proc : 0.f;
        }
        // (p and y of every class are read whatever the tests say, and dpred is stored behind the loop: the loads of a row go out
        // together, not one round trip to memory after the other)
        for (int c = 0; c < C; ++c) {
            const float p = pred[gr * C + c], y = y_all[gr * C + c];
            const float g = dloss[0] * (1.f / (float)B) * coef * (-y / p);
            dz[tid][c] = (r < ns && p >= eps && p <= 1.f - eps) ? g : 0.f;
        }
        for (int c = 0; c < C; ++c) dpred[gr * C + c] = dz[tid][c];
        cls_dz_row(pred + gr * C, dz[tid], C);
    }
    __syncthreads();
    cls_bwd_tail<CT>(feat, Wc, nullptr, dfeat, part, dz, r0, CLS_ROWS, D, C);   // (Kmax % CLS_ROWS == 0: every row exists)
}
// (plain kernels under the names a recorded step holds)
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ feat, const float* __restrict__ Wc,
                                                       const float* __restrict__ pred, const float* __restrict__ y_all,
                                                       const int32_t* __restrict__ n_sp, const int32_t* __restrict__ n_l,
                                                       const float* __restrict__ dloss, float eps, float prop_weight,
                                                       float* __restrict__ terms, float* __restrict__ dpred,
                                                       float* __restrict__ dfeat, float* __restrict__ part, int B, int Kmax,
                                                       int D) {
    __shared__ float sh[256];
    __shared__ float dz[CLS_ROWS][2];
    head_bwd_body<2>(sh, dz, feat, Wc, pred, y_all, n_sp, n_l, dloss, eps, prop_weight, terms, dpred, dfeat, part, B, Kmax, D, 2);
}
__global__ __launch_bounds__(256) void head_bwd_c_kernel(const float* __restrict__ feat, const float* __restrict__ Wc,
                                                         const float* __restrict__ pred, const float* __restrict__ y_all,
                                                         const int32_t* __restrict__ n_sp, const int32_t* __restrict__ n_l,
                                                         const float* __restrict__ dloss, float eps, float prop_weight,
                                                         float* __restrict__ terms, float* __restrict__ dpred,
                                                         float* __restrict__ dfeat, float* __restrict__ part, int B, int Kmax,
                                                         int D, int C) {
    __shared__ float sh[256];
    __shared__ float dz[CLS_ROWS][WESUP_MAX_CLASSES];
    head_bwd_body<0>(sh, dz, feat, Wc, pred, y_all, n_sp, n_l, dloss, eps, prop_weight, terms, dpred, dfeat, part, B, Kmax, D, C);
}
// ws: wesup_classifier_bwd_c_workspace_bytes(B * Kmax, D, C); it holds the per-block partial sums of the classifier's weight
// gradient until wesup_classifier_bwd_c_finish adds them up (any stream behind this launch: nothing on the way to the fc layers'
// gradients reads dWc / dbc).
extern "C" int wesup_head_bwd_c(const float* feat, const float* Wc, const float* pred, const float* y_all, const int32_t* n_sp,
                                const int32_t* n_l, const float* dloss, float eps, float prop_weight, float* terms, float* dpred,
                                float* dfeat, int B, int Kmax, int D, int C, void* ws, size_t ws_bytes, void* stream) {
    if (!feat || !Wc || !pred || !y_all || !n_sp || !n_l || !dloss || !terms || !dpred || !dfeat || !ws || B <= 0 || Kmax <= 0 ||
        (Kmax % CLS_ROWS) || D <= 0 || !cls_c_range(C))
        return WESUP_ERR_INVALID;
    const int R = B * Kmax;
    if (ws_bytes < wesup_classifier_bwd_c_workspace_bytes(R, D, C)) return WESUP_ERR_WORKSPACE;
    const dim3 grid(R / CLS_ROWS);
    hipStream_t st = (hipStream_t)stream;
    if (C == 2)
        WESUP_LAUNCH(head_bwd_kernel, grid, dim3(256), 0, st, feat, Wc, pred, y_all, n_sp, n_l, dloss, eps, prop_weight, terms,
                     dpred, dfeat, (float*)ws, B, Kmax, D);
    else
        WESUP_LAUNCH(head_bwd_c_kernel, grid, dim3(256), 0, st, feat, Wc, pred, y_all, n_sp, n_l, dloss, eps, prop_weight, terms,
                     dpred, dfeat, (float*)ws, B, Kmax, D, C);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
extern "C" int wesup_classifier_bwd_c_finish(const void* ws, size_t ws_bytes, float* dWc, float* dbc, int R, int D, int C,
                                             void* stream) {
    if (!ws || !dWc || !dbc || R <= 0 || D <= 0 || !cls_c_range(C)) return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_classifier_bwd_c_workspace_bytes(R, D, C)) return WESUP_ERR_WORKSPACE;
    cls_reduce_launch(ws, dWc, dbc, R, D, C, (hipStream_t)stream);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
// two classes: the _c entries with C = 2
extern "C" int wesup_head_bwd(const float* feat, const float* Wc, const float* pred, const float* y_all, const int32_t* n_sp,
                              const int32_t* n_l, const float* dloss, float eps, float prop_weight, float* terms, float* dpred,
                              float* dfeat, int B, int Kmax, int D, int C, void* ws, size_t ws_bytes, void* stream) {
    if (C != 2) return WESUP_ERR_INVALID;
    return wesup_head_bwd_c(feat, Wc, pred, y_all, n_sp, n_l, dloss, eps, prop_weight, terms, dpred, dfeat, B, Kmax, D, 2, ws,
                            ws_bytes, stream);
}
extern "C" int wesup_classifier_bwd_finish(const void* ws, size_t ws_bytes, float* dWc, float* dbc, int R, int D, void* stream) {
    return wesup_classifier_bwd_c_finish(ws, ws_bytes, dWc, dbc, R, D, 2, stream);
}

// generic _cross_entropy on (n, C)
__global__ __launch_bounds__(256) void ce_fwd_kernel(const float* __restrict__ y_hat, const float* __restrict__ y_true,
                                                     const float* __restrict__ cw, float eps, float* __restrict__ out2,
                                                     int n, int C) {
    __shared__ float sh[256];
    float s = 0.f, cnt = 0.f;
    for (int r = threadIdx.x; r < n; r += 256) {
        float ys;
        s += ce_row(y_hat + (long)r * C, y_true + (long)r * C, C, eps, &ys, cw);
        cnt += (ys > 0.f) ? 1.f : 0.f;
    }
    s = block_sum256(s, sh);
    cnt = block_sum256(cnt, sh);
    if (threadIdx.x == 0) {
        out2[0] = s;
        out2[1] = cnt;
        out2[2] = (cnt > 0.f) ? s / cnt : 0.f;      // models/wesup.py:88-96
        out2[3] = 0.f;
    }
}
__global__ void ce_bwd_kernel(const float* __restrict__ y_hat, const float* __restrict__ y_true,
                              const float* __restrict__ cw, const float* __restrict__ out2,
                              const float* __restrict__ dloss, float eps, float* __restrict__ dy, long total, int C) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const float cnt = out2[1];
    const float p = y_hat[idx];
    float g = 0.f;
    if (cnt > 0.f && p >= eps && p <= 1.f - eps) g = dloss[0] * (-y_true[idx] / p) / cnt;
    if (cw) g *= cw[idx % C];
    dy[idx] = g;
}
extern "C" int wesup_cross_entropy_fwd(const float* y_hat, const float* y_true, const float* class_weights, float eps,
                                       float* out2, int n, int C, void* stream) {
    if (!y_hat || !y_true || !out2 || n < 0 || C <= 0) return WESUP_ERR_INVALID;
    WESUP_LAUNCH(ce_fwd_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, y_hat, y_true, class_weights, eps, out2,
                       n, C);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
extern "C" int wesup_cross_entropy_bwd(const float* y_hat, const float* y_true, const float* class_weights,
                                       const float* out2, const float* dloss, float eps, float* dy_hat, int n, int C,
                                       void* stream) {
    if (!y_hat || !y_true || !out2 || !dloss || !dy_hat || n <= 0 || C <= 0) return WESUP_ERR_INVALID;
    const long total = (long)n * C;
    WESUP_LAUNCH(ce_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, y_hat,
                       y_true, class_weights, out2, dloss, eps, dy_hat, total, C);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

// ------------------------------------------------------------------ SGD with momentum + weight decay
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ v, size_t n, float lr,
                           float mu, float wd, float gs, int first) {
    const size_t n4 = n / 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pp = ld4(p + 4 * i);
        const float4 gg = ld4(g + 4 * i);
        float4 vv = first ? make_float4(0.f, 0.f, 0.f, 0.f) : ld4(v + 4 * i);
        const float gx = gg.x * gs + wd * pp.x, gy = gg.y * gs + wd * pp.y;
        const float gz = gg.z * gs + wd * pp.z, gw = gg.w * gs + wd * pp.w;
        vv.x = first ? gx : mu * vv.x + gx;
        vv.y = first ? gy : mu * vv.y + gy;
        vv.z = first ? gz : mu * vv.z + gz;
        vv.w = first ? gw : mu * vv.w + gw;
        pp.x -= lr * vv.x;
        pp.y -= lr * vv.y;
        pp.z -= lr * vv.z;
        pp.w -= lr * vv.w;
        st4(v + 4 * i, vv);
        st4(p + 4 * i, pp);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = n4 * 4 + threadIdx.x;
        const float gi = g[i] * gs + wd * p[i];
        const float vi = first ? gi : mu * v[i] + gi;
        v[i] = vi;
        p[i] -= lr * vi;
    }
}
extern "C" int wesup_sgd_step(float* p, const float* g, float* v, size_t n, float lr, float momentum, float weight_decay,
                              float grad_scale, int first_step, void* stream) {
    if (!p || !g || !v || n == 0) return WESUP_ERR_INVALID;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)v) & 15) return WESUP_ERR_INVALID;
    const size_t n4 = n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    WESUP_LAUNCH(sgd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, v, n, lr, momentum,
                       weight_decay, grad_scale, first_step);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

// ------------------------------------------------------------------ accuracy / dice sums
// SEG_BLOCKS blocks per image write partial sums; a second tiny kernel adds them in a fixed order.
#define SEG_BLOCKS 64
__global__ __launch_bounds__(256) void seg_metrics_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ mask,
                                                          float* __restrict__ part, int HW, int C) {
    __shared__ float sh[256];
    const int b = blockIdx.y;
    float eq = 0.f, pg = 0.f, sp = 0.f, sg = 0.f;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += SEG_BLOCKS * 256) {
        const float P = rintf(pred[(long)b * HW + p]);        // round half to even, as torch.round
        int gi = 0;
        uint8_t best = mask[((long)b * C) * HW + p];
        for (int c = 1; c < C; ++c) {
            const uint8_t v = mask[((long)b * C + c) * HW + p];
            if (v > best) { best = v; gi = c; }
        }
        const float G = (float)gi;
        eq += (P == G) ? 1.f : 0.f;
        pg += P * G;
        sp += P;
        sg += G;
    }
    eq = block_sum256(eq, sh);
    pg = block_sum256(pg, sh);
    sp = block_sum256(sp, sh);
    sg = block_sum256(sg, sh);
    if (threadIdx.x == 0) {
        float* o = part + ((long)b * SEG_BLOCKS + blockIdx.x) * 4;
        o[0] = eq; o[1] = pg; o[2] = sp; o[3] = sg;
    }
}
__global__ void seg_metrics_reduce(const float* __restrict__ part, float* __restrict__ out4, int B) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * 4) return;
    const int b = idx >> 2, k = idx & 3;
    float s = 0.f;
    for (int i = 0; i < SEG_BLOCKS; ++i) s += part[((long)b * SEG_BLOCKS + i) * 4 + k];
    out4[idx] = s;
}
extern "C" size_t wesup_seg_metrics_workspace_bytes(int B) { return B > 0 ? (size_t)B * SEG_BLOCKS * 4 * sizeof(float) : 0; }
extern "C" int wesup_seg_metrics(const float* pred, const uint8_t* mask, float* out4, int B, int HW, int C, void* ws,
                                 size_t ws_bytes, void* stream) {
    if (!pred || !mask || !out4 || !ws || B <= 0 || HW <= 0 || C <= 0) return WESUP_ERR_INVALID;
    if (ws_bytes < (size_t)B * SEG_BLOCKS * 4 * sizeof(float)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    WESUP_LAUNCH(seg_metrics_kernel, dim3(SEG_BLOCKS, B), dim3(256), 0, st, pred, mask, (float*)ws, HW, C);
    WESUP_LAUNCH(seg_metrics_reduce, dim3(ceil_div(B * 4, 64)), dim3(64), 0, st, (const float*)ws, out4, B);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

// ------------------------------------------------------------------ class maps and their confusion table (more than two classes)
// paint: the index of a superpixel's largest probability (the first maximum: ties go to the lowest class), once per superpixel
// row into ws, then one gather per pixel -- C is not scanned per pixel.
__global__ void row_argmax_kernel(const float* __restrict__ sp_pred, float* __restrict__ cls, long rows, int C) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const float* p = sp_pred + r * C;
    float best = p[0];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
        const float v = p[c];
        if (v > best) { best = v; bi = c; }
    }
    cls[r] = (float)bi;
}
__global__ void paint_rows_kernel(const float* __restrict__ cls, const int32_t* __restrict__ new_row, float* __restrict__ pred,
                                  long HW, int Kmax, long total) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const long b = idx / HW;
    pred[idx] = cls[b * Kmax + new_row[idx]];
}
extern "C" size_t wesup_paint_argmax_workspace_bytes(int B, int Kmax) {
    return (B > 0 && Kmax > 0) ? (size_t)B * Kmax * sizeof(float) : 0;
}
extern "C" int wesup_paint_argmax(const float* sp_pred, const int32_t* new_row, float* pred, int B, int HW, int Kmax, int C,
                                  void* ws, size_t ws_bytes, void* stream) {
    if (!sp_pred || !new_row || !pred || !ws || B <= 0 || HW <= 0 || Kmax <= 0 || !cls_c_range(C)) return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_paint_argmax_workspace_bytes(B, Kmax)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long rows = (long)B * Kmax, total = (long)B * HW;
    WESUP_LAUNCH(row_argmax_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, sp_pred, (float*)ws, rows, C);
    WESUP_LAUNCH(paint_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)ws, new_row, pred,
                 (long)HW, Kmax, total);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
// conf[b][g][p]: pixels of image b with ground-truth class g (the first maximum over the mask's C planes, as seg_metrics_kernel)
// and predicted class p.  Integer counts: a block adds its pixels up in LDS, then adds its table to the image's -- integer sums
// do not depend on the order.  The entry zeroes conf and status itself.  A predicted value outside [0, C) sets status.
__global__ __launch_bounds__(256) void seg_confusion_kernel(const float* __restrict__ pred, const uint8_t* __restrict__ mask,
                                                            int32_t* __restrict__ conf, int32_t* __restrict__ status, int HW,
                                                            int C) {
    __shared__ int32_t tab[WESUP_MAX_CLASSES * WESUP_MAX_CLASSES];
    const int b = blockIdx.y;
    if (threadIdx.x < C * C) tab[threadIdx.x] = 0;
    __syncthreads();
    for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += SEG_BLOCKS * 256) {
        const float P = rintf(pred[(long)b * HW + p]);
        int gi = 0;
        uint8_t best = mask[((long)b * C) * HW + p];
        for (int c = 1; c < C; ++c) {
            const uint8_t v = mask[((long)b * C + c) * HW + p];
            if (v > best) { best = v; gi = c; }
        }
        if (P >= 0.f && P < (float)C) atomicAdd(&tab[gi * C + (int)P], 1);
        else atomicOr(status, 1);                 // (a NaN lands here too)
    }
    __syncthreads();
    if (threadIdx.x < C * C && tab[threadIdx.x] != 0) atomicAdd(&conf[(long)b * C * C + threadIdx.x], tab[threadIdx.x]);
}
extern "C" int wesup_seg_confusion(const float* pred, const uint8_t* mask, int32_t* conf, int32_t* status, int B, int HW, int C,
                                   void* stream) {
    if (!pred || !mask || !conf || !status || B <= 0 || HW <= 0 || !cls_c_range(C)) return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    int rc = wesup_fill_words_(conf, 0u, (size_t)B * C * C, st);
    if (rc == WESUP_OK) rc = wesup_fill_words_(status, 0u, 1, st);
    if (rc != WESUP_OK) return rc;
    WESUP_LAUNCH(seg_confusion_kernel, dim3(SEG_BLOCKS, B), dim3(256), 0, st, pred, mask, conf, status, HW, C);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

// ------------------------------------------------------------------ misc
extern "C" int wesup_abi_version(void) { return 6; }
extern "C" const char* wesup_strerror(int code) {
    switch (code) {
        case WESUP_OK: return "ok";
        case WESUP_ERR_INVALID: return "invalid argument (shape, alignment or null pointer)";
        case WESUP_ERR_LAUNCH: return "HIP kernel launch failed";
        case WESUP_ERR_WORKSPACE: return "workspace too small";
        default: return "unknown error";
    }
}
