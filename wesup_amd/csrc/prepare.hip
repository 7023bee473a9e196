// Weak-label preparation on the GPU: the integer label-map passes behind wesup_amd/prepare.py, the mirror of the
// reference's scripts/generate_points.py, generate_spl_masks.py and search_slic_params.py.
//   wesup_label_stats  pixel count and the sums of the row / column indexes of every label: the size and the centroid numerator
//                      of every region of an image in one pass (the scripts make one `mask == idx` + np.where pass per region);
//   wesup_sp_vote      per superpixel the sum and the count of a uint8 map, the rounded mean (half to even, in integers) painted
//                      back, and the number of pixels that keep their value -- run_param_group of search_slic_params.py;
//   wesup_spl_paint    out[h][w][c] = some point of class c lies in the superpixel of (h, w) -- generate_spl_masks.py.
// Integer data and integer arithmetic only: the results depend neither on the order of the atomics nor on the run.  Every kernel
// walks its image in a grid-stride loop with 64-bit pixel indexes; a label outside its table sets the image's status word and is
// skipped, never used as an index.
//
// Tables: a block adds into a private table in LDS when the table fits (PR_STATS_LDS_LABELS / PR_VOTE_LDS_IDS entries) and
// flushes its non-zero entries with one global atomic each; above that the adds go to global memory directly.  In both forms a
// thread walks a few consecutive pixels and adds a run of equal labels once (inside a region that is one add instead of eight).
#include "common.hpp"

#define PR_BLOCK 256
#define PR_STATS_PIX 8               // consecutive pixels per thread and stride of wesup_label_stats
#define PR_VOTE_PIX 4                // of wesup_sp_vote: one int4 of labels, one 32-bit word of values
#define PR_MAX_BLOCKS 1024           // blocks per image: bounds the flushes of the private tables
#define PR_STATS_LDS_LABELS 2048     // 3 x 64-bit counters per label: 48 KB
#define PR_VOTE_LDS_IDS 4096         // 2 x 32-bit counters per id: 32 KB
#define PR_MAX_SIDE (1 << 22)        // H, W: row / column sums of 2^40 pixels stay below 2^62
#define PR_MAX_TABLE (1l << 26)      // entries of a table (L + 1, K, K * C)

namespace {

typedef unsigned long long u64;

template <bool LDS>
__global__ __launch_bounds__(PR_BLOCK) void pr_stats_kernel(const int32_t* __restrict__ labels, u64* __restrict__ stats,
                                                            int32_t* __restrict__ status, long HW, int W, int L) {
    extern __shared__ u64 pr_tab64[];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = 3 * (L + 1);
    if (LDS) {
        for (int i = tid; i < n; i += PR_BLOCK) pr_tab64[i] = 0;
        __syncthreads();
    }
    const int32_t* lab = labels + (long)b * HW;
    u64* g = stats + (long)b * n;
    int bad = 0;
    const long step = (long)gridDim.x * PR_BLOCK * PR_STATS_PIX;
    for (long p0 = ((long)blockIdx.x * PR_BLOCK + tid) * PR_STATS_PIX; p0 < HW; p0 += step) {
        const long p1 = min(HW, p0 + PR_STATS_PIX);
        long row = p0 / W;
        int col = (int)(p0 - row * W);
        int key = -1;
        u64 cnt = 0, sr = 0, sc = 0;
        for (long p = p0; p < p1; ++p) {
            const int l = lab[p];
            if (l < 0 || l > L) bad = 1;
            else {
                if (l != key) {
                    if (cnt) {
                        u64* t = (LDS ? pr_tab64 : g) + 3 * key;
                        atomicAdd(t, cnt); atomicAdd(t + 1, sr); atomicAdd(t + 2, sc);
                    }
                    key = l;
                    cnt = sr = sc = 0;
                }
                ++cnt;
                sr += (u64)row;
                sc += (u64)col;
            }
            if (++col == W) { col = 0; ++row; }
        }
        if (cnt) {
            u64* t = (LDS ? pr_tab64 : g) + 3 * key;
            atomicAdd(t, cnt); atomicAdd(t + 1, sr); atomicAdd(t + 2, sc);
        }
    }
    if (bad) atomicOr(&status[b], 1);
    if (LDS) {
        __syncthreads();
        for (int i = tid; i < n; i += PR_BLOCK) {
            const u64 v = pr_tab64[i];
            if (v) atomicAdd(&g[i], v);
        }
    }
}

// tbl[b][k] = {sum of values, pixels} of superpixel k
template <bool LDS>
__global__ __launch_bounds__(PR_BLOCK) void pr_vote_sum_kernel(const int32_t* __restrict__ labels, const uint8_t* __restrict__ values,
                                                               uint32_t* __restrict__ tbl, int32_t* __restrict__ status, long HW,
                                                               int K, int vec) {
    extern __shared__ uint32_t pr_tab32[];
    const int b = blockIdx.y, tid = threadIdx.x;
    if (LDS) {
        for (int i = tid; i < 2 * K; i += PR_BLOCK) pr_tab32[i] = 0;
        __syncthreads();
    }
    const int32_t* lab = labels + (long)b * HW;
    const uint8_t* val = values + (long)b * HW;
    uint32_t* g = tbl + (long)b * 2 * K;
    int bad = 0;
    const long step = (long)gridDim.x * PR_BLOCK * PR_VOTE_PIX;
    for (long p0 = ((long)blockIdx.x * PR_BLOCK + tid) * PR_VOTE_PIX; p0 < HW; p0 += step) {
        int l[PR_VOTE_PIX];
        uint32_t v[PR_VOTE_PIX];
        int n = PR_VOTE_PIX;
        if (vec && p0 + PR_VOTE_PIX <= HW) {
            const int4 l4 = *reinterpret_cast<const int4*>(lab + p0);
            const uint32_t v4 = *reinterpret_cast<const uint32_t*>(val + p0);
            l[0] = l4.x; l[1] = l4.y; l[2] = l4.z; l[3] = l4.w;
#pragma unroll
            for (int i = 0; i < PR_VOTE_PIX; ++i) v[i] = (v4 >> (8 * i)) & 0xffu;
        } else {
            n = (int)min((long)PR_VOTE_PIX, HW - p0);
#pragma unroll
            for (int i = 0; i < PR_VOTE_PIX; ++i) {
                l[i] = i < n ? lab[p0 + i] : -1;
                v[i] = i < n ? val[p0 + i] : 0u;
            }
        }
        int key = -1;
        uint32_t cnt = 0, sum = 0;
#pragma unroll
        for (int i = 0; i < PR_VOTE_PIX; ++i) {
            if (i >= n) continue;
            if (l[i] < 0 || l[i] >= K) { bad = 1; continue; }
            if (l[i] != key) {
                if (cnt) {
                    uint32_t* t = (LDS ? pr_tab32 : g) + 2 * key;
                    atomicAdd(t, sum); atomicAdd(t + 1, cnt);
                }
                key = l[i];
                cnt = sum = 0;
            }
            ++cnt;
            sum += v[i];
        }
        if (cnt) {
            uint32_t* t = (LDS ? pr_tab32 : g) + 2 * key;
            atomicAdd(t, sum); atomicAdd(t + 1, cnt);
        }
    }
    if (bad) atomicOr(&status[b], 1);
    if (LDS) {
        __syncthreads();
        for (int i = tid; i < 2 * K; i += PR_BLOCK) {
            const uint32_t x = pr_tab32[i];
            if (x) atomicAdd(&g[i], x);
        }
    }
}

// tbl[b][k][0] = round-half-to-even(sum / count) in integers (numpy's mean().round() of uint8 values); an id without a pixel: 0
__global__ void pr_vote_round_kernel(uint32_t* __restrict__ tbl, long n) {
    const long step = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint32_t sum = tbl[2 * i], cnt = tbl[2 * i + 1];
        uint32_t q = 0;
        if (cnt) {
            q = sum / cnt;
            const u64 r2 = 2ull * (sum - q * cnt);
            if (r2 > cnt) ++q;
            else if (r2 == cnt) q += q & 1u;
        }
        tbl[2 * i] = q;
    }
}

// painted = the vote of the pixel's superpixel (painted may be NULL); agree[b] += pixels whose vote equals their value
__global__ __launch_bounds__(PR_BLOCK) void pr_vote_paint_kernel(const int32_t* __restrict__ labels,
                                                                 const uint8_t* __restrict__ values,
                                                                 const uint32_t* __restrict__ tbl, uint8_t* __restrict__ painted,
                                                                 u64* __restrict__ agree, long HW, int K, int vec) {
    __shared__ u64 wsum[PR_BLOCK / 64];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int32_t* lab = labels + (long)b * HW;
    const uint8_t* val = values + (long)b * HW;
    uint8_t* out = painted ? painted + (long)b * HW : nullptr;
    const uint32_t* t = tbl + (long)b * 2 * K;
    u64 same = 0;
    const long step = (long)gridDim.x * PR_BLOCK * PR_VOTE_PIX;
    for (long p0 = ((long)blockIdx.x * PR_BLOCK + tid) * PR_VOTE_PIX; p0 < HW; p0 += step) {
        if (vec && p0 + PR_VOTE_PIX <= HW) {
            const int4 l4 = *reinterpret_cast<const int4*>(lab + p0);
            const uint32_t v4 = *reinterpret_cast<const uint32_t*>(val + p0);
            const int l[PR_VOTE_PIX] = {l4.x, l4.y, l4.z, l4.w};
            uint32_t o4 = 0;
#pragma unroll
            for (int i = 0; i < PR_VOTE_PIX; ++i) {
                if (l[i] < 0 || l[i] >= K) continue;                // (reported by the sum kernel; painted 0, never agreeing)
                const uint32_t q = t[2 * l[i]];
                o4 |= q << (8 * i);
                same += q == ((v4 >> (8 * i)) & 0xffu);
            }
            if (out) *reinterpret_cast<uint32_t*>(out + p0) = o4;
        } else {
            const long p1 = min(HW, p0 + PR_VOTE_PIX);
            for (long p = p0; p < p1; ++p) {
                const int l = lab[p];
                uint32_t q = 0;
                if (l >= 0 && l < K) {
                    q = t[2 * l];
                    same += q == (uint32_t)val[p];
                }
                if (out) out[p] = (uint8_t)q;
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) same += __shfl_xor(same, off);
    if ((tid & 63) == 0) wsum[tid >> 6] = same;
    __syncthreads();
    if (tid == 0) {
        for (int i = 1; i < PR_BLOCK / 64; ++i) same += wsum[i];
        if (same) atomicAdd(&agree[b], same);
    }
}

// flags[k][c] = 1 for every point (row, col, class) in the superpixel k of its pixel; status |= 2 for a point outside the image
// or the classes, |= 1 for a label outside [0, K)
__global__ void pr_spl_flag_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ points,
                                   uint8_t* __restrict__ flags, int32_t* __restrict__ status, int H, int W, int K, int C, int P) {
    const int step = gridDim.x * blockDim.x;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P; i += step) {
        const int r = points[3 * i], c = points[3 * i + 1], cls = points[3 * i + 2];
        if (r < 0 || r >= H || c < 0 || c >= W || cls < 0 || cls >= C) { atomicOr(status, 2); continue; }
        const int l = labels[(long)r * W + c];
        if (l < 0 || l >= K) { atomicOr(status, 1); continue; }
        flags[(long)l * C + cls] = 1;                               // (every writer stores the same byte)
    }
}
__global__ __launch_bounds__(PR_BLOCK) void pr_spl_paint_kernel(const int32_t* __restrict__ labels,
                                                                const uint8_t* __restrict__ flags, uint8_t* __restrict__ out,
                                                                int32_t* __restrict__ status, long HW, int K, int C) {
    int bad = 0;
    const long step = (long)gridDim.x * PR_BLOCK;
    for (long p = (long)blockIdx.x * PR_BLOCK + threadIdx.x; p < HW; p += step) {
        const int l = labels[p];
        const bool ok = l >= 0 && l < K;
        if (!ok) bad = 1;
        for (int c = 0; c < C; ++c) out[p * C + c] = ok ? flags[(long)l * C + c] : (uint8_t)0;
    }
    if (bad) atomicOr(status, 1);
}

inline bool pr_bad_image(int B, int H, int W) {
    return B <= 0 || B > 65535 || H <= 0 || W <= 0 || H > PR_MAX_SIDE || W > PR_MAX_SIDE || (long)H * W > (1l << 40) ||
           (long)B * H * W > (1l << 40);
}
inline unsigned pr_blocks(long HW, int per_block) {
    const long n = (HW + per_block - 1) / per_block;
    return (unsigned)(n < PR_MAX_BLOCKS ? n : PR_MAX_BLOCKS);
}
// the counters of wesup_sp_vote are 32 bits wide: the largest sum is 255 per pixel
inline bool pr_bad_vote(int B, int H, int W, int K) {
    return pr_bad_image(B, H, W) || K <= 0 || K > PR_MAX_TABLE || 255l * H * W >= (1l << 32);
}
inline bool pr_bad_paint(int H, int W, int K, int C) {
    return pr_bad_image(1, H, W) || K <= 0 || C <= 0 || C > 256 || (long)K * C > PR_MAX_TABLE;
}

}  // namespace

extern "C" int wesup_prepare_lds_entries(int which) {
    return which == 0 ? PR_STATS_LDS_LABELS : which == 1 ? PR_VOTE_LDS_IDS : 0;
}

extern "C" int wesup_label_stats(const int32_t* labels, int64_t* stats, int32_t* status, int B, int H, int W, int L, void* stream) {
    if (!labels || !stats || !status || pr_bad_image(B, H, W) || L < 0 || L >= PR_MAX_TABLE || ((uintptr_t)stats & 7))
        return WESUP_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W;
    const int n = 3 * (L + 1);
    if (wesup_fill_words_(stats, 0u, (size_t)B * n * 2, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (wesup_fill_words_(status, 0u, (size_t)B, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    const dim3 grid(pr_blocks(HW, PR_BLOCK * PR_STATS_PIX), B);
    if (L + 1 <= PR_STATS_LDS_LABELS)
        WESUP_LAUNCH(pr_stats_kernel<true>, grid, dim3(PR_BLOCK), (size_t)n * 8, st, labels, (u64*)stats, status, HW, W, L);
    else
        WESUP_LAUNCH(pr_stats_kernel<false>, grid, dim3(PR_BLOCK), 0, st, labels, (u64*)stats, status, HW, W, L);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_sp_vote_workspace_bytes(int B, int H, int W, int K) {
    if (pr_bad_vote(B, H, W, K)) return 0;
    return align_up((size_t)B * K * 8, 256);                                    // {sum -> vote, count} per id
}

extern "C" int wesup_sp_vote(const int32_t* labels, const uint8_t* values, uint8_t* painted, int64_t* agree, int32_t* status, int B,
                             int H, int W, int K, void* ws, size_t ws_bytes, void* stream) {
    if (!labels || !values || !agree || !status || !ws || pr_bad_vote(B, H, W, K) || ((uintptr_t)agree & 7) || ((uintptr_t)ws & 3))
        return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_sp_vote_workspace_bytes(B, H, W, K)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W;
    uint32_t* tbl = (uint32_t*)ws;
    // one int4 of labels and one word of values / painted per step: every image has to start on such a boundary
    const int vec = (B == 1 || HW % PR_VOTE_PIX == 0) && !((uintptr_t)labels & 15) && !((uintptr_t)values & 3) &&
                    !((uintptr_t)painted & 3);
    if (wesup_fill_words_(tbl, 0u, (size_t)B * K * 2, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (wesup_fill_words_(agree, 0u, (size_t)B * 2, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (wesup_fill_words_(status, 0u, (size_t)B, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    const dim3 grid(pr_blocks(HW, PR_BLOCK * PR_VOTE_PIX), B);
    if (K <= PR_VOTE_LDS_IDS)
        WESUP_LAUNCH(pr_vote_sum_kernel<true>, grid, dim3(PR_BLOCK), (size_t)K * 8, st, labels, values, tbl, status, HW, K, vec);
    else
        WESUP_LAUNCH(pr_vote_sum_kernel<false>, grid, dim3(PR_BLOCK), 0, st, labels, values, tbl, status, HW, K, vec);
    const long ids = (long)B * K;
    WESUP_LAUNCH(pr_vote_round_kernel, dim3(pr_blocks(ids, PR_BLOCK)), dim3(PR_BLOCK), 0, st, tbl, ids);
    WESUP_LAUNCH(pr_vote_paint_kernel, grid, dim3(PR_BLOCK), 0, st, labels, values, (const uint32_t*)tbl, painted, (u64*)agree, HW,
                 K, vec);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

extern "C" size_t wesup_spl_paint_workspace_bytes(int K, int C) {
    if (K <= 0 || C <= 0 || C > 256 || (long)K * C > PR_MAX_TABLE) return 0;
    return align_up((size_t)K * C, 256);                                        // the flag table
}

extern "C" int wesup_spl_paint(const int32_t* labels, const int32_t* points, uint8_t* out, int32_t* status, int H, int W, int K,
                               int C, int P, void* ws, size_t ws_bytes, void* stream) {
    if (!labels || !out || !status || !ws || pr_bad_paint(H, W, K, C) || P < 0 || (P > 0 && !points) || ((uintptr_t)ws & 3))
        return WESUP_ERR_INVALID;
    if (ws_bytes < wesup_spl_paint_workspace_bytes(K, C)) return WESUP_ERR_WORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const long HW = (long)H * W;
    uint8_t* flags = (uint8_t*)ws;
    if (wesup_fill_words_(flags, 0u, align_up((size_t)K * C, 4) / 4, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (wesup_fill_words_(status, 0u, 1, st) != WESUP_OK) return WESUP_ERR_LAUNCH;
    if (P > 0)
        WESUP_LAUNCH(pr_spl_flag_kernel, dim3(pr_blocks(P, PR_BLOCK)), dim3(PR_BLOCK), 0, st, labels, points, flags, status, H, W, K,
                     C, P);
    WESUP_LAUNCH(pr_spl_paint_kernel, dim3(pr_blocks(HW, PR_BLOCK)), dim3(PR_BLOCK), 0, st, labels, (const uint8_t*)flags, out,
                 status, HW, K, C);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
