// Host side of wesup_sp_pool_mat_fwd / wesup_sp_pool_mat_bwd (superpixel.hip): which of the two routes a product of the
// interpolation-pooling matrix takes, and which operands the entries refuse.  Plain C++ (no HIP): tools/pool_mat_route_check.cpp
// compiles it on its own under the host sanitizers.
#pragma once
#include <cstdint>
#include <cstdlib>

// Size rule, on the matrix entries per image (Kmax * hw).  Wm[b][r][.] is the mean of <= 4 bilinear weights per pixel of
// superpixel r: a row has about (pixels of r) / (pixels per cell) + its rim non-zero cells, a column the 2 - 6 superpixels that
// touch the cell, and the dense GEMM multiplies the other > 99 % zeros.  The sparse route (one kernel that walks the non-zeros)
// costs one read of the matrix and one launch, so it wins wherever the GEMM is more than launch latency;
// profiles/pool_mat_micro.txt has both routes alone.  Two floors hold the bound up, whatever the micro-benchmark says:
//   - 16 384 entries, below which a product is a handful of 64 x 64 tiles and nothing is to be gained;
//   - the recorded 3 x 64 x 48 step, whose launch list is pinned node by node (tests/golden/plan_nodes_c2_64x48.json): its
//     superpixel tables are padded to Kmax = 64 rows, so its largest matrix is 64 rows x 32 * 24 cells = 49 152 entries, and
//     that product must stay on the GEMM launches.
// 65 536 is the next power of two above both.  WESUP_POOL_MAT_SPARSE_MIN moves the bound for the A/B (0: never sparse,
// 1: always); read at every call, not cached, so that one process can measure both routes.
#define WESUP_POOL_MAT_SPARSE_MIN_DEFAULT 65536l
static inline long pool_mat_sparse_min() {
    const char* e = getenv("WESUP_POOL_MAT_SPARSE_MIN");
    return e ? atol(e) : WESUP_POOL_MAT_SPARSE_MIN_DEFAULT;
}
static inline bool pool_mat_sparse(int Kmax, int hw) {
    const long bound = pool_mat_sparse_min();
    return bound > 0 && Kmax > 0 && hw > 0 && (long)Kmax * hw >= bound;
}

// What both routes need of the operands: s / ds are [B][hw][C] contiguous, the superpixel-side operand is the C channels at
// channel `off` of [B][Kmax][ld] rows.  (The GEMM route adds its own conditions -- Kmax, hw multiples of 4 -- in its entry.)
static inline bool pool_mat_operands_ok(const void* Wm, const void* WmT, const void* s, const void* sp, int ld, int off, int B,
                                        int Kmax, int hw, int C) {
    if (!Wm || !WmT || !s || !sp) return false;
    if (B <= 0 || B > 65535 || Kmax <= 0 || Kmax > (1 << 22) || hw <= 0 || hw > 8192 || C <= 0 || (C % 4)) return false;   // grids
    if (ld <= 0 || (ld % 4) || off < 0 || (off % 4) || (long)off + C > (long)ld) return false;       // the slice fits its row
    if ((((uintptr_t)s | (uintptr_t)sp) & 15) != 0) return false;                                      // 16-byte loads / stores
    return true;
}
