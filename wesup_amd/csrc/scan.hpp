// The exclusive prefix scan of the device library, stated once: the scan of one block in LDS, and the bodies of
// the device-wide scan in three launches -- every block's total, one block that scans the totals, and an apply pass that rescans
// its block and adds the block's offset.  The kernels stay where they are (slic.hip, regions.hip, contour.hip, measure.hip,
// raster.hip; superpixel.hip uses the block scan alone) under their own names: pointer set-up, the gate, the call, the store of
// the total.
//
// N is the block size: blockDim.x == N, a multiple of 64, and the block of a pass is blockIdx.x.  Every function here holds
// barriers, so ALL N threads of a block reach it or none does: a caller's gate (a header word) and its batch offset (blockIdx.y)
// are the same for the whole block, and both come before the call.  Elements past n read as 0 and are never stored.
// All of it is in namespace scan: slic.hip's kernels are called scan_block_sums and scan_apply themselves.
#pragma once
#include "common.hpp"

namespace scan {

// Exclusive scan of N values, one per thread, over sh[N] (Hillis-Steele); the sum of all N in *total.  The last barrier frees sh
// for the next call.
template <typename T, int N>
__device__ __forceinline__ T block_scan(T v, T* sh, T* total) {
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int off = 1; off < N; off <<= 1) {
        const T t = (tid >= off) ? sh[tid - off] : (T)0;
        __syncthreads();
        sh[tid] += t;
        __syncthreads();
    }
    const T incl = sh[tid];
    *total = sh[N - 1];
    __syncthreads();
    return incl - v;
}

// Pass 1: the sum of load(i) over the block's N elements i < n, valid in thread 0 only.  Wave shuffles, then N / 64 words of LDS.
template <typename T, int N, typename Load>
__device__ __forceinline__ T scan_block_total(Load load, long n) {
    __shared__ T sh[N / 64];
    const int tid = threadIdx.x;
    const long i = (long)blockIdx.x * N + tid;
    T v = i < n ? load(i) : (T)0;
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if ((tid & 63) == 0) sh[tid >> 6] = v;
    __syncthreads();
    T s = 0;
    if (tid == 0)
        for (int w = 0; w < N / 64; ++w) s += sh[w];
    return s;
}

// Pass 2, one block: v[0 .. n) -> its exclusive scan in place, in rounds of N with a running carry; the sum of all n in *total
// (every thread).
template <typename T, int N>
__device__ __forceinline__ void scan_small(T* __restrict__ v, int n, T* total) {
    __shared__ T sh[N];
    T run = 0;
    for (int i0 = 0; i0 < n; i0 += N) {
        const int i = i0 + threadIdx.x;
        T tot;
        const T e = block_scan<T, N>(i < n ? v[i] : (T)0, sh, &tot);
        if (i < n) v[i] = run + e;
        run += tot;
    }
    *total = run;
}

// Pass 3: store(i, offset + the exclusive scan of load(.) inside the block) for the block's elements i < n; offset is the
// block's entry of the scanned totals.
template <typename T, int N, typename Load, typename Store>
__device__ __forceinline__ void scan_apply(Load load, Store store, T offset, long n) {
    __shared__ T sh[N];
    const long i = (long)blockIdx.x * N + threadIdx.x;
    T tot;
    const T e = block_scan<T, N>(i < n ? load(i) : (T)0, sh, &tot);
    if (i < n) store(i, offset + e);
}

}  // namespace scan
