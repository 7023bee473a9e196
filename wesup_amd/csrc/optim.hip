// Fused Adam / AdamW over the flat parameter buffer (torch.optim.Adam / AdamW without amsgrad), for a step that is recorded once
// and replayed: a recorded launch carries its scalar arguments as bytes, so whatever moves from step to step -- the count t,
// the bias corrections formed from it, the learning rate a scheduler changes -- lives in a 32-byte device block (AdamState)
// that one launch of the plan advances (adam_tick_kernel) and the update launches read.
//
//   tick:    t += 1;  step_size = lr / (1 - b1^t);  inv_sqrt_bc2 = 1 / sqrt(1 - b2^t);  decay = 1 - lr wd
//            -- in double, each rounded to float once, as torch forms them from Python floats
//   update:  g' = g gs;  Adam: g' += wd p;  AdamW: p *= decay;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g' g';
//            p -= step_size m / (sqrt(v) inv_sqrt_bc2 + eps)
//
// m and v start as zeros: no first-step case.  The update is elementwise and reads the block only: any split of the buffer
// into 16-byte aligned ranges behind one tick is the one launch, bit for bit.
#include "common.hpp"

struct alignas(16) AdamState {
    double lr;              // what the host pushes (optim.py push_hyper): the optimiser's lr as the double it is
    int t;                  // optimiser steps so far
    float step_size;        // lr / (1 - b1^t)
    float inv_sqrt_bc2;     // 1 / sqrt(1 - b2^t)
    float decay;            // 1 - lr wd (AdamW)
    int pad_[2];
};
static_assert(sizeof(AdamState) == 32, "the schedule state is 32 bytes (optim.py lays it out by hand)");

// b = 1 - (1 - b): the complements come in as floats rounded from the host's doubles, and 1 - b^t is made of them -- at t = 1 it
// IS the complement.  The float of b2 = 0.999 itself is off by 1.3e-8, i.e. by 1.3e-5 of 1 - b2.
__global__ __launch_bounds__(64) void adam_tick_kernel(AdamState* __restrict__ st, float omb1, float omb2, float wd) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const int t = st->t + 1;
    const double lr = st->lr;
    const double b1 = 1.0 - (double)omb1, b2 = 1.0 - (double)omb2;
    const double bc1 = 1.0 - pow(b1, (double)t), bc2 = 1.0 - pow(b2, (double)t);
    st->t = t;
    st->step_size = (float)(lr / bc1);
    st->inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    st->decay = (float)(1.0 - lr * (double)wd);
}

extern "C" int wesup_adam_tick(void* state, float one_minus_beta1, float one_minus_beta2, float weight_decay, void* stream) {
    if (!state || ((uintptr_t)state & 15)) return WESUP_ERR_INVALID;
    WESUP_LAUNCH(adam_tick_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, (AdamState*)state, one_minus_beta1,
                 one_minus_beta2, weight_decay);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}

struct AdamHyper {          // launch arguments: fixed over a run, part of a plan's signature (runner.py)
    float b1, omb1, b2, omb2, eps, wd, gs;
    int decoupled;
};
WESUP_NO_PADDING(AdamHyper, 32);

template <int DECOUPLED>
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamHyper& h, float step_size,
                                             float inv_sqrt_bc2, float decay) {
    g *= h.gs;
    if (DECOUPLED) p *= decay;
    else g += h.wd * p;
    m = h.b1 * m + h.omb1 * g;
    v = h.b2 * v + h.omb2 * g * g;
    p -= step_size * m / (sqrtf(v) * inv_sqrt_bc2 + h.eps);
}

// The shape of sgd_kernel (loss.hip): a float4 per thread and trip, at most 2048 blocks of 256 striding over n / 4, block 0
// finishes the n & 3 tail.  28 bytes per element: p, g, m, v in; p, m, v out.  The three factors sit at one address for the whole
// grid: uniform loads, once per thread.
template <int DECOUPLED>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, size_t n, const AdamState* __restrict__ st,
                                                   AdamHyper h) {
    const float step_size = st->step_size, inv_sqrt_bc2 = st->inv_sqrt_bc2, decay = st->decay;
    const size_t n4 = n / 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pp = ld4(p + 4 * i);
        const float4 gg = ld4(g + 4 * i);
        float4 mm = ld4(m + 4 * i);
        float4 vv = ld4(v + 4 * i);
        adam_element<DECOUPLED>(pp.x, gg.x, mm.x, vv.x, h, step_size, inv_sqrt_bc2, decay);
        adam_element<DECOUPLED>(pp.y, gg.y, mm.y, vv.y, h, step_size, inv_sqrt_bc2, decay);
        adam_element<DECOUPLED>(pp.z, gg.z, mm.z, vv.z, h, step_size, inv_sqrt_bc2, decay);
        adam_element<DECOUPLED>(pp.w, gg.w, mm.w, vv.w, h, step_size, inv_sqrt_bc2, decay);
        st4(m + 4 * i, mm);
        st4(v + 4 * i, vv);
        st4(p + 4 * i, pp);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const size_t i = n4 * 4 + threadIdx.x;
        float pi = p[i], mi = m[i], vi = v[i];
        adam_element<DECOUPLED>(pi, g[i], mi, vi, h, step_size, inv_sqrt_bc2, decay);
        m[i] = mi;
        v[i] = vi;
        p[i] = pi;
    }
}

extern "C" int wesup_adam_step(float* p, const float* g, float* m, float* v, size_t n, const void* state, float beta1,
                               float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float weight_decay,
                               float grad_scale, int decoupled, void* stream) {
    if (!p || !g || !m || !v || !state || n == 0) return WESUP_ERR_INVALID;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)state) & 15) return WESUP_ERR_INVALID;
    const size_t n4 = n / 4;
    size_t blocks = (n4 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    const AdamHyper h = {beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay, grad_scale, decoupled ? 1 : 0};
    const AdamState* st = (const AdamState*)state;
    if (decoupled)
        WESUP_LAUNCH(adam_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, st, h);
    else
        WESUP_LAUNCH(adam_kernel<0>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, st, h);
    WESUP_CHECK_LAUNCH();
    return WESUP_OK;
}
