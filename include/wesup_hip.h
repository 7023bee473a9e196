/*
 * libwesup_hip.so -- C ABI of the MI355X (gfx950) WESUP training-step hot path.
 *
 * Drop-in boundary: the reference is pure Python on stock
 * ATen ops (no native layer), so each entry below replaces the ATen op
 * sequence at the cited reference lines.  A maintainer binds them with ctypes
 * (see INTEGRATION.md); no torch types appear in any signature.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host";
 *   - activations are NHWC fp32 ([B][H][W][C], C contiguous), index tensors int32;
 *   - `stream` is a hipStream_t passed as void*; entries never synchronise,
 *     never allocate, never throw; scratch comes in through (ws, ws_bytes) with
 *     a matching *_workspace_bytes() query;
 *   - return 0 (WESUP_OK) or a negative WESUP_ERR_* code (wesup_strerror()).
 */
#ifndef WESUP_HIP_H
#define WESUP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WESUP_OK 0
#define WESUP_ERR_INVALID (-1)   /* bad shape / null pointer / unsupported size */
#define WESUP_ERR_LAUNCH (-2)    /* hipLaunch failed */
#define WESUP_ERR_WORKSPACE (-3) /* workspace too small */

/* classes of the C-way head (the *_c entries, wesup_paint_argmax, wesup_seg_confusion): 2 <= C <= WESUP_MAX_CLASSES */
#define WESUP_MAX_CLASSES 16
/* feature width of the head (wesup_propagate, wesup_head_fwd, wesup_head_fwd_c): 1 <= D <= WESUP_HEAD_MAX_D.  The propagation
 * kernel keeps 256 labelled rows of D + 1 floats and 16 rows of D floats in LDS, 1088 D + 1024 bytes: 163 136 B of the CU's
 * 160 KiB (163 840 B) at D = 149, 164 224 B at D = 150.  From D = 60 (more than 64 KiB) the entries raise the kernel's dynamic
 * LDS limit once; a wider D is WESUP_ERR_INVALID and nothing is launched. */
#define WESUP_HEAD_MAX_D 149

/* flags for wesup_gemm_nt.  Order: result = relu_in(A) . B^T + bias; MASK; ACCUM adds the old C; RELU_OUT clamps what is stored */
#define WESUP_RELU_IN 1    /* A := max(A, 0) while loading */
#define WESUP_RELU_OUT 2   /* C := max(C, 0) */
#define WESUP_ACCUM 4      /* C += result */
#define WESUP_MASK 8       /* result := mask > 0 ? result : 0 (ReLU backward) */

int wesup_abi_version(void);   /* 6 (round 6: the tile-form pooling entries of ABI 5, wesup_sp_tiles / wesup_sp_pool_tiles_*, are gone) */
/* The two debug entries only work in the debug build of the library (make -C wesup_amd/csrc debug ->
 * libwesup_hip_debug.so, GEMM kernels compiled with the in-kernel clock probe and the per-block trace); the shipped
 * library's kernels carry neither and both entries return WESUP_ERR_INVALID there.
 * debug, host-synchronous: shader clock (MHz) held during the main loop of the last wesup_gemm_nt / conv3x3 fwd /
 * dgrad launch (s_memtime / s_memrealtime of block 0) */
int wesup_debug_clock(double* mhz_out /* host */);
/* debug, host-synchronous: per-block {start, loop start, loop end, end} timestamps (100 MHz ticks) of NT launches */
int wesup_debug_set_trace(void* device_buf);
const char* wesup_strerror(int code);

/* ------------------------------------------------------------------ layout packing
 * models/wesup.py:263-279 feeds NCHW (1,3,H,W); the kernels want NHWC with the
 * 3 image channels padded to 4.  Conv weights stay in torch's (Co,Ci,3,3) layout
 * in the state_dict; they are re-packed per step. */
int wesup_pack_input(const float* img_nchw, float* out_nhwc4, int B, int H, int W, void* stream);
/* w_fwd  [Co][Kf], Kf = wesup_conv3x3_kpad(Ci): k = ((ci/32)*9 + kh*3+kw)*32 + ci%32 for Ci >= 32 (32-channel chunk,
 *         tap, channel: the taps of a chunk are consecutive K-steps); image layer: k = (kh*3+kw)*4 + ci, zero padded
 * w_dgrad[Ci][9*Co]: k = ((co/32)*9 + (2-kh)*3+(2-kw))*32 + co%32          (either panel may be NULL) */
int wesup_conv3x3_kpad(int Ci);
int wesup_pack_conv3x3_weight(const float* w_kcrs, float* w_fwd, float* w_dgrad, int Co, int Ci, void* stream);
int wesup_transpose(const float* in, float* out, int rows, int cols, void* stream);
/* n <= 40 transposes in one launch (the weight panels the input-gradient GEMMs of the side convs / fc layers read,
 * models/wesup.py:213-232; the interpolation-pooling matrices of a batch); items is a HOST array */
typedef struct WesupTransposeItem { const float* in; float* out; int rows, cols; } WesupTransposeItem;
int wesup_transpose_batched(const WesupTransposeItem* items /* host */, int n, void* stream);

/* ------------------------------------------------------------------ input pipeline
 * replaces the per-item CPU augmentation (albumentations) of utils/data.py:116-133,302-327 for a batch of decoded,
 * resized uint8 images: flips + shift/scale/rotate as ONE inverse affine map per image (bilinear image, nearest mask,
 * reflect-101 borders), HueSaturationValue, RandomBrightnessContrast, ToTensor.  params: 12 floats per image
 * {a00,a01,a02,a10,a11,a12 (output pixel -> source), alpha, beta, hue, sat, val, 0}.  mask_hw / out_mask may be NULL.
 * out_img fp32 [B][3][H][W] in [0,1]; out_mask uint8 one-hot [B][C][H][W] (class index 255 = no class).
 * elastic_field (optional, NULL = none): ElasticTransform's displacement field (utils/data.py:124, albumentations
 * ElasticTransform(alpha=1, sigma=50): gaussian_filter(U(-1,1), sigma) * alpha per axis), as a coarse grid [B][2][hc][wc]
 * (dx plane, dy plane; one value per cell x cell pixels, already smoothed -- wesup_amd.utils.data.elastic_field), sampled
 * bilinearly; elastic_params: 12 floats per image {e00,e01,e02,e10,e11,e12 (source grid -> the grid the field is defined
 * on = the transform's own forward affine), l00,l01,l10,l11 (linear part of its inverse), on (0/1), 0}. */
int wesup_augment(const uint8_t* img_hwc, const uint8_t* mask_hw, const float* params, const float* elastic_field,
                  const float* elastic_params, int hc, int wc, int cell, float* out_img_nchw,
                  uint8_t* out_mask_chw, int B, int H, int W, int C, void* stream);
/* Appearance transforms that need a neighbourhood, on the un-warped uint8 images and in the reference's order
 * (utils/data.py:119-125, 306-312): HueSaturationValue -> RandomBrightnessContrast -> CLAHE (8x8 tiles on the L channel
 * of 8-bit Lab, OpenCV's algorithm) -> Blur (3x3 box), every stage rounding to uint8.  params: 8 floats per image
 * {alpha, beta, hue, sat, val, clahe_clip (0 = off), blur (0/1), 0}.  img, out: [B][H][W][3] uint8 (out != img).
 * Run wesup_augment afterwards with neutral colour parameters for the geometry, ToTensor and the one-hot mask. */
size_t wesup_appearance_workspace_bytes(int B, int H, int W);
int wesup_appearance(const uint8_t* img_hwc, const float* params, uint8_t* out_hwc, int B, int H, int W,
                     void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ VGG16 3x3 convs (K1/K2/K12)
 * replaces torchvision VGG16 Conv2d(k=3,pad=1)+ReLU (models/wesup.py:199,279) and its autograd.
 * y is the PRE-ReLU output (the hook taps it, models/wesup.py:246-253); the next
 * layer applies ReLU while loading (relu_in).  x has Cin channels (4 for the image).
 * Arguments of the direct entries (wesup_conv3x3_fwd, _fwd_side, _dgrad, _wgrad); anything else is WESUP_ERR_INVALID and
 * nothing is launched:
 *   - the channel count of the output tensor (Cout forward, Cin for dgrad) is a multiple of 4, that of the input tensor
 *     4 (the image) or a power of two >= 32; wgrad: Cout a multiple of 32;
 *   - x, w, y, y_relu, bias, dy, mask_src, dx, side_w, side_bias, side_out and the wgrad workspace are 16-byte aligned
 *     (dw_kcrs and db: 4-byte);
 *   - B*H*W * max(Cin, Cout) < 2^31 (wgrad: B*H*W < 2^31);
 *   - the kernels find a pixel's (image, row, column) by multiply-high divisions by W and H (csrc/common.hpp, FastDiv:
 *     m = ceil(2^40 / d), exact for n*d <= 2^40 and n*m < 2^64), so B*H*W * W <= 2^40, B*H * H <= 2^40 and
 *     (B*H*W - 1) * ceil(2^40 / W) < 2^64, (B*H - 1) * ceil(2^40 / H) < 2^64 -- the last two bind only when B*H or B
 *     reaches 2^24. */
/* ws (optional, may be NULL): room for the partial accumulator tiles of the stream-K blocks that balance a short last
 * round of tiles over all block slots; without it the plain tiling is used.  Size for (Cin -> Cout); for dgrad ask
 * with the channel counts swapped.  One workspace per stream that may run concurrently. */
size_t wesup_conv3x3_workspace_bytes(int B, int H, int W, int Cin, int Cout);
/* y_relu (optional, may be NULL): a second output max(y, 0).  A layer's ReLU'd output is read 9 taps x (Cout/128)
 * times by the next layer's forward and again by its wgrad; applying the ReLU once where the value is produced instead
 * of on every load takes 32 vector instructions per 64 MFMAs out of both loops (relu_in = 0 on the ReLU'd copy). */
int wesup_conv3x3_fwd(const float* x, const float* w_fwd, const float* bias, float* y, float* y_relu,
                      int B, int H, int W, int Cin, int Cout, int relu_in,
                      void* ws, size_t ws_bytes, void* stream);
/* The same forward for a layer with Cout in {64, 128}, with the layer's 1x1 side conv (models/wesup.py:256-266:
 * Conv2d(Cout, Cout/2, 1) on the hooked conv output) fused into the epilogue: side_out[pixel*ld_side + c] =
 * sum_k y[pixel][k] * side_w[c][k] + side_bias[c] for c < Cout/2, computed from the output tile while it is in LDS
 * (y is not read a second time).  side_w row-major (Cout/2, Cout) = the Conv2d weight; side_bias may be NULL. */
int wesup_conv3x3_fwd_side(const float* x, const float* w_fwd, const float* bias, float* y, float* y_relu,
                           const float* side_w, const float* side_bias, float* side_out, int ld_side,
                           int B, int H, int W, int Cin, int Cout, int relu_in, void* stream);
/* dx = conv_transpose(dy) ; if mask_src: dx = mask_src > 0 ? dx : 0 ; if accumulate: dx += old dx */
int wesup_conv3x3_dgrad(const float* dy, const float* w_dgrad, const float* mask_src, float* dx,
                        int B, int H, int W, int Cin, int Cout, int accumulate,
                        void* ws, size_t ws_bytes, void* stream);
/* dw in torch layout (Co,Ci,3,3); db (Co).  Ci is the TRUE channel count (3 for the image,
 * whose tensor has 4); relu_in applies ReLU to x while loading. */
size_t wesup_conv3x3_wgrad_workspace_bytes(int B, int H, int W, int Ci, int Cout);
int wesup_conv3x3_wgrad(const float* x, const float* dy, float* dw_kcrs, float* db,
                        int B, int H, int W, int Ci, int Cout, int relu_in,
                        void* ws, size_t ws_bytes, void* stream);
/* The same dw / db through the Winograd F(m x m, 3x3) domain, m = 2 or 4 (the scheme of the non-fused Winograd
 * backward-filter algorithms of vendor conv libraries; it replaces autograd of the reference's Conv2d(k=3,pad=1),
 * models/wesup.py:199): both tensors are transformed per m x m output tile (workspace: P x tiles x (Ci + Cout) floats +
 * split-K slabs, P = (m+2)^2 positions, tiles = B * ceil(H/m) * ceil(W/m)), P TN GEMMs with K = tiles accumulate the
 * transformed filter gradient, and G^T (.) G maps it back to 3x3.  2.25x (m = 2) / 4x (m = 4) fewer multiply-adds than
 * the direct form; same result up to fp32 rounding (1-3e-6 of the tensor's maximum, the direct kernels' own level: m = 4
 * uses the interpolation points 0, +-3/4, +-3/2, inf, ~4x more accurate in fp32 than the textbook 0, +-1, +-2, inf).  Ci, Cout multiples of 4, >= 32 (meant for the 128..512-channel layers); x has Ci
 * channels. */
size_t wesup_conv3x3_wgrad_winograd_workspace_bytes(int B, int H, int W, int Ci, int Cout, int m);
/* v_pre (optional): the transformed input [P][tiles][Ci] kept by wesup_conv3x3_fwd_winograd of the same layer and the
 * same m; then x may be NULL and its transform pass is skipped. */
int wesup_conv3x3_wgrad_winograd(const float* x, const float* v_pre, const float* dy, float* dw_kcrs, float* db,
                                 int B, int H, int W, int Ci, int Cout, int relu_in, int m,
                                 void* ws, size_t ws_bytes, void* stream);
/* Forward and input gradient of the deep layers in the same domain:  V = B^T d B per (m+2) x (m+2) input patch, P batched
 * NT GEMMs M_p = V_p . U_p^T (one launch), Y = A^T M A + the epilogue of wesup_conv3x3_fwd / _dgrad (bias, second ReLU'd
 * output / ReLU mask, accumulate).  U = G g G^T comes from wesup_winograd_pack_weight (once per step):
 * u_fwd [P][Cout][Cin], u_dgrad [P][Cin][Cout] (rotated filter), P*Cin*Cout floats each.  Workspace: transformed
 * input + transformed output, P x tiles x (Cin + Cout) floats (dgrad: ask with the channel counts swapped).
 * v_keep (optional): where the forward leaves V for the weight gradient (P x tiles x Cin floats).
 * y_pool (optional): a third output (B, H/2, W/2, Cout) = the 2x2 / stride-2 max-pool that follows the layer
 * (models/wesup.py:199, torchvision's MaxPool2d(2, 2); an m x m output tile holds (m/2)^2 pooling windows), ReLU'd if
 * pool_relu.  Cin % 32 == 0, Cout % 4 == 0; the results equal the direct kernels' up to fp32 rounding (see above). */
size_t wesup_winograd_weight_floats(int Cin, int Cout, int m);
long wesup_winograd_tiles(int B, int H, int W, int m);
int wesup_winograd_pack_weight(const float* w_kcrs, float* u_fwd, float* u_dgrad, int Cout, int Cin, int m, void* stream);
/* the F(4x4,3x3) filters of several layers in ONE launch (what n calls of wesup_winograd_pack_weight(..., m = 4) write; the
 * step re-derives 12 + 12 filter sets per iteration); layers is a HOST array, at most 32 non-NULL panels in all */
typedef struct WesupWinoFilter { const float* w; float* u_fwd; float* u_dgrad; int Cout, Cin; } WesupWinoFilter;
int wesup_winograd_pack_weights(const WesupWinoFilter* layers /* host */, int n, void* stream);
size_t wesup_conv3x3_winograd_workspace_bytes(int B, int H, int W, int Cin, int Cout, int m);
int wesup_conv3x3_fwd_winograd(const float* x, const float* u_fwd, const float* bias, float* y, float* y_relu,
                               float* y_pool, int pool_relu, float* v_keep,
                               int B, int H, int W, int Cin, int Cout, int relu_in, int m,
                               void* ws, size_t ws_bytes, void* stream);
int wesup_conv3x3_dgrad_winograd(const float* dy, const float* u_dgrad, const float* mask_src, float* dx,
                                 int B, int H, int W, int Cin, int Cout, int accumulate, int m,
                                 void* ws, size_t ws_bytes, void* stream);
/* The input gradient of a layer that FOLLOWS a max-pool, taken straight through the pooling's backward (autograd of
 * ReLU -> MaxPool2d(2,2), models/wesup.py:199; m = 4 only): dy (B,H,W,Cout) at pooled resolution; nothing is written at
 * that resolution -- every value is added to unpool_dst (B,Hu,Wu,Cin), the gradient w.r.t. the pre-pool activations
 * unpool_src (same shape; H == Hu/2, W == Wu/2), at the FIRST maximum of its 2x2 window (torch's scan order) if that
 * maximum is positive.  Same result as wesup_conv3x3_dgrad_winograd + wesup_maxpool2_bwd(accumulate = 1), which read and
 * re-wrote all four positions of every window. */
int wesup_conv3x3_dgrad_winograd_unpool(const float* dy, const float* u_dgrad, const float* unpool_src, float* unpool_dst,
                                        int B, int H, int W, int Hu, int Wu, int Cin, int Cout, int m,
                                        void* ws, size_t ws_bytes, void* stream);
/* The three passes on their own (the two entries above chain them): x (B,H,W,C) -> V [P][tiles][C];
 * nbatch NT products of one shape in one launch, C_b = A_b . B_b^T (element strides between the entries; K % 32 == 0);
 * Mt [P][tiles][C] -> y = A^T M A + bias, masked by mask_src > 0, added to the old y if accumulate, with the optional
 * second output y_relu = max(y, 0).  plane_elems: elements between two of the P position planes of V / Mt (0: tiles * C);
 * larger when a sub-batch works inside the planes of a whole batch, which is how the engine can pipeline the memory-bound
 * transforms of one half of the batch under the GEMM of the other.  plane_elems must be a multiple of 4 and, unless 0, at
 * least tiles * C (WESUP_ERR_INVALID otherwise); what lies between two planes is neither read nor written.  The entries that
 * take it are wesup_winograd_input_transform[_bits], _output_transform[_unpool] and the three _gemm_output_transform* (there
 * for V); _outgrad_transform, _dual_transform[_unpool] and the composite entries always work on dense planes. */
int wesup_winograd_input_transform(const float* x, float* V, long plane_elems, int B, int H, int W, int C, int relu_in,
                                   int m, void* stream);
int wesup_gemm_nt_batched(const float* A, int lda, long strideA, const float* B, int ldb, long strideB,
                          float* C, int ldc, long strideC, int nbatch, int M, int N, int K, void* stream);
/* ... with a bias vector per product (strideBias elements apart; bias may be NULL): several 1x1 side convs of one shape
 * (models/wesup.py:208-209,253: Conv2d(C, C/2, 1) on the hooked conv outputs of the layers that share a resolution) and their
 * input gradients as one launch each */
int wesup_gemm_nt_batched_bias(const float* A, int lda, long strideA, const float* B, int ldb, long strideB,
                               const float* bias, long strideBias, float* C, int ldc, long strideC,
                               int nbatch, int M, int N, int K, void* stream);
int wesup_winograd_output_transform(const float* Mt, long plane_elems, const float* bias, const float* mask_src, float* y,
                                    float* y_relu, float* y_pool, int pool_relu, int B, int H, int W, int C,
                                    int accumulate, int m, void* stream);
/* ... with the max-pool backward as its epilogue (the last pass of wesup_conv3x3_dgrad_winograd_unpool; m = 4) */
int wesup_winograd_output_transform_unpool(const float* Mt, long plane_elems, const float* bias, const float* mask_src,
                                           const float* unpool_src, float* unpool_dst, int B, int H, int W, int Hu, int Wu,
                                           int C, int m, void* stream);
/* The batched products and the output transform in ONE kernel (m = 4; K = 64 or 128 channels of the product, N % 64 == 0):
 * V [36][tiles][K] x U [36][N][K] -> y (B,H,W,N) = A^T (V_p . U_p^T) A + the epilogue of wesup_winograd_output_transform
 * (bias, mask_src, accumulate, y_pool) or of its _unpool form (unpool_src / unpool_dst (B,Hu,Wu,N), y = NULL): the
 * transformed output [36][tiles][N] is never written.  At these widths the separate passes are HBM-bound on exactly that
 * tensor; wesup_conv3x3_fwd/dgrad_winograd[_unpool] take this route by themselves (WESUP_WINO_FUSED=0: never, 1: forward only).
 * Results equal the two-kernel route's up to fp32 summation order. */
int wesup_winograd_fused_supported(int K, int N, int m);
/* ... and whether a problem of `tiles` tiles takes it (0: the grid of the one-kernel route would be too small, < 200 blocks) */
int wesup_winograd_fused_route(int K, int N, int m, long tiles);
int wesup_winograd_set_fused_min_blocks(int blocks);   /* tuning knob of that rule (default 200); returns the previous value */      /* 0: no; 1: the conv entries take the one-kernel route for this
                                                                 product in the forward; 2: in the input gradient as well */
int wesup_winograd_gemm_output_transform(const float* V, long plane_elems, const float* U, const float* bias,
                                         const float* mask_src, float* y, float* y_pool, int pool_relu,
                                         const float* unpool_src, float* unpool_dst, int Hu, int Wu,
                                         int B, int H, int W, int K, int N, int accumulate, void* stream);
/* ... with the destination's OLD content replaced by a gather: with the side conv of a native-resolution layer applied
 * behind the superpixel mean (the two commute, models/wesup.py:246-261,281-285), the side-branch gradient of that layer's
 * conv output is constant over a superpixel: side [B][Kmax][N] one row per superpixel, new_row [B][pixels] the pixel's row,
 * area_new [B][Kmax]; value(pixel) = side[new_row[pixel]] / area_new[new_row[pixel]] (what wesup_upsample_bwd would write).
 * y form: y = value(pixel) + (mask_src > 0 ? result : 0).  unpool form (unpool_src (B,Hu,Wu,N) given, y is the (B,Hu,Wu,N)
 * destination, Hu and Wu even): every position of a 2x2 window = its value, the first positive maximum of unpool_src gets
 * the window's result on top.  The destination is written, never read. */
int wesup_winograd_gemm_output_transform_gather(const float* V, long plane_elems, const float* U, const float* mask_src,
                                                float* y, const float* unpool_src, int Hu, int Wu, const float* side,
                                                const int32_t* new_row, const int32_t* area_new, int Kmax,
                                                int B, int H, int W, int K, int N, void* stream);
/* One pass over a gradient tensor for both of its F(4x4) transforms: V = B^T dY B (6x6 patches; the input of the layer's input
 * gradient) and dM = A dY A^T (4x4 cores; the second operand of its weight gradient), plus the per-block column sums of dy the
 * bias gradient is folded from (bias_part, optional: [wesup_winograd_bias_rows(B,H,W,C)][C]; 0 rows = this C is not covered).
 * wesup_conv3x3_wgrad_winograd_pre: the weight gradient from those operands and the forward's kept transformed input v_pre
 * (wesup_conv3x3_fwd_winograd's v_keep): batched TN products + filter-gradient reduce, the transform passes already done. */
long wesup_winograd_bias_rows(int B, int H, int W, int C);
int wesup_winograd_dual_transform(const float* dy, float* V, float* dM, float* bias_part, int B, int H, int W, int C,
                                  void* stream);
/* The same for the gradient of a layer in front of a 2x2 max-pool, without that gradient in memory:
 * dy(b,h,w,c) = side(b,h,w,c) + (code(b,h/2,w/2,c) picks this position of the window ? dP(b,h/2,w/2,c) : 0), formed while
 * loading.  dP (B,H/2,W/2,C): the input gradient of the layer above at pooled resolution; code (B,H/2,W/2,C/4) uint16: the
 * forward's pooling decisions (wesup_winograd_gemm_output_transform_ex's pool_code); H, W even.  side: the side-branch
 * gradient, dense (B,H,W,C) with new_row NULL, or rows [B][Kmax][C] (divided by their areas already) gathered per pixel by
 * new_row [B][H*W], as wesup_conv3x3_dgrad_winograd_gather takes them.  V, dM and bias_part equal wesup_winograd_dual_transform
 * of the tensor the unpooling epilogues (wesup_conv3x3_dgrad_winograd_unpool / _gather) would have written, bit for bit.
 * side, dP and the label map each below 4 GiB (WESUP_ERR_INVALID otherwise: the kernel's offsets are 32-bit). */
int wesup_winograd_dual_transform_unpool(const float* side, const int32_t* new_row, int Kmax, const float* dP,
                                         const unsigned short* code, float* V, float* dM, float* bias_part, int B, int H, int W,
                                         int C, void* stream);
int wesup_conv3x3_wgrad_winograd_pre(const float* v_pre, const float* dm_pre, const float* bias_part, int bias_rows,
                                     float* dw_kcrs, float* db, int B, int H, int W, int Ci, int Cout,
                                     void* ws, size_t ws_bytes, void* stream);
/* Compact forms of what the backward needs of the forward's activations (F(4x4) route; 16x resp. 32x smaller than the tensors
 * they replace).  relu_bits [B][H][W][C/4] bytes: bit j of byte q = x[..., 4q + j] > 0 -- the ReLU decisions of the layer that
 * produced x, written by the input transform of the layer that consumes it (it reads x anyway).  pool codes
 * [B][H/2][W/2][C/4] uint16, 3 bits per channel of the quad: 0 = the window's maximum is not positive, k + 1 = first maximum at
 * window position k (row-major: torch's scan order) -- the max-pool's decisions, written by the epilogue that pools.
 * wesup_winograd_gemm_output_transform_ex: every option of the one-kernel route.  mask_bits instead of mask_src; pool_code
 * OUT (needs y_pool); unpool_code IN instead of reading unpool_src (then optional); side != NULL selects the gather forms. */
int wesup_winograd_input_transform_bits(const float* x, float* V, long plane_elems, unsigned char* relu_bits,
                                        int B, int H, int W, int C, int relu_in, void* stream);
int wesup_winograd_gemm_output_transform_ex(const float* V, long plane_elems, const float* U, const float* bias,
                                            const float* mask_src, const unsigned char* mask_bits, float* y, float* y_pool,
                                            int pool_relu, unsigned short* pool_code, const float* unpool_src,
                                            const unsigned short* unpool_code, float* unpool_dst, int Hu, int Wu,
                                            const float* side, const int32_t* new_row, const int32_t* area_new, int Kmax,
                                            int B, int H, int W, int K, int N, int accumulate, void* stream);
/* wesup_conv3x3_dgrad_winograd(accumulate = 1) resp. wesup_conv3x3_dgrad_winograd_unpool (unpool_src given; dx is then
 * (B,Hu,Wu,Cin)) with that gather in the epilogue instead of a materialised side-branch gradient in dx.  m = 4; product shapes
 * with wesup_winograd_fused_supported(Cout, Cin, 4) == 2, otherwise WESUP_ERR_INVALID (materialise, use the forms above).
 * area_new == NULL (here and in the two gather entries above): the rows of `side` are divided by their areas already --
 * wesup_scale_rows_by_area(side, area_new, B * Kmax, Cin): x[row][:] *= 1 / area[row] (0 where area is 0) -- so the epilogue
 * gathers one row per pixel and nothing else (conv1_2's input gradient alone 387 -> 349 us at configs[1]). */
int wesup_scale_rows_by_area(float* x, const int32_t* area, long rows, int C, void* stream);
int wesup_conv3x3_dgrad_winograd_gather(const float* dy, const float* u_dgrad, const float* mask_src,
                                        const float* unpool_src, float* dx, const float* side, const int32_t* new_row,
                                        const int32_t* area_new, int Kmax, int B, int H, int W, int Hu, int Wu,
                                        int Cin, int Cout, void* ws, size_t ws_bytes, void* stream);
/* The weight gradient's own transforms: dy (B,H,W,C) -> dM [P][tiles][C] = A dY A^T per m x m tile; and the way back from
 * the split-K slabs of the P transformed filter gradients ([P][S][Cout*Cin + Cout], each slab followed by the Cout
 * column sums of its dM operand) to dw (Cout,Cin,3,3) = G^T (sum over S) G.  The bias gradient db = sum over pixels of dy:
 * m = 2, the column sums of dM at position (1,1) (index 5; filter_grad's db); m = 4 (its point set 0, +-3/4, +-3/2, inf
 * has no position that is a plain sum), the optional db of the outgrad transform, summed from the values it loads anyway
 * (ws: wesup_winograd_outgrad_workspace_bytes; db must be NULL for m = 2 there, and for m = 4 in filter_grad).
 * filter_grad: slab_stride = elements between two splits (>= Cout*Cin + Cout), batch_stride = between two positions
 * (>= S * slab_stride); any such strides, pair counts and alignment are accepted -- m = 4 reads 16 bytes at a time only where
 * Cout*Cin, both strides and the pointer allow it, and gives the same bits either way. */
size_t wesup_winograd_outgrad_workspace_bytes(int B, int H, int W, int C, int m);
int wesup_winograd_outgrad_transform(const float* dy, float* dM, float* db, int B, int H, int W, int C, int m,
                                     void* ws, size_t ws_bytes, void* stream);
int wesup_winograd_filter_grad(const float* slabs, long slab_stride, long batch_stride, int S, float* dw_kcrs, float* db,
                               int Cout, int Cin, int m, void* stream);

/* ------------------------------------------------------------------ generic fp32 MFMA GEMMs
 * side 1x1 convs (models/wesup.py:208-209,253), fc_layers (models/wesup.py:213-220,288) and their grads.
 * nt:  C[M][N] = epilogue( A[M][K] . B[N][K]^T + bias[N] )      (K % 32 == 0, rows 16B aligned)
 * tn:  C[M][N] = A[K][M]^T . B[K][N]      (weight gradients; deterministic split-K)
 * colsum: out[N] = sum_m A[m][n]          (bias gradients without a weight gradient next to them) */
size_t wesup_gemm_nt_workspace_bytes(int M, int N, int K);      /* stream-K partial tiles; ws may be NULL */
int wesup_gemm_nt(const float* A, int lda, const float* B, int ldb, const float* bias,
                  float* C, int ldc, const float* mask, int ldmask,
                  int M, int N, int K, int flags, void* ws, size_t ws_bytes, void* stream);
size_t wesup_gemm_tn_workspace_bytes(int M, int N, int K);
/* colsum_a (optional, [M]): also out[m] = sum_k A[k][m] -- the bias gradient that goes with a weight gradient --
 * accumulated from the staged A tiles, so A is not read a second time.
 * Round 5: a product whose tiles fill the chip without splitting K (>= 600 tiles) runs ONE split and, without colsum_a (C 8-byte
 * aligned, ldc even), stores straight into C: no slab, no reduce launch; ws is still required (and may go unused). */
int wesup_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, float* colsum_a,
                  int M, int N, int K, int relu_b, void* ws, size_t ws_bytes, void* stream);
/* nbatch products of one shape in one launch: C_b = A_b^T . B_b, element strides between batch entries */
size_t wesup_gemm_tn_batched_workspace_bytes(int nbatch, int M, int N, int K);
/* length of the K ranges whose sums that entry adds in ascending order (>= K: one range); equal ranges, i.e. not the
 * weighted split of a single product of 128 x 128 tiles */
int wesup_gemm_tn_batched_k_per_split(int nbatch, int M, int N, int K);
int wesup_gemm_tn_batched(const float* A, int lda, long strideA, const float* B, int ldb, long strideB,
                          float* C, int ldc, long strideC, int nbatch, int M, int N, int K, int relu_b,
                          void* ws, size_t ws_bytes, void* stream);
size_t wesup_colsum_workspace_bytes(int M, int N);
int wesup_colsum(const float* A, int lda, float* out, int M, int N, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ pooling / upsampling (K2/K4)
 * maxpool: nn.MaxPool2d(2,2) after ReLU == ReLU after maxpool; operates on pre-ReLU y (relu_out applies the ReLU to
 * the pooled values as it stores them). */
int wesup_maxpool2_fwd(const float* y, float* yp, int B, int H, int W, int C, int relu_out /* yp = max(pool, 0) */,
                       void* stream);
/* dy[p] = (p is the first max of its window and y[p] > 0 ? dyp[window] : 0) (+ dy[p] if accumulate) */
int wesup_maxpool2_bwd(const float* y, const float* dyp, float* dy, int B, int H, int W, int C,
                       int accumulate, void* stream);
/* F.interpolate(bilinear, align_corners=True) (models/wesup.py:254-255) into channel slice
 * [coff, coff+C) of the feature-map tensor fm [B][H][W][ldf]. */
int wesup_upsample_fwd(const float* s, float* fm, int B, int h, int w, int H, int W, int C,
                       int ldf, int coff, void* stream);
/* ds[q][c] = sum_p wgt(p,q) * src(p)[coff+c].  src(p) = dfm[b][p][.] when new_row == NULL; otherwise the
 * pooling backward is fused in: src(p) = g[b][new_row[b][p]][.] / area[b][new_row[b][p]]  (ldf = row stride) */
int wesup_upsample_bwd(const float* dfm_or_g, const int32_t* new_row, const int32_t* area_new,
                       float* ds, int B, int h, int w, int H, int W, int C, int ldf, int coff,
                       int Kmax, void* stream);
/* The fused form (new_row given) for n <= 3 layers that share one coarse resolution (h, w) != (H, W), one launch:
 * ds_i [B][h][w][C_i] from g_i [B][Kmax][C_i] (dense rows, C_0 + .. + C_{n-1} <= 768); the scan of a cell's window of
 * full-resolution pixels is shared by the layers.  Same values as n calls of wesup_upsample_bwd. */
int wesup_upsample_bwd_group(const float* g0, const float* g1, const float* g2, float* ds0, float* ds1, float* ds2,
                             int C0, int C1, int C2, int n, const int32_t* new_row, const int32_t* area_new, int B,
                             int h, int w, int H, int W, int Kmax, void* stream);

/* ------------------------------------------------------------------ superpixels (K6/K8/K9)
 * wesup_sp_preprocess replaces _preprocess_superpixels (models/wesup.py:18-63) without dense maps.
 *   labels [B][HW] ids 0..n-1 (contiguous), mask [B][C][HW] uint8 {0,1} or NULL, Kmax >= max id+1
 * outputs (all [B][Kmax...] padded; rows are in the reference's order: labelled ids ascending, then unlabelled):
 *   n_sp[B], n_l[B], perm[B][Kmax] (row->id), inv_perm[B][Kmax] (id->row), area_new[B][Kmax] (by row),
 *   sp_labels[B][Kmax][C] f32 multi-hot (rows >= n_l zero), new_row[B][HW], row_start[B][Kmax+1],
 *   pix_sorted[B][HW] (pixels grouped by row, ascending pixel index inside a row),
 *   status[B]: 0 ok, 1 = label id >= Kmax, 2 = empty id below max (the reference would produce NaN). */
size_t wesup_sp_preprocess_workspace_bytes(int B, int HW, int C, int Kmax);
int wesup_sp_preprocess(const int32_t* labels, const uint8_t* mask, int B, int HW, int C, int Kmax,
                        int32_t* n_sp, int32_t* n_l, int32_t* perm, int32_t* inv_perm, int32_t* area_new,
                        float* sp_labels, int32_t* new_row, int32_t* row_start, int32_t* pix_sorted,
                        int32_t* status, int32_t* seg_start /* or NULL */, int32_t* unit_row /* or NULL */, int Umax,
                        void* ws, size_t ws_bytes, void* stream);
/* (the segment table of wesup_sp_segments is written on the way when seg_start / unit_row [B][Kmax+1] / [B][Umax] are given.
 *  Four launches, every phase parallel over chunks resp. ids: sums zeroed; per-chunk histograms in LDS, added to the image's
 *  sums with integer atomics (exact in any order); chunk prefixes beside the per-image ordering; placement.
 *  Limits: Kmax <= 16384 and Kmax * (2 + C) <= 81920 (LDS of the histogram pass: C <= 3 at Kmax = 16384), B <= 65535; no
 *  library-side state -- any number of streams may call it concurrently, each with a workspace of its own.) */
/* dense compat: labels[p] = argmax_n sp_maps[n][p] (first max), as models/wesup.py:295 does */
int wesup_spmaps_to_labels(const float* sp_maps, int32_t* labels, int N, int HW, void* stream);
/* scatter-mean: sp_feat[b][r][c] = (1/area_r) sum_{p in row r} fm[b][p][c]   (torch.mm, models/wesup.py:283-285) */
int wesup_sp_max_units(int HW, int Kmax);      /* upper bound of segments per image: Kmax + HW / 512 */
/* segment table for load-balanced pooling: a superpixel row is cut into segments of <= 512 pixels;
 * seg_start[B][Kmax+1] (exclusive scan of segments per row), unit_row[B][Umax] (segment -> row) */
int wesup_sp_segments(const int32_t* row_start, int B, int Kmax, int Umax, int32_t* seg_start, int32_t* unit_row,
                      void* stream);
size_t wesup_sp_pool_workspace_bytes(int B, int Umax, int C);   /* partial sums of multi-segment rows */
int wesup_sp_pool_fwd(const float* fm, const int32_t* pix_sorted, const int32_t* row_start,
                      const int32_t* seg_start, const int32_t* unit_row, float* sp_feat,
                      int B, int HW, int ldf, int C, int Kmax, int Umax, void* ws, size_t ws_bytes, void* stream);
/* fused upsample + scatter-mean: sp_feat[b][r][coff+c] = (1/area_r) sum_{p in row r} bilinear_ac(s[b], p)[c], s = side
 * output [B][h][w][C] (C in {32,64,128,256} or a multiple of 256, which goes in slabs of 256 channels); equals
 * wesup_upsample_fwd followed by wesup_sp_pool_fwd on that slice without materialising the (HW x 2112) feature map (models/wesup.py:254-261 + :283-285) */
int wesup_sp_pool_upsample_fwd(const float* s, const int32_t* pix_sorted, const int32_t* row_start,
                               const int32_t* seg_start, const int32_t* unit_row, float* sp_feat,
                               int B, int h, int w, int H, int W, int C, int ldo, int coff, int Kmax, int Umax,
                               void* ws, size_t ws_bytes, void* stream);

/* the same linear map as a matrix over the h*w cells of a coarse side output:
 * Wm[b][r][q] = (1/area_r) sum_{p in row r} bilinear_ac weight of cell q at pixel p     ([B][Kmax][h*w], h*w <= 8192).
 * Then  sp_feat[b][:, slice] = Wm[b] . s[b]  and  ds[b] = Wm[b]^T . g[b][:, slice]  are wesup_gemm_tn calls
 * (on Wm^T resp. Wm); used for the deep layers, where Wm is small (models/wesup.py:254-261 + :283-285 and autograd) */
int wesup_sp_interp_matrix(const int32_t* pix_sorted, const int32_t* row_start, float* Wm,
                           int B, int H, int W, int h, int w, int Kmax, void* stream);
/* The two products of Wm, each by the route its size asks for.  Operands: Wm [B][Kmax][hw] and its transpose WmT [B][hw][Kmax],
 * s / ds [B][hw][C] contiguous, and the C channels at channel `off` of the superpixel-side rows sp / gsp [B][Kmax][ld]
 * (C, ld, off multiples of 4, off + C <= ld, hw <= 8192).
 *   fwd:  sp[b][r][off..off+C) = sum_q Wm[b][r][q] s[b][q][.]        bwd:  ds[b][q][.] = sum_r Wm[b][r][q] gsp[b][r][off..off+C)
 * Below the size rule (wesup_sp_pool_mat_route(Kmax, hw) == 0: Kmax * hw under 65 536 entries, or under what
 * WESUP_POOL_MAT_SPARSE_MIN says -- 0: never sparse, 1: always) they issue exactly wesup_gemm_tn_batched on WmT resp. Wm, with its
 * conditions (Kmax, hw multiples of 4) and its workspace (wesup_gemm_tn_batched_workspace_bytes(B, Kmax, C, hw) resp.
 * (B, hw, C, Kmax)).  Above it one kernel walks the non-zeros of each row (column) in ascending index, adding in the order of the dense product's own additions (its K ranges): a fixed-order sum,
 * no atomics, bitwise reproducible, no workspace (ws may be NULL); an all-zero row (column) gives exact zeros. */
int wesup_sp_pool_mat_route(int Kmax, int hw);
int wesup_sp_pool_mat_fwd(const float* Wm, const float* WmT, const float* s, float* sp, int ld, int off,
                          int B, int Kmax, int hw, int C, void* ws, size_t ws_bytes, void* stream);
int wesup_sp_pool_mat_bwd(const float* Wm, const float* WmT, const float* gsp, int ld, int off, float* ds,
                          int B, int Kmax, int hw, int C, void* ws, size_t ws_bytes, void* stream);
/* dfm[b][p][c] = g[b][new_row[p]][c] / area[new_row[p]] */
int wesup_sp_pool_bwd(const float* g, const int32_t* new_row, const int32_t* area_new, float* dfm,
                      int B, int HW, int ldf, int C, int Kmax, void* stream);
/* paint-back (models/wesup.py:294-304): pred[b][p] = sp_pred[b][new_row[p]][cls] */
int wesup_paint_fwd(const float* sp_pred, const int32_t* new_row, float* pred, int B, int HW, int Kmax,
                    int C, int cls, void* stream);

/* ------------------------------------------------------------------ SLIC superpixels
 * replaces the CPU skimage.segmentation.slic call of WESUPTrainer.preprocess (models/wesup.py:471-476).
 * img [B][3][H][W] RGB in [0,1]; labels [B][HW] get contiguous ids 0..n_labels[b]-1 (4-connected superpixels,
 * numbered in raster order of their first pixel).  Third-party algorithm, parity unpinned (see csrc/slic.hip). */
int wesup_slic_num_centers(int H, int W, int n_segments);
size_t wesup_slic_workspace_bytes(int B, int H, int W, int n_segments);
int wesup_slic(const float* img_nchw, int32_t* labels, int32_t* n_labels, int B, int H, int W, int n_segments,
               float compactness, int max_iter, int enforce_connectivity, float min_size_factor,
               void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ head, loss, optimiser (K7/K10/K11/K13)
 * classifier Linear(D,2)+Softmax(dim=1) (models/wesup.py:229-232,292).  The two-class entries of this block run the kernels of the
 * _c entries below, instantiated for C = 2 (csrc/loss.hip); wesup_classifier_fwd alone takes any D > 0 (beyond D = 8191, where
 * Wc | bc no longer fit 64 KiB of LDS, its kernel reads them from global memory). */
int wesup_classifier_fwd(const float* feat, const float* Wc, const float* bc, float* pred, int R, int D, void* stream);
/* given dpred: dfeat[R][D] (masked by feat > 0: fc_layers' last ReLU), dWc[2][D], dbc[2] */
size_t wesup_classifier_bwd_workspace_bytes(int R, int D);
int wesup_classifier_bwd(const float* feat, const float* Wc, const float* pred, const float* dpred,
                         const float* dfeat_extra, float* dfeat, float* dWc, float* dbc, int R, int D,
                         void* ws, size_t ws_bytes, void* stream);
/* _label_propagate (models/wesup.py:99-139) per image on padded rows.  y_all[b][r][:] = sp_labels for
 * r < n_l, propagated pseudo label for n_l <= r < n_sp (zeros if max similarity <= threshold), 0 beyond.
 * src_idx/max_sim [B][Kmax] (entries for unlabelled rows; -1/0 elsewhere).  D <= WESUP_HEAD_MAX_D (above). */
int wesup_propagate(const float* feat, const float* sp_labels, const int32_t* n_sp, const int32_t* n_l,
                    float threshold, int enable, float* y_all, int32_t* src_idx, float* max_sim,
                    int B, int Kmax, int D, int C, void* stream);
/* _cross_entropy + compute_loss (models/wesup.py:66-96,492-531), per image then mean over images:
 * terms[b] = {sup_sum, sup_cnt, prop_sum, prop_cnt, prop_label_sum, loss_b, 0, 0}; loss[0] = mean_b loss_b = (sum over b in
 * ascending order, in fp32) / B -- or loss == NULL: no second launch, the caller forms that mean from terms */
int wesup_loss_fwd(const float* pred, const float* y_all, const int32_t* n_sp, const int32_t* n_l,
                   float eps, float prop_weight, float* terms, float* loss, int B, int Kmax, int C, void* stream);
/* dpred = dloss[0] * d loss / d pred */
int wesup_loss_bwd(const float* pred, const float* y_all, const int32_t* n_sp, const int32_t* n_l,
                   const float* terms, const float* dloss, float eps, float prop_weight, float* dpred,
                   int B, int Kmax, int C, void* stream);
/* ABI 5 -- the head of the training step in two launches instead of six (the chain between the fc layers' forward and their
 * backward is a chain of launch latencies).  Bit-identical to the entries they combine.
 * wesup_head_fwd  = wesup_classifier_fwd + wesup_propagate (both read feat (B*Kmax, D); pred (B*Kmax, 2)).
 * wesup_head_bwd  = wesup_loss_fwd (terms only) + wesup_loss_bwd + the first kernel of wesup_classifier_bwd: terms (B, 8),
 *                   dpred (B*Kmax, 2), dfeat (B*Kmax, D); Kmax % 64 == 0, C == 2; ws as wesup_classifier_bwd_workspace_bytes.
 * wesup_classifier_bwd_finish: dWc (2, D), dbc (2) from the partial sums wesup_head_bwd left in ws -- on any stream behind it
 *                   (models/wesup.py:66-139,229-232,492-531).
 * wesup_head_fwd takes labels of any width C > 0 and writes two columns of pred; wesup_head_bwd, wesup_classifier_bwd,
 * wesup_classifier_bwd_workspace_bytes and wesup_classifier_bwd_finish are their _c forms called with C = 2. */
int wesup_head_fwd(const float* feat, const float* Wc, const float* bc, float* pred, const float* sp_labels,
                   const int32_t* n_sp, const int32_t* n_l, float threshold, int enable, float* y_all, int32_t* src_idx,
                   float* max_sim, int B, int Kmax, int D, int C, void* stream);
int wesup_head_bwd(const float* feat, const float* Wc, const float* pred, const float* y_all, const int32_t* n_sp,
                   const int32_t* n_l, const float* dloss, float eps, float prop_weight, float* terms, float* dpred,
                   float* dfeat, int B, int Kmax, int D, int C, void* ws, size_t ws_bytes, void* stream);
int wesup_classifier_bwd_finish(const void* ws, size_t ws_bytes, float* dWc, float* dbc, int R, int D, void* stream);
/* ------------------------------------------------------------------ the C-way head, 2 <= C <= WESUP_MAX_CLASSES
 * One kernel body per operation: called with C = 2 an entry launches the instantiation with the class count as a compile-time
 * constant (prop_kernel, head_bwd_kernel, classifier_bwd_reduce: the two-class step's launch list does not move, and its bits are
 * pinned to the last commit with two-class kernels of its own by tests/golden/head_two_class_bits.json), with more classes the one
 * with the run-time count.  Outside the range of C every entry returns WESUP_ERR_INVALID.
 * wesup_classifier_fwd_c: pred (R, C) = softmax(feat (R, D) . Wc (C, D)^T + bc): logits by fmaf in ascending k, the maximum
 *   subtracted, exponentials summed in ascending class order, one reciprocal.  A streaming kernel (pixel inference runs it with
 *   R = B*H*W): Wc / bc in LDS once per block, rows as float4 where D % 4 == 0, logits in registers; D <= 512.
 * wesup_classifier_bwd_c: dz_c = p_c (dp_c - sum_j dp_j p_j); dfeat = (sum_c dz_c Wc[c][k] + dfeat_extra) where feat > 0, else 0;
 *   dWc (C, D), dbc (C) from per-64-row partial sums added in fixed order (no float atomics).  Class sums: the first product,
 *   then fmaf in ascending class order.
 * wesup_head_fwd_c = wesup_classifier_fwd_c + wesup_propagate in one launch; wesup_head_bwd_c = wesup_loss_fwd (terms only) +
 *   wesup_loss_bwd + the first kernel of wesup_classifier_bwd_c in one launch (Kmax % 64 == 0), wesup_classifier_bwd_c_finish
 *   adds the partial sums it left in ws up.  Bit-identical to the separate entries at the same C. */
int wesup_classifier_fwd_c(const float* feat, const float* Wc, const float* bc, float* pred, int R, int D, int C, void* stream);
size_t wesup_classifier_bwd_c_workspace_bytes(int R, int D, int C);
int wesup_classifier_bwd_c(const float* feat, const float* Wc, const float* pred, const float* dpred,
                           const float* dfeat_extra, float* dfeat, float* dWc, float* dbc, int R, int D, int C,
                           void* ws, size_t ws_bytes, void* stream);
int wesup_head_fwd_c(const float* feat, const float* Wc, const float* bc, float* pred, const float* sp_labels,
                     const int32_t* n_sp, const int32_t* n_l, float threshold, int enable, float* y_all, int32_t* src_idx,
                     float* max_sim, int B, int Kmax, int D, int C, void* stream);
int wesup_head_bwd_c(const float* feat, const float* Wc, const float* pred, const float* y_all, const int32_t* n_sp,
                     const int32_t* n_l, const float* dloss, float eps, float prop_weight, float* terms, float* dpred,
                     float* dfeat, int B, int Kmax, int D, int C, void* ws, size_t ws_bytes, void* stream);
int wesup_classifier_bwd_c_finish(const void* ws, size_t ws_bytes, float* dWc, float* dbc, int R, int D, int C, void* stream);
/* class-map paint-back: pred[b][p] = (float) argmax_c sp_pred[b][new_row[p]][c], the first maximum (ties go to the lowest class).
 * The argmax is taken once per superpixel row into ws (B * Kmax floats), then gathered per pixel. */
size_t wesup_paint_argmax_workspace_bytes(int B, int Kmax);
int wesup_paint_argmax(const float* sp_pred, const int32_t* new_row, float* pred, int B, int HW, int Kmax, int C,
                       void* ws, size_t ws_bytes, void* stream);
/* conf (B, C, C) int32: pixels per (ground-truth class = first maximum over the mask's C planes, predicted class = pred as a
 * class index).  conf and status[0] are zeroed by the entry; a predicted value outside [0, C) (or NaN) sets status[0] and is
 * not counted.  Integer adds in LDS per block, then integer adds to the table: the result does not depend on the order. */
int wesup_seg_confusion(const float* pred, const uint8_t* mask, int32_t* conf, int32_t* status, int B, int HW, int C,
                        void* stream);
/* generic _cross_entropy (models/wesup.py:66-96) on (n, C): out2[4] = {sum(-y log clamp(yhat) [* class_weights[c]]),
 * #rows with sum(y) > 0, loss = sum/#rows (0 if no row is labelled), 0}; class_weights (C,) or NULL (models/wesup.py:93-94) */
int wesup_cross_entropy_fwd(const float* y_hat, const float* y_true, const float* class_weights, float eps, float* out2,
                            int n, int C, void* stream);
int wesup_cross_entropy_bwd(const float* y_hat, const float* y_true, const float* class_weights, const float* out2,
                            const float* dloss, float eps, float* dy_hat, int n, int C, void* stream);
/* torch.optim.SGD step (models/wesup.py:445-451): g' = g*grad_scale + wd*p; v = first ? g' : mu*v + g'; p -= lr*v */
int wesup_sgd_step(float* p, const float* g, float* v, size_t n, float lr, float momentum, float weight_decay,
                   float grad_scale, int first_step, void* stream);
/* torch.optim.Adam / AdamW (no amsgrad) for a recorded step (csrc/optim.hip).  `state` is a 32-byte, 16-byte aligned device block
 * the optimiser owns: { double lr; int32 t; float step_size, inv_sqrt_bc2, decay; 8 bytes unused }.  The host writes lr (and t,
 * from a checkpoint); wesup_adam_tick -- one thread -- forms t += 1, step_size = lr / (1 - b1^t), inv_sqrt_bc2 = 1 / sqrt(1 - b2^t),
 * decay = 1 - lr wd in double with b = 1 - (double) one_minus_b, and rounds each to float once.  wesup_adam_step reads the three
 * factors from the block:  g' = g grad_scale;  decoupled ? p *= decay : g' += wd p;  m = b1 m + (1 - b1) g';
 * v = b2 v + (1 - b2) g' g';  p -= step_size m / (sqrt(v) inv_sqrt_bc2 + eps).  one_minus_beta* are the floats of the host's
 * doubles 1 - beta (1.f - 0.999f is wrong in the fifth digit).  Pointers 16-byte aligned, n > 0: else WESUP_ERR_INVALID. */
int wesup_adam_tick(void* state, float one_minus_beta1, float one_minus_beta2, float weight_decay, void* stream);
int wesup_adam_step(float* p, const float* g, float* m, float* v, size_t n, const void* state, float beta1,
                    float one_minus_beta1, float beta2, float one_minus_beta2, float eps, float weight_decay,
                    float grad_scale, int decoupled, void* stream);
/* accuracy / dice inputs (utils/metrics.py:31-45,112-135): out[b] = {#(P==G), sum(P*G), sum(P), sum(G)} with
 * P = round(pred) (half to even, models/wesup.py:534), G = argmax_c mask (first max).  The sums are formed in float: they are
 * the exact integers while every one of them stays below 2^24 = 16 777 216 (an image of up to 2^24 pixels with P, G in {0, 1};
 * with class indices up to C - 1 the bound is on sum(P*G) <= (C - 1)^2 HW); beyond that they are rounded. */
size_t wesup_seg_metrics_workspace_bytes(int B);
int wesup_seg_metrics(const float* pred, const uint8_t* mask, float* out4, int B, int HW, int C,
                      void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ mask post-processing and challenge scoring (csrc/regions.hip)
 * Integer image processing of predicted masks on the device: what scipy.ndimage / numpy do on the host in evaluate.py, infer.py
 * and utils/metrics.py, bit for bit.  Masks are uint8 [B][H][W] (a pixel is set when it is non-zero), label maps int32.
 *
 * wesup_cc_label: connected components (connectivity 4 or 8, anything else is WESUP_ERR_INVALID) of the pixels where
 * (mask != 0) == (value != 0); labels = 0 for the other pixels and 1..n_labels[b] in raster order of a component's first pixel
 * (scipy.ndimage.label). */
size_t wesup_cc_label_workspace_bytes(int B, int H, int W);
int wesup_cc_label(const uint8_t* mask, int32_t* labels, int32_t* n_labels, int B, int H, int W, int connectivity, int value,
                   void* ws, size_t ws_bytes, void* stream);
/* evaluate.remove_small_regions (scripts/evaluate_glas.py:29-43): 8-connected foreground components smaller than min_size
 * pixels are erased, then background components of the RESULT smaller than min_size are filled; out is {0, 1}, out != mask */
size_t wesup_remove_small_regions_workspace_bytes(int B, int H, int W);
int wesup_remove_small_regions(const uint8_t* mask, uint8_t* out, int B, int H, int W, int min_size, void* ws, size_t ws_bytes,
                               void* stream);
/* binary erosion (op 0), dilation (op 1), opening (op 2) with footprint uint8 [fh][fw] (device memory, fh * fw <= 1024) and
 * scipy.ndimage's conventions: origin at size / 2, dilation with the mirrored footprint, border mode 'reflect' -- equal to
 * grey_erosion / grey_dilation / grey_opening on {0, 1} input.  out != mask; ws only for the opening. */
size_t wesup_binary_morph_workspace_bytes(int B, int H, int W, int op);
int wesup_binary_morph(const uint8_t* mask, uint8_t* out, const uint8_t* footprint, int B, int H, int W, int fh, int fw, int op,
                       void* ws, size_t ws_bytes, void* stream);
/* table [B][nS + 1][nG + 1] = pixels per (label in S, label in G), zeroed here; status[b] |= 1 for a label outside the table;
 * (nS + 1) * (nG + 1) <= 2^26 */
int wesup_contingency(const int32_t* S, const int32_t* G, int32_t* table, int32_t* status, int B, int HW, int nS, int nG,
                      void* stream);
/* pixels sorted by label 0..L (L < 16384), ascending index inside a label: the pixels of label l are
 * pix[b][start[b][l] .. start[b][l + 1]), start / bstart [B][L + 2], pix / bpix [B][HW].  bstart / bpix: the same lists of the
 * labels >= 1 restricted to boundary pixels (a 4-neighbour outside the object or outside the image).  status[b] |= 1 for a
 * label > L (negative labels are skipped). */
size_t wesup_label_sort_workspace_bytes(int B, int H, int W, int L);
int wesup_label_sort(const int32_t* labels, int32_t* start, int32_t* pix, int32_t* bstart, int32_t* bpix, int32_t* status, int B,
                     int H, int W, int L, void* ws, size_t ws_bytes, void* stream);
/* d2[i] = max over the pixels p of object pairs[i][0] of map X of min over the pixels q of object pairs[i][1] of map Y of
 * |p - q|^2 (one image pair; H, W <= 32767): lists of X and label map + boundary lists of Y from wesup_label_sort.  0 when the
 * first object lies inside the second, -1 for an object id outside [1, LX] x [1, LY].  The square root is the host's. */
int wesup_directed_hausdorff_sq(const int32_t* pairs, const int32_t* start_x, const int32_t* pix_x, const int32_t* labels_y,
                                const int32_t* bstart_y, const int32_t* bpix_y, int32_t* d2, int P, int H, int W, int LX, int LY,
                                void* stream);

/* ------------------------------------------------------------------ splitting touching objects (csrc/split.hip)
 * Masks uint8 [B][H][W] (non-zero = foreground), label maps and distance maps int32 [B][H][W]; B, H, W <= 65535.  All integer,
 * equal to the numpy restatement in wesup_amd/split.py bit for bit.  Every entry returns WESUP_ERR_INVALID for a null pointer, a
 * non-positive or oversized shape, a short workspace and the argument ranges named below, on the host and before any launch.
 *
 * wesup_edt_sq: d2 = 0 on the background, elsewhere min(cap, squared Euclidean distance to the nearest background pixel of the same
 * image); pixels outside the image are not background (scipy.ndimage.distance_transform_edt); 1 <= cap <= 65025. */
#define WESUP_SPLIT_SEG 64   /* the row pass stages segments of this many pixels, WESUP_SPLIT_ROWS rows per block */
#define WESUP_SPLIT_ROWS 4
#define WESUP_SPLIT_TILE 32  /* the growth kernel's tile edge */
#define WESUP_SPLIT_HALO 8   /* ... and its halo: the most rounds of one launch */
size_t wesup_edt_sq_workspace_bytes(int B, int H, int W);
int wesup_edt_sq(const uint8_t* mask, int32_t* d2, int B, int H, int W, int cap, void* ws, size_t ws_bytes, void* stream);
/* `launches` launches of `rounds` synchronous growth rounds each (rounds even, 2 .. WESUP_SPLIT_HALO), the first of them round
 * number first_round >= 1 (odd rounds look at the 4-neighbourhood, even rounds at the 8-neighbourhood): in a round every foreground
 * pixel without a label takes the smallest positive label among its neighbours as they stood before the round.  seeds: any int32
 * (labels up to 2^31 - 1), values <= 0 and values on the background count as no label; labels receives the map after the last
 * launch (0 on the background).  seeds, labels and ws are three maps that share no byte with each other, with mask or with
 * changed: anything else is WESUP_ERR_INVALID.  changed (one device word) is zeroed here before the last launch and set to 1 when a pixel took a label in that
 * launch: 0 means the map is the fixed point (a launch holds a round of either kind), whatever the earlier launches did. */
size_t wesup_label_grow_workspace_bytes(int B, int H, int W);
int wesup_label_grow(const uint8_t* mask, const int32_t* seeds, int32_t* labels, int32_t* changed, int B, int H, int W,
                     int first_round, int launches, int rounds, void* ws, size_t ws_bytes, void* stream);
/* out = 0 on the background and where a pixel's label a > 0 has an 8-neighbour with a label 0 < b < a; 1 elsewhere.  out shares
 * no byte with mask or labels */
int wesup_label_cut(const uint8_t* mask, const int32_t* labels, uint8_t* out, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------ surface-distance metrics (csrc/surface.hip)
 * Masks and border maps uint8 [B][H][W] (non-zero = set), distance maps int32 [B][H][W]; the shapes of the section above.  All
 * integer but the two sums of square roots, equal to the numpy restatement in wesup_amd/surface.py bit for bit.  Every entry
 * returns WESUP_ERR_INVALID for a null pointer, a non-positive or oversized shape, a short workspace and overlapping operands, on
 * the host and before any launch.
 *
 * wesup_edt_full: the exact squared Euclidean distance map, without a cap: d2 = 0 where the mask is 0, elsewhere the squared
 * distance to the nearest zero pixel of the same image (pixels outside the image are not zero pixels), WESUP_EDT_NONE everywhere
 * in an image without a zero pixel.  invert = 1 transforms (mask == 0) instead.  Shapes with (H-1)^2 + (W-1)^2 >=
 * WESUP_EDT_NONE are refused (the workspace query returns 0).  Three launches whatever the data; the column pass works on chunks
 * of WESUP_EDT_CHUNK rows and blocks of WESUP_EDT_COLS columns, the row pass on WESUP_EDT_ROWS rows of WESUP_EDT_SEG pixels per
 * block and scans outward until dx^2 reaches the best value so far: O(W) per pixel at worst. */
#define WESUP_EDT_NONE 2147483647
#define WESUP_EDT_CHUNK 64
#define WESUP_EDT_COLS 256
#define WESUP_EDT_SEG 64
#define WESUP_EDT_ROWS 4
size_t wesup_edt_full_workspace_bytes(int B, int H, int W);
int wesup_edt_full(const uint8_t* mask, int32_t* d2, int B, int H, int W, int invert, void* ws, size_t ws_bytes, void* stream);
/* out = 1 where the mask is set and one of the pixel's four neighbours is 0 or lies outside the image, 0 elsewhere */
int wesup_mask_border(const uint8_t* mask, uint8_t* out, int B, int H, int W, void* stream);
/* The raw quantities of the surface metrics of B image pairs: border_p / border_g the two border maps, d2_to_g / d2_to_p the
 * distance maps to the borders (wesup_edt_full of the border maps with invert = 1).  stats [B][WESUP_SURFACE_STATS] 8-byte slots
 * that stay on the device: int64 n_p, n_g, max_pg, max_gp, within_p, within_g (d2 <= t2), lo, hi, then float64 sum_pg, sum_gp (the
 * roots of d2_to_g over border_p and of d2_to_p over border_g, reduced in a fixed order: the same input gives the same bits).
 * lo and hi are the order statistics k = floor((n - 1) * q_frac) and min(k + 1, n - 1) of the n = n_p + n_g squared distances of
 * both directions together, the ranks derived on the device; q_frac_bits carries the bits of the float64 q_frac in [0, 1].  An
 * empty border: its count, maximum and sum are 0; both empty: lo = hi = 0.  Eleven launches (eight of them the select's), no read-back. */
#define WESUP_SURFACE_STATS 10
size_t wesup_surface_stats_workspace_bytes(int B, int H, int W);
int wesup_surface_stats(const uint8_t* border_p, const uint8_t* border_g, const int32_t* d2_to_g, const int32_t* d2_to_p,
                        void* stats, int B, int H, int W, long t2, long q_frac_bits, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ object outlines (csrc/contour.hip)
 * Label maps int32 [B][H][W]; B <= 65535 and 4 B H W < 2^31 (slots and crack indices are int32).  All integer, equal to the
 * sequential tracer wesup_amd/contour.py:trace_host word for word.  A crack is a unit edge between a pixel of label l > 0 and a
 * 4-neighbour of another label or the outside, directed with the pixel on its left (sides N W S E = 0 1 2 3, slot 4 (r W + c) +
 * side); its successor is the first of right turn, straight on, left turn that is a crack of l, so the cracks fall into rings.
 * Every entry returns WESUP_ERR_INVALID for a null pointer, a bad shape, a short workspace, negative counts and overlapping
 * operands, on the host and before any launch.
 *
 * The workspace: wesup_contour_workspace_bytes serves every map of the shape (4 B H W cracks), 0 for a bad shape;
 * wesup_contour_trace_workspace_bytes is what a map of n_cracks cracks needs (what the entries ask for: wesup_contour_count
 * takes n_cracks = 0), 0 for a bad shape and for n_cracks outside 0 .. 4 B H W.
 *
 * wesup_contour_count: counts [B][2] = the cracks and the corners of every image (a crack starts a corner when its predecessor
 * has another direction).  Local work: no ring is followed.
 *
 * wesup_contour_trace: n_cracks / n_corners the totals of counts over the batch, ring_cap the records rings holds (rings never
 * exceed corners / 4).  rings [ring_cap][WESUP_CONTOUR_RING] int32, 8-byte aligned: image, label, index of the first vertex,
 * vertices, cracks, xmin, ymin, xmax, ymax, leader slot (the ring's smallest, within its image), area2 as one int64 (positive:
 * an outer ring, counter-clockwise on screen; negative: a hole).  Rings in the order of (image, leader slot); verts [n_corners][2]
 * int32 (x, y) ring after ring, each from its leader on; n_rings [B].  When the map does not hold exactly n_cracks cracks and
 * n_corners corners, or holds more than ring_cap rings, status[0] |= 1 and no word of rings or verts is written (n_rings is
 * zeroed); status is never cleared here.  18 + ceil(log2 n_cracks) launches whatever the data. */
#define WESUP_CONTOUR_RING 12
size_t wesup_contour_workspace_bytes(int B, int H, int W);
size_t wesup_contour_trace_workspace_bytes(int B, int H, int W, int n_cracks);
int wesup_contour_count(const int32_t* labels, int32_t* counts, int B, int H, int W, void* ws, size_t ws_bytes, void* stream);
int wesup_contour_trace(const int32_t* labels, int32_t* rings, int32_t* verts, int32_t* n_rings, int32_t* status, int B, int H,
                        int W, int n_cracks, int n_corners, int ring_cap, void* ws, size_t ws_bytes, void* stream);

/* Ring simplification: the exact integer Douglas-Peucker of wesup_amd/contour.py:simplify_host, word for word.
 * rings [R][WESUP_CONTOUR_RING] and verts [V][2] as wesup_contour_trace leaves them: every ring of at least one vertex, the vertex
 * ranges consecutive from 0 to V in ring order; tol_q4 the tolerance in sixteenths of a pixel, 0 .. WESUP_SIMPLIFY_TOL_MAX.
 * rings_out [R] records (image, label, cracks and leader slot as given; first vertex, vertices, bounding box and area2 of the kept
 * vertices), verts_out of capacity V, flags [R] (bit 0: emitted as traced because fewer than 3 vertices were left or area2 lost
 * its sign; bit 1: emitted as traced because the record's bounding box spans 32768 or more), counts [WESUP_SIMPLIFY_COUNTS]:
 * kept vertices, rings with flag 1, rings with flag 2, status.  Records whose ranges are not as above set status = 1, and no
 * vertex, record or flag is written.  WESUP_ERR_INVALID on the host and before any launch for a null pointer, negative sizes,
 * R > V, V > 2^28, tol_q4 out of range, a short workspace, overlapping operands and rings / rings_out that are not 8-byte
 * aligned.  Seven launches whatever the data (two when R = 0); the level loop runs inside one kernel, at most n levels for a
 * ring of n vertices.  No floating point; integer atomics only, so two runs give the same words. */
#define WESUP_SIMPLIFY_TOL_MAX 4096
#define WESUP_SIMPLIFY_COUNTS 4
size_t wesup_contour_simplify_workspace_bytes(int R, int V);
int wesup_contour_simplify(const int32_t* rings, int R, const int32_t* verts, int V, int tol_q4, int32_t* rings_out,
                           int32_t* verts_out, int32_t* flags, int32_t* counts, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ object measurements (csrc/measure.hip)
 * Label maps int32 [B][H][W] with labels 0 .. L (0: background); B <= 65535, H, W <= 32768, L + 1 <= 2^20, B (L + 1) <= 2^26.
 * All integer, equal to wesup_amd/measure.py:measure_host word for word.  Every entry returns WESUP_ERR_INVALID for a null
 * pointer, a bad shape, a short workspace, negative counts and overlapping operands, on the host and before any launch.
 *
 * wesup_measure_limit(which): 0 the labels (L + 1) up to which a block keeps its moment table in LDS, 1
 * WESUP_MEASURE_HULL_CHUNK, 2 WESUP_MEASURE_WORDS, 3 the largest H / W, 4 the largest L + 1, 5 the largest n_prof; -1 otherwise.
 *
 * wesup_measure_workspace_bytes: what a call with a profile capacity of n_prof needs (wesup_measure_profile_count takes
 * n_prof = 0); 0 for a bad shape.
 *
 * wesup_measure_profile_count: count[0] = the sum over the labels present of (rmax - rmin + 2), the lines of pixel corners every
 * label spans: the profile capacity wesup_object_measure needs; twice that bounds the hull vertices.  status [B] is zeroed,
 * then bit 0 of an image is set by a label outside [0, L] (skipped, never used as an index).
 *
 * wesup_object_measure: d2 NULL or int32 [B][H][W], values >= 0 (a distance map); table [B][L + 1][WESUP_MEASURE_WORDS] int64:
 * 0 pixels, 1-5 the sums of r, c, r^2, r c, c^2, 6-9 rmin cmin rmax cmax ((H, W, -1, -1) for an absent label, whose other
 * words are 0; the row of label 0 is 0), 10-12 border pixels of the classes A B C, 13-15 bit quads Q1 Q3 QD, 16 hull area2,
 * 17 hull vertices, 18 the squared maximum Feret diameter, 19-20 the lattice indices y (W + 1) + x of its pair, 21 the maximum of
 * d2, 22 the first pixel r W + c that attains it (both 0 without d2), 23 the index of the first hull vertex.  hull_verts
 * [vert_cap][2] int32 (x, y): the strict vertices of the convex hull of the label's pixel corners, image by image and label
 * by label, each from its smallest (y, x) down the left side first.  status [B] as above; when the map needs more than n_prof
 * profile lines or has more than vert_cap hull vertices, bit 1 is set on every image and no word of table or hull_verts is
 * written.  19 launches whatever the data (9 for n_prof = 0). */
#define WESUP_MEASURE_WORDS 24
#define WESUP_MEASURE_HULL_CHUNK 256
int wesup_measure_limit(int which);
size_t wesup_measure_workspace_bytes(int B, int H, int W, int L, int n_prof);
int wesup_measure_profile_count(const int32_t* labels, int64_t* count, int32_t* status, int B, int H, int W, int L, void* ws,
                                size_t ws_bytes, void* stream);
int wesup_object_measure(const int32_t* labels, const int32_t* d2, int64_t* table, int32_t* hull_verts, int32_t* status, int B,
                         int H, int W, int L, int n_prof, int vert_cap, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ polygon fill (csrc/raster.hip)
 * General polygons in, label maps and class maps out; all integer, equal to wesup_amd/raster.py:fill_host bit for bit.
 * Coordinates are fixed point with WESUP_RASTER_FRAC_BITS fractional bits: one pixel is 256 units, pixel (r, c) covers
 * [c, c+1] x [r, r+1] and has its centre at (Xc, Yc) = (256 c + 128, 256 r + 128).  A feature is a list of rings (outer rings,
 * holes and the parts of a multi-polygon alike), a ring a cyclic list of n >= 1 vertices.  An edge with its ends ordered so that
 * y0 < y1 counts for a pixel iff y0 <= Yc < y1 and (x1 - x0)(Yc - y0) <= (Xc - x0)(y1 - y0) (int64 products; horizontal edges
 * never count); a feature covers a pixel iff an odd number of its edges counts (even-odd; tops and left sides inclusive, bottoms
 * and right sides exclusive); labels [B][H][W] int32 = 1 + the largest index among the features of the image that cover the
 * pixel, 0 where none does; with values, out8 [B][H][W] uint8 = values[label - 1], 0 where the label is 0.
 *
 * Operands in CSR form, device memory: verts [V][2] int32 (x, y), 8-byte aligned; ring_first [R + 1]; feature_first_ring
 * [F + 1]; feature_image [F]; values [F] uint8 and out8 together or both NULL.  B H W < 2^31, H, W <= 2^21.  verts may be NULL
 * for V = 0, feature_image and values for F = 0.  WESUP_ERR_INVALID for a null pointer otherwise, a bad shape, negative counts,
 * a short workspace (wesup_polygon_fill_workspace_bytes(B, H, W, F); 0 for a bad shape) and overlapping operands, on the host
 * and before any launch.  status[0] is zeroed here; a feature with a vertex outside +-2^28, an image index outside [0, B), ring
 * offsets that leave [0, R] or decrease, or a ring of it whose vertex offsets leave [0, V] or decrease sets status[0] |= 1 and
 * paints nothing (nothing behind a refused offset is read).  F = 0 or V = 0 gives a zeroed map.
 *
 * Six launches whatever the data, seven with values (F = 0: two, three with values); no read-back: the fill kernel's grid is
 * fixed and strides over the tiles (WESUP_RASTER_TILE_ROWS x WESUP_RASTER_TILE_COLS pixels, aligned to the image) of the
 * features' clipped bounding boxes, counted and scanned on the device; feature and tile counts are bounded by no grid limit.
 * Labels are raised by an integer atomicMax: the result does not depend on the order in which blocks run.
 *
 * wesup_raster_limit(which): 0 WESUP_RASTER_TILE_ROWS, 1 WESUP_RASTER_TILE_COLS, 2 WESUP_RASTER_BLOCK (threads that walk a
 * feature's edges together), 3 the largest |coordinate| (2^28), 4 WESUP_RASTER_FRAC_BITS, 5 the fill kernel's grid; -1 otherwise. */
#define WESUP_RASTER_FRAC_BITS 8
#define WESUP_RASTER_TILE_ROWS 64
#define WESUP_RASTER_TILE_COLS 64
#define WESUP_RASTER_BLOCK 256
int wesup_raster_limit(int which);
size_t wesup_polygon_fill_workspace_bytes(int B, int H, int W, int F);
int wesup_polygon_fill(const int32_t* verts, const int32_t* ring_first, const int32_t* feature_first_ring,
                       const int32_t* feature_image, const uint8_t* values, int32_t* labels, uint8_t* out8, int32_t* status, int B,
                       int H, int W, int F, int R, int V, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ painted object comparisons (csrc/paint.hip)
 * wesup_object_match: tables [B][nS + 1][nG + 1] as wesup_contingency writes them (nS, nG: the maxima of the batch), nS_dev /
 * nG_dev [B]: each image's own object counts (wesup_cc_label's n_labels); cells outside an image's own counts are not read.
 * match [B][nS + 1]: for a row p in 1..nS_dev[b] the column g >= 1 with 2 * table[p][g] > area[g] (area[g] = the sum of column g
 * over the image's rows) of the largest area, the lowest g among equal areas, or max(nS_dev[b], nG_dev[b]) + p when there is
 * none; 0 for row 0 and the rows past nS_dev[b]  (reference scripts/paint_masks.py:50-70). */
size_t wesup_object_match_workspace_bytes(int B, int nG);
int wesup_object_match(const int32_t* table, const int32_t* nS_dev, const int32_t* nG_dev, int32_t* match, int B, int nS, int nG,
                       void* ws, size_t ws_bytes, void* stream);
/* out [B][HW][3] uint8 = the low three bytes (R, G, B in this order) of lut[b][labels[b][pixel]], lut [B][n_lut] one 32-bit word
 * per label; a label outside [0, n_lut) is never used as an index: its pixel is black and status[b] |= 1 (status is zeroed
 * here). */
int wesup_label_paint(const int32_t* labels, const int32_t* lut, uint8_t* out, int32_t* status, int B, int HW, int n_lut,
                      void* stream);

/* ------------------------------------------------------------------ window inference on large images (csrc/tiles.hip)
 * The device ends of infer_tile.py: cutting an image into the network's input windows and merging the per-window predictions.
 * The window lattice is tops[n_h] x lefts[n_w] (int32, device memory, sorted, first 0, last size - p: infer_tile.window_grid);
 * window k, row-major, has its corner at (tops[k / n_w], lefts[k % n_w]).  Both entries return WESUP_ERR_INVALID for a null
 * pointer, p < 1, p > H, p > W, n_h < 1 or n_w < 1 (and count < 1, first < 0 / C < 1); no workspace, no host sync.
 *
 * wesup_window_gather: img uint8 [H][W][3] -> out fp32 [count][3][p][p], the windows first .. first + count - 1 scaled to
 * [0, 1] exactly as ATen's uint8 -> float -> div_(255.) does on the device (a multiplication by the fp32 reciprocal); an index
 * >= n_h * n_w repeats the last window (the padding of a ragged final batch). */
int wesup_window_gather(const uint8_t* img, const int32_t* tops, const int32_t* lefts, float* out, int H, int W, int n_h, int n_w,
                        int p, int first, int count, void* stream);
/* pred fp32 [n_h * n_w][p][p][C] -> out fp64 [H][W][C]: the mean over the windows that cover a pixel -- the values (rintf of
 * them with round_first: half to even) added as doubles in ascending window order and divided by the count once, which is
 * infer_tile.combine_patches_to_image bit for bit */
int wesup_window_merge(const float* pred, const int32_t* tops, const int32_t* lefts, double* out, int H, int W, int C, int n_h,
                       int n_w, int p, int round_first, void* stream);
/* Test-time augmentation over the views of a square window (infer_tile.apply_view / invert_view): view
 * v = r + 4 f, a left-right mirror first when f, then r counter-clockwise quarter turns.  A view list comes by value: n_views
 * and `views`, four bits per view, the first view in the lowest bits.  WESUP_ERR_INVALID without a launch for n_views outside
 * 1 .. 8, an index above 7 or a repeated index, and for what the entries above refuse.  The entries above (and
 * wesup_window_merge_classes below) are these with n_views = 1, views = 0: one kernel and one set of checks per pair.
 *
 * wesup_window_gather_views: wesup_window_gather over the slots of windows x views -- slot s = first + n is window s / n_views
 * under view views[s % n_views], a slot past the last repeats the last; out[n] is _to_tensor(apply_view(window, v)) bit for bit. */
int wesup_window_gather_views(const uint8_t* img, const int32_t* tops, const int32_t* lefts, float* out, int H, int W, int n_h,
                              int n_w, int p, int n_views, uint32_t views, int first, int count, void* stream);
/* pred fp32 [n_h * n_w][n_views][p][p][C], every prediction in the space of its view -> out fp64 [H][W][C]: per covering window
 * in ascending order its views in list order, each turned back (read through the inverse index), added as doubles onto 0.0 and
 * divided once by covering windows x n_views: infer_tile.combine_views_to_image bit for bit; round_first as above */
int wesup_window_merge_views(const float* pred, const int32_t* tops, const int32_t* lefts, double* out, int H, int W, int C,
                             int n_h, int n_w, int p, int n_views, uint32_t views, int round_first, void* stream);

/* ------------------------------------------------------------------ whole-image multi-scale pixel inference (csrc/pixel.hip)
 * pixel_infer.py:38-56 rescales an image by every factor of --scales (bilinear, align_corners=True), runs the pixel-wise
 * model, resizes class 1 back and averages.  Source coordinates are torch's fp32 formula (csrc/bilinear.hpp).
 *
 * wesup_image_resize_u8: img uint8 [H][W][3] -> out fp32 [3][h][w] = bilinear_ac(img / 255.f): to_tensor + F.interpolate
 * (pixel_infer.py:40,46); at h == H, w == W the value is img / 255.f bit for bit. */
int wesup_image_resize_u8(const uint8_t* img, float* out, int H, int W, int h, int w, void* stream);
/* out[H][W] = (accumulate ? out : 0) + alpha * bilinear_ac(in); in is an [h][w] plane whose elements sit `stride` floats
 * apart (2: class 1 of an [h][w][2] prediction, read in place).  alpha = 1 / len(scales): the mean needs no pass of its own */
int wesup_plane_resize_acc(const float* in, float* out, int h, int w, int H, int W, int stride, float alpha, int accumulate,
                           void* stream);
/* First fc layer of the pixel head from per-resolution products:
 *   out[b][y][x][n] = ReLU(bias[n] + p0[b][y][x][n] + sum_r bilinear_ac(levels[r].p[b])(y, x)[n]),  r < n_levels <= 4,
 * p0 / out [B][H][W][N], levels[r].p [B][h][w][N], N % 4 == 0, every pointer 16-byte aligned.  Every level is interpolated
 * straight to (H, W).  out may be p0 (an element reads only its own element of p0).  levels is a HOST array */
typedef struct WesupCoarseMap { const float* p; int h, w; } WesupCoarseMap;
int wesup_pixel_gather_fwd(const float* p0, const float* bias, float* out, const WesupCoarseMap* levels /* host */, int n_levels,
                           int B, int H, int W, int N, void* stream);

/* ------------------------------------------------------------------ whole-slide evaluation: the DP2019 patch pipeline (csrc/slide.hip)
 * test_dp2019_pipeline.py:18-71,158-172 cuts a slide into zero-padded p x p patches, runs infer.py (input_size) or pixel_infer.py
 * (one scale) on each and pastes the predictions back.  The patch lattice of an (H, W) slide: n_h = ceil(H / p) rows of
 * n_w = ceil(W / p) patches; patch k (row-major) has its corner at (k / n_w * p, k % n_w * p); texels beyond the slide are 0.
 * p > H and p > W are fine (one padded patch).  Sizes: 1 <= H, W, p <= 2^30 and n_h * n_w < 2^31; H * W itself is not limited
 * (every offset into the slide is 64-bit: a slide may exceed 2^31 bytes); a pass's tensors are indexed in 64 bit as well.
 * All three entries: WESUP_ERR_INVALID without a launch for a null pointer, a non-positive size, count < 1, first < 0, a mode /
 * align_corners outside {0, 1} or stride < 1; no workspace, no host sync.
 *
 * wesup_patch_gather_resize: img uint8 [H][W][3] -> out fp32 [count][3][h][w], the patches first .. first + count - 1, each
 * (patch / 255.f) resized bilinearly from p x p to h x w (the same byte -> float expression as wesup_image_resize_u8).
 * align_corners = 1: pixel_infer.py's resize, the coordinates of every other resampling kernel here -- a patch wholly inside
 * the slide equals wesup_image_resize_u8 of it bit for bit.  align_corners = 0: infer.py's F.interpolate(mode='bilinear'),
 * torch's src = max(scale * (dst + 0.5) - 0.5, 0).  The neighbour clamp is at the PATCH border and a texel beyond the slide
 * reads as 0 (pad, then resize -- not a clamp to the slide's edge).  An index >= n_h * n_w repeats the last patch (the padding of
 * a ragged final batch). */
int wesup_patch_gather_resize(const uint8_t* img, float* out, int H, int W, int p, int h, int w, int align_corners, int first,
                              int count, void* stream);
/* pred fp32 [count][h][w], elements `stride` floats apart (2: class 1 of an (h, w, 2) prediction, read in place) -> out uint8
 * [H][W]: every slide pixel inside one of the patches first .. first + count - 1 becomes 255 * rintf(v) (half to even), v = the
 * patch's prediction resized to p x p.  mode 0 (infer.py): F.interpolate(mode='nearest'), source index min(floorf(dst * scale),
 * in - 1), scale = (float)in / p.  mode 1 (pixel_infer.py, one scale): bilinear, align_corners -- wesup_plane_resize_acc's
 * arithmetic at alpha = 1.  Lattice pixels beyond the slide (combine_single's crop) and patches past the end of the lattice are
 * not written; nothing else of out is touched. */
int wesup_patch_scatter_u8(const float* pred, uint8_t* out, int H, int W, int p, int h, int w, int stride, int mode, int first,
                           int count, void* stream);
/* S, G uint8 [n] -> out4 int64 [4] (8-byte aligned, zeroed here) = {#(s == g), #(s > 0 && g > 0), #(s > 0), #(g > 0)}, after
 * x -> 255 - x on both maps with `negative` (compute_metrics(negative=True), test_dp2019_pipeline.py:100-111).  Integer counts,
 * exact in any order; accuracy = eq / n and dice = 2 * inter / (sumG + sumS + 1e-7) are the host's, in float64. */
int wesup_mask_scores(const uint8_t* S, const uint8_t* G, int64_t* out4, long n, int negative, void* stream);
/* The two entries above over a patch list: list int32 [n_list] in device memory, n_list >= 1 (a null list or
 * n_list < 1 is WESUP_ERR_INVALID).  Slot i of the pass, 0 <= i < count, stands for list[first + i].  The gather reads
 * list[min(first + i, n_list - 1)]: a ragged last pass repeats the last listed patch.  The scatter skips a slot with
 * first + i >= n_list.  A list value outside [0, n_h * n_w) never becomes an address: its slot is left unwritten (gather) or
 * skipped (scatter).  A listed patch gets the bits the plain entry gives it. */
int wesup_patch_gather_resize_list(const uint8_t* img, float* out, int H, int W, int p, int h, int w, int align_corners, int first,
                                   int count, const int32_t* list, int n_list, void* stream);
int wesup_patch_scatter_u8_list(const float* pred, uint8_t* out, int H, int W, int p, int h, int w, int stride, int mode, int first,
                                int count, const int32_t* list, int n_list, void* stream);

/* ------------------------------------------------------------------ tissue selection for whole-slide evaluation (csrc/tissue.hip)
 * Which patches of the lattice above hold tissue (the host statement is wesup_amd/slide.py: pixel_value,
 * patch_histograms, otsu_threshold, select_patches, and the kernels equal it bit for bit).  A pixel's value v in 0 .. 255:
 * channel 0 (luma) (77 R + 150 G + 29 B + 128) >> 8, channel 1 (chroma) max(R, G, B) - min(R, G, B).  Tissue: luma v <= t, chroma
 * v > t, t = -1 every pixel.  All entries: WESUP_ERR_INVALID without a launch for a null pointer, sizes outside the lattice's,
 * p > 65535 (a cell of hist is a uint32), H * W > 2^32 (Otsu's integers stay below 2^64), a channel outside {0, 1}, a threshold
 * outside [-1, 254] or min_ppm outside [0, 10^6].  Integer adds only, no workspace, no host sync.
 *
 * wesup_patch_value_hist: img uint8 [H][W][3] -> hist uint32 [n_h * n_w][256] (zeroed here), hist[k][v] = the slide pixels of
 * patch k with value v; the zero padding is never counted.  One read of the slide.  The grid is at most WESUP_TISSUE_MAX_BLOCKS
 * blocks striding over items of about WESUP_TISSUE_ITEM_PIXELS pixels, max(1, WESUP_TISSUE_ITEM_PIXELS / p) rows of one patch. */
#define WESUP_TISSUE_MAX_BLOCKS 2048
#define WESUP_TISSUE_ITEM_PIXELS 8192
#define WESUP_TISSUE_LIST_CHUNK 256 /* patches per step of the ordered compaction */
int wesup_patch_value_hist(const uint8_t* img, uint32_t* hist, int H, int W, int p, int channel, void* stream);
/* hist -> total int64 [256] (8-byte aligned) = the sum over the patches; t = threshold, or with threshold = -1 Otsu's over total:
 * for t = 0 .. 254 ascending, w0 = sum_{i <= t} h_i, s0 = sum_{i <= t} i h_i, D = w0 (N - w0), skipped where D = 0;
 * num = |S w0 - s0 N| exactly (128 bits), x = (double)(num >> 64) * 2^64 + (double)(num mod 2^64), q = x * x / (double)D, no
 * contraction; the first t with the largest q under a strict >, or -1 when no t has D > 0 (a one-level slide).
 * counts uint32 [n] = the tissue pixels of every patch (a prefix or suffix sum of its histogram).  list int32 [n]: the kept patches
 * in ascending order, kept = counts[k] >= 1 and counts[k] * 10^6 >= min_ppm * area_k, area_k the patch's pixels inside the slide
 * (t = -1 keeps every patch); list beyond n_keep is not written.  info int32 [8] = {t, n_keep, n, flat (1 when t = -1), 0, 0, 0, 0}. */
int wesup_tissue_select(const uint32_t* hist, int H, int W, int p, int channel, int threshold, int min_ppm, int32_t* info,
                        int64_t* total, uint32_t* counts, int32_t* list, void* stream);
/* out uint8 [H][W] = 255 where the pixel is tissue under t = info[0] (read on the device), else 0 */
int wesup_tissue_mask_u8(const uint8_t* img, const int32_t* info, uint8_t* out, int H, int W, int channel, void* stream);

/* ------------------------------------------------------------------ class maps for more than two classes (csrc/classmap.hip)
 * The merge, the resize back, the paste and the scoring of the three sections above as reductions over the C values of a pixel
 * (DESIGN.md 3.15).  A pixel's class is the first maximum over ascending c under a strict > (no comparison with a NaN is true: a
 * NaN behind the first entry is never the maximum, a row whose first entry is NaN gives class 0); class
 * maps are uint8 class indices.  All entries: WESUP_ERR_INVALID without a launch for C outside [2, WESUP_MAX_CLASSES], a null
 * pointer or a size the one-plane entry refuses; no workspace, no host sync.  A class index that comes in as data (a vote, a
 * painted map, a label byte) is never used as an address: one outside [0, C) -- a NaN included -- is not counted and sets
 * *status (int32, device memory) to non-zero.
 *
 * wesup_window_merge_classes: the lattice of wesup_window_merge.  votes = 0: pred fp32 [n_h * n_w][p][p][C] probabilities; per
 * pixel and class wesup_window_merge's fp64 mean over the covering windows, then the first maximum -- the argmax of
 * infer_tile.combine_patches_to_image.  votes = 1: pred fp32 [n_h * n_w][p][p] class indices (rintf of them); every covering
 * window votes, the first maximum of the integer counts.  out uint8 [H][W]; *status is zeroed here. */
int wesup_window_merge_classes(const float* pred, const int32_t* tops, const int32_t* lefts, uint8_t* out, int32_t* status, int H,
                               int W, int C, int n_h, int n_w, int p, int votes, void* stream);
/* wesup_window_merge_classes over windows x views (wesup_window_merge_views' view list and order): pred fp32
 * [n_h * n_w][n_views][p][p][C] probabilities (votes = 0) or [n_h * n_w][n_views][p][p] class indices (votes = 1: every
 * (window, view) votes), each in the space of its view: infer_tile.combine_views_to_classes bit for bit */
int wesup_window_merge_classes_views(const float* pred, const int32_t* tops, const int32_t* lefts, uint8_t* out, int32_t* status,
                                     int H, int W, int C, int n_h, int n_w, int p, int n_views, uint32_t views, int votes,
                                     void* stream);
/* in fp32 [h][w][C] -> out fp32 [H][W][C] = (accumulate ? out : 0) + alpha * bilinear_ac(in): every plane c is
 * wesup_plane_resize_acc of in[..., c] (stride C) bit for bit; the four corner vectors are read once per pixel */
int wesup_planes_resize_acc(const float* in, float* out, int h, int w, int H, int W, int C, float alpha, int accumulate,
                            void* stream);
/* in fp32 [n][C] -> out uint8 [n]: the first maximum of every row */
int wesup_class_argmax_u8(const float* in, uint8_t* out, long n, int C, void* stream);
/* wesup_patch_scatter_u8 with a class index as the pasted byte: the same lattice, crop and "nothing else of out is touched".
 * mode 0: pred fp32 [count][h][w] class indices (rintf of them), the nearest texel; an index outside [0, C) pastes 0 and sets
 * *status.  mode 1: pred fp32 [count][h][w][C] probabilities, per class the value of wesup_planes_resize_acc at alpha = 1, then
 * the first maximum.  *status is OR-ed into, not zeroed: it collects over the passes of a slide (the caller zeroes it once). */
int wesup_patch_scatter_classes_u8(const float* pred, uint8_t* out, int32_t* status, int H, int W, int p, int h, int w, int C,
                                   int mode, int first, int count, void* stream);
/* ... over a patch list, as wesup_patch_scatter_u8_list; a list value outside the lattice is skipped and sets *status */
int wesup_patch_scatter_classes_u8_list(const float* pred, uint8_t* out, int32_t* status, int H, int W, int p, int h, int w, int C,
                                        int mode, int first, int count, const int32_t* list, int n_list, void* stream);
/* S, G uint8 [n] class-index maps (n <= 2^40) -> conf int64 [C][C] (8-byte aligned), conf[g][s] = positions with ground truth g
 * predicted as s: utils.metrics.confusion.  Integer counts in LDS, integer adds of the non-zero cells: exact in any order.  conf
 * and *status are zeroed here. */
int wesup_label_confusion(const uint8_t* S, const uint8_t* G, int64_t* conf, int32_t* status, long n, int C, void* stream);

/* ------------------------------------------------------------------ weak-label preparation (csrc/prepare.hip)
 * The integer label-map passes of wesup_amd/prepare.py (scripts/generate_points.py, generate_spl_masks.py and
 * search_slic_params.py of the reference).  Label maps are int32, images at most 2^22 on a side.  All entries: WESUP_ERR_INVALID
 * without a launch for a null pointer, a non-positive size, a table size outside its range or a shape whose sums the counters
 * cannot hold; a label outside its table sets bit 0 of the image's status word and is skipped; results are exact integers in
 * any order of the atomics.
 *
 * wesup_prepare_lds_entries: the largest table that a block keeps privately in LDS -- labels (L + 1) of wesup_label_stats for
 * which = 0, ids (K) of wesup_sp_vote for which = 1; larger tables are added to in global memory. */
int wesup_prepare_lds_entries(int which);
/* labels [B][H][W] in [0, L] -> stats int64 [B][L + 1][3] (8-byte aligned, zeroed here) = {pixels, sum of the row indexes, sum of
 * the column indexes} per label: the size and the centroid numerator of every region in one pass.  L < 2^26. */
int wesup_label_stats(const int32_t* labels, int64_t* stats, int32_t* status, int B, int H, int W, int L, void* stream);
/* labels [B][H][W] in [0, K), values uint8 [B][H][W]: every superpixel votes the mean of its values rounded half to even in
 * integers (q, r = divmod(sum, count); q + 1 if 2r > count, q + (q & 1) if 2r == count, else q: numpy's mean().round(); 0 for an
 * id without a pixel).  painted uint8 [B][H][W] (may be NULL) = the vote of each pixel's superpixel; agree int64 [B] (8-byte
 * aligned, zeroed here) = pixels whose vote equals their value.  The counters are 32 bits wide: 255 * H * W < 2^32, K <= 2^26. */
size_t wesup_sp_vote_workspace_bytes(int B, int H, int W, int K);
int wesup_sp_vote(const int32_t* labels, const uint8_t* values, uint8_t* painted, int64_t* agree, int32_t* status, int B, int H,
                  int W, int K, void* ws, size_t ws_bytes, void* stream);
/* labels [H][W] in [0, K), points int32 [P][3] of (row, col, class) inside the image and the classes (status |= 2 otherwise: the
 * caller wraps and checks) -> out uint8 [H][W][C]: out[h][w][c] = 1 iff a point of class c lies in the superpixel of (h, w).  A
 * K x C flag table, then the paint; P = 0 (points may be NULL) gives all zeros.  C <= 256, K * C <= 2^26. */
size_t wesup_spl_paint_workspace_bytes(int K, int C);
int wesup_spl_paint(const int32_t* labels, const int32_t* points, uint8_t* out, int32_t* status, int H, int W, int K, int C, int P,
                    void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ exact t-SNE of superpixel features (csrc/tsne.hip)
 * The embedding the reference's plot_tsne.py asks sklearn.manifold.TSNE() for, method 'exact', two output dimensions.  All
 * matrices are dense row-major fp32: x [n][d], d2 and p [n][n], y / upd / gains [n][2] (8-byte aligned).  2 <= n <=
 * WESUP_TSNE_MAX_N (p is 4 GiB there), 1 <= d <= WESUP_TSNE_MAX_D, 0 < perplexity < n; outside that, or with a null pointer,
 * every entry returns WESUP_ERR_INVALID without a launch.  No floating-point atomics: the same input gives the same bits. */
#define WESUP_TSNE_MAX_N 32768
#define WESUP_TSNE_MAX_D 4096
#define WESUP_TSNE_STATS 4
/* d2[i][j] = sum_k (x[i][k] - x[j][k])^2, from differences in ascending k: bit-symmetric, the diagonal exactly 0 */
int wesup_tsne_sqdist(const float* x, int n, int d, float* d2, void* stream);
/* scikit-learn's search for beta[i] (start 1, double / halve while a bound is infinite, else bisect; at most 100 steps; stop at
 * |H_i - log perplexity| <= 1e-5) on d2[i][:] minus the row's smallest off-diagonal entry, then p = max((C + C^T) / max(sum, eps),
 * eps) with C the conditional rows, eps = 2.220446049250313e-16 and p[i][i] = 0; p is bit-symmetric.  beta [n]: the value each
 * row's C was built with.  d2 and p must not overlap. */
size_t wesup_tsne_affinities_workspace_bytes(int n);
int wesup_tsne_affinities(const float* d2, int n, float perplexity, float* p, float* beta, void* ws, size_t ws_bytes, void* stream);
/* Enqueues `iters` gradient iterations (0 <= iters <= 65536) on y with scikit-learn's delta-bar-delta rule: g = 4 (att - rep / Z)
 * with p scaled by `exaggeration` (> 0), gains += 0.2 where upd g < 0 else *= 0.8, floored at min_gain (>= 0), upd = momentum upd -
 * lr g gains (momentum >= 0, lr > 0), y += upd.  The last iteration also writes stats [WESUP_TSNE_STATS] = {KL divergence of the
 * UNexaggerated p, |g|_2 of the exaggerated gradient, Z, sum p log p}, all at the y that iteration started from.  iters = 0 moves
 * nothing and writes the stats of y as it stands. */
size_t wesup_tsne_iterate_workspace_bytes(int n);
int wesup_tsne_iterate(const float* p, float* y, float* upd, float* gains, float* stats, int n, int iters, float exaggeration,
                       float momentum, float lr, float min_gain, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------ stain normalisation and stain jitter (csrc/stain.hip)
 * Macenko normalisation of H&E images (Macenko et al., ISBI 2009) and its augmentation twin, a jitter of the two stain
 * concentrations (the reference has neither).  Images are (B, H, W, 3) uint8. */
/* Exact order statistics: out[r] = the element that np.sort(keys)[ranks[r]] names, bit for bit (-0 sorts in front of +0, NaNs by
 * their bits at the two ends), 1 <= n_ranks <= WESUP_SELECT_MAX_RANKS.  ranks is a DEVICE array (a rank outside [0, n) is taken
 * to the nearest end).  Radix select, four passes of 8 bits over the same keys: per pass a histogram launch of
 * min(WESUP_SELECT_MAX_BLOCKS, ceil(n / WESUP_SELECT_BLOCK)) blocks and a one-block step.
 * workspace = 256 + blocks * WESUP_SELECT_MAX_RANKS * 256 * 4 bytes. */
#define WESUP_SELECT_BLOCK 256
#define WESUP_SELECT_MAX_BLOCKS 256
#define WESUP_SELECT_MAX_RANKS 4
size_t wesup_select_f32_workspace_bytes(long n);
int wesup_select_f32(const float* keys, long n, const long* ranks, int n_ranks, float* out, void* ws, size_t ws_bytes,
                     void* stream);
/* The same for int32 keys 0 .. 2^31 - 1 (a negative key is outside the contract): np.sort(keys)[ranks], through the same passes --
 * on a pattern with the sign bit clear the select's key map is a pure bit map that keeps the integer order, NaN patterns included. */
size_t wesup_select_i32_workspace_bytes(long n);
int wesup_select_i32(const int32_t* keys, long n, const long* ranks, int n_ranks, int32_t* out, void* ws, size_t ws_bytes,
                     void* stream);
/* The fit of image b, WESUP_STAIN_BLOCK floats (64 bytes) that stay on the device:
 *   [0..5] HE[c][k] (c = r, g, b; k = 0 "H", 1 "E"), [6..11] pinv[k][c], [12..13] maxC[k], [14] n_tissue, [15] valid (1 or 0;
 *   an invalid fit is all zeros but n_tissue). */
#define WESUP_STAIN_BLOCK 16
/* OD = -log((v + 1) / io) per channel; tissue = all three OD >= beta; the fit samples every stride-th row and column
 * (ceil(H / stride) * ceil(W / stride) <= 2^24 samples per image).  Tissue covariance, its two leading eigenvectors, the
 * alpha-th and (100 - alpha)-th percentile of the angle in their plane, the two stain vectors (the redder one first), the
 * pseudo-inverse, the 99th percentile of both concentrations over ALL samples.  Invalid: n_tissue < min_tissue (>= 2),
 * |det(HE^T HE)| < 1e-6 (parallel vectors), or a maxC below 1e-6.  One chain of launches, no host read-back.
 * The workspace also holds the stages (wesup_stain_fit_stage_offset, bytes from ws): MOMENTS [B][10] doubles {n, sum r g b,
 * sum rr rg rb gg gb bb} of the tissue OD; SCRATCH [B] slots of 256 bytes that start with the eigenvectors V[c][k] as 6 doubles;
 * PHI [B][samples] floats (+inf where not tissue); CONC [B][2][samples] floats. */
#define WESUP_STAIN_STAGE_MOMENTS 0
#define WESUP_STAIN_STAGE_SCRATCH 1
#define WESUP_STAIN_STAGE_PHI 2
#define WESUP_STAIN_STAGE_CONC 3
size_t wesup_stain_fit_workspace_bytes(int B, int H, int W, int stride);
size_t wesup_stain_fit_stage_offset(int B, int H, int W, int stride, int stage);
int wesup_stain_fit(const uint8_t* img, float* blocks, int B, int H, int W, int stride, float io, float alpha, float beta,
                    int min_tissue, void* ws, size_t ws_bytes, void* stream);
/* Per pixel, with the source fit of image b, the destination block (dst_stride = 0: one for all, WESUP_STAIN_BLOCK: one each)
 * and jitter[b] = {a_H, b_H, a_E, b_E} (NULL: 1, 0, 1, 0):  c = pinv_s OD;  c' = c (maxC_d / maxC_s) a + b;
 * OD' = HE_d c' + keep_residual (OD - HE_s c);  v' = rint(clamp(io exp(-OD') - 1, 0, 255)).  An invalid source or destination
 * makes the image a plain copy.  out == img is allowed (any other overlap is refused). */
int wesup_stain_apply(const uint8_t* img, uint8_t* out, const float* src_blocks, const float* dst_blocks, int dst_stride,
                      const float* jitter, float keep_residual, int B, int H, int W, float io, void* stream);

/* ------------------------------------------------------------------ entries by the names of SURVEY.md 8(b)
 * One call per ATen op of the reference for a binding that replaces them one by one; each is a thin entry over the
 * kernels above (csrc/named.hip).  Matrices are row-major with the channel / feature index contiguous (NHWC pixels). */
/* K9 (models/wesup.py:34-42): area[B][Kmax] = pixels per superpixel id, counts[B][Kmax][C] = mask pixels per (id, class)
 * (counts may be NULL without a mask); status[b] |= 1 when an id is outside [0, Kmax) */
int wesup_sp_stats(const int32_t* labels, const uint8_t* mask, int B, int HW, int C, int Kmax, int32_t* area,
                   int32_t* counts, int32_t* status, void* stream);
/* K3 (models/wesup.py:208-209,253): Conv2d(Cin, Cout, 1) on P = B*h*w pixels; w [Cout][Cin]; w_t = w transposed */
size_t wesup_conv1x1_workspace_bytes(int P, int Cin, int Cout);
int wesup_conv1x1_fwd(const float* x, const float* w, const float* bias, float* y, int P, int Cin, int Cout,
                      void* ws, size_t ws_bytes, void* stream);
int wesup_conv1x1_dgrad(const float* dy, const float* w_t, float* dx, int P, int Cin, int Cout, int accumulate,
                        void* ws, size_t ws_bytes, void* stream);
int wesup_conv1x1_wgrad(const float* dy, const float* x, float* dw, float* db, int P, int Cin, int Cout,
                        void* ws, size_t ws_bytes, void* stream);
/* K7 (models/wesup.py:213-220,288): Linear(In, Out) [+ ReLU]; bwd: dw, db and (dx != NULL) dx = dy . w masked by
 * relu_src > 0 when the layer's input came out of a ReLU (relu_src = that input, [R][In]) */
size_t wesup_linear_workspace_bytes(int R, int In, int Out);
int wesup_linear_fwd(const float* x, const float* w, const float* bias, float* y, int R, int In, int Out, int relu,
                     void* ws, size_t ws_bytes, void* stream);
int wesup_linear_bwd(const float* dy, const float* x, const float* w_t, const float* relu_src, float* dx, float* dw,
                     float* db, int R, int In, int Out, void* ws, size_t ws_bytes, void* stream);
/* K4 (models/wesup.py:254-255): F.interpolate(mode='bilinear', align_corners=True), dense form, into / from the channel
 * slice [coff, coff + C) of a [B][H][W][ld_out] tensor */
int wesup_upsample_bilinear_ac_fwd(const float* s, float* out, int B, int h, int w, int H, int W, int C, int ld_out,
                                   int coff, void* stream);
int wesup_upsample_bilinear_ac_bwd(const float* dout, float* ds, int B, int h, int w, int H, int W, int C, int ld_out,
                                   int coff, void* stream);
/* K11 (models/wesup.py:231 Softmax + :66-96 _cross_entropy) fused: probs = softmax(logits) is written out, out2 as in
 * wesup_cross_entropy_fwd; bwd gives d loss / d logits */
int wesup_softmax_ce_fwd(const float* logits, const float* y_true, const float* class_weights, float eps, float* probs,
                         float* out2, int n, int C, void* stream);
int wesup_softmax_ce_bwd(const float* probs, const float* y_true, const float* class_weights, const float* out2,
                         const float* dloss, float eps, float* dlogits, int n, int C, void* stream);

/* ------------------------------------------------------------------ step plans (ABI 4)
 * The reference walks one training iteration in Python every step (models/base.py:184-211); so does the engine above this
 * library, ~330 launches on three streams.  A plan records that walk ONCE -- every launch this thread issues through the
 * library between wesup_plan_begin and wesup_plan_end is executed as usual and appended with its kernel, grid, stream and a
 * byte copy of its arguments; ordering edges and copies likewise -- and wesup_plan_replay re-issues the recording from C.
 * Nothing is re-derived at replay: the caller replays a plan only while every buffer the recorded step touched is alive at
 * the same address and the shapes / hyper-parameters are those of the recording (inputs go into buffers the plan knows). */
typedef struct WesupPlan WesupPlan;
int wesup_plan_create(WesupPlan** out /* host */);
int wesup_plan_destroy(WesupPlan* plan);
int wesup_plan_begin(WesupPlan* plan);            /* this thread records into plan (one at a time per thread) */
int wesup_plan_end(WesupPlan* plan);
int wesup_plan_size(const WesupPlan* plan);       /* nodes so far: a position to split a replay at */
int wesup_plan_kernels(const WesupPlan* plan);    /* kernel launches among them */
int wesup_plan_replay(const WesupPlan* plan, int first, int last);      /* nodes [first, last) in recorded order */
/* 0 = the two recordings are identical (kernels, geometry, streams, argument bytes, edges, copies); k > 0 = they first
 * differ at node k - 1: something the walk produces moved between the two steps and the older plan must not be replayed */
int wesup_plan_diff(const WesupPlan* a, const WesupPlan* b);
const char* wesup_plan_node_name(const WesupPlan* plan, int node);   /* kernel name, "<record s>", "<wait s>", "<copy n>" */
void* wesup_plan_node_stream(const WesupPlan* plan, int node);
/* diagnostics (environment WESUP_PLAN_TIMING=1): host nanoseconds the latest replay spent issuing the node, and when */
int wesup_plan_node_host_ns(const WesupPlan* plan, int node, long long* out2 /* host */);
/* Ordering edges between streams on a fixed pool of events addressed by slot (0 .. wesup_sync_slots() - 1): record marks
 * the work queued so far on `stream`, wait makes `stream` wait for the slot's latest mark.  Both act at once and, while the
 * thread records a plan, become nodes of it.  wesup_sync_synchronize blocks the HOST until the mark is reached (the one
 * wait of an iteration: the loss read-back). */
int wesup_sync_slots(void);
int wesup_sync_record(int slot, void* stream);
int wesup_sync_wait(int slot, void* stream);
int wesup_sync_synchronize(int slot);
int wesup_sync_query(int slot);                   /* 1 reached, 0 not yet */
/* recordable copies and fills: device -> pinned host, device -> device, 32-bit words */
int wesup_copy_to_host(void* dst_host_pinned, const void* src, size_t bytes, void* stream);
int wesup_copy(void* dst, const void* src, size_t bytes, void* stream);
int wesup_fill_words(void* ptr, uint32_t value, size_t words, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WESUP_HIP_H */
