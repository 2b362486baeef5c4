/*
 * tdgp.h -- C ABI of libtdgp_hip.so: the MI355X (gfx950) generator-forward hot path of 3DGP.
 *
 * Conventions:
 *   - plain pointers and sizes only; every data pointer is a DEVICE pointer unless marked "host";
 *   - the library never allocates, frees or synchronises: the caller owns all memory (outputs and
 *     workspaces are caller-allocated) and passes the HIP stream to launch on;
 *   - every function returns 0 on success or a negative TDGP_E* code; tdgp_last_error() returns a
 *     thread-local message.  Nothing throws across the ABI;
 *   - fp32 unless a `dtype` argument says otherwise (TDGP_F32 / TDGP_F16 / TDGP_BF16; TDGP_F64 for the two plugin ops);
 *   - re-entrant.  Process-wide state is limited to: the init-once kernel tables, the two switches tdgp_set_conv_arith (algorithm of
 *     the large 3x3 layers; default 0 = fp32 MFMA) and tdgp_profile_enable (per-kernel event timing; default off), and the launch
 *     geometry cached per kernel instantiation and device (resident blocks per CU, CU count, raised LDS caps), and the device-fault
 *     word (tdgp_device_fault).  Nothing else is remembered between calls.
 *
 * Each entry point cites the reference interface it replaces (file:line under the reference tree).
 * The reference binds its two native ops through pybind (bias_act.cpp:94, upfirdn2d.cpp:102); the
 * modulated convolution and the renderer have no native boundary in the reference (plain PyTorch
 * functions) -- their entry points here take the same operands as those Python functions.
 */
#ifndef TDGP_H
#define TDGP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TDGP_OK            0
#define TDGP_EINVAL       -1   /* bad argument (shape / range / null)         */
#define TDGP_EUNSUPPORTED -2   /* valid request this build has no kernel for  */
#define TDGP_ELAUNCH      -3   /* HIP launch error                            */
#define TDGP_EWORKSPACE   -4   /* workspace too small                         */

#define TDGP_F32  0
#define TDGP_F16  1
#define TDGP_BF16 2
#define TDGP_F64  3   /* tdgp_bias_act / tdgp_bias_act_grad / tdgp_upfirdn2d only (bias_act.cpp:77, upfirdn2d.cpp:63: ..._FLOATING_TYPES_AND_HALF); compute type double */

typedef void* tdgp_stream_t;   /* hipStream_t */

int         tdgp_version(void);
const char* tdgp_last_error(void);

/* Per-kernel timing (the reference wraps its ops in torch.autograd.profiler ranges: src/torch_utils/misc.py:101-106).
 * tdgp_profile_enable(1) makes every launch record a HIP event pair on its stream; tdgp_profile_report() waits for
 * the recorded events (the ONLY entry point that blocks) and writes "<kernel> <launches> <total_ms> <min_ms> <max_ms>"
 * lines into a HOST buffer, returning the bytes needed.  tdgp_profile_enable(0/1) also clears previous records. */
int     tdgp_profile_enable(int on);
int64_t tdgp_profile_report(char* buf, int64_t cap);

/* Device-fault word.  The producer / consumer field kernel bounds its in-kernel waits (a protocol bug or a multi-millisecond stall under
 * a debugger / thread-trace profiler must never hang the GPU); a wait that runs out ORs a code into one int of pinned HOST memory (the
 * single allocation this library makes: 64 bytes, hipHostMalloc, on first use) instead of completing silently with wrong numbers.
 * tdgp_device_fault(0) returns the word, tdgp_device_fault(1) returns and clears it -- meaningful after the stream has been synchronised
 * by the caller.  While it is non-zero tdgp_triplane_field / tdgp_importance_from_coarse / tdgp_merge_composite / tdgp_ray_march return
 * TDGP_ELAUNCH (checked on the host at entry, no synchronisation).  No reference counterpart (its ops cannot time out).
 * codes: 1 = field ring, producer side; 2 = field ring, consumer side. */
int     tdgp_device_fault(int clear);

/* ---------------------------------------------------------------------------------------------
 * bias_act forward:  y = clamp(gain * act(x + b[(i / stepB) % sizeB]))
 * replaces: src/torch_utils/ops/bias_act.cpp:32 `bias_act(x,b,xref,yref,dy,grad=0,dim,act,alpha,gain,clamp)`
 * act = the reference's cuda_idx 1..9 (bias_act.py:21-31); clamp < 0 disables; b may be NULL.
 * n <= INT_MAX (bias_act.cpp:40).  x and y dense with identical layout.
 * --------------------------------------------------------------------------------------------- */
int tdgp_bias_act(const void* x, const void* b, void* y, int64_t n, int sizeB, int64_t stepB,
                  int act, float alpha, float gain, float clamp, int dtype, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * bias_act first / second derivative (the training-side forms of the same plugin call).
 * replaces: src/torch_utils/ops/bias_act.cpp:32 `bias_act(x,b,xref,yref,dy,grad,dim,act,alpha,gain,clamp)` with grad = 1, 2
 *   grad 1:  y = x * dy * gain * act'(xref + b)       x = incoming gradient        (bias_act.py:172-178)
 *   grad 2:  y = x * dy * gain * act''(xref + b)      x = second-order gradient    (bias_act.py:190-197)
 * derivatives are written through yref / gain (xref for swish) exactly as bias_act.cu:60-133; with clamp >= 0 the result is 0
 * where the forward output yref lay outside (-clamp, clamp).  xref / yref / dy / b may be NULL (read as 0 / 0 / 1 / 0).
 * --------------------------------------------------------------------------------------------- */
int tdgp_bias_act_grad(const void* x, const void* b, const void* xref, const void* yref, const void* dy, void* y, int64_t n,
                       int sizeB, int64_t stepB, int grad, int act, float alpha, float gain, float clamp, int dtype,
                       tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * upfirdn2d forward on [N,C,H,W] with arbitrary element strides.
 * replaces: src/torch_utils/ops/upfirdn2d.cpp:16
 *   `upfirdn2d(x,f,upx,upy,downx,downy,padx0,padx1,pady0,pady1,flip,gain)`
 * f: fp32 [fH,fW] contiguous.  outH/outW must equal (in*up + pad0 + pad1 - f + down) / down.
 * x_strides / y_strides: host arrays of 4 element strides (N,C,H,W).
 * --------------------------------------------------------------------------------------------- */
int tdgp_upfirdn2d(const void* x, const float* f, void* y, int N, int C, int inH, int inW,
                   const int64_t* x_strides, int outH, int outW, const int64_t* y_strides,
                   int fH, int fW, int upx, int upy, int downx, int downy,
                   int padx0, int padx1, int pady0, int pady1, int flip, float gain,
                   int dtype, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Modulated convolution (new native boundary; the reference runs cuDNN grouped convs from Python).
 * replaces: src/training/networks_stylegan2.py:31 `modulated_conv2d(x, weight, styles, noise, up,
 *           padding=k//2, resample_filter, demodulate, flip_weight=(up==1), fused_modconv=True)`
 *           + conv2d_resample.py:46 + the bias_act that follows it in SynthesisLayer/ToRGBLayer
 *           (networks_stylegan2.py:139-144,170-171), + for ToRGB the skip-connection
 *           `img = upsample2d(img) + y` (networks_stylegan2.py:265-269).
 *
 * Weights are static across calls, so they are packed once:
 *   tdgp_modconv_pack_bytes  -> bytes of the packed buffer for (Cout,Cin,k)
 *   tdgp_modconv_pack        -> wpack ([Cin/4][k*k][Cout][4 channels], zero padded, + sum_taps w^2 per (c,o))
 * Forward:
 *   y[b,o] = clamp( act( d[b,o] * conv(x[b]*s[b,:], W)[o] + noise + bias[o] ) * gain )  (+ skip term, added after the clamp)
 *   d[b,o] = rsqrt(sum_c s[b,c]^2 * wsq[o,c] + 1e-8) if demodulate else 1
 *   up=2: transposed conv (stride 2) followed by the 4x4 FIR `fir4x4` with gain 4 (pad 1,1,1,1).
 *   fir4x4: HOST pointer to the 16 filter taps (a static 64-byte buffer: upfirdn2d.setup_filter([1,3,3,1])).
 * noise: NULL, or [H,W] (noise_bstride = 0), or [B,1,H,W] (noise_bstride = H*W); already multiplied
 *        by noise_strength by the caller.
 * skip: NULL or the previous-resolution image (same layout as the output: [B,Cout,H/2,W/2] for out_layout 0,
 *       [B,Cout/feat,H/2,W/2,feat] for out_layout 1) to be FIR-upsampled x2 with `fir4x4` (gain 4) and added
 *       (only with up=1, k=1).
 * out_layout: 0 = NCHW, 1 = plane-major channel-last [B, Cout/feat, H, W, feat] (the renderer's layout;
 *       `feat` = out_feat).
 * dcoef: NULL (the call computes d itself when demodulate != 0) or the [B,Cout] coefficients precomputed by
 *       tdgp_demod_batch for this layer.
 * workspace: tdgp_modconv2d_workspace_bytes(...) bytes (0 allowed when it returns 0).
 * k in {1, 3, 5} with padding k/2; up=2 needs k=3.  styles = NULL: plain convolution -- this is how the 5x5
 *       `Conv2dLayer`s of the depth adaptor run (src/training/layers.py:221-236: conv2d_resample + bias_act).
 * --------------------------------------------------------------------------------------------- */
int64_t tdgp_modconv_pack_bytes(int Cout, int Cin, int k);
int     tdgp_modconv_pack(const float* weight, void* wpack, int Cout, int Cin, int k, tdgp_stream_t stream);
/* The workspace size is decided by the shape alone: an upper bound over every kernel family the shape can take, whatever the arithmetic mode
 * (tdgp_set_conv_arith), the alignment of the tensors and the output layout of the call turn out to be. */
int64_t tdgp_modconv2d_workspace_bytes(int B, int Cin, int Cout, int H, int W, int k, int up);
/* 1 when tdgp_modconv2d would take a folded x2 layer (out_layout 2, Cout4 = 4 x Cout parity channels) of this shape on the F(4x4) kernels
 * under the current arithmetic mode, else 0 -- a host-side query (no launch) the binding makes before folding and packing the weights. */
int     tdgp_modconv2d_takes_folded_up2(int B, int Cin, int Cout4, int H, int W);
/* Which kernel family tdgp_modconv2d runs a call as -- the launch plan the call itself reads, so a caller (a benchmark pricing a layer, a
 * test pinning the selection) asks instead of mirroring the conditions.
 * replaces: nothing in the reference (cuDNN picks its algorithm out of sight); answers: the dispatch of tdgp_modconv2d.
 * Same shape arguments as the workspace query + out_layout; `flags` = TDGP_PATHQ_* facts of the call (ALIGNED: x, y and the noise map 16-byte
 * aligned, noise batch stride a multiple of 4 floats; LRELU: the activation of a synthesis layer -- lrelu, alpha 0.2, gain sqrt 2, no clamp --,
 * clear: linear, gain 1).  Returns a tdgp_conv_path under the current arithmetic mode, or a negative TDGP_E* code for a call tdgp_modconv2d
 * would refuse.  Host-side only: no launch, no GPU needed. */
typedef enum tdgp_conv_path {
    TDGP_PATH_DIRECT = 0,        /* conv_mfma_kernel: 3x3 / 5x5, any width */
    TDGP_PATH_CONV3 = 1,         /* conv3_mfma_kernel: 3x3 / 5x5 with W % 32 == 0 */
    TDGP_PATH_SPLIT3 = 2,        /* split-bf16 arithmetic (mode 1), 3x3 */
    TDGP_PATH_WINO2 = 3,         /* Winograd F(2x2,3x3) */
    TDGP_PATH_WINO4 = 4,         /* Winograd F(4x4,3x3): input transform pass + GEMM */
    TDGP_PATH_WINO4F = 5,        /* F(4x4) with the input transform inside the GEMM kernel */
    TDGP_PATH_WINO4_SPLITK = 6,  /* F(4x4), input channels split 2 or 4 ways (too few items for the chip) */
    TDGP_PATH_WINO4_FOLDED = 7,  /* out_layout 2: x2 layer folded into four parity 3x3 kernels on F(4x4) */
    TDGP_PATH_UP = 8,            /* up = 2: transposed convolution + FIR pass */
    TDGP_PATH_TORGB = 9,         /* 1x1, channel-last planes (+ fused skip): torgb_mfma_kernel */
    TDGP_PATH_CONV1 = 10         /* any other 1x1: conv_mfma_kernel */
} tdgp_conv_path;
enum { TDGP_PATHQ_STYLES = 1, TDGP_PATHQ_SKIP = 2, TDGP_PATHQ_NOISE = 4, TDGP_PATHQ_DEMODULATE = 8, TDGP_PATHQ_ALIGNED = 16, TDGP_PATHQ_LRELU = 32 };
int     tdgp_modconv2d_path(int B, int Cin, int Cout, int H, int W, int k, int up, int out_layout, int flags);
int     tdgp_modconv2d(const float* x, const void* wpack, const float* styles, const float* dcoef, const float* noise,
                       int64_t noise_bstride, const float* bias, const float* fir4x4, const float* skip,
                       float* y, int B, int Cin, int Cout, int H, int W, int k, int up, int demodulate,
                       int act, float alpha, float gain, float clamp, int out_layout, int out_feat,
                       void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);

/* The reduced-precision blocks of the backbone -- BASELINE configs[4]; replaces the reference's `use_fp16` path
 * (networks_stylegan2.py:50-53, :237 `dtype = float16 if use_fp16`, :286-304 / networks_epigraf.py:99-108 `num_fp16_res`, conv_clamp 256)
 * with bfloat16 in the place of float16.  Same arguments as tdgp_modconv2d except:
 *   x: bf16 NCHW [B,Cin,H,W];
 *   y: bf16 NCHW [B,Cout,H*up,W*up] for the 3x3 layers; for the ToRGB form (k = 1, up = 1, out_layout = 1, optional skip) the fp32
 *      channel-last planes, as in tdgp_modconv2d (the skip image stays fp32, :268).
 * bf16 weights x bf16 (style-scaled) activations on v_mfma_f32_32x32x16_bf16, fp32 accumulation; demodulation, noise, bias,
 * activation, gain, clamp in fp32; the reference's rounding points behind the accumulator (conv output, + noise, bias_act output; the
 * bias itself is rounded as in `self.bias.to(x.dtype)`), and the skip is added AFTER the clamp.
 * Forms taken: 3x3 with Cin % 32 == 0 and Cin <= 2048 (and W % 32 == 0, H >= 8 for up = 1; W even for up = 2); the channel-last ToRGB
 * with Cout <= 96.  The stride-1 kernel keeps the styles of two samples per block, which covers its 10-row window only for H >= 8:
 * smaller images are refused like every other form without a bf16 kernel.  Anything else returns
 * TDGP_EUNSUPPORTED -- decided before anything is launched: widen x to fp32 and call tdgp_modconv2d.  `noise` must be 16-byte aligned with
 * a batch stride that is a multiple of 4 floats (TDGP_EINVAL otherwise; tdgp_modconv2d takes any float* and falls back to scalar
 * loads).  Workspace: tdgp_modconv2d_workspace_bytes of the same shape.
 * tdgp_cast_f32_bf16: x.to(bf16) (round to nearest even) at the first reduced-precision block (:250). */
int     tdgp_modconv2d_bf16(const void* x_bf16, const void* wpack, const float* styles, const float* dcoef, const float* noise,
                            int64_t noise_bstride, const float* bias, const float* fir4x4, const float* skip,
                            void* y, int B, int Cin, int Cout, int H, int W, int k, int up, int demodulate,
                            int act, float alpha, float gain, float clamp, int out_layout, int out_feat,
                            void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);
int     tdgp_cast_f32_bf16(const float* x, void* y_bf16, int64_t n, tdgp_stream_t stream);

/* Plain x2 transposed convolution (the adjoint of a 3x3 stride-2 convolution, conv2d_gradfix.py:126-129):
 *   y [B,Cout,2H+1,2W+1] = conv_transpose2d(x * styles[:, :, None, None], w.transpose(0,1), stride=2),   w [Cout,Cin,3,3] packed by
 * tdgp_modconv_pack (the weights of the up-sampling synthesis layers; for the input gradient of y' = conv2d(a, W, stride 2) pass
 * x = dy' and w = W.transpose(0,1)).  styles may be NULL.  workspace: tdgp_modconv2d_workspace_bytes(B, Cin, Cout, H, W, 3, 2). */
int     tdgp_conv_transpose2d_x2(const float* x, const void* wpack, const float* styles, float* y, int B, int Cin, int Cout,
                                 int H, int W, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);

/* Arithmetic of the large 3x3 convolutions of tdgp_modconv2d.  All modes are fp32 in, fp32 accumulate, fp32 out:
 *   0 (default) = fp32 MFMA; stride-1 layers with W % 32 == 0, H % 8 == 0, Cin % 8 == 0, Cin >= 64 whose launch has at least one
 *       64-channel x 64-tile block per CU run as Winograd F(2x2,3x3) -- the convolution's exact algebra with 16 instead of 36
 *       multiplies per 2x2 outputs, transforms and products in fp32 (what cuDNN selects for the reference's fp32 3x3 convolutions,
 *       training_loop.py:76-77 keeps TF32 off); measured as close to the exactly rounded result as the direct sum (<= 5e-6 of the
 *       tensor scale).  Every other layer: direct sums;
 *   2 = fp32 MFMA, direct sums in every layer (the summation structure of a plain convolution; results differ from mode 0 in the last
 *       bits only);
 *   4 = as 0, but the F(4x4) layers with few input channels (Cin <= 128, the 256^2 / 512^2 blocks) keep their input transform as a pass
 *       of its own instead of inside the GEMM kernel (round 6, modconv_wino4f.inc): the SAME bits as mode 0 (same transform arithmetic,
 *       same summation order) -- an A/B and test switch;
 *   1 = (stride 1 with W % 32 == 0 and the x2 transposed form, launches of >= 256 tiles with styles present and Cin % 16 == 0) every
 *       fp32 operand split into three bf16 pieces, six piece products per multiply on the bf16 MFMA with fp32 accumulation
 *       (fp32-grade results, <= 4e-6 of the exact layer output; layers outside those conditions keep the fp32 kernels).
 * Process-wide; returns the previous mode (negative on error). */
int     tdgp_set_conv_arith(int mode);

/* Demodulation coefficients d[b,o] = rsqrt(sum_c s[b,c]^2 * sum_tap W[o,c,tap]^2 + 1e-8) (networks_stylegan2.py:62) of SEVERAL
 * layers in one launch.  meta: int64 [num_layers, 6] on the device = (address of the layer's sum_tap W^2 table, i.e. its wpack +
 * tdgp_modconv_wsq_offset(...) bytes; float offset of its [B,Cin] styles block in styles_all; Cin; Cout; Cout rounded up to 4;
 * float offset of its [B,Cout] block in dcoef_all).  max_cout = the largest Cout among them. */
int64_t tdgp_modconv_wsq_offset(int Cout, int Cin, int k);
int     tdgp_demod_batch(const float* styles_all, const int64_t* meta, float* dcoef_all, int B, int num_layers,
                         int max_cout, tdgp_stream_t stream);

/* Batched style affines for all layers of the backbone in one launch:
 *   out[obase + b*olen + oidx] = ((ws[b, widx, :] . A[row, :]) * (1/sqrt(w_dim)) + abias[row]) * row_scale[row]
 * replaces: the per-layer `self.affine(w)` FullyConnectedLayer calls (networks_stylegan2.py:130,169;
 * layers.py:42-58) and ToRGB's `* weight_gain` (:169).
 * A: concatenated affine weights [rows_total, w_dim]; abias [rows_total]; row_scale [rows_total] (1, or 1/sqrt(Cin)
 * for ToRGB); row_meta: int32 [rows_total,4] = (widx, obase, olen, oidx) so that layer l owns the contiguous block
 * styles[obase_l : obase_l + B*Cin_l] viewed as [B, Cin_l]. */
int tdgp_style_affine(const float* ws, const float* A, const float* abias, const int32_t* row_meta,
                      const float* row_scale, float* styles, int B, int num_ws, int w_dim, int rows_total,
                      tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Convolution weight gradient.
 * replaces: src/torch_utils/ops/conv2d_gradfix.py:141-150 `Conv2dGradWeight.forward` (aten::convolution_backward, output_mask
 *           [0,1,0]; non-transposed, groups 1, dilation 1):
 *   dw[o,c,ky,kx] = sum_{b,oy,ox} dy[b,o,oy,ox] * x[b,c, oy*stride + ky - pad, ox*stride + kx - pad]      (zero outside x)
 * x [B,Cin,H,W], dy [B,Cout,OH,OW] with OH = (H + 2 pad - k) / stride + 1 (likewise OW), dw [Cout,Cin,k,k], k <= 7.
 * The pixel sum is split over blocks; the slices are added in slice order (run-to-run deterministic).
 * workspace: tdgp_conv2d_weight_grad_workspace_bytes(B, Cin, Cout, OH, k) bytes.
 * (The input gradient of a stride-1 'same' convolution is tdgp_modconv2d on dy with the flipped, transposed weights.)
 * --------------------------------------------------------------------------------------------- */
int64_t tdgp_conv2d_weight_grad_workspace_bytes(int B, int Cin, int Cout, int OH, int k);
/* Plain strided convolution (correlation; groups 1, dilation 1; k in {1,3}, stride in {1,2}, any padding):
 *   y[b,o,oy,ox] = bias[o] + sum_{c,ky,kx} w[o,c,ky,kx] * x[b,c, oy*stride + ky - pad, ox*stride + kx - pad]
 * replaces: torch.nn.functional.conv2d as reached from conv2d_gradfix.py:34-39 for the forms the fused kernels do not cover -- the
 *           adjoint of the x2 transposed convolution (conv2d_gradfix.py:126-129) and the down-sampling convolutions of
 *           conv2d_resample.py:104-107.  w [Cout,Cin,k,k] as stored by the modules; bias may be NULL. */
int     tdgp_conv2d(const float* x, const float* w, const float* bias, float* y, int B, int Cin, int Cout, int H, int W,
                    int OH, int OW, int k, int stride, int pad, tdgp_stream_t stream);
int     tdgp_conv2d_weight_grad(const float* x, const float* dy, float* dw, void* workspace, int64_t workspace_bytes, int B,
                                int Cin, int Cout, int H, int W, int OH, int OW, int k, int stride, int pad,
                                tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Camera + rays.
 * replaces: src/training/rendering_utils.py:194 `compute_cam2world_matrix(camera_params)`,
 *           src/training/tri_plane_renderer.py:487 `sample_rays(c2w, fov, resolution, patch_params)`
 * fov in degrees; fov_stride 1 = per-sample tensor, 0 = one shared scalar. patch_* may be NULL.
 * Ray r of sample b is pixel (row r / w, col r % w).
 * --------------------------------------------------------------------------------------------- */
int tdgp_cam2world(const float* angles, const float* radius, const float* look_at, float* c2w, int B,
                   tdgp_stream_t stream);
int tdgp_sample_rays(const float* c2w, const float* fov, int fov_stride, const float* patch_scales,
                     const float* patch_offsets, float* ray_o, float* ray_d, int B, int h, int w,
                     tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Renderer pieces.
 * replaces (all src/training/tri_plane_renderer.py unless noted):
 *   :208  ImportanceRenderer.sample_stratified            -> tdgp_sample_stratified
 *   :560  simple_tri_plane_renderer + networks_epigraf.py:46 TriPlaneMLP.forward -> tdgp_triplane_field
 *   :353 / :300  ClassicalRayMarcher / MipRayMarcher2      -> tdgp_ray_march
 *   :237,:257  sample_importance / sample_pdf              -> tdgp_sample_importance
 *   :196  unify_samples                                    -> tdgp_unify_samples
 *   :126  ImportanceRenderer.forward (whole chain)         -> the fused pair
 *                 tdgp_importance_from_coarse + tdgp_merge_composite
 * marcher: 0 = classical, 1 = mip.
 * --------------------------------------------------------------------------------------------- */

/* u [rays,S] uniforms -> sdist [rays,S] (s-space) and, if tdist != NULL, t = s*t_far + (1-s)*t_near. */
int tdgp_sample_stratified(const float* u, float* sdist, float* tdist, int64_t rays, int S, int marcher,
                           float t_near, float t_far, tdgp_stream_t stream);

/* The marchers' density activation as a function of its own: out[i] = max(x, 0) when flags bit 3 (relu clamp) is set, else the softplus
 * of x = sigma[i] + density_bias -- the routine the march kernels apply, so that a threshold taken over `out` (the cut_quantile option,
 * tri_plane_renderer.py:324-326, :366-368: `x < quantile(x)` on the activated densities) compares like with like. */
int tdgp_density_activation(const float* sigma, float* out, int64_t n, int flags, float density_bias, tdgp_stream_t stream);

/* NCHW planes [B,3F,H,W] -> plane-major channel-last [B,3,H,W,F] (the field kernel's layout). */
int tdgp_planes_to_hwc(const float* planes_nchw, float* planes_hwc, int B, int F, int H, int W,
                       tdgp_stream_t stream);

/* The lookup alone (round 6): feats [B,P,F] = mean over the three planes of the bilinear samples (align_corners, zero padding) at coords [B,P,3] / scale
 * -- what simple_tri_plane_renderer hands to TriPlaneMLP (tri_plane_renderer.py:575-586, networks_epigraf.py:55: `x.mean(dim=1)`), in torch's own
 * evaluation order.  For decoders the fused kernel below does not cover (tri_plane.mlp.n_layers != 2, has_view_cond: networks_epigraf.py:35-43), whose
 * layers the binding then runs as eager tensor ops like the reference.  planes_hwc [B,3,H,W,F], F % 4 == 0. */
int tdgp_triplane_features(const float* planes_hwc, const float* coords, float* feats, int B, int64_t P, int F, int H, int W,
                           float scale, tdgp_stream_t stream);

/* Tri-plane bilinear lookup (align_corners, zero padding) + mean + tiny MLP, fused.
 * planes_hwc: [B,3,H,W,F].  Points are given either as coords [B,P,3] (ray_o = NULL), or as rays:
 * ray_o/ray_d [B,R,3] and t [B,R,S] with P = R*S, point p = ray p/S at depth t[p].  In ray mode `ray_w` > 0 declares that
 * the R rays of a sample form a [R/ray_w, ray_w] image (ray r = pixel (r / ray_w, r % ray_w)): the kernel then walks 4x4-pixel
 * tiles for cache locality (results are identical); ray_w = 0 keeps the linear point order.
 * w0 [hid,F], b0 [hid], w1 [4,hid], b1 [4] are the RAW module parameters (gains 1/sqrt(F), 1/sqrt(hid),
 * lrelu 0.2 * sqrt(2) applied inside, layers.py:39-58).
 * out: rgbs [B,P,4] = (r,g,b,sigma); marcher=1 applies sigmoid*1.002-0.001 to rgb (networks_epigraf.py:61-62).
 * tap_idx: optional int32 [B,P,3,2] = (floor ix, floor iy) per plane, for integer-row parity tests.
 * sigma_noise / density_noise: training-time density noise (tri_plane_renderer.py:185-186): sigma += sigma_noise[b,p] * density_noise
 *          with sigma_noise [B,P] standard-normal draws; density_noise = 0 (sigma_noise may be NULL) turns it off.
 * Requires (F, hid) from the table of instantiated kernels (csrc/field.hip, FIELD_CASE):
 *     (32,64) (32,32) (32,128) (32,16)   (16,64) (16,32) (16,16)   (8,64) (8,32) (8,16)   (64,64) (64,128);
 * every other pair returns TDGP_EUNSUPPORTED before anything is launched.  (The gradient below has its own, different range -- F in {8,16,24,32}
 * and any hid in 1..64 -- so of this table it takes the nine pairs with F <= 32 and hid <= 64.) */
int tdgp_triplane_field(const float* planes_hwc, const float* coords, const float* ray_o, const float* ray_d,
                        const float* t, const float* w0, const float* b0, const float* w1, const float* b1,
                        const float* sigma_noise, float density_noise, float* rgbs, int32_t* tap_idx, int B, int64_t P,
                        int S, int ray_w, int F, int H, int W, int hid, float scale, int marcher, tdgp_stream_t stream);

/* Gradient of tdgp_triplane_field in coords mode: autograd through simple_tri_plane_renderer + TriPlaneMLP
 * (tri_plane_renderer.py:560-588 -- grid_sample backward --, networks_epigraf.py:46-68) w.r.t. the planes and the four MLP tensors.
 * d_out [B,P,4] = gradient w.r.t. (r,g,b,sigma) as tdgp_triplane_field returns them.  d_planes_hwc [B,3,H,W,F] is ACCUMULATED
 * into with fp32 atomics (zero it first; NULL skips it; like torch's grid_sampler backward its last bits vary run to run);
 * d_w0 [hid,F], d_b0 [hid], d_w1 [4,hid], d_b1 [4] are written, deterministically.  d_coords [B,P,3] (NULL skips it) receives the
 * gradient w.r.t. the sample positions -- grid_sampler's grid gradient (taps outside a plane read as zero, x (size - 1) / 2 for
 * align_corners) through the plane mean and `coords / scale`: what the camera parameters are trained through (loss.py:69-83 applies the
 * camera adaptor inside run_G; rendering_utils.py:194-218 and tri_plane_renderer.py:487-527 are differentiable in the reference).
 * Requires F in {8,16,24,32}, hid <= 64.
 * workspace: tdgp_triplane_field_grad_workspace_bytes(B, P, F, hid) bytes. */
int64_t tdgp_triplane_field_grad_workspace_bytes(int B, int64_t P, int F, int hid);
int     tdgp_triplane_field_grad(const float* planes_hwc, const float* coords, const float* w0, const float* b0,
                                 const float* w1, const float* b1, const float* d_out, float* d_planes_hwc, float* d_w0,
                                 float* d_b0, float* d_w1, float* d_b1, float* d_coords, void* workspace, int64_t workspace_bytes,
                                 int B, int64_t P, int F, int H, int W, int hid, float scale, int marcher, tdgp_stream_t stream);

/* tdgp_triplane_field for the 3- and 4-layer decoders (tri_plane.mlp.n_layers = 3, 4; networks_epigraf.py:35-43: FC(F -> hid, lrelu),
 * n_layers - 2 x FC(hid -> hid, lrelu), FC(hid -> 4)).  Same contract in every other respect: coords or ray mode, `ray_w` image walk (results
 * are identical), tap_idx rows (equal to tdgp_triplane_field's on the same points), sigma_noise / density_noise, marcher, rgbs [B,P,4].
 * w, b: HOST arrays of n_layers DEVICE pointers to the RAW module parameters: w[0] [hid,F], w[1 .. n_layers-2] [hid,hid], w[n_layers-1] [4,hid],
 * b[i] the matching biases (gains 1/sqrt(fan_in), lrelu 0.2 * sqrt(2) applied inside).
 * Takes n_layers 3 and 4 with F in {8,16,32} x hid in {16,32,64}, or F = hid = 64; everything else -- n_layers 2 (tdgp_triplane_field is the
 * only route of two-layer decoders), hid 128 (two hidden layers' operands do not fit the LDS) -- returns TDGP_EUNSUPPORTED before any launch. */
int tdgp_triplane_field_deep(const float* planes_hwc, const float* coords, const float* ray_o, const float* ray_d,
                             const float* t, const float* const* w, const float* const* b, int n_layers,
                             const float* sigma_noise, float density_noise, float* rgbs, int32_t* tap_idx, int B, int64_t P,
                             int S, int ray_w, int F, int H, int W, int hid, float scale, int marcher, tdgp_stream_t stream);

/* Gradient of tdgp_triplane_field_deep in coords mode, with tdgp_triplane_field_grad's semantics: forward values are recomputed; d_planes_hwc
 * is ACCUMULATED into with fp32 atomics (zero it first; NULL skips it); d_coords [B,P,3] is optional (NULL skips it); d_w[i] / d_b[i] (HOST
 * arrays of n_layers DEVICE pointers, shapes of w[i] / b[i]) are written, reduced wave -> block -> grid in a fixed order: identical bytes run
 * to run.  Requires n_layers 3 or 4, F in {8,16,24,32}, hid <= 64 (else TDGP_EUNSUPPORTED).
 * workspace: tdgp_triplane_field_deep_grad_workspace_bytes(B, P, F, hid, n_layers) bytes (-1 for an n_layers it does not take). */
int64_t tdgp_triplane_field_deep_grad_workspace_bytes(int B, int64_t P, int F, int hid, int n_layers);
int     tdgp_triplane_field_deep_grad(const float* planes_hwc, const float* coords, const float* const* w, const float* const* b,
                                      int n_layers, const float* d_out, float* d_planes_hwc, float* const* d_w, float* const* d_b,
                                      float* d_coords, void* workspace, int64_t workspace_bytes, int B, int64_t P, int F, int H, int W,
                                      int hid, float scale, int marcher, tdgp_stream_t stream);

/* Generic marcher on [rays,S,C] colours, [rays,S] densities/depths (2 <= S <= 1024: a merged list of up to 512 + 512 samples; C <= 8).
 * Lists longer than 256 round alpha's exp from fp64; S > 1024 -> TDGP_EUNSUPPORTED.
 * weights: [rays,S] (classical, or mip with inf depth) / [rays,S-1] (mip without); may be NULL.
 * flags: bit0 use_inf_depth, bit1 last_back (classical), bit2 white_back (mip), bit3 clamp_mode relu.
 * cut_threshold: the `cut_quantile` option (tri_plane_renderer.py:324-326, 366-368): activated densities below it are set to 0
 * before alpha; the caller computes it (the reference takes torch.quantile over the whole activated-density tensor); 0 = off. */
int tdgp_ray_march(const float* colors, const float* densities, const float* depths, float* rgb,
                   float* depth, float* weights, float* final_T, int64_t rays, int S, int C, int marcher,
                   int flags, float density_bias, float cut_threshold, tdgp_stream_t stream);

/* Gradient of tdgp_ray_march: autograd through ClassicalRayMarcher / MipRayMarcher2 (:353-398, :299-349).
 * d_rgb [rays,C], d_depth [rays] (may be NULL), d_weights [rays,M] (may be NULL; M as in tdgp_ray_march) ->
 * d_colors [rays,S,C], d_densities [rays,S] (gradient w.r.t. the RAW densities, through softplus / relu).  Depths carry no
 * gradient.  C in {1,3,4}, S <= 256 (the gradient path's limit: S + N <= 256 merged samples); marcher / flags / density_bias as in
 * tdgp_ray_march. */
int tdgp_ray_march_grad(const float* colors, const float* densities, const float* depths, const float* d_rgb,
                        const float* d_depth, const float* d_weights, float* d_colors, float* d_densities,
                        int64_t rays, int S, int C, int marcher, int flags, float density_bias, tdgp_stream_t stream);

/* sample_importance: z [rays,S] (s-space), weights [rays,Wn], u [rays,N] -> samples [rays,N].
 * Optional outputs: inds/below/above int32 [rays,N] (searchsorted right=True, clamped), cdf [rays,Wn-1].
 * 4 <= S <= 512, 3 <= Wn <= S, N >= 1: the pdf row (Wn - 2 <= 510 entries) is normalised in torch's CPU summation order, which
 * is restated up to 575 entries; S > 512 -> TDGP_EUNSUPPORTED. */
int tdgp_sample_importance(const float* z, const float* weights, const float* u, float* samples,
                           int32_t* inds, int32_t* below, int32_t* above, float* cdf,
                           int64_t rays, int S, int Wn, int N, int marcher, tdgp_stream_t stream);

/* unify_samples: concat + stable sort by depth + gather; perm (int32 [rays,S1+S2]) optional.  S1, S2 >= 1, S1 + S2 <= 1024.
 * On ties the order is the stable one (the reference's torch.sort(stable=False) orders equal depths its own way beyond 16 elements). */
int tdgp_unify_samples(const float* d1, const float* c1, const float* s1, int S1,
                       const float* d2, const float* c2, const float* s2, int S2,
                       float* d, float* c, float* s, int32_t* perm, int64_t rays, int C,
                       tdgp_stream_t stream);

/* Fused chain, step 1: coarse march (s-space depths) -> importance sampling -> fine depths in t-space.
 * rgbs_coarse [rays,S,4], sdist [rays,S], u_fine [rays,N] -> tdist_fine [rays,N] WRITTEN IN ASCENDING DEPTH ORDER (stable):
 * the reference keeps draw order and sorts coarse+fine together afterwards, so the final composite is unchanged, but the
 * second field pass becomes spatially coherent and the merge below is a merge of two sorted lists.
 * Optional: sdist_fine [rays,N] and inds int32 [rays,N] in DRAW order; fine_perm int32 [rays,N]: draw index of sorted slot.
 * cut_threshold as in tdgp_ray_march (here and in tdgp_merge_composite).  4 <= S <= 512, 1 <= N <= 512 (as tdgp_sample_importance);
 * beyond -> TDGP_EUNSUPPORTED. */
int tdgp_importance_from_coarse(const float* rgbs_coarse, const float* sdist, const float* u_fine,
                                float* tdist_fine, float* sdist_fine, int32_t* inds, int32_t* fine_perm,
                                int64_t rays, int S, int N, int marcher, int flags, float density_bias,
                                float cut_threshold, float t_near, float t_far, tdgp_stream_t stream);

/* Fused chain, step 2: merge coarse+fine by depth (stable, coarse before fine on ties), march in t-space.
 * rgbs_* [rays,S*,4], t_* [rays,S*] (any order; ascending lists take a fast path) -> rgb [rays,3], depth [rays],
 * wsum [rays], final_T [rays]; perm optional int32 [rays,S1+S2] = index into the concatenation [coarse ; fine in draw
 * order] (fine_perm, optional, maps the fine list's slots back to draw order; NULL = identity).  S1, S2 >= 1, S1 + S2 <= 1024. */
int tdgp_merge_composite(const float* rgbs_coarse, const float* t_coarse, int S1,
                         const float* rgbs_fine, const float* t_fine, int S2,
                         float* rgb, float* depth, float* wsum, float* final_T, int32_t* perm,
                         const int32_t* fine_perm, int64_t rays, int marcher, int flags, float density_bias,
                         float cut_threshold, tdgp_stream_t stream);

/* ImportanceRenderer.forward (tri_plane_renderer.py:126-170) as ONE call: stratified samples -> field -> coarse march -> importance samples ->
 * field -> merge + march.  planes_hwc [B,3,H,W,F]; w0 [hid,F], b0 [hid], w1 [4,hid], b1 [4] raw module parameters; ray_o / ray_d [B,R,3];
 * u_coarse [B*R,S], u_fine [B*R,N] the two uniform draws (tri_plane_renderer.py:225,279) -> rgb [B*R,3], depth [B*R], wsum [B*R] (may be NULL),
 * final_T [B*R] (may be NULL).  ray_w > 0: the R rays are a [R/ray_w, ray_w] image (4x4-pixel tiles, same results); scale = box_size / 2;
 * flags as in tdgp_ray_march; no cut_quantile / density noise / intermediates (those go through the staged entry points above).
 * Same kernels, same bits as tdgp_sample_stratified + tdgp_triplane_field + tdgp_importance_from_coarse + tdgp_triplane_field +
 * tdgp_merge_composite.  workspace: tdgp_render_fused_workspace_bytes(B, R, S, N) bytes, 16-byte aligned, caller-owned.
 * Limits: 4 <= S <= 512, 1 <= N <= 512 (tdgp_importance_from_coarse), and B * R * max(S, N) <= INT32_MAX / 4 points per field pass
 * (tdgp_triplane_field): the caller splits larger renders by images or runs of image rows. */
int64_t tdgp_render_fused_workspace_bytes(int B, int64_t R, int S, int N);
int     tdgp_render_fused(const float* planes_hwc, const float* w0, const float* b0, const float* w1, const float* b1,
                          const float* ray_o, const float* ray_d, const float* u_coarse, const float* u_fine,
                          float* rgb, float* depth, float* wsum, float* final_T,
                          int B, int64_t R, int ray_w, int S, int N, int F, int H, int W, int hid, float scale,
                          float t_near, float t_far, int marcher, int flags, float density_bias,
                          void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);

/* [B, h*w, 3] ray colours -> [B,3,h,w] image (networks_epigraf.py:242). */
int tdgp_rays_to_image(const float* rgb, float* img, int B, int hw, tdgp_stream_t stream);

/* Ray-major fp32 frames -> uint8 image grids, the [T,H,W,3] block a video / image encoder takes (inference_utils.py:113-117 `generate`'s value
 * chain, scripts/inference.py:66,74-75 make_grid + `(x * 255).to(uint8)` + permute, which the reference runs on the host).
 * frames [num_frames, h*w, C] fp32 (the renderer's rgb, C = 3, or depth, C = 1: replicated to three channels) -> out [images, GH, GW, 3] uint8.
 * Tile k of output image i shows frame i * stride_image + k * stride_tile; an index >= num_frames is TDGP_EINVAL.
 * Layout = torchvision make_grid(nrow, padding, pad_value = 0): xmaps = min(nrow, tiles), ymaps = ceil(tiles / xmaps),
 *   GH = (h + padding) * ymaps + padding, GW = (w + padding) * xmaps + padding, tile k at row (k / xmaps) * (h + padding) + padding and column
 *   (k % xmaps) * (w + padding) + padding; every byte outside a tile (the cells of a ragged last row too) is 0; tiles == 1: the tile itself,
 *   unpadded (GH = h, GW = w).
 * Values, each operation rounded once in fp32 as torch's CPU kernels evaluate them: y = x, or with `normalise` y = ((x - mid) / range) * 2 (IEEE
 *   division); y = min(max(y, -1), 1); z = y * 0.5 + 0.5; byte = trunc(z * 255); NaN -> 0.
 * One writer per output byte, no atomics, no workspace: the same bytes on every run.  frames and out 4-byte aligned; one output image < 2^31 bytes. */
int tdgp_frames_to_grid_u8(const float* frames, int64_t num_frames, int h, int w, int C, uint8_t* out, int images, int tiles,
                           int64_t stride_image, int64_t stride_tile, int nrow, int padding, int normalise, float mid, float range,
                           tdgp_stream_t stream);

/* The image tail of the perceptual path length in one launch (src/metrics/perceptual_path_length.py:71-85: centre crop, box mean down to
 * 256^2, `(img + 1) * (255 / 2)`, grey replicated; with the reshape of networks_epigraf.py:242 in front of it).
 * frames [num_frames, h*w, C] fp32 ray-major (the renderer's rgb; C = 1 or 3) -> out [num_frames, 3, oh, ow] fp32 in [0, 255].
 * Window: the whole frame, or with `crop` rows [3c, 7c) and columns [2c, 6c) for c = h / 8 (needs h == w and c >= 1, else TDGP_EINVAL).
 * Both window sides must divide by `factor` >= 1; oh, ow = the window sides / factor.
 * Values: factor == 1: y = (x + 1.0f) * 127.5f, two fp32 roundings, no FMA contraction -- the bits of torch's CPU chain.
 *   factor > 1: the factor x factor box is summed in fp64 in row-major order, divided by factor^2 in fp64 and rounded once to fp32 (the
 *   correctly rounded mean; torch's fp32 `mean` is within factor^2 * 2^-24 * max|x| of it); then the same two operations.
 * C == 1 is written to all three channels.  One writer per element, no atomics, no workspace: the same bytes on every run.  Arguments are
 * checked before any launch; num_frames == 0 is a no-op.  frames and out 4-byte aligned; h * w < 2^31. */
int tdgp_ppl_frames(const float* frames, int64_t num_frames, int h, int w, int C, int crop, int factor, float* out, tdgp_stream_t stream);

/* The differential distance of the perceptual path length (perceptual_path_length.py:88-89: `(l0 - l1).square().sum(1) / epsilon ** 2` on
 * the two halves of the detector's output, in torch two full-width temporaries and an fp32 sum next to cancellation).
 * feats [2n, W] fp32 contiguous, row i paired with row n + i (the layout `chunk(2)` splits) -> out[i], i < n.
 * Arithmetic: d = a - b in fp32 (one rounding); d * d and every addition in fp64; out[i] = (float)(sum * inv_scale), rounded once;
 *   inv_scale = 1 / (epsilon * epsilon), computed by the caller in double.  NaN and Inf propagate (into their own row only).
 * The summation tree is fixed by W alone: a row is cut into segments of 16384 elements, one block each; inside a segment an element's
 *   place in the sum follows from its index, never from its address (rows are only 4-byte aligned when W % 4 != 0: a quad is read by one
 *   16-byte load where its address allows and by four 4-byte loads otherwise, and enters the same sum either way); the segment partials of a
 *   row are added in index order by a finishing pass.  Neither the number of segments nor their bounds depend on n, so a row's bits do not
 *   depend on the call it is computed in.  No atomics, one writer per partial and output: the same bytes on every run.
 * `out` may point anywhere (4-byte aligned) into a larger buffer; only out[0 .. n) is written.  n == 0 is a no-op.
 * Limits: 1 <= W < 2^31 and 0 <= n <= 65535; W < 1 or n < 0: TDGP_EINVAL, above the upper ends: TDGP_EUNSUPPORTED.
 * workspace: tdgp_pair_sqdist_workspace_bytes(n, W) bytes (0 when a row is one segment; -1 for a shape it refuses), 8-byte aligned,
 * caller-owned; too small: TDGP_EWORKSPACE.  A streaming reduction: its point is the defined fp64 arithmetic, reproducible bytes and the
 * absent temporaries, not speed -- the generator and the caller's detector are the expensive part of the metric. */
int64_t tdgp_pair_sqdist_workspace_bytes(int64_t n, int64_t W);
int     tdgp_pair_sqdist(const float* feats, int64_t n, int64_t W, double inv_scale, float* out, void* workspace, int64_t workspace_bytes,
                         tdgp_stream_t stream);

/* create_voxel_coords (scripts/extract_geometry.py:55-76; torch CPU ops over the whole grid there): the coordinates of grid indices
 * [i0, i0 + n) of a res^3 grid -> coords [n,3], bit for bit the reference's fp32 chain: the index converted to fp32 (inexact above 2^24),
 * y = (idx / res) % res and x = ((idx / res) / res) % res as UNFLOORED fp32 divisions, z from the integer remainder, then
 * `* voxel_size + origin` in two roundings.  voxel_size = cube_size / (res - 1) and origin_{x,y,z} = voxel_origin[{2,1,0}] - cube_size / 2
 * are computed by the caller in double and rounded once.  2 <= res <= 2048. */
int tdgp_voxel_coords(float* coords, int64_t i0, int64_t n, int res, float voxel_size, float origin_x, float origin_y, float origin_z,
                      tdgp_stream_t stream);

/* Marching cubes on a contiguous fp32 volume [D,H,W] (mcubes.marching_cubes on a host copy of the grid, scripts/extract_geometry.py:38-40).
 * tdgp_mcubes_count classifies every cell (corner inside <=> value >= thresh), counts triangles and owned sign-changing edges, scans
 * the per-block sums in a launch of its own and leaves the totals as two int64 (V, T) at the START of the workspace -- the one pair of
 * numbers the caller reads back, to size the outputs.  tdgp_mcubes_emit (same volume, threshold and workspace) then writes
 * vertices [V,3] fp32 in index units, axis order (d, h, w), each at p0 + (thresh - v0) / (v1 - v0) along its edge, and
 * triangles [T,3] int32 into them: one shared vertex per sign-changing edge, normals toward lower values.
 * Order: vertices by owning grid point (the edge's lower end) then axis, triangles by cell then table order (csrc/mc_table.inc,
 * written by tools/gen_mc_table.py); no atomics, identical bytes from run to run; no kernel waits on another block.
 * workspace: tdgp_mcubes_workspace_bytes(D, H, W) bytes (about 6 per grid point; -1 for a shape it refuses), 16-byte aligned, caller-owned.
 * Every side >= 2, D * H * W <= INT32_MAX; V >= 2^29 or T > INT32_MAX -> TDGP_EUNSUPPORTED.  Writes never pass the V / T given. */
int64_t tdgp_mcubes_workspace_bytes(int D, int H, int W);
int     tdgp_mcubes_count(const float* volume, int D, int H, int W, float thresh, void* workspace, int64_t workspace_bytes,
                          tdgp_stream_t stream);
int     tdgp_mcubes_emit(const float* volume, int D, int H, int W, float thresh, void* workspace, int64_t workspace_bytes,
                         float* vertices, int64_t V, int32_t* triangles, int64_t T, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Shape frames (csrc/iso_surface.hip; nothing in the reference: its scripts/extract_geometry.py stops at a mesh file): the per-ray tail that
 * turns densities along rays into a surface -- the first crossing of a density level, its refinement, a normal, a shade -- between passes of
 * the field kernels:  field (ray mode, S) -> tdgp_iso_bracket -> field (ray mode, N) -> tdgp_iso_locate -> field (coords mode, 7 points
 * per ray) -> tdgp_iso_shade.
 * Arithmetic contract of all three: every fp32 operation is rounded once, in the order written below (no contraction into FMA); `/` and
 * sqrtf are correctly rounded; comparisons are ordered (a NaN compares false); one writer per output element, no atomics, no workspace: the
 * same bytes on every run.  Arguments are checked before any launch; rays == 0 is a no-op.  Limits: 2 <= S <= 512, 1 <= N <= 64 (outside:
 * TDGP_EINVAL below the lower ends, TDGP_EUNSUPPORTED above the upper ones), rays <= 2^30.
 * A `sigma` input is a pointer plus an element stride: value i is sigma[i * stride].  Stride 4 on a pointer to column 3 of rows [., 4] (the
 * field kernels' rgbs) reads them in place, one dword per sample (the cache lines of the whole rows are fetched; nothing is gathered into a
 * copy).
 *
 * tdgp_iso_bracket: sigma [rays,S] (strided), t [rays,S] ascending -> idx int32 [rays], t_fine [rays,N].
 *   idx = min{k : sigma[k] >= level}, or S if there is none.
 *   1 <= idx <= S-1, lo = t[idx-1], hi = t[idx]:  t_fine[j] = lo + (hi - lo) * (float(j+1) / float(N)) for j < N-1, t_fine[N-1] = hi exactly
 *   (the known crossing is always the last fine sample).  idx == 0: every t_fine[j] = t[0].  idx == S: every t_fine[j] = t[S-1] (valid
 *   depths, ignored later).
 *
 * tdgp_iso_locate: the coarse sigma / t, idx, the fine sigma_fine [rays,N] (strided) / t_fine, ray_o / ray_d [rays,3] -> t_hit [rays],
 *   status int32 [rays], points [rays,7,3].
 *   idx == S: status 0 (miss), t_hit = t_miss.  idx == 0: status 2 (the level is met at the near plane), t_hit = t[0].  Otherwise status 1:
 *   j = first fine sample with sigma_fine >= level, else N-1; the high side is fine sample j, the low side fine sample j-1, or the coarse
 *   sample idx-1 when j == 0;  a = (level - s_lo) / (s_hi - s_lo);  if not (a >= 0 && a <= 1) then a = 1;  t_hit = t_lo + (t_hi - t_lo) * a.
 *   For every ray, misses included: x_c = o_c + d_c * t_hit; points[0] = x, points[1+2i] = x + h e_i, points[2+2i] = x - h e_i (only
 *   component i is changed), so that the next field pass is dense.  (An idx outside [0, S] is clamped into it.)
 *
 * tdgp_iso_shade: stencil [rays,7,4] (the field's rgbs at `points`), status, ray_d -> rgb [rays,3], normal [rays,3] (may
 *   be NULL).  light / albedo / background: HOST pointers to 3 floats; light == NULL is a headlight.
 *   g_i = sigma(+i) - sigma(-i);  q = (gx*gx + gy*gy) + gz*gz;  if q > 0 and q < inf: n_i = (-g_i) / sqrtf(q), else
 *   n_i = (-d_i) / sqrtf((dx*dx + dy*dy) + dz*dz);  l = light, or that same normalised -d;  c = (nx*lx + ny*ly) + nz*lz;  if not (c > 0)
 *   then c = 0;  v = ambient + (1 - ambient) * c.
 *   mode 0 (shaded): out_c = (albedo_c * v) * 2 - 1.  mode 1 (normals): out = n.  mode 2 (colour): k_c = stencil[0].rgb_c * 0.5 + 0.5;
 *   if not (k_c > 0) then k_c = 0; if k_c > 1 then k_c = 1;  out_c = (k_c * v) * 2 - 1.
 *   status 0: out = background, normal = 0.  Any other status is shaded as a hit.
 * --------------------------------------------------------------------------------------------- */
int tdgp_iso_bracket(const float* sigma, int64_t sigma_stride, const float* t, int64_t rays, int S, int N, float level, int32_t* idx,
                     float* t_fine, tdgp_stream_t stream);
int tdgp_iso_locate(const float* sigma, int64_t sigma_stride, const float* t, const int32_t* idx, const float* sigma_fine,
                    int64_t sigma_fine_stride, const float* t_fine, const float* ray_o, const float* ray_d, int64_t rays, int S, int N,
                    float level, float h, float t_miss, float* t_hit, int32_t* status, float* points, tdgp_stream_t stream);
int tdgp_iso_shade(const float* stencil, const int32_t* status, const float* ray_d, int64_t rays, int mode, const float* light, float ambient,
                   const float* albedo, const float* background, float* rgb, float* normal, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh frames (csrc/mesh_raster.hip; nothing in the reference): the indexed mesh tdgp_mcubes_emit leaves on the device, in world units
 * (geometry.grid_to_world), seen from the cameras of tdgp_sample_rays -- a visibility-buffer rasteriser for triangles smaller than a pixel:
 *   tdgp_mesh_visibility -> tdgp_mesh_resolve -> tdgp_mesh_shade        (or, for normals from the field: -> field (coords mode, the 7
 *   points per ray tdgp_mesh_resolve wrote) -> tdgp_iso_shade).
 * Arithmetic contract of all three: every floating-point operation is rounded once, in the order written below (no contraction into FMA);
 * `(double)` of a float is exact, `(double)` of an int64 and `(float)` of a double round to nearest even (the former is exact below 2^53);
 * `/` and sqrt are correctly rounded in either width; comparisons are ordered (a NaN compares false).  Coverage is decided in exact int64
 * arithmetic.  Arguments are checked before any launch; empty inputs are no-ops (C == 0 or rays == 0: nothing is written; T == 0: vis is
 * only cleared); a vertex index outside [0, V) skips its triangle and is never dereferenced.
 * The atomic: tdgp_mesh_visibility merges candidates with ONE unsigned 64-bit atomic minimum per covered pixel (global_atomic_umin_x2 on
 * gfx950, a single native instruction, no compare-and-swap loop).  It is the library's first atomic whose result is not a floating-point
 * sum: a minimum of integers does not depend on the order of its operands, so vis is the same bytes on every run and under every
 * permutation of the triangles or of the launch order; ties in t go to the lower triangle index.
 *
 * tdgp_mesh_visibility: vertices [V,3] fp32 (world), triangles [T,3] int32, c2w [C,4,4] (m below, row-major, as tdgp_cam2world writes it:
 *   columns right / up / -forward / position), focal [C] fp32 = 1 / tan(fov / 2) (computed by the caller in float64 and rounded once),
 *   ray_d [C,h*w,3] of tdgp_sample_rays -> vis uint64 [C,h*w].  2 <= h, w <= 16384, C*h*w <= 2^30, C*T <= 2^38, near > 0, cull 0 (none),
 *   1 (back faces dropped), 2 (front faces dropped).  vis is first set to all ones (empty).  Then per (camera, triangle k), in double:
 *     per vertex i:  p_j = (double)v_j - (double)m[j][3];   xc = (p0*m[0][0] + p1*m[1][0]) + p2*m[2][0];   yc likewise with column 1;
 *       zc = (p0*f0 + p1*f1) + p2*f2 with f_j = -m[j][2] (the depth along the camera axis).  not (zc >= near): the triangle is dropped whole
 *       (there is no clipper).   fx = ((((xc*focal)/zc) + 1) * ((w-1)*0.5)) * 256;   fy = ((1 - ((yc*focal)/zc)) * ((h-1)*0.5)) * 256;
 *       not (|fx| < 2^30 and |fy| < 2^30): dropped.   X_i = rint(fx), Y_i = rint(fy) (round half to even), iz_i = 1 / zc.
 *       Pixel (row, col) has its centre at (X, Y) = (256 col, 256 row): the ray through x = -1 + 2 col/(w-1), y = 1 - 2 row/(h-1), z = -focal.
 *     area2 = (X1-X0)*(Y2-Y0) - (Y1-Y0)*(X2-X0) in int64.  area2 == 0: skipped.  The screen's y points down, so a triangle whose stored winding
 *       is counter-clockwise as the camera sees it (its normal faces the camera; marching cubes: toward lower density) has area2 < 0 and is a
 *       front face: cull 1 drops area2 > 0, cull 2 drops area2 < 0.  s = sign(area2).
 *     For every pixel of the bounding box [ceil(min X / 256), floor(max X / 256)] x [likewise in Y] clamped to the frame, with P its centre:
 *       edge i runs from vertex a = i+1 to b = i+2 (mod 3):  dx = s*(X_b - X_a), dy = s*(Y_b - Y_a),  e_i = dx*(P_y - Y_a) - dy*(P_x - X_a);
 *       the pixel is covered iff for all three edges e_i > 0, or e_i == 0 and the edge is a top or a left one (dy < 0, or dy == 0 and dx > 0):
 *       a pixel centre on an edge shared by two triangles belongs to exactly one of them.  e_0 + e_1 + e_2 == |area2|.
 *       depth = (double)|area2| / (((double)e_0*iz_0 + (double)e_1*iz_1) + (double)e_2*iz_2)     (perspective-correct: 1/z is linear on the screen)
 *       t = (float)(depth / (((double)d0*f0 + (double)d1*f1) + (double)d2*f2)) for that pixel's own ray_d, so that o + t d is the hit whatever the
 *       length of d.   not (t > 0 and t < inf): skipped.   key = ((uint64)bits(t) << 32) | (uint32)k;   vis[pixel] = min(vis[pixel], key).
 *   Work shape: one lane per (camera, triangle); a lane whose clamped bounding box is wider or taller than 8 pixels hands its triangle to its
 *   wave (64 lanes stride the box), so a frame-filling triangle costs h*w/64 steps of one wave.
 *
 * tdgp_mesh_resolve: vis [rays], the mesh, ray_o / ray_d [rays,3], vertex_rgb [V,3] or NULL -> t_hit [rays], status int32 [rays], tri int32
 *   [rays], normal [rays,3], colour [rays,3] (NULL exactly when vertex_rgb is), points [rays,7,3].  One writer per element, no atomics.
 *   vis all ones, or naming a triangle outside [0, T) or with a vertex outside [0, V): a miss -- status 0, t_hit = t_miss, tri = -1, normal =
 *   colour = 0.  Otherwise status 1, tri = low word, t_hit = the float in the high word, and with a = v1 - v0, b = v2 - v0 in double:
 *   g = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0);  q = (g0*g0 + g1*g1) + g2*g2;  if q > 0 and q < inf: n_c = (float)(g_c / sqrt(q)), else
 *   (fp32) n_c = (-d_c) / sqrtf((d0*d0 + d1*d1) + d2*d2), tdgp_iso_shade's own fallback.
 *   For every ray, misses included (fp32): x_c = o_c + d_c * t_hit and the seven points of tdgp_iso_locate around it with h = step.
 *   colour (double): e = x - v0;  d11 = (a.a), d12 = (a.b), d22 = (b.b), e1 = (e.a), e2 = (e.b), each (u0*w0 + u1*w1) + u2*w2;
 *   den = d11*d22 - d12*d12;  b1 = (d22*e1 - d12*e2) / den;  b2 = (d11*e2 - d12*e1) / den;  if not (b1 >= 0) then b1 = 0, the same for b2;
 *   sum = b1 + b2;  if sum > 1: b1 = b1 / sum, b2 = b2 / sum;  b0 = (1 - b1) - b2;  colour_c = (float)((b0*c0 + b1*c1) + b2*c2) with c_i vertex i's.
 *
 * tdgp_mesh_shade: normal, status, ray_d, colour (may be NULL unless mode is 2) -> rgb [rays,3].  tdgp_iso_shade's arithmetic from n on, in
 *   fp32: l = light, or (-d_c) / sqrtf((d0*d0 + d1*d1) + d2*d2);  c = (n0*l0 + n1*l1) + n2*l2;  if not (c > 0) then c = 0;
 *   v = ambient + (1 - ambient) * c.  mode 0: out_c = (albedo_c * v) * 2 - 1.  mode 1: out = n.  mode 2: k_c = colour_c (already in [0, 1]: the
 *   * 0.5 + 0.5 of tdgp_iso_shade is applied once per vertex, mesh.vertex_colours); if not (k_c > 0) then k_c = 0; if k_c > 1 then k_c = 1;
 *   out_c = (k_c * v) * 2 - 1.  status 0: out = background.  light / albedo / background: HOST pointers to 3 floats.
 * --------------------------------------------------------------------------------------------- */
int tdgp_mesh_visibility(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const float* c2w, const float* focal,
                         const float* ray_d, int C, int h, int w, float near_, int cull, uint64_t* vis, tdgp_stream_t stream);
int tdgp_mesh_resolve(const uint64_t* vis, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const float* ray_o,
                      const float* ray_d, int64_t rays, float step, float t_miss, const float* vertex_rgb, float* t_hit, int32_t* status,
                      int32_t* tri, float* normal, float* colour, float* points, tdgp_stream_t stream);
int tdgp_mesh_shade(const float* normal, const int32_t* status, const float* ray_d, const float* colour, int64_t rays, int mode,
                    const float* light, float ambient, const float* albedo, const float* background, float* rgb, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Multisampled mesh frames (csrc/mesh_raster.hip, csrc/mesh_hit.h): S = 4 or 16 coverage samples per pixel in one pass, with the fraction of
 * a pixel the mesh covers.    tdgp_mesh_visibility_ms -> tdgp_mesh_resolve_ms        (two launches and 8 bytes per sample between them)
 * The rules of the mesh frames above hold unchanged: the arithmetic contract, the checks, the empty inputs, the one order-free atomic.
 * THE PATTERNS, offsets (ox, oy) from the pixel centre in 1/256 pixel, x to the right and y down, in sample order:
 *   S = 4  (a rotated grid):  (-32,-96), (96,-32), (-96,32), (32,96).
 *   S = 16 (the 4 x 4 grid):  ox = -96 + 64*(j % 4),  oy = -96 + 64*(j / 4).
 *   Sample j of pixel (row, col) sits at the integer position (sx, sy) = (256 col + ox_j, 256 row + oy_j).  Any other S is TDGP_EINVAL.
 * THE RAY OF A SAMPLE (double), the projection of tdgp_mesh_visibility inverted -- no ray table is read:
 *   u = (((double)sx / (256 * ((w-1)*0.5))) - 1) / focal;   v = (1 - ((double)sy / (256 * ((h-1)*0.5)))) / focal;   len = sqrt((u*u + v*v) + 1).
 *   Its origin is the camera's position o_c = m[c][3]; its direction d_c = (float)(((u*m[c][0] + v*m[c][1]) + (double)(-m[c][2])) / len).
 *
 * tdgp_mesh_visibility_ms: the mesh, c2w [C,4,4], focal [C] -> vis uint64 [C,h*w,S], first set to all ones.  C*h*w*S <= 2^30, C*T <= 2^38.
 *   Per (camera, triangle): the vertices, the culls, the near test, area2 and s EXACTLY as tdgp_mesh_visibility, once for all S samples.
 *   For every sample position P = (sx, sy) of the frame inside the triangle's box (min X <= sx <= max X, min Y <= sy <= max Y): e_i at P, the
 *   cover test with the top-left rule and depth as tdgp_mesh_visibility writes them;   t = (float)(depth * len);   not (t > 0 and t < inf):
 *   skipped;   key = ((uint64)bits(t) << 32) | (uint32)k;   vis[pixel][j] = min(vis[pixel][j], key).
 *   Work shape: one lane per (camera, triangle).  The positions of the 16-pattern form one regular lattice of pitch 64 (four per pixel each
 *   way), those of the 4-pattern one per pixel on each of its four rows: a lane walks the lattice box of its triangle -- the work of
 *   tdgp_mesh_visibility at 4x (2x) the resolution, not S tests per touched pixel -- and a box wider or taller than 8 candidates is handed
 *   to the wave, as in tdgp_mesh_visibility.
 *
 * tdgp_mesh_resolve_ms: vis [C,h*w,S], the mesh, c2w, focal, vertex_normal [V,3] or NULL (face normals), vertex_rgb [V,3] or NULL, image
 *   uint8 [H,W,3] or NULL with (n, r, W, H) its atlas and filter as tdgp_mesh_sample_texture takes them (at most one of vertex_rgb and image;
 *   mode 2 needs one), mode / light / ambient / albedo / background as tdgp_mesh_shade (HOST pointers) -> rgb [C*h*w,3], coverage [C*h*w],
 *   status int32 [C*h*w], depth [C*h*w], tri int32 [C*h*w], normal [C*h*w,3].  One lane per sample, no per-sample buffer.  Per sample j:
 *   a miss (tdgp_mesh_resolve's rule on the key): colour_j = background.  A hit: t = the float in the high word, x_c = o_c + d_c * t (fp32);
 *   n = tdgp_mesh_resolve's face normal (its fallback reads this d);  with vertex_normal: b0, b1, b2 of tdgp_mesh_resolve at x and
 *   tdgp_mesh_interp_normals' normal, the face normal staying where that one leaves it;  mode 2: tdgp_mesh_resolve's colour from vertex_rgb,
 *   or tdgp_mesh_sample_texture's from the image, at the same weights;  colour_j = tdgp_mesh_shade's out for (n, d, colour).
 *   Each of those is ONE __device__ function (csrc/mesh_hit.h, mesh_bary.h, shade.h) compiled into the one-sample kernels and into this one.
 *   Per pixel:  rgb_c = (float)(((..((0.0 + (double)colour_0c) + (double)colour_1c) ..) + (double)colour_(S-1)c) / (double)S);
 *   coverage = (float)hits / (float)S (exact: S is a power of two);  status = hits > 0;  depth, tri, normal = t, k, n of the hit sample with
 *   the smallest t (fp32 `<`, a tie goes to the lower sample index);  no hit: depth = t_miss, tri = -1, normal = 0.
 * --------------------------------------------------------------------------------------------- */
int tdgp_mesh_visibility_ms(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const float* c2w, const float* focal, int C,
                            int h, int w, int samples, float near_, int cull, uint64_t* vis, tdgp_stream_t stream);
int tdgp_mesh_resolve_ms(const uint64_t* vis, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const float* c2w,
                         const float* focal, int C, int h, int w, int samples, float t_miss, const float* vertex_normal, const float* vertex_rgb,
                         const uint8_t* image, int n, int r, int W, int H, int filter, int mode, const float* light, float ambient,
                         const float* albedo, const float* background, float* rgb, float* coverage, int32_t* status, float* depth, int32_t* tri,
                         float* normal, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh components (csrc/mesh_components.hip; the reference's users split the mesh on the host with trimesh): connected components of the
 * indexed mesh tdgp_mcubes_emit leaves on the device, per-component measurements, and an order-preserving filter.
 *   tdgp_mesh_labels -> tdgp_mesh_component_ids -> tdgp_mesh_component_stats (+ a stable sort by the caller) -> tdgp_mesh_component_sums
 *   -> (the caller chooses keep[K]) -> tdgp_mesh_compact_count -> tdgp_mesh_compact_emit
 * Common: triangles [T,3] int32, 0 <= T, V <= 2^31 - 1; a triangle with an index outside [0, V) is skipped by every kernel and the index is
 * never dereferenced.  Two vertices are connected when a triangle names both (triangles sharing ONE vertex are in one component); a vertex no
 * triangle names is a component of its own; degenerate and duplicate triangles connect what they name.  Workspaces are caller-owned, 16-byte
 * aligned, sized by the *_workspace_bytes queries (-1 for sizes they refuse); no kernel waits for another workgroup; integer outputs are
 * pure functions of the inputs and every floating-point output is the same bytes on every run.
 *
 * tdgp_mesh_labels: label[v] = the smallest vertex index of v's component (int32 [V]).  A lock-free union-find over a parent array in the
 *   workspace with parent[v] <= v at all times (the larger root is linked under the smaller by a compare-and-swap; a failed one is retried from
 *   the value it returned, and the larger of the pair strictly decreases, so the retry is bounded); every access to the array in that pass is an
 *   agent-scope relaxed atomic.  The first int64 of the workspace receives the number of failed compare-and-swaps of the call (a diagnostic).
 * tdgp_mesh_component_ids: component[v] int32 = the dense id of v's component, 0 .. K-1 in the order of the components' smallest vertices;
 *   K is left as one int64 at the START of the workspace, the one number the caller reads back.
 * tdgp_mesh_component_stats: component [V], K -> tri_count int64 [K] (a triangle belongs to the component of its FIRST vertex), vert_count
 *   int64 [K], bbox_min / bbox_max fp32 [K,3] (exact minima / maxima; -0 orders below +0), and per triangle t: tri_key int32 [T] (its component;
 *   K for a skipped triangle) and the two terms, in double from the fp32 vertices a, b, c widened exactly, every operation rounded once:
 *     u = b - a, w = c - a, n = (u1*w2 - u2*w1, u2*w0 - u0*w2, u0*w1 - u1*w0);  area_term = 0.5 * sqrt((n0*n0 + n1*n1) + n2*n2);
 *     x = (b1*c2 - b2*c1, b2*c0 - b0*c2, b0*c1 - b1*c0);  vol_term = (a0*x0 + a1*x1) + a2*x2      (six times the signed volume of the tetrahedron
 *     (0, a, b, c): the division by 6 is applied ONCE to the sum, so integer coordinates give exact volumes).
 *   Counts and boxes use integer atomics (exact, order-independent); nothing is summed in floating point here.
 * tdgp_mesh_component_sums: order int64 [T] = the triangle indices sorted by tri_key with the triangle order kept inside a key (a stable
 *   sort), start int64 [K] = the exclusive prefix sum of tri_count -> area [K], volume [K] in double.  THE SUMMATION ORDER, per component with
 *   its n triangles t_0 < t_1 < ... < t_{n-1}: lane l of 256 adds the terms of t_l, t_{l+256}, t_{l+512}, ... in that order onto 0.0; then for
 *   d = 128, 64, ..., 1 lane l < d adds lane l + d's partial onto its own; area = lane 0's, volume = lane 0's / 6.
 * tdgp_mesh_compact_count: keep uint8 [K] -> V' = vertices whose component is kept, T' = triangles all three of whose corners are kept, as two
 *   int64 at the START of the workspace (the one pair read back).  tdgp_mesh_compact_emit (same inputs and workspace): the kept vertices
 *   in their original order [V',3], the kept triangles in their original order re-indexed [T',3], vertex_map int32 [V] (new index or -1), and
 *   for each of num_attr fp32 arrays [V, attr_channels[i]] its kept rows [V', attr_channels[i]].  attr_in / attr_out / attr_channels are HOST
 *   arrays (of device pointers / of ints).  Positions come from scans alone; writes never pass the V' / T' given.
 * --------------------------------------------------------------------------------------------- */
int64_t tdgp_mesh_labels_workspace_bytes(int64_t T, int64_t V);
int     tdgp_mesh_labels(const int32_t* triangles, int64_t T, int64_t V, int32_t* label, void* workspace, int64_t workspace_bytes,
                         tdgp_stream_t stream);
int64_t tdgp_mesh_component_ids_workspace_bytes(int64_t V);
int     tdgp_mesh_component_ids(const int32_t* label, int64_t V, int32_t* component, void* workspace, int64_t workspace_bytes,
                                tdgp_stream_t stream);
int     tdgp_mesh_component_stats(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const int32_t* component, int64_t K,
                                  int64_t* tri_count, int64_t* vert_count, float* bbox_min, float* bbox_max, int32_t* tri_key,
                                  double* area_term, double* vol_term, tdgp_stream_t stream);
int     tdgp_mesh_component_sums(const int64_t* order, const int64_t* start, const int64_t* tri_count, int64_t K, int64_t T,
                                 const double* area_term, const double* vol_term, double* area, double* volume, tdgp_stream_t stream);
int64_t tdgp_mesh_compact_workspace_bytes(int64_t T, int64_t V);
int     tdgp_mesh_compact_count(const int32_t* triangles, int64_t T, int64_t V, const int32_t* component, const uint8_t* keep, int64_t K,
                                void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);
int     tdgp_mesh_compact_emit(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const int32_t* component,
                               const uint8_t* keep, int64_t K, void* workspace, int64_t workspace_bytes, float* out_vertices, int64_t V_out,
                               int32_t* out_triangles, int64_t T_out, int32_t* vertex_map, const void* const* attr_in, void* const* attr_out,
                               const int32_t* attr_channels, int num_attr, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh surfaces (csrc/mesh_surface.hip; the reference's users smooth the mesh and take its vertex normals on the host, trimesh / MeshLab):
 * the vertex -> triangle incidence of the indexed mesh on the device, in a defined order, and the gathers over it.
 *   tdgp_mesh_corner_table -> tdgp_mesh_vertex_normals | tdgp_mesh_boundary_vertices | tdgp_mesh_smooth_step (ping-pong, one table)
 *   tdgp_mesh_resolve -> tdgp_mesh_interp_normals -> tdgp_mesh_shade        (smooth-shaded mesh frames without a field pass)
 * Common: the rules of the two blocks above, unchanged -- triangles [T,3] int32, vertices [V,3] fp32; a triangle naming an index outside
 * [0, V) is skipped by every kernel and the index is never dereferenced; arguments are checked before any launch; empty inputs are no-ops;
 * workspaces are caller-owned, 16-byte aligned, sized by the *_workspace_bytes query (-1 for sizes it refuses); no kernel waits for another
 * workgroup; there are no floating-point atomics; every floating-point operation is rounded once, in the order written (no contraction into
 * FMA); `(double)` of a float is exact, `(float)` of a double rounds to nearest even; `/` and sqrt are correctly rounded; comparisons are
 * ordered.  Here 3 T <= 2^31 - 1 and V <= 2^31 - 2 (corner ids and start[V] are int32).
 *
 * tdgp_mesh_corner_table: corner 3t + i is slot i of triangle t.  -> degree int32 [V] = the number of corners of non-skipped triangles that
 *   name v (a triangle naming v twice counts twice);  start int32 [V+1] = the exclusive prefix sum of degree, start[V] = the total;  corner
 *   int32, a buffer of 3 T entries of which the first start[V] are written: for each vertex v, at [start[v], start[v+1]), its corners in
 *   ASCENDING CORNER ID.  The total is also left as one int64 at the START of the workspace, the one number the caller reads back.  The table
 *   is a pure function of `triangles`: the counts are integer atomics (order-independent), start comes from scans, and a corner's position
 *   inside its vertex's range is its RANK there (the number of smaller corner ids of the range, counted from a scratch list in the workspace
 *   whose own order is not relied upon) -- never the arrival order of an atomic.  Cost per vertex O(degree^2) reads spread over degree lanes.
 *   V == 0: start[0] = 0 and the total 0 are written, nothing else.
 *
 * The three gathers take (start, corner) as given -- a caller may pass a table of its own.  The range of v is [start[v], start[v+1]) clamped
 * into [0, min(start[V], 3T)] (`corner` must hold start[V] entries); d = the length of that range.  An entry outside [0, 3T), or whose
 * triangle is skipped, adds nothing and is not dereferenced.  One lane per vertex; each sum below is SEQUENTIAL in table order, so the
 * outputs are pure functions of the arrays as given (the same bytes on every run) but, unlike vis, NOT invariant under a permutation of
 * the triangles.
 *
 * tdgp_mesh_vertex_normals: weight 0 (area) | 1 (uniform) -> normal_out [V,3] fp32.  In double, s = 0; for each corner of v in table order,
 *   with t = corner / 3 and v0, v1, v2 the triangle's vertices widened:  a = v1 - v0, b = v2 - v0,
 *   g = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0)  (tdgp_mesh_resolve's g).   weight 0: s_c = s_c + g_c.   weight 1: q = (g0*g0 + g1*g1)
 *   + g2*g2; if q > 0 and q < inf: s_c = s_c + g_c / sqrt(q), else the corner adds nothing.   Then q = (s0*s0 + s1*s1) + s2*s2; if q > 0 and
 *   q < inf: n_c = (float)(s_c / sqrt(q)), else n = 0 (so does a vertex no triangle names).
 *
 * tdgp_mesh_boundary_vertices: -> rim_out uint8 [V].  A neighbour of v is the vertex in the next or the previous slot of one of v's corners
 *   (v itself is not its own neighbour).  rim[v] = 1 iff some neighbour w is named next to v in exactly ONE of v's triangles (a triangle
 *   naming v in two slots is one triangle): v lies on an edge that one triangle uses.  Integer only; a pure function of the mesh.  The count
 *   is direct -- for each of the 2 d candidates, one walk over the d corners: O(d^2) per vertex; a vertex of more than 32 corners has its
 *   candidates spread over its wave.
 *
 * tdgp_mesh_smooth_step: factor (finite double), pinned uint8 [V] or NULL -> vertices_out [V,3], which must not overlap vertices_in.  Per
 *   vertex with d > 0 and not pinned, in double, s = 0; for each corner (t, i) in table order:  s = s + (double)v[tri[t][(i+1)%3]], then
 *   s = s + (double)v[tri[t][(i+2)%3]], component-wise.   m_c = s_c / (double)(2 d);   out_c = (float)(x_c + factor * (m_c - x_c)) with x the
 *   vertex's own position widened.  Pinned and d == 0 vertices are copied bit for bit.  (The umbrella operator with multiplicity: on a closed
 *   manifold every neighbour is counted twice, which is the plain neighbour mean -- no de-duplication is needed.)
 *
 * tdgp_mesh_interp_normals: tri int32 [rays], status int32 [rays], t_hit [rays] as tdgp_mesh_resolve wrote them, ray_o / ray_d [rays,3], the
 *   mesh, vertex_normal [V,3] -> normal [rays,3] IN PLACE.  Per ray with status == 1 and a triangle inside [0, T) whose indices lie in [0, V):
 *   x_c = o_c + d_c * t_hit (fp32, as tdgp_mesh_resolve forms it);  b0, b1, b2 EXACTLY tdgp_mesh_resolve's colour weights (one __device__
 *   function, csrc/mesh_bary.h, serves both);  m_c = (b0*n0_c + b1*n1_c) + b2*n2_c in double with n_i the vertex normals widened;
 *   q = (m0*m0 + m1*m1) + m2*m2;  if q > 0 and q < inf: normal_c = (float)(m_c / sqrt(q)), else the face normal already there stays.  Every
 *   other ray is not touched.  One writer per element.
 * --------------------------------------------------------------------------------------------- */
int64_t tdgp_mesh_corner_table_workspace_bytes(int64_t T, int64_t V);
int     tdgp_mesh_corner_table(const int32_t* triangles, int64_t T, int64_t V, int32_t* degree, int32_t* start, int32_t* corner,
                               void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);
int     tdgp_mesh_vertex_normals(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const int32_t* start,
                                 const int32_t* corner, int weight, float* normal_out, tdgp_stream_t stream);
int     tdgp_mesh_boundary_vertices(const int32_t* triangles, int64_t T, int64_t V, const int32_t* start, const int32_t* corner,
                                    uint8_t* rim_out, tdgp_stream_t stream);
int     tdgp_mesh_smooth_step(const float* vertices_in, const int32_t* triangles, int64_t T, int64_t V, const int32_t* start,
                              const int32_t* corner, double factor, const uint8_t* pinned, float* vertices_out, tdgp_stream_t stream);
int     tdgp_mesh_interp_normals(const int32_t* tri, const int32_t* status, const float* t_hit, const float* ray_o, const float* ray_d,
                                 int64_t rays, const float* vertices, int64_t V, const int32_t* triangles, int64_t T,
                                 const float* vertex_normal, float* normal, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh simplification (csrc/mesh_simplify.hip; the reference's users decimate a host copy of the mesh, trimesh / MeshLab): vertex clustering
 * on a uniform grid, each cluster's representative placed by its error quadric (Rossignac-Borrel 1993; Lindstrom 2000).
 *   tdgp_mesh_cluster_keys -> [stable sort of the keys: the caller's] -> tdgp_mesh_cluster_ids
 *   -> tdgp_mesh_cluster_triangles_relabel -> [stable sorts of the rotated triples: the caller's] -> _triangles_count -> _triangles_emit
 *   -> tdgp_mesh_corner_table(cluster_triangles, T, C) -> tdgp_mesh_cluster_place, tdgp_mesh_cluster_attribute
 * Common: the rules of the mesh blocks above, unchanged (skipped indices, checked arguments, empty inputs, caller-owned 16-byte aligned
 * workspaces sized by a query that answers -1 for sizes it refuses, no waiting between workgroups, no floating-point atomics, every
 * floating-point operation rounded once in the order written).  3 T <= 2^31 - 1, V <= 2^31 - 2.  cell and origin are three doubles each
 * on the HOST; every cell[c] is positive and finite, every origin[c] finite.  Every output is a pure function of the arrays as given.
 *
 * tdgp_mesh_cluster_keys: -> key int64 [V].  Per axis c, in double: q_c = floor(((double)v_c - origin_c) / cell_c).  If every q_c lies in
 *   [-2^20, 2^20): key = ((q_2 + 2^20) * 2^21 + (q_1 + 2^20)) * 2^21 + (q_0 + 2^20) -- the index (k_z * N + k_y) * N + k_x, N = 2^21, of the
 *   cell on a lattice whose indices are biased by 2^20 so that a key is never negative; it ascends with (q_2, q_1, q_0).  Otherwise (a
 *   non-finite coordinate, a cell outside the lattice) key = -1: the vertex belongs to no cluster.
 *
 * tdgp_mesh_cluster_ids: sorted_key int64 [V] ascending and order int32 [V], the STABLE permutation that sorted it (sorted_key[i] =
 *   key[order[i]]; equal keys by ascending vertex id; keys of -1 first) -> cluster int32 [V], start int32 (a buffer of V + 1 entries of which
 *   the first C + 1 are written), cluster_key int64 (a buffer of V entries, C written), and C as one int64 at the START of the workspace: the
 *   one number the caller reads back.  Position i is a head when sorted_key[i] >= 0 and (i == 0 or sorted_key[i-1] != sorted_key[i]); the id
 *   of a head is the number of heads before it (scans, no atomics), so clusters are numbered by ascending key.  start[id] = i and
 *   cluster_key[id] = sorted_key[i] at a head, start[C] = V: the members of cluster c are order[start[c] : start[c+1]], ascending vertex id,
 *   and order[0 : start[0]] are the vertices of no cluster.  cluster[order[i]] = the id of the run i lies in, -1 where sorted_key[i] < 0 (and
 *   for a vertex `order` does not name).  V == 0: start[0] = 0, C = 0.
 *
 * tdgp_mesh_cluster_triangles_relabel: -> cluster_triangles int32 [T,3] and rotated int32 [T,3].  cluster_triangles[t][i] =
 *   cluster[triangles[t][i]] (negative ids as -1), or -1 in all three slots when any index of t lies outside [0, V): what
 *   tdgp_mesh_corner_table takes with V = C.  A triangle SURVIVES when its three clusters are >= 0 and pairwise distinct; rotated[t] is then
 *   its triple rotated so that the smallest id comes first (the winding is kept: (a, b, c) and (a, c, b) stay different), else (-1, -1, -1).
 *
 * tdgp_mesh_cluster_triangles_count: rotated, perm int32 [T] or NULL -> keep uint8 [T] and the number kept as one int64 at the START of the
 *   workspace.  perm NULL: keep[t] = t survives.  perm: a permutation that sorts the rows of `rotated` lexicographically, STABLE (equal rows by
 *   ascending t): keep[perm[i]] = perm[i] survives and (i == 0 or rotated[perm[i-1]] != rotated[perm[i]]) -- of the triangles that share a
 *   triple up to rotation, the one of lowest index.  An entry of perm outside [0, T) is passed over.
 * tdgp_mesh_cluster_triangles_emit: the same workspace, untouched since the count -> out_triangles int32 [T_out,3] = cluster_triangles[t] for
 *   the kept t in ascending t, triangle_map int32 [T_out] = those t.  Positions come from scans; one beyond T_out is not written.
 *
 * tdgp_mesh_cluster_place: placement 0 (mean) | 1 (quadric) -> out_vertices [C,3] fp32.  One lane per cluster,
 *   everything in double and sequential.  The cell indices q_c are decoded from cluster_key; centre_c = origin_c + ((double)q_c + 0.5) *
 *   cell_c.  A position p of vertex v is RELATIVE: p_c = (double)v_c - centre_c.
 *   mean: s = 0; for each member in `order`: s_c = s_c + p_c; m_c = s_c / (double)members.   x = m.
 *   quadric: (corner_start, corner) is the corner table of cluster_triangles with V = C (ranges clamped as the gathers above clamp them).
 *   A = 0 (upper triangle), b = 0.  For each corner of the cluster in table order, t = corner / 3, with p0, p1, p2 the relative positions of
 *   triangles[t]'s vertices (a triangle naming an index outside [0, V) adds nothing):  e1 = p1 - p0, e2 = p2 - p0,
 *   n = (e1_1*e2_2 - e1_2*e2_1, e1_2*e2_0 - e1_0*e2_2, e1_0*e2_1 - e1_1*e2_0),  d = -((n_0*p0_0 + n_1*p0_1) + n_2*p0_2),
 *   A_rc = A_rc + n_r*n_c for r <= c,  b_r = b_r + n_r*d.  Once per corner: a triangle with two corners in the cluster counts twice, and a
 *   triangle that collapses counts too.  No corner: x = m.  Otherwise r_c = -b_c - ((A_c0*m_0 + A_c1*m_1) + A_c2*m_2), and the symmetric A is
 *   diagonalised by cyclic Jacobi: u = I; 8 sweeps over the pairs (0,1), (0,2), (1,2); a pair (p, q; the third index r) with a_pq == 0 is
 *   skipped, else  theta = (a_qq - a_pp) / (2 * a_pq),  t = (theta >= 0 ? 1 : -1) / (|theta| + sqrt(theta*theta + 1)),  c = 1 / sqrt(t*t + 1),
 *   s = t*c;  a_pp = a_pp - t*a_pq, a_qq = a_qq + t*a_pq, a_pq = a_qp = 0;  a_rp = a_pr = c*a_rp - s*a_rq and a_rq = a_qr = s*a_rp + c*a_rq
 *   (both from the old values);  for k = 0, 1, 2: u_kp = c*u_kp - s*u_kq and u_kq = s*u_kp + c*u_kq (old values).  l_i = a_ii,
 *   l_max = the largest.  For i = 0, 1, 2 with l_i > rank_tol * l_max: coef = ((u_0i*r_0 + u_1i*r_1) + u_2i*r_2) / l_i, x_c = x_c + u_ci*coef.
 *   If any x_c is not inside [-cell_c * 0.5, cell_c * 0.5] (NaN included): x = m (Lindstrom's fallback).
 *   Both: out_c = (float)(centre_c + x_c).
 * tdgp_mesh_cluster_attribute: attribute fp32 [V, channels], 1 <= channels <= 64 -> out fp32 [C, channels]: per cluster and channel the sum
 *   of the members' values in `order`, in double, divided by their number, rounded once.
 * --------------------------------------------------------------------------------------------- */
int     tdgp_mesh_cluster_keys(const float* vertices, int64_t V, const double* cell, const double* origin, int64_t* key, tdgp_stream_t stream);
int64_t tdgp_mesh_cluster_ids_workspace_bytes(int64_t V);
int     tdgp_mesh_cluster_ids(const int64_t* sorted_key, const int32_t* order, int64_t V, int32_t* cluster, int32_t* start,
                              int64_t* cluster_key, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);
int     tdgp_mesh_cluster_triangles_relabel(const int32_t* triangles, int64_t T, int64_t V, const int32_t* cluster,
                                            int32_t* cluster_triangles, int32_t* rotated, tdgp_stream_t stream);
int64_t tdgp_mesh_cluster_triangles_workspace_bytes(int64_t T);
int     tdgp_mesh_cluster_triangles_count(const int32_t* rotated, const int32_t* perm, int64_t T, uint8_t* keep, void* workspace,
                                          int64_t workspace_bytes, tdgp_stream_t stream);
int     tdgp_mesh_cluster_triangles_emit(const int32_t* cluster_triangles, int64_t T, const uint8_t* keep, void* workspace,
                                         int64_t workspace_bytes, int32_t* out_triangles, int64_t T_out, int32_t* triangle_map,
                                         tdgp_stream_t stream);
int     tdgp_mesh_cluster_place(const float* vertices, int64_t V, const int32_t* order, const int32_t* start, const int64_t* cluster_key,
                                int64_t C, const double* cell, const double* origin, const int32_t* triangles, int64_t T,
                                const int32_t* corner_start, const int32_t* corner, int placement, double rank_tol, float* out_vertices,
                                tdgp_stream_t stream);
int     tdgp_mesh_cluster_attribute(const float* attribute, int channels, int64_t V, const int32_t* order, const int32_t* start, int64_t C,
                                    float* out, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh decimation (csrc/mesh_decimate.hip; the reference's users decimate a host copy of the mesh, trimesh / MeshLab): round-based quadric
 * edge collapse (Garland-Heckbert 1997) with a link-condition test.  Every round collapses an independent set of edges at once.
 *   tdgp_mesh_corner_table -> tdgp_mesh_boundary_vertices (once: the rim is FIXED from round 0) -> tdgp_mesh_decimate_quadrics (once)
 *   per round: tdgp_mesh_corner_table -> _decimate_candidates -> _decimate_claim -> _decimate_select -> [the count is read back; with a target
 *   the caller keeps the kmax smallest keys: a sort is plumbing] -> _decimate_apply -> tdgp_mesh_cluster_triangles_relabel (cluster = parent)
 *   -> _triangles_count (perm NULL) -> _triangles_emit;   at the end: _decimate_gather_count -> _decimate_gather -> _triangles_relabel
 * Common: the rules of the mesh blocks above, unchanged (skipped indices are never dereferenced, checked arguments, empty inputs, caller-owned
 * 16-byte aligned workspaces sized by a query that answers -1 for sizes it refuses, no waiting between workgroups, no floating-point atomics,
 * every floating-point operation rounded once in the order written, `/` and sqrt correctly rounded).  3 T <= 2^31 - 1, V <= 2^31 - 2.  The
 * working arrays live across the rounds in DOUBLE: position [V,3], quadric [V,10] (the upper triangle of the symmetric 4x4 in the order 00 01
 * 02 03 11 12 13 22 23 33), weight [V], attribute [V,channels]; parent int32 [V] starts as the identity and parent[removed] = survivor is
 * never undone (a vertex is alive while parent[v] == v; the current triangles name alive vertices only).  (start, corner) is the corner
 * table of the CURRENT triangles with V vertices, ranges clamped as the gathers of the mesh-surface block clamp them; N(v) is the set of
 * vertices in the next or previous slot of v's corners.  Every output is a pure function of the arrays as given.
 *
 * tdgp_mesh_decimate_quadrics: position = the vertices widened.  Per vertex, Q = 0, w = 0; for each of its corners in table order, with p0, p1,
 *   p2 the triangle's vertices in SLOT order, widened:  e1 = p1 - p0, e2 = p2 - p0,  n = (e1_1*e2_2 - e1_2*e2_1, e1_2*e2_0 - e1_0*e2_2,
 *   e1_0*e2_1 - e1_1*e2_0),  l = sqrt((n_0*n_0 + n_1*n_1) + n_2*n_2);  unless 0 < l < inf the triangle adds nothing;  q = (n_0/l, n_1/l, n_2/l,
 *   -((q_0*p0_0 + q_1*p0_1) + q_2*p0_2)),  g = l * 0.5;  Q_rc = Q_rc + (g*q_r)*q_c for r <= c;  w = w + g.
 *
 * tdgp_mesh_decimate_candidates: one lane per corner k = 3t + i, a = tri[t][i], b = tri[t][(i+1)%3] -> key uint64 [3T], placement double [3T,3],
 *   opposite int32 [3T,2] (the last two written for passing corners only).  max_error 0: no bound.  key = all ones unless ALL of:
 *   a < b;  not (rim[a] and rim[b]) (rim uint8 [V] or NULL);  exactly two of a's corners lie in triangles that name b -- c and d are their third
 *   vertices, in table order -- and c != d;  c and d have more than 3 corners each;  no vertex of N(a) other than a, b, c, d is in N(b) (the link
 *   condition |N(a) n N(b)| == 2);  Q = Q_a + Q_b, w = w_a + w_b, A = the 3x3 of Q, bv = (Q_03, Q_13, Q_23);  x = p_a if rim[a], else p_b if
 *   rim[b], else the minimiser of tdgp_mesh_cluster_place (r = -bv - A m, the 8-sweep Jacobi, the eigen-directions above rank_tol * l_max:
 *   csrc/quadric_solve.h serves both) started from m = (p_a + p_b) * 0.5, and m itself if any x_c is not finite;
 *   Ax_c = (A_c0*x_0 + A_c1*x_1) + A_c2*x_2,  cost = (((x_0*Ax_0 + x_1*Ax_1) + x_2*Ax_2) + 2 * ((bv_0*x_0 + bv_1*x_1) + bv_2*x_2)) + Q_33;
 *   cost is not NaN, and below 0 it counts as 0;  with a bound, cost <= (max_error*max_error) * w: the area-weighted RMS distance to the
 *   accumulated planes, not the Hausdorff distance (that one is measured by the mesh-distance block below);  no flip: for every corner of a whose triangle does not name b (then of b, not naming a),
 *   with p the triangle's positions in slot order and p' the same with that corner's slot moved to x,  n0 = cross(p1-p0, p2-p0),
 *   n1 = cross(p'1-p'0, p'2-p'0),  (n0_0*n1_0 + n0_1*n1_1) + n0_2*n1_2 > 0.
 *   Then key = (bits of (float)cost << 32) | mix(k), with mix(h): h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16
 *   on uint32 -- a bijection, so no two corners share a key, and on flat regions (every cost exactly 0) the order is scattered, not a chain.
 * tdgp_mesh_decimate_claim: best uint64 [V] = all ones, then every passing corner does best[v] = min(best[v], key) for v in {a, b} u N(a) u
 *   N(b): ONE unsigned 64-bit atomic minimum per vertex (tdgp_mesh_visibility's), whose result does not depend on the order of its operands.
 * tdgp_mesh_decimate_select: flag[k] = 1 iff key[k] is not all ones and best[v] == key[k] for v in {a, b, c, d};  selected int32 (a buffer of
 *   3 T entries) = the flagged corners, ascending; their number as one int64 at the START of the workspace.  Two selected edges cannot touch
 *   each other's one-rings or share an opposite vertex, so every test above still holds when all of them are collapsed together.
 * tdgp_mesh_decimate_apply: one lane per entry of `selected` [K] (the caller may have trimmed it).  The survivor s is b when rim[b] and not
 *   rim[a], else a; r is the other.  From the OLD p_a, p_b:  d = p_b - p_a,  t = (((x_0-a_0)*d_0 + (x_1-a_1)*d_1) + (x_2-a_2)*d_2) / ((d_0*d_0 +
 *   d_1*d_1) + d_2*d_2), clamped into [0, 1] (NaN -> 0);  attribute_s = (1 - t)*attribute_a + t*attribute_b per channel;  Q_s = Q_a + Q_b,
 *   w_s = w_a + w_b,  p_s = x = placement[k];  parent[r] = s.
 * tdgp_mesh_decimate_gather_count: the number of alive vertices as one int64 at the START of the workspace (scans).
 * tdgp_mesh_decimate_gather: the same workspace, untouched -> out_vertices fp32 [V_out,3] and out_attribute fp32 [V_out,channels] = the alive
 *   vertices in ascending id, each double rounded once;  vertex_map int32 [V] = the output index of the alive vertex at the end of v's parent
 *   chain (followed for at most max_hops steps: the number of rounds suffices), -1 if none.
 * --------------------------------------------------------------------------------------------- */
int     tdgp_mesh_decimate_quadrics(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const int32_t* start,
                                    const int32_t* corner, double* position, double* quadric, double* weight, tdgp_stream_t stream);
int     tdgp_mesh_decimate_candidates(const double* position, const double* quadric, const double* weight, const uint8_t* rim,
                                      const int32_t* triangles, int64_t T, int64_t V, const int32_t* start, const int32_t* corner,
                                      double max_error, double rank_tol, uint64_t* key, double* placement, int32_t* opposite,
                                      tdgp_stream_t stream);
int     tdgp_mesh_decimate_claim(const uint64_t* key, const int32_t* triangles, int64_t T, int64_t V, const int32_t* start,
                                 const int32_t* corner, uint64_t* best, tdgp_stream_t stream);
int64_t tdgp_mesh_decimate_select_workspace_bytes(int64_t T);
int     tdgp_mesh_decimate_select(const uint64_t* key, const uint64_t* best, const int32_t* opposite, const int32_t* triangles, int64_t T,
                                  int64_t V, uint8_t* flag, int32_t* selected, void* workspace, int64_t workspace_bytes,
                                  tdgp_stream_t stream);
int     tdgp_mesh_decimate_apply(const int32_t* selected, int64_t K, const int32_t* triangles, int64_t T, int64_t V, const uint8_t* rim,
                                 const double* placement, double* position, double* quadric, double* weight, double* attribute,
                                 int channels, int32_t* parent, tdgp_stream_t stream);
int64_t tdgp_mesh_decimate_gather_workspace_bytes(int64_t V);
int     tdgp_mesh_decimate_gather_count(const int32_t* parent, int64_t V, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);
int     tdgp_mesh_decimate_gather(const double* position, const double* attribute, int channels, const int32_t* parent, int64_t V,
                                  int64_t max_hops, void* workspace, int64_t workspace_bytes, float* out_vertices, int64_t V_out,
                                  float* out_attribute, int32_t* vertex_map, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh distance (csrc/mesh_distance.hip; the reference's users measure a simplified mesh against its source in MeshLab / Metro): a uniform
 * grid over the triangles, the closest point of a mesh per query point, surface samples, and the statistics of their distances -- the
 * sampled two-sided surface distance (maximum = Hausdorff, area-weighted mean and RMS) that `max_error` above is NOT.
 *   grid:    _prepare -> [bounds, count and area sum read back] -> per try: _grid_count -> [the pair total read back; too many cells or pairs:
 *            the cell doubles] -> _grid_emit -> [a STABLE sort of the pairs by cell: plumbing] -> _cell_start
 *   query:   _closest (the walk through the grid, or brute_force = 1: the scan over all triangles)
 *   samples: _prepare -> _sample_count -> [the total read back] -> _sample_emit;   statistics: _closest -> _reduce -> [one read-back]
 * Common: the rules of the mesh blocks above, unchanged (checked arguments, empty inputs, caller-owned workspaces sized by a query that
 * answers -1 for sizes it refuses, no waiting between workgroups, no floating-point atomics, positions from scans only, every
 * floating-point operation in DOUBLE on the fp32 inputs widened exactly, rounded once in the order written, `/` and sqrt correctly
 * rounded).  T, V, N, P, S <= 2^31 - 1.  dot(x, y) = (x_0*y_0 + x_1*y_1) + x_2*y_2;  cross(x, y) = (x_1*y_2 - x_2*y_1, x_2*y_0 - x_0*y_2,
 * x_0*y_1 - x_1*y_0).  A triangle is VALID when its three indices are distinct and inside [0, V) and its nine coordinates are finite; the
 * others are never dereferenced and never listed.  Triangle ids always are indices into the input array.
 *
 * THE DISTANCE d2(p; a, b, c) and the closest point q:  ab = b - a, ac = c - a, ap = p - a, n = cross(ab, ac), nn = dot(n, n).
 *   Face case, when nn > 0 and dot(cross(c - b, p - b), n) >= 0 and dot(cross(a - c, p - c), n) >= 0 and dot(cross(ab, ap), n) >= 0:
 *   s = dot(ap, n), f = s / nn, q = p - n*f, d2 = s*s / nn.   Otherwise d2 = +inf and, for (x, y) = (a, b), (b, c), (c, a) in that order:
 *   e = y - x, ee = dot(e, e), t = 0 when ee == 0 else dot(p - x, e) / ee clamped into [0, 1], r = x + t*e, dd = dot(p - r, p - r); dd < d2
 *   replaces (d2, q) by (dd, r).  A collinear or point-like triangle has nn == 0 and is the union of its edges.  The closest triangle of a
 *   point has the smallest d2, ties to the smallest id: any traversal that never skips it returns the bits of the scan over all triangles.
 *
 * tdgp_mesh_distance_prepare: valid uint8 [T];  box fp32 [T,6] = the minimum and the maximum of the three vertices per axis (zeros when not
 *   valid);  area double [T] = 0.5 * sqrt(nn) (0 when not valid).
 * THE GRID (lo fp32 [3], cell fp32 > 0, dims int [3], each >= 1, their product <= 2^24; host memory):  the cell of a coordinate x on axis k
 *   is floor((x - lo_k) / cell) clamped into [0, dims_k - 1];  cell (cx, cy, cz) has the key (cz*dims_1 + cy)*dims_0 + cx.  The caller takes
 *   lo / hi = the minimum / maximum of the boxes of valid triangles, dims_k = floor((hi_k - lo_k) / cell) + 1, and the default cell
 *   (float)(2 * sqrt(area sum / valid count)) with the area summed by tdgp_mesh_distance_reduce.
 * tdgp_mesh_distance_grid_count: counts int32 [T] = the number of cells the box of a valid triangle overlaps (the product of its three cell
 *   ranges), 0 when not valid.
 * tdgp_mesh_distance_grid_emit: pair_cell / pair_triangle int32 [P], P = the sum of the counts: triangle t writes its cells (z outermost, x
 *   innermost) from the exclusive scan of the counts on.  Sorted by cell with a stable sort, every cell's list ascends in triangle id.
 * tdgp_mesh_distance_cell_start: cell_start int32 [cells + 1] from the sorted keys: cell_start[c] = the number of pairs with a key < c.
 * tdgp_mesh_distance_closest: one lane per point.  A point with a coordinate that is not finite: sqdist = distance = closest = NaN,
 *   triangle = -1, nothing is walked.  Else the minimum of d2 over the valid triangles (brute_force) or over the walk:  c_k = the point's
 *   cell, a_k = p_k - lo_k;  for r = 0, 1, ... max(dims) - 1: every cell at Chebyshev distance exactly r from c that lies in the grid has its
 *   list evaluated;  then for every axis k, with g = (|a_k| + mc) * 2^-48:  if c_k - r > 0 the low side is open, mc = (c_k - r)*cell (an exact
 *   product) and its distance is max(0, (a_k - mc) - g);  if c_k + r < dims_k - 1 the high side is open, mc = (c_k + r + 1)*cell and its
 *   distance is max(0, (mc - a_k) - g).  No open side: stop.  lb = the smallest of them: stop when (lb*lb) * (1 - 2^-40) > the running
 *   minimum.  (A triangle no visited cell lists lies wholly beyond one open side; g covers the rounding of the cell arithmetic, the factor
 *   that of d2 itself on triangles that are not needles.)  The loop ends after max(dims) shells at the latest.
 *   Outputs: sqdist double [N] = d2, distance fp32 [N] = (float)sqrt(d2), triangle int32 [N], closest fp32 [N,3] = q rounded once;  no valid
 *   triangle (or P == 0 on the walk): +inf, +inf, -1, NaN.  evaluated int32 [N] or NULL: the number of d2 evaluations of the point.
 * tdgp_mesh_distance_sample_count: counts int32 [T] = k*k + 3 for a valid triangle, k = ceil(sqrt(the largest of dot(e, e) over b - a, c - b,
 *   a - c) / spacing) clamped into [1, 64];  0 when not valid.
 * tdgp_mesh_distance_sample_emit: S = the sum of the counts.  From the exclusive scan of the counts on, triangle t writes: its three
 *   vertices, weight 0;  then for i = 0 .. k-1, j = 0 .. k-1-i:  u = (i + 1/3) / k, v = (j + 1/3) / k (1/3 the double constant);  then for
 *   i = 0 .. k-2, j = 0 .. k-2-i:  u = (i + 2/3) / k, v = (j + 2/3) / k;  the point (float)((a + u*ab) + v*ac) per axis, weight
 *   (0.5 * sqrt(nn)) / (k*k), triangle t.
 * tdgp_mesh_distance_reduce: weight double [N], distance fp32 [N] or NULL -> at the START of the workspace five 8-byte fields: the sums of w,
 *   of w*d and of w*(d*d) (d widened; the last two 0 without distances), the maximum of d as a double, its index as int64 (the lowest index
 *   among equals; NaN never is the maximum; -1 when there is none).  THE ORDER: block b of 256 holds elements 256 b .. 256 b + 255, zeros
 *   past N, and slot i takes slot i + s for s = 128, 64, ... 1;  then ONE block: slot t adds the block results t, t + 256, ... in that
 *   order, starting from 0, and the same tree follows.
 * --------------------------------------------------------------------------------------------- */
int     tdgp_mesh_distance_prepare(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, uint8_t* valid, float* box,
                                   double* area, tdgp_stream_t stream);
int     tdgp_mesh_distance_grid_count(const float* box, const uint8_t* valid, int64_t T, const float* lo, float cell, const int* dims,
                                      int32_t* counts, tdgp_stream_t stream);
int64_t tdgp_mesh_distance_scan_workspace_bytes(int64_t T);
int     tdgp_mesh_distance_grid_emit(const float* box, const int32_t* counts, int64_t T, const float* lo, float cell, const int* dims,
                                     void* workspace, int64_t workspace_bytes, int32_t* pair_cell, int32_t* pair_triangle, int64_t P,
                                     tdgp_stream_t stream);
int     tdgp_mesh_distance_cell_start(const int32_t* sorted_cell, int64_t P, int64_t cells, int32_t* cell_start, tdgp_stream_t stream);
int     tdgp_mesh_distance_closest(const float* points, int64_t N, const float* vertices, const int32_t* triangles, int64_t T, int64_t V,
                                   const uint8_t* valid, const float* lo, float cell, const int* dims, const int32_t* cell_start,
                                   const int32_t* pair_triangle, int64_t P, int brute_force, double* sqdist, float* distance,
                                   int32_t* triangle, float* closest, int32_t* evaluated, tdgp_stream_t stream);
int     tdgp_mesh_distance_sample_count(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const uint8_t* valid,
                                        float spacing, int32_t* counts, tdgp_stream_t stream);
int     tdgp_mesh_distance_sample_emit(const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const int32_t* counts,
                                       float spacing, void* workspace, int64_t workspace_bytes, float* points, double* weight,
                                       int32_t* triangle, int64_t S, tdgp_stream_t stream);
int64_t tdgp_mesh_distance_reduce_workspace_bytes(int64_t N);
int     tdgp_mesh_distance_reduce(const double* weight, const float* distance, int64_t N, void* workspace, int64_t workspace_bytes,
                                  tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh rays (csrc/mesh_rays.hip; the reference's users cast rays and bake ambient occlusion in MeshLab / Blender): what a ray hits on a
 * mesh, over THE GRID of the block above exactly as its entry points fill it (vertices, triangles, valid, lo, cell, dims, cell_start,
 * pair_triangle: the members of one grid; a grid of more than one cell needs a finite cell).
 *   tdgp_mesh_rays_cast  first hit or any hit of N rays, by the walk through the grid or (brute_force = 1) by the scan over all triangles
 *   tdgp_mesh_rays_ao    ambient occlusion of N points: R rays per point in any-hit mode, the unoccluded ones counted
 * Common: the rules of the block above, unchanged (checked arguments, N == 0 launches nothing, no workspace, no atomics, every
 * floating-point operation in DOUBLE, rounded once in the order written, `/` and sqrt correctly rounded, comparisons ordered).
 *
 * THE RAY AND THE TRIANGLE, hit(o, d; a, b, c; t_min, t_max) with o, d doubles and the corners fp32 widened exactly (the translate / shear /
 * scale form of Woop, Benthin and Wald, "Watertight Ray/Triangle Intersection", JCGT 2013):
 *   per ray:  kz = the axis of the largest |d_k|, ties to the lowest index;  kx = (kz + 1) mod 3, ky = (kx + 1) mod 3, the two swapped when
 *     d[kz] < 0;  Sx = d[kx] / d[kz],  Sy = d[ky] / d[kz],  Sz = 1 / d[kz].
 *   per corner p of (a, b, c):  P = p - o per axis;  Px = P[kx] - Sx*P[kz],  Py = P[ky] - Sy*P[kz],  Pz = Sz*P[kz].
 *   U = Cx*By - Cy*Bx,  V = Ax*Cy - Ay*Cx,  W = Bx*Ay - By*Ax.   A miss when one of U, V, W is < 0 and one is > 0 (zeros are inside).
 *   det = (U + V) + W;  a miss when det == 0.   t = ((U*Az + V*Bz) + W*Cz) / det.   Accepted iff t_min <= t <= t_max.
 *   Reported per hit: t;  bary = ((float)(V / det), (float)(W / det)), the weights of corners b and c (the convention of csrc/mesh_bary.h);
 *   side = +1 when det > 0, else -1.  The map into the ray's frame keeps orientation (an even permutation and Sz > 0, or an odd one and
 *   Sz < 0) and sends d to +z, and det = -(the z component of cross(B - A, C - A) in that frame): det > 0 iff the normal of the stored
 *   winding, cross(b - a, c - a), points against d -- the ray meets the side that normal points to.
 *   WATERTIGHT: (Px, Py) depends on p and the ray alone, never on the triangle.  For an edge (p, q) shared by two triangles, one holds it
 *   as Qx*Py - Qy*Px and the other as Px*Qy - Py*Qx: products commute and x - y = -(y - x) exactly, so the two edge functions are the same
 *   bits up to sign.  A ray for which one is < 0 finds the other > 0, and zeros are inside: no ray passes between two triangles that share
 *   an edge.  (Plain Moeller-Trumbore, which forms its edges per triangle, does not have this property.)
 *   THE HIT of a ray is the accepted VALID triangle with the smallest t, ties to the smallest index: independent of the visiting order, so
 *   any traversal that never skips the minimiser returns the bits of the scan over all valid triangles (brute_force = 1, the yardstick).
 *   A triangle whose projected area is at the rounding level of its edge functions (a needle seen end-on, a ray through the line of a
 *   collinear triangle) can be accepted at a t that leaves its own box; only for such a hit may walk and scan differ.
 *
 * THE WALK (one lane per ray, one-wave blocks).  P == 0: nothing is hit.  A grid of ONE cell: its list is tested, nothing else is computed.
 *   Else the axes are taken in the ray's order (x, y, z) = (kx, ky, kz), z the major one:  a_k = o_k - lo_k,  top_k = dims_k * cell,
 *   mag = the sum over x, y, z in that order of ((|o_k| + |lo_k|) + top_k),  slack = mag * 2^-48  (everything the walk computes on any axis
 *   is below mag, its roundings below 2^-50 mag).  floorcell(v, n) = floor(v / cell) clamped into [0, n - 1]: the very division and floor
 *   that listed the triangles, so it is monotone against them.
 *   1. The window:  t0 = t_min, t1 = t_max;  per axis x, y, z with the planes p0 = -slack, p1 = top_k + slack:  d_k == 0: nothing is hit
 *      unless p0 <= a_k <= p1;  else ta = (p0 - a_k) / d_k, tb = (p1 - a_k) / d_k, t0 = max(t0, min(ta, tb)), t1 = min(t1, max(ta, tb)).
 *      Nothing is hit unless t0 <= t1.
 *   2. z0 = a_z + t0*d_z, z1 = a_z + t1*d_z;  up = d_z > 0;  s = floorcell(up ? z0 - slack : z0 + slack, dims_z), the last slab
 *      floorcell(up ? z1 + slack : z1 - slack, dims_z).  At most dims_z slabs are taken, s moving by +1 (up) or -1:
 *      ta = ((s*cell - slack) - a_z) * Sz,  tb = (((s + 1)*cell + slack) - a_z) * Sz  (s*cell is an exact product),
 *      te = max(min(ta, tb), t0),  tx = min(max(ta, tb), t1).   STOP when te > the running minimum of t (any-hit: never).
 *      When te <= tx:  xa = a_x + te*d_x, xb = a_x + tx*d_x, columns floorcell(min(xa, xb) - slack, dims_x) .. floorcell(max(xa, xb) + slack,
 *      dims_x), rows likewise on y; the list of every cell of that rectangle in slab s is tested (y outer, x inner, the list in order).
 *      STOP after the last slab.
 *   Conservative: a hit at parameter t lies in its triangle's fp32 box, so some cell (cx, cy, cz) that lists the triangle has
 *   cz*cell - g <= a_z + t*d_z <= (cz + 1)*cell + g with g far below slack; slab cz therefore is among those taken, its [te, tx] holds t,
 *   and because |d_x|, |d_y| <= |d_z| the rectangle, grown by slack and mapped through the monotone floorcell, meets the triangle's
 *   column and row ranges.  A triangle not yet tested has t >= te of every slab not yet taken (te never decreases), which is why the stop
 *   is sound.  A triangle listed in several visited cells is tested again: the minimum cannot depend on it, and no "seen" set is kept.
 *   Any-hit mode leaves at the first accepted triangle and reports only the flag.
 *
 * tdgp_mesh_rays_cast: origins, directions fp32 [N,3], widened exactly;  t_min finite, t_min <= t_max (t_max may be +inf; else
 *   TDGP_EINVAL);  brute_force, any_hit in {0, 1}.  any_hit == 0 -> t double [N], depth fp32 [N] = (float)t, triangle int32 [N], bary fp32
 *   [N,2], side int8 [N] (hit may be NULL);  a ray with a component that is not finite or with d == (0, 0, 0): NaN, NaN, -1, NaN, 0;  a
 *   miss: +inf, +inf, -1, NaN, 0.  any_hit == 1 -> hit uint8 [N] only (the other five may be NULL): 1 iff some valid triangle is accepted
 *   (0 for a bad ray), which is triangle >= 0 of the first-hit mode.  evaluated int32 [N] or NULL: the triangle tests of the ray.
 * tdgp_mesh_rays_ao: points, normals fp32 [N,3];  tables fp32 [K,R,3] (unit directions round +z; the caller builds them), R in {16, 32, 64},
 *   K a power of two <= 64;  bias fp32 >= 0 finite, radius fp32 > 0 (+inf allowed), both widened.  One lane per (point i, direction k), a
 *   wave holds 64 / R points.  A point or a normal with a component that is not finite, or the normal (0, 0, 0): NaN.  Else
 *   j = 0 when K == 1, else ((uint32)i * 2654435761u) >> (32 - log2 K);  (x, y, z) = tables[j][k] widened;
 *   len = sqrt((n0*n0 + n1*n1) + n2*n2), N = (n0 / len, n1 / len, n2 / len);  the frame of Duff et al. ("Building an Orthonormal Basis,
 *   Revisited", JCGT 2017):  sg = Nz >= 0 ? 1 : -1,  a = -1 / (sg + Nz),  b = (Nx*Ny) * a,
 *   T = (1 + ((sg*Nx)*Nx)*a,  sg*b,  (-sg)*Nx),   B = (b,  sg + (Ny*Ny)*a,  -Ny);
 *   d_c = (x*T_c + y*B_c) + z*N_c,   o_c = p_c + bias*N_c;   the ray (o, d) is cast by THE WALK in any-hit mode over [0, radius] (a ray that
 *   is not finite or has d == 0 counts as unoccluded).  occlusion fp32 [N] = (float)(the number of unoccluded rays of the point) /
 *   (float)R: one 64-bit ballot and a population count over the point's R lanes -- an integer, whatever the order; P == 0 gives 1.
 * --------------------------------------------------------------------------------------------- */
int     tdgp_mesh_rays_cast(const float* origins, const float* directions, int64_t N, double t_min, double t_max, const float* vertices,
                            const int32_t* triangles, int64_t T, int64_t V, const uint8_t* valid, const float* lo, float cell, const int* dims,
                            const int32_t* cell_start, const int32_t* pair_triangle, int64_t P, int brute_force, int any_hit, double* t,
                            float* depth, int32_t* triangle, float* bary, int8_t* side, uint8_t* hit, int32_t* evaluated, tdgp_stream_t stream);
int     tdgp_mesh_rays_ao(const float* points, const float* normals, int64_t N, const float* tables, int K, int R, float bias, float radius,
                          const float* vertices, const int32_t* triangles, int64_t T, int64_t V, const float* lo, float cell, const int* dims,
                          const int32_t* cell_start, const int32_t* pair_triangle, int64_t P, float* occlusion, tdgp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Mesh textures (csrc/mesh_texture.hip; the reference's users bake a texture in MeshLab / Blender after decimating): a per-triangle atlas
 * whose layout is a pure function of the triangle count, filled from the field, and fetched at the hits of a mesh frame.
 *   tdgp_atlas_points -> [the field's colour at the points: the caller's] -> tdgp_atlas_texels
 *   tdgp_mesh_resolve -> tdgp_mesh_sample_texture -> tdgp_mesh_shade        (where tdgp_mesh_interp_normals sits for the normals)
 * Common: the rules of the mesh blocks above, unchanged -- triangles [T,3] int32, vertices [V,3] fp32, 0 <= T, V <= 2^31 - 1; a triangle
 * naming an index outside [0, V) is never dereferenced; arguments are checked before any launch; one writer per element, no atomics, no
 * workspace; every floating-point operation is rounded once in the order written (no contraction into FMA); `(double)` of a float or an
 * integer is exact, `(float)` of a double rounds to nearest even; `/` is correctly rounded; comparisons are ordered.
 *
 * THE ATLAS of T triangles at n texels (2 <= n <= 64; TDGP_EINVAL outside):  S = n + 2;  P = ceil(T / 2);  r = the smallest integer with
 *   r*r >= P;  W = r*S;  H = ceil(P / r)*S (T == 0: r = W = H = 0, nothing is launched).  W, H <= 16384, else TDGP_EUNSUPPORTED; any other
 *   (r, W, H) than these is TDGP_EINVAL.  The image is uint8 [H,W,3], row 0 at the top.  Tile k has its origin at (X0, Y0) = ((k % r)*S,
 *   (k / r)*S) and holds triangle 2k ("lower") and triangle 2k + 1 ("upper").  Texel (px, py) of a tile belongs to the lower triangle iff
 *   px + py <= n, else to the upper one; the owner's texel coordinates are (qx, qy) = (px, py) for the lower and (S-1-px, S-1-py) for the
 *   upper triangle, and its barycentric coordinates  b1 = qx / (n-1),  b2 = qy / (n-1),  b0 = (1 - b1) - b2  in double, NOT CLAMPED.
 *   Texel centres with qx + qy <= n - 1 lie on the triangle: its corners and edges are texel centres (v0 at q = (0,0), v1 at (n-1,0), v2 at
 *   (0,n-1)).  The diagonals beyond the hypotenuse (one for a lower, two for an upper triangle) are the gutter: they are sampled on the
 *   triangle's plane just outside it, b0 < 0.  This extrapolation is what makes a bilinear fetch reproduce a colour that is linear in
 *   position exactly, the hypotenuse included: the four taps of any point of the triangle lie in the triangle's own half tile.
 *   A texel of a tile >= P, and the upper half of the last tile when T is odd, is unowned.
 *
 * tdgp_atlas_points: -> points fp32 [H*W,3], owner int32 [H*W], one lane per texel, texel-major (texel i is row i / W, column i % W).
 *   owner = the triangle's index; -1 for an unowned texel and for a triangle with a vertex outside [0, V).  Owned:
 *   point_c = (float)((b0*v0_c + b1*v1_c) + b2*v2_c) in double with v_i the triangle's vertices widened.  owner -1: the point (0, 0, 0).
 *   There is no division other than by n - 1: a needle or a triangle of no area is well defined.
 *
 * tdgp_atlas_texels: rgb = the colour of texel i at rgb[i*rgb_stride + c], c = 0, 1, 2 (3 <= rgb_stride <= 1024 elements: the field's
 *   [., 4] rows are read in place), in the renderer's range [-1, 1]; owner int32 [texels]; fill = a HOST pointer to 3 bytes -> image uint8
 *   [texels,3].  A call may cover any run of texels (the pointers offset alike).  owner >= 0, in fp32:  k = c * 0.5 + 0.5;  if not (k > 0)
 *   then k = 0 (so does a NaN);  if k > 1 then k = 1;  byte = (uint8)rintf(k * 255) (round half to even).  owner < 0: byte_c = fill_c.
 *
 * tdgp_mesh_sample_texture: tri int32 [rays], status int32 [rays], t_hit [rays] as tdgp_mesh_resolve wrote them, ray_o / ray_d [rays,3], the
 *   mesh, image uint8 [H,W,3], (n, r, W, H) its atlas, filter 0 (nearest) | 1 (bilinear) -> colour fp32 [rays,3] in [0, 1], what
 *   tdgp_mesh_shade takes in mode 2.  A ray with status != 1, or a triangle k outside [0, T) or with an index outside [0, V): colour = 0.
 *   Otherwise x_c = o_c + d_c * t_hit (fp32, as tdgp_mesh_resolve forms it);  b0, b1, b2 EXACTLY tdgp_mesh_resolve's colour weights (one
 *   __device__ function, csrc/mesh_bary.h, serves all three kernels: they are clamped onto the triangle);  in double  u = b1 * (n-1),
 *   v = b2 * (n-1);  the tile coordinates are (tx, ty) = (u, v) for a lower (k even) and ((S-1) - u, (S-1) - v) for an upper triangle,
 *   each then brought into [0, S-1]: if not (tx >= 0) then tx = 0 (so does a NaN); if tx > S-1 then tx = S-1.  The tile is k / 2.
 *   nearest: x = rint(tx), y = rint(ty) (round half to even);  colour_c = (float)((double)byte(X0 + x, Y0 + y, c) / 255).
 *   bilinear: x0 = floor(tx), y0 = floor(ty);  fx = tx - x0, fy = ty - y0;  x1 = min(x0 + 1, S-1), y1 = min(y0 + 1, S-1) (the tap index is
 *   clamped to the tile);  gx = 1 - fx, gy = 1 - fy;  w00 = gx*gy, w10 = fx*gy, w01 = gx*fy, w11 = fx*fy;  t_ij = (double)byte(X0 + x_i,
 *   Y0 + y_j, c);  colour_c = (float)(((w00*t00 + w10*t10) + (w01*t01 + w11*t11)) / 255).
 * --------------------------------------------------------------------------------------------- */
int     tdgp_atlas_points(const float* vertices, int64_t V, const int32_t* triangles, int64_t T, int n, int r, int W, int H, float* points,
                          int32_t* owner, tdgp_stream_t stream);
int     tdgp_atlas_texels(const float* rgb, int64_t rgb_stride, const int32_t* owner, int64_t texels, const uint8_t* fill, uint8_t* image,
                          tdgp_stream_t stream);
int     tdgp_mesh_sample_texture(const int32_t* tri, const int32_t* status, const float* t_hit, const float* ray_o, const float* ray_d,
                                 int64_t rays, const float* vertices, int64_t V, const int32_t* triangles, int64_t T, const uint8_t* image,
                                 int n, int r, int W, int H, int filter, float* colour, tdgp_stream_t stream);

/* Exact order statistics without a sort: the quantile behind the marchers' `cut_quantile` option (tri_plane_renderer.py:324-326, 366-368:
 * torch.quantile of the activated densities; the non-flatness score renders with 0.5, non_flatness_score.py:9-11).
 * out3[0] = sorted(x)[k_lo] and out3[1] = sorted(x)[k_hi], exact bits; out3[2] = torch.lerp(out3[0], out3[1], weight), i.e.
 * a + w (b - a) for |w| < 0.5 and b - (b - a)(1 - w) otherwise, each as ONE fused multiply-add on the rounded difference (and 1 - w): the
 * way torch's GPU lerp kernel is compiled, which is what makes out3[2] the float torch.quantile returns on the device.  The caller turns (q, n) into
 * (k_lo, k_hi, weight) -- renderer.quantile_ranks restates torch.quantile's fp32 rank arithmetic.
 * -0.0 counts as +0.0; if any element is NaN all three outputs are NaN (as torch.quantile); every other value orders as a float.
 * Radix select over an order-preserving key in three passes of 11 / 11 / 10 bits (csrc/metrics.hip): x is read three times, nothing is
 * written but 48 KiB of histograms, nothing is read back, integer counts only: identical bytes from run to run.
 * 1 <= n <= 2^31 - 1; 0 <= k_lo <= k_hi <= k_lo + 1, k_hi < n; x and out3 4-byte aligned (any offset into a buffer works).
 * workspace: tdgp_quantile_select_workspace_bytes(n) bytes (-1 for an n it refuses), 16-byte aligned, caller-owned. */
int64_t tdgp_quantile_select_workspace_bytes(int64_t n);
int     tdgp_quantile_select(const float* x, int64_t n, int64_t k_lo, int64_t k_hi, float weight, float* out3, void* workspace,
                             int64_t workspace_bytes, tdgp_stream_t stream);

/* Depth maps [images, pixels] fp32 -> histograms [images, bins] int32: steps 1b and 2 of the non-flatness score on the device
 * (non_flatness_score.py:12 `clamp(min_depth, max_depth)`, :15 / :30 one torch.histc per depth map on a host tensor).
 * Per element in fp32, nothing fused: x = clamp(depth, lo, hi); bin = min((int)((x - lo) * bins / (hi - lo)), bins - 1), the product
 * rounded before the division -- torch.histc's arithmetic on a CPU tensor (dividing first differs next to bin edges unless `bins` or
 * `hi - lo` is a power of two).  A NaN depth is counted in no bin (the caller's row-sum check, :32-33, reports it).
 * 2 <= bins <= 1024, 1 <= pixels < 2^24 (a count stays exact as fp32), 1 <= images <= 65535, lo < hi finite.  `hist` is overwritten. */
int tdgp_depth_histc(const float* depth, int64_t images, int64_t pixels, float lo, float hi, int bins, int32_t* hist, tdgp_stream_t stream);

/* Precision / recall (src/metrics/precision_recall.py): the k-NN distance passes without a distance matrix in memory.  The reference
 * takes torch.cdist in fp16 over 10 000 x 10 000 blocks, copies every block to the host and runs kthvalue / <= there.
 * The distance, fixed so that a CPU check can be bit exact: features rounded to fp16 (RNE, as `.to(torch.float16)`);
 *   d2(i,j) = max(|a_i|^2 + |b_j|^2 - 2 a_i.b_j, 0): the dot product on v_mfma_f32_32x32x16_f16 (fp16 operands, fp32 accumulation), the
 *             norms summed in fp32 from the ROUNDED values, fl(fl(|a_i|^2 + |b_j|^2) - 2 dot);
 *   d = sqrtf(d2) correctly rounded, then rounded once to fp16 (RNE; overflow -> +inf).  Everything downstream compares these fp16 values;
 *   a NaN distance sorts last and compares false (torch.kthvalue / <=).
 * tdgp_pr_pack: x [n,F] fp32 -> packed [n,Fpad] fp16 bits, columns F..Fpad-1 zero, and norms [n] fp32.  Fpad: a multiple of 32 (the K step
 *   of the tile loop, two MFMA steps), F <= Fpad <= 65536; packed 16-byte aligned.
 * tdgp_pr_kth: kth[i] = the k1-th smallest (k1 = k + 1) of d(i, j) over ALL nc columns as fp16 bits [nr], i.e.
 *   dist.kthvalue(nhood_size + 1): when rows == cols the self distance is one of the candidates, duplicates count separately; fewer than k1
 *   non-NaN distances -> NaN (0x7e00).  1 <= k1 <= 8 and k1 <= nc.
 * tdgp_pr_member: member[i] = 1 if some column j has d(probe i, j) <= kth[j], else 0; uint8 [np].  kth: fp16 bits [nc] (a NaN entry admits
 *   nobody).
 * Both sets of a call must have been packed with the SAME Fpad (one Fpad argument serves both; the calls cannot check it).
 * Both run one tile kernel (128 x 128 tiles, each block a run of 8 column tiles) that leaves a partial per (run, row) in the workspace --
 * a sorted list of squared distances / one byte -- and a small merge kernel: no atomics, no kernel waits on another block, one writer per
 * partial, so the same bytes on every run whatever the block order.  1 <= nr, np, nc <= 2^24.
 * workspace: tdgp_pr_{kth,member}_workspace_bytes bytes (-1 for a shape they refuse), 16-byte aligned, caller-owned. */
int     tdgp_pr_pack(const float* x, int64_t n, int F, uint16_t* packed, int Fpad, float* norms, tdgp_stream_t stream);
int64_t tdgp_pr_kth_workspace_bytes(int64_t nr, int64_t nc, int k1);
int     tdgp_pr_kth(const uint16_t* rows, const float* row_norms, int64_t nr, const uint16_t* cols, const float* col_norms, int64_t nc, int Fpad,
                    int k1, uint16_t* kth, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);
int64_t tdgp_pr_member_workspace_bytes(int64_t np, int64_t nc);
int     tdgp_pr_member(const uint16_t* probes, const float* probe_norms, int64_t np, const uint16_t* cols, const float* col_norms,
                       const uint16_t* kth, int64_t nc, int Fpad, uint8_t* member, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);

/* FID feature moments (src/metrics/metric_utils.py:128-161: `x.sum(0)` and `x.T @ x` in fp64 per feature block, on host arrays): the running
 * raw moments of fp32 rows on the device.  rows [n,F] fp32 contiguous; s1 [F] and s2 [F,F] fp64, caller-owned running totals.
 * On return s1[f] += sum_i rows[i,f] and s2[f,g] += sum_i rows[i,f] * rows[i,g].
 * Arithmetic: every row value is widened fp32 -> fp64 (exact), every product is formed in fp64 (exact: 24 + 24 significand bits fit in 53),
 *   only the additions round; nothing is accumulated in fp32.  The Gram part runs on v_mfma_f64_16x16x4_f64.
 * s2 is symmetric bit for bit on return: 64 x 64 tiles on and above the diagonal are computed, each is written to both sides, and of a
 *   diagonal tile only the elements on or above the diagonal are used (whatever s2 held below the diagonal is overwritten by the mirror).
 * Rows and columns past n or F enter as zeros.  A NaN / Inf row value propagates as in IEEE arithmetic (0 * Inf = NaN).
 * Partition, a function of (n, F) alone: tiles x runs of rows, a run at least 512 rows long and tiles x runs <= 2048 blocks where that leaves
 *   more than one run.  One run adds in place; several runs leave one partial per (run, tile) in the workspace, and a merge kernel adds them to
 *   s2 in run order: no atomics, one writer per value, the same bytes on every run.
 * 0 <= n < 2^31 (n = 0: nothing is done), 1 <= F <= 16384, no alignment requirement on F; s1 / s2 / workspace 8-byte aligned.
 * workspace: tdgp_moments_workspace_bytes(n, F) bytes (-1 for a shape it refuses), caller-owned.  A refused shape or a workspace that is too
 * small returns TDGP_EINVAL before anything is launched. */
int64_t tdgp_moments_workspace_bytes(int64_t n, int F);
int     tdgp_moments_add(const float* rows, int64_t n, int F, double* s1, double* s2, void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);

/* Gaussian log-likelihood scores of feature rows ("Instance Selection for GANs", scripts/data_scripts/run_instance_selection.py:29-33: scikit-learn's
 * one-component GaussianMixture, float32 throughout for float32 features): the Mahalanobis part on the device, csrc/gaussian.hip.
 * rows [n,F] fp32 contiguous; mu [F] fp64; P [F,F] fp64 row-major, UPPER triangular: the precision Cholesky factor P = L^-T with L L^T = Sigma.
 * No element of P below the diagonal is ever read (the caller may leave anything there).  maha [n] fp64 is overwritten:
 *   maha[i] = sum_j ( sum_{k <= j} (rows[i,k] - mu[k]) * P[k,j] )^2.
 * Arithmetic: every row value is widened fp32 -> fp64 (exact); d = x - mu is rounded once in fp64; the contraction runs on
 *   v_mfma_f64_16x16x4_f64 with fp64 accumulation; squares and their sums are fp64; nothing is held in fp32.  Rows and columns past n or F enter as
 *   zeros.  A NaN / Inf row value propagates as in IEEE arithmetic into that row's result (0 * Inf = NaN, as numpy's `d @ triu(P)`); no other row
 *   sees it.
 * A row's result is a fixed function of that row, mu, P and F: the same bits whatever n is, wherever the row stands in the call and whichever
 *   mode runs, so a caller may pass rows in chunks of any size.  No atomics, one writer per value: the same bytes on every run.
 * 64-row x 64-column tiles of y = d P; the K loop of column tile tj stops at min(F, 64 (tj + 1)): the zero half of the triangle costs nothing.
 * Two modes, a function of (n, F) alone (tdgp_gaussian_maha_mode; -1 for a refused shape):
 *   TDGP_MAHA_DIRECT  F <= 64, or at least 512 row tiles (n > 32704): one block per row tile walks the column tiles in order and adds each tile's
 *                     per-row sum of squares q_t to the row's total; the workspace is not touched (16 bytes);
 *   TDGP_MAHA_SPLIT   otherwise: one block per (row tile, column tile) writes q_t to workspace[t][row]; a merge kernel adds q_0 + q_1 + ... in the
 *                     same order; the workspace is ceil(F / 64) * n * 8 bytes.
 * 0 <= n < 2^31 (n = 0: nothing is done), 1 <= F <= 16384, no alignment requirement on F; rows 4-byte, mu / P / maha / workspace 8-byte aligned.
 * workspace: tdgp_gaussian_maha_workspace_bytes(n, F) bytes (-1 for a shape it refuses), caller-owned.  A refused shape or a workspace that is too
 * small returns TDGP_EINVAL before anything is launched. */
#define TDGP_MAHA_DIRECT 0
#define TDGP_MAHA_SPLIT 1
int     tdgp_gaussian_maha_mode(int64_t n, int F);
int64_t tdgp_gaussian_maha_workspace_bytes(int64_t n, int F);
int     tdgp_gaussian_maha(const float* rows, int64_t n, int F, const double* mu, const double* P, double* maha, void* workspace,
                           int64_t workspace_bytes, tdgp_stream_t stream);

/* ADA augmentation pipe (src/training/augment.py of the reference), csrc/augment.hip.  All tensors fp32, contiguous, NCHW.
 * tdgp_augment_params: every per-sample parameter in one launch.  cfg: TDGP_AUGMENT_CFG_FLOATS floats on the HOST, the constructor's
 *   arguments in its order (xflip, rotate90, xint, xint_max, scale, rotate, aniso, xfrac, scale_std, rotate_max, aniso_std, xfrac_std,
 *   brightness, contrast, lumaflip, hue, saturation, brightness_std, contrast_std, hue_max, saturation_std, imgfilter, imgfilter_bands[4],
 *   imgfilter_std, noise, cutout, noise_std, cutout_size).  p: the strength, one float on the device.  Either `uniforms`
 *   [B, TDGP_AUGMENT_UNIFORMS] in [0, 1) and `normals` [B, TDGP_AUGMENT_NORMALS] (device), or use_percentile != 0 and `percentile`: the
 *   reference's debug_percentile (every draw replaced by that quantile of its distribution; the post-rotation is zero).
 *   Outputs (device; a null pointer skips that group): G_inv [B,3,3] pixel_out -> pixel_in, C [B,4,4], gains [B,4] of the band filter,
 *   noise_sigma [B], cutout [B,4] = (size_x, size_y, centre_x, centre_y).  Plain fp32 in the reference's order of operations.
 *   num_channels: hue and saturation are left out for a one-channel image.
 * tdgp_augment_geom: y = the geometric stage (margins over the whole batch, reflect pad, x2 upsampling with f, bilinear sampling through
 *   G_inv with zeros outside the padded image, x2 downsampling with f, crop) in one kernel; f: the 12 normalised low-pass taps (device).
 *   G_inv rows 0-1 are used (affine).  2 <= H, W <= 8192, B <= 65535.  Nothing is read back, no intermediate image is stored.
 * tdgp_augment_geom_adj: dx = the adjoint of the same operator applied to dy.  No atomics: the same bytes on every run.
 *   workspace: tdgp_augment_geom_adj_workspace_bytes bytes (-1 for a refused shape), 4-byte aligned, caller-owned.
 * tdgp_augment_color: y[:, :ncc] = C[:, :3, :3] x[:, :ncc] + C[:, :3, 3] (ncc = 3), or the scalar form of one colour channel (ncc = 1);
 *   the other channels pass through; then + noise * noise_sigma[b] (noise [B,C,H,W] or null), then the cutout mask (cutout [B,4] or null).
 *   Cmat null: no matrix.  transposed != 0 uses the transposed 3x3; with use_bias = 0 and no noise that is the adjoint.  x == y is allowed. */
#define TDGP_AUGMENT_CFG_FLOATS 31
#define TDGP_AUGMENT_UNIFORMS 29
#define TDGP_AUGMENT_NORMALS 12
int     tdgp_augment_params(const float* cfg, const float* p, int B, int H, int W, int num_channels, const float* uniforms, const float* normals,
                            int use_percentile, float percentile, float* G_inv, float* Cmat, float* gains, float* noise_sigma, float* cutout,
                            tdgp_stream_t stream);
int     tdgp_augment_geom(const float* x, const float* G_inv, const float* f, float* y, int B, int C, int H, int W, tdgp_stream_t stream);
int64_t tdgp_augment_geom_adj_workspace_bytes(int B, int C, int H, int W);
int     tdgp_augment_geom_adj(const float* dy, const float* G_inv, const float* f, float* dx, int B, int C, int H, int W, void* workspace,
                              int64_t workspace_bytes, tdgp_stream_t stream);
int     tdgp_augment_color(const float* x, float* y, const float* Cmat, int transposed, int use_bias, const float* noise, const float* noise_sigma,
                           const float* cutout, int B, int C, int H, int W, int num_color_channels, tdgp_stream_t stream);

/* Step tail of a training phase (training_loop.py:334-347: gradient exchange, sanitising, clipping, Adam) and the per-batch EMA update
 * (:357-367), csrc/step_tail.hip.  Multi-tensor kernels: ONE launch covers every tensor, a block works on one chunk of
 * TDGP_STEP_TAIL_CHUNK elements of one tensor, found through a chunk -> tensor map the caller builds.  All tensors fp32, contiguous,
 * 4-byte aligned (16-byte accesses where pointer and remaining length allow, scalar ones at ragged heads and tails).  No atomics, no
 * kernel waits on another: the same bytes on every run.  `chunk` must be TDGP_STEP_TAIL_CHUNK (a caller built against another constant
 * is refused).
 * A table is a DEVICE array of int64 words: `rows` rows of num_tensors words each, then num_blocks words "tensor of block b", then
 * num_blocks words "first element of block b inside its tensor".  Every block's range must lie inside its tensor; the caller guarantees it.
 *   step table (5 rows): parameter pointer, exp_avg pointer, exp_avg_sq pointer, element count, offset in the flat buffer (elements)
 *   ema table  (4 rows): source pointer, destination pointer, element count, kind (0: dst <- lerp(src, dst, beta); 1: dst <- src)
 * The table that changes from step to step (3 rows of num_tensors words, device): gradient pointer; -(lr / (1 - beta1^t)) and
 *   sqrt(1 - beta2^t) of the tensor's own step count t, each a double's bits.  They come from the host, in Python floats as torch does.
 * tdgp_grads_pack: flat[off_t + i] = grad_t[i] for every tensor t of the step table; grad_table: row 0 of the per-step table.  Replaces
 *   torch.cat.
 * tdgp_grads_sanitise_norm: in place on flat[0 .. total): x / world, then NaN -> 0, +inf -> 1e5, -inf -> -1e5 (the order of
 *   distributed.allreduce_gradients); block b writes partials[b] = the sum of the fp64 squares of its sanitised fp32 values, summed in fp64
 *   in a fixed order; a second one-block launch sums the partials in a fixed order and writes norm[0] = sqrt(sum) (fp64).
 *   num_partials must be ceil(total / chunk).
 * tdgp_adam_step: torch.optim.Adam's update (no amsgrad, no weight decay, no maximize) of every tensor of the step table with
 *   g = flat[off_t + i] * c, c = min(1, max_norm / (norm[0] + 1e-6)) (max_norm < 0: c = 1, norm may be null):
 *   m += (1 - beta1) (g - m); v = beta2 v + (1 - beta2) g g; p -= (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps), the two
 *   t-dependent factors read per tensor from step_table (all three rows are passed).  flat is not rescaled.  m, v and p are each evaluated in fp64 from the fp32
 *   operands and rounded once (as is the lerp of tdgp_ema_update).
 * tdgp_ema_update: every pair of the ema table; beta == 0 turns every kind-0 pair into a bitwise copy. */
#define TDGP_STEP_TAIL_CHUNK 4096
int     tdgp_grads_pack(const int64_t* grad_table, const int64_t* table, int num_tensors, int64_t num_blocks, int chunk, float* flat, int64_t total,
                        tdgp_stream_t stream);
int     tdgp_grads_sanitise_norm(float* flat, int64_t total, int world, int chunk, double* partials, int64_t num_partials, double* norm,
                                 tdgp_stream_t stream);
int     tdgp_adam_step(const int64_t* table, const int64_t* step_table, int num_tensors, int64_t num_blocks, int chunk, const float* flat,
                       int64_t total, const double* norm, double max_norm, double beta1, double beta2, double eps, tdgp_stream_t stream);
int     tdgp_ema_update(const int64_t* table, int num_tensors, int64_t num_blocks, int chunk, double beta, tdgp_stream_t stream);

/* Anti-aliased resampling with Pillow's arithmetic, csrc/resample.hip: the operation behind the reference's dataset scripts
 * (scripts/utils.py:116-120 center_resize_crop; the bicubic eval transform of scripts/data_scripts/extract_features.py), which reach it
 * through torchvision -> PIL.Image.resize.  All images of a call have one size and share one set of tables.
 *   src [B, H, W, C] (C in {1, 3}; the 16-bit entry: [B, H, W]), channel-last, contiguous.  The crop window (x0, y0, w, h) on the source is
 *   resampled to oh x ow, exactly as if it had been cropped first.
 *   Tables (device), one pair per axis, built by the caller in float64 for (w -> ow) and (h -> oh): bounds int32 [out, 2] = (first source
 *   index, number of taps), coeffs [out, ksize].  The pair of an axis whose size does not change must be NULL and that pass is not run;
 *   with both NULL the call copies the window.  Entries are clamped to the source extent before use.
 *   8 bit : int32 coefficients, round(w * 2^22) half away from zero; one output = clip((2^21 + sum pixel * k) >> 22, 0, 255) in int32.
 *           The caller asserts 255 * sum|k| + 2^21 < 2^31 when it builds a table.
 *   16 bit: float64 coefficients; ss = 0.0; ss += double(pixel) * k in tap order, every product and every sum rounded (nothing fused);
 *           v = int(ss + 0.5) for ss >= 0, int(ss - 0.5) otherwise.  saturate = 0 stores Pillow's byte pair hi = clip(v >> 8, 0, 255),
 *           lo = clip(v % 256, 0, 255) (C's %): 0 for v < 0 and 0xFF00 | (v & 255) for v > 65535; saturate = 1 stores 65535 for v > 65535.
 *           The rows between the passes always hold Pillow's bytes, so the two modes differ only where the LAST pass overflows.
 *   The horizontal pass runs first and rounds to the sample type; its rows [B, h, ow, C] are the only intermediate and live in `workspace`
 *   (tdgp_resample_workspace_bytes: 0 unless both passes run; -1 for a refused shape; aligned to a sample).
 * tdgp_resample_u8_to_f32: the same two passes, then the window (cx0, cy0, cw, ch) of the resized image, then
 *   ((float(v) / 255.0f) - mean[c]) / std[c], each fp32 operation rounded on its own, both divisions true divisions; stored channel-first,
 *   dst [B, C, ch, cw] fp32.  mean / std: C floats each on the HOST.  Only the kept columns pass through the workspace ([B, h, cw, C] bytes,
 *   tdgp_resample_u8_to_f32_workspace_bytes); the resized image itself is never stored.
 * Limits: every size <= 32768 per axis, B <= 65535 per call; any ksize (a tap loop).  Offsets are 64-bit.  Launches on `stream`; no
 * atomics; only the output rows (and the workspace) are written; nothing is read back. */
int64_t tdgp_resample_workspace_bytes(int64_t B, int h, int w, int oh, int ow, int C, int sample_bytes);
int     tdgp_resample_u8(const uint8_t* src, int64_t B, int H, int W, int C, int x0, int y0, int w, int h, const int32_t* hbounds,
                         const int32_t* hcoeffs, int hksize, const int32_t* vbounds, const int32_t* vcoeffs, int vksize, uint8_t* dst, int oh, int ow,
                         void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);
int     tdgp_resample_u16(const uint16_t* src, int64_t B, int H, int W, int x0, int y0, int w, int h, const int32_t* hbounds, const double* hcoeffs,
                          int hksize, const int32_t* vbounds, const double* vcoeffs, int vksize, uint16_t* dst, int oh, int ow, int saturate,
                          void* workspace, int64_t workspace_bytes, tdgp_stream_t stream);
int64_t tdgp_resample_u8_to_f32_workspace_bytes(int64_t B, int h, int w, int oh, int ow, int C, int cw);
int     tdgp_resample_u8_to_f32(const uint8_t* src, int64_t B, int H, int W, int C, int x0, int y0, int w, int h, const int32_t* hbounds,
                                const int32_t* hcoeffs, int hksize, const int32_t* vbounds, const int32_t* vcoeffs, int vksize, int oh, int ow, int cx0,
                                int cy0, int cw, int ch, const float* mean, const float* std, float* dst, void* workspace, int64_t workspace_bytes,
                                tdgp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TDGP_H */
