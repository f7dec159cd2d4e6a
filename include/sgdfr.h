/*
 * sgdfr.h -- C ABI of libsgdfr_hip.so: the MI355X (gfx950) StyleGAN2 generator hot path.
 *
 * Every entry point takes raw device pointers + sizes + a hipStream_t (passed as void*),
 * launches asynchronously on that stream, never synchronises, never allocates, and returns
 * 0 on success or a non-zero code with a message available from sgdfr_last_error().
 * Tensors are fp32, contiguous, NCHW unless a stride argument says otherwise.
 * Outputs are caller-allocated (the reference's natives allocate internally; the host mirror
 * in stylegan_directions_face_reenactment_amd/ does the torch.empty for them).
 *
 * Reference interface each symbol replaces (paths relative to the reference repo,
 * libs/gan/StyleGAN2/ unless noted):
 *
 *   sgdfr_fused_bias_act_f32   op/fused_bias_act.cpp:14-24  fused.fused_bias_act(input,bias,refer,act,grad,alpha,scale)
 *                              (kernel op/fused_bias_act_kernel.cu:18-49)
 *   sgdfr_upfirdn2d_f32        op/upfirdn2d.cpp:15-26       upfirdn2d.upfirdn2d(input,kernel,up_x,up_y,down_x,down_y,pad_x0..pad_y1)
 *                              (kernel op/upfirdn2d_kernel.cu:52-137; unlike :172-223 unsupported combos are an ERROR, never a silent no-op)
 *   sgdfr_linear_f32           model.py:148-157 EqualLinear.forward (F.linear + fused_leaky_relu),
 *                              libs/models/direction_matrix.py:41-48 (nn.Linear)
 *   sgdfr_pixelnorm_f32        model.py:11-16   PixelNorm.forward
 *   sgdfr_latent_prepare_f32   model.py:494-508 truncation + W->W+ broadcast, libs/utilities/generic.py:116-135 shift add
 *   sgdfr_modconv_prepack_f32  model.py:215,218-220,236 (scale*weight) -- layout change + sum-of-squares for demodulation
 *   sgdfr_style_demod_f32      model.py:235-240 modulation(style) and rsqrt(sum w^2 + 1e-8)
 *   sgdfr_styles_batched_f32   the same for all 20 modulated convs of Generator.forward (model.py:520-531) at once
 *   sgdfr_modconv2d_fwd_f32    model.py:232-273 ModulatedConv2d.forward (+ :282-287 NoiseInjection, op/fused_act.py:81-86
 *                              FusedLeakyReLU folded into the epilogue); the reference has NO native kernel for this --
 *                              its boundary is the Python method
 *   sgdfr_blur_bias_act_f32    model.py:257 Blur after the transposed conv (upfirdn2d pad (1,1)) + noise + bias + lrelu
 *   sgdfr_torgb_fwd_f32        model.py:350-359 ToRGB.forward (1x1 modconv, bias, Upsample(skip) :38-46, add)
 *   sgdfr_make_shift_f32       run_inference.py:201-254 Inference.make_shift, libs/utilities/utils_train.py:127-175 make_shift_vector
 *   sgdfr_make_shift_random_f32 libs/utilities/utils_train.py:227-286 (single-direction half of make_shift_vector_50)
 *   sgdfr_gt_reenacted_f32     libs/utilities/utils_train.py:291-374 get_params_gt_reenacted (per-row host loop with one
 *                              device->host read of target_indices there; one launch here), with batch_euler2axis of
 *                              libs/DECA/decalib/utils/rotation_converter.py:306-307
 *   sgdfr_pairloss_forward_f32 / _backward_f32  libs/utilities/utils_train.py:435-499 calculate_losses_paired: torch_range_1_to_255
 *                              (libs/utilities/image_utils.py:87-94), the pixel-wise L1 and the latent L1 regulariser
 *   sgdfr_sweep_plan_f32 / _rows_f32  libs/configs/config_directions.py:42-85 get_direction_info and the np.arange / one_hot loops of
 *                              run_facial_editing.py:172-189 and libs/utilities/visualization.py:46-60, for all ladders at once
 *   sgdfr_sweep_frames_f32     face_pool (AdaptiveAvgPool2d), add_border, tensor_to_image + astype(uint8) of the same scripts
 *   sgdfr_video_frames_f32     face_pool + generate_grid_image + tensor_to_image + np.uint8 + cvtColor of run_inference.py:180-195
 *   sgdfr_video_frames_px      the same frames from the uint8 target crops of preprocess_image (utils_inference.py:61-82), unconverted
 *   sgdfr_shaperender_forward_f32  libs/DECA/decalib/utils/renderer.py:237-293 SRenderY.render_shape (pytorch3d's rasterize_meshes there)
 */
#ifndef SGDFR_H
#define SGDFR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SGDFR_ABI_VERSION 23

/* modes of sgdfr_modconv2d_fwd_f32 */
#define SGDFR_MODE_PLAIN3 0 /* 3x3, pad 1, same resolution                      (model.py:267-271) */
#define SGDFR_MODE_UP3 1    /* 3x3 transposed stride 2 -> phase planes of size (H+1)x(W+1) (model.py:246-256) */
#define SGDFR_MODE_DOWN3 2  /* adjoint of UP3: 3x3 stride-2 conv reading phase planes [B,Cin,4,H+1,W+1] -> [B,Cout,H,W]
                               (the dX of the transposed conv; autograd of model.py:254) */

/* activation codes of sgdfr_linear_f32 */
#define SGDFR_ACT_NONE 0
#define SGDFR_ACT_LRELU 1 /* lrelu(v, slope) * gain */

int sgdfr_abi_version(void);
const char* sgdfr_last_error(void);

/* y[i] = act(x[i] + bias[(i / step_b) % size_b]) * scale ; act==3 (lrelu) only, grad in {0,1,2}:
 *   grad 0: y = (v>0 ? v : alpha*v) * scale, v = x + b
 *   grad 1: y = (ref>0 ? x : alpha*x) * scale           (bias ignored by callers: pass NULL)
 *   grad 2: y = 0
 * bias / ref may be NULL ("empty tensor" in the reference). */
int sgdfr_fused_bias_act_f32(const float* x, const float* bias, const float* ref, float* y, int64_t n,
                             int step_b, int size_b, int act, int grad, float alpha, float scale,
                             void* stream);

/* x [major, in_h, in_w, minor] -> y [major, out_h, out_w, minor],
 * out = ((in*up + pad0 + pad1 - k) / down) + 1 per axis; kernel k [kh, kw] is applied flipped
 * (true convolution).  Negative pads crop. */
int sgdfr_upfirdn2d_f32(const float* x, const float* k, float* y, int major, int in_h, int in_w, int minor,
                        int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1,
                        int pad_y0, int pad_y1, void* stream);

/* The two natives for every dtype the reference dispatches (AT_DISPATCH_FLOATING_TYPES_AND_HALF: fused_bias_act_kernel.cu:79,
 * upfirdn2d_kernel.cu:225): x / bias / ref / k / y all of `dtype`; half is computed in float and rounded once, double in double.
 * SGDFR_DTYPE_F32 forwards to the _f32 entry points above. */
#define SGDFR_DTYPE_F32 0
#define SGDFR_DTYPE_F16 1
#define SGDFR_DTYPE_F64 2
int sgdfr_fused_bias_act(const void* x, const void* bias, const void* ref, void* y, int64_t n, int step_b, int size_b, int act,
                         int grad, float alpha, float scale, int dtype, void* stream);
int sgdfr_upfirdn2d(const void* x, const void* k, void* y, int major, int in_h, int in_w, int minor, int kh, int kw, int up_x,
                    int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0, int pad_y1, int dtype, void* stream);

/* y[m, n] = act( (sum_k x[m*ldx + k] * w[n*K + k]) * wscale + bias[n] * bscale ), m<M, n<N.
 * bias may be NULL.  act: SGDFR_ACT_*. */
int sgdfr_linear_f32(const float* x, int64_t ldx, const float* w, const float* bias, float* y, int64_t ldy,
                     int M, int N, int K, float wscale, float bscale, int act, float slope, float gain,
                     void* stream);

/* y[b,:] = x[b,:] * rsqrt(mean(x[b,:]^2) + eps) */
int sgdfr_pixelnorm_f32(const float* x, float* y, int B, int D, float eps, void* stream);
/* its adjoint: dx[b,:] = r*g - x * r^3 * mean(g*x), r = rsqrt(mean(x^2) + eps)   (autograd of model.py:11-16) */
int sgdfr_pixelnorm_bwd_f32(const float* x, const float* g, float* dx, int B, int D, float eps, void* stream);

/* out[b,l,:] = t + psi * (v - t),   v = w[b,(l),:] + (l < shift_layers ? shift[b,(l),:] : 0)
 *   w:     [B, L, D] if w_is_plus else [B, D] (broadcast over l)
 *   shift: NULL, or [B, shift_layers, D] if shift_is_plus else [B, D] (added to the first shift_layers rows)
 *   trunc: NULL (no truncation, psi ignored) or [D]
 * Order matches generic.py:116-135 then model.py:494-500: shift first, truncation after. */
int sgdfr_latent_prepare_f32(const float* w, int w_is_plus, const float* shift, int shift_is_plus,
                             int shift_layers, const float* trunc, float psi, float* out, int B, int L, int D,
                             void* stream);

/* weight [Cout, Cin, k, k] -> wp [Cin, k*k, Cout] = weight * 1/sqrt(Cin*k*k)  and
 *                              q  [Cout, Cin]     = sum_taps wp^2 ,  qt [Cin, Cout] = q^T   (q, qt may be NULL) */
int sgdfr_modconv_prepack_f32(const float* weight, float* wp, float* q, float* qt, int Cout, int Cin, int k,
                              void* stream);

/* weight [Cout, Cin, k, k] -> wt [Cout, k*k, Cin] * 1/sqrt(Cin*k*k), taps reversed when flip != 0: the weight pack of
 * the ADJOINT convs (dL/dx): sgdfr_modconv2d_fwd_f32 with (Cin, Cout) exchanged, s <- d, d <- s;
 * PLAIN3 backward uses flip = 1 in mode PLAIN3, UP3 backward uses flip = 0 in mode DOWN3. */
int sgdfr_modconv_prepack_t_f32(const float* weight, float* wt, int Cout, int Cin, int k, int flip, void* stream);

/* s[b,i] = (sum_j style[b*ld_style + j] * mod_w[i*D + j]) / sqrt(D) + mod_b[i]
 * d[b,o] = rsqrt( sum_i s[b,i]^2 * q[o*Cin + i] + 1e-8 )        (skipped when d == NULL) */
int sgdfr_style_demod_f32(const float* style, int64_t ld_style, const float* mod_w, const float* mod_b,
                          const float* q, float* s, float* d, int B, int D, int Cin, int Cout, void* stream);

/* All style modulations and demodulation coefficients of one generator forward in two launches
 * (sgdfr_style_demod_f32 for every layer at once).  `layers` is a HOST array; layer i reads
 * latent[:, latent_index, :] of latent [B, L, D] and writes s [B,cin] and, when d != NULL, d [B,cout]. */
#define SGDFR_MAX_STYLE_LAYERS 40
typedef struct sgdfr_style_layer {
    const float* mod_w; /* [cin, D] */
    const float* mod_b; /* [cin]    */
    const float* q;     /* [cout, cin] or NULL */
    float* s;           /* [B, cin]  */
    float* d;           /* [B, cout] or NULL */
    int cin, cout, latent_index;
    /* Range plan of the fp16-split conv (csrc/split.hip), optional -- needs d.  A demodulated conv is invariant to a
     * per-image scale of its style row: y = d * conv(x*s, W) = (d * 2^-e) * conv(x * (s * 2^e), W).  With s_n / d_n given,
     * the launch also writes s_n[b,:] = s[b,:] * 2^e_b and d_n[b,:] = d[b,:] * 2^-e_b (exact powers of two) with e_b chosen
     * so that the conv's fp16 operand x*s_n*2^-4 tops out `headroom` binades below the fp16 maximum:
     *     e_b = 18 - headroom - L - floor(log2 max_i |s[b,i]|),   |x| < 2^L
     * L = x_log2, or floor(log2 *x_absmax)+1 when x_absmax (one fp32 bit pattern = max |x| over the input, written by
     * sgdfr_absmax_f32) is given.  The convs then see the same product range whatever the scale of the styles. */
    float* s_n;               /* [B, cin] or NULL */
    float* d_n;               /* [B, cout] or NULL */
    const unsigned* x_absmax; /* device, 1 word, or NULL */
    int x_log2, headroom;
} sgdfr_style_layer;
int sgdfr_styles_batched_f32(const float* latent, int B, int L, int D, const sgdfr_style_layer* layers, int n_layers,
                             void* stream);

/* The range plan above for ONE layer whose s / d already exist (autograd forward, stand-alone layer calls):
 * s_n = s * 2^e_b, d_n = d * 2^-e_b.  x_absmax: device words of fp32 bit patterns, one per image (x_absmax_bstride 1), n per
 * image whose maximum counts (x_absmax_bstride n > 1: the per-plane words of sgdfr_act_grad_reduce_f32), one for the whole batch
 * (0), or NULL (then |x| < 2^x_log2 is taken on trust). */
int sgdfr_split_range_f32(const float* s, const float* d, float* s_n, float* d_n, const unsigned* x_absmax,
                          int x_absmax_bstride, int x_log2, int headroom, int B, int Cin, int Cout, void* stream);

/* out[b] (or out[0] when per_image == 0) = bit pattern of max |x| over image b (over everything): non-negative floats order
 * like their bit patterns, so this is an atomicMax on words the call zeroes first.  A NaN or Inf anywhere gives a word
 * >= 0x7f800000.  x_bstride 0 = one image shared by the batch: only out[0] is written. */
int sgdfr_absmax_f32(const float* x, int64_t x_bstride, int64_t n_per_image, int B, unsigned* out, int per_image,
                     void* stream);

/* Shared-weight modulated 3x3 convolution on fp32 MFMA.
 *   x      [B, Cin, H, W]  (x_bstride = Cin*H*W, or 0 to broadcast one [Cin,H,W] constant over the batch)
 *   wp     [Cin, 9, Cout]  from sgdfr_modconv_prepack_f32
 *   s      [B, Cin], d [B, Cout] (d may be NULL = no demodulation)
 * mode PLAIN3: y [B, Cout, H, W] = act( d * conv3x3(x*s) + noise_w[0]*noise + bias[o] ), act = lrelu(slope)*gain
 *              when `act` != 0; noise [H*W] with noise_bstride 0 (shared) or H*W (per sample); noise/noise_w/bias
 *              may be NULL.
 * mode UP3:    y [B, Cout, 4, H+1, W+1] = d * conv_transpose2d(x*s, stride 2) split by output parity:
 *              plane ph = 2*(oy&1) + (ox&1) holds T[oy, ox] at [oy>>1, ox>>1]; entries of the odd planes that fall
 *              outside the (2H+1)x(2W+1) result are written as exact zeros.  noise/bias/act are NOT applied
 *              (sgdfr_blur_bias_act_f32 does that after the FIR).
 * mode DOWN3:  x is [B, Cin, 4, H+1, W+1] parity planes (x_bstride = Cin*4*(H+1)*(W+1)), y [B, Cout, H, W]:
 *              y[b,n,a,c] = d[b,n] * sum_{i,ky,kx} s[b,i] * T_i[2a+ky, 2c+kx] * wp[i][ky*3+kx][n]  (+ bias, act like PLAIN3;
 *              noise must be NULL).  With wp = transposed pack it is dL/dx of mode UP3. */
int sgdfr_modconv2d_fwd_f32(const float* x, int64_t x_bstride, const float* wp, const float* s, const float* d,
                            const float* noise, int64_t noise_bstride, const float* noise_w, const float* bias,
                            float* y, int B, int Cin, int Cout, int H, int W, int mode, int act, float slope,
                            float gain, void* stream);

/* K-sliced form of sgdfr_modconv2d_fwd_f32 (modes PLAIN3 / UP3) for launches too small to fill the chip (single-frame
 * reenactment, 4x4 / 8x8 layers): `splits` replicas of the tile grid each reduce a slice of the input channels into
 * partials [splits][elements of y]; a second launch adds them in a fixed order (deterministic) and applies the epilogue.
 * sgdfr_modconv2d_splitk_hint returns the recommended number of slices (1 = use the plain entry point). */
int sgdfr_modconv2d_splitk_hint(int B, int Cin, int Cout, int H, int W, int mode);
int sgdfr_modconv2d_splitk_f32(const float* x, int64_t x_bstride, const float* wp, const float* s, const float* d,
                               const float* noise, int64_t noise_bstride, const float* noise_w, const float* bias, float* y,
                               float* partials, int splits, int B, int Cin, int Cout, int H, int W, int mode, int act,
                               float slope, float gain, void* stream);

/* Winograd F(2x2,3x3) form of mode PLAIN3 (same result up to fp32 rounding, 2.25x fewer MFMA ops).
 *   sgdfr_modconv_prepack_wino_f32: weight [Cout,Cin,3,3] -> u [Cin][Cout][16] = (G g G^T) / sqrt(9*Cin), the four 16-byte
 *       quads of each 16-vector stored at slot (quad ^ (cout & 3)) (LDS bank swizzle, opaque to callers);
 *       transpose_flip != 0 packs the ADJOINT conv instead: u [Cout][Cin][16] of the 180-degree rotated, transposed kernel
 *   sgdfr_modconv2d_wino_supported: 1 when the shape can use it (Cin % 8 == 0, Cout % 64 == 0, H and W even)
 *   sgdfr_modconv2d_wino_f32: arguments as sgdfr_modconv2d_fwd_f32(mode PLAIN3) with u in place of wp, plus `zeros`:
 *       a device buffer of >= 16 zero bytes (the global->LDS DMA reads padding positions from it) */
int sgdfr_modconv_prepack_wino_f32(const float* weight, float* u, int Cout, int Cin, int transpose_flip, void* stream);
int sgdfr_modconv2d_wino_supported(int B, int Cin, int Cout, int H, int W);
int sgdfr_modconv2d_wino_f32(const float* x, int64_t x_bstride, const float* u, const float* s, const float* d,
                             const float* noise, int64_t noise_bstride, const float* noise_w, const float* bias,
                             const float* zeros, float* y, int B, int Cin, int Cout, int H, int W, int act, float slope,
                             float gain, void* stream);

/* t [B*C, 4, H+1, W+1] (phase planes from MODE_UP3) -> y [B, C, 2H, 2W]:
 *   y = act( upfirdn2d(T, fir[4,4], pad=(1,1)) + noise_w[0]*noise[oy,ox] + bias[c] )   (model.py:257,287, fused_act.py:81)
 * y_absmax (optional, [B*C] words ZEROED by the caller): fp32 bit pattern of max |y| per (image, channel) plane from the same pass --
 * the range plan of the fp16-split conv that reads y (sgdfr_split_range_f32 with x_absmax_bstride = C), instead of a separate
 * sgdfr_absmax_f32 pass over y (autograd forward). */
int sgdfr_blur_bias_act_f32(const float* t, const float* fir, const float* noise, int64_t noise_bstride,
                            const float* noise_w, const float* bias, float* y, int B, int C, int H, int W, int act,
                            float slope, float gain, unsigned int* y_absmax, void* stream);

/* sgdfr_blur_bias_act_f32 with the result multiplied by the NEXT layer's modulation s_next [B,C] and written in that layer's
 * split input form xs [B][C/8][2][2H*2W][8] (see sgdfr_to_split_f32) instead of fp32 NCHW.  plane_stride: 0 = t is the dense
 * planar [B*C][4][(H+1)*(W+1)]; otherwise t is the interleaved [B*C][plane_stride][px][py] form of sgdfr_modconv2d_split_f32
 * (16-byte aligned).  wino = 2 | 4 (W = 8 ... 64; wino = 4 on interleaved planes also W = 128): xs receives the
 * Winograd input form [B][C/8][wino+2][2][2H*2W/wino][8] of sgdfr_to_wsplit_f32(f = wino) instead (2x / 1.5x the bytes), for
 * sgdfr_modconv2d_wsplit_f32. */
int sgdfr_blur_bias_act_split_f32(const float* t, const float* fir, const float* noise, int64_t noise_bstride,
                                  const float* noise_w, const float* bias, const float* s_next, unsigned short* xs, int B, int C,
                                  int H, int W, int64_t plane_stride, int arith, int wino, int act, float slope, float gain,
                                  unsigned int* sat, void* stream);

/* y[b,j,p] = sum_i w_rgb[j*Cin+i]/sqrt(Cin) * s[b,i] * x[b,i,p] + bias[j]
 *          + (skip ? upfirdn2d(skip[b,j] (H/2 x W/2), fir[4,4], up=2, pad=(2,1))[p] : 0),  j<3 */
int sgdfr_torgb_fwd_f32(const float* x, const float* w_rgb, const float* s, const float* bias, const float* skip,
                        const float* fir, float* y, int B, int Cin, int H, int W, void* stream);

/* Split-operand arithmetic of the 3x3 modulated convs (same contract as sgdfr_modconv2d_fwd_f32 modes PLAIN3 / UP3,
 * ModulatedConv2d.forward model.py:232-273): fp32 operands are split into two 16-bit terms hi + lo and contracted as
 * hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_{f16,bf16} with fp32 accumulation.  `arith` selects the terms:
 *   SGDFR_SPLIT_FP16  fp16 hi+lo = 22 operand bits (fp32-grade; 7.7e-6 max-abs vs an fp64 evaluation of the 256x256 generator).
 *                     THE DEFAULT of the Python host layer (functional.PRECISION = 'fp16x3') for inference and the autograd
 *                     forward.  fp16 has 5 exponent bits: the host supplies styles / demodulation scaled by an exact power of
 *                     two per image (the "range plan", sgdfr_styles_batched_f32 / sgdfr_split_range_f32) so the largest operand
 *                     sits a few binades under 65504.  Operands that still leave the range, or are NaN/Inf, are CLAMPED AND
 *                     COUNTED in the caller's saturation word (below) -- never silently.
 *   SGDFR_SPLIT_BF16  bf16 hi+lo = 16 operand bits, full fp32 exponent range (~1.2e-4 on the same images; contract 1e-3).
 *                     Selected AUTOMATICALLY by the host layer as the fallback of a generator whose saturation word became
 *                     non-zero (the affected batch is re-rendered before it is returned by the verified entry points:
 *                     generate_image, ReenactmentSession, Generator.forward(verify_range=True)), or explicitly.
 * A caller pins an arithmetic with functional.set_precision('fp32' | 'fp16x3' | 'bf16x3') / SGDFR_PRECISION, or per call through
 * the `arith` argument here ('fp32' = the sgdfr_modconv2d_fwd_f32 / _wino_f32 kernels, no split entry point involved).
 *
 * Saturation words: every entry point that converts to the fp16 terms takes `unsigned int* sat`: a device word the kernel
 * atomically adds its count of clamped / non-finite operand pairs to (one word per generator, or per batch in flight: the
 * owner zeroes and reads it; nothing is shared between generators or streams).  NULL = the legacy device-wide counter read
 * by sgdfr_split_saturation_count().
 *   sgdfr_modconv_prepack_split_elems: uint16 elements of the packed weight buffer (= 2*9*Cin*Cout, Cout rounded up to the 64-wide cout tiles of the pack:
 *     a forward pack may have Cout = 32 mod 64, its last tile is half padding)
 *   sgdfr_modconv_prepack_split_f32:   weight [Cout,Cin,3,3] -> 16-bit hi/lo of weight/sqrt(9 Cin) in kernel order;
 *                                      transpose_flip = 1 packs the adjoint conv (Cin outputs, Cout inputs, taps rotated),
 *                                      2 the adjoint of the transposed conv (channels swapped, taps stored phase by phase):
 *                                      dL/dx of the plain conv is then the same PLAIN3 kernel
 *   sgdfr_modconv2d_split_supported:   1 when the shape can use it.  Every mode: Cin % 16 == 0 and a tileable H x W.
 *                                      PLAIN3, UP3: Cout % 64 == 0, or Cout % 64 == 32 (forward packs: the last cout tile is
 *                                      half padding).  DOWN3: Cout % 128 == 0.  Tileable -- PLAIN3, W <= 64: 256 (Cout % 128
 *                                      == 0) or 512 pixels are whole rows of whole images (PT % W == 0 and H W % PT == 0) or
 *                                      whole images (PT % (H W) == 0); W > 64: W % 64 == 0 and H % (PT / 64) == 0.  UP3, DOWN3:
 *                                      any H; the staged range of PT + W + 3 positions and the style table must fit the LDS,
 *                                      which ends UP3 at W = 701 and DOWN3 at W = 381.  A pre-split input
 *                                      (..._split_xin_supported) needs more: PLAIN3 every supported shape; UP3 Cout % 128 != 0
 *                                      or the deep plan (B (H+1) (W+1) (Cout / 64) >= 65536), and room for a third weight slot
 *                                      on the row-stage plan (W <= 637 at Cin = 16, 573 at Cin = 512); DOWN3 as above.  tests/test_cpu_split_edges.py pins each of these from both sides.
 *   sgdfr_modconv2d_split_f32:         arguments as sgdfr_modconv2d_wino_f32 with wsp in place of u, plus mode:
 *                                      PLAIN3, or UP3 = stride-2 transposed conv into parity planes
 *                                      [B,Cout,4,H+1,W+1] exactly as sgdfr_modconv2d_fwd_f32(mode UP3) writes them;
 *                                      ksplit > 1 (see ..._ksplit_hint; layers too small to fill the chip) slices the
 *                                      channel blocks over extra thread blocks into `partials` [ksplit][numel(y)] and
 *                                      reduces them in fixed order (deterministic).
 *                                      rgb_part != NULL (PLAIN3, ksplit == 1) also fuses the 1x1 ToRGB conv that follows
 *                                      the layer (ToRGB.forward model.py:350-359): rgb_w [3][Cout], rgb_s [B][Cout] (its
 *                                      modulation), rgb_part [B][T*3][H*W] with T = ..._split_cout_tiles(); channel t*3+j
 *                                      holds the sum over cout tile t, so sgdfr_torgb_fwd_f32 over those T*3 channels with
 *                                      indicator weights finishes it (+ bias + upsampled skip) without re-reading x;
 *                                      with rgb_part, y may be NULL: the activation is then not stored at all (last layer of
 *                                      the generator: only its ToRGB consumes it) */
#define SGDFR_SPLIT_BF16 0   /* bf16 hi+lo: 16 mantissa bits, fp32 range   (~1e-4 on the 256x256 generator) */
#define SGDFR_SPLIT_FP16 1   /* fp16 hi+lo: 22 mantissa bits = fp32-grade; operands range-shifted by exact powers of two,
                                |x*s| saturates at 1.04e6 */
#define SGDFR_SPLIT_FP16F8 2 /* fp16 main term + fp8 (e4m3) cross terms: the "lo" chunk of eight channels holds (8 x fp8 | 8 x fp8)
                                instead of 8 x fp16, both cross terms of 32 K-elements are one v_mfma_scale_f32_32x32x64_f8f6f4:
                                2 MFMA units per product instead of 3, ~1e-5 of max|y| per layer (5e-5 in F(4,3) form).  Taken by
                                the F(4,3) wide-tile conv (sgdfr_modconv2d_wsplit_f32, f = 4), the transposed conv's deep plan and
                                the 4-wave plain plan (sgdfr_modconv2d_split_f8_ok), their packs and the producers of their inputs */
int64_t sgdfr_modconv_prepack_split_elems(int Cout, int Cin);
int sgdfr_modconv_prepack_split_f32(const float* weight, unsigned short* wsp, int Cout, int Cin, int arith, int transpose_flip,
                                    unsigned int* sat, void* stream);
int sgdfr_modconv2d_split_supported(int B, int Cin, int Cout, int H, int W, int mode);
int sgdfr_modconv2d_split_f8_ok(int B, int Cin, int Cout, int H, int W, int mode);      /* arith = SGDFR_SPLIT_FP16F8 allowed (UP3 deep plan, x_is_split = 1, forward pack of the same arith) */
int sgdfr_modconv2d_split_f32(const float* x, int64_t x_bstride, const unsigned short* wsp, const float* s, const float* d,
                              const float* noise, int64_t noise_bstride, const float* noise_w, const float* bias,
                              const float* zeros, float* y, float* partials, int ksplit, const float* rgb_w,
                              const float* rgb_s, float* rgb_part, int x_is_split, unsigned short* xs_out, const float* s_next,
                              int B, int Cin, int Cout, int H, int W, int mode, int64_t plane_stride, int arith, int act,
                              float slope, float gain, unsigned int* sat, void* stream);
/* plane_stride (UP3, ksplit <= 1; 0 = dense planar planes y [B][Cout][4][(H+1)*(W+1)]): positions per (image, cout) of the
 * INTERLEAVED form y [B][Cout][plane_stride][px][py] -- the four parity phases of a super-pixel are one 16-byte quad (element
 * 2*px + py), >= (H+1)*(W+1) positions, the same bytes in total.  A multiple of 32 positions keeps every store run of the kernel
 * on whole 128-byte lines (dense planes are odd-sized: their stores run at half the write bandwidth), a lane stores one quad
 * instead of four dwords, and sgdfr_blur_bias_act_split_f32 (same stride) fetches a super-pixel with one 16-byte load. */
/* x [B,Cin,H,W], s [B,Cin] -> xs [B][Cin/8][2][H*W][8] 16-bit: x*s already split (and range-shifted) the way the kernel
 * stages it; sgdfr_modconv2d_split_f32(x = xs, s = NULL, x_is_split = 1) then fills LDS by DMA only.  Producers can emit
 * that form directly: sgdfr_modconv2d_split_f32(xs_out, s_next = the NEXT layer's modulation [B,Cout]) (y may then be NULL)
 * and sgdfr_blur_bias_act_f32's split variant, so activations between layers never exist as fp32 in HBM. */
/* fp16-split operand pairs clamped to +-65504 by split launches that were given sat = NULL, on the current device since the
 * last reset (launches with their own saturation word do not count here).  Synchronises the device; < 0 on a HIP error. */
long long sgdfr_split_saturation_count(int reset);
int sgdfr_modconv2d_split_xin_supported(int B, int Cin, int Cout, int H, int W, int mode);   /* x_is_split allowed for this shape */
int sgdfr_to_split_f32(const float* x, const float* s, unsigned short* xs, int B, int Cin, int H, int W, int arith,
                       unsigned int* sat, void* stream);
/* Backward of the transposed conv on the split kernels (autograd of ModulatedConv2d.forward model.py:246-256; consumers
 * trainer.py:188, optimization.py:67): dL/d(x*s) = the stride-2 3x3 conv of the gradient's parity planes with the transposed
 * kernel = sgdfr_modconv2d_split_f32(mode = SGDFR_MODE_DOWN3, x_is_split = 1, Cin = plane channels C, Cout = channels of
 * dL/dx, H x W = size of x, weights packed with transpose_flip = 2).  Its input is written by
 *   sgdfr_planes_to_split_f32: gt [B,C,4,H+1,W+1] fp32 (gradient of the parity planes), d [B,C] or NULL (the per-plane
 *                              scale: the layer's demodulation) -> xs [B][(ph*C + c)/8][2][(H+1)*(W+1)][8] 16-bit, the
 *                              phase-major split form of gt*d (16-byte aligned, 4 bytes per element). */
int sgdfr_planes_to_split_f32(const float* gt, const float* d, unsigned short* xs, int B, int C, int H, int W, int arith,
                              unsigned int* sat, void* stream);
/* sgdfr_blur_adjoint_f32 followed by sgdfr_planes_to_split_f32 in one pass (frozen generator: nothing else reads the fp32
 * plane gradient): g [B,C,2H,2W] -> xs as above (times d [B,C] or 1), asum[b,c] = sum gT*t when the forward planes
 * t [B,C,4,H+1,W+1] are given (the demodulation gradient; asum is zeroed first). */
int sgdfr_blur_adjoint_split_f32(const float* g, const float* fir, const float* t, const float* d, unsigned short* xs,
                                 float* asum, int B, int C, int H, int W, int arith, unsigned int* sat, void* stream);
int sgdfr_modconv2d_split_cout_tiles(int B, int Cin, int Cout, int H, int W, int mode);
/* the cout tiling of a launch with x_is_split = 1 and ksplit <= 1 (its tiling plan may differ: T of rgb_part [B][T*3][H*W]) */
int sgdfr_modconv2d_split_cout_tiles_xin(int B, int Cin, int Cout, int H, int W, int mode);
int sgdfr_modconv2d_split_ksplit_hint(int B, int Cin, int Cout, int H, int W, int mode);
/* Host-only, for tests: the tiling plan of a launch (xin_whole = 1: x_is_split = 1 and ksplit <= 1) as
 * cfg | NEX << 4 | simgs << 8 | half cout tile << 20 (cfg: the plan index of csrc/split.hip, NEX: staging slots per thread,
 * simgs: images a pixel tile may touch), or -1 when the shape is not supported. */
int sgdfr_modconv2d_split_plan_info(int B, int Cin, int Cout, int H, int W, int mode, int xin_whole);

/* ---- The plain 3x3 modulated conv in 1-D Winograd form on the split-operand matrix cores (csrc/wsplit.hip; replaces the same
 * reference lines as sgdfr_modconv2d_split_f32 mode PLAIN3: ModulatedConv2d.forward model.py:232-273 + NoiseInjection
 * model.py:284-293 + FusedLeakyReLU op/fused_act.py:79-86).  Along image rows f neighbouring outputs come from f+2 transformed
 * inputs, kernel rows stay direct: F(2,3) (f = 2: 4 multiplies instead of 6, 2/3 of the MFMA work) or F(4,3) (f = 4: 6 instead of
 * 12, 1/2; interpolation points 0, +-1, +-2, inf).  The transforms are applied to fp32 values before the hi/lo split, so the
 * products keep the arithmetic of `arith` (same SGDFR_SPLIT_* constants, same saturation rule); |V| <= 2 max|x*s| (f = 2) /
 * 10 max|x*s| (f = 4): plan 1 / 4 more binades of headroom.
 *   sgdfr_to_wsplit_f32:               x [B,Cin,H,W], s [B,Cin] -> vs "WS" [B][Cin/8][t f+2][hi,lo][H*W/f][8] 16-bit: V = B^T (x*s)
 *                                      per tile of f outputs, d_j = (x*s)[f*tile-1+j] (zero outside the row); f = 2: V0 = d0-d2,
 *                                      V1 = d1+d2, V2 = d2-d1, V3 = d1-d3.  Producers may emit it directly
 *                                      (sgdfr_blur_bias_act_split_f32 with wino = f).
 *   sgdfr_modconv_prepack_wsplit_f32:  weight [Cout,Cin,3,3] -> U = G (weight/sqrt(9 Cin)) per kernel row, 16-bit hi/lo in
 *                                      kernel order, sgdfr_modconv_prepack_wsplit_elems() uint16 elements (= 2*3*(f+2)*Cin*Cout + an 8-element trailer).
 *   sgdfr_modconv2d_wsplit_supported:  Cin % 16 == 0, Cout % 128 == 0, W/f a multiple of the patch width (f = 2: min(16, W/2)
 *                                      >= 8 tiles; f = 4: min(8, W/4) >= 4), H a multiple of the patch height (256 / (f * width)).
 *   sgdfr_modconv2d_wsplit_f32:        outputs as sgdfr_modconv2d_split_f32 (PLAIN3, ksplit = 1, x_is_split = 1): y (may be
 *                                      NULL when xs_out or rgb_part is given), the next conv's split input xs_out (+ s_next),
 *                                      ToRGB partial sums rgb_part [B][(Cout/128)*3][H*W] (+ rgb_w, rgb_s).
 * arith = SGDFR_SPLIT_FP16F8 (f = 4 only, in all three calls and in sgdfr_blur_bias_act_split_f32 with wino = 4; the direct kernels'
 * side of it -- sgdfr_to_split_f32, sgdfr_modconv_prepack_split_f32, sgdfr_modconv2d_split_f32 where sgdfr_modconv2d_split_f8_ok(),
 * sgdfr_blur_bias_act_split_f32 with wino = 0 -- uses the same chunk format): the fp16 main
 * term plus BOTH cross terms in fp8 -- the 16-byte lo chunk of eight channels holds two 8-byte halves (channels 0-3, 4-7) of
 * (4 x e4m3 lo * 2^7 | 4 x e4m3 hi * 2^-4) for activations and (4 x e4m3 hi * 2^-EW | 4 x e4m3 lo * 2^(11-EW)) for weights; the
 * pack's 16-byte trailer keeps max |w * scale|, from which the kernels derive EW.  Same buffer sizes and shapes as the fp16 forms.
 * The conv then runs on the wide-tile kernel only (csrc/wswide.hip: Cin % 32 == 0, Cin >= 64, W % 32 == 0, H % 16 == 0, d and
 * bias given) and fails otherwise; sgdfr_modconv2d_wsplit_wide() = 1 for the shapes whose F(4,3) launch takes that kernel by its
 * tile count anyway (what a host asks before choosing the arithmetic for a layer).  ~5e-5 of max|y| per layer (fp16x3: 4e-6),
 * 1.3-1.5x the speed of the three-product form (scripts/f8_layer_probe.py). */
int sgdfr_modconv2d_wsplit_supported(int B, int Cin, int Cout, int H, int W, int f);
int sgdfr_modconv2d_wsplit_wide(int B, int Cin, int Cout, int H, int W);
/* OR-ed into `arith` of sgdfr_modconv2d_wsplit_f32 (f = 4, either tile size, xs_out given): the hand-over's lo chunks leave as the fp8
 * cross-term operands of SGDFR_SPLIT_FP16F8 -- for a next conv launched with that arithmetic (sgdfr_modconv2d_split_f32, mode UP3,
 * where sgdfr_modconv2d_split_f8_ok() = 1: the transposed conv's deep plan, nine taps pair up per phase with (1,1) beside zeros;
 * mode PLAIN3 where it says so: the 4-wave plan of short-K layers, fed by sgdfr_blur_bias_act_split_f32(arith = FP16F8, wino = 0)). */
#define SGDFR_SPLIT_HANDOVER_F8 0x100
int64_t sgdfr_modconv_prepack_wsplit_elems(int Cout, int Cin, int f);
int sgdfr_modconv_prepack_wsplit_f32(const float* weight, unsigned short* wsp, int Cout, int Cin, int f, int arith,
                                     unsigned int* sat, void* stream);
int sgdfr_to_wsplit_f32(const float* x, const float* s, unsigned short* vs, int B, int Cin, int H, int W, int f, int arith,
                        unsigned int* sat, void* stream);
int sgdfr_modconv2d_wsplit_f32(const unsigned short* v, const unsigned short* wsp, const float* d, const float* noise,
                               int64_t noise_bstride, const float* noise_w, const float* bias, const float* zeros, float* y,
                               const float* rgb_w, const float* rgb_s, float* rgb_part, unsigned short* xs_out,
                               const float* s_next, int B, int Cin, int Cout, int H, int W, int f, int arith, int act,
                               float slope, float gain, unsigned int* sat, void* stream);

/* The rest of ToRGB.forward (model.py:350-359) when its 1x1 conv was accumulated by sgdfr_modconv2d_split_f32(rgb_part):
 *   y[b,j,p] = sum_{t<T} part[b, t*3+j, p] + bias[j] + (skip ? upfirdn2d(skip[b,j], fir[4,4], up=2, pad=(2,1))[p] : 0) */
int sgdfr_torgb_finish_f32(const float* part, int T, const float* bias, const float* skip, const float* fir, float* y, int B,
                           int H, int W, void* stream);

/* sgdfr_torgb_finish_f32 whose result leaves as uint8 HWC instead of fp32 planes -- the output side of the path fused into the
 * last ToRGB (scaling of libs/utilities/image_utils.py:87-110, identical to sgdfr_image_to_u8_f32 applied to
 * the fp32 result):  y[b][oy][x_offset + ox][c] = u8(rgb[b, swap_rb ? 2-c : c, oy, ox]),  row_pitch bytes per row, so the
 * frame can be written as one panel of a wider grid (x_offset, row_pitch multiples of 4). */
int sgdfr_torgb_finish_u8_f32(const float* part, int T, const float* bias, const float* skip, const float* fir,
                              unsigned char* y, int64_t row_pitch, int x_offset, int swap_rb, int B, int H, int W,
                              void* stream);

/* x [B,3,H,W] fp32 -> y [B,H,W,3] uint8:  trunc( (clamp(x,-1,1) + 1) / (2 + 1e-5) * 255 )
 * (libs/utilities/image_utils.py:87-110 tensor_to_image / torch_range_1_to_255, then the writers' uint8 cast) */
int sgdfr_image_to_u8_f32(const float* x, unsigned char* y, int B, int H, int W, void* stream);

/* K panels [B,3,H,W] fp32 side by side -> y [B,H,K*W,3] uint8 video frames, same scaling as above.
 * `panels` / `bstrides` are HOST arrays of K device pointers / batch strides in floats (0 = the same image in
 * every frame, e.g. the source; a NULL panel is skipped -- its columns keep what sgdfr_torgb_finish_u8_f32 wrote).
 * Batched generate_grid_image + tensor_to_image + np.uint8
 * (libs/utilities/utils_inference.py:11-33, run_inference.py:188-194); swap_rb != 0 also applies that path's
 * cv2.cvtColor(.., COLOR_BGR2RGB) channel swap. */
#define SGDFR_MAX_GRID_PANELS 4
int sgdfr_grid_to_u8_f32(const float* const* panels, const int64_t* bstrides, int K, unsigned char* y, int B, int H,
                         int W, int swap_rb, void* stream);

/* ---- shift-vector construction (the DirectionMatrix input), SURVEY.md §8f-2 ---------------------------------------- */

/* One learned direction: which 3DMM parameter feeds it and how it is placed on the shift axis.
 *   SGDFR_DIR_ANGLE: position = angle[col] * a / b      (a = shift_scale, b = angle_scales[col]; col 0 yaw, 1 pitch, 2 roll)
 *   SGDFR_DIR_JAW:   position = a * pose[col] + b       (col = 3 in the reference, params['pose'][:, 3])
 *   SGDFR_DIR_EXP:   position = a * alpha_exp[col] + b  (a, b from the line through (min,-shift_scale), (max,+shift_scale),
 *                                                        libs/utilities/generic.py:84-104)
 *   SGDFR_DIR_ZERO:  the direction is not driven (its entry stays 0) */
#define SGDFR_DIR_ZERO 0
#define SGDFR_DIR_ANGLE 1
#define SGDFR_DIR_JAW 2
#define SGDFR_DIR_EXP 3
#define SGDFR_MAX_DIRECTIONS 64
struct sgdfr_direction {
    int kind;
    int col;
    double a;
    double b;
};

/* shift[n,k] = position_k(target n) - position_k(source n) for N frames in one launch: the batched, sync-free counterpart of
 * run_inference.py:201-254 Inference.make_shift (arith 0: float32 angle scaling, float64 divide / a*x+b / difference, one
 * final rounding -- the numpy scalar arithmetic of that function) and of libs/utilities/utils_train.py:127-175
 * make_shift_vector (arith 1: every operation rounded to float32 as torch does on float32 tensors; division is a true
 * division as in torch's CPU kernel -- the CUDA kernel multiplies by a rounded reciprocal, 1 ulp apart).
 * Source arrays have batch strides in floats (0 = one source identity for all frames, the run_inference case); target
 * arrays are contiguous [N,3], [N,pose_dim], [N,exp_dim].  `table` is a HOST array of D entries (passed by value to the
 * kernel). */
int sgdfr_make_shift_f32(const float* ang_s, int64_t ang_s_bstride, const float* pose_s, int64_t pose_s_bstride,
                         const float* exp_s, int64_t exp_s_bstride, const float* ang_t, const float* pose_t,
                         const float* exp_t, int pose_dim, int exp_dim, const struct sgdfr_direction* table, int D,
                         float* shift, int N, int arith, void* stream);

/* Second half of make_shift_vector_50 (libs/utilities/utils_train.py:227-286): sample n moves along ONE direction which[n]
 * (device int32 [N]) by (lo - hi) * u[n] + hi with lo/hi = -/+shift_scale - position(source n), float32 arithmetic; every
 * other entry of its row is 0.  which / u are drawn by the caller (np.random.choice / torch.rand in the reference). */
int sgdfr_make_shift_random_f32(const float* ang_s, const float* pose_s, const float* exp_s, int pose_dim, int exp_dim,
                                const int* which, const float* u, float shift_scale, const struct sgdfr_direction* table,
                                int D, float* shift, int N, void* stream);

/* Ground-truth coefficients of the `disentanglement_50` training step (libs/utilities/utils_train.py:291-374
 * get_params_gt_reenacted) for the whole batch in one launch, one thread per row; B must be even.
 *   rows <  B/2: pose_gt / exp_gt = the target's pose / alpha_exp;
 *   rows >= B/2: the source's, then table[which[row - B/2]] (device int32 [B/2], the indices make_shift_vector_50 drew) moves
 *     one coefficient by shift[row, which] (shift [B,D], the vector make_shift_vector_50 returned):
 *     SGDFR_DIR_ANGLE col c: start = angle[c] * shift_scale / b, angle[c] <- (start + shift) * b / shift_scale (b = angle_scales[c]),
 *       the three angles (degrees) -> radians -> euler_to_quaternion -> quaternion_to_angle_axis (rotation_converter.py:48-90,
 *       256-303, both `where` branches), then pose[0] = aa[1], pose[1] = -aa[0], pose[2] = aa[2] (the reference's swap);
 *     SGDFR_DIR_JAW / SGDFR_DIR_EXP col c: x <- ((a * x + b + shift) - b) / a on pose[c] / alpha_exp[c];
 *     SGDFR_DIR_ZERO, or an index outside 0..D-1: the row stays the source's (the reference's ifs fall through).
 * float32 arithmetic as sgdfr_make_shift_f32's arith 1: one rounding per operation, no fma, true division.  Against the
 * reference on CPU tensors: bit-identical except the three rotated pose entries, which carry the device library's sinf /
 * cosf / atan2f.  All arrays contiguous: pose [B,pose_dim] (pose_dim >= 3), alpha_exp [B,exp_dim], angles [B,3]; the outputs
 * must not overlap the inputs. */
int sgdfr_gt_reenacted_f32(const float* pose_s, const float* exp_s, const float* ang_s, const float* pose_t, const float* exp_t,
                           int pose_dim, int exp_dim, const float* shift, const int* which, float shift_scale,
                           const struct sgdfr_direction* table, int D, float* pose_gt, float* exp_gt, int B, void* stream);

/* The loss arithmetic of the paired training step (libs/utilities/utils_train.py:435-499 calculate_losses_paired), csrc/pairloss.hip:
 * a mean absolute difference of two contiguous float32 arrays x, y of n elements, with the reference's [-1,1] -> [0,255] image
 * transform (libs/utilities/image_utils.py:87-94 torch_range_1_to_255) folded in.
 *   SGDFR_PAIRLOSS_PLAIN:    loss[0] = mean |x - y|                                   (L1Loss(shifted_latents, target_w))
 *   SGDFR_PAIRLOSS_RANGE255: loss[0] = mean |t(y) - t(x)|, t(v) = (clamp(v,-1,1) + 1) / (2 + 1e-5) * 255, one float32 rounding per
 *                            operation in that order, true division (losses.py:14-18 on the transformed images); x255 / y255, where
 *                            not NULL, receive t(x) / t(y) from the same pass (LPIPS reads them).  They must not alias x, y.
 * sgdfr_pairloss_forward_f32: one streaming launch writes per-block partial sums into `workspace` (at least
 *   sgdfr_pairloss_workspace_bytes(n) bytes; pass min(n, INT_MAX) to the query, the size no longer grows there), a second launch
 *   adds them in a fixed order and divides by n.  The grid, the element -> thread assignment and the order of every addition depend
 *   on n alone, not on the pointers' alignment: two calls on equal data give equal bits.  No atomics, no host synchronisation.
 * sgdfr_pairloss_backward_f32: one launch, dx[i] =
 *   PLAIN:    sign(x - y) * (g / n)
 *   RANGE255: m(x) * ((g255[i] + sign(t(x) - t(y)) * (g / n)) * 255 / (2 + 1e-5)), m(x) = 1 on -1 <= x <= 1 (bounds included) and
 *             exactly 0 elsewhere (torch's clamp backward), sign(0) = 0 (torch's L1Loss backward); t is recomputed.
 *   g = grad_loss[0], a DEVICE scalar (NULL: 0); g255 = grad_x255, the upstream gradient of the materialised t(x) (NULL: 0;
 *   RANGE255 only).  y gets no gradient.  dx may not alias x or y.
 * 16-byte loads and stores where every pointer of the call is 16-byte aligned, dword accesses of the same elements otherwise. */
#define SGDFR_PAIRLOSS_PLAIN 0
#define SGDFR_PAIRLOSS_RANGE255 1
int64_t sgdfr_pairloss_workspace_bytes(int n);
int sgdfr_pairloss_forward_f32(const float* x, const float* y, int64_t n, int mode, float* x255, float* y255, float* loss,
                               void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_pairloss_backward_f32(const float* x, const float* y, int64_t n, int mode, const float* grad_loss,
                                const float* grad_x255, float* dx, void* stream);

/* ---- direction sweeps (run_facial_editing.py:144-207 interpolate, libs/utilities/visualization.py:13-73), csrc/sweep.hip ---- */

/* One ladder: what libs/configs/config_directions.py:42-85 get_direction_info returns for one source along one direction, and the
 * lengths of the two loops that walk it: n_lo = len(np.arange(min_shift, start, step)), n_hi = len(np.arange(start, max_shift, step)).
 * start / min_shift / max_shift hold the reference's values exactly (float64 on angle directions, float32 widened on the others). */
struct sgdfr_sweep_record {
    double start;
    double min_shift;
    double max_shift;
    double step;
    int n_lo;
    int n_hi;
};

/* get_direction_info for N source rows x K requested directions in one launch: records[n * K + j] describes source row n along
 * direction dirs[j] (`dirs`, like `table`, is a HOST array; table as sgdfr_make_shift_f32 takes it, built the way the trainer's is:
 * per-dataset angle rows, the jaw at count_pose - 1).  angles [N,3], pose [N,pose_dim], alpha_exp [N,exp_dim] and records are
 * device arrays.  step = shift_scale / shifts_count.  The arithmetic reproduces the reference's mixed dtypes operation by operation
 * (one rounding each, no fma):
 *   SGDFR_DIR_ANGLE: start = (double)fl32(angle * fl32(shift_scale)) / b; min = -sc - start, max = (sc - start) + 1e-5 and both
 *     length quotients ceil((stop - first) / step) in float64;
 *   SGDFR_DIR_JAW / SGDFR_DIR_EXP: start = fl32(fl32(a) * x) + fl32(b) in float32; min, max and the quotients in float32 with sc, 1e-5
 *     and step rounded to float32 first (NumPy >= 2 weak scalars against a 0-d float32 array).
 * A requested direction of kind SGDFR_DIR_ZERO (absent from the dataset) is refused before the launch.
 * sgdfr_sweep_plan_host runs the same per-ladder function over HOST arrays: no GPU is touched. */
int sgdfr_sweep_plan_f32(const float* angles, const float* pose, const float* alpha_exp, int pose_dim, int exp_dim,
                         const struct sgdfr_direction* table, int D, const int* dirs, int K, double shift_scale, int shifts_count,
                         struct sgdfr_sweep_record* records, int N, void* stream);
int sgdfr_sweep_plan_host(const float* angles, const float* pose, const float* alpha_exp, int pose_dim, int exp_dim,
                          const struct sgdfr_direction* table, int D, const int* dirs, int K, double shift_scale, int shifts_count,
                          struct sgdfr_sweep_record* records, int N);

/* The ladders as DirectionMatrix input: rows [R,D] float32, row r = one_hot(D, value, dirs[j]) (libs/utilities/utils.py:62-65), every
 * other column exactly 0.  Pair p = n * K + j owns rows row_offset[p] .. row_offset[p] + n_lo + n_hi - 1 (row_offset: device int32
 * [N*K], the exclusive prefix sum of the lengths): first np.arange(min_shift, start, step) ascending, then
 * np.arange(start, max_shift, step) ascending.  value_i = first + i * delta in float64, rounded to float32 once, with
 * delta = (first + step) - first in float64 on angle directions and (double)fl32(first + fl32(step)) - first on the others.
 * row_k[r] = j (the position in dirs), is_start[r] = 1 on the first row of the second part (the row interpolate draws the red box
 * on), both device int32 [R].  A row that the offsets do not cover is left zero with row_k = -1.
 * sgdfr_sweep_rows_host does the same over HOST arrays (rows in pair order, R must equal the records' total). */
int sgdfr_sweep_rows_f32(const struct sgdfr_sweep_record* records, const int* row_offset, const struct sgdfr_direction* table, int D,
                         const int* dirs, int K, int N, float* rows, int* row_k, int* is_start, int R, void* stream);
int sgdfr_sweep_rows_host(const struct sgdfr_sweep_record* records, const struct sgdfr_direction* table, int D, const int* dirs, int K,
                          int N, float* rows, int* row_k, int* is_start, int64_t R);

/* Rendered rows -> what the editing scripts consume, in one pass: x [R,3,P*f,P*f] float32, f = 1, 2 or 4.  Outputs, each skipped when
 * NULL:
 *   pooled   [R,3,P,P] float32: the f x f mean, summed row by row and left to right, divided by f*f last
 *            (AdaptiveAvgPool2d((P,P)) for these factors);
 *   bordered [R,3,P,P] float32: pooled with add_border (libs/utilities/image_utils.py:129-137: 3 pixels, R = 1, G = B = -1) on the
 *            rows whose is_start flag (device int32 [R]) is set; needs P >= 7;
 *   frames   [R,P,panels*P,3] uint8: tensor_to_image(...).astype(uint8) of the pooled value (the arithmetic of
 *            sgdfr_image_to_u8_f32), never bordered; panels = 2 puts src [R or 1,3,P,P] (src_bstride = 3*P*P or 0) in the left
 *            panel (run_facial_editing.py:198-203).
 * 16-byte loads when P*f is a multiple of 4 and x is 16-byte aligned, dword loads of the same elements in the same order otherwise:
 * the results do not depend on the path.  No atomics, no LDS. */
int sgdfr_sweep_frames_f32(const float* x, int R, int P, int f, const int* is_start, const float* src, int64_t src_bstride,
                           float* pooled, float* bordered, unsigned char* frames, int panels, void* stream);

/* The pooled image loss of PTI above 256^2 (what libs/optimization.py:50-58 has to compare is the image generic.py:146-148 hands
 * out, AdaptiveAvgPool2d((256,256)) of the generator's): x [B,3,P*f,P*f] float32, real [B,3,P,P], f = 1, 2 or 4, 1 <= P <= 8192,
 * 1 <= B <= 4096.
 * sgdfr_pool_mse_f32: one walk over x (the walk of sgdfr_sweep_frames_f32: pooled [B,3,P,P] has its bits) that also sums
 *   (pooled - real)^2: per lane over its pixels, per block through the wave sums and LDS into partial[blockIdx.x] of the workspace,
 *   then one block adds the partials in a fixed order, in double, and writes mse[0] = sum / (3*B*P*P).  No float atomics: the same bits from call
 *   to call (the 16-byte and the dword walk group the terms differently, so the last bits of mse depend on the path; pooled does
 *   not).  workspace: sgdfr_pool_mse_workspace_bytes(B, P) bytes (-1 for sizes out of range).
 * sgdfr_pool_mse_bwd_f32: one launch, dx [B,3,P*f,P*f] = (g_pooled[b,c,Y/f,X/f] + g_mse[0] * 2 (pooled - real) / (3*B*P*P)) / f^2;
 *   g_pooled [B,3,P,P] and g_mse (a device scalar) may each be NULL (= zeros).  16-byte stores when P*f is a multiple of 4 and dx is
 *   16-byte aligned, dword stores of the same values otherwise.
 * No host synchronisation, everything on `stream`. */
int64_t sgdfr_pool_mse_workspace_bytes(int B, int P);
int sgdfr_pool_mse_f32(const float* x, const float* real, int B, int P, int f, float* pooled, float* mse, void* workspace,
                       int64_t workspace_bytes, void* stream);
int sgdfr_pool_mse_bwd_f32(const float* g_pooled, const float* pooled, const float* real, const float* g_mse, int B, int P, int f,
                           float* dx, void* stream);

/* Rendered rows -> grid video frames in one pass (the frames of a session that pools, reenact.ReenactmentSession(pool_to=...)):
 * x [B,3,P*f,P*f] float32, f = 1, 2 or 4 -> frames [B,P,(n_left+1)*P,3] uint8.  Panels 0 .. n_left-1 (n_left <= 3) are
 * `panels[k]` [B or 1,3,P,P] float32 with batch stride `bstrides[k]` (3*P*P, or 0 = the same image in every frame); both are HOST
 * arrays, as sgdfr_grid_to_u8_f32 takes them, and a NULL panel leaves its columns of `frames` as they are.  The last panel is the
 * f x f mean of x in sgdfr_sweep_frames_f32's arithmetic (summed row by row and left to right, divided by f*f last).  Every byte is
 * sgdfr_image_to_u8_f32's; swap_rb != 0 stores the channels in reverse order in every panel, as sgdfr_grid_to_u8_f32 does.  The
 * bytes equal sgdfr_sweep_frames_f32(pooled) followed by sgdfr_grid_to_u8_f32 without the float intermediate.  16-byte loads of x
 * when P*f is a multiple of 4 and x is 16-byte aligned, dword loads of the same elements otherwise; byte stores.  No atomics, no LDS.
 * This entry is an adapter: it launches sgdfr_video_frames_px's kernels with every panel described as an SGDFR_PANEL_F32 table
 * without an index, of 1 row (stride 0) or B rows; the window walk is the one under sgdfr_sweep_frames_f32 too. */
int sgdfr_video_frames_f32(const float* x, int B, int P, int f, const float* const* panels, const int64_t* bstrides, int n_left,
                           unsigned char* frames, int swap_rb, void* stream);

/* One left panel of sgdfr_video_frames_px: a table of `rows` images on the device.  kind SGDFR_PANEL_F32: float32 planar
 * [rows,3,P,P] in [-1,1], as sgdfr_video_frames_f32 takes them; SGDFR_PANEL_U8: uint8 interleaved [rows,P,P,3] RGB, the alignment
 * crop's own bytes (sgdfr_facecrop_forward_u8).  Frame b shows row index[b] of the table when `index` (device int32 [B]) is given,
 * clamped into [0, rows): a bad index shows a wrong row and never reads outside the table.  Without an index rows is B (frame b
 * shows row b) or 1 (the same image in every frame).  data NULL leaves the panel's columns of `frames` as they are. */
#define SGDFR_PANEL_F32 0
#define SGDFR_PANEL_U8 1
struct sgdfr_video_panel {
    const void* data;
    const int* index;
    int kind;
    int rows;
};

/* sgdfr_video_frames_f32 with typed, indexed left panels (`panels`: a HOST array of n_left <= 3 descriptors) and an optional x:
 * x NULL leaves the last panel of `frames` as it is (the generator's last ToRGB launch has already written it, sgdfr_torgb_finish_u8_f32)
 * and f is then ignored.  A float32 panel gives the bytes sgdfr_video_frames_f32 gives (that entry runs these kernels).  A uint8 byte u goes through the two maps its
 * float crop goes through: the crop kernel's fl32(u / 255) * 2 - 1, then sgdfr_image_to_u8_f32's trunc((v + 1) / (2 + 1e-5) * 255)
 * -- not the identity: the 1e-5 in the divisor makes every u >= 1 come out as u - 1 (0 stays 0).  The pooled panel, swap_rb, the
 * 16-byte loads of x and the dword path are sgdfr_video_frames_f32's; a lane reads the 3 * (4 / f) consecutive bytes of its pixels
 * from a uint8 panel (as dwords where they are whole aligned dwords), so a wave reads one contiguous span of a panel row.  Byte
 * stores.  No atomics, no LDS. */
int sgdfr_video_frames_px(const float* x, int B, int P, int f, const struct sgdfr_video_panel* panels, int n_left,
                          unsigned char* frames, int swap_rb, void* stream);

/* ---- backward helpers (autograd of model.py:232-359 as restated in SURVEY.md Appendix C) ------------------------ */

/* Activation gradient + per-(b,c) reductions (op/fused_act.py:19-37 and the adjoints of model.py:287, :240):
 *   g_pre = g_out * (out > 0 ? 1 : slope) * gain
 *   sums[b,c,0] = sum g_pre ; sums[b,c,1] = sum g_pre * noise ;
 *   sums[b,c,2] = sum g_pre * y (want_y != 0), y = lrelu^-1(out) - noise_w*noise - bias[c]  (= d * conv output)
 * g_absmax (optional, [B,C] words): fp32 bit pattern of max |g_pre| per (image, channel) plane, from the same pass -- the range
 * plan of the fp16-split dL/dx conv that consumes g_pre (sgdfr_split_range_f32 with x_absmax_bstride = C). */
int sgdfr_act_grad_reduce_f32(const float* g_out, const float* out, const float* noise, int64_t noise_bstride,
                              const float* noise_w, const float* bias, float* g_pre, float* sums, int B, int C, int HW,
                              float slope, float gain, int want_y, unsigned int* g_absmax, void* stream);

/* Adjoint of the FIR of sgdfr_blur_bias_act_f32 (op/upfirdn2d.py:104-121 for pad (1,1)): g [B,C,2H,2W] ->
 * gt parity planes [B,C,4,H+1,W+1]; with t (forward planes) also asum[b,c] = sum gt * t. */
int sgdfr_blur_adjoint_f32(const float* g, const float* fir, const float* t, float* gt, float* asum, int B, int C, int H,
                           int W, void* stream);

/* dx = gu * s[b,c] (dx may alias gu) ; r[b,c] = sum_q x[b,c,q] * gu[b,c,q]   (x_bstride 0 = broadcast constant) */
int sgdfr_scale_reduce_f32(const float* gu, const float* x, int64_t x_bstride, const float* s, float* dx, float* r, int B,
                           int C, int HW, void* stream);

/* ToRGB backward: dx[b,i,p] = s[b,i]/sqrt(Cin) * sum_j w_rgb[j,i] g[b,j,p] ; r[b,j,i] = sum_p x[b,i,p] g[b,j,p] */
int sgdfr_torgb_bwd_f32(const float* x, const float* g, const float* w_rgb, const float* s, float* dx, float* r, int B,
                        int Cin, int H, int W, void* stream);

/* One pass over a saved StyledConv activation `out` [B,C,HW] in the backward of the frozen generator (libs/trainer.py:177-189:
 * only A is optimised).  The gradient of `out` arrives as up to three terms,
 *     g = gu * s_next[b,c]                                             (gu [B,C,HW] = dL/d(x*s) of the conv that reads `out`)
 *       + s_rgb[b,c]/sqrt(C) * sum_j w_rgb[j,c] * g_rgb[b,j,p]         (g_rgb [B,3,HW] = gradient of the ToRGB that reads `out`)
 *       + g_add                                                        (any of the three may be NULL, not all)
 * and the pass returns, besides everything sgdfr_act_grad_reduce_f32 computes from g for the layer that PRODUCED `out`
 * (g_pre, sums [B,C,3], g_absmax [B,C]):  r_next[b,c] += sum_p out*gu  (sgdfr_scale_reduce_f32's r)  and
 * r_rgb[b,j,c] += sum_p out*g_rgb[b,j]  (sgdfr_torgb_bwd_f32's r).  zero_outputs != 0: the call zeroes sums / g_absmax / r_next /
 * r_rgb first; 0: the caller carved them out of a zeroed workspace (one memset per backward instead of four per layer). */
int sgdfr_grad_join_f32(const float* out, const float* gu, const float* s_next, const float* g_rgb, const float* w_rgb,
                        const float* s_rgb, const float* g_add, const float* noise, int64_t noise_bstride, const float* noise_w,
                        const float* bias, float* g_pre, float* sums, unsigned int* g_absmax, float* r_next, float* r_rgb, int B,
                        int C, int HW, float slope, float gain, int want_y, int zero_outputs, void* stream);

/* Backward of sgdfr_styles_batched_f32 with respect to the latent (frozen weights), all layers in two launches:
 *   ds_l = gs_l + s_l * ((-(a_l / d_l) * d_l^3) @ qt_l^T)      demodulated 3x3 conv (a = d * dL/dd: sums[:,:,2] of the activation-
 *                                                             gradient pass with a_stride 3, or the blur adjoint's asum, stride 1)
 *   ds_l = gs_l                                                a == NULL
 *   ds_l[b,i] = (sum_j rgb_r[b,j,i] * rgb_w[j,i]) / sqrt(cin)  ToRGB (rgb_r [B,3,cin] = sum_p x*g_j, rgb_w [3,cin])
 *   glat[b, latent_index_l, :] = sum_l ds_l[b,:] @ mod_w_l / sqrt(D);  latent rows no layer reads are written as zeros. */
typedef struct sgdfr_style_grad_layer {
    const float* gs;    /* [B, cin] or NULL (rgb_r given) */
    const float* rgb_r; /* [B, 3, cin] or NULL */
    const float* rgb_w; /* [3, cin] */
    const float* a;     /* [B, cout] with element stride a_stride, or NULL */
    const float* d;     /* [B, cout] */
    const float* s;     /* [B, cin] */
    const float* qt;    /* [cin, cout] */
    const float* mod_w; /* [cin, D] */
    float* ds;          /* [B, cin] out */
    float* gmod_w;      /* [cin, D] out or NULL: dL/d(modulation weight) = ds^T @ latent[:, latent_index] / sqrt(D)  (model.py:148-157) */
    float* gmod_b;      /* [cin] out or NULL:    dL/d(modulation bias)   = sum_b ds */
    int64_t a_stride;
    int cin, cout, latent_index;
} sgdfr_style_grad_layer;
/* latent [B,L,D]: needed (non-NULL) only when some layer asks for gmod_w / gmod_b (PTI trains them, libs/optimization.py:31-40);
 * glat may be NULL when only those are wanted. */
int sgdfr_styles_batched_bwd_f32(const sgdfr_style_grad_layer* layers, int n_layers, const float* latent, float* glat, int B, int L,
                                 int D, void* stream);

/* dq[o,i] = sum_b (-0.5 * (a/d) * d^3)[b,o] * s[b,i]^2 = dL/dQ of the demodulation (Q = sum_k Wc^2), the term
 * sgdfr_modconv_wgrad_finish*_f32 adds to the weight gradient; a = d * dL/dd with element stride a_stride (see above). */
int sgdfr_demod_dq_f32(const float* a, int64_t a_stride, const float* d, const float* s, float* dq, int B, int Cin, int Cout,
                       void* stream);

/* The small parameter gradients of one generator backward in ONE launch (the reference gets them from autograd's sum ops:
 * op/fused_act.py:32-37 for the bias, model.py:287 for the noise strength, model.py:350-359 for ToRGB):
 *   SGDFR_PGRAD_BIAS   out[c]     = sum_b in[b,c,0]                       in = sums [B,C,3] of the activation-gradient pass
 *   SGDFR_PGRAD_NOISE  out[0]     = sum_{b,c} in[b,c,1]
 *   SGDFR_PGRAD_RGB_W  out[j,i]   = scale * sum_b in[b,j,i] * aux[b,i]    in = r_rgb [B,3,C], aux = s [B,C], scale = 1/sqrt(C)
 *   SGDFR_PGRAD_RGB_B  out[j]    += sum_{b,p} in[b,j,p]                   in = g_rgb [B,3,HW]; out must be ZEROED by the caller */
#define SGDFR_PGRAD_BIAS 0
#define SGDFR_PGRAD_NOISE 1
#define SGDFR_PGRAD_RGB_W 2
#define SGDFR_PGRAD_RGB_B 3
#define SGDFR_MAX_PARAM_GRADS 64
typedef struct sgdfr_param_grad {
    const float* in;
    const float* aux;
    float* out;
    int kind, C, HW;
    float scale;
} sgdfr_param_grad;
int sgdfr_param_grads_f32(const sgdfr_param_grad* entries, int n, int B, void* stream);

/* One Adam step (torch.optim.Adam as libs/optimization.py:41,66-68 uses it: no weight decay, no amsgrad) over a list of parameter
 * tensors in ONE launch: p, g (gradient), m (exp_avg), v (exp_avg_sq), n elements each; step[0] = the step count t >= 1 as a float on
 * the device (the caller increments it before the call, so a captured step needs no host value):
 *   m += (g - m)(1 - beta1) ; v = v beta2 + (1 - beta2) g^2 ; p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps) */
#define SGDFR_MAX_ADAM_TENSORS 96
typedef struct sgdfr_adam_tensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
} sgdfr_adam_tensor;
int sgdfr_adam_f32(const sgdfr_adam_tensor* tensors, int n, const float* step, float lr, float beta1, float beta2, float eps, void* stream);

/* ds[b,i] = gs[b,i] + s[b,i] * sum_o (-gd[b,o] * d[b,o]^3) * qt[i,o]   (chain rule through d = rsqrt(sum s^2 q + eps)) */
int sgdfr_demod_grad_f32(const float* gd, const float* d, const float* qt, const float* s, const float* gs, float* ds,
                         int B, int Cin, int Cout, void* stream);

/* Weight gradient of the modulated conv in the packed layout (split-K fp32 MFMA, atomically accumulated):
 *   dwp[i][ky*3+kx][o] = sum_{b,p} (d*g)[b,o,shifted p] * (x*s)[b,i,p]
 * mode PLAIN3: g = activation-gradient [B,Cout,H,W];  mode UP3: g = parity planes [B,Cout,4,H+1,W+1] from
 * sgdfr_blur_adjoint_f32.  x [B,Cin,H,W] (x_bstride 0 = broadcast), dwp [Cin,9,Cout] (zeroed here). */
int sgdfr_modconv_wgrad_f32(const float* g, const float* d, const float* x, int64_t x_bstride, const float* s, float* dwp,
                            int B, int Cin, int Cout, int H, int W, int mode, void* stream);

/* dweight[o][i][k] = (dwp[i][k][o] + 2 * wp[i][k][o] * dq[o][i]) / sqrt(9*Cin):  un-pack, add the demodulation path
 * (dq = dL/dQ [Cout,Cin], NULL without demodulation) and apply the equalised-lr scale of model.py:215,236. */
int sgdfr_modconv_wgrad_finish_f32(const float* dwp, const float* wp, const float* dq, float* dweight, int Cout, int Cin,
                                   void* stream);
/* The same gradient without atomics (deterministic, and ~0.3 ms faster per layer: every layer of the 256x256 generator
 * ends up with ~9.4 M atomic adds): sgdfr_modconv_wgrad_ksplit() = number of pixel slices K of a shape (0: the shape needs
 * the direct kernel, use sgdfr_modconv_wgrad_f32); ..._parts_f32 stores slice sums to part [K][9][Cout][Cin]; ..._finish_parts_f32
 * adds the slices in fixed order and applies what sgdfr_modconv_wgrad_finish_f32 applies. */
int sgdfr_modconv_wgrad_ksplit(int B, int Cin, int Cout, int H, int W, int mode);
int sgdfr_modconv_wgrad_parts_f32(const float* g, const float* d, const float* x, int64_t x_bstride, const float* s, float* part,
                                  int B, int Cin, int Cout, int H, int W, int mode, void* stream);
int sgdfr_modconv_wgrad_finish_parts_f32(const float* part, int ksplit, const float* wp, const float* dq, float* dweight,
                                         int Cout, int Cin, void* stream);
/* sgdfr_modconv_wgrad_finish_parts_f32 with the demodulation term taken from the ORIGINAL weight tensor weight [Cout][Cin][3][3]
 * (= wp / scale transposed) instead of the packed copy: every stream of the launch is then contiguous (the packed form forces 4-byte
 * gathers at a stride of 9*Cout floats); slices are summed four-way interleaved, in fixed order (deterministic, not the bits of the
 * sequential sum).  Instead of dq the call may take what sgdfr_demod_dq_f32 takes -- a (= d * dL/dd, element stride a_stride), d [B,Cout],
 * s [B,Cin] -- and forms dq itself (same expression and order): one launch less per layer. */
int sgdfr_modconv_wgrad_finish_parts_oik_f32(const float* part, int ksplit, const float* weight, const float* dq, const float* a,
                                             int64_t a_stride, const float* d, const float* s, int B, float* dweight, int Cout, int Cin,
                                             void* stream);

/* LPIPS (AlexNet, v0.1) distance and its input gradient (libs/criteria/lpips/lpips.py:28-34, networks.py:53-63,78-85, utils.py:6-12),
 * csrc/lpips.hip.  Images x, y [rows,3,H,W] fp32 in [-1,1], H, W in 31..4096 (unsupported sizes return an error).
 * sgdfr_lpips_prepack_f32: params = host array of 17 device pointers in the order conv0 weight, conv0 bias, conv3 w, b, conv6 w, b,
 *   conv8 w, b, conv10 w, b (torchvision layout [Cout][Cin][k][k]), mean[3], std[3], lin0..lin4 ([C_t] each) -> pack of
 *   sgdfr_lpips_pack_elems() floats (forward and flipped input-gradient weights; rebuild it whenever a parameter changes).
 * sgdfr_lpips_features_f32: the five post-ReLU taps of rows_x images of x followed by rows_y images of y (y may be NULL with
 *   rows_y = 0) into feats (sgdfr_lpips_feature_elems(rows_x + rows_y) floats: tap t is [rows, C_t, h_t, w_t], taps in order).
 * sgdfr_lpips_distance_f32: loss[0] = (1/B) sum_t sum_b mean_hw sum_c lin_t[c] (n_x - n_y)^2 between images 0..B-1 of fx (rows_x
 *   rows) and images y_row0.. of fy (rows_y rows; y_bcast 1: image y_row0 for every b).
 * sgdfr_lpips_backward_f32: dx [B,3,H,W] = grad_loss[0] (device scalar) * dL/dx of that distance; the gradient of y is not formed.
 * workspace: device scratch of at least sgdfr_lpips_workspace_bytes(B, H, W) bytes (its size passed as workspace_bytes), B = the
 *   batch of x; features accept rows_x + rows_y in {B, 2B}.  Deterministic (no float atomics), no host synchronisation. */
int64_t sgdfr_lpips_pack_elems(void);
int64_t sgdfr_lpips_feature_elems(int rows, int H, int W);
int64_t sgdfr_lpips_workspace_bytes(int B, int H, int W);
int sgdfr_lpips_prepack_f32(const float* const* params, float* pack, void* stream);
int sgdfr_lpips_features_f32(const float* x, int rows_x, const float* y, int rows_y, int H, int W, const float* pack, float* feats,
                             void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_lpips_distance_f32(const float* fx, int rows_x, const float* fy, int rows_y, int y_row0, int y_bcast, int B, int H, int W,
                             const float* pack, float* loss, void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_lpips_backward_f32(const float* grad_loss, const float* fx, int rows_x, const float* fy, int rows_y, int y_row0, int y_bcast,
                             int B, int H, int W, const float* pack, float* dx, void* workspace, int64_t workspace_bytes, void* stream);

/* ArcFace identity-loss backbone, IR-SE-50 at 112x112 in eval mode (libs/criteria/id_loss.py:20-25, model_irse.py:9-48,
 * helpers.py:57-121), csrc/idloss.hip.  Images x, y [rows,3,H,W] fp32; crop 1 takes [35:223, 32:220] with PyTorch slice clamping,
 * crop 0 the whole image; then AdaptiveAvgPool2d(112).  An empty window or a side above 8192 returns an error.
 * sgdfr_idloss_prepack_f32: params = host array of 245 device pointers with every BatchNorm folded on the host:
 *   stem w0 [64,3,3,3] (BN folded), b0 [64], PReLU a0 [64];
 *   per unit (24): BN1 scale s1 [Cin], shift t1 [Cin], conv1 w1 [D,Cin,3,3], PReLU a1 [D], conv2 w2 [D,D,3,3] (BN2 folded), b2 [D],
 *     SE fc1 [D/16,D], fc2 [D,D/16], shortcut conv wsc [D,Cin] (BN folded), bsc [D] (both NULL where Cin == D);
 *   head wh [512,25088] (BN2d and BN1d folded), bh [512]
 *   -> pack of sgdfr_idloss_pack_elems() floats (forward and input-gradient weights; rebuild it whenever a parameter changes).
 * sgdfr_idloss_forward_f32: emb [rows_x + rows_y, 512] = l2-normalised embeddings of the rows of x followed by those of y (y may
 *   be NULL with rows_y = 0; rows_y <= rows_x).  The split-K plan follows rows_x, so x's results do not depend on rows_y.
 *   saved (NULL: nothing is kept) receives sgdfr_idloss_saved_elems(rows_x) floats for the backward.
 * sgdfr_idloss_backward_f32: dx [rows,3,H,W] = dL/dx for grad_emb [rows,512] = dL/de of x's embeddings, from the saved buffer of a
 *   forward with rows_x = rows, the same H, W, crop and pack.  Zero outside the crop window.
 * workspace: device scratch of at least sgdfr_idloss_workspace_bytes(rows, H, W) bytes, rows = rows_x + rows_y for the forward.
 * Deterministic (no float atomics), no host synchronisation, everything on `stream`. */
int64_t sgdfr_idloss_pack_elems(void);
int64_t sgdfr_idloss_saved_elems(int rows);
int64_t sgdfr_idloss_workspace_bytes(int rows, int H, int W);
int sgdfr_idloss_prepack_f32(const float* const* params, float* pack, void* stream);
int sgdfr_idloss_forward_f32(const float* x, int rows_x, const float* y, int rows_y, int H, int W, int crop, const float* pack,
                             float* emb, float* saved, void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_idloss_backward_f32(const float* grad_emb, const float* saved, int rows, int H, int W, int crop, const float* pack,
                              float* dx, void* workspace, int64_t workspace_bytes, void* stream);

/* FLAME decode at DECA's sizes, its backward to the 3DMM coefficients, and the shape / mouth / eye L1 terms
 * (libs/DECA/decalib/deca.py:229-239, models/FLAME.py:175-214, models/lbs.py, utils/util.py:227-237, libs/criteria/losses.py:20-62),
 * csrc/flame.hip.  Sizes are fixed: 5023 vertices, 150 shape + expression components, 36 pose-corrective components, 5 joints with
 * parents [-1,0,1,1,1] and zero neck / eye poses, 68 + 68 landmarks, 79 dynamic contour rows.
 * sgdfr_flame_prepack_f32: params = host array of 15 device pointers: v_template [5023*3], shapedirs [5023*3][150], posedirs
 *   [36][5023*3], lbs_weights [5023][5], the joint regressor folded on the host, J_template [5*3] and Jdirs [5*3][150]
 *   (J = J_template + Jdirs . betas), the corner vertices (int32) and barycentric weights of the static [51][3], full [68][3] and
 *   dynamic [79][17][3] landmarks, and the inverse landmark index: offsets [5024] (int32), slots [n_csr] (int32: 0..50 static,
 *   51..118 full, 119 + 17 * row + j dynamic) and weights [n_csr] -> pack of sgdfr_flame_pack_elems() floats.  The size arguments
 *   are checked against the sizes above (n_csr = 4386).
 * sgdfr_flame_decode_f32: rows coefficient sets (shape [rows,100], exp [rows,50], pose [rows,6]) followed by rows_b sets of a second
 *   group (may be NULL with rows_b = 0), R = rows + rows_b.  project 1: cam [R,3] -> landmarks2d [R,68,2], landmarks3d [R,68,3],
 *   trans_verts [R,5023,3] in pixels of a 224-pixel image; project 0: the FLAME.forward triple, landmarks2d [R,68,3], landmarks3d
 *   [R,68,3], trans_verts and cam unused.  saved receives sgdfr_flame_saved_elems(R) floats: per row 256 floats of pose state (the
 *   dynamic contour row as int32 at index 201), v_posed [5023*3] and the un-projected vertices [5023*3]; a row range of it serves the
 *   backward of that range.
 * sgdfr_flame_decode_backward_f32: dshape [rows,100], dexp [rows,50], dpose [rows,6], dcam [rows,3] (may be NULL) for cotangents of
 *   the three outputs (each may be NULL = zero), times gscale[0] when gscale (device scalar) is given; the dynamic row is a constant.
 * sgdfr_shape_loss_f32: landmarks2d [2*rows,68,2] and trans_verts [2*rows,5023,3] hold the ground-truth rows followed by the
 *   reenacted rows.  loss[0] = total; terms[0..2] = lambda-weighted shape / mouth / eye terms, terms[3..5] the plain terms (8 floats);
 *   g_landmarks2d [rows,68,2] and g_trans_verts [rows,5023,3] receive the cotangents of the total for the reenacted rows.
 * workspace: device scratch of at least sgdfr_flame_workspace_bytes(rows) bytes.  Deterministic (no float atomics), no host
 * synchronisation, everything on `stream`: 3 launches per decode, 2 per loss, 2 per backward. */
int64_t sgdfr_flame_pack_elems(void);
int64_t sgdfr_flame_saved_elems(int rows);
int64_t sgdfr_flame_workspace_bytes(int rows);
int sgdfr_flame_prepack_f32(const void* const* params, int n_vertices, int n_betas, int n_pose_feature, int n_joints, int n_dynamic_rows,
                            int n_csr, float* pack, void* stream);
int sgdfr_flame_decode_f32(const float* shape, const float* exp, const float* pose, int rows, const float* shape_b, const float* exp_b,
                           const float* pose_b, int rows_b, const float* cam, const float* pack, int project, float* landmarks2d,
                           float* landmarks3d, float* trans_verts, float* saved, void* stream);
int sgdfr_flame_decode_backward_f32(const float* g_landmarks2d, const float* g_landmarks3d, const float* g_trans_verts,
                                    const float* gscale, int rows, const float* pack, int project, const float* saved, float* dshape,
                                    float* dexp, float* dpose, float* dcam, void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_shape_loss_f32(const float* landmarks2d, const float* trans_verts, int rows, float lambda_shape, float lambda_mouth,
                         float lambda_eye, float* loss, float* terms, float* g_landmarks2d, float* g_trans_verts, void* workspace,
                         int64_t workspace_bytes, void* stream);

/* DECA's coefficient encoder in eval mode (libs/DECA/decalib/models/encoders.py ResnetEncoder(outsize=236), models/resnet.py:21-118,
 * datasets/datasets.py:57-82, libs/utilities/image_utils.py:87-94, utils/rotation_converter.py:312-360), csrc/deca.hip.
 * Images x [rows,3,H,W] fp32 in [-1,1] (values beyond are clamped); mat [rows,2,3] maps an output pixel (u, v, 1) of the 224x224 crop
 * to a source pixel (x, y), sampled bilinearly with zero padding.
 * sgdfr_deca_prepack_f32: params = host array of 134 device pointers with every BatchNorm folded on the host:
 *   stem w0 [64,3,7,7], b0 [64]; per bottleneck (16): w1 [P,Cin], b1 [P], w2 [P,P,3,3], b2 [P], w3 [4P,P], b3 [4P], projection
 *   wd [4P,Cin], bd [4P] (both NULL where the shortcut is the identity); regressor fc1 [1024,2048], [1024], fc2 [236,1024], [236]
 *   -> pack of sgdfr_deca_pack_elems() floats (forward and input-gradient weights; rebuild it whenever a parameter changes).
 * sgdfr_deca_forward_f32: crop [rows,3,224,224] in [0,1], params [rows,236], angles [rows,3] = the Euler angles in degrees of
 *   parameters 200..202.  saved (NULL: nothing is kept) receives sgdfr_deca_saved_elems(rows) bytes: one per ReLU decision and
 *   max-pool choice.  debug (NULL: off) receives sgdfr_deca_debug_elems(rows) floats: the stem, the pool, each stage's first and
 *   last bottleneck output and the pooled features, each [rows, ...].
 * sgdfr_deca_backward_f32: dx [rows,3,H,W] = dL/dx for grad_params [rows,236], from the saved bytes of a forward with the same rows,
 *   x, mat, H, W and pack.  Exactly zero where |x| > 1.
 * sgdfr_deca_crop_f32 / sgdfr_deca_crop_backward_f32: the front alone (range map, crop, / 255) and its adjoint to x for a cotangent
 *   grad_crop [rows,3,224,224].
 * workspace: device scratch of at least sgdfr_deca_workspace_bytes(rows, H, W) bytes.  The split-K plan follows the row count only.
 * Deterministic (no float atomics), no host synchronisation, everything on `stream`. */
int64_t sgdfr_deca_pack_elems(void);
int64_t sgdfr_deca_saved_elems(int rows);
int64_t sgdfr_deca_debug_elems(int rows);
int64_t sgdfr_deca_workspace_bytes(int rows, int H, int W);
int sgdfr_deca_prepack_f32(const float* const* params, float* pack, void* stream);
int sgdfr_deca_crop_f32(const float* x, const float* mat, int rows, int H, int W, float* crop, void* stream);
int sgdfr_deca_crop_backward_f32(const float* grad_crop, const float* x, const float* mat, int rows, int H, int W, float* dx,
                                 void* stream);
int sgdfr_deca_forward_f32(const float* x, const float* mat, int rows, int H, int W, const float* pack, float* crop, float* params,
                           float* angles, uint8_t* saved, float* debug, void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_deca_backward_f32(const float* grad_params, const float* x, const float* mat, const uint8_t* saved, int rows, int H, int W,
                            const float* pack, float* dx, void* workspace, int64_t workspace_bytes, void* stream);

/* The 2D-FAN-4 landmark detector in eval mode (libs/face_models/fan_model/models.py:145-202 FAN(4), landmarks_estimation.py:50-88 and
 * :143-185, fan_model/utils.py:63-97 and :140-165, libs/DECA/decalib/datasets/detectors.py:38-41), csrc/fan.hip.  Forward only.
 * Images x [rows,3,H,W] fp32, 0..255 (SGDFR_FAN_RANGE_255) or [-1,1] mapped to 0..255 as torch_range_1_to_255 does
 * (SGDFR_FAN_RANGE_GAN); faces [rows,4] fp32 on the device: x0, y0, x1, y1 of the face box.  Centre, scale and the integer window are
 * computed on the device in float32 in the reference's order of operations.
 * sgdfr_fan_prepack_f32: params = host array of 735 device pointers, BatchNorms folded on the host to (g, h) = (w rsqrt(var + eps),
 *   b - mean g):  stem w0 [64,3,7,7] and b0 [64] with bn1 folded in;  per ConvBlock (59: conv2, conv3, conv4, then per stack
 *   b1_4 b2_4 b3_4 b1_3 ... b3_1 b2_plus_1 top_m) g1 h1 w1 g2 h2 w2 g3 h3 w3 and the projection's gd hd wd (NULL where in == out);
 *   per stack conv_last w [256,256], b [256] with bn_end folded in, l w [68,256], b [68];  per stack but the last bl w [256,256],
 *   al w [256,68], bl b + al b [256]  -> pack of sgdfr_fan_pack_elems() floats (rebuild it whenever a parameter changes).
 * sgdfr_fan_crop_f32: the front alone -> crop [rows,3,256,256] in [0,1].
 * sgdfr_fan_network_f32: crop -> the last stack's heatmaps [rows,68,64,64].  debug (NULL: off) receives sgdfr_fan_debug_elems(rows)
 *   floats: the stem [rows,64,128,128], conv4's output [rows,256,64,64], then per stack the hourglass output [rows,256,64,64] and
 *   the heatmaps [rows,68,64,64].
 * sgdfr_fan_decode_f32: heatmaps -> pts [rows,68,2] (crop pixels), pts_img [rows,68,2] (image pixels, integer-valued) and, when boxes
 *   is not NULL, boxes [rows,4] = min x, min y, max x, max y of pts_img.  sgdfr_fan_boxes_f32: the boxes of any [rows,68,2] points.
 * sgdfr_fan_forward_f32: crop + network + decode in one call.
 * workspace: device scratch of at least sgdfr_fan_workspace_bytes(rows, H, W) bytes.  The split-K plan follows the row count only.
 * Deterministic (no float atomics), no host synchronisation, everything on `stream`. */
#define SGDFR_FAN_RANGE_255 0
#define SGDFR_FAN_RANGE_GAN 1
int64_t sgdfr_fan_pack_elems(void);
int64_t sgdfr_fan_debug_elems(int rows);
int64_t sgdfr_fan_workspace_bytes(int rows, int H, int W);
int sgdfr_fan_prepack_f32(const float* const* params, float* pack, void* stream);
int sgdfr_fan_crop_f32(const float* x, const float* faces, int rows, int H, int W, int input_range, float* crop, void* stream);
int sgdfr_fan_network_f32(const float* crop, int rows, const float* pack, float* heatmaps, float* debug, void* workspace,
                          int64_t workspace_bytes, void* stream);
int sgdfr_fan_decode_f32(const float* heatmaps, const float* faces, int rows, float* pts, float* pts_img, float* boxes, void* stream);
int sgdfr_fan_boxes_f32(const float* pts_img, int rows, float* boxes, void* stream);
int sgdfr_fan_forward_f32(const float* x, const float* faces, int rows, int H, int W, int input_range, const float* pack,
                          float* heatmaps, float* pts, float* pts_img, float* boxes, float* debug, void* workspace,
                          int64_t workspace_bytes, void* stream);

/* The rest of LandmarksEstimation (landmarks_estimation.py:155-181): flip_input, the Gaussian draw of fan_model/utils.py:13-60 and
 * the 3D landmark type on ResNetDepth (fan_model/models.py:58-95 and :205-265, csrc/fandepth.hip).  Forward only.
 * sgdfr_fan_flip_add_f32: hm2 [2 rows,68,64,64], rows 0..rows-1 the heatmaps of the crops and rows..2 rows-1 those of their mirrors
 *   -> out[b,c,y,x] = hm2[b,c,y,x] + hm2[rows+b, pairs[c], y, 63-x], pairs = shuffle_lr's table (utils.py:256-260).
 * sgdfr_fan_draw_f32: pts [rows,68,2] crop pixels (any float) -> maps [rows,68,256,256]: zeros and, where pts.x > 0 and the window
 *   is not rejected by draw_gaussian's test, its 13x13 Gaussian (sigma 2) placed by the reference's 1-based index arithmetic.  The
 *   table is _gaussian(13) evaluated in double on the host and rounded to float once.  A non-finite coordinate draws nothing.
 * sgdfr_fandepth_prepack_f32: params = host array of 312 device pointers, every BatchNorm folded on the host: stem w0 [64,71,7,7],
 *   b0 [64]; per bottleneck (50 = 3 + 8 + 36 + 3) w1 [P,Cin], b1 [P], w2 [P,P,3,3], b2 [P], w3 [4P,P], b3 [4P] and, for the first of
 *   each layer only, the projection's wd [4P,Cin], bd [4P]; fc w [68,2048], b [68] -> pack of sgdfr_fandepth_pack_elems() floats.
 * sgdfr_fandepth_network_f32: crop [rows,3,256,256] in [0,1] and maps [rows,68,256,256] (the 71 input channels, never concatenated)
 *   -> depth [rows,68].  debug (NULL: off) receives sgdfr_fandepth_debug_elems(rows) floats: the stem [rows,64,128,128], the
 *   max-pool [rows,64,64,64], the outputs of layer1..4 ([rows,256,64,64], [rows,512,32,32], [rows,1024,16,16], [rows,2048,8,8]) and
 *   the pooled features [rows,2048] (AvgPool2d(7) on 8x8: rows and columns 0..6).
 * sgdfr_fan_forward3d_f32: front, network (once on 2 rows crops with the mirrors behind when flip != 0, then flip_add), decode and,
 *   when depth_pack is not NULL, draw, depth network and pts_img3 [rows,68,3] = (pts_img.x, pts_img.y, depth * (1 / (256 / (200
 *   scale)))), each operation rounded on its own.  hm2 [2 rows,68,64,64] is scratch for flip != 0 (else NULL); maps
 *   [rows,68,256,256], depth [rows,68] and pts_img3 are outputs of the 3D part (NULL without depth_pack).  workspace holds
 *   sgdfr_fan_workspace_bytes(flip ? 2 rows : rows, H, W) bytes and debug sgdfr_fan_debug_elems of the same row count;
 *   depth_workspace holds sgdfr_fandepth_workspace_bytes(rows) bytes.
 * Deterministic (no float atomics), no host synchronisation, everything on `stream`. */
int64_t sgdfr_fandepth_pack_elems(void);
int64_t sgdfr_fandepth_debug_elems(int rows);
int64_t sgdfr_fandepth_workspace_bytes(int rows);
int sgdfr_fandepth_prepack_f32(const float* const* params, float* pack, void* stream);
int sgdfr_fandepth_network_f32(const float* crop, const float* maps, int rows, const float* pack, float* depth, float* debug,
                               void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_fan_flip_add_f32(const float* hm2, int rows, float* out, void* stream);
int sgdfr_fan_draw_f32(const float* pts, int rows, float* maps, void* stream);
int sgdfr_fan_forward3d_f32(const float* x, const float* faces, int rows, int H, int W, int input_range, int flip, const float* pack,
                            const float* depth_pack, float* hm2, float* heatmaps, float* pts, float* pts_img, float* boxes, float* maps,
                            float* depth, float* pts_img3, float* debug, void* workspace, int64_t workspace_bytes,
                            void* depth_workspace, int64_t depth_workspace_bytes, void* stream);

/* The S3FD face detector in eval mode (libs/face_models/sfd/net_s3fd.py s3fd, detect.py:36-81 batch_detect, bbox.py:44-66 nms and
 * :93-111 decode, sfd_detector.py:31-47 detect_from_batch), csrc/s3fd.hip.  Forward only.
 * Images x [rows,3,H,W] fp32 with 0..255 values, 1..256 rows, each side 32..4096, rows*H*W <= 2^24.  subtract_mean != 0 subtracts
 * (104, 117, 123) per channel inside the image as detect() does; batch_detect, the path the reference uses, does not.
 * sgdfr_s3fd_prepack_f32: params = host array of 50 device pointers: w [Cout,Cin,k,k] and b [Cout] of the 19 trunk convs in forward
 *   order (conv1_1 ... conv5_3, fc6, fc7, conv6_1, conv6_2, conv7_1, conv7_2), then per level (conv3_3, conv4_3, conv5_3, fc7,
 *   conv6_2, conv7_2) the conf and loc filters concatenated, w [conf+4,C,3,3] and b [conf+4] (conf = 4 at level 0, else 2), the
 *   L2Norm weight of levels 0-2 folded in per input channel on the host -> pack of sgdfr_s3fd_pack_elems() floats (rebuild it
 *   whenever a parameter changes).
 * sgdfr_s3fd_level_dims: hw[12] = (h, w) of the six level maps for an H x W image.
 * sgdfr_s3fd_network_f32: maps receives sgdfr_s3fd_map_elems(rows, H, W) floats: per level cls [rows,2,h,w] (level 0 after the
 *   max-out of its three background logits) then reg [rows,4,h,w], the twelve outputs of s3fd.forward in its order.  debug (NULL:
 *   off) receives sgdfr_s3fd_debug_elems(rows, H, W) floats: conv1_2, conv2_2, conv3_3, conv4_3, conv5_3, fc6, fc7, conv6_2, conv7_2
 *   behind their ReLU and in front of a pool, each [rows,C,h,w], then the reciprocal L2 norms of conv3_3, conv4_3, conv5_3 [rows,h,w].
 * sgdfr_s3fd_candidates_f32: heads = host array of six device pointers, level l [rows, conf+4, h_l, w_l] (the raw head output, conf
 *   channels first), hw = host array of the twelve map sizes.  Max-out, softmax score of channel 1, score > threshold, box decode
 *   against the prior (stride 2^(l+2), centre stride/2 + index*stride, size 4 strides, variances 0.1 / 0.2) -> cand
 *   [rows,capacity,5] = x1, y1, x2, y2, score in (level, y, x) order, count [rows] = the true number even beyond capacity, valid
 *   [rows] = 0 where count > capacity (the list then holds the first `capacity`).  capacity 1..16384.
 * sgdfr_s3fd_nms_f32: per row the first min(count, capacity) candidates: those above 0.5 sorted by score descending (ties: candidate
 *   index ascending), greedy suppression at IoU > 0.3 with "+ 1" areas in float32 -> boxes [rows,capacity,5] in descending score
 *   order (zeros behind the kept ones), index [rows,capacity] = each kept box's candidate index (-1 behind), kept [rows].
 * sgdfr_s3fd_forward_f32: network + candidates + nms in one call; boxes, index and kept may all be NULL (no selection), maps and
 *   debug may be NULL.
 * workspace: device scratch of at least sgdfr_s3fd_workspace_bytes(rows, H, W) bytes.  The split-K plan follows rows, H and W only.
 * Deterministic (no float atomics), no host synchronisation, everything on `stream`: counts stay on the device. */
int64_t sgdfr_s3fd_pack_elems(void);
int64_t sgdfr_s3fd_debug_elems(int rows, int H, int W);
int64_t sgdfr_s3fd_map_elems(int rows, int H, int W);
int64_t sgdfr_s3fd_workspace_bytes(int rows, int H, int W);
int sgdfr_s3fd_level_dims(int H, int W, int* hw);
int sgdfr_s3fd_prepack_f32(const float* const* params, float* pack, void* stream);
int sgdfr_s3fd_network_f32(const float* x, int rows, int H, int W, int subtract_mean, const float* pack, float* maps, float* debug,
                           void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_s3fd_candidates_f32(const float* const* heads, const int* hw, int rows, float threshold, int capacity, float* cand, int* count,
                              int* valid, void* stream);
int sgdfr_s3fd_nms_f32(const float* cand, const int* count, int rows, int capacity, float* boxes, int* index, int* kept, void* stream);
int sgdfr_s3fd_forward_f32(const float* x, int rows, int H, int W, int subtract_mean, const float* pack, float threshold, int capacity,
                           float* cand, int* count, int* valid, float* boxes, int* index, int* kept, float* maps, float* debug,
                           void* workspace, int64_t workspace_bytes, void* stream);

/* The e4e W+ encoder in eval mode (libs/gan/encoder4editing/psp_encoders.py:33-53 and :122-199 Encoder4Editing(50, 'ir_se', R),
 * helpers.py:57-140), csrc/e4e.hip.  Forward only, as in the reference (every call there is under no_grad).
 * Images x [rows,3,R,R] fp32 in [-1,1]; R a multiple of 16 in 32..256 (so that every style head ends at 1x1), 1..256 rows,
 * rows*R*R <= 2^24.  w receives [rows, style_count, 512] with style_count = sgdfr_e4e_style_count(R) = 2 floor(log2 R) - 2:
 * w[:,0] = w0, w[:,i] = w0 + delta_i.  No latent average is added, as in the reference.
 * sgdfr_e4e_prepack_f32: params = host array of sgdfr_e4e_param_count(R) device pointers (423 at R = 256), BatchNorms folded on the
 *   host to (g, h) = (w rsqrt(var + eps), b - mean g):
 *     stem: w0 [64,3,3,3] with the stem BN folded in, b0 [64], PReLU slope a0 [64];
 *     per unit (24, as for the identity loss): BN1 g1 [Cin], h1 [Cin], conv1 w1 [D,Cin,3,3], PReLU slope a1 [D], conv2 w2 [D,D,3,3]
 *       with BN2 folded in, b2 [D], SE fc1 [D/16,D], fc2 [D,D/16], the shortcut conv wsc [D,Cin] with its BN folded in and bsc [D]
 *       (both NULL where Cin == D: the shortcut is a strided subsample);
 *     latlayer1 w [512,256], b [512]; latlayer2 w [512,128], b [512];
 *     per style head, in order: per conv (4 for heads 0-2, 5 for heads 3-6, 6 behind) w [512,512,3,3], b [512]; then the EqualLinear
 *       weight times 1/sqrt(512) [512,512] and its bias [512]
 *   -> pack of sgdfr_e4e_pack_elems(R) floats (rebuild it whenever a parameter changes).
 * sgdfr_e4e_forward_f32: debug (NULL: off) receives sgdfr_e4e_debug_elems(rows, R) floats: the stem [rows,64,R,R], unit 0's output
 *   [rows,64,R/2,R/2], unit 3's [rows,128,R/4,R/4], c1 [rows,128,R/4,R/4], c2 [rows,256,R/8,R/8], c3 [rows,512,R/16,R/16],
 *   p2 [rows,512,R/8,R/8], p1 [rows,512,R/4,R/4] and the head vectors in front of the EqualLinears [rows,style_count,512].
 * A bad R, rows < 1 or a workspace below sgdfr_e4e_workspace_bytes(rows, R) bytes is an error (the size functions return -1 for
 *   sizes out of range).  The split-K plan follows rows and R only.
 * Deterministic (no float atomics), no host synchronisation, everything on `stream`.
 * The `_n` entries take the head count `styles` beside the input side: the reference's style_count = 2 log2(image_resolution) - 2
 *   (psp_encoders.py:143-156), 8..18 for an image_resolution of 32..1024, independent of R (the 512 and 1024 generators' encoders
 *   read the same 256 x 256 crop and have 16 and 18 heads: heads 0-2 on c3, 3-6 on p2, 7..styles-1 on p1).  R as above.  Every entry
 *   without `_n` is its `_n` form at styles = sgdfr_e4e_style_count(R); sgdfr_e4e_param_count_n(256, 18) = 423 + 4 * 14.  The
 *   workspace's two parked head-map buffers hold max(64, 8 (styles - 7)) R^2 floats per row: the layout of styles <= 15 is unchanged.
 *   The split-K plan follows rows, R and styles only. */
int sgdfr_e4e_style_count(int R);
int sgdfr_e4e_param_count(int R);
int64_t sgdfr_e4e_pack_elems(int R);
int64_t sgdfr_e4e_debug_elems(int rows, int R);
int64_t sgdfr_e4e_workspace_bytes(int rows, int R);
int sgdfr_e4e_prepack_f32(const float* const* params, int R, float* pack, void* stream);
int sgdfr_e4e_forward_f32(const float* x, int rows, int R, const float* pack, float* w, float* debug, void* workspace,
                          int64_t workspace_bytes, void* stream);
int sgdfr_e4e_param_count_n(int R, int styles);
int64_t sgdfr_e4e_pack_elems_n(int R, int styles);
int64_t sgdfr_e4e_debug_elems_n(int rows, int R, int styles);
int64_t sgdfr_e4e_workspace_bytes_n(int rows, int R, int styles);
int sgdfr_e4e_prepack_n_f32(const float* const* params, int R, int styles, float* pack, void* stream);
int sgdfr_e4e_forward_n_f32(const float* x, int rows, int R, int styles, const float* pack, float* w, float* debug, void* workspace,
                            int64_t workspace_bytes, void* stream);

/* The FFHQ alignment crop in front of the e4e encoder (libs/face_models/ffhq_cropping.py:13-69 crop_using_landmarks with
 * pad_img_to_fit_bbox and crop_from_bbox), csrc/facecrop.hip.  frames [rows,H,W,3] uint8, landmarks [rows,68,2] fp32, both on the
 * device; 1..1024 rows, H, W and max_size in 1..4096, out_size S in 1..1024.
 * Box, in the reference's integer semantics: centre = round((min + max) / 2) in fp32, half to even; size = (int) max(extent_x,
 *   extent_y); centre_y -= size / 6; box = centre -+ size.  boxes [rows,4] = x1, y1, x2, y2 and sizes [rows] (zeros for landmarks
 *   that are not finite or lie beyond 1e6).
 * valid [rows] = 0 where size < 1, size > max_size (the workspace's capacity), a border is wider than the frame dimension it reflects
 *   (the reference's border repeats there; this is the one deviation) or the padded frame would exceed the workspace (a box far
 *   outside the frame); such a row's crop is zeros (and its e4e row 0.0) and no other row is affected.
 * Rows whose box leaves the frame: symmetric border (cv2.BORDER_REFLECT), the feather mask from the four border widths with 1e-10
 *   for a zero width, scipy's separable Gaussian (sigma 5, 41 taps, 'reflect', axis 0 then axis 1, double weights and accumulator,
 *   fp32 after each axis) over the whole padded frame, img += (blur - img) * clip(3 mask + 1, 0, 1), the per-channel np.median of
 *   the padded frame as an exact selection (integer atomics: reproducible), img += (median - img) * clip(mask, 0, 1), truncation to
 *   uint8.  Rows whose box is inside the frame go straight to the resize.
 * Resize: Pillow's 8-bit bicubic resampler (Resample.c: coefficients in double, 22-bit integers, horizontal pass, uint8, vertical
 *   pass), bit-exact, with the coefficients of each row's crop side 2 size computed on the device.
 * crops [rows,S,S,3] uint8; e4e (NULL: off) [rows,3,S,S] fp32 = u8 / 255 * 2 - 1 in that fp32 order; boxes and sizes may be NULL;
 *   crop_float (NULL: off) receives rows * (2 max_size)^2 * 3 floats: per row, at offset row * (2 max_size)^2 * 3, the dense
 *   [2 size, 2 size, 3] crop in front of the truncation.
 * workspace: device scratch of at least sgdfr_facecrop_workspace_bytes(rows, H, W, max_size) bytes (-1 for sizes out of range).
 * Deterministic, no host synchronisation, everything on `stream`. */
int64_t sgdfr_facecrop_workspace_bytes(int rows, int H, int W, int max_size);
int sgdfr_facecrop_boxes_f32(const float* landmarks, int rows, int* boxes, int* sizes, void* stream);
int sgdfr_facecrop_forward_u8(const uint8_t* frames, const float* landmarks, int rows, int H, int W, int out_size, int max_size,
                              uint8_t* crops, int* valid, float* e4e, int* boxes, int* sizes, float* crop_float, void* workspace,
                              int64_t workspace_bytes, void* stream);

/* DECA's shape renderer (libs/DECA/decalib/utils/renderer.py:237-293 SRenderY.render_shape, :28-78 Pytorch3dRasterizer at its fixed
 * settings, utils/util.py:193-225 vertex_normals, :227-237 batch_orth_proj with deca.py:175), csrc/shaperender.hip.  Forward only.
 * A general triangle mesh: vertices [rows,V,3] fp32, faces [F,3] int32 shared by all rows, and the vertex -> corner table of the faces:
 *   csr_offsets [V+1], csr_entries [3F] = face * 3 + corner of every corner that names the vertex, ascending per vertex.  The caller
 *   vouches for index ranges; an index outside 0..V-1 only drops its face.  rows 1..4096, V and F 1..2^24.
 * sgdfr_shaperender_normals_f32: normals [rows,V,3]: per corner k of a face the cross product (v[k+1] - v[k]) x (v[k+2] - v[k]), summed
 *   per vertex in table order, then n / max(|n|, 1e-6); a vertex no face names gets zeros.
 * sgdfr_shaperender_forward_f32: exactly one of cam [rows,3] = (s, tx, ty) and projected [rows,V,3].  With cam: X = s (x + tx),
 *   Y = -s (y + ty), Z = -s z + z_offset; with projected: Z + z_offset only (render_shape uses z_offset = 10).
 *   Rasteriser at S x S, 1..4096: the centre of pixel (row i, column j) is p = ((2j+1)/S - 1, (2i+1)/S - 1);
 *   edge(p;u,v) = (p.x-u.x)(v.y-u.y) - (p.y-u.y)(v.x-u.x), area = edge(c;a,b), w0 = edge(p;b,c) / (area + 1e-8), w1 = edge(p;c,a) / ..,
 *   w2 = edge(p;a,b) / ..; a face with |area| <= 1e-8 or all three Z < 0 is skipped; a pixel is covered iff w0, w1, w2 > 0 strictly
 *   (both windings, no clipping of the barycentrics, no perspective correction); z = w0 Za + w1 Zb + w2 Zc, dropped when z < 0; the
 *   smallest z wins, the lower face index on equal z.  These restate pytorch3d's rasterize_meshes at blur_radius 0 and one face per
 *   pixel with the x, y flip of renderer.py:53 folded in; the tie rule is this library's.
 *   pix_to_face [rows,S,S] int32 (-1: none; the index counts within the mesh), zbuf [rows,S,S] and bary [rows,S,S,3] (-1 where no
 *   face covers): each may be NULL.
 *   shape (NULL: rasterise only; vertices, the table, lights, alpha and background are then unused) [rows,3,S,S]: with N the world normal
 *   and Tz the z of the projected vertices' normal, both interpolated with w and not re-normalised: albedo = (w0+w1+w2) 180/255,
 *   shading_c = mean_l clamp(N . d_l, 0, 1) I_lc for lights [light_rows = 1 or rows, L <= 8, 6] = direction (normalised here), intensity;
 *   alpha = covered (Tz < 0.15);  out = albedo shading alpha + background (1 - alpha), background [rows,3,S,S] or NULL for 0;
 *   gan_range != 0 writes clamp(out, 0, 1) 2 - 1 instead.  alpha [rows,1,S,S] may be NULL.
 * workspace: device scratch of at least sgdfr_shaperender_workspace_bytes(rows, V, F) bytes (-1 for sizes out of range).
 * Five launches (project, normals twice, face setup, raster + shade), no atomics: bit-identical from call to call; no host
 * synchronisation, everything on `stream`. */
int64_t sgdfr_shaperender_workspace_bytes(int rows, int V, int F);
int sgdfr_shaperender_normals_f32(const float* vertices, int rows, int V, const int* faces, int F, const int* csr_offsets,
                                  const int* csr_entries, float* normals, void* stream);
int sgdfr_shaperender_forward_f32(const float* vertices, const float* projected, const float* cam, float z_offset, int rows, int V,
                                  const int* faces, int F, const int* csr_offsets, const int* csr_entries, int S, const float* lights,
                                  int light_rows, int L, const float* background, int gan_range, float* shape, float* alpha,
                                  int* pix_to_face, float* zbuf, float* bary, void* workspace, int64_t workspace_bytes, void* stream);
/* sgdfr_shaperender_detail_f32: sgdfr_shaperender_forward_f32 with the detail panel of DECA.decode_deca (deca.py:187-189) from the same
 *   rasterisation.  In addition: face_uv [F,3,2], the first two components of the renderer's face_uvcoords; uv_normals [rows,3,Su,Su], the
 *   UV detail normal map; Su 1..4096.  vertices, the vertex table and lights are always needed.  Every output may be NULL:
 *   shape, alpha, pix_to_face, zbuf, bary as above (shape has the bits sgdfr_shaperender_forward_f32 writes);
 *   grid [rows,S,S,2] = g = sum_k w_k face_uv[f][k], (0, 0) where no face covers (ops['grid']);
 *   detail_normal_images [rows,3,S,S] = N = covered * bilinear(uv_normals[row], g), with F.grid_sample's rules at align_corners False and
 *     zero padding: ix = ((g.x + 1) Su - 1) / 2, iy likewise, the four neighbours weighted (1 - frac) and frac, a neighbour outside the
 *     map adding nothing;
 *   shape_detail [rows,3,S,S]: the expression of `shape` with the shading normal replaced by N (albedo, alpha, background, gan_range as
 *     above).
 *   The reference adds z_offset to the projected vertices in place on each of its three render calls; with an orthographic projection
 *   that changes nothing while |z| < 10, and here z_offset is applied once. */
int sgdfr_shaperender_detail_f32(const float* vertices, const float* projected, const float* cam, float z_offset, int rows, int V,
                                 const int* faces, int F, const int* csr_offsets, const int* csr_entries, int S, const float* lights,
                                 int light_rows, int L, const float* background, int gan_range, const float* face_uv,
                                 const float* uv_normals, int Su, float* shape, float* shape_detail, float* grid,
                                 float* detail_normal_images, float* alpha, int* pix_to_face, float* zbuf, float* bary, void* workspace,
                                 int64_t workspace_bytes, void* stream);

/* DECA's detail path in eval mode (libs/DECA/decalib/models/decoders.py Generator(181, 1, 0.01, 'bilinear'), deca.py:114-141
 * displacement2normal / displacement2vertex, utils/renderer.py:331-340 world2uv), csrc/detail.hip.  Forward only.
 * D_detail: latent [rows,181] = cat(pose[:, 3:], exp, detail) -> Linear 181->8192 + BatchNorm(128), seen as [rows,128,8,8] -> five times
 *   (2x bilinear upsample, conv3x3 pad 1, BatchNorm, LeakyReLU 0.2) to 128@16^2, 64@32^2, 64@64^2, 32@128^2, 16@256^2 -> conv3x3 16->1,
 *   tanh, * out_scale -> uv_z [rows,1,256,256].  1..256 rows.  The upsample is upsample_bilinear2d at align_corners False: source
 *   coordinate max(0, (i + 0.5) / 2 - 0.5), upper neighbour clamped to h - 1; the conv's zero padding applies to the upsampled map.
 * sgdfr_detail_prepack_f32: params = host array of 14 device pointers, BatchNorms folded on the host (the five behind the convs are
 *   nn.BatchNorm2d(C, 0.8): eps = 0.8): the Linear's weight [8192,181] and bias [8192] with the first BatchNorm folded in per channel
 *   c = row / 64; per conv (six) w [Cout,Cin,3,3] and b [Cout] -> pack of sgdfr_detail_pack_elems() floats.
 * sgdfr_detail_decode_f32: taps (NULL: off) receives per stage [rows, ...]: the Linear's output [rows,128,8,8], then the five layers'
 *   outputs, 1941504 floats a row; the layers then write there directly.  workspace of at least sgdfr_detail_workspace_bytes(rows)
 *   bytes (-1 for rows out of range).  Seven launches plus the finish of a layer that splits K.
 * sgdfr_detail_upconv_f32: the layer kernel alone: x [rows,Cin,h,w], filter [Cout,Cin,3,3] (transposed into the workspace first), bias
 *   [Cout] -> y [rows,Cout,up ? 2h : h,up ? 2w : w] = lrelu(conv3x3(up ? upsample2x(x) : x) + bias, slope); slope = 1: no activation.
 *   rows 1..4096, Cin and Cout 1..1024, h and w 1..256, at most 2^28 output pixels; workspace of at least
 *   sgdfr_detail_upconv_workspace_bytes(Cin, Cout) bytes.  One 64-pixel x (Cout <= 16 ? 16 : 64)-channel tile per block; the split-K
 *   plan follows rows, the sizes and the channel counts only.
 * UV space.  The layout's table pix_to_face [S,S] int32 (-1: none) and bary [S,S,3] come from sgdfr_shaperender_forward_f32 on the UV
 *   vertices; faces [F,3] index the V mesh vertices; 13 <= S <= 1024.
 * sgdfr_detail_world2uv_f32: values [rows,V,3] -> out [rows,3,S,S] = sum_k bary_k values[faces[f][k]], 0 where no face covers.
 * sgdfr_detail_uvnormals_f32: uv_z [rows,1,S,S], vertices and normals [rows,V,3], mask and fixed_dis [S,S] -> uv_normals [rows,3,S,S]:
 *   the dense vertex of a texel is P = (uv_v + (uv_z mask) uv_n) + fixed_dis uv_n with uv_v, uv_n = world2uv of the vertices, normals;
 *   the dense faces are util.generate_triangles(S, S): per quad (y, x), x in [2, S-3), y in [5, S-6), x outermost, the two faces
 *   (a, c, b), (b, c, d) of a = y S + x, b = a + 1, c = a + S, d = c + 1; the normals follow sgdfr_shaperender_normals_f32's rule over
 *   them, summed in ascending (face, corner) order; a texel outside the meshed rectangle gets zeros.  dense_vertices (NULL: off)
 *   receives P as [rows,S*S,3] (displacement2vertex).  One launch, no atomics.
 * Deterministic, no host synchronisation, everything on `stream`. */
int64_t sgdfr_detail_pack_elems(void);
int64_t sgdfr_detail_workspace_bytes(int rows);
int64_t sgdfr_detail_upconv_workspace_bytes(int Cin, int Cout);
int sgdfr_detail_prepack_f32(const float* const* params, float* pack, void* stream);
int sgdfr_detail_decode_f32(const float* latent, int rows, const float* pack, float out_scale, float* uv_z, float* taps, void* workspace,
                            int64_t workspace_bytes, void* stream);
int sgdfr_detail_upconv_f32(const float* x, const float* w, const float* bias, int rows, int Cin, int Cout, int h, int wd, float slope, int up,
                            float* y, void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_detail_world2uv_f32(const float* values, int rows, int V, const int* faces, int F, const int* pix_to_face, const float* bary, int S,
                              float* out, void* stream);
int sgdfr_detail_uvnormals_f32(const float* uv_z, const float* vertices, const float* normals, int rows, int V, const int* faces, int F,
                               const int* pix_to_face, const float* bary, const float* mask, const float* fixed_dis, int S, float* uv_normals,
                               float* dense_vertices, void* stream);

/* DECA's texture side (libs/DECA/decalib/models/FLAME.py:216-262 FLAMETex, utils/renderer.py:121-206 SRenderY.forward and add_SHlight,
 * 295-329 render_depth / render_normal, deca.py:143-148 visofp and 180-199), csrc/texture.hip, csrc/shaperender.hip, csrc/flame.hip.
 * Forward only.
 * FLAMETex: albedo [rows,3,uv,uv] = (mean + basis . code) at the source size Hs x Ws x 3, nearest-neighbour resized to uv x uv, channels
 *   flipped [2,1,0].  1 <= uv <= 1024, 1 <= n_tex <= 200, Hs and Ws 1..4096, rows 1..4096.
 * sgdfr_flametex_prepack_f32: params = host array of 4 device pointers: texture_mean [Hs*Ws*3], texture_basis [Hs*Ws*3][n_tex], and the
 *   source row of every output row and source column of every output column, int32 [uv] each (F.interpolate's nearest rule, evaluated
 *   on the host) -> pack of sgdfr_flametex_pack_elems(uv, n_tex) floats: mean [3][uv][uv], then basis [n_tex][3][uv][uv], kept texels
 *   only, channels already flipped.
 * sgdfr_flametex_forward_f32: code [rows,n_tex] -> albedo = mean + sum_k basis_k code[row][k], k ascending, one fmaf each: a row's bits
 *   do not depend on the batch.  One launch; the pack is streamed from memory once per group of 32 rows.
 * sgdfr_shaperender_texture_f32: SRenderY.forward from the rasterisation of sgdfr_shaperender_forward_f32 (same vertices / projected /
 *   cam / z_offset arguments and workspace).  face_uv [F,3,2]; albedo [rows,3,Su,Su] (NULL without images and albedo_images);
 *   sh_lights [rows,9,3] or NULL; sh_constants: HOST array of the 9 factors of renderer.py:114-119.  With w the barycentrics of the covering face and all attributes 0 where none covers,
 *   every output may be NULL:
 *   grid [rows,S,S,2] as sgdfr_shaperender_detail_f32 writes it, bit for bit; alpha_images [rows,1,S,S] = 1 where a face covers (no
 *   front-facing mask); pos_mask [rows,1,S,S] = 1 where the interpolated z of the projected vertices' normals is < -0.05;
 *   normal_images [rows,3,S,S] = alpha * interpolated world normal (not renormalised); shading_images [rows,3,S,S] = sum_k
 *   sh_lights[k][c] (basis_k(n) constant_k), k ascending, basis = (1, x, y, z, xy, xz, yz, x^2 - y^2, 3 z^2 - 1) of the interpolated
 *   normal -- NOT masked: c0 L0 - c8 L8 where no face covers -- and 0 without sh_lights; albedo_images [rows,3,S,S] = alpha *
 *   bilinear(albedo, grid) (the grid_sample rules above); images = albedo_images * shading_images (albedo_images without sh_lights);
 *   normals and transformed_normals [rows,V,3]: the vertex normals of the world and of the projected vertices; pix_to_face, zbuf, bary
 *   as above.  Five launches, six with transformed_normals.
 * sgdfr_shaperender_attr_f32: values [rows,V,D], D 1..3, interpolated over the rasterisation of `projected` (z + z_offset) -> out
 *   [rows,D,S,S], 0 where no face covers (render_normal; render_depth with the normalised depth as the value).  Three launches.
 * sgdfr_texture_uv_f32: the UV texture pass in one launch over [rows,S,S]: uv_shading = add_SHlight(uv_normals [rows,3,S,S], light
 *   [rows,9,3]); uv_texture = albedo * uv_shading (albedo [rows,3,S,S], NULL: no texture model); uv_pverts = world2uv(trans_verts
 *   [rows,V,3]) through the layout's table (pix_to_face [S,S], bary [S,S,3], faces [F,3]), 0 where no face covers; uv_gt = bilinear(images
 *   [rows,3,H,W], uv_pverts.xy), so an uncovered texel samples the image centre; uv_texture_gt = uv_gt mask + (uv_texture, or 1 without
 *   albedo) (1 - mask) 0.7 with mask [S,S].  Every output may be NULL; S 1..1024, H and W 1..4096.
 * sgdfr_flame_visofp_f32: values [rows,n_vertices,3] gathered at n landmarks (corners int32 [n,3] vertex indices, bary [n,3]) ->
 *   vis [rows,n,1] = 1 where the gathered z < threshold; gathered [rows,n,3] (NULL: off).
 * Deterministic, no host synchronisation, everything on `stream`. */
int64_t sgdfr_flametex_pack_elems(int uv, int n_tex);
int sgdfr_flametex_prepack_f32(const void* const* params, int Hs, int Ws, int uv, int n_tex, float* pack, void* stream);
int sgdfr_flametex_forward_f32(const float* code, int rows, const float* pack, int uv, int n_tex, float* albedo, void* stream);
int sgdfr_shaperender_texture_f32(const float* vertices, const float* projected, const float* cam, float z_offset, int rows, int V,
                                  const int* faces, int F, const int* csr_offsets, const int* csr_entries, int S, const float* sh_lights,
                                  const float* sh_constants, const float* face_uv, const float* albedo, int Su, float* images,
                                  float* albedo_images, float* alpha_images, float* pos_mask, float* shading_images, float* grid,
                                  float* normal_images, float* normals, float* transformed_normals, int* pix_to_face, float* zbuf, float* bary,
                                  void* workspace, int64_t workspace_bytes, void* stream);
int sgdfr_shaperender_attr_f32(const float* projected, float z_offset, int rows, int V, const int* faces, int F, int S, const float* values,
                               int D, float* out, int* pix_to_face, float* zbuf, float* bary, void* workspace, int64_t workspace_bytes,
                               void* stream);
int sgdfr_texture_uv_f32(const float* albedo, const float* uv_normals, const float* light, const float* sh_constants, const float* trans_verts,
                         const float* images, int rows, int V, int H, int W, const int* faces, int F, const int* pix_to_face, const float* bary,
                         const float* mask, int S, float* uv_shading, float* uv_texture, float* uv_texture_gt, float* uv_pverts, float* uv_gt,
                         void* stream);
int sgdfr_flame_visofp_f32(const float* values, int rows, int n_vertices, const int* corners, const float* bary, int n, float threshold,
                           float* vis, float* gathered, void* stream);

/* Measurement aid (csrc/probe.hip; no reference counterpart): the rate v_mfma_f32_32x32x16_{f16,bf16} sustains on THIS device,
 * in 16-bit TFLOP/s -- arith SGDFR_SPLIT_FP16/BF16; lds_fragments 1: operands re-read from LDS at the split conv's ratio
 * (8 ds_read_b128 per 12 MFMAs), 0: register operands; random_operands 1: random mantissas, 0: zeros.  The chip clocks to its
 * power budget and MFMA power follows operand toggling, so the random-operand figure (not the nominal 2.5 PFLOP/s) is what a
 * kernel on real data can reach; bench.py prints it beside the roofline.  blocks <= 0: 256 (one 8-wave block per CU);
 * scratch: blocks*512 floats of device memory.  Synchronises `stream`. */
int sgdfr_mfma_ceiling_probe(int arith, int lds_fragments, int random_operands, int iters, int blocks, float* scratch,
                             double* tflops16, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SGDFR_H */
