/* C ABI of csrc/conv2d.hip: the kernel behind ddsp_amd.training.nn's conv2d / SpatialConv2D / ResNet and
 * training.encoders.ResnetSinusoidalEncoder (a 2-D convolution of a channel-last tensor, TF 'same' padding, strides on both axes),
 * and its adjoint in x.  Typed from ddsp_amd/_lib.py CONV2D_SIGNATURES (not part of include/ddsp_amd.h: DESIGN.md section 8).
 * Return codes, pointer and stream conventions are those of include/ddsp_amd.h: device pointers to contiguous fp32,
 * `stream` a hipStream_t, every launch enqueued on it in one linear chain, no allocation, copy or synchronisation.
 *
 * The shape arguments always describe the FORWARD convolution: an image [batch, h, w, ch_in], a kernel [kh, kw, ch_in, ch_out]
 * (the Keras layout), strides (sh, sw), and the output [batch, out_h, out_w, ch_out] with TF's 'same' rule
 * (tensorflow/core/framework/kernel_shape_util.cc GetWindowedOutputSizeVerbose):
 *   out_h = ceil(h / sh), total_h = max((out_h - 1) sh + kh - h, 0), top = total_h / 2 (the odd row goes behind); w alike.
 *
 * Limits (DDSP_ERR_UNSUPPORTED beyond, checked before anything is launched): ch_in, ch_out <= DDSP_CONV2D_MAX_CHANNELS,
 * kh * kw <= DDSP_CONV2D_MAX_TAPS, sh, sw <= DDSP_CONV2D_MAX_STRIDE, h, w <= 2^30, and batch * h * w * ch_in,
 * batch * out_h * out_w * ch_out and kh * kw * ch_in * ch_out all < 2^31.  batch = 0 is a no-op. */
#ifndef DDSP_AMD_CONV2D_ABI_H_
#define DDSP_AMD_CONV2D_ABI_H_
#include <stddef.h>
#include "../../include/ddsp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DDSP_CONV2D_MAX_CHANNELS 1024
#define DDSP_CONV2D_MAX_TAPS 64
#define DDSP_CONV2D_MAX_STRIDE 8

#define DDSP_CONV2D_RELU_INPUT 0x1u    /* act = ReLU, applied to x as it is loaded (identity without) */
#define DDSP_CONV2D_ADJOINT 0x2u       /* the call is the adjoint in x of the convolution the shape arguments describe */
#define DDSP_CONV2D_MASK_OUTPUT 0x4u   /* the sum is multiplied by (mask_src > 0): relu'(x), as tf.nn.relu's gradient takes it */

/* Bytes of scratch ddsp_conv2d_f32 needs for this shape and these flags (0 where it needs none, or outside the limits). */
size_t ddsp_conv2d_workspace_bytes(int batch, int h, int w, int ch_in, int ch_out, int kh, int kw, int sh, int sw, unsigned flags);

/* Forward (without DDSP_CONV2D_ADJOINT): x [batch, h, w, ch_in]; y, addend, mask_src [batch, out_h, out_w, ch_out]; bias [ch_out]:
 *   y[b, oh, ow, co] = addend + mask * (bias[co] + sum_{i, j, ci} act(x[b, oh sh + i - top, ow sw + j - left, ci]) W[i, j, ci, co])
 * Adjoint: x is the gradient [batch, out_h, out_w, ch_out]; y, addend, mask_src [batch, h, w, ch_in]; bias [ch_in]:
 *   y[b, r, c, ci] = addend + mask * (bias[ci] + sum g[b, (r + top - i) / sh, (c + left - j) / sw, co] W[i, j, ci, co])
 * over the taps (i, j) for which both divisions are exact and in range: a gather, no atomics.
 * Positions outside the image contribute 0.  W is the forward kernel [kh, kw, ch_in, ch_out] in both directions.  bias and addend
 * may be NULL (0); mask_src is read only with DDSP_CONV2D_MASK_OUTPUT (mask = 1 without).
 * A produced width (ch_out forward, ch_in adjoint) that is a multiple of 16 runs on the matrix cores (fp16 hi / lo operands, x
 * behind a power-of-two scale per batch row, W behind one per call, the K axis the flattened (i, j, channel)); every other width
 * on the vector ALU and without a workspace.  A batch row's values depend on that row and W alone. */
int ddsp_conv2d_f32(const float* x, const float* W, const float* bias, const float* addend, const float* mask_src, float* y,
                    void* workspace, size_t workspace_bytes, int batch, int h, int w, int ch_in, int ch_out, int kh, int kw, int sh,
                    int sw, unsigned flags, void* stream);

#ifdef __cplusplus
}
#endif
#endif
