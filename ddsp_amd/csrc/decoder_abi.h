/* C ABI of csrc/decoder.hip: the kernels behind ddsp_amd.training.nn's Fc / Rnn layers and training.decoders.RnnFcDecoder.
 * Typed from ddsp_amd/_lib.py DECODER_SIGNATURES (not part of include/ddsp_amd.h yet: DESIGN.md section 8 says why).
 * Return codes, pointer and stream conventions are those of include/ddsp_amd.h: device pointers to contiguous fp32,
 * `stream` a hipStream_t, every launch enqueued on it in one linear chain, no allocation, copy or synchronisation. */
#ifndef DDSP_AMD_DECODER_ABI_H_
#define DDSP_AMD_DECODER_ABI_H_
#include <stddef.h>
#include "../../include/ddsp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* activations of ddsp_bias_norm_act_f32 */
#define DDSP_ACT_LINEAR 0
#define DDSP_ACT_LEAKY_RELU 1      /* slope 0.2 (tf.nn.leaky_relu) */
#define DDSP_ACT_RELU 2
#define DDSP_ACT_SIGMOID 3
#define DDSP_ACT_TANH 4

#define DDSP_GRU_MAX_HIDDEN 2048   /* beyond: DDSP_ERR_UNSUPPORTED */

/* y = act(gamma * xhat + beta), xhat = (v - mean(v)) * rstd, v = x + bias, rstd = 1 / sqrt(var(v) + eps), biased two-pass
 * variance over the `ch` entries of a row.  x, y [rows, ch]; bias, gamma, beta [ch].  xhat [rows, ch] and rstd [rows] are
 * written when both are given (what the backward needs), or both NULL. */
int ddsp_bias_norm_act_f32(const float* x, const float* bias, const float* gamma, const float* beta, float* y, float* xhat,
                           float* rstd, size_t rows, int ch, int act, float eps, void* stream);

size_t ddsp_bias_norm_act_backward_workspace_bytes(size_t rows, int ch);

/* dx [rows, ch] and dparams [3, ch] = (dgamma, dbeta, dbias) from dy and what the forward saved.  The parameter gradients
 * are per-wavefront partial rows in the workspace, summed in ascending order: no atomics. */
int ddsp_bias_norm_act_backward_f32(const float* dy, const float* xhat, const float* rstd, const float* gamma, const float* beta,
                                    float* dx, float* dparams, void* workspace, size_t workspace_bytes, size_t rows, int ch,
                                    int act, void* stream);

size_t ddsp_gru_forward_workspace_bytes(int batch, int hidden);

/* The Keras GRU recurrence (reset_after, gates z, r, h), one launch per time step.
 * mx [batch, steps, 3 hidden] = x kernel + bias[0]; recurrent_kernel [hidden, 3 hidden]; recurrent_bias [3 hidden];
 * h0 [batch, hidden]; y [batch, steps, hidden].  saved [4, batch, steps, hidden] = (z, r, hh, mh_h) or NULL. */
int ddsp_gru_forward_f32(const float* mx, const float* recurrent_kernel, const float* recurrent_bias, const float* h0, float* y,
                         float* saved, void* workspace, size_t workspace_bytes, int batch, int steps, int hidden, void* stream);

size_t ddsp_gru_backward_workspace_bytes(int batch, int hidden);

/* The backward scan, t = steps - 1 .. 0, one launch per step.  dy, y [batch, steps, hidden]; saved as the forward wrote it.
 * Writes d_in = (da_z, da_r, da_h) and d_rec = (da_z, da_r, da_h r), both [batch, steps, 3 hidden], and dh0 [batch, hidden];
 * the weight gradients are matrix products of these over all steps, left to the caller. */
int ddsp_gru_backward_f32(const float* dy, const float* y, const float* h0, const float* saved, const float* recurrent_kernel,
                          float* d_in, float* d_rec, float* dh0, void* workspace, size_t workspace_bytes, int batch, int steps,
                          int hidden, void* stream);

#ifdef __cplusplus
}
#endif
#endif
