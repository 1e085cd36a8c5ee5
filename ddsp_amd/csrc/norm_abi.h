/* C ABI of csrc/group_norm.hip: the kernel behind ddsp_amd.training.nn's normalize_op / Normalize / ConditionalNorm (instance,
 * layer and group normalisation of a channel-last tensor).
 * Typed from ddsp_amd/_lib.py NORM_SIGNATURES (not part of include/ddsp_amd.h yet: DESIGN.md section 8 says why).
 * Return codes, pointer and stream conventions are those of include/ddsp_amd.h: device pointers to contiguous fp32,
 * `stream` a hipStream_t, every launch enqueued on it in one linear chain, no allocation, copy or synchronisation.
 *
 * x is [n, s, c] (s = height * width), channels last; group g of `groups` holds the c / groups adjacent channels
 * g c / groups .. (g + 1) c / groups - 1.  groups = c is instance norm, groups = 1 layer norm.
 * Limits: n * s * c < 2^31 (DDSP_ERR_UNSUPPORTED beyond); groups must divide c (DDSP_ERR_BAD_SHAPE); n = 0 is a no-op. */
#ifndef DDSP_AMD_NORM_ABI_H_
#define DDSP_AMD_NORM_ABI_H_
#include <stddef.h>
#include "../../include/ddsp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t ddsp_group_norm_workspace_bytes(size_t n, size_t s, int c, int groups);

/* xhat = (x - mean) * rstd, rstd = 1 / sqrt(var + eps), mean and biased variance over the s * c / groups elements of each
 * (batch row, group); y = xhat * scale + shift, or y = xhat when scale and shift are both NULL (they come together).
 * scale, shift [c]; mean, rstd [n, groups], written when both are given (what the backward keeps), or both NULL.
 * A group whose variance is exactly 0 has mean = its value exactly, so xhat = 0 there. */
int ddsp_group_norm_f32(const float* x, const float* scale, const float* shift, float* y, float* mean, float* rstd, void* workspace,
                        size_t workspace_bytes, size_t n, size_t s, int c, int groups, float eps, void* stream);

size_t ddsp_group_norm_backward_workspace_bytes(size_t n, size_t s, int c, int groups);

/* dx [n, s, c] from dy, x and the mean and rstd the forward wrote (xhat is recomputed, never stored):
 * dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * scale (dy when scale is NULL), means over the group.
 * dscale[ch] = sum over n, s of dy * xhat and dshift[ch] = sum of dy, both [c], when both are given (scale must be too), or
 * both NULL: per-block partial rows in the workspace, summed in ascending order.  No atomics anywhere. */
int ddsp_group_norm_backward_f32(const float* dy, const float* x, const float* mean, const float* rstd, const float* scale, float* dx,
                                 float* dscale, float* dshift, void* workspace, size_t workspace_bytes, size_t n, size_t s, int c,
                                 int groups, void* stream);

#ifdef __cplusplus
}
#endif
#endif
