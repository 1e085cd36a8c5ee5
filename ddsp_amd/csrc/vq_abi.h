/* C ABI of csrc/vq.hip: the kernels behind ddsp_amd.training.nn's vq_assign / vq_statistics / VectorQuantization (the nearest
 * centroid of every vector of a batch, and the per-centroid counts and sums of a batch).
 * Typed from ddsp_amd/_lib.py VQ_SIGNATURES (not part of include/ddsp_amd.h yet: DESIGN.md section 8 says why).
 * Return codes, pointer and stream conventions are those of include/ddsp_amd.h: device pointers to contiguous fp32 (int32 for
 * the indices), `stream` a hipStream_t, every launch enqueued on it in one linear chain, no allocation, copy or synchronisation.
 *
 * x is [rows, heads * dims]: vector (i, h) is x[i, h dims : (h + 1) dims], read in place.  e is [k, dims].
 *
 * Limits (DDSP_ERR_UNSUPPORTED beyond, checked before anything is launched): k <= DDSP_VQ_MAX_CENTROIDS,
 * dims <= DDSP_VQ_MAX_DIMS, rows * heads < 2^31.  rows = 0 is a no-op. */
#ifndef DDSP_AMD_VQ_ABI_H_
#define DDSP_AMD_VQ_ABI_H_
#include <stddef.h>
#include "../../include/ddsp_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DDSP_VQ_MAX_CENTROIDS 4096
#define DDSP_VQ_MAX_DIMS 512

/* Bytes of scratch ddsp_vq_assign_f32 needs for this codebook (0 where the shape is outside the limits). */
size_t ddsp_vq_workspace_bytes(int k, int dims);

/* c[i, h] = argmin_j (|e_j|^2 / 2 - x_ih . e_j), which is argmin_j |x_ih - e_j|^2; of exactly equal scores the lowest j.
 * z[i, h dims + d] = e[c[i, h], d] bit for bit.  c is int32 [rows, heads], z is [rows, heads * dims].
 * A vector with a non-finite entry gets c = 0, and NaN in z where x is non-finite (e_0's values elsewhere).
 * k a multiple of 16 runs on the matrix cores (fp16 hi / lo operands, every vector of x behind its own power-of-two scale, e
 * behind one per call); every other k on the vector ALU.  Identical rows of e have identical score bits on either path.
 * No atomics; a vector's c and z depend on that vector and e alone.  Nothing of size [rows * heads, k] is written. */
int ddsp_vq_assign_f32(const float* x, const float* e, int* c, float* z, void* workspace, size_t workspace_bytes, int rows, int heads,
                       int k, int dims, void* stream);

/* counts[j] = #{(i, h): c[i, h] = j}; sums[j, d] = sum of x[i, h dims + d] over those (i, h), added in fp64 in ascending
 * (h, i) order and rounded once.  counts [k], sums [k, dims].  Entries of c outside [0, k) are counted nowhere.
 * No atomics: the same bits on every run. */
int ddsp_vq_statistics_f32(const float* x, const int* c, float* counts, float* sums, int rows, int heads, int k, int dims, void* stream);

#ifdef __cplusplus
}
#endif
#endif
