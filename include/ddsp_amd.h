/*
 * ddsp_amd.h — C ABI of the MI355X (gfx950) additive-synthesis hot path.
 *
 * The reference (magenta/ddsp) has no native code and no FFI: its boundary for this
 * path is the Python class API `ddsp.processors.Processor` (ddsp/processors.py:37-76)
 * as implemented by `ddsp.synths.Harmonic` (ddsp/synths.py:55-146),
 * `ddsp.synths.FilteredNoise` (ddsp/synths.py:149-196) and `ddsp.processors.Add`
 * (ddsp/processors.py:162-176).  The entry points below are what a binding for that
 * class API calls (see INTEGRATION.md for the ctypes stub a maintainer would add);
 * each one names the reference code it replaces.
 *
 * Conventions
 *   - every pointer is DEVICE memory owned by the caller, fp32, contiguous,
 *     row-major [batch, time, channel] exactly as the reference lays tensors out;
 *   - `stream` is a hipStream_t passed as void*; calls only enqueue work on it and
 *     never synchronise, allocate or free;
 *   - return value: DDSP_OK or a negative DDSP_ERR_* (programmer errors only; the
 *     reference's ValueErrors are raised by the host layer before the call);
 *   - `workspace` is caller-provided scratch of at least *_workspace_bytes() bytes,
 *     16-byte aligned, contents undefined on entry and exit.
 */
#ifndef DDSP_AMD_H_
#define DDSP_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DDSP_OK 0
#define DDSP_ERR_NULL_POINTER (-1)
#define DDSP_ERR_BAD_SHAPE (-2)
#define DDSP_ERR_UNSUPPORTED (-3)   /* shape outside what the kernels implement */
#define DDSP_ERR_WORKSPACE (-4)     /* workspace too small or misaligned */
#define DDSP_ERR_LAUNCH (-5)        /* hipGetLastError() != hipSuccess after a launch */

/* ---- flags for the Harmonic entry points (ddsp/synths.py:59-66 ctor kwargs) ------- */
#define DDSP_HARM_SCALE_EXP_SIGMOID 0x1u  /* scale_fn=core.exp_sigmoid (else scale_fn=None) */
#define DDSP_HARM_NORMALIZE_NYQUIST 0x2u  /* normalize_below_nyquist=True */
#define DDSP_HARM_AMP_LINEAR 0x4u         /* amp_resample_method='linear' (else 'window') */
#define DDSP_HARM_ANGULAR_CUMSUM 0x8u     /* use_angular_cumsum=True (phase) */
#define DDSP_HARM_NO_AUDIO_RATE_MASK 0x10u      /* internal to the streaming entry: no per-sample Nyquist mask */
#define DDSP_HARM_INPUTS_ARE_AMPLITUDES 0x20u   /* streaming entry: harmonic_distribution=None (core.py:1149-1150) */
#define DDSP_HARM_DIRECT_SUM 0x40u        /* ddsp_harmonic_f32: sum the harmonics sample by sample (sine recurrence on the
                                             vector ALUs) even where the matrix-core wavetable kernel applies */

/* ---- flags for the FilteredNoise entry points (ddsp/synths.py:153-163) ------------ */
#define DDSP_NOISE_SCALE_EXP_SIGMOID 0x1u /* scale_fn=core.exp_sigmoid on (mag + initial_bias) */
#define DDSP_NOISE_FIR_VECTOR_ALU 0x8u    /* ddsp_filtered_noise_f32, canonical filter (65 bands, full window, frames of 64 c samples):
                                             keep the time-varying FIR on the vector ALUs (noise_fused65_kernel) instead of the
                                             default matrix-core kernel (noise_mfma65_kernel: IR design and FIR as fp16 hi/lo-split
                                             MFMA products, fp32 accumulation) */
#define DDSP_NOISE_BITS_23 0x10u          /* generated noise (noise == NULL) with 23-bit samples - the 2^23 levels of the reference's
                                             tf.random.uniform (ddsp/synths.py:192-193) - instead of 2048 levels.  The Python mirror
                                             sets it by default since round 6 (FilteredNoise(noise_bits=23) is the class default;
                                             noise_bits=11 clears it); see ddsp_filtered_noise_f32.  The backward call
                                             takes the same flag so that it regenerates the same samples. */

/* Library / build identification: "ddsp_amd <version> gfx950". */
const char* ddsp_version(void);

/* No entry point of this library synchronises or allocates, with ONE exception: the constant operand tables of the
 * matrix-core kernels (the wavetable kernels' sine fragments per device; the general FilteredNoise / frequency_impulse_response
 * kernels' design matrix per device, band count and window size) are made on the host and copied to the device, synchronously,
 * the first time a shape needs them.  ddsp_prepare makes them NOW for the current device: call it before capturing a HIP graph
 * (a synchronous copy inside a capture is an error) or before a latency-critical first call.  n_harmonics <= 0 / n_noise_bands
 * < 2 skip their part; shapes whose kernels need no tables (more than 200 harmonics, the canonical 65-band filter with the
 * full window, whose tables are compile-time constants - it still has a design matrix for its backward pass) are no-ops. */
int ddsp_prepare(int n_harmonics, int n_noise_bands, int window_size);

/* ------------------------------------------------------------------------------------
 * Harmonic.get_controls  (ddsp/synths.py:94-121; core.exp_sigmoid core.py:386-404,
 * core.normalize_harmonics core.py:894-907, remove_above_nyquist core.py:869-891,
 * safe_divide core.py:207-210).
 *   amplitudes            [B,F,1]  in
 *   harmonic_distribution [B,F,K]  in
 *   f0_hz                 [B,F,1]  in
 *   ctl_amplitudes        [B,F,1]  out
 *   ctl_harmonic_distribution [B,F,K] out
 * flags: DDSP_HARM_SCALE_EXP_SIGMOID, DDSP_HARM_NORMALIZE_NYQUIST.
 */
int ddsp_harmonic_controls_f32(const float* amplitudes, const float* harmonic_distribution,
                               const float* f0_hz, float* ctl_amplitudes,
                               float* ctl_harmonic_distribution, int B, int F, int K,
                               int sample_rate, unsigned flags, void* stream);

/* ------------------------------------------------------------------------------------
 * Harmonic.get_signal  (ddsp/synths.py:123-146 -> core.harmonic_synthesis
 * core.py:1048-1111: get_harmonic_frequencies :1028-1045, resample 'linear' :573-642,
 * upsample_with_windows :645-714, oscillator_bank :912-962, angular_cumsum :800-866).
 * Inputs are CONTROLS (already scaled / normalised).  audio [B,N] out.
 * flags: DDSP_HARM_AMP_LINEAR, DDSP_HARM_ANGULAR_CUMSUM.
 * Requires N % F == 0 (the reference requires it for 'window'; DDSP_ERR_UNSUPPORTED
 * otherwise).
 */
size_t ddsp_harmonic_workspace_bytes(int B, int F, int K, int N);
int ddsp_harmonic_signal_f32(const float* ctl_amplitudes,
                             const float* ctl_harmonic_distribution, const float* f0_hz,
                             float* audio, void* workspace, size_t workspace_bytes, int B,
                             int F, int K, int N, int sample_rate, unsigned flags,
                             void* stream);

/* Validation-only variant of ddsp_harmonic_signal_f32 that follows the reference's fp32 op order
 * exactly, including the strictly sequential phase accumulation of tf.cumsum (ddsp/core.py:955)
 * or angular_cumsum (:800-866, chunk 1000).  One lane per (row, harmonic), serial in time: slow by
 * construction, used by the parity tests to compare full-length clips with the fp32-faithful
 * oracle.  flags: DDSP_HARM_AMP_LINEAR, DDSP_HARM_ANGULAR_CUMSUM.  audio [B,N] out. */
int ddsp_harmonic_signal_tf_order_f32(const float* ctl_amplitudes,
                                      const float* ctl_harmonic_distribution, const float* f0_hz,
                                      float* audio, int B, int F, int K, int N, int sample_rate,
                                      unsigned flags, void* stream);

/* ------------------------------------------------------------------------------------
 * Backward pass of ddsp_harmonic_f32 (inputs_are_controls = 0) / ddsp_harmonic_signal_f32
 * (inputs_are_controls = 1): the gradients tf.GradientTape forms through
 * ddsp/synths.py:94-146 in ddsp/training/trainers.py:162-171.
 *   grad_audio [B,N] in;  grad_amplitudes [B,F,1], grad_harmonic_distribution [B,F,K] out.
 * f0_hz is a constant of this call (its gradient is ddsp_harmonic_f0_grad_f32); the Nyquist masks
 * have zero gradient, as tf.where gives them.  flags as ddsp_harmonic_f32.  K <= 256, N/F <= 2048.
 * workspace: ddsp_harmonic_backward_workspace_bytes(B,F,K,N).
 */
size_t ddsp_harmonic_backward_workspace_bytes(int B, int F, int K, int N);
int ddsp_harmonic_backward_f32(const float* amplitudes, const float* harmonic_distribution,
                               const float* f0_hz, const float* grad_audio, float* grad_amplitudes,
                               float* grad_harmonic_distribution, void* workspace,
                               size_t workspace_bytes, int B, int F, int K, int N, int sample_rate,
                               unsigned flags, int inputs_are_controls, void* stream);
/* The frame-rate half of that backward pass on its own: dL/d (amplitudes * harmonic_distribution) [B,F,K] in
 * (core.harmonic_synthesis' product, ddsp/core.py:1097), through Harmonic.get_controls (exp_sigmoid, the frame-rate Nyquist
 * mask, safe_divide by the sum: ddsp/synths.py:94-121) to dL/d amplitudes [B,F,1] and dL/d harmonic_distribution [B,F,K].
 * With ddsp_oscillator_bank_grad_amplitudes_f32 and ddsp_resample_ex_backward_f32 the backward pass of the materialised
 * chain ('nearest' / 'cubic' envelopes, n_samples that is not a multiple of n_frames).  K <= 512. */
int ddsp_harmonic_controls_backward_f32(const float* amplitudes, const float* harmonic_distribution, const float* f0_hz,
                                        const float* grad_harmonic_amplitudes, float* grad_amplitudes,
                                        float* grad_harmonic_distribution, int B, int F, int K, int sample_rate,
                                        unsigned flags, int inputs_are_controls, void* stream);

/* ------------------------------------------------------------------------------------
 * core.streaming_harmonic_synthesis (ddsp/core.py:1114-1164) with harmonic_oscillator_bank
 * (core.py:966-1025, angular cumsum): one chunk of audio from frame-wise controls with the
 * fundamental's phase carried in and out (the VST model, ddsp/training/inference.py:446-472,
 * calls it with F = 2 frames per hop).
 *   amplitudes [B,F,1], harmonic_distribution [B,F,K] (normalised with the frame-rate Nyquist
 *   mask, core.py:1141-1148; with DDSP_HARM_INPUTS_ARE_AMPLITUDES the harmonic amplitudes are
 *   amplitudes * harmonic_distribution as given - pass ones [B,F,1] for the reference's
 *   harmonic_distribution=None), f0_hz [B,F,1],
 *   initial_phase [B] radians or NULL (= 0), audio [B,N] out, final_phase [B] out or NULL:
 *   (sum of omega mod 2 pi) + initial_phase, as the reference returns it.
 * There is no audio-rate Nyquist mask on this path (as in the reference).  N % F == 0.
 * flags: DDSP_HARM_AMP_LINEAR (amp_resample_method, default 'linear' in the reference),
 * DDSP_HARM_INPUTS_ARE_AMPLITUDES.  workspace: ddsp_harmonic_workspace_bytes(B,F,K,N).
 */
int ddsp_harmonic_streaming_f32(const float* amplitudes, const float* harmonic_distribution,
                                const float* f0_hz, const float* initial_phase, float* audio,
                                float* final_phase, void* workspace, size_t workspace_bytes,
                                int B, int F, int K, int N, int sample_rate, unsigned flags,
                                void* stream);

/* ------------------------------------------------------------------------------------
 * Harmonic.__call__  == get_signal(**get_controls(...))  (ddsp/processors.py:53-68),
 * fused: raw network outputs in, audio out, the [B,F,K] controls never round-trip
 * through fp32 HBM tensors unless the caller asks for them.
 *   ctl_amplitudes / ctl_harmonic_distribution: NULL, or out buffers that receive the
 *   controls dict (return_outputs_dict=True).
 * flags: all DDSP_HARM_*.
 */
int ddsp_harmonic_f32(const float* amplitudes, const float* harmonic_distribution,
                      const float* f0_hz, float* audio, float* ctl_amplitudes,
                      float* ctl_harmonic_distribution, void* workspace,
                      size_t workspace_bytes, int B, int F, int K, int N, int sample_rate,
                      unsigned flags, void* stream);

/* Harmonic.__call__ with the processors.Add that follows it fused in (ddsp/processors.py:162-176;
 * every shipped DAG ends Harmonic, FilteredNoise, Add: ddsp/training/gin/models/ae.gin:49-56):
 *   audio[B,N] = Harmonic(amplitudes, harmonic_distribution, f0_hz) + add_signal[B,N]
 * in one launch - one [B,N] stream written (14.44 instead of 18.44 bytes per sample for the
 * Harmonic + FilteredNoise + Add group).  add_signal may be `audio` itself.
 * Bit-identical to ddsp_harmonic_f32 followed by ddsp_add_f32.  Returns DDSP_ERR_UNSUPPORTED where
 * the wavetable kernel does not apply (hop % 64 != 0, K > 200, non-default flags): the caller
 * then uses the two separate entries. */
int ddsp_harmonic_add_f32(const float* amplitudes, const float* harmonic_distribution,
                          const float* f0_hz, const float* add_signal, float* audio, int B, int F,
                          int K, int N, int sample_rate, unsigned flags, void* stream);

/* ------------------------------------------------------------------------------------
 * FilteredNoise.get_controls  (ddsp/synths.py:165-179):
 *   ctl_magnitudes[B,F,M] = exp_sigmoid(magnitudes + initial_bias)   (or identity copy).
 */
int ddsp_filtered_noise_controls_f32(const float* magnitudes, float* ctl_magnitudes, int B,
                                     int F, int M, float initial_bias, unsigned flags,
                                     void* stream);

/* ------------------------------------------------------------------------------------
 * core.frequency_impulse_response  (ddsp/core.py:1534-1565 +
 * apply_window_to_impulse_response :1477-1531): ctl magnitudes [B,F,M] -> causal,
 * windowed FIR taps [B,F,L].  ddsp_fir_size() gives L for (M, window_size).
 */
int ddsp_fir_size(int M, int window_size);
/* core.apply_window_to_impulse_response (core.py:1477-1531) on its own, any response length: [rows, L0] zero-phase (causal != 0:
 * causal) responses -> [rows, ddsp_window_impulse_response_size(L0, window_size)] windowed causal ones. */
int ddsp_window_impulse_response_size(int L0, int window_size);
int ddsp_apply_window_to_impulse_response_f32(const float* impulse_response, float* out, long rows, int L0, int window_size,
                                              int causal, void* stream);
int ddsp_frequency_impulse_response_f32(const float* ctl_magnitudes, float* impulse_response,
                                        int B, int F, int M, int window_size, void* stream);

/* ------------------------------------------------------------------------------------
 * FilteredNoise.get_signal  (ddsp/synths.py:181-196 -> core.frequency_filter
 * core.py:1628-1655 -> fft_convolve :1382-1473, crop_and_compensate_delay :1338-1379).
 *   magnitudes [B,F,M]: raw (flags has DDSP_NOISE_SCALE_EXP_SIGMOID: get_controls is
 *                       fused in) or controls (flag clear: pure get_signal).
 *   noise      [B,N] or NULL.  NULL: uniform noise in (-1,1) is generated on chip, the
 *              stand-in for the reference's tf.random.uniform (synths.py:192-193), whose
 *              stateful stream cannot be reproduced outside TensorFlow.  The generator is
 *              Philox4x32-10 with key = (seed low word, seed high word) and counter
 *              (n >> 3, batch_offset + row, c2, 0) for sample n of a row; this library's
 *              contract (csrc/common.h; oracle/ddsp_oracle.py::device_uniform_noise
 *              restates both forms bit for bit):
 *                flag clear (11 bits, c2 = 0; FilteredNoise(noise_bits=11)): eight samples per block; sample n is the
 *                  11-bit field k = bits [10:0] (n even) or [26:16] (n odd) of word
 *                  (n >> 1) & 3, value (2 k - 2047) / 2048 - 2048 equally spaced levels,
 *                  zero mean, variance 1/3 to 2e-7, every value exactly an fp16 number
 *                  (the matrix-core FIR then needs no lo part for its noise operand);
 *                DDSP_NOISE_BITS_23 (c2 = 1 + ((n >> 2) & 1); what FilteredNoise() asks for by default): four samples per block;
 *                  sample n is word n & 3: its top 23 bits as the mantissa of u in [1,2),
 *                  value 2 u - 3 - the 2^23 levels TensorFlow's fp32 uniforms have.
 *              Non-NULL is the parity entry: the same maths as effects.FIRFilter
 *              (ddsp/effects.py:311-324) / core.frequency_filter on supplied audio, at
 *              any scale (it is normalised by a power of two before the fp16 hi/lo
 *              split of the matrix-core kernels and the outputs are scaled back).
 *   audio      [B,N] out.   ctl_magnitudes: NULL or [B,F,M] out (controls dict).
 * Frames: frame_size = ceil(N/F) and ceil(N/frame_size) must equal F (the reference's
 * ValueError, core.py:1451-1457) else DDSP_ERR_BAD_SHAPE.
 * Workspace: the taps [B,F,L] for the shapes that design them in a launch of their own,
 * plus - for filters that reach across more frames than a tiled kernel holds (510 taps
 * on frames of 5 samples: the plain sum of ddsp_fft_convolve_f32 takes those) - a row of
 * generated noise per clip; always ask ddsp_filtered_noise_workspace_bytes() with the
 * call's own (B, F, M, N, window_size).
 */
size_t ddsp_filtered_noise_workspace_bytes(int B, int F, int M, int N, int window_size);
int ddsp_filtered_noise_f32(const float* magnitudes, const float* noise, float* audio,
                            float* ctl_magnitudes, void* workspace, size_t workspace_bytes,
                            int B, int F, int M, int N, int window_size, float initial_bias,
                            unsigned flags, uint64_t seed, uint64_t batch_offset,
                            void* stream);

/* ------------------------------------------------------------------------------------
 * Backward pass of ddsp_filtered_noise_f32: dL/d magnitudes [B,F,M] from grad_audio [B,N]
 * (the gradient tf.GradientTape forms through ddsp/synths.py:165-196).  `noise` as in the forward
 * call: the tensor that was supplied, or NULL with the same seed / batch_offset so that the noise is
 * regenerated.  Any band count / window (M = 65 with the full window has its own fast kernel).
 * workspace: ddsp_filtered_noise_backward_workspace_bytes.
 */
size_t ddsp_filtered_noise_backward_workspace_bytes(int B, int F, int M, int N);
int ddsp_filtered_noise_backward_f32(const float* magnitudes, const float* noise,
                                     const float* grad_audio, float* grad_magnitudes,
                                     void* workspace, size_t workspace_bytes, int B, int F, int M,
                                     int N, int window_size, float initial_bias, unsigned flags,
                                     uint64_t seed, uint64_t batch_offset, void* stream);

/* ------------------------------------------------------------------------------------
 * core.fft_convolve(audio, impulse_response, padding='same', delay_compensation)
 * (ddsp/core.py:1382-1473) evaluated as the equivalent direct time-varying FIR.
 *   audio [B,N], impulse_response [Bir,F,L] with Bir == B or Bir == 1 (broadcast,
 *   core.py:1433-1434), out [B,N].  delay_compensation < 0 selects (L-1)/2 - 1.
 */
int ddsp_fft_convolve_same_f32(const float* audio, const float* impulse_response, float* out,
                               int B, int Bir, int F, int L, int N, int delay_compensation,
                               void* stream);

/* ------------------------------------------------------------------------------------
 * Long single-frame convolution: effects.Reverb.get_signal (ddsp/effects.py:100-117) and
 * core.fft_convolve (ddsp/core.py:1382-1473) with a 2-D impulse response (one frame,
 * core.py:1428-1430), padding='same':
 *     out[b][n] = sum_k ir[b][k] * audio[b][n + delay - k]   (+ audio[b][n] with ADD_DRY),
 * i.e. crop_and_compensate_delay (core.py:1338-1379) with start = delay >= 0
 * (Reverb passes delay_compensation=0).  ir [Bir,L], Bir == B or 1 (tiled over the batch,
 * effects.py:62-69 / core.py:1433-1434).  DDSP_CONV_MASK_TAP0 zeroes tap 0 as
 * Reverb._mask_dry_ir does (effects.py:50-60).  Evaluated as a partitioned overlap-save FFT
 * convolution with LDS-resident 8192-point FFTs; any L < 2^28 (up to 16 partitions of 4096 taps stay in a
 * register window of the multiply-add pass; beyond - vst_48k.gin's 72 000 taps - a plain pass re-reads them).
 * workspace: ddsp_fft_convolve_long_workspace_bytes(...) bytes, 16-byte aligned.
 */
#define DDSP_CONV_ADD_DRY 1u
#define DDSP_CONV_MASK_TAP0 2u
#define DDSP_CONV_REVERSE_AUDIO 4u   /* _ex only: logical audio sample g is stored at N-1-g   */
#define DDSP_CONV_REVERSE_IR 8u      /* _ex only: logical tap k is stored at L-1-k            */
#define DDSP_CONV_REVERSE_OUT 16u    /* _ex only: logical output n is written to n_out-1-n    */
#define DDSP_CONV_ZERO_OUT0 32u      /* _ex only: logical output 0 is written as 0 (dL/d ir: the masked dry tap has no gradient) */
size_t ddsp_fft_convolve_long_workspace_bytes(int B, int Bir, int N, int L, int delay);
int ddsp_fft_convolve_long_f32(const float* audio, const float* impulse_response, float* out,
                               void* workspace, size_t workspace_bytes, int B, int Bir, int N,
                               int L, int delay, unsigned flags, void* stream);
/* The same convolution with n_out outputs per row (out [B,n_out], out[b][n] = y[n + delay] of the
 * full linear convolution y) and optional index reversal of either input or of the output: the two
 * correlations of the Reverb backward pass are
 *   dL/d audio = reverse( conv(reverse(g), ir)[0:N] )           (REVERSE_AUDIO | REVERSE_OUT)
 *   dL/d ir[k] = conv(g, reverse(audio))[N-1+k], k < L          (REVERSE_IR on the audio passed as "ir",
 *                                                                 n_out = L, delay = N-1)
 * The "impulse response" of a call may be any length below 2^28.  ADD_DRY needs n_out == N. */
size_t ddsp_fft_convolve_long_ex_workspace_bytes(int B, int Bir, int N, int L, int n_out, int delay);
int ddsp_fft_convolve_long_ex_f32(const float* audio, const float* impulse_response, float* out,
                                  void* workspace, size_t workspace_bytes, int B, int Bir, int N,
                                  int L, int n_out, int delay, unsigned flags, void* stream);
/* out[l] = sum_b x[b][l] (row 0 first: a fixed order), out[0] = 0 when zero_first: what collects dL/d ir of a Reverb whose one
 * impulse response serves the whole batch (ddsp/effects.py:62-80; the dry tap is masked, :50-60) from the rows' correlations. */
int ddsp_sum_rows_f32(const float* x, float* out, int B, int L, int zero_first, void* stream);

/* ------------------------------------------------------------------------------------
 * losses.SpectralLoss.call, forward pass (ddsp/losses.py:189-243), loss_type 'L1', magnitude and
 * log-magnitude terms:
 *     *loss = sum over fft_sizes of  mag_weight * mean|mag_t - mag_a| + logmag_weight * mean|safe_log mag_t - safe_log mag_a|
 * with mag = |tf.signal.stft(frame_length=S, frame_step=S/4, pad_end=True)| (spectral_ops.py:34-47,
 * 67-70), safe_log per core.py:213-216.  target_audio, audio [B,N] and loss (one float) are device
 * pointers; fft_sizes is a HOST array of n_sizes (<= 16) frame sizes: powers of two in [16, 8192] or (round 6) 3 * 2^k in [48, 6144] -
 * gin/models/vst/vst_48k.gin:56 -, frames of 4 hops zero-padded to the 4 F / 3 points tf.signal.stft transforms (S / 2 + 1 bins).
 * workspace: ddsp_spectral_loss_workspace_bytes(...) bytes (per-block fp64 partial sums; the
 * result does not depend on scheduling).
 */
size_t ddsp_spectral_loss_workspace_bytes(int B, int N, const int* fft_sizes, int n_sizes);
int ddsp_spectral_loss_f32(const float* target_audio, const float* audio, float* loss,
                           void* workspace, size_t workspace_bytes, int B, int N,
                           const int* fft_sizes, int n_sizes, float mag_weight,
                           float logmag_weight, void* stream);

/* Backward pass of ddsp_spectral_loss_f32 with respect to `audio`: grad_audio [B,N] (overwritten)
 * = grad_loss[0] * dL/d audio, grad_loss a device pointer to one float.  |z| has gradient z/|z|
 * (0 at 0), safe_log passes a gradient only where its argument is positive.  Overlapping frames
 * add with fp32 atomics: the last bit may differ between runs. */
int ddsp_spectral_loss_backward_f32(const float* target_audio, const float* audio,
                                    const float* grad_loss, float* grad_audio, int B, int N,
                                    const int* fft_sizes, int n_sizes, float mag_weight,
                                    float logmag_weight, void* stream);

/* Loss value and dL/d audio (for dL/dloss = 1) in one pass: the frame spectra are computed once
 * for both, which is how a training step calls it (the caller scales grad_audio by the upstream
 * gradient).  loss: one float; workspace as ddsp_spectral_loss_f32. */
int ddsp_spectral_loss_value_and_grad_f32(const float* target_audio, const float* audio, float* loss,
                                          float* grad_audio, void* workspace,
                                          size_t workspace_bytes, int B, int N,
                                          const int* fft_sizes, int n_sizes, float mag_weight,
                                          float logmag_weight, void* stream);

/* The same gradient, bit-reproducible (opt-in): run to run, whatever else runs on the chip, and for a row whatever the other rows
 * hold (a row's gradient depends on that row's data and on B alone).  No float atomics: every block stores its stretch of
 * overlap-added samples to a slab of its own in grad_workspace, and a second, stream-ordered kernel writes each grad_audio[b][n]
 * once, as the sum in this order:  g = 0;  for each entry of fft_sizes IN THE ORDER LISTED, g += (t = 0; t += the value of each
 * block of that size that covers sample n, in ascending block index);  fp32 throughout.  (ddsp_stft_mag_backward_det_f32 and
 * ddsp_stft_frames_mag_backward_det_f32 below add one scale in the same way: grad_audio[b][n] = grad_audio[b][n] + t - a loss
 * built from them scale after scale, the loudness term last, follows the same contract.)
 * grad_workspace: ddsp_spectral_loss_grad_workspace_bytes(...) bytes, 16-byte aligned = 4 B sum over sizes of (blocks per row x
 * floats per block): a block takes G = max(1, 4096 / S) frames of hop F / 4 (S: the transform's size) and holds (G + 3) F / 4
 * floats; transforms of 8192 points take one frame per block and hold F floats.  73 930 752 bytes at B = 32, N = 64 000 and the
 * six default sizes.  0 where ddsp_spectral_loss_workspace_bytes returns 0.  A NULL grad_workspace is DDSP_ERR_NULL_POINTER, a
 * short or misaligned one DDSP_ERR_WORKSPACE; the other arguments as in the two functions above. */
size_t ddsp_spectral_loss_grad_workspace_bytes(int B, int N, const int* fft_sizes, int n_sizes);
int ddsp_spectral_loss_backward_det_f32(const float* target_audio, const float* audio, const float* grad_loss,
                                        float* grad_audio, int B, int N, const int* fft_sizes, int n_sizes,
                                        float mag_weight, float logmag_weight, void* grad_workspace,
                                        size_t grad_workspace_bytes, void* stream);
int ddsp_spectral_loss_value_and_grad_det_f32(const float* target_audio, const float* audio, float* loss,
                                              float* grad_audio, void* workspace, size_t workspace_bytes, int B, int N,
                                              const int* fft_sizes, int n_sizes, float mag_weight,
                                              float logmag_weight, void* grad_workspace, size_t grad_workspace_bytes,
                                              void* stream);

/* ---- the general form of losses.SpectralLoss (ddsp/losses.py:131-243): every term, loss_type and the weights mask ----
 * The 'L1' mag + logmag loss of the shipped configs is ddsp_spectral_loss_f32 above (spectra stay in LDS).  These three
 * entries serve the rest of the reference's argument space on spectrograms materialised in HBM, one FFT size at a time:
 *
 * ddsp_stft_mag_f32: spectral_ops.compute_mag (ddsp/spectral_ops.py:67-70; tf.signal.stft: frames of fft_size every
 *   fft_size/4, zero pad_end, periodic Hann) of two signals at once: target_mag, mag [B, frames, fft_size/2+1],
 *   frames = ceil(N / (fft_size/4)).
 * ddsp_spectral_terms_f32: for one FFT size, adds
 *     mag_weight * D(T, V) + delta_time_weight * D(diff_t T, diff_t V) + delta_freq_weight * D(diff_f T, diff_f V)
 *     + cumsum_freq_weight * D(cumsum_f T, cumsum_f V) + logmag_weight * D(safe_log T, safe_log V)
 *   to *loss_accumulator (fp64, device; `first` != 0 starts it at 0) and rewrites *loss (fp32) with the running total;
 *   D = losses.mean_difference (ddsp/losses.py:102-128) with loss_type DDSP_LOSS_L1 / _L2 / _COSINE and the optional
 *   `weights` mask of shape [weights_b, weights_f, weights_k] (each extent 1 or the term's; NULL: no mask).  Terms
 *   with weight <= 0 are skipped, as in the reference.  grad_value_mag (may be NULL) [B, frames, bins] receives
 *   d(this size's contribution)/dV.  Deterministic (fixed-order fp64 sums).
 * ddsp_stft_mag_backward_f32: grad_audio [B,N] += d|STFT(audio)|^T grad_mag  (|z| has gradient z/|z|, 0 at 0). */
#define DDSP_LOSS_L1 0
#define DDSP_LOSS_L2 1
#define DDSP_LOSS_COSINE 2
int ddsp_stft_mag_f32(const float* target_audio, const float* audio, float* target_mag, float* mag, int B, int N,
                      int fft_size, void* stream);
size_t ddsp_spectral_terms_workspace_bytes(int B, int frames);
int ddsp_spectral_terms_f32(const float* target_mag, const float* value_mag, const float* weights, int weights_b,
                            int weights_f, int weights_k, float* grad_value_mag, double* loss_accumulator, float* loss,
                            void* workspace, size_t workspace_bytes, int B, int frames, int bins, int loss_type,
                            float mag_weight, float delta_time_weight, float delta_freq_weight,
                            float cumsum_freq_weight, float logmag_weight, int first, void* stream);
int ddsp_stft_mag_backward_f32(const float* audio, const float* grad_mag, float* grad_audio, int B, int N, int fft_size,
                               void* stream);
/* ..._det: the same sum without float atomics (slabs in `workspace` + a gather; the order is stated at
 * ddsp_spectral_loss_grad_workspace_bytes): grad_audio[b][n] = grad_audio[b][n] + (this scale's covering blocks, ascending), a
 * plain read-modify-write.  workspace: ..._workspace_bytes(...) bytes (0: a size the call refuses), 16-byte aligned; NULL is
 * DDSP_ERR_NULL_POINTER, short or misaligned DDSP_ERR_WORKSPACE. */
size_t ddsp_stft_mag_backward_workspace_bytes(int B, int N, int fft_size);
int ddsp_stft_mag_backward_det_f32(const float* audio, const float* grad_mag, float* grad_audio, void* workspace,
                                   size_t workspace_bytes, int B, int N, int fft_size, void* stream);
/* fft_size of the two calls above: a power of two in [16, 8192], or any other EVEN frame size in [34, 8190] (gin/models/vst/
 * vst_48k.gin:56 asks for 6144, 3072 .. 192; any since round 6) - tf.signal.stft then transforms the enclosing power of two S,
 * the frame zero-padded, every int(fft_size / 4) samples: bins = S / 2 + 1.
 *
 * The loudness term of SpectralLoss (ddsp/losses.py:238-242 -> spectral_ops.compute_loudness, spectral_ops.py:253-324), in the
 * same materialised form.  ddsp_stft_frames_mag_f32: |STFT| of ONE signal under the caller's frame geometry - frames of
 * fft_size samples (a power of two in [64, 8192]) every `hop`, the first starting pad_left samples before sample 0 (zeros
 * outside the row; compute_loudness: fft_size 2048, hop sample_rate / 250, pad_left 1024, n_frames 1 + N / hop), periodic Hann
 * -> mag [B, n_frames, fft_size/2+1]; ..._backward: grad_audio += its adjoint applied to grad_mag (overlapping frames are
 * added with fp32 atomics: the LAST BITS of this gradient - and of ddsp_stft_mag_backward_f32's for frames of 3 * 2^k samples,
 * and of ddsp_spectral_loss_backward_f32's - depend on the order the frames arrive in; every FORWARD entry point, and the synths'
 * backward passes, are bit-reproducible run to run).
 * ddsp_loudness_from_mag_f32 (weighting: `bins` entries, caller-checked - the Python mirror refuses an n_fft whose spectrogram has
 * another bin count): loudness [B, n_frames] = max(10 log10(max(pmin, mean_k weighting[k] mag[k]^2)) - ref_db, -range_db),
 * pmin = 10^(-range_db/10) (core.power_to_db, core.py:253-267); `weighting` [bins] = 10^(A_weighting/10), made by the caller
 * (librosa's published A-curve: oracle/ddsp_oracle.py::a_weighting_db).  ..._backward: grad_mag [B, n_frames, bins]. */
int ddsp_stft_frames_mag_f32(const float* audio, float* mag, int B, int N, int fft_size, int hop, int pad_left, int n_frames,
                             void* stream);
/* spectral_ops.stft (ddsp/spectral_ops.py:34-47: tf.signal.stft, fft_length=None) - the complex spectrum itself under the same
 * geometry: frames of frame_size samples (even, <= fft_size; periodic Hann of frame_size) zero-padded to fft_size, a power of two
 * in [64, 8192].  spectrum: [B, n_frames, fft_size/2 + 1] pairs (re, im), fp32.  Forward only. */
int ddsp_stft_frames_f32(const float* audio, float* spectrum, int B, int N, int fft_size, int frame_size, int hop, int pad_left,
                         int n_frames, void* stream);
/* ddsp_stft_frames_mag_f32 for frames shorter than the transform (spectral_ops.compute_mag at any even size: frame_size samples
 * under a periodic Hann of frame_size, zero-padded to fft_size).  Forward only. */
int ddsp_stft_frames_mag_ex_f32(const float* audio, float* mag, int B, int N, int fft_size, int frame_size, int hop, int pad_left,
                                int n_frames, void* stream);
int ddsp_stft_frames_mag_backward_f32(const float* audio, const float* grad_mag, float* grad_audio, int B, int N, int fft_size,
                                      int hop, int pad_left, int n_frames, void* stream);
/* ..._det: as ddsp_stft_mag_backward_det_f32, under the caller's frame geometry (a block of G = 8192 / fft_size frames holds
 * (G - 1) hop + fft_size floats; the loudness geometry has up to nine covering blocks per sample). */
size_t ddsp_stft_frames_mag_backward_workspace_bytes(int B, int N, int fft_size, int hop, int pad_left, int n_frames);
int ddsp_stft_frames_mag_backward_det_f32(const float* audio, const float* grad_mag, float* grad_audio, void* workspace,
                                          size_t workspace_bytes, int B, int N, int fft_size, int hop, int pad_left, int n_frames,
                                          void* stream);
/* spectral_ops.compute_mel / compute_logmel / compute_mfcc (ddsp/spectral_ops.py:73-133) under the frame geometry of
 * ddsp_stft_frames_mag_ex_f32, in one kernel: the magnitudes stay on chip, only out [B, n_frames, bins] (DDSP_MEL_LINEAR: the mel
 * spectrogram; DDSP_MEL_LOG: log(where(mel <= 0, eps, mel))) or [B, n_frames, mfcc_bins] (DDSP_MEL_MFCC: the first mfcc_bins
 * coefficients of the scaled DCT-II of the log-mel values) is written.  The mel matrix travels by its bands: bands [3][bins]
 * int32 - first spectrogram bin, number of bins, index of the band's first weight in `weights` (n_weights floats; a band of
 * no bins is an all-zero column); dct_t [bins][mfcc_bins] is the DCT table, TRANSPOSED (DDSP_MEL_MFCC only, else may be null).
 * Limits (DDSP_ERR_UNSUPPORTED beyond): bins <= fft_size, mfcc_bins <= bins.  Forward only; bit-reproducible. */
#define DDSP_MEL_LINEAR 0
#define DDSP_MEL_LOG 1
#define DDSP_MEL_MFCC 2
int ddsp_mel_features_f32(const float* audio, const int* bands, const float* weights, const float* dct_t, float* out, int B, int N,
                          int fft_size, int frame_size, int hop, int pad_left, int n_frames, int bins, int mfcc_bins,
                          int n_weights, int mode, float eps, void* stream);
/* spectral_ops.compute_rms_energy / compute_power (ddsp/spectral_ops.py:223-249): frames of frame_size samples (any size >= 1)
 * every `hop`, the first pad_left samples before sample 0, zeros outside the row -> out [B, n_frames]: sqrt(mean x^2), or with
 * DDSP_ENERGY_DB core.amplitude_to_db of it, max(10 log10(max(pmin, rms^2)) - ref_db, -range_db), pmin = 10^(-range_db / 10). */
#define DDSP_ENERGY_DB 0x1u
int ddsp_frame_energy_f32(const float* audio, float* out, int B, int N, int frame_size, int hop, int pad_left, int n_frames,
                          float ref_db, float range_db, unsigned flags, void* stream);
/* core.power_to_db / amplitude_to_db (p0 = ref_db, p1 = range_db) / db_to_power / db_to_amplitude (ddsp/core.py:247-277) on n
 * values. */
#define DDSP_DB_POWER_TO_DB 0
#define DDSP_DB_AMPLITUDE_TO_DB 1
#define DDSP_DB_TO_POWER 2
#define DDSP_DB_TO_AMPLITUDE 3
int ddsp_db_convert_f32(const float* in, float* out, size_t n, int op, float p0, float p1, void* stream);
int ddsp_loudness_from_mag_f32(const float* mag, const float* weighting, float* loudness, int B, int n_frames, int bins,
                               float range_db, float ref_db, void* stream);
int ddsp_loudness_from_mag_backward_f32(const float* mag, const float* weighting, const float* grad_loudness, float* grad_mag,
                                        int B, int n_frames, int bins, float range_db, float ref_db, void* stream);

/* Uniform noise exactly as ddsp_filtered_noise_f32 generates it (noise==NULL). out [B,N].
 * _ex: noise_bits = 11 (the flag-clear form, what ddsp_uniform_noise_f32 makes) or 23 (DDSP_NOISE_BITS_23's: the Python
 * mirror's default). */
int ddsp_uniform_noise_f32(float* out, int B, int N, uint64_t seed, uint64_t batch_offset,
                           void* stream);
int ddsp_uniform_noise_ex_f32(float* out, int B, int N, uint64_t seed, uint64_t batch_offset,
                              int noise_bits, void* stream);

/* processors.Add.get_signal (ddsp/processors.py:174-176): out = a + b, n elements. */
int ddsp_add_f32(const float* signal_one, const float* signal_two, float* out, size_t n,
                 void* stream);

/* core.oscillator_bank (ddsp/core.py:912-962) on materialised audio-rate envelopes [B,N,K]:
 * Nyquist mask, phase = inclusive cumsum over time of 2*pi*f/sr, sum_k A_k sin(phase_k).
 * out is [B,N] (sum_sinusoids != 0) or [B,N,K].  The phase scan runs in fp64 revolutions.
 * (synths.Harmonic never materialises these tensors; this entry serves direct callers.) */
size_t ddsp_oscillator_bank_workspace_bytes(int B, int N, int K);
int ddsp_oscillator_bank_f32(const float* frequency_envelopes, const float* amplitude_envelopes,
                             float* out, void* workspace, size_t workspace_bytes, int B, int N,
                             int K, int sample_rate, int sum_sinusoids, void* stream);
/* dL/d amplitude_envelopes [B,N,K] of ddsp_oscillator_bank_f32 given dL/d audio [B,N]: grad_audio[n] where the frequency is
 * below Nyquist, times sin(phase[n,k]) (the output is linear in the amplitudes).  Workspace as the forward's. */
int ddsp_oscillator_bank_grad_amplitudes_f32(const float* frequency_envelopes, const float* grad_audio,
                                             float* grad_amplitude_envelopes, void* workspace, size_t workspace_bytes,
                                             int B, int N, int K, int sample_rate, void* stream);
/* dL/d frequency_envelopes [B,N,K]: phase[n] = (2 pi / sr) sum_{t <= n} f[t] (ddsp/core.py:950-955), so
 * dL/d f[t,k] = (2 pi / sr) sum_{n >= t} grad_audio[n] A[n,k] mask[n,k] cos(phase[n,k]) (the Nyquist mask, tf.where, passes none).
 * Workspace: TWICE ddsp_oscillator_bank_workspace_bytes. */
int ddsp_oscillator_bank_grad_frequencies_f32(const float* frequency_envelopes, const float* amplitude_envelopes,
                                              const float* grad_audio, float* grad_frequency_envelopes, void* workspace,
                                              size_t workspace_bytes, int B, int N, int K, int sample_rate, void* stream);
/* dL/d f0_hz [B,F,1] from dL/d harmonic_frequencies [B,F,K] (= f0 [1..K] (1 + harmonic_shifts), ddsp/core.py:1086-1090;
 * harmonic_shifts may be NULL). */
int ddsp_harmonic_frequencies_backward_f32(const float* grad_harmonic_frequencies, const float* harmonic_shifts,
                                           float* grad_f0_hz, int B, int F, int K, void* stream);

/* core.resample (ddsp/core.py:573-642) for [B,F,C] -> [B,N,C], add_endpoint=True:
 *   window == 0: method='linear' (tf.compat.v1.image.resize BILINEAR, align_corners=False);
 *   window == 1: method='window' (core.upsample_with_windows :645-714); needs N % F == 0.
 * The synth kernels evaluate these envelopes on the fly; this entry is for direct callers. */
int ddsp_resample_f32(const float* x, float* out, int B, int F, int N, int C, int window,
                      void* stream);

/* core.resample (ddsp/core.py:573-642), the whole argument space: [B,F,C] -> [B,N,C] (a 4-D input
 * [B,F,n_freq,C] is the same call with C = n_freq*C: the width axis is resized 1:1), up- or down-sampling.
 *   method: DDSP_RESAMPLE_NEAREST / _LINEAR / _CUBIC = tf.compat.v1.image.resize NEAREST_NEIGHBOR / BILINEAR /
 *           BICUBIC (legacy kernels: no half-pixel centres, align_corners = !add_endpoint; bicubic with the
 *           1024-entry A = -0.75 table and clamped indices); DDSP_RESAMPLE_WINDOW = core.upsample_with_windows
 *           (:645-714; upsampling only, N divisible by F, or by F-1 when add_endpoint == 0, else
 *           DDSP_ERR_BAD_SHAPE - the reference's ValueErrors are raised by the host layer first).
 * (ddsp/csrc/general.hip) */
#define DDSP_RESAMPLE_NEAREST 0
#define DDSP_RESAMPLE_LINEAR 1
#define DDSP_RESAMPLE_CUBIC 2
#define DDSP_RESAMPLE_WINDOW 3
int ddsp_resample_ex_f32(const float* x, float* out, int B, int F, int N, int C, int method,
                         int add_endpoint, void* stream);
/* Its adjoint - what tf.GradientTape forms through core.resample (ddsp/training/trainers.py:162-171): grad_out [B,N,C] ->
 * grad_in [B,F,C], grad_in[j] = sum_t W[t][j] grad_out[t] with the forward's own fp32 positions, clamped indices and
 * weights; gathered per frame (no atomics: deterministic).  (csrc/general.hip) */
int ddsp_resample_ex_backward_f32(const float* grad_out, float* grad_in, int B, int F, int N, int C, int method,
                                  int add_endpoint, void* stream);

/* core.fft_convolve (ddsp/core.py:1382-1473) with any crop (crop_and_compensate_delay :1338-1379):
 *     out[b][n] = z[b][n + start],  n < n_out,   z[m] = sum_i audio[i] * ir[frame(i)][m - i]
 * (z = the overlap-added framed FFT products = the direct time-varying FIR; zero beyond its support).
 * padding='valid' is n_out = L + N - 1, 'same' is n_out = N; start = delay_compensation, or
 * (L-1)/2 - 1 when that is negative.  audio [B,N], impulse_response [Bir,F,L] with Bir == B or 1,
 * out [B,n_out].  frame_size = ceil(N/F) and ceil(N/frame_size) must equal F (DDSP_ERR_BAD_SHAPE).
 * General shapes, one thread per output; ddsp_fft_convolve_same_f32 is the fast entry for 'same'. */
int ddsp_fft_convolve_f32(const float* audio, const float* impulse_response, float* out, int B, int Bir,
                          int F, int L, int N, int n_out, int start, void* stream);

/* The adjoint of ddsp_fft_convolve_f32 (what tf.GradientTape forms through core.fft_convolve, ddsp/core.py:1382-1473, and
 * crop_and_compensate_delay, :1338-1379; effects.FIRFilter, ddsp/effects.py:283-324, trains through it).  With
 * frame(i) = i / frame_size, frame_size = ceil(N/F), and grad_out [B,n_out] = dL/d out (terms whose grad_out index leaves
 * [0, n_out) drop):
 *     grad_audio[b][i]               = sum_k ir[b or 0][frame(i)][k] * grad_out[b][i + k - start]
 *     grad_impulse_response[b][f][k] = sum_{i in frame f} audio[b][i] * grad_out[b][i + k - start]
 * impulse_response [Bir,F,L], Bir == B or 1; grad_audio [B,N]; grad_impulse_response [B,F,L] - one per row: for a
 * broadcast response (Bir == 1) add the rows with ddsp_sum_rows_f32(x, out, B, F*L, 0).  Any (F, L, N, n_out, start >= 0):
 * grad_audio runs a kernel with the taps of a tile's frames in LDS, or one thread per sample where those do not fit.
 * No atomics, fixed summation order: the same bits on every call.  B > 65535 (grad_ir also F > 65535): DDSP_ERR_UNSUPPORTED.
 * (csrc/fir_grad.hip) */
int ddsp_fft_convolve_grad_audio_f32(const float* grad_out, const float* impulse_response, float* grad_audio, int B, int Bir,
                                     int F, int L, int N, int n_out, int start, void* stream);
int ddsp_fft_convolve_grad_ir_f32(const float* grad_out, const float* audio, float* grad_impulse_response, int B, int F, int L,
                                  int N, int n_out, int start, void* stream);

/* core.sinc_impulse_response (ddsp/core.py:1576-1625; core.sinc :1568-1573): cutoff_frequency [rows] (the reference's
 * [B,T,1]) -> impulse_response [rows, L], L = ddsp_sinc_impulse_response_size(window_size) = 2 (window_size / 2) + 1:
 *     c = cutoff * 2 / sample_rate (sample_rate > 0; sample_rate == 0 is the reference's None: c = cutoff),
 *     x_j = c (j - half), |x_j| < 1e-20 replaced by 1e-20;  s_j = sin(pi x_j) / (pi x_j);
 *     w_j = 0.54 - 0.46 cos(2 pi j / (L - 1))   (tf.signal.hamming_window(L): L is odd, and TensorFlow's windows of odd
 *           length divide by L - 1 whether periodic or not; L == 1: [1.0]);
 *     h_j = w_j s_j / |sum_j w_j s_j|;   high_pass != 0: h_j <- delta(j, half) - h_j.
 * _backward: grad_impulse_response [rows, L] -> grad_cutoff_frequency [rows], through the quotient, the abs (the sign of
 * the sum) and the high-pass negation; its sums run in fp64 in a fixed order.  (csrc/fir_grad.hip) */
int ddsp_sinc_f32(const float* in, float* out, size_t n, float threshold, void* stream);   /* core.sinc on n values */
int ddsp_sinc_impulse_response_size(int window_size);
int ddsp_sinc_impulse_response_f32(const float* cutoff_frequency, float* impulse_response, size_t rows, int window_size,
                                   float sample_rate, int high_pass, void* stream);
int ddsp_sinc_impulse_response_backward_f32(const float* cutoff_frequency, const float* grad_impulse_response,
                                            float* grad_cutoff_frequency, size_t rows, int window_size, float sample_rate,
                                            int high_pass, void* stream);

/* The adjoint of ddsp_frequency_impulse_response_f32 (core.frequency_impulse_response, ddsp/core.py:1534-1565), which is
 * linear in the magnitudes: grad_magnitudes[r][m] = sum_k design[k][m] * grad_impulse_response[r][k], with design [L,M] =
 * the impulse responses of the M unit magnitude vectors, transposed.  L <= 12288, else DDSP_ERR_UNSUPPORTED.
 * (csrc/fir_grad.hip) */
int ddsp_frequency_impulse_response_backward_f32(const float* grad_impulse_response, const float* design, float* grad_magnitudes,
                                                 size_t rows, int M, int L, void* stream);

/* The adjoint of ddsp_exp_sigmoid_f32: grad_in = grad_out * log(exponent) * (y - threshold) * (1 - sigmoid(in)), elementwise. */
int ddsp_exp_sigmoid_backward_f32(const float* in, const float* grad_out, float* grad_in, size_t n, float exponent,
                                  float max_value, float threshold, void* stream);

/* out[i] = x[i] * scale[0] (scale: one float in device memory): the upstream scalar of a loss's backward pass applied
 * to a stored gradient - the chain rule tf.GradientTape applies through SpectralLoss (ddsp/training/trainers.py:162-171). */
int ddsp_scale_f32(const float* x, const float* scale, float* out, size_t n, void* stream);

/* core.harmonic_oscillator_bank (ddsp/core.py:966-1025) on audio-rate inputs: frequency [B,N,1] (one fundamental per clip),
 * amplitude_envelopes [B,N,K], initial_phase [B] radians or NULL -> audio [B,N] = sum_k A[n,k] sin((k+1) phase[n]),
 * phase = cumsum(2 pi f / sr) + initial_phase, and final_phase [B] = phase[N-1] (use_angular_cumsum != 0: the scan's
 * part wrapped to [0, 2 pi) as core.angular_cumsum leaves it, ddsp/core.py:800-866).  No Nyquist mask, as in the
 * reference.  The phase scan runs in fp64 revolutions.  Caller: core.streaming_harmonic_synthesis with envelopes
 * the closed-form kernel does not take, ddsp/training/inference.py:446-472 through it. */
size_t ddsp_harmonic_oscillator_bank_workspace_bytes(int B, int N);
int ddsp_harmonic_oscillator_bank_f32(const float* frequency, const float* amplitude_envelopes,
                                      const float* initial_phase, float* audio, float* final_phase,
                                      void* workspace, size_t workspace_bytes, int B, int N, int K,
                                      int sample_rate, int use_angular_cumsum, void* stream);

/* The frame-rate tensors core.harmonic_synthesis builds before resampling (ddsp/core.py:1080-1098,
 * get_harmonic_frequencies :1028-1045), fp32 in the reference's op order:
 *   harmonic_frequencies[B,F,K] = (f0_hz * (k+1)) * (1 + harmonic_shifts)      (shifts may be NULL)
 *   harmonic_amplitudes [B,F,K] = amplitudes * harmonic_distribution           (distribution NULL: amplitudes)
 * Used for the arguments the fused kernels do not take (harmonic_shifts, amp_resample_method 'nearest' /
 * 'cubic'): the host layer then follows the reference's own chain resample -> oscillator_bank on these. */
int ddsp_harmonic_envelopes_f32(const float* amplitudes, const float* harmonic_distribution,
                                const float* f0_hz, const float* harmonic_shifts,
                                float* harmonic_frequencies, float* harmonic_amplitudes, int B, int F,
                                int K, void* stream);

/* dL/d f0_hz [B,F,1] of Harmonic given grad_audio [B,N]: the gradient tf.GradientTape forms through
 * tf.cumsum and tf.sin (ddsp/core.py:950-960) and the bilinear resize of the frequencies (:1101).  Inputs
 * are the CONTROLS (ddsp_harmonic_controls_f32 / get_controls outputs) and f0_hz; the Nyquist masks have
 * zero gradient.  flags: DDSP_HARM_AMP_LINEAR.  N % F == 0.  workspace:
 * ddsp_harmonic_f0_grad_workspace_bytes(B,F,K,N). */
size_t ddsp_harmonic_f0_grad_workspace_bytes(int B, int F, int K, int N);
int ddsp_harmonic_f0_grad_f32(const float* ctl_amplitudes, const float* ctl_harmonic_distribution,
                              const float* f0_hz, const float* grad_audio, float* grad_f0,
                              void* workspace, size_t workspace_bytes, int B, int F, int K, int N,
                              int sample_rate, unsigned flags, void* stream);

/* effects.ExpDecayReverb._get_ir (ddsp/effects.py:144-151):
 *     ir[b][i] = G(gain[b]) * exp(-(2 + exp(decay[b])) * t_i) * noise[i],   t = linspace(0, 1, L)
 * gain, decay [B] (the reference's [B,1]); noise [L]: ONE burst shared by the batch, as the reference draws
 * tf.random.uniform([1, L], -1, 1) (ddsp_uniform_noise_f32 with B = 1 is the on-chip stand-in); ir [B,L] out.
 * flags: DDSP_DECAY_SCALE_EXP_SIGMOID = scale_fn is core.exp_sigmoid (else gain is used as given).
 * _backward: grad_ir [B,L] in, grad_gain / grad_decay [B] out; workspace:
 * ddsp_exp_decay_ir_backward_workspace_bytes(B, L). */
#define DDSP_DECAY_SCALE_EXP_SIGMOID 0x1u
int ddsp_exp_decay_ir_f32(const float* gain, const float* decay, const float* noise, float* ir, int B, int L,
                          unsigned flags, void* stream);
size_t ddsp_exp_decay_ir_backward_workspace_bytes(int B, int L);
int ddsp_exp_decay_ir_backward_f32(const float* gain, const float* decay, const float* noise,
                                   const float* grad_ir, float* grad_gain, float* grad_decay,
                                   void* workspace, size_t workspace_bytes, int B, int L, unsigned flags,
                                   void* stream);

/* processors.Mix (ddsp/processors.py:180-233), the constant-power crossfade next to processors.Add:
 *   ddsp_sigmoid_f32: tf.nn.sigmoid on n values (get_controls, :207; in may equal out);
 *   ddsp_mix_f32:     out[r][c] = sqrt(|m[r]|) * signal_one[r][c] + (1 - sqrt(|m[r] - 1|)) * signal_two[r][c]
 *                     for rows = batch * n_time time steps of C channels (get_signal, :231-233);
 *   ddsp_sigmoid_backward_f32, ddsp_mix_backward_f32: their adjoints, what tf.GradientTape takes through the two
 *                     (grad_in = grad_out s (1 - s); grad_one = sqrt|m| g, grad_two = (1 - sqrt|m - 1|) g, grad_level [rows] =
 *                     sum_c g (one sign(m) / (2 sqrt|m|) - two sign(m - 1) / (2 sqrt|m - 1|)); any of the three outputs may be
 *                     NULL; no atomics: bit-reproducible). */
int ddsp_sigmoid_f32(const float* in, float* out, size_t n, void* stream);
int ddsp_mix_f32(const float* signal_one, const float* signal_two, const float* mix_level, float* out,
                 size_t rows, int C, void* stream);
int ddsp_sigmoid_backward_f32(const float* in, const float* grad_out, float* grad_in, size_t n, void* stream);
int ddsp_mix_backward_f32(const float* signal_one, const float* signal_two, const float* mix_level, const float* grad_out,
                          float* grad_one, float* grad_two, float* grad_level, size_t rows, int C, void* stream);

/* Small pieces of ddsp/core.py that the synths only use fused inside their kernels, callable on their own (the reference
 * exports them; nothing on the hot path calls these):
 *   ddsp_safe_divide_f32           core.safe_divide (ddsp/core.py:207-210): out = numerator / where(denominator == 0, eps,
 *                                  denominator); numerator, out [rows, C]; denominator [rows, den_cols], den_cols = C or 1;
 *   ddsp_safe_log_f32              core.safe_log (:213-216): log(where(x <= 0, eps, x));
 *   ddsp_harmonic_frequencies_f32  core.get_harmonic_frequencies (:1028-1045): frequencies [rows] -> out [rows, n_harmonics],
 *                                  out[r][k] = fl32(frequencies[r] * (k + 1));
 *   ddsp_remove_above_nyquist_f32  core.remove_above_nyquist (:869-891): out = where(frequency >= sample_rate / 2, 0,
 *                                  amplitude) on n values (same shape); sample_rate is a float as in the reference, which
 *                                  compares with `sample_rate / 2.0` whatever number it is handed;
 *   ddsp_angular_cumsum_f32        core.angular_cumsum (:800-866): angular_frequency [B, T, C] (radians per sample) -> the
 *                                  accumulated phase in [0, 2 pi), [B, T, C].  The scan runs in fp64 revolutions (chunk sums,
 *                                  wrapped prefix, running phase): the reference's `chunk_size` has no counterpart - the
 *                                  result is exact to fp32 rounding for any length, where the reference's fp32 chunks drift.
 *                                  workspace: ddsp_angular_cumsum_workspace_bytes(B, T, C), 8-byte aligned. */
int ddsp_safe_divide_f32(const float* numerator, const float* denominator, float* out, size_t rows, int C,
                         int den_cols, float eps, void* stream);
int ddsp_safe_log_f32(const float* x, float* out, size_t n, float eps, void* stream);
int ddsp_harmonic_frequencies_f32(const float* frequencies, float* out, size_t rows, int n_harmonics, void* stream);
int ddsp_remove_above_nyquist_f32(const float* frequency_envelopes, const float* amplitude_envelopes, float* out,
                                  size_t n, float sample_rate, void* stream);
size_t ddsp_angular_cumsum_workspace_bytes(int B, int T, int C);
int ddsp_angular_cumsum_f32(const float* angular_frequency, float* out, void* workspace, size_t workspace_bytes,
                            int B, int T, int C, void* stream);

/* core.exp_sigmoid (ddsp/core.py:386-404), elementwise on n values (in may equal out). */
int ddsp_exp_sigmoid_f32(const float* in, float* out, size_t n, float exponent,
                         float max_value, float threshold, void* stream);

/* ------------------------------------------------------------------------------------
 * Wavetable synthesis and the modulated delay (ddsp/core.py:1167-1313, ddsp/synths.py:199-258,
 * ddsp/effects.py:327-392).  Nothing of size [B, N, W] or [B, N, max_length] is ever built.
 *
 * ddsp_wavetable_f32: synths.Wavetable / core.wavetable_synthesis.
 *   amplitudes [B,F,1], f0_hz [B,F,1] (N % F == 0, F + 1 < N: the 'window' envelope's own conditions),
 *   wavetables [B,Fw,W] with any Fw >= 1 (Fw == 1: a static table; Fw == N: one table per sample; otherwise
 *   linearly resampled to N as core.resample does), audio [B,N] out.
 *   flags: DDSP_WT_SCALE_EXP_SIGMOID applies core.exp_sigmoid to amplitudes and wavetables (Wavetable.get_controls).
 *   Fw == F and W <= 8192 run the fused kernel with both frames' tables in LDS (wt_fused_kernel); the rest gathers.
 * ddsp_wavetable_backward_f32: grad_audio [B,N] in; grad_amplitudes [B,F,1], grad_wavetables [B,Fw,W] and
 *   grad_f0_hz [B,F,1] out (with the flag, through exp_sigmoid to the raw inputs).  W <= 16384.  Deterministic.
 */
#define DDSP_WT_SCALE_EXP_SIGMOID 0x1u
int ddsp_wavetable_f32(const float* amplitudes, const float* wavetables, const float* f0_hz, float* audio, int B,
                       int F, int Fw, int W, int N, float sample_rate, unsigned flags, void* stream);
size_t ddsp_wavetable_backward_workspace_bytes(int B, int F, int Fw, int W, int N);
int ddsp_wavetable_backward_f32(const float* amplitudes, const float* wavetables, const float* f0_hz,
                                const float* grad_audio, float* grad_amplitudes, float* grad_wavetables,
                                float* grad_f0_hz, void* workspace, size_t workspace_bytes, int B, int F, int Fw,
                                int W, int N, float sample_rate, unsigned flags, void* stream);

/* core.linear_lookup (ddsp/core.py:1167-1213): phase [B,N], wavetables [B,Fw,W] with Fw == 1 or Fw == N, out [B,N].
 * out = sum_i relu(1 - |phase W - i|) w[i mod W] over the points i = 0 .. W: the phase is NOT wrapped, a phase
 * outside [0, 1] fades to 0 within one table step.  The backward call gives dL/d phase [B,N] and
 * dL/d wavetables [B,Fw,W] (W <= 16384). */
int ddsp_linear_lookup_f32(const float* phase, const float* wavetables, float* out, int B, int N, int Fw, int W,
                           void* stream);
size_t ddsp_linear_lookup_backward_workspace_bytes(int B, int N);
int ddsp_linear_lookup_backward_f32(const float* phase, const float* wavetables, const float* grad_out,
                                    float* grad_phase, float* grad_wavetables, void* workspace,
                                    size_t workspace_bytes, int B, int N, int Fw, int W, void* stream);

/* core.variable_length_delay (ddsp/core.py:1286-1313) and effects.ModDelay.get_signal around it:
 *   out = gain * lookup(phase * phase_scale + phase_offset) (+ audio with DDSP_DELAY_ADD_DRY),
 * the lookup reading point i < max_length as audio[n - i] (0 before the clip) and point max_length as audio[n],
 * the reference's appended wrap point.  phase, audio, out [B,N]; gain [B,N] or NULL (gain 1).
 * DDSP_DELAY_GAIN_EXP_SIGMOID / DDSP_DELAY_PHASE_SIGMOID apply ModDelay.get_controls' default scale functions.
 * Backward: grad_phase, grad_audio [B,N] out, grad_gain [B,N] out (NULL exactly when gain is).  Deterministic. */
#define DDSP_DELAY_ADD_DRY 0x1u
#define DDSP_DELAY_GAIN_EXP_SIGMOID 0x2u
#define DDSP_DELAY_PHASE_SIGMOID 0x4u
int ddsp_variable_length_delay_f32(const float* phase, const float* audio, const float* gain, float* out, int B, int N,
                                   int max_length, float phase_scale, float phase_offset, unsigned flags,
                                   void* stream);
size_t ddsp_variable_length_delay_backward_workspace_bytes(int B, int N);
int ddsp_variable_length_delay_backward_f32(const float* phase, const float* audio, const float* gain,
                                            const float* grad_out, float* grad_phase, float* grad_audio,
                                            float* grad_gain, void* workspace, size_t workspace_bytes, int B, int N,
                                            int max_length, float phase_scale, float phase_offset, unsigned flags,
                                            void* stream);

/* ------------------------------------------------------------------------------------
 * synths.Sinusoidal (ddsp/synths.py:260-323) and the frequency scale functions under it (ddsp/core.py:219-348,
 * 414-507).  Nothing of size [B, N, K] is ever built (csrc/sinusoidal.hip).
 *
 * flags:
 *   DDSP_SIN_AMP_EXP_SIGMOID   amp_scale_fn = core.exp_sigmoid on the amplitudes;
 *   DDSP_SIN_FREQ_SIGMOID      freq_scale_fn = core.frequencies_sigmoid(depth, hz_min, hz_max), depth <= 64;
 *   DDSP_SIN_FREQ_SOFTMAX      freq_scale_fn = core.frequencies_softmax(depth, hz_min, hz_max), any depth
 *                              (both at once: DDSP_ERR_UNSUPPORTED; neither: the frequencies are in Hz, depth is ignored);
 *   DDSP_SIN_MASK_NYQUIST      core.remove_above_nyquist at frame rate, which Sinusoidal.get_controls applies whenever
 *                              it has a freq_scale_fn;
 *   DDSP_SIN_AMP_LINEAR        amp_resample_method 'linear' (default: 'window').
 *
 * ddsp_sinusoidal_controls_f32: Sinusoidal.get_controls on `rows` = B * F frames.  amplitudes [rows, K] (NULL together
 *   with ctl_amplitudes: the frequency scale function on its own), frequencies [rows, K * depth] -> ctl_amplitudes,
 *   ctl_frequencies [rows, K].  ddsp_sinusoidal_controls_backward_f32 is its adjoint (the Nyquist mask passes no
 *   gradient to the frequencies; grad_ctl_frequencies may be NULL for zero).
 * ddsp_sinusoidal_signal_f32: Sinusoidal.get_signal, controls [B,F,K] (Hz) -> audio [B,N].  Scale flags: UNSUPPORTED.
 * ddsp_sinusoidal_f32: get_signal(**get_controls(...)) from the raw network outputs, amplitudes [B,F,K] and
 *   frequencies [B,F,K*depth]; ctl_amplitudes / ctl_frequencies [B,F,K]: both NULL, or both out (the controls dict).
 * ddsp_sinusoidal_backward_f32: grad_audio [B,N] -> grad_amplitudes [B,F,K], grad_frequencies [B,F,K*depth] with respect
 *   to the inputs the same flags describe (no scale flag: the controls).  No atomics: the same bits on every run and
 *   for any sub-batch.
 * All need N % F == 0 (DDSP_ERR_UNSUPPORTED otherwise: the host layer then follows the chain of materialised
 * envelopes, ddsp_resample_ex_f32 + ddsp_oscillator_bank_f32 and their adjoints).  Any K, any hop.
 * The frequency envelope is the legacy bilinear resize of the frames (the last one held), the phase the INCLUSIVE
 * cumulative sum in fp64 cycles, and a sample whose interpolated frequency is >= sample_rate / 2 contributes nothing.
 */
#define DDSP_SIN_AMP_EXP_SIGMOID 0x1u
#define DDSP_SIN_FREQ_SIGMOID 0x2u
#define DDSP_SIN_FREQ_SOFTMAX 0x4u
#define DDSP_SIN_MASK_NYQUIST 0x8u
#define DDSP_SIN_AMP_LINEAR 0x10u
int ddsp_sinusoidal_controls_f32(const float* amplitudes, const float* frequencies, float* ctl_amplitudes,
                                 float* ctl_frequencies, size_t rows, int K, int depth, float hz_min, float hz_max,
                                 float sample_rate, unsigned flags, void* stream);
int ddsp_sinusoidal_controls_backward_f32(const float* amplitudes, const float* frequencies,
                                          const float* grad_ctl_amplitudes, const float* grad_ctl_frequencies,
                                          float* grad_amplitudes, float* grad_frequencies, size_t rows, int K, int depth,
                                          float hz_min, float hz_max, float sample_rate, unsigned flags, void* stream);
size_t ddsp_sinusoidal_workspace_bytes(int B, int F, int K, int N);
int ddsp_sinusoidal_signal_f32(const float* amplitudes, const float* frequencies, float* audio, void* workspace,
                               size_t workspace_bytes, int B, int F, int K, int N, float sample_rate, unsigned flags,
                               void* stream);
int ddsp_sinusoidal_f32(const float* amplitudes, const float* frequencies, float* audio, float* ctl_amplitudes,
                        float* ctl_frequencies, void* workspace, size_t workspace_bytes, int B, int F, int K, int N,
                        int depth, float hz_min, float hz_max, float sample_rate, unsigned flags, void* stream);
size_t ddsp_sinusoidal_backward_workspace_bytes(int B, int F, int K, int N);
int ddsp_sinusoidal_backward_f32(const float* amplitudes, const float* frequencies, const float* grad_audio,
                                 float* grad_amplitudes, float* grad_frequencies, void* workspace, size_t workspace_bytes,
                                 int B, int F, int K, int N, int depth, float hz_min, float hz_max, float sample_rate,
                                 unsigned flags, void* stream);

/* The elementwise conversions of ddsp/core.py:219-348 on n values:
 *   MIDI_TO_HZ 440 * 2^((x - 69) / 12) (ZERO_SILENCE: MIDI 0 -> 0 Hz); HZ_TO_MIDI its inverse with x <= 0 -> 0;
 *   UNIT_TO_MIDI p0 + (p1 - p0) x (CLIP: x clipped to [0, 1] first); MIDI_TO_UNIT (x - p0) / (p1 - p0) (CLIP: the
 *   result clipped); LOGB log(where(x <= 0, p1, x)) / p0 with p0 the safe log of the base and p1 = eps. */
#define DDSP_CONVERT_MIDI_TO_HZ 0
#define DDSP_CONVERT_MIDI_TO_HZ_ZERO_SILENCE 1
#define DDSP_CONVERT_HZ_TO_MIDI 2
#define DDSP_CONVERT_UNIT_TO_MIDI 3
#define DDSP_CONVERT_UNIT_TO_MIDI_CLIP 4
#define DDSP_CONVERT_MIDI_TO_UNIT 5
#define DDSP_CONVERT_MIDI_TO_UNIT_CLIP 6
#define DDSP_CONVERT_LOGB 7
int ddsp_unit_convert_f32(const float* in, float* out, size_t n, int op, float p0, float p1, void* stream);

/* ------------------------------------------------------------------------------------
 * The sinusoidal consistency losses (ddsp/losses.py:689-1061) and core.sinusoidal_to_harmonic (ddsp/core.py:733-781):
 * csrc/consistency.hip.  `rows` = B * T frames; a block owns a frame, nothing of size [rows, C, K], [rows, K, K] or
 * [rows, H, K] is built, forward or backward, and no call needs a workspace.  No atomics: the same bits on every run and
 * for any subset of the rows.  Bounds (DDSP_ERR_UNSUPPORTED beyond): K, K_target, H <= 1024; n_harmonic_points <= 256;
 * n_harmonic_gaussians <= 4096; any C.
 *
 * ddsp_twm_loss_tensors_f32: TWMLoss.get_loss_tensors.  f0_candidates [rows, C], freqs / amps [rows, K] ->
 *   sinusoids_loss, harmonics_loss [rows, C].  _backward_: the two incoming gradients [rows, C] and the forward's
 *   sinusoids_loss -> grad_f0_candidates [rows, C], grad_freqs, grad_amps [rows, K].
 * ddsp_twm_softmin_f32: per frame sum_c L_c softmax(-L / temperature)_c with L = w_s S + w_h H -> frame_loss [rows]
 *   (TWMLoss.call is its mean divided by C); _backward_ its adjoint.
 * ddsp_twm_nanargmin_f32: TWMLoss.predict_f0: the candidate of the smallest L that is not NaN -> f0_hz [rows];
 *   *all_nan_flag (zeroed by the caller) is set to 1 if some frame has no such candidate.
 * ddsp_kde_nll_f32: KDEConsistencyLoss.nll, source amps / freqs [rows, K], target [rows, K_target] -> nll [rows];
 *   _backward_: grad_nll [rows] -> the four gradients.
 * ddsp_sinusoidal_to_harmonic_f32: sin_amps / sin_freqs [rows, K], f0_hz [rows] -> harm_amp [rows], harm_dist [rows, H];
 *   flags: DDSP_S2H_NORMALIZE.  _backward_: grad_harm_amp [rows], grad_harm_dist [rows, H] -> the three gradients.
 * ddsp_mean_f32: out[0] = scale * mean(x[0 .. n)) in fixed-order fp64 partials; _backward_: grad_x[i] = grad_out[0] scale / n.
 * ddsp_row_mean_f32: tf.reduce_mean(x, axis=-1), [rows, K] -> [rows]; _backward_ its adjoint.
 * ddsp_unit_convert_backward_f32: grad_in = grad_out * d op(in) / d in for DDSP_CONVERT_HZ_TO_MIDI and
 *   DDSP_CONVERT_LOG_FLOOR (log10(max(p1, x)), p0 = ln 10: losses.amp_loss(log=True)).
 */
#define DDSP_S2H_NORMALIZE 0x1u
#define DDSP_CONVERT_LOG_FLOOR 8
int ddsp_twm_loss_tensors_f32(const float* f0_candidates, const float* freqs, const float* amps, float* sinusoids_loss,
                              float* harmonics_loss, size_t rows, int C, int K, int n_harmonic_points,
                              int n_harmonic_gaussians, float sinusoids_scale, float harmonics_scale, float sample_rate,
                              void* stream);
int ddsp_twm_loss_tensors_backward_f32(const float* f0_candidates, const float* freqs, const float* amps,
                                       const float* sinusoids_loss, const float* grad_sinusoids_loss,
                                       const float* grad_harmonics_loss, float* grad_f0_candidates, float* grad_freqs,
                                       float* grad_amps, size_t rows, int C, int K, int n_harmonic_points,
                                       int n_harmonic_gaussians, float sinusoids_scale, float harmonics_scale,
                                       float sample_rate, void* stream);
int ddsp_twm_softmin_f32(const float* sinusoids_loss, const float* harmonics_loss, float* frame_loss, size_t rows, int C,
                         float sinusoids_weight, float harmonics_weight, float temperature, void* stream);
int ddsp_twm_softmin_backward_f32(const float* sinusoids_loss, const float* harmonics_loss, const float* grad_frame_loss,
                                  float* grad_sinusoids_loss, float* grad_harmonics_loss, size_t rows, int C,
                                  float sinusoids_weight, float harmonics_weight, float temperature, void* stream);
int ddsp_twm_nanargmin_f32(const float* sinusoids_loss, const float* harmonics_loss, const float* f0_candidates, float* f0_hz,
                           int* all_nan_flag, size_t rows, int C, float sinusoids_weight, float harmonics_weight,
                           void* stream);
int ddsp_kde_nll_f32(const float* amps, const float* freqs, const float* amps_target, const float* freqs_target, float* nll,
                     size_t rows, int K, int K_target, float scale_target, void* stream);
int ddsp_kde_nll_backward_f32(const float* amps, const float* freqs, const float* amps_target, const float* freqs_target,
                              const float* grad_nll, float* grad_amps, float* grad_freqs, float* grad_amps_target,
                              float* grad_freqs_target, size_t rows, int K, int K_target, float scale_target, void* stream);
int ddsp_sinusoidal_to_harmonic_f32(const float* sin_amps, const float* sin_freqs, const float* f0_hz, float* harm_amp,
                                    float* harm_dist, size_t rows, int K, int H, float harmonic_width, float sample_rate,
                                    unsigned flags, void* stream);
int ddsp_sinusoidal_to_harmonic_backward_f32(const float* sin_amps, const float* sin_freqs, const float* f0_hz,
                                             const float* grad_harm_amp, const float* grad_harm_dist, float* grad_sin_amps,
                                             float* grad_sin_freqs, float* grad_f0_hz, size_t rows, int K, int H,
                                             float harmonic_width, float sample_rate, unsigned flags, void* stream);
int ddsp_mean_f32(const float* x, float* out, size_t n, float scale, void* stream);
int ddsp_mean_backward_f32(const float* grad_out, float* grad_x, size_t n, float scale, void* stream);
int ddsp_row_mean_f32(const float* x, float* out, size_t rows, int K, void* stream);
int ddsp_row_mean_backward_f32(const float* grad_out, float* grad_x, size_t rows, int K, void* stream);
int ddsp_unit_convert_backward_f32(const float* in, const float* grad_out, float* grad_in, size_t n, int op, float p0,
                                   float p1, void* stream);

/* ------------------------------------------------------------------------------------
 * losses.wasserstein_distance (ddsp/losses.py:632-686) and, with DDSP_WASSERSTEIN_MIDI, the per-frame distance of
 * WassersteinConsistencyLoss (:584-629): csrc/wasserstein.hip.  A block owns a row: the row's n_u + n_v values are ranked,
 * scanned and reduced in LDS; no call needs a workspace, nothing of size [rows, n_u + n_v] is built, forward or backward.
 * No atomics: the same bits on every run and for any subset of the rows.
 *
 * ddsp_wasserstein_f32: u_values [rows, n_u], v_values [rows, n_v], u_weights [rows, n_u] or NULL, v_weights [rows, n_v] or
 *   NULL -> distance [rows] = (sum_i delta_i |U_i - V_i|^p)^(1/p) over the stably sorted concatenation of the values.  The
 *   weights are used as they are, NOT normalised (the reference computes the normalised CDF and drops it); a NULL side has
 *   the CDF index / n_side.  A row with a NaN among its values or weights gives NaN; the other rows are unaffected.
 *   flags: DDSP_WASSERSTEIN_MIDI - the values are frequencies in Hz and are compared as hz_to_midi(value) (f <= 0 -> 0).
 * ddsp_wasserstein_backward_f32: the same inputs and grad_distance [rows] -> grad_u_values, grad_v_values, and grad_u_weights /
 *   grad_v_weights (NULL exactly where the weights are NULL, else DDSP_ERR_NULL_POINTER).  It recomputes the forward pass;
 *   every gradient element is written once.  Among exactly tied values the gradient of a value is one of the valid
 *   one-sided choices (the sum over a group of tied values is the group's derivative).
 * Bounds (DDSP_ERR_UNSUPPORTED beyond): n_u, n_v <= 1024 each; p = 1 or 2.  The ranking compares every pair of a row's
 * values: its cost is quadratic in n_u + n_v.
 */
#define DDSP_WASSERSTEIN_MIDI 0x1
int ddsp_wasserstein_f32(const float* u_values, const float* v_values, const float* u_weights, const float* v_weights,
                         float* distance, size_t rows, int n_u, int n_v, int p, int flags, void* stream);
int ddsp_wasserstein_backward_f32(const float* u_values, const float* v_values, const float* u_weights, const float* v_weights,
                                  const float* grad_distance, float* grad_u_values, float* grad_v_values, float* grad_u_weights,
                                  float* grad_v_weights, size_t rows, int n_u, int n_v, int p, int flags, void* stream);

/* ------------------------------------------------------------------------------------
 * losses.HmmTranscriber (ddsp/losses.py:246-345): csrc/hmm.hip.  The hidden Markov model of the constructor (:275-304) over
 * n_pitches states: a uniform initial distribution; transitions `hold` on the diagonal and `other` elsewhere (the caller
 * passes the two numbers, hold + (n_pitches - 1) other = 1); observations (pitch, amps) with independent normal densities -
 * state 0 ("off"): pitch ~ N(n_pitches / 2, n_pitches), amps ~ N(amps_off_center, amps_off_scale); state s >= 1: pitch ~
 * N(s, midi_std), amps ~ N(amps_on_center, amps_on_scale).  A block owns a row and walks its steps in order; a step costs
 * O(n_pitches), and nothing of size [n_pitches, n_pitches] or [rows, steps, n_pitches] is built by the forward-only calls.
 * No atomics: the same bits on every run and for any subset of the rows.
 *
 * ddsp_hmm_log_prob_f32: pitch [rows, steps], amps [rows, steps] -> log_prob [rows], the log-likelihood of the observations
 *   (tfp's HiddenMarkovModel.log_prob).  The forward variables are kept normalised and their scales are summed in fp64 and
 *   as integer exponents; observations far from every state (amps = 50, pitch = -300) give a finite value.
 * ddsp_hmm_log_prob_backward_f32: the same inputs and grad_log_prob [rows] -> grad_pitch, grad_amps [rows, steps] by the
 *   forward-backward recursion.  It recomputes the forward pass into `workspace`
 *   (ddsp_hmm_log_prob_backward_workspace_bytes(rows, steps, n_pitches) = rows * steps * n_pitches floats; DDSP_ERR_WORKSPACE
 *   if smaller); every gradient element is written once.
 * ddsp_hmm_viterbi_f32: -> states [rows, steps] (int32), the most likely state sequence (posterior_mode); among equals the
 *   lowest index, as argmax.  `workspace` (ddsp_hmm_viterbi_workspace_bytes: a bit per step and state, an int per step)
 *   holds the back trace.
 * Bounds (DDSP_ERR_UNSUPPORTED beyond): 2 <= n_pitches <= 1024; hold >= other > 0.  Any number of steps.
 */
int ddsp_hmm_log_prob_f32(const float* pitch, const float* amps, float* log_prob, size_t rows, int steps, int n_pitches,
                          double hold, double other, double midi_std, double amps_on_center, double amps_on_scale,
                          double amps_off_center, double amps_off_scale, void* stream);
size_t ddsp_hmm_log_prob_backward_workspace_bytes(int rows, int steps, int n_pitches);
int ddsp_hmm_log_prob_backward_f32(const float* pitch, const float* amps, const float* grad_log_prob, float* grad_pitch,
                                   float* grad_amps, void* workspace, size_t workspace_bytes, size_t rows, int steps,
                                   int n_pitches, double hold, double other, double midi_std, double amps_on_center,
                                   double amps_on_scale, double amps_off_center, double amps_off_scale, void* stream);
size_t ddsp_hmm_viterbi_workspace_bytes(int rows, int steps, int n_pitches);
int ddsp_hmm_viterbi_f32(const float* pitch, const float* amps, int* states, void* workspace, size_t workspace_bytes,
                         size_t rows, int steps, int n_pitches, double hold, double other, double midi_std,
                         double amps_on_center, double amps_on_scale, double amps_off_center, double amps_off_scale,
                         void* stream);

/* ------------------------------------------------------------------------------------
 * The note pooling of ddsp/training/nn.py:375-557: csrc/notes.hip.  mask is [rows, steps, notes], x [rows, steps, dims],
 * per-note tensors [rows, notes, dims].  Nothing of size rows * steps * notes * dims exists, and nothing of size
 * rows * steps * notes but the mask; the cost of the moments and of the spread follows the mask's non-zero entries.  Every
 * formula holds for any fp32 mask (weights m in the mean, m^2 in the variance).  No workspace, no atomics, fixed summation
 * orders: the same bits on every run and for any subset of the rows.
 *
 * ddsp_note_mask_f32: pitch [rows, steps] (and onset [rows, steps], or NULL) -> mask of 0.0 / 1.0, every element written.
 *   onset == NULL: get_note_mask (:375-425) - step 0 starts region 0, step p in 1 .. steps - 2 starts a region when
 *   pitch[p] != pitch[p - 1], THE LAST STEP NEVER DOES; note_on_only keeps the regions whose pitch sum (hence mean) is > 0.
 *   onset != NULL: get_note_mask_from_onset (:428-476) - step p >= 1 advances the region index by (int)onset[p];
 *   note_on_only keeps the steps with pitch > 0.  Steps whose region index is outside [0, max_regions) get a zero row.
 * ddsp_note_moments_f32: get_note_moments (:484-520).  Per (row, note), in ascending time and fp64: length = sum m (0 -> 1e-7,
 *   core.safe_divide), mean = sum m x / length, then a second pass for std = sqrt(sum (m (x - mean))^2 / length) and
 *   s2 = sum m^2 (x - mean) (what the backward needs).  mean_lo = mean - (float)mean, what the fp32 result lost of the fp64
 *   mean (the backward's x - mean cancels on notes of nearly equal values).  std, s2, mean_lo and lengths ([rows, notes], the
 *   safe length) may each be NULL (s2 needs std).  flags & DDSP_NOTES_SUM: `mean` receives sum m x without the division (the adjoint of the spread
 *   in its values); std, s2, mean_lo and lengths must be NULL.
 * ddsp_note_spread_f32: out[r, t, :] = sum_n m (a[r, n, :] + c[r, n, :] m (x[r, t, :] - mean[r, n, :] - mean_lo[r, n, :])); c may be
 *   NULL (then x, mean and mean_lo are not read), and mean_lo may be NULL where c is given.  c == NULL is the forward of pool_over_notes (:523-547) and, with dims = 1, of
 *   get_short_note_loss_mask (:550-557); with c it is the backward of the moments in x.
 * Bounds (DDSP_ERR_UNSUPPORTED beyond): max_regions <= 1024 in ddsp_note_mask_f32; rows * notes and rows * steps below 2^31;
 * dims <= 256 * 65535.  steps >= 2 for the mask (DDSP_ERR_BAD_SHAPE).
 */
#define DDSP_NOTES_SUM 0x1
int ddsp_note_mask_f32(const float* pitch, const float* onset, float* mask, size_t rows, int steps, int max_regions,
                       int note_on_only, void* stream);
int ddsp_note_moments_f32(const float* x, const float* mask, float* mean, float* std, float* s2, float* mean_lo, float* lengths,
                          size_t rows, int steps, int notes, int dims, int flags, void* stream);
int ddsp_note_spread_f32(const float* mask, const float* a, const float* c, const float* x, const float* mean, const float* mean_lo,
                         float* out, size_t rows, int steps, int notes, int dims, void* stream);

/* ------------------------------------------------------------------------------------
 * The rest of ddsp/core.py: csrc/critical_bands.hip, csrc/harmonic_wavetable.hip, csrc/scale_fns.hip.  No workspace, no
 * atomics, fixed summation orders: the same bits on every run and for a row alone or in a batch.
 *
 * ddsp_critical_bands_f32: core.frequencies_critical_bands (:510-569) on `rows` = B * T frames.  freqs [rows, K * depth]
 *   (a sinusoid's `depth` values side by side) -> out [rows, K]:
 *     out = soft_limit(f_center[k] + bandwidth_scale * bandwidths[k] * sum_d tanh(freqs[k, d]) * depth_modifier[d], hz_min, hz_max)
 *   with soft_limit(x, lo, hi) = softplus(x) + lo - softplus(x - (hi - lo)).  f_center, bandwidths [K] and depth_modifier
 *   [depth] are device tables of the caller (the host layer: the bark / mel grid, its ERBs, depth_scale^-d).  The loads
 *   are coalesced for every depth; the sum over d runs in ascending d in one thread.
 * ddsp_critical_bands_backward_f32: grad_out [rows, K] -> grad_freqs [rows, K * depth]; recomputes the forward's sum, so
 *   nothing but freqs is saved.
 *   K, depth >= 1 (else DDSP_ERR_BAD_SHAPE); rows * K below 2^31 (else DDSP_ERR_UNSUPPORTED).
 *
 * ddsp_harmonic_wavetable_f32: core.harmonic_distribution_to_wavetable (:1217-1235).  hd [rows, K] -> out [rows, L]:
 *     out[r, n] = scale * sum_{k = 1 .. K} w_k hd[r, k - 1] cos(2 pi k n / L),   w_k = 1, but w_{L/2} = 1/2
 *   (the irfft of the distribution padded to L / 2 + 1 bins; the reference's scale is n_wavetable / L), one fused kernel on
 *   the LDS transforms of the STFT kernels.  ddsp_harmonic_wavetable_backward_f32: grad_out [rows, L] -> grad_hd [rows, K].
 *   L even and K <= L / 2 (else DDSP_ERR_BAD_SHAPE); L a power of two in [64, 8192] (else DDSP_ERR_UNSUPPORTED: the host
 *   layer takes other lengths through its general path).
 *
 * ddsp_scale_convert_f32 / ddsp_scale_convert_backward_f32 (grad_in = grad_out * d op(in) / d in) on n values:
 *   HZ_TO_BARK 26.81 / (1 + 1960 / x) - 0.53 and BARK_TO_HZ 1960 / (26.81 / (x + 0.53) - 1), IEEE results at the poles
 *   (hz_to_bark(0) = -0.53, bark_to_hz(-0.53) = 0); HZ_TO_MEL 2595 log10(1 + x / 700) with core.logb's safe log;
 *   MEL_TO_HZ 700 (10^(x / 2595) - 1); HZ_TO_ERB 0.108 x + 24.7; SOFT_LIMIT with p0 = x_min, p1 = x_max; LOG_SCALE
 *   exp((1 - u) ln p0 + u ln p1), u = (x + 1) / 2, p0 = min_x, p1 = max_x; SYM_EXP_SIGMOID exp_sigmoid(p0 (|x| / 2 - 1)),
 *   p0 = width, slope 0 at x = 0; NAN_TO_NUM p0 where x is NaN (no gradient there), x elsewhere.
 *   An unknown op is DDSP_ERR_BAD_SHAPE.
 */
#define DDSP_SCALE_HZ_TO_BARK 0
#define DDSP_SCALE_BARK_TO_HZ 1
#define DDSP_SCALE_HZ_TO_MEL 2
#define DDSP_SCALE_MEL_TO_HZ 3
#define DDSP_SCALE_HZ_TO_ERB 4
#define DDSP_SCALE_SOFT_LIMIT 5
#define DDSP_SCALE_LOG_SCALE 6
#define DDSP_SCALE_SYM_EXP_SIGMOID 7
#define DDSP_SCALE_NAN_TO_NUM 8
int ddsp_critical_bands_f32(const float* freqs, float* out, size_t rows, int K, int depth, const float* f_center,
                            const float* bandwidths, const float* depth_modifier, float bandwidth_scale, float hz_min,
                            float hz_max, void* stream);
int ddsp_critical_bands_backward_f32(const float* freqs, const float* grad_out, float* grad_freqs, size_t rows, int K,
                                     int depth, const float* f_center, const float* bandwidths, const float* depth_modifier,
                                     float bandwidth_scale, float hz_min, float hz_max, void* stream);
int ddsp_harmonic_wavetable_f32(const float* hd, float* out, size_t rows, int K, int L, float scale, void* stream);
int ddsp_harmonic_wavetable_backward_f32(const float* grad_out, float* grad_hd, size_t rows, int K, int L, float scale,
                                         void* stream);
int ddsp_scale_convert_f32(const float* in, float* out, size_t n, int op, float p0, float p1, void* stream);
int ddsp_scale_convert_backward_f32(const float* in, const float* grad_out, float* grad_in, size_t n, int op, float p0,
                                    float p1, void* stream);

/* ------------------------------------------------------------------------------------
 * Tracing (the reference has none beyond wall-clock logs): opt-in
 * HIP-event brackets around individual kernels, recorded on the stream they are launched
 * on.  ddsp_profile_begin(mask, max_records) turns it on for the kernels whose bit is set
 * in `mask` (bit i = kernel id i, names via ddsp_profile_kernel_name); ddsp_profile_end
 * synchronises the recorded events, fills total_ms[ddsp_profile_kernel_count()] and
 * counts[...], and turns tracing off.  Not for use under stream capture.
 */
int ddsp_profile_kernel_count(void);
const char* ddsp_profile_kernel_name(int kernel_id);
int ddsp_profile_begin(unsigned kernel_mask, int max_records);
/* As ddsp_profile_begin, but only every `stride`-th launch of each selected kernel is bracketed
 * (the first one always is).  A bracketed launch carries a start marker and a stop event, which
 * costs ~5 us of queue time each; sampling keeps a timed region honest while still measuring the
 * kernel inside it.  stride < 1 -> DDSP_ERR_BAD_SHAPE. */
int ddsp_profile_begin_sampled(unsigned kernel_mask, int max_records, int stride);
int ddsp_profile_end(double* total_ms, int* counts);

#ifdef __cplusplus
}
#endif
#endif /* DDSP_AMD_H_ */
