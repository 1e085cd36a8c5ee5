"""ctypes binding of the C ABI in include/ddsp_amd.h.

The product path has NO fallback: if `libddsp_amd.so` is missing or a symbol is absent
this module raises, and every processor that needs a kernel fails loudly.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libddsp_amd.so')

c_f32p = ctypes.c_void_p      # device pointers travel as integers (tensor.data_ptr())
c_int, c_uint, c_size_t = ctypes.c_int, ctypes.c_uint, ctypes.c_size_t
c_u64, c_float, c_voidp = ctypes.c_uint64, ctypes.c_float, ctypes.c_void_p
c_double = ctypes.c_double

# name -> (restype, argtypes); must list every symbol declared in include/ddsp_amd.h
SIGNATURES = {
    'ddsp_version': (ctypes.c_char_p, []),
    'ddsp_harmonic_controls_f32': (c_int, [c_f32p] * 5 + [c_int] * 4 + [c_uint, c_voidp]),
    'ddsp_harmonic_workspace_bytes': (c_size_t, [c_int] * 4),
    'ddsp_harmonic_signal_f32': (c_int, [c_f32p] * 4 + [c_voidp, c_size_t] + [c_int] * 5 +
                                 [c_uint, c_voidp]),
    'ddsp_harmonic_signal_tf_order_f32': (c_int, [c_f32p] * 4 + [c_int] * 5 + [c_uint, c_voidp]),
    'ddsp_harmonic_f32': (c_int, [c_f32p] * 6 + [c_voidp, c_size_t] + [c_int] * 5 +
                          [c_uint, c_voidp]),
    'ddsp_harmonic_add_f32': (c_int, [c_f32p] * 5 + [c_int] * 5 + [c_uint, c_voidp]),
    'ddsp_filtered_noise_controls_f32': (c_int, [c_f32p] * 2 + [c_int] * 3 +
                                         [c_float, c_uint, c_voidp]),
    'ddsp_fir_size': (c_int, [c_int, c_int]),
    'ddsp_frequency_impulse_response_f32': (c_int, [c_f32p] * 2 + [c_int] * 4 + [c_voidp]),
    'ddsp_filtered_noise_workspace_bytes': (c_size_t, [c_int] * 5),
    'ddsp_filtered_noise_f32': (c_int, [c_f32p] * 4 + [c_voidp, c_size_t] + [c_int] * 5 +
                                [c_float, c_uint, c_u64, c_u64, c_voidp]),
    'ddsp_filtered_noise_backward_workspace_bytes': (c_size_t, [c_int] * 4),
    'ddsp_filtered_noise_backward_f32': (c_int, [c_f32p] * 4 + [c_voidp, c_size_t] + [c_int] * 5 +
                                         [c_float, c_uint, c_u64, c_u64, c_voidp]),
    'ddsp_fft_convolve_same_f32': (c_int, [c_f32p] * 3 + [c_int] * 6 + [c_voidp]),
    'ddsp_harmonic_backward_workspace_bytes': (c_size_t, [c_int] * 4),
    'ddsp_harmonic_backward_f32': (c_int, [c_f32p] * 6 + [c_voidp, c_size_t] + [c_int] * 5 +
                                   [c_uint, c_int, c_voidp]),
    'ddsp_harmonic_streaming_f32': (c_int, [c_f32p] * 6 + [c_voidp, c_size_t] + [c_int] * 5 +
                                    [c_uint, c_voidp]),
    'ddsp_fft_convolve_long_workspace_bytes': (c_size_t, [c_int] * 5),
    'ddsp_fft_convolve_long_ex_workspace_bytes': (c_size_t, [c_int] * 6),
    'ddsp_fft_convolve_long_ex_f32': (c_int, [c_f32p] * 3 + [c_voidp, c_size_t] + [c_int] * 6 +
                                      [c_uint, c_voidp]),
    'ddsp_fft_convolve_long_f32': (c_int, [c_f32p] * 3 + [c_voidp, c_size_t] + [c_int] * 5 +
                                   [c_uint, c_voidp]),
    'ddsp_spectral_loss_workspace_bytes': (c_size_t, [c_int, c_int, ctypes.POINTER(c_int), c_int]),
    'ddsp_spectral_loss_f32': (c_int, [c_f32p] * 3 + [c_voidp, c_size_t, c_int, c_int,
                                                      ctypes.POINTER(c_int), c_int, c_float, c_float,
                                                      c_voidp]),
    'ddsp_spectral_loss_backward_f32': (c_int, [c_f32p] * 4 + [c_int, c_int, ctypes.POINTER(c_int), c_int,
                                                           c_float, c_float, c_voidp]),
    'ddsp_spectral_loss_value_and_grad_f32': (c_int, [c_f32p] * 4 + [c_voidp, c_size_t, c_int, c_int,
                                                                 ctypes.POINTER(c_int), c_int, c_float,
                                                                 c_float, c_voidp]),
    'ddsp_spectral_loss_grad_workspace_bytes': (c_size_t, [c_int, c_int, ctypes.POINTER(c_int), c_int]),
    'ddsp_spectral_loss_backward_det_f32': (c_int, [c_f32p] * 4 + [c_int, c_int, ctypes.POINTER(c_int), c_int,
                                                               c_float, c_float, c_voidp, c_size_t, c_voidp]),
    'ddsp_spectral_loss_value_and_grad_det_f32': (c_int, [c_f32p] * 4 + [c_voidp, c_size_t, c_int, c_int,
                                                                     ctypes.POINTER(c_int), c_int, c_float,
                                                                     c_float, c_voidp, c_size_t, c_voidp]),
    'ddsp_stft_mag_backward_workspace_bytes': (c_size_t, [c_int] * 3),
    'ddsp_stft_mag_backward_det_f32': (c_int, [c_f32p] * 3 + [c_voidp, c_size_t] + [c_int] * 3 + [c_voidp]),
    'ddsp_stft_frames_mag_backward_workspace_bytes': (c_size_t, [c_int] * 6),
    'ddsp_stft_frames_mag_backward_det_f32': (c_int, [c_f32p] * 3 + [c_voidp, c_size_t] + [c_int] * 6 + [c_voidp]),
    'ddsp_stft_mag_f32': (c_int, [c_f32p] * 4 + [c_int] * 3 + [c_voidp]),
    'ddsp_spectral_terms_workspace_bytes': (c_size_t, [c_int] * 2),
    'ddsp_spectral_terms_f32': (c_int, [c_f32p] * 3 + [c_int] * 3 + [c_f32p, c_voidp, c_f32p, c_voidp, c_size_t] +
                                [c_int] * 4 + [ctypes.c_float] * 5 + [c_int, c_voidp]),
    'ddsp_stft_mag_backward_f32': (c_int, [c_f32p] * 3 + [c_int] * 3 + [c_voidp]),
    'ddsp_window_impulse_response_size': (c_int, [c_int, c_int]),
    'ddsp_apply_window_to_impulse_response_f32': (c_int, [c_f32p, c_f32p, ctypes.c_long, c_int, c_int, c_int, c_voidp]),
    'ddsp_stft_frames_mag_f32': (c_int, [c_f32p] * 2 + [c_int] * 6 + [c_voidp]),
    'ddsp_stft_frames_f32': (c_int, [c_f32p] * 2 + [c_int] * 7 + [c_voidp]),
    'ddsp_stft_frames_mag_ex_f32': (c_int, [c_f32p] * 2 + [c_int] * 7 + [c_voidp]),
    'ddsp_stft_frames_mag_backward_f32': (c_int, [c_f32p] * 3 + [c_int] * 6 + [c_voidp]),
    'ddsp_mel_features_f32': (c_int, [c_f32p] * 5 + [c_int] * 11 + [c_float, c_voidp]),
    'ddsp_frame_energy_f32': (c_int, [c_f32p] * 2 + [c_int] * 6 + [c_float] * 2 + [c_uint, c_voidp]),
    'ddsp_db_convert_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_float, c_float, c_voidp]),
    'ddsp_loudness_from_mag_f32': (c_int, [c_f32p] * 3 + [c_int] * 3 + [ctypes.c_float] * 2 + [c_voidp]),
    'ddsp_loudness_from_mag_backward_f32': (c_int, [c_f32p] * 4 + [c_int] * 3 + [ctypes.c_float] * 2 + [c_voidp]),
    'ddsp_uniform_noise_f32': (c_int, [c_f32p, c_int, c_int, c_u64, c_u64, c_voidp]),
    'ddsp_prepare': (c_int, [c_int, c_int, c_int]),
    'ddsp_uniform_noise_ex_f32': (c_int, [c_f32p, c_int, c_int, c_u64, c_u64, c_int, c_voidp]),
    'ddsp_add_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_voidp]),
    'ddsp_exp_sigmoid_f32': (c_int, [c_f32p] * 2 + [c_size_t] + [c_float] * 3 + [c_voidp]),
    'ddsp_oscillator_bank_workspace_bytes': (c_size_t, [c_int] * 3),
    'ddsp_oscillator_bank_f32': (c_int, [c_f32p] * 3 + [c_voidp, c_size_t] + [c_int] * 5 + [c_voidp]),
    'ddsp_resample_f32': (c_int, [c_f32p] * 2 + [c_int] * 5 + [c_voidp]),
    'ddsp_resample_ex_f32': (c_int, [c_f32p] * 2 + [c_int] * 6 + [c_voidp]),
    'ddsp_sum_rows_f32': (c_int, [c_f32p] * 2 + [c_int] * 3 + [c_voidp]),
    'ddsp_resample_ex_backward_f32': (c_int, [c_f32p] * 2 + [c_int] * 6 + [c_voidp]),
    'ddsp_oscillator_bank_grad_amplitudes_f32': (c_int, [c_f32p] * 3 + [c_voidp, c_size_t] + [c_int] * 4 + [c_voidp]),
    'ddsp_oscillator_bank_grad_frequencies_f32': (c_int, [c_f32p] * 4 + [c_voidp, c_size_t] + [c_int] * 4 + [c_voidp]),
    'ddsp_harmonic_frequencies_backward_f32': (c_int, [c_f32p] * 3 + [c_int] * 3 + [c_voidp]),
    'ddsp_harmonic_controls_backward_f32': (c_int, [c_f32p] * 6 + [c_int] * 4 + [c_uint, c_int, c_voidp]),
    'ddsp_fft_convolve_f32': (c_int, [c_f32p] * 3 + [c_int] * 7 + [c_voidp]),
    'ddsp_harmonic_envelopes_f32': (c_int, [c_f32p] * 6 + [c_int] * 3 + [c_voidp]),
    'ddsp_scale_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_voidp]),
    'ddsp_harmonic_oscillator_bank_workspace_bytes': (c_size_t, [c_int] * 2),
    'ddsp_harmonic_oscillator_bank_f32': (c_int, [c_f32p] * 5 + [c_voidp, c_size_t] + [c_int] * 5 + [c_voidp]),
    'ddsp_harmonic_f0_grad_workspace_bytes': (c_size_t, [c_int] * 4),
    'ddsp_harmonic_f0_grad_f32': (c_int, [c_f32p] * 5 + [c_voidp, c_size_t] + [c_int] * 5 +
                                  [c_uint, c_voidp]),
    'ddsp_exp_decay_ir_f32': (c_int, [c_f32p] * 4 + [c_int] * 2 + [c_uint, c_voidp]),
    'ddsp_exp_decay_ir_backward_workspace_bytes': (c_size_t, [c_int] * 2),
    'ddsp_exp_decay_ir_backward_f32': (c_int, [c_f32p] * 6 + [c_voidp, c_size_t] + [c_int] * 2 + [c_uint, c_voidp]),
    'ddsp_sigmoid_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_voidp]),
    'ddsp_mix_f32': (c_int, [c_f32p] * 4 + [c_size_t, c_int, c_voidp]),
    'ddsp_sigmoid_backward_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_voidp]),
    'ddsp_mix_backward_f32': (c_int, [c_f32p] * 7 + [c_size_t, c_int, c_voidp]),
    'ddsp_safe_divide_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_int, c_int, ctypes.c_float, c_voidp]),
    'ddsp_safe_log_f32': (c_int, [c_f32p] * 2 + [c_size_t, ctypes.c_float, c_voidp]),
    'ddsp_harmonic_frequencies_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_voidp]),
    'ddsp_remove_above_nyquist_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_float, c_voidp]),
    'ddsp_angular_cumsum_workspace_bytes': (c_size_t, [c_int] * 3),
    'ddsp_angular_cumsum_f32': (c_int, [c_f32p] * 2 + [c_voidp, c_size_t] + [c_int] * 3 + [c_voidp]),
    'ddsp_wavetable_f32': (c_int, [c_f32p] * 4 + [c_int] * 5 + [c_float, c_uint, c_voidp]),
    'ddsp_wavetable_backward_workspace_bytes': (c_size_t, [c_int] * 5),
    'ddsp_wavetable_backward_f32': (c_int, [c_f32p] * 7 + [c_voidp, c_size_t] + [c_int] * 5 + [c_float, c_uint, c_voidp]),
    'ddsp_linear_lookup_f32': (c_int, [c_f32p] * 3 + [c_int] * 4 + [c_voidp]),
    'ddsp_linear_lookup_backward_workspace_bytes': (c_size_t, [c_int] * 2),
    'ddsp_linear_lookup_backward_f32': (c_int, [c_f32p] * 5 + [c_voidp, c_size_t] + [c_int] * 4 + [c_voidp]),
    'ddsp_variable_length_delay_f32': (c_int, [c_f32p] * 4 + [c_int] * 3 + [c_float] * 2 + [c_uint, c_voidp]),
    'ddsp_variable_length_delay_backward_workspace_bytes': (c_size_t, [c_int] * 2),
    'ddsp_variable_length_delay_backward_f32': (c_int, [c_f32p] * 7 + [c_voidp, c_size_t] + [c_int] * 3 + [c_float] * 2 +
                                                [c_uint, c_voidp]),
    'ddsp_sinusoidal_controls_f32': (c_int, [c_f32p] * 4 + [c_size_t, c_int, c_int] + [c_float] * 3 + [c_uint, c_voidp]),
    'ddsp_sinusoidal_controls_backward_f32': (c_int, [c_f32p] * 6 + [c_size_t, c_int, c_int] + [c_float] * 3 + [c_uint, c_voidp]),
    'ddsp_sinusoidal_workspace_bytes': (c_size_t, [c_int] * 4),
    'ddsp_sinusoidal_signal_f32': (c_int, [c_f32p] * 3 + [c_voidp, c_size_t] + [c_int] * 4 + [c_float, c_uint, c_voidp]),
    'ddsp_sinusoidal_f32': (c_int, [c_f32p] * 5 + [c_voidp, c_size_t] + [c_int] * 5 + [c_float] * 3 + [c_uint, c_voidp]),
    'ddsp_sinusoidal_backward_workspace_bytes': (c_size_t, [c_int] * 4),
    'ddsp_sinusoidal_backward_f32': (c_int, [c_f32p] * 5 + [c_voidp, c_size_t] + [c_int] * 5 + [c_float] * 3 + [c_uint, c_voidp]),
    'ddsp_unit_convert_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_float, c_float, c_voidp]),
    'ddsp_twm_loss_tensors_f32': (c_int, [c_f32p] * 5 + [c_size_t] + [c_int] * 4 + [c_float] * 3 + [c_voidp]),
    'ddsp_twm_loss_tensors_backward_f32': (c_int, [c_f32p] * 9 + [c_size_t] + [c_int] * 4 + [c_float] * 3 + [c_voidp]),
    'ddsp_twm_softmin_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_int] + [c_float] * 3 + [c_voidp]),
    'ddsp_twm_softmin_backward_f32': (c_int, [c_f32p] * 5 + [c_size_t, c_int] + [c_float] * 3 + [c_voidp]),
    'ddsp_twm_nanargmin_f32': (c_int, [c_f32p] * 4 + [c_voidp, c_size_t, c_int] + [c_float] * 2 + [c_voidp]),
    'ddsp_kde_nll_f32': (c_int, [c_f32p] * 5 + [c_size_t, c_int, c_int, c_float, c_voidp]),
    'ddsp_kde_nll_backward_f32': (c_int, [c_f32p] * 9 + [c_size_t, c_int, c_int, c_float, c_voidp]),
    'ddsp_sinusoidal_to_harmonic_f32': (c_int, [c_f32p] * 5 + [c_size_t, c_int, c_int, c_float, c_float, c_uint, c_voidp]),
    'ddsp_sinusoidal_to_harmonic_backward_f32': (c_int, [c_f32p] * 8 + [c_size_t, c_int, c_int, c_float, c_float, c_uint, c_voidp]),
    'ddsp_mean_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_float, c_voidp]),
    'ddsp_mean_backward_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_float, c_voidp]),
    'ddsp_row_mean_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_voidp]),
    'ddsp_row_mean_backward_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_voidp]),
    'ddsp_unit_convert_backward_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_int, c_float, c_float, c_voidp]),
    'ddsp_wasserstein_f32': (c_int, [c_f32p] * 5 + [c_size_t] + [c_int] * 4 + [c_voidp]),
    'ddsp_wasserstein_backward_f32': (c_int, [c_f32p] * 9 + [c_size_t] + [c_int] * 4 + [c_voidp]),
    'ddsp_hmm_log_prob_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_int, c_int] + [c_double] * 7 + [c_voidp]),
    'ddsp_hmm_log_prob_backward_workspace_bytes': (c_size_t, [c_int] * 3),
    'ddsp_hmm_log_prob_backward_f32': (c_int, [c_f32p] * 5 + [c_voidp, c_size_t, c_size_t, c_int, c_int] + [c_double] * 7 + [c_voidp]),
    'ddsp_hmm_viterbi_workspace_bytes': (c_size_t, [c_int] * 3),
    'ddsp_hmm_viterbi_f32': (c_int, [c_f32p] * 3 + [c_voidp, c_size_t, c_size_t, c_int, c_int] + [c_double] * 7 + [c_voidp]),
    'ddsp_note_mask_f32': (c_int, [c_f32p] * 3 + [c_size_t] + [c_int] * 3 + [c_voidp]),
    'ddsp_note_moments_f32': (c_int, [c_f32p] * 7 + [c_size_t] + [c_int] * 4 + [c_voidp]),
    'ddsp_note_spread_f32': (c_int, [c_f32p] * 7 + [c_size_t] + [c_int] * 3 + [c_voidp]),
    'ddsp_fft_convolve_grad_audio_f32': (c_int, [c_f32p] * 3 + [c_int] * 7 + [c_voidp]),
    'ddsp_fft_convolve_grad_ir_f32': (c_int, [c_f32p] * 3 + [c_int] * 6 + [c_voidp]),
    'ddsp_sinc_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_float, c_voidp]),
    'ddsp_sinc_impulse_response_size': (c_int, [c_int]),
    'ddsp_sinc_impulse_response_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_float, c_int, c_voidp]),
    'ddsp_sinc_impulse_response_backward_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_int, c_float, c_int, c_voidp]),
    'ddsp_frequency_impulse_response_backward_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_int, c_int, c_voidp]),
    'ddsp_exp_sigmoid_backward_f32': (c_int, [c_f32p] * 3 + [c_size_t] + [c_float] * 3 + [c_voidp]),
    'ddsp_critical_bands_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_int] + [c_f32p] * 3 + [c_float] * 3 + [c_voidp]),
    'ddsp_critical_bands_backward_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_int, c_int] + [c_f32p] * 3 + [c_float] * 3 + [c_voidp]),
    'ddsp_harmonic_wavetable_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_int, c_float, c_voidp]),
    'ddsp_harmonic_wavetable_backward_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_int, c_float, c_voidp]),
    'ddsp_scale_convert_f32': (c_int, [c_f32p] * 2 + [c_size_t, c_int, c_float, c_float, c_voidp]),
    'ddsp_scale_convert_backward_f32': (c_int, [c_f32p] * 3 + [c_size_t, c_int, c_float, c_float, c_voidp]),
    'ddsp_profile_kernel_count': (c_int, []),
    'ddsp_profile_kernel_name': (ctypes.c_char_p, [c_int]),
    'ddsp_profile_begin': (c_int, [c_uint, c_int]),
    'ddsp_profile_begin_sampled': (c_int, [c_uint, c_int, c_int]),
    'ddsp_profile_end': (c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(c_int)]),
}

# name -> (restype, argtypes) of the entries of csrc/decoder_abi.h (training.nn's layers, training.decoders).  A table of its
# own for now: tests pin SIGNATURES to include/ddsp_amd.h and to a layout table; decoder_entry() types these on any library object.
DECODER_SIGNATURES = {
    'ddsp_bias_norm_act_f32': (c_int, [c_f32p] * 7 + [c_size_t, c_int, c_int, c_float, c_voidp]),
    'ddsp_bias_norm_act_backward_workspace_bytes': (c_size_t, [c_size_t, c_int]),
    'ddsp_bias_norm_act_backward_f32': (c_int, [c_f32p] * 7 + [c_voidp, c_size_t, c_size_t, c_int, c_int, c_voidp]),
    'ddsp_gru_forward_workspace_bytes': (c_size_t, [c_int] * 2),
    'ddsp_gru_forward_f32': (c_int, [c_f32p] * 6 + [c_voidp, c_size_t] + [c_int] * 3 + [c_voidp]),
    'ddsp_gru_backward_workspace_bytes': (c_size_t, [c_int] * 2),
    'ddsp_gru_backward_f32': (c_int, [c_f32p] * 8 + [c_voidp, c_size_t] + [c_int] * 3 + [c_voidp]),
}

# name -> (restype, argtypes) of the entries of csrc/norm_abi.h (training.nn's normalize_op / Normalize), typed by norm_entry():
# a table of its own for the same reason.
NORM_SIGNATURES = {
    'ddsp_group_norm_workspace_bytes': (c_size_t, [c_size_t, c_size_t, c_int, c_int]),
    'ddsp_group_norm_f32': (c_int, [c_f32p] * 6 + [c_voidp, c_size_t, c_size_t, c_size_t, c_int, c_int, c_float, c_voidp]),
    'ddsp_group_norm_backward_workspace_bytes': (c_size_t, [c_size_t, c_size_t, c_int, c_int]),
    'ddsp_group_norm_backward_f32': (c_int, [c_f32p] * 8 + [c_voidp, c_size_t, c_size_t, c_size_t, c_int, c_int, c_voidp]),
}

# name -> (restype, argtypes) of the entries of csrc/conv_abi.h (training.nn's dilated_conv / Conv2D / DilatedConvStack), typed by
# conv_entry(): a table of its own for the same reason.
CONV_SIGNATURES = {
    'ddsp_dilated_conv_workspace_bytes': (c_size_t, [c_int] * 5),
    'ddsp_dilated_conv_f32': (c_int, [c_f32p] * 6 + [c_voidp, c_size_t] + [c_int] * 7 + [c_uint, c_voidp]),
}

# name -> (restype, argtypes) of the entries of csrc/conv2d_abi.h (training.nn's conv2d / SpatialConv2D / ResNet), typed by
# conv2d_entry(): a table of its own for the same reason.
CONV2D_SIGNATURES = {
    'ddsp_conv2d_workspace_bytes': (c_size_t, [c_int] * 9 + [c_uint]),
    'ddsp_conv2d_f32': (c_int, [c_f32p] * 6 + [c_voidp, c_size_t] + [c_int] * 9 + [c_uint, c_voidp]),
}

# name -> (restype, argtypes) of the entries of csrc/vq_abi.h (training.nn's vq_assign / vq_statistics / VectorQuantization), typed
# by vq_entry(): a table of its own for the same reason.
VQ_SIGNATURES = {
    'ddsp_vq_workspace_bytes': (c_size_t, [c_int] * 2),
    'ddsp_vq_assign_f32': (c_int, [c_f32p] * 4 + [c_voidp, c_size_t] + [c_int] * 4 + [c_voidp]),
    'ddsp_vq_statistics_f32': (c_int, [c_f32p] * 4 + [c_int] * 4 + [c_voidp]),
}

# flags (mirror include/ddsp_amd.h)
HARM_SCALE_EXP_SIGMOID = 0x1
HARM_NORMALIZE_NYQUIST = 0x2
HARM_AMP_LINEAR = 0x4
HARM_ANGULAR_CUMSUM = 0x8
HARM_INPUTS_ARE_AMPLITUDES = 0x20
HARM_DIRECT_SUM = 0x40
NOISE_SCALE_EXP_SIGMOID = 0x1
NOISE_FIR_VECTOR_ALU = 0x8
NOISE_BITS_23 = 0x10
DECAY_SCALE_EXP_SIGMOID = 0x1
WT_SCALE_EXP_SIGMOID = 0x1
DELAY_ADD_DRY = 0x1
DELAY_GAIN_EXP_SIGMOID = 0x2
DELAY_PHASE_SIGMOID = 0x4
SIN_AMP_EXP_SIGMOID = 0x1
SIN_FREQ_SIGMOID = 0x2
SIN_FREQ_SOFTMAX = 0x4
SIN_MASK_NYQUIST = 0x8
SIN_AMP_LINEAR = 0x10
SIN_MAX_SIGMOID_DEPTH = 64
CONVERT_OPS = {'midi_to_hz': 0, 'midi_to_hz_zero_silence': 1, 'hz_to_midi': 2, 'unit_to_midi': 3, 'unit_to_midi_clip': 4,
               'midi_to_unit': 5, 'midi_to_unit_clip': 6, 'logb': 7, 'log_floor': 8}
SCALE_OPS = {'hz_to_bark': 0, 'bark_to_hz': 1, 'hz_to_mel': 2, 'mel_to_hz': 3, 'hz_to_erb': 4, 'soft_limit': 5, 'log_scale': 6,
             'sym_exp_sigmoid': 7, 'nan_to_num': 8}
HARMONIC_WAVETABLE_SIZES = (64, 8192)   # powers of two the fused kernel of csrc/harmonic_wavetable.hip transforms
DB_OPS = {'power_to_db': 0, 'amplitude_to_db': 1, 'db_to_power': 2, 'db_to_amplitude': 3}
MEL_MODES = {'mel': 0, 'logmel': 1, 'mfcc': 2}
ENERGY_DB = 0x1
S2H_NORMALIZE = 0x1
WASSERSTEIN_MIDI = 0x1
CONSISTENCY_MAX_K = 1024                # sinusoids / harmonics a frame's block stages in LDS (csrc/consistency.hip, wasserstein.hip)
CONSISTENCY_MAX_POINTS = 256
CONSISTENCY_MAX_GAUSSIANS = 4096
HMM_MAX_PITCHES = 1024                  # states of HmmTranscriber a block holds in registers (csrc/hmm.hip)
NOTES_SUM = 0x1
ACTIVATIONS = {'linear': 0, 'leaky_relu': 1, 'relu': 2, 'sigmoid': 3, 'tanh': 4}    # DDSP_ACT_* of csrc/decoder_abi.h
GRU_MAX_HIDDEN = 2048                   # units of the GRU (csrc/decoder.hip)
NOTES_MAX_REGIONS = 1024                # regions whose note-on flags get_note_mask's block keeps in LDS (csrc/notes.hip)
RESAMPLE_METHODS = {'nearest': 0, 'linear': 1, 'cubic': 2, 'window': 3}
LOSS_TYPES = {'L1': 0, 'L2': 1, 'COSINE': 2}
CONVD_RELU_INPUT = 0x1                  # DDSP_CONVD_* of csrc/conv_abi.h
CONVD_TRANSPOSE_W = 0x2
CONVD_MASK_OUTPUT = 0x4
CONVD_MAX_CHANNELS = 1024               # ch_in, ch_out of the dilated convolution (csrc/dilated_conv.hip)
CONVD_MAX_TAPS = 16
CONV2D_RELU_INPUT = 0x1                 # DDSP_CONV2D_* of csrc/conv2d_abi.h
CONV2D_ADJOINT = 0x2
CONV2D_MASK_OUTPUT = 0x4
CONV2D_MAX_CHANNELS = 1024              # ch_in, ch_out of the 2-D convolution (csrc/conv2d.hip)
CONV2D_MAX_TAPS = 64                    # kh * kw
CONV2D_MAX_STRIDE = 8
CONV2D_MAX_SIDE = 2 ** 30               # h, w
VQ_MAX_CENTROIDS = 4096                 # DDSP_VQ_* of csrc/vq_abi.h: k and the width of a head of the vector quantizer (csrc/vq.hip)
VQ_MAX_DIMS = 512
CONV_ADD_DRY = 0x1
CONV_MASK_TAP0 = 0x2
CONV_REVERSE_AUDIO = 0x4
CONV_REVERSE_IR = 0x8
CONV_REVERSE_OUT = 0x10
CONV_ZERO_OUT0 = 0x20

ERR_UNSUPPORTED = -3
ERRORS = {-1: 'DDSP_ERR_NULL_POINTER', -2: 'DDSP_ERR_BAD_SHAPE', -3: 'DDSP_ERR_UNSUPPORTED',
          -4: 'DDSP_ERR_WORKSPACE', -5: 'DDSP_ERR_LAUNCH'}

_lib = None


class DdspLibraryError(RuntimeError):
  pass


def load():
  """Load libddsp_amd.so (once) and type every entry point.  Raises if unavailable."""
  global _lib
  if _lib is not None:
    return _lib
  if not os.path.exists(LIB_PATH):
    raise DdspLibraryError(
        'HIP library not built: %s is missing. Run `python -c "import __graft_entry__ as g; '
        'g.build()"` (or `python -m ddsp_amd.build`). There is no CPU fallback.' % LIB_PATH)
  # torch must be imported first so that libamdhip64.so.7 resolves to the HIP runtime torch
  # already loaded: one runtime per process, device pointers are shared with torch.
  import torch  # noqa: F401
  lib = ctypes.CDLL(LIB_PATH)
  for name, (restype, argtypes) in SIGNATURES.items():
    fn = getattr(lib, name)       # AttributeError here == a declared symbol is not exported
    fn.restype = restype
    fn.argtypes = argtypes
  for name in DECODER_SIGNATURES:
    decoder_entry(lib, name)
  for name in NORM_SIGNATURES:
    norm_entry(lib, name)
  for name in CONV_SIGNATURES:
    conv_entry(lib, name)
  for name in CONV2D_SIGNATURES:
    conv2d_entry(lib, name)
  for name in VQ_SIGNATURES:
    vq_entry(lib, name)
  _lib = lib
  return lib


def decoder_entry(lib, name):
  """Entry `name` of DECODER_SIGNATURES on `lib` (whatever load() returned), typed; typing twice changes nothing."""
  fn = getattr(lib, name)         # AttributeError here == the library was built without csrc/decoder.hip
  fn.restype, fn.argtypes = DECODER_SIGNATURES[name]
  return fn


def norm_entry(lib, name):
  """Entry `name` of NORM_SIGNATURES on `lib` (whatever load() returned), typed; typing twice changes nothing."""
  fn = getattr(lib, name)         # AttributeError here == the library was built without csrc/group_norm.hip
  fn.restype, fn.argtypes = NORM_SIGNATURES[name]
  return fn


def conv_entry(lib, name):
  """Entry `name` of CONV_SIGNATURES on `lib` (whatever load() returned), typed; typing twice changes nothing."""
  fn = getattr(lib, name)         # AttributeError here == the library was built without csrc/dilated_conv.hip
  fn.restype, fn.argtypes = CONV_SIGNATURES[name]
  return fn


def conv2d_entry(lib, name):
  """Entry `name` of CONV2D_SIGNATURES on `lib` (whatever load() returned), typed; typing twice changes nothing."""
  fn = getattr(lib, name)         # AttributeError here == the library was built without csrc/conv2d.hip
  fn.restype, fn.argtypes = CONV2D_SIGNATURES[name]
  return fn


def vq_entry(lib, name):
  """Entry `name` of VQ_SIGNATURES on `lib` (whatever load() returned), typed; typing twice changes nothing."""
  fn = getattr(lib, name)         # AttributeError here == the library was built without csrc/vq.hip
  fn.restype, fn.argtypes = VQ_SIGNATURES[name]
  return fn


def check(rc, what):
  if rc != 0:
    raise DdspLibraryError('%s failed: %s (%d)' % (what, ERRORS.get(rc, 'unknown'), rc))


def profile_begin(kernel_names=None, max_records=4096, stride=1):
  """Start per-kernel HIP-event tracing; kernel_names=None traces every kernel.

  stride=n brackets only every n-th launch of each selected kernel (a bracketed launch costs
  ~5 us of queue time, so a timed region samples instead of bracketing everything)."""
  lib = load()
  n = lib.ddsp_profile_kernel_count()
  names = [lib.ddsp_profile_kernel_name(i).decode() for i in range(n)]
  mask = 0
  for i, nm in enumerate(names):
    if kernel_names is None or nm in kernel_names:
      mask |= 1 << i
  check(lib.ddsp_profile_begin_sampled(mask, int(max_records), int(stride)),
        'ddsp_profile_begin_sampled')


def profile_end():
  """Stop tracing; returns {kernel_name: (total_ms, count)} for kernels that ran."""
  lib = load()
  n = lib.ddsp_profile_kernel_count()
  ms = (ctypes.c_double * n)()
  cnt = (c_int * n)()
  check(lib.ddsp_profile_end(ms, cnt), 'ddsp_profile_end')
  return {lib.ddsp_profile_kernel_name(i).decode(): (ms[i], cnt[i])
          for i in range(n) if cnt[i] > 0}
