"""The table tests/test_gpu_layouts.py is driven by: one Row per public callable of ddsp_amd that reaches the kernel library -
its name, the call, and how each tensor argument is made.  A new entry point is one more row; tests/test_layouts_table.py
checks that every C entry of ddsp_amd._lib.SIGNATURES is reached by some row or named in EXEMPT with its reason.

Shapes are the smallest at which each address-dependent dispatch of csrc/ has its SHAPE condition true, so that the pointer
alone decides ("Layouts and addresses", has the branch / condition / case table):
  Harmonic       B=2, F=8, hop 64, K=8 (F % 4 == 0, K % 4 == 0); K=100 once for the table kernel's wide rows
  FilteredNoise  F=8, N=512, 65 bands and 64 (M % 4 == 0)
  fft_convolve   an even tap count; 128 taps on frames of 64 for the tiled kernel
  SpectralLoss   N=512 (N % 4 == 0), fft sizes (128, 64)
  wavetables     64 points
  Reverb         N=512, L=256, one impulse response and one per row
  the rest       B=2, T=5..16, K=8"""
import numpy as np
import torch

import ddsp_amd.training.nn  # noqa: F401  (rows reach it as ddsp.training.nn)


class Arg:
  """One tensor argument: `make(rng)` gives its fp32 values; grad - the entry is differentiable in it; expand - the axis along
  which the entry broadcasts it (the 'expanded' variant holds it with stride 0 there)."""

  def __init__(self, name, shape, make, grad=True, expand=None):
    self.name, self.shape, self.make, self.grad, self.expand = name, tuple(shape), make, grad, expand

  def values(self, rng):
    out = np.asarray(self.make(rng, self.shape), np.float32)
    assert out.shape == self.shape, (self.name, out.shape, self.shape)
    return out


def N(name, *shape, scale=1.0, **kw):
  return Arg(name, shape, lambda rng, s: scale * rng.standard_normal(s), **kw)


def U(name, *shape, lo=0.1, hi=1.0, **kw):
  return Arg(name, shape, lambda rng, s: rng.uniform(lo, hi, s), **kw)


def F(name, shape, fn, **kw):
  return Arg(name, shape, lambda rng, s: fn(rng, s), **kw)


class Row:
  """name; call(ddsp, *tensors) -> a tensor, a tuple / list / dict of tensors; the arguments.  scalar: no output has two axes longer than 1 (no
  transposed gradient seed).  numpy: the entry takes numpy arrays (core.tf_float32 documents it; the few that look at a tensor's
  device before converting do not).  atomic_grad: the gradient is overlap-added with fp32 atomics, whose order the README excepts
  from bit-stability (SpectralLoss without deterministic=True): outputs are held to bits, the gradient to the suite's bound for
  "same kernel, atomics order only" (tests/test_gpu_parity.py: 1e-5 of the largest gradient)."""

  def __init__(self, name, call, args, scalar=False, numpy=True, atomic_grad=False):
    self.name, self.call, self.args, self.scalar, self.numpy = name, call, list(args), scalar, numpy
    self.atomic_grad = atomic_grad

  @property
  def differentiable(self):
    return any(a.grad for a in self.args)


B, T, K = 2, 5, 8
FR, HOP = 8, 64
NS = FR * HOP          # 512


def _harmonic(kernel='auto', method='window', n=NS, **kw):
  def call(d, amps, hd, f0):
    synth = d.synths.Harmonic(n_samples=n, amp_resample_method=method, **kw)
    synth.kernel = kernel
    return synth(amps, hd, f0)
  return call


def _harmonic_args(k=K, f=FR):
  return [N('amplitudes', B, f, 1, expand=0), N('harmonic_distribution', B, f, k, expand=0),
          U('f0_hz', B, f, 1, lo=180.0, hi=260.0, expand=0)]


def _noise(window_size=0, supplied=True, kernel='auto', **kw):
  def call(d, mags, *noise):
    synth = d.synths.FilteredNoise(n_samples=NS, window_size=window_size, **kw)     # (a new one: the call counter keys the noise)
    synth.kernel = kernel
    return synth(mags, noise=noise[0]) if supplied else synth(mags)
  return call


def _noise_args(m, supplied=True):
  args = [N('magnitudes', B, FR, m, expand=0)]
  return args + [U('noise', B, NS, lo=-1.0, hi=1.0, grad=False)] if supplied else args


def _group(d, amps, hd, f0, mags, ir):
  dag = [(d.synths.Harmonic(n_samples=NS), ['amps', 'hd', 'f0']),
         (d.synths.FilteredNoise(n_samples=NS, window_size=0), ['mags']),
         (d.processors.Add(), ['filtered_noise/signal', 'harmonic/signal']),
         (d.effects.Reverb(reverb_length=256), ['add/signal', 'ir'])]
  return d.processors.ProcessorGroup(dag=dag)(dict(amps=amps, hd=hd, f0=f0, mags=mags, ir=ir))


def _spectral(**kw):
  def call(d, target, audio, *weights):
    loss = d.losses.SpectralLoss(fft_sizes=(128, 64), **kw)
    return loss(target, audio, weights=weights[0]) if weights else loss(target, audio)
  return call


def _audio(name='audio', n=NS, **kw):
  return N(name, B, n, scale=0.3, **kw)


def _note_mask_values(rng, shape):
  mask = np.zeros(shape, np.float32)
  mask[:, :4, 0] = 1.0
  mask[:, 4:9, 1] = 1.0
  mask[:, 9:, 2] = 1.0
  return mask


def _pitch_values(rng, shape):
  steps = np.array([60, 60, 60, 62, 62, 0, 0, 64, 64, 64, 64, 65], np.float32)
  return np.broadcast_to(steps[None, :, None], shape).copy()


def _elementwise(fn_name, **kwargs):
  return lambda d, x: getattr(d.core, fn_name)(x, **kwargs)


def _ew_row(fn_name, lo, hi, grad=True, **kwargs):
  return Row('core.' + fn_name, _elementwise(fn_name, **kwargs), [U('x', B, T, K, lo=lo, hi=hi, grad=grad)])


ROWS = [
    # ---- synths and processors
    Row('Harmonic/table', _harmonic(), _harmonic_args()),
    Row('Harmonic/table_k100', _harmonic(), _harmonic_args(k=100)),
    Row('Harmonic/direct', _harmonic(kernel='direct'), _harmonic_args()),
    Row('Harmonic/chain_linear', _harmonic(method='linear'), _harmonic_args()),
    Row('Harmonic/chain_cubic', _harmonic(method='cubic'), _harmonic_args()),
    Row('FilteredNoise/m65_supplied', _noise(), _noise_args(65)),
    Row('FilteredNoise/m64_supplied', _noise(), _noise_args(64)),
    Row('FilteredNoise/m65_generated', _noise(supplied=False), _noise_args(65, False)),
    Row('FilteredNoise/m64_generated', _noise(supplied=False), _noise_args(64, False)),
    Row('FilteredNoise/m65_vector', _noise(kernel='vector'), _noise_args(65)),
    Row('FilteredNoise/m33_w17', _noise(window_size=17), _noise_args(33)),
    Row('Sinusoidal', lambda d, a, f: d.synths.Sinusoidal(n_samples=320)(a, f), [N('amplitudes', B, T, K, expand=0), N('frequencies', B, T, K, expand=0)]),
    Row('Wavetable', lambda d, a, w, f: d.synths.Wavetable(n_samples=320)(a, w, f),
        [N('amplitudes', B, T, 1, expand=0), N('wavetables', B, T, 64, expand=0), U('f0_hz', B, T, 1, lo=100.0, hi=400.0, expand=0)]),
    Row('Add', lambda d, a, b: d.processors.Add()(a, b), [_audio('signal_one', expand=0), _audio('signal_two', expand=0)]),
    Row('Mix', lambda d, a, b, m: d.processors.Mix()(a, b, m), [_audio('signal_one'), _audio('signal_two'), N('mix_level', B, FR, 1)]),
    Row('ProcessorGroup', _group, _harmonic_args() + [N('magnitudes', B, FR, 65, expand=0), N('ir', B, 256, scale=0.05, expand=0)]),
    # ---- effects
    Row('Reverb/ir_per_row', lambda d, a, ir: d.effects.Reverb(reverb_length=256)(a, ir), [_audio(), N('ir', B, 256, scale=0.05)]),
    Row('Reverb/one_ir', lambda d, a, ir: d.effects.Reverb(reverb_length=256)(a, ir), [_audio(), N('ir', 1, 256, scale=0.05)]),
    Row('ExpDecayReverb', lambda d, a, g, dec: d.effects.ExpDecayReverb(reverb_length=256)(a, g, dec),
        [_audio(), N('gain', B, 1), N('decay', B, 1)]),
    Row('FilteredNoiseReverb', lambda d, a, m: d.effects.FilteredNoiseReverb(reverb_length=256, window_size=17, n_frames=4, n_filter_banks=8)(a, m),
        [_audio(), N('magnitudes', B, 4, 8)]),
    Row('FIRFilter', lambda d, a, m: d.effects.FIRFilter(window_size=0)(a, m), [_audio(n=320), N('magnitudes', B, T, 9)]),
    Row('ModDelay', lambda d, a, g, p: d.effects.ModDelay()(a, g, p), [_audio(n=320), N('gain', B, 320, 1), N('phase', B, 320, 1)]),
    # ---- losses
    Row('SpectralLoss', _spectral(logmag_weight=1.0), [_audio('target_audio', grad=False), _audio()], scalar=True, atomic_grad=True),
    Row('SpectralLoss/deterministic', _spectral(logmag_weight=1.0, deterministic=True), [_audio('target_audio', grad=False), _audio()],
        scalar=True),
    Row('SpectralLoss/general', _spectral(delta_time_weight=1.0, delta_freq_weight=1.0, cumsum_freq_weight=1.0, loudness_weight=1.0),
        [_audio('target_audio', grad=False), _audio()], scalar=True, atomic_grad=True),
    Row('SpectralLoss/weights', _spectral(), [_audio('target_audio', grad=False), _audio(), U('weights', B, 1, 1, grad=False)], scalar=True,
        atomic_grad=True),
    Row('mean_difference/L1', lambda d, t, v, w: d.losses.mean_difference(t, v, 'L1', w),
        [N('target', B, T, K), N('value', B, T, K), U('weights', B, T, K, grad=False)], scalar=True),
    Row('mean_difference/L2', lambda d, t, v, w: d.losses.mean_difference(t, v, 'L2', w),
        [N('target', B, T, K), N('value', B, T, K), U('weights', B, T, K, grad=False)], scalar=True),
    Row('mean_difference/COSINE', lambda d, t, v, w: d.losses.mean_difference(t, v, 'COSINE', w),
        [N('target', B, T, K), N('value', B, T, K), U('weights', B, T, 1, grad=False)], scalar=True),
    Row('KDEConsistencyLoss', lambda d, aa, fa, ab, fb: d.losses.KDEConsistencyLoss()(aa, fa, ab, fb),
        [U('amps_a', B, T, K), U('freqs_a', B, T, K, lo=100.0, hi=4000.0), U('amps_b', B, T, K), U('freqs_b', B, T, K, lo=100.0, hi=4000.0)],
        scalar=True),
    Row('TWMLoss', lambda d, c, f, a: d.losses.TWMLoss()(c, f, a),
        [U('f0_candidates', B, T, 4, lo=100.0, hi=400.0), U('freqs', B, T, K, lo=100.0, hi=4000.0), U('amps', B, T, K)], scalar=True),
    Row('wasserstein_distance', lambda d, u, v, uw, vw: d.losses.wasserstein_distance(u, v, uw, vw),
        [N('u_values', B, T, K), N('v_values', B, T, K), U('u_weights', B, T, K), U('v_weights', B, T, K)]),
    Row('WassersteinConsistencyLoss', lambda d, aa, fa, ab, fb: d.losses.WassersteinConsistencyLoss()(aa, fa, ab, fb),
        [U('amps_a', B, T, K), U('freqs_a', B, T, K, lo=100.0, hi=4000.0), U('amps_b', B, T, K), U('freqs_b', B, T, K, lo=100.0, hi=4000.0)],
        scalar=True),
    Row('HmmTranscriber.nll', lambda d, p, a: d.losses.HmmTranscriber(n_timesteps=16, n_pitches=8).nll(p, a, per_example_loss=True),
        [U('pitches', B, 16, 1, lo=0.0, hi=7.0), U('amps', B, 16, 1, lo=0.0, hi=2.0)], scalar=True),
    Row('HmmTranscriber.predict_midi', lambda d, p, a: d.losses.HmmTranscriber(n_timesteps=16, n_pitches=8).predict_midi(p, a),
        [U('pitches', B, 16, 1, lo=0.0, hi=7.0, grad=False), U('amps', B, 16, 1, lo=0.0, hi=2.0, grad=False)]),
    # ---- spectral ops
    Row('spectral_ops.stft', lambda d, a: torch.view_as_real(d.spectral_ops.stft(a, frame_size=128)), [_audio(grad=False)]),
    Row('spectral_ops.compute_mag', lambda d, a: d.spectral_ops.compute_mag(a, size=128), [_audio(grad=False)]),
    Row('spectral_ops.compute_loudness', lambda d, a: d.spectral_ops.compute_loudness(a, n_fft=128), [_audio(grad=False)]),
    Row('spectral_ops.compute_mel', lambda d, a: d.spectral_ops.compute_mel(a, bins=16, fft_size=128), [_audio(grad=False)]),
    Row('spectral_ops.compute_logmel', lambda d, a: d.spectral_ops.compute_logmel(a, bins=16, fft_size=128), [_audio(grad=False)]),
    Row('spectral_ops.compute_mfcc', lambda d, a: d.spectral_ops.compute_mfcc(a, fft_size=128, mel_bins=16, mfcc_bins=5), [_audio(grad=False)]),
    Row('spectral_ops.compute_rms_energy', lambda d, a: d.spectral_ops.compute_rms_energy(a, frame_size=128), [_audio(grad=False)]),
    Row('spectral_ops.compute_power', lambda d, a: d.spectral_ops.compute_power(a, frame_size=128), [_audio(grad=False)]),
    # ---- core
    Row('core.fft_convolve/same_tiled_128', lambda d, a, ir: d.core.fft_convolve(a, ir), [_audio(), N('impulse_response', B, FR, 128, scale=0.05)]),
    Row('core.fft_convolve/same_even', lambda d, a, ir: d.core.fft_convolve(a, ir), [_audio(n=320), N('impulse_response', B, T, 16, scale=0.1)]),
    Row('core.fft_convolve/valid_even', lambda d, a, ir: d.core.fft_convolve(a, ir, padding='valid'),
        [_audio(n=320), N('impulse_response', B, T, 16, scale=0.1)]),
    Row('core.fft_convolve/one_ir', lambda d, a, ir: d.core.fft_convolve(a, ir), [_audio(n=320), N('impulse_response', 1, T, 16, scale=0.1)]),
    Row('core.frequency_filter', lambda d, a, m: d.core.frequency_filter(a, m, window_size=16), [_audio(n=320), U('magnitudes', B, T, 9)]),
    Row('core.sinc_filter', lambda d, a, c: d.core.sinc_filter(a, c, window_size=16, sample_rate=16000),
        [_audio(n=320), U('cutoff_frequency', B, T, 1, lo=500.0, hi=4000.0)]),
    Row('core.oscillator_bank', lambda d, f, a: d.core.oscillator_bank(f, a), [U('frequency_envelopes', B, 320, K, lo=100.0, hi=4000.0, grad=False),
                                                                                U('amplitude_envelopes', B, 320, K, grad=False)]),
    Row('core.linear_lookup', lambda d, p, w: d.core.linear_lookup(p, w), [U('phase', B, 320, 1, lo=0.0, hi=1.0), N('wavetables', B, 320, 64)]),
    Row('core.variable_length_delay', lambda d, p, a: d.core.variable_length_delay(p, a, max_length=64),
        [U('phase', B, 320, 1, lo=0.0, hi=1.0), _audio(n=320)]),
    Row('core.sinusoidal_to_harmonic', lambda d, a, f, f0: d.core.sinusoidal_to_harmonic(a, f, f0, n_harmonics=K),
        [U('sin_amps', B, T, K), U('sin_freqs', B, T, K, lo=100.0, hi=4000.0), U('f0_hz', B, T, 1, lo=100.0, hi=400.0)]),
    Row('core.frequencies_critical_bands/depth1', lambda d, x: d.core.frequencies_critical_bands(x), [N('freqs', B, T, K)]),
    Row('core.frequencies_critical_bands/depth4', lambda d, x: d.core.frequencies_critical_bands(x, depth=4), [N('freqs', B, T, 4 * K)]),
    Row('core.harmonic_distribution_to_wavetable/fused', lambda d, x: d.core.harmonic_distribution_to_wavetable(x, n_wavetable=64),
        [U('harmonic_distribution', B, T, K)]),
    Row('core.harmonic_distribution_to_wavetable/irfft', lambda d, x: d.core.harmonic_distribution_to_wavetable(x, n_wavetable=48),
        [U('harmonic_distribution', B, T, K)]),
    Row('core.exp_sigmoid', lambda d, x: d.core.exp_sigmoid(x), [N('x', B, T, K)]),
    Row('core.streaming_harmonic_synthesis', lambda d, f, a, hd: d.core.streaming_harmonic_synthesis(f, a, hd, n_samples=NS),
        [U('frequencies', B, FR, 1, lo=180.0, hi=260.0, grad=False), U('amplitudes', B, FR, 1, grad=False),
         U('harmonic_distribution', B, FR, K, grad=False)]),
    # ---- note pooling
    Row('nn.get_note_mask', lambda d, q: d.training.nn.get_note_mask(q, max_regions=4), [F('q_pitch', (B, 12, 1), _pitch_values, grad=False)]),
    Row('nn.get_note_moments', lambda d, x, m: d.training.nn.get_note_moments(x, m), [N('x', B, 12, 4), F('note_mask', (B, 12, 3), _note_mask_values, grad=False)]),
    Row('nn.pool_over_notes', lambda d, x, m: d.training.nn.pool_over_notes(x, m),
        [N('x', B, 12, 4), F('note_mask', (B, 12, 3), _note_mask_values, grad=False, expand=0)]),
]
for _method in ('nearest', 'linear', 'cubic', 'window'):
  ROWS.append(Row('core.resample/' + _method, (lambda m: lambda d, x: d.core.resample(x, 320, method=m))(_method), [N('inputs', B, T, K, grad=False)]))
ROWS += [
    _ew_row('midi_to_hz', 20.0, 90.0, grad=False), _ew_row('hz_to_midi', 50.0, 4000.0, grad=False), _ew_row('unit_to_midi', 0.0, 1.0, grad=False),
    _ew_row('midi_to_unit', 20.0, 90.0, grad=False), _ew_row('unit_to_hz', 0.0, 1.0, grad=False, hz_min=20.0, hz_max=8000.0),
    _ew_row('hz_to_unit', 50.0, 4000.0, grad=False, hz_min=20.0, hz_max=8000.0),
    _ew_row('power_to_db', 1e-4, 2.0, grad=False), _ew_row('amplitude_to_db', 1e-3, 2.0, grad=False), _ew_row('db_to_power', -60.0, 3.0, grad=False),
    _ew_row('db_to_amplitude', -60.0, 3.0, grad=False),
    _ew_row('hz_to_bark', 50.0, 4000.0), _ew_row('bark_to_hz', 1.0, 20.0), _ew_row('hz_to_mel', 50.0, 4000.0), _ew_row('mel_to_hz', 50.0, 2500.0),
    _ew_row('hz_to_erb', 50.0, 4000.0), _ew_row('soft_limit', -2.0, 3.0), _ew_row('log_scale', -1.0, 1.0, min_x=20.0, max_x=8000.0),
    _ew_row('sym_exp_sigmoid', -3.0, 3.0), _ew_row('nan_to_num', -1.0, 1.0), _ew_row('logb', 0.1, 100.0, grad=False),
    _ew_row('safe_log', 0.1, 100.0, grad=False),
]

ROWS += [
    # ---- the two-step forms of the synths, and the rest of core that reaches the library
    Row('Harmonic.get_controls', lambda d, a, h, f: d.synths.Harmonic(n_samples=NS).get_controls(a, h, f),
        [N('amplitudes', B, FR, 1, grad=False), N('harmonic_distribution', B, FR, K, grad=False), U('f0_hz', B, FR, 1, lo=180.0, hi=260.0, grad=False)]),
    Row('Harmonic.get_signal', lambda d, a, h, f: d.synths.Harmonic(n_samples=NS).get_signal(a, h, f),
        [U('amplitudes', B, FR, 1, grad=False), U('harmonic_distribution', B, FR, K, grad=False), U('f0_hz', B, FR, 1, lo=180.0, hi=260.0, grad=False)]),
    Row('core.harmonic_synthesis/tf_op_order', lambda d, f, a, h: d.core.harmonic_synthesis(f, a, harmonic_distribution=h, n_samples=NS, tf_op_order=True),
        [U('frequencies', B, FR, 1, lo=180.0, hi=260.0, grad=False), U('amplitudes', B, FR, 1, grad=False), U('harmonic_distribution', B, FR, K, grad=False)]),
    # 72 harmonics: two blocks of 64 add into an audio buffer the entry clears first (two addends: the order cannot show)
    Row('core.harmonic_synthesis/tf_op_order_k72', lambda d, f, a, h: d.core.harmonic_synthesis(f, a, harmonic_distribution=h, n_samples=NS, tf_op_order=True),
        [U('frequencies', B, FR, 1, lo=60.0, hi=100.0, grad=False), U('amplitudes', B, FR, 1, grad=False), U('harmonic_distribution', B, FR, 72, grad=False)]),
    Row('core.harmonic_oscillator_bank', lambda d, f, a: d.core.harmonic_oscillator_bank(f, a),
        [U('frequency', B, 320, 1, lo=180.0, hi=260.0, grad=False), U('amplitude_envelopes', B, 320, K, grad=False)]),
    Row('FilteredNoise.get_controls', lambda d, m: d.synths.FilteredNoise(n_samples=NS).get_controls(m), [N('magnitudes', B, FR, 64, grad=False)]),
    Row('FilteredNoise.get_signal', lambda d, m, z: d.synths.FilteredNoise(n_samples=NS, window_size=0).get_signal(m, noise=z),
        [U('magnitudes', B, FR, 65), U('noise', B, NS, lo=-1.0, hi=1.0, grad=False)]),
    Row('Sinusoidal.get_controls', lambda d, a, f: d.synths.Sinusoidal(n_samples=320).get_controls(a, f),
        [N('amplitudes', B, T, K, grad=False), N('frequencies', B, T, K, grad=False)]),
    Row('Sinusoidal.get_signal', lambda d, a, f: d.synths.Sinusoidal(n_samples=320).get_signal(a, f),
        [U('amplitudes', B, T, K), U('frequencies', B, T, K, lo=100.0, hi=4000.0)]),
    Row('Sinusoidal/chain_linear', lambda d, a, f: d.synths.Sinusoidal(n_samples=320, amp_resample_method='linear')(a, f),
        [N('amplitudes', B, T, K), N('frequencies', B, T, K)]),
    Row('SpectralLoss/value_only', _spectral(logmag_weight=1.0), [_audio('target_audio', grad=False), _audio(grad=False)], scalar=True),
    Row('SpectralLoss/general_deterministic', _spectral(delta_time_weight=1.0, loudness_weight=1.0, deterministic=True),
        [_audio('target_audio', grad=False), _audio()], scalar=True),
    Row('TWMLoss.predict_f0', lambda d, c, f, a: torch.as_tensor(d.losses.TWMLoss().predict_f0(c, f, a)),
        [U('f0_candidates', B, T, 4, lo=100.0, hi=400.0, grad=False), U('freqs', B, T, K, lo=100.0, hi=4000.0, grad=False), U('amps', B, T, K, grad=False)]),
    Row('losses.freq_loss', lambda d, f, t: d.losses.freq_loss(f, t), [U('f_hz', B, T, 1, lo=100.0, hi=400.0), U('f_hz_target', B, T, 1, lo=100.0, hi=400.0)],
        scalar=True),
    Row('core.angular_cumsum', lambda d, x: d.core.angular_cumsum(x), [U('angular_frequency', B, 320, K, lo=0.0, hi=3.0, grad=False)]),
    Row('core.apply_window_to_impulse_response', lambda d, x: d.core.apply_window_to_impulse_response(x, window_size=8),
        [N('impulse_response', B, T, 16, grad=False)]),
    Row('core.frequency_impulse_response', lambda d, m: d.core.frequency_impulse_response(m, window_size=16), [U('magnitudes', B, T, 9)]),
    Row('core.sinc_impulse_response', lambda d, c: d.core.sinc_impulse_response(c, window_size=16, sample_rate=16000),
        [U('cutoff_frequency', B, T, 1, lo=500.0, hi=4000.0)]),
    Row('core.sinc', lambda d, x: d.core.sinc(x), [N('x', B, T, K, grad=False)]),
    Row('core.get_harmonic_frequencies', lambda d, f: d.core.get_harmonic_frequencies(f, K), [U('frequencies', B, T, 1, lo=100.0, hi=400.0, grad=False)]),
    Row('core.remove_above_nyquist', lambda d, f, a: d.core.remove_above_nyquist(f, a),
        [U('frequency_envelopes', B, T, K, lo=100.0, hi=12000.0, grad=False), U('amplitude_envelopes', B, T, K, grad=False)]),
    Row('core.safe_divide', lambda d, a, b: d.core.safe_divide(a, b), [N('numerator', B, T, K, grad=False), N('denominator', B, T, K, grad=False)]),
    Row('core.wavetable_synthesis', lambda d, f, a, w: d.core.wavetable_synthesis(f, a, w, n_samples=320),
        [U('frequencies', B, T, 1, lo=100.0, hi=400.0), U('amplitudes', B, T, 1), N('wavetables', B, T, 64)]),
    Row('core.frequencies_sigmoid', lambda d, x: d.core.frequencies_sigmoid(x, depth=2), [N('freqs', B, T, 2 * K)]),
    Row('core.frequencies_softmax', lambda d, x: d.core.frequencies_softmax(x, depth=4), [N('freqs', B, T, 4 * K)]),
]

BY_NAME = {row.name: row for row in ROWS}
assert len(BY_NAME) == len(ROWS)

# C entries no row reaches, each with its reason.  tests/test_layouts_table.py fails on an entry that is neither reached nor here,
# and on an entry listed here that a row does reach.
EXEMPT = {
    'ddsp_version': 'takes no tensor',
    'ddsp_prepare': 'takes no tensor: it makes the constant tables of a shape ahead of time',
    'ddsp_profile_kernel_count': 'the profile entries take no tensor',
    'ddsp_profile_kernel_name': 'the profile entries take no tensor',
    'ddsp_profile_begin': 'the profile entries take no tensor',
    'ddsp_profile_begin_sampled': 'the profile entries take no tensor',
    'ddsp_profile_end': 'the profile entries take no tensor',
    'ddsp_sinc_impulse_response_size': 'takes no tensor, and the Python layer works the size out itself',
    'ddsp_fft_convolve_long_workspace_bytes': 'a size query of the C ABI the Python layer does not use (it asks the _ex one)',
    'ddsp_fft_convolve_long_f32': 'C ABI only: ddsp_fft_convolve_long_ex_f32 with n_out = N, which core.fft_convolve_long calls',
    'ddsp_uniform_noise_f32': 'C ABI only: ddsp_uniform_noise_ex_f32 at 11 bits; it writes an allocation of its own and reads no tensor',
    'ddsp_spectral_loss_backward_f32': 'C ABI only: SpectralLoss takes value and gradient from one pass (ddsp_spectral_loss_value_and_grad_f32)',
    'ddsp_spectral_loss_backward_det_f32': 'C ABI only: as ddsp_spectral_loss_backward_f32, for deterministic=True',
}

# rows that are framework ops from end to end (kept: the issue of the layouts is the Python layer's as much as the kernels')
FRAMEWORK_ONLY = {'core.harmonic_distribution_to_wavetable/irfft'}
