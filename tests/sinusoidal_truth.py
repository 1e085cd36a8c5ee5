"""fp64 numpy truth for synths.Sinusoidal and the frequency scale functions under it (TEST INFRASTRUCTURE), written from the
closed forms rather than from the reference's op chain:

  frequency envelope  f_j + (f_{j+1} - f_j) r / hop inside frame j, the last frame held (legacy bilinear resize);
  amplitude envelope  A_j (1 - w(r)) + A_{j+1} w(r), w = 0.5 - 0.5 cos(pi r / hop) ('window') or r / hop ('linear');
  phase               the INCLUSIVE cumulative sum of the frequency envelope, in cycles;
  mask                a sample whose interpolated frequency is >= sample_rate / 2 contributes nothing, and no gradient.

tests/test_sinusoidal_host.py checks it against oracle.resample + oracle.oscillator_bank in fp64 and its gradients
against central differences."""
import numpy as np

LN10 = float(np.log(10.0))


def sigmoid(x):
  x = np.asarray(x, np.float64)
  return 0.5 * (1.0 + np.tanh(0.5 * x))


def exp_sigmoid(x):
  return 2.0 * sigmoid(x) ** LN10 + 1e-7


def exp_sigmoid_grad(x):
  s = sigmoid(x)
  return 2.0 * LN10 * s ** LN10 * (1.0 - s)


def logb(x, base=2.0, eps=1e-5):
  x = np.asarray(x, np.float64)
  den = np.log(eps if base <= 0 else base)
  return np.log(np.where(x <= 0, eps, x)) / (eps if den == 0 else den)


def hz_to_midi(hz):
  hz = np.asarray(hz, np.float64)
  return np.where(hz <= 0, 0.0, 12.0 * (np.log2(np.where(hz <= 0, 1.0, hz)) - np.log2(440.0)) + 69.0)


def midi_to_hz(notes, midi_zero_silence=False):
  notes = np.asarray(notes, np.float64)
  hz = 440.0 * 2.0 ** ((notes - 69.0) / 12.0)
  return np.where(notes == 0, 0.0, hz) if midi_zero_silence else hz


def unit_to_midi(unit, midi_min=20.0, midi_max=90.0, clip=False):
  unit = np.asarray(unit, np.float64)
  return midi_min + (midi_max - midi_min) * (np.clip(unit, 0, 1) if clip else unit)


def midi_to_unit(midi, midi_min=20.0, midi_max=90.0, clip=False):
  unit = (np.asarray(midi, np.float64) - midi_min) / (midi_max - midi_min)
  return np.clip(unit, 0, 1) if clip else unit


def unit_to_hz(unit, hz_min, hz_max, clip=False):
  return midi_to_hz(unit_to_midi(unit, float(hz_to_midi(hz_min)), float(hz_to_midi(hz_max)), clip))


def hz_to_unit(hz, hz_min, hz_max, clip=False):
  return midi_to_unit(hz_to_midi(hz), float(hz_to_midi(hz_min)), float(hz_to_midi(hz_max)), clip)


def _depth_axis(freqs, depth):
  freqs = np.asarray(freqs, np.float64)
  if freqs.ndim == 3:
    b, t, c = freqs.shape
    return freqs.reshape(b, t, c // depth, depth)
  return freqs


def sigmoid_ranges(depth, hz_min=0.0, hz_max=8000.0):
  """[(lo, hi)] of the `depth` terms of frequencies_sigmoid (the host-side loop of the reference)."""
  lo_copy, remainder = hz_min, hz_max - hz_min
  scale_factor = remainder ** (1.0 / depth)
  out = []
  for i in range(depth):
    if i == depth - 1:
      hi, lo = remainder, lo_copy
    else:
      hi, lo = remainder * (1.0 - 1.0 / scale_factor), 0.0
      remainder -= hi
    out.append((lo, hi))
  return out


def frequencies_sigmoid(freqs, depth=1, hz_min=0.0, hz_max=8000.0, grad=False):
  x = _depth_axis(freqs, depth)
  s = sigmoid(x)
  hz = np.zeros(x.shape[:-1])
  dx = np.zeros(x.shape)
  for i, (lo, hi) in enumerate(sigmoid_ranges(x.shape[-1], hz_min, hz_max)):
    m_lo, m_hi = float(hz_to_midi(lo)), float(hz_to_midi(hi))
    term = midi_to_hz(m_lo + (m_hi - m_lo) * s[..., i])
    hz += term
    dx[..., i] = term * np.log(2.0) / 12.0 * (m_hi - m_lo) * s[..., i] * (1.0 - s[..., i])
  return (hz, dx) if grad else hz


def frequencies_softmax(freqs, depth=1, hz_min=20.0, hz_max=8000.0, grad=False):
  x = _depth_axis(freqs, depth)
  e = np.exp(x - x.max(-1, keepdims=True))
  p = e / e.sum(-1, keepdims=True)
  bins = np.linspace(0.0, 1.0, x.shape[-1])
  unit = (p * bins).sum(-1)
  m_lo, m_hi = float(hz_to_midi(hz_min)), float(hz_to_midi(hz_max))
  hz = midi_to_hz(m_lo + (m_hi - m_lo) * unit)
  if not grad:
    return hz
  dx = (hz * np.log(2.0) / 12.0 * (m_hi - m_lo))[..., None] * p * (bins - unit[..., None])
  return hz, dx


def harmonic_to_sinusoidal(harm_amp, harm_dist, f0_hz, sample_rate=16000):
  harm_amp, harm_dist, f0_hz = (np.asarray(t, np.float64) for t in (harm_amp, harm_dist, f0_hz))
  k = harm_dist.shape[-1]
  freqs = f0_hz * np.arange(1, k + 1)
  dist = np.where(freqs >= sample_rate / 2.0, 0.0, harm_dist)
  total = dist.sum(-1, keepdims=True)
  return harm_amp * dist / np.where(total == 0, 1e-7, total), freqs


def get_controls(amplitudes, frequencies, sample_rate=16000, amp_scale=True, freq_fn=frequencies_sigmoid):
  """Sinusoidal.get_controls; freq_fn is one of this module's scale functions (or a lambda of one), or None."""
  a = exp_sigmoid(amplitudes) if amp_scale else np.asarray(amplitudes, np.float64)
  f = np.asarray(frequencies, np.float64)
  if freq_fn is not None:
    f = freq_fn(f)
    a = np.where(f >= sample_rate / 2.0, 0.0, a)
  return a, f


def envelopes(amplitudes, frequencies, n_samples, method='window'):
  """-> (amplitude envelope, frequency envelope, the two frame weights), [B, N, K] / [hop]."""
  a, f = np.asarray(amplitudes, np.float64), np.asarray(frequencies, np.float64)
  b, n_frames, k = a.shape
  assert f.shape == a.shape and n_samples % n_frames == 0 and method in ('window', 'linear')
  hop = n_samples // n_frames
  lerp = np.arange(hop) / hop
  w = lerp if method == 'linear' else 0.5 - 0.5 * np.cos(np.pi * lerp)
  a_next = np.concatenate([a[:, 1:], a[:, -1:]], 1)
  f_next = np.concatenate([f[:, 1:], f[:, -1:]], 1)
  a_env = a[:, :, None, :] * (1.0 - w)[None, None, :, None] + a_next[:, :, None, :] * w[None, None, :, None]
  f_env = f[:, :, None, :] + (f_next - f)[:, :, None, :] * lerp[None, None, :, None]
  return a_env.reshape(b, n_samples, k), f_env.reshape(b, n_samples, k), w, lerp


def get_signal(amplitudes, frequencies, n_samples, sample_rate=16000, method='window', parts=False):
  a_env, f_env, w, lerp = envelopes(amplitudes, frequencies, n_samples, method)
  mask = f_env < sample_rate / 2.0
  phase = np.cumsum(f_env, axis=1) / sample_rate                   # cycles, inclusive
  phase -= np.floor(phase)
  audio = (np.where(mask, a_env, 0.0) * np.sin(2.0 * np.pi * phase)).sum(-1)
  return (audio, a_env, mask, phase, w, lerp) if parts else audio


def amplitude_sum(amplitudes, frequencies, n_samples, sample_rate=16000, method='window'):
  """max over the samples of the summed (masked) amplitude envelopes: the scale of the forward tolerance."""
  a_env, f_env, _, _ = envelopes(amplitudes, frequencies, n_samples, method)
  return float(np.abs(np.where(f_env < sample_rate / 2.0, a_env, 0.0)).sum(-1).max())


def get_signal_backward(amplitudes, frequencies, grad_audio, n_samples, sample_rate=16000, method='window'):
  """Analytic (dL/d amplitudes, dL/d frequencies) of get_signal, both [B, F, K]."""
  _, a_env, mask, phase, w, lerp = get_signal(amplitudes, frequencies, n_samples, sample_rate, method, parts=True)
  b, n, k = a_env.shape
  n_frames = np.asarray(amplitudes).shape[1]
  hop = n // n_frames
  g = np.asarray(grad_audio, np.float64)[:, :, None] * mask
  d_a_env = (g * np.sin(2.0 * np.pi * phase)).reshape(b, n_frames, hop, k)
  c = g * a_env * np.cos(2.0 * np.pi * phase) * (2.0 * np.pi / sample_rate)
  d_f_env = np.cumsum(c[:, ::-1], axis=1)[:, ::-1].reshape(b, n_frames, hop, k)       # inclusive suffix sum

  def adjoint(d_env, weight):
    lo = (d_env * (1.0 - weight)[None, None, :, None]).sum(2)
    hi = (d_env * weight[None, None, :, None]).sum(2)
    out = lo.copy()
    out[:, 1:] += hi[:, :-1]
    out[:, -1] += hi[:, -1]                                                            # the held last frame
    return out

  return adjoint(d_a_env, w), adjoint(d_f_env, lerp)


def sinusoidal(amplitudes, frequencies, n_samples, sample_rate=16000, method='window', amp_scale=True,
               freq_fn=frequencies_sigmoid):
  a, f = get_controls(amplitudes, frequencies, sample_rate, amp_scale, freq_fn)
  return get_signal(a, f, n_samples, sample_rate, method)


def sinusoidal_backward(amplitudes, frequencies, grad_audio, n_samples, sample_rate=16000, method='window', amp_scale=True,
                        freq_fn=None, freq_fn_grad=None, controls=None):
  """Gradients with respect to the RAW inputs.  freq_fn_grad(x) -> (hz, d hz / d x [.., K, depth]).  controls: the fp32
  (amplitudes, frequencies) the synthesis actually ran on - the synthesis' gradient is then taken there (one fp32 ulp of a
  frequency moves the phase of a long clip by more than the gradient tolerance), the scale functions' derivatives at the
  raw inputs."""
  amplitudes, frequencies = np.asarray(amplitudes, np.float64), np.asarray(frequencies, np.float64)
  a = exp_sigmoid(amplitudes) if amp_scale else amplitudes
  if freq_fn_grad is not None:
    f, dx = freq_fn_grad(frequencies)
    a = np.where(f >= sample_rate / 2.0, 0.0, a)
  else:
    f, dx = frequencies, None
  if controls is not None:
    a, f = (np.asarray(t, np.float64) for t in controls)
  ga, gf = get_signal_backward(a, f, grad_audio, n_samples, sample_rate, method)
  if freq_fn_grad is not None:
    ga = np.where(f >= sample_rate / 2.0, 0.0, ga)
    gf = (gf[..., None] * dx).reshape(frequencies.shape)
  if amp_scale:
    ga = ga * exp_sigmoid_grad(amplitudes)
  return ga, gf


def control_inputs(seed, b, n_frames, k, sample_rate=16000, f_lo=20.0, f_hi=None, a_hi=1.0):
  """Random controls: amplitudes in [0, a_hi], frequencies log-uniform in [f_lo, f_hi], at least 1 Hz away from Nyquist."""
  rng = np.random.default_rng(seed)
  f_hi = sample_rate / 2.0 - 2.0 if f_hi is None else f_hi
  amps = rng.uniform(0.0, a_hi, (b, n_frames, k)).astype(np.float32)
  freqs = np.exp(rng.uniform(np.log(f_lo), np.log(f_hi), (b, n_frames, k))).astype(np.float32)
  return amps, freqs
