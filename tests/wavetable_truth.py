"""fp64 truth for core.linear_lookup, core.wavetable_synthesis, core.variable_length_delay, synths.Wavetable and
effects.ModDelay (ddsp/core.py:1167-1313, ddsp/synths.py:199-258, ddsp/effects.py:327-392), with analytic gradients.
TEST INFRASTRUCTURE ONLY: numpy, nothing of it is ever imported by ddsp_amd.

The lookups are evaluated as the two-point lerp the reference's relu weights amount to (`dense_lookup` is the
reference's own sum over all W + 1 points, for small shapes: tests/test_wavetable_host.py holds the two together).
Envelopes come from oracle.ddsp_oracle.resample in fp64, the linear one at exact positions t F / N."""
import numpy as np

from oracle import ddsp_oracle as O

F64 = np.float64


def exp_sigmoid(x):
  x = np.asarray(x, F64)
  return 2.0 * (1.0 / (1.0 + np.exp(-x))) ** np.log(10.0) + 1e-7


def exp_sigmoid_grad(x):
  x = np.asarray(x, F64)
  s = 1.0 / (1.0 + np.exp(-x))
  return 2.0 * np.log(10.0) * s ** np.log(10.0) * (1.0 - s)


def sigmoid(x):
  return 1.0 / (1.0 + np.exp(-np.asarray(x, F64)))


def dense_lookup(phase, tables):
  """The reference's formulation: phase [B,N], tables [B,W] or [B,N,W] -> [B,N]; O(B N W) memory."""
  phase, tables = np.asarray(phase, F64), np.asarray(tables, F64)
  if tables.ndim == 2:
    tables = tables[:, None, :]
  tables = np.concatenate([tables, tables[..., 0:1]], axis=-1)
  n_points = tables.shape[-1]
  grid = np.linspace(0.0, 1.0, n_points)
  dist = np.abs(phase[:, :, None] - grid[None, None, :]) * (n_points - 1)
  return (np.maximum(1.0 - dist, 0.0) * tables).sum(-1)


def _split(x):
  i0 = np.floor(x)
  return i0.astype(np.int64), x - i0


def _points(tables, t_index, pnt, W):
  """tables [B,Fw,W] read at (b, t_index[b?,n], point pnt[b,n]); points outside [0, W] do not exist (value 0)."""
  valid = (pnt >= 0) & (pnt <= W)
  idx = np.where(valid, pnt % W, 0)
  b = np.arange(tables.shape[0])[:, None]
  return np.where(valid, tables[b, t_index, idx], 0.0), valid, idx


def linear_lookup(phase, tables, grad_out=None):
  """phase [B,N] (taken at the values given: pass the fp32 array to evaluate at the fp32 phases), tables [B,W] / [B,1,W] /
  [B,N,W].  Returns out, or (out, grad_phase, grad_tables) with grad_out."""
  phase, tables = np.asarray(phase, F64), np.asarray(tables, F64)
  squeeze = tables.ndim == 2
  if squeeze:
    tables = tables[:, None, :]
  B, N = phase.shape
  W = tables.shape[-1]
  t_index = np.zeros((1, N), np.int64) if tables.shape[1] == 1 else np.arange(N)[None, :]
  i0, fr = _split(phase * W)
  v0, ok0, idx0 = _points(tables, t_index, i0, W)
  v1, ok1, idx1 = _points(tables, t_index, i0 + 1, W)
  out = v0 * (1.0 - fr) + v1 * fr
  if grad_out is None:
    return out
  g = np.asarray(grad_out, F64)
  g_phase = g * W * (v1 - v0)
  g_tables = np.zeros_like(tables)
  b = np.broadcast_to(np.arange(B)[:, None], (B, N))
  tt = np.broadcast_to(t_index, (B, N))
  np.add.at(g_tables, (b, tt, idx0), np.where(ok0, g * (1.0 - fr), 0.0))
  np.add.at(g_tables, (b, tt, idx1), np.where(ok1, g * fr, 0.0))
  return out, g_phase, (g_tables[:, 0] if squeeze else g_tables)


def _window_weights(F, N):
  """a(t) = a[j] (1 - w) + a[min(j + 1, F - 1)] w: upsample_with_windows in closed form (checked against the oracle)."""
  hop = N // F
  t = np.arange(N)
  j, r = t // hop, t % hop
  return j, np.minimum(j + 1, F - 1), 0.5 - 0.5 * np.cos(np.pi * r / hop)


def _linear_weights(F, N):
  """Legacy bilinear at the exact position t F / N, the last frame held."""
  t = np.arange(N, dtype=np.int64)
  j = (t * F) // N
  return j, np.minimum(j + 1, F - 1), ((t * F) % N) / float(N)


def wavetable_synthesis(frequencies, amplitudes, wavetables, n_samples, sample_rate=16000, grad_out=None, scale=False):
  """frequencies, amplitudes [B,F,1]; wavetables [B,W] or [B,Fw,W].  scale=True applies exp_sigmoid to amplitudes and
  wavetables first (synths.Wavetable with its default scale_fn) and returns gradients with respect to the raw inputs.
  Returns audio [B,N], or (audio, grad_amplitudes, grad_wavetables, grad_frequencies)."""
  f_in = np.asarray(frequencies, F64)
  a_raw, w_raw = np.asarray(amplitudes, F64), np.asarray(wavetables, F64)
  a_in, w_in = (exp_sigmoid(a_raw), exp_sigmoid(w_raw)) if scale else (a_raw, w_raw)
  squeeze = w_in.ndim == 2
  tables = w_in[:, None, :] if squeeze else w_in
  B, F, _ = a_in.shape
  N, Fw, W = int(n_samples), tables.shape[1], tables.shape[2]
  a = O.resample(a_in, N, 'window', dtype=F64)[:, :, 0]
  with O.exact_resize_positions():
    f = O.resample(f_in, N, dtype=F64)[:, :, 0]
  vel = f / float(sample_rate)
  phase = (np.cumsum(vel, axis=1) - vel) % 1.0                 # exclusive: phase(0) = 0
  i0, fr = _split(phase * W)
  i0 = np.minimum(i0, W - 1)
  fr = phase * W - i0
  i1 = (i0 + 1) % W
  jw, hw, wf = _linear_weights(Fw, N)
  b = np.arange(B)[:, None]
  c0, c1, n0, n1 = tables[b, jw[None], i0], tables[b, jw[None], i1], tables[b, hw[None], i0], tables[b, hw[None], i1]
  vc, vn = c0 * (1 - fr) + c1 * fr, n0 * (1 - fr) + n1 * fr
  v = vc * (1 - wf) + vn * wf
  out = a * v
  if grad_out is None:
    return out
  g = np.asarray(grad_out, F64)
  bb = np.broadcast_to(b, (B, N))
  # tables
  g_tab = np.zeros_like(tables)
  ga = g * a
  for frame, wgt in ((jw, 1 - wf), (hw, wf)):
    ff = np.broadcast_to(frame[None], (B, N))
    np.add.at(g_tab, (bb, ff, i0), ga * wgt * (1 - fr))
    np.add.at(g_tab, (bb, ff, i1), ga * wgt * fr)
  # amplitudes: adjoint of the window upsampling
  ja, ha, ww = _window_weights(F, N)
  g_amp = np.zeros((B, F))
  np.add.at(g_amp, (bb, np.broadcast_to(ja[None], (B, N))), g * v * (1 - ww))
  np.add.at(g_amp, (bb, np.broadcast_to(ha[None], (B, N))), g * v * ww)
  # f0: d out / d phase, reverse exclusive scan, adjoint of the linear upsampling
  slope = (c1 - c0) * (1 - wf) + (n1 - n0) * wf
  dphi = ga * W * slope / float(sample_rate)
  rev = np.cumsum(dphi[:, ::-1], axis=1)[:, ::-1]
  s_after = rev - dphi
  jf, hf, wl = _linear_weights(F, N)
  g_f0 = np.zeros((B, F))
  np.add.at(g_f0, (bb, np.broadcast_to(jf[None], (B, N))), s_after * (1 - wl))
  np.add.at(g_f0, (bb, np.broadcast_to(hf[None], (B, N))), s_after * wl)
  if scale:
    g_tab = g_tab * exp_sigmoid_grad(w_raw[:, None, :] if squeeze else w_raw)
    g_amp = g_amp * exp_sigmoid_grad(a_raw[:, :, 0])
  return out, g_amp[:, :, None], (g_tab[:, 0] if squeeze else g_tab), g_f0[:, :, None]


def variable_length_delay(phase, audio, max_length, gain=None, phase_scale=1.0, phase_offset=0.0, add_dry=False,
                          grad_out=None):
  """phase, audio [B,N], gain [B,N] or None: gain * lookup(phase * phase_scale + phase_offset) (+ audio).
  Point i < L reads audio[n - i] (0 before the clip), point L reads audio[n] (the reference's appended wrap point).
  Returns out, or (out, grad_phase, grad_audio, grad_gain)."""
  phase, audio = np.asarray(phase, F64), np.asarray(audio, F64)
  B, N = audio.shape
  L = int(max_length)
  gn = np.ones((B, N)) if gain is None else np.asarray(gain, F64)
  i0, fr = _split((phase * phase_scale + phase_offset) * L)
  n = np.arange(N)[None, :]
  b = np.broadcast_to(np.arange(B)[:, None], (B, N))

  def tap(pnt):
    valid = (pnt >= 0) & (pnt <= L)
    src = np.where(pnt == L, n, n - pnt)
    valid = valid & (src >= 0)
    src = np.where(valid, src, 0)
    return np.where(valid, audio[b, src], 0.0), valid, src

  t0, ok0, s0 = tap(i0)
  t1, ok1, s1 = tap(i0 + 1)
  wet = t0 * (1 - fr) + t1 * fr
  out = wet * gn + (audio if add_dry else 0.0)
  if grad_out is None:
    return out
  g = np.asarray(grad_out, F64)
  g_phase = g * gn * L * (t1 - t0) * phase_scale
  g_gain = g * wet
  g_audio = g.copy() if add_dry else np.zeros((B, N))
  np.add.at(g_audio, (b, s0), np.where(ok0, g * gn * (1 - fr), 0.0))
  np.add.at(g_audio, (b, s1), np.where(ok1, g * gn * fr, 0.0))
  return out, g_phase, g_audio, g_gain


def mod_delay(audio, gain, phase, center_ms=15.0, depth_ms=10.0, sample_rate=16000, add_dry=True, scale=True, grad_out=None):
  """effects.ModDelay.__call__ with its default scale functions (scale=True) or none: gain, phase [B,N].
  Returns out, or (out, grad_audio, grad_gain, grad_phase) with respect to the raw inputs."""
  gain_raw, phase_raw = np.asarray(gain, F64), np.asarray(phase, F64)
  gn, ph = (exp_sigmoid(gain_raw), sigmoid(phase_raw)) if scale else (gain_raw, phase_raw)
  max_ms = center_ms + depth_ms
  L = int(sample_rate / 1000.0 * max_ms)
  res = variable_length_delay(ph, audio, L, gn, depth_ms / max_ms, center_ms / max_ms, add_dry, grad_out)
  if grad_out is None:
    return res
  out, g_phase, g_audio, g_gain = res
  if scale:
    g_gain = g_gain * exp_sigmoid_grad(gain_raw)
    g_phase = g_phase * ph * (1.0 - ph)
  return out, g_audio, g_gain, g_phase


# ---- inputs shared by the CPU, emulated and GPU tests ---------------------------------------------------------
def smooth_tables(rng, B, Fw, W, n_harmonics=8):
  """Band-limited tables: n_harmonics sinusoids with random amplitudes and phases per frame."""
  k = np.arange(1, n_harmonics + 1)
  amp = rng.uniform(0.2, 1.0, (B, Fw, n_harmonics)) / k
  ph = rng.uniform(0, 2 * np.pi, (B, Fw, n_harmonics))
  x = np.arange(W) / W
  return (amp[..., None] * np.sin(2 * np.pi * k[:, None] * x[None, :] + ph[..., None])).sum(-2).astype(np.float32)


def synthesis_inputs(seed, B, F, W, Fw=None, rough=False, f_lo=30.0, f_hi=7900.0):
  rng = np.random.default_rng(seed)
  Fw = F if Fw is None else Fw
  tables = rng.uniform(-1, 1, (B, Fw, W)).astype(np.float32) if rough else smooth_tables(rng, B, Fw, W)
  amps = rng.uniform(0.1, 1.0, (B, F, 1)).astype(np.float32)
  f0 = np.exp(rng.uniform(np.log(f_lo), np.log(f_hi), (B, F, 1))).astype(np.float32)
  return amps, tables, f0
