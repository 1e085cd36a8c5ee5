"""fp64 restatement of the part of ddsp/core.py that ddsp_amd mirrors in csrc/scale_fns.hip, critical_bands.hip and
harmonic_wavetable.hip - the psychoacoustic scales, soft_limit, log_scale, sym_exp_sigmoid, nan_to_num,
frequencies_critical_bands and harmonic_distribution_to_wavetable - with the analytic gradients of each, and the
tolerances the tests hold the kernels to.  numpy only; every function takes the fp32 inputs the kernels get and works in
float64 from there.  TEST INFRASTRUCTURE: nothing in ddsp_amd imports this."""
import numpy as np


def _f64(x):
  return np.asarray(x, dtype=np.float64)


# ---- elementwise (ddsp/core.py:202-238, 351-411) --------------------------------------------------------------------
def softplus(x):
  x = _f64(x)
  return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
  x = _f64(x)
  e = np.exp(-np.abs(x))
  return np.where(x >= 0.0, 1.0 / (1.0 + e), e / (1.0 + e))


def hz_to_bark(hz):
  with np.errstate(divide='ignore'):
    return 26.81 / (1.0 + (1960.0 / _f64(hz))) - 0.53


def d_hz_to_bark(hz):
  return 26.81 * 1960.0 / (_f64(hz) + 1960.0) ** 2


def bark_to_hz(bark):
  with np.errstate(divide='ignore'):
    return 1960.0 / (26.81 / (_f64(bark) + 0.53) - 1.0)


def d_bark_to_hz(bark):
  return 26.81 * 1960.0 / (26.81 - (_f64(bark) + 0.53)) ** 2


def hz_to_mel(hz):
  u = 1.0 + _f64(hz) / 700.0
  return 2595.0 * (np.log(np.where(u <= 0.0, 1e-5, u)) / np.log(10.0))          # logb: safe_log(x) / safe_log(10)


def d_hz_to_mel(hz):
  hz = _f64(hz)
  u = 1.0 + hz / 700.0
  return np.where(u <= 0.0, 0.0, (2595.0 / np.log(10.0)) / np.where(u <= 0.0, 1.0, 700.0 + hz))


def mel_to_hz(mel):
  return 700.0 * (10.0 ** (_f64(mel) / 2595.0) - 1.0)


def d_mel_to_hz(mel):
  return 700.0 * np.log(10.0) / 2595.0 * 10.0 ** (_f64(mel) / 2595.0)


def hz_to_erb(hz):
  return 0.108 * _f64(hz) + 24.7


def d_hz_to_erb(hz):
  return np.full(np.shape(hz), 0.108)


def soft_limit(x, x_min=0.0, x_max=1.0):
  x = _f64(x)
  return softplus(x) + x_min - softplus(x - (x_max - x_min))


def d_soft_limit(x, x_min=0.0, x_max=1.0):
  x = _f64(x)
  return sigmoid(x) - sigmoid(x - (x_max - x_min))


def log_scale(x, min_x, max_x):
  u = (_f64(x) + 1.0) / 2.0
  return np.exp((1.0 - u) * np.log(min_x) + u * np.log(max_x))


def d_log_scale(x, min_x, max_x):
  return log_scale(x, min_x, max_x) * 0.5 * (np.log(max_x) - np.log(min_x))


def exp_sigmoid(x, exponent=10.0, max_value=2.0, threshold=1e-7):
  return max_value * np.exp(-np.log(exponent) * softplus(-_f64(x))) + threshold


def sym_exp_sigmoid(x, width=8.0):
  return exp_sigmoid(width * (np.abs(_f64(x)) / 2.0 - 1.0))


def d_sym_exp_sigmoid(x, width=8.0):
  x = _f64(x)
  z = width * (np.abs(x) / 2.0 - 1.0)
  return 2.0 * np.exp(-np.log(10.0) * softplus(-z)) * np.log(10.0) * sigmoid(-z) * (width / 2.0) * np.sign(x)


def nan_to_num(x, value=0.0):
  x = _f64(x)
  return np.where(np.isnan(x), value, x)


def d_nan_to_num(x, value=0.0):
  return np.where(np.isnan(_f64(x)), 0.0, 1.0)


def elementwise_tolerance(truth):
  """|ours - truth| <= 2e-6 |truth| + 2e-6 max |truth| over the grid: the figure the existing conversions are held to."""
  truth = _f64(truth)
  finite = np.abs(truth[np.isfinite(truth)])
  return 2e-6 * np.abs(truth) + 2e-6 * (float(finite.max()) if finite.size else 1.0)


# ---- frequencies_critical_bands (ddsp/core.py:510-569) --------------------------------------------------------------
def critical_band_tables(n_sinusoids, depth=1, depth_scale=10.0, hz_min=20.0, hz_max=8000.0, scale='bark'):
  """(f_center [K], bandwidths [K], depth_modifier [depth]) in float64."""
  if scale == 'bark':
    f_center = bark_to_hz(np.linspace(hz_to_bark(hz_min), hz_to_bark(hz_max), n_sinusoids))
  else:
    f_center = mel_to_hz(np.linspace(hz_to_mel(hz_min), hz_to_mel(hz_max), n_sinusoids))
  with np.errstate(under='ignore'):
    depth_modifier = np.float64(depth_scale) ** -np.arange(depth, dtype=np.float64)
  return f_center, hz_to_erb(f_center), depth_modifier


def _depth_axis(x, n_sinusoids, depth):
  x = _f64(x)
  return x.reshape(x.shape[:2] + (n_sinusoids, depth))


def critical_bands(x, n_sinusoids, depth=1, depth_scale=10.0, bandwidth_scale=1.0, hz_min=20.0, hz_max=8000.0, scale='bark'):
  """x [B, T, K * depth] (or [B, T, K, depth]) -> [B, T, K]."""
  f_center, bw, dm = critical_band_tables(n_sinusoids, depth, depth_scale, hz_min, hz_max, scale)
  modifier = np.sum(np.tanh(_depth_axis(x, n_sinusoids, depth)) * dm, axis=-1)
  return soft_limit(f_center + bandwidth_scale * bw * modifier, hz_min, hz_max)


def critical_bands_grad(x, g_out, n_sinusoids, depth=1, depth_scale=10.0, bandwidth_scale=1.0, hz_min=20.0, hz_max=8000.0,
                        scale='bark'):
  """d sum(g_out * out) / d x, in x's own shape."""
  f_center, bw, dm = critical_band_tables(n_sinusoids, depth, depth_scale, hz_min, hz_max, scale)
  t = np.tanh(_depth_axis(x, n_sinusoids, depth))
  f = f_center + bandwidth_scale * bw * np.sum(t * dm, axis=-1)
  coef = _f64(g_out) * d_soft_limit(f, hz_min, hz_max) * bandwidth_scale * bw
  return (coef[..., None] * dm * (1.0 - t * t)).reshape(np.shape(x))


def critical_bands_magnitude(n_sinusoids, depth=1, depth_scale=10.0, bandwidth_scale=1.0, hz_min=20.0, hz_max=8000.0, scale='bark'):
  """M: the largest intermediate the fp32 chain can hold; the result is a difference of two numbers of that size."""
  f_center, bw, dm = critical_band_tables(n_sinusoids, depth, depth_scale, hz_min, hz_max, scale)
  return max(float(hz_max), float(np.max(f_center + abs(bandwidth_scale) * bw * np.sum(dm))))


def critical_bands_tolerance(*args, **kwargs):
  """5e-7 M per element: eight fp32 ulps of M (a 2-ulp tanh, the table casts, two softplus and the sums)."""
  return 5e-7 * critical_bands_magnitude(*args, **kwargs)


def critical_bands_grad_tolerance(x, g_out, n_sinusoids, depth=1, depth_scale=10.0, bandwidth_scale=1.0, hz_min=20.0, hz_max=8000.0,
                                  scale='bark'):
  """(2e-6 + 1.25e-7 M) R with R = max |g_out bandwidth_scale bw[k] depth_modifier[d] (1 - tanh^2 x)|: the sigmoid factors
  have slope <= 1/4 and see f with up to the forward's error of 5e-7 M."""
  _, bw, dm = critical_band_tables(n_sinusoids, depth, depth_scale, hz_min, hz_max, scale)
  t = np.tanh(_depth_axis(x, n_sinusoids, depth))
  r = float(np.max(np.abs((_f64(g_out) * bandwidth_scale * bw)[..., None] * dm * (1.0 - t * t))))
  m = critical_bands_magnitude(n_sinusoids, depth, depth_scale, bandwidth_scale, hz_min, hz_max, scale)
  return (2e-6 + 1.25e-7 * m) * r


# ---- harmonic_distribution_to_wavetable (ddsp/core.py:1217-1235) ----------------------------------------------------
def wavetable_length(n_harmonics, n_wavetable):
  return 2 * (n_harmonics + int(n_wavetable / 2 - n_harmonics))


def wavetable(hd, n_wavetable=2048):
  """The reference's own chain: pad (one zero for DC in front, n_pad behind), irfft, times n_wavetable / 2."""
  hd = _f64(hd)
  k = hd.shape[-1]
  n_pad = int(n_wavetable / 2 - k)
  assert n_pad >= 0
  fft_in = np.pad(hd, [(0, 0)] * (hd.ndim - 1) + [(1, n_pad)])
  return np.fft.irfft(fft_in.astype(np.complex128), axis=-1) * (n_wavetable / 2)


def wavetable_closed_form(hd, n_wavetable=2048):
  """(n_wavetable / L) sum_k w_k hd[k - 1] cos(2 pi k n / L), w_k = 1 but w_{L/2} = 1/2."""
  hd = _f64(hd)
  k = hd.shape[-1]
  length = wavetable_length(k, n_wavetable)
  w = np.ones(k)
  if k == length // 2:
    w[-1] = 0.5
  basis = np.cos(2.0 * np.pi * np.outer(np.arange(1, k + 1), np.arange(length)) / length)
  return (n_wavetable / length) * ((hd * w) @ basis)


def wavetable_grad(g, n_harmonics, n_wavetable=2048):
  """d sum(g * table) / d hd: scale * w_k * Re rfft(g)[k], k = 1 .. K."""
  g = _f64(g)
  length = g.shape[-1]
  assert length == wavetable_length(n_harmonics, n_wavetable)
  w = np.ones(n_harmonics)
  if n_harmonics == length // 2:
    w[-1] = 0.5
  return (n_wavetable / length) * w * np.fft.rfft(g, axis=-1).real[..., 1:n_harmonics + 1]


def wavetable_tolerance(truth, n_harmonics, n_wavetable):
  """3e-6 (n_wavetable / L) max(1, max |truth|): the figure compute_mag is held to for the same transform code."""
  return 3e-6 * (n_wavetable / wavetable_length(n_harmonics, n_wavetable)) * max(1.0, float(np.max(np.abs(truth))))


def wavetable_grad_tolerance(g, n_harmonics, n_wavetable):
  """3e-6 (n_wavetable / L) max(1, max_k |rfft(g)_k|)."""
  spectrum = np.abs(np.fft.rfft(_f64(g), axis=-1))
  return 3e-6 * (n_wavetable / wavetable_length(n_harmonics, n_wavetable)) * max(1.0, float(spectrum.max()))
