"""Host-side mirror of the `ddsp.core` functions on the Harmonic / FilteredNoise path.

Same names, argument meaning and ValueErrors as the reference (`ddsp/core.py`), but the
arithmetic runs in the hand-written gfx950 kernels behind the C ABI of
`include/ddsp_amd.h`.  Tensors are `torch.Tensor`s in HBM; torch is plumbing only
(allocation, streams) - there is no torch / CPU compute fallback.
"""
import math

import numpy as np
import torch

from ddsp_amd import _lib


# --------------------------------------------------------------------------------------
# plumbing
# --------------------------------------------------------------------------------------
def _device():
  if not torch.cuda.is_available():
    raise _lib.DdspLibraryError(
        'ddsp_amd needs an AMD GPU (torch.cuda.is_available() is False); '
        'there is no CPU fallback.')
  return torch.device('cuda', torch.cuda.current_device())


def tf_float32(x):
  """core.tf_float32 (ddsp/core.py:31-36): anything -> contiguous fp32 tensor in HBM."""
  if type(x) is torch.Tensor and x.is_cuda and x.dtype is torch.float32 and x.is_contiguous():
    _check_current_device(x)
    return x                                  # the common case: nothing to do (host overhead matters)
  if isinstance(x, torch.Tensor):
    if not x.is_cuda:
      x = x.to(_device())
    else:
      _check_current_device(x)
    return x.to(torch.float32).contiguous()
  return torch.as_tensor(np.asarray(x, dtype=np.float32), device=_device()).contiguous()


def aligned16(x):
  """`x` (contiguous fp32) itself when it starts on a 16-byte boundary, else a copy in an allocation of its own, which does.
  A contiguous view (`flat[a:b].view(...)`, `batch[r:r + 1]`, a chunk of a gradient bucket) starts on any 4-byte boundary.
  For the pointers by whose alignment a C entry picks its kernel (the supplied noise of ddsp_filtered_noise_f32, the audio and the
  impulse response of ddsp_fft_convolve_same_f32 / ddsp_fft_convolve_f32) and for ddsp_add_f32, which takes no other: the result
  then never depends on the address.  The copy runs only for such views; an allocation of torch's is aligned to 256 bytes or more."""
  return x if x.data_ptr() % 16 == 0 else x.clone(memory_format=torch.contiguous_format)


def _check_current_device(x):
  """Every kernel is enqueued on the CURRENT device's current stream (one process per GPU is the model): a tensor
  that lives on another GPU of the process would be handed to a stream of the wrong device.  Fail loudly."""
  if x.device.index != torch._C._cuda_getDevice():
    raise ValueError('tensor on {} but the current device is cuda:{}: ddsp_amd launches on the current device - wrap the '
                     'call in `with torch.cuda.device({})`'.format(x.device, torch._C._cuda_getDevice(), x.device.index))


def _stream():
  """Raw hipStream_t of torch's current stream (the C call: torch.cuda.current_stream() alone
  costs ~4 us of Python per launch, more than the launch itself)."""
  return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice())


def _stream_of(device):
  """Raw handle of torch's current stream ON `device` (which need not be the current device)."""
  index = device.index if device.index is not None else torch._C._cuda_getDevice()
  return torch._C._cuda_getCurrentRawStream(index)


# Whether torch's current stream is being captured into a graph: the one predicate Workspace asks, for CUDA devices only (it
# asks the GPU runtime, which a machine without a GPU does not have).  The C call itself, for the reason _stream gives.
_capturing = torch._C._cuda_isCurrentStreamCapturing


def require_no_grad(op, *tensors):
  """The raw kernel wrappers return tensors without a grad_fn.  Where no torch.autograd node covers an op, an input
  that requires grad must fail loudly instead of silently cutting the graph (a branch summed through Add would just
  stop training): the differentiable entries are the Processors' __call__ (Harmonic, FilteredNoise,
  Reverb, ...) and FilteredNoise.get_signal."""
  if torch.is_grad_enabled():
    for t in tensors:
      if isinstance(t, torch.Tensor) and t.requires_grad:
        raise NotImplementedError(
            '{}: an input requires grad, but this entry point has no backward pass on the MI355X path; call it '
            'under torch.no_grad() / on detached tensors, or go through the Processor __call__'.format(op))


_ws_bytes_cache = {}


def cached_workspace_bytes(fn_name, *shape):
  """Workspace size queries are pure functions of the shape: one ctypes call per new shape."""
  key = (fn_name,) + shape
  n = _ws_bytes_cache.get(key)
  if n is None:
    n = getattr(_lib.load(), fn_name)(*shape)
    _ws_bytes_cache[key] = n
  return n


class Workspace:
  """Grow-only scratch buffers in HBM, one per (device, stream): kernels enqueued on different streams never share
  scratch, and a buffer is only ever replaced by work enqueued behind its last user on the same stream (the caching
  allocator hands a freed block back to the stream it was allocated on).  A Processor instance may therefore be
  called from several streams; each stream pays for its own scratch.  The stream is the current one of the tensor's
  device, which is the current device (tf_float32 refuses tensors of another GPU: kernels launch on the current one); at most `kMaxStreams` buffers are kept, least recently used first out (short-lived streams do not pile up
  scratch, and a recycled stream handle finds a buffer that was last used on that very handle).

  A captured graph holds the scratch pointer as a kernel argument, and it usually is the pointer of a buffer made during
  the warm-up on the capture stream, outside the graph's own pool.  A buffer handed out while the current stream is
  capturing is therefore kept for as long as this Workspace lives: neither growth nor the eviction above frees it, so
  every replay finds its scratch.  Buffers handed out only outside a capture are replaced and evicted as before."""
  kMaxStreams = 8

  def __init__(self):
    self._bufs = {}            # insertion order = recency (a hit is re-inserted)
    self._captured = {}        # id -> buffer a capture was handed: never freed while self lives

  def get(self, nbytes, device):
    nbytes = max(int(nbytes), 16)
    stream = _stream_of(device) if device.type == 'cuda' else None
    key = (device, stream)
    buf = self._bufs.pop(key, None)
    if buf is None or buf.numel() < nbytes:
      buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    self._bufs[key] = buf
    while len(self._bufs) > self.kMaxStreams:
      self._bufs.pop(next(iter(self._bufs)))
    if stream and _capturing():            # (handle 0, the null stream, cannot be captured: the eager default pays no query)
      self._captured[id(buf)] = buf
    return buf


_default_ws = Workspace()


# --------------------------------------------------------------------------------------
# dict helpers used by the DAG plumbing  (ddsp/core.py:39-129)
# --------------------------------------------------------------------------------------
def make_iterable(x):
  """Wrap in a list if not iterable, return empty list if None (ddsp/core.py:39-47)."""
  if x is None:
    return []
  if isinstance(x, (np.ndarray, torch.Tensor, dict, str)):
    return [x]
  return x if hasattr(x, '__iter__') else [x]


def to_dict(x, keys):
  """Converts list to a dictionary with supplied keys (ddsp/core.py:50-61)."""
  if isinstance(x, dict):
    return x
  x = make_iterable(x)
  if len(keys) != len(x):
    raise ValueError(f'Keys: {keys} must be the same length as {x}')
  return dict(zip(keys, x))


def nested_keys(nested_dict, delimiter='/', prefix=''):
  """Returns a flattened list of nested key strings (ddsp/core.py:76-102)."""
  keys = []
  for k, v in nested_dict.items():
    key = k if prefix == '' else f'{prefix}{delimiter}{k}'
    if not isinstance(v, dict):
      keys.append(key)
    else:
      keys += nested_keys(v, prefix=key)
  return keys


def nested_lookup(nested_key, nested_dict, delimiter='/'):
  """Returns the value of a nested dict according to "key/key/key" (ddsp/core.py:105-129)."""
  value = nested_dict
  for key in nested_key.split(delimiter):
    try:
      value = value[key]
    except KeyError:
      raise KeyError(f'Key \'{key}\' as a part of nested key \'{nested_key}\' '
                     'not found during nested dictionary lookup, out of '
                     f'available keys: {nested_keys(nested_dict)}')
  return value


# --------------------------------------------------------------------------------------
# scaling  (ddsp/core.py:386-404)
# --------------------------------------------------------------------------------------
def exp_sigmoid(x, exponent=10.0, max_value=2.0, threshold=1e-7):
  """Exponentiated sigmoid: max_value * sigmoid(x)**log(exponent) + threshold."""
  x = tf_float32(x)
  if _needs_grad(x):
    return _ExpSigmoidFunction.apply(x, float(exponent), float(max_value), float(threshold))
  return _exp_sigmoid_run(x, float(exponent), float(max_value), float(threshold))


def _exp_sigmoid_run(x, exponent, max_value, threshold):
  out = torch.empty_like(x)
  rc = _lib.load().ddsp_exp_sigmoid_f32(x.data_ptr(), out.data_ptr(), x.numel(), exponent, max_value, threshold, _stream())
  _lib.check(rc, 'ddsp_exp_sigmoid_f32')
  return out


class _ExpSigmoidFunction(torch.autograd.Function):
  """torch.autograd node of core.exp_sigmoid (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, x, exponent, max_value, threshold):
    ctx.save_for_backward(x)
    ctx.constants = (exponent, max_value, threshold)
    return _exp_sigmoid_run(x.detach(), exponent, max_value, threshold)

  @staticmethod
  def backward(ctx, grad_out):
    x, = ctx.saved_tensors
    grad_out = tf_float32(grad_out)
    grad_in = torch.empty_like(x)
    rc = _lib.load().ddsp_exp_sigmoid_backward_f32(x.data_ptr(), grad_out.data_ptr(), grad_in.data_ptr(), x.numel(),
                                                   *ctx.constants, _stream())
    _lib.check(rc, 'ddsp_exp_sigmoid_backward_f32')
    return grad_in, None, None, None


def safe_divide(numerator, denominator, eps=1e-7):
  """core.safe_divide (ddsp/core.py:207-210): numerator / where(denominator == 0, eps, denominator).

  The shapes are broadcast the way TF would; a denominator that only broadcasts along the last axis ([..., 1], what
  normalize_harmonics passes) is read in place."""
  numerator, denominator = tf_float32(numerator), tf_float32(denominator)
  require_no_grad('core.safe_divide', numerator, denominator)
  shape = torch.broadcast_shapes(numerator.shape, denominator.shape)
  num = numerator.expand(shape).contiguous()
  if len(shape) == 0:
    num, den_cols, den = num.reshape(1, 1), 1, denominator.reshape(1, 1).contiguous()
  elif denominator.dim() == len(shape) and tuple(denominator.shape[:-1]) == tuple(shape[:-1]) and denominator.shape[-1] == 1 \
      and shape[-1] != 1:
    den_cols, den = 1, denominator.contiguous()
  else:
    den_cols, den = int(shape[-1]), denominator.expand(shape).contiguous()
  cols = int(shape[-1]) if len(shape) else 1
  out = torch.empty(shape, dtype=torch.float32, device=num.device)
  rc = _lib.load().ddsp_safe_divide_f32(num.data_ptr(), den.data_ptr(), out.data_ptr(), num.numel() // max(cols, 1), cols,
                                        den_cols, float(eps), _stream())
  _lib.check(rc, 'ddsp_safe_divide_f32')
  return out


def safe_log(x, eps=1e-5):
  """core.safe_log (ddsp/core.py:213-216): log of x, non-positive entries replaced by eps first."""
  x = tf_float32(x).contiguous()
  require_no_grad('core.safe_log', x)
  out = torch.empty_like(x)
  rc = _lib.load().ddsp_safe_log_f32(x.data_ptr(), out.data_ptr(), x.numel(), float(eps), _stream())
  _lib.check(rc, 'ddsp_safe_log_f32')
  return out


def diff(x, axis=-1):
  """core.diff (ddsp/core.py:171-199): the finite difference along an axis, one element shorter there.

  Two slices and a subtraction in torch (differentiable); the reference's ValueError for an axis out of range."""
  x = tf_float32(x)
  ndim = x.dim()
  if axis >= ndim or axis < -ndim:
    raise ValueError('Invalid axis index: %d for tensor with only %d axes.' % (axis, ndim))
  lead = (slice(None),) * (axis % ndim)
  return x[lead + (slice(1, None),)] - x[lead + (slice(None, -1),)]


def get_harmonic_frequencies(frequencies, n_harmonics):
  """core.get_harmonic_frequencies (ddsp/core.py:1028-1045): [batch, :, 1] fundamentals -> [batch, :, n_harmonics]."""
  frequencies = tf_float32(frequencies).contiguous()
  require_no_grad('core.get_harmonic_frequencies', frequencies)
  if frequencies.dim() < 1 or frequencies.shape[-1] != 1:
    raise ValueError('frequencies must be [batch_size, :, 1], got {}'.format(tuple(frequencies.shape)))
  k = int(n_harmonics)
  out = torch.empty(tuple(frequencies.shape[:-1]) + (k,), dtype=torch.float32, device=frequencies.device)
  rc = _lib.load().ddsp_harmonic_frequencies_f32(frequencies.data_ptr(), out.data_ptr(), frequencies.numel(), k, _stream())
  _lib.check(rc, 'ddsp_harmonic_frequencies_f32')
  return out


def remove_above_nyquist(frequency_envelopes, amplitude_envelopes, sample_rate=16000):
  """core.remove_above_nyquist (ddsp/core.py:869-891): amplitudes of oscillators at or above sample_rate / 2 set to 0."""
  frequency_envelopes, amplitude_envelopes = tf_float32(frequency_envelopes), tf_float32(amplitude_envelopes)
  require_no_grad('core.remove_above_nyquist', frequency_envelopes, amplitude_envelopes)
  shape = torch.broadcast_shapes(frequency_envelopes.shape, amplitude_envelopes.shape)
  f = frequency_envelopes.expand(shape).contiguous()
  a = amplitude_envelopes.expand(shape).contiguous()
  out = torch.empty(shape, dtype=torch.float32, device=a.device)
  rc = _lib.load().ddsp_remove_above_nyquist_f32(f.data_ptr(), a.data_ptr(), out.data_ptr(), a.numel(), float(sample_rate),
                                                 _stream())
  _lib.check(rc, 'ddsp_remove_above_nyquist_f32')
  return out


def angular_cumsum(angular_frequency, chunk_size=1000):
  """core.angular_cumsum (ddsp/core.py:800-866): the accumulated phase in [0, 2 pi), shape [batch, time, ...].

  The scan runs in fp64 revolutions on chip (sums per chunk of 256 samples, a wrapped prefix over the chunks, the
  running phase inside each): `chunk_size` - the reference's guard against fp32 accumulation error - is accepted and has
  nothing to control; the result is the exactly accumulated phase rounded to fp32, where the reference's fp32 chunks are
  up to ~1e-2 rad off after a 4 s clip (a 3 kHz oscillator at 16 kHz).  Axis 0 is the batch and axis 1 time, as the reference's code has it; a 1-D input is
  taken as one clip."""
  del chunk_size
  w = tf_float32(angular_frequency)
  require_no_grad('core.angular_cumsum', w)
  if w.dim() < 1:
    raise ValueError('angular_frequency must be [batch, time, ...], got a scalar')
  squeeze = w.dim() == 1
  if squeeze:
    w = w[None]
  shape = tuple(w.shape)
  b, t = shape[0], shape[1]
  c = 1
  for d in shape[2:]:
    c *= int(d)
  w = w.contiguous()
  out = torch.empty(shape, dtype=torch.float32, device=w.device)
  if w.numel() == 0:
    return out[0] if squeeze else out
  lib = _lib.load()
  ws = _default_ws.get(lib.ddsp_angular_cumsum_workspace_bytes(b, t, c), w.device)
  rc = lib.ddsp_angular_cumsum_f32(w.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), b, t, c, _stream())
  _lib.check(rc, 'ddsp_angular_cumsum_f32')
  return out[0] if squeeze else out


# --------------------------------------------------------------------------------------
# resampling  (ddsp/core.py:573-714) - stand-alone; the synths evaluate it on the fly
# --------------------------------------------------------------------------------------
def resample(inputs, n_timesteps, method='linear', add_endpoint=True):
  """core.resample (ddsp/core.py:573-642): [n_frames] / [B, n_frames] / [B, n_frames, C] /
  [B, n_frames, n_freq, C] -> n_timesteps along time; methods 'nearest', 'linear', 'cubic', 'window'.  Differentiable in the
  input (the adjoint kernel, ddsp_resample_ex_backward_f32); the forward is the same call, to the bit, with or without a gradient."""
  inputs = tf_float32(inputs)
  is_1d, is_2d, is_4d = inputs.dim() == 1, inputs.dim() == 2, inputs.dim() == 4
  if is_1d:
    inputs = inputs[None, :, None]
  elif is_2d:
    inputs = inputs[:, :, None]
  if method not in RESAMPLE_METHODS:
    raise ValueError('Method ({}) is invalid. Must be one of {}.'.format(
        method, "['nearest', 'linear', 'cubic', 'window']"))
  if method == 'window':
    outputs = upsample_with_windows(inputs, n_timesteps, add_endpoint)     # ValueError unless 3-D
  elif is_4d:
    # tf.image.resize on [B, n_frames, n_freq, C] leaves the n_freq axis alone (core.py:613-621)
    b, f, q, c = inputs.shape
    outputs = _resample_call(inputs.reshape(b, f, q * c), int(n_timesteps), method, add_endpoint)
    outputs = outputs.reshape(b, int(n_timesteps), q, c)
  elif inputs.dim() == 3:
    outputs = _resample_call(inputs, int(n_timesteps), method, add_endpoint)
  else:
    raise ValueError('resample() takes 1-D to 4-D inputs, got shape {}'.format(tuple(inputs.shape)))
  if is_1d:
    outputs = outputs[0, :, 0]
  elif is_2d:
    outputs = outputs[:, :, 0]
  return outputs


def upsample_with_windows(inputs, n_timesteps, add_endpoint=True):
  """core.upsample_with_windows (ddsp/core.py:645-714): overlapping Hann windows,
  [B, n_frames, C] -> [B, n_timesteps, C]."""
  inputs = tf_float32(inputs)
  if inputs.dim() != 3:
    raise ValueError('Upsample_with_windows() only supports 3 dimensions, '
                     'not {}.'.format(tuple(inputs.shape)))
  n_frames = int(inputs.shape[1]) + (1 if add_endpoint else 0)   # the reference appends the endpoint frame
  n_intervals = n_frames - 1
  if n_frames >= n_timesteps:
    raise ValueError('Upsample with windows cannot be used for downsampling'
                     'More input frames ({}) than output timesteps ({})'.format(
                         n_frames, n_timesteps))
  if n_intervals <= 0 or n_timesteps % n_intervals != 0.0:
    raise ValueError(
        'For upsampling, the target the number of timesteps must be divisible '
        'by the number of input frames{}. (timesteps:{}, frames:{}, '
        'add_endpoint={}).'.format('' if add_endpoint else ' - 1', n_timesteps, n_frames, add_endpoint))
  return _resample_call(inputs, int(n_timesteps), 'window', add_endpoint)


class _ResampleFunction(torch.autograd.Function):
  """torch.autograd node of core.resample / upsample_with_windows on [B,F,C] (plumbing: both directions are C-ABI calls).
  Resampling is linear in its input: the backward is the adjoint kernel (ddsp_resample_ex_backward_f32), a gather with a fixed
  order of additions.  Nothing is kept for it but the shape."""

  @staticmethod
  def forward(ctx, inputs, n_timesteps, method, add_endpoint):
    ctx.args = (tuple(inputs.shape), n_timesteps, method, add_endpoint)
    return _resample_run(inputs, n_timesteps, method, add_endpoint)

  @staticmethod
  def backward(ctx, grad_out):
    (b, f, c), n_timesteps, method, add_endpoint = ctx.args
    grad_out = tf_float32(grad_out)
    grad_in = torch.empty((b, f, c), dtype=torch.float32, device=grad_out.device)
    if b and c:
      rc = _lib.load().ddsp_resample_ex_backward_f32(grad_out.data_ptr(), grad_in.data_ptr(), b, f, n_timesteps, c,
                                                     _lib.RESAMPLE_METHODS[method], 1 if add_endpoint else 0, _stream())
      _lib.check(rc, 'ddsp_resample_ex_backward_f32')
    return grad_in, None, None, None


def _resample_call(inputs, n_timesteps, method, add_endpoint):
  """[B,F,C] -> [B,N,C], differentiable in the input: the same forward call with or without a gradient."""
  inputs = inputs.contiguous()
  if _needs_grad(inputs):
    return _ResampleFunction.apply(inputs, n_timesteps, method, add_endpoint)
  return _resample_run(inputs, n_timesteps, method, add_endpoint)


def _resample_run(inputs, n_timesteps, method, add_endpoint):
  """[B,F,C] -> [B,N,C]: 'linear' / 'window' with the endpoint go to the stand-alone kernel of the hot
  path's own forms (ddsp_resample_f32), every other combination to the general one (ddsp_resample_ex_f32)."""
  b, f, c = inputs.shape
  out = torch.empty((b, n_timesteps, c), dtype=torch.float32, device=inputs.device)
  if b == 0 or c == 0:
    return out
  lib = _lib.load()
  if add_endpoint and method in ('linear', 'window'):
    rc = lib.ddsp_resample_f32(inputs.data_ptr(), out.data_ptr(), b, f, n_timesteps, c,
                               1 if method == 'window' else 0, _stream())
    _lib.check(rc, 'ddsp_resample_f32')
  else:
    rc = lib.ddsp_resample_ex_f32(inputs.data_ptr(), out.data_ptr(), b, f, n_timesteps, c,
                                  _lib.RESAMPLE_METHODS[method], 1 if add_endpoint else 0, _stream())
    _lib.check(rc, 'ddsp_resample_ex_f32')
  return out


def normalize_harmonics(harmonic_distribution, f0_hz=None, sample_rate=None):
  """core.normalize_harmonics (ddsp/core.py:894-907): optional Nyquist removal, then sum-normalise."""
  harmonic_distribution = tf_float32(harmonic_distribution)
  require_no_grad('core.normalize_harmonics', harmonic_distribution, f0_hz)
  b, f, k = harmonic_distribution.shape
  bandlimit = sample_rate is not None and f0_hz is not None
  f0 = tf_float32(f0_hz) if bandlimit else torch.zeros((b, f, 1), device=harmonic_distribution.device)
  ones = torch.ones((b, f, 1), dtype=torch.float32, device=harmonic_distribution.device)
  ctl_amp, ctl_hd = torch.empty_like(ones), torch.empty_like(harmonic_distribution)
  rc = _lib.load().ddsp_harmonic_controls_f32(
      ones.data_ptr(), harmonic_distribution.data_ptr(), f0.data_ptr(), ctl_amp.data_ptr(),
      ctl_hd.data_ptr(), b, f, k, int(sample_rate) if bandlimit else 2,
      _lib.HARM_NORMALIZE_NYQUIST if bandlimit else 0, _stream())
  _lib.check(rc, 'ddsp_harmonic_controls_f32')
  return ctl_hd


def get_fft_size(frame_size, ir_size, power_of_2=True):
  """core.get_fft_size (ddsp/core.py:1317-1335); host arithmetic, kept for API completeness."""
  convolved_frame_size = ir_size + frame_size - 1
  if power_of_2:
    return int(2**np.ceil(np.log2(convolved_frame_size)))
  from scipy import fftpack
  return int(fftpack.next_fast_len(convolved_frame_size))


def crop_and_compensate_delay(audio, audio_size, ir_size, padding, delay_compensation):
  """core.crop_and_compensate_delay (ddsp/core.py:1338-1379): a slice, no arithmetic."""
  if padding == 'valid':
    crop_size = ir_size + audio_size - 1
  elif padding == 'same':
    crop_size = audio_size
  else:
    raise ValueError('Padding must be \'valid\' or \'same\', instead '
                     'of {}.'.format(padding))
  total_size = int(audio.shape[-1])
  crop = total_size - crop_size
  start = ((ir_size - 1) // 2 - 1 if delay_compensation < 0 else delay_compensation)
  end = crop - start
  return audio[:, start:-end]


def oscillator_bank(frequency_envelopes, amplitude_envelopes, sample_rate=16000,
                    sum_sinusoids=True, use_angular_cumsum=False):
  """core.oscillator_bank (ddsp/core.py:912-962) on [batch, n_samples, n_sinusoids] envelopes.

  The phase scan runs in fp64 revolutions on chip, so both settings of `use_angular_cumsum`
  give the same (more exact) result.
  """
  del use_angular_cumsum
  frequency_envelopes = tf_float32(frequency_envelopes)
  amplitude_envelopes = tf_float32(amplitude_envelopes)
  require_no_grad('core.oscillator_bank', frequency_envelopes, amplitude_envelopes)
  if frequency_envelopes.dim() != 3 or frequency_envelopes.shape != amplitude_envelopes.shape:
    raise ValueError('frequency and amplitude envelopes must both be [batch, n_samples, n_sinusoids]'
                     ', got {} and {}'.format(tuple(frequency_envelopes.shape),
                                              tuple(amplitude_envelopes.shape)))
  b, n, k = frequency_envelopes.shape
  lib = _lib.load()
  out = torch.empty((b, n) if sum_sinusoids else (b, n, k), dtype=torch.float32,
                    device=frequency_envelopes.device)
  ws = _default_ws.get(lib.ddsp_oscillator_bank_workspace_bytes(b, n, k), frequency_envelopes.device)
  rc = lib.ddsp_oscillator_bank_f32(frequency_envelopes.data_ptr(), amplitude_envelopes.data_ptr(),
                                    out.data_ptr(), ws.data_ptr(), ws.numel(), b, n, k,
                                    int(sample_rate), 1 if sum_sinusoids else 0, _stream())
  _lib.check(rc, 'ddsp_oscillator_bank_f32')
  return out


# --------------------------------------------------------------------------------------
# harmonic synthesis  (ddsp/core.py:1048-1111)
# --------------------------------------------------------------------------------------
RESAMPLE_METHODS = ['nearest', 'linear', 'cubic', 'window']


def _check_amp_method(method, n_frames, n_samples):
  """The argument checks of core.resample / upsample_with_windows (core.py:633-634, 677-693)."""
  if method not in RESAMPLE_METHODS:
    raise ValueError('Method ({}) is invalid. Must be one of {}.'.format(
        method, "['nearest', 'linear', 'cubic', 'window']"))
  if method == 'window':
    if n_frames + 1 >= n_samples:
      raise ValueError('Upsample with windows cannot be used for downsampling'
                       'More input frames ({}) than output timesteps ({})'.format(
                           n_frames + 1, n_samples))
    if n_samples % n_frames != 0:
      raise ValueError(
          'For upsampling, the target the number of timesteps must be divisible '
          'by the number of input frames{}. (timesteps:{}, frames:{}, '
          'add_endpoint={}).'.format('', n_samples, n_frames + 1, True))


def _on_closed_form_kernels(method, n_frames, n_samples):
  """True where the synthesis kernels' closed forms apply ('window' / 'linear' envelopes, n_samples a
  multiple of n_frames); other argument combinations follow the reference's own chain of materialised
  envelopes (_harmonic_synthesis_materialised)."""
  return method in ('window', 'linear') and n_samples % n_frames == 0


def _harmonic_flags(scale, normalize, amp_resample_method, use_angular_cumsum):
  flags = 0
  if scale:
    flags |= _lib.HARM_SCALE_EXP_SIGMOID
  if normalize:
    flags |= _lib.HARM_NORMALIZE_NYQUIST
  if amp_resample_method == 'linear':
    flags |= _lib.HARM_AMP_LINEAR
  if use_angular_cumsum:
    flags |= _lib.HARM_ANGULAR_CUMSUM
  return flags


def _broadcast_batch(*tensors):
  """[1, frames, channels] inputs beside [batch, ..] ones: the reference's elementwise products broadcast them over the batch
  (its own test does: ddsp/core_test.py:549-590 passes shifts and a distribution of batch 1 with frequencies of batch 2).
  None passes through; anything else is left for the shape checks."""
  batches = [int(t.shape[0]) for t in tensors if t is not None and t.dim() == 3]
  b = max(batches) if batches else 1
  return tuple(t.expand(b, -1, -1).contiguous() if t is not None and t.dim() == 3 and t.shape[0] == 1 and b > 1 else t
               for t in tensors)


def _check_harmonic_shapes(amplitudes, harmonic_distribution, f0_hz):
  if harmonic_distribution.dim() != 3:
    raise ValueError('harmonic_distribution must be [batch, n_frames, n_harmonics], got {}'
                     .format(tuple(harmonic_distribution.shape)))
  b, f, _ = harmonic_distribution.shape
  for name, t in (('amplitudes', amplitudes), ('f0_hz', f0_hz)):
    if tuple(t.shape) != (b, f, 1):
      raise ValueError('{} must have shape [{}, {}, 1], got {}'.format(
          name, b, f, tuple(t.shape)))
  return b, f, harmonic_distribution.shape[2]


def harmonic_synthesis(frequencies, amplitudes, harmonic_shifts=None,
                       harmonic_distribution=None, n_samples=64000, sample_rate=16000,
                       amp_resample_method='window', use_angular_cumsum=False,
                       workspace=None, tf_op_order=False):
  """core.harmonic_synthesis (ddsp/core.py:1048-1111): frame-rate controls -> audio [batch, n_samples].

  'window' / 'linear' amplitude envelopes without harmonic_shifts (everything synths.Harmonic and the
  shipped gin configs ask for) run the closed-form synthesis kernels; harmonic_shifts, 'nearest' / 'cubic'
  envelopes and n_samples that is not a multiple of n_frames follow the reference's own chain
  (frame-rate tensors -> resample -> oscillator_bank) on materialised [B, N, K] envelopes.
  tf_op_order=True (extension, validation only) runs the slow kernel that follows the reference's
  fp32 op order exactly, sequential phase accumulation included.
  """
  frequencies, amplitudes = tf_float32(frequencies), tf_float32(amplitudes)
  if harmonic_shifts is not None:
    harmonic_shifts = tf_float32(harmonic_shifts)
  require_no_grad('core.harmonic_synthesis (Harmonic.__call__ is the differentiable entry)', frequencies, amplitudes,
                  harmonic_shifts, harmonic_distribution)
  if harmonic_distribution is not None:
    harmonic_distribution = tf_float32(harmonic_distribution)
  frequencies, amplitudes, harmonic_shifts, harmonic_distribution = _broadcast_batch(frequencies, amplitudes, harmonic_shifts,
                                                                                     harmonic_distribution)
  if harmonic_distribution is None:
    if harmonic_shifts is not None:                          # n_harmonics from the shifts (core.py:1082-1084)
      return _harmonic_synthesis_materialised(frequencies, amplitudes, harmonic_shifts, None, int(n_samples),
                                              int(sample_rate), amp_resample_method, use_angular_cumsum)
    harmonic_distribution = torch.ones_like(amplitudes)
  harmonic_distribution = tf_float32(harmonic_distribution)
  b, f, k = _check_harmonic_shapes(amplitudes, harmonic_distribution, frequencies)
  _check_amp_method(amp_resample_method, f, int(n_samples))
  if harmonic_shifts is not None or not _on_closed_form_kernels(amp_resample_method, f, int(n_samples)):
    if tf_op_order:
      raise NotImplementedError('tf_op_order covers the closed-form kernels\' argument space only')
    return _harmonic_synthesis_materialised(frequencies, amplitudes, harmonic_shifts, harmonic_distribution,
                                            int(n_samples), int(sample_rate), amp_resample_method,
                                            use_angular_cumsum)
  lib = _lib.load()
  audio = torch.empty((b, int(n_samples)), dtype=torch.float32, device=amplitudes.device)
  if tf_op_order:
    rc = lib.ddsp_harmonic_signal_tf_order_f32(
        amplitudes.data_ptr(), harmonic_distribution.data_ptr(), frequencies.data_ptr(),
        audio.data_ptr(), b, f, k, int(n_samples), int(sample_rate),
        _harmonic_flags(False, False, amp_resample_method, use_angular_cumsum), _stream())
    _lib.check(rc, 'ddsp_harmonic_signal_tf_order_f32')
    return audio
  nbytes = lib.ddsp_harmonic_workspace_bytes(b, f, k, int(n_samples))
  ws = (workspace or _default_ws).get(nbytes, amplitudes.device)
  harmonic_distribution = aligned16(harmonic_distribution)     # (the entry picks its kernel by this address)
  rc = lib.ddsp_harmonic_signal_f32(
      amplitudes.data_ptr(), harmonic_distribution.data_ptr(), frequencies.data_ptr(),
      audio.data_ptr(), ws.data_ptr(), ws.numel(), b, f, k, int(n_samples), int(sample_rate),
      _harmonic_flags(False, False, amp_resample_method, use_angular_cumsum), _stream())
  _lib.check(rc, 'ddsp_harmonic_signal_f32')
  return audio


def _harmonic_synthesis_materialised(frequencies, amplitudes, harmonic_shifts, harmonic_distribution,
                                     n_samples, sample_rate, amp_resample_method, use_angular_cumsum):
  """The reference's chain op for op (ddsp/core.py:1080-1111), each op a kernel of this library:
  harmonic_frequencies = f0 [1..K] (1 + shifts), harmonic_amplitudes = amplitudes * distribution
  (ddsp_harmonic_envelopes_f32), resample both to [B, N, K], oscillator_bank."""
  if amplitudes.dim() != 3 or amplitudes.shape[2] != 1 or frequencies.shape != amplitudes.shape:
    raise ValueError('frequencies and amplitudes must both be [batch, n_frames, 1], got {} and {}'.format(
        tuple(frequencies.shape), tuple(amplitudes.shape)))
  b, f, _ = amplitudes.shape
  per_harmonic = harmonic_distribution if harmonic_distribution is not None else harmonic_shifts
  if per_harmonic.dim() != 3 or tuple(per_harmonic.shape[:2]) != (b, f):
    raise ValueError('per-harmonic controls must be [{}, {}, n_harmonics], got {}'.format(
        b, f, tuple(per_harmonic.shape)))
  k = int(per_harmonic.shape[2])
  if harmonic_shifts is not None and tuple(harmonic_shifts.shape) != (b, f, k):
    raise ValueError('harmonic_shifts must be [{}, {}, {}], got {}'.format(b, f, k, tuple(harmonic_shifts.shape)))
  if amp_resample_method not in RESAMPLE_METHODS:
    raise ValueError('Method ({}) is invalid. Must be one of {}.'.format(
        amp_resample_method, "['nearest', 'linear', 'cubic', 'window']"))
  dev = amplitudes.device
  harmonic_frequencies = torch.empty((b, f, k), dtype=torch.float32, device=dev)
  harmonic_amplitudes = torch.empty((b, f, k), dtype=torch.float32, device=dev)
  rc = _lib.load().ddsp_harmonic_envelopes_f32(
      amplitudes.data_ptr(), harmonic_distribution.data_ptr() if harmonic_distribution is not None else None,
      frequencies.data_ptr(), harmonic_shifts.data_ptr() if harmonic_shifts is not None else None,
      harmonic_frequencies.data_ptr(), harmonic_amplitudes.data_ptr(), b, f, k, _stream())
  _lib.check(rc, 'ddsp_harmonic_envelopes_f32')
  frequency_envelopes = resample(harmonic_frequencies, n_samples)
  amplitude_envelopes = resample(harmonic_amplitudes, n_samples, method=amp_resample_method)
  return oscillator_bank(frequency_envelopes, amplitude_envelopes, sample_rate=sample_rate,
                         use_angular_cumsum=use_angular_cumsum)


def harmonic_oscillator_bank(frequency, amplitude_envelopes, initial_phase=None, sample_rate=16000,
                             use_angular_cumsum=True, workspace=None):
  """core.harmonic_oscillator_bank (ddsp/core.py:966-1025) -> (audio [batch, n_samples], final_phase [batch, 1, 1]).

  Audio-rate inputs: `frequency` [batch, n_samples, 1] (one fundamental per clip), `amplitude_envelopes`
  [batch, n_samples, n_sinusoids], `initial_phase` [batch, 1, 1] radians.  audio = sum_k A_k sin((k+1) phase),
  phase = cumsum(2 pi f / sr) + initial_phase, no Nyquist mask (as the reference); final_phase is the phase of the
  last sample, with the scan's part wrapped to [0, 2 pi) when use_angular_cumsum (the reference's default here).
  """
  frequency, amplitude_envelopes = tf_float32(frequency), tf_float32(amplitude_envelopes)
  require_no_grad('core.harmonic_oscillator_bank', frequency, amplitude_envelopes, initial_phase)
  if amplitude_envelopes.dim() != 3 or frequency.dim() != 3 or frequency.shape[2] != 1 or \
      tuple(frequency.shape[:2]) != tuple(amplitude_envelopes.shape[:2]):
    raise ValueError('frequency must be [batch, n_samples, 1] and amplitude_envelopes [batch, n_samples, n_sinusoids], '
                     'got {} and {}'.format(tuple(frequency.shape), tuple(amplitude_envelopes.shape)))
  b, n, k = amplitude_envelopes.shape
  dev = amplitude_envelopes.device
  if initial_phase is not None:
    initial_phase = tf_float32(initial_phase).reshape(-1)
    if initial_phase.numel() != b:
      raise ValueError('initial_phase must be [batch, 1, 1], got {} values for batch {}'.format(
          initial_phase.numel(), b))
    initial_phase = initial_phase.contiguous()
  audio = torch.empty((b, n), dtype=torch.float32, device=dev)
  final_phase = torch.empty((b, 1, 1), dtype=torch.float32, device=dev)
  if b == 0 or n == 0:
    return audio, final_phase
  lib = _lib.load()
  ws = (workspace or _default_ws).get(cached_workspace_bytes('ddsp_harmonic_oscillator_bank_workspace_bytes', b, n), dev)
  rc = lib.ddsp_harmonic_oscillator_bank_f32(
      frequency.data_ptr(), amplitude_envelopes.data_ptr(),
      initial_phase.data_ptr() if initial_phase is not None else None, audio.data_ptr(), final_phase.data_ptr(),
      ws.data_ptr(), ws.numel(), b, n, k, int(sample_rate), 1 if use_angular_cumsum else 0, _stream())
  _lib.check(rc, 'ddsp_harmonic_oscillator_bank_f32')
  return audio, final_phase


def streaming_harmonic_synthesis(frequencies, amplitudes, harmonic_distribution=None,
                                 initial_phase=None, n_samples=64000, sample_rate=16000,
                                 amp_resample_method='linear', workspace=None):
  """core.streaming_harmonic_synthesis (ddsp/core.py:1114-1164) -> (audio, final_phase).

  One chunk of audio [batch, n_samples] from frame-wise controls, with the fundamental's phase
  carried in (`initial_phase` [batch, 1, 1], radians) and out (`final_phase` [batch, 1, 1] =
  (sum of omega mod 2 pi) + initial_phase, as harmonic_oscillator_bank returns it with its
  default angular cumsum, core.py:1002-1012).  No audio-rate Nyquist mask, as in the reference.
  """
  frequencies, amplitudes = tf_float32(frequencies), tf_float32(amplitudes)
  flags = _lib.HARM_AMP_LINEAR if amp_resample_method == 'linear' else 0
  require_no_grad('core.streaming_harmonic_synthesis', frequencies, amplitudes, harmonic_distribution, initial_phase)
  n = int(n_samples)
  if harmonic_distribution is None and amplitudes.dim() == 3 and amplitudes.shape[-1] != 1:
    # amplitudes given PER HARMONIC [batch, n_frames, n_harmonics] and no distribution: the reference then takes them as the
    # harmonic amplitudes themselves (core.py:1150-1151, `harmonic_amplitudes = amplitudes` - its docstring says [.., 1], its code
    # takes any last axis; tools/fuzz_parity.py found this entry raising): the chain on materialised envelopes
    if frequencies.dim() != 3 or frequencies.shape[-1] != 1 or frequencies.shape[:2] != amplitudes.shape[:2]:
      raise ValueError('frequencies must have shape [{}, {}, 1], got {}'.format(amplitudes.shape[0], amplitudes.shape[1],
                                                                               tuple(frequencies.shape)))
    _check_amp_method(amp_resample_method, int(amplitudes.shape[1]), n)
    frequency_envelope = resample(frequencies, n)
    amplitude_envelopes = resample(amplitudes.contiguous(), n, method=amp_resample_method)
    return harmonic_oscillator_bank(frequency_envelope, amplitude_envelopes, initial_phase, sample_rate=sample_rate,
                                    workspace=workspace)
  if harmonic_distribution is None:
    harmonic_distribution = torch.ones_like(amplitudes)
    flags |= _lib.HARM_INPUTS_ARE_AMPLITUDES
  harmonic_distribution = tf_float32(harmonic_distribution)
  frequencies, amplitudes, harmonic_distribution = _broadcast_batch(frequencies, amplitudes, harmonic_distribution)
  b, f, k = _check_harmonic_shapes(amplitudes, harmonic_distribution, frequencies)
  _check_amp_method(amp_resample_method, f, n)
  if amp_resample_method not in ('linear', 'window') or n % f:
    # the closed-form kernel knows the two envelopes the shipped configs use on whole frames; everything else follows
    # the reference's own chain on materialised envelopes (core.py:1144-1164): normalize_harmonics, resample both,
    # harmonic_oscillator_bank - each a kernel of this library
    if flags & _lib.HARM_INPUTS_ARE_AMPLITUDES:
      harmonic_amplitudes = amplitudes
    else:
      hd_norm = normalize_harmonics(harmonic_distribution, frequencies, sample_rate)
      # amplitudes * distribution on ddsp_harmonic_envelopes_f32 (its harmonic-frequency output is not needed here)
      harmonic_amplitudes = torch.empty_like(hd_norm)
      unused = torch.empty_like(hd_norm)
      rc = _lib.load().ddsp_harmonic_envelopes_f32(
          amplitudes.data_ptr(), hd_norm.data_ptr(), frequencies.data_ptr(), None, unused.data_ptr(),
          harmonic_amplitudes.data_ptr(), b, f, k, _stream())
      _lib.check(rc, 'ddsp_harmonic_envelopes_f32')
    frequency_envelope = resample(frequencies, n)
    amplitude_envelopes = resample(harmonic_amplitudes, n, method=amp_resample_method)
    return harmonic_oscillator_bank(frequency_envelope, amplitude_envelopes, initial_phase, sample_rate=sample_rate,
                                    workspace=workspace)
  if n % f:
    raise ValueError('streaming_harmonic_synthesis needs n_samples ({}) to be a multiple of '
                     'n_frames ({}) on the MI355X path.'.format(n, f))
  dev = amplitudes.device
  if initial_phase is not None:
    initial_phase = tf_float32(initial_phase).reshape(-1)
    if initial_phase.numel() != b:
      raise ValueError('initial_phase must be [batch, 1, 1], got {} values for batch {}'.format(
          initial_phase.numel(), b))
    initial_phase = initial_phase.contiguous()
  lib = _lib.load()
  audio = torch.empty((b, n), dtype=torch.float32, device=dev)
  final_phase = torch.empty((b, 1, 1), dtype=torch.float32, device=dev)
  ws = (workspace or _default_ws).get(cached_workspace_bytes('ddsp_harmonic_workspace_bytes', b, f, k, n), dev)
  rc = lib.ddsp_harmonic_streaming_f32(
      amplitudes.data_ptr(), harmonic_distribution.data_ptr(), frequencies.data_ptr(),
      initial_phase.data_ptr() if initial_phase is not None else None, audio.data_ptr(),
      final_phase.data_ptr(), ws.data_ptr(), ws.numel(), b, f, k, n, int(sample_rate), flags,
      _stream())
  _lib.check(rc, 'ddsp_harmonic_streaming_f32')
  return audio, final_phase


# --------------------------------------------------------------------------------------
# time-varying FIR  (ddsp/core.py:1382-1565, 1628-1655)
# --------------------------------------------------------------------------------------
def frequency_impulse_response(magnitudes, window_size=0):
  """core.frequency_impulse_response: [B,F,M] (or [B,M]) magnitudes -> causal windowed IR."""
  magnitudes = tf_float32(magnitudes)
  squeeze = magnitudes.dim() == 2
  if squeeze:
    magnitudes = magnitudes[:, None, :].contiguous()
  if _needs_grad(magnitudes):
    ir = _FrequencyImpulseResponseFunction.apply(magnitudes, int(window_size))
  else:
    ir = _frequency_impulse_response_run(magnitudes, int(window_size))
  return ir[:, 0, :] if squeeze else ir


def _frequency_impulse_response_run(magnitudes, window_size):
  b, f, m = magnitudes.shape
  lib = _lib.load()
  size = lib.ddsp_fir_size(m, window_size)
  _lib.check(min(size, 0), 'ddsp_fir_size')
  ir = torch.empty((b, f, size), dtype=torch.float32, device=magnitudes.device)
  rc = lib.ddsp_frequency_impulse_response_f32(magnitudes.data_ptr(), ir.data_ptr(), b, f, m, window_size, _stream())
  _lib.check(rc, 'ddsp_frequency_impulse_response_f32')
  return ir


_design_cache = {}


def _fir_design(n_bands, window_size, device):
  """The design of frequency_impulse_response as a matrix [ir_size, n_bands]: it is linear in the magnitudes, so its columns
  are the impulse responses of the unit magnitude vectors - made by the forward kernel itself, once per (bands, window,
  device).  The backward pass multiplies by its transpose (ddsp_frequency_impulse_response_backward_f32)."""
  key = (n_bands, window_size, str(device))
  design = _design_cache.get(key)
  if design is None:
    with torch.no_grad():
      unit = torch.eye(n_bands, dtype=torch.float32, device=device)[None].contiguous()
      design = _frequency_impulse_response_run(unit, window_size)[0].t().contiguous()
    _design_cache[key] = design
  return design


class _FrequencyImpulseResponseFunction(torch.autograd.Function):
  """torch.autograd node of core.frequency_impulse_response (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, magnitudes, window_size):
    ctx.shape, ctx.window_size = tuple(magnitudes.shape), window_size
    return _frequency_impulse_response_run(magnitudes.detach(), window_size)

  @staticmethod
  def backward(ctx, grad_ir):
    b, f, m = ctx.shape
    grad_ir = tf_float32(grad_ir)
    size = int(grad_ir.shape[-1])
    design = _fir_design(m, ctx.window_size, grad_ir.device)
    grad_mag = torch.empty(ctx.shape, dtype=torch.float32, device=grad_ir.device)
    rc = _lib.load().ddsp_frequency_impulse_response_backward_f32(grad_ir.data_ptr(), design.data_ptr(), grad_mag.data_ptr(),
                                                                  b * f, m, size, _stream())
    if rc == _lib.ERR_UNSUPPORTED:
      raise NotImplementedError('the backward pass of frequency_impulse_response holds impulse responses of at most 12288 taps, '
                                'got {}'.format(size))
    _lib.check(rc, 'ddsp_frequency_impulse_response_backward_f32')
    return grad_mag, None


def apply_window_to_impulse_response(impulse_response, window_size=0, causal=False):
  """core.apply_window_to_impulse_response (ddsp/core.py:1477-1531): Hann-window a series of zero-phase (`causal`: causal)
  impulse responses [..., ir_size] and return them causal, cropped to the window when it is shorter."""
  impulse_response = tf_float32(impulse_response)
  require_no_grad('core.apply_window_to_impulse_response', impulse_response)
  if impulse_response.dim() < 1 or impulse_response.shape[-1] < 1:
    raise ValueError('impulse_response must be [..., ir_size], got {}'.format(tuple(impulse_response.shape)))
  l0 = int(impulse_response.shape[-1])
  lib = _lib.load()
  l = lib.ddsp_window_impulse_response_size(l0, int(window_size))
  flat = impulse_response.reshape(-1, l0).contiguous()
  out = torch.empty((flat.shape[0], l), dtype=torch.float32, device=flat.device)
  if flat.shape[0]:
    rc = lib.ddsp_apply_window_to_impulse_response_f32(flat.data_ptr(), out.data_ptr(), flat.shape[0], l0, int(window_size),
                                                       1 if causal else 0, _stream())
    _lib.check(rc, 'ddsp_apply_window_to_impulse_response_f32')
  return out.reshape(tuple(impulse_response.shape[:-1]) + (l,))


def _crop_range(audio_size, n_ir_frames, ir_size, padding, delay_compensation):
  """(start as requested, first kept index, number of kept samples) of the slice
  crop_and_compensate_delay (ddsp/core.py:1338-1379) takes from the overlap-added FFT frames of
  fft_convolve - python slice semantics included: audio[:, start:-end] is empty when the FFT size leaves
  nothing to crop at the end (end <= 0) or start is negative (ir_size <= 2 with automatic compensation)."""
  if padding == 'valid':
    crop_size = ir_size + audio_size - 1
  elif padding == 'same':
    crop_size = audio_size
  else:
    raise ValueError('Padding must be \'valid\' or \'same\', instead '
                     'of {}.'.format(padding))
  frame_size = int(np.ceil(audio_size / n_ir_frames))
  total_size = (n_ir_frames - 1) * frame_size + get_fft_size(frame_size, ir_size, power_of_2=True)
  start = (ir_size - 1) // 2 - 1 if delay_compensation < 0 else int(delay_compensation)
  end = (total_size - crop_size) - start
  kept = range(total_size)[start:-end]
  return start, (kept[0] if len(kept) else 0), len(kept)


def fft_convolve(audio, impulse_response, padding='same', delay_compensation=-1):
  """core.fft_convolve (ddsp/core.py:1382-1473), evaluated as the equivalent direct time-varying FIR
  (one long impulse response: as a partitioned FFT convolution), cropped as
  crop_and_compensate_delay (:1338-1379) crops the overlap-added FFT frames."""
  audio, impulse_response = tf_float32(audio), tf_float32(impulse_response)
  if audio.dim() != 2:
    raise ValueError('audio must be [batch, audio_timesteps], got {}'.format(tuple(audio.shape)))
  batch_size, audio_size = audio.shape
  if impulse_response.dim() == 2:
    impulse_response = impulse_response[:, None, :].contiguous()
  batch_size_ir, n_ir_frames, ir_size = impulse_response.shape
  if batch_size_ir == 1 and batch_size > 1:
    batch_size_ir_eff = batch_size        # broadcast (core.py:1433-1434), done in-kernel
  else:
    batch_size_ir_eff = batch_size_ir
  if batch_size != batch_size_ir_eff:
    raise ValueError('Batch size of audio ({}) and impulse response ({}) must '
                     'be the same.'.format(batch_size, batch_size_ir))
  _check_frames(audio_size, n_ir_frames)
  start_requested, start, n_out = _crop_range(audio_size, n_ir_frames, ir_size, padding, delay_compensation)
  if n_out == 0:
    return torch.empty((batch_size, 0), dtype=torch.float32, device=audio.device)
  crop = (start_requested, start, n_out, int(delay_compensation))
  if _needs_grad(audio, impulse_response):
    return _FftConvolveFunction.apply(audio, impulse_response, crop)
  return _fft_convolve_run(audio, impulse_response, crop)


def _fft_convolve_run(audio, impulse_response, crop):
  """fft_convolve on checked arguments: audio [B, N], impulse_response [B or 1, F, L], crop = (start as requested, first kept
  index, number of kept samples, delay_compensation)."""
  start_requested, start, n_out, delay_compensation = crop
  audio, impulse_response = aligned16(audio), aligned16(impulse_response)     # (the C entries pick their kernel by these addresses)
  batch_size, audio_size = audio.shape
  batch_size_ir, n_ir_frames, ir_size = impulse_response.shape
  if n_ir_frames == 1 and ir_size > LONG_IR_TAPS:
    # one long IR (a reverb): partitioned FFT convolution instead of the direct FIR
    return fft_convolve_long(audio, impulse_response[:, 0, :], delay=start, n_out=n_out)
  out = torch.empty((batch_size, n_out), dtype=torch.float32, device=audio.device)
  lib = _lib.load()
  rc = _lib.ERR_UNSUPPORTED
  if n_out == audio_size and start == start_requested:
    rc = lib.ddsp_fft_convolve_same_f32(
        audio.data_ptr(), impulse_response.data_ptr(), out.data_ptr(), batch_size, batch_size_ir,
        n_ir_frames, ir_size, audio_size, int(delay_compensation), _stream())
    if rc != _lib.ERR_UNSUPPORTED:     # a time-varying IR beyond the tiled kernel's LDS budget takes the general one
      _lib.check(rc, 'ddsp_fft_convolve_same_f32')
  if rc == _lib.ERR_UNSUPPORTED:
    rc = lib.ddsp_fft_convolve_f32(
        audio.data_ptr(), impulse_response.data_ptr(), out.data_ptr(), batch_size, batch_size_ir,
        n_ir_frames, ir_size, audio_size, n_out, start, _stream())
    _lib.check(rc, 'ddsp_fft_convolve_f32')
  return out


def _sum_rows(x, n_rows):
  """[n_rows, ...] -> [1, ...]: the rows added in row order (ddsp_sum_rows_f32)."""
  out = torch.empty((1,) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
  _lib.check(_lib.load().ddsp_sum_rows_f32(x.data_ptr(), out.data_ptr(), n_rows, x.numel() // n_rows, 0, _stream()),
             'ddsp_sum_rows_f32')
  return out


def _fft_convolve_backward(audio, impulse_response, grad_out, crop, need_audio, need_ir):
  """dL/d audio [B, N] and dL/d impulse_response [B or 1, F, L] of _fft_convolve_run: the two correlations of
  csrc/fir_grad.hip; for the one long impulse response of the FFT route the same two as FFT convolutions with reversed
  indices, as effects.Reverb runs them."""
  _, start, n_out, _ = crop
  b, n = audio.shape
  b_ir, f, l = impulse_response.shape
  g = tf_float32(grad_out)
  lib = _lib.load()
  grad_audio = grad_ir = None
  if f == 1 and l > LONG_IR_TAPS:
    if need_audio:       # dL/d audio = reverse(conv(reverse(g), ir)[n_out - N + start : n_out + start])
      grad_audio = fft_convolve_long(g, impulse_response[:, 0, :], delay=n_out - n + start, n_out=n, reverse_audio=True,
                                     reverse_out=True)
    if need_ir:          # dL/d ir[k] = conv(g, reverse(audio))[N - 1 - start + k]; taps below start - N + 1 meet no output
      k0 = max(0, start - n + 1)
      grad_ir = torch.zeros((b, 1, l), dtype=torch.float32, device=g.device) if k0 else None
      if l > k0:
        part = fft_convolve_long(g, audio, delay=n - 1 - start + k0, n_out=l - k0, reverse_ir=True)
        if k0:
          grad_ir[:, 0, k0:] = part
        else:
          grad_ir = part[:, None, :]
  else:
    if need_audio:
      grad_audio = torch.empty((b, n), dtype=torch.float32, device=g.device)
      rc = lib.ddsp_fft_convolve_grad_audio_f32(g.data_ptr(), impulse_response.data_ptr(), grad_audio.data_ptr(), b, b_ir, f, l, n,
                                                n_out, start, _stream())
      if rc == _lib.ERR_UNSUPPORTED:
        raise NotImplementedError('the backward pass of fft_convolve holds at most 65535 rows, got {}'.format(b))
      _lib.check(rc, 'ddsp_fft_convolve_grad_audio_f32')
    if need_ir:
      grad_ir = torch.empty((b, f, l), dtype=torch.float32, device=g.device)
      rc = lib.ddsp_fft_convolve_grad_ir_f32(g.data_ptr(), audio.data_ptr(), grad_ir.data_ptr(), b, f, l, n, n_out, start, _stream())
      if rc == _lib.ERR_UNSUPPORTED:
        raise NotImplementedError('the backward pass of fft_convolve holds at most 65535 rows and 65535 frames, got {} and {}'
                                  .format(b, f))
      _lib.check(rc, 'ddsp_fft_convolve_grad_ir_f32')
  if grad_ir is not None and b_ir == 1 and b > 1:
    grad_ir = _sum_rows(grad_ir.contiguous(), b)       # one impulse response for the batch collects the rows' gradients
  return grad_audio, grad_ir


class _FftConvolveFunction(torch.autograd.Function):
  """torch.autograd node of core.fft_convolve (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, audio, impulse_response, crop):
    ctx.save_for_backward(audio, impulse_response)
    ctx.crop = crop
    return _fft_convolve_run(audio.detach(), impulse_response.detach(), crop)

  @staticmethod
  def backward(ctx, grad_out):
    audio, impulse_response = ctx.saved_tensors
    grad_audio, grad_ir = _fft_convolve_backward(audio.detach(), impulse_response.detach(), grad_out, ctx.crop,
                                                 ctx.needs_input_grad[0], ctx.needs_input_grad[1])
    return grad_audio, grad_ir, None


LONG_IR_TAPS = 1024       # single-frame IRs longer than this take the FFT path


def fft_convolve_long(audio, impulse_response, delay=0, add_dry=False, mask_tap0=False,
                      workspace=None, n_out=None, reverse_audio=False, reverse_ir=False,
                      reverse_out=False, zero_out0=False):
  """out[b, n] = sum_k ir[b, k] audio[b, n + delay - k] (+ audio[b, n]) for one IR per row.

  The single-frame case of core.fft_convolve (ddsp/core.py:1428-1430, padding='same',
  crop start = delay) as effects.Reverb uses it (ddsp/effects.py:113-117), evaluated by
  ddsp_fft_convolve_long_ex_f32.  impulse_response [batch or 1, ir_size].  n_out (default
  n_samples) outputs per row; the reverse_* switches read an input / write the output with its
  index reversed (the correlations of the Reverb backward pass).
  """
  audio, impulse_response = tf_float32(audio), tf_float32(impulse_response)
  if audio.dim() != 2 or impulse_response.dim() != 2:
    raise ValueError('audio must be [batch, n_samples] and impulse_response [batch, ir_size], got '
                     '{} and {}'.format(tuple(audio.shape), tuple(impulse_response.shape)))
  b, n = audio.shape
  b_ir, l = impulse_response.shape
  if b_ir != b and b_ir != 1:
    raise ValueError('Batch size of audio ({}) and impulse response ({}) must '
                     'be the same.'.format(b, b_ir))
  if delay < 0:
    raise ValueError('delay must be >= 0, got {}'.format(delay))
  n_out = n if n_out is None else int(n_out)
  lib = _lib.load()
  nbytes = cached_workspace_bytes('ddsp_fft_convolve_long_ex_workspace_bytes', b, b_ir, n, l, n_out,
                                  int(delay))
  ws = (workspace if workspace is not None else Workspace()).get(nbytes, audio.device)
  out = torch.empty((b, n_out), dtype=torch.float32, device=audio.device)
  flags = ((_lib.CONV_ADD_DRY if add_dry else 0) | (_lib.CONV_MASK_TAP0 if mask_tap0 else 0) |
           (_lib.CONV_REVERSE_AUDIO if reverse_audio else 0) | (_lib.CONV_REVERSE_IR if reverse_ir else 0) |
           (_lib.CONV_REVERSE_OUT if reverse_out else 0) | (_lib.CONV_ZERO_OUT0 if zero_out0 else 0))
  rc = lib.ddsp_fft_convolve_long_ex_f32(audio.data_ptr(), impulse_response.data_ptr(), out.data_ptr(),
                                         ws.data_ptr(), ws.numel(), b, b_ir, n, l, n_out, int(delay),
                                         flags, _stream())
  if rc == -3:
    raise NotImplementedError('the FFT convolution holds fewer than 2**28 taps per row and at most 65535 rows, got {} taps, '
                              '{} rows'.format(l, b))
  _lib.check(rc, 'ddsp_fft_convolve_long_ex_f32')
  return out


def _check_frames(audio_size, n_ir_frames):
  """The frame-count check of core.fft_convolve (ddsp/core.py:1446-1457)."""
  frame_size = int(np.ceil(audio_size / n_ir_frames))
  n_audio_frames = int(math.ceil(audio_size / frame_size))
  if n_audio_frames != n_ir_frames:
    raise ValueError(
        'Number of Audio frames ({}) and impulse response frames ({}) do not '
        'match. For small hop size = ceil(audio_size / n_ir_frames), '
        'number of impulse response frames must be a multiple of the audio '
        'size.'.format(n_audio_frames, n_ir_frames))


def frequency_filter(audio, magnitudes, window_size=0, padding='same'):
  """core.frequency_filter = fft_convolve(audio, frequency_impulse_response(magnitudes))."""
  impulse_response = frequency_impulse_response(magnitudes, window_size=window_size)
  return fft_convolve(audio, impulse_response, padding=padding)


def sinc(x, threshold=1e-20):
  """core.sinc (ddsp/core.py:1568-1573): sin(pi x) / (pi x), |x| < threshold replaced by threshold.  Forward only on its own
  (sinc_impulse_response / sinc_filter are the differentiable entries)."""
  x = tf_float32(x)
  require_no_grad('core.sinc (sinc_impulse_response / sinc_filter are the differentiable entries)', x)
  out = torch.empty_like(x)
  _lib.check(_lib.load().ddsp_sinc_f32(x.data_ptr(), out.data_ptr(), x.numel(), float(threshold), _stream()), 'ddsp_sinc_f32')
  return out


def _sinc_ir_run(cutoff, window_size, sample_rate, high_pass, size):
  ir = torch.empty(tuple(cutoff.shape[:-1]) + (size,), dtype=torch.float32, device=cutoff.device)
  rc = _lib.load().ddsp_sinc_impulse_response_f32(cutoff.data_ptr(), ir.data_ptr(), cutoff.numel(), window_size, sample_rate,
                                                  1 if high_pass else 0, _stream())
  _lib.check(rc, 'ddsp_sinc_impulse_response_f32')
  return ir


class _SincImpulseResponseFunction(torch.autograd.Function):
  """torch.autograd node of core.sinc_impulse_response (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, cutoff, window_size, sample_rate, high_pass, size):
    ctx.save_for_backward(cutoff)
    ctx.args = (window_size, sample_rate, 1 if high_pass else 0)
    return _sinc_ir_run(cutoff.detach(), window_size, sample_rate, high_pass, size)

  @staticmethod
  def backward(ctx, grad_ir):
    cutoff, = ctx.saved_tensors
    grad_ir = tf_float32(grad_ir)
    grad_cutoff = torch.empty_like(cutoff)
    rc = _lib.load().ddsp_sinc_impulse_response_backward_f32(cutoff.data_ptr(), grad_ir.data_ptr(), grad_cutoff.data_ptr(),
                                                             cutoff.numel(), *ctx.args, _stream())
    _lib.check(rc, 'ddsp_sinc_impulse_response_backward_f32')
    return grad_cutoff, None, None, None, None


def sinc_impulse_response(cutoff_frequency, window_size=512, sample_rate=None, high_pass=False):
  """core.sinc_impulse_response (ddsp/core.py:1576-1625): cutoff_frequency [batch, n_time, 1] (Hertz when sample_rate is
  given, else a fraction of Nyquist; a scalar gives one filter, [1, 1, size]) -> Hamming-windowed sinc low-pass (high_pass:
  spectrally inverted) impulse responses [batch, n_time, (window_size // 2) * 2 + 1], normalised to unit gain.  The caller's
  tensor is left as it is (the reference scales a numpy argument in place).  Differentiable in cutoff_frequency."""
  cutoff = tf_float32(cutoff_frequency)
  if cutoff.dim() == 0:
    cutoff = cutoff.reshape(1, 1, 1)
  if cutoff.dim() != 3 or cutoff.shape[-1] != 1:
    raise ValueError('cutoff_frequency must be [batch_size, n_time, 1] or a scalar, got {}'.format(tuple(cutoff.shape)))
  window_size = int(window_size)
  if window_size < 0:
    raise ValueError('window_size must not be negative, got {}'.format(window_size))
  if sample_rate is not None and not float(sample_rate) > 0.0:
    raise ValueError('sample_rate must be positive, got {}'.format(sample_rate))
  rate = 0.0 if sample_rate is None else float(sample_rate)
  size = (window_size // 2) * 2 + 1
  if cutoff.numel() == 0:
    return torch.empty(tuple(cutoff.shape[:-1]) + (size,), dtype=torch.float32, device=cutoff.device)
  if _needs_grad(cutoff):
    return _SincImpulseResponseFunction.apply(cutoff, window_size, rate, bool(high_pass), size)
  return _sinc_ir_run(cutoff, window_size, rate, bool(high_pass), size)


def sinc_filter(audio, cutoff_frequency, window_size=512, sample_rate=None, padding='same', high_pass=False):
  """core.sinc_filter (ddsp/core.py:1658-1690) = fft_convolve(audio, sinc_impulse_response(cutoff_frequency, ...)) with the
  default delay compensation, which takes window_size // 2 - 1 samples off the start: the output lags the input by one
  sample, as the reference's does.  Differentiable in audio and cutoff_frequency."""
  impulse_response = sinc_impulse_response(cutoff_frequency, window_size=window_size, sample_rate=sample_rate,
                                           high_pass=high_pass)
  return fft_convolve(audio, impulse_response, padding=padding)


def prepare(n_harmonics=0, n_noise_bands=0, window_size=0):
  """Make the constant operand tables of the matrix-core kernels for these shapes on the current device now (C ABI
  ddsp_prepare): the one thing in the library that allocates and copies synchronously, once per device and shape, on first
  use otherwise - which must not happen inside a HIP-graph capture."""
  _lib.check(_lib.load().ddsp_prepare(int(n_harmonics), int(n_noise_bands), int(window_size)), 'ddsp_prepare')


def uniform_noise(batch_size, n_samples, seed=0, batch_offset=0, noise_bits=23):
  """The on-chip stand-in for tf.random.uniform([B, N], -1, 1) (ddsp/synths.py:192-193): what FilteredNoise generates
  for itself: the 2^23 levels of an fp32 uniform (noise_bits=23, the default) or 2048 levels (noise_bits=11)."""
  if noise_bits not in (11, 23):
    raise ValueError('noise_bits must be 11 or 23, got {!r}'.format(noise_bits))
  out = torch.empty((int(batch_size), int(n_samples)), dtype=torch.float32, device=_device())
  rc = _lib.load().ddsp_uniform_noise_ex_f32(out.data_ptr(), int(batch_size), int(n_samples),
                                             int(seed), int(batch_offset), int(noise_bits), _stream())
  _lib.check(rc, 'ddsp_uniform_noise_ex_f32')
  return out


# --------------------------------------------------------------------------------------
# wavetable synthesis and the variable-length delay  (ddsp/core.py:1167-1313)
# --------------------------------------------------------------------------------------
_wavetable_ws = Workspace()


def _needs_grad(*tensors):
  return torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)


def _lookup_shapes(phase, wavetables):
  """phase [B,N,1] / [B,N] -> [B,N]; wavetables [B,W] / [B,1,W] / [B,N,W] -> [B,Fw,W] (ddsp/core.py:1184-1190)."""
  if wavetables.dim() == 2:
    wavetables = wavetables[:, None, :]
  if phase.dim() == 3 and phase.shape[-1] == 1:
    phase = phase[:, :, 0]
  if phase.dim() != 2 or wavetables.dim() != 3:
    raise ValueError('phase must be [batch, n_samples, 1] or [batch, n_samples] and wavetables [batch, n_samples, n_wavetable] '
                     'or [batch, n_wavetable], got {} and {}'.format(tuple(phase.shape), tuple(wavetables.shape)))
  b, n = phase.shape
  if wavetables.shape[0] == 1 and b > 1:
    wavetables = wavetables.expand(b, -1, -1)
  if wavetables.shape[0] != b or wavetables.shape[1] not in (1, n) or wavetables.shape[2] < 1:
    raise ValueError('wavetables {} do not broadcast against phase {}'.format(tuple(wavetables.shape), tuple(phase.shape)))
  return phase.contiguous(), wavetables.contiguous()


class _LinearLookupFunction(torch.autograd.Function):
  """torch.autograd node of core.linear_lookup (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, phase, wavetables):
    ctx.save_for_backward(phase, wavetables)
    b, n = phase.shape
    out = torch.empty((b, n), dtype=torch.float32, device=phase.device)
    if out.numel():
      rc = _lib.load().ddsp_linear_lookup_f32(phase.data_ptr(), wavetables.data_ptr(), out.data_ptr(), b, n,
                                              wavetables.shape[1], wavetables.shape[2], _stream())
      _lib.check(rc, 'ddsp_linear_lookup_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    phase, wavetables = ctx.saved_tensors
    b, n = phase.shape
    grad_out = tf_float32(grad_out)
    grad_phase, grad_tables = torch.empty_like(phase), torch.empty_like(wavetables)
    if grad_out.numel():
      lib = _lib.load()
      ws = _wavetable_ws.get(cached_workspace_bytes('ddsp_linear_lookup_backward_workspace_bytes', b, n), phase.device)
      rc = lib.ddsp_linear_lookup_backward_f32(phase.data_ptr(), wavetables.data_ptr(), grad_out.data_ptr(),
                                               grad_phase.data_ptr(), grad_tables.data_ptr(), ws.data_ptr(), ws.numel(), b, n,
                                               wavetables.shape[1], wavetables.shape[2], _stream())
      _lib.check(rc, 'ddsp_linear_lookup_backward_f32')
    return grad_phase, grad_tables


def linear_lookup(phase, wavetables):
  """core.linear_lookup (ddsp/core.py:1167-1213): lookup from wavetables with linear interpolation, [batch, n_samples].

  sum_i relu(1 - |phase W - i|) w[i mod W] over the W + 1 points of the table with its first sample appended, evaluated as
  the two-point lerp it is (the reference builds three [batch, n_samples, W + 1] tensors).  The phase is not wrapped: outside
  [0, 1] the result fades to 0 within one table step, as the reference's weights do.  Differentiable in both arguments."""
  phase, wavetables = tf_float32(phase), tf_float32(wavetables)
  phase2, tables3 = _lookup_shapes(phase, wavetables)
  if _needs_grad(phase, wavetables):
    return _LinearLookupFunction.apply(phase2, tables3)
  return _LinearLookupFunction.forward(_NoCtx(), phase2, tables3)


class _NoCtx:
  """Stands in for the autograd context when nothing requires grad (the forward bodies are shared)."""

  def save_for_backward(self, *tensors):
    pass


def _wavetable_shapes(frequencies, amplitudes, wavetables, n_samples):
  """-> contiguous amplitudes [B,F,1], wavetables [B,Fw,W], frequencies [B,F,1]; the reference's ValueErrors."""
  if wavetables.dim() == 2:
    wavetables = wavetables[:, None, :]
  if frequencies.dim() == 2:
    frequencies = frequencies[:, :, None]
  if amplitudes.dim() == 2:
    amplitudes = amplitudes[:, :, None]
  if wavetables.dim() != 3 or wavetables.shape[-1] < 1:
    raise ValueError('wavetables must be [batch, n_wavetable] or [batch, n_frames, n_wavetable], got {}'.format(
        tuple(wavetables.shape)))
  if frequencies.dim() != 3 or frequencies.shape[-1] != 1 or amplitudes.dim() != 3 or amplitudes.shape[-1] != 1:
    raise ValueError('frequencies and amplitudes must be [batch, n_frames, 1], got {} and {}'.format(
        tuple(frequencies.shape), tuple(amplitudes.shape)))
  amplitudes, wavetables, frequencies = _broadcast_batch(amplitudes, wavetables, frequencies)
  b, f, _ = amplitudes.shape
  _check_amp_method('window', f, int(n_samples))          # the amplitude envelope's own conditions (core.py:677-693)
  if tuple(frequencies.shape) != (b, f, 1):
    raise ValueError('frequencies {} and amplitudes {} must have the same batch size and number of frames'.format(
        tuple(frequencies.shape), tuple(amplitudes.shape)))
  if wavetables.shape[0] != b:
    raise ValueError('wavetables {} must have the batch size of the amplitudes {}'.format(
        tuple(wavetables.shape), tuple(amplitudes.shape)))
  return amplitudes.contiguous(), wavetables.contiguous(), frequencies.contiguous()


class _WavetableFunction(torch.autograd.Function):
  """torch.autograd node of core.wavetable_synthesis / synths.Wavetable (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, amplitudes, wavetables, frequencies, n_samples, sample_rate, flags):
    ctx.save_for_backward(amplitudes, wavetables, frequencies)
    ctx.args = (int(n_samples), float(sample_rate), int(flags))
    b, f, _ = amplitudes.shape
    out = torch.empty((b, int(n_samples)), dtype=torch.float32, device=amplitudes.device)
    if b:
      rc = _lib.load().ddsp_wavetable_f32(amplitudes.data_ptr(), wavetables.data_ptr(), frequencies.data_ptr(), out.data_ptr(),
                                          b, f, wavetables.shape[1], wavetables.shape[2], int(n_samples), float(sample_rate),
                                          int(flags), _stream())
      _lib.check(rc, 'ddsp_wavetable_f32')
    return out

  @staticmethod
  def backward(ctx, grad_audio):
    amplitudes, wavetables, frequencies = ctx.saved_tensors
    n_samples, sample_rate, flags = ctx.args
    b, f, _ = amplitudes.shape
    fw, w = wavetables.shape[1], wavetables.shape[2]
    grad_audio = tf_float32(grad_audio)
    g_amp, g_tab, g_f0 = torch.empty_like(amplitudes), torch.empty_like(wavetables), torch.empty_like(frequencies)
    if b:
      lib = _lib.load()
      ws = _wavetable_ws.get(cached_workspace_bytes('ddsp_wavetable_backward_workspace_bytes', b, f, fw, w, n_samples),
                             amplitudes.device)
      rc = lib.ddsp_wavetable_backward_f32(amplitudes.data_ptr(), wavetables.data_ptr(), frequencies.data_ptr(),
                                           grad_audio.data_ptr(), g_amp.data_ptr(), g_tab.data_ptr(), g_f0.data_ptr(),
                                           ws.data_ptr(), ws.numel(), b, f, fw, w, n_samples, sample_rate, flags, _stream())
      _lib.check(rc, 'ddsp_wavetable_backward_f32')
    return g_amp, g_tab, g_f0, None, None, None


def _wavetable(frequencies, amplitudes, wavetables, n_samples, sample_rate, flags):
  frequencies, amplitudes, wavetables = tf_float32(frequencies), tf_float32(amplitudes), tf_float32(wavetables)
  amps3, tables3, freq3 = _wavetable_shapes(frequencies, amplitudes, wavetables, n_samples)
  if _needs_grad(frequencies, amplitudes, wavetables):
    return _WavetableFunction.apply(amps3, tables3, freq3, n_samples, sample_rate, flags)
  return _WavetableFunction.forward(_NoCtx(), amps3, tables3, freq3, n_samples, sample_rate, flags)


def wavetable_synthesis(frequencies, amplitudes, wavetables, n_samples=64000, sample_rate=16000):
  """core.wavetable_synthesis (ddsp/core.py:1236-1283): monophonic wavetable synthesizer, [batch, n_samples].

  frequencies, amplitudes [batch, n_frames, 1]; wavetables [batch, n_wavetable] (static) or [batch, n_table_frames,
  n_wavetable] (resampled linearly to n_samples, as the reference does; n_table_frames is free).  The amplitude envelope
  is the 'window' upsampling, the phase the exclusive cumulative sum of the linearly upsampled frequency in cycles,
  wrapped to [0, 1).  One kernel per call; the tables are read at frame rate and no [batch, n_samples, n_wavetable] tensor
  exists.  Differentiable in all three inputs."""
  return _wavetable(frequencies, amplitudes, wavetables, n_samples, sample_rate, 0)


class _DelayFunction(torch.autograd.Function):
  """torch.autograd node of core.variable_length_delay / effects.ModDelay (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, phase, audio, gain, max_length, phase_scale, phase_offset, flags):
    ctx.save_for_backward(phase, audio, gain)
    ctx.args = (int(max_length), float(phase_scale), float(phase_offset), int(flags))
    b, n = audio.shape
    out = torch.empty_like(audio)
    if out.numel():
      rc = _lib.load().ddsp_variable_length_delay_f32(phase.data_ptr(), audio.data_ptr(),
                                                      gain.data_ptr() if gain is not None else None, out.data_ptr(), b, n,
                                                      int(max_length), float(phase_scale), float(phase_offset), int(flags),
                                                      _stream())
      _lib.check(rc, 'ddsp_variable_length_delay_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    phase, audio, gain = ctx.saved_tensors
    max_length, phase_scale, phase_offset, flags = ctx.args
    b, n = audio.shape
    grad_out = tf_float32(grad_out)
    g_phase, g_audio = torch.empty_like(phase), torch.empty_like(audio)
    g_gain = torch.empty_like(gain) if gain is not None else None
    if grad_out.numel():
      lib = _lib.load()
      ws = _wavetable_ws.get(cached_workspace_bytes('ddsp_variable_length_delay_backward_workspace_bytes', b, n), audio.device)
      rc = lib.ddsp_variable_length_delay_backward_f32(
          phase.data_ptr(), audio.data_ptr(), gain.data_ptr() if gain is not None else None, grad_out.data_ptr(),
          g_phase.data_ptr(), g_audio.data_ptr(), g_gain.data_ptr() if g_gain is not None else None, ws.data_ptr(), ws.numel(),
          b, n, max_length, phase_scale, phase_offset, flags, _stream())
      _lib.check(rc, 'ddsp_variable_length_delay_backward_f32')
    return g_phase, g_audio, g_gain, None, None, None, None


def _delay(phase, audio, gain, max_length, phase_scale, phase_offset, flags):
  """phase / gain [B,N,1] or [B,N], audio [B,N] -> [B,N] (the body of variable_length_delay and ModDelay.get_signal)."""
  phase, audio = tf_float32(phase), tf_float32(audio)
  gain = tf_float32(gain) if gain is not None else None
  if audio.dim() != 2:
    raise ValueError('audio must be [batch, n_samples], got {}'.format(tuple(audio.shape)))
  b, n = audio.shape

  def flat(x, name):
    if x.dim() == 3 and x.shape[-1] == 1:
      x = x[:, :, 0]
    if x.dim() != 2 or x.shape[1] != n or x.shape[0] not in (1, b):
      raise ValueError('{} must be [batch, n_samples, 1] or [batch, n_samples] for audio {}, got {}'.format(
          name, tuple(audio.shape), tuple(x.shape)))
    return x.expand(b, n).contiguous()

  if int(max_length) < 1:
    raise ValueError('max_length must be at least 1, got {}'.format(max_length))
  phase2 = flat(phase, 'phase')
  gain2 = flat(gain, 'gain') if gain is not None else None
  audio2 = audio.contiguous()
  if _needs_grad(phase, audio, gain):
    return _DelayFunction.apply(phase2, audio2, gain2, max_length, phase_scale, phase_offset, flags)
  return _DelayFunction.forward(_NoCtx(), phase2, audio2, gain2, max_length, phase_scale, phase_offset, flags)


def variable_length_delay(phase, audio, max_length=512):
  """core.variable_length_delay (ddsp/core.py:1286-1313): delay audio by a time-varying amount, [batch, n_samples].

  phase in [0, 1] is a delay of 0 .. max_length samples, linearly interpolated between the two neighbouring taps, which are
  read straight from `audio` (zero before the clip's start): the reference's [batch, n_samples, max_length] frame tensor is
  never built.  As in the reference, the point at full phase is the appended wrap point and reads the UNDELAYED sample.
  Differentiable in both arguments."""
  return _delay(phase, audio, None, max_length, 1.0, 0.0, 0)


# --------------------------------------------------------------------------------------
# unit / MIDI / Hz conversions and the frequency scale functions  (ddsp/core.py:219-348, 414-507)
# --------------------------------------------------------------------------------------
def _convert(op, x, p0=0.0, p1=0.0):
  x = tf_float32(x)
  require_no_grad('core.' + op.replace('_clip', '').replace('_zero_silence', ''), x)
  out = torch.empty_like(x)
  if x.numel():
    rc = _lib.load().ddsp_unit_convert_f32(x.data_ptr(), out.data_ptr(), x.numel(), _lib.CONVERT_OPS[op], float(p0), float(p1),
                                           _stream())
    _lib.check(rc, 'ddsp_unit_convert_f32')
  return out


def logb(x, base=2.0, eps=1e-5):
  """core.logb (ddsp/core.py:219-221): safe_log(x, eps) / safe_log(base, eps), the divisor made safe the same way."""
  den = math.log(eps if base <= 0.0 else base)
  return _convert('logb', x, eps if den == 0.0 else den, eps)


def midi_to_hz(notes, midi_zero_silence=False):
  """core.midi_to_hz (ddsp/core.py:280-297): 440 * 2^((notes - 69) / 12); MIDI 0 -> 0 Hz with midi_zero_silence."""
  return _convert('midi_to_hz_zero_silence' if midi_zero_silence else 'midi_to_hz', notes)


def hz_to_midi(frequencies):
  """core.hz_to_midi (ddsp/core.py:300-306): 12 (log2 f - log2 440) + 69, frequencies <= 0 map to MIDI 0."""
  return _convert('hz_to_midi', frequencies)


def _hz_to_midi_number(hz):
  hz = float(hz)
  return 0.0 if hz <= 0.0 else 12.0 * (math.log2(hz) - math.log2(440.0)) + 69.0


def unit_to_midi(unit, midi_min=20.0, midi_max=90.0, clip=False):
  """core.unit_to_midi (ddsp/core.py:309-315): the unit interval [0, 1] to MIDI notes."""
  return _convert('unit_to_midi_clip' if clip else 'unit_to_midi', unit, midi_min, midi_max)


def midi_to_unit(midi, midi_min=20.0, midi_max=90.0, clip=False):
  """core.midi_to_unit (ddsp/core.py:318-324): MIDI notes to the unit interval [0, 1]."""
  return _convert('midi_to_unit_clip' if clip else 'midi_to_unit', midi, midi_min, midi_max)


DB_RANGE = 80.0


def _convert_db(op, x, p0=0.0, p1=0.0):
  x = tf_float32(x).contiguous()
  require_no_grad('core.' + op, x)
  out = torch.empty_like(x)
  if x.numel():
    rc = _lib.load().ddsp_db_convert_f32(x.data_ptr(), out.data_ptr(), x.numel(), _lib.DB_OPS[op], float(p0), float(p1), _stream())
    _lib.check(rc, 'ddsp_db_convert_f32')
  return out


def power_to_db(power, ref_db=0.0, range_db=DB_RANGE, use_tf=True):
  """core.power_to_db (ddsp/core.py:253-267): max(10 log10(max(10^(-range_db / 10), power)) - ref_db, -range_db).  `use_tf` is
  accepted and ignored (one implementation)."""
  del use_tf
  return _convert_db('power_to_db', power, ref_db, range_db)


def amplitude_to_db(amplitude, ref_db=0.0, range_db=DB_RANGE, use_tf=True):
  """core.amplitude_to_db (ddsp/core.py:247-250): power_to_db of amplitude^2."""
  del use_tf
  return _convert_db('amplitude_to_db', amplitude, ref_db, range_db)


def db_to_power(db):
  """core.db_to_power (ddsp/core.py:275-277): 10^(db / 10)."""
  return _convert_db('db_to_power', db)


def db_to_amplitude(db):
  """core.db_to_amplitude (ddsp/core.py:270-272): db_to_power(db / 2)."""
  return _convert_db('db_to_amplitude', db)


def unit_to_hz(unit, hz_min, hz_max, clip=False):
  """core.unit_to_hz (ddsp/core.py:327-336): [0, 1] to [hz_min, hz_max] on a logarithmic scale (the bounds are numbers)."""
  return midi_to_hz(unit_to_midi(unit, _hz_to_midi_number(hz_min), _hz_to_midi_number(hz_max), clip))


def hz_to_unit(hz, hz_min, hz_max, clip=False):
  """core.hz_to_unit (ddsp/core.py:339-348): [hz_min, hz_max] to [0, 1] on a logarithmic scale (the bounds are numbers)."""
  return midi_to_unit(hz_to_midi(hz), _hz_to_midi_number(hz_min), _hz_to_midi_number(hz_max), clip)


def _depth_layout(freqs, depth):
  """[B, T, K * depth] or [B, T, K, depth] -> (contiguous [B, T, K * depth], K, depth) (ddsp/core.py:414-420, 441-445)."""
  if freqs.dim() == 4:
    b, t, k, depth = freqs.shape
    return freqs.reshape(b, t, k * depth).contiguous(), int(k), int(depth)
  if freqs.dim() != 3:
    raise ValueError('freqs must be [batch, time, n_sinusoids * depth] or [batch, time, n_sinusoids, depth], got {}'.format(
        tuple(freqs.shape)))
  depth = int(depth)
  if depth < 1 or freqs.shape[-1] % depth != 0:
    raise ValueError('the last axis of freqs ({}) is not a multiple of depth ({})'.format(freqs.shape[-1], depth))
  return freqs.contiguous(), int(freqs.shape[-1]) // depth, depth


class _FrequencyScaleFunction(torch.autograd.Function):
  """torch.autograd node of core.frequencies_sigmoid / frequencies_softmax (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, freqs, k, depth, hz_min, hz_max, flag):
    ctx.save_for_backward(freqs)
    ctx.args = (k, depth, hz_min, hz_max, flag)
    b, t, _ = freqs.shape
    out = torch.empty((b, t, k), dtype=torch.float32, device=freqs.device)
    if out.numel():
      rc = _lib.load().ddsp_sinusoidal_controls_f32(None, freqs.data_ptr(), None, out.data_ptr(), b * t, k, depth, hz_min, hz_max,
                                                    2.0, flag, _stream())
      _lib.check(rc, 'ddsp_sinusoidal_controls_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    freqs, = ctx.saved_tensors
    k, depth, hz_min, hz_max, flag = ctx.args
    b, t, _ = freqs.shape
    grad_out = tf_float32(grad_out)
    grad = torch.empty_like(freqs)
    if grad.numel():
      rc = _lib.load().ddsp_sinusoidal_controls_backward_f32(None, freqs.data_ptr(), None, grad_out.data_ptr(), None, grad.data_ptr(),
                                                             b * t, k, depth, hz_min, hz_max, 2.0, flag, _stream())
      _lib.check(rc, 'ddsp_sinusoidal_controls_backward_f32')
    return grad, None, None, None, None, None


def _frequency_scale(freqs, depth, hz_min, hz_max, flag):
  raw = tf_float32(freqs)
  flat, k, depth = _depth_layout(raw, depth)
  if flag == _lib.SIN_FREQ_SIGMOID and depth > _lib.SIN_MAX_SIGMOID_DEPTH:
    raise NotImplementedError('frequencies_sigmoid takes up to {} terms per sinusoid on the MI355X path, got depth={}'.format(
        _lib.SIN_MAX_SIGMOID_DEPTH, depth))
  args = (flat, k, depth, float(hz_min), float(hz_max), flag)
  if _needs_grad(raw):
    return _FrequencyScaleFunction.apply(*args)
  return _FrequencyScaleFunction.forward(_NoCtx(), *args)


def frequencies_softmax(freqs, depth=1, hz_min=20.0, hz_max=8000.0):
  """core.frequencies_softmax (ddsp/core.py:423-456): softmax over `depth` network outputs per sinusoid, the expected
  position on a unit grid mapped logarithmically to [hz_min, hz_max] Hz.  freqs [batch, time, n_sinusoids * depth] or
  [batch, time, n_sinusoids, depth] -> [batch, time, n_sinusoids].  One kernel; differentiable."""
  return _frequency_scale(freqs, depth, hz_min, hz_max, _lib.SIN_FREQ_SOFTMAX)


def frequencies_sigmoid(freqs, depth=1, hz_min=0.0, hz_max=8000.0):
  """core.frequencies_sigmoid (ddsp/core.py:459-507): a sum of `depth` sigmoids per sinusoid, each mapped logarithmically to
  its share of [hz_min, hz_max] (the shares shrink by a constant factor; their bounds are host-side constants).  Shapes
  as frequencies_softmax.  One kernel; differentiable; depth <= 64."""
  return _frequency_scale(freqs, depth, hz_min, hz_max, _lib.SIN_FREQ_SIGMOID)


def harmonic_to_sinusoidal(harm_amp, harm_dist, f0_hz, sample_rate=16000):
  """core.harmonic_to_sinusoidal (ddsp/core.py:784-794): controls of a harmonic synth -> (amplitudes, frequencies) of a
  sinusoidal one, both [batch, n_frames, n_harmonics]: harmonics at or above Nyquist removed, the distribution
  renormalised, multiplied by the amplitude."""
  harm_amp, harm_dist, f0_hz = tf_float32(harm_amp), tf_float32(harm_dist), tf_float32(f0_hz)
  require_no_grad('core.harmonic_to_sinusoidal', harm_amp, harm_dist, f0_hz)
  if harm_dist.dim() == 3 and harm_amp.dim() < 3:        # the reference multiplies: a number broadcasts (core_test.py:98)
    harm_amp = harm_amp.reshape((1,) * (3 - harm_amp.dim()) + tuple(harm_amp.shape)).expand(
        harm_dist.shape[0], harm_dist.shape[1], 1).contiguous()
  harm_amp, harm_dist, f0_hz = _broadcast_batch(harm_amp, harm_dist, f0_hz)
  b, f, k = _check_harmonic_shapes(harm_amp, harm_dist, f0_hz)
  harm_dist = normalize_harmonics(harm_dist, f0_hz, sample_rate)
  freqs, amps = torch.empty_like(harm_dist), torch.empty_like(harm_dist)
  if freqs.numel():
    rc = _lib.load().ddsp_harmonic_envelopes_f32(harm_amp.data_ptr(), harm_dist.data_ptr(), f0_hz.data_ptr(), None, freqs.data_ptr(),
                                                 amps.data_ptr(), b, f, k, _stream())
    _lib.check(rc, 'ddsp_harmonic_envelopes_f32')
  return amps, freqs


# --------------------------------------------------------------------------------------
# sinusoidal_to_harmonic and the differentiable pieces under the consistency losses  (csrc/consistency.hip)
# --------------------------------------------------------------------------------------
def _frames3(name, x):
  if x.dim() != 3:
    raise ValueError('{} must be [batch, time, n], got shape {}'.format(name, tuple(x.shape)))
  return x


class _SinusoidalToHarmonicFunction(torch.autograd.Function):
  """torch.autograd node of core.sinusoidal_to_harmonic (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, sin_amps, sin_freqs, f0_hz, args):
    ctx.save_for_backward(sin_amps, sin_freqs, f0_hz)
    ctx.args = args
    b, t, k = sin_amps.shape
    h = args[0]
    harm_amp = torch.empty((b, t, 1), dtype=torch.float32, device=sin_amps.device)
    harm_dist = torch.empty((b, t, h), dtype=torch.float32, device=sin_amps.device)
    if b * t:
      rc = _lib.load().ddsp_sinusoidal_to_harmonic_f32(sin_amps.data_ptr(), sin_freqs.data_ptr(), f0_hz.data_ptr(),
                                                       harm_amp.data_ptr(), harm_dist.data_ptr(), b * t, k, *args, _stream())
      _lib.check(rc, 'ddsp_sinusoidal_to_harmonic_f32')
    return harm_amp, harm_dist

  @staticmethod
  def backward(ctx, grad_amp, grad_dist):
    sin_amps, sin_freqs, f0_hz = ctx.saved_tensors
    b, t, k = sin_amps.shape
    grad_amp, grad_dist = tf_float32(grad_amp), tf_float32(grad_dist)
    g_amps, g_freqs, g_f0 = torch.empty_like(sin_amps), torch.empty_like(sin_freqs), torch.empty_like(f0_hz)
    if b * t:
      rc = _lib.load().ddsp_sinusoidal_to_harmonic_backward_f32(
          sin_amps.data_ptr(), sin_freqs.data_ptr(), f0_hz.data_ptr(), grad_amp.data_ptr(), grad_dist.data_ptr(),
          g_amps.data_ptr(), g_freqs.data_ptr(), g_f0.data_ptr(), b * t, k, *ctx.args, _stream())
      _lib.check(rc, 'ddsp_sinusoidal_to_harmonic_backward_f32')
    return g_amps, g_freqs, g_f0, None


def sinusoidal_to_harmonic(sin_amps, sin_freqs, f0_hz, harmonic_width=0.1, n_harmonics=100, sample_rate=16000,
                           normalize=False):
  """core.sinusoidal_to_harmonic (ddsp/core.py:733-781): extract harmonic components from sinusoids given a fundamental.

  sin_amps, sin_freqs [batch, time, n_sinusoids], f0_hz [batch, time, 1] -> (harm_amp [batch, time, 1], harm_dist
  [batch, time, n_harmonics]).  One kernel per direction, a block per frame: the [batch, time, n_harmonics, n_sinusoids]
  weights the reference builds five times are never stored.  Differentiable in all three inputs.  Up to 1024 sinusoids
  and 1024 harmonics."""
  sin_amps, sin_freqs, f0_hz = tf_float32(sin_amps), tf_float32(sin_freqs), tf_float32(f0_hz)
  _frames3('sin_amps', sin_amps), _frames3('sin_freqs', sin_freqs), _frames3('f0_hz', f0_hz)
  if sin_amps.shape != sin_freqs.shape or f0_hz.shape[:2] != sin_amps.shape[:2] or f0_hz.shape[2] != 1:
    raise ValueError('sin_amps and sin_freqs must be [batch, time, n_sinusoids] and f0_hz [batch, time, 1], got {}, {} and {}'.format(
        tuple(sin_amps.shape), tuple(sin_freqs.shape), tuple(f0_hz.shape)))
  k, h = int(sin_amps.shape[2]), int(n_harmonics)
  if k < 1 or h < 1:
    raise ValueError('sinusoidal_to_harmonic needs at least one sinusoid and one harmonic, got {} and {}'.format(k, h))
  if k > _lib.CONSISTENCY_MAX_K or h > _lib.CONSISTENCY_MAX_K:
    raise NotImplementedError('sinusoidal_to_harmonic takes up to {} sinusoids and harmonics on the MI355X path, got {} and {}'.format(
        _lib.CONSISTENCY_MAX_K, k, h))
  args = (h, float(harmonic_width), float(sample_rate), _lib.S2H_NORMALIZE if normalize else 0)
  if _needs_grad(sin_amps, sin_freqs, f0_hz):
    return _SinusoidalToHarmonicFunction.apply(sin_amps, sin_freqs, f0_hz, args)
  return _SinusoidalToHarmonicFunction.forward(_NoCtx(), sin_amps, sin_freqs, f0_hz, args)


class _ConvertFunction(torch.autograd.Function):
  """ddsp_unit_convert_f32 with its adjoint, for the two conversions the consistency losses differentiate through."""

  @staticmethod
  def forward(ctx, x, op, p0, p1):
    ctx.save_for_backward(x)
    ctx.args = (_lib.CONVERT_OPS[op], float(p0), float(p1))
    out = torch.empty_like(x)
    if x.numel():
      rc = _lib.load().ddsp_unit_convert_f32(x.data_ptr(), out.data_ptr(), x.numel(), *ctx.args, _stream())
      _lib.check(rc, 'ddsp_unit_convert_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    x, = ctx.saved_tensors
    grad_out = tf_float32(grad_out)
    grad = torch.empty_like(x)
    if x.numel():
      rc = _lib.load().ddsp_unit_convert_backward_f32(x.data_ptr(), grad_out.data_ptr(), grad.data_ptr(), x.numel(), *ctx.args,
                                                      _stream())
      _lib.check(rc, 'ddsp_unit_convert_backward_f32')
    return grad, None, None, None


def _convert_diff(op, x, p0=0.0, p1=0.0):
  x = tf_float32(x)
  if _needs_grad(x):
    return _ConvertFunction.apply(x, op, p0, p1)
  ctx = _NoCtx()
  return _ConvertFunction.forward(ctx, x, op, p0, p1)


def _hz_to_midi_diff(frequencies):
  """hz_to_midi as losses.freq_loss needs it: differentiable (frequencies <= 0 pass no gradient).  The public
  core.hz_to_midi keeps refusing tensors that require grad."""
  return _convert_diff('hz_to_midi', frequencies)


def _log10_floor(x, amin):
  """core.log10(tf.maximum(amin, x)) (ddsp/losses.py:499-502), differentiable: the gradient reaches x where x > amin."""
  return _convert_diff('log_floor', x, math.log(10.0), amin)


class _MeanFunction(torch.autograd.Function):
  """scale * tf.reduce_mean(x) as a 0-dim tensor: fixed-order fp64 partials (ddsp_mean_f32)."""

  @staticmethod
  def forward(ctx, x, scale):
    ctx.shape, ctx.scale = x.shape, float(scale)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    if x.numel() == 0:
      return out.fill_(float('nan'))
    rc = _lib.load().ddsp_mean_f32(x.data_ptr(), out.data_ptr(), x.numel(), ctx.scale, _stream())
    _lib.check(rc, 'ddsp_mean_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    grad_out = tf_float32(grad_out).reshape(1)
    grad = torch.empty(ctx.shape, dtype=torch.float32, device=grad_out.device)
    if grad.numel():
      rc = _lib.load().ddsp_mean_backward_f32(grad_out.data_ptr(), grad.data_ptr(), grad.numel(), ctx.scale, _stream())
      _lib.check(rc, 'ddsp_mean_backward_f32')
    return grad, None


def _mean(x, scale=1.0):
  x = tf_float32(x)
  if _needs_grad(x):
    return _MeanFunction.apply(x, scale)
  return _MeanFunction.forward(_NoCtx(), x, scale)


class _RowMeanFunction(torch.autograd.Function):
  """tf.reduce_mean(x, axis=-1) (ddsp_row_mean_f32)."""

  @staticmethod
  def forward(ctx, x):
    ctx.shape = x.shape
    out = torch.empty(x.shape[:-1], dtype=torch.float32, device=x.device)
    if out.numel():
      rc = _lib.load().ddsp_row_mean_f32(x.data_ptr(), out.data_ptr(), out.numel(), x.shape[-1], _stream())
      _lib.check(rc, 'ddsp_row_mean_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    grad_out = tf_float32(grad_out)
    grad = torch.empty(ctx.shape, dtype=torch.float32, device=grad_out.device)
    if grad.numel():
      rc = _lib.load().ddsp_row_mean_backward_f32(grad_out.data_ptr(), grad.data_ptr(), grad_out.numel(), ctx.shape[-1], _stream())
      _lib.check(rc, 'ddsp_row_mean_backward_f32')
    return grad


def _row_mean(x):
  x = tf_float32(x)
  if _needs_grad(x):
    return _RowMeanFunction.apply(x)
  return _RowMeanFunction.forward(_NoCtx(), x)


# --------------------------------------------------------------------------------------
# the rest of ddsp/core.py: psychoacoustic scales, soft_limit / log_scale / sym_exp_sigmoid, critical bands, harmonic
# wavetables (csrc/scale_fns.hip, critical_bands.hip, harmonic_wavetable.hip) and host plumbing
# --------------------------------------------------------------------------------------
class _ScaleFunction(torch.autograd.Function):
  """ddsp_scale_convert_f32 with its adjoint (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, x, op, p0, p1):
    ctx.save_for_backward(x)
    ctx.args = (_lib.SCALE_OPS[op], float(p0), float(p1))
    out = torch.empty_like(x)
    if x.numel():
      rc = _lib.load().ddsp_scale_convert_f32(x.data_ptr(), out.data_ptr(), x.numel(), *ctx.args, _stream())
      _lib.check(rc, 'ddsp_scale_convert_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    x, = ctx.saved_tensors
    grad_out = tf_float32(grad_out)
    grad = torch.empty_like(x)
    if x.numel():
      rc = _lib.load().ddsp_scale_convert_backward_f32(x.data_ptr(), grad_out.data_ptr(), grad.data_ptr(), x.numel(), *ctx.args,
                                                       _stream())
      _lib.check(rc, 'ddsp_scale_convert_backward_f32')
    return grad, None, None, None


def _scale(op, x, p0=0.0, p1=0.0):
  x = tf_float32(x)
  if _needs_grad(x):
    return _ScaleFunction.apply(x, op, p0, p1)
  return _ScaleFunction.forward(_NoCtx(), x, op, p0, p1)


def hz_to_bark(hz):
  """core.hz_to_bark (ddsp/core.py:351-353): 26.81 / (1 + 1960 / hz) - 0.53 (Traunmuller 1990); hz_to_bark(0) = -0.53."""
  return _scale('hz_to_bark', hz)


def bark_to_hz(bark):
  """core.bark_to_hz (ddsp/core.py:356-358): 1960 / (26.81 / (bark + 0.53) - 1); bark_to_hz(-0.53) = 0."""
  return _scale('bark_to_hz', bark)


def hz_to_mel(hz):
  """core.hz_to_mel (ddsp/core.py:361-363): 2595 logb(1 + hz / 700, 10), with logb's safe logarithm."""
  return _scale('hz_to_mel', hz)


def mel_to_hz(mel):
  """core.mel_to_hz (ddsp/core.py:366-368): 700 (10^(mel / 2595) - 1)."""
  return _scale('mel_to_hz', mel)


def hz_to_erb(hz):
  """core.hz_to_erb (ddsp/core.py:371-382): equivalent rectangular bandwidths, 0.108 hz + 24.7 (Moore & Glasberg 1996)."""
  return _scale('hz_to_erb', hz)


def soft_limit(x, x_min=0.0, x_max=1.0):
  """core.soft_limit (ddsp/core.py:236-238): softplus(x) + x_min - softplus(x - (x_max - x_min)).  As in the reference a
  value well inside the range comes out as x + x_min."""
  return _scale('soft_limit', x, x_min, x_max)


def log_scale(x, min_x, max_x):
  """core.log_scale (ddsp/core.py:229-233): [-1, 1] logarithmically to [min_x, max_x] (the bounds are positive numbers)."""
  if not (float(min_x) > 0.0 and float(max_x) > 0.0):
    raise ValueError('log_scale needs positive bounds, got min_x={} and max_x={}'.format(min_x, max_x))
  return _scale('log_scale', x, min_x, max_x)


def sym_exp_sigmoid(x, width=8.0):
  """core.sym_exp_sigmoid (ddsp/core.py:407-411): exp_sigmoid(width (|x| / 2 - 1)); the gradient at x = 0 is 0, as tf.abs has it."""
  return _scale('sym_exp_sigmoid', x, width)


def nan_to_num(x, value=0.0):
  """core.nan_to_num (ddsp/core.py:202-204): NaNs replaced by `value`; the gradient passes where x is not NaN."""
  return _scale('nan_to_num', x, value)


def log10(x, eps=1e-5):
  """core.log10 (ddsp/core.py:224-226): logb(x, 10, eps).  Forward only, like logb."""
  return logb(x, base=10.0, eps=eps)


class _GradientReversalFunction(torch.autograd.Function):
  @staticmethod
  def forward(ctx, x):
    return x.view_as(x)

  @staticmethod
  def backward(ctx, grad_out):
    return -grad_out


def gradient_reversal(x):
  """core.gradient_reversal (ddsp/core.py:241-243): the identity forward, the gradient negated."""
  x = tf_float32(x)
  return _GradientReversalFunction.apply(x) if _needs_grad(x) else x


# ---- frequencies_critical_bands  (ddsp/core.py:510-569) ----
def _np_hz_to_bark(hz):
  return 26.81 / (1.0 + (1960.0 / hz)) - 0.53


def _np_bark_to_hz(bark):
  return 1960.0 / (26.81 / (bark + 0.53) - 1.0)


def _np_hz_to_mel(hz):
  return 2595.0 * (np.log(np.where(1.0 + hz / 700.0 <= 0.0, 1e-5, 1.0 + hz / 700.0)) / np.log(10.0))


def _np_mel_to_hz(mel):
  return 700.0 * (10.0**(mel / 2595.0) - 1.0)


def critical_band_tables(n_sinusoids, depth=1, depth_scale=10.0, hz_min=20.0, hz_max=8000.0, scale='bark'):
  """The constants of frequencies_critical_bands as float32 arrays: (f_center [n_sinusoids], bandwidths [n_sinusoids],
  depth_modifier [depth]).  The centres lie evenly on the bark scale (scale == 'bark') or the mel scale (any other string,
  as in the reference) between hz_min and hz_max, the bandwidths are their ERBs; both are made in float64 and rounded once.
  depth_modifier = depth_scale^-d in float32, as tf.range(depth, dtype=float32) makes it."""
  with np.errstate(divide='ignore', over='ignore', under='ignore'):
    if scale == 'bark':
      grid = np.linspace(_np_hz_to_bark(np.float64(hz_min)), _np_hz_to_bark(np.float64(hz_max)), int(n_sinusoids))
      f_center = _np_bark_to_hz(grid)
    else:
      grid = np.linspace(_np_hz_to_mel(np.float64(hz_min)), _np_hz_to_mel(np.float64(hz_max)), int(n_sinusoids))
      f_center = _np_mel_to_hz(grid)
    bandwidths = 0.108 * f_center + 24.7
    depth_modifier = np.power(np.float32(depth_scale), -np.arange(int(depth), dtype=np.float32)).astype(np.float32)
  return f_center.astype(np.float32), bandwidths.astype(np.float32), depth_modifier


_critical_band_cache = {}


def _critical_band_device_tables(key, device):
  """critical_band_tables(*key) on `device`, made once per argument tuple and device."""
  ck = key + (str(device),)
  tables = _critical_band_cache.get(ck)
  if tables is None:
    tables = tuple(torch.as_tensor(t, device=device).contiguous() for t in critical_band_tables(*key))
    _critical_band_cache[ck] = tables
  return tables


class _CriticalBandsFunction(torch.autograd.Function):
  """torch.autograd node of core.frequencies_critical_bands (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, freqs, tables, k, depth, bandwidth_scale, hz_min, hz_max):
    ctx.save_for_backward(freqs)
    ctx.args = (k, depth) + tuple(t.data_ptr() for t in tables) + (bandwidth_scale, hz_min, hz_max)
    ctx.tables = tables
    b, t, _ = freqs.shape
    out = torch.empty((b, t, k), dtype=torch.float32, device=freqs.device)
    if out.numel():
      rc = _lib.load().ddsp_critical_bands_f32(freqs.data_ptr(), out.data_ptr(), b * t, *ctx.args, _stream())
      _lib.check(rc, 'ddsp_critical_bands_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    freqs, = ctx.saved_tensors
    b, t, _ = freqs.shape
    grad_out = tf_float32(grad_out)
    grad = torch.empty_like(freqs)
    if grad.numel():
      rc = _lib.load().ddsp_critical_bands_backward_f32(freqs.data_ptr(), grad_out.data_ptr(), grad.data_ptr(), b * t, *ctx.args,
                                                        _stream())
      _lib.check(rc, 'ddsp_critical_bands_backward_f32')
    return grad, None, None, None, None, None, None


def frequencies_critical_bands(freqs, depth=1, depth_scale=10.0, bandwidth_scale=1.0, hz_min=20.0, hz_max=8000.0, scale='bark'):
  """core.frequencies_critical_bands (ddsp/core.py:510-569): centre frequencies evenly spaced on the bark (scale='bark') or mel
  (any other string) scale between hz_min and hz_max, each moved within bandwidth_scale ERBs of its centre by
  sum_d tanh(freqs[..., d]) depth_scale^-d and passed through soft_limit(hz_min, hz_max).  freqs [batch, time,
  n_sinusoids * depth] or [batch, time, n_sinusoids, depth] -> [batch, time, n_sinusoids].  One kernel per direction with
  coalesced loads at every depth (csrc/critical_bands.hip); differentiable; any depth >= 1."""
  raw = tf_float32(freqs)
  flat, k, depth = _depth_layout(raw, depth)
  tables = _critical_band_device_tables((k, depth, float(depth_scale), float(hz_min), float(hz_max), 'bark' if scale == 'bark' else 'mel'),
                                        flat.device)
  args = (flat, tables, k, depth, float(bandwidth_scale), float(hz_min), float(hz_max))
  if _needs_grad(raw):
    return _CriticalBandsFunction.apply(*args)
  return _CriticalBandsFunction.forward(_NoCtx(), *args)


# ---- harmonic_distribution_to_wavetable  (ddsp/core.py:1217-1235) ----
def harmonic_wavetable_length(n_harmonics, n_wavetable):
  """Points of the table harmonic_distribution_to_wavetable returns: 2 (n_harmonics + int(n_wavetable / 2 - n_harmonics)),
  which is n_wavetable when that is even and n_wavetable - 1 when it is odd.  ValueError where the reference's tf.pad
  fails on a negative padding (more harmonics than n_wavetable / 2)."""
  n_pad = int(n_wavetable / 2 - n_harmonics)
  if n_harmonics < 1 or n_pad < 0 or n_wavetable / 2 - n_harmonics < 0:
    raise ValueError('harmonic_distribution_to_wavetable: {} harmonics do not fit a wavetable of {} points (at most '
                     'n_wavetable / 2)'.format(n_harmonics, n_wavetable))
  return 2 * (int(n_harmonics) + n_pad)


def _harmonic_wavetable_fused(length):
  lo, hi = _lib.HARMONIC_WAVETABLE_SIZES
  return lo <= length <= hi and length & (length - 1) == 0


class _HarmonicWavetableFunction(torch.autograd.Function):
  """torch.autograd node of core.harmonic_distribution_to_wavetable on the fused kernel (both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, hd, length, scale):
    ctx.args = (int(hd.shape[-1]), length, scale)
    rows = hd.numel() // hd.shape[-1]
    out = torch.empty(tuple(hd.shape[:-1]) + (length,), dtype=torch.float32, device=hd.device)
    if rows:
      rc = _lib.load().ddsp_harmonic_wavetable_f32(hd.data_ptr(), out.data_ptr(), rows, *ctx.args, _stream())
      _lib.check(rc, 'ddsp_harmonic_wavetable_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    k, length, scale = ctx.args
    grad_out = tf_float32(grad_out)
    grad = torch.empty(tuple(grad_out.shape[:-1]) + (k,), dtype=torch.float32, device=grad_out.device)
    if grad.numel():
      rc = _lib.load().ddsp_harmonic_wavetable_backward_f32(grad_out.data_ptr(), grad.data_ptr(), grad.numel() // k, k, length, scale,
                                                            _stream())
      _lib.check(rc, 'ddsp_harmonic_wavetable_backward_f32')
    return grad, None, None


def harmonic_distribution_to_wavetable(harmonic_distribution, n_wavetable=2048):
  """core.harmonic_distribution_to_wavetable (ddsp/core.py:1217-1235): [batch, time, n_harmonics] -> wavetables
  [batch, time, L] for core.wavetable_synthesis / synths.Wavetable, L = harmonic_wavetable_length(n_harmonics, n_wavetable):
  table[n] = (n_wavetable / L) sum_k w_k hd[k - 1] cos(2 pi k n / L), the reference's pad -> irfft -> scale.

  L a power of two from 64 to 8192 runs one fused kernel per direction (csrc/harmonic_wavetable.hip); any other length -
  an odd n_wavetable gives L = n_wavetable - 1 - takes the reference's own chain with torch.fft.irfft.  Differentiable."""
  hd = tf_float32(harmonic_distribution)
  if hd.dim() < 1:
    raise ValueError('harmonic_distribution must be [..., n_harmonics], got a scalar')
  k = int(hd.shape[-1])
  length = harmonic_wavetable_length(k, n_wavetable)
  if not _harmonic_wavetable_fused(length):
    fft_in = torch.nn.functional.pad(hd, (1, length // 2 - k))
    return torch.fft.irfft(torch.complex(fft_in, torch.zeros_like(fft_in)), n=length) * (n_wavetable / 2)
  scale = float(n_wavetable) / float(length)
  if _needs_grad(hd):
    return _HarmonicWavetableFunction.apply(hd, length, scale)
  return _HarmonicWavetableFunction.forward(_NoCtx(), hd, length, scale)


# ---- host plumbing  (ddsp/core.py:64-75, 132-168, 717-729) ----
def copy_if_tf_function(x):
  """core.copy_if_tf_function (ddsp/core.py:64-75): the reference copies inside a tf.function; there is none here."""
  return x


def leaf_key(nested_key, delimiter='/'):
  """Returns the leaf node key name of "key/key/key" (ddsp/core.py:132-145)."""
  return nested_key.split(delimiter)[-1]


def map_shape(x):
  """Recursively infer tensor shapes for a (nested) dictionary of tensors, as lists of ints (ddsp/core.py:148-150)."""
  if isinstance(x, dict):
    return {k: map_shape(v) for k, v in x.items()}
  if isinstance(x, (list, tuple)):
    return type(x)(map_shape(v) for v in x)
  return [int(d) for d in np.shape(x)] if not isinstance(x, torch.Tensor) else [int(d) for d in x.shape]


def pad_axis(x, padding=(0, 0), axis=0, **pad_kwargs):
  """core.pad_axis (ddsp/core.py:153-168): pads one axis of a tensor by (before, after).  pad_kwargs are tf.pad's `mode`
  ('CONSTANT', 'REFLECT', 'SYMMETRIC') and `constant_values`, as spectral_ops.pad takes them.  Host plumbing (torch)."""
  x = tf_float32(x)
  mode = str(pad_kwargs.pop('mode', 'CONSTANT')).upper()
  constant_values = pad_kwargs.pop('constant_values', 0)
  if pad_kwargs:
    raise TypeError('pad_axis got unexpected keyword arguments {}'.format(sorted(pad_kwargs)))
  before, after = (int(p) for p in padding)
  if before < 0 or after < 0:
    raise ValueError('Paddings must be non-negative, got {}'.format(tuple(padding)))
  if x.dim() == 0 or not -x.dim() <= axis < x.dim():
    raise ValueError('Invalid axis index: %d for tensor with only %d axes.' % (axis, x.dim()))
  n = int(x.shape[axis])
  x = x.movedim(axis, -1)
  if mode == 'CONSTANT':
    out = torch.nn.functional.pad(x, (before, after), value=float(constant_values))
  elif mode in ('REFLECT', 'SYMMETRIC'):
    skip = 1 if mode == 'REFLECT' else 0
    if max(before, after) + skip > n:
      raise ValueError('{} padding of {} needs at least {} samples, got {}'.format(mode, max(before, after),
                                                                                 max(before, after) + skip, n))
    left = x[..., skip:skip + before].flip(-1)
    right = x[..., n - skip - after:n - skip].flip(-1)
    out = torch.cat([left, x, right], dim=-1)
  else:
    raise ValueError('`mode` must be one of CONSTANT, REFLECT, SYMMETRIC, received ({}).'.format(mode))
  return out.movedim(-1, axis).contiguous()


def center_crop(audio, frame_size):
  """core.center_crop (ddsp/core.py:717-729): removes the padding of centred frames, audio[:, p:-p] with p = frame_size // 2
  (python slice semantics included: p = 0 leaves nothing, as in the reference)."""
  pad_amount = int(frame_size // 2)
  return audio[:, pad_amount:-pad_amount]
