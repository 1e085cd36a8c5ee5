"""Losses: the multi-scale spectrogram loss (mirror of ddsp/losses.py:41-48, 102-128, 131-243).

SURVEY.md section 8(f) rank 2.  What `gin/models/ae.gin:36-41` uses - loss_type 'L1' with the magnitude and
log-magnitude terms - runs fused kernels whose spectra never leave LDS (csrc/spectral_loss.hip).  The rest of the
reference's argument space - delta_time / delta_freq / cumsum_freq terms, 'L2' and 'COSINE', the `weights` mask -
runs on spectrograms materialised in HBM, one FFT size at a time (csrc/spectral_terms.hip); the loudness term
(spectral_ops.compute_loudness, spectral_ops.py:253-324) likewise, under its own frame geometry.  `mean_difference` is the
reference's public function on the same kernels.
The call is a torch.autograd node: the gradient reaches `audio` (not `target_audio`, as a training step needs it).
"""
import ctypes

import numpy as np
import torch

from ddsp_amd import _lib
from ddsp_amd import core
from ddsp_amd import dags


def a_weighting_linear(sample_rate, n_fft):
  """10 ** (A_weighting / 10) at the bins of an n_fft-point transform: the A-curve librosa publishes (IEC 61672; clipped at -80 dB,
  f = 0) - what spectral_ops.compute_loudness multiplies the power by (spectral_ops.py:307-312).  A constant table made on the
  host in double precision, as every constant table of this library (oracle/ddsp_oracle.py::a_weighting_db restates the same
  formula for the tests)."""
  f_sq = (np.arange(n_fft // 2 + 1, dtype=np.float64) * (sample_rate / n_fft)) ** 2
  c = np.array([12194.217, 20.598997, 107.65265, 737.86223]) ** 2.0
  with np.errstate(divide='ignore'):
    db = 2.0 + 20.0 * (np.log10(c[0]) + 2 * np.log10(f_sq) - np.log10(f_sq + c[0]) - np.log10(f_sq + c[1])
                       - 0.5 * np.log10(f_sq + c[2]) - 0.5 * np.log10(f_sq + c[3]))
  return (10.0 ** (np.maximum(-80.0, db) / 10.0)).astype(np.float32)


class Loss:
  """Base class. Duck typing: losses just must implement get_losses_dict() (losses.py:41-48)."""

  def __init__(self, name):
    self.name = name

  def __call__(self, *args, **kwargs):
    return self.call(*args, **kwargs)

  def get_losses_dict(self, *args, **kwargs):
    """Returns a dictionary of losses for the model."""
    loss = self(*args, **kwargs)
    return {self.name: loss}


class LossGroup(dags.DAGLayer):
  """Compute a group of loss layers on an outputs dictionary (ddsp/losses.py:51-97): a DAG of `(loss, [input key, ...])` nodes
  -> one flat dictionary {loss name: scalar}."""

  def __init__(self, dag, **kwarg_losses):
    super().__init__(dag, **kwarg_losses)
    self.loss_names = self.module_names

  @property
  def losses(self):
    return [getattr(self, name) for name in self.loss_names]

  def call(self, outputs, **kwargs):
    dag_outputs = super().call(outputs, **kwargs)
    loss_outputs = {}
    for k in self.loss_names:
      loss_outputs.update(dag_outputs[k])
    return loss_outputs

  def get_losses_dict(self, outputs, **kwargs):
    return self(outputs, **kwargs)


_MD_MAX_LAST = 4097                    # kStMaxBins of csrc/spectral_terms.hip: the longest row a block of the term kernels holds
_md_ws = core.Workspace()


def _md_view(shape):
  """Any shape -> the [batch, rows, last axis] view the term kernels take (the last axis is what 'COSINE' reduces)."""
  shape = tuple(int(v) for v in shape)
  if len(shape) == 0:
    return 1, 1, 1
  if len(shape) == 1:
    return 1, 1, shape[0]
  rows = 1
  for v in shape[1:-1]:
    rows *= v
  return shape[0], rows, shape[-1]


def _md_raw(target, value, loss_type, weights, want_grad):
  """One call of ddsp_spectral_terms_f32 with the magnitude term alone: (loss, d loss / d value or None)."""
  dev = value.device
  loss = torch.empty((), dtype=torch.float32, device=dev)
  if value.numel() == 0:
    # tf.reduce_mean over no elements is NaN; cosine_distance's weighted mean divides safely: 0 (losses.py:118-124)
    loss.fill_(0.0 if loss_type == 'COSINE' else float('nan'))
    return loss, (torch.zeros_like(value) if want_grad else None)
  b, f, k = _md_view(value.shape)
  w = None
  if weights is not None:
    w = core.tf_float32(weights if isinstance(weights, torch.Tensor) else torch.as_tensor(weights, dtype=torch.float32))
    core.require_no_grad('mean_difference weights', w)
    if w.numel() == 1:
      w = w.reshape(1, 1, 1).contiguous()
    else:
      # `difference * weights` ('L1' / 'L2') or weights against [..., 1] ('COSINE'): materialised at the shape it multiplies
      full = tuple(value.shape[:-1]) + (1,) if loss_type == 'COSINE' else tuple(value.shape)
      if w.dim() > len(full):
        raise ValueError('weights of shape {} do not broadcast against {}'.format(tuple(w.shape), full))
      try:
        w = w.expand(full).contiguous()
      except RuntimeError:
        raise ValueError('weights of shape {} do not broadcast against {}'.format(tuple(w.shape), full))
      w = w.reshape(b, f, 1 if loss_type == 'COSINE' else k)
  if k > _MD_MAX_LAST:
    if loss_type == 'COSINE':
      raise NotImplementedError('mean_difference(COSINE) along an axis of more than {} elements is not built on the MI355X '
                                'path (got {})'.format(_MD_MAX_LAST, k))
    # 'L1' / 'L2' are means over every element: any factorisation of the element count serves (the mask, materialised, with it)
    total = b * f * k
    cols = next(c for c in range(4096, 0, -1) if total % c == 0)
    b, f, k = 1, total // cols, cols
    if w is not None and w.numel() != 1:
      w = w.reshape(b, f, k)
  acc = torch.empty((), dtype=torch.float64, device=dev)
  grad = torch.empty_like(value) if want_grad else None
  ws = _md_ws.get(core.cached_workspace_bytes('ddsp_spectral_terms_workspace_bytes', b, f), dev)
  wb, wf, wk = (int(v) for v in w.shape) if w is not None else (0, 0, 0)
  rc = _lib.load().ddsp_spectral_terms_f32(
      target.data_ptr(), value.data_ptr(), w.data_ptr() if w is not None else None, wb, wf, wk,
      grad.data_ptr() if want_grad else None, acc.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(), b, f, k,
      _lib.LOSS_TYPES[loss_type], 1.0, 0.0, 0.0, 0.0, 0.0, 1, core._stream())
  _lib.check(rc, 'ddsp_spectral_terms_f32')
  return loss, grad


class _MeanDifferenceFunction(torch.autograd.Function):
  """torch.autograd node of mean_difference.  Every loss type is symmetric in its two arguments, so d / d target is d / d value
  of the call with the arguments exchanged."""

  @staticmethod
  def forward(ctx, target, value, loss_type, weights):
    loss, grad_value = _md_raw(target, value, loss_type, weights, ctx.needs_input_grad[1])
    grad_target = _md_raw(value, target, loss_type, weights, True)[1] if ctx.needs_input_grad[0] else None
    ctx.has = (grad_target is not None, grad_value is not None)
    ctx.save_for_backward(*[g for g in (grad_target, grad_value) if g is not None])
    return loss

  @staticmethod
  def backward(ctx, grad_loss):
    saved = list(ctx.saved_tensors)
    grad_target = _scale(saved.pop(0), grad_loss) if ctx.has[0] else None
    grad_value = _scale(saved.pop(0), grad_loss) if ctx.has[1] else None
    return grad_target, grad_value, None, None


def mean_difference(target, value, loss_type='L1', weights=None):
  """Common loss functions (ddsp/losses.py:102-128): the mean of |difference * weights| ('L1') or difference**2 * weights ('L2'),
  or tf.losses.cosine_distance along the last axis ('COSINE') - on the kernels SpectralLoss's general form runs its terms on
  (ddsp_spectral_terms_f32: fixed-order fp64 sums), differentiable in `target` and `value`.

  Raises:
    ValueError: If loss_type is not an allowed value.
  """
  loss_type = loss_type.upper()
  if loss_type not in _lib.LOSS_TYPES:
    raise ValueError('Loss type ({}), must be '
                     '"L1", "L2", or "COSINE"'.format(loss_type))
  target, value = core.tf_float32(target), core.tf_float32(value)
  if target.shape != value.shape:
    core.require_no_grad('mean_difference of tensors that broadcast against each other', target, value)
    target, value = torch.broadcast_tensors(target, value)
  target, value = target.contiguous(), value.contiguous()
  if torch.is_grad_enabled() and (target.requires_grad or value.requires_grad):
    return _MeanDifferenceFunction.apply(target, value, loss_type, weights)
  return _md_raw(target, value, loss_type, weights, False)[0]


class _TakesDeterministic(type):
  """SpectralLoss.__init__ keeps the parameter list of the reference's constructor (ddsp/losses.py:140-187; tests/test_host_api.py
  holds it to that list).  `deterministic` is this library's own, so it is not one of them: the class takes it, by keyword only,
  when it is called - SpectralLoss(..., deterministic=True) - checks it there and sets it on the new instance."""

  def __call__(cls, *args, deterministic=None, **kwargs):
    if not (deterministic is None or isinstance(deterministic, bool)):
      raise ValueError('deterministic must be True, False or None, got {!r}'.format(deterministic))
    loss = super().__call__(*args, **kwargs)
    loss.deterministic = deterministic
    return loss


class SpectralLoss(Loss, metaclass=_TakesDeterministic):
  """Multi-scale spectrogram loss (ddsp/losses.py:131-243).

  deterministic: how dL/d audio adds its overlapping frames.  False: fp32 atomics (the last bits depend on the order the blocks
  arrive in).  True: every block stores its stretch to a slab of its own and a second kernel adds each sample's few slabs in a
  fixed order - the scales in the order of `fft_sizes`, within a scale the covering blocks in ascending order, the loudness term
  last: the same bits run to run, and a row's gradient does not depend on the other rows' data.  Costs a second workspace
  (74 MB at batch 32 x 64 000 samples with the default sizes).  None (the default): True exactly when
  torch.are_deterministic_algorithms_enabled() at the time of the call.  The loss VALUE is the same bits either way.
  A keyword of the call SpectralLoss(..., deterministic=...) only (any other value: ValueError), and a plain attribute afterwards."""

  def __init__(self,
               fft_sizes=(2048, 1024, 512, 256, 128, 64),
               loss_type='L1',
               mag_weight=1.0,
               delta_time_weight=0.0,
               delta_freq_weight=0.0,
               cumsum_freq_weight=0.0,
               logmag_weight=0.0,
               loudness_weight=0.0,
               name='spectral_loss'):
    super().__init__(name=name)
    self.deterministic = None                # (set by the call of the class: _TakesDeterministic)
    self._grad_ws = core.Workspace()         # the slabs of the deterministic gradient (per device and stream, as _ws)
    self.fft_sizes = fft_sizes
    self.loss_type = loss_type
    self.mag_weight = mag_weight
    self.delta_time_weight = delta_time_weight
    self.delta_freq_weight = delta_freq_weight
    self.cumsum_freq_weight = cumsum_freq_weight
    self.logmag_weight = logmag_weight
    self.loudness_weight = loudness_weight
    self._ws = core.Workspace()

  def call(self, target_audio, audio, weights=None):
    """Scalar loss (0-dim tensor in HBM) between two batches of audio [batch, n_samples(, 1)]."""
    if self.loss_type.upper() not in ('L1', 'L2', 'COSINE'):
      # losses.mean_difference (losses.py:102-128) raises when it is CALLED: a loss whose every weight is zero never calls it
      if max(self.mag_weight, self.delta_time_weight, self.delta_freq_weight, self.cumsum_freq_weight, self.logmag_weight,
             self.loudness_weight) > 0:
        raise ValueError('Loss type ({}), must be '
                         '"L1", "L2", or "COSINE"'.format(self.loss_type.upper()))
      return torch.zeros((), dtype=torch.float32, device=core._device())
    target_audio, audio = core.tf_float32(target_audio), core.tf_float32(audio)
    if target_audio.dim() == 3:
      target_audio = target_audio[..., 0].contiguous()
    if audio.dim() == 3:
      audio = audio[..., 0].contiguous()
    if target_audio.dim() != 2 or target_audio.shape != audio.shape:
      raise ValueError('target_audio and audio must both be [batch, n_samples], got {} and {}'.format(
          tuple(target_audio.shape), tuple(audio.shape)))
    plain_terms = (self.loss_type.upper() != 'L1' or weights is not None or self.delta_time_weight > 0 or
                   self.delta_freq_weight > 0 or self.cumsum_freq_weight > 0 or self.loudness_weight > 0)
    # frame sizes the fused 'L1' kernels take: 2^k in [16, 8192] and, since round 6, 3 * 2^k in [48, 6144] (vst_48k.gin:56 asks for
    # 6144, 3072 .. 192; 8192-point transforms one frame and one signal at a time: stft_l1_big_kernel); any other even size on the
    # plain kernels
    others = [v for v in self.fft_sizes if not self._fused_size(v)]
    if not plain_terms and others and len(others) < len(self.fft_sizes):
      # the loss is a sum over its scales (losses.py:199-236): the fused kernels for the scales they take, the plain ones for the rest
      fused_part, plain_part = self._split_by_kernel(others)
      return fused_part.call(target_audio, audio) + plain_part.call(target_audio, audio)
    general = plain_terms or bool(others)
    if general:
      weights = self._weights_tensor(weights, audio.device)
      if torch.is_grad_enabled() and audio.requires_grad:
        return _SpectralLossGeneralFunction.apply(target_audio.detach(), audio, self, weights)
      return self._general(target_audio, audio, weights, want_grad=False)[0]
    if torch.is_grad_enabled() and audio.requires_grad:
      return _SpectralLossFunction.apply(target_audio.detach(), audio, self)
    return self._forward(target_audio, audio)

  def _slabs(self):
    """Whether this call takes the reproducible gradient (the slab kernels + the gather)."""
    if self.deterministic is None:
      return bool(torch.are_deterministic_algorithms_enabled())
    return bool(self.deterministic)

  @staticmethod
  def _fused_size(v):
    v = int(v)
    return (16 <= v <= 8192 and not v & (v - 1)) or (48 <= v <= 6144 and v % 3 == 0 and not (v // 3) & (v // 3 - 1))

  def _split_by_kernel(self, others):
    key = tuple(int(v) for v in self.fft_sizes)
    if getattr(self, '_split_key', None) != key:
      kw = dict(loss_type=self.loss_type, mag_weight=self.mag_weight, logmag_weight=self.logmag_weight)
      self._split_parts = (SpectralLoss(fft_sizes=tuple(v for v in self.fft_sizes if v not in others), **kw),
                           SpectralLoss(fft_sizes=tuple(others), **kw))
      self._split_key = key
    for part in self._split_parts:           # (the weights are plain attributes a caller may change between calls)
      part.mag_weight, part.logmag_weight = self.mag_weight, self.logmag_weight
      part.deterministic = self.deterministic
    return self._split_parts

  @staticmethod
  def _weights_tensor(weights, device):
    """`weights` of losses.mean_difference: None, a number, or a mask of rank <= 3 -> None or a [b, f, k] tensor."""
    if weights is None:
      return None
    w = core.tf_float32(weights if isinstance(weights, torch.Tensor) else torch.as_tensor(weights, dtype=torch.float32))
    core.require_no_grad('SpectralLoss weights', w)
    if w.dim() > 3:
      raise ValueError('weights must broadcast against [batch, frames, bins], got shape {}'.format(tuple(w.shape)))
    return w.reshape((1,) * (3 - w.dim()) + tuple(w.shape)).contiguous()

  def _general(self, target_audio, audio, weights, want_grad):
    """The reference's loop over FFT sizes (losses.py:199-236) on materialised spectrograms -> (loss, grad_audio)."""
    b, n = audio.shape
    lib = _lib.load()
    dev = audio.device
    loss_type = _lib.LOSS_TYPES[self.loss_type.upper()]
    term_w = [float(self.mag_weight), float(self.delta_time_weight), float(self.delta_freq_weight),
              float(self.cumsum_freq_weight), float(self.logmag_weight)]
    loss = torch.empty((), dtype=torch.float32, device=dev)
    acc = torch.empty((), dtype=torch.float64, device=dev)
    grad_audio = torch.zeros_like(audio) if want_grad else None
    if not self.fft_sizes and not self.loudness_weight > 0:
      loss.zero_()
      return loss, grad_audio
    for z, size in enumerate(self.fft_sizes):
      size = int(size)
      pow2 = 16 <= size <= 4096 and not size & (size - 1)
      other = (34 <= size <= 8190 and size % 2 == 0 and size & (size - 1)) or size == 8192       # (vst_48k.gin: 6144, 3072 .. 192; any since round 6)
      if not (pow2 or other):
        raise ValueError('fft_sizes must be powers of two in [16, 8192] or even sizes in [34, 8190] on the MI355X path (odd frames, '
                         'and frames of fewer than 34 samples that are not powers of two, are not built), got {}'.format(
                             tuple(self.fft_sizes)))
      # spectral_ops.stft (spectral_ops.py:40-45): tf.signal.stft with fft_length=None transforms the ENCLOSING power of two
      frames, bins = -(-n // (size // 4)), (1 << (size - 1).bit_length()) // 2 + 1
      wb = wf = wk = 0
      if weights is not None:
        wb, wf, wk = (int(v) for v in weights.shape)
        # the mask must broadcast against every term it meets, as `difference * weights` does in the reference
        dims = [(frames, bins)] * 5
        dims[1], dims[2] = (frames - 1, bins), (frames, bins - 1)
        for on, (tf_, tk) in zip(term_w, dims):
          if on > 0 and (wb not in (1, b) or wf not in (1, tf_) or wk not in (1, tk)):
            raise ValueError('weights of shape {} do not broadcast against a term of shape {}'.format(
                tuple(weights.shape), (b, tf_, tk)))
        if loss_type == _lib.LOSS_TYPES['COSINE'] and wk != 1:
          raise ValueError('COSINE weights must broadcast against [batch, frames, 1], got {}'.format(tuple(weights.shape)))
      target_mag = torch.empty((b, frames, bins), dtype=torch.float32, device=dev)
      mag = torch.empty_like(target_mag)
      rc = lib.ddsp_stft_mag_f32(target_audio.data_ptr(), audio.data_ptr(), target_mag.data_ptr(), mag.data_ptr(), b, n,
                                 size, core._stream())
      _lib.check(rc, 'ddsp_stft_mag_f32')
      cot = torch.empty_like(mag) if want_grad else None
      ws = self._ws.get(core.cached_workspace_bytes('ddsp_spectral_terms_workspace_bytes', b, frames), dev)
      rc = lib.ddsp_spectral_terms_f32(
          target_mag.data_ptr(), mag.data_ptr(), weights.data_ptr() if weights is not None else None, wb, wf, wk,
          cot.data_ptr() if want_grad else None, acc.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(), b, frames,
          bins, loss_type, *term_w, 1 if z == 0 else 0, core._stream())
      _lib.check(rc, 'ddsp_spectral_terms_f32')
      if want_grad and self._slabs():
        slabs = self._grad_ws.get(core.cached_workspace_bytes('ddsp_stft_mag_backward_workspace_bytes', b, n, size), dev)
        rc = lib.ddsp_stft_mag_backward_det_f32(audio.data_ptr(), cot.data_ptr(), grad_audio.data_ptr(), slabs.data_ptr(),
                                                slabs.numel(), b, n, size, core._stream())
        _lib.check(rc, 'ddsp_stft_mag_backward_det_f32')
      elif want_grad:
        rc = lib.ddsp_stft_mag_backward_f32(audio.data_ptr(), cot.data_ptr(), grad_audio.data_ptr(), b, n, size,
                                            core._stream())
        _lib.check(rc, 'ddsp_stft_mag_backward_f32')
    if self.loudness_weight > 0:
      self._loudness_term(target_audio, audio, weights, loss, acc, grad_audio, first=not self.fft_sizes)
    if (self.delta_time_weight > 0 and self.loss_type.upper() in ('L1', 'L2') and
        any(-(-n // (int(size) // 4)) < 2 for size in self.fft_sizes)):
      # a clip of ONE frame at some size: the reference's delta-time term is the mean of an empty difference - NaN
      # (tf.reduce_mean over no elements, losses.py:102-128, 213-216), and so is the loss it returns.  ('COSINE' goes through
      # tf.compat.v1.losses.cosine_distance, whose weighted mean divides safely: 0 for no elements - what the kernel adds.)
      loss.fill_(float('nan'))
    return loss, grad_audio

  # spectral_ops.compute_loudness as SpectralLoss calls it (losses.py:238-242: n_fft = 2048, everything else the defaults of
  # spectral_ops.py:253-260: 16 kHz, 250 frames a second, 80 dB of range, reference 0 dB, centre padding)
  LOUDNESS_N_FFT, LOUDNESS_SAMPLE_RATE, LOUDNESS_FRAME_RATE, LOUDNESS_RANGE_DB, LOUDNESS_REF_DB = 2048, 16000, 250, 80.0, 0.0
  _a_weighting = {}

  @classmethod
  def _loudness_weighting(cls, device):
    key = str(device)
    if key not in cls._a_weighting:
      cls._a_weighting[key] = torch.as_tensor(a_weighting_linear(cls.LOUDNESS_SAMPLE_RATE, cls.LOUDNESS_N_FFT), device=device)
    return cls._a_weighting[key]

  def _loudness_term(self, target_audio, audio, weights, loss, acc, grad_audio, first):
    """loss += loudness_weight * mean_difference(compute_loudness(target), compute_loudness(audio)) (losses.py:238-242) and, if
    grad_audio is given, its gradient: |STFT| under compute_loudness's frames (ddsp_stft_frames_mag_f32), the A-weighted mean power
    in dB per frame (ddsp_loudness_from_mag_f32), the difference term on [batch, 1, frames] (ddsp_spectral_terms_f32), and back."""
    b, n = audio.shape
    lib = _lib.load()
    dev = audio.device
    n_fft = self.LOUDNESS_N_FFT
    hop = self.LOUDNESS_SAMPLE_RATE // self.LOUDNESS_FRAME_RATE
    frames, bins = 1 + n // hop, n_fft // 2 + 1
    wt = self._loudness_weighting(dev)
    loud, mags = [], []
    for x in (target_audio, audio):
      mag = torch.empty((b, frames, bins), dtype=torch.float32, device=dev)
      _lib.check(lib.ddsp_stft_frames_mag_f32(x.data_ptr(), mag.data_ptr(), b, n, n_fft, hop, n_fft // 2, frames, core._stream()),
                 'ddsp_stft_frames_mag_f32')
      ld = torch.empty((b, 1, frames), dtype=torch.float32, device=dev)
      _lib.check(lib.ddsp_loudness_from_mag_f32(mag.data_ptr(), wt.data_ptr(), ld.data_ptr(), b, frames, bins,
                                                self.LOUDNESS_RANGE_DB, self.LOUDNESS_REF_DB, core._stream()),
                 'ddsp_loudness_from_mag_f32')
      loud.append(ld); mags.append(mag)
    wb = wf = wk = 0
    if weights is not None:
      # (`weights` multiplies the [batch, frames] difference in the reference: a [batch, frames, 1]-shaped mask reads as
      #  [batch, 1, frames] here only if it is broadcast along what it does not have - kept to masks of one value per clip)
      wb, wf, wk = (int(v) for v in weights.shape)
      if wf != 1 or wk != 1:
        raise ValueError('with loudness_weight > 0 the weights mask must be one value per clip ([batch, 1, 1]), got {}'.format(
            tuple(weights.shape)))
    want_grad = grad_audio is not None
    cot = torch.empty_like(loud[1]) if want_grad else None
    ws = self._ws.get(core.cached_workspace_bytes('ddsp_spectral_terms_workspace_bytes', b, 1), dev)
    rc = lib.ddsp_spectral_terms_f32(
        loud[0].data_ptr(), loud[1].data_ptr(), weights.data_ptr() if weights is not None else None, wb, wf, wk,
        cot.data_ptr() if want_grad else None, acc.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(), b, 1, frames,
        _lib.LOSS_TYPES[self.loss_type.upper()], float(self.loudness_weight), 0.0, 0.0, 0.0, 0.0, 1 if first else 0,
        core._stream())
    _lib.check(rc, 'ddsp_spectral_terms_f32')
    if want_grad:
      grad_mag = mags[0]                                         # (the target's magnitudes are done with: their buffer)
      _lib.check(lib.ddsp_loudness_from_mag_backward_f32(mags[1].data_ptr(), wt.data_ptr(), cot.data_ptr(), grad_mag.data_ptr(),
                                                         b, frames, bins, self.LOUDNESS_RANGE_DB, self.LOUDNESS_REF_DB,
                                                         core._stream()), 'ddsp_loudness_from_mag_backward_f32')
      if self._slabs():
        slabs = self._grad_ws.get(core.cached_workspace_bytes('ddsp_stft_frames_mag_backward_workspace_bytes', b, n, n_fft, hop,
                                                              n_fft // 2, frames), dev)
        _lib.check(lib.ddsp_stft_frames_mag_backward_det_f32(audio.data_ptr(), grad_mag.data_ptr(), grad_audio.data_ptr(),
                                                             slabs.data_ptr(), slabs.numel(), b, n, n_fft, hop, n_fft // 2,
                                                             frames, core._stream()),
                   'ddsp_stft_frames_mag_backward_det_f32')
      else:
        _lib.check(lib.ddsp_stft_frames_mag_backward_f32(audio.data_ptr(), grad_mag.data_ptr(), grad_audio.data_ptr(), b, n, n_fft,
                                                         hop, n_fft // 2, frames, core._stream()),
                   'ddsp_stft_frames_mag_backward_f32')

  def _sizes(self):
    return (ctypes.c_int * len(self.fft_sizes))(*[int(v) for v in self.fft_sizes])

  def _slab_workspace(self, audio):
    b, n = audio.shape
    sizes = tuple(int(v) for v in self.fft_sizes)
    # (the size query takes a ctypes array: cached under the sizes themselves)
    key = ('ddsp_spectral_loss_grad_workspace_bytes', b, n) + sizes
    nbytes = core._ws_bytes_cache.get(key)
    if nbytes is None:
      nbytes = _lib.load().ddsp_spectral_loss_grad_workspace_bytes(b, n, self._sizes(), len(sizes))
      core._ws_bytes_cache[key] = nbytes
    return self._grad_ws.get(nbytes, audio.device)

  def _forward(self, target_audio, audio):
    b, n = audio.shape
    sizes = self._sizes()
    lib = _lib.load()
    nbytes = lib.ddsp_spectral_loss_workspace_bytes(b, n, sizes, len(self.fft_sizes))
    if nbytes == 0:
      raise ValueError('fft_sizes must be at most 16 sizes the fused kernels take (2**k in [16, 8192], 3 * 2**k in [48, 6144]), got {}'.format(
          tuple(self.fft_sizes)))
    ws = self._ws.get(nbytes, audio.device)
    loss = torch.empty((), dtype=torch.float32, device=audio.device)
    rc = lib.ddsp_spectral_loss_f32(target_audio.data_ptr(), audio.data_ptr(), loss.data_ptr(),
                                    ws.data_ptr(), ws.numel(), b, n, sizes, len(self.fft_sizes),
                                    float(self.mag_weight), float(self.logmag_weight), core._stream())
    _lib.check(rc, 'ddsp_spectral_loss_f32')
    return loss

  def _value_and_grad(self, target_audio, audio):
    b, n = audio.shape
    sizes = self._sizes()
    lib = _lib.load()
    nbytes = lib.ddsp_spectral_loss_workspace_bytes(b, n, sizes, len(self.fft_sizes))
    if nbytes == 0:
      raise ValueError('fft_sizes must be at most 16 sizes the fused kernels take (2**k in [16, 8192], 3 * 2**k in [48, 6144]), got {}'.format(
          tuple(self.fft_sizes)))
    ws = self._ws.get(nbytes, audio.device)
    loss = torch.empty((), dtype=torch.float32, device=audio.device)
    grad_audio = torch.empty_like(audio)
    if self._slabs():
      slabs = self._slab_workspace(audio)
      rc = lib.ddsp_spectral_loss_value_and_grad_det_f32(
          target_audio.data_ptr(), audio.data_ptr(), loss.data_ptr(), grad_audio.data_ptr(), ws.data_ptr(),
          ws.numel(), b, n, sizes, len(self.fft_sizes), float(self.mag_weight), float(self.logmag_weight),
          slabs.data_ptr(), slabs.numel(), core._stream())
      _lib.check(rc, 'ddsp_spectral_loss_value_and_grad_det_f32')
      return loss, grad_audio
    rc = lib.ddsp_spectral_loss_value_and_grad_f32(
        target_audio.data_ptr(), audio.data_ptr(), loss.data_ptr(), grad_audio.data_ptr(), ws.data_ptr(),
        ws.numel(), b, n, sizes, len(self.fft_sizes), float(self.mag_weight), float(self.logmag_weight),
        core._stream())
    _lib.check(rc, 'ddsp_spectral_loss_value_and_grad_f32')
    return loss, grad_audio

  def _backward(self, target_audio, audio, grad_loss):
    b, n = audio.shape
    grad_loss = core.tf_float32(grad_loss).reshape(1).contiguous()
    grad_audio = torch.empty_like(audio)
    if self._slabs():
      slabs = self._slab_workspace(audio)
      rc = _lib.load().ddsp_spectral_loss_backward_det_f32(
          target_audio.data_ptr(), audio.data_ptr(), grad_loss.data_ptr(), grad_audio.data_ptr(), b, n,
          self._sizes(), len(self.fft_sizes), float(self.mag_weight), float(self.logmag_weight),
          slabs.data_ptr(), slabs.numel(), core._stream())
      _lib.check(rc, 'ddsp_spectral_loss_backward_det_f32')
      return grad_audio
    rc = _lib.load().ddsp_spectral_loss_backward_f32(
        target_audio.data_ptr(), audio.data_ptr(), grad_loss.data_ptr(), grad_audio.data_ptr(), b, n,
        self._sizes(), len(self.fft_sizes), float(self.mag_weight), float(self.logmag_weight),
        core._stream())
    _lib.check(rc, 'ddsp_spectral_loss_backward_f32')
    return grad_audio


def _scale(grad_audio, grad_loss):
  """grad_audio * (the upstream scalar dL/dloss), on ddsp_scale_f32."""
  grad_loss = core.tf_float32(grad_loss).reshape(1).contiguous()
  out = torch.empty_like(grad_audio)
  rc = _lib.load().ddsp_scale_f32(grad_audio.data_ptr(), grad_loss.data_ptr(), out.data_ptr(), grad_audio.numel(),
                                  core._stream())
  _lib.check(rc, 'ddsp_scale_f32')
  return out


class _SpectralLossFunction(torch.autograd.Function):
  """torch.autograd node of SpectralLoss.call: the gradient flows to `audio` only."""

  @staticmethod
  def forward(ctx, target_audio, audio, loss_obj):
    # value and gradient in one pass (the frame spectra are computed once for both)
    loss, grad_audio = loss_obj._value_and_grad(target_audio, audio.detach())
    ctx.save_for_backward(grad_audio)
    return loss

  @staticmethod
  def backward(ctx, grad_loss):
    (grad_audio,) = ctx.saved_tensors
    return None, _scale(grad_audio, grad_loss), None


class _SpectralLossGeneralFunction(torch.autograd.Function):
  """torch.autograd node of the general SpectralLoss: value and dL/d audio come out of the same pass."""

  @staticmethod
  def forward(ctx, target_audio, audio, loss_obj, weights):
    loss, grad_audio = loss_obj._general(target_audio, audio.detach(), weights, want_grad=True)
    ctx.save_for_backward(grad_audio)
    return loss

  @staticmethod
  def backward(ctx, grad_loss):
    (grad_audio,) = ctx.saved_tensors
    return None, _scale(grad_audio, grad_loss), None, None


# --------------------------------------------------------------------------------------
# Consistency losses (ddsp/losses.py:489-578, 689-1076).  csrc/consistency.hip holds the kernels of KDEConsistencyLoss, TWMLoss
# and core.sinusoidal_to_harmonic, csrc/wasserstein.hip those of WassersteinConsistencyLoss / wasserstein_distance; the thin
# ones run on mean_difference.  A loss is a sum of up to three 0-dim terms, each the output of a kernel; the terms are added
# as 0-dim tensors (as SpectralLoss adds its fused and plain parts).  csrc/hmm.hip holds the kernels of HmmTranscriber.
# Not built: EmbeddingLoss, the CREPE classes.
# --------------------------------------------------------------------------------------
def amp_loss(amp, amp_target, loss_type='L1', weights=None, log=False, amin=1e-5):
  """Loss comparing two amplitudes (scale logarithmically) (ddsp/losses.py:492-504)."""
  if log:
    amp = core._log10_floor(amp, amin)
    amp_target = core._log10_floor(amp_target, amin)
  return mean_difference(amp, amp_target, loss_type, weights)


def freq_loss(f_hz, f_hz_target, loss_type='L1', weights=None):
  """Loss comparing two frequencies, in MIDI (ddsp/losses.py:507-513)."""
  f_midi = core._hz_to_midi_diff(f_hz)
  f_midi_target = core._hz_to_midi_diff(f_hz_target)
  return mean_difference(f_midi, f_midi_target, loss_type, weights)


def _weighted(weight, loss):
  """weight * loss for a 0-dim loss, on ddsp_mean_f32 (the mean of one element, scaled)."""
  return core._mean(loss.reshape(1), float(weight))


class FilteredNoiseConsistencyLoss(Loss):
  """Consistency loss for synthesizer controls (ddsp/losses.py:516-530)."""

  def __init__(self, weight=1.0, name='filtered_noise_consistency_loss'):
    super().__init__(name=name)
    self.weight = weight

  def call(self, noise_magnitudes, noise_magnitudes_target):
    return _weighted(self.weight, amp_loss(noise_magnitudes, noise_magnitudes_target))


class HarmonicConsistencyLoss(Loss):
  """Consistency loss for synthesizer controls (ddsp/losses.py:533-578): a dictionary of three weighted terms."""

  def __init__(self, amp_weight=1.0, dist_weight=1.0, f0_weight=1.0, amp_threshold=1e-4, name='harmonic_consistency_loss'):
    super().__init__(name=name)
    self.amp_weight = amp_weight
    self.dist_weight = dist_weight
    self.f0_weight = f0_weight
    self.amp_threshold = amp_threshold

  def call(self, harm_amp, harm_amp_target, harm_dist, harm_dist_target, f0_hz, f0_hz_target):
    losses_dict = {}
    # mask where the target is below the threshold amplitude: a comparison, not differentiable - a weight
    target = core.tf_float32(harm_amp_target).detach()
    threshold = torch.full((1,), float(self.amp_threshold), dtype=torch.float32, device=target.device)
    weights = core.tf_float32(target >= threshold)
    losses_dict['harm_amp_loss'] = _weighted(self.amp_weight, amp_loss(harm_amp, harm_amp_target))
    losses_dict['harm_dist_loss'] = _weighted(self.dist_weight, amp_loss(harm_dist, harm_dist_target, weights=weights))
    losses_dict['f0_hz_loss'] = _weighted(self.f0_weight, freq_loss(f0_hz, f0_hz_target, weights=weights))
    return losses_dict

  def get_losses_dict(self, *args, **kwargs):
    return self(*args, **kwargs)


class ParamLoss(Loss):
  """Loss on the mean difference between any two tensors (ddsp/losses.py:1064-1076)."""

  def __init__(self, weight=1.0, loss_type='L1', name='param_loss'):
    super().__init__(name=name)
    self.weight = weight
    self.loss_type = loss_type

  def call(self, pred, target, weights=None):
    return _weighted(self.weight, mean_difference(pred, target, self.loss_type, weights))


def _sinusoid_frames(names, tensors, same_last=True):
  """[batch, time, n] tensors that share batch and time (and the last axis, if same_last) -> contiguous fp32."""
  out = [core.tf_float32(t) for t in tensors]
  shapes = ', '.join('{} {}'.format(n, tuple(t.shape)) for n, t in zip(names, out))
  if any(t.dim() != 3 for t in out) or any(t.shape[:2] != out[0].shape[:2] for t in out):
    raise ValueError('expected [batch, time, n] tensors with equal batch and time, got ' + shapes)
  if same_last and any(t.shape[2] != out[0].shape[2] for t in out):
    raise ValueError('the last axes must be equal, got ' + shapes)
  if any(t.shape[2] < 1 for t in out):
    raise ValueError('the last axes must not be empty, got ' + shapes)
  return out


class _KdeNllFunction(torch.autograd.Function):
  """torch.autograd node of KDEConsistencyLoss.nll (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, amps, freqs, amps_target, freqs_target, scale):
    ctx.save_for_backward(amps, freqs, amps_target, freqs_target)
    ctx.scale = scale
    b, t, k = amps.shape
    nll = torch.empty((b, t), dtype=torch.float32, device=amps.device)
    if b * t:
      rc = _lib.load().ddsp_kde_nll_f32(amps.data_ptr(), freqs.data_ptr(), amps_target.data_ptr(), freqs_target.data_ptr(),
                                        nll.data_ptr(), b * t, k, amps_target.shape[2], scale, core._stream())
      _lib.check(rc, 'ddsp_kde_nll_f32')
    return nll

  @staticmethod
  def backward(ctx, grad_nll):
    amps, freqs, amps_target, freqs_target = ctx.saved_tensors
    b, t, k = amps.shape
    grad_nll = core.tf_float32(grad_nll)
    grads = [torch.empty_like(x) for x in (amps, freqs, amps_target, freqs_target)]
    if b * t:
      rc = _lib.load().ddsp_kde_nll_backward_f32(amps.data_ptr(), freqs.data_ptr(), amps_target.data_ptr(), freqs_target.data_ptr(),
                                                 grad_nll.data_ptr(), *[g.data_ptr() for g in grads], b * t, k,
                                                 amps_target.shape[2], ctx.scale, core._stream())
      _lib.check(rc, 'ddsp_kde_nll_backward_f32')
    return grads[0], grads[1], grads[2], grads[3], None


class KDEConsistencyLoss(Loss):
  """Compare similarity of two traces of sinusoids using kernels (ddsp/losses.py:689-813): a Gaussian kernel density estimate
  in both directions, in MIDI, and the difference of the mean amplitudes.  The [batch, time, K, K] tensors of the reference
  are never built (csrc/consistency.hip: a block per frame); up to 1024 sinusoids on either side."""

  def __init__(self, weight_a=1.0, weight_b=1.0, weight_mean_amp=1.0, scale_a=0.1, scale_b=0.1, name='kde_consistency_loss'):
    super().__init__(name=name)
    self.weight_a = weight_a
    self.weight_b = weight_b
    self.weight_mean_amp = weight_mean_amp
    self.scale_a = scale_a
    self.scale_b = scale_b

  def call(self, amps_a, freqs_a, amps_b, freqs_b):
    """Scalar, weighted -log p(a|b) - log p(b|a) (+ the mean-amplitude term).  A term whose weight is not > 0 is skipped."""
    amps_a, freqs_a = _sinusoid_frames(('amps_a', 'freqs_a'), (amps_a, freqs_a))
    amps_b, freqs_b = _sinusoid_frames(('amps_b', 'freqs_b'), (amps_b, freqs_b))
    loss = 0.0
    if self.weight_a > 0.0:
      loss = loss + core._mean(self.nll(amps_a, freqs_a, amps_b, freqs_b, self.scale_b), self.weight_a)
    if self.weight_b > 0.0:
      loss = loss + core._mean(self.nll(amps_b, freqs_b, amps_a, freqs_a, self.scale_a), self.weight_b)
    if self.weight_mean_amp > 0.0:
      loss = loss + _weighted(self.weight_mean_amp, mean_difference(core._row_mean(amps_a), core._row_mean(amps_b), 'L1'))
    return loss

  def nll(self, amps, freqs, amps_target, freqs_target, scale_target):
    """-log p(source | target), [batch, time]."""
    amps, freqs = _sinusoid_frames(('amps', 'freqs'), (amps, freqs))
    amps_target, freqs_target = _sinusoid_frames(('amps_target', 'freqs_target'), (amps_target, freqs_target))
    _sinusoid_frames(('amps', 'amps_target'), (amps, amps_target), same_last=False)
    if max(amps.shape[2], amps_target.shape[2]) > _lib.CONSISTENCY_MAX_K:
      raise NotImplementedError('KDEConsistencyLoss takes up to {} sinusoids on the MI355X path, got {} and {}'.format(
          _lib.CONSISTENCY_MAX_K, amps.shape[2], amps_target.shape[2]))
    args = (amps, freqs, amps_target, freqs_target, float(scale_target))
    if core._needs_grad(*args[:4]):
      return _KdeNllFunction.apply(*args)
    return _KdeNllFunction.forward(core._NoCtx(), *args)


class _TwmTensorsFunction(torch.autograd.Function):
  """torch.autograd node of TWMLoss.get_loss_tensors (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, f0_candidates, freqs, amps, args):
    b, t, c = f0_candidates.shape
    sin_loss = torch.empty((b, t, c), dtype=torch.float32, device=freqs.device)
    harm_loss = torch.empty_like(sin_loss)
    if b * t:
      rc = _lib.load().ddsp_twm_loss_tensors_f32(f0_candidates.data_ptr(), freqs.data_ptr(), amps.data_ptr(), sin_loss.data_ptr(),
                                                 harm_loss.data_ptr(), b * t, c, freqs.shape[2], *args, core._stream())
      _lib.check(rc, 'ddsp_twm_loss_tensors_f32')
    ctx.save_for_backward(f0_candidates, freqs, amps, sin_loss)
    ctx.args = args
    return sin_loss, harm_loss

  @staticmethod
  def backward(ctx, grad_sin, grad_harm):
    f0_candidates, freqs, amps, sin_loss = ctx.saved_tensors
    b, t, c = f0_candidates.shape
    grad_sin, grad_harm = core.tf_float32(grad_sin), core.tf_float32(grad_harm)
    grads = [torch.empty_like(x) for x in (f0_candidates, freqs, amps)]
    if b * t:
      rc = _lib.load().ddsp_twm_loss_tensors_backward_f32(
          f0_candidates.data_ptr(), freqs.data_ptr(), amps.data_ptr(), sin_loss.data_ptr(), grad_sin.data_ptr(), grad_harm.data_ptr(),
          *[g.data_ptr() for g in grads], b * t, c, freqs.shape[2], *ctx.args, core._stream())
      _lib.check(rc, 'ddsp_twm_loss_tensors_backward_f32')
    return grads[0], grads[1], grads[2], None


class _TwmSoftminFunction(torch.autograd.Function):
  """Per frame sum_c L_c softmax(-L / temperature)_c, L = w_s S + w_h H (ddsp/losses.py:917-920)."""

  @staticmethod
  def forward(ctx, sin_loss, harm_loss, args):
    ctx.save_for_backward(sin_loss, harm_loss)
    ctx.args = args
    b, t, c = sin_loss.shape
    out = torch.empty((b, t), dtype=torch.float32, device=sin_loss.device)
    if b * t:
      rc = _lib.load().ddsp_twm_softmin_f32(sin_loss.data_ptr(), harm_loss.data_ptr(), out.data_ptr(), b * t, c, *args, core._stream())
      _lib.check(rc, 'ddsp_twm_softmin_f32')
    return out

  @staticmethod
  def backward(ctx, grad_out):
    sin_loss, harm_loss = ctx.saved_tensors
    b, t, c = sin_loss.shape
    grad_out = core.tf_float32(grad_out)
    g_sin, g_harm = torch.empty_like(sin_loss), torch.empty_like(harm_loss)
    if b * t:
      rc = _lib.load().ddsp_twm_softmin_backward_f32(sin_loss.data_ptr(), harm_loss.data_ptr(), grad_out.data_ptr(), g_sin.data_ptr(),
                                                     g_harm.data_ptr(), b * t, c, *ctx.args, core._stream())
      _lib.check(rc, 'ddsp_twm_softmin_backward_f32')
    return g_sin, g_harm, None


class TWMLoss(Loss):
  """Two-way Mismatch, encourages sinusoids to be harmonics of the best f0 candidate (ddsp/losses.py:819-1061).

  Loss = -log p(sinusoids | harmonics) - log p(harmonics | sinusoids) per candidate, a softmin over the candidates.  The
  [batch, time, candidates, sinusoids, gaussians] and [batch, time, candidates, points, sinusoids] tensors of the reference are
  never built (csrc/consistency.hip: a block per frame).  Up to 1024 sinusoids, 256 harmonic points, 4096 harmonic
  Gaussians, any number of candidates."""

  def __init__(self, sinusoids_weight=1.0, harmonics_weight=1.0, sinusoids_scale=0.5, harmonics_scale=0.2, n_harmonic_points=10,
               n_harmonic_gaussians=30, softmin_temperature=1.0, sample_rate=16000, name='twm_loss'):
    super().__init__(name=name)
    self.softmin_temperature = softmin_temperature
    self.sample_rate = sample_rate
    self.sinusoids_weight = sinusoids_weight
    self.harmonics_weight = harmonics_weight
    self.sinusoids_scale = sinusoids_scale
    self.n_harmonic_points = n_harmonic_points
    self.harmonics_scale = harmonics_scale
    self.n_harmonic_gaussians = n_harmonic_gaussians

  def call(self, f0_candidates, freqs, amps):
    """Scalar: the mean over [batch, time, candidates] of L softmax(-L / temperature), L the weighted sum of the two tensors."""
    sinusoids_loss, harmonics_loss = self.get_loss_tensors(f0_candidates, freqs, amps)
    args = (sinusoids_loss, harmonics_loss,
            (float(self.sinusoids_weight), float(self.harmonics_weight), float(self.softmin_temperature)))
    if core._needs_grad(sinusoids_loss, harmonics_loss):
      frame_loss = _TwmSoftminFunction.apply(*args)
    else:
      frame_loss = _TwmSoftminFunction.forward(core._NoCtx(), *args)
    return core._mean(frame_loss, 1.0 / sinusoids_loss.shape[2])

  def predict_f0(self, f0_candidates, freqs, amps):
    """The most likely f0 among the candidates at each timestep: numpy array [batch, time, 1].  The arg-min runs on the
    device and ignores NaN (np.nanargmin); a frame whose losses are all NaN raises ValueError, as numpy does."""
    with torch.no_grad():
      sinusoids_loss, harmonics_loss = self.get_loss_tensors(f0_candidates, freqs, amps)
      f0_candidates = core.tf_float32(f0_candidates)
      b, t, c = sinusoids_loss.shape
      f0_hz = torch.empty((b, t, 1), dtype=torch.float32, device=sinusoids_loss.device)
      flag = torch.zeros((1,), dtype=torch.int32, device=sinusoids_loss.device)
      if b * t:
        rc = _lib.load().ddsp_twm_nanargmin_f32(sinusoids_loss.data_ptr(), harmonics_loss.data_ptr(), f0_candidates.data_ptr(),
                                                f0_hz.data_ptr(), flag.data_ptr(), b * t, c, float(self.sinusoids_weight),
                                                float(self.harmonics_weight), core._stream())
        _lib.check(rc, 'ddsp_twm_nanargmin_f32')
      if int(flag.cpu()[0]):
        raise ValueError('All-NaN slice encountered')
      return f0_hz.cpu().numpy()

  def get_loss_tensors(self, f0_candidates, freqs, amps):
    """(-log p(sinusoids | harmonics), -log p(harmonics | sinusoids)), both [batch, time, f0_candidate]."""
    freqs, amps = _sinusoid_frames(('freqs', 'amps'), (freqs, amps))
    f0_candidates, _ = _sinusoid_frames(('f0_candidates', 'freqs'), (f0_candidates, freqs), same_last=False)
    p, g = int(self.n_harmonic_points), int(self.n_harmonic_gaussians)
    if p < 1 or g < 1:
      raise ValueError('n_harmonic_points and n_harmonic_gaussians must be at least 1, got {} and {}'.format(p, g))
    if freqs.shape[2] > _lib.CONSISTENCY_MAX_K or p > _lib.CONSISTENCY_MAX_POINTS or g > _lib.CONSISTENCY_MAX_GAUSSIANS:
      raise NotImplementedError('TWMLoss takes up to {} sinusoids, {} harmonic points and {} harmonic gaussians on the MI355X path, '
                                'got {}, {} and {}'.format(_lib.CONSISTENCY_MAX_K, _lib.CONSISTENCY_MAX_POINTS,
                                                           _lib.CONSISTENCY_MAX_GAUSSIANS, freqs.shape[2], p, g))
    args = (p, g, float(self.sinusoids_scale), float(self.harmonics_scale), float(self.sample_rate))
    if core._needs_grad(f0_candidates, freqs, amps):
      return _TwmTensorsFunction.apply(f0_candidates, freqs, amps, args)
    return _TwmTensorsFunction.forward(core._NoCtx(), f0_candidates, freqs, amps, args)


class _WassersteinFunction(torch.autograd.Function):
  """torch.autograd node of wasserstein_distance on [rows, n] tensors (plumbing: both directions are C-ABI calls)."""

  @staticmethod
  def forward(ctx, u_values, v_values, u_weights, v_weights, p, flags):
    ctx.save_for_backward(u_values, v_values, u_weights, v_weights)
    ctx.args = (u_values.shape[1], v_values.shape[1], p, flags)
    rows = u_values.shape[0]
    distance = torch.empty((rows,), dtype=torch.float32, device=u_values.device)
    if rows:
      rc = _lib.load().ddsp_wasserstein_f32(u_values.data_ptr(), v_values.data_ptr(), _ptr(u_weights), _ptr(v_weights),
                                            distance.data_ptr(), rows, *ctx.args, core._stream())
      _lib.check(rc, 'ddsp_wasserstein_f32')
    return distance

  @staticmethod
  def backward(ctx, grad_distance):
    u_values, v_values, u_weights, v_weights = ctx.saved_tensors
    grad_distance = core.tf_float32(grad_distance)
    grads = [None if x is None else torch.empty_like(x) for x in (u_values, v_values, u_weights, v_weights)]
    if u_values.shape[0]:
      rc = _lib.load().ddsp_wasserstein_backward_f32(u_values.data_ptr(), v_values.data_ptr(), _ptr(u_weights), _ptr(v_weights),
                                                     grad_distance.data_ptr(), *[_ptr(g) for g in grads], u_values.shape[0],
                                                     *ctx.args, core._stream())
      _lib.check(rc, 'ddsp_wasserstein_backward_f32')
    return grads[0], grads[1], grads[2], grads[3], None, None


def _ptr(x):
  return None if x is None else x.data_ptr()


def _wasserstein(u_values, v_values, u_weights, v_weights, p, flags):
  """wasserstein_distance on contiguous fp32 tensors, [..., n_u] against [..., n_v] -> [...]."""
  p = float(p)
  if p not in (1.0, 2.0):
    raise NotImplementedError('wasserstein_distance is built for p = 1 and p = 2 on the MI355X path, got p = {}'.format(p))
  names = ('u_values', 'v_values', 'u_weights', 'v_weights')
  tensors = (u_values, v_values, u_weights, v_weights)
  shapes = ', '.join('{} {}'.format(n, tuple(t.shape)) for n, t in zip(names, tensors) if t is not None)
  if u_values.dim() < 1 or v_values.dim() < 1 or u_values.shape[:-1] != v_values.shape[:-1]:
    raise ValueError('expected [..., n] tensors with equal batch shapes, got ' + shapes)
  for values, weights in ((u_values, u_weights), (v_values, v_weights)):
    if weights is not None and weights.shape != values.shape:
      raise ValueError('weights must have the shape of their values, got ' + shapes)
  n_u, n_v = u_values.shape[-1], v_values.shape[-1]
  if n_u < 1 or n_v < 1:
    raise ValueError('the last axes must not be empty, got ' + shapes)
  if max(n_u, n_v) > _lib.CONSISTENCY_MAX_K:
    raise NotImplementedError('wasserstein_distance takes up to {} samples a side on the MI355X path, got {} and {}'.format(
        _lib.CONSISTENCY_MAX_K, n_u, n_v))
  batch = u_values.shape[:-1]
  args = [None if t is None else t.reshape(-1, t.shape[-1]) for t in tensors] + [int(p), flags]
  if core._needs_grad(*tensors):
    return _WassersteinFunction.apply(*args).reshape(batch)
  return _WassersteinFunction.forward(core._NoCtx(), *args).reshape(batch)


def wasserstein_distance(u_values, v_values, u_weights, v_weights, p=1.0):
  """Differentiable 1-D Wasserstein distance (ddsp/losses.py:632-686), adapted there from scipy.stats.

  u_values [..., n_u], v_values [..., n_v] with equal batch shapes; u_weights / v_weights of their values' shapes, or None;
  p: 1 (Wasserstein) or 2 (energy) -> [...].  As in the reference THE WEIGHTS ARE NOT NORMALISED (it computes the normalised
  CDF and drops the result): only a side with weights=None has a CDF that ends at 1.  One fused kernel per direction
  (csrc/wasserstein.hip: a block per row sorts, scans and reduces in LDS); up to 1024 samples a side."""
  u_values, v_values = core.tf_float32(u_values), core.tf_float32(v_values)
  u_weights = None if u_weights is None else core.tf_float32(u_weights)
  v_weights = None if v_weights is None else core.tf_float32(v_weights)
  return _wasserstein(u_values, v_values, u_weights, v_weights, p, 0)


class WassersteinConsistencyLoss(Loss):
  """Compare similarity of two traces of sinusoids using wasserstein distance (ddsp/losses.py:584-629; EXPERIMENTAL there).

  The mean over [batch, time] of weight * wasserstein_distance(hz_to_midi(freqs_a), hz_to_midi(freqs_b), amps_a, amps_b, p=1).
  Two quirks of the reference are kept: the amplitudes weigh the frequencies WITHOUT being normalised (see
  wasserstein_distance), and the distance is computed only inside `if self.midi:` - with midi=False, as with weight <= 0,
  the loss is the float 0.0.  hz_to_midi is taken inside the kernel: no MIDI tensor is built.  Up to 1024 sinusoids a side."""

  def __init__(self, weight=1.0, midi=True, name='wasserstein_consistency_loss'):
    super().__init__(name=name)
    self.weight = weight
    self.midi = midi

  def call(self, amps_a, freqs_a, amps_b, freqs_b):
    """Scalar, weighted wasserstein distance."""
    loss = 0.0
    if self.weight > 0.0 and self.midi:
      amps_a, freqs_a = _sinusoid_frames(('amps_a', 'freqs_a'), (amps_a, freqs_a))
      amps_b, freqs_b = _sinusoid_frames(('amps_b', 'freqs_b'), (amps_b, freqs_b))
      _sinusoid_frames(('amps_a', 'amps_b'), (amps_a, amps_b), same_last=False)
      loss = core._mean(_wasserstein(freqs_a, freqs_b, amps_a, amps_b, 1.0, _lib.WASSERSTEIN_MIDI), self.weight)
    return loss


class _HmmLogProbFunction(torch.autograd.Function):
  """torch.autograd node of HmmTranscriber's log-likelihood on [rows, steps] tensors (plumbing: both directions are C-ABI
  calls; the backward call recomputes the forward variables into scratch, so nothing but the inputs is kept)."""

  @staticmethod
  def forward(ctx, pitch, amps, model):
    ctx.save_for_backward(pitch, amps)
    ctx.model = model
    rows, steps = pitch.shape
    log_prob = torch.empty((rows,), dtype=torch.float32, device=pitch.device)
    if rows:
      rc = _lib.load().ddsp_hmm_log_prob_f32(pitch.data_ptr(), amps.data_ptr(), log_prob.data_ptr(), rows, steps, *model,
                                             core._stream())
      _lib.check(rc, 'ddsp_hmm_log_prob_f32')
    return log_prob

  @staticmethod
  def backward(ctx, grad_log_prob):
    pitch, amps = ctx.saved_tensors
    rows, steps = pitch.shape
    grad_log_prob = core.tf_float32(grad_log_prob)
    grads = [torch.empty_like(pitch), torch.empty_like(amps)]
    if rows:
      nbytes = core.cached_workspace_bytes('ddsp_hmm_log_prob_backward_workspace_bytes', rows, steps, ctx.model[0])
      ws = core._default_ws.get(nbytes, pitch.device)
      rc = _lib.load().ddsp_hmm_log_prob_backward_f32(pitch.data_ptr(), amps.data_ptr(), grad_log_prob.data_ptr(),
                                                      grads[0].data_ptr(), grads[1].data_ptr(), ws.data_ptr(), ws.numel(), rows,
                                                      steps, *ctx.model, core._stream())
      _lib.check(rc, 'ddsp_hmm_log_prob_backward_f32')
    return grads[0], grads[1], None


class HmmTranscriber:
  """HMM initialized for decoding MIDI from Pitch and Amps (ddsp/losses.py:246-345).

  Discrete hidden states for each midi pitch, f0 observations (in midi).  State 0 is "off" (pitch ~ N(n_pitches / 2,
  n_pitches), amps ~ N(amps_off_center, amps_off_scale)); state s >= 1 has pitch ~ N(s, midi_std) and amps ~
  N(amps_on_center, amps_on_scale).  The initial distribution is uniform; a state is held with probability 1 - 1 / avg_length
  and left for each other state with equal probability.  That matrix is `other` everywhere plus `hold - other` on the
  diagonal, so a step of the forward algorithm, of its backward pass and of the Viterbi recursion costs O(n_pitches)
  (csrc/hmm.hip: a block walks a row; nothing of size [n_pitches, n_pitches] or [batch, steps, n_pitches, n_pitches] exists).

  Of tfp.distributions.HiddenMarkovModel, which the reference class derives from, this is log_prob (as `nll`) and
  posterior_mode (as `predict_midi`).  OUT OF SCOPE: sampling, posterior_marginals as a public method, arbitrary transition or
  observation models, and the distribution objects the reference keeps as attributes.  Limits of the MI355X path
  (NotImplementedError): 2 <= n_pitches <= 1024; avg_length >= n_pitches / (n_pitches - 1), i.e. holding a state is at least
  as likely as any one jump.

  Args:
    avg_length: Prior over average note length between transitions.
    midi_std: Prior over f0 variance (in midi) allowed around discrete states.
    amps_on_center: Center amplitude of the "on" state.
    amps_on_scale: Variance amplitude of the "on" state.
    amps_off_center: Center amplitude of the "off" state.
    amps_off_scale: Variance amplitude of the "off" state.
    n_timesteps: Number of timesteps in the batch to unroll the HMM.
    n_pitches: Number of pitches (starting from 0) to use as HMM states.
    weight: Weighting of the nll loss term.
  """

  def __init__(self, avg_length=200, midi_std=0.5, amps_on_center=1.5, amps_on_scale=0.5, amps_off_center=0.0,
               amps_off_scale=0.1, n_timesteps=1000, n_pitches=128, weight=1.0):
    if not 2 <= n_pitches <= _lib.HMM_MAX_PITCHES:
      raise NotImplementedError('HmmTranscriber takes 2 <= n_pitches <= {} on the MI355X path, got n_pitches = {}'.format(
          _lib.HMM_MAX_PITCHES, n_pitches))
    if min(midi_std, amps_on_scale, amps_off_scale) <= 0.0 or avg_length <= 0.0:
      raise ValueError('avg_length and the scales must be positive, got avg_length = {}, midi_std = {}, amps_on_scale = {}, '
                       'amps_off_scale = {}'.format(avg_length, midi_std, amps_on_scale, amps_off_scale))
    # Transition is heavily peaked around diagonal and uniform otherwise; the rows are renormalised as the reference's are
    hold = 1.0 - 1.0 / avg_length
    other = (1.0 - hold) / (n_pitches - 1)
    total = hold + (n_pitches - 1) * other
    hold, other = hold / total, other / total
    if hold < other:
      raise NotImplementedError('HmmTranscriber needs hold >= other on the MI355X path, i.e. avg_length >= n_pitches / '
                                '(n_pitches - 1) = {}, got avg_length = {}'.format(n_pitches / (n_pitches - 1.0), avg_length))
    self.avg_length = avg_length
    self.midi_std = midi_std
    self.n_timesteps = n_timesteps
    self.n_pitches = n_pitches
    self.weight = weight
    self._model = (int(n_pitches), hold, other, float(midi_std), float(amps_on_center), float(amps_on_scale),
                   float(amps_off_center), float(amps_off_scale))

  def __call__(self, pitch, amps):
    return self.nll(pitch, amps)

  @staticmethod
  def straight_through(x, x_quant):
    """Straight through estimation."""
    return x - (x - x_quant).detach()

  def _observations(self, pitch, amps):
    """[batch, n_timesteps, 1] each -> contiguous fp32 [batch, n_timesteps]."""
    pitch, amps = core.tf_float32(pitch), core.tf_float32(amps)
    if pitch.shape != amps.shape:
      raise ValueError('pitch and amps must have equal shapes, got {} and {}'.format(tuple(pitch.shape), tuple(amps.shape)))
    if pitch.dim() != 3 or pitch.shape[2] != 1:
      raise ValueError('expected [batch, n_timesteps, 1] tensors, got {}'.format(tuple(pitch.shape)))
    if pitch.shape[1] != self.n_timesteps:
      raise ValueError('the model is unrolled over n_timesteps = {} steps, got {}'.format(self.n_timesteps, pitch.shape[1]))
    return pitch.reshape(pitch.shape[:2]), amps.reshape(amps.shape[:2])

  def log_prob(self, pitch, amps):
    """Log-likelihood of the observations, [batch]; differentiable in pitch and amps."""
    pitch, amps = self._observations(pitch, amps)
    if core._needs_grad(pitch, amps):
      return _HmmLogProbFunction.apply(pitch, amps, self._model)
    return _HmmLogProbFunction.forward(core._NoCtx(), pitch, amps, self._model)

  def nll(self, pitch, amps, per_example_loss=False):
    """Negative log-likelihood per a timestep: weight * mean over the batch (0-dim), or [batch] with per_example_loss."""
    log_prob = self.log_prob(pitch, amps)
    scale = -float(self.weight) / self.n_timesteps
    if per_example_loss:
      return log_prob * scale                 # [batch] numbers: a framework op, as the reference's own `self.weight * loss`
    return core._mean(log_prob, scale)

  def predict_midi(self, pitch, amps, channel_dim=True, dtype=torch.float32):
    """Viterbi decode most likely hidden state as the quantized MIDI signal: [batch, n_timesteps, 1], or [batch, n_timesteps]
    with channel_dim=False.  No gradient flows through it (see straight_through)."""
    pitch, amps = self._observations(pitch, amps)
    pitch, amps = pitch.detach(), amps.detach()
    rows, steps = pitch.shape
    states = torch.empty((rows, steps), dtype=torch.int32, device=pitch.device)
    if rows:
      nbytes = core.cached_workspace_bytes('ddsp_hmm_viterbi_workspace_bytes', rows, steps, self.n_pitches)
      ws = core._default_ws.get(nbytes, pitch.device)
      rc = _lib.load().ddsp_hmm_viterbi_f32(pitch.data_ptr(), amps.data_ptr(), states.data_ptr(), ws.data_ptr(), ws.numel(), rows,
                                            steps, *self._model, core._stream())
      _lib.check(rc, 'ddsp_hmm_viterbi_f32')
    q_pitch = states.to(dtype)
    return q_pitch[:, :, None] if channel_dim else q_pitch
