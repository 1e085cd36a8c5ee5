"""ddsp/training/nn.py on the MI355X: the note pooling (csrc/notes.hip), the layers RnnFcDecoder is made of (csrc/decoder.hip), the
normalisations the encoders use (csrc/group_norm.hip) and the dilated convolution stack (csrc/dilated_conv.hip).

NOTE POOLING (ddsp/training/nn.py:357-557): straight_through_int_quantization, get_note_mask, get_note_mask_from_onset,
get_note_lengths, get_note_moments, pool_over_notes and get_short_note_loss_mask - what MidiAutoencoder and ZMidiAutoencoder pool
their per-note features with.

The reference builds [batch, time, notes, dims] four times between x and the pooled result; here nothing of that size
exists, and nothing of size [batch, time, notes] but the mask itself.  The moments and the pooling are exact for ANY fp32
mask (weights m in the mean, m ** 2 in the variance), and their cost follows the mask's non-zero entries.

THE GRADIENT OF THE STANDARD DEVIATION AT ZERO.  The reference's std is `(...) ** 0.5`, whose derivative is unbounded where
the variance is exactly 0: every empty region, every one-step note, every constant stretch - so in every real call.  The
contract here: where a note's variance in a dimension is exactly 0, that entry of the std contributes 0 to dL/dx;
everywhere else the gradient is the analytic one.  No gradient flows into a mask.

Limits (NotImplementedError): max_regions <= 1024; batch * notes and batch * time below 2 ** 31.

LAYERS (ddsp/training/nn.py:48-339, 844-934, 1327-1337): DictLayer, OutputSplitsLayer, ensure_4d, inv_ensure_4d, split_to_dict,
get_nonlinearity, Fc, FcStack, FcStackOut, Rnn, StatelessRnn, RnnFc, RnnSandwich, over torch.Tensors.  They are torch.nn.Modules
whose weights are torch.nn.Parameters under the reference's (Keras) names and layouts - Dense: kernel [in, out], bias [out];
LayerNormalization: gamma, beta, epsilon 1e-3; GRU: kernel [in, 3 H], recurrent_kernel [H, 3 H], bias [2, 3 H], gates z, r, h,
reset_after - built on the first call or through build(in_ch), with Keras' initialisers.  The matrix products whose M is
batch * time are torch.matmul (plumbing); bias + LayerNorm + activation and the recurrence are the kernels of csrc/decoder.hip,
forward and backward.  There is no CPU fallback: without the built library or a GPU the layers raise DdspLibraryError.
NOT BUILT (ValueError): rnn_type='lstm', bidir=True.

NORMALISATION (ddsp/training/nn.py:561-611, 1065-1136): normalize_op, Normalize, ConditionalScaleAndShift, ConditionalNorm,
get_norm, Identity, get_embedding.  normalize_op - instance, layer or group normalisation of a channel-last [batch, h, w, ch]
tensor, eps 1e-5 - and Normalize's scale and shift run in ONE kernel each way (csrc/group_norm.hip; C ABI csrc/norm_abi.h):
two-pass moments, nothing activation-sized kept for the backward but x itself, no atomics, the same bits for a batch row alone
and inside a batch.  The conditional scale and shift and the embedding's gather are framework ops.

DILATED CONVOLUTIONS (ddsp/training/nn.py:1153-1323): dilated_conv, Conv2D, Conv2DTranspose, DilatedConvStack.  ReLU -> dilated
1-D convolution with 'same' padding of a channel-last tensor, forward and the gradient in x, is ONE kernel (csrc/dilated_conv.hip;
C ABI csrc/conv_abi.h): matrix cores with fp16 hi / lo operands when ch_out is a multiple of 16, the vector ALU otherwise; no
padded copy, no atomics, the same bits for a batch row alone and inside a batch.  The weight gradients are K matrix products of
the framework.  The strided resamplers, FiLM's multiply-add and the residual add are framework ops.
NOT BUILT (ValueError): spectral_norm=True; and SpectralNormalization itself.

RESNET (ddsp/training/nn.py:697-839): conv2d, SpatialConv2D, MaxPool2D, NormReluConv, ResidualLayer, ResidualStack, ResNet.
(ReLU ->) 2-D convolution with 'same' padding and strides on both axes (+ addend), forward and the gradient in x, is ONE kernel
(csrc/conv2d.hip; C ABI csrc/conv2d_abi.h), the sibling of the dilated one: the product's K axis is the flattened (kh, kw, ch_in),
no im2col buffer, no padded copy, no atomics.  The normalisations stay on csrc/group_norm.hip; the ReLU behind them rides the
convolution's load and the residual add its epilogue.  The weight gradients are kh * kw matrix products of the framework; the max
pool and FiLM's multiply-add are framework ops.

VECTOR QUANTIZATION (ddsp/training/nn.py:1342-1461): vq_assign, vq_statistics, VectorQuantization.  The nearest centroid of every
vector and the per-centroid counts and sums of a batch are fused kernels (csrc/vq.hip; C ABI csrc/vq_abi.h): the reference's
[n, k] distance and one-hot matrices are never built, the heads are read in place.  Matrix cores with fp16 hi / lo operands when k
is a multiple of 16, the vector ALU otherwise; ties go to the lowest index; fp64 sums in a fixed order, no atomics.  The centroids,
the restarts and the moving averages are framework ops on [k, D].
Limits (NotImplementedError): k <= 4096, depth / num_heads <= 512, rows * num_heads below 2 ** 31.

THE REST (ddsp/training/nn.py:343-356, 615-694, 1141-1149): straight_through_softmax, straight_through_choice, polyphase_resample,
PolyphaseResample (framework ops, on host tensors too) and SingleGru (the GRU and LayerNormalization above)."""
import inspect
import math

import torch

from ddsp_amd import _lib
from ddsp_amd import core


# ------------------ Straight-through Estimators -------------------------------
def straight_through_int_quantization(x):
  """Rounds tensor to nearest integer using a straight through estimator (ddsp/training/nn.py:359-371).

  Values are rounded half to even, as tf.math.round does, and are not assumed to be scaled.  Returns the quantized x with
  gradients as if no quantization happened.  Framework ops."""
  x = core.tf_float32(x)
  return x + (torch.round(x) - x).detach()


def straight_through_softmax(logits):
  """Straight-through estimator of a one-hot categorical distribution (ddsp/training/nn.py:343-350).

  Returns (sample, probs): probs = softmax(logits) over the last axis; sample is one draw per distribution from torch's generator,
  one-hot in value - stop_gradient(sample - probs * sample) + probs * sample - with the gradient of probs * sample.  Framework ops,
  on the tensor's own device (host tensors too)."""
  logits = torch.as_tensor(logits)
  logits = logits if logits.is_floating_point() else logits.to(torch.float32)
  probs = torch.softmax(logits, dim=-1)
  flat = probs.detach().reshape(-1, probs.shape[-1])
  drawn = torch.multinomial(flat, 1) if flat.numel() else torch.zeros((flat.shape[0], 1), dtype=torch.int64, device=flat.device)
  sample = torch.zeros_like(flat).scatter_(1, drawn, 1.0).reshape(probs.shape)
  p_sample = probs * sample
  return (sample - p_sample).detach() + p_sample, probs


def straight_through_choice(logits, values):
  """Straight-through estimator of choosing a value using a boolean mask (ddsp/training/nn.py:353-356): [..., n] -> [..., 1]."""
  choice, _ = straight_through_softmax(logits)
  return torch.sum(choice * torch.as_tensor(values, device=choice.device), dim=-1, keepdim=True)


# ------------------ plumbing ---------------------------------------------------
def _check_limits(rows, steps, notes):
  if notes > _lib.NOTES_MAX_REGIONS:
    raise NotImplementedError('the note masks take max_regions <= {} on the MI355X path, got {}'.format(
        _lib.NOTES_MAX_REGIONS, notes))
  if rows * max(steps, notes) >= 2 ** 31:
    raise NotImplementedError('batch * notes and batch * time must stay below 2 ** 31, got batch = {}, time = {}, notes = {}'
                              .format(rows, steps, notes))


def _run_mask(q_pitch, onset, max_regions, note_on_only):
  rows, steps = q_pitch.shape
  mask = torch.empty((rows, steps, max_regions), dtype=torch.float32, device=q_pitch.device)
  if rows:
    rc = _lib.load().ddsp_note_mask_f32(q_pitch.data_ptr(), None if onset is None else onset.data_ptr(), mask.data_ptr(), rows,
                                        steps, max_regions, 1 if note_on_only else 0, core._stream())
    _lib.check(rc, 'ddsp_note_mask_f32')
  return mask


def _run_moments(x, mask, want_std, want_backward, sum_only=False):
  """x [b, t, d], mask [b, t, n] -> (mean, std, s2, mean_lo, safe lengths); the entries not asked for are None."""
  rows, steps, dims = x.shape
  notes = mask.shape[2]
  new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
  mean = new(rows, notes, dims)
  std = new(rows, notes, dims) if want_std else None
  s2 = new(rows, notes, dims) if want_std and want_backward else None
  mean_lo = new(rows, notes, dims) if want_std and want_backward else None
  lengths = new(rows, notes) if want_backward else None
  if rows:
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = _lib.load().ddsp_note_moments_f32(x.data_ptr(), mask.data_ptr(), mean.data_ptr(), ptr(std), ptr(s2), ptr(mean_lo), ptr(lengths),
                                           rows, steps, notes, dims, _lib.NOTES_SUM if sum_only else 0, core._stream())
    _lib.check(rc, 'ddsp_note_moments_f32')
  return mean, std, s2, mean_lo, lengths


def _run_spread(mask, a, c=None, x=None, mean=None, mean_lo=None):
  """out[b, t, :] = sum_n m (a[b, n, :] + c[b, n, :] m (x[b, t, :] - mean[b, n, :] - mean_lo[b, n, :])) -> [b, t, d]."""
  rows, steps, notes = mask.shape
  dims = a.shape[2]
  out = torch.empty((rows, steps, dims), dtype=torch.float32, device=mask.device)
  if rows:
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = _lib.load().ddsp_note_spread_f32(mask.data_ptr(), a.data_ptr(), ptr(c), ptr(x), ptr(mean), ptr(mean_lo), out.data_ptr(), rows,
                                          steps, notes, dims, core._stream())
    _lib.check(rc, 'ddsp_note_spread_f32')
  return out


class _NoteMomentsFunction(torch.autograd.Function):
  """torch.autograd node of get_note_moments in x (plumbing: both directions are C-ABI calls).  Kept for the backward: x, the
  mask and the [batch, notes(, dims)] results - mean, std, S2 = sum m^2 (x - mean), the safe lengths L, and what the fp32 mean
  lost of the fp64 one (x - mean cancels on a note of nearly equal values).  The backward is
  one spread: dL/dx[t] = sum_n m (a + c m (x[t] - mean)), a = (g_mean - 2 A S2) / L, c = 2 A, A = g_std / (2 std L), and
  A = 0 where std is exactly 0 (the module's contract)."""

  @staticmethod
  def forward(ctx, x, mask, want_std):
    needs = not isinstance(ctx, core._NoCtx)
    mean, std, s2, mean_lo, lengths = _run_moments(x, mask, want_std, needs)
    ctx.save_for_backward(x, mask, mean, std, s2, mean_lo, lengths)
    if want_std:
      return mean, std
    return mean

  @staticmethod
  def backward(ctx, grad_mean, grad_std=None):
    x, mask, mean, std, s2, mean_lo, lengths = ctx.saved_tensors
    inv_len = (1.0 / lengths)[:, :, None]
    a = core.tf_float32(grad_mean) * inv_len
    if std is None or grad_std is None:
      return _run_spread(mask, a.contiguous()), None, None
    positive = std > 0.0
    big_a = torch.where(positive, core.tf_float32(grad_std) * inv_len / (2.0 * torch.where(positive, std, torch.ones_like(std))),
                        torch.zeros_like(std))
    c = 2.0 * big_a
    a = a - c * s2 * inv_len
    return _run_spread(mask, a.contiguous(), c.contiguous(), x, mean, mean_lo), None, None


class _NoteSpreadFunction(torch.autograd.Function):
  """torch.autograd node of values [batch, notes, dims], mask -> sum_n m values [batch, time, dims]; its adjoint in the
  values is the masked sum over time, the moments kernel without its division."""

  @staticmethod
  def forward(ctx, values, mask):
    ctx.save_for_backward(mask)
    return _run_spread(mask, values)

  @staticmethod
  def backward(ctx, grad_out):
    mask, = ctx.saved_tensors
    return _run_moments(core.tf_float32(grad_out), mask, False, False, sum_only=True)[0], None


def _moments(x, mask, want_std):
  if core._needs_grad(x):
    return _NoteMomentsFunction.apply(x, mask, want_std)
  return _NoteMomentsFunction.forward(core._NoCtx(), x, mask, want_std)


def _spread(values, mask):
  if core._needs_grad(values):
    return _NoteSpreadFunction.apply(values, mask)
  return _NoteSpreadFunction.forward(core._NoCtx(), values, mask)


def _x_and_mask(op, x, note_mask, allow_2d):
  """-> contiguous fp32 x [b, t, d], mask [b, t, n], and whether x came as [b, t]."""
  x, note_mask = core.tf_float32(x), core.tf_float32(note_mask)
  core.require_no_grad(op + ' (note_mask)', note_mask)
  is_2d = x.dim() == 2
  if x.dim() != 3 and not (allow_2d and is_2d):
    raise ValueError('{}: x must be [batch, time, dims]{}, got {}'.format(op, ' or [batch, time]' if allow_2d else '',
                                                                          tuple(x.shape)))
  if note_mask.dim() != 3:
    raise ValueError('{}: note_mask must be [batch, time, notes], got {}'.format(op, tuple(note_mask.shape)))
  if tuple(note_mask.shape[:2]) != tuple(x.shape[:2]):
    raise ValueError('{}: x {} and note_mask {} must agree in batch and time'.format(op, tuple(x.shape), tuple(note_mask.shape)))
  if is_2d:
    x = x[:, :, None]
  if min(x.shape[1:]) < 1 or note_mask.shape[2] < 1:
    raise ValueError('{}: time, dims and notes must be at least 1, got x {} and note_mask {}'.format(
        op, tuple(x.shape), tuple(note_mask.shape)))
  if x.shape[0] * max(x.shape[1], note_mask.shape[2]) >= 2 ** 31:
    raise NotImplementedError('{}: batch * notes and batch * time must stay below 2 ** 31'.format(op))
  return x, note_mask, is_2d


def _pitch_2d(op, name, q):
  q = core.tf_float32(q)
  if q.dim() == 3:
    q = q[:, :, 0].contiguous()
  if q.dim() != 2:
    raise ValueError('{}: {} must be [batch, n_timesteps] or [batch, n_timesteps, 1], got {}'.format(op, name, tuple(q.shape)))
  if q.shape[1] < 2:
    raise ValueError('{}: needs at least 2 time steps (the reference returns a mask of the wrong length for fewer), got {}'
                     .format(op, q.shape[1]))
  return q.detach()


def _check_regions(op, max_regions):
  max_regions = int(max_regions)
  if max_regions < 1:
    raise ValueError('{}: max_regions must be at least 1, got {}'.format(op, max_regions))
  return max_regions


# Masking ----------------------------------------------------------------------
def get_note_mask(q_pitch, max_regions=100, note_on_only=True):
  """Get a binary mask for each note from a monophonic instrument (ddsp/training/nn.py:375-425).

  Each transition of the q_pitch value creates a new region. Returns the mask of each region, written by one kernel.
  The reference's edge rule is kept exactly (:398-411): step 0 starts region 0; step p in 1 .. t - 2 starts a region when
  |q[p] - q[p - 1]| > 0; THE LAST STEP NEVER STARTS ONE - it joins the region before it even when its pitch differs, so a
  region need not be constant.  Steps whose region index is >= max_regions get an all-zero row.  No gradient flows through
  the mask: a q_pitch that requires grad gives a mask that does not.  Non-finite pitches are outside the contract.

  Args:
    q_pitch: A quantized value, such as pitch or velocity. Shape [batch, n_timesteps] or [batch, n_timesteps, 1];
      n_timesteps >= 2 (ValueError otherwise).
    max_regions: Maximum number of note regions to consider in the sequence. Also, the channel dimension of the output
      mask. Each value transition defines a new region, e.g. each note-on and note-off count as a separate region.
      At most 1024 (NotImplementedError).
    note_on_only: Return a mask that is true only for regions where the pitch is greater than 0: the region's mean pitch
      as get_note_moments gives it, i.e. the sign of the region's sum.

  Returns:
    A binary fp32 mask of each region [batch, n_timesteps, max_regions].
  """
  q_pitch = _pitch_2d('get_note_mask', 'q_pitch', q_pitch)
  max_regions = _check_regions('get_note_mask', max_regions)
  _check_limits(q_pitch.shape[0], q_pitch.shape[1], max_regions)
  return _run_mask(q_pitch, None, max_regions, note_on_only)


def get_note_mask_from_onset(q_pitch, onset, max_regions=100, note_on_only=True):
  """Get a binary mask for each note from a monophonic instrument (ddsp/training/nn.py:428-476).

  Each onset creates a new region: step 0 starts region 0, step p >= 1 advances the region index by int(onset[p])
  (truncation, as tf.cast).  Returns the mask of each region.  No gradient flows through it.  Non-finite values are outside
  the contract.

  Args:
    q_pitch: A quantized value, such as pitch or velocity. Shape [batch, n_timesteps] or [batch, n_timesteps, 1].
    onset: Binary onset in shape [batch, n_timesteps] or [batch, n_timesteps, 1]. 1 represents onset.
    max_regions: Maximum number of note regions to consider in the sequence. Also, the channel dimension of the output
      mask.  At most 1024 (NotImplementedError).
    note_on_only: Return a mask that is true only where the pitch is greater than 0 - per TIME STEP here (:470-474).

  Returns:
    A binary fp32 mask of each region [batch, n_timesteps, max_regions].
  """
  q_pitch = _pitch_2d('get_note_mask_from_onset', 'q_pitch', q_pitch)
  onset = _pitch_2d('get_note_mask_from_onset', 'onset', onset)
  if q_pitch.shape != onset.shape:
    raise ValueError('get_note_mask_from_onset: q_pitch {} and onset {} must have equal shapes'.format(
        tuple(q_pitch.shape), tuple(onset.shape)))
  max_regions = _check_regions('get_note_mask_from_onset', max_regions)
  _check_limits(q_pitch.shape[0], q_pitch.shape[1], max_regions)
  return _run_mask(q_pitch, onset, max_regions, note_on_only)


def get_note_lengths(note_mask):
  """Count the lengths of each note [batch, time, notes] -> [batch, notes] (a framework sum)."""
  return core.tf_float32(note_mask).sum(1)


def get_note_moments(x, note_mask, return_std=True):
  """Return the moments of value xm, pooled over the length of the note (ddsp/training/nn.py:484-520).

  mean = sum_t m x / L and std = sqrt(sum_t (m (x - mean)) ** 2 / L), L = sum_t m with core.safe_divide's rule (a zero
  length becomes 1e-7: an empty region has mean 0 and std 0) - exact for any fp32 mask, summed in fp64 in ascending time, the
  variance in the reference's two-pass form.  Differentiable in x; where a note's variance in a dimension is exactly 0 the
  std contributes 0 to the gradient there (see the module's docstring).  The mask may not require grad.

  Args:
    x: Value to be pooled, [batch, time, dims] or [batch, time].
    note_mask: Binary mask of notes [batch, time, notes].
    return_std: Also return the standard deviation for each note.

  Returns:
    Values pooled over each note region, [batch, notes, dims] or [batch, notes].
    Returns only mean if return_std=False, else mean and std.
  """
  x, note_mask, is_2d = _x_and_mask('get_note_moments', x, note_mask, True)
  out = _moments(x, note_mask, bool(return_std))
  if return_std:
    return (out[0][:, :, 0], out[1][:, :, 0]) if is_2d else out
  return out[:, :, 0] if is_2d else out


def pool_over_notes(x, note_mask, return_std=True):
  """Return the time-distributed average value of x pooled over the note (ddsp/training/nn.py:523-547).

  pooled[b, t, :] = sum_n m[b, t, n] moment[b, n, :]: the moments of get_note_moments, handed back to the steps of each note.
  Differentiable in x, with the module's rule for a variance of exactly 0.

  Args:
    x: Value to be pooled, [batch, time, dims].
    note_mask: Binary mask of notes [batch, time, notes].
    return_std: Also return the standard deviation for each note.

  Returns:
    Values pooled over each note region, [batch, time, dims].
    Returns only mean if return_std=False, else mean and std.
  """
  x, note_mask, _ = _x_and_mask('pool_over_notes', x, note_mask, False)
  if return_std:
    x_notes, x_notes_std = _moments(x, note_mask, True)
    return _spread(x_notes, note_mask), _spread(x_notes_std, note_mask)
  return _spread(_moments(x, note_mask, False), note_mask)


def get_short_note_loss_mask(note_mask, note_lengths, note_pitches, min_length=40):
  """Creates a 1-D binary mask for notes shorter than min_length (ddsp/training/nn.py:550-557): [batch, time].

  sum_n m[b, t, n] * (note_lengths[b, n] < min_length and note_pitches[b, n] > 0); no gradient flows through it."""
  note_mask = core.tf_float32(note_mask).detach()
  note_lengths, note_pitches = core.tf_float32(note_lengths).detach(), core.tf_float32(note_pitches).detach()
  if note_mask.dim() != 3:
    raise ValueError('get_short_note_loss_mask: note_mask must be [batch, time, notes], got {}'.format(tuple(note_mask.shape)))
  want = (note_mask.shape[0], note_mask.shape[2])
  if tuple(note_lengths.shape) != want or tuple(note_pitches.shape) != want:
    raise ValueError('get_short_note_loss_mask: note_lengths {} and note_pitches {} must be [batch, notes] = {}'.format(
        tuple(note_lengths.shape), tuple(note_pitches.shape), want))
  if min(note_mask.shape[1:]) < 1:
    raise ValueError('get_short_note_loss_mask: time and notes must be at least 1, got {}'.format(tuple(note_mask.shape)))
  short_notes = ((note_lengths < min_length) & (note_pitches > 0.0)).to(torch.float32)
  return _run_spread(note_mask, short_notes[:, :, None].contiguous())[:, :, 0]


# ------------------ the layers of RnnFcDecoder ------------------------------------------------------------------------
class DictLayer(torch.nn.Module):
  """Wrap a layer to take dictionary inputs and outputs (ddsp/training/nn.py:48-246).

  A subclass writes `call(self, a, b, c=None) -> ['x', 'y']`; all return values are converted to a dictionary, even if
  call() returns a tuple.  Without input_keys / output_keys they are inferred from call()'s argument names and return
  annotation; arguments with defaults become default_input_keys, looked up in the input dictionaries but not required."""

  def __init__(self, input_keys=None, output_keys=None, **kwargs):
    name = kwargs.pop('name', None)
    if kwargs:
      raise TypeError('DictLayer: unknown arguments {}'.format(sorted(kwargs)))
    super().__init__()
    self.name = name
    if not input_keys:
      input_keys = self.get_argument_names('call')
      self.default_input_keys = list(self.get_default_argument_names('call'))
      self.default_input_values = list(self.get_default_argument_values('call'))
    else:
      # Manually specifying input keys overwrites default arguments.
      self.default_input_keys = []
      self.default_input_values = []
    output_keys = output_keys or self.get_return_annotations('call')
    self.input_keys = list(input_keys)
    self.output_keys = list(output_keys)

  @property
  def all_input_keys(self):
    """Full list of inputs and outputs."""
    return self.input_keys + self.default_input_keys

  @property
  def n_inputs(self):
    """Dynamically computed in case input_keys is changed in subclass init."""
    return len(self.all_input_keys)

  def forward(self, *inputs, **kwargs):
    return self.call(*inputs, **kwargs)

  def __call__(self, *inputs, **kwargs):
    """Any dict among `inputs` is merged and input_keys are read out of it ('a/b' looks up nested dicts); tensor arguments come
    first, then the looked-up keys, then defaults.  Returns call()'s dict, or its outputs under output_keys."""
    input_dict = {}
    for v in inputs:
      if isinstance(v, dict):
        input_dict.update(v)
    inputs = [v for v in inputs if not isinstance(v, dict)]
    for key in self.all_input_keys:
      if key in kwargs:
        input_dict[key] = kwargs[key]
    kwargs = {k: v for k, v in kwargs.items() if k not in self.all_input_keys}
    for key in self.input_keys:
      try:
        inputs.append(core.nested_lookup(key, input_dict))
      except KeyError:
        pass
    for key, value in zip(self.default_input_keys, self.default_input_values):
      try:
        inputs.append(core.nested_lookup(key, input_dict))
      except KeyError:
        if len(inputs) < self.n_inputs:
          inputs.append(value)
    if len(inputs) != self.n_inputs:
      raise TypeError(f'{len(inputs)} input tensors extracted from inputs'
                      '(including default args) but the layer expects '
                      f'{self.n_inputs} tensors.\n'
                      f'Input keys: {self.input_keys}\n'
                      f'Default keys: {self.default_input_keys}\n'
                      f'Default values: {self.default_input_values}\n'
                      f'Input dictionaries: {input_dict}\n'
                      f'Input Tensors (Args, Dicts, and Defaults): {inputs}\n')
    outputs = super().__call__(*inputs, **kwargs)
    if isinstance(outputs, dict):
      return outputs
    outputs = core.make_iterable(outputs)
    if len(self.output_keys) != len(outputs):
      raise ValueError(f'Output keys ({self.output_keys}) must have the same'
                       f'length as outputs ({outputs})')
    return dict(zip(self.output_keys, outputs))

  def get_argument_names(self, method):
    """Get list of strings for names of required arguments to method."""
    spec = inspect.getfullargspec(getattr(self, method))
    if spec.defaults:
      return spec.args[1:-len(spec.defaults)]
    return spec.args[1:]

  def get_default_argument_names(self, method):
    """Get list of strings for names of default arguments to method."""
    spec = inspect.getfullargspec(getattr(self, method))
    return spec.args[-len(spec.defaults):] if spec.defaults else []

  def get_default_argument_values(self, method):
    """Get list of default values of the default arguments to method."""
    spec = inspect.getfullargspec(getattr(self, method))
    return spec.defaults if spec.defaults else []

  def get_return_annotations(self, method):
    """Get list of strings of return annotations of method."""
    spec = inspect.getfullargspec(getattr(self, method))
    return core.make_iterable(spec.annotations['return'])


# ------------------------ Shapes ----------------------------------------------
def ensure_4d(x):
  """Add extra dimensions to make sure tensor has height and width."""
  if x.dim() == 2:
    return x[:, None, None, :]
  if x.dim() == 3:
    return x[:, :, None, :]
  return x


def inv_ensure_4d(x, n_dims):
  """Remove excess dims, inverse of ensure_4d() function."""
  if n_dims == 2:
    return x[:, 0, 0, :]
  if n_dims == 3:
    return x[:, :, 0, :]
  return x


# ------------------ Utilities -------------------------------------------------
def split_to_dict(tensor, tensor_splits):
  """Split a tensor into a dictionary of multiple tensors."""
  labels = [v[0] for v in tensor_splits]
  sizes = [int(v[1]) for v in tensor_splits]
  return dict(zip(labels, torch.split(tensor, sizes, dim=-1)))


NONLINEARITIES = {
    'leaky_relu': lambda x: torch.nn.functional.leaky_relu(x, 0.2),       # tf.nn.leaky_relu's slope
    'relu': torch.relu,
    'sigmoid': torch.sigmoid,
    'tanh': torch.tanh,
    'linear': lambda x: x,
}


def _activation_code(nonlinearity):
  if nonlinearity not in _lib.ACTIVATIONS:
    raise ValueError('nonlinearity {!r} is not supported; supported: {}'.format(nonlinearity, sorted(_lib.ACTIVATIONS)))
  return _lib.ACTIVATIONS[nonlinearity]


def get_nonlinearity(nonlinearity):
  """Get nonlinearity function by name: 'leaky_relu' (slope 0.2), 'relu', 'sigmoid', 'tanh', 'linear' (framework ops; the Fc
  layers run the same functions inside their kernel)."""
  _activation_code(nonlinearity)
  return NONLINEARITIES[nonlinearity]


_norm_ws = core.Workspace()
_gru_ws = core.Workspace()
LAYER_NORM_EPSILON = 1e-3            # tf.keras.layers.LayerNormalization's default


def _decoder_entry(name):
  return _lib.decoder_entry(_lib.load(), name)


def _checked(rc, what):
  if rc == _lib.ERR_UNSUPPORTED:
    raise ValueError('{}: beyond the limits of the MI355X path (DDSP_ERR_UNSUPPORTED)'.format(what))
  _lib.check(rc, what)


class _BiasNormActFunction(torch.autograd.Function):
  """torch.autograd node of act(gamma * LayerNorm(x + bias) + beta) over the last axis of x [rows, ch] (plumbing: both
  directions are C-ABI calls).  Kept for the backward: xhat, rstd, gamma, beta."""

  @staticmethod
  def forward(ctx, x, bias, gamma, beta, act, eps):
    needs = not isinstance(ctx, core._NoCtx)
    rows, ch = x.shape
    y = torch.empty_like(x)
    xhat = torch.empty_like(x) if needs else None
    rstd = torch.empty((rows,), dtype=torch.float32, device=x.device) if needs else None
    ptr = lambda t: None if t is None else t.data_ptr()
    rc = _decoder_entry('ddsp_bias_norm_act_f32')(x.data_ptr(), bias.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(),
                                                  ptr(xhat), ptr(rstd), rows, ch, act, eps, core._stream())
    _checked(rc, 'ddsp_bias_norm_act_f32')
    ctx.save_for_backward(xhat, rstd, gamma, beta)
    ctx.act = act
    return y

  @staticmethod
  def backward(ctx, grad_y):
    xhat, rstd, gamma, beta = ctx.saved_tensors
    rows, ch = xhat.shape
    grad_y = core.tf_float32(grad_y)
    dx = torch.empty_like(xhat)
    dparams = torch.empty((3, ch), dtype=torch.float32, device=xhat.device)
    ws = _norm_ws.get(_decoder_entry('ddsp_bias_norm_act_backward_workspace_bytes')(rows, ch), xhat.device)
    rc = _decoder_entry('ddsp_bias_norm_act_backward_f32')(grad_y.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
                                                           beta.data_ptr(), dx.data_ptr(), dparams.data_ptr(), ws.data_ptr(), ws.numel(),
                                                           rows, ch, ctx.act, core._stream())
    _checked(rc, 'ddsp_bias_norm_act_backward_f32')
    return dx, dparams[2], dparams[0], dparams[1], None, None


def bias_norm_act(x, bias, gamma, beta, nonlinearity='linear', epsilon=LAYER_NORM_EPSILON):
  """nonlinearity(gamma * (v - mean(v)) / sqrt(var(v) + epsilon) + beta), v = x + bias, moments over the last axis (biased
  variance, two passes): one kernel each way instead of the dozen elementwise and reduction ops of the framework chain.
  Differentiable in x, bias, gamma and beta; a row of equal values gives xhat = 0 and a finite gradient."""
  act = _activation_code(nonlinearity)
  x, bias, gamma, beta = core.tf_float32(x), core.tf_float32(bias), core.tf_float32(gamma), core.tf_float32(beta)
  ch = x.shape[-1] if x.dim() else 0
  if x.dim() < 1 or ch < 1 or tuple(bias.shape) != (ch,) or tuple(gamma.shape) != (ch,) or tuple(beta.shape) != (ch,):
    raise ValueError('bias_norm_act: x must be [..., ch] with ch >= 1 and bias, gamma, beta [ch], got {}, {}, {}, {}'.format(
        tuple(x.shape), tuple(bias.shape), tuple(gamma.shape), tuple(beta.shape)))
  flat = x.reshape(-1, ch)
  if core._needs_grad(flat, bias, gamma, beta):
    y = _BiasNormActFunction.apply(flat, bias, gamma, beta, act, float(epsilon))
  else:
    y = _BiasNormActFunction.forward(core._NoCtx(), flat, bias, gamma, beta, act, float(epsilon))
  return y.reshape(x.shape)


class _GruFunction(torch.autograd.Function):
  """torch.autograd node of the recurrence: (mx [b, t, 3 H], recurrent_kernel [H, 3 H], recurrent bias [3 H], h0 [b, H]) ->
  y [b, t, H].  Both scans are C-ABI calls, one launch per step; the recurrent weight gradients are matrix products over all
  steps at once.  Kept for the backward: y, h0, the recurrent kernel and z, r, hh, mh_h of every step (batch * time * 4 H floats)."""

  @staticmethod
  def forward(ctx, mx, rk, rb, h0):
    needs = not isinstance(ctx, core._NoCtx)
    b, t, h3 = mx.shape
    h = h3 // 3
    y = torch.empty((b, t, h), dtype=torch.float32, device=mx.device)
    saved = torch.empty((4, b, t, h), dtype=torch.float32, device=mx.device) if needs else None
    if b:
      ws = _gru_ws.get(_decoder_entry('ddsp_gru_forward_workspace_bytes')(b, h), mx.device)
      rc = _decoder_entry('ddsp_gru_forward_f32')(mx.data_ptr(), rk.data_ptr(), rb.data_ptr(), h0.data_ptr(), y.data_ptr(),
                                                  None if saved is None else saved.data_ptr(), ws.data_ptr(), ws.numel(), b, t, h,
                                                  core._stream())
      _checked(rc, 'ddsp_gru_forward_f32')
    ctx.save_for_backward(y, h0, saved, rk)
    return y

  @staticmethod
  def backward(ctx, grad_y):
    y, h0, saved, rk = ctx.saved_tensors
    b, t, h = y.shape
    grad_y = core.tf_float32(grad_y)
    d_in = torch.empty((b, t, 3 * h), dtype=torch.float32, device=y.device)
    d_rec = torch.empty_like(d_in)
    dh0 = torch.empty_like(h0)
    if b:
      ws = _gru_ws.get(_decoder_entry('ddsp_gru_backward_workspace_bytes')(b, h), y.device)
      rc = _decoder_entry('ddsp_gru_backward_f32')(grad_y.data_ptr(), y.data_ptr(), h0.data_ptr(), saved.data_ptr(), rk.data_ptr(),
                                                   d_in.data_ptr(), d_rec.data_ptr(), dh0.data_ptr(), ws.data_ptr(), ws.numel(), b, t, h,
                                                   core._stream())
      _checked(rc, 'ddsp_gru_backward_f32')
    h_prev = torch.cat([h0[:, None, :], y[:, :-1, :]], dim=1).reshape(b * t, h)
    flat_rec = d_rec.reshape(b * t, 3 * h)
    return d_in, torch.matmul(h_prev.t(), flat_rec), flat_rec.sum(0), dh0


def gru_recurrence(mx, recurrent_kernel, recurrent_bias, initial_state=None):
  """The Keras GRU loop (reset_after=True, gates z, r, h) on a given input projection mx = x kernel + bias[0]:
  mh = h recurrent_kernel + recurrent_bias; z = sigmoid(mx_z + mh_z); r = sigmoid(mx_r + mh_r); hh = tanh(mx_h + r mh_h);
  h' = z h + (1 - z) hh.  -> all states [batch, time, H].  Differentiable in every argument.  One launch per step each way; the
  same bits on every run and for any subset of the batch rows.  H up to 2048 (ValueError beyond); on the matrix-core path
  (H a multiple of 16) the initial state must lie inside fp16's range."""
  mx, rk, rb = core.tf_float32(mx), core.tf_float32(recurrent_kernel), core.tf_float32(recurrent_bias)
  if mx.dim() != 3 or mx.shape[1] < 1 or mx.shape[2] < 3 or mx.shape[2] % 3:
    raise ValueError('gru_recurrence: mx must be [batch, time >= 1, 3 H], got {}'.format(tuple(mx.shape)))
  b, _, h3 = mx.shape
  h = h3 // 3
  if tuple(rk.shape) != (h, h3) or tuple(rb.shape) != (h3,):
    raise ValueError('gru_recurrence: recurrent_kernel must be [H, 3 H] and recurrent_bias [3 H] for H = {}, got {} and {}'.format(
        h, tuple(rk.shape), tuple(rb.shape)))
  if h > _lib.GRU_MAX_HIDDEN:
    raise ValueError('gru_recurrence: at most {} units on the MI355X path, got {}'.format(_lib.GRU_MAX_HIDDEN, h))
  if initial_state is None:
    h0 = torch.zeros((b, h), dtype=torch.float32, device=mx.device)
  else:
    h0 = core.tf_float32(initial_state)
    if tuple(h0.shape) != (b, h):
      raise ValueError('gru_recurrence: the initial state must be [batch, H] = {}, got {}'.format((b, h), tuple(h0.shape)))
  if core._needs_grad(mx, rk, rb, h0):
    return _GruFunction.apply(mx, rk, rb, h0)
  return _GruFunction.forward(core._NoCtx(), mx, rk, rb, h0)


def _glorot_uniform(fan_in, fan_out):
  limit = math.sqrt(6.0 / (fan_in + fan_out))
  return torch.empty((fan_in, fan_out), dtype=torch.float32).uniform_(-limit, limit)


class _Lazy(torch.nn.Module):
  """Weights are made on the first call, when the input width is known, or by build(in_ch)."""

  def __init__(self):
    super().__init__()
    self.built = False

  def _ensure_built(self, in_ch):
    if not self.built:
      self.build(int(in_ch))

  def _param(self, value):
    return torch.nn.Parameter(value.to(core._device()))


class Dense(_Lazy):
  """tf.keras.layers.Dense(units): x kernel + bias; kernel [in, out] glorot-uniform, bias [out] zeros.  The product is
  torch.addmm (plumbing)."""

  def __init__(self, units):
    super().__init__()
    self.units = int(units)

  def build(self, in_ch):
    self.kernel = self._param(_glorot_uniform(in_ch, self.units))
    self.bias = self._param(torch.zeros(self.units))
    self.built = True

  def project(self, x):
    """x kernel, without the bias (Fc's kernel adds it): [..., in] -> [rows, out]."""
    x = core.aligned16(core.tf_float32(x))           # the framework's product may not pick its kernel by the address
    self._ensure_built(x.shape[-1])
    return torch.matmul(x.reshape(-1, x.shape[-1]), self.kernel), x.shape[:-1] + (self.units,)

  def forward(self, x):
    flat, shape = self.project(x)
    return (flat + self.bias).reshape(shape)


class LayerNormalization(_Lazy):
  """tf.keras.layers.LayerNormalization() over the last axis: gamma (ones), beta (zeros), epsilon 1e-3, biased variance."""

  def __init__(self, epsilon=LAYER_NORM_EPSILON):
    super().__init__()
    self.epsilon = float(epsilon)

  def build(self, in_ch):
    self.gamma = self._param(torch.ones(in_ch))
    self.beta = self._param(torch.zeros(in_ch))
    self.built = True

  def forward(self, x):
    x = core.tf_float32(x)
    self._ensure_built(x.shape[-1])
    return bias_norm_act(x, torch.zeros_like(self.beta), self.gamma, self.beta, 'linear', self.epsilon)


class GRU(_Lazy):
  """tf.keras.layers.GRU(units, return_sequences, return_state): kernel [in, 3 H] glorot-uniform, recurrent_kernel [H, 3 H]
  orthogonal, bias [2, 3 H] zeros (row 0 input bias, row 1 recurrent bias), gates z, r, h, reset_after=True, zero initial state
  unless one is given.  The input projection of all steps is one torch.addmm; the recurrence is gru_recurrence."""

  def __init__(self, units, return_sequences=False, return_state=False):
    super().__init__()
    self.units = int(units)
    self.return_sequences = bool(return_sequences)
    self.return_state = bool(return_state)

  def build(self, in_ch):
    h = self.units
    self.kernel = self._param(_glorot_uniform(in_ch, 3 * h))
    self.recurrent_kernel = self._param(torch.nn.init.orthogonal_(torch.empty((h, 3 * h), dtype=torch.float32)))
    self.bias = self._param(torch.zeros((2, 3 * h)))
    self.built = True

  def forward(self, x, initial_state=None):
    x = core.aligned16(core.tf_float32(x))
    if x.dim() != 3:
      raise ValueError('GRU: x must be [batch, time, channels], got {}'.format(tuple(x.shape)))
    self._ensure_built(x.shape[-1])
    b, t, ch = x.shape
    mx = torch.addmm(self.bias[0], x.reshape(b * t, ch), self.kernel).reshape(b, t, 3 * self.units)
    y = gru_recurrence(mx, self.recurrent_kernel, self.bias[1], initial_state)
    state = y[:, -1, :]
    out = y if self.return_sequences else state
    return (out, state) if self.return_state else out


# ------------------ Normalization ---------------------------------------------
_group_norm_ws = core.Workspace()
NORMALIZE_EPSILON = 1e-5             # normalize_op's default


def _norm_entry(name):
  return _lib.norm_entry(_lib.load(), name)


class _GroupNormFunction(torch.autograd.Function):
  """torch.autograd node of group normalisation over x [N, S, C] with optional scale / shift [C] (plumbing: both directions are
  C-ABI calls).  Kept for the backward: x, scale and the [N, G] means and rstds - no activation-sized xhat."""

  @staticmethod
  def forward(ctx, x, scale, shift, groups, eps):
    needs = not isinstance(ctx, core._NoCtx)
    n, s, c = x.shape
    y = torch.empty_like(x)
    mean = torch.empty((n, groups), dtype=torch.float32, device=x.device) if needs else None
    rstd = torch.empty((n, groups), dtype=torch.float32, device=x.device) if needs else None
    ptr = lambda t: None if t is None else t.data_ptr()
    if n:
      ws = _group_norm_ws.get(_norm_entry('ddsp_group_norm_workspace_bytes')(n, s, c, groups), x.device)
      rc = _norm_entry('ddsp_group_norm_f32')(x.data_ptr(), ptr(scale), ptr(shift), y.data_ptr(), ptr(mean), ptr(rstd), ws.data_ptr(),
                                              ws.numel(), n, s, c, groups, eps, core._stream())
      _checked(rc, 'ddsp_group_norm_f32')
    ctx.save_for_backward(x, scale, mean, rstd)
    ctx.groups = groups
    return y

  @staticmethod
  def backward(ctx, grad_y):
    x, scale, mean, rstd = ctx.saved_tensors
    n, s, c = x.shape
    grad_y = core.tf_float32(grad_y)
    dx = torch.empty_like(x)
    dscale = torch.empty_like(scale) if scale is not None else None
    dshift = torch.empty_like(scale) if scale is not None else None
    ptr = lambda t: None if t is None else t.data_ptr()
    ws = _group_norm_ws.get(_norm_entry('ddsp_group_norm_backward_workspace_bytes')(n, s, c, ctx.groups), x.device)
    rc = _norm_entry('ddsp_group_norm_backward_f32')(grad_y.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), ptr(scale),
                                                     dx.data_ptr(), ptr(dscale), ptr(dshift), ws.data_ptr(), ws.numel(), n, s, c,
                                                     ctx.groups, core._stream())
    _checked(rc, 'ddsp_group_norm_backward_f32')
    return dx, dscale, dshift, None, None


def _group_norm(x, norm_type, scale=None, shift=None, eps=NORMALIZE_EPSILON):
  """x [batch, h, w, ch] of any layout or dtype, scale / shift [ch] or None -> the normalised tensor, one kernel each way.  The
  arguments are checked before anything touches the device."""
  shape = tuple(x.shape) if hasattr(x, 'shape') else tuple(torch.as_tensor(x).shape)
  if len(shape) != 4:
    raise ValueError('normalize_op: x must be [batch, height, width, channels], got {}'.format(shape))
  b, h, w, ch = shape
  n_groups = {'instance': ch, 'layer': 1, 'group': 32}[norm_type]
  if min(h, w, ch) < 1:
    raise ValueError('normalize_op: height, width and channels must be at least 1, got {}'.format(shape))
  if ch % n_groups:
    raise ValueError("normalize_op: norm_type='group' takes channels in multiples of 32, got {}".format(ch))
  x = core.tf_float32(x)
  flat = x.reshape(b, h * w, ch)
  if core._needs_grad(flat, scale, shift):
    y = _GroupNormFunction.apply(flat, scale, shift, n_groups, float(eps))
  else:
    y = _GroupNormFunction.forward(core._NoCtx(), flat, scale, shift, n_groups, float(eps))
  return y.reshape(x.shape)


def normalize_op(x, norm_type='layer', eps=1e-5):
  """Apply either Group, Instance, or Layer normalization, or None (ddsp/training/nn.py:561-575).

  x [batch, height, width, channels] of any layout or dtype; moments (biased variance) over height, width and the channels of a
  group, per batch row: 'instance' has a group per channel, 'layer' one group, 'group' 32 groups of adjacent channels
  (ValueError unless channels is a multiple of 32); an unknown norm_type raises the reference's KeyError; None returns x.
  (x - mean) / sqrt(var + eps), one kernel of csrc/group_norm.hip each way.  Differentiable in x.  A group of equal values
  gives 0 and a finite gradient.  batch * height * width * channels must stay below 2 ** 31 (ValueError)."""
  if norm_type is None:
    return x
  return _group_norm(x, norm_type, eps=eps)


class Normalize(_Lazy):
  """Normalization layer with learnable parameters (ddsp/training/nn.py:578-603): normalize_op, then * scale + shift, fused into
  the one kernel.  Weights: scale (ones) and shift (zeros), both [1, 1, 1, ch] as Keras holds them."""

  def __init__(self, norm_type='layer'):
    super().__init__()
    self.norm_type = norm_type

  def build(self, in_ch):
    self.scale = self._param(torch.ones((1, 1, 1, in_ch)))
    self.shift = self._param(torch.zeros((1, 1, 1, in_ch)))
    self.built = True

  def forward(self, x):
    x = core.tf_float32(x)
    self._ensure_built(x.shape[-1])
    n_dims = x.dim()
    x = ensure_4d(x)
    if self.norm_type is not None:
      x = _group_norm(x, self.norm_type, self.scale.reshape(-1), self.shift.reshape(-1))
    else:
      x = (x * self.scale) + self.shift
    return inv_ensure_4d(x, n_dims)


class ConditionalScaleAndShift(_Lazy):
  """Conditional scaling and shifting after normalization (ddsp/training/nn.py:1075-1099): (x, z) -> x * scale(z) + shift(z),
  or x + shift(z) with shift_only; scale and shift are the halves of one Dense of z.  Framework ops."""

  def __init__(self, shift_only=False):
    super().__init__()
    self.shift_only = shift_only
    self.dense = None

  def build(self, in_ch):
    self.x_ch = int(in_ch)
    self.dense = Dense(self.x_ch if self.shift_only else 2 * self.x_ch)
    self.built = True

  def forward(self, inputs):
    x, z = inputs
    self._ensure_built(x.shape[-1])
    if self.shift_only:
      return x + self.dense(z)
    scale_shift = self.dense(z)
    return (x * scale_shift[..., :self.x_ch]) + scale_shift[..., self.x_ch:]


class ConditionalNorm(torch.nn.Module):
  """Apply normalization and then conditional scale and shift (ddsp/training/nn.py:1102-1136).

  inputs: the pair (x [batch, height, width, ch], z broadcastable to it); norm_type 'group', 'instance' or 'layer'."""

  def __init__(self, norm_type='instance', shift_only=False):
    super().__init__()
    self.norm_type = norm_type
    self.conditional_scale_and_shift = ConditionalScaleAndShift(shift_only=shift_only)

  def forward(self, inputs):
    x, z = inputs
    x = normalize_op(x, norm_type=self.norm_type)
    return self.conditional_scale_and_shift([x, z])


def get_norm(norm_type, conditional, shift_only):
  """Helper function to get conditional norm if needed."""
  if conditional:
    return ConditionalNorm(norm_type=norm_type, shift_only=shift_only)
  return Normalize(norm_type)


class Identity(torch.nn.Module):
  """Utility identity layer."""

  def forward(self, x):
    return x


# ------------------ Embeddings ------------------------------------------------
class Embedding(_Lazy):
  """tf.keras.layers.Embedding(input_dim, output_dim): weight `embeddings` [input_dim, output_dim], uniform in +-0.05; integer ids of
  any shape -> [..., output_dim], a framework gather."""

  def __init__(self, input_dim, output_dim):
    super().__init__()
    self.input_dim, self.output_dim = int(input_dim), int(output_dim)

  def build(self, unused_in_ch=None):
    self.embeddings = self._param(torch.empty((self.input_dim, self.output_dim), dtype=torch.float32).uniform_(-0.05, 0.05))
    self.built = True

  def forward(self, ids):
    if not self.built:
      self.build()
    ids = torch.as_tensor(ids).to(device=self.embeddings.device, dtype=torch.long)
    return torch.nn.functional.embedding(ids, self.embeddings)


def get_embedding(vocab_size=1024, n_dims=256):
  """Get a real-valued embedding from an integer."""
  return Embedding(input_dim=vocab_size, output_dim=n_dims)


# ---------------- Stacks ------------------------------------------------------
class _Sequential(torch.nn.Module):
  def __init__(self, layers):
    super().__init__()
    self.layers = torch.nn.ModuleList(layers)

  def forward(self, x):
    for layer in self.layers:
      x = layer(x)
    return x


class Fc(_Lazy):
  """Makes a Dense -> LayerNorm -> Leaky ReLU layer (ddsp/training/nn.py:844-853): torch.matmul, then ONE kernel for
  bias + LayerNorm + activation.  Weights: dense.kernel, dense.bias, layer_norm.gamma, layer_norm.beta."""

  def __init__(self, ch=128, nonlinearity='leaky_relu'):
    super().__init__()
    _activation_code(nonlinearity)
    self.nonlinearity = nonlinearity
    self.dense = Dense(ch)
    self.layer_norm = LayerNormalization()

  def build(self, in_ch):
    self.dense.build(in_ch)
    self.layer_norm.build(self.dense.units)
    self.built = True

  def forward(self, x):
    x = core.tf_float32(x)
    self._ensure_built(x.shape[-1])
    flat, shape = self.dense.project(x)
    return bias_norm_act(flat, self.dense.bias, self.layer_norm.gamma, self.layer_norm.beta, self.nonlinearity,
                         self.layer_norm.epsilon).reshape(shape)


class FcStack(_Sequential):
  """Stack Dense -> LayerNorm -> Leaky ReLU layers."""

  def __init__(self, ch=256, layers=2, nonlinearity='leaky_relu'):
    super().__init__([Fc(ch, nonlinearity) for _ in range(layers)])


def _gru_only(rnn_type, bidir=False):
  if rnn_type not in ('gru', 'lstm'):
    raise ValueError("rnn_type must be 'gru' or 'lstm', got {!r}".format(rnn_type))
  if rnn_type == 'lstm':
    raise ValueError("rnn_type='lstm' is not built on the MI355X path; only 'gru' is")
  if bidir:
    raise ValueError('bidir=True is not built on the MI355X path; only the forward GRU is')


class Rnn(torch.nn.Module):
  """Single RNN layer (ddsp/training/nn.py:866-879).  Only rnn_type='gru' with bidir=False is built (ValueError otherwise)."""

  def __init__(self, dims, rnn_type, return_sequences=True, bidir=False):
    super().__init__()
    _gru_only(rnn_type, bidir)
    self.rnn = GRU(dims, return_sequences=return_sequences)

  def forward(self, x):
    return self.rnn(x)


class StatelessRnn(torch.nn.Module):
  """Stateless unidirectional RNN for streaming models (ddsp/training/nn.py:883-904)."""

  def __init__(self, dims, rnn_type):
    super().__init__()
    _gru_only(rnn_type)
    self.rnn = GRU(dims, return_sequences=True, return_state=True)

  def forward(self, x, state):
    """x [batch, T, dims_in], state [batch, dims] (the last output) -> y [batch, T, dims], new_state [batch, dims]."""
    y, new_state = self.rnn(x, initial_state=state)
    return y, new_state


class RnnFc(_Sequential):
  """RNN layer -> fully connected -> LayerNorm -> Activation fn (ddsp/training/nn.py:908-916).  The reference hands `bidir` to
  Rnn's third positional argument, which is return_sequences; here it goes where its name says and every Rnn returns sequences."""

  def __init__(self, rnn_feat, out_feat, rnn_type='lstm', nonlinearity='sigmoid', bidir=False, n_rnn=1):
    layers = [Rnn(rnn_feat, rnn_type, bidir=bidir) for _ in range(n_rnn)]
    layers.append(Fc(out_feat, nonlinearity=nonlinearity))
    super().__init__(layers)


class RnnSandwich(_Sequential):
  """RNN Sandwiched by two FC Stacks."""

  def __init__(self, fc_stack_ch=256, fc_stack_layers=2, rnn_ch=512, rnn_type='gru'):
    super().__init__([FcStack(fc_stack_ch, fc_stack_layers), Rnn(rnn_ch, rnn_type), FcStack(fc_stack_ch, fc_stack_layers)])


class SingleGru(_Sequential):
  """GRU(gru_dim, return_sequences=True) -> LayerNormalization (ddsp/training/nn.py:1141-1149)."""

  def __init__(self, gru_dim=128):
    super().__init__([GRU(gru_dim, return_sequences=True), LayerNormalization()])


# ------------------ Resampling ------------------------------------------------
def polyphase_resample(x, stride=2, resample_type='down', trim_or_pad='pad'):
  """Resample by 'space_to_depth' conversion of time and channels (ddsp/training/nn.py:615-675).

    Downsampling: [batch, time, ch] --> [batch, time/stride, ch*stride]
    Upsampling:   [batch, time, ch] --> [batch, time*stride, ch/stride]

  A pad or a trim and a reshape: framework ops on the tensor's own device (host tensors too), differentiable by themselves.  As in
  the reference, anything but 'pad' trims - the end of time going down, the last channels going up.

  Args:
    x: [batch, time, ch] or [batch, time, 1, ch].
    stride: Amount to resample by.
    resample_type: 'up' or 'down'.
    trim_or_pad: 'trim' or 'pad'. What to do if time or channels cannot be evenly divided by stride.

  Returns:
    A resampled tensor, of x's rank.
  """
  x = torch.as_tensor(x)
  is_4d = x.dim() == 4
  if is_4d:
    x = x[:, :, 0, :]
  n_time, n_ch = x.shape[1], x.shape[2]
  if resample_type == 'down':
    if trim_or_pad == 'pad':
      pad = (stride - n_time % stride) % stride
      x = torch.nn.functional.pad(x, (0, 0, 0, pad)) if pad > 0 else x
    else:
      trim = n_time % stride
      x = x[:, :-trim, :] if trim > 0 else x
    n_time = x.shape[1]
    x_reshape = x.reshape(-1, n_time // stride, n_ch * stride)
  elif resample_type == 'up':
    if trim_or_pad == 'pad':
      pad = (stride - n_ch % stride) % stride
      x = torch.nn.functional.pad(x, (0, pad)) if pad > 0 else x
    else:
      trim = n_ch % stride
      if trim > 0:
        x = x[:, :, :-trim]
    n_ch = x.shape[2]
    x_reshape = x.reshape(-1, n_time * stride, n_ch // stride)
  else:
    raise ValueError('`resample_type` must be either "up" or "down"')
  return x_reshape[:, :, None, :] if is_4d else x_reshape


class PolyphaseResample(torch.nn.Module):
  """Resample by interleaving time and channels (ddsp/training/nn.py:679-694)."""

  def __init__(self, stride=2, resample_type='down', trim_or_pad='pad'):
    super().__init__()
    self.stride = stride
    self.resample_type = resample_type
    self.trim_or_pad = trim_or_pad

  def forward(self, x):
    return polyphase_resample(x, self.stride, self.resample_type, self.trim_or_pad)


# ------------------ Dilated convolutions --------------------------------------
_conv_ws = core.Workspace()


def _conv_entry(name):
  return _lib.conv_entry(_lib.load(), name)


def same_pad_left(kernel_size, dilation):
  """Rows of zeros TF's 'same' padding puts in FRONT of a stride-1 convolution: the total is (kernel_size - 1) * dilation and
  the odd one goes behind (tensorflow/core/framework/kernel_shape_util.cc GetWindowedOutputSizeVerbose: pad_before = total / 2)."""
  return ((int(kernel_size) - 1) * int(dilation)) // 2


def _run_dilated_conv(x, kernel, bias, dilation, pad_left, flags, mask_src=None, addend=None):
  """One ddsp_dilated_conv_f32 call on contiguous fp32 tensors: x [b, t, ch_in] -> [b, t, ch_out]; kernel [K, ch_in, ch_out], or
  [K, ch_out, ch_in] with CONVD_TRANSPOSE_W."""
  b, t, ch_in = x.shape
  taps = kernel.shape[0]
  ch_out = kernel.shape[1] if flags & _lib.CONVD_TRANSPOSE_W else kernel.shape[2]
  y = torch.empty((b, t, ch_out), dtype=torch.float32, device=x.device)
  if b:
    ptr = lambda v: None if v is None else v.data_ptr()
    ws = _conv_ws.get(_conv_entry('ddsp_dilated_conv_workspace_bytes')(b, t, ch_in, ch_out, taps), x.device)
    rc = _conv_entry('ddsp_dilated_conv_f32')(x.data_ptr(), kernel.data_ptr(), ptr(bias), ptr(addend), ptr(mask_src), y.data_ptr(),
                                              ws.data_ptr(), ws.numel(), b, t, ch_in, ch_out, taps, dilation, pad_left, flags,
                                              core._stream())
    _checked(rc, 'ddsp_dilated_conv_f32')
  return y


class _DilatedConvFunction(torch.autograd.Function):
  """torch.autograd node of the dilated convolution: (x [b, t, ch_in], kernel [K, ch_in, ch_out], bias [ch_out] or None) ->
  [b, t, ch_out].  Forward and the gradient in x are C-ABI calls (the same kernel; the adjoint takes the reversed, transposed taps
  and the mirrored padding, and multiplies by relu'(x) = (x > 0) in its epilogue).  The gradients whose reduction runs over
  batch * time are the framework's: K matrix products over views of one relu(x), and a column sum.  Kept for the backward: x and
  the kernel."""

  @staticmethod
  def forward(ctx, x, kernel, bias, dilation, relu_input):
    pad_left = same_pad_left(kernel.shape[0], dilation)
    y = _run_dilated_conv(x, kernel, bias, dilation, pad_left, _lib.CONVD_RELU_INPUT if relu_input else 0)
    ctx.save_for_backward(x, kernel)
    ctx.dilation, ctx.relu_input, ctx.has_bias = dilation, relu_input, bias is not None
    return y

  @staticmethod
  def backward(ctx, grad_y):
    x, kernel = ctx.saved_tensors
    taps, ch_in, ch_out = kernel.shape
    d, t = ctx.dilation, x.shape[1]
    pad_left = same_pad_left(taps, d)
    grad_y = core.tf_float32(grad_y)
    dx = dk = db = None
    if ctx.needs_input_grad[0]:
      flags = _lib.CONVD_TRANSPOSE_W | (_lib.CONVD_MASK_OUTPUT if ctx.relu_input else 0)
      dx = _run_dilated_conv(grad_y, kernel, None, d, (taps - 1) * d - pad_left, flags, mask_src=x if ctx.relu_input else None)
    if ctx.needs_input_grad[1]:
      a = torch.relu(x) if ctx.relu_input else x
      dk = torch.zeros_like(kernel)
      for k in range(taps):
        shift = k * d - pad_left                      # y[t] takes a[t + shift]
        lo, hi = max(0, -shift), min(t, t - shift)
        if hi > lo:
          dk[k] = torch.matmul(a[:, lo + shift:hi + shift].transpose(1, 2), grad_y[:, lo:hi]).sum(0)      # views: nothing is copied
    if ctx.has_bias and ctx.needs_input_grad[2]:
      db = grad_y.reshape(-1, ch_out).sum(0)
    return dx, dk, db, None, None


def dilated_conv(x, kernel, bias=None, dilation=1, relu_input=False):
  """A dilated 1-D convolution over time of a channel-last tensor, TF 'same' padding, stride 1 - tf.keras.layers.Conv2D(ch_out,
  (K, 1), dilation_rate=(dilation, 1), padding='same') on [batch, time, 1, ch_in] - with an optional ReLU on its input, in one
  kernel each way (csrc/dilated_conv.hip; C ABI csrc/conv_abi.h):

    y[b, t, co] = bias[co] + sum_k sum_ci act(x[b, t + k * dilation - pad_left, ci]) * kernel[k, ci, co]

  rows outside [0, time) contributing 0 and pad_left = same_pad_left(K, dilation).  ReLU is applied as x is loaded, the bias
  added as y is written; there is no padded copy and nothing of size [batch, time, K * ch_in].  ch_out in multiples of 16 runs on
  the matrix cores (fp16 hi / lo operands behind a power-of-two scale per batch row of x), every other width on the vector ALU.
  The same bits on every run, for a row alone and for any sub-batch.

  Args:
    x: [batch, time, ch_in] or [batch, time, 1, ch_in], of any layout or dtype.
    kernel: [K, ch_in, ch_out] or the Keras layout [K, 1, ch_in, ch_out].
    bias: [ch_out] or None.
    dilation: The dilation rate, >= 1.
    relu_input: Apply ReLU to x first (its gradient at 0 is 0, as tf.nn.relu's).

  Returns:
    [batch, time, ch_out], or [batch, time, 1, ch_out] for a 4-D x.  Differentiable in x, kernel and bias.

  Raises:
    ValueError: shapes that do not fit, or beyond the limits of the MI355X path - ch_in, ch_out <= 1024, K <= 16,
      (K - 1) * dilation < 2 ** 31, batch * time * channels < 2 ** 31.  Checked before anything touches the device.
  """
  x_shape = tuple(x.shape) if hasattr(x, 'shape') else tuple(torch.as_tensor(x).shape)
  k_shape = tuple(kernel.shape) if hasattr(kernel, 'shape') else tuple(torch.as_tensor(kernel).shape)
  is_4d = len(x_shape) == 4
  if len(x_shape) not in (3, 4) or (is_4d and x_shape[2] != 1):
    raise ValueError('dilated_conv: x must be [batch, time, ch_in] or [batch, time, 1, ch_in], got {}'.format(x_shape))
  if len(k_shape) not in (3, 4) or (len(k_shape) == 4 and k_shape[1] != 1):
    raise ValueError('dilated_conv: kernel must be [K, ch_in, ch_out] or [K, 1, ch_in, ch_out], got {}'.format(k_shape))
  batch, steps, ch_in = x_shape[0], x_shape[1], x_shape[-1]
  taps, ch_out = k_shape[0], k_shape[-1]
  dilation = int(dilation)
  if k_shape[-2] != ch_in or min(steps, ch_in, ch_out, taps) < 1:
    raise ValueError('dilated_conv: x {} and kernel {} must agree in ch_in, and time, K and the channels be at least 1'.format(
        x_shape, k_shape))
  if bias is not None and tuple(bias.shape) != (ch_out,):
    raise ValueError('dilated_conv: bias must be [ch_out] = {}, got {}'.format((ch_out,), tuple(bias.shape)))
  if dilation < 1:
    raise ValueError('dilated_conv: dilation must be at least 1, got {}'.format(dilation))
  if max(ch_in, ch_out) > _lib.CONVD_MAX_CHANNELS or taps > _lib.CONVD_MAX_TAPS:
    raise ValueError('dilated_conv: at most {} channels and {} taps on the MI355X path, got ch_in = {}, ch_out = {}, K = {}'.format(
        _lib.CONVD_MAX_CHANNELS, _lib.CONVD_MAX_TAPS, ch_in, ch_out, taps))
  if (taps - 1) * dilation >= 2 ** 31 or batch * steps * max(ch_in, ch_out) >= 2 ** 31:
    raise ValueError('dilated_conv: (K - 1) * dilation and batch * time * channels must stay below 2 ** 31, got x {}, kernel {}, '
                     'dilation {}'.format(x_shape, k_shape, dilation))
  x, kernel = core.tf_float32(x).reshape(batch, steps, ch_in), core.tf_float32(kernel).reshape(taps, ch_in, ch_out)
  bias = None if bias is None else core.tf_float32(bias)
  if core._needs_grad(x, kernel, bias):
    y = _DilatedConvFunction.apply(x, kernel, bias, dilation, bool(relu_input))
  else:
    y = _DilatedConvFunction.forward(core._NoCtx(), x, kernel, bias, dilation, bool(relu_input))
  return y[:, :, None, :] if is_4d else y


def _conv_kernel_init(shape, initializer):
  """A Keras conv kernel [k, 1, a, b]: 'glorot_uniform' with fans k * a and k * b, or 'orthogonal' over the [k * a, b] flattening."""
  k, _, a, b = shape
  if initializer == 'glorot_uniform':
    limit = math.sqrt(6.0 / (k * a + k * b))
    return torch.empty(shape, dtype=torch.float32).uniform_(-limit, limit)
  if initializer == 'orthogonal':
    return torch.nn.init.orthogonal_(torch.empty((k * a, b), dtype=torch.float32)).reshape(shape)
  raise ValueError("kernel_initializer must be 'glorot_uniform' or 'orthogonal', got {!r}".format(initializer))


def _single(value, what):
  """k of (k, 1), or k itself."""
  if isinstance(value, (tuple, list)):
    if len(value) != 2 or value[1] != 1:
      raise ValueError('{} must be k or (k, 1): the convolutions run over time only, got {!r}'.format(what, value))
    value = value[0]
  if int(value) < 1:
    raise ValueError('{} must be at least 1, got {!r}'.format(what, value))
  return int(value)


class Conv2D(_Lazy):
  """tf.keras.layers.Conv2D(filters, (k, 1), (s, 1), dilation_rate=(d, 1), padding='same') on [batch, time, 1, ch] (or
  [batch, time, ch]).  Weights under the Keras names and layouts: kernel [k, 1, in, out] ('glorot_uniform' with fans k * in and
  k * out, or 'orthogonal' over the [k * in, out] flattening), bias [out] zeros.

  Stride 1 is dilated_conv (one kernel each way).  A stride s > 1 - the stack's downsampler - is framework ops: F.pad and
  F.conv1d on the permuted tensor, with TF's 'same' rule (tensorflow/core/framework/kernel_shape_util.cc
  GetWindowedOutputSizeVerbose: out = ceil(T / s), total = max((out - 1) * s + k - T, 0), pad_before = total // 2, the rest
  behind)."""

  def __init__(self, filters, kernel_size, strides=1, dilation_rate=1, kernel_initializer='glorot_uniform'):
    super().__init__()
    self.filters = _single(filters, 'filters')
    self.kernel_size = _single(kernel_size, 'kernel_size')
    self.strides = _single(strides, 'strides')
    self.dilation_rate = _single(dilation_rate, 'dilation_rate')
    if self.strides > 1 and self.dilation_rate > 1:
      raise ValueError('Conv2D: strides > 1 and dilation_rate > 1 together are not supported (as in Keras)')
    if kernel_initializer not in ('glorot_uniform', 'orthogonal'):
      raise ValueError("kernel_initializer must be 'glorot_uniform' or 'orthogonal', got {!r}".format(kernel_initializer))
    self.kernel_initializer = kernel_initializer

  def build(self, in_ch):
    self.kernel = self._param(_conv_kernel_init((self.kernel_size, 1, in_ch, self.filters), self.kernel_initializer))
    self.bias = self._param(torch.zeros(self.filters))
    self.built = True

  def forward(self, x, relu_input=False):
    self._ensure_built(x.shape[-1])
    if self.strides == 1:
      return dilated_conv(x, self.kernel, self.bias, self.dilation_rate, relu_input)
    x = core.tf_float32(x)
    if relu_input:
      x = torch.relu(x)
    n_dims = x.dim()
    if n_dims not in (3, 4) or (n_dims == 4 and x.shape[2] != 1):
      raise ValueError('Conv2D: x must be [batch, time, ch] or [batch, time, 1, ch], got {}'.format(tuple(x.shape)))
    x = x.reshape(x.shape[0], x.shape[1], x.shape[-1])
    steps, k, s = x.shape[1], self.kernel_size, self.strides
    total = max((-(-steps // s) - 1) * s + k - steps, 0)
    x = torch.nn.functional.pad(x.permute(0, 2, 1), (total // 2, total - total // 2))
    y = torch.nn.functional.conv1d(x, self.kernel[:, 0].permute(2, 1, 0), self.bias, stride=s).permute(0, 2, 1)
    return ensure_4d(y) if n_dims == 4 else y


class Conv2DTranspose(_Lazy):
  """tf.keras.layers.Conv2DTranspose(filters, (k, 1), (s, 1), padding='same') on [batch, time, 1, ch] (or [batch, time, ch]) -> time
  * s rows: the stack's upsampler (k = 2 s).  Weights under the Keras names and layouts: kernel [k, 1, out, in], bias [out] zeros.

  It is the transpose of the 'same' convolution of stride s that maps length T * s to T, whose padding in front is
  pad_before = max((T - 1) * s + k - T * s, 0) // 2 (tensorflow/core/framework/kernel_shape_util.cc GetWindowedOutputSizeVerbose;
  tensorflow/python/ops/nn_ops.py conv2d_transpose computes the input gradient of that convolution), = s // 2 for k = 2 s:
  y[j] = full[j + pad_before], j < T * s, with full[j] = sum_i sum_ci x[i, ci] kernel[j - i * s, 0, co, ci].  Framework ops:
  F.conv_transpose1d on the permuted tensor, then the crop."""

  def __init__(self, filters, kernel_size, strides=1, kernel_initializer='glorot_uniform'):
    super().__init__()
    self.filters = _single(filters, 'filters')
    self.kernel_size = _single(kernel_size, 'kernel_size')
    self.strides = _single(strides, 'strides')
    if self.kernel_size < self.strides:
      raise ValueError('Conv2DTranspose: kernel_size {} must be at least strides {}'.format(self.kernel_size, self.strides))
    if kernel_initializer not in ('glorot_uniform', 'orthogonal'):
      raise ValueError("kernel_initializer must be 'glorot_uniform' or 'orthogonal', got {!r}".format(kernel_initializer))
    self.kernel_initializer = kernel_initializer

  def build(self, in_ch):
    self.kernel = self._param(_conv_kernel_init((self.kernel_size, 1, self.filters, in_ch), self.kernel_initializer))
    self.bias = self._param(torch.zeros(self.filters))
    self.built = True

  def forward(self, x):
    x = core.tf_float32(x)
    self._ensure_built(x.shape[-1])
    n_dims = x.dim()
    if n_dims not in (3, 4) or (n_dims == 4 and x.shape[2] != 1):
      raise ValueError('Conv2DTranspose: x must be [batch, time, ch] or [batch, time, 1, ch], got {}'.format(tuple(x.shape)))
    x = x.reshape(x.shape[0], x.shape[1], x.shape[-1])
    steps, k, s = x.shape[1], self.kernel_size, self.strides
    before = max((steps - 1) * s + k - steps * s, 0) // 2
    full = torch.nn.functional.conv_transpose1d(x.permute(0, 2, 1), self.kernel[:, 0].permute(2, 1, 0), self.bias, stride=s)
    y = full[:, :, before:before + steps * s].permute(0, 2, 1)
    return ensure_4d(y) if n_dims == 4 else y


class DilatedConvLayer(torch.nn.Module):
  """The reference's `dilated_conv` Sequential (ddsp/training/nn.py:1226-1237): Activation(relu) -> Conv2D, here one kernel.  The
  convolution's weights are conv.kernel and conv.bias."""

  def __init__(self, conv):
    super().__init__()
    self.conv = conv

  def forward(self, x):
    return self.conv(x, relu_input=True)


class DilatedConvStack(torch.nn.Module):
  """Stack of dilated 1-D convolutions, optional conditioning at each layer (ddsp/training/nn.py:1153-1323).

  conv_in, then stacks * layers_per_stack residual layers x = x + norm(conv(relu(x))) whose dilation is dilation ** depth inside
  a stack (a negative `dilation` decreases with depth), with resampling layers between the stacks if asked for.  The
  convolutions are dilated_conv (ReLU, taps and bias in one kernel each way), the norms Normalize / ConditionalNorm (one kernel
  each way); FiLM's multiply-add, the residual add and the two resamplers are framework ops.  spectral_norm=True is not built
  (ValueError)."""

  def __init__(self,
               ch=256,
               layers_per_stack=5,
               stacks=2,
               kernel_size=3,
               dilation=2,
               norm_type=None,
               resample_type=None,
               resample_stride=1,
               stacks_per_resample=1,
               resample_after_convolve=True,
               spectral_norm=False,
               ortho_init=False,
               shift_only=False,
               conditional=False,
               **kwargs):
    """Constructor.

    Args:
      ch: Number of channels in each convolution layer.
      layers_per_stack: Convolution layers in each 'stack'. Dilation increases exponentially with layer depth inside a stack.
      stacks: Number of convolutions stacks.
      kernel_size: Size of convolution kernel.
      dilation: Exponent base of dilation factor within a stack.
      norm_type: Type of normalization before each nonlinearity, choose from 'layer', 'instance', or 'group'.
      resample_type: Whether to 'upsample' or 'downsample' the signal. None performs no resampling.
      resample_stride: Stride for upsample or downsample layers.
      stacks_per_resample: Number of stacks per a resample layer.
      resample_after_convolve: Ordering of convolution and resampling. If True, apply `stacks_per_resample` stacks of
        convolution then a resampling layer. If False, apply the opposite order.
      spectral_norm: Not built on the MI355X path (ValueError if True).
      ortho_init: Orthogonally initialize the kernel weights.
      shift_only: Learn/condition only shifts of normalization and not scale.
      conditional: Use conditioning signal to modulate shifts (and scales) of normalization (FiLM), instead of learned
        parameters.
      **kwargs: name.

    Returns:
      Convolved and resampled signal. If inputs shape is [batch, time, ch_in], output shape is [batch, time_out, ch], where `ch`
      is the class kwarg, and `time_out` is resample_stride ** (stacks // stacks_per_resample) times smaller or larger than
      `time` depending on whether `resample_type` is upsampling or downsampling.
    """
    name = kwargs.pop('name', None)
    if kwargs:
      raise TypeError('DilatedConvStack: unknown arguments {}'.format(sorted(kwargs)))
    if spectral_norm:
      raise ValueError('spectral_norm=True is not built on the MI355X path')
    super().__init__()
    self.name = name
    self.conditional = conditional
    self.norm_type = norm_type
    self.resample_after_convolve = resample_after_convolve

    initializer = 'orthogonal' if ortho_init else 'glorot_uniform'

    def conv(ch, k, stride=1, dilation=1, transpose=False):
      """Make a convolution layer."""
      if transpose:
        return Conv2DTranspose(ch, (k, 1), (stride, 1), kernel_initializer=initializer)
      return Conv2D(ch, (k, 1), (stride, 1), dilation_rate=(dilation, 1), kernel_initializer=initializer)

    # Layer Factories.
    def dilated_conv_layer(i):
      """Generates a dilated convolution layer, based on `i` depth in stack."""
      if dilation > 0:
        dilation_rate = int(dilation ** i)
      else:
        # If dilation is negative, decrease dilation with depth instead of increasing.
        dilation_rate = int((-dilation) ** (layers_per_stack - i - 1))
      return DilatedConvLayer(conv(ch, kernel_size, 1, dilation_rate))

    def resample_layer():
      """Generates a resampling layer."""
      if resample_type == 'downsample':
        return conv(ch, resample_stride, resample_stride)
      elif resample_type == 'upsample':
        return conv(ch, resample_stride * 2, resample_stride, transpose=True)
      else:
        raise ValueError(f'invalid resample type: {resample_type}, '
                         'must be either `upsample` or `downsample`.')

    # Layers.
    self.conv_in = conv(ch, kernel_size)
    self.layers = torch.nn.ModuleList()
    self.norms = torch.nn.ModuleList()
    self.resample_layers = torch.nn.ModuleList()

    # Stacks.
    for i in range(stacks):
      # Option: Resample before convolve.
      if (resample_type and not self.resample_after_convolve and
          i % stacks_per_resample == 0):
        self.resample_layers.append(resample_layer())

      # Convolve.
      for j in range(layers_per_stack):
        # Convolution.
        layer = dilated_conv_layer(j)
        # Normalization / scale and shift.
        if self.conditional:
          norm = ConditionalNorm(norm_type=norm_type, shift_only=shift_only)
        else:
          norm = Normalize(norm_type=norm_type)

        # Add to the stack.
        self.layers.append(layer)
        self.norms.append(norm)

      # Option: Resample after convolve.
      if (resample_type and self.resample_after_convolve and
          (i + 1) % stacks_per_resample == 0):
        self.resample_layers.append(resample_layer())

    # For forward pass, calculate layers per a resample.
    if len(self.resample_layers):
      self.layers_per_resample = len(self.layers) // len(self.resample_layers)
    else:
      self.layers_per_resample = 0

  def forward(self, inputs):
    """Forward pass: x [batch, time, ch_in] (or 4-D), or the pair (x, z) when conditional -> [batch, time_out, ch]."""
    # Get inputs.
    if self.conditional:
      x, z = inputs
      x = ensure_4d(core.tf_float32(x))
      z = ensure_4d(core.tf_float32(z))
    else:
      x = inputs
      x = ensure_4d(core.tf_float32(x))

    # Run them through the network.
    x = self.conv_in(x)

    # Stacks.
    for i, (layer, norm) in enumerate(zip(self.layers, self.norms)):

      # Optional: Resample before conv.
      if (len(self.resample_layers) and not self.resample_after_convolve and
          i % self.layers_per_resample == 0):
        x = self.resample_layers[i // self.layers_per_resample](x)

      # Scale and shift by conditioning.
      if self.conditional:
        y = layer(x)
        x = x + norm([y, z])

      # Regular residual network.
      else:
        x = x + norm(layer(x))

      # Optional: Resample after conv.
      if (len(self.resample_layers) and self.resample_after_convolve and
          (i + 1) % self.layers_per_resample == 0):
        x = self.resample_layers[i // self.layers_per_resample](x)

    return x[:, :, 0, :]  # Convert back to 3-D.


class FcStackOut(torch.nn.Module):
  """Stack of FC layers with variable hidden and output dims."""

  def __init__(self, ch, layers, n_out):
    super().__init__()
    self.stack = FcStack(ch, layers)
    self.dense_out = Dense(n_out)

  def forward(self, x):
    return self.dense_out(self.stack(x))


class OutputSplitsLayer(DictLayer):
  """A DictLayer that splits an output tensor into a dictionary of tensors (ddsp/training/nn.py:249-298): a subclass writes
  compute_output(*inputs) -> one tensor, which runs through a final Dense and is split according to output_splits."""

  def __init__(self, input_keys=None, output_splits=(('amps', 1), ('harmonic_distribution', 40)), **kwargs):
    input_keys = input_keys or self.get_argument_names('compute_output')
    super().__init__(input_keys=input_keys, output_keys=[v[0] for v in output_splits], **kwargs)
    self.output_splits = output_splits
    self.n_out = sum([v[1] for v in output_splits])
    self.dense_out = Dense(self.n_out)

  def call(self, *inputs, **unused_kwargs):
    """Run compute_output(), dense output layer, then split to a dictionary."""
    output = self.compute_output(*inputs)
    return split_to_dict(self.dense_out(output), self.output_splits)

  def compute_output(self, *inputs):
    """Takes tensors as input, runs network, and outputs a single tensor (usually [batch, time, channels])."""
    raise NotImplementedError


# ------------------ 2-D convolutions and the ResNet ---------------------------
_conv2d_ws = core.Workspace()
_DKERNEL_PARTIAL_ELEMENTS = 1 << 24      # 64 MiB of partial kernel gradients per tap, at the most


def _conv2d_entry(name):
  return _lib.conv2d_entry(_lib.load(), name)


def same_padding(size, kernel_size, stride):
  """TF's 'same' rule along one axis (tensorflow/core/framework/kernel_shape_util.cc GetWindowedOutputSizeVerbose):
  -> (out, before, behind) with out = ceil(size / stride), total = max((out - 1) * stride + kernel_size - size, 0),
  before = total // 2 and the odd cell behind."""
  size, kernel_size, stride = int(size), int(kernel_size), int(stride)
  out = -(-size // stride)
  total = max((out - 1) * stride + kernel_size - size, 0)
  return out, total // 2, total - total // 2


def _run_conv2d(x, kernel, bias, strides, flags, image=None, mask_src=None, addend=None):
  """One ddsp_conv2d_f32 call on contiguous fp32 tensors; kernel [kh, kw, ch_in, ch_out].  Forward: x [b, h, w, ch_in] ->
  [b, out_h, out_w, ch_out].  With CONV2D_ADJOINT x is the gradient [b, out_h, out_w, ch_out], `image` the forward input's (h, w),
  -> [b, h, w, ch_in]."""
  kh, kw, ch_in, ch_out = kernel.shape
  b = x.shape[0]
  if flags & _lib.CONV2D_ADJOINT:
    h, w = image
    y = torch.empty((b, h, w, ch_in), dtype=torch.float32, device=x.device)
  else:
    h, w = x.shape[1], x.shape[2]
    y = torch.empty((b, same_padding(h, kh, strides[0])[0], same_padding(w, kw, strides[1])[0], ch_out), dtype=torch.float32,
                    device=x.device)
  if b:
    ptr = lambda v: None if v is None else v.data_ptr()
    shape = (b, h, w, ch_in, ch_out, kh, kw, strides[0], strides[1])
    ws = _conv2d_ws.get(_conv2d_entry('ddsp_conv2d_workspace_bytes')(*shape, flags), x.device)
    rc = _conv2d_entry('ddsp_conv2d_f32')(x.data_ptr(), kernel.data_ptr(), ptr(bias), ptr(addend), ptr(mask_src), y.data_ptr(),
                                          ws.data_ptr(), ws.numel(), *shape, flags, core._stream())
    _checked(rc, 'ddsp_conv2d_f32')
  return y


class _Conv2dFunction(torch.autograd.Function):
  """torch.autograd node of the 2-D convolution: (x [b, h, w, ch_in], kernel [kh, kw, ch_in, ch_out], bias [ch_out] or None, addend
  [b, out_h, out_w, ch_out] or None) -> [b, out_h, out_w, ch_out].  Forward and the gradient in x are C-ABI calls (the same kernel;
  the adjoint gathers the gradient through the inverse of the position map and multiplies by relu'(x) = (x > 0) in its epilogue).
  The gradients whose reduction runs over batch * positions are the framework's: kh * kw matrix products over strided views of one
  padded act(x), and a column sum.  The addend's gradient is grad_y.  Kept for the backward: x and the kernel."""

  @staticmethod
  def forward(ctx, x, kernel, bias, addend, strides, relu_input):
    y = _run_conv2d(x, kernel, bias, strides, _lib.CONV2D_RELU_INPUT if relu_input else 0, addend=addend)
    ctx.save_for_backward(x, kernel)
    ctx.strides, ctx.relu_input, ctx.has_bias, ctx.has_addend = strides, relu_input, bias is not None, addend is not None
    return y

  @staticmethod
  def backward(ctx, grad_y):
    x, kernel = ctx.saved_tensors
    kh, kw, ch_in, ch_out = kernel.shape
    (sh, sw), (h, w) = ctx.strides, x.shape[1:3]
    grad_y = core.tf_float32(grad_y)
    dx = dk = db = None
    if ctx.needs_input_grad[0]:
      flags = _lib.CONV2D_ADJOINT | (_lib.CONV2D_MASK_OUTPUT if ctx.relu_input else 0)
      dx = _run_conv2d(grad_y, kernel, None, ctx.strides, flags, image=(h, w), mask_src=x if ctx.relu_input else None)
    if ctx.needs_input_grad[1]:
      (out_h, top, bottom), (out_w, left, right) = same_padding(h, kh, sh), same_padding(w, kw, sw)
      a = torch.nn.functional.pad(torch.relu(x) if ctx.relu_input else x, (0, 0, left, right, top, bottom))   # the one copy
      # One long reduction over batch * positions would run on a handful of workgroups: it is cut into groups - image rows while
      # their [groups, ch_in, ch_out] partial products stay small, batch rows otherwise - one batched product each, summed after.
      groups = x.shape[0] * out_h if x.shape[0] * out_h * ch_in * ch_out <= _DKERNEL_PARTIAL_ELEMENTS else x.shape[0]
      g = grad_y.reshape(groups, -1, ch_out)
      dk = torch.empty_like(kernel)
      for i in range(kh):
        for j in range(kw):                             # y[oh, ow] takes a[oh sh + i, ow sw + j]: a strided view
          view = a[:, i:i + (out_h - 1) * sh + 1:sh, j:j + (out_w - 1) * sw + 1:sw, :]
          dk[i, j] = torch.matmul(view.reshape(groups, -1, ch_in).transpose(1, 2), g).sum(0)
    if ctx.has_bias and ctx.needs_input_grad[2]:
      db = grad_y.reshape(-1, ch_out).sum(0)
    return dx, dk, db, (grad_y if ctx.has_addend and ctx.needs_input_grad[3] else None), None, None


def _pair(value, what):
  """(a, b) of an int or a pair, each at least 1."""
  pair = tuple(value) if isinstance(value, (tuple, list)) else (value, value)
  if len(pair) != 2 or min(int(v) for v in pair) < 1:
    raise ValueError('{} must be an int or a pair of ints, each at least 1, got {!r}'.format(what, value))
  return int(pair[0]), int(pair[1])


def conv2d(x, kernel, bias=None, strides=(1, 1), relu_input=False, addend=None):
  """A 2-D convolution of a channel-last tensor with TF 'same' padding and strides on both axes - tf.keras.layers.Conv2D(ch_out,
  (kh, kw), strides, padding='same') on [batch, h, w, ch_in] - with an optional ReLU on its input and an optional addend on its
  output, in one kernel each way (csrc/conv2d.hip; C ABI csrc/conv2d_abi.h):

    y[b, oh, ow, co] = addend + bias[co] + sum_{i, j, ci} act(x[b, oh * sh + i - top, ow * sw + j - left, ci]) * kernel[i, j, ci, co]

  positions outside the image contributing 0; out, top and left per axis are same_padding's.  ReLU is applied as x is loaded, bias
  and addend as y is written; there is no padded copy and nothing of size [batch, positions, kh * kw * ch_in].  ch_out in multiples
  of 16 runs on the matrix cores (fp16 hi / lo operands behind a power-of-two scale per batch row of x; the K axis is the flattened
  (i, j, ci)), every other width on the vector ALU.  The same bits on every run, for a row alone and for any sub-batch.

  Args:
    x: [batch, h, w, ch_in], of any layout or dtype.
    kernel: [kh, kw, ch_in, ch_out], the Keras layout.
    bias: [ch_out] or None.
    strides: (sh, sw) or one int for both.
    relu_input: Apply ReLU to x first (its gradient at 0 is 0, as tf.nn.relu's).
    addend: [batch, out_h, out_w, ch_out] or None: added to the result in the kernel's epilogue (a residual connection).

  Returns:
    [batch, out_h, out_w, ch_out].  Differentiable in x, kernel, bias and addend.

  Raises:
    ValueError: shapes that do not fit, or beyond the limits of the MI355X path - ch_in, ch_out <= 1024, kh * kw <= 64,
      strides <= 8, h, w <= 2 ** 30 and every element count < 2 ** 31.  Checked before anything touches the device.
  """
  x_shape = tuple(x.shape) if hasattr(x, 'shape') else tuple(torch.as_tensor(x).shape)
  k_shape = tuple(kernel.shape) if hasattr(kernel, 'shape') else tuple(torch.as_tensor(kernel).shape)
  if len(x_shape) != 4:
    raise ValueError('conv2d: x must be [batch, h, w, ch_in], got {}'.format(x_shape))
  if len(k_shape) != 4:
    raise ValueError('conv2d: kernel must be [kh, kw, ch_in, ch_out], got {}'.format(k_shape))
  sh, sw = _pair(strides, 'conv2d: strides')
  batch, h, w, ch_in = x_shape
  kh, kw, _, ch_out = k_shape
  if k_shape[2] != ch_in or min(h, w, ch_in, ch_out, kh, kw) < 1:
    raise ValueError('conv2d: x {} and kernel {} must agree in ch_in, and h, w, kh, kw and the channels be at least 1'.format(
        x_shape, k_shape))
  if bias is not None and tuple(bias.shape) != (ch_out,):
    raise ValueError('conv2d: bias must be [ch_out] = {}, got {}'.format((ch_out,), tuple(bias.shape)))
  if max(ch_in, ch_out) > _lib.CONV2D_MAX_CHANNELS or kh * kw > _lib.CONV2D_MAX_TAPS or max(sh, sw) > _lib.CONV2D_MAX_STRIDE:
    raise ValueError('conv2d: at most {} channels, {} taps and stride {} on the MI355X path, got ch_in = {}, ch_out = {}, kernel {} x {}, '
                     'strides {}'.format(_lib.CONV2D_MAX_CHANNELS, _lib.CONV2D_MAX_TAPS, _lib.CONV2D_MAX_STRIDE, ch_in, ch_out, kh, kw,
                                         (sh, sw)))
  out_h, out_w = same_padding(h, kh, sh)[0], same_padding(w, kw, sw)[0]
  if max(h, w) > _lib.CONV2D_MAX_SIDE or max(batch * h * w * ch_in, batch * out_h * out_w * ch_out, kh * kw * ch_in * ch_out) >= 2 ** 31:
    raise ValueError('conv2d: h and w must stay at or below 2 ** 30 and batch * h * w * ch_in, batch * out_h * out_w * ch_out and the '
                     'kernel below 2 ** 31 elements, got x {}, kernel {}, strides {}'.format(x_shape, k_shape, (sh, sw)))
  if addend is not None and tuple(addend.shape) != (batch, out_h, out_w, ch_out):
    raise ValueError('conv2d: addend must be [batch, out_h, out_w, ch_out] = {}, got {}'.format((batch, out_h, out_w, ch_out),
                                                                                            tuple(addend.shape)))
  x, kernel = core.tf_float32(x), core.tf_float32(kernel)
  bias = None if bias is None else core.tf_float32(bias)
  addend = None if addend is None else core.tf_float32(addend)
  if core._needs_grad(x, kernel, bias, addend):
    return _Conv2dFunction.apply(x, kernel, bias, addend, (sh, sw), bool(relu_input))
  return _Conv2dFunction.forward(core._NoCtx(), x, kernel, bias, addend, (sh, sw), bool(relu_input))


class SpatialConv2D(_Lazy):
  """tf.keras.layers.Conv2D(filters, (kh, kw), (sh, sw), padding='same') on [batch, h, w, ch]: conv2d, one kernel each way, the 1 x 1
  projections included.  Weights under the Keras names and layouts: kernel [kh, kw, in, out] ('glorot_uniform' with fans
  kh * kw * in and kh * kw * out), bias [out] zeros.  (Conv2D is the (k, 1) layer over time of the dilated stack.)"""

  def __init__(self, filters, kernel_size, strides=(1, 1), kernel_initializer='glorot_uniform'):
    super().__init__()
    self.filters = int(filters)
    if self.filters < 1:
      raise ValueError('SpatialConv2D: filters must be at least 1, got {!r}'.format(filters))
    self.kernel_size = _pair(kernel_size, 'SpatialConv2D: kernel_size')
    self.strides = _pair(strides, 'SpatialConv2D: strides')
    if kernel_initializer != 'glorot_uniform':
      raise ValueError("SpatialConv2D: kernel_initializer must be 'glorot_uniform', got {!r}".format(kernel_initializer))
    self.kernel_initializer = kernel_initializer

  def build(self, in_ch):
    kh, kw = self.kernel_size
    limit = math.sqrt(6.0 / (kh * kw * in_ch + kh * kw * self.filters))
    self.kernel = self._param(torch.empty((kh, kw, in_ch, self.filters), dtype=torch.float32).uniform_(-limit, limit))
    self.bias = self._param(torch.zeros(self.filters))
    self.built = True

  def forward(self, x, relu_input=False, addend=None):
    self._ensure_built(x.shape[-1])
    return conv2d(x, self.kernel, self.bias, self.strides, relu_input, addend)


class MaxPool2D(torch.nn.Module):
  """tf.keras.layers.MaxPool2D(pool_size, strides, padding) on [batch, h, w, ch] (framework ops).  padding='same' is TF's rule
  (same_padding: the odd cell behind, which F.max_pool2d's own symmetric padding is not); the padded cells are -inf and never win."""

  def __init__(self, pool_size=(2, 2), strides=None, padding='same'):
    super().__init__()
    self.pool_size = _pair(pool_size, 'MaxPool2D: pool_size')
    self.strides = self.pool_size if strides is None else _pair(strides, 'MaxPool2D: strides')
    if padding not in ('same', 'valid'):
      raise ValueError("MaxPool2D: padding must be 'same' or 'valid', got {!r}".format(padding))
    self.padding = padding

  def forward(self, x):
    if len(x.shape) != 4:
      raise ValueError('MaxPool2D: x must be [batch, h, w, ch], got {}'.format(tuple(x.shape)))
    x = core.tf_float32(x).permute(0, 3, 1, 2)
    if self.padding == 'same':
      (_, top, bottom), (_, left, right) = (same_padding(n, k, s) for n, k, s in zip(x.shape[2:], self.pool_size, self.strides))
      x = torch.nn.functional.pad(x, (left, right, top, bottom), value=float('-inf'))
    return torch.nn.functional.max_pool2d(x, self.pool_size, self.strides).permute(0, 2, 3, 1)


class NormReluConv(torch.nn.Module):
  """Norm -> ReLU -> Conv layer (ddsp/training/nn.py:698-709): Normalize (csrc/group_norm.hip), then conv2d with the ReLU on its
  load; `addend` rides the convolution's epilogue.  Weights: norm.scale, norm.shift, conv.kernel, conv.bias."""

  def __init__(self, ch, k, s, norm_type):
    """Downsample frequency by stride."""
    super().__init__()
    self.norm = Normalize(norm_type)
    self.conv = SpatialConv2D(ch, (k, k), (1, s))

  def forward(self, x, addend=None):
    return self.conv(self.norm(x), relu_input=True, addend=addend)


class ResidualLayer(torch.nn.Module):
  """A single layer for ResNet, with a bottleneck (ddsp/training/nn.py:712-756).  The ReLU behind norm_input is applied by the two
  convolutions that read it, on their loads, and x + r by the last convolution's epilogue."""

  def __init__(self, ch, stride, shortcut, norm_type, conditional, shift_only):
    """Downsample frequency by stride, upsample channels by 4."""
    super().__init__()
    ch_out = 4 * ch
    self.shortcut = shortcut
    self.conditional = conditional

    # Layers.
    self.norm_input = get_norm(norm_type, conditional, shift_only)

    if self.shortcut:
      self.conv_proj = SpatialConv2D(ch_out, (1, 1), (1, stride))
    self.bottleneck = torch.nn.ModuleList([
        SpatialConv2D(ch, (1, 1), (1, 1)),
        NormReluConv(ch, 3, stride, norm_type),
        NormReluConv(ch_out, 1, 1, norm_type),
    ])

  def forward(self, inputs):
    if self.conditional:
      x, z = inputs
      r = ensure_4d(core.tf_float32(x))
      x = self.norm_input((r, ensure_4d(core.tf_float32(z))))
    else:
      r = ensure_4d(core.tf_float32(inputs))
      x = self.norm_input(r)

    # The projection shortcut should come after the first norm and ReLU
    # since it performs a 1x1 convolution.
    r = self.conv_proj(x, relu_input=True) if self.shortcut else r
    x = self.bottleneck[0](x, relu_input=True)
    x = self.bottleneck[1](x)
    return self.bottleneck[2](x, addend=r)


class ResidualStack(torch.nn.Module):
  """LayerNorm -> ReLU -> Conv layer (ddsp/training/nn.py:759-802): per (ch, n_layers, stride) one ResidualLayer with the projection
  shortcut and the stride and n_layers - 1 without, then a Normalize and the nonlinearity.  inputs: x, or [x, z] if conditional."""

  def __init__(self, filters, block_sizes, strides, norm_type, conditional=False, shift_only=False, nonlinearity='relu'):
    """ResNet layers."""
    super().__init__()
    self.conditional = conditional
    layers = []
    for (ch, n_layers, stride) in zip(filters, block_sizes, strides):

      # Only the first block per residual_stack uses shortcut and strides.
      layers.append(ResidualLayer(ch, stride, True, norm_type, conditional, shift_only))

      # Add the additional (n_layers - 1) layers to the stack.
      for _ in range(1, n_layers):
        layers.append(ResidualLayer(ch, 1, False, norm_type, conditional, shift_only))

    layers.append(Normalize(norm_type))
    self.layers = torch.nn.ModuleList(layers)
    self.activation = get_nonlinearity(nonlinearity)

  def forward(self, inputs):
    if self.conditional:
      x, z = inputs
      z = core.tf_float32(z)                            # once: every layer reads the same fp32 tensor, and its gradient is one fp32 sum
    else:
      x = inputs

    for layer in self.layers:
      is_cond = self.conditional and isinstance(layer, ResidualLayer)
      l_in = [x, z] if is_cond else x
      x = layer(l_in)
    return self.activation(x)


class ResNet(torch.nn.Module):
  """Residual network (ddsp/training/nn.py:805-839): a 7 x 7 stem striding the second axis by 2, a (1, 3) max pool striding it by 2,
  and two ResidualStacks; [batch, frames, bins, 1] -> [batch, frames, ceil(bins / 32), 32 ch].  An unknown size raises the
  reference's KeyError.  inputs: x, or [x, z] if conditional."""

  def __init__(self, size='large', norm_type='layer', conditional=False, shift_only=False):
    super().__init__()
    self.conditional = conditional
    size_dict = {
        'small': (32, [2, 3, 4]),
        'medium': (32, [3, 4, 6]),
        'large': (64, [3, 4, 6]),
    }
    ch, blocks = size_dict[size]
    self.layers = torch.nn.ModuleList([
        SpatialConv2D(64, (7, 7), (1, 2)),
        MaxPool2D(pool_size=(1, 3), strides=(1, 2), padding='same'),
        ResidualStack([ch, 2 * ch, 4 * ch], blocks, [1, 2, 2], norm_type, conditional, shift_only),
        ResidualStack([8 * ch], [3], [2], norm_type, conditional, shift_only)
    ])

  def forward(self, inputs):
    if self.conditional:
      x, z = inputs
      z = core.tf_float32(z)
    else:
      x = inputs

    for layer in self.layers:
      is_cond = self.conditional and isinstance(layer, ResidualStack)
      l_in = [x, z] if is_cond else x
      x = layer(l_in)
    return x


# ------------------ Vector Quantization ---------------------------------------
_vq_ws = core.Workspace()


def _vq_entry(name):
  return _lib.vq_entry(_lib.load(), name)


def _vq_shapes(op, x_shape, num_heads, k):
  """-> (rows, dims) of x [..., depth] cut into num_heads vectors of `dims` per row; the errors of the vector quantizer."""
  num_heads, k = int(num_heads), int(k)
  if len(x_shape) < 1 or x_shape[-1] < 1:
    raise ValueError('{}: x must be [..., depth] with depth >= 1, got {}'.format(op, tuple(x_shape)))
  if num_heads < 1 or k < 1:
    raise ValueError('{}: k and num_heads must be at least 1, got k = {}, num_heads = {}'.format(op, k, num_heads))
  if x_shape[-1] % num_heads != 0:
    raise ValueError('Input depth must be a multiple of the number of heads.')
  rows, dims = math.prod(x_shape[:-1]), x_shape[-1] // num_heads
  if k > _lib.VQ_MAX_CENTROIDS or dims > _lib.VQ_MAX_DIMS:
    raise NotImplementedError('{}: at most {} centroids of {} dims per head on the MI355X path, got k = {}, depth / num_heads = {}'
                              .format(op, _lib.VQ_MAX_CENTROIDS, _lib.VQ_MAX_DIMS, k, dims))
  if rows * num_heads >= 2 ** 31:
    raise NotImplementedError('{}: rows * num_heads must stay below 2 ** 31, got rows = {}, num_heads = {}'.format(op, rows, num_heads))
  return rows, dims


def vq_assign(x, e, num_heads=1):
  """The nearest centroid of every vector of x, and that centroid (ddsp/training/nn.py:1417-1431), in fused kernels
  (csrc/vq.hip; C ABI csrc/vq_abi.h): no [n, k] distance matrix exists.

  Row i of x holds num_heads vectors x[i, h * D : (h + 1) * D], D = depth / num_heads, read in place.  c is the argmin over j of
  |e_j|^2 / 2 - x . e_j, which is the argmin of the distance; of exactly equal scores the LOWEST index wins, as tf.argmin decides
  (identical centroids have identical score bits).  k in multiples of 16 runs on the matrix cores (fp16 hi / lo operands, every
  vector behind its own power-of-two scale), every other k on the vector ALU.  The same bits on every run, for a row alone and
  inside any batch.  A vector with a non-finite entry gets c = 0; z_q is NaN where x is not finite.

  Args:
    x: [..., depth], of any rank >= 1, layout or dtype.
    e: The centroids, [k, depth / num_heads].
    num_heads: Vectors per row of x.

  Returns:
    (z_q, c): z_q of x's shape, e[c] bit for bit; c int64 [..., num_heads].  Not differentiable.

  Raises:
    ValueError: shapes that do not fit.
    NotImplementedError: beyond the limits of the MI355X path - k <= 4096, depth / num_heads <= 512, rows * num_heads < 2 ** 31.
  """
  shape = tuple(x.shape) if hasattr(x, 'shape') else tuple(torch.as_tensor(x).shape)
  e_shape = tuple(e.shape) if hasattr(e, 'shape') else tuple(torch.as_tensor(e).shape)
  if len(e_shape) != 2:
    raise ValueError('vq_assign: e must be [k, depth / num_heads], got {}'.format(e_shape))
  num_heads = int(num_heads)
  rows, dims = _vq_shapes('vq_assign', shape, num_heads, e_shape[0])
  if e_shape[1] != dims:
    raise ValueError('vq_assign: e must be [k, depth / num_heads] = [k, {}], got {}'.format(dims, e_shape))
  x, e = core.tf_float32(x).detach(), core.tf_float32(e).detach()
  k = e_shape[0]
  z = torch.empty_like(x)
  c = torch.empty((rows, num_heads), dtype=torch.int32, device=x.device)
  if rows:
    ws = _vq_ws.get(_vq_entry('ddsp_vq_workspace_bytes')(k, dims), x.device)
    rc = _vq_entry('ddsp_vq_assign_f32')(x.data_ptr(), e.data_ptr(), c.data_ptr(), z.data_ptr(), ws.data_ptr(), ws.numel(), rows, num_heads,
                                         k, dims, core._stream())
    _lib.check(rc, 'ddsp_vq_assign_f32')
  return z, c.to(torch.int64).reshape(shape[:-1] + (num_heads,))


def vq_statistics(x, c, k, num_heads=1):
  """How many vectors of x each centroid was given, and their sums (ddsp/training/nn.py:1436-1438), in one kernel (csrc/vq.hip):
  no one-hot matrix exists.  The sums are added in fp64 in the reference's x_flat order (head-major, then rows) and rounded once;
  no atomics, the same bits on every run.  Entries of c outside [0, k) are counted nowhere.

  Args:
    x: [..., depth], of any layout or dtype.
    c: Integer indices [..., num_heads], as vq_assign returns them.
    k: Number of centroids.
    num_heads: Vectors per row of x.

  Returns:
    (counts [k], sums [k, depth / num_heads]), fp32.  Not differentiable.
  """
  shape = tuple(x.shape) if hasattr(x, 'shape') else tuple(torch.as_tensor(x).shape)
  num_heads, k = int(num_heads), int(k)
  rows, dims = _vq_shapes('vq_statistics', shape, num_heads, k)
  c = torch.as_tensor(c)
  if tuple(c.shape) != shape[:-1] + (num_heads,) or c.is_floating_point() or c.is_complex():
    raise ValueError('vq_statistics: c must hold integers of shape {}, got {} of {}'.format(shape[:-1] + (num_heads,), c.dtype,
                                                                                          tuple(c.shape)))
  x = core.tf_float32(x).detach()
  c = c.to(device=x.device, dtype=torch.int32).contiguous()
  counts = torch.empty((k,), dtype=torch.float32, device=x.device)
  sums = torch.empty((k, dims), dtype=torch.float32, device=x.device)
  rc = _vq_entry('ddsp_vq_statistics_f32')(x.data_ptr() if rows else None, c.data_ptr() if rows else None, counts.data_ptr(), sums.data_ptr(),
                                           rows, num_heads, k, dims, core._stream())
  _lib.check(rc, 'ddsp_vq_statistics_f32')
  return counts, sums


class _StraightThroughFunction(torch.autograd.Function):
  """z_q's values with the identity as the gradient in x: the reference's x + stop_gradient(z - x) without its rounding."""

  @staticmethod
  def forward(ctx, x, z_q):
    return z_q.view_as(z_q)

  @staticmethod
  def backward(ctx, grad_z):
    return grad_z, None


def _divide_no_nan(sums, counts):
  """tf.math.divide_no_nan(sums, counts[:, None]): 0 where the count is 0."""
  counts = counts[:, None]
  return torch.where(counts == 0, torch.zeros_like(sums), sums / counts)


class VectorQuantization(torch.nn.Module):
  """Vector quantization using exponential moving average (ddsp/training/nn.py:1342-1461).

  The state is two buffers under the reference's variable names, made on the first call or by build(depth): counts [k] and
  sums [k, depth / num_heads], zeros; the centroids are e = divide_no_nan(sums, counts).  The assignment and the batch statistics
  are vq_assign and vq_statistics (csrc/vq.hip); the centroids, the restarts and the moving averages are framework ops on [k, D].

  forward(x, training=False) -> (z, c): z has the values of e[c] and the identity as its gradient in x (nothing flows into the
  state); c is int64 [..., num_heads].  With training=True the reference's restart rule runs first - keep = counts * k >
  restart_threshold * n, n = num_heads * rows; the r-th restarted centroid (in index order) becomes the r-th of min(restarts, n)
  distinct uniformly drawn vectors of the batch, those beyond n take U[0, 1) values - written with fixed-shape ops (a cumulative
  rank, randperm, rand, where: no nonzero, no host synchronisation), and afterwards counts -= (1 - gamma) (counts - batch counts),
  the same for sums, in place.  The draws come from torch's generator, so the training call is not capturable into a graph; the
  eval call is.

  Non-finite x: c = 0 for that vector and NaN in z where x is not finite.  In training mode such a vector's NaN reaches sums
  and from there every later call, as in the reference: outside the contract.
  Averaging the state across data-parallel replicas (the reference's VariableAggregation.MEAN) is not built."""

  def __init__(self, k, gamma=0.99, restart_threshold=0.0, num_heads=1, commitment_loss_weight=0.2, name='vector_quantization'):
    super().__init__()
    self.k = int(k)
    self.gamma = gamma
    self.restart_threshold = restart_threshold
    self.num_heads = int(num_heads)
    self.commitment_loss_weight = commitment_loss_weight
    self.name = name
    self.built = False

  def build(self, depth):
    depth = int(depth)
    _vq_shapes('VectorQuantization', (1, depth), self.num_heads, self.k)
    self.depth = depth
    self.register_buffer('counts', torch.zeros((self.k,), dtype=torch.float32, device=core._device()))
    self.register_buffer('sums', torch.zeros((self.k, depth // self.num_heads), dtype=torch.float32, device=core._device()))
    self.built = True

  def centroids(self):
    return _divide_no_nan(self.sums, self.counts)

  def _restarted(self, x, e):
    """The centroids of a training call: those whose count has fallen to the threshold are drawn anew."""
    heads, dims = self.num_heads, self.depth // self.num_heads
    rows = x.numel() // self.depth
    n = heads * rows
    keep = self.counts * self.k > self.restart_threshold * n
    rank = torch.cumsum((~keep).to(torch.int64), 0) - 1                  # the r-th restart, in index order
    drawn = torch.rand((self.k, dims), dtype=torch.float32, device=x.device)
    if n:
      pick = torch.randperm(n, device=x.device)[rank.clamp(0, n - 1)]   # x_flat rows: distinct while rank < n
      vectors = x.reshape(n, dims)[(pick % rows) * heads + pick // rows]        # x_flat row m = h rows + i is vector i heads + h
      drawn = torch.where((rank < n)[:, None], vectors, drawn)
    return torch.where(keep[:, None], e, drawn)

  def forward(self, x, training=False):
    x = core.tf_float32(x)
    if not self.built:
      self.build(x.shape[-1])
    if x.shape[-1] != self.depth:
      raise ValueError('VectorQuantization: built for depth {}, got x {}'.format(self.depth, tuple(x.shape)))
    with torch.no_grad():
      e = self.centroids()
      if training:
        e = self._restarted(x, e)
      z_q, c = vq_assign(x, e, self.num_heads)
      if training:
        counts, sums = vq_statistics(x, c, self.k, self.num_heads)
        self.counts.sub_((1 - self.gamma) * (self.counts - counts))
        self.sums.sub_((1 - self.gamma) * (self.sums - sums))
    z = _StraightThroughFunction.apply(x, z_q) if core._needs_grad(x) else z_q
    return z, c

  def unquantize(self, c):
    """The centroids of the indices c [..., num_heads] -> [..., depth] (a gather of the framework's)."""
    c = torch.as_tensor(c, device=self.sums.device)
    return self.centroids()[c].reshape(tuple(c.shape[:-1]) + (self.depth,))

  def committment_loss(self, z, z_q):
    """Encourage encoder to output embeddings close to the current centroids."""
    from ddsp_amd import losses
    z_q = core.tf_float32(z_q).detach()
    return self.commitment_loss_weight * losses.mean_difference(z, z_q, loss_type='L2')

  def get_losses_dict(self, z, z_q):
    return {self.name + '_commitment_loss': self.committment_loss(z, z_q)}
