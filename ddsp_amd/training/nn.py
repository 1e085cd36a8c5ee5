"""The note pooling of ddsp/training/nn.py:357-557 on the MI355X (csrc/notes.hip).

Of the reference's `training.nn` these pure tensor functions exist: straight_through_int_quantization, get_note_mask,
get_note_mask_from_onset, get_note_lengths, get_note_moments, pool_over_notes and get_short_note_loss_mask - what
MidiAutoencoder and ZMidiAutoencoder pool their per-note features with.  OUT OF SCOPE: the Keras layers and everything
else of `training/`.

The reference builds [batch, time, notes, dims] four times between x and the pooled result; here nothing of that size
exists, and nothing of size [batch, time, notes] but the mask itself.  The moments and the pooling are exact for ANY fp32
mask (weights m in the mean, m ** 2 in the variance), and their cost follows the mask's non-zero entries.

THE GRADIENT OF THE STANDARD DEVIATION AT ZERO.  The reference's std is `(...) ** 0.5`, whose derivative is unbounded where
the variance is exactly 0: every empty region, every one-step note, every constant stretch - so in every real call.  The
contract here: where a note's variance in a dimension is exactly 0, that entry of the std contributes 0 to dL/dx;
everywhere else the gradient is the analytic one.  No gradient flows into a mask.

Limits (NotImplementedError): max_regions <= 1024; batch * notes and batch * time below 2 ** 31."""
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
