"""Where a NaN or an Inf goes, on every entry point ("Non-finite values").

One value - NaN, +Inf or -Inf - is planted at one element of the LAST batch row of one tensor argument; everything else is the
clean call of tests/test_gpu_layouts.py (its rows, its values, its reference, its bit comparison).  Three rules:

  R1 memory  the call returns (or raises the ValueError the Python layer documents).  What keeps a value from moving an address
             is the audit table of DESIGN.md; this module holds the result in place.
  R2 rows    batch row 0 of every per-row output and per-row gradient is bit-equal to the clean call.  Excused by name:
             nonfinite_table.EXEMPT_ROWS.
  R3 NaN     weak form, every row: the poisoned batch row's outputs hold at least one non-finite element - unless
             nonfinite_table.KEEPS_FINITE names the line of the reference that drops the element, and then every output IS finite.
             strong form, the operations whose fp64 truth tests/ already holds: the non-finite mask of every output and of every
             gradient is a SUPERSET of the truth's (the kernel may spread a NaN further inside the batch row - block scales, the
             fp16 split's Inf - Inf - never lose one).  NaN and +-Inf.

Then extreme FINITE values on the split-fp16 kernels: one batch row scaled by 1e30 and by 1e-30 (common.h's pow2_exponent
clamps), the other row bit-equal, the scaled row inside the module's own tolerance relative to its size.

tests/test_nonfinite_emulated.py runs this module through the SIMT emulation on the CPU; tests/test_nonfinite_table.py holds the
two lists of nonfinite_table.py to the kernels.  Every case is one small call: the module's 839 cases take 6.0 s on the MI355X
(the slowest, 1.4 s, is the first call of the process) and a little over two minutes under the emulation."""
import numpy as np
import pytest
import torch

import decoder_truth as DT
import dilated_conv_truth as CT
import encoder_truth as ET
import layout_table as L
import nonfinite_table as NF
import test_gpu_layouts as G
import wavetable_truth as WT

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = L.B


# ---- planting ------------------------------------------------------------------------------------------------------------
def poisoned_values(row, ai, value):
  """The row's own values with `value` at plant_index of argument ai."""
  values = [x.clone() for x in G._base_values(row)]
  values[ai][NF.plant_index(row, row.args[ai], [v.cpu().numpy() for v in values])] = value
  return values


def run_poisoned(ddsp, row, ai, value):
  """-> (outputs, gradients) of the poisoned call and of the clean one; None when the Python layer refuses the value."""
  leaves = [i for i, a in enumerate(row.args) if a.grad]
  ref_outs, ref_grads = G._reference(ddsp, row)
  try:
    outs, grads, _ = G._run(ddsp, row, poisoned_values(row, ai, value), leaves)
  except ValueError:
    return None
  assert len(outs) == len(ref_outs)
  return outs, grads, ref_outs, ref_grads


def _is_per_row(row, t):
  return not row.scalar and t.dim() >= 1 and t.shape[0] == B


def row0_differences(row, ai, outs, grads, ref_outs, ref_grads):
  """R2: what of batch row 0 is not the clean call's, as a list of messages."""
  found = []
  if not NF.per_row(row, row.args[ai]):
    return found
  for n, (o, r) in enumerate(zip(outs, ref_outs)):
    if _is_per_row(row, o):
      try:
        G._same_bits('output %d, batch row 0' % n, o[0], r[0])
      except AssertionError as e:
        found.append(str(e))
  for i, g in grads.items():
    if g is None or not NF.per_row(row, row.args[i]):
      continue
    try:
      G._same_gradient(row, 'gradient of %s, batch row 0' % row.args[i].name, g[0], ref_grads[i][0])
    except AssertionError as e:
      found.append(str(e))
  return found


def non_finite_outputs(row, ai, outs):
  """R3, weak form: the number of non-finite elements in the outputs of the poisoned batch row."""
  count = 0
  for o in outs:
    if not o.is_floating_point():
      continue
    part = o[B - 1] if (_is_per_row(row, o) and NF.per_row(row, row.args[ai])) else o
    count += int((~torch.isfinite(part)).sum())
  return count


def _cases():
  return [pytest.param(row.name, ai, vname, id='%s-%s-%s' % (row.name, arg.name, vname))
          for row in NF.ROWS for ai, arg in enumerate(row.args) for vname in NF.VALUES]


@pytest.mark.parametrize('name, ai, vname', _cases())
def test_one_non_finite_value_stays_in_its_row_and_does_not_vanish(ddsp, name, ai, vname):
  row = NF.BY_NAME[name]
  arg = row.args[ai]
  result = run_poisoned(ddsp, row, ai, NF.VALUES[vname])                        # R1: it returns
  if result is None:
    return
  outs, grads, ref_outs, ref_grads = result
  if name not in NF.EXEMPT_ROWS:                                                # R2
    found = row0_differences(row, ai, outs, grads, ref_outs, ref_grads)
    assert not found, '%s, %s in %s: %s' % (name, vname, arg.name, '; '.join(found))
  if vname == 'nan':                                                            # R3, weak form
    count = non_finite_outputs(row, ai, outs)
    if (name, arg.name) in NF.KEEPS_FINITE:
      assert count == 0, '%s: KEEPS_FINITE names %s, yet %d output elements are not finite' % (name, arg.name, count)
    else:
      assert count > 0, '%s: the NaN in %s is gone - every output of its batch row is finite' % (name, arg.name)


# ---- R3, strong form -----------------------------------------------------------------------------------------------------
def _dev(x):
  return torch.as_tensor(np.asarray(x, np.float32), device=DEV)


def _mask(x):
  x = x.detach().cpu() if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x))
  return ~torch.isfinite(x.double())


def assert_superset(case, got, truth):
  """Every element the truth makes non-finite is non-finite from the kernel.  The truth's mask must not be empty: a truth that
  drops the planted value would make this test hold nothing."""
  want, have = _mask(truth), _mask(got)
  assert want.shape == have.shape, (case, want.shape, have.shape)
  lost = int((want & ~have).sum())
  print(case, dict(truth=int(want.sum()), kernel=int(have.sum()), lost=lost))
  assert lost == 0, '%s: %d of the %d elements the fp64 truth makes non-finite are finite from the kernel' % (case, lost, int(want.sum()))
  return int(want.sum())


def strong_form(case, fn_ours, fn_truth, inputs, plant, value, needs_grad=None):
  """inputs: numpy fp32 arrays; plant = (input index, element index).  fn_ours(*device tensors) and fn_truth(*fp64 torch tensors)
  -> a tensor or a list of them.  Outputs and the gradient of every input in needs_grad (all by default), cotangent of ones."""
  inputs = [np.array(v, np.float32) for v in inputs]
  inputs[plant[0]][plant[1]] = value
  needs_grad = list(range(len(inputs))) if needs_grad is None else needs_grad

  def run(fn, tensors):
    leaves = [t.requires_grad_(i in needs_grad) for i, t in enumerate(tensors)]
    outs = fn(*leaves)
    outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]
    live = [o for o in outs if o.requires_grad]
    grads = torch.autograd.grad(live, [leaves[i] for i in needs_grad], [torch.ones_like(o) for o in live], allow_unused=True) if live else ()
    return [o.detach() for o in outs], dict(zip(needs_grad, grads))

  outs, grads = run(fn_ours, [_dev(v) for v in inputs])
  t_outs, t_grads = run(fn_truth, [torch.as_tensor(v, dtype=torch.float64) for v in inputs])
  marked = 0
  for n, (o, t) in enumerate(zip(outs, t_outs)):
    marked += assert_superset('%s output %d' % (case, n), o, t)
  # (an Inf may saturate in the truth itself - a sigmoid gate, a floor -, and then there is nothing to keep; a NaN may not)
  assert marked > 0 or value == value, case + ': the truth makes no output element non-finite - the planted NaN reaches nothing'
  for i in needs_grad:
    if t_grads[i] is not None:
      assert grads[i] is not None, (case, i)
      assert_superset('%s gradient of input %d' % (case, i), grads[i], t_grads[i])


VALUES3 = [pytest.param(v, id=k) for k, v in NF.VALUES.items()]


def _rng(seed, *shape, scale=1.0):
  return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(np.float32)


@pytest.mark.parametrize('value', VALUES3)
@pytest.mark.parametrize('relu', [False, True], ids=['plain', 'relu'])
@pytest.mark.parametrize('ch', [4, 16])
def test_dilated_conv_keeps_what_the_truth_keeps(ddsp, ch, relu, value):
  """ch 16: the MFMA kernel; ch 4: the plain one.  The value sits in x (+Inf and NaN survive a ReLU; -Inf becomes 0 in the truth
  too, and then there is nothing to keep)."""
  from ddsp_amd.training import nn
  x, k, b = _rng(1, 2, 5, 6), _rng(2, 3, 6, ch, scale=0.3), _rng(3, ch, scale=0.3)
  strong_form('dilated_conv ch=%d relu=%s' % (ch, relu), lambda x, k, b: nn.dilated_conv(x, k, b, dilation=2, relu_input=relu),
              lambda x, k, b: CT.conv(x, k, b, dilation=2, relu_input=relu), [x, k, b], (0, (1, 2, 3)), value)


@pytest.mark.parametrize('value', VALUES3)
def test_dilated_conv_stack_of_one_layer_keeps_what_the_truth_keeps(ddsp, value):
  """conv_in, then one residual layer: ReLU -> dilated convolution -> layer norm, added to its input.  Weights drawn as
  tests/test_gpu_dilated_conv.py draws them; the output and the gradient in x."""
  import test_gpu_dilated_conv as CG
  from ddsp_amd.training import nn
  stack = nn.DilatedConvStack(ch=16, layers_per_stack=1, stacks=1, norm_type='layer')
  x = _rng(27, 2, 5, 6)
  stack(_dev(x))                                        # builds
  w = CG._draw(stack, np.random.default_rng(26))
  config = CG._stack_config(stack)
  x[1, 2, 3] = value
  xd = _dev(x).requires_grad_(True)
  y = stack(xd)
  gx, = torch.autograd.grad(y, [xd], torch.ones_like(y))
  xt = torch.as_tensor(x, dtype=torch.float64).requires_grad_(True)
  t = CT.stack(xt, None, CG._stack_weights(w, '', config, 0), config)
  gt, = torch.autograd.grad(t, [xt], torch.ones_like(t))
  assert assert_superset('DilatedConvStack output', y.detach(), t.detach()) > 0
  assert_superset('DilatedConvStack gradient of x', gx, gt)


@pytest.mark.parametrize('value', VALUES3)
@pytest.mark.parametrize('ch', [8, 513])
@pytest.mark.parametrize('act', ['linear', 'leaky_relu', 'relu', 'sigmoid', 'tanh'])
def test_bias_norm_act_keeps_what_the_truth_keeps(ddsp, act, ch, value):
  from ddsp_amd.training import nn
  x, b, g, be = _rng(4, 2, 3, ch), _rng(5, ch), _rng(6, ch), _rng(7, ch)
  strong_form('bias_norm_act %s ch=%d' % (act, ch), lambda x, b, g, be: nn.bias_norm_act(x, b, g, be, act),
              lambda x, b, g, be: DT.bias_norm_act(x, b, g, be, act), [x, b, g, be], (0, (1, 1, ch // 2)), value)


@pytest.mark.parametrize('value', VALUES3)
@pytest.mark.parametrize('where', ['mx', 'h0', 'recurrent_kernel'])
@pytest.mark.parametrize('hidden', [3, 16])
def test_gru_keeps_what_the_truth_keeps(ddsp, hidden, where, value):
  """hidden 16: the MFMA kernel; 3: the plain one."""
  from ddsp_amd.training import nn
  h = hidden
  mx, rk, rb, h0 = _rng(8, 2, 4, 3 * h), _rng(9, h, 3 * h, scale=0.3), _rng(10, 3 * h, scale=0.3), _rng(11, 2, h, scale=0.5)
  plant = {'mx': (0, (1, 1, h + 1)), 'h0': (3, (1, 1)), 'recurrent_kernel': (1, (1, 2 * h + 1))}[where]
  strong_form('gru hidden=%d %s' % (h, where), lambda mx, rk, rb, h0: nn.gru_recurrence(mx, rk, rb, h0),
              lambda mx, rk, rb, h0: DT.gru_recurrence(mx, rk, rb, h0), [mx, rk, rb, h0], plant, value)


@pytest.mark.parametrize('value', VALUES3)
@pytest.mark.parametrize('shape', [(2, 5, 2, 64), (2, 70, 1, 256)], ids=['one_block', 'split'])
@pytest.mark.parametrize('norm', ['instance', 'layer', 'group'])
def test_normalize_op_keeps_what_the_truth_keeps(ddsp, norm, shape, value):
  from ddsp_amd.training import nn
  x = _rng(12, *shape)
  strong_form('normalize_op %s %s' % (norm, shape), lambda x: nn.normalize_op(x, norm), lambda x: ET.normalize_op(x, norm), [x],
              (0, (1, shape[1] // 2, 0, shape[3] // 2)), value)


@pytest.mark.parametrize('value', VALUES3)
@pytest.mark.parametrize('fn', ['power_to_db', 'amplitude_to_db'])
def test_db_conversions_keep_what_the_truth_keeps(ddsp, fn, value):
  """core.power_to_db is max(10 log10(max(amin, p)) - ref, -range) (ddsp/core.py:253-277), tf.maximum: a NaN operand is a NaN
  result, as torch.maximum's.  (-Inf is a power below the floor: finite in the truth, and then there is nothing to keep.)"""
  x = np.random.default_rng(13).uniform(1e-3, 2.0, (2, 5, 8)).astype(np.float32)

  def truth(p):
    p = p * p if fn == 'amplitude_to_db' else p
    floor = torch.tensor(10.0 ** (-80.0 / 10.0), dtype=torch.float64)
    return torch.maximum(10.0 * torch.log10(torch.maximum(floor, p)), torch.tensor(-80.0, dtype=torch.float64))
  strong_form(fn, lambda p: getattr(ddsp.core, fn)(p), truth, [x], (0, (1, 2, 3)), value, needs_grad=[])


@pytest.mark.parametrize('value', VALUES3)
@pytest.mark.parametrize('fn', ['compute_loudness', 'compute_power'])
def test_loudness_and_power_keep_what_the_truth_keeps(ddsp, fn, value):
  """Both are a dB conversion of a sum over a frame of samples: every frame that holds the sample is non-finite (NaN, and +-Inf
  through its square or its transform)."""
  audio = _rng(14, 2, 512, scale=0.3)
  n = 137
  if fn == 'compute_power':
    ours = lambda a: ddsp.spectral_ops.compute_power(a, frame_size=128)
    hop = 16000 // 250
    frames = ours(_dev(audio)).shape[1]
    truth_mask = np.zeros((2, frames), bool)
    for f in range(frames):                                            # 'center' padding: frame f covers [f hop - 64, f hop + 64)
      truth_mask[1, f] = f * hop - 64 <= n < f * hop + 64
  else:
    ours = lambda a: ddsp.spectral_ops.compute_loudness(a, n_fft=128)
    frames = ours(_dev(audio)).shape[1]
    hop = 16000 // 250
    truth_mask = np.zeros((2, frames), bool)
    for f in range(frames):
      truth_mask[1, f] = f * hop - 64 <= n < f * hop + 64
  assert truth_mask.any()
  audio[1, n] = value
  got = ours(_dev(audio))
  truth = np.where(truth_mask, np.nan, 0.0).reshape(got.shape)
  assert_superset(fn, got, truth)


@pytest.mark.parametrize('value', VALUES3)
@pytest.mark.parametrize('where', ['phase', 'tables'])
def test_linear_lookup_keeps_what_the_truth_keeps(ddsp, where, value):
  phase = np.random.default_rng(15).uniform(0.0, 1.0, (2, 40)).astype(np.float32)
  tables = _rng(16, 2, 40, 16)
  if where == 'phase':
    phase[1, 7] = value
  else:
    i0 = int(np.floor(phase[1, 7] * 16))
    tables[1, 7, i0 % 16] = value                                      # a point the sample reads
  g = np.ones((2, 40), np.float32)
  with np.errstate(all='ignore'):
    t_out, t_gp, t_gt = WT.linear_lookup(phase, tables, grad_out=g)
  p, w = _dev(phase[:, :, None]).requires_grad_(True), _dev(tables).requires_grad_(True)
  out = ddsp.core.linear_lookup(p, w)
  gp, gw = torch.autograd.grad(out, [p, w], torch.ones_like(out))
  case = 'linear_lookup %s' % where
  assert assert_superset(case + ' output', out.detach().reshape(2, 40), t_out) > 0
  assert_superset(case + ' gradient of phase', gp.reshape(2, 40), t_gp)
  assert_superset(case + ' gradient of tables', gw, t_gt)


@pytest.mark.parametrize('value', VALUES3)
@pytest.mark.parametrize('where', ['phase', 'audio'])
@pytest.mark.parametrize('op', ['variable_length_delay', 'ModDelay'])
def test_delays_keep_what_the_truth_keeps(ddsp, op, where, value):
  n = 320
  audio = _rng(17, 2, n, scale=0.3)
  g = np.ones((2, n), np.float32)
  if op == 'ModDelay':
    gain, phase = _rng(18, 2, n), _rng(19, 2, n)
  else:
    gain, phase = None, np.random.default_rng(19).uniform(0.0, 1.0, (2, n)).astype(np.float32)
  if where == 'phase':
    phase[1, 200] = value
  else:
    audio[1, 200] = value
  a, p = _dev(audio).requires_grad_(True), _dev(phase[:, :, None]).requires_grad_(True)
  with np.errstate(all='ignore'):
    if op == 'ModDelay':
      gn = _dev(gain[:, :, None]).requires_grad_(True)
      out = ddsp.effects.ModDelay()(a, gn, p)
      t_out, t_ga, t_gg, t_gp = WT.mod_delay(audio, gain, phase, grad_out=g)
      ga, gg, gp = torch.autograd.grad(out, [a, gn, p], torch.ones_like(out))
      assert_superset(op + ' gradient of gain', gg.reshape(2, n), t_gg)
    else:
      out = ddsp.core.variable_length_delay(p, a, max_length=64)
      t_out, t_gp, t_ga, _ = WT.variable_length_delay(phase, audio, 64, grad_out=g)
      ga, gp = torch.autograd.grad(out, [a, p], torch.ones_like(out))
  case = '%s %s' % (op, where)
  assert assert_superset(case + ' output', out.detach().reshape(2, n), t_out) > 0 or value == value       # (ModDelay: sigmoid(+-Inf) is 0 or 1)
  assert_superset(case + ' gradient of audio', ga, t_ga)
  assert_superset(case + ' gradient of phase', gp.reshape(2, n), t_gp)


def _stft_mag(x, size, overlap=0.75):
  """|STFT| as ddsp.spectral_ops.compute_mag: frames of `size`, hop size (1 - overlap), Hann, zero padded at the end."""
  hop = int(size * (1.0 - overlap))
  n = x.shape[-1]
  frames = -(-n // hop)
  padded = torch.nn.functional.pad(x, (0, (frames - 1) * hop + size - n))
  window = torch.hann_window(size, periodic=True, dtype=x.dtype)
  return torch.stft(padded, size, hop, size, window, center=False, return_complex=True).abs().transpose(1, 2)


def spectral_loss_truth(target, audio, fft_sizes=(128, 64), mag_weight=1.0, logmag_weight=1.0):
  """losses.SpectralLoss (ddsp/losses.py:144-207) in fp64 torch under autograd: mean |difference| of the magnitudes and of
  safe_log of them."""
  loss = 0.0
  for size in fft_sizes:
    t, v = _stft_mag(target, size), _stft_mag(audio, size)
    loss = loss + mag_weight * (t - v).abs().mean()
    loss = loss + logmag_weight * (torch.log(t + 1e-5) - torch.log(v + 1e-5)).abs().mean()
  return loss


@pytest.mark.parametrize('value', VALUES3)
@pytest.mark.parametrize('deterministic', [False, True], ids=['atomics', 'deterministic'])
def test_spectral_loss_gradient_keeps_what_the_truth_keeps(ddsp, deterministic, value):
  target, audio = _rng(20, 2, 512, scale=0.3), _rng(21, 2, 512, scale=0.3)
  loss = ddsp.losses.SpectralLoss(fft_sizes=(128, 64), logmag_weight=1.0, deterministic=deterministic)
  strong_form('SpectralLoss deterministic=%s' % deterministic, lambda t, a: loss(t, a), spectral_loss_truth, [target, audio],
              (1, (1, 300)), value, needs_grad=[1])


# ---- extreme finite values on the split-fp16 kernels -----------------------------------------------------------------------
SCALES = [pytest.param(1e30, id='1e30'), pytest.param(1e-30, id='1e-30')]


TENSOR_RATIO, TENSOR_FLOOR = 4.0, 8 * 2.0 ** -24       # tests/test_gpu_decoder.py, test_gpu_dilated_conv.py: 4 x the fp32 mode's error, eight ulp


def _scaled_inputs(inputs, which, scale):
  scaled = [np.array(v, np.float32) for v in inputs]
  scaled[which][1] *= np.float32(scale)
  return scaled


def _layer_row_at_scale(case, fn, truth, inputs, which, scale):
  """Batch row 1 of inputs[which] times `scale`: row 0 keeps the bits of the unscaled call, row 1 is held to the tolerance of the
  layer's own module - 4 x the error of the truth's fp32 mode, at least eight fp32 ulp, of the row's largest magnitude."""
  out_clean = fn(*[_dev(v) for v in inputs])
  scaled = _scaled_inputs(inputs, which, scale)
  out = fn(*[_dev(v) for v in scaled])
  G._same_bits(case + ': batch row 0', out[0], out_clean[0])
  want = truth(*scaled)[1].numpy()
  faithful = truth(*scaled, dtype=torch.float32)[1].numpy().astype(np.float64)
  size = float(np.abs(want).max())
  err, ref_err = float(np.abs(out[1].double().cpu().numpy() - want).max()) / size, float(np.abs(faithful - want).max()) / size
  print(case, dict(err=err, reference_fp32_err=ref_err, size=size))
  assert np.isfinite(err) and err <= max(TENSOR_RATIO * ref_err, TENSOR_FLOOR), (case, err, ref_err)


@pytest.mark.parametrize('scale', SCALES)
def test_dilated_conv_row_at_an_extreme_scale(ddsp, scale):
  from ddsp_amd.training import nn
  x, k, b = _rng(1, 2, 5, 6), _rng(2, 3, 6, 16, scale=0.3), np.zeros(16, np.float32)
  _layer_row_at_scale('dilated_conv x %g' % scale, lambda x, k, b: nn.dilated_conv(x, k, b, dilation=2),
                      lambda x, k, b, **kw: CT.conv(x, k, b, dilation=2, **kw), [x, k, b], 0, scale)


@pytest.mark.parametrize('scale', SCALES)
def test_gru_row_at_an_extreme_scale(ddsp, scale):
  """1e30 saturates every gate of the row (the states are +-1 and 0 exactly), 1e-30 leaves the recurrence to the biases."""
  from ddsp_amd.training import nn
  h = 16
  mx, rk, rb, h0 = _rng(8, 2, 4, 3 * h), _rng(9, h, 3 * h, scale=0.3), _rng(10, 3 * h, scale=0.3), _rng(11, 2, h, scale=0.5)
  _layer_row_at_scale('gru mx %g' % scale, lambda *a: nn.gru_recurrence(*a), lambda *a, **kw: DT.gru_recurrence(*a, **kw),
                      [mx, rk, rb, h0], 0, scale)


def _signal_row_at_scale(case, fn, ref, inputs, which, scale):
  """The same for the two entries that are linear in the scaled argument: out(s x) / s against the fp64 result of x, at the
  tolerance tests/test_gpu_parity.py holds them to at any scale (2e-6 + 1e-5 of the largest sample)."""
  out_clean = fn(*[_dev(v) for v in inputs])
  out = fn(*[_dev(v) for v in _scaled_inputs(inputs, which, scale)])
  G._same_bits(case + ': batch row 0', out[0], out_clean[0])
  got = out[1].double().cpu().numpy() / float(np.float32(scale))
  err, tol = float(np.abs(got - ref[1]).max()), 2e-6 + 1e-5 * float(np.abs(ref[1]).max())
  print(case, dict(err=err, tol=tol))
  assert np.isfinite(err) and err <= tol, (case, err, tol)


@pytest.mark.parametrize('scale', SCALES)
def test_fft_convolve_row_at_an_extreme_scale(ddsp, scale):
  from oracle import ddsp_oracle as O
  audio, ir = _rng(22, 2, 512), _rng(23, 2, 8, 128, scale=0.09)
  _signal_row_at_scale('fft_convolve audio %g' % scale, lambda a, h: ddsp.core.fft_convolve(a, h), O.fft_convolve(audio, ir, dtype=np.float64),
                       [audio, ir], 0, scale)


@pytest.mark.parametrize('scale', SCALES)
def test_filtered_noise_row_of_supplied_noise_at_an_extreme_scale(ddsp, scale):
  from oracle import ddsp_oracle as O
  mags = _rng(24, 2, 8, 65)
  noise = np.random.default_rng(25).uniform(-1.0, 1.0, (2, 512)).astype(np.float32)
  _signal_row_at_scale('FilteredNoise noise %g' % scale, lambda m, z: ddsp.synths.FilteredNoise(n_samples=512, window_size=0)(m, noise=z),
                       O.filtered_noise(mags, noise, 0, dtype=np.float64), [mags, noise], 1, scale)


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  import ddsp_amd.training.nn  # noqa: F401
  assert G.DEV == DEV, 'the helpers of tests/test_gpu_layouts.py must run on the device this module runs on'
  return ddsp_amd
