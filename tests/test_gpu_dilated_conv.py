"""ddsp_amd.training.nn's dilated_conv, Conv2D, Conv2DTranspose and DilatedConvStack and training.decoders.DilatedConvDecoder on the
MI355X against tests/dilated_conv_truth.py (the reference's arithmetic as explicit shifted sums in fp64 at the fp32 inputs).
tests/test_dilated_conv_emulated.py runs this module through the SIMT emulation on the CPU.

Tolerances are those of tests/test_gpu_decoder.py: an output's error against the fp64 truth may be up to
4 x that of the truth's fp32 mode on the same case, with a floor of eight fp32 ulp of the tensor's largest magnitude; each
gradient 2e-4 of its largest element.  Every comparison is appended to the file DDSP_PARITY_LOG names, when it is set.

Convolution cases (batch, time, ch_in, ch_out, K, dilation), the smallest at which each part can go wrong: the smallest shape; the
reference test's widths (plain kernel); one MFMA tile shorter than 16 rows with K shorter than a 32-deep step, the halo past both
ends, and (dilation 8 on 5 rows) the outer taps wholly in the padding; one row past a tile with a K tail; even K (asymmetric
padding); conv_in of the shipped decoder (2 -> 128); the shipped width on more than one 64-row block; 17 column tiles (three
column chunks, the last of one tile); the full length at the largest shipped dilation.  Each runs forward and for all three
gradients, with and without ReLU.  Kernels are drawn at sqrt(2 / (K ch_in)): a layer neither dies nor grows.

Bit-stability is claimed for dilated_conv only (forward and the gradient in x): the framework's matrix products and reductions
may pick their kernels by the row count.

Measured on the MI355X: see profiles/dilated_conv_parity_errors.jsonl and DESIGN.md section 8."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import dilated_conv_truth as T
from ddsp_amd import _lib
from ddsp_amd.training import decoders, nn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRAD_RTOL = 2e-4
TENSOR_RATIO = 4.0
TENSOR_FLOOR = 8 * 2.0 ** -24          # eight fp32 ulp of the tensor's largest magnitude

CONV_CASES = [(1, 1, 1, 1, 1, 1), (1, 20, 2, 4, 3, 1), (1, 20, 4, 4, 3, 4), (2, 5, 16, 16, 3, 2), (2, 5, 16, 16, 3, 8), (2, 17, 48, 32, 3, 1),
              (2, 9, 16, 16, 2, 1), (2, 9, 16, 16, 4, 3), (2, 33, 2, 128, 3, 1), (3, 70, 128, 128, 3, 16), (2, 20, 32, 272, 3, 2),
              (1, 1000, 16, 16, 3, 256)]
SHIPPED = (3, 70, 128, 128, 3, 16)


def _log(case, **figures):
  print(case, figures)
  path = os.environ.get('DDSP_PARITY_LOG')
  if path:
    with open(path, 'a') as f:
      f.write(json.dumps(dict(case=case, **{k: float(v) for k, v in figures.items()})) + '\n')


def _dev(*arrays, grad=False):
  return [torch.as_tensor(a, device=DEV).requires_grad_(grad) for a in arrays]


def _np(x):
  return x.detach().cpu().numpy().astype(np.float64)


def _check_tensor(case, got, truth, faithful):
  got, truth, faithful = _np(got), np.asarray(truth, np.float64), np.asarray(faithful, np.float64)
  scale = float(np.max(np.abs(truth)))
  scale = scale if scale > 0.0 else 1.0
  err = float(np.max(np.abs(got - truth))) / scale
  ref_err = float(np.max(np.abs(faithful - truth))) / scale
  _log(case, kernel_err=err, reference_fp32_err=ref_err, scale=scale)
  assert got.shape == truth.shape and np.isfinite(got).all()
  assert err <= max(TENSOR_RATIO * ref_err, TENSOR_FLOOR), (case, err, ref_err)


def _check_grad(case, got, truth, scale=None):
  """2e-4 of the gradient's largest element (`scale`, where the caller knows the gradient to be zero by construction)."""
  g = _np(got)
  scale = scale or max(float(np.max(np.abs(truth))), 1e-30)
  err = float(np.max(np.abs(g - truth))) / scale
  _log(case, grad_err=err, scale=scale)
  assert g.shape == truth.shape and np.isfinite(g).all()
  assert err <= GRAD_RTOL, (case, err)


def _rng(name):
  return np.random.default_rng(zlib.crc32(('dilated_conv/' + name).encode()))


def _f32(rng, *shape, scale=1.0, shift=0.0):
  return (shift + scale * rng.standard_normal(shape)).astype(np.float32)


def _kernel_scale(taps, ch_in):
  return float(np.sqrt(2.0 / (taps * ch_in)))


# ---- the convolution ------------------------------------------------------------------------------------------------------
def _truths(ins, cot, dilation, relu):
  fn = lambda *a, **k: T.conv(*a, dilation=dilation, relu_input=relu, **k)
  return dict(ins=ins, cot=cot, truth=fn(*ins).numpy(), fp32=fn(*ins, dtype=torch.float32).numpy(), grads=T.grads(fn, ins, [cot]))


@functools.lru_cache(maxsize=None)
def _conv_case(batch, steps, ch_in, ch_out, taps, dilation, relu, x_scale=1.0, loud_row=None):
  rng = _rng('conv/%d/%d/%d/%d/%d/%d' % (batch, steps, ch_in, ch_out, taps, dilation))
  x = _f32(rng, batch, steps, ch_in) * np.float32(x_scale)
  if loud_row is not None:
    x[loud_row] *= np.float32(1e4)
  ins = (x, _f32(rng, taps, ch_in, ch_out, scale=_kernel_scale(taps, ch_in)), _f32(rng, ch_out, scale=0.1 * x_scale))
  return _truths(ins, _f32(rng, batch, steps, ch_out), dilation, relu)


def _run_conv(c, dilation, relu):
  ins = _dev(*c['ins'], grad=True)
  with torch.no_grad():
    plain = nn.dilated_conv(*ins, dilation=dilation, relu_input=relu)             # the forward-only route
  y = nn.dilated_conv(*ins, dilation=dilation, relu_input=relu)
  assert y.requires_grad and not plain.requires_grad and torch.equal(y.detach(), plain)
  return y, torch.autograd.grad(y, ins, _dev(c['cot'])[0])


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('batch, steps, ch_in, ch_out, taps, dilation', CONV_CASES)
def test_dilated_conv(ddsp, batch, steps, ch_in, ch_out, taps, dilation, relu):
  c = _conv_case(batch, steps, ch_in, ch_out, taps, dilation, relu)
  name = 'conv/b%d_t%d_i%d_o%d_k%d_d%d/%s' % (batch, steps, ch_in, ch_out, taps, dilation, 'relu' if relu else 'linear')
  y, grads = _run_conv(c, dilation, relu)
  _check_tensor(name + '/y', y, c['truth'], c['fp32'])
  for which, got, want in zip(('x', 'kernel', 'bias'), grads, c['grads']):
    _check_grad('%s/grad_%s' % (name, which), got, want)


def test_dilated_conv_takes_keras_layouts_and_no_bias(ddsp):
  c = _conv_case(2, 9, 16, 16, 4, 3, True)
  x, kernel, _ = _dev(*c['ins'], grad=True)
  y = nn.dilated_conv(x[:, :, None, :], kernel[:, None], None, dilation=3, relu_input=True)
  assert y.shape == (2, 9, 1, 16)
  truth = lambda x_, k_, **kw: T.conv(x_, k_, None, 3, True, **kw)
  _check_tensor('conv/keras_layouts/y', y[:, :, 0], truth(*c['ins'][:2]).numpy(), truth(*c['ins'][:2], dtype=torch.float32).numpy())
  for which, got, want in zip(('x', 'kernel'), torch.autograd.grad(y, [x, kernel], _dev(c['cot'])[0][:, :, None, :]),
                              T.grads(truth, c['ins'][:2], [c['cot']])):
    _check_grad('conv/keras_layouts/grad_' + which, got, want)


@pytest.mark.parametrize('variant', ['x_1e-6', 'x_1e6', 'row_1e4'])
def test_dilated_conv_at_any_scale_error_per_batch_row(ddsp, variant):
  """Activations are not assumed to lie in fp16's range, and a quiet batch row keeps its bits of precision beside a loud one: the
  error of every batch row is measured against that row's own largest magnitude."""
  kw = {'x_1e-6': dict(x_scale=1e-6), 'x_1e6': dict(x_scale=1e6), 'row_1e4': dict(loud_row=1)}[variant]
  c = _conv_case(*SHIPPED, True, **kw)
  y, grads = _run_conv(c, SHIPPED[5], True)
  for row in range(SHIPPED[0]):
    _check_tensor('conv/%s/row%d/y' % (variant, row), y[row], c['truth'][row], c['fp32'][row])
    _check_grad('conv/%s/row%d/grad_x' % (variant, row), grads[0][row], c['grads'][0][row])
  for which, got, want in zip(('kernel', 'bias'), grads[1:], c['grads'][1:]):
    _check_grad('conv/%s/grad_%s' % (variant, which), got, want)


@pytest.mark.parametrize('ch', [4, 16], ids=['plain', 'mfma'])
def test_relu_gradient_is_zero_at_zero_and_below(ddsp, ch):
  rng = _rng('relu_at_zero/%d' % ch)
  x = _f32(rng, 2, 9, ch)
  x[rng.random(x.shape) < 0.3] = 0.0
  x[0, 0, 0], x[1, 8, ch - 1] = 0.0, -0.0
  ins = (x, _f32(rng, 3, ch, ch, scale=_kernel_scale(3, ch)), _f32(rng, ch, scale=0.1))
  c = _truths(ins, _f32(rng, 2, 9, ch), 2, True)
  y, grads = _run_conv(c, 2, True)
  _check_tensor('conv/relu_at_zero/%d/y' % ch, y, c['truth'], c['fp32'])
  dead = torch.as_tensor(x <= 0.0)
  assert bool(dead.any()) and not bool(grads[0].cpu()[dead].any()) and bool(grads[0].cpu()[~dead].all())
  for which, got, want in zip(('x', 'kernel', 'bias'), grads, c['grads']):
    _check_grad('conv/relu_at_zero/%d/grad_%s' % (ch, which), got, want)


@pytest.mark.parametrize('ch', [4, 16], ids=['plain', 'mfma'])
def test_the_adjoint_folds_an_addend_into_its_epilogue(ddsp, ch):
  """The entry's optional addend (the residual branch's gradient): one fp32 addition behind the masked sum."""
  rng = _rng('addend/%d' % ch)
  dy, x, addend = _dev(_f32(rng, 2, 9, ch), _f32(rng, 2, 9, ch), _f32(rng, 2, 9, ch))
  kernel, = _dev(_f32(rng, 3, ch, ch, scale=_kernel_scale(3, ch)))
  flags = _lib.CONVD_TRANSPOSE_W | _lib.CONVD_MASK_OUTPUT
  pad = 2 * 2 - nn.same_pad_left(3, 2)
  without = nn._run_dilated_conv(dy, kernel, None, 2, pad, flags, mask_src=x)
  with_addend = nn._run_dilated_conv(dy, kernel, None, 2, pad, flags, mask_src=x, addend=addend)
  assert torch.equal(with_addend, without + addend) and bool(without.any())


def test_limits_raise_before_any_launch(ddsp):
  reached = []
  load = _lib.load

  class Counting:
    def __getattr__(self, name):
      reached.append(name)
      return getattr(load(), name)

  x, = _dev(np.zeros((1, 1, 2), np.float32))
  try:
    _lib.load = Counting
    for bad_x, kernel, dilation in [(torch.zeros(1, 4, 1040), torch.zeros(1, 1040, 16), 1), (torch.zeros(1, 4, 2), torch.zeros(3, 2, 1040), 1),
                                    (torch.zeros(1, 4, 2), torch.zeros(17, 2, 4), 1), (torch.zeros(1, 4, 2), torch.zeros(3, 2, 4), 2 ** 30),
                                    (x.expand(1 << 16, 1 << 14, 2), torch.zeros(3, 2, 4), 1), (x.expand(1 << 16, 1 << 5, 2), torch.zeros(3, 2, 1024), 1)]:
      with pytest.raises(ValueError, match='MI355X path|2 \\*\\* 31'):
        nn.dilated_conv(bad_x, kernel, None, dilation)
  finally:
    _lib.load = load
  assert not reached


# ---- the resamplers (framework ops) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('steps, stride', [(8, 2), (9, 2), (10, 3)])
def test_strided_conv2d_and_conv2d_transpose(ddsp, steps, stride):
  rng = _rng('resample/%d/%d' % (steps, stride))
  x_host, cot_down, cot_up = _f32(rng, 2, steps, 3), _f32(rng, 2, -(-steps // stride), 4), _f32(rng, 2, steps * stride, 4)
  for name, layer, truth, cot in (('down', nn.Conv2D(4, stride, stride), T.downsample, cot_down),
                                  ('up', nn.Conv2DTranspose(4, 2 * stride, stride), T.upsample, cot_up)):
    layer.build(3)
    w = _draw(layer, rng)
    x, = _dev(x_host, grad=True)
    y = layer(x)
    fn = lambda *a, **k: truth(*a, stride, **k)
    ins = (x_host, w['kernel'], w['bias'])
    case = 'resample/%s/t%d_s%d' % (name, steps, stride)
    _check_tensor(case + '/y', y, fn(*ins).numpy(), fn(*ins, dtype=torch.float32).numpy())
    assert layer(x[:, :, None, :]).shape == (2, cot.shape[1], 1, 4)
    for which, got, want in zip(('x', 'kernel', 'bias'), torch.autograd.grad(y, [x, layer.kernel, layer.bias], _dev(cot)[0]), T.grads(fn, ins, [cot])):
      _check_grad('%s/grad_%s' % (case, which), got, want)


# ---- the stack and the decoder ------------------------------------------------------------------------------------------------
def _draw(module, rng):
  """Overwrites every weight of a BUILT module with drawn values and returns them by parameter name: convolution kernels at
  sqrt(2 / fan_in) (He: a ReLU layer keeps its scale), Dense kernels at 0.3 / sqrt(fan_in / 16), the norms' scales near 0.3 -
  eighteen residual layers stay of order 1 - and everything else at 0.1."""
  out = {}
  with torch.no_grad():
    for name, param in module.named_parameters():
      leaf = name.rsplit('.', 1)[-1]
      if leaf == 'kernel' and param.dim() == 4:
        value = _f32(rng, *param.shape, scale=_kernel_scale(param.shape[0], param.shape[2]))
      elif leaf == 'kernel':
        value = _f32(rng, *param.shape, scale=0.3 / np.sqrt(max(param.shape[0] / 16.0, 1.0)))
      elif leaf == 'scale':
        value = _f32(rng, *param.shape, scale=0.03, shift=0.3)
      else:
        value = _f32(rng, *param.shape, scale=0.1)
      param.copy_(torch.as_tensor(value))
      out[name] = value
  return out


def _stack_config(stack):
  resample = stack.resample_layers[0] if len(stack.resample_layers) else None
  return dict(dilations=[layer.conv.dilation_rate for layer in stack.layers], norm_type=stack.norm_type, conditional=stack.conditional,
              shift_only=stack.conditional and stack.norms[0].conditional_scale_and_shift.shift_only,
              resample_type=None if resample is None else ('upsample' if isinstance(resample, nn.Conv2DTranspose) else 'downsample'),
              resample_stride=None if resample is None else resample.strides, layers_per_resample=stack.layers_per_resample,
              resample_after_convolve=stack.resample_after_convolve)


def _stack_weights(w, prefix, config, n_resample):
  norm = ('conditional_scale_and_shift.dense.kernel', 'conditional_scale_and_shift.dense.bias') if config['conditional'] else ('scale', 'shift')
  pair = lambda stem, leaves=('kernel', 'bias'): tuple(w['%s%s.%s' % (prefix, stem, leaf)] for leaf in leaves)
  n = len(config['dilations'])
  return dict(conv_in=pair('conv_in'), layers=[pair('layers.%d.conv' % i) for i in range(n)], norms=[pair('norms.%d' % i, norm) for i in range(n)],
              resample=[pair('resample_layers.%d' % i) for i in range(n_resample)])


def _structural_zero_scale(which, want):
  """A convolution's bias in front of a normalisation whose groups are single channels ('instance'; 'group' at 32 channels) has a
  gradient of exactly 0: the norm subtracts each channel's mean over time.  The fp64 truth gives its own rounding (1e-15), of which
  no fp32 sum of the same cotangents can be within 2e-4.  Such a gradient - the truth's largest element below 1e-12 of the same
  convolution's kernel gradient - is held to 2e-4 of THAT gradient's largest element instead: both are sums of the same
  cotangents over batch and time, the kernel's weighted by activations of order 1.  -> that scale, or None for the usual rule."""
  if not which.endswith('.conv.bias'):
    return None
  kernel_scale = float(np.max(np.abs(want[which[:-len('bias')] + 'kernel'])))
  return kernel_scale if float(np.max(np.abs(want[which]))) < 1e-12 * kernel_scale else None


def _check_stack(name, batch, steps, ch_in, z_ch, **kwargs):
  rng = _rng(name)
  stack = nn.DilatedConvStack(**kwargs)
  x_host, z_host = _f32(rng, batch, steps, ch_in), _f32(rng, batch, steps, z_ch)
  x, z = _dev(x_host, z_host, grad=True)
  feed = [x, z] if stack.conditional else x
  stack(feed)                                           # builds
  w = _draw(stack, rng)
  names = list(w)
  config = _stack_config(stack)
  y = stack(feed)

  def fn(*args, dtype=torch.float64):
    ins, rest = (args[:2], args[2:]) if stack.conditional else ((args[0], None), args[1:])
    return T.stack(ins[0], ins[1], _stack_weights(dict(zip(names, rest)), '', config, len(stack.resample_layers)), config, dtype=dtype)

  args = [x_host] + ([z_host] if stack.conditional else []) + [w[n] for n in names]
  truth = fn(*args)
  assert y.shape == truth.shape
  _check_tensor(name + '/y', y, truth.numpy(), fn(*args, dtype=torch.float32).numpy())
  cot = _f32(rng, *truth.shape)
  leaves = [x] + ([z] if stack.conditional else []) + [p for _, p in stack.named_parameters()]
  grads = torch.autograd.grad(y, leaves, _dev(cot)[0])
  labels = ['x'] + (['z'] if stack.conditional else []) + names
  want = dict(zip(labels, T.grads(fn, args, [cot])))
  for which, got in zip(labels, grads):
    _check_grad('%s/grad_%s' % (name, which), got, want[which], scale=_structural_zero_scale(which, want))
  return stack


@pytest.mark.parametrize('mode', ['unconditional', 'film', 'shift_only'])
@pytest.mark.parametrize('norm_type', [None, 'layer', 'instance', 'group'])
def test_dilated_conv_stack(ddsp, norm_type, mode):
  stack = _check_stack('stack/%s/%s' % (norm_type, mode), 2, 12, 3, 5, ch=32, layers_per_stack=3, stacks=2, dilation=-2, norm_type=norm_type,
                       conditional=mode != 'unconditional', shift_only=mode == 'shift_only')
  assert [layer.conv.dilation_rate for layer in stack.layers] == [4, 2, 1, 4, 2, 1]


@pytest.mark.parametrize('after', [True, False], ids=['resample_after', 'resample_before'])
@pytest.mark.parametrize('resample_type', ['upsample', 'downsample'])
def test_dilated_conv_stack_resamples(ddsp, resample_type, after):
  stack = _check_stack('stack/%s/%s' % (resample_type, 'after' if after else 'before'), 2, 12, 3, 5, ch=16, layers_per_stack=2, stacks=2,
                       norm_type='layer', resample_type=resample_type, resample_stride=2, resample_after_convolve=after)
  assert len(stack.resample_layers) == 2


def _check_decoder(name, batch, steps, z_ch, splits, **kwargs):
  rng = _rng(name)
  keys = ['ld_scaled', 'f0_scaled']
  dec = decoders.DilatedConvDecoder(input_keys=keys, output_splits=splits, conditioning_keys=('z',) if z_ch else None, **kwargs)
  host = {k: _f32(rng, batch, steps, 1) for k in keys}
  if z_ch:
    host['z'] = _f32(rng, batch, steps, z_ch)
  feed = {k: _dev(v)[0] for k, v in host.items()}
  out = dec(feed)                                       # builds
  out_keys = [k for k, _ in splits]
  assert list(out) == out_keys and dec.input_keys == keys + (['z'] if z_ch else [])
  w = _draw(dec, rng)
  names = list(w)
  stack = dec.dilated_conv_stack
  config = _stack_config(stack)
  out = dec(feed)
  for (k, n) in splits:
    assert out[k].shape == (batch, steps, n)

  def fn(*args, dtype=torch.float64):
    ins, rest = args[:len(host)], dict(zip(names, args[len(host):]))
    weights = _stack_weights(rest, 'dilated_conv_stack.', config, 0)
    weights['dense_out'] = (rest['dense_out.kernel'], rest['dense_out.bias'])
    return T.decoder(ins[:2], ins[2:], weights, config, splits, dtype=dtype)

  args = [host[k] for k in host] + [w[n] for n in names]
  truth, fp32 = fn(*args), fn(*args, dtype=torch.float32)
  for k, a, b in zip(out_keys, truth, fp32):
    _check_tensor('%s/%s' % (name, k), out[k], a.numpy(), b.numpy())
  cots = [_f32(rng, *t.shape) for t in truth]
  grads = torch.autograd.grad([out[k] for k in out_keys], [p for _, p in dec.named_parameters()], _dev(*cots))
  want = T.grads(fn, args, cots)[len(host):]
  assert len(grads) == len(names) == len(want)
  for which, got, truth_grad in zip(names, grads, want):          # every weight
    _check_grad('%s/grad_%s' % (name, which), got, truth_grad)


@pytest.mark.parametrize('z_ch', [0, 6], ids=['no_z', 'z'])
def test_dilated_conv_decoder_at_the_reference_test_configuration(ddsp, z_ch):
  """ddsp/training/decoders_test.py: ch=4, layers_per_stack=3, stacks=2, splits (1, 10, 10), batch 1, 20 steps."""
  _check_decoder('decoder/small/' + ('z' if z_ch else 'no_z'), 1, 20, z_ch, (('amps', 1), ('harmonic_distribution', 10), ('noise_magnitudes', 10)),
                 ch=4, layers_per_stack=3, stacks=2)


@pytest.mark.parametrize('z_ch', [0, 16], ids=['no_z', 'z'])
def test_dilated_conv_decoder_at_the_midiae_configuration(ddsp, z_ch):
  """gin/models/midiae/midiae.gin: ch=128, layers_per_stack=9, stacks=2, norm_type='layer', splits (1, 60, 65); 30 frames."""
  _check_decoder('decoder/midiae/' + ('z' if z_ch else 'no_z'), 2, 30, z_ch, (('amplitudes', 1), ('harmonic_distribution', 60), ('magnitudes', 65)),
                 ch=128, layers_per_stack=9, stacks=2, norm_type='layer')


# ---- bit-stability of the hand-written kernel ------------------------------------------------------------------------------
def _conv_everything(x, kernel, bias, cot, dilation):
  leaves = _dev(x, kernel, bias, grad=True)
  y = nn.dilated_conv(*leaves, dilation=dilation, relu_input=True)
  dx, = torch.autograd.grad(y, leaves[:1], _dev(cot)[0])
  return [y.detach(), dx]


@pytest.mark.parametrize('batch, steps, ch_in, ch_out, taps, dilation', [(3, 20, 4, 4, 3, 4), (3, 70, 48, 32, 3, 2)])
def test_dilated_conv_same_bits_twice_row_alone_and_sub_batch(ddsp, batch, steps, ch_in, ch_out, taps, dilation):
  c = _conv_case(batch, steps, ch_in, ch_out, taps, dilation, True, loud_row=1)     # the rows differ in scale by 1e4
  (x, kernel, bias), cot = c['ins'], c['cot']
  first, second = _conv_everything(x, kernel, bias, cot, dilation), _conv_everything(x, kernel, bias, cot, dilation)
  for a, b in zip(first, second):
    assert torch.equal(a, b)
  for rows in (slice(0, 1), slice(2, 3), slice(1, 3)):                              # a row alone, the last alone, a sub-batch
    for a, r in zip(first, _conv_everything(x[rows], kernel, bias, cot[rows], dilation)):
      assert torch.equal(a[rows], r)


def test_dilated_conv_replays_from_a_captured_graph(ddsp):
  """No host synchronisation, no allocation by the library, every launch on the current stream in one chain: forward and
  backward are captured once with torch.cuda.graph and replayed - the same bits as the eager call."""
  if DEV != 'cuda' or not torch.cuda.is_available():
    pytest.skip('needs real streams and graphs: left to the GPU run')
  rng = _rng('graph/conv')
  host = [_f32(rng, 2, 20, 16), _f32(rng, 3, 16, 32, scale=_kernel_scale(3, 16)), _f32(rng, 32, scale=0.1)]
  other = _f32(rng, 2, 20, 16, scale=3.0)
  static = _dev(*host, grad=True)
  cot, = _dev(_f32(rng, 2, 20, 32))

  def step(leaves):
    y = nn.dilated_conv(*leaves, dilation=2, relu_input=True)
    return [y] + list(torch.autograd.grad(y, leaves, cot))

  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    step(static)
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    captured = step(static)
  for x_new in (host[0], other, other):
    with torch.no_grad():
      static[0].copy_(torch.as_tensor(x_new))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, step(_dev(x_new, *host[1:], grad=True))):
      assert torch.equal(a.detach(), b.detach())


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  return ddsp_amd
