"""ddsp_amd.training.nn's conv2d, SpatialConv2D, MaxPool2D, NormReluConv, ResidualLayer, ResidualStack and ResNet and
training.encoders' ResnetSinusoidalEncoder and SinusoidalToHarmonicEncoder on the MI355X against tests/resnet_truth.py (the
reference's arithmetic as explicit shifted sums in fp64 at the fp32 inputs).  tests/test_resnet_emulated.py runs this module
through the SIMT emulation on the CPU.

Tolerances are those of tests/test_gpu_dilated_conv.py: an output's error against the fp64 truth may be up to
4 x that of the truth's fp32 mode on the same case, with a floor of eight fp32 ulp of the tensor's largest magnitude; each
gradient 2e-4 of its largest element; a gradient that is zero by construction (a convolution's bias in front of a normalisation
that subtracts every channel's own mean) is held to 2e-4 of the same convolution's kernel gradient, as _structural_zero_scale
argues there.  Every comparison is appended to the file DDSP_PARITY_LOG names, when it is set.

Convolution cases (batch, H, W, ch_in, ch_out, kh, kw, sh, sw), the smallest at which each part can go wrong: the smallest shape;
the plain kernel; an even width at stride 2 (no column of padding in front, one behind) and an odd one (one and one); the stem (one
channel, 49 taps in two 32-deep steps, an image lower than the kernel so that whole tap rows lie in the padding); a K tail with
64-position runs that cross image rows and end mid-row; several blocks per batch row; a 1 x 1 with 17 column tiles (three column
chunks); the strided projection; even kernels with strides on both axes and stride 3 (every phase of the adjoint's divisibility
test); ch_in a multiple of 8 but not of 32.  Each runs forward and for all three gradients, with and without ReLU.  Kernels are
drawn at sqrt(2 / (kh kw ch_in)): a layer neither dies nor grows.

Bit-stability is claimed for conv2d only (forward and the gradient in x): the framework's matrix products and reductions may pick
their kernels by the row count.

Measured on the MI355X: see profiles/resnet_parity_errors.jsonl and DESIGN.md section 8."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import resnet_truth as T
from ddsp_amd import _lib, spectral_ops
from ddsp_amd.training import encoders, nn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRAD_RTOL = 2e-4
TENSOR_RATIO = 4.0
TENSOR_FLOOR = 8 * 2.0 ** -24          # eight fp32 ulp of the tensor's largest magnitude

CONV_CASES = [(1, 1, 1, 1, 1, 1, 1, 1, 1), (1, 5, 6, 2, 4, 3, 3, 1, 1), (2, 5, 6, 16, 16, 3, 3, 1, 2), (2, 5, 7, 16, 16, 3, 3, 1, 2),
              (2, 3, 9, 1, 16, 7, 7, 1, 2), (2, 9, 11, 48, 32, 3, 3, 1, 1), (2, 70, 5, 32, 32, 3, 3, 1, 2), (1, 4, 5, 32, 272, 1, 1, 1, 1),
              (2, 4, 8, 16, 32, 1, 1, 1, 2), (2, 6, 10, 16, 16, 2, 4, 2, 3), (2, 3, 4, 24, 16, 3, 3, 1, 1)]
SCALE_CASE = (3, 9, 11, 48, 32, 3, 3, 1, 1)


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
  return np.random.default_rng(zlib.crc32(('resnet/' + name).encode()))


def _f32(rng, *shape, scale=1.0, shift=0.0):
  return (shift + scale * rng.standard_normal(shape)).astype(np.float32)


def _kernel_scale(kh, kw, ch_in):
  return float(np.sqrt(2.0 / (kh * kw * ch_in)))


def _out_shape(batch, h, w, ch_out, kh, kw, sh, sw):
  return batch, T.same_padding(h, kh, sh)[0], T.same_padding(w, kw, sw)[0], ch_out


# ---- the convolution ------------------------------------------------------------------------------------------------------
def _truths(ins, cot, strides, relu):
  fn = lambda *a, **k: T.conv2d(*a, strides=strides, relu_input=relu, **k)
  return dict(ins=ins, cot=cot, truth=fn(*ins).numpy(), fp32=fn(*ins, dtype=torch.float32).numpy(), grads=T.grads(fn, ins, [cot]))


@functools.lru_cache(maxsize=None)
def _conv_case(batch, h, w, ch_in, ch_out, kh, kw, sh, sw, relu, x_scale=1.0, loud_row=None):
  rng = _rng('conv/' + '/'.join(str(v) for v in (batch, h, w, ch_in, ch_out, kh, kw, sh, sw)))
  x = _f32(rng, batch, h, w, ch_in) * np.float32(x_scale)
  if loud_row is not None:
    x[loud_row] *= np.float32(1e4)
  ins = (x, _f32(rng, kh, kw, ch_in, ch_out, scale=_kernel_scale(kh, kw, ch_in)), _f32(rng, ch_out, scale=0.1 * x_scale))
  return _truths(ins, _f32(rng, *_out_shape(batch, h, w, ch_out, kh, kw, sh, sw)), (sh, sw), relu)


def _run_conv(c, strides, relu):
  ins = _dev(*c['ins'], grad=True)
  with torch.no_grad():
    plain = nn.conv2d(*ins, strides=strides, relu_input=relu)                        # the forward-only route
  y = nn.conv2d(*ins, strides=strides, relu_input=relu)
  assert y.requires_grad and not plain.requires_grad and torch.equal(y.detach(), plain)
  return y, torch.autograd.grad(y, ins, _dev(c['cot'])[0])


def _case_name(case):
  return 'b%d_h%d_w%d_i%d_o%d_k%dx%d_s%dx%d' % case


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('case', CONV_CASES, ids=_case_name)
def test_conv2d(ddsp, case, relu):
  c = _conv_case(*case, relu)
  name = 'conv2d/%s/%s' % (_case_name(case), 'relu' if relu else 'linear')
  y, grads = _run_conv(c, case[7:], relu)
  _check_tensor(name + '/y', y, c['truth'], c['fp32'])
  for which, got, want in zip(('x', 'kernel', 'bias'), grads, c['grads']):
    _check_grad('%s/grad_%s' % (name, which), got, want)


@pytest.mark.parametrize('variant', ['x_1e-6', 'x_1e6', 'row_1e4'])
def test_conv2d_at_any_scale_error_per_batch_row(ddsp, variant):
  """Activations are not assumed to lie in fp16's range, and a quiet batch row keeps its bits of precision beside a loud one: the
  error of every batch row is measured against that row's own largest magnitude."""
  kw = {'x_1e-6': dict(x_scale=1e-6), 'x_1e6': dict(x_scale=1e6), 'row_1e4': dict(loud_row=1)}[variant]
  c = _conv_case(*SCALE_CASE, True, **kw)
  y, grads = _run_conv(c, SCALE_CASE[7:], True)
  for row in range(SCALE_CASE[0]):
    _check_tensor('conv2d/%s/row%d/y' % (variant, row), y[row], c['truth'][row], c['fp32'][row])
    _check_grad('conv2d/%s/row%d/grad_x' % (variant, row), grads[0][row], c['grads'][0][row])
  for which, got, want in zip(('kernel', 'bias'), grads[1:], c['grads'][1:]):
    _check_grad('conv2d/%s/grad_%s' % (variant, which), got, want)


@pytest.mark.parametrize('ch', [4, 16], ids=['plain', 'mfma'])
def test_relu_gradient_is_zero_at_zero_and_below(ddsp, ch):
  rng = _rng('relu_at_zero/%d' % ch)
  x = _f32(rng, 2, 5, 6, ch)
  x[rng.random(x.shape) < 0.3] = 0.0
  x[0, 0, 0, 0], x[1, 4, 5, ch - 1] = 0.0, -0.0
  ins = (x, _f32(rng, 3, 3, ch, ch, scale=_kernel_scale(3, 3, ch)), _f32(rng, ch, scale=0.1))
  c = _truths(ins, _f32(rng, 2, 5, 3, ch), (1, 2), True)
  y, grads = _run_conv(c, (1, 2), True)
  _check_tensor('conv2d/relu_at_zero/%d/y' % ch, y, c['truth'], c['fp32'])
  dead = torch.as_tensor(x <= 0.0)
  assert bool(dead.any()) and not bool(grads[0].cpu()[dead].any()) and bool(grads[0].cpu()[~dead].all())
  for which, got, want in zip(('x', 'kernel', 'bias'), grads, c['grads']):
    _check_grad('conv2d/relu_at_zero/%d/grad_%s' % (ch, which), got, want)


@pytest.mark.parametrize('ch', [4, 16], ids=['plain', 'mfma'])
def test_the_addend_in_the_epilogue_is_the_separate_add_to_the_bit(ddsp, ch):
  """One fp32 addition behind the biased sum, forward (the residual connection) and in the adjoint's entry; its gradient is the
  cotangent itself."""
  rng = _rng('addend/%d' % ch)
  x, kernel, bias = _dev(_f32(rng, 2, 5, 6, ch), _f32(rng, 3, 3, ch, ch, scale=_kernel_scale(3, 3, ch)), _f32(rng, ch, scale=0.1))
  addend, cot = _dev(_f32(rng, 2, 5, 3, ch), _f32(rng, 2, 5, 3, ch))
  without = nn.conv2d(x, kernel, bias, (1, 2), relu_input=True)
  assert torch.equal(nn.conv2d(x, kernel, bias, (1, 2), relu_input=True, addend=addend), without + addend) and bool(without.any())
  addend.requires_grad_(True)
  grad, = torch.autograd.grad(nn.conv2d(x, kernel, bias, (1, 2), relu_input=True, addend=addend), [addend], cot)
  assert torch.equal(grad, cot)
  flags = _lib.CONV2D_ADJOINT | _lib.CONV2D_MASK_OUTPUT
  residual, = _dev(_f32(rng, 2, 5, 6, ch))
  dx = nn._run_conv2d(cot, kernel, None, (1, 2), flags, image=(5, 6), mask_src=x)
  assert torch.equal(nn._run_conv2d(cot, kernel, None, (1, 2), flags, image=(5, 6), mask_src=x, addend=residual), dx + residual)
  assert bool(dx.any())


def test_limits_raise_before_any_launch(ddsp):
  reached = []
  load = _lib.load

  class Counting:
    def __getattr__(self, name):
      reached.append(name)
      return getattr(load(), name)

  x, = _dev(np.zeros((1, 1, 1, 2), np.float32))
  z = torch.zeros
  try:
    _lib.load = Counting
    for bad_x, kernel, strides in [(z(1, 2, 2, 1040), z(1, 1, 1040, 16), 1), (z(1, 2, 2, 2), z(3, 3, 2, 1040), 1),
                                   (z(1, 2, 2, 2), z(9, 8, 2, 4), 1), (z(1, 2, 2, 2), z(3, 3, 2, 4), (1, 9)), (z(1, 2, 2, 2), z(3, 3, 2, 4), (9, 1)),
                                   (x.expand(1 << 16, 1 << 7, 1 << 7, 2), z(3, 3, 2, 4), 1), (x.expand(1 << 16, 32, 32, 2), z(3, 3, 2, 1024), 1),
                                   (x[..., :1].expand(1, (1 << 30) + 1, 1, 1), z(1, 1, 1, 1), 1)]:
      with pytest.raises(ValueError, match='MI355X path|2 \\*\\* 31'):
        nn.conv2d(bad_x, kernel, None, strides)
  finally:
    _lib.load = load
  assert not reached
  assert nn.conv2d(x[:0], z(3, 3, 2, 4, device=DEV)).shape == (0, 1, 1, 4)            # batch = 0 is a no-op


# ---- the layers ---------------------------------------------------------------------------------------------------------------
def _draw(module, rng):
  """Overwrites every weight of a BUILT module with drawn values and returns them by parameter name: convolution kernels at
  sqrt(2 / (kh kw ch_in)) (He: a ReLU layer keeps its scale), Dense kernels at 0.3 / sqrt(fan_in / 16), the norms' scales near 0.3 -
  a deep stack of residual layers stays of order 1 - and everything else at 0.1."""
  out = {}
  with torch.no_grad():
    for name, param in module.named_parameters():
      leaf = name.rsplit('.', 1)[-1]
      if leaf == 'kernel' and param.dim() == 4:
        value = _f32(rng, *param.shape, scale=_kernel_scale(*param.shape[:3]))
      elif leaf == 'kernel':
        value = _f32(rng, *param.shape, scale=0.3 / np.sqrt(max(param.shape[0] / 16.0, 1.0)))
      elif leaf == 'scale':
        value = _f32(rng, *param.shape, scale=0.03, shift=0.3)
      else:
        value = _f32(rng, *param.shape, scale=0.1)
      param.copy_(torch.as_tensor(value))
      out[name] = value
  return out


def _structural_zero_scale(which, want):
  """tests/test_gpu_dilated_conv.py's rule for the layers here: a convolution's bias whose every later use passes through a
  normalisation with single-channel groups ('instance'; 'group' at 32 channels) has a gradient of exactly 0, of whose fp64
  rounding (1e-15) no fp32 sum can be within 2e-4.  Such a gradient - the truth's largest element below 1e-12 of the same
  convolution's kernel gradient - is held to 2e-4 of THAT gradient's largest element.  -> that scale, or None for the usual rule."""
  kernel = which[:-len('bias')] + 'kernel'
  if not which.endswith('.bias') or kernel not in want or want[kernel].ndim != 4:
    return None
  kernel_scale = float(np.max(np.abs(want[kernel])))
  return kernel_scale if float(np.max(np.abs(want[which]))) < 1e-12 * kernel_scale else None


def _check_module(name, module, call, host, truth, rng, data=()):
  """module: built by call(module, *tensors) (-> a tensor or a list of them); host: the input arrays, all differentiated but those
  whose index `data` names; truth(w, *inputs, dtype=) -> the same outputs from the weights by parameter name."""
  feed = [_dev(v, grad=i not in data)[0] for i, v in enumerate(host)]
  call(module, *feed)                                   # builds
  w = _draw(module, rng)
  names = list(w)
  outs = call(module, *feed)
  outs = list(outs) if isinstance(outs, (list, tuple)) else [outs]

  def fn(*args, dtype=torch.float64):
    out = truth(dict(zip(names, args[len(host):])), *args[:len(host)], dtype=dtype)
    return list(out) if isinstance(out, (list, tuple)) else [out]

  args = list(host) + [w[n] for n in names]
  truths, fp32 = fn(*args), fn(*args, dtype=torch.float32)
  assert len(outs) == len(truths)
  for i, (got, a, b) in enumerate(zip(outs, truths, fp32)):
    _check_tensor('%s/y%d' % (name, i), got, a.numpy(), b.numpy())
  cots = [_f32(rng, *t.shape) for t in truths]
  params = dict(module.named_parameters())
  labels = ['in%d' % i for i in range(len(host))] + names
  want = dict(zip(labels, T.grads(fn, args, cots)))
  live = [(label, leaf) for label, leaf in zip(labels, feed + [params[n] for n in names]) if leaf.requires_grad]
  grads = torch.autograd.grad(outs, [leaf for _, leaf in live], _dev(*cots), allow_unused=True)
  for (which, _), got in zip(live, grads):
    assert got is not None or not np.any(want[which]), which
    if got is not None:
      _check_grad('%s/grad_%s' % (name, which), got, want[which], scale=_structural_zero_scale(which, want))
  return module


@pytest.mark.parametrize('shortcut', [True, False], ids=['shortcut', 'identity'])
def test_residual_layer(ddsp, shortcut):
  rng = _rng('layer/%s' % shortcut)
  stride = 2 if shortcut else 1
  layer = nn.ResidualLayer(4, stride, shortcut, 'layer', False, False)
  _check_module('residual_layer/' + ('shortcut' if shortcut else 'identity'), layer, lambda m, x: m(x), [_f32(rng, 2, 5, 7, 16)],
                lambda w, x, dtype: T.residual_layer(w, '', x, None, stride, 'layer', dtype=dtype), rng)
  assert hasattr(layer, 'conv_proj') == shortcut and [n for n, _ in layer.named_children()][:1] == ['norm_input']


@pytest.mark.parametrize('mode', ['unconditional', 'film', 'shift_only'])
@pytest.mark.parametrize('norm_type', ['layer', 'instance', 'group'])
def test_residual_stack(ddsp, norm_type, mode):
  rng = _rng('stack/%s/%s' % (norm_type, mode))
  filters, ch_in = ([32, 64], 32) if norm_type == 'group' else ([16, 32], 8)      # 'group' takes widths in multiples of 32
  conditional, shift_only = mode != 'unconditional', mode == 'shift_only'
  stack = nn.ResidualStack(filters, [2, 1], [1, 2], norm_type, conditional, shift_only)
  host = [_f32(rng, 2, 6, 10, ch_in)] + ([_f32(rng, 2, 6, 1, 5)] if conditional else [])
  call = (lambda m, x, z: m([x, z])) if conditional else (lambda m, x: m(x))
  truth = lambda w, x, z=None, dtype=torch.float64: T.residual_stack(w, '', x, z, [2, 1], [1, 2], norm_type, conditional, shift_only, dtype)
  _check_module('residual_stack/%s/%s' % (norm_type, mode), stack, call, host, truth, rng)
  assert len(stack.layers) == 4 and [hasattr(l, 'conv_proj') for l in stack.layers[:3]] == [True, False, True]


@pytest.mark.parametrize('width', [9, 10])
def test_max_pool_2d(ddsp, width):
  rng = _rng('pool/%d' % width)
  x_host, cot = _f32(rng, 2, 3, width, 4), _f32(rng, 2, 3, -(-width // 2), 4)
  x, = _dev(x_host, grad=True)
  y = nn.MaxPool2D(pool_size=(1, 3), strides=(1, 2), padding='same')(x)
  fn = lambda a, dtype=torch.float64: T.max_pool(a, (1, 3), (1, 2), dtype)
  _check_tensor('max_pool/w%d/y' % width, y, fn(x_host).numpy(), fn(x_host, dtype=torch.float32).numpy())
  assert np.array_equal(_np(y), fn(x_host).numpy())                                  # a selection: exact
  _check_grad('max_pool/w%d/grad_x' % width, torch.autograd.grad(y, [x], _dev(cot)[0])[0], T.grads(fn, [x_host], [cot])[0])


def test_resnet_small(ddsp):
  rng = _rng('resnet/small')
  net = _check_module('resnet/small', nn.ResNet('small'), lambda m, x: m(x), [_f32(rng, 1, 3, 9, 1)],
                      lambda w, x, dtype: T.resnet(w, '', x, 'small', dtype=dtype), rng)
  assert net(_dev(_f32(rng, 1, 3, 9, 1))[0]).shape == (1, 3, 1, 1024)
  with pytest.raises(KeyError):
    nn.ResNet('tiny')


def test_resnet_sinusoidal_encoder(ddsp):
  rng = _rng('encoder/resnet')
  splits = (('frequencies', 6), ('amplitudes', 3), ('noise_magnitudes', 5))
  logmel = lambda audio: spectral_ops.compute_logmel(audio, bins=16, fft_size=256)
  with pytest.raises(KeyError):
    encoders.ResnetSinusoidalEncoder(splits, logmel)                                 # the default size='tiny', as in the reference
  enc = encoders.ResnetSinusoidalEncoder(splits, logmel, size='small')
  audio, = _dev(_f32(rng, 2, 2048, scale=0.3))
  mag = logmel(audio).detach().cpu().numpy()

  def call(m, mag_dev):
    m.spectral_fn = lambda a: mag_dev                   # the truth starts behind the spectral kernel (tests/test_gpu_features.py)
    out = m(audio)
    assert list(out) == [k for k, _ in splits]
    return [out[k] for k, _ in splits]

  _check_module('encoder/resnet', enc, call, [mag], lambda w, m, dtype: T.resnet_sinusoidal_encoder(w, m, 'small', len(splits), dtype), rng)
  enc.spectral_fn = logmel
  out = enc(audio)
  assert [tuple(out[k].shape) for k, _ in splits] == [(2, mag.shape[1], n) for _, n in splits]
  assert torch.equal(out['amplitudes'], call(enc, torch.as_tensor(mag, device=DEV))[1])


def test_sinusoidal_to_harmonic_encoder(ddsp):
  rng = _rng('encoder/s2h')
  enc = encoders.SinusoidalToHarmonicEncoder(net=nn.RnnSandwich(fc_stack_ch=16, fc_stack_layers=2, rnn_ch=16), n_harmonics=10, sample_rate=2000)
  freqs = (60.0 + 800.0 * rng.random((2, 5, 4))).astype(np.float32)
  amps = (0.1 + rng.random((2, 5, 4))).astype(np.float32)

  def call(m, f, a):
    out = m(sin_freqs=f, sin_amps=a)
    assert list(out) == ['harm_amp', 'harm_dist', 'f0_hz']
    return [out[k] for k in out]

  _check_module('encoder/s2h', enc, call, [freqs, amps],
                lambda w, f, a, dtype: T.sinusoidal_to_harmonic_encoder(w, f, a, 10, sample_rate=2000, dtype=dtype), rng,
                data=(0,))                              # core.hz_to_unit carries no backward: the frequencies are data, as in the model
  out = enc(sin_freqs=_dev(freqs)[0], sin_amps=_dev(amps)[0])
  assert out['harm_amp'].shape == (2, 5, 1) and out['harm_dist'].shape == (2, 5, 10) and out['f0_hz'].shape == (2, 5, 1)
  dist = _np(out['harm_dist'])
  assert (dist == 0.0).any() and np.allclose(dist.sum(-1), 1.0, atol=1e-5)            # harmonics above Nyquist are gone


# ---- bit-stability of the hand-written kernel ------------------------------------------------------------------------------
def _conv_everything(x, kernel, bias, cot, strides):
  leaves = _dev(x, kernel, bias, grad=True)
  y = nn.conv2d(*leaves, strides=strides, relu_input=True)
  dx, = torch.autograd.grad(y, leaves[:1], _dev(cot)[0])
  return [y.detach(), dx]


@pytest.mark.parametrize('case', [(3, 5, 6, 2, 4, 3, 3, 1, 1), (3, 70, 5, 32, 32, 3, 3, 1, 2)], ids=_case_name)
def test_conv2d_same_bits_twice_row_alone_and_sub_batch(ddsp, case):
  c = _conv_case(*case, True, loud_row=1)                                            # the rows differ in scale by 1e4
  (x, kernel, bias), cot, strides = c['ins'], c['cot'], case[7:]
  first, second = _conv_everything(x, kernel, bias, cot, strides), _conv_everything(x, kernel, bias, cot, strides)
  for a, b in zip(first, second):
    assert torch.equal(a, b)
  for rows in (slice(0, 1), slice(2, 3), slice(1, 3)):                              # a row alone, the last alone, a sub-batch
    for a, r in zip(first, _conv_everything(x[rows], kernel, bias, cot[rows], strides)):
      assert torch.equal(a[rows], r)


def test_conv2d_replays_from_a_captured_graph(ddsp):
  """No host synchronisation, no allocation by the library, every launch on the current stream in one chain: forward and
  backward are captured once with torch.cuda.graph and replayed - the same bits as the eager call."""
  if DEV != 'cuda' or not torch.cuda.is_available():
    pytest.skip('needs real streams and graphs: left to the GPU run')
  rng = _rng('graph/conv2d')
  host = [_f32(rng, 2, 5, 6, 16), _f32(rng, 3, 3, 16, 32, scale=_kernel_scale(3, 3, 16)), _f32(rng, 32, scale=0.1)]
  other = _f32(rng, 2, 5, 6, 16, scale=3.0)
  static = _dev(*host, grad=True)
  cot, = _dev(_f32(rng, 2, 5, 3, 32))

  def step(leaves):
    y = nn.conv2d(*leaves, strides=(1, 2), relu_input=True)
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
