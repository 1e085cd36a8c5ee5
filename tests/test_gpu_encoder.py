"""ddsp_amd.training.nn's normalisations (csrc/group_norm.hip), core.resample's gradient and training.encoders on the MI355X
against tests/encoder_truth.py (the reference's arithmetic in fp64 at the fp32 inputs).  tests/test_encoder_emulated.py runs this
module through the SIMT emulation on the CPU.

Tolerances (as tests/test_gpu_decoder.py applies them): an output's error against the fp64 truth may be up
to 4 x that of the truth's fp32 mode on the same case, with a floor of eight fp32 ulp of the tensor's largest magnitude; each
gradient 2e-4 of its largest element.  Every comparison is appended to the file DDSP_PARITY_LOG names, when it is set.

Norm cases (N, S, C, type), the smallest at which each part can go wrong: a one-element group (y = shift); a few rows of three
channels; the encoder's own shape (C = 30 divides nothing); C one past a wavefront; one row; group edges inside a wavefront; a
layer norm whose batch row is exactly one block's chunk (64 x 256 = 16384 floats), one split over three blocks with a short
last chunk (a wavefront merges the 768 chunk-channels) and one over five (1280: a block merges them); an instance norm and a
group norm split over two blocks; C > 256 (channel tiles) in one block and split.
x = 100 + N(0, 1) is where a one-pass E[x^2] - mean^2 fails the 4 x rule (tests/test_encoder_host.py shows it on the CPU).

The encoders are checked DOWNSTREAM of their MFCCs: the truth is applied to the MFCCs the product itself returned (MFCC parity is
tests/test_gpu_features.py's business, and normalisation would amplify its error by an amount nobody has derived).

Measured on the MI355X: see profiles/encoder_parity_errors.jsonl and DESIGN.md section 8."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import encoder_truth as T
from ddsp_amd.training import encoders, nn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRAD_RTOL = 2e-4
TENSOR_RATIO = 4.0
TENSOR_FLOOR = 8 * 2.0 ** -24          # eight fp32 ulp of the tensor's largest magnitude

NORM_CASES = [(1, 1, 1, 'instance'), (2, 5, 3, 'instance'), (2, 250, 30, 'instance'), (3, 67, 65, 'instance'), (2, 1, 64, 'layer'),
              (2, 33, 96, 'group'), (2, 64, 256, 'layer'), (2, 130, 256, 'layer'), (2, 260, 256, 'layer'), (2, 700, 30, 'instance'),
              (2, 200, 96, 'group'), (2, 9, 300, 'instance'), (2, 70, 300, 'layer')]
RESAMPLE_SHAPES = [(9, 640, 3), (12, 96, 5), (30, 7, 2)]
METHODS = ['nearest', 'linear', 'cubic', 'window']


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


def _check_grad(case, got, truth):
  """2e-4 of the gradient's largest element."""
  g = _np(got)
  scale = max(float(np.max(np.abs(truth))), 1e-30)
  err = float(np.max(np.abs(g - truth))) / scale
  _log(case, grad_err=err, scale=scale)
  assert g.shape == truth.shape and np.isfinite(g).all()
  assert err <= GRAD_RTOL, (case, err)


def _rng(name):
  return np.random.default_rng(zlib.crc32(('encoder/' + name).encode()))


def _f32(rng, *shape, scale=1.0, shift=0.0):
  return (shift + scale * rng.standard_normal(shape)).astype(np.float32)


# ---- normalize_op / Normalize ---------------------------------------------------------------------------------------------
def _hw(s):
  return (s // 3, 3) if s % 3 == 0 and s > 3 else (s, 1)


@functools.lru_cache(maxsize=None)
def _norm_case(n, s, c, norm_type, affine, kind='normal'):
  """kind: 'normal'; 'offset' (x = 100 + N(0, 1)); 'constant' (one group of batch row 1 holds one value)."""
  rng = _rng('norm/%d/%d/%d/%s/%d/%s' % (n, s, c, norm_type, affine, kind))
  h, w = _hw(s)
  x = _f32(rng, n, h, w, c, shift=100.0 if kind == 'offset' else 0.0)
  if kind == 'constant':
    x[1, :, :, :(1 if norm_type == 'instance' else c)] = np.float32(0.7)
  ins = (x,) + ((_f32(rng, 1, 1, 1, c, scale=0.3, shift=1.0), _f32(rng, 1, 1, 1, c, scale=0.3)) if affine else ())
  cot = _f32(rng, n, h, w, c)
  if affine:
    fn = lambda x_, sc, sh, dtype=torch.float64: T.normalize(x_, sc, sh, norm_type, dtype)
  else:
    fn = lambda x_, dtype=torch.float64: T.normalize_op(x_, norm_type, dtype=dtype)
  return dict(ins=ins, cot=cot, norm_type=norm_type, truth=fn(*ins).numpy(), fp32=fn(*ins, dtype=torch.float32).numpy(),
              grads=T.grads(fn, ins, [cot]))


def _run_norm(c):
  """-> y, the gradients of (x[, scale, shift]); checks that the forward-only route gives the bits of the autograd route."""
  x, = _dev(c['ins'][0], grad=True)
  if len(c['ins']) > 1:
    layer = nn.Normalize(c['norm_type'])
    layer.build(x.shape[-1])
    assert layer.scale.shape == (1, 1, 1, x.shape[-1]) and layer.shift.shape == (1, 1, 1, x.shape[-1])
    with torch.no_grad():
      layer.scale.copy_(torch.as_tensor(c['ins'][1]))
      layer.shift.copy_(torch.as_tensor(c['ins'][2]))
    call, leaves = layer, [x, layer.scale, layer.shift]
  else:
    call, leaves = (lambda v: nn.normalize_op(v, c['norm_type'])), [x]
  with torch.no_grad():
    plain = call(x)
  y = call(x)
  assert y.requires_grad and not plain.requires_grad and torch.equal(y.detach(), plain)
  return y, torch.autograd.grad(y, leaves, _dev(c['cot'])[0])


def _check_norm(name, c):
  y, grads = _run_norm(c)
  _check_tensor(name + '/y', y, c['truth'], c['fp32'])
  for which, got, want in zip(('x', 'scale', 'shift'), grads, c['grads']):
    _check_grad('%s/grad_%s' % (name, which), got, want)
  return y, grads


@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'scale_shift'])
@pytest.mark.parametrize('n, s, c, norm_type', NORM_CASES)
def test_normalize(ddsp, n, s, c, norm_type, affine):
  case = _norm_case(n, s, c, norm_type, affine)
  y, _ = _check_norm('norm/%dx%dx%d/%s/%s' % (n, s, c, norm_type, 'affine' if affine else 'plain'), case)
  if (n, s, c) == (1, 1, 1):                             # a one-element group: xhat = 0 exactly
    assert torch.equal(y.detach().cpu().reshape(-1), torch.as_tensor(case['ins'][2]).reshape(-1) if affine else torch.zeros(1))


@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'scale_shift'])
def test_normalize_at_a_large_mean(ddsp, affine):
  """x = 100 + N(0, 1): E[x^2] - mean^2 in fp32 loses the variance's digits here; two passes do not."""
  _check_norm('norm/offset100/' + ('affine' if affine else 'plain'), _norm_case(2, 40, 8, 'instance', affine, 'offset'))


@pytest.mark.parametrize('n, s, c, norm_type', [(2, 40, 8, 'instance'), (2, 5, 64, 'layer'), (2, 130, 256, 'layer')])
@pytest.mark.parametrize('affine', [False, True], ids=['plain', 'scale_shift'])
def test_normalize_with_a_constant_group(ddsp, n, s, c, norm_type, affine):
  """A group whose variance is exactly 0: xhat = 0 (y = shift), and everything finite."""
  case = _norm_case(n, s, c, norm_type, affine, 'constant')
  y, grads = _check_norm('norm/constant/%dx%dx%d/%s/%s' % (n, s, c, norm_type, 'affine' if affine else 'plain'), case)
  width = 1 if norm_type == 'instance' else c
  got = y.detach().cpu()[1, :, :, :width]
  want = torch.as_tensor(case['ins'][2])[0, :, :, :width].expand_as(got) if affine else torch.zeros_like(got)
  assert torch.equal(got, want)
  assert all(bool(torch.isfinite(g).all()) for g in grads)


@pytest.mark.parametrize('n, s, c, norm_type', [(3, 67, 65, 'instance'), (3, 33, 96, 'group'), (3, 130, 256, 'layer'), (3, 260, 256, 'layer')])
def test_normalize_same_bits_twice_row_alone_and_in_the_batch(ddsp, n, s, c, norm_type):
  case = _norm_case(n, s, c, norm_type, True)
  (y1, g1), (y2, g2) = _run_norm(case), _run_norm(case)
  assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
  alone = dict(case, ins=(case['ins'][0][1:2],) + case['ins'][1:], cot=case['cot'][1:2])
  y, g = _run_norm(alone)
  assert torch.equal(y, y1[1:2]) and torch.equal(g[0], g1[0][1:2])         # dscale / dshift are sums over the batch


def test_normalize_op_arguments(ddsp):
  x, = _dev(_f32(_rng('args'), 2, 3, 1, 4))
  assert nn.normalize_op(x, None) is x
  with pytest.raises(KeyError):
    nn.normalize_op(x, 'batch')
  with pytest.raises(ValueError, match='multiples of 32'):
    nn.normalize_op(x, 'group')
  with pytest.raises(ValueError, match=r'\[batch, height, width, channels\]'):
    nn.normalize_op(x[0], 'layer')
  assert nn.normalize_op(x[:0], 'layer').shape == (0, 3, 1, 4)
  assert isinstance(nn.get_norm('layer', False, False), nn.Normalize) and isinstance(nn.get_norm('layer', True, True), nn.ConditionalNorm)
  assert nn.Identity()(x) is x
  three = nn.Normalize('instance')(x[:, :, 0, :])                          # ensure_4d / inv_ensure_4d around the one call
  assert three.shape == (2, 3, 4) and torch.equal(three, nn.Normalize('instance')(x)[:, :, 0, :])


def test_normalize_replays_from_a_captured_graph(ddsp):
  """No host synchronisation, no allocation by the library, every launch on the current stream in one chain: forward and
  backward, one-block and split, are captured once with torch.cuda.graph and replayed - the same bits as the eager call."""
  if DEV != 'cuda' or not torch.cuda.is_available():
    pytest.skip('needs real streams and graphs: left to the GPU run')
  rng = _rng('graph/norm')
  shapes = [(2, 33, 1, 96), (2, 130, 1, 256)]
  host = [_f32(rng, *s) for s in shapes]
  other = [_f32(rng, *s) for s in shapes]
  static = _dev(*host, grad=True)
  layers = [nn.Normalize('group'), nn.Normalize('layer')]
  for layer, s in zip(layers, shapes):
    layer.build(s[-1])
  cots = _dev(*[_f32(rng, *s) for s in shapes])

  def step(xs):
    out = []
    for layer, x, cot in zip(layers, xs, cots):
      y = layer(x)
      out += [y] + list(torch.autograd.grad(y, [x, layer.scale, layer.shift], cot))
    return out

  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    step(static)
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    captured = step(static)
  for new in (host, other, other):
    with torch.no_grad():
      for s, v in zip(static, new):
        s.copy_(torch.as_tensor(v))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, step(_dev(*new, grad=True))):
      assert torch.equal(a.detach(), b.detach())


def test_conditional_norm(ddsp):
  rng = _rng('conditional_norm')
  for shift_only in (False, True):
    x_host, z_host, cot = _f32(rng, 2, 5, 3, 8), _f32(rng, 2, 1, 1, 4), _f32(rng, 2, 5, 3, 8)
    kernel, bias = _f32(rng, 4, 8 if shift_only else 16, scale=0.3), _f32(rng, 8 if shift_only else 16, scale=0.3)
    layer = nn.ConditionalNorm('instance', shift_only=shift_only)
    x, z = _dev(x_host, z_host, grad=True)
    layer([x, z])                                        # builds
    dense = layer.conditional_scale_and_shift.dense
    with torch.no_grad():
      dense.kernel.copy_(torch.as_tensor(kernel))
      dense.bias.copy_(torch.as_tensor(bias))
    y = layer([x, z])
    fn = lambda *a, dtype=torch.float64: T.conditional_norm(*a, 'instance', shift_only, dtype)
    ins = (x_host, z_host, kernel, bias)
    name = 'conditional_norm/' + ('shift_only' if shift_only else 'scale_shift')
    _check_tensor(name + '/y', y, fn(*ins).numpy(), fn(*ins, dtype=torch.float32).numpy())
    grads = torch.autograd.grad(y, [x, z, dense.kernel, dense.bias], _dev(cot)[0])
    for which, got, want in zip(('x', 'z', 'kernel', 'bias'), grads, T.grads(fn, ins, [cot])):
      _check_grad('%s/grad_%s' % (name, which), got, want)


# ---- core.resample with a gradient ----------------------------------------------------------------------------------------
def _resample_cases():
  out = []
  for f, n, c in RESAMPLE_SHAPES:
    for method in METHODS:
      for add_endpoint in (True, False):
        if method == 'window':                           # upsampling only, n_samples a multiple of the number of intervals
          if n < f:
            continue
          n_ = (f if add_endpoint else f - 1) * max(2, n // f)
        else:
          n_ = n
        out.append(pytest.param(f, n_, c, method, add_endpoint, id='%dto%dx%d-%s-%s' % (f, n_, c, method, 'endpoint' if add_endpoint else 'corners')))
  return out


def _own_matrix(ddsp, f, n, method, add_endpoint):
  """The forward call applied to the identity: [n, f]."""
  eye = np.zeros((f, f, 1), np.float32)
  eye[np.arange(f), np.arange(f), 0] = 1.0
  return _np(ddsp.core.resample(eye, n, method=method, add_endpoint=add_endpoint))[:, :, 0].T


@pytest.mark.parametrize('f, n, c, method, add_endpoint', _resample_cases())
def test_resample_gradient_is_the_transpose_of_its_own_matrix(ddsp, f, n, c, method, add_endpoint):
  rng = _rng('resample/%d/%d/%d/%s/%d' % (f, n, c, method, add_endpoint))
  x_host, cot = _f32(rng, 2, f, c), _f32(rng, 2, n, c)
  x, = _dev(x_host, grad=True)
  y = ddsp.core.resample(x, n, method=method, add_endpoint=add_endpoint)
  assert y.requires_grad and y.shape == (2, n, c)
  plain = ddsp.core.resample(x.detach(), n, method=method, add_endpoint=add_endpoint)
  assert not plain.requires_grad and torch.equal(y.detach(), plain)        # the same forward, to the bit
  with torch.no_grad():
    assert torch.equal(ddsp.core.resample(x, n, method=method, add_endpoint=add_endpoint), plain)
  grad, = torch.autograd.grad(y, [x], _dev(cot)[0])
  ref = np.einsum('nf,bnc->bfc', _own_matrix(ddsp, f, n, method, add_endpoint), cot.astype(np.float64))
  err = float(np.max(np.abs(_np(grad) - ref)))
  _log('resample_grad/%dto%dx%d/%s/%d' % (f, n, c, method, add_endpoint), err=err, bound=1e-6 + 2e-6 * np.abs(ref).max())
  assert err <= 1e-6 + 2e-6 * np.abs(ref).max()
  again, = torch.autograd.grad(ddsp.core.resample(x, n, method=method, add_endpoint=add_endpoint), [x], _dev(cot)[0])
  assert torch.equal(grad, again)


def test_resample_gradient_of_1d_4d_and_windows(ddsp):
  rng = _rng('resample/dims')
  f, n = 9, 36
  matrix = _own_matrix(ddsp, f, n, 'linear', True)
  for shape, spec in (((f,), 'nf,n->f'), ((2, f), 'nf,bn->bf'), ((2, f, 3, 2), 'nf,bnqc->bfqc')):
    x, = _dev(_f32(rng, *shape), grad=True)
    y = ddsp.core.resample(x, n)
    cot = _f32(rng, *y.shape)
    grad, = torch.autograd.grad(y, [x], _dev(cot)[0])
    ref = np.einsum(spec, matrix, cot.astype(np.float64))
    assert grad.shape == x.shape and float(np.max(np.abs(_np(grad) - ref))) <= 1e-6 + 2e-6 * np.abs(ref).max()
    assert torch.equal(y.detach(), ddsp.core.resample(x.detach(), n))
  x, = _dev(_f32(rng, 2, f, 3), grad=True)
  y = ddsp.core.upsample_with_windows(x, n)
  cot = _f32(rng, 2, n, 3)
  grad, = torch.autograd.grad(y, [x], _dev(cot)[0])
  ref = np.einsum('nf,bnc->bfc', _own_matrix(ddsp, f, n, 'window', True), cot.astype(np.float64))
  assert float(np.max(np.abs(_np(grad) - ref))) <= 1e-6 + 2e-6 * np.abs(ref).max()


# ---- the encoders ---------------------------------------------------------------------------------------------------------
def _draw(module, rng):
  """Overwrites every weight of a BUILT module with drawn values (kernels at 0.3 / sqrt(fan_in / 16), scale near 1, the rest at
  0.1) and returns them by parameter name."""
  out = {}
  with torch.no_grad():
    for name, param in module.named_parameters():
      leaf = name.rsplit('.', 1)[-1]
      if leaf in ('kernel', 'recurrent_kernel'):
        value = _f32(rng, *param.shape, scale=0.3 / np.sqrt(max(param.shape[0] / 16.0, 1.0)))
      elif leaf == 'scale':
        value = _f32(rng, *param.shape, scale=0.1, shift=1.0)
      else:
        value = _f32(rng, *param.shape, scale=0.1)
      param.copy_(torch.as_tensor(value))
      out[name] = value
  return out


def _audio(rng, batch, n_samples):
  t = np.arange(n_samples) / 16000.0
  tones = np.stack([np.sin(2 * np.pi * (220.0 * (b + 1)) * t * (1.0 + 0.3 * t * 16000.0 / n_samples)) for b in range(batch)])
  return (0.5 * tones + 0.1 * rng.standard_normal((batch, n_samples))).astype(np.float32)


MFCC_RNN_NAMES = ['z_norm.scale', 'z_norm.shift', 'rnn.rnn.kernel', 'rnn.rnn.recurrent_kernel', 'rnn.rnn.bias', 'dense_out.kernel',
                  'dense_out.bias']


def _check_mfcc_rnn_encoder(name, rnn_channels, time_steps):
  rng = _rng(name)
  audio, = _dev(_audio(rng, 2, 2048))
  f0_scaled, = _dev(_f32(rng, 2, time_steps, 1))
  enc = encoders.MfccTimeDistributedRnnEncoder(rnn_channels=rnn_channels, z_dims=4, z_time_steps=1000)
  assert enc.input_keys == ['audio', 'f0_scaled'] and enc.output_keys == ['z'] and (enc.fft_size, enc.overlap) == (256, 0.75)
  feed = dict(audio=audio, f0_scaled=f0_scaled)
  assert list(enc(feed)) == ['z']                        # builds
  w = _draw(enc, rng)
  assert list(w) == MFCC_RNN_NAMES and w['z_norm.scale'].shape == (1, 1, 1, 30) and w['dense_out.kernel'].shape == (rnn_channels, 4)
  mfccs = enc.compute_mfccs(audio)
  assert mfccs.shape == (2, 32, 30) and not mfccs.requires_grad
  z = enc(feed)['z']
  assert z.shape == (2, time_steps, 4) and z.requires_grad
  fn = lambda *a, dtype=torch.float64: T.mfcc_rnn_encoder(_np(mfccs), *a, time_steps, dtype)
  flat = [w[n] for n in MFCC_RNN_NAMES]
  _check_tensor(name + '/z', z, fn(*flat).numpy(), fn(*flat, dtype=torch.float32).numpy())
  cot = _f32(rng, 2, time_steps, 4)
  grads = torch.autograd.grad(z, [p for _, p in enc.named_parameters()], _dev(cot)[0])
  for which, got, want in zip(MFCC_RNN_NAMES, grads, T.grads(fn, flat, [cot])):
    _check_grad('%s/grad_%s' % (name, which), got, want)


@pytest.mark.parametrize('time_steps', [32, 40], ids=['same_frames', 'resampled'])
def test_mfcc_time_distributed_rnn_encoder(ddsp, time_steps):
  _check_mfcc_rnn_encoder('mfcc_rnn_encoder/t%d' % time_steps, 16, time_steps)


def test_mfcc_time_distributed_rnn_encoder_on_the_plain_gru_kernel(ddsp):
  _check_mfcc_rnn_encoder('mfcc_rnn_encoder/h3', 3, 40)


def test_mfcc_encoder(ddsp):
  rng = _rng('mfcc_encoder')
  audio, f0_scaled = _dev(_audio(rng, 2, 1024), _f32(rng, 2, 12, 1))
  enc = encoders.MfccEncoder(fft_sizes=(256, 128), mel_bins=(32, 16), mfcc_bins=(8, 5), time_steps=10)
  feed = dict(audio=audio, f0_scaled=f0_scaled)
  enc(feed)
  w = _draw(enc, rng)
  assert list(w) == ['norm_out.scale', 'norm_out.shift']
  mfccs = enc.compute_mfccs(audio)
  assert mfccs.shape == (2, 10, 13)
  z = enc(feed)['z']
  assert z.shape == (2, 12, 13)
  fn = lambda *a, dtype=torch.float64: T.mfcc_encoder(_np(mfccs), *a, 12, dtype)
  flat = [w['norm_out.scale'], w['norm_out.shift']]
  _check_tensor('mfcc_encoder/z', z, fn(*flat).numpy(), fn(*flat, dtype=torch.float32).numpy())
  cot = _f32(rng, 2, 12, 13)
  for which, got, want in zip(('scale', 'shift'), torch.autograd.grad(z, [enc.norm_out.scale, enc.norm_out.shift], _dev(cot)[0]),
                              T.grads(fn, flat, [cot])):
    _check_grad('mfcc_encoder/grad_' + which, got, want)


def test_aggregate_features_encoder(ddsp):
  rng = _rng('aggregate')
  f0_host, ld_host = _f32(rng, 2, 6, 1), _f32(rng, 2, 6, 1)
  enc = encoders.AggregateFeaturesEncoder(ch=8)
  assert enc.input_keys == ['f0_scaled', 'ld_scaled', 'f0_scaled']
  f0, ld = _dev(f0_host, ld_host, grad=True)
  enc(dict(f0_scaled=f0, ld_scaled=ld))
  w = _draw(enc, rng)
  z = enc(dict(f0_scaled=f0, ld_scaled=ld))['z']
  assert z.shape == (2, 6, 8)                           # one frame, expanded to the conditioning's six
  fn = lambda *a, dtype=torch.float64: T.aggregate_features_encoder(*a, 6, dtype)
  ins = (f0_host, ld_host, w['fc.kernel'], w['fc.bias'])
  _check_tensor('aggregate/z', z, fn(*ins).numpy(), fn(*ins, dtype=torch.float32).numpy())
  cot = _f32(rng, 2, 6, 8)
  for which, got, want in zip(('f0', 'ld', 'kernel', 'bias'), torch.autograd.grad(z, [f0, ld, enc.fc.kernel, enc.fc.bias], _dev(cot)[0]),
                              T.grads(fn, ins, [cot])):
    _check_grad('aggregate/grad_' + which, got, want)


@pytest.mark.parametrize('skip_expand', [True, False])
def test_one_hot_encoder(ddsp, skip_expand):
  rng = _rng('one_hot')
  enc = encoders.OneHotEncoder(vocab_size=16, n_dims=4, skip_expand=skip_expand)
  assert enc.input_keys == ['instrument', 'f0_scaled']
  ids = torch.as_tensor([[3], [11]], device=DEV)
  f0_scaled, = _dev(_f32(rng, 2, 5, 1))
  z = enc(dict(instrument=ids, f0_scaled=f0_scaled))['z']
  table = enc.embedding.embeddings
  assert table.shape == (16, 4) and float(table.detach().abs().max()) <= 0.05
  assert z.shape == ((2, 1, 4) if skip_expand else (2, 5, 4))
  want = table.detach()[ids[:, 0]][:, None, :].expand_as(z)
  assert torch.equal(z.detach(), want) if skip_expand else torch.allclose(z.detach(), want, rtol=0, atol=1e-8)
  grad, = torch.autograd.grad(z.sum(), [table])
  rows = torch.zeros(16, device=DEV)
  rows[ids[:, 0]] = float(z.shape[1])
  assert torch.allclose(grad, rows[:, None].expand(16, 4), rtol=0, atol=1e-5)


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  return ddsp_amd
