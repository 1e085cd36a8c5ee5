"""ddsp_amd.training.nn's layers and training.decoders.RnnFcDecoder on the MI355X against tests/decoder_truth.py (the
reference's arithmetic in fp64 at the fp32 inputs).  tests/test_decoder_emulated.py runs this module through the SIMT
emulation on the CPU.

Tolerances (as tests/test_gpu_notes.py and tests/test_gpu_hmm.py apply them): an output's error against
the fp64 truth may be up to 4 x that of the truth's fp32 mode on the same case, with a floor of eight fp32 ulp of the tensor's
largest magnitude; each gradient 2e-4 of its largest element.  Every comparison is appended to the file DDSP_PARITY_LOG names,
when it is set.

GRU cases (batch, time, in, H), the smallest at which each part can go wrong: the smallest legal; the reference's test width
(plain kernel); one MFMA tile with K shorter than a 32-deep step; a K tail and an odd batch; one past a 16-row tile; the shipped
widths; the full-length recurrence (1000 launches each way).  bias + LayerNorm + activation cases (rows, ch): one channel, two,
one wavefront, one past it, the register limit, a looping row, more rows than one block's wavefronts.  Weights are drawn at
scale 0.25 - 0.3: the recurrence is neither dead nor chaotic.

Bit-stability is claimed for the hand-written kernels only (the GRU on a given input projection, the norm kernel): the
framework's matrix products may pick their kernels by the row count.

Measured on the MI355X: see profiles/decoder_parity_errors.jsonl and DESIGN.md section 8."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import decoder_truth as T
from ddsp_amd.training import decoders, nn, preprocessing

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRAD_RTOL = 2e-4
TENSOR_RATIO = 4.0
TENSOR_FLOOR = 8 * 2.0 ** -24          # eight fp32 ulp of the tensor's largest magnitude

GRU_CASES = [(1, 1, 1, 1), (2, 4, 4, 3), (2, 7, 5, 16), (3, 5, 8, 48), (17, 3, 4, 32), (2, 6, 1024, 512), (2, 1000, 4, 16)]
NORM_CASES = [(1, 1), (3, 2), (5, 64), (5, 65), (4, 512), (2, 1000), (257, 8)]
ACTIVATIONS = ['leaky_relu', 'relu', 'sigmoid', 'tanh', 'linear']


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
  return np.random.default_rng(zlib.crc32(('decoder/' + name).encode()))


def _f32(rng, *shape, scale=1.0, shift=0.0):
  return (shift + scale * rng.standard_normal(shape)).astype(np.float32)


# ---- bias + LayerNorm + activation ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _norm_case(rows, ch, act, constant_row=False):
  rng = _rng('norm/%d/%d/%s/%d' % (rows, ch, act, constant_row))
  x = _f32(rng, rows, ch)
  if constant_row:
    x[1, :] = np.float32(0.7)
  ins = (x, np.zeros(ch, np.float32) if constant_row else _f32(rng, ch, scale=0.3), _f32(rng, ch, scale=0.3, shift=1.0), _f32(rng, ch, scale=0.3))
  cot = _f32(rng, rows, ch)
  fn = lambda *a, **k: T.bias_norm_act(*a, act, **k)
  return dict(ins=ins, cot=cot, truth=fn(*ins).numpy(), fp32=fn(*ins, dtype=torch.float32).numpy(), grads=T.grads(fn, ins, [cot]))


def _run_norm(c, act):
  ins = _dev(*c['ins'], grad=True)
  with torch.no_grad():
    plain = nn.bias_norm_act(*ins, act)                 # the forward-only route
  y = nn.bias_norm_act(*ins, act)
  assert y.requires_grad and not plain.requires_grad and torch.equal(y.detach(), plain)
  return y, torch.autograd.grad(y, ins, _dev(c['cot'])[0])


@pytest.mark.parametrize('act', ACTIVATIONS)
@pytest.mark.parametrize('rows, ch', NORM_CASES)
def test_bias_norm_act(ddsp, rows, ch, act):
  c = _norm_case(rows, ch, act)
  name = 'norm/%dx%d/%s' % (rows, ch, act)
  y, grads = _run_norm(c, act)
  _check_tensor(name + '/y', y, c['truth'], c['fp32'])
  for which, got, want in zip(('x', 'bias', 'gamma', 'beta'), grads, c['grads']):
    _check_grad('%s/grad_%s' % (name, which), got, want)


def test_bias_norm_act_on_a_constant_row(ddsp):
  """A row whose variance is exactly 0: xhat = 0, y = act(beta), and a finite gradient (epsilon is 1e-3)."""
  c = _norm_case(3, 65, 'leaky_relu', True)
  y, grads = _run_norm(c, 'leaky_relu')
  beta = torch.as_tensor(c['ins'][3])
  assert torch.equal(y.detach().cpu()[1], torch.where(beta > 0, beta, 0.2 * beta))
  _check_tensor('norm/constant_row/y', y, c['truth'], c['fp32'])
  for which, got, want in zip(('x', 'bias', 'gamma', 'beta'), grads, c['grads']):
    _check_grad('norm/constant_row/grad_' + which, got, want)


# ---- the GRU --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gru_case(batch, steps, width, hidden, with_state):
  rng = _rng('gru/%d/%d/%d/%d/%d' % (batch, steps, width, hidden, with_state))
  ins = [_f32(rng, batch, steps, width), _f32(rng, width, 3 * hidden, scale=0.3 / np.sqrt(max(width / 16.0, 1.0))),
         _f32(rng, hidden, 3 * hidden, scale=0.3 / np.sqrt(max(hidden / 16.0, 1.0))), _f32(rng, 2, 3 * hidden, scale=0.3)]
  if with_state:
    ins.append(_f32(rng, batch, hidden, scale=0.5))
  cot = _f32(rng, batch, steps, hidden)
  return dict(ins=tuple(ins), cot=cot, truth=T.gru(*ins).numpy(), fp32=T.gru(*ins, dtype=torch.float32).numpy(),
              grads=T.grads(T.gru, ins, [cot]))


def _gru_layer(c, **kw):
  """nn.GRU holding the case's weights -> (layer, x, state or None); all of them leaves."""
  width, hidden = c['ins'][1].shape[0], c['ins'][2].shape[0]
  layer = nn.GRU(hidden, **kw)
  layer.build(width)
  with torch.no_grad():
    for param, value in zip((layer.kernel, layer.recurrent_kernel, layer.bias), c['ins'][1:4]):
      param.copy_(torch.as_tensor(value))
  x, = _dev(c['ins'][0], grad=True)
  state = _dev(c['ins'][4], grad=True)[0] if len(c['ins']) > 4 else None
  return layer, x, state


@pytest.mark.parametrize('with_state', [False, True], ids=['zero_state', 'given_state'])
@pytest.mark.parametrize('batch, steps, width, hidden', GRU_CASES)
def test_gru(ddsp, batch, steps, width, hidden, with_state):
  c = _gru_case(batch, steps, width, hidden, with_state)
  name = 'gru/b%d_t%d_i%d_h%d/%s' % (batch, steps, width, hidden, 'state' if with_state else 'zero')
  layer, x, state = _gru_layer(c, return_sequences=True)
  assert layer.kernel.shape == (width, 3 * hidden) and layer.recurrent_kernel.shape == (hidden, 3 * hidden) and layer.bias.shape == (2, 3 * hidden)
  with torch.no_grad():
    plain = layer(x, state)
  y = layer(x, state)
  assert torch.equal(y.detach(), plain)
  _check_tensor(name + '/y', y, c['truth'], c['fp32'])
  leaves = [x, layer.kernel, layer.recurrent_kernel, layer.bias] + ([state] if with_state else [])
  grads = torch.autograd.grad(y, leaves, _dev(c['cot'])[0])
  for which, got, want in zip(('x', 'kernel', 'recurrent_kernel', 'bias', 'state'), grads, c['grads']):
    _check_grad('%s/grad_%s' % (name, which), got, want)


def test_gru_return_sequences_false_and_return_state(ddsp):
  c = _gru_case(3, 5, 8, 48, True)
  layer, x, state = _gru_layer(c, return_sequences=False, return_state=True)
  last, new_state = layer(x, state)
  assert last.shape == (3, 48) and torch.equal(last, new_state)
  _check_tensor('gru/last_only/y', last, c['truth'][:, -1], c['fp32'][:, -1])
  cot = np.ascontiguousarray(c['cot'][:, -1])
  want = T.grads(lambda *a: T.gru(*a)[:, -1], c['ins'], [cot])
  grads = torch.autograd.grad(last, [x, layer.kernel, layer.recurrent_kernel, layer.bias, state], _dev(cot)[0])
  for which, got, truth in zip(('x', 'kernel', 'recurrent_kernel', 'bias', 'state'), grads, want):
    _check_grad('gru/last_only/grad_' + which, got, truth)


def test_gru_limits(ddsp):
  with pytest.raises(ValueError, match='2048'):
    nn.gru_recurrence(torch.zeros(1, 1, 3 * 2064), torch.zeros(2064, 3 * 2064), torch.zeros(3 * 2064))
  with pytest.raises(ValueError):
    nn.gru_recurrence(torch.zeros(1, 0, 3), torch.zeros(1, 3), torch.zeros(3))
  # 1000 is no multiple of 16: the plain kernel, at a width past 512
  rng = _rng('gru/h1000')
  mx, rk, rb = _f32(rng, 1, 2, 3000), _f32(rng, 1000, 3000, scale=0.03), _f32(rng, 3000, scale=0.3)
  y = nn.gru_recurrence(*_dev(mx, rk, rb))
  _check_tensor('gru/h1000/y', y, T.gru_recurrence(mx, rk, rb).numpy(), T.gru_recurrence(mx, rk, rb, dtype=torch.float32).numpy())


# ---- composed layers ------------------------------------------------------------------------------------------------------
def _draw(module, rng):
  """Overwrites every weight of a BUILT module with drawn values (kernels at 0.3 / sqrt(fan_in / 16) or 0.3, gamma near 1, the
  rest at 0.1) and returns them by parameter name."""
  out = {}
  with torch.no_grad():
    for name, param in module.named_parameters():
      leaf = name.rsplit('.', 1)[-1]
      if leaf in ('kernel', 'recurrent_kernel'):
        value = _f32(rng, *param.shape, scale=0.3 / np.sqrt(max(param.shape[0] / 16.0, 1.0)))
      elif leaf == 'gamma':
        value = _f32(rng, *param.shape, scale=0.1, shift=1.0)
      else:
        value = _f32(rng, *param.shape, scale=0.1)
      param.copy_(torch.as_tensor(value))
      out[name] = value
  return out


def _fc_weights(w, prefix, layers):
  return [tuple(w['%slayers.%d.%s' % (prefix, i, leaf)] for leaf in ('dense.kernel', 'dense.bias', 'layer_norm.gamma', 'layer_norm.beta'))
          for i in range(layers)]


@pytest.mark.parametrize('ch, layers, width', [(2, 1, 3), (64, 3, 5)])
def test_fc_stack(ddsp, ch, layers, width):
  rng = _rng('fc_stack/%d/%d' % (ch, layers))
  x_host, cot = _f32(rng, 2, 4, width), _f32(rng, 2, 4, ch)
  stack = nn.FcStack(ch, layers)
  x, = _dev(x_host, grad=True)
  stack(x)                                              # builds
  w = _draw(stack, rng)
  names = list(w)
  assert names[:4] == ['layers.0.dense.kernel', 'layers.0.dense.bias', 'layers.0.layer_norm.gamma', 'layers.0.layer_norm.beta']
  y = stack(x)
  assert y.shape == (2, 4, ch)

  def truth(x_, *flat, dtype=torch.float64):
    return T.fc_stack(x_, [flat[4 * i: 4 * i + 4] for i in range(layers)], dtype=dtype)

  flat = [w[n] for n in names]
  name = 'fc_stack/ch%d_l%d' % (ch, layers)
  _check_tensor(name + '/y', y, truth(x_host, *flat).numpy(), truth(x_host, *flat, dtype=torch.float32).numpy())
  grads = torch.autograd.grad(y, [x] + [p for _, p in stack.named_parameters()], _dev(cot)[0])
  for which, got, want in zip(['x'] + names, grads, T.grads(truth, [x_host] + flat, [cot])):
    _check_grad('%s/grad_%s' % (name, which), got, want)


def _decoder_truth_fn(names, n_inputs, layers, splits, stateless):
  """(inputs..., [state], weights in `names` order) -> the truth's outputs."""
  def fn(*args, dtype=torch.float64):
    inputs, rest = list(args[:n_inputs]), list(args[n_inputs:])
    state = rest.pop(0) if stateless else None
    w = dict(zip(names, rest))
    weights = dict(input_stacks=[_fc_weights(w, 'input_stacks.%d.' % i, layers) for i in range(n_inputs)],
                   gru=(w['rnn.rnn.kernel'], w['rnn.rnn.recurrent_kernel'], w['rnn.rnn.bias']),
                   out_stack=_fc_weights(w, 'out_stack.', layers), dense_out=(w['dense_out.kernel'], w['dense_out.bias']))
    return T.rnn_fc_decoder(inputs, weights, splits, state=state, dtype=dtype)
  return fn


def _check_decoder(name, rnn_channels, ch, layers, splits, batch, steps, stateless):
  rng = _rng(name)
  keys = ['ld_scaled', 'f0_scaled']
  host = {k: _f32(rng, batch, steps, 1) for k in keys}
  state_host = _f32(rng, batch, rnn_channels, scale=0.5)
  dec = decoders.RnnFcDecoder(rnn_channels=rnn_channels, rnn_type='gru', ch=ch, layers_per_stack=layers, stateless=stateless,
                              input_keys=keys, output_splits=splits)
  feed = {k: _dev(v)[0] for k, v in host.items()}
  if stateless:
    feed['state'] = _dev(state_host, grad=True)[0]
  out = dec(feed)                                       # builds
  out_keys = [k for k, _ in splits] + (['state'] if stateless else [])
  assert list(out) == out_keys and dec.input_keys == keys + (['state'] if stateless else [])
  w = _draw(dec, rng)
  names = list(w)
  out = dec(feed)
  for (k, n) in splits:
    assert out[k].shape == (batch, steps, n)
  if stateless:
    assert out['state'].shape == (batch, rnn_channels) and not torch.equal(out['state'].detach(), feed['state'].detach())
  fn = _decoder_truth_fn(names, len(keys), layers, splits, stateless)
  args = [host[k] for k in keys] + ([state_host] if stateless else []) + [w[n] for n in names]
  truth, fp32 = fn(*args), fn(*args, dtype=torch.float32)
  for k, a, b in zip(out_keys, truth, fp32):
    _check_tensor('%s/%s' % (name, k), out[k], a.numpy(), b.numpy())
  cots = [_f32(rng, *t.shape) for t in truth]
  leaves = ([feed['state']] if stateless else []) + [p for _, p in dec.named_parameters()]
  grads = torch.autograd.grad([out[k] for k in out_keys], leaves, _dev(*cots))
  want = T.grads(fn, args, cots)[len(keys):]
  for which, got, truth_grad in zip((['state'] if stateless else []) + names, grads, want):
    _check_grad('%s/grad_%s' % (name, which), got, truth_grad)


@pytest.mark.parametrize('stateless', [False, True], ids=['stateful', 'stateless'])
def test_rnn_fc_decoder_at_the_reference_test_configuration(ddsp, stateless):
  """ddsp/training/decoders_test.py: rnn_channels=3, ch=2, layers_per_stack=1, two inputs, splits (1, 10), batch 2, 4 steps."""
  _check_decoder('decoder/small/' + ('stateless' if stateless else 'stateful'), 3, 2, 1, (('amps', 1), ('harmonic_distribution', 10)), 2, 4,
                 stateless)


def test_rnn_fc_decoder_at_the_shipped_widths(ddsp):
  _check_decoder('decoder/512', 512, 512, 3, (('amps', 1), ('harmonic_distribution', 100), ('noise_magnitudes', 65)), 2, 6, False)


# ---- bit-stability of the hand-written kernels ---------------------------------------------------------------------------
def _gru_everything(mx, rk, rb, h0):
  leaves = _dev(mx, rk, rb, h0, grad=True)
  y = nn.gru_recurrence(*leaves)
  weights = torch.linspace(0.5, 1.5, y[0].numel(), device=DEV).reshape(y.shape[1:]).expand_as(y).contiguous()
  d_mx, d_h0 = torch.autograd.grad(y, [leaves[0], leaves[3]], weights)
  return [y.detach(), d_mx, d_h0]


@pytest.mark.parametrize('batch, steps, hidden', [(3, 5, 3), (17, 4, 48)])
def test_gru_same_bits_twice_row_alone_and_in_the_batch(ddsp, batch, steps, hidden):
  rng = _rng('bits/gru/%d' % hidden)
  mx, rk, rb, h0 = _f32(rng, batch, steps, 3 * hidden), _f32(rng, hidden, 3 * hidden, scale=0.3), _f32(rng, 3 * hidden, scale=0.3), _f32(rng, batch, hidden, scale=0.5)
  first, second = _gru_everything(mx, rk, rb, h0), _gru_everything(mx, rk, rb, h0)
  for a, b in zip(first, second):
    assert torch.equal(a, b)
  alone = _gru_everything(mx[:1], rk, rb, h0[:1])
  for a, r in zip(first, alone):
    assert torch.equal(a[:1], r)


@pytest.mark.parametrize('rows, ch', [(9, 65), (3, 1000)])
def test_norm_same_bits_twice_row_alone_and_in_the_batch(ddsp, rows, ch):
  c = _norm_case(rows, ch, 'tanh')
  (y1, g1), (y2, g2) = _run_norm(c, 'tanh'), _run_norm(c, 'tanh')
  assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
  alone = dict(ins=(c['ins'][0][:1],) + c['ins'][1:], cot=c['cot'][:1])
  y, g = _run_norm(alone, 'tanh')
  assert torch.equal(y, y1[:1]) and torch.equal(g[0], g1[0][:1])          # the parameter gradients are sums over the rows


def test_gru_replays_from_a_captured_graph(ddsp):
  """No host synchronisation, no allocation by the library, every launch on the current stream in one chain: forward and
  backward of the recurrence are captured once with torch.cuda.graph and replayed - the same bits as the eager call."""
  if DEV != 'cuda' or not torch.cuda.is_available():
    pytest.skip('needs real streams and graphs: left to the GPU run')
  rng = _rng('graph/gru')
  batch, steps, hidden = 2, 8, 16
  host = [_f32(rng, batch, steps, 3 * hidden), _f32(rng, hidden, 3 * hidden, scale=0.3), _f32(rng, 3 * hidden, scale=0.3), _f32(rng, batch, hidden, scale=0.5)]
  other = _f32(rng, batch, steps, 3 * hidden)
  static = _dev(*host, grad=True)
  cot, = _dev(_f32(rng, batch, steps, hidden))

  def step():
    y = nn.gru_recurrence(*static)
    return [y] + list(torch.autograd.grad(y, static, cot))

  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    step()
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    captured = step()
  for mx_new in (host[0], other, other):
    with torch.no_grad():
      static[0].copy_(torch.as_tensor(mx_new))
    graph.replay()
    torch.cuda.synchronize()
    eager = _dev(mx_new, *host[1:], grad=True)
    y = nn.gru_recurrence(*eager)
    for a, b in zip(captured, [y] + list(torch.autograd.grad(y, eager, cot))):
      assert torch.equal(a.detach(), b.detach())


# ---- end to end ------------------------------------------------------------------------------------------------------------
def test_preprocessor_decoder_synths_and_loss_end_to_end(ddsp):
  """f0_hz / loudness_db -> F0LoudnessPreprocessor -> RnnFcDecoder -> ProcessorGroup(Harmonic + FilteredNoise + Add) ->
  SpectralLoss: a finite loss and a finite, non-zero gradient in every decoder weight."""
  rng = _rng('end_to_end')
  frames, n_samples = 8, 512
  f0_hz = (220.0 + 20.0 * rng.standard_normal((1, 4))).astype(np.float32)
  loudness_db = (-30.0 + 5.0 * rng.standard_normal((1, 4))).astype(np.float32)
  target = (0.1 * rng.standard_normal((1, n_samples))).astype(np.float32)
  pre = preprocessing.F0LoudnessPreprocessor(time_steps=frames, compute_loudness=False)
  features = pre(dict(f0_hz=f0_hz, loudness_db=loudness_db))
  assert list(features) == ['f0_hz', 'loudness_db', 'f0_scaled', 'ld_scaled'] and features['f0_scaled'].shape == (1, frames, 1)
  torch.manual_seed(7)
  dec = decoders.RnnFcDecoder(rnn_channels=32, ch=32, layers_per_stack=2, input_keys=('ld_scaled', 'f0_scaled'),
                              output_splits=(('amps', 1), ('harmonic_distribution', 16), ('noise_magnitudes', 9)))
  controls = dec(features)
  dag = [(ddsp.synths.Harmonic(n_samples=n_samples), ['amps', 'harmonic_distribution', 'f0_hz']),
         (ddsp.synths.FilteredNoise(n_samples=n_samples, window_size=0), ['noise_magnitudes']),
         (ddsp.processors.Add(), ['filtered_noise/signal', 'harmonic/signal'])]
  audio = ddsp.processors.ProcessorGroup(dag=dag)(dict(controls, f0_hz=features['f0_hz']))
  loss = ddsp.losses.SpectralLoss(fft_sizes=(128, 64))(_dev(target)[0], audio)
  assert loss.dim() == 0 and bool(torch.isfinite(loss))
  params = dict(dec.named_parameters())
  assert len(params) == 4 * 2 * 3 + 3 + 2
  grads = torch.autograd.grad(loss, list(params.values()))
  for name, grad in zip(params, grads):
    assert bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0.0, name


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  return ddsp_amd
