"""ddsp_amd.training.nn on the MI355X against tests/notes_truth.py (the reference's chain in fp64 at the fp32 inputs).
tests/test_notes_emulated.py runs this module through the SIMT emulation on the CPU.

Tolerances (as tests/test_gpu_hmm.py applies them): masks, lengths and the short-note mask EXACTLY;
output tensors: the kernel's error against the fp64 truth may be up to 4 x that of the truth helper's fp32 mode on the same
case, with a floor of eight fp32 ulp of the tensor's largest magnitude; gradients 2e-4 of the largest element of each
gradient.  Every comparison is appended to the file DDSP_PARITY_LOG names, when it is set.

Shapes (time, max_regions, dims) at batch 2, the smallest at which each part can go wrong: the smallest legal; the worked
example of tests/test_notes_host.py (also with max_regions = 2, so that steps fall off the end); small odd sizes; one
wavefront of everything; one past a wavefront; past a 256-step scan chunk; the shipped shape; a row that is ONE note over the
whole clip (the long accumulation); more regions than max_regions.

Measured on the MI355X: see profiles/notes_parity_errors.jsonl and DESIGN.md section 8."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import notes_truth as T
from ddsp_amd.training import nn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRAD_RTOL = 2e-4
TENSOR_RATIO = 4.0
TENSOR_FLOOR = 8 * 2.0 ** -24          # eight fp32 ulp of the tensor's largest magnitude
BATCH = 2

# name -> (time, max_regions, dims, mean note length, row 0 is one note)
CASES = {
    't2_n1_d1': (2, 1, 1, 1, False),
    't7_n4_d1': (7, 4, 1, 2, False),
    't7_n2_d1': (7, 2, 1, 2, False),
    't33_n5_d3': (33, 5, 3, 5, False),
    't64_n64_d64': (64, 64, 64, 2, False),
    't65_n65_d65': (65, 65, 65, 2, False),
    't257_n100_d128': (257, 100, 128, 3, False),
    't1000_n100_d128': (1000, 100, 128, 12, False),
    't1000_n100_d16_one_note': (1000, 100, 16, 12, True),
    't1000_n100_d16_short_notes': (1000, 100, 16, 4, False),
}
NAMES = list(CASES)
WORKED_EXAMPLE = [60, 60, 0, 0, 62, 62, 64]


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


def _f64(*tensors):
  return [t.detach().numpy().astype(np.float64) for t in tensors]


def _seq(out):
  return list(out) if isinstance(out, (tuple, list)) else [out]


def _moment_truths(case, x, mask, tag):
  """Everything the truth says about get_note_moments and pool_over_notes of (x, mask), under keys that start with `tag`."""
  for fn_name, fn in (('moments', T.moments), ('pool', T.pool)):
    for std in (True, False):
      key = '%s/%s/%s' % (tag, fn_name, 'std' if std else 'mean')
      case[key] = _f64(*_seq(fn(x, mask, std)))
      case[key + '/fp32'] = _f64(*_seq(fn(x, mask, std, dtype=torch.float32)))
      case[key + '/grad'] = T.grads(lambda v, f=fn, s=std: f(v, mask, s), (x,), case[tag + '/cot/' + fn_name][:2 if std else 1])


@functools.lru_cache(maxsize=None)
def _case(name):
  """The inputs of a case and everything the truth says about them, computed once and never changed."""
  steps, regions, dims, mean_length, one_note = CASES[name]
  rng = np.random.default_rng(zlib.crc32(('notes/' + name).encode()))
  q, onset = T.make_pitch(rng, BATCH, steps, mean_length)
  if steps == 7:
    q[0] = WORKED_EXAMPLE
  if one_note:
    q[0] = 60.0
  x = rng.standard_normal((BATCH, steps, dims)).astype(np.float32)
  case = dict(name=name, q=q, onset=onset, x=x, regions=regions)
  for on_only in (True, False):
    case['mask', on_only] = T.get_note_mask(q, regions, on_only).numpy().astype(np.float32)
    case['onset_mask', on_only] = T.get_note_mask_from_onset(q, onset, regions, on_only).numpy().astype(np.float32)
  mask = case['mask', False]
  case['lengths'] = T.get_note_lengths(torch.as_tensor(mask)).numpy()
  case['pitches'] = T.get_note_moments(q, mask, return_std=False, dtype=torch.float32).numpy()
  case['short'] = T.get_short_note_loss_mask(torch.as_tensor(mask), torch.as_tensor(case['lengths']), torch.as_tensor(case['pitches']),
                                             min_length=mean_length).numpy()
  cot = lambda *shape: rng.standard_normal(shape).astype(np.float32)
  case['3d/cot/moments'] = [cot(BATCH, regions, dims), cot(BATCH, regions, dims)]
  case['3d/cot/pool'] = [cot(BATCH, steps, dims), cot(BATCH, steps, dims)]
  _moment_truths(case, x, mask, '3d')
  return case


def _check_tensor(case, got, truth, faithful):
  got = _np(got)
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


def _check_moments_and_pooling(c, x_host, mask_host, tag):
  """Both functions, return_std both ways: values, then the gradient in x under a random cotangent on every output."""
  mask, = _dev(mask_host)
  for fn_name, fn in (('moments', nn.get_note_moments), ('pool', nn.pool_over_notes)):
    for std in (True, False):
      key = '%s/%s/%s' % (tag, fn_name, 'std' if std else 'mean')
      x, = _dev(x_host, grad=True)
      with torch.no_grad():
        plain = _seq(fn(x, mask, return_std=std))                 # the forward-only route
      outs = _seq(fn(x, mask, return_std=std))
      assert len(outs) == (2 if std else 1)
      for i, (out, flat) in enumerate(zip(outs, plain)):
        assert out.requires_grad and not flat.requires_grad and torch.equal(out.detach(), flat)
        _check_tensor('%s/%s/out%d' % (c['name'], key, i), out, c[key][i], c[key + '/fp32'][i])
      cots = _dev(*c[tag + '/cot/' + fn_name][:len(outs)])
      grad, = torch.autograd.grad(outs, x, cots)
      _check_grad('%s/%s/grad' % (c['name'], key), grad, c[key + '/grad'][0])


@pytest.mark.parametrize('name', NAMES)
def test_masks_lengths_and_short_note_mask(ddsp, name):
  c = _case(name)
  q, onset = _dev(c['q'], c['onset'])
  for on_only in (True, False):
    for got, want in ((nn.get_note_mask(q, c['regions'], on_only), c['mask', on_only]),
                      (nn.get_note_mask(q[:, :, None], max_regions=c['regions'], note_on_only=on_only), c['mask', on_only]),
                      (nn.get_note_mask_from_onset(q, onset, c['regions'], on_only), c['onset_mask', on_only]),
                      (nn.get_note_mask_from_onset(q[:, :, None], onset[:, :, None], c['regions'], on_only), c['onset_mask', on_only])):
      assert got.dtype is torch.float32 and not got.requires_grad
      assert np.array_equal(got.cpu().numpy(), want), (name, on_only)
  mask, = _dev(c['mask', False])
  lengths = nn.get_note_lengths(mask)
  assert np.array_equal(lengths.cpu().numpy(), c['lengths'])
  pitches = nn.get_note_moments(q, mask, return_std=False)
  _check_tensor(name + '/note_pitches', pitches, T.get_note_moments(c['q'], c['mask', False], False).numpy(), c['pitches'].astype(np.float64))
  steps, _, _, mean_length, _ = CASES[name]
  short = nn.get_short_note_loss_mask(mask, lengths, _dev(c['pitches'])[0], min_length=mean_length)
  assert short.shape == (BATCH, steps) and np.array_equal(short.cpu().numpy(), c['short'])
  if steps >= 33:
    assert 0.0 < c['short'].mean() < 1.0, 'the case must have short and long notes'


def test_masks_take_no_gradient(ddsp):
  c = _case('t33_n5_d3')
  q, onset = _dev(c['q'], c['onset'], grad=True)
  assert not nn.get_note_mask(q, 5).requires_grad and not nn.get_note_mask_from_onset(q, onset, 5).requires_grad
  x, mask = _dev(c['x'], c['mask', False], grad=True)
  with pytest.raises(NotImplementedError, match='note_mask'):
    nn.get_note_moments(x, mask)
  with pytest.raises(NotImplementedError, match='note_mask'):
    nn.pool_over_notes(x, mask)


@pytest.mark.parametrize('name', NAMES)
def test_moments_pooling_and_gradients(ddsp, name):
  c = _case(name)
  _check_moments_and_pooling(c, c['x'], c['mask', False], '3d')


@functools.lru_cache(maxsize=None)
def _case_2d(name):
  c = _case(name)
  steps, regions = c['x'].shape[1], c['regions']
  rng = np.random.default_rng(zlib.crc32(('notes/2d/' + name).encode()))
  x = np.ascontiguousarray(c['x'][:, :, 0])
  out = dict(name=name + '/2d', x=x)
  cots = [rng.standard_normal((BATCH, regions)).astype(np.float32) for _ in range(2)]
  mask = c['mask', True]
  out['truth'] = _f64(*T.moments(x, mask, True))
  out['fp32'] = _f64(*T.moments(x, mask, True, dtype=torch.float32))
  out['grad'] = T.grads(lambda v: T.moments(v, mask, True), (x,), cots)[0]
  out['cots'] = cots
  return out


@pytest.mark.parametrize('name', NAMES)
def test_moments_of_2d_x_on_the_note_on_mask(ddsp, name):
  """x [batch, time] -> [batch, notes]; the note_on_only mask has empty regions (silences, and regions past the last note)."""
  c, c2 = _case(name), _case_2d(name)
  x, = _dev(c2['x'], grad=True)
  mask, = _dev(c['mask', True])
  outs = nn.get_note_moments(x, mask)
  for i, out in enumerate(outs):
    assert out.shape == (BATCH, c['regions'])
    _check_tensor('%s/out%d' % (c2['name'], i), out, c2['truth'][i], c2['fp32'][i])
  grad, = torch.autograd.grad(outs, x, _dev(*c2['cots']))
  _check_grad(c2['name'] + '/grad', grad, c2['grad'])
  mean_only = nn.get_note_moments(x, mask, return_std=False)
  assert torch.equal(mean_only.detach(), outs[0].detach())


@functools.lru_cache(maxsize=None)
def _case_non_binary():
  steps, regions, dims = 33, 5, 3
  rng = np.random.default_rng(zlib.crc32(b'notes/non_binary'))
  x = rng.standard_normal((BATCH, steps, dims)).astype(np.float32)
  mask = np.where(rng.uniform(size=(BATCH, steps, regions)) < 0.3, rng.uniform(0.0, 2.0, (BATCH, steps, regions)), 0.0).astype(np.float32)
  mask[mask < 1e-3] = 0.0
  mask[1, :, 4] = 0.0                                                  # and one empty note
  cot = lambda *shape: rng.standard_normal(shape).astype(np.float32)
  case = dict(name='non_binary_t33_n5_d3', x=x, mask=mask)
  case['nb/cot/moments'] = [cot(BATCH, regions, dims), cot(BATCH, regions, dims)]
  case['nb/cot/pool'] = [cot(BATCH, steps, dims), cot(BATCH, steps, dims)]
  _moment_truths(case, x, mask, 'nb')
  return case


def test_non_binary_mask(ddsp):
  """30 % non-zeros drawn from (0, 2): weights m in the mean, m ** 2 in the variance, several notes per step."""
  c = _case_non_binary()
  assert 0.2 < (c['mask'] != 0.0).mean() < 0.4 and ((c['mask'] != 0.0).sum(-1) > 1).any()
  _check_moments_and_pooling(c, c['x'], c['mask'], 'nb')


@functools.lru_cache(maxsize=None)
def _case_empty():
  """Row 0: a four-step note on which x is CONSTANT in dimension 1, a silence, two one-step notes, a long note; 8 regions for 5
  used.  Row 1: one-step notes throughout, which overflow the 8 regions."""
  steps, regions, dims = 33, 8, 3
  rng = np.random.default_rng(zlib.crc32(b'notes/empty'))
  q = np.zeros((BATCH, steps), np.float32)
  q[0, :4], q[0, 4:9], q[0, 9], q[0, 10], q[0, 11:] = 60.0, 0.0, 61.0, 62.0, 64.0
  q[1] = 40.0 + np.arange(steps)
  x = (3.0 * rng.standard_normal((BATCH, steps, dims))).astype(np.float32)
  x[0, :4, 1] = np.float32(0.7)
  mask = T.get_note_mask(q, regions, True).numpy().astype(np.float32)
  case = dict(name='empty_t33_n8_d3', q=q, x=x, mask=mask)
  cots = [rng.standard_normal((BATCH, regions, dims)).astype(np.float32) for _ in range(2)]
  cots[1][0, 0, 1] = 0.0                                               # the constant dimension's std: its gradient is not taken
  case['cots'] = cots
  case['truth'] = _f64(*T.get_note_moments(x, mask))
  case['fp32'] = _f64(*T.get_note_moments(x, mask, dtype=torch.float32))
  case['grad'] = T.grads(lambda v: T.get_note_moments(v, mask), (x,), cots)[0]
  case['pool'] = _f64(*T.pool_over_notes(x, mask))
  return case


def test_empty_regions_one_step_notes_and_a_constant_dimension(ddsp):
  c = _case_empty()
  lengths = c['mask'].sum(1)
  assert (lengths[0] == [4, 0, 1, 1, 22, 0, 0, 0]).all() and (lengths[1] == 1).all()
  x, = _dev(c['x'], grad=True)
  q, = _dev(c['q'])
  mask = nn.get_note_mask(q, 8)
  assert np.array_equal(mask.cpu().numpy(), c['mask'])
  mean, std = nn.get_note_moments(x, mask)
  # the constant dimension apart, the project's tolerance; its std against an ABSOLUTE one: the floor times the scale of x
  keep = np.ones(c['truth'][1].shape, bool)
  keep[0, 0, 1] = False
  _check_tensor(c['name'] + '/mean', mean, c['truth'][0], c['fp32'][0])
  _check_tensor(c['name'] + '/std', torch.where(torch.as_tensor(keep, device=DEV), std, torch.zeros_like(std)),
                np.where(keep, c['truth'][1], 0.0), np.where(keep, c['fp32'][1], 0.0))
  constant_err = abs(float(std.detach()[0, 0, 1]) - c['truth'][1][0, 0, 1])
  _log(c['name'] + '/constant_dimension_std', abs_err=constant_err, truth=c['truth'][1][0, 0, 1])
  assert constant_err <= TENSOR_FLOOR * float(np.max(np.abs(c['x'])))
  # empty regions and one-step notes: mean 0 / the value itself, std exactly 0, and finite gradients
  got_mean, got_std = mean.detach().cpu().numpy(), std.detach().cpu().numpy()
  empty = lengths == 0
  assert (got_mean[empty] == 0.0).all() and (got_std[empty] == 0.0).all() and (got_std[lengths == 1] == 0.0).all()
  assert np.array_equal(got_mean[1], c['x'][1, :8])
  grad, = torch.autograd.grad((mean, std), x, _dev(*c['cots']))
  _check_grad(c['name'] + '/grad', grad, c['grad'])
  assert (grad[1, 8:] == 0.0).all()                                    # steps past the last region belong to no note
  pooled = nn.pool_over_notes(x, mask)
  for i in range(2):
    _check_tensor('%s/pool%d' % (c['name'], i), pooled[i], c['pool'][i], c['pool'][i])


def _everything(q, onset, x, regions):
  q, onset = _dev(q, onset)
  x, = _dev(x, grad=True)
  masks = [nn.get_note_mask(q, regions, True), nn.get_note_mask(q, regions, False), nn.get_note_mask_from_onset(q, onset, regions)]
  mask = masks[1]
  moments = nn.get_note_moments(x, mask)
  pooled = nn.pool_over_notes(x, mask)
  weights = [torch.linspace(0.5, 1.5, o[0].numel(), device=DEV).reshape(o.shape[1:]).expand_as(o).contiguous() for o in moments + pooled]
  grads = [torch.autograd.grad(moments, x, weights[:2])[0], torch.autograd.grad(pooled, x, weights[2:])[0]]
  short = nn.get_short_note_loss_mask(mask, nn.get_note_lengths(mask), nn.get_note_moments(q, mask, False), 3)
  return masks + [o.detach() for o in moments + pooled] + grads + [short]


@pytest.mark.parametrize('name', ['t33_n5_d3', 't65_n65_d65', 't257_n100_d128'])
def test_same_bits_twice_row_alone_and_in_the_batch(ddsp, name):
  c = _case(name)
  first = _everything(c['q'], c['onset'], c['x'], c['regions'])
  second = _everything(c['q'], c['onset'], c['x'], c['regions'])
  for a, b in zip(first, second):
    assert torch.equal(a, b)
  alone = _everything(c['q'][:1], c['onset'][:1], c['x'][:1], c['regions'])
  for a, r in zip(first, alone):
    assert torch.equal(a[:1], r)


def test_pool_over_notes_replays_from_a_captured_graph(ddsp):
  """No host synchronisation, no read-back, every launch on the current stream: pool_over_notes is captured once with
  torch.cuda.graph and replayed on new x written into the captured buffer - the same bits as the eager call."""
  if DEV != 'cuda' or not torch.cuda.is_available():
    pytest.skip('needs real streams and graphs: left to the GPU run')
  c = _case('t257_n100_d128')
  mask, = _dev(c['mask', False])
  x_first, x_second = _dev(c['x'], np.ascontiguousarray(c['x'][::-1]))
  static_x = x_first.clone()
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side), torch.no_grad():
    nn.pool_over_notes(static_x, mask)
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side), torch.no_grad():
    captured = nn.pool_over_notes(static_x, mask)
  for x_new in (x_first, x_second):
    static_x.copy_(x_new)
    graph.replay()
    torch.cuda.synchronize()
    with torch.no_grad():
      eager = nn.pool_over_notes(x_new, mask)
    for a, b in zip(captured, eager):
      assert torch.equal(a, b)
  flipped = x_second.cpu().numpy()                                     # the replay worked on the NEW x, not on the captured one
  _check_tensor(c['name'] + '/graph/pool_mean', captured[0], _f64(T.pool(flipped, c['mask', False])[0])[0],
                _f64(T.pool(flipped, c['mask', False], dtype=torch.float32)[0])[0])


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  return ddsp_amd
