"""ddsp_amd.training.nn's vq_assign, vq_statistics and VectorQuantization on the MI355X against tests/vq_truth.py (the reference's
chain in fp64 at the fp32 inputs).  tests/test_vq_emulated.py runs this module through the SIMT emulation on the CPU.

THE INDEX RULE.  No index is compared blindly: two centroids may lie closer to a vector than fp32 can tell apart.  With
GAP = (D + 32) * 2^-23 * (|x|^2 + max_j |e_j|^2) - two scores, each off by at most 2^-22 (|x|^2 + |e|^2) from the 22-bit split
of the matrix-core operands plus the worst-case fp32 accumulation over D terms, then doubled - a vector DECIDES when its fp64
runner-up distance exceeds its fp64 minimum by more than GAP.  Every deciding vector's index must be the fp64 argmin exactly; for
the others the chosen centroid's fp64 distance must lie within GAP of the minimum.  The non-deciding share of a random case is a
condition of the case, asserted at 2 % at the most.  z_q is e[c] bit for bit.

Assignment cases (rows, k, D, heads), the smallest at which each part can go wrong: the smallest legal; the plain kernel; one
column tile with D shorter than a 32-deep step and one row past a 16-row tile; a D tail and the running argmin over three column
tiles; heads read in place; more rows than a block; a wide codebook (eight column chunks).

Statistics: counts are exact; sums may err by 4 x the fp32 one-hot chain's error on the same case, with a floor of eight fp32
ulp of the largest magnitude (as tests/test_gpu_decoder.py applies it).  Every comparison is appended to
the file DDSP_PARITY_LOG names, when it is set.

Measured on the MI355X: see profiles/vq_parity_errors.jsonl and DESIGN.md section 8."""
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import vq_truth as T
from ddsp_amd.training import nn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GRAD_RTOL = 2e-4
TENSOR_RATIO = 4.0
TENSOR_FLOOR = 8 * 2.0 ** -24          # eight fp32 ulp of the tensor's largest magnitude
MAX_UNDECIDED = 0.02

ASSIGN_CASES = [(1, 1, 1, 1), (5, 3, 3, 1), (17, 16, 8, 1), (33, 48, 40, 1), (40, 32, 32, 3), (1025, 16, 16, 1), (64, 1024, 64, 1)]


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


def _rng(name):
  return np.random.default_rng(zlib.crc32(('vq/' + name).encode()))


def _f32(rng, *shape, scale=1.0, shift=0.0):
  return (shift + scale * rng.standard_normal(shape)).astype(np.float32)


def _check_tensor(case, got, truth, faithful):
  got, truth, faithful = _np(got), np.asarray(truth, np.float64), np.asarray(faithful, np.float64)
  scale = float(np.max(np.abs(truth))) if truth.size else 0.0
  scale = scale if scale > 0.0 else 1.0
  err = float(np.max(np.abs(got - truth))) / scale if truth.size else 0.0
  ref_err = float(np.max(np.abs(faithful - truth))) / scale if truth.size else 0.0
  _log(case, kernel_err=err, reference_fp32_err=ref_err, scale=scale)
  assert got.shape == truth.shape and np.isfinite(got).all()
  assert err <= max(TENSOR_RATIO * ref_err, TENSOR_FLOOR), (case, err, ref_err)


def _flat_order(c, heads):
  """c [..., heads] -> the x_flat (head-major) order of the truth's distance matrix."""
  return np.asarray(c).reshape(-1, heads).T.reshape(-1)


def _check_assign(case, x, e, heads, z, c, distance_only=False, max_undecided=MAX_UNDECIDED):
  """The index rule of the module docstring, and z = e[c] bit for bit."""
  x, e = np.asarray(x), np.asarray(e)
  k, dims = e.shape
  z_truth, c_truth, d = T.assign(x, e, heads)
  d = d.numpy()
  flat = T.x_flat(x, heads).numpy()
  gap = (dims + 32) * 2.0 ** -23 * ((flat ** 2).sum(1) + (e.astype(np.float64) ** 2).sum(1).max())
  ordered = np.sort(d, axis=1)
  runner_up = ordered[:, 1] if k > 1 else np.full(len(d), np.inf)
  decides = runner_up - ordered[:, 0] > gap
  got = _flat_order(c.cpu().numpy(), heads)
  want = _flat_order(c_truth.numpy(), heads)
  assert c.dtype == torch.int64 and tuple(c.shape) == tuple(x.shape[:-1]) + (heads,) and got.min() >= 0 and got.max() < k
  excess = d[np.arange(len(d)), got] - ordered[:, 0]
  undecided = 1.0 - float(decides.mean())
  _log(case, undecided_share=undecided, wrong_among_deciding=float((got != want)[decides].sum()), worst_excess_over_gap=float((excess / gap).max()),
       smallest_margin_over_gap=float(((runner_up - ordered[:, 0]) / gap).min()))
  assert (excess <= gap).all(), (case, float((excess / gap).max()))
  if not distance_only:
    assert undecided <= max_undecided, (case, undecided)
    assert (got == want)[decides].all(), (case, int((got != want)[decides].sum()))
  assert tuple(z.shape) == tuple(x.shape) and z.dtype == torch.float32
  picked = torch.as_tensor(e)[c.cpu().reshape(-1, heads)].reshape(x.shape)
  assert torch.equal(z.cpu(), picked), case


@functools.lru_cache(maxsize=None)
def _assign_case(rows, k, dims, heads, shift=0.0):
  rng = _rng('assign/%d/%d/%d/%d/%g' % (rows, k, dims, heads, shift))
  return _f32(rng, rows, heads * dims, shift=shift), _f32(rng, k, dims, shift=shift)


# ---- the assignment ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rows, k, dims, heads', ASSIGN_CASES)
def test_assign(ddsp, rows, k, dims, heads):
  x, e = _assign_case(rows, k, dims, heads)
  z, c = nn.vq_assign(*_dev(x, e), num_heads=heads)
  _check_assign('assign/%dx%dx%dx%d' % (rows, k, dims, heads), x, e, heads, z, c)


def test_assign_restores_the_shape(ddsp):
  rng = _rng('assign/shape')
  x, e = _f32(rng, 2, 7, 1, 16), _f32(rng, 32, 8)
  z, c = nn.vq_assign(*_dev(x, e), num_heads=2)
  assert tuple(z.shape) == (2, 7, 1, 16) and tuple(c.shape) == (2, 7, 1, 2)
  _check_assign('assign/shape', x, e, 2, z, c)
  flat_z, flat_c = nn.vq_assign(*_dev(x.reshape(14, 16), e), num_heads=2)
  assert torch.equal(flat_z.reshape(z.shape), z) and torch.equal(flat_c.reshape(c.shape), c)
  z1, c1 = nn.vq_assign(*_dev(x[0, 0, 0], e), num_heads=2)                       # rank 1
  assert tuple(z1.shape) == (16,) and tuple(c1.shape) == (2,) and torch.equal(z1, z[0, 0, 0]) and torch.equal(c1, c[0, 0, 0])


@pytest.mark.parametrize('k', [64, 13])
def test_assign_clustered(ddsp, k):
  """x = e_j + 0.05 noise: every vector decides, so every index is exact - and is j."""
  rng = _rng('assign/clustered/%d' % k)
  e = _f32(rng, k, 16)
  j = rng.integers(0, k, 300)
  x = e[j] + _f32(rng, 300, 16, scale=0.05)
  z, c = nn.vq_assign(*_dev(x, e))
  _check_assign('assign/clustered/%d' % k, x, e, 1, z, c, max_undecided=0.0)
  assert np.array_equal(c.cpu().numpy()[:, 0], j)


@pytest.mark.parametrize('k', [32, 7])
def test_assign_adversarial_offset(ddsp, k):
  """Both tensors shifted by 30: the scores cancel eleven bits and many vectors fall under the gap.  The distance rule alone."""
  x, e = _assign_case(200, k, 16, 1, shift=30.0)
  z, c = nn.vq_assign(*_dev(x, e))
  _check_assign('assign/offset30/%d' % k, x, e, 1, z, c, distance_only=True)


# ---- ties ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [32, 3])
def test_an_all_zero_codebook_gives_index_zero(ddsp, k):
  x = _f32(_rng('ties/zero/%d' % k), 37, 16)
  z, c = nn.vq_assign(*_dev(x, np.zeros((k, 8), np.float32)), num_heads=2)
  assert not c.any() and not z.any() and tuple(c.shape) == (37, 2)


@pytest.mark.parametrize('k, low, high', [(32, 5, 21), (3, 1, 2)])
def test_identical_centroids_resolve_to_the_lower_index(ddsp, k, low, high):
  rng = _rng('ties/duplicate/%d' % k)
  e = _f32(rng, k, 8)
  e[high] = e[low]
  near = e[low] + _f32(rng, 40, 8, scale=0.01)                                  # vectors whose nearest centroid is the duplicated one
  x = np.concatenate([near, _f32(rng, 60, 8), e[low][None]])
  z, c = nn.vq_assign(*_dev(x, e))
  c = c.cpu().numpy()[:, 0]
  assert not (c == high).any() and (c[:40] == low).all() and c[-1] == low
  assert torch.equal(z.cpu(), torch.as_tensor(e)[c])


# ---- the statistics -----------------------------------------------------------------------------------------------------------
def _stats_cases():
  rng = _rng('stats')
  empty = rng.integers(0, 7, (50, 1))
  empty[empty >= 3] += 1                                                       # nobody in cluster 3
  return {
      'empty_cluster': (_f32(rng, 50, 5), empty, 8, 1),
      'one_cluster': (_f32(rng, 1025, 3, shift=0.5), np.full((1025, 1), 2), 4, 1),
      'heads3': (_f32(rng, 41, 21), rng.integers(0, 5, (41, 3)), 5, 3),
      'wide': (_f32(rng, 9, 300), rng.integers(0, 3, (9, 1)), 3, 1),          # more dims than one wavefront's 256
      'rank3': (_f32(rng, 3, 90, 8), rng.integers(0, 6, (3, 90, 2)), 6, 2),
      'long_lists': (_f32(rng, 9000, 2, shift=1.0), (rng.random((9000, 1)) < 0.01).astype(np.int64), 2, 1),   # a wavefront's list fills up and is added in parts
  }


@pytest.mark.parametrize('name', ['empty_cluster', 'one_cluster', 'heads3', 'wide', 'rank3', 'long_lists'])
def test_statistics(ddsp, name):
  x, c, k, heads = _stats_cases()[name]
  counts, sums = nn.vq_statistics(*_dev(x, c), k, num_heads=heads)
  want_counts, want_sums = T.statistics(x, c, k, heads)
  _, fp32_sums = T.statistics(x, c, k, heads, dtype=torch.float32)
  assert counts.dtype == torch.float32 and tuple(counts.shape) == (k,) and tuple(sums.shape) == (k, x.shape[-1] // heads)
  assert np.array_equal(_np(counts), want_counts.numpy()) and float(counts.sum()) == c.size
  _check_tensor('stats/%s/sums' % name, sums, want_sums.numpy(), fp32_sums.numpy())
  if name == 'empty_cluster':
    assert float(counts[3]) == 0.0 and not sums[3].any()
  again = nn.vq_statistics(*_dev(x, c), k, num_heads=heads)
  assert torch.equal(again[0], counts) and torch.equal(again[1], sums)          # run to run


# ---- the layer ------------------------------------------------------------------------------------------------------------------
def _layer_with_state(rng, k, depth, heads, **kwargs):
  layer = nn.VectorQuantization(k, num_heads=heads, **kwargs)
  layer.build(depth)
  counts = (1.0 + rng.random(k) * 5.0).astype(np.float32)
  sums = (_f32(rng, k, depth // heads) * counts[:, None]).astype(np.float32)
  with torch.no_grad():
    layer.counts.copy_(torch.as_tensor(counts))
    layer.sums.copy_(torch.as_tensor(sums))
  return layer, counts, sums


@pytest.mark.parametrize('k, heads', [(16, 2), (5, 1)])
def test_two_training_calls_without_restarts(ddsp, k, heads):
  rng = _rng('layer/train/%d/%d' % (k, heads))
  depth, gamma = 8 * heads, 0.9
  layer, counts, sums = _layer_with_state(rng, k, depth, heads, gamma=gamma, restart_threshold=-1.0)
  assert layer.counts.device.type == torch.device(DEV).type
  for call in range(2):
    x = _f32(rng, 3, 20, depth)
    before = (layer.counts.cpu().clone(), layer.sums.cpu().clone())
    e = layer.centroids().cpu().numpy()                                         # the very centroids the call sees
    z, c = layer(_dev(x)[0], training=True)
    _check_assign('layer/train/%d/%d/call%d' % (k, heads, call), x, e, heads, z, c)
    # the truth from the SAME state and the indices the rule has just accepted: the moving averages
    want = T.training_step(x, *before, gamma, heads)
    faithful = T.training_step(x, *before, gamma, heads, dtype=torch.float32)
    assert torch.equal(c.cpu(), want[1]), 'a vector under the gap: draw another case'
    _check_tensor('layer/train/%d/%d/call%d/z' % (k, heads, call), z, want[0].numpy(), faithful[0].numpy())
    _check_tensor('layer/train/%d/%d/call%d/counts' % (k, heads, call), layer.counts, want[2].numpy(), faithful[2].numpy())
    _check_tensor('layer/train/%d/%d/call%d/sums' % (k, heads, call), layer.sums, want[3].numpy(), faithful[3].numpy())


def test_eval_call_unquantize_and_the_straight_through_gradient(ddsp):
  rng = _rng('layer/eval')
  layer, counts, sums = _layer_with_state(rng, 32, 16, 2)
  x, w = _dev(_f32(rng, 4, 9, 16), _f32(rng, 4, 9, 16))
  x.requires_grad_(True)
  z, c = layer(x)
  assert torch.equal(layer.counts.cpu(), torch.as_tensor(counts)) and torch.equal(layer.sums.cpu(), torch.as_tensor(sums))   # eval: no update
  assert z.requires_grad and tuple(c.shape) == (4, 9, 2) and torch.equal(layer.unquantize(c), z.detach())
  grad, = torch.autograd.grad((z * w).sum(), x)
  assert torch.equal(grad, w)
  plain_z, plain_c = layer(x.detach())
  assert not plain_z.requires_grad and torch.equal(plain_z, z.detach()) and torch.equal(plain_c, c)
  assert set(layer.state_dict()) == {'counts', 'sums'}


def test_commitment_loss(ddsp):
  rng = _rng('layer/loss')
  layer, _, _ = _layer_with_state(rng, 32, 16, 1, commitment_loss_weight=0.3)
  x = _f32(rng, 5, 7, 16)
  enc, = _dev(x, grad=True)
  z, _ = layer(enc)
  loss = layer.committment_loss(enc, z)
  grad, = torch.autograd.grad(loss, enc)
  want, want_grad = T.commitment_loss(x, _np(z), 0.3)
  faithful, _ = T.commitment_loss(x, _np(z), 0.3, dtype=torch.float32)
  _check_tensor('layer/loss', loss, want.numpy(), faithful.numpy())
  g = _np(grad)
  err = float(np.max(np.abs(g - want_grad.numpy()))) / float(np.max(np.abs(want_grad.numpy())))
  _log('layer/loss/grad', grad_err=err)
  assert err <= GRAD_RTOL
  losses = layer.get_losses_dict(enc, z)
  assert list(losses) == ['vector_quantization_commitment_loss'] and torch.equal(losses['vector_quantization_commitment_loss'], loss)


def _segments(values, heads):
  """The head segments of [..., depth] as a set of byte strings."""
  a = np.ascontiguousarray(values.detach().cpu().numpy().reshape(-1, values.shape[-1] // heads))
  return [row.tobytes() for row in a]


def test_restarts_draw_the_centroids_from_the_batch(ddsp):
  """A fresh layer: every count is 0, so every centroid restarts.  n >= k: all of them become vectors of the batch."""
  torch.manual_seed(11)
  rng = _rng('layer/restart/many')
  k, heads, gamma = 16, 2, 0.99
  layer = nn.VectorQuantization(k, gamma=gamma, num_heads=heads)
  x = _f32(rng, 40, 8)
  z, c = layer(_dev(x)[0], training=True)
  n = 40 * heads
  vectors = set(_segments(torch.as_tensor(x), heads))
  got = _segments(z, heads)
  assert all(s in vectors for s in got) and len(set(got)) <= k
  assert abs(float(layer.counts.sum()) - (1 - gamma) * n) <= 1e-5 * (1 - gamma) * n
  assert tuple(layer.sums.shape) == (k, 4) and int(c.min()) >= 0 and int(c.max()) < k


def test_restarts_beyond_the_batch_are_uniform(ddsp):
  """n < k: a segment of z is a vector of the batch or one of the U[0, 1) centroids."""
  torch.manual_seed(12)
  rng = _rng('layer/restart/few')
  layer = nn.VectorQuantization(16)
  x = _f32(rng, 3, 4, shift=3.0)
  z, _ = layer(_dev(x)[0], training=True)
  vectors = set(_segments(torch.as_tensor(x), 1))
  for row, s in zip(z.cpu().numpy(), _segments(z, 1)):
    assert s in vectors or ((row >= 0.0) & (row < 1.0)).all()


def test_depth_must_split_into_the_heads(ddsp):
  with pytest.raises(ValueError, match='Input depth must be a multiple of the number of heads.'):
    nn.VectorQuantization(8, num_heads=3)(_dev(np.zeros((2, 8), np.float32))[0])


def test_single_gru(ddsp):
  torch.manual_seed(3)
  stack = nn.SingleGru(gru_dim=16)
  y = stack(_dev(_f32(_rng('single_gru'), 2, 5, 4))[0])
  assert [type(m) for m in stack.layers] == [nn.GRU, nn.LayerNormalization] and stack.layers[0].return_sequences
  assert tuple(y.shape) == (2, 5, 16) and bool(torch.isfinite(y).all())
  assert sorted(name for name, _ in stack.named_parameters()) == ['layers.0.bias', 'layers.0.kernel', 'layers.0.recurrent_kernel',
                                                                   'layers.1.beta', 'layers.1.gamma']


# ---- bit stability, views, non-finite values --------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [32, 5])
def test_same_bits_twice_and_for_a_row_alone(ddsp, k):
  rng = _rng('bits/%d' % k)
  x, e = _dev(_f32(rng, 70, 24), _f32(rng, k, 12))
  z, c = nn.vq_assign(x, e, num_heads=2)
  z2, c2 = nn.vq_assign(x, e, num_heads=2)
  assert torch.equal(z, z2) and torch.equal(c, c2)
  for row in (0, 17, 69):
    z1, c1 = nn.vq_assign(x[row:row + 1] * 1.0, e, num_heads=2)
    assert torch.equal(z1[0], z[row]) and torch.equal(c1[0], c[row])


@pytest.mark.parametrize('k', [16, 3])
def test_views_and_dtypes_give_the_contiguous_fp32_bits(ddsp, k):
  rng = _rng('views/%d' % k)
  e, = _dev(_f32(rng, k, 8))
  big, = _dev(_f32(rng, 11, 40))
  one, = _dev(_f32(rng, 1, 16))
  half = big[:, :16].to(torch.float16)
  views = {
      'offset': big[1:, 3:19],
      'transposed': big[:, :16].t().contiguous().t(),
      'expanded': one.expand(6, 16),
      'fp64': big[:, :16].to(torch.float64),
      'fp16': half,
      'bf16': big[:, :16].to(torch.bfloat16),
  }
  for name, view in views.items():
    assert name in ('fp64', 'fp16', 'bf16') or not view.is_contiguous(), name
    fresh = view.to(torch.float32).contiguous().clone()
    z, c = nn.vq_assign(view, e, num_heads=2)
    z0, c0 = nn.vq_assign(fresh, e, num_heads=2)
    assert z.dtype == torch.float32 and z.is_contiguous() and torch.equal(z, z0) and torch.equal(c, c0), name
    counts, sums = nn.vq_statistics(view, c.to(torch.int32), k, num_heads=2)
    counts0, sums0 = nn.vq_statistics(fresh, c0, k, num_heads=2)
    assert torch.equal(counts, counts0) and torch.equal(sums, sums0), name
  e_view = torch.cat([e, e], 1)[:, 3:11]
  z, c = nn.vq_assign(big[:, :16], e_view.to(torch.float64), num_heads=2)
  z0, c0 = nn.vq_assign(big[:, :16].contiguous(), e_view.contiguous(), num_heads=2)
  assert torch.equal(z, z0) and torch.equal(c, c0)


@pytest.mark.parametrize('k', [16, 3])
def test_non_finite_vectors_take_index_zero_and_keep_their_nan(ddsp, k):
  rng = _rng('nonfinite/%d' % k)
  x, e = _f32(rng, 20, 16), _f32(rng, k, 8)
  clean_z, clean_c = nn.vq_assign(*_dev(x, e), num_heads=2)
  x[1, 2] = np.nan
  x[3, 8:] = np.inf
  x[4, 0] = -np.inf
  x[19, 15] = np.nan
  z, c = nn.vq_assign(*_dev(x, e), num_heads=2)
  z, c = z.cpu().numpy(), c.cpu().numpy()
  hit = np.zeros((20, 2), bool)
  hit[1, 0] = hit[3, 1] = hit[4, 0] = hit[19, 1] = True
  assert (c[hit] == 0).all() and np.array_equal(c[~hit], clean_c.cpu().numpy()[~hit])
  assert np.array_equal(np.isnan(z), ~np.isfinite(x))
  segments, x_segments = z.reshape(20, 2, 8), x.reshape(20, 2, 8)
  for i, h in zip(*np.nonzero(hit)):
    keep = np.isfinite(x_segments[i, h])
    assert np.array_equal(segments[i, h][keep], e[0][keep])
  assert np.array_equal(segments[~hit], clean_z.cpu().numpy().reshape(20, 2, 8)[~hit])


# ---- graphs -------------------------------------------------------------------------------------------------------------------
def test_eval_call_and_commitment_loss_replay_from_a_captured_graph(ddsp):
  """No host synchronisation, no allocation by the library, every launch on the current stream in one chain: the eval call and
  the commitment loss, forward and backward, are captured once with torch.cuda.graph and replayed - the eager bits."""
  if DEV != 'cuda' or not torch.cuda.is_available():
    pytest.skip('needs real streams and graphs: left to the GPU run')
  rng = _rng('graph')
  layer, _, _ = _layer_with_state(rng, 32, 16, 2)
  first, other = _f32(rng, 6, 10, 16), _f32(rng, 6, 10, 16)
  static, = _dev(first, grad=True)

  def step(x):
    z, c = layer(x)
    loss = layer.committment_loss(x, z)
    return [z, c, loss] + list(torch.autograd.grad(loss, x))

  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    step(static)
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph, stream=side):
    captured = step(static)
  for x_new in (first, other, other):
    with torch.no_grad():
      static.copy_(torch.as_tensor(x_new))
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, step(_dev(x_new, grad=True)[0])):
      assert torch.equal(a.detach(), b.detach())


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  return ddsp_amd
