"""The 2-D convolution and the ResNet layers of ddsp_amd.training on offset, strided and non-fp32 tensors, with a NaN or an Inf in
them, and replayed from a captured graph - the properties the project holds on every entry point, for the public entries that
reach csrc/conv2d.hip: conv2d (the MFMA and the plain kernel), SpatialConv2D, ResidualStack (conditional), ResNet and
ResnetSinusoidalEncoder.

  layouts     tests/test_gpu_layouts.py's one property: a call on tensors of any layout or dtype returns the bits of the same call
              on freshly allocated contiguous fp32 copies of the same values, outputs and input gradients.  The helpers are that
              module's; the rows are here because the C entries behind them sit in ddsp_amd._lib.CONV2D_SIGNATURES, outside the
              table tests/layout_table.py is held to - so this file carries its own coverage check: every name of
              CONV2D_SIGNATURES is reached by a row or EXEMPT with a reason.
  non-finite  DESIGN.md section 9 with tests/test_gpu_nonfinite.py's helpers: a NaN or an Inf in batch row 1 leaves row 0's bits
              (no row is excused), a NaN does not vanish, and what the fp64 truth makes non-finite is non-finite from the kernel.
  graphs      a training step of a small ResidualStack, captured once and replayed on new values, under the criterion
              tests/test_gpu_graph_replay.py applies to the three networks.

A layer's weights are drawn by its initialisers under a fixed seed at every call, so the variant and its reference hold the same
weights.  tests/test_resnet_layouts_emulated.py runs this module through the SIMT emulation on the CPU."""
import zlib

import numpy as np
import pytest
import torch

import layout_table as L
import nonfinite_table as NF
import resnet_truth as RT
import test_gpu_graph_replay as GR
import test_gpu_layouts as GL
import test_gpu_nonfinite as NFT
from ddsp_amd import _lib, spectral_ops
from ddsp_amd.training import encoders, nn

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B, H, W, CH = 2, 5, 6, 16
STRIDES = (1, 2)
SPLITS = (('frequencies', 4), ('amplitudes', 2))


def _seeded(make):
  torch.manual_seed(20261020)
  return make()


def _stack(d, x, z):
  return _seeded(lambda: nn.ResidualStack([4], [2], [2], 'layer', conditional=True))([x, z])


def _encoder(d, audio):
  logmel = lambda a: spectral_ops.compute_logmel(a, bins=16, fft_size=256)
  return _seeded(lambda: encoders.ResnetSinusoidalEncoder(SPLITS, logmel, size='small'))(audio)


def _conv_args(ch_out):
  return [L.N('x', B, H, W, CH), L.N('kernel', 3, 3, CH, ch_out, scale=0.1), L.N('bias', ch_out, scale=0.3),
          L.N('addend', B, H, W // 2, ch_out)]


_conv = lambda d, x, k, b, a: nn.conv2d(x, k, b, STRIDES, relu_input=True, addend=a)
ROWS = [
    L.Row('conv2d', _conv, _conv_args(CH)),
    L.Row('conv2d_plain_kernel', _conv, _conv_args(3)),
    L.Row('SpatialConv2D', lambda d, x: _seeded(lambda: nn.SpatialConv2D(CH, (3, 3), STRIDES))(x), [L.N('x', B, H, W, 8)]),
    L.Row('ResidualStack', _stack, [L.N('x', B, H, W, 8), L.N('z', B, H, 1, 4)]),
    L.Row('ResNet', lambda d, x: _seeded(lambda: nn.ResNet('small'))(x), [L.N('x', B, 3, 9, 1)]),
    L.Row('ResnetSinusoidalEncoder', _encoder, [L.N('audio', B, 1024, scale=0.3, grad=False)]),
]
BY_NAME = {row.name: row for row in ROWS}
EXEMPT = {}        # C entry -> why no row reaches it


def _variant_cases():
  return [pytest.param(row.name, variant, id='%s-%s' % (row.name, variant)) for row in ROWS for variant in GL.VARIANTS
          if any(GL._applies(variant, a, row) for a in row.args)]


@pytest.mark.parametrize('name, variant', _variant_cases())
def test_layout_gives_the_bits_of_fresh_contiguous_fp32(ddsp, name, variant):
  row = BY_NAME[name]
  on = [i for i, a in enumerate(row.args) if GL._applies(variant, a, row)]
  for i in on:                                                   # each argument alone
    GL._check_case(ddsp, row, variant, [i])
  if len(on) > 1:                                                # all at once
    GL._check_case(ddsp, row, variant, on)


class _Counting:
  """The library with every entry point looked up through it noted down."""

  def __init__(self, lib):
    self._lib, self.reached = lib, set()

  def __getattr__(self, name):
    self.reached.add(name)
    return getattr(self._lib, name)


def test_every_conv2d_entry_is_reached_by_a_row_or_exempt_with_a_reason(ddsp):
  load = _lib.load
  counting = _Counting(load())
  try:
    _lib.load = lambda: counting
    for row in ROWS:
      GL._run(ddsp, row, GL._base_values(row), [i for i, a in enumerate(row.args) if a.grad])
  finally:
    _lib.load = load
  missing = sorted(set(_lib.CONV2D_SIGNATURES) - counting.reached - set(EXEMPT))
  assert not missing, 'conv2d entries no row reaches and EXEMPT does not name: %s' % missing
  assert set(EXEMPT) <= set(_lib.CONV2D_SIGNATURES) and not set(EXEMPT) & counting.reached
  assert all(isinstance(reason, str) and len(reason) > 10 for reason in EXEMPT.values())


# ---- non-finite values -----------------------------------------------------------------------------------
def _nonfinite_cases():
  return [pytest.param(row.name, ai, vname, id='%s-%s-%s' % (row.name, arg.name, vname))
          for row in ROWS for ai, arg in enumerate(row.args) for vname in NF.VALUES]


@pytest.mark.parametrize('name, ai, vname', _nonfinite_cases())
def test_one_non_finite_value_stays_in_its_row_and_does_not_vanish(ddsp, name, ai, vname):
  """R1: the call returns.  R2: batch row 0 keeps the bits of the clean call - no row is excused.  R3, weak form: the NaN's batch
  row holds a non-finite output."""
  row = BY_NAME[name]
  result = NFT.run_poisoned(ddsp, row, ai, NF.VALUES[vname])
  assert result is not None, '%s: the Python layer refused the value' % name
  outs, grads, ref_outs, ref_grads = result
  found = NFT.row0_differences(row, ai, outs, grads, ref_outs, ref_grads)
  assert not found, '%s, %s in %s: %s' % (name, vname, row.args[ai].name, '; '.join(found))
  if vname == 'nan':
    assert NFT.non_finite_outputs(row, ai, outs) > 0, '%s: the NaN in %s is gone - every output of its batch row is finite' % (name, row.args[ai].name)


@pytest.mark.parametrize('value', NFT.VALUES3)
@pytest.mark.parametrize('relu', [False, True], ids=['plain', 'relu'])
@pytest.mark.parametrize('ch', [4, 16])
def test_conv2d_keeps_what_the_truth_keeps(ddsp, ch, relu, value):
  """ch 16: the MFMA kernel; ch 4: the plain one.  The value sits in x (+Inf and NaN survive a ReLU; -Inf becomes 0 in the truth
  too, and then there is nothing to keep)."""
  x, k, b = NFT._rng(41, 2, 5, 6, 8), NFT._rng(42, 3, 3, 8, ch, scale=0.3), NFT._rng(43, ch, scale=0.3)
  NFT.strong_form('conv2d ch=%d relu=%s' % (ch, relu), lambda x, k, b: nn.conv2d(x, k, b, STRIDES, relu_input=relu),
                  lambda x, k, b: RT.conv2d(x, k, b, STRIDES, relu_input=relu), [x, k, b], (0, (1, 2, 3, 4)), value)


@pytest.mark.parametrize('value', NFT.VALUES3)
def test_residual_layer_keeps_what_the_truth_keeps(ddsp, value):
  """Layer norm -> ReLU -> the projection and the bottleneck -> x + r.  Weights drawn as tests/test_gpu_resnet.py draws them; the
  output and the gradient in x."""
  import test_gpu_resnet as RG
  layer = nn.ResidualLayer(4, 2, True, 'layer', False, False)
  x = NFT._rng(44, 2, 5, 6, 8)
  layer(NFT._dev(x))                                    # builds
  w = RG._draw(layer, np.random.default_rng(45))
  x[1, 2, 3, 4] = value
  xd = NFT._dev(x).requires_grad_(True)
  y = layer(xd)
  gx, = torch.autograd.grad(y, [xd], torch.ones_like(y))
  xt = torch.as_tensor(x, dtype=torch.float64).requires_grad_(True)
  t = RT.residual_layer(w, '', xt, None, 2, 'layer')
  gt, = torch.autograd.grad(t, [xt], torch.ones_like(t))
  assert NFT.assert_superset('ResidualLayer output', y.detach(), t.detach()) > 0
  NFT.assert_superset('ResidualLayer gradient of x', gx, gt)


# ---- a graphed training step ----------------------------------------------------------------------------------------------------
def test_residual_stack_training_step_replays_from_a_captured_graph(ddsp):
  """Forward + backward into the parameters' .grad, captured once and replayed on two new inputs: outputs and every parameter
  gradient have the bits of the eager step.  Between the capture and the second replay another stack runs eagerly at batch 8 on
  the capture stream - it shares nn's module-global workspaces with the captured one - and the captured scratch must be alive
  before each replay."""
  GR._needs_graphs()
  import test_gpu_resnet as RG
  rng = np.random.default_rng(zlib.crc32(b'graph_replay/ResidualStack'))
  feed = lambda batch: [t for t in RG._dev(RG._f32(rng, batch, H, W, 8), RG._f32(rng, batch, H, 1, 4))]
  stacks = []
  for _ in range(2):
    stack = nn.ResidualStack([4, 8], [2, 1], [1, 2], 'layer', conditional=True)
    with torch.no_grad():
      stack(feed(2))                                    # builds
    RG._draw(stack, rng)
    stacks.append(stack)
  net, other = stacks
  names, params = [n for n, _ in net.named_parameters()], [p for _, p in net.named_parameters()]
  static = feed(2)
  with torch.no_grad():
    cot = torch.as_tensor(RG._f32(rng, *net(static).shape), device=DEV)

  def step():
    out = net(static)
    torch.autograd.backward([out], [cot])
    return [out]

  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    step()
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  for p in params:
    p.grad = None                                                 # the capture allocates them: static tensors of the graph's pool
  graph = torch.cuda.CUDAGraph()
  with GR._recording() as handed:
    with torch.cuda.graph(graph, stream=side):
      outs = step()
  assert handed.items, 'the capture asked for no scratch: this test would check nothing'
  grads = [p.grad for p in params]
  assert all(g is not None for g in grads), [n for n, g in zip(names, grads) if g is None]
  try:
    for n in range(2):
      if n == 1:
        with torch.cuda.stream(side):
          big = other(feed(8))
          torch.autograd.grad([big], list(other.parameters()), [torch.ones_like(big)])
        torch.cuda.synchronize()
      handed.assert_alive('before replay %d' % n)
      new = feed(2)
      with torch.no_grad():
        for s, v in zip(static, new):
          s.copy_(v)
      graph.replay()
      torch.cuda.synchronize()
      eager = [net(new)]
      eager_grads = torch.autograd.grad(eager, params, [cot])
      GR._assert_bits('ResidualStack outputs, replay %d' % n, outs, eager)
      for which, g, r in zip(names, grads, eager_grads):
        GL._same_bits('ResidualStack gradient of %s, replay %d' % (which, n), g, r)
  finally:
    for p in params:
      p.grad = None


@pytest.fixture(scope='module')
def ddsp():
  import ddsp_amd
  assert GL.DEV == DEV and NFT.DEV == DEV and GR.DEV == DEV, 'the borrowed helpers must run on the device this module runs on'
  return ddsp_amd
