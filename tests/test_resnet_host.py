"""Host tests of the 2-D convolution and the ResNet layers (no GPU): tests/resnet_truth.py's explicit shifted sums against an
independent statement in fp64 - F.conv2d / F.max_pool2d on an explicitly F.pad-ded permuted tensor - to 1e-12 in values and
gradients, the asymmetric cases included (an even width at stride 2, even kernel sizes); the truth's gather form of the adjoint
against autograd of the truth; the output-size and padding arithmetic at the model's own widths; constructor defaults and argument
order against values typed in from the reference; weight names, layouts and initialiser fans (the kernels through the SIMT
emulation, on host memory); every ValueError and limit with no device present; the C ABI of csrc/conv2d_abi.h against
ddsp_amd._lib.CONV2D_SIGNATURES and the built library, and its error codes."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resnet_truth as T
from ddsp_amd import _lib
from ddsp_amd import build as build_mod
from ddsp_amd.training import encoders, nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12

# (h, w, ch_in, ch_out, kh, kw, sh, sw): the GPU tests' geometries and a few more
GEOMETRIES = [(1, 1, 1, 1, 1, 1, 1, 1), (5, 6, 2, 4, 3, 3, 1, 1), (5, 6, 3, 2, 3, 3, 1, 2), (5, 7, 3, 2, 3, 3, 1, 2), (3, 9, 1, 4, 7, 7, 1, 2),
              (9, 11, 3, 2, 3, 3, 1, 1), (4, 5, 3, 5, 1, 1, 1, 1), (4, 8, 2, 3, 1, 1, 1, 2), (6, 10, 2, 3, 2, 4, 2, 3), (7, 7, 2, 2, 4, 2, 3, 2),
              (8, 8, 2, 2, 2, 2, 2, 2), (5, 5, 1, 2, 1, 1, 3, 3)]


def _close(a, b):
  a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
  assert a.shape == b.shape
  assert float(np.max(np.abs(a - b))) <= TOL * max(1.0, float(np.max(np.abs(b)))), float(np.max(np.abs(a - b)))


def _tf_same(n, k, s):
  """Typed in from kernel_shape_util.cc: (out, pad_before, pad_after)."""
  out = (n + s - 1) // s
  needed = max(0, (out - 1) * s + k - n)
  return out, needed // 2, needed - needed // 2


# ---- the truth against an independent implementation ---------------------------------------------------------------------
@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('h, w, ch_in, ch_out, kh, kw, sh, sw', GEOMETRIES)
def test_truth_conv2d_is_conv2d_of_torch_on_the_explicitly_padded_tensor(h, w, ch_in, ch_out, kh, kw, sh, sw, relu):
  rng = np.random.default_rng(31)
  x, kernel, bias = rng.standard_normal((2, h, w, ch_in)), rng.standard_normal((kh, kw, ch_in, ch_out)), rng.standard_normal(ch_out)
  (out_h, top, bottom), (out_w, left, right) = _tf_same(h, kh, sh), _tf_same(w, kw, sw)
  addend, cot = rng.standard_normal((2, out_h, out_w, ch_out)), rng.standard_normal((2, out_h, out_w, ch_out))
  leaves = [torch.tensor(v, requires_grad=True) for v in (x, kernel, bias, addend)]
  a = F.relu(leaves[0]) if relu else leaves[0]
  padded = F.pad(a.permute(0, 3, 1, 2), (left, right, top, bottom))               # TF 'same': the odd cell goes behind
  want = F.conv2d(padded, leaves[1].permute(3, 2, 0, 1), leaves[2], stride=(sh, sw)).permute(0, 2, 3, 1) + leaves[3]
  assert want.shape == (2, out_h, out_w, ch_out)
  fn = lambda x_, k_, b_, a_: T.conv2d(x_, k_, b_, (sh, sw), relu, a_)
  _close(fn(x, kernel, bias, addend).numpy(), want.detach().numpy())
  assert T.conv2d(x, kernel, None, (sh, sw), relu, dtype=torch.float32).dtype is torch.float32
  for got, ref in zip(T.grads(fn, (x, kernel, bias, addend), [cot]), torch.autograd.grad(want, leaves, torch.tensor(cot))):
    _close(got, ref.numpy())


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('h, w, ch_in, ch_out, kh, kw, sh, sw', GEOMETRIES)
def test_the_gather_form_of_the_adjoint_is_autograd_of_the_truth(h, w, ch_in, ch_out, kh, kw, sh, sw, relu):
  rng = np.random.default_rng(32)
  x, kernel = rng.standard_normal((2, h, w, ch_in)), rng.standard_normal((kh, kw, ch_in, ch_out))
  x[0, 0, 0, 0] = 0.0
  g = rng.standard_normal((2, _tf_same(h, kh, sh)[0], _tf_same(w, kw, sw)[0], ch_out))
  want, = T.grads(lambda x_: T.conv2d(x_, kernel, None, (sh, sw), relu), [x], [g])
  _close(T.conv2d_adjoint(g, kernel, (h, w), (sh, sw), x if relu else None).numpy(), want)


@pytest.mark.parametrize('h, w, ph, pw, sh, sw', [(3, 9, 1, 3, 1, 2), (3, 10, 1, 3, 1, 2), (5, 6, 2, 2, 2, 2), (5, 7, 3, 2, 2, 3), (4, 4, 2, 4, 1, 1)])
def test_truth_max_pool_is_max_pool2d_of_torch_on_the_explicitly_padded_tensor(emulated, h, w, ph, pw, sh, sw):
  rng = np.random.default_rng(33)
  x = rng.standard_normal((2, h, w, 3)) - 3.0                                      # all negative: a padded 0 would win
  (out_h, top, bottom), (out_w, left, right) = _tf_same(h, ph, sh), _tf_same(w, pw, sw)
  leaf = torch.tensor(x, requires_grad=True)
  padded = F.pad(leaf.permute(0, 3, 1, 2), (left, right, top, bottom), value=-np.inf)
  want = F.max_pool2d(padded, (ph, pw), (sh, sw)).permute(0, 2, 3, 1)
  assert want.shape == (2, out_h, out_w, 3)
  fn = lambda x_: T.max_pool(x_, (ph, pw), (sh, sw))
  _close(fn(x).numpy(), want.detach().numpy())
  cot = rng.standard_normal(tuple(want.shape))
  _close(T.grads(fn, [x], [cot])[0], torch.autograd.grad(want, [leaf], torch.tensor(cot))[0].numpy())
  layer = nn.MaxPool2D((ph, pw), (sh, sw))                                         # framework ops: runs on host memory
  assert np.array_equal(layer(torch.tensor(x, dtype=torch.float32)).numpy(), fn(x.astype(np.float32)).numpy().astype(np.float32))


def test_output_sizes_and_padding_at_the_models_own_widths():
  """[frames, 229 bins] through ResNet: the stem and the pool halve, the stacks stride by 1, 2, 2 and 2."""
  widths = [229]
  for k, s in [(7, 2), (3, 2), (3, 1), (3, 2), (3, 2), (3, 2)]:
    out, before, behind = nn.same_padding(widths[-1], k, s)
    assert (out, before, behind) == T.same_padding(widths[-1], k, s) == _tf_same(widths[-1], k, s)
    assert behind - before in (0, 1) and (out - 1) * s + k - widths[-1] <= before + behind
    widths.append(out)
  assert widths == [229, 115, 58, 58, 29, 15, 8]
  assert nn.same_padding(229, 7, 2) == (115, 3, 3) and nn.same_padding(115, 3, 2) == (58, 1, 1) and nn.same_padding(58, 3, 2) == (29, 0, 1)
  assert nn.same_padding(29, 3, 2) == (15, 1, 1) and nn.same_padding(15, 3, 2) == (8, 1, 1) and nn.same_padding(58, 1, 2) == (29, 0, 0)
  assert nn.same_padding(125, 7, 1) == (125, 3, 3) and nn.same_padding(6, 2, 2) == (3, 0, 0) and nn.same_padding(10, 4, 3) == (4, 1, 2)


# ---- the reference's interface --------------------------------------------------------------------------------------------
def _signature(cls):
  return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:] if p.kind is not p.VAR_KEYWORD]


def test_constructor_arguments_order_and_defaults_are_the_references():
  # typed in from ddsp/training/nn.py:702, 716-717, 763-770, 809-810 and ddsp/training/encoders.py:139-145, 183-193
  empty = inspect.Parameter.empty
  assert _signature(nn.NormReluConv) == [('ch', empty), ('k', empty), ('s', empty), ('norm_type', empty)]
  assert _signature(nn.ResidualLayer) == [('ch', empty), ('stride', empty), ('shortcut', empty), ('norm_type', empty), ('conditional', empty),
                                          ('shift_only', empty)]
  assert _signature(nn.ResidualStack) == [('filters', empty), ('block_sizes', empty), ('strides', empty), ('norm_type', empty),
                                          ('conditional', False), ('shift_only', False), ('nonlinearity', 'relu')]
  assert _signature(nn.ResNet) == [('size', 'large'), ('norm_type', 'layer'), ('conditional', False), ('shift_only', False)]
  sig = dict(_signature(encoders.ResnetSinusoidalEncoder))
  assert list(sig) == ['output_splits', 'spectral_fn', 'size'] and sig['size'] == 'tiny'
  assert sig['output_splits'] == (('frequencies', 100 * 64), ('amplitudes', 100), ('noise_magnitudes', 60))
  sig = dict(_signature(encoders.SinusoidalToHarmonicEncoder))
  assert list(sig) == ['net', 'n_harmonics', 'f0_depth', 'amp_scale_fn', 'freq_scale_fn', 'sample_rate']
  assert (sig['net'], sig['n_harmonics'], sig['f0_depth'], sig['sample_rate']) == (None, 100, 64, 16000)
  assert [(p.name, p.default) for p in inspect.signature(nn.conv2d).parameters.values()] == [
      ('x', empty), ('kernel', empty), ('bias', None), ('strides', (1, 1)), ('relu_input', False), ('addend', None)]
  assert _signature(nn.SpatialConv2D) == [('filters', empty), ('kernel_size', empty), ('strides', (1, 1)), ('kernel_initializer', 'glorot_uniform')]


def test_layer_lists_of_the_reference():
  layer = nn.ResidualLayer(8, 2, True, 'layer', False, False)
  assert [n for n, _ in layer.named_children()] == ['norm_input', 'conv_proj', 'bottleneck']
  assert (layer.conv_proj.filters, layer.conv_proj.kernel_size, layer.conv_proj.strides) == (32, (1, 1), (1, 2))
  b0, b1, b2 = layer.bottleneck
  assert (b0.filters, b0.kernel_size, b0.strides) == (8, (1, 1), (1, 1))
  assert (b1.conv.filters, b1.conv.kernel_size, b1.conv.strides, b1.norm.norm_type) == (8, (3, 3), (1, 2), 'layer')
  assert (b2.conv.filters, b2.conv.kernel_size, b2.conv.strides) == (32, (1, 1), (1, 1))
  assert not hasattr(nn.ResidualLayer(8, 1, False, 'layer', False, False), 'conv_proj')
  assert isinstance(nn.ResidualLayer(8, 1, False, 'instance', True, True).norm_input, nn.ConditionalNorm)
  for size, (ch, blocks) in T.SIZES.items():
    net = nn.ResNet(size)
    stem, pool, first, second = net.layers
    assert (stem.filters, stem.kernel_size, stem.strides) == (64, (7, 7), (1, 2))
    assert (pool.pool_size, pool.strides, pool.padding) == ((1, 3), (1, 2), 'same')
    assert len(first.layers) == sum(blocks) + 1 and len(second.layers) == 4 and isinstance(first.layers[-1], nn.Normalize)
    strides = [l.bottleneck[1].conv.strides for l in first.layers[:-1]]
    assert strides == [(1, s) for s in T.stack_strides(blocks, [1, 2, 2])]
    assert [l.shortcut for l in first.layers[:-1]] == [i == 0 for n in blocks for i in range(n)]
    assert second.layers[0].conv_proj.filters == 32 * ch
  with pytest.raises(KeyError):
    nn.ResNet('tiny')
  with pytest.raises(KeyError):
    encoders.ResnetSinusoidalEncoder()                                             # the reference's default size fails the same way


def test_every_value_error_and_limit_without_a_device():
  with pytest.raises(ValueError, match='over time only'):
    nn.Conv2D(4, (3, 3))                                                           # Conv2D keeps its (k, 1) contract
  with pytest.raises(ValueError, match='kernel_initializer'):
    nn.SpatialConv2D(4, 3, kernel_initializer='orthogonal')
  with pytest.raises(ValueError, match='kernel_size'):
    nn.SpatialConv2D(4, (3, 0))
  with pytest.raises(ValueError, match='strides'):
    nn.SpatialConv2D(4, 3, (1, 2, 3))
  with pytest.raises(ValueError, match='padding'):
    nn.MaxPool2D((1, 3), (1, 2), padding='full')
  with pytest.raises(ValueError, match='x must be'):
    nn.MaxPool2D((1, 3))(torch.zeros(2, 3, 4))
  x, kernel = torch.zeros(1, 4, 5, 2), torch.zeros(3, 3, 2, 4)
  z = torch.zeros
  for bad_x, bad_kernel, bias, strides, addend, match in [
      (z(4, 5, 2), kernel, None, 1, None, 'x must be'), (x, z(3, 2, 4), None, 1, None, 'kernel must be'),
      (x, z(3, 3, 3, 4), None, 1, None, 'agree in ch_in'), (z(1, 0, 5, 2), kernel, None, 1, None, 'at least 1'),
      (x, kernel, z(3), 1, None, 'bias must be'), (x, kernel, None, 0, None, 'strides'), (x, kernel, None, (1, 2, 3), None, 'strides'),
      (x, kernel, None, (1, 2), z(1, 4, 5, 4), 'addend must be'),
      (z(1, 1, 1, 1040), z(1, 1, 1040, 16), None, 1, None, '1024'), (x, z(3, 3, 2, 1040), None, 1, None, '1024'),
      (x, z(9, 8, 2, 4), None, 1, None, '64 taps'), (x, kernel, None, (9, 1), None, 'stride 8'), (x, kernel, None, (1, 9), None, 'stride 8'),
      (z(1, 1, 1, 2).expand(1 << 16, 1 << 7, 1 << 7, 2), kernel, None, 1, None, '2 \\*\\* 31'),
      (z(1, 1, 1, 2).expand(1 << 16, 32, 32, 2), z(3, 3, 2, 1024), None, 1, None, '2 \\*\\* 31'),
      (z(1, 1, 1, 1).expand(1, (1 << 30) + 1, 1, 1), z(1, 1, 1, 1), None, 1, None, '2 \\*\\* 30')]:
    with pytest.raises(ValueError, match=match):                                  # before anything touches the device: none is here
      nn.conv2d(bad_x, bad_kernel, bias, strides, addend=addend)


def test_layers_construct_without_a_gpu_and_fail_loudly_when_called():
  net = nn.ResNet('small')
  assert not net.layers[0].built
  if not torch.cuda.is_available():
    with pytest.raises(_lib.DdspLibraryError):
      net(torch.zeros(1, 3, 9, 1))
    with pytest.raises(_lib.DdspLibraryError):
      nn.conv2d(torch.zeros(1, 4, 5, 2), torch.zeros(3, 3, 2, 16))


# ---- weights (the kernels through the SIMT emulation, on host memory) ----------------------------------------------------------
@pytest.fixture
def emulated():
  from tests.hip_emu import emu_simt
  if not os.path.exists(emu_simt.CLANG):
    pytest.skip('the SIMT emulation builds with the ROCm clang++, which this machine does not have')
  with emu_simt.emulated():
    yield


def test_weight_names_layouts_and_initialiser_fans(emulated):
  torch.manual_seed(5)
  stack = nn.ResidualStack([4], [2], [2], 'layer', conditional=True)
  y = stack([torch.randn(2, 3, 6, 8), torch.randn(2, 3, 1, 5)])
  assert y.shape == (2, 3, 3, 16) and bool(torch.isfinite(y).all()) and float(y.detach().min()) >= 0.0
  shapes = {name: tuple(p.shape) for name, p in stack.named_parameters()}
  cond = lambda stem, ch: {stem + '.conditional_scale_and_shift.dense.kernel': (5, 2 * ch), stem + '.conditional_scale_and_shift.dense.bias': (2 * ch,)}
  conv = lambda stem, kh, kw, ci, co: {stem + '.kernel': (kh, kw, ci, co), stem + '.bias': (co,)}
  norm = lambda stem, ch: {stem + '.scale': (1, 1, 1, ch), stem + '.shift': (1, 1, 1, ch)}
  want = {}
  for n, ch_in in ((0, 8), (1, 16)):
    stem = 'layers.%d.' % n
    want.update(cond(stem + 'norm_input', ch_in))
    if n == 0:
      want.update(conv(stem + 'conv_proj', 1, 1, ch_in, 16))
    want.update(conv(stem + 'bottleneck.0', 1, 1, ch_in, 4))
    want.update(norm(stem + 'bottleneck.1.norm', 4))
    want.update(conv(stem + 'bottleneck.1.conv', 3, 3, 4, 4))
    want.update(norm(stem + 'bottleneck.2.norm', 4))
    want.update(conv(stem + 'bottleneck.2.conv', 1, 1, 4, 16))
  want.update(norm('layers.2', 16))
  assert shapes == want
  conv = nn.SpatialConv2D(6, (3, 5), (1, 2))
  conv.build(10)
  limit = (6.0 / (15 * 10 + 15 * 6)) ** 0.5                                       # glorot_uniform: fans kh kw in and kh kw out
  peak = float(conv.kernel.detach().abs().max())
  assert tuple(conv.kernel.shape) == (3, 5, 10, 6) and 0.9 * limit < peak <= limit and tuple(conv.bias.shape) == (6,) and not conv.bias.any()
  assert conv(torch.randn(2, 4, 7, 10)).shape == (2, 4, 4, 6)


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
  build_mod.build()
  return _lib.load()


def test_every_conv2d_signature_is_declared_and_exported(lib):
  header = open(os.path.join(ROOT, 'ddsp_amd', 'csrc', 'conv2d_abi.h')).read()
  flags = dict((name, int(value.rstrip('u'), 0)) for name, value in re.findall(r'#define DDSP_(CONV2D_[A-Z_]+) (\w+)', header))
  header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
  declared = set(re.findall(r'\b(ddsp_[a-z0-9_]+)\s*\(', header))
  assert declared and declared == set(_lib.CONV2D_SIGNATURES), declared ^ set(_lib.CONV2D_SIGNATURES)
  for other in (_lib.SIGNATURES, _lib.DECODER_SIGNATURES, _lib.NORM_SIGNATURES, _lib.CONV_SIGNATURES):
    assert not set(_lib.CONV2D_SIGNATURES) & set(other)
  public = open(os.path.join(ROOT, 'include', 'ddsp_amd.h')).read()
  for name in declared:
    assert hasattr(lib, name) and name not in public, name
    fn = _lib.conv2d_entry(lib, name)                     # idempotent
    assert fn.argtypes == _lib.CONV2D_SIGNATURES[name][1] and _lib.conv2d_entry(lib, name).restype is _lib.CONV2D_SIGNATURES[name][0]
  assert 'conv2d.hip' in build_mod.SOURCES
  assert flags == {name: getattr(_lib, name) for name in ('CONV2D_MAX_CHANNELS', 'CONV2D_MAX_TAPS', 'CONV2D_MAX_STRIDE', 'CONV2D_RELU_INPUT',
                                                            'CONV2D_ADJOINT', 'CONV2D_MASK_OUTPUT')}


def test_workspace_queries(lib):
  ws = lib.ddsp_conv2d_workspace_bytes
  adjoint = _lib.CONV2D_ADJOINT
  assert ws(2, 5, 6, 2, 4, 3, 3, 1, 1, 0) == 0                                  # the plain kernel needs none
  assert ws(2, 5, 6, 16, 16, 3, 3, 1, 2, 0) == 512 + 256 + 5 * 1 * 128 * 16     # header, row partials, (step, tile) fragments hi / lo: K = 144
  assert ws(32, 125, 229, 1, 64, 7, 7, 1, 2, 0) == 512 + 32 * 16 * 4 + 2 * 4 * 128 * 16       # the stem: 49 taps in two steps
  assert ws(32, 125, 229, 1, 64, 7, 7, 1, 2, adjoint) == 0                      # its adjoint produces one channel: the plain kernel
  assert ws(2, 4, 8, 16, 32, 1, 1, 1, 2, adjoint) == 512 + 256 + 1 * 1 * 128 * 16             # K = 32 gradient channels, one tile of ch_in
  assert ws(0, 5, 6, 16, 16, 3, 3, 1, 1, 0) == 0 and ws(1, 5, 6, 1040, 16, 3, 3, 1, 1, 0) == 0 and ws(1, 5, 6, 16, 16, 9, 8, 1, 1, 0) == 0
  assert ws(1, 5, 6, 16, 16, 3, 3, 9, 1, 0) == 0 and ws(1 << 11, 1 << 5, 1 << 5, 16, 1 << 10, 1, 1, 1, 1, 0) == 0


def test_null_pointers_bad_shapes_and_limits_return_codes(lib):
  p = 64                                                                       # any non-null value: nothing is launched
  conv = lib.ddsp_conv2d_f32
  ok = dict(x=p, w=p, bias=None, addend=None, mask=None, y=p, ws=None, ws_bytes=0, batch=1, h=4, width=5, ch_in=2, ch_out=16, kh=3, kw=3, sh=1,
            sw=2, flags=0, stream=None)
  call = lambda **kw: conv(*dict(ok, **kw).values())
  assert call(x=None) == -1 and call(w=None) == -1 and call(y=None) == -1
  assert call(flags=_lib.CONV2D_MASK_OUTPUT) == -1                               # a mask without its source
  assert call() == -1                                                            # the matrix-core path without a workspace
  assert call(ws=p, ws_bytes=16) == -4
  for bad in (dict(batch=-1), dict(h=0), dict(width=0), dict(ch_in=0), dict(ch_out=0), dict(kh=0), dict(kw=0), dict(sh=0), dict(sw=0),
              dict(flags=0x8)):
    assert call(**bad) == -2, bad
  for beyond in (dict(ch_in=1040), dict(ch_out=1040), dict(kh=9, kw=8), dict(sh=9), dict(sw=9), dict(h=(1 << 30) + 1, width=1, ch_in=1),
                 dict(batch=1 << 11, h=1 << 5, width=1 << 5, ch_in=1 << 10), dict(batch=1 << 11, h=1 << 5, width=1 << 5, sw=1, ch_out=1 << 10)):
    assert call(**beyond) == -3, beyond
  assert call(batch=0) == 0                                                      # no rows: nothing to do
